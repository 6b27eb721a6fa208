"""GPU: aocr_label_components and aocr_clean_page against the flood-fill restatement (tests/components_ref.py) and against hand answers, and
Model.recognize_page(clean=...) against the restatement's cleaning followed by its segmentation.  Raw ABI calls; every comparison is exact
equality of whole buffers over poison: the labels with the padding between W and labels_pitch, the rows of comps_dev beyond the count, the
output page with the padding between W and out_pitch, over garbage-filled scratch, at odd pitches and unaligned bases.  The shapes are built
from the tile of csrc/components.hip, read from its source: they are the smallest at which each seam of the kernels is crossed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import components_ref as CR
import segment_ref as R
from components_cases import (CLEAN_CASES, LABEL_CASES, MOTIVE_BOXES, MOTIVE_CLEAN, MOTIVE_SEG, border_crossers, checkerboard, corner_diagonals,
                              framed_text, motive_page, serpentine, u_shape)
from page_harness import csrc_constants, expect_placed, garbage_scratch, guarded_words, place, poisoned
from segment_cases import SEEDED_SHAPES, seeded_page

pytestmark = pytest.mark.gpu

POISON = 0xABABABAB
SENTINEL = -7
GUARD_ROWS = 4
OUT_FILL = 0x5A          # the poison of aocr_clean_page's output buffer
OUT_TAIL = 16            # bytes of that buffer behind the last row's pitch


def _tile():
    t = csrc_constants("components.hip", ("CC_TILE_H", "CC_TILE_W"))
    assert len(t) == 2
    return t["CC_TILE_H"], t["CC_TILE_W"]


def _scratch(cuda, need):
    return garbage_scratch(cuda, need, 1 << 12)


def _label(cuda, page, thr=128, light=0, conn=8, pitch=None, offset=0, lp=None, mc=4096, comps=True, shape=None, scratch=None, labels=True,
           info=True, no_scratch=False):
    """raw aocr_label_components: (the whole label buffer (H, lp) plus 8 guard words as the device left it, comps (mc + GUARD_ROWS, 6), info, status)."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=255 if light else 0)
    lp = lp or page.shape[1]
    lab = torch.from_numpy(np.full(page.shape[0] * lp + 8, POISON, np.uint32).view(np.int32)).to(cuda)
    cm = guarded_words(cuda, max(mc, 1), GUARD_ROWS, SENTINEL, torch.int32, width=6)
    inf = guarded_words(cuda, 4, 0, SENTINEL, torch.int32)
    if scratch is None:
        scratch = _scratch(cuda, aocr.lib.aocr_components_scratch_bytes(*page.shape))
    st = aocr.lib.aocr_label_components(None, C.c_void_p(addr), pitch, H, W, thr, light, conn, None if no_scratch else aocr.ptr(scratch),
                                        aocr.ptr(lab) if labels else None, lp, mc, aocr.ptr(cm) if comps else None, aocr.ptr(inf) if info else None)
    torch.cuda.synchronize()
    return lab.cpu().numpy().view(np.uint32), cm.cpu().numpy(), inf.cpu().numpy(), st


def _expect_labels(labels, lp=None):
    H, W = labels.shape
    lp = lp or W
    buf = np.full(H * lp + 8, POISON, np.uint32)
    np.lib.stride_tricks.as_strided(buf, (H, W), (4 * lp, 4))[:] = labels.view(np.uint32)
    return buf


def _check_label(cuda, page, want, what, thr=128, light=0, conn=8, pitch=None, offset=0, lp=None, mc=4096, scratch=None):
    labels, comps, info = want
    got, got_comps, got_info, st = _label(cuda, page, thr, light, conn, pitch, offset, lp, mc, scratch=scratch)
    assert st == 0, what
    np.testing.assert_array_equal(got_info, info, err_msg=str(what))
    np.testing.assert_array_equal(got, _expect_labels(labels, lp), err_msg=str(what))
    n = min(len(comps), mc)
    np.testing.assert_array_equal(got_comps[:n], comps[:n], err_msg=str(what))
    assert (got_comps[n:] == SENTINEL).all(), what


@functools.lru_cache(maxsize=None)
def _seeded_ref(shape, thr, light, conn):
    H, W, _, _, seed = shape
    page = seeded_page(H, W, seed, bool(light))
    page.setflags(write=False)
    return page, CR.label_components(page, thr, light, conn, max_components=page.size)


def _clean(cuda, page, params, pitch=None, offset=0, op=None, shape=None, out=True, counts=True, no_scratch=False, reserved=0, out_fill=OUT_FILL):
    """raw aocr_clean_page: (the whole output buffer (H, op) plus 16 guard bytes, counts, status)."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=255 if params.get("light_text") else 0)
    op = op or page.shape[1]
    o = poisoned(cuda, page.shape[0] * op + OUT_TAIL, out_fill)
    cnt = guarded_words(cuda, 8, 0, SENTINEL, torch.int32)
    p = aocr.CleanParams(**params)
    p.reserved[0] = reserved
    sc = _scratch(cuda, aocr.lib.aocr_clean_scratch_bytes(*page.shape))
    st = aocr.lib.aocr_clean_page(None, C.c_void_p(addr), pitch, H, W, C.byref(p), None if no_scratch else aocr.ptr(sc), aocr.ptr(o) if out else None, op,
                                  aocr.ptr(cnt) if counts else None)
    torch.cuda.synchronize()
    return o.cpu().numpy(), cnt.cpu().numpy(), st


def _expect_out(page, op=None, out_fill=OUT_FILL):
    return expect_placed(page, op, 0, poison=out_fill, tail=OUT_TAIL)


# ---- aocr_label_components ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("thr,light", [(128, 0), (-1, 0), (128, 1), (-1, 1)], ids=["fixed", "otsu", "fixed_light", "otsu_light"])
@pytest.mark.parametrize("shape", SEEDED_SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SEEDED_SHAPES])
def test_labels_match_restatement_on_seeded_pages(cuda, shape, thr, light, conn):
    H, W, pitch, offset, _ = shape
    TH, TW = _tile()
    if (H, W) == (300, 700):
        assert H > 2 * TH and W > 2 * TW
    page, want = _seeded_ref(shape, thr, light, conn)
    if thr < 0 and H > 1:
        assert 0 <= want[2][0] <= 254 and want[2][2] > 1
    for lp in (W, W + 3):
        _check_label(cuda, page, want, (shape, lp), thr, light, conn, pitch, offset, lp, mc=65536)


@pytest.mark.parametrize("case", LABEL_CASES, ids=[c["name"] for c in LABEL_CASES])
def test_label_hand_cases(cuda, case):
    _check_label(cuda, case["page"], (case["labels"], case["comps"], case["info"]), case["name"], case["threshold"], case["light_text"],
                 case["connectivity"])


def _shape_pages():
    TH, TW = _tile()
    return [("1xN", np.zeros((1, 2 * TW + 3), np.uint8)), ("Nx1", np.zeros((2 * TH + 3, 1), np.uint8)),
            ("1xN_dashes", np.where(np.arange(2 * TW + 3) % 3 == 2, 255, 0).astype(np.uint8)[None, :]),
            ("Nx1_dashes", np.where(np.arange(2 * TH + 3) % 3 == 2, 255, 0).astype(np.uint8)[:, None]),
            ("all_ink", np.zeros((2 * TH + 1, TW + 1), np.uint8)), ("all_paper", np.full((2 * TH + 1, TW + 1), 255, np.uint8)),
            ("checkerboard", checkerboard(2 * TH + 1, 2 * TW + 2)), ("corner_diagonals", corner_diagonals(TH, TW)),
            ("border_crossers", border_crossers(TH, TW)), ("u_shape", u_shape(TH, TW)), ("serpentine", serpentine(TH, TW)),
            ("framed_text", framed_text(TH, TW)), ("w_tile_plus_1", seeded_page(TH + 2, TW + 1, 11)), ("w_odd", seeded_page(2 * TH, TW + 7, 12))]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["1xN", "Nx1", "1xN_dashes", "Nx1_dashes", "all_ink", "all_paper", "checkerboard", "corner_diagonals",
                                  "border_crossers", "u_shape", "serpentine", "framed_text", "w_tile_plus_1", "w_odd"])
def test_tile_seams(cuda, name, conn):
    TH, TW = _tile()
    page = dict(_shape_pages())[name]
    H, W = page.shape
    want = CR.label_components(page, 128, 0, conn, max_components=page.size)
    n = int(want[2][2])
    if name == "checkerboard":
        assert n == (int((page == 0).sum()) if conn == 4 else 1)
    if name == "corner_diagonals":
        assert n == (4 if conn == 4 else 2)
    if name in ("u_shape", "serpentine", "all_ink", "1xN", "Nx1"):
        assert n == 1
    if name == "serpentine":
        assert H >= 3 * TH and W > 3 * TW
    if name == "framed_text":
        assert n > 1 and want[1][0].tolist()[:5] == [0, 0, W, H, 0]
    if name == "w_tile_plus_1":
        assert W == TW + 1
    if name == "w_odd":
        assert W % 4 != 0
    _check_label(cuda, page, want, (name, conn), conn=conn, pitch=W + 5, offset=3, lp=W + 1, mc=65536)


def test_truncation_null_comps_and_reused_scratch(cuda):
    import aocr
    TH, TW = _tile()
    page = checkerboard(2 * TH + 1, 2 * TW + 2)
    want = CR.label_components(page, 128, 0, 4, max_components=page.size)
    n = int(want[2][2])
    assert n > 100
    scratch = _scratch(cuda, aocr.lib.aocr_components_scratch_bytes(*page.shape))
    for mc in (1, 100, n, n + 5):                                              # the same scratch, call after call
        _check_label(cuda, page, want, ("mc", mc), conn=4, mc=mc, scratch=scratch)
    got, comps, info, st = _label(cuda, page, conn=4, comps=False, scratch=scratch)
    assert st == 0 and (comps == SENTINEL).all()
    np.testing.assert_array_equal(info, want[2])
    np.testing.assert_array_equal(got, _expect_labels(want[0]))
    _check_label(cuda, page, CR.label_components(page, 128, 0, 8), "conn 8 after 4", conn=8, scratch=scratch)


def test_otsu_without_a_threshold_labels_nothing(cuda):
    page = np.full((20, 70), 93, np.uint8)
    for light in (0, 1):
        _check_label(cuda, page, (np.full(page.shape, -1, np.int32), np.zeros((0, 6), np.int32), np.array([-1, 0, 0, 0], np.int32)), light, thr=-1,
                     light=light)


def test_invalid_arguments_leave_the_outputs_untouched(cuda):
    import aocr
    page = seeded_page(40, 100, 3)
    for kw, word in ((dict(no_scratch=True), "NULL"), (dict(labels=False), "NULL"), (dict(info=False), "NULL"), (dict(lp=99), "labels_pitch"),
                     (dict(shape=(0, 100)), "page size"), (dict(shape=(40, 101)), "pitch"), (dict(shape=(16384, 4097), pitch=100), "page size"),
                     (dict(thr=255), "threshold"), (dict(thr=-2), "threshold"), (dict(conn=6), "connectivity"), (dict(mc=0), "max_components"),
                     (dict(mc=65537), "max_components")):
        a = dict(lp=100)
        a.update(kw)
        got, comps, info, st = _label(cuda, page, **a)
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (got == POISON).all() and (comps == SENTINEL).all() and (info == SENTINEL).all(), kw
    need = aocr.lib.aocr_components_scratch_bytes(40, 100)
    assert need + (1 << 15) <= 1 << 17
    arena = torch.full(((1 << 17) // 8,), -1, dtype=torch.int64, device=cuda)          # every address below lies inside it
    base = arena.data_ptr()
    arena.view(torch.uint8)[:4000] = torch.from_numpy(page.reshape(-1)).to(cuda)
    inf = torch.full((4,), SENTINEL, dtype=torch.int32, device=cuda)
    before = arena.clone()
    for labels_at, sc_at in ((2000, 1 << 15), (0, 1 << 15), ((1 << 15) + 1024, 1 << 15), (1 << 14, 1 << 14)):
        st = aocr.lib.aocr_label_components(None, C.c_void_p(base), 100, 40, 100, 128, 0, 8, C.c_void_p(base + sc_at), C.c_void_p(base + labels_at), 100,
                                            16, None, aocr.ptr(inf))
        assert st != 0 and "overlap" in aocr.last_error(), (labels_at, sc_at)
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and (inf.cpu().numpy() == SENTINEL).all()

    ok = dict(threshold=128, connectivity=8, min_area=2, max_w=0, max_h=0)
    for kw, word in ((dict(params=dict(ok, connectivity=5)), "connectivity"), (dict(params=dict(ok, min_area=0)), "min_area"),
                     (dict(params=dict(ok, max_w=-1)), "max_w"), (dict(params=dict(ok, threshold=300)), "threshold"), (dict(reserved=1), "reserved"),
                     (dict(out=False), "NULL"), (dict(counts=False), "NULL"), (dict(no_scratch=True), "NULL"), (dict(op=99), "out_pitch"),
                     (dict(shape=(40, 101)), "pitch")):
        a = dict(params=ok, op=100)
        a.update(kw)
        out, counts, st = _clean(cuda, page, a.pop("params"), **a)
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (out == 0x5A).all() and (counts == SENTINEL).all(), kw
    cnt = torch.full((8,), SENTINEL, dtype=torch.int32, device=cuda)
    p = aocr.CleanParams(**ok)
    need = aocr.lib.aocr_clean_scratch_bytes(40, 100)
    assert need + (1 << 15) <= 1 << 17
    for out_at, sc_at in ((2000, 1 << 15), ((1 << 15) + 64, 1 << 15)):
        st = aocr.lib.aocr_clean_page(None, C.c_void_p(base), 100, 40, 100, C.byref(p), C.c_void_p(base + sc_at), C.c_void_p(base + out_at), 100, aocr.ptr(cnt))
        assert st != 0 and "overlap" in aocr.last_error(), (out_at, sc_at)
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and (cnt.cpu().numpy() == SENTINEL).all()


# ---- aocr_clean_page ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CLEAN_CASES, ids=[c["name"] for c in CLEAN_CASES])
def test_clean_hand_cases(cuda, case):
    H, W = case["page"].shape
    for pitch, offset, op in ((W, 0, W), (W + 7, 5, W + 3)):
        out, counts, st = _clean(cuda, case["page"], case["params"], pitch, offset, op)
        assert st == 0
        np.testing.assert_array_equal(counts, case["counts"], err_msg=case["name"])
        np.testing.assert_array_equal(out, _expect_out(case["out"], op), err_msg=case["name"])
    if case["name"] == "nothing":
        np.testing.assert_array_equal(case["out"], case["page"])


@pytest.mark.parametrize("conn", [4, 8])
def test_clean_matches_restatement_on_a_seeded_page(cuda, conn):
    H, W, pitch, offset, seed = SEEDED_SHAPES[-1]
    for thr, light in ((128, 0), (-1, 1)):
        page = seeded_page(H, W, seed, bool(light))
        params = dict(threshold=thr, light_text=light, connectivity=conn, min_area=4, max_w=18, max_h=9)
        want, want_counts = CR.clean_page(page, **params)
        assert want_counts[1] > 0 and want_counts[2] > 0 and 0 < want_counts[5] < want_counts[4]
        out, counts, st = _clean(cuda, page, params, pitch, offset, W + 9)
        assert st == 0
        np.testing.assert_array_equal(counts, want_counts)
        np.testing.assert_array_equal(out, _expect_out(want, W + 9))
    gray = np.full((30, 90), 200, np.uint8)                                      # Otsu finds no threshold: a copy
    out, counts, st = _clean(cuda, gray, dict(threshold=-1, connectivity=conn))
    assert st == 0 and counts.tolist() == [0, 0, 0, -1, 0, 0, 0, 0]
    np.testing.assert_array_equal(out, _expect_out(gray))


def test_motivating_page_end_to_end(cuda):
    import aocr
    clean, dirty = motive_page(), motive_page(True, True, True)
    seg = aocr.SegmentParams(**MOTIVE_SEG)
    big = torch.zeros((70, 140), dtype=torch.uint8, device=cuda)                 # a view: odd base, pitch 140
    big[3:63, 7:127] = torch.from_numpy(dirty).to(cuda)
    view = big[3:63, 7:127]
    boxes, counts = aocr.segment_page_device(view, seg)
    assert counts.cpu().tolist()[:2] != [6, 2]
    out, ccounts = aocr.clean_page_device(view, aocr.CleanParams(**MOTIVE_CLEAN))
    want_out, want_counts = CR.clean_page(dirty, **MOTIVE_CLEAN)
    assert out.shape == (60, 120) and out.dtype == torch.uint8
    np.testing.assert_array_equal(out.cpu().numpy(), clean)
    np.testing.assert_array_equal(want_out, clean)
    np.testing.assert_array_equal(ccounts.cpu().numpy(), want_counts)
    boxes, counts = aocr.segment_page_device(out, seg)
    assert counts.cpu().tolist() == [6, 2, 128, 0]
    np.testing.assert_array_equal(boxes.cpu().numpy()[:6], np.array(MOTIVE_BOXES, np.int32))
    same, scounts = aocr.clean_page_device(torch.from_numpy(clean).to(cuda), aocr.CleanParams(**MOTIVE_CLEAN))
    np.testing.assert_array_equal(same.cpu().numpy(), clean)                     # nothing to remove: bit for bit
    assert scounts.cpu().tolist() == [6, 0, 0, 128, 6 * 264, 0, 0, 0]
    labels, comps, info = aocr.label_components_device(view, threshold=128, connectivity=4, max_components=16)
    wl, wc, wi = CR.label_components(dirty, 128, 0, 4)
    assert labels.shape == (60, 120) and comps.shape == (16, 6)
    np.testing.assert_array_equal(labels.cpu().numpy(), wl)
    np.testing.assert_array_equal(info.cpu().numpy(), wi)
    np.testing.assert_array_equal(comps.cpu().numpy()[:len(wc)], wc)
    assert (comps.cpu().numpy()[len(wc):] == 0).all()
    with pytest.raises(aocr.AocrError):
        aocr.clean_page_device(view, aocr.CleanParams(connectivity=5))
    with pytest.raises(aocr.AocrError):
        aocr.label_components_device(view, max_components=0)


def test_recognize_page_clean(cuda):
    import aocr
    from model_harness import make
    B, W = 32, 100
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=W, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    dirty = motive_page(True, True, True)
    params = aocr.SegmentParams(**MOTIVE_SEG)
    before = m.recognize_page(dirty, params, width=100)                          # today's path, before any clean call
    assert (before.n_found, before.n_lines) != (6, 2)

    res = m.recognize_page(dirty, params, width=100, clean=aocr.CleanParams(**MOTIVE_CLEAN))
    assert (res.n_found, res.n_lines, res.threshold, res.truncated) == (6, 2, 128, False)
    np.testing.assert_array_equal(res.boxes, np.array(MOTIVE_BOXES, np.int32)[:, :4])
    np.testing.assert_array_equal(res.line, [0, 0, 0, 1, 1, 1])
    assert (res.clean_components, res.clean_specks, res.clean_rules, res.clean_ink_removed) == (12, 4, 2, 4 + 56 + 106)
    ref = m.recognize([np.ascontiguousarray(motive_page()[b[1]:b[3], b[0]:b[2]]) for b in res.boxes], width=100)
    np.testing.assert_array_equal(res.labels, ref.labels)                        # the crops are cut from the cleaned page
    assert res.text == ref.text

    dflt = dict(CR.DEFAULTS, threshold=128)                                      # clean=True: the defaults with the threshold and light_text of params
    want_out, want_counts = CR.clean_page(dirty, **dflt)
    want_boxes, want_seg = R.segment_page(want_out, **MOTIVE_SEG)
    true_res = m.recognize_page(dirty, params, width=100, clean=True)
    assert (true_res.n_found, true_res.n_lines) == (int(want_seg[0]), int(want_seg[1]))
    np.testing.assert_array_equal(true_res.boxes, want_boxes[:, :4])
    np.testing.assert_array_equal(true_res.ink, want_boxes[:, 5])
    assert (true_res.clean_components, true_res.clean_specks, true_res.clean_rules, true_res.clean_ink_removed) == tuple(
        int(want_counts[i]) for i in (0, 1, 2, 5))
    assert true_res.clean_specks == 4 and true_res.clean_rules == 0             # a 60-row page has nothing higher than 200 rows

    both = m.recognize_page(dirty, params, width=100, clean=aocr.CleanParams(**MOTIVE_CLEAN), deskew=aocr.SkewParams(threshold=128, n_steps=4),
                            layout=aocr.LayoutParams(gap_x=200, gap_y=200))      # the counts ride with the skew and the layout readback
    assert (both.clean_components, both.clean_specks, both.clean_rules, both.clean_ink_removed) == (12, 4, 2, 166)
    assert both.skew_steps == 0 and both.n_blocks == 1 and both.n_found == 6
    np.testing.assert_array_equal(both.boxes, res.boxes)
    skewed = m.recognize_page(dirty, params, width=100, clean=aocr.CleanParams(**MOTIVE_CLEAN), deskew=aocr.SkewParams(threshold=128, n_steps=4))
    assert skewed.clean_rules == 2 and skewed.skew_steps == 0
    np.testing.assert_array_equal(skewed.boxes, res.boxes)

    after = m.recognize_page(dirty, params, width=100, clean=None)              # clean=None is the call as it was
    off = m.recognize_page(dirty, params, width=100, clean=False)
    for r in (after, off):
        assert sorted(vars(r)) == sorted(vars(before)) and not hasattr(r, "clean_specks")
        for k in ("boxes", "line", "ink", "labels", "scores", "widths"):
            np.testing.assert_array_equal(getattr(r, k), getattr(before, k))
        assert r.text == before.text and (r.n_found, r.n_lines, r.threshold, r.truncated) == (before.n_found, before.n_lines, before.threshold, before.truncated)
    print(f"[recognize_page clean] dirty: {before.n_found} boxes in {before.n_lines} lines; cleaned: {res.n_found} in {res.n_lines}; "
          f"clean=True: {true_res.n_found} in {true_res.n_lines}")
    m.check_health()
    m.shutdown()
