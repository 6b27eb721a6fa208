"""GPU: aocr_ink_integral and aocr_layout_blocks against the numpy restatement (tests/layout_ref.py) and against hand answers, and
Model.recognize_page(layout=...) against the restatement's block-by-block segmentation.  Every comparison is exact equality of whole
buffers over poison: the table with the padding between W+1 and sat_pitch, the rows of blocks_dev beyond the count, over garbage-filled
scratch.  tests/test_layout_cpu.py shows on the restatement alone what the two-column page used here is cut into."""
import ctypes as C

import numpy as np
import pytest
import torch

import layout_ref as L
import segment_ref as R
from layout_cases import CASES, TWO_COL, two_column_page
from page_harness import csrc_constants, garbage_scratch, guarded_words, place
from segment_cases import SEEDED_SHAPES, seeded_page

pytestmark = pytest.mark.gpu

POISON = 0xABABABAB
SENTINEL = -7
GUARD_ROWS = 4


def _integral(cuda, page, threshold=-1, light_text=0, pitch=None, offset=0, sat_pitch=None, shape=None, scratch=True, sat=True, info=True):
    """raw aocr_ink_integral into a poisoned table over garbage scratch: (the whole table buffer (H+1, sat_pitch) plus 8 guard words as the
    device left it, info, status, the device tensor)."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=0)           # the bytes around the page are ink, were they read
    sat_pitch = sat_pitch or page.shape[1] + 1
    buf = torch.from_numpy(np.full((page.shape[0] + 1) * sat_pitch + 8, POISON, np.uint32).view(np.int32)).to(cuda)
    inf = guarded_words(cuda, 4, 0, SENTINEL, torch.int32)
    need = aocr.lib.aocr_integral_scratch_bytes(H, W)
    sc = garbage_scratch(cuda, need, 1 << 12)
    st = aocr.lib.aocr_ink_integral(None, C.c_void_p(addr), pitch, H, W, threshold, light_text, aocr.ptr(sc) if scratch else None,
                                    aocr.ptr(buf) if sat else None, sat_pitch, aocr.ptr(inf) if info else None)
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32), inf.cpu().numpy(), st, buf


def _expect_table(S, sat_pitch=None):
    H1, W1 = S.shape
    sat_pitch = sat_pitch or W1
    buf = np.full(H1 * sat_pitch + 8, POISON, np.uint32)
    np.lib.stride_tricks.as_strided(buf, (H1, W1), (4 * sat_pitch, 4))[:] = S
    return buf


def _blocks(cuda, sat_dev, sat_pitch, H, W, params, max_blocks, scratch=None, sat=True, out=True, counts=True, reserved=0):
    """raw aocr_layout_blocks on a device table: (blocks (max_blocks + GUARD_ROWS, 6) with SENTINEL in the rows that were not written, counts,
    status)."""
    import aocr
    p = aocr.LayoutParams(**params)
    p.reserved = reserved
    need = aocr.lib.aocr_layout_scratch_bytes(H, W, max_blocks)
    if scratch is None:
        scratch = garbage_scratch(cuda, need, 1 << 12)
    blocks = guarded_words(cuda, max(max_blocks, 1), GUARD_ROWS, SENTINEL, torch.int32, width=6)
    cnt = guarded_words(cuda, 4, 0, SENTINEL, torch.int32)
    st = aocr.lib.aocr_layout_blocks(None, aocr.ptr(sat_dev) if sat else None, sat_pitch, H, W, C.byref(p), aocr.ptr(scratch), max_blocks,
                                     aocr.ptr(blocks) if out else None, aocr.ptr(cnt) if counts else None)
    torch.cuda.synchronize()
    return blocks.cpu().numpy(), cnt.cpu().numpy(), st


def _check_blocks(got, got_counts, want, want_counts, what):
    np.testing.assert_array_equal(got_counts, want_counts, err_msg=str(what))
    n = len(want)
    np.testing.assert_array_equal(got[:n], want, err_msg=str(what))
    assert (got[n:] == SENTINEL).all(), what


def _tiling():
    """the tile sizes of csrc/layout.hip."""
    return csrc_constants("layout.hip", ("SAT_ROWS", "SAT_COLS", "SCAN_GROUPS"))


@pytest.mark.parametrize("thr,light", [(128, 0), (-1, 0), (128, 1), (-1, 1)], ids=["fixed", "otsu", "fixed_light", "otsu_light"])
@pytest.mark.parametrize("shape", SEEDED_SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SEEDED_SHAPES])
def test_table_matches_restatement_on_seeded_pages(cuda, shape, thr, light):
    H, W, pitch, offset, seed = shape
    page = seeded_page(H, W, seed, bool(light))
    S, info = L.ink_integral(page, thr, light)
    if thr < 0 and H > 1:
        assert 0 <= info[0] <= 254 and 0 < info[1] < H * W
    for sat_pitch in (W + 1, ((W + 1 + 3) & ~3) + 4):
        got, got_info, st, _ = _integral(cuda, page, thr, light, pitch, offset, sat_pitch)
        assert st == 0
        np.testing.assert_array_equal(got_info, info, err_msg=str((shape, sat_pitch)))
        np.testing.assert_array_equal(got, _expect_table(S, sat_pitch), err_msg=str((shape, sat_pitch)))


@pytest.mark.parametrize("shape,all_ink", [((8, 4100), False), ((4100, 8), True)], ids=["wide", "tall_all_ink"])
def test_long_axis_pages_cross_every_seam(cuda, shape, all_ink):
    H, W = shape
    t = _tiling()
    assert len(t) == 3
    if W > H:      # more than four column chunks: left carries over several chunks, a last chunk narrower than a word row
        assert W > 4 * t["SAT_COLS"] and W % t["SAT_COLS"] != 0
    else:          # more row segments than one workgroup of tiles owns, a ragged last one, several segments per scan group
        assert H > 4 * t["SAT_ROWS"] * t["SCAN_GROUPS"] and H % t["SAT_ROWS"] != 0
    page = np.zeros((H, W), np.uint8) if all_ink else seeded_page(H, W, 4100 + H)
    S, info = L.ink_integral(page, 128)
    if all_ink:
        assert info[1] == H * W
    got, got_info, st, _ = _integral(cuda, page, 128, 0, W + 3, 1, W + 6)
    assert st == 0
    np.testing.assert_array_equal(got_info, info)
    np.testing.assert_array_equal(got, _expect_table(S, W + 6))


def test_one_pixel_pages(cuda):
    for v, thr, light, ink in ((0, 128, 0, 1), (255, 128, 0, 0), (255, 128, 1, 1), (128, 128, 0, 1), (129, 128, 0, 0), (7, -1, 0, 0)):
        got, info, st, _ = _integral(cuda, np.full((1, 1), v, np.uint8), thr, light)
        assert st == 0 and info.tolist() == [thr, ink, 0, 0], (v, thr, light, info)
        assert got[:4].tolist() == [0, 0, 0, ink] and (got[4:] == POISON).all()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_cases(cuda, case):
    H, W = case["page"].shape
    got, info, st, sat = _integral(cuda, case["page"], case["threshold"], case["light_text"])
    assert st == 0
    np.testing.assert_array_equal(info, case["info"])
    blocks, counts, st = _blocks(cuda, sat, W + 1, H, W, case["params"], case["max_blocks"])
    assert st == 0
    _check_blocks(blocks, counts, case["blocks"], case["counts"], case["name"])


def test_two_column_page_matches_restatement(cuda):
    page = two_column_page()
    H, W = page.shape
    S, info = L.ink_integral(page, 128)
    sat_pitch = W + 5
    got, got_info, st, sat = _integral(cuda, page, 128, 0, W + 24, 7, sat_pitch)
    assert st == 0
    np.testing.assert_array_equal(got_info, info)
    np.testing.assert_array_equal(got, _expect_table(S, sat_pitch))
    import aocr
    need = aocr.lib.aocr_layout_scratch_bytes(H, W, 1024)
    scratch = garbage_scratch(cuda, need, 0)                                          # exactly the queried size
    seen = set()
    for min_ink, max_blocks in ((2, 256), (1, 256), (2, 1), (2, 1024), (1, 5), (2, 256)):
        params = dict(L.DEFAULTS, min_ink=min_ink, **TWO_COL)
        want, want_counts = L.layout_blocks(S, max_blocks, **params)
        blocks, counts, st = _blocks(cuda, sat, sat_pitch, H, W, params, max_blocks, scratch)     # the same scratch, call after call
        assert st == 0
        _check_blocks(blocks, counts, want, want_counts, (min_ink, max_blocks))
        seen.add(tuple(want_counts.tolist()))
    assert (5, 3, 0, 0) in seen and (5, 3, 1, 0) in seen and (1, 0, 0, 1) in seen and any(c[3] == 1 and c[1] > 0 for c in seen), seen
    # a speckled page under tight gaps: many small regions, several levels
    noisy = seeded_page(300, 700, 300700)
    Sn, _ = L.ink_integral(noisy, 128)
    _, _, st, satn = _integral(cuda, noisy, 128)
    tight = dict(L.DEFAULTS, min_ink=1, gap_x=5, gap_y=3, max_depth=4, min_block_w=3, min_block_h=3, min_block_ink=4)
    for max_blocks in (1024, 40):
        want, want_counts = L.layout_blocks(Sn, max_blocks, **tight)
        blocks, counts, st = _blocks(cuda, satn, 701, 300, 700, tight, max_blocks, scratch)
        assert st == 0
        _check_blocks(blocks, counts, want, want_counts, ("noisy", max_blocks))
        print(f"[layout] noisy page max_blocks {max_blocks}: counts {counts.tolist()}")
    assert want_counts[3] == 1 and want_counts[1] >= 1


def test_invalid_arguments_leave_the_outputs_untouched(cuda):
    import aocr
    page = seeded_page(40, 100, 3)
    for kw, word in ((dict(scratch=False), "NULL"), (dict(sat=False), "NULL"), (dict(info=False), "NULL"), (dict(sat_pitch=100), "sat_pitch"),
                     (dict(shape=(0, 100)), "page size"), (dict(shape=(40, 101)), "pitch"), (dict(shape=(16384, 4097), pitch=100), "page size"),
                     (dict(threshold=255), "threshold"), (dict(threshold=-2), "threshold")):
        got, info, st, _ = _integral(cuda, page, **dict(dict(threshold=128), **kw))
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (got == POISON).all() and (info == SENTINEL).all(), kw
    # a table that overlaps the page, or the scratch
    assert aocr.lib.aocr_integral_scratch_bytes(40, 100) + (1 << 15) <= 1 << 16
    arena = torch.full(((1 << 16) // 8,), -1, dtype=torch.int64, device=cuda)          # every address below lies inside it
    base = arena.data_ptr()
    arena.view(torch.uint8)[:4000] = torch.from_numpy(page.reshape(-1)).to(cuda)
    inf = torch.full((4,), SENTINEL, dtype=torch.int32, device=cuda)
    before = arena.clone()
    for page_at, sat_at, sc_at in ((0, 2000, 1 << 15), (0, 0, 1 << 15), (0, 4096, 4096 + 1024), (0, 4096 + 1024, 4096)):
        st = aocr.lib.aocr_ink_integral(None, C.c_void_p(base + page_at), 100, 40, 100, 128, 0, C.c_void_p(base + sc_at), C.c_void_p(base + sat_at),
                                        101, aocr.ptr(inf))
        assert st != 0 and "overlap" in aocr.last_error(), (page_at, sat_at, sc_at)
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and (inf.cpu().numpy() == SENTINEL).all()

    _, _, st, sat = _integral(cuda, page, 128)
    assert st == 0
    ok = dict(L.DEFAULTS)
    for kw, word in ((dict(params=dict(ok, max_depth=0)), "max_depth"), (dict(params=dict(ok, max_depth=17)), "max_depth"),
                     (dict(params=dict(ok, gap_y=0)), "gap_y"), (dict(params=dict(ok, min_ink=0)), "min_ink"),
                     (dict(params=dict(ok, min_block_w=0)), "min_block"), (dict(reserved=1), "reserved"), (dict(sat=False), "NULL"),
                     (dict(out=False), "NULL"), (dict(counts=False), "NULL"), (dict(sat_pitch=100), "sat_pitch"), (dict(max_blocks=0), "max_blocks"),
                     (dict(max_blocks=1025), "max_blocks"), (dict(shape=(16384, 4097)), "page size")):
        a = dict(params=ok, max_blocks=8, sat_pitch=101, shape=(40, 100))
        a.update(kw)
        H, W = a.pop("shape")
        blocks, counts, st = _blocks(cuda, sat, a.pop("sat_pitch"), H, W, a.pop("params"), a.pop("max_blocks"), **a)
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (blocks == SENTINEL).all() and (counts == SENTINEL).all(), kw
    blocks, counts, st = _blocks(cuda, sat, 101, 40, 100, ok, 8, scratch=sat)         # the scratch inside the table
    assert st != 0 and "overlap" in aocr.last_error() and (blocks == SENTINEL).all()


def test_python_surface_on_a_view(cuda):
    import aocr
    page = two_column_page()
    H, W = page.shape
    big = torch.zeros((H + 9, W + 30), dtype=torch.uint8, device=cuda)
    big[4:4 + H, 11:11 + W] = torch.from_numpy(page.copy()).to(cuda)
    view = big[4:4 + H, 11:11 + W]
    sat, info = aocr.ink_integral_device(view, threshold=128)
    S, want_info = L.ink_integral(page, 128)
    assert sat.shape == (H + 1, W + 1) and sat.dtype == torch.int32 and sat.stride(0) >= W + 1
    assert np.array_equal(sat.cpu().numpy(), S) and np.array_equal(info.cpu().numpy(), want_info)
    sat_o, info_o = aocr.ink_integral_device(view)                                   # Otsu
    So, want_o = L.ink_integral(page)
    assert np.array_equal(sat_o.cpu().numpy(), So) and np.array_equal(info_o.cpu().numpy(), want_o)
    blocks, counts, info = aocr.layout_page_device(view, aocr.LayoutParams(min_ink=2), threshold=128)
    want, want_counts, _ = L.layout_page(page, 128, 0, min_ink=2, **TWO_COL)
    assert blocks.shape == (256, 6) and np.array_equal(counts.cpu().numpy(), want_counts) and want_counts[0] == 5
    assert np.array_equal(blocks.cpu().numpy()[:5], want) and (blocks.cpu().numpy()[5:] == 0).all()
    with pytest.raises(aocr.AocrError):
        aocr.layout_page_device(view, aocr.LayoutParams(max_depth=0))
    with pytest.raises(aocr.AocrError):
        aocr.layout_page_device(view, max_blocks=2000)


def test_recognize_page_layout(cuda):
    import aocr
    from model_harness import make
    B, W = 32, 100
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=W, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    page = two_column_page().copy()
    params = aocr.SegmentParams(threshold=128)
    seg = dict(R.DEFAULTS, threshold=128)
    before = m.recognize_page(page, params, width=100)                               # today's path, before any layout call
    want_blocks, want_counts, _ = L.layout_page(page, 128, 0, min_ink=2, **TWO_COL)
    want, want_ids, want_lines, want_found, _ = L.segment_blocks(page, want_blocks, **seg)

    res = m.recognize_page(page, params, width=100, layout=aocr.LayoutParams(min_ink=2))
    assert res.n_blocks == 5 and not res.layout_overflow and res.threshold == 128 and not res.truncated
    np.testing.assert_array_equal(res.blocks, want_blocks[:, :4])
    np.testing.assert_array_equal(res.block_depth, want_blocks[:, 4])
    assert res.n_found == want_found == len(want) and res.n_lines == want_lines
    np.testing.assert_array_equal(res.boxes, want[:, :4])
    np.testing.assert_array_equal(res.block, want_ids)
    np.testing.assert_array_equal(res.line, want[:, 4])
    np.testing.assert_array_equal(res.ink, want[:, 5])
    order = [(int(b), int(l), int(x[0])) for b, l, x in zip(res.block, res.line, res.boxes)]
    assert order == sorted(order)                                                    # reading order: block, then line, then x
    for c0 in range(0, len(want), B):                                                # labels: recognize on the same crops
        idx = np.arange(c0, min(c0 + B, len(want)))
        ref = m.recognize([np.ascontiguousarray(page[b[1]:b[3], b[0]:b[2]]) for b in res.boxes[idx]], width=100)
        np.testing.assert_array_equal(res.labels[idx], ref.labels)
        np.testing.assert_array_equal(res.scores[idx], ref.scores)
        assert [res.text[i] for i in idx] == ref.text

    true_res = m.recognize_page(page, params, width=100, layout=True)                # the defaults: min_ink 1, the speck is cut out and dropped
    np.testing.assert_array_equal(true_res.boxes, want[:, :4])
    cut = m.recognize_page(page, params, width=100, layout=aocr.LayoutParams(min_ink=2), max_boxes=3)    # max_boxes applies per block
    assert cut.truncated and len(cut.text) == 15 and cut.n_found == want_found and cut.block.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
    empty = m.recognize_page(np.full((40, 60), 255, np.uint8), layout=True)
    assert empty.boxes.shape == (0, 4) and empty.n_blocks == 0 and empty.blocks.shape == (0, 4) and empty.text == [] and empty.threshold == -1

    after = m.recognize_page(page, params, width=100, layout=None)                   # layout=None is the call as it was
    off = m.recognize_page(page, params, width=100, layout=False)
    for r in (after, off):
        assert sorted(vars(r)) == sorted(vars(before)) and not hasattr(r, "blocks")
        for k in ("boxes", "line", "ink", "labels", "scores", "widths"):
            np.testing.assert_array_equal(getattr(r, k), getattr(before, k))
        assert r.text == before.text and (r.n_found, r.n_lines, r.threshold, r.truncated) == (before.n_found, before.n_lines, before.threshold, before.truncated)
    whole, wc = R.segment_page(page, **seg)
    np.testing.assert_array_equal(before.boxes, whole[:, :4])
    print(f"[recognize_page layout] {res.n_found} boxes in {res.n_lines} lines of {res.n_blocks} blocks; as one column: {before.n_found} in {before.n_lines}")
    m.check_health()
    m.shutdown()
