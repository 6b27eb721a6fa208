"""GPU: aocr_invert_panels against the restatement (tests/panels_ref.py) and against hand answers, and Model.recognize_page(panels=...)
against the restatement's chain panels -> (clean ->) segmentation.  Raw ABI calls through page_harness; every comparison is exact equality
of the whole poisoned output buffer (the padding between W and out_pitch and the tail included), of panels_dev and counts_dev over
sentinels, over garbage-filled scratch, at pitch W and at an odd pitch with an unaligned base.  The shapes are built from the PN_ constants
of csrc/panels.hip, read from its source: they are the smallest at which each seam of the kernels is crossed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import components_ref as CR
import panels_ref as PR
import segment_ref as R
from page_harness import csrc_constants, expect_placed, garbage_scratch, guarded_words, place, poisoned
from panels_cases import CASES, SEEDED, SEEDED_SHAPES, SMALL, diamond, panel_page, rotated_slab

pytestmark = pytest.mark.gpu

SENTINEL = -7
OUT_FILL = 0x5A          # the poison of the output buffer
OUT_TAIL = 16            # bytes of that buffer behind the last row's pitch
GUARD = 3                # rows of panels_dev behind max_panels


def _consts():
    return csrc_constants("panels.hip", ("PN_SEG_W", "PN_THREADS", "PN_MAX", "PN_GRID"))


def _invert(cuda, page, params, max_panels=16, pitch=None, offset=0, op=None, shape=None, out=True, counts=True, panels=True, no_scratch=False,
            reserved=0, raw=None):
    """raw aocr_invert_panels: (the whole output buffer, panels_dev with its guard rows, counts, status)."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=255 if params.get("light_text") else 0)
    op = op or page.shape[1]
    o = poisoned(cuda, page.shape[0] * op + OUT_TAIL, OUT_FILL)
    cnt = guarded_words(cuda, 8, 0, SENTINEL, torch.int32)
    rows = guarded_words(cuda, max(min(max_panels, 1024), 1), GUARD, SENTINEL, torch.int32, 8)
    p = aocr.PanelParams()
    for k, v in dict(params, **(raw or {})).items():                            # field by field: the constructor turns bad values down
        setattr(p, k, v)
    p.reserved = reserved
    sc = garbage_scratch(cuda, aocr.lib.aocr_panels_scratch_bytes(page.shape[0], page.shape[1], max(min(max_panels, 1024), 1)), 1 << 12)
    st = aocr.lib.aocr_invert_panels(None, C.c_void_p(addr), pitch, H, W, C.byref(p), None if no_scratch else aocr.ptr(sc),
                                     aocr.ptr(o) if out else None, op, max_panels, aocr.ptr(rows) if panels else None, aocr.ptr(cnt) if counts else None)
    torch.cuda.synchronize()
    return o.cpu().numpy(), rows.cpu().numpy(), cnt.cpu().numpy(), st


def _check(cuda, page, params, what, max_panels=16, pitch=None, offset=0, op=None, want=None):
    want_out, want_panels, want_counts = want if want is not None else PR.invert_panels(page, max_panels, **params)
    out, rows, counts, st = _invert(cuda, page, params, max_panels, pitch, offset, op)
    assert st == 0, what
    np.testing.assert_array_equal(counts, want_counts, err_msg=str(what))
    n = len(want_panels)
    np.testing.assert_array_equal(rows[:n], want_panels, err_msg=str(what))
    assert (rows[n:] == SENTINEL).all(), what                                   # rows beyond the examined candidates are untouched
    np.testing.assert_array_equal(out, expect_placed(want_out, op, 0, poison=OUT_FILL, tail=OUT_TAIL), err_msg=str(what))
    return want_out, want_panels, want_counts


def _both_pitches(cuda, page, params, what, max_panels=16, want=None):
    W = page.shape[1]
    want = want if want is not None else PR.invert_panels(page, max_panels, **params)
    for pitch, offset, op in ((W, 0, W), (W + 7, 5, W + 3)):
        _check(cuda, page, params, (what, pitch), max_panels, pitch, offset, op, want=want)
    return want


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_cases(cuda, case):
    _both_pitches(cuda, case["page"], case["params"], case["name"], want=(case["out"], case["panels"], case["counts"]))


def _bar(w, h, holes=0, H=20, W=60):
    page = np.full((H, W), 255, np.uint8)
    page[3:3 + h, 5:5 + w] = 0
    page[4, 6:6 + 2 * holes:2] = 255
    return page


def test_box_size_at_and_under_the_minimum(cuda):
    for w, h, found in ((8, 4, 1), (7, 4, 0), (8, 3, 0)):
        _, _, counts = _both_pitches(cuda, _bar(w, h, 1), SMALL, (w, h))
        assert counts[1] == found


def test_fill_and_inside_percent_at_the_boundary_and_one_pixel_past_it(cuda):
    for holes, ok in ((40, 1), (41, 0)):                                        # hull 100: 60 ink pixels pass fill_percent 60, 59 do not
        page = np.full((12, 40), 255, np.uint8)
        page[3:8, 5:25] = 0
        for y, x in [(y, x) for y in (4, 5, 6) for x in range(6, 24)][:holes]:
            page[y, x] = 255
        _, rows, _ = _both_pitches(cuda, page, SMALL, ("fill", holes))
        assert rows[0].tolist()[5:] == [100 - holes, 100, ok]
    for holes, ok in ((4, 1), (3, 0)):                                          # hull 200: 4 light pixels are 2 %, 3 are not
        _, rows, _ = _both_pitches(cuda, _bar(25, 8, holes), SMALL, ("inside", holes))
        assert rows[0].tolist()[5:] == [200 - holes, 200, ok]
    _, rows, _ = _both_pitches(cuda, _bar(25, 8, 0), dict(SMALL, min_inside_percent=0), "solid bar, inside 0")
    assert rows[0].tolist()[5:] == [200, 200, 1]


def test_hull_not_box_for_a_diamond_and_a_rotated_slab(cuda):
    for name, page, params in (("diamond", diamond(12), dict(SMALL, fill_percent=80)), ("rotated", rotated_slab(30, 90), dict(SMALL, fill_percent=80)),
                               ("rotated_light", rotated_slab(30, 90, light=True), dict(SMALL, fill_percent=80, light_text=1))):
        out, rows, counts = _both_pitches(cuda, page, params, name)
        x0, y0, x1, y1, _, _, hull, ok = rows[0].tolist()
        assert ok == 1 and hull < (x1 - x0) * (y1 - y0)
        for y, x in ((y0, x0), (y0, x1 - 1), (y1 - 1, x0), (y1 - 1, x1 - 1)):
            assert out[y, x] == page[y, x]


def test_touching_all_four_borders(cuda):
    page = np.zeros((20, 70), np.uint8)
    page[5, 3:60:2] = 255
    page[11:13, 10:20] = 255
    out, rows, counts = _both_pitches(cuda, page, SMALL, "borders")
    assert rows[0].tolist()[:4] == [0, 0, 70, 20] and counts[3] == 1
    np.testing.assert_array_equal(out, 255 - page)


def test_diagonal_touch_under_both_connectivities(cuda):
    page = np.full((14, 40), 255, np.uint8)
    page[1:6, 2:14] = 0
    page[6:11, 14:26] = 0
    page[3, 4:10:2] = 255
    page[8, 16:22:2] = 255
    _, _, c4 = _both_pitches(cuda, page, dict(SMALL, connectivity=4, fill_percent=40), "conn4")
    _, _, c8 = _both_pitches(cuda, page, dict(SMALL, connectivity=8, fill_percent=40), "conn8")
    assert c4[:4].tolist() == [2, 2, 2, 2] and c8[:4].tolist() == [1, 1, 1, 1]


def _slabs_page(H, W, tops_lefts, w=10, h=5):
    page = np.full((H, W), 255, np.uint8)
    for y, x in tops_lefts:
        page[y:y + h, x:x + w] = 0
        page[y + 2, x + 2:x + w - 2:2] = 255
    return page


def test_max_panels_cuts_the_list_and_keeps_the_sentinel(cuda):
    page = _slabs_page(40, 40, [(2, 4), (12, 4), (22, 4), (32, 4)])
    for mp in (1, 2, 3, 4, 5):
        out, rows, counts = _both_pitches(cuda, page, SMALL, ("max_panels", mp), max_panels=mp)
        assert counts[1:4].tolist() == [4, min(mp, 4), min(mp, 4)] and len(rows) == min(mp, 4)
        if mp < 4:
            np.testing.assert_array_equal(out[2 + 10 * mp:], page[2 + 10 * mp:])                  # the later slabs are copied uninverted


def test_candidates_at_the_segment_seams(cuda):
    k = _consts()
    S = k["PN_SEG_W"]
    assert S == 64 and k["PN_THREADS"] == 256
    W = 3 * S + 9
    # first pixels in the last column of a segment, the first of the next, several in one segment and in one row, and on the rows around a
    # workgroup's four; the glyphs between them are components that are no candidates
    tops = [(1, S - 1), (1, S + 12), (1, S + 24), (1, 2 * S), (4, 3), (4, 2 * S - 11), (5, 3 * S - 2), (11, 0), (11, 11), (11, 22), (11, 33), (11, 44)]
    page = _slabs_page(18, W, tops)
    page[8, 5:W:7] = 0
    out, rows, counts = _both_pitches(cuda, page, SMALL, "seams", max_panels=16)
    assert counts[1:4].tolist() == [12, 12, 12] and counts[0] > 12
    assert sorted(rows[:, 4].tolist()) == rows[:, 4].tolist()                   # label order
    out, rows, counts = _both_pitches(cuda, page, SMALL, "seams cut", max_panels=7)
    assert counts[1:4].tolist() == [12, 7, 7]


def test_spans_at_every_offset_mod_16(cuda):
    """one ragged component: row r starts at column 20 + r % 16 and ends at 100 + r // 16 -- every pair of offsets mod 16, at an output pitch
    that is a multiple of 16 and at an odd one"""
    H, W = 260, 150
    page = np.full((H, W), 255, np.uint8)
    for r in range(256):
        page[2 + r, 20 + r % 16:100 + r // 16] = 0
    page[3:257:2, 40:90:2] = 255
    want = PR.invert_panels(page, 4, **SMALL)
    assert want[2][3] == 1 and want[1][0].tolist()[:4] == [20, 2, 115, 258]
    for pitch, offset, op in ((W, 0, 160), (W + 7, 5, W + 3), (176, 16, 176)):
        _check(cuda, page, SMALL, ("mod16", op), 4, pitch, offset, op, want=want)


@pytest.mark.parametrize("shape", [(8, 4100), (4100, 8)], ids=["8x4100", "4100x8"])
def test_long_and_high_pages(cuda, shape):
    k = _consts()
    H, W = shape
    assert max(H, W) - 2 > k["PN_GRID"] * (k["PN_THREADS"] // 64)               # more (candidate, row) pairs than the spans grid has waves
    page = np.full(shape, 255, np.uint8)
    page[1:H - 1, 1:W - 1] = 0                                                   # one slab nearly as large as the page
    if W > H:
        page[3, 5:W - 5:3] = 255
        page[5, 2000:2100] = 255
    else:
        page[5:H - 5:3, 3] = 255
        page[2000:2100, 5] = 255
    params = dict(SMALL, min_w=6, min_h=6)
    out, rows, counts = _both_pitches(cuda, page, params, shape)
    assert counts[3] == 1 and rows[0][6] == (H - 2) * (W - 2)


@functools.lru_cache(maxsize=None)
def _seeded_ref(H, W, seed, thr, light):
    painted, plain, rects = panel_page(H, W, seed, bool(light))
    painted.setflags(write=False)
    return painted, plain, rects, PR.invert_panels(painted, 16, threshold=thr, light_text=light, **SEEDED)


@pytest.mark.parametrize("thr,light", [(128, 0), (-1, 0), (128, 1), (-1, 1)], ids=["fixed", "otsu", "fixed_light", "otsu_light"])
@pytest.mark.parametrize("shape", SEEDED_SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SEEDED_SHAPES])
def test_matches_restatement_on_seeded_pages(cuda, shape, thr, light):
    H, W, pitch, offset, seed = shape
    painted, plain, rects, want = _seeded_ref(H, W, seed, thr, light)
    assert want[2][3] == len(rects) >= 1 and want[2][0] > 50
    np.testing.assert_array_equal(want[0], plain)                               # the page before the slabs were painted
    params = dict(threshold=thr, light_text=light, **SEEDED)
    for op in (W, W + 3):
        _check(cuda, painted, params, (shape, op), 16, pitch, offset, op, want=want)


def test_two_calls_null_panels_and_the_python_mirror(cuda):
    import aocr
    H, W, pitch, offset, seed = SEEDED_SHAPES[2]
    painted, plain, rects, want = _seeded_ref(H, W, seed, -1, 0)
    params = dict(threshold=-1, light_text=0, **SEEDED)
    a = _invert(cuda, painted, params, 16, pitch, offset, W + 3)
    b = _invert(cuda, painted, params, 16, pitch, offset, W + 3)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    out, rows, counts, st = _invert(cuda, painted, params, 16, panels=False)
    assert st == 0 and (rows == SENTINEL).all()
    np.testing.assert_array_equal(counts, want[2])
    np.testing.assert_array_equal(out, expect_placed(want[0], None, 0, poison=OUT_FILL, tail=OUT_TAIL))
    dev = torch.from_numpy(np.array(painted)).to(cuda)
    o, p, c = aocr.invert_panels_device(dev, aocr.PanelParams(**params), 16)
    np.testing.assert_array_equal(o.cpu().numpy(), want[0])
    np.testing.assert_array_equal(c.cpu().numpy(), want[2])
    np.testing.assert_array_equal(p.cpu().numpy()[:len(want[1])], want[1])
    assert (p.cpu().numpy()[len(want[1]):] == 0).all()
    view = dev[:, 3:200]                                                        # a view: pitch 257, an odd base
    wv = PR.invert_panels(painted[:, 3:200], 16, **params)
    o, p, c = aocr.invert_panels_device(view, aocr.PanelParams(**params), 16)
    np.testing.assert_array_equal(o.cpu().numpy(), wv[0])
    np.testing.assert_array_equal(c.cpu().numpy(), wv[2])


def test_invalid_arguments_leave_the_outputs_untouched(cuda):
    import aocr
    page = CASES[0]["page"]
    H, W = page.shape
    for kw, word in ((dict(reserved=1), "reserved"), (dict(raw=dict(fill_percent=60, min_inside_percent=41)), "more than 100"),
                     (dict(raw=dict(fill_percent=0)), "fill_percent"), (dict(raw=dict(min_inside_percent=100)), "min_inside_percent"),
                     (dict(raw=dict(min_w=0)), "min_w"), (dict(raw=dict(connectivity=5)), "connectivity"), (dict(raw=dict(threshold=255)), "threshold"),
                     (dict(max_panels=0), "max_panels"), (dict(max_panels=1025), "max_panels"), (dict(no_scratch=True), "NULL"),
                     (dict(out=False), "NULL"), (dict(counts=False), "NULL"), (dict(op=W - 1), "out_pitch"), (dict(shape=(H, W + 1)), "pitch"),
                     (dict(shape=(0, W)), "page size")):
        a = dict(op=W)
        a.update(kw)
        out, rows, counts, st = _invert(cuda, page, dict(SMALL), **a)
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (out == OUT_FILL).all() and (counts == SENTINEL).all() and (rows == SENTINEL).all(), kw
    assert aocr.lib.aocr_panels_scratch_bytes(0, 10, 4) == 0 and aocr.lib.aocr_panels_scratch_bytes(10, 10, 0) == 0
    assert aocr.lib.aocr_panels_scratch_bytes(10, 10, 1025) == 0 and aocr.lib.aocr_panels_scratch_bytes(16384, 4097, 4) == 0
    need = aocr.lib.aocr_panels_scratch_bytes(H, W, 4)
    assert 0 < need and need + (1 << 15) <= 1 << 17
    arena = torch.full(((1 << 17) // 8,), -1, dtype=torch.int64, device=cuda)          # every address below lies inside it
    base = arena.data_ptr()
    arena.view(torch.uint8)[:H * W] = torch.from_numpy(page.reshape(-1)).to(cuda)
    cnt = torch.full((8,), SENTINEL, dtype=torch.int32, device=cuda)
    before = arena.clone()
    p = aocr.PanelParams(**SMALL)
    free = 1 << 14                                                                      # behind the page, in front of the scratch at 1 << 15
    for out_at, sc_at, cnt_at, rows_at in ((H * W - 1, 1 << 15, None, None), ((1 << 15) + 64, 1 << 15, None, None), (free, 512, None, None),
                                           (free, 1 << 15, 100, None), (free, 1 << 15, free + 8, None), (free, 1 << 15, (1 << 15) + 8, None),
                                           (free, 1 << 15, None, 100), (free, 1 << 15, None, free + 8), (free, 1 << 15, None, (1 << 15) + 8),
                                           (free, 1 << 15, free + 4096, free + 4096 - 64)):
        st = aocr.lib.aocr_invert_panels(None, C.c_void_p(base), W, H, W, C.byref(p), C.c_void_p(base + sc_at), C.c_void_p(base + out_at), W, 4,
                                         None if rows_at is None else C.c_void_p(base + rows_at),
                                         aocr.ptr(cnt) if cnt_at is None else C.c_void_p(base + cnt_at))
        assert st != 0 and "overlap" in aocr.last_error(), (out_at, sc_at, cnt_at, rows_at)
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and (cnt.cpu().numpy() == SENTINEL).all()


def _model_page():
    """two lines of dark words on paper, and between them a slab 210 rows high (higher than clean's default max_h) that carries six lines of
    light words"""
    page = np.full((280, 300), 255, np.uint8)
    for y in (8, 256):
        for x in range(24, 260, 40):
            page[y:y + 12, x:x + 24] = 0
    slab = (20, 30, 280, 240)
    page[slab[1]:slab[3], slab[0]:slab[2]] = 0
    for y in range(44, 220, 32):
        for x in range(36, 250, 44):
            page[y:y + 12, x:x + 26] = 255
    return page, slab


def _inside(box, rect):
    return rect[0] <= box[0] and box[2] <= rect[2] and rect[1] <= box[1] and box[3] <= rect[3]


def test_recognize_page_panels(cuda, monkeypatch):
    import aocr
    from model_harness import make
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=32, W=100, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    page, slab = _model_page()
    SEG = dict(threshold=128, min_line_h=4, word_gap=8, min_word_w=2, pad_x=0, pad_y=0)
    params = aocr.SegmentParams(**SEG)
    want_out, want_panels, want_counts = PR.invert_panels(page, 256, **dict(PR.DEFAULTS, threshold=128))
    assert want_counts[1:4].tolist() == [1, 1, 1] and tuple(want_panels[0][:4]) == slab
    want_boxes, _ = R.segment_page(want_out, **SEG)
    n_on_slab = sum(_inside(b, slab) for b in want_boxes)
    assert n_on_slab == 30 and len(want_boxes) == 42

    before = m.recognize_page(page, params)                                     # today's path: the slab is one box, its words are lost
    assert not any(_inside(b, slab) and (b[2] - b[0]) < 100 for b in before.boxes)
    res = m.recognize_page(page, params, panels=True)
    np.testing.assert_array_equal(res.boxes, want_boxes[:, :4])
    np.testing.assert_array_equal(res.line, want_boxes[:, 4])
    np.testing.assert_array_equal(res.ink, want_boxes[:, 5])
    np.testing.assert_array_equal(res.panels, want_panels)
    np.testing.assert_array_equal(res.panel_counts, want_counts)
    assert res.panels.shape == (1, 8) and res.panels.dtype == np.int32 and res.panel_counts.dtype == np.int64
    ref = m.recognize_page(want_out, params)                                    # the crops are cut from the page with the slab inverted
    np.testing.assert_array_equal(res.labels, ref.labels)
    assert res.text == ref.text
    custom = m.recognize_page(page, params, panels=aocr.PanelParams(threshold=128, min_w=400))
    assert custom.panel_counts[1] == 0 and custom.panels.shape == (0, 8)
    np.testing.assert_array_equal(custom.boxes, before.boxes)

    # clean=True alone paints the slab over (210 rows > max_h) with the words on it; with panels=True in front of it they stay
    lost = m.recognize_page(page, params, clean=True)
    assert lost.clean_rules == 1 and not any(_inside(b, slab) for b in lost.boxes) and lost.n_found == 12
    cleaned_out, ccounts = CR.clean_page(want_out, **dict(CR.DEFAULTS, threshold=128))
    cboxes, _ = R.segment_page(cleaned_out, **SEG)
    kept = m.recognize_page(page, params, clean=True, panels=True)
    np.testing.assert_array_equal(kept.boxes, cboxes[:, :4])
    assert kept.clean_rules == 0 and sum(_inside(b, slab) for b in kept.boxes) == n_on_slab
    np.testing.assert_array_equal(kept.panel_counts, want_counts)
    lay = m.recognize_page(page, params, panels=True, deskew=aocr.SkewParams(threshold=128, n_steps=4), layout=aocr.LayoutParams(gap_x=400, gap_y=400))
    np.testing.assert_array_equal(lay.panel_counts, want_counts)                # the rider comes back with the layout's readback too
    np.testing.assert_array_equal(lay.panels, want_panels)
    with pytest.raises(ValueError, match="PanelParams"):
        m.recognize_page(page, params, panels=3)

    for off in (None, False):                                                   # panels=None is the call as it was
        b = m.recognize_page(page, params, panels=off)
        assert sorted(vars(before)) == sorted(vars(b)) and not hasattr(b, "panels")
        for k, v in vars(before).items():
            assert np.array_equal(v, getattr(b, k)) if isinstance(v, np.ndarray) else v == getattr(b, k), k

    reads = []
    real_cpu = torch.Tensor.cpu
    real_boxes = m._page_boxes

    def counted(*a, **k):
        monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *aa, **kk: (reads.append(t.numel()), real_cpu(t, *aa, **kk))[1])
        try:
            return real_boxes(*a, **k)
        finally:
            monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)

    monkeypatch.setattr(m, "_page_boxes", counted)
    for layout in (None, aocr.LayoutParams(gap_x=400, gap_y=400)):
        reads[:] = []
        m.recognize_page(page, params, layout=layout)
        without, reads[:] = list(reads), []
        m.recognize_page(page, params, layout=layout, panels=True)
        assert len(reads) == len(without) == 2 and reads[0] == without[0] + 8 + 8 * 256, (layout, without, reads)
    monkeypatch.setattr(m, "_page_boxes", real_boxes)
    # and over the whole call, on a page without panels (the same boxes, so the same crops and chunks)
    plain = want_out
    totals = []
    for kw in ({}, dict(panels=True)):
        reads[:] = []
        monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *aa, **kk: (reads.append(t.numel()), real_cpu(t, *aa, **kk))[1])
        try:
            r = m.recognize_page(plain, params, **kw)
        finally:
            monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
        totals.append(len(reads))
    assert totals[0] == totals[1] and r.panel_counts[3] == 0
    m.check_health()
    m.shutdown()
