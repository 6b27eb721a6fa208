"""GPU: aocr_segment_page_spaced against the numpy restatement (tests/spacing_ref.py) and against hand answers, and
Model.recognize_page(spacing=...).  Everything here is exact: integers, and the Otsu scores as doubles computed operation for operation as
the restatement computes them.  Every raw call gets a page placed at an odd address inside a larger buffer of ink, scratch full of -1,
and outputs full of a sentinel with guard rows behind them."""
import ctypes as C

import numpy as np
import pytest
import torch

import segment_ref as R
import spacing_ref as SR
from page_harness import garbage_scratch, guarded_words, place
from segment_cases import SEEDED, SEEDED_SHAPES, seeded_page
from spacing_atlas import stacked_page
from spacing_cases import CASES, HAND

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD_ROWS = 4           # rows behind max_boxes boxes and behind max_lines spacing rows: they must keep their sentinel


def _spaced(cuda, page, params, spacing, max_boxes=64, pitch=None, offset=0, max_lines=None, want_rows=True):
    """raw aocr_segment_page_spaced: (boxes (max_boxes + GUARD_ROWS, 6), counts, rows (max_lines + GUARD_ROWS, 8), status), SENTINEL
    wherever nothing was written."""
    import aocr
    H, W = page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=0)           # the bytes around the page are ink, were they read
    p, sp = aocr.SegmentParams(**params), aocr.SpacingParams(**spacing)
    need = aocr.lib.aocr_segment_spaced_scratch_bytes(H, W, max_boxes)
    assert need > 0
    scratch = garbage_scratch(cuda, need, 0)
    max_lines = (H + 1) // 2 if max_lines is None else max_lines
    boxes = guarded_words(cuda, max_boxes, GUARD_ROWS, SENTINEL, torch.int32, width=6)
    counts = guarded_words(cuda, 4, 0, SENTINEL, torch.int32)
    rows = guarded_words(cuda, max_lines, GUARD_ROWS, SENTINEL, torch.int32, width=8)
    st = aocr.lib.aocr_segment_page_spaced(None, C.c_void_p(addr), pitch, H, W, C.byref(p), C.byref(sp), aocr.ptr(scratch), max_boxes,
                                           aocr.ptr(boxes), aocr.ptr(counts), max_lines, aocr.ptr(rows) if want_rows else None)
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), counts.cpu().numpy(), rows.cpu().numpy(), st


def _check(got, ref, what, max_lines=None):
    (gb, gc, gr, st), (rb, rc, rr) = got, ref
    assert st == 0, what
    np.testing.assert_array_equal(gc, rc, err_msg=str(what))
    np.testing.assert_array_equal(gb[:len(rb)], rb, err_msg=str(what))
    assert (gb[len(rb):] == SENTINEL).all(), what
    n = len(rr) if max_lines is None else min(len(rr), max_lines)
    np.testing.assert_array_equal(gr[:n], rr[:n], err_msg=str(what))
    assert (gr[n:] == SENTINEL).all(), what


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_painted_pages(cuda, case):
    H, W = case["page"].shape
    got = _spaced(cuda, case["page"], case["params"], case["spacing"], 16, pitch=W + 5, offset=3)
    _check(got, (case["boxes"], case["counts"], case["rows"]), case["name"])


_seeded_ref = {}


def _seeded(shape, thr, light, spacing_name):
    """the restatement on a seeded page, computed once per (page, parameters) and shared"""
    key = (shape, thr, light, spacing_name)
    if key not in _seeded_ref:
        H, W, _, _, seed = shape
        page = seeded_page(H, W, seed, bool(light))
        params = dict(SEEDED, threshold=thr, light_text=light)
        spacing = dict(HAND=HAND, DEFAULTS=SR.SPACING)[spacing_name]
        _seeded_ref[key] = (page, params, spacing, SR.segment_page_spaced(page, max_boxes=512, spacing=spacing, **params))
    return _seeded_ref[key]


@pytest.mark.parametrize("thr,light,spacing_name", [(128, 0, "HAND"), (-1, 0, "DEFAULTS"), (-1, 1, "HAND")], ids=["fixed", "otsu", "otsu_light"])
@pytest.mark.parametrize("shape", SEEDED_SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SEEDED_SHAPES])
def test_matches_restatement_on_seeded_pages(cuda, shape, thr, light, spacing_name):
    H, W, pitch, offset, _ = shape
    page, params, spacing, ref = _seeded(shape, thr, light, spacing_name)
    if H >= 300:                                             # a page that takes one branch only must not pass silently
        flags = set((ref[2][:, 1] & 3).tolist())
        assert len(flags) >= 2 and len(set(ref[2][:, 0].tolist())) >= 2, ref[2]
    got = _spaced(cuda, page, params, spacing, 512, pitch, offset)
    print(f"[spacing] {H}x{W} pitch {pitch} offset {offset} thr {thr} light {light}: counts {got[1].tolist()} gaps {got[2][:len(ref[2]), 0].tolist()}")
    _check(got, ref, shape)


def test_one_pixel_page(cuda):
    params = dict(R.DEFAULTS, threshold=128, min_line_h=1, min_word_w=1, pad_x=0, pad_y=0)
    for v, want in ((0, 1), (255, 0)):
        b, c, r, st = _spaced(cuda, np.full((1, 1), v, np.uint8), params, SR.SPACING, 4)
        assert st == 0 and c.tolist() == [want, want, 128, 0]
        assert (b[want:] == SENTINEL).all() and (r[want:] == SENTINEL).all()
        if want:                                             # h 1: lo = max(1, 0), hi = max(1, 0), the default max(1, 0): 1; no gap
            assert b[0].tolist() == [0, 0, 1, 1, 0, 1] and r[0].tolist() == [1, 1, 0, 0, 0, 1, 0, 0]


def test_widest_page(cuda):
    """40 x 16384: find_runs takes sixteen elements per thread, in both of the spaced kernel's passes."""
    page = np.tile(seeded_page(40, 100, 3), (1, 164))[:, :16384]             # the 40 x 100 seeded page side by side: three long lines
    params = dict(SEEDED, threshold=-1, light_text=0)
    ref = SR.segment_page_spaced(page, max_boxes=4096, spacing=HAND, **params)
    assert ref[1][0] >= 1000 and ref[2][:, 2].max() >= 1000 and len(set(ref[2][:, 0].tolist())) >= 2, (ref[1], ref[2])
    _check(_spaced(cuda, page, params, HAND, 4096, 16384 + 3, 1), ref, "40x16384")


def test_stacked_atlas_page(cuda):
    """the 131 x 470 atlas page above its 3x enlargement: the restatement's boxes, which are the placed words (test_spacing_cpu.py)."""
    page, placed = stacked_page()
    params = dict(R.DEFAULTS, threshold=128, min_word_w=2, pad_x=0, pad_y=0)
    ref = SR.segment_page_spaced(page, max_boxes=64, spacing=SR.SPACING, **params)
    assert [(int(b[0]), int(b[2])) for b in ref[0]] == [w for row in placed for w in row]
    got = _spaced(cuda, page, params, SR.SPACING, 64, page.shape[1] + 1, 7)
    _check(got, ref, "stacked")
    assert got[2][:3, 0].max() < got[2][3:6, 0].min()
    otsu = dict(params, threshold=-1)                        # Otsu on anti-aliased glyphs: the restatement's answer
    _check(_spaced(cuda, page, otsu, SR.SPACING, 64), SR.segment_page_spaced(page, max_boxes=64, spacing=SR.SPACING, **otsu), "stacked otsu")


def test_max_lines_null_rows_and_truncation(cuda):
    page, params, spacing, ref = _seeded(SEEDED_SHAPES[4], 128, 0, "HAND")
    lines = int(ref[1][1])
    assert lines >= 8 and ref[1][0] > 40
    _check(_spaced(cuda, page, params, spacing, 512, max_lines=3), ref, "max_lines 3", max_lines=3)       # rows 3.. keep the sentinel
    _check(_spaced(cuda, page, params, spacing, 512, max_lines=0), ref, "max_lines 0", max_lines=0)
    b, c, r, st = _spaced(cuda, page, params, spacing, 512, want_rows=False)                              # spacing_dev = NULL
    assert (r == SENTINEL).all()
    _check((b, c, r, st), ref, "NULL rows", max_lines=0)
    b, c, r, st = _spaced(cuda, page, params, spacing, 40)                                                # fewer boxes than found
    assert st == 0 and c.tolist() == ref[1].tolist() and c[0] > 40
    np.testing.assert_array_equal(b[:40], ref[0][:40])
    assert (b[40:] == SENTINEL).all()
    np.testing.assert_array_equal(r[:lines], ref[2])


def test_bit_identical_between_calls_and_pitches(cuda):
    page, params, spacing, ref = _seeded(SEEDED_SHAPES[4], -1, 0, "DEFAULTS")
    H, W = page.shape
    a = _spaced(cuda, page, params, spacing, 512)
    for other in (_spaced(cuda, page, params, spacing, 512), _spaced(cuda, page, params, spacing, 512, pitch=W + 37, offset=5),
                  _spaced(cuda, page, params, spacing, 512, pitch=1024, offset=16)):
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], other[:3]))
    assert a[1][0] > 50


def test_equal_gaps_equal_segment_page(cuda):
    """where the restatement says every band ends with the same G, boxes and counts equal aocr_segment_page(word_gap=G), on the device."""
    import aocr
    hit = 0
    for shape in SEEDED_SHAPES[1:]:
        H, W, _, _, seed = shape
        page = seeded_page(H, W, seed)
        params = dict(SEEDED, threshold=-1, light_text=0)
        spacing = dict(HAND, min_gaps=10 ** 6, lo_percent=10, default_percent=10, hi_percent=10)     # h < 20: max(1, h / 10) = 1
        ref = SR.segment_page_spaced(page, max_boxes=512, spacing=spacing, **params)
        gaps = set(ref[2][:, 0].tolist())
        if len(gaps) != 1:
            continue
        G = gaps.pop()
        hit += 1
        got = _spaced(cuda, page, params, spacing, 512)
        _check(got, ref, shape)
        dev, addr, pitch = place(cuda, page, None, 0, fill=0)
        p = aocr.SegmentParams(**dict(params, word_gap=G))
        boxes = guarded_words(cuda, 512, GUARD_ROWS, SENTINEL, torch.int32, width=6)
        counts = guarded_words(cuda, 4, 0, SENTINEL, torch.int32)
        scratch = garbage_scratch(cuda, aocr.lib.aocr_segment_scratch_bytes(H, W, 512), 0)
        assert aocr.lib.aocr_segment_page(None, C.c_void_p(addr), pitch, H, W, C.byref(p), aocr.ptr(scratch), 512, aocr.ptr(boxes), aocr.ptr(counts)) == 0
        torch.cuda.synchronize()
        assert np.array_equal(boxes.cpu().numpy(), got[0]) and np.array_equal(counts.cpu().numpy(), got[1])
    assert hit >= 2


def test_invalid_arguments_leave_the_outputs_untouched(cuda):
    import aocr
    page = seeded_page(40, 100, 3)
    good = dict(SEEDED, threshold=128, light_text=0)
    bad_seg = [("threshold", 255), ("min_row_ink", 0), ("min_line_h", 0), ("min_word_w", 0), ("merge_gap", -1), ("word_gap", 0), ("word_gap", -3),
               ("pad_x", -1), ("pad_y", -1)]
    bad_sp = [("min_gaps", 0), ("lo_percent", 0), ("lo_percent", 30), ("default_percent", 90), ("hi_percent", 401), ("hi_percent", 20),
              ("ratio_percent", 99), ("ratio_percent", 100001)]
    for field, v in bad_seg:
        b, c, r, st = _spaced(cuda, page, dict(good, **{field: v}), HAND, 16)
        assert st != 0 and field in aocr.last_error(), (field, aocr.last_error())
        assert (b == SENTINEL).all() and (c == SENTINEL).all() and (r == SENTINEL).all(), field
    for field, v in bad_sp:
        b, c, r, st = _spaced(cuda, page, good, dict(HAND, **{field: v}), 16)
        assert st != 0 and ("percent" in aocr.last_error() or "min_gaps" in aocr.last_error()), (field, aocr.last_error())
        assert (b == SENTINEL).all() and (c == SENTINEL).all() and (r == SENTINEL).all(), field
    dev, addr, pitch = place(cuda, page)
    p, sp = aocr.SegmentParams(**good), aocr.SpacingParams(**HAND)
    res = aocr.SpacingParams(**HAND)
    res.reserved[2] = 5
    boxes = torch.full((16, 6), SENTINEL, dtype=torch.int32, device=cuda)
    counts = torch.full((4,), SENTINEL, dtype=torch.int32, device=cuda)
    rows = torch.full((20, 8), SENTINEL, dtype=torch.int32, device=cuda)
    scratch = torch.empty(1 << 16, dtype=torch.int64, device=cuda)
    A = dict(page=C.c_void_p(addr), pitch=pitch, H=40, W=100, p=C.byref(p), sp=C.byref(sp), scratch=aocr.ptr(scratch), mb=16, boxes=aocr.ptr(boxes),
             counts=aocr.ptr(counts), ml=20, rows=aocr.ptr(rows))
    for change, word in ((dict(H=0), "page size"), (dict(W=0), "page size"), (dict(H=16385), "page size"), (dict(W=16385, pitch=16385), "page size"),
                         (dict(H=16384, W=4097, pitch=4097), "page size"), (dict(pitch=99), "pitch"), (dict(mb=0), "max_boxes"),
                         (dict(mb=4097), "max_boxes"), (dict(ml=-1), "max_lines"), (dict(page=None), "NULL"), (dict(p=None), "NULL"),
                         (dict(sp=None), "NULL"), (dict(scratch=None), "NULL"), (dict(boxes=None), "NULL"), (dict(counts=None), "NULL"),
                         (dict(sp=C.byref(res)), "reserved"), (dict(rows=C.c_void_p(rows.data_ptr() + 2)), "aligned"),
                         (dict(scratch=C.c_void_p(scratch.data_ptr() + 8)), "aligned"), (dict(rows=aocr.ptr(scratch)), "overlaps"),
                         (dict(rows=C.c_void_p(addr)), "overlaps")):
        a = dict(A, **change)
        st = aocr.lib.aocr_segment_page_spaced(None, a["page"], a["pitch"], a["H"], a["W"], a["p"], a["sp"], a["scratch"], a["mb"], a["boxes"],
                                               a["counts"], a["ml"], a["rows"])
        assert st != 0 and word in aocr.last_error(), (change, aocr.last_error())
    torch.cuda.synchronize()
    assert (boxes == SENTINEL).all() and (counts == SENTINEL).all() and (rows == SENTINEL).all()
    assert np.array_equal(dev.cpu().numpy()[:40 * 100].reshape(40, 100), page)


def test_python_surface_takes_a_view(cuda):
    import aocr
    page, params, spacing, ref = _seeded(SEEDED_SHAPES[3], -1, 0, "DEFAULTS")
    H, W = page.shape
    big = torch.zeros((H + 9, W + 30), dtype=torch.uint8, device=cuda)
    big[4:4 + H, 11:11 + W] = torch.from_numpy(page).to(cuda)
    view = big[4:4 + H, 11:11 + W]
    boxes, counts, rows = aocr.segment_page_spaced_device(view, aocr.SegmentParams(**params), None, max_boxes=512)
    assert rows.shape == ((H + 1) // 2, 8) and boxes.shape == (512, 6)
    n, lines = len(ref[0]), len(ref[2])
    assert np.array_equal(counts.cpu().numpy(), ref[1]) and np.array_equal(boxes.cpu().numpy()[:n], ref[0])
    assert np.array_equal(rows.cpu().numpy()[:lines], ref[2]) and not rows[lines:].any() and not boxes[n:].any()
    few = aocr.segment_page_spaced_device(view, aocr.SegmentParams(**params), aocr.SpacingParams(), max_boxes=512, max_lines=2)[2]
    assert np.array_equal(few.cpu().numpy(), ref[2][:2])
    crops = aocr.crop_lines_device(view, boxes, counts, 64)                                   # the boxes and counts feed the crops unchanged
    assert crops.shape == (512, 1, 32, 64) and (crops[n:] == 255.0).all()
    with pytest.raises(aocr.AocrError):
        aocr.segment_page_spaced_device(view, aocr.SegmentParams(word_gap=0))


# ---- Model.recognize_page(spacing=...) ---------------------------------------------------------------------------------------------------------
def _two_block_page():
    """two columns set in two sizes, a gutter of 60 columns between them: the two-line page of spacing_cases' line A left, its line B right"""
    from segment_cases import paint
    from spacing_cases import bars
    left = bars(4, 10, 2, 3, [1, 1, 4, 1, 1, 4, 1, 1]) + bars(30, 10, 2, 3, [1, 1, 4, 1, 1, 4, 1, 1])
    right = bars(4, 30, 110, 8, [5, 5, 14, 5, 5, 14, 5, 5]) + bars(50, 30, 110, 8, [5, 5, 14, 5, 5, 14, 5, 5])
    return paint(90, 250, left + right)


def test_recognize_page_spacing(cuda, monkeypatch):
    import aocr
    from model_harness import make
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=32, W=100, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    page, placed = stacked_page()
    seg = dict(R.DEFAULTS, threshold=128, min_word_w=2)
    params = aocr.SegmentParams(**seg)
    ref = SR.segment_page_spaced(page, max_boxes=1024, spacing=SR.SPACING, **seg)
    plain = m.recognize_page(page, params)

    res = m.recognize_page(page, params, spacing=True)
    np.testing.assert_array_equal(res.boxes, ref[0][:, :4])
    np.testing.assert_array_equal(res.line, ref[0][:, 4])
    np.testing.assert_array_equal(res.ink, ref[0][:, 5])
    np.testing.assert_array_equal(res.word_gaps, ref[2][:, 0])
    np.testing.assert_array_equal(res.spacing_flags, ref[2][:, 1])
    np.testing.assert_array_equal(res.spacing_gaps, ref[2][:, 2])
    assert res.word_gaps.dtype == res.spacing_flags.dtype == res.spacing_gaps.dtype == np.int32
    assert res.n_found == len(ref[0]) == sum(len(r) for r in placed) and res.n_lines == 6 and len(res.word_gaps) == 6
    assert plain.n_found > res.n_found                                                # the fixed gap of 12 splits the large lines
    for w in sorted(set(res.widths.tolist())):                                        # the crops are those of the boxes: recognise agrees
        idx = np.nonzero(res.widths == w)[0]
        again = m.recognize([np.ascontiguousarray(page[b[1]:b[3], b[0]:b[2]]) for b in res.boxes[idx]], width=int(w))
        np.testing.assert_array_equal(res.labels[idx], again.labels)
    custom = m.recognize_page(page, params, spacing=aocr.SpacingParams(**HAND))
    np.testing.assert_array_equal(custom.word_gaps, SR.segment_page_spaced(page, spacing=HAND, **seg)[2][:, 0])
    with pytest.raises(ValueError, match="SpacingParams"):
        m.recognize_page(page, params, spacing=3)

    for off in (None, False):                                                         # spacing=None is the call as it was
        b = m.recognize_page(page, params, spacing=off)
        assert sorted(vars(plain)) == sorted(vars(b)) and not hasattr(b, "word_gaps")
        for k, v in vars(plain).items():
            assert np.array_equal(v, getattr(b, k)) if isinstance(v, np.ndarray) else v == getattr(b, k), k

    two = _two_block_page()
    small = aocr.SegmentParams(threshold=128, min_line_h=3, min_word_w=2, pad_x=0, pad_y=0)
    lay = m.recognize_page(two, small, layout=aocr.LayoutParams(gap_x=40), spacing=aocr.SpacingParams(**HAND))
    assert lay.n_blocks == 2 and lay.n_lines == 4 and lay.n_found == 12
    assert lay.word_gaps.tolist() == [3, 3, 10, 10] and lay.spacing_flags.tolist() == [0, 0, 0, 0] and lay.spacing_gaps.tolist() == [8, 8, 8, 8]
    assert lay.line.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 and lay.block.tolist() == [0] * 6 + [1] * 6
    assert m.recognize_page(two, small, layout=aocr.LayoutParams(gap_x=40)).n_found != 12

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
    for layout in (None, aocr.LayoutParams(gap_x=40)):
        reads[:] = []
        m.recognize_page(two, small, layout=layout)
        without, reads[:] = list(reads), []
        m.recognize_page(two, small, layout=layout, spacing=True)
        assert len(reads) == len(without) == 2 and reads[0] == without[0], (layout, without, reads)
    empty = m.recognize_page(np.full((40, 60), 255, np.uint8), spacing=True)
    assert empty.boxes.shape == (0, 4) and empty.word_gaps.shape == (0,) and empty.spacing_flags.shape == (0,)
    m.check_health()
    m.shutdown()
