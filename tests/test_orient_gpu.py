"""GPU: aocr_rotate_page against numpy.rot90 and aocr_estimate_orientation against the numpy restatement (tests/orient_ref.py), through the C
ABI, and Model.recognize_page(orient=...) against the call without it.  Everything is exact equality: every byte of the output buffer (the
turned page, and the poison everywhere else), every word of the estimate."""
import ctypes as C

import numpy as np
import pytest
import torch

import orient_ref as R
from orient_cases import PAINTED, SHAPES, text_page
from page_harness import expect_placed, garbage_scratch, guarded_words, place, poisoned
from segment_cases import paint, seeded_page

pytestmark = pytest.mark.gpu

SENTINEL = -7
POISON = 0xAB
TAIL = 32                # bytes of the turned page's buffer behind the last row's pitch


def _rotate(cuda, page, quarter, out_pitch, out_offset, orient_words=None, pitch=None, offset=0, shape=None):
    """raw aocr_rotate_page into a poisoned buffer sized for the output of `quarter`: (the whole buffer as the device left it, status)."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=99)
    Ho = page.shape[1] if quarter & 1 else page.shape[0]
    buf = poisoned(cuda, out_offset + Ho * max(out_pitch, 1) + TAIL, POISON)
    od = torch.tensor(orient_words, dtype=torch.int32, device=cuda) if orient_words is not None else None
    st = aocr.lib.aocr_rotate_page(None, C.c_void_p(addr), pitch, H, W, aocr.ptr(od), quarter, C.c_void_p(buf.data_ptr() + out_offset), out_pitch)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st


def _expect(page, q, quarter, out_pitch, out_offset):
    turned = np.rot90(page, -q)
    Ho, Wo = turned.shape
    assert (Ho, Wo) == (page.shape[::-1] if quarter & 1 else page.shape)
    return expect_placed(turned, out_pitch, out_offset, poison=POISON, tail=TAIL)


_pages = {}


def _seeded(H, W):
    if (H, W) not in _pages:
        _pages[(H, W)] = seeded_page(H, W, 31 * H + W)
    return _pages[(H, W)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SHAPES])
def test_rotate_matches_rot90(cuda, shape):
    """every byte of the output buffer for q = 0..3: the turned page, and the poison before the base, between Wo and the pitch and behind the
    last row.  A tight output at the buffer's base, and one with a wider pitch at an odd base."""
    H, W, pitch, offset = shape
    page = _seeded(H, W)
    for q in range(4):
        Wo = H if q & 1 else W
        for out_pitch, out_offset in ((Wo, 0), (Wo + 5, 3)):
            got, st = _rotate(cuda, page, q, out_pitch, out_offset, None, pitch, offset)
            assert st == 0
            np.testing.assert_array_equal(got, _expect(page, q, q, out_pitch, out_offset), err_msg=str((shape, q, out_pitch)))


def test_rotate_takes_the_half_turn_from_the_device(cuda):
    H, W, pitch, offset = SHAPES[6]
    page = _seeded(H, W)
    for quarter in (0, 1):
        Wo = H if quarter & 1 else W
        got, st = _rotate(cuda, page, quarter, Wo + 5, 3, [2, 11, 12, 13, 14, 0, 0, 0], pitch, offset)      # a half turn more
        assert st == 0
        np.testing.assert_array_equal(got, _expect(page, quarter + 2, quarter, Wo + 5, 3))
        got, st = _rotate(cuda, page, quarter, Wo, 0, [1, 0, 0, 0, 0, 0, 0, 0])                              # the odd bit is ignored
        np.testing.assert_array_equal(got, _expect(page, quarter, quarter, Wo, 0))
        got, st = _rotate(cuda, page, quarter + 2, Wo, 0, [3, 0, 0, 0, 0, 0, 0, 0])                          # 2 + 2 = 0, 3 + 2 = 1
        np.testing.assert_array_equal(got, _expect(page, quarter, quarter, Wo, 0))


def test_rotate_invalid_arguments_leave_the_output_untouched(cuda):
    import aocr
    page = _seeded(70, 257)
    for kw, word in ((dict(quarter=4, out_pitch=257), "quarter"), (dict(quarter=-1, out_pitch=257), "quarter"),
                     (dict(quarter=0, out_pitch=257, shape=(0, 257)), "page size"), (dict(quarter=1, out_pitch=70, shape=(70, 0)), "page size"),
                     (dict(quarter=0, out_pitch=256), "out_pitch"), (dict(quarter=1, out_pitch=69), "out_pitch"),
                     (dict(quarter=3, out_pitch=257, pitch=256), "pitch")):
        shape = kw.pop("shape", None)
        pitch = kw.pop("pitch", None)
        H, W = shape or page.shape
        dev, addr, p = place(cuda, page)
        buf = poisoned(cuda, 257 * 257 + 32, POISON)
        st = aocr.lib.aocr_rotate_page(None, C.c_void_p(addr), pitch or p, H, W, None, kw["quarter"], aocr.ptr(buf), kw["out_pitch"])
        torch.cuda.synchronize()
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (buf == POISON).all(), kw
    dev, addr, p = place(cuda, page)
    assert aocr.lib.aocr_rotate_page(None, C.c_void_p(addr), p, 70, 257, None, 1, None, 70) != 0 and "out_dev" in aocr.last_error()
    assert aocr.lib.aocr_rotate_page(None, C.c_void_p(addr), p, 70, 257, None, 1, C.c_void_p(addr + 100), 70) != 0 and "overlap" in aocr.last_error()
    assert aocr.lib.aocr_rotate_page(None, None, p, 70, 257, None, 1, C.c_void_p(addr), 70) != 0
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy()[:70 * 257].reshape(70, 257), page)


# ---- aocr_estimate_orientation -----------------------------------------------------------------------------------------------------------------
def _estimate(cuda, page, threshold, light, pitch=None, offset=0, shape=None):
    """raw aocr_estimate_orientation: (orient (8) then 4 sentinels, status); the scratch holds garbage."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=255 if light else 0)
    need = aocr.lib.aocr_orient_scratch_bytes(max(H, 1), max(W, 1))
    scratch = garbage_scratch(cuda, need, 1 << 12)
    out = guarded_words(cuda, 8, 4, SENTINEL, torch.int32)
    st = aocr.lib.aocr_estimate_orientation(None, C.c_void_p(addr), pitch, H, W, threshold, light, aocr.ptr(scratch), aocr.ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy(), st


def _check(cuda, page, threshold, light, pitch=None, offset=0, what=""):
    want = R.estimate_orientation(page, threshold, light)
    for _ in range(2):                                                            # twice: the same words
        got, st = _estimate(cuda, page, threshold, light, pitch, offset)
        assert st == 0, what
        np.testing.assert_array_equal(got[:8], want, err_msg=str(what))
        assert (got[8:] == SENTINEL).all(), what
    return want


@pytest.mark.parametrize("thr,light", [(128, 0), (-1, 0), (128, 1), (-1, 1)], ids=["fixed", "otsu", "fixed_light", "otsu_light"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SHAPES])
def test_estimate_matches_restatement(cuda, shape, thr, light):
    """the bytes around the page are ink (the pitch gap and the base offset hold what the threshold takes for ink): a read beside the page
    changes the counts."""
    H, W, pitch, offset = shape
    page = _seeded(H, W) if not light else (255 - _seeded(H, W)).astype(np.uint8)
    want = _check(cuda, page, thr, light, pitch, offset, shape)
    print(f"[orient] {H}x{W} pitch {pitch} offset {offset} thr {thr} light {light}: {want[:5].tolist()}")
    if H >= 63 and W >= 63:
        assert want[1] > 0 and want[2] > 0 and want[4] > want[1], "the page has no ink"


@pytest.mark.parametrize("case", PAINTED, ids=[c["name"] for c in PAINTED])
def test_estimate_painted_pages(cuda, case):
    want = _check(cuda, case["page"], case["threshold"], case["light_text"], what=case["name"])
    np.testing.assert_array_equal(want, case["want"])
    W = case["page"].shape[1]
    _check(cuda, case["page"], case["threshold"], case["light_text"], W + 7, 5, what=case["name"])


def test_estimate_swaps_under_a_quarter_turn_and_python_surface(cuda):
    import aocr
    page = _seeded(300, 700)
    a = _check(cuda, page, -1, 0)
    turned = aocr.rotate_page_device(torch.from_numpy(page).to(cuda), 1)
    assert turned.shape == (700, 300) and np.array_equal(turned.cpu().numpy(), np.rot90(page, -1))
    b = aocr.estimate_orientation_device(turned).cpu().numpy()
    assert (b[1], b[2], b[3], b[4]) == (a[2], a[1], a[3], a[4]) and b[0] == 1 - a[0] and a[1] != a[2]
    big = torch.zeros((309, 730), dtype=torch.uint8, device=cuda)                # a non-contiguous view; the half turn from the device words
    big[4:304, 11:711] = torch.from_numpy(page).to(cuda)
    view = big[4:304, 11:711]
    half = torch.tensor([2, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=cuda)
    assert np.array_equal(aocr.rotate_page_device(view, 1, half).cpu().numpy(), np.rot90(page, -3))
    assert np.array_equal(aocr.estimate_orientation_device(view, 128, 0).cpu().numpy(), R.estimate_orientation(page, 128, 0))
    with pytest.raises(ValueError):
        aocr.rotate_page_device(view, 4)


def test_estimate_invalid_arguments_leave_the_output_untouched(cuda):
    import aocr
    page = _seeded(70, 257)
    for thr, shape, pitch, word in ((255, None, None, "threshold"), (-2, None, None, "threshold"), (128, (0, 257), None, "page size"),
                                    (128, (70, 16385), 16385, "page size"), (128, None, 256, "pitch")):
        got, st = _estimate(cuda, page, thr, 0, pitch, 0, shape)
        assert st != 0 and word in aocr.last_error(), (thr, shape, pitch, aocr.last_error())
        assert (got == SENTINEL).all()
    assert aocr.lib.aocr_orient_scratch_bytes(0, 5) == 0 and aocr.lib.aocr_orient_scratch_bytes(16384, 4097) == 0
    assert aocr.lib.aocr_orient_scratch_bytes(16384, 4096) % 16 == 0 and aocr.lib.aocr_orient_scratch_bytes(1, 1) > 0
    dev, addr, p = place(cuda, page)
    out = torch.full((8,), SENTINEL, dtype=torch.int32, device=cuda)
    scratch = torch.empty(1 << 10, dtype=torch.int64, device=cuda)
    assert aocr.lib.aocr_estimate_orientation(None, C.c_void_p(addr), p, 70, 257, 128, 0, None, aocr.ptr(out)) != 0
    assert aocr.lib.aocr_estimate_orientation(None, C.c_void_p(addr), p, 70, 257, 128, 0, aocr.ptr(scratch), None) != 0
    assert aocr.lib.aocr_estimate_orientation(None, C.c_void_p(addr), p, 70, 257, 128, 0, C.c_void_p(scratch.data_ptr() + 8), aocr.ptr(out)) != 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- Model.recognize_page(orient=...) -----------------------------------------------------------------------------------------------------------
RECTS = [(4, 14, 6, 40), (4, 14, 50, 70), (4, 14, 90, 139), (24, 33, 3, 20), (24, 33, 31, 60), (46, 58, 10, 80), (46, 58, 100, 128)]   # y0 y1 x0 x1


def test_recognize_page_orient(cuda):
    import aocr
    from model_harness import make
    B, W = 32, 100
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=W, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    H, PW = 64, 150
    page = paint(H, PW, RECTS)
    rects_xyxy = sorted([x0, y0, x1, y1] for y0, y1, x0, x1 in RECTS)
    params = aocr.SegmentParams(threshold=128, min_row_ink=1, merge_gap=2, min_line_h=3, word_gap=4, min_word_w=2, pad_x=0, pad_y=0)
    base = m.recognize_page(page, params, width=100)
    assert sorted(base.boxes.tolist()) == rects_xyxy and base.n_lines == 3                # the boxes are the painted rectangles
    for k in ("orientation", "orient_runs", "orient_scores", "source_boxes"):
        assert not hasattr(base, k)
    for none in (None, False):                                                            # orient=None is the call as it was
        same = m.recognize_page(page, params, width=100, orient=none)
        assert sorted(vars(same)) == sorted(vars(base))
        for k, v in vars(base).items():
            assert np.array_equal(v, getattr(same, k)) if isinstance(v, np.ndarray) else v == getattr(same, k), k

    for q0 in range(4):
        given = np.ascontiguousarray(np.rot90(page, -q0))                                 # the page as the scanner gave it
        q = (4 - q0) % 4
        res = m.recognize_page(given, params, width=100, orient=q)
        np.testing.assert_array_equal(res.boxes, base.boxes)
        np.testing.assert_array_equal(res.labels, base.labels)
        np.testing.assert_array_equal(res.scores, base.scores)
        assert res.text == base.text and res.orientation == q and res.orient_runs is None and res.orient_scores is None
        np.testing.assert_array_equal(res.source_boxes, R.unrotate_boxes(res.boxes, q, *given.shape))
        again = np.full(given.shape, 255, np.uint8)                                       # source_boxes are the rectangles of the page as given
        for x0, y0, x1, y1 in res.source_boxes.tolist():
            again[y0:y1, x0:x1] = 0
        np.testing.assert_array_equal(again, given)
    with pytest.raises(ValueError):
        m.recognize_page(page, params, width=100, orient=4)

    # with deskew, source_corners goes back through the shear and then the rotation: slope 0 here, so the corners are those of source_boxes
    res = m.recognize_page(np.ascontiguousarray(np.rot90(page, -1)), params, width=100, orient=3, deskew=aocr.SkewParams(threshold=128, n_steps=0))
    sb = res.source_boxes
    want = np.stack([np.stack([sb[:, 0], sb[:, 1]], 1), np.stack([sb[:, 0], sb[:, 3] - 1], 1), np.stack([sb[:, 2] - 1, sb[:, 3] - 1], 1),
                     np.stack([sb[:, 2] - 1, sb[:, 1]], 1)], 1)
    assert res.skew_slope_q16 == 0 and res.source_corners.shape == want.shape
    for i in range(len(sb)):
        assert sorted(map(tuple, res.source_corners[i].tolist())) == sorted(map(tuple, want[i].tolist()))

    # automatic: a quarter-turned page of atlas text
    upright = text_page(0, 1, 3)
    given = np.ascontiguousarray(np.rot90(upright, -1))
    auto = m.recognize_page(given, width=100, orient=True)
    ref = R.estimate_orientation(given)
    assert ref[0] == 1 and auto.orient_runs == (int(ref[1]), int(ref[2]))
    assert auto.orientation in (1, 3) and len(auto.orient_scores) == 2 and all(np.isfinite(auto.orient_scores))
    assert auto.orientation == (1 + (2 if auto.orient_scores[1] > auto.orient_scores[0] else 0)) % 4
    assert auto.n_lines == 3 and len(auto.text) == len(auto.boxes) > 3
    np.testing.assert_array_equal(auto.source_boxes, R.unrotate_boxes(auto.boxes, auto.orientation, *given.shape))
    fixed = m.recognize_page(given, width=100, orient=auto.orientation)                   # the same turn asked for by number: the same reading
    np.testing.assert_array_equal(fixed.boxes, auto.boxes)
    np.testing.assert_array_equal(fixed.labels, auto.labels)
    np.testing.assert_array_equal(fixed.scores, auto.scores)
    print(f"[recognize_page orient] runs {auto.orient_runs} scores {auto.orient_scores} -> {auto.orientation} quarter turns, {len(auto.text)} boxes")
    empty = m.recognize_page(np.full((40, 60), 255, np.uint8), orient=True)
    assert empty.orientation == 0 and empty.orient_runs == (0, 0) and empty.orient_scores == (0.0, 0.0) and empty.source_boxes.shape == (0, 4)
    m.check_health()
    m.shutdown()
