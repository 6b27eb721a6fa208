"""CPU: the numpy restatement of aocr_binarize_page (tests/binarize_ref.py) alone: the hand answers, the property that the fixed threshold
127 on the output is the local decision, and the result the call exists for -- a stained, faded page that no global threshold can segment
segments like the clean page once binarised."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import binarize_ref as B
import flatten_ref as F
import segment_ref as R
from binarize_cases import CASES, FADED, FADED_ROW, PAPER, STAIN, STAIN_CORE, hard_of, stained_page
from segment_cases import seeded_page

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases(case):
    _, page, (r, k, rng), want = case
    got, counts = B.binarize(page, r, k, rng)
    np.testing.assert_array_equal(got, want)
    assert counts[0] == (want <= 127).sum() and counts[3] == 0
    hard, hard_counts = B.binarize(page, r, k, rng, hard=1)
    np.testing.assert_array_equal(hard, hard_of(want))
    assert hard_counts.tolist() == counts.tolist()
    inv, inv_counts = B.binarize((255 - page).astype(np.uint8), r, k, rng, light_text=1)      # light_text is the mirror image
    np.testing.assert_array_equal(inv, 255 - want)
    assert inv_counts.tolist() == counts.tolist()


def test_constant_pages_hold_no_ink_and_k0_is_the_mean():
    for c in (1, 2, 93, 254, 255):
        out, counts = B.binarize(np.full((9, 11), c, np.uint8), 3)
        assert counts.tolist() == [0, c * 205 // 256, c * 205 // 256, 0] and (out >= 128).all()
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, size=(12, 17), dtype=np.uint8)
    T = B.thresholds(page.astype(np.int64), 2, 0, 128)
    S, nx = F.window_sum(page.astype(np.int64), 2, 1)
    S, ny = F.window_sum(S, 2, 0)
    np.testing.assert_array_equal(T, S // (ny[:, None] * nx[None, :]))
    np.testing.assert_array_equal(T, B.thresholds(page.astype(np.int64), 2, 0, 1))           # R drops out with k = 0


def test_thresholds_equal_the_double_loop_with_isqrt():
    """every pixel of two small pages against the header's own loop and math.isqrt; and the vectorised square root on its hard cases."""
    for H, W, seed, r, k, rng in ((9, 37, 9037, 3, 51, 128), (23, 19, 7, 63, 255, 1), (14, 30, 2, 1, 128, 255)):
        page = seeded_page(H, W, seed)
        T = B.thresholds(page.astype(np.int64), r, k, rng)
        want = np.array([[B.threshold_at(page, x, y, r, k, rng) for x in range(W)] for y in range(H)])
        np.testing.assert_array_equal(T, want)
    q = np.array([0, 1, 2, 3, 94906265, 2965820, 2965821], np.int64)
    D = np.concatenate([q * q, q[1:] * q[1:] - 1, q * q + 2 * q, np.array([(1 << 43) - 1])])
    np.testing.assert_array_equal(B.isqrt(D), [math.isqrt(int(d)) for d in D])


@pytest.mark.parametrize("light_text", [0, 1], ids=["dark", "light"])
@pytest.mark.parametrize("hard", [0, 1], ids=["gray", "hard"])
def test_threshold_127_on_the_output_is_the_local_decision(hard, light_text):
    for H, W, seed, r, k, rng in ((40, 100, 3, 3, 51, 128), (70, 257, 70257, 20, 51, 128), (40, 100, 4, 5, 255, 1), (33, 65, 8, 2, 0, 255)):
        page = seeded_page(H, W, seed, light=bool(light_text))
        v = 255 - page.astype(np.int64) if light_text else page.astype(np.int64)
        ink = v <= B.thresholds(v, r, k, rng)
        out, counts = B.binarize(page, r, k, rng, light_text, hard)
        np.testing.assert_array_equal((out > 127) if light_text else (out <= 127), ink)      # is_ink(out, 127, light_text) of page_common.h
        assert counts[0] == ink.sum() and (rng == 1) == bool(ink.all()) and ink.any()   # R = 1 with k = 255 / 256: T is far above 255
        if hard:
            assert set(np.unique(out).tolist()) <= {0, 255}
            gray, _ = B.binarize(page, r, k, rng, light_text, 0)
            np.testing.assert_array_equal(out, hard_of(gray))                                 # the two modes agree on the ink map


def test_gray_output_keeps_the_order_of_the_levels_on_either_side():
    """inside one window class the gray output is monotone in v: darker ink stays darker, lighter paper lighter (the anti-aliasing)."""
    T = 150
    v = np.arange(256)
    out = np.where(v <= T, (v * 127) // T, np.minimum(255, 128 + ((v - T - 1) * 127) // (254 - T)))
    assert (np.diff(out) >= 0).all() and out[T] == 127 and out[T + 1] == 128 and out[0] == 0 and out[255] == 255


def _lines_and_boxes(page, **kw):
    boxes, counts = R.segment_page(page, **kw)
    return boxes, int(counts[0]), int(counts[1])


def test_stained_faded_page_no_global_threshold_segments_it_binarize_does():
    clean, stained = stained_page()
    want, n_boxes, n_lines = _lines_and_boxes(clean)
    assert (n_boxes, n_lines) == (109, 15)
    y0, y1, x0, x1 = STAIN_CORE
    core = stained[y0:y1, x0:x1]
    assert core.max() == STAIN < FADED == stained[FADED_ROW:][clean[FADED_ROW:] < 128].max() and stained.max() == PAPER
    results = {}
    for t in list(range(255)) + [-1]:                                          # every fixed threshold, and Otsu's
        _, nb, nl = _lines_and_boxes(stained, threshold=t)
        results[t] = (nb, nl)
        assert nl < 15, (t, nb, nl)                                            # lines lost (the faded half) or merged (under the stain)
    print(f"[binarize ref] global thresholds on the stained page: Otsu {results[-1]}, t=100 {results[100]}, t=139 {results[139]}, "
          f"t=174 {results[174]}, t=175 {results[175]}, t=200 {results[200]} (boxes, lines; the clean page (109, 15))")
    flat = F.flatten(stained, 16)
    fb, fnb, fnl = _lines_and_boxes(flat)
    print(f"[binarize ref] flatten(16) + Otsu on the stained page: {fnb} boxes in {fnl} lines")
    assert fnl < 15                                                            # 58 boxes in 8 lines: flatten does not touch the faded ink
    for hard in (0, 1):
        out, counts = B.binarize(stained, hard=hard)
        got, nb, nl = _lines_and_boxes(out, threshold=127)
        assert (nb, nl) == (109, 15), (hard, nb, nl)
        np.testing.assert_array_equal(got[:, :5], want[:, :5])
        np.testing.assert_array_equal((out <= 127), clean < 128)              # the ink map is the clean page's, pixel for pixel
        print(f"[binarize ref] hard={hard}: counts {counts.tolist()}")
    inv, _ = B.binarize((255 - stained).astype(np.uint8), light_text=1)
    got, nb, nl = _lines_and_boxes(inv, threshold=127, light_text=1)
    assert (nb, nl) == (109, 15)
    np.testing.assert_array_equal(got[:, :5], want[:, :5])


def test_params_struct_exports_and_stage_arguments():
    import aocr
    from aocr.page_pipeline import binarize_stage, binarized_params
    p = aocr.BinarizeParams()
    assert (p.radius, p.k_q8, p.range, p.light_text, p.hard, list(p.reserved)) == (20, 51, 128, 0, 0, [0, 0, 0]) and C.sizeof(p) == 32
    assert {k: getattr(p, k) for k in B.DEFAULTS} == B.DEFAULTS
    q = aocr.BinarizeParams(radius=7, k_q8=90, range=64, light_text=1, hard=1)
    assert (q.radius, q.k_q8, q.range, q.light_text, q.hard) == (7, 90, 64, 1, 1)
    hdr = open(os.path.join(ROOT, "include", "aocr.h")).read()
    body = re.search(r"typedef struct aocr_binarize_params \{(.*?)\} aocr_binarize_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(1), int(m.group(2) or 1)) for m in re.finditer(r"int32_t\s+(\w+)(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("radius", 1), ("k_q8", 1), ("range", 1), ("light_text", 1), ("hard", 1), ("reserved", 3)]
    assert [(n, C.sizeof(t) // 4) for n, t in aocr.BinarizeParams._fields_] == fields
    for n in ("aocr_binarize_scratch_bytes", "aocr_binarize_page"):
        assert n in aocr._lib.SIGNATURES
    for n in ("BinarizeParams", "binarize_page_device"):
        assert n in aocr.__all__ and n in aocr.page.__all__ and hasattr(aocr, n)
    assert aocr.lib.aocr_binarize_scratch_bytes(3508, 2480, 20) > 0 and aocr.lib.aocr_binarize_scratch_bytes(16384, 4096, 63) > 0
    for H, W, r in ((0, 10, 20), (10, 16385, 20), (16384, 4097, 20), (10, 10, 0), (10, 10, 64), (10, 10, -1)):
        assert aocr.lib.aocr_binarize_scratch_bytes(H, W, r) == 0 and "bad sizes" in aocr.last_error()
    sig = inspect.signature(aocr.Model.recognize_page)
    assert sig.parameters["binarize"].default is None
    seg = aocr.SegmentParams(light_text=1, word_gap=9)
    assert binarize_stage("page", None, seg, None) == ("page", None, None) and binarize_stage("page", None, seg, False) == ("page", None, None)
    for bad in (3, "yes", 1.5, aocr.FlattenParams()):
        with pytest.raises(ValueError, match="BinarizeParams"):
            binarize_stage("page", None, seg, bad)
    fixed = binarized_params(seg)                                              # Otsu becomes 127 on a copy
    assert fixed is not seg and seg.threshold == -1 and fixed.threshold == 127
    assert [getattr(fixed, f) for f, _ in seg._fields_][1:] == [getattr(seg, f) for f, _ in seg._fields_][1:]
    mine = aocr.SegmentParams(threshold=90)
    assert binarized_params(mine) is mine
