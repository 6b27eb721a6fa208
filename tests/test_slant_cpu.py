"""CPU: the restatement of aocr_estimate_slant and of the slanted crop's virtual rectangle (tests/slant_ref.py) against what include/aocr.h
promises -- planted bar words come back exactly, the sign convention and the tie order on hand-written cases, the flag rows -- and
aocr.page.slant_extent against a loop.  tests/test_slant_gpu.py holds the kernels against the same restatement."""
import os
import re

import numpy as np
import pytest

import slant_ref as R
from slant_cases import DEFAULTS, GLYPH_WORDS, PLANTED_K, STROKE, bar_page, bar_word, glyph_word, seeded_page, stroke_5x7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bar_words_come_back_exactly():
    page, boxes, ks = bar_page()
    assert tuple(ks) == PLANTED_K
    slant, scores = R.estimate_slant(page, boxes, len(boxes), **DEFAULTS)
    np.testing.assert_array_equal(slant[:, 0], ks)
    np.testing.assert_array_equal(slant[:, 1], ks * 4096)
    assert (slant[:, 2] == 0).all() and (slant[:, 3] == 5 * 2 * 40).all()
    for i, k in enumerate(ks):                                   # ten full columns of 40, and nothing else reaches that
        assert scores[i, 12 + k] == 10 * 40 * 40 and (np.delete(scores[i], 12 + k) < 10 * 40 * 40).all()
    plain = R.estimate_slant(page, boxes, len(boxes), plain=True, **DEFAULTS)
    assert np.array_equal(plain[0], slant) and np.array_equal(plain[1], scores)


def test_sign_convention_on_the_hand_written_stroke():
    """rows 0..4 inked at columns 5 4 3 2 1: the top is to the right of the foot, a positive slant.  cy = 2; candidate 8 (s = 65536) has the
    offsets +2 +1 0 -1 -2 and reads column 3 in every row: P = [.., 5, ..], score 25.  Candidate 7 (s = 57344) rounds to the same offsets and
    comes first in 0, -1, +1, ...: it wins.  Candidate 4 (s = 32768) has offsets +1 +1 0 0 -1: the pixels land on columns 4 3 3 2 2, score
    1 + 4 + 4 = 9.  Candidate 0 and every negative one leave five columns of one pixel: 5."""
    slant, scores = R.estimate_slant(stroke_5x7(True), [(0, 0, 7, 5)], 1, plain=True, **STROKE)
    assert scores[0].tolist() == [5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 7, 9, 9, 11, 17, 25, 25]
    assert slant[0].tolist() == [7, 7 * 8192, 0, 5]
    slant, scores = R.estimate_slant(stroke_5x7(False), [(0, 0, 7, 5)], 1, plain=True, **STROKE)
    assert scores[0].tolist() == [25, 25, 17, 11, 9, 9, 7, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5] and slant[0].tolist() == [-7, -7 * 8192, 0, 5]
    assert np.array_equal(R.estimate_slant(stroke_5x7(True), [(0, 0, 7, 5)], 1, **STROKE)[1], R.estimate_slant(stroke_5x7(True), [(0, 0, 7, 5)], 1, plain=True, **STROKE)[1])


def test_ties_flags_and_thresholds():
    blank = np.full((20, 30), 255, np.uint8)
    dot = blank.copy()
    dot[7, 11] = 0
    for page, ink, score in ((blank, 0, 0), (dot, 1, 1)):        # every candidate scores the same: 0 wins
        slant, scores = R.estimate_slant(page, [(2, 2, 28, 18)], 1, **DEFAULTS)
        assert slant[0].tolist() == [0, 0, 0, ink] and (scores == score).all()
    tall = np.zeros((300, 12), np.uint8)
    slant, scores = R.estimate_slant(tall, [(0, 0, 12, 257), (0, 0, 12, 256), (5, 5, 5, 9), (9, 3, 4, 8), (40, 0, 50, 10), (-9, -9, 99, 999)], 6, **DEFAULTS)
    assert slant[0].tolist() == [0, 0, 1, 12 * 257] and not scores[0].any()            # taller than 256 rows: the ink only
    assert slant[1].tolist()[1:] == [0, 0, 12 * 256] and scores[1, 12] == 12 * 256 * 256
    assert [s.tolist() for s in slant[2:5]] == [[0, 0, 2, 0]] * 3 and not scores[2:5].any()      # empty, inverted, off the page
    assert slant[5].tolist() == [0, 0, 1, 300 * 12]                                     # clamped to the page on the way in
    # nothing is ink at -1, whatever light_text says; K = 0 has the one candidate
    for light in (0, 1):
        s, sc = R.estimate_slant(dot, [(2, 2, 28, 18)], 1, threshold=-1, light_text=light, step_q16=4096, n_steps=3)
        assert s[0].tolist() == [0, 0, 0, 0] and not sc.any()
    s, sc = R.estimate_slant(dot, [(2, 2, 28, 18)], 1, threshold=128, light_text=1, step_q16=1, n_steps=0)
    assert s[0].tolist() == [0, 0, 0, 26 * 16 - 1] and sc.shape == (1, 1)
    # ink of a neighbour inside the page but outside the box does not count
    page, box = bar_word(5)
    crowded = page.copy()
    crowded[:, :int(box[0])] = 0
    crowded[:, int(box[2]):] = 0
    assert all(np.array_equal(a, b) for a, b in zip(R.estimate_slant(page, [box], 1, **DEFAULTS), R.estimate_slant(crowded, [box], 1, **DEFAULTS)))


def test_plain_loops_and_bincount_agree_on_the_seeded_page():
    page, boxes = seeded_page()
    small = [i for i, b in enumerate(boxes) if 0 < (int(b[2]) - int(b[0])) * (int(b[3]) - int(b[1])) < 4000]
    assert len(small) >= 5
    for kw in (DEFAULTS, dict(DEFAULTS, light_text=1, n_steps=5, step_q16=8192)):
        fast = R.estimate_slant(page, boxes[small], len(small), **kw)
        plain = R.estimate_slant(page, boxes[small], len(small), plain=True, **kw)
        assert np.array_equal(fast[0], plain[0]) and np.array_equal(fast[1], plain[1])


def test_slant_view():
    page, boxes = seeded_page()
    for b in ((30, 40, 90, 72), (-5, -5, 40, 30), (1280, 40, 1400, 100)):
        x0, y0, x1, y1 = R.clamp_box(b, *page.shape)
        np.testing.assert_array_equal(R.slant_view(page, b, 0, 7), page[y0:y1, x0:x1])          # s = 0 is the box itself
    assert R.slant_view(page, (50, 20, 40, 10), 4096, 0) is None
    # s = 65536 on 4 rows (cy = 2): offsets +2 +1 0 -1, D = 2; row r of V is the box's row moved right by D - off
    tiny = np.arange(1, 13, dtype=np.uint8).reshape(4, 3)
    want = np.array([[1, 2, 3, 0, 0, 0, 0], [0, 4, 5, 6, 0, 0, 0], [0, 0, 7, 8, 9, 0, 0], [0, 0, 0, 10, 11, 12, 0]], np.uint8)
    np.testing.assert_array_equal(R.slant_view(tiny, (0, 0, 3, 4), 65536, 0), want)
    np.testing.assert_array_equal(R.slant_view(tiny, (0, 0, 3, 4), 10 ** 6, 0), want)          # clamped to 65536
    np.testing.assert_array_equal(R.slant_view(tiny, (0, 0, 3, 4), -10 ** 6, 9), R.slant_view(tiny, (0, 0, 3, 4), -65536, 9))
    # the ink of a bar word comes back upright: every column of V is all ink or all paper
    page, box = bar_word(-7)
    V = R.slant_view(page, box, -7 * 4096, 255)
    dark = (V < 128).sum(axis=0)
    assert set(dark.tolist()) == {0, 40} and (dark == 40).sum() == 10


def test_slant_extent_against_a_loop():
    import aocr
    rng = np.random.default_rng(5)
    boxes = np.stack([rng.integers(0, 50, 60), rng.integers(0, 400, 60), rng.integers(0, 90, 60), rng.integers(0, 800, 60),
                      np.zeros(60, np.int64), np.zeros(60, np.int64)], axis=1).astype(np.int32)
    s = rng.integers(-70000, 70000, 60)
    s[:4] = (0, 65536, -65536, 10 ** 6)
    got = aocr.page.slant_extent(boxes, s)
    assert got.dtype == np.int32 and got.shape == (60,)
    np.testing.assert_array_equal(got, R.slant_extent(boxes, s))
    assert (got[(boxes[:, 2] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 1])] == 0).all() and got.max() > 100
    assert aocr.slant_extent([(0, 0, 10, 32)], [49152]).tolist() == [12] and aocr.slant_extent(np.zeros((0, 6), np.int32), []).shape == (0,)


def test_glyph_words_land_within_one_step():
    for word, face, k in GLYPH_WORDS:
        page, box = glyph_word(word, face, k)
        slant, _ = R.estimate_slant(page, [box], 1, **DEFAULTS)
        assert slant[0, 2] == 0 and abs(int(slant[0, 0]) - k) <= 1, (word, face, k, slant[0].tolist())


def test_the_library_declares_binds_and_exports_the_calls():
    import aocr
    hdr = open(os.path.join(ROOT, "include", "aocr.h")).read()
    assert re.search(r"#define AOCR_SLANT_MAX_H 256\b", hdr) and aocr._lib.SLANT_MAX_H == R.MAX_H == 256
    for n in ("aocr_slant_scratch_bytes", "aocr_estimate_slant", "aocr_crop_lines_slanted"):
        assert n in aocr._lib.SIGNATURES and getattr(aocr.lib, n) is not None and re.search(r"\b%s\(" % n, hdr)
    p = aocr.SlantParams()
    assert (p.threshold, p.light_text, p.step_q16, p.n_steps, list(p.reserved)) == (-1, 0, 4096, 12, [0, 0, 0, 0])
    import ctypes
    assert ctypes.sizeof(p) == 32
    assert aocr.lib.aocr_slant_scratch_bytes(1000, 12) >= 1000 * 26 * 8 and aocr.lib.aocr_slant_scratch_bytes(1000, 12) % 256 == 0
    for args in ((-1, 12), (65536, 12), (10, -1), (10, 65)):
        assert aocr.lib.aocr_slant_scratch_bytes(*args) == 0 and "bad sizes" in aocr.last_error(), args
    import inspect
    assert inspect.signature(aocr.Model.recognize_page).parameters["deslant"].default is None
    with pytest.raises(ValueError):
        aocr.page_pipeline.slant_params(aocr.SegmentParams(), 5)
