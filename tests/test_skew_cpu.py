"""CPU: the numpy restatement of aocr_estimate_skew / aocr_deskew_page (tests/skew_ref.py) alone: the conditions the GPU tests lean on hold
here -- a planted skew is found to within one step, the deskewed page segments like the straight one, the hand answers, the tie order."""
import numpy as np
import pytest

import segment_ref as R
import skew_ref as S
from skew_cases import PLANTED, PLANTED_K0, SEGMENT, planted_page, tie_page


@pytest.mark.parametrize("k0", PLANTED_K0)
def test_planted_skew_is_found_and_removed(k0):
    straight, skewed = planted_page(k0)
    _, c0 = R.segment_page(straight, **SEGMENT)
    assert c0[1] == 15 and c0[0] > 100                                     # 15 lines of several words each
    skew, scores = S.estimate_skew(skewed, **PLANTED)
    print(f"[skew ref] planted {k0}: estimate {skew.tolist()}")
    assert abs(int(skew[0]) - k0) <= 1 and skew[1] == skew[0] * 64 and skew[2] == 128 and skew[3] == 0
    assert len(scores) == 201 and scores[int(skew[0]) + 100] == scores.max()
    _, c = R.segment_page(S.deskew(skewed, int(skew[1])), **SEGMENT)
    assert c[0] == c0[0] and c[1] == c0[1], (c, c0)                        # the straight page's boxes and lines again
    _, cs = R.segment_page(skewed, **SEGMENT)
    if abs(k0) >= 40:
        assert cs[1] < c0[1], cs                                           # without deskew the lines run into each other
    if k0 == 0:
        assert np.array_equal(skewed, straight)


def test_one_ink_row_by_hand():
    """one inked row of a 20 x 96 page, three strips of 32 with centres 16, 48, 80 about cx = 48.  k = 0 puts all 96 pixels into one profile
    row: 96^2.  Step 4096 gives k = +-1 the offsets (-+2, 0, +-2): three profile rows of 32 pixels, 3 * 32^2."""
    page = np.full((20, 96), 255, np.uint8)
    page[7] = 0
    assert S.offsets(96, 4096) == [-2, 0, 2] and S.offsets(96, -4096) == [2, 0, -2] and S.offsets(96, 0) == [0, 0, 0]
    skew, scores = S.estimate_skew(page, threshold=128, step_q16=4096, n_steps=1)
    assert scores.tolist() == [3 * 32 * 32, 96 * 96, 3 * 32 * 32] and skew.tolist() == [0, 0, 128, 0]
    # equal scores everywhere (one strip: every offset moves the whole row): k = 0 by the order
    one = np.full((9, 32), 255, np.uint8)
    one[4] = 0
    skew, scores = S.estimate_skew(one, threshold=128, step_q16=4096, n_steps=4)
    assert set(scores.tolist()) == {32 * 32} and skew[0] == 0
    # no candidates, no ink, no threshold
    assert S.estimate_skew(page, threshold=128, n_steps=0)[0].tolist() == [0, 0, 128, 0]
    blank = S.estimate_skew(np.full((9, 40), 255, np.uint8), threshold=128, n_steps=3)
    assert blank[0].tolist() == [0, 0, 128, 0] and not blank[1].any()
    assert S.estimate_skew(np.full((9, 40), 77, np.uint8), n_steps=3)[0].tolist() == [0, 0, -1, 0]


def test_two_strips_one_candidate_aligns():
    """W = 64, strip 0 inked on row 5, strip 1 on row 9; step 4096: the offsets of k are (-k, +k), so k = +2 reads rows r-2 and r+2: r = 7
    for both.  No other candidate of -4..4 aligns them."""
    page = np.full((16, 64), 255, np.uint8)
    page[5, :32] = 0
    page[9, 32:] = 0
    assert S.offsets(64, 8192) == [-2, 2] and S.offsets(64, -4096) == [1, -1]
    skew, scores = S.estimate_skew(page, threshold=128, step_q16=4096, n_steps=4)
    assert scores.tolist() == [2048] * 6 + [4096] + [2048] * 2 and skew.tolist() == [2, 8192, 128, 0]
    out = S.deskew(page, 8192)
    # the shear is per pixel: on output row 7 the columns 12..19 read row 5 (offset -2) and 44..51 read row 9 (+2); sx = x there
    assert (out[7, 12:20] == 0).all() and (out[7, 44:52] == 0).all() and (out[7, 20:44] == 255).all()


def test_tie_goes_to_the_negative_candidate():
    skew, scores = S.estimate_skew(tie_page(), threshold=128, step_q16=4096, n_steps=4)
    assert scores[3] == scores[5] == scores.max() == 5120 and (np.delete(scores, [3, 5]) == 3072).all()
    assert skew.tolist() == [-1, -4096, 128, 0]


def test_deskew_identity_fill_and_corners():
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, size=(37, 53), dtype=np.uint8)
    assert np.array_equal(S.deskew(page, 0), page)
    H, W = page.shape
    for s in (64, -4096, 16384, -16384, 99999):
        out = S.deskew(page, s, fill=7)
        sc = min(max(s, -16384), 16384)
        assert np.array_equal(out, S.deskew(page, sc, fill=7))              # clamped
        boxes = np.array([[3, 4, 20, 15], [0, 0, W, H], [25, 18, 26, 19], [10, 30, 50, 37]])
        corners = S.source_corners(boxes, s, H, W)
        assert corners.shape == (4, 4, 2)
        seen_inside = seen_outside = 0
        for bx, cs in zip(boxes, corners):
            for (x, y), (sx, sy) in zip(((bx[0], bx[1]), (bx[2] - 1, bx[1]), (bx[2] - 1, bx[3] - 1), (bx[0], bx[3] - 1)), cs):
                if 0 <= sx < W and 0 <= sy < H:
                    assert out[y, x] == page[sy, sx]
                    seen_inside += 1
                else:
                    assert out[y, x] == 7
                    seen_outside += 1
        assert seen_inside >= 8 and (abs(sc) < 4096 or seen_outside >= 1)
    assert np.array_equal(S.source_corners(boxes, 0, H, W)[0], [[3, 4], [19, 4], [19, 14], [3, 14]])


def test_product_source_corners_is_the_restatement():
    import aocr
    rng = np.random.default_rng(8)
    b = rng.integers(0, 500, size=(20, 6))
    b[:, 2:4] += b[:, 0:2] + 1
    for s in (0, 320, -2560, 16384, -70000):
        assert np.array_equal(aocr.source_corners(b, s, 600, 800), S.source_corners(b, s, 600, 800))
    assert aocr.source_corners(np.zeros((0, 4), np.int32), 64, 10, 10).shape == (0, 4, 2)


def test_params_struct_and_exports():
    import ctypes as C
    import aocr
    p = aocr.SkewParams()
    assert (p.threshold, p.light_text, p.step_q16, p.n_steps) == (-1, 0, 64, 96) and C.sizeof(p) == 16
    for n in ("aocr_skew_scratch_bytes", "aocr_estimate_skew", "aocr_deskew_page"):
        assert n in aocr._lib.SIGNATURES
    assert aocr.lib.aocr_skew_scratch_bytes(3508, 2480, 96) > 0
    for H, W, K in ((0, 10, 1), (10, 16385, 1), (16384, 4097, 1), (10, 10, 257), (10, 10, -1)):
        assert aocr.lib.aocr_skew_scratch_bytes(H, W, K) == 0 and "bad sizes" in aocr.last_error()
