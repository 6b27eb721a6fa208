"""CPU: the numpy restatement of the colour stage (tests/colour_ref.py) against independent formulations -- colorsys for the hue class,
fractions for the balance table, hand-made histograms for the paper estimate -- the host-side argument checks, and the premise of the page
that tests/test_colour_gpu.py reads: dropping the coloured marks gives back the boxes of the unmarked page, plain luma does not."""
import colorsys
from fractions import Fraction

import numpy as np
import pytest

import colour_ref as K
import segment_ref as R
from colour_cases import MARKED_BOXES, MARKED_DROP, MARKED_SEG, PAPER_TINT, all_paper, marked_page, random_rgb


def test_hue_class_matches_colorsys_away_from_the_boundaries():
    """class k is the 60-degree sector centred on k * 60 degrees.  A colour is left out when moving one channel by one level could take it
    across a boundary at 30 + k * 60 degrees: the integer rule and the float hue may then disagree on the side."""
    levels = np.arange(0, 256, 15)
    checked = 0
    for r in levels:
        for g in levels:
            for b in levels:
                if max(r, g, b) == min(r, g, b):
                    continue
                hues = [colorsys.rgb_to_hsv(*(np.clip(np.array([r, g, b]) + d, 0, 255) / 255.0))[0] * 360.0
                        for d in ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
                sectors = {int(((h + 30.0) % 360.0) // 60.0) for h in hues}
                if len(sectors) != 1 or any(abs(((h + 30.0) % 60.0)) < 1e-9 for h in hues):
                    continue
                cls, c = K.hue_class(r, g, b)
                assert int(cls) == sectors.pop(), (r, g, b)
                assert int(c) == max(r, g, b) - min(r, g, b)
                checked += 1
    assert checked > 3000


def test_primaries_secondaries_and_the_orange_boundary():
    for rgb, want in (((255, 0, 0), K.RED), ((255, 255, 0), K.YELLOW), ((0, 255, 0), K.GREEN), ((0, 255, 255), K.CYAN), ((0, 0, 255), K.BLUE),
                      ((255, 0, 255), K.MAGENTA), ((255, 128, 0), K.YELLOW), ((255, 127, 0), K.RED)):
        assert int(K.hue_class(*rgb)[0]) == want, rgb


def test_balance_table_matches_fractions():
    for p in (1, 2, 3, 100, 127, 128, 200, 240, 250, 254, 255):
        # v * 255 / p rounded half up.  For even p the integer rule adds exactly p / 2; for odd p it adds (p - 1) / 2, which rounds the same
        # way because a quotient by an odd p never has a fractional part of exactly 1/2
        exact = [min(255, (Fraction(v * 255, p) + Fraction(1, 2)).__floor__()) for v in range(256)]
        assert K.lut(p).tolist() == exact, p
    assert K.lut(255).tolist() == list(range(256))                     # the identity
    assert K.lut(200)[200] == 255 and K.lut(200)[255] == 255 and K.lut(200)[100] == 128


def test_window_mode_on_hand_made_histograms():
    h = np.zeros(256, np.int64)
    h[200] = 10
    assert K.window_mode(h, 128) == 202                                 # the windows of 198..202 all hold 10: the largest v
    h[204] = 1
    assert K.window_mode(h, 128) == 202                                 # 202's window is the only one that holds both
    h[:] = 0
    h[255] = 7
    assert K.window_mode(h, 128) == 255                                 # the window is clipped at 255
    h[:] = 0
    h[254] = 5
    h[250] = 5
    assert K.window_mode(h, 128) == 252                                 # both inside 250..254 only
    h[:] = 0
    h[100] = 50
    assert K.window_mode(h, 128) == 255                                 # no pixel >= paper_min
    h[127] = 50
    assert K.window_mode(h, 128) == 255                                 # 127 is inside 128's window, but it is no pixel >= paper_min
    h[128] = 1
    assert K.window_mode(h, 128) == 129                                 # 128 and 129 see 127, 128: 51 each; the larger v
    h[:] = 0
    h[130] = 3
    h[140] = 3
    assert K.window_mode(h, 128) == 142                                 # a tie between two windows: the larger v
    assert K.window_mode(h, 135) == 142
    assert K.window_mode(h, 143) == 255


def test_estimate_and_gray_on_a_small_page():
    rgb = all_paper(4, 5)
    rgb[0, 0] = (255, 0, 0)
    words = K.estimate_paper(rgb)
    assert words.tolist() == [252, 242, 202, 1] + [0] * 12             # a constant channel: the windows of v-2..v+2 tie, the largest v
    gray, out = K.gray_page(rgb, words, drop=1 << K.RED, fill=9)
    paper = (77 * int(K.lut(252)[250]) + 150 * int(K.lut(242)[240]) + 29 * int(K.lut(202)[200]) + 128) >> 8
    assert gray[0, 0] == 9 and (gray.reshape(-1)[1:] == paper).all() and paper == 253
    assert out.tolist()[:4] == [252, 242, 202, 1] and out[4 + K.RED] == 1 and out[10] == 1 and out[4:11].sum() == 2
    same, out2 = K.gray_page(rgb, None, balance=0)
    assert same[1, 1] == (77 * 250 + 150 * 240 + 29 * 200 + 128) >> 8 and out2.tolist()[:4] == [255, 255, 255, 0]
    red, _ = K.gray_page(rgb, None, balance=0, weights=(256, 0, 0))
    np.testing.assert_array_equal(red, rgb[:, :, 0])
    dark, _ = K.gray_page(rgb, None, balance=0, mode=1)
    np.testing.assert_array_equal(dark, rgb.min(axis=2))


def test_colour_params_validation():
    import aocr
    p = aocr.ColourParams()
    assert (list(p.weights), p.mode, p.balance, list(p.paper), p.paper_min, p.chroma_min, p.drop, p.fill) == \
        ([77, 150, 29], 0, 1, [-1, -1, -1], 128, 64, 0, 255)
    assert (aocr.HUE_RED, aocr.HUE_YELLOW, aocr.HUE_GREEN, aocr.HUE_CYAN, aocr.HUE_BLUE, aocr.HUE_MAGENTA) == tuple(range(6))
    q = aocr.ColourParams(weights=(256, 0, 0), mode=1, balance=0, paper=(250, 240, 200), paper_min=1, chroma_min=255, drop=63, fill=0)
    assert list(q.paper) == [250, 240, 200] and q.drop == 63
    for bad in (dict(weights=(77, 150, 30)), dict(weights=(-1, 257, 0)), dict(weights=(128, 128)), dict(mode=2), dict(mode=-1), dict(balance=2),
                dict(paper=(0, 10, 10)), dict(paper=(10, 10, 256)), dict(paper=(10, 10)), dict(paper_min=0), dict(paper_min=256),
                dict(chroma_min=0), dict(chroma_min=256), dict(drop=-1), dict(drop=64), dict(fill=-1), dict(fill=256)):
        with pytest.raises(ValueError):
            aocr.ColourParams(**bad)


def test_scratch_bytes_rejects_bad_sizes():
    import aocr
    assert aocr.lib.aocr_colour_scratch_bytes(70, 257) > 0
    for H, W in ((0, 10), (10, 0), (-1, 10), (16385, 1), (1, 16385), (16384, 8192)):
        assert aocr.lib.aocr_colour_scratch_bytes(H, W) == 0, (H, W)
        assert "bad sizes" in aocr.last_error()


def test_integer_luma_stays_within_one_level_of_rgb2y():
    """the number DESIGN.md section 21 quotes: over all 2^24 colours, (77 r + 150 g + 29 b + 128) >> 8 against round(0.299 r + 0.587 g +
    0.114 b) (255 * rgb2y of a pixel in 0..1)."""
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    worst = 0
    for r in range(256):
        mine = (77 * r + 150 * g + 29 * b + 128) >> 8
        ref = np.floor(0.299 * r + 0.587 * g + 0.114 * b + 0.5).astype(np.int64)
        worst = max(worst, int(np.abs(mine - ref).max()))
    assert worst == 1


def test_premise_dropping_the_marks_gives_back_the_unmarked_boxes():
    want = np.array(MARKED_BOXES, np.int32)
    plain, _ = K.gray(marked_page(marks=False))
    boxes, counts = R.segment_page(plain, **MARKED_SEG)
    np.testing.assert_array_equal(boxes, want)
    assert counts[1] == 2

    rgb = marked_page()
    clean, words = K.gray(rgb, drop=MARKED_DROP)
    assert words[:4].tolist() == [PAPER_TINT[0] + 2, PAPER_TINT[1] + 2, PAPER_TINT[2] + 2, 1]       # noiseless paper: the tie's largest v
    boxes, counts = R.segment_page(clean, **MARKED_SEG)
    np.testing.assert_array_equal(boxes, want)
    assert words[4 + K.RED] > 0 and words[4 + K.YELLOW] > 0 and words[4 + K.BLUE] > 0 and words[10] == words[4:10].sum()

    luma, words = K.gray(rgb)                                           # nothing dropped: the rule joins the lines, the speck fuses two words
    boxes, counts = R.segment_page(luma, **MARKED_SEG)
    assert counts[1] < 2 or len(boxes) < len(want)
    assert words[10] == 0

    host, _ = K.gray_page(rgb, None, balance=0)                          # the reduction a caller does on the host today
    boxes, counts = R.segment_page(host, **MARKED_SEG)
    assert counts[1] < 2 or len(boxes) < len(want)


def test_random_pages_populate_both_sides_of_the_chroma_threshold():
    rgb = random_rgb(70, 43, 7043)
    _, words = K.gray_page(rgb, None, balance=0)
    assert (words[4:10] > 0).all() and 0 < words[4:10].sum() < 70 * 43
