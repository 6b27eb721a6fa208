"""CPU: the restatement of aocr_estimate_glyph_size and aocr_resize_page (tests/scale_ref.py) against what include/aocr.h promises --
the resize identities, the hand-painted glyph cases, the atlas pages -- aocr.scale_plan, and the motive: a page scanned at half the
resolution loses words under the default segment parameters and gets them back after estimate, plan and resize."""
import numpy as np
import pytest

import orient_cases as OC
import scale_cases as SC
import scale_ref as S
import segment_ref as SR


def _seeded(H, W):
    return np.random.default_rng(31 * H + W).integers(0, 256, (H, W), dtype=np.uint8)


# ---- the resize ------------------------------------------------------------------------------------------------------------------------------
def test_prefix_sum_form_is_the_definition():
    for H, W, Ho, Wo in ((7, 9, 7, 9), (7, 9, 3, 4), (7, 9, 20, 31), (16, 16, 2, 2), (3, 3, 24, 24), (1, 7, 1, 3), (7, 1, 15, 1), (63, 129, 47, 100)):
        p = _seeded(H, W)
        np.testing.assert_array_equal(S.resize_page(p, Ho, Wo), S.resize_direct(p, Ho, Wo), err_msg=str((H, W, Ho, Wo)))


def test_equal_sizes_copy():
    p = _seeded(33, 65)
    np.testing.assert_array_equal(S.resize_page(p, 33, 65), p)


@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_integer_shrink_is_the_rounded_block_mean(k):
    p = _seeded(5 * k, 7 * k).astype(np.int64)
    want = (p.reshape(5, k, 7, k).sum(axis=(1, 3)) + k * k // 2) // (k * k)
    np.testing.assert_array_equal(S.resize_page(p.astype(np.uint8), 5, 7), want)


@pytest.mark.parametrize("scale", [2, 4])
def test_integer_shrink_is_orient_cases_shrunk(scale):
    """orient_cases.shrunk's formula on the atlas itself: every glyph cell of a face shrunk in one call."""
    pixels, _ = OC.atlas()
    G, gh, gw = pixels[0].shape
    sheet = np.ascontiguousarray(pixels[0].reshape(G * gh, gw))
    want = OC.shrunk(0, scale)[0].reshape(G * gh // scale, gw // scale)
    np.testing.assert_array_equal(S.resize_page(sheet, G * gh // scale, gw // scale), want)


@pytest.mark.parametrize("k", [2, 3, 8])
def test_integer_growth_is_kron(k):
    p = _seeded(6, 11)
    np.testing.assert_array_equal(S.resize_page(p, 6 * k, 11 * k), np.kron(p, np.ones((k, k), np.uint8)))


def test_a_constant_page_stays_constant():
    for v in (0, 1, 127, 254, 255):
        assert (S.resize_page(np.full((13, 29), v, np.uint8), 31, 10) == v).all()
        assert (S.resize_page(np.full((13, 29), v, np.uint8), 5, 57) == v).all()


# ---- the estimator ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.HAND, ids=[c["name"] for c in SC.HAND])
def test_hand_cases(case):
    np.testing.assert_array_equal(S.estimate_glyph_size(case["page"], **case["params"]), case["want"])


_atlas_words = {}


def _atlas_estimate(face, scale):
    if (face, scale) not in _atlas_words:
        _atlas_words[(face, scale)] = S.estimate_glyph_size(SC.text_page(face, scale), threshold=128)
    return _atlas_words[(face, scale)]


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("face", [0, 1, 2])
def test_atlas_median(face, scale):
    g = _atlas_estimate(face, scale)
    print(f"[glyph size] face {face} scale {scale}: {g.tolist()}")
    assert g[0] == SC.ATLAS_MEDIAN[(scale, face)] and g[1] <= g[0] <= g[2] and g[3] >= 300


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("face", [0, 1, 2])
def test_atlas_estimate_is_unchanged_under_a_quarter_turn(face, scale):
    turned = np.ascontiguousarray(np.rot90(SC.text_page(face, scale)))
    np.testing.assert_array_equal(S.estimate_glyph_size(turned, threshold=128), _atlas_estimate(face, scale))


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("face", [0, 1, 2])
def test_atlas_estimate_doubles_under_kron(face, scale):
    g = _atlas_estimate(face, scale)
    twice = np.kron(SC.text_page(face, scale), np.ones((2, 2), np.uint8))
    assert S.estimate_glyph_size(twice, threshold=128)[0] == 2 * g[0]                       # the size; dots of side 1 now count, n may grow
    big = S.estimate_glyph_size(twice, threshold=128, min_size=4, max_size=1024)            # with the limits doubled too, everything doubles
    np.testing.assert_array_equal(big[:3], 2 * g[:3])
    np.testing.assert_array_equal(big[3:6], g[3:6])
    assert big[6] == 4 * g[6]


def test_atlas_shrunk_four_times_is_noise():
    """what min_glyphs and the quartiles are for: at a quarter of the atlas size the quartiles span 2..4."""
    g = S.estimate_glyph_size(OC.text_page(0, 4), threshold=128)
    assert 2 <= g[1] <= g[2] <= 4


# ---- aocr.scale_plan -------------------------------------------------------------------------------------------------------------------------
def test_scale_plan_dead_band_rounding_clamps_and_min_glyphs():
    import aocr
    plan = aocr.scale_plan
    # target 16, tolerance 1.25: 16 / 20 = 1 / 1.25 and 16 / 13 = 1.23 are inside, 21 and 12 (16 / 12 = 1.33) outside
    for size in (13, 14, 16, 18, 20):
        assert plan(size, 100, 600, 800) is None, size
    assert plan(21, 100, 600, 800) == ((2 * 800 * 16 + 21) // 42, (2 * 600 * 16 + 21) // 42) == (610, 457)
    assert plan(12, 100, 600, 800) == (1067, 800)                                          # 800 * 16 / 12 = 1066.67 rounds up
    assert plan(32, 100, 601, 801) == (401, 301)                                           # 400.5 and 300.5 round up: (2*L*t + size) // (2*size)
    assert plan(8, 100, 600, 800) == (1600, 1200)
    p = aocr.ScaleParams(target=32, tolerance=1.0)
    assert plan(32, 100, 600, 800, p) is None and plan(31, 100, 600, 800, p) == (826, 619)
    # min_glyphs and an empty estimate
    assert plan(8, 7, 600, 800) is None and plan(8, 8, 600, 800) == (1600, 1200) and plan(0, 100, 600, 800) is None
    assert plan(8, 3, 600, 800, aocr.ScaleParams(min_glyphs=3)) == (1600, 1200)
    # the clamps: a factor of 8 either way, 1..16384, Ho*Wo <= 2^26
    assert plan(1, 100, 60, 80) == (640, 480)                                              # 16x asked for, 8x given
    assert plan(512, 100, 600, 801) == (101, 75)                                           # 1 / 32 asked for, ceil(L / 8) given
    assert plan(2, 100, 100, 4000) == (16384, 800)
    Wo, Ho = plan(4, 100, 4000, 4000)                                                      # 16000 x 16000 asked for
    assert Ho * Wo <= 1 << 26 and Wo == Ho and (Wo + 1) * (Ho + 1) > 1 << 26
    Wo, Ho = plan(4, 100, 16384, 4096)                                                     # 16384 x 16384 after the side clamp
    assert Ho * Wo <= 1 << 26 and Wo <= 16384 and Ho <= 16384 and 4096 <= 8 * Wo and 16384 <= 8 * Ho
    # the restatement agrees wherever the product clamp is not met
    for size in range(1, 70):
        for H, W in ((600, 800), (61, 1009), (3508, 2480)):
            want = S.scale_plan(size, 50, H, W)
            if want is None or want[0] * want[1] <= 1 << 26:
                assert plan(size, 50, H, W) == want, (size, H, W)
    x, y = aocr.unscale_points([0, 799], [0, 599], 1200, 1600, 600, 800)
    np.testing.assert_array_equal(x, [0.5, 1598.5])
    np.testing.assert_array_equal(y, [0.5, 1198.5])
    d = aocr.ScaleParams()
    assert (d.target, d.tolerance, d.min_glyphs) == (16, 1.25, 8)
    assert (d.glyph.threshold, d.glyph.connectivity, d.glyph.min_size, d.glyph.max_size, d.glyph.max_aspect) == (-1, 8, 2, 512, 8)


# ---- the motive --------------------------------------------------------------------------------------------------------------------------------
def test_motive_default_segmentation_loses_words_at_half_resolution_and_scale_brings_them_back():
    """24 words, 18 columns apart, at the atlas size: the default segment parameters (word_gap 12) find all 24.  Scanned at half the
    resolution the spaces are 9 columns and the defaults find 9 boxes.  The estimate reads 8 pixels on that page, the plan doubles it, and the
    defaults find 24 again.  The three counts are those of DESIGN.md section 19."""
    page, n_words = SC.word_page()
    H, W = page.shape
    native = SR.segment_page(page)[1]
    small = S.resize_page(page, H // 2, (W + 1) // 2)
    lost = SR.segment_page(small)[1]
    g = S.estimate_glyph_size(small)
    plan = S.scale_plan(int(g[0]), int(g[3]), *small.shape)
    assert g[0] == 8 and plan == (2 * small.shape[1], 2 * small.shape[0])
    back = SR.segment_page(S.resize_page(small, plan[1], plan[0]))[1]
    print(f"[scale motive] words {n_words}: native {native.tolist()}, half {lost.tolist()}, glyph {g.tolist()}, plan {plan}, rescaled {back.tolist()}")
    assert (int(native[0]), int(lost[0]), int(back[0])) == SC.MOTIVE_COUNTS and n_words == SC.MOTIVE_COUNTS[0]
    assert native[1] == lost[1] == back[1] == 4
    assert S.scale_plan(*[int(v) for v in S.estimate_glyph_size(page)[[0, 3]]], H, W) is None          # the native page is left alone
