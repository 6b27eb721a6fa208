"""CPU: the numpy restatement of the rectification specs (tests/rectify_ref.py) against hand-computed answers and its own consequences, and
the host-only aocr_rectify_plan against it with exact equality of the nine doubles and the two sizes."""
import ctypes as C

import numpy as np
import pytest

import rectify_cases as RC
import rectify_ref as R
import segment_ref as S
from segment_cases import seeded_page


def test_plan_of_an_axis_aligned_rectangle_is_exact():
    x0, y0, w, h = 7, 11, 40, 25
    (Wo, Ho), c = R.rectify_plan([x0, y0, x0 + w, y0, x0 + w, y0 + h, x0, y0 + h])
    assert (Wo, Ho) == (w + 1, h + 1)
    np.testing.assert_array_equal(c, [w * h, 0, x0 * w * h, 0, h * w, y0 * w * h, 0, 0, w * h])       # g = h = 0: integers below 2^53
    y, x = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    X, Y, dn = R.warp_points(c, x, y)
    np.testing.assert_array_equal(X, x + x0)
    np.testing.assert_array_equal(Y, y + y0)
    page = seeded_page(60, 70, 3)
    np.testing.assert_array_equal(R.warp_page(page, c, 255, Ho, Wo), page[y0:y0 + h + 1, x0:x0 + w + 1])


def test_plan_default_sizes_at_perfect_squares_and_one_below():
    # a parallelogram: top and bottom edges (30, 40), 2500 = 50^2 exactly; left and right (0, 60), 3600 = 60^2
    assert R.rectify_plan([0, 0, 30, 40, 30, 100, 0, 60])[0] == (51, 61)
    # edges (8, 4): 80 = 9^2 - 1, one below a square: 8; (0, 12): 144 = 12^2
    assert R.rectify_plan([0, 0, 8, 4, 8, 16, 0, 12])[0] == (9, 13)
    # a diamond, every edge (12, 12): 288 = 17^2 - 1: 16
    assert R.rectify_plan([0, 0, 12, 12, 0, 24, -12, 12])[0] == (17, 17)
    # the longer of the two opposite edges counts: top 2500 against bottom (29, 40) 2441; left 3600 against right (-1, 60) 3601 -> 60
    assert R.rectify_plan([0, 0, 30, 40, 29, 100, 0, 60])[0] == (51, 61)
    # top (48, 14) 2500 against bottom (49, 14) 2597 = 51^2 - 4 -> 50; left (0, 24) 576 = 24^2 against right (1, 24) 577 -> 24
    assert R.rectify_plan([0, 0, 48, 14, 49, 38, 0, 24])[0] == (51, 25)
    # a size given is taken as it is, the other one is still computed
    assert R.rectify_plan([0, 0, 30, 40, 29, 100, 0, 60], 17, 0)[0] == (17, 61)
    assert R.rectify_plan([0, 0, 30, 40, 29, 100, 0, 60], 0, 9)[0] == (51, 9)


BAD_QUADS = {
    "not_convex": [0, 0, 50, 0, 10, 10, 0, 50],
    "counter_clockwise": [0, 0, 0, 50, 50, 50, 50, 0],
    "repeated_corner": [0, 0, 50, 0, 50, 0, 0, 50],
    "all_the_same": [5, 5, 5, 5, 5, 5, 5, 5],
    "collinear": [0, 0, 10, 0, 20, 0, 30, 0],
    "bow_tie": [0, 0, 50, 0, 0, 50, 50, 50],
}


@pytest.mark.parametrize("name", sorted(BAD_QUADS))
def test_plan_rejects_bad_quads(name):
    with pytest.raises(ValueError):
        R.rectify_plan(BAD_QUADS[name])


def test_plan_rejects_an_oversized_output():
    big = [0, 0, 16384, 0, 16384, 100, 0, 100]
    with pytest.raises(ValueError, match="16385"):
        R.rectify_plan(big)
    assert R.rectify_plan(big, 16384, 0)[0] == (16384, 101)
    with pytest.raises(ValueError):
        R.rectify_plan([0, 0, 9000, 0, 9000, 9000, 0, 9000])                  # 9001^2 > 2^26
    with pytest.raises(ValueError):
        R.rectify_plan([0, 0, 10, 0, 10, 10, 0, 10], 8193, 8192)


def _random_quads(n, seed):
    """seeded convex quads: a rectangle's corners, each moved by less than a third of the shorter side."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        w, h = rng.randint(8, 3000, 2)
        x0, y0 = rng.randint(-50, 2000, 2)
        j = rng.randint(-(min(w, h) // 3), min(w, h) // 3 + 1, 8)
        q = [x0 + j[0], y0 + j[1], x0 + w + j[2], y0 + j[3], x0 + w + j[4], y0 + h + j[5], x0 + j[6], y0 + h + j[7]]
        if R.quad_valid(q):
            out.append([int(v) for v in q])
    return out


def _all_quads():
    qs = [c["quad"] for c in RC.PHOTO_QUADS.values()] + [RC.text_photo()[2]]
    for H, W, _, _ in RC.WARP_SHAPES:
        if H >= 2 and W >= 2:
            qs += [RC.image_quad(H, W), [W // 3, 0, W - 1 - W // 3, 1, W - 1, H - 1, 0, H - 2],
                   [-(W // 3), -(H // 4), W + W // 5, H // 6, W - 1, H + H // 3, W // 5, H - 1]]
    return qs + _random_quads(300, 20261019)


def test_warp_points_sends_the_output_corners_to_the_quad():
    for q in _all_quads():
        (Wo, Ho), c = R.rectify_plan(q)
        X, Y, dn = R.warp_points(c, [0, Wo - 1, Wo - 1, 0], [0, 0, Ho - 1, Ho - 1])
        assert (dn > 0).all()
        np.testing.assert_allclose(np.stack([X, Y], 1).reshape(-1), q, rtol=0, atol=1e-9, err_msg=str(q))


def test_photo_quads_are_found_exactly():
    """every make_photo case: the corners are the unique extremes of x+y and x-y over the polygon (checked here), the sheet is one component,
    and the restatement returns them, with Otsu and with a fixed threshold."""
    for name, c in RC.PHOTO_QUADS.items():
        ph, q = RC.photo(name)
        ys, xs = np.nonzero(R.inside_quad(q, c["H"], c["W"]))
        for key, pick, corner in ((xs + ys, np.min, 0), (xs - ys, np.max, 1), (xs + ys, np.max, 2), (xs - ys, np.min, 3)):
            at = np.nonzero(key == pick(key))[0]
            assert len(at) == 1 and [xs[at[0]], ys[at[0]]] == q[2 * corner:2 * corner + 2], (name, corner)
        for thr in (-1, 128):
            got = R.find_page_quad(ph, thr, 0)
            assert got[:8].tolist() == q and got[11] == 1 and got[12:].tolist() == [0, 0, 0, 0], (name, thr, got)
            assert got[8] == (thr if thr >= 0 else got[8]) and 60 <= got[8] < 175
    ph, q = RC.photo("keystone")
    got = R.find_page_quad((255 - ph).astype(np.uint8), -1, 1)
    assert got[:8].tolist() == q and got[11] == 1


def test_quad_cases_known_answers():
    cases = {c["name"]: c for c in RC.quad_cases()}
    f = lambda n: R.find_page_quad(cases[n]["page"], cases[n]["threshold"], cases[n]["dark_paper"]).tolist()
    assert f("one_gray") == [0] * 8 + [-1, 0, 0, 0] + [0] * 4
    assert f("one_gray_fixed") == [0, 0, 64, 0, 64, 19, 0, 19, 128, 20 * 65, 1, 1, 0, 0, 0, 0]
    assert f("one_pixel") == [31, 7] * 4 + [128, 1, 1, 0] + [0] * 4
    assert f("one_row")[8:12] == [128, 57, 1, 0]
    assert f("rect_w64") == [4, 5, 60, 5, 60, 32, 4, 32, 40, 28 * 57, 1, 1, 0, 0, 0, 0]
    assert f("rect_dark_paper_w65") == [4, 5, 61, 5, 61, 32, 4, 32, 40, 28 * 58, 1, 1, 0, 0, 0, 0]
    assert f("larger_wins")[:8] == [50, 22, 124, 22, 124, 47, 50, 47] and f("larger_wins")[9:11] == [26 * 75, 2]
    assert f("larger_wins_first")[:8] == [4, 3, 79, 3, 79, 39, 4, 39]
    assert f("equal_smaller_label")[:8] == [70, 10, 99, 10, 99, 29, 70, 29] and f("equal_smaller_label")[9:11] == [600, 2]
    assert f("equal_same_row")[:8] == [5, 10, 34, 10, 34, 29, 5, 29]
    assert f("touching_diagonally")[9:11] == [15 * 35 + 25 * 80, 1]                     # 8-connected: one sheet
    assert f("all_borders_w63")[:8] == [0, 0, 62, 0, 62, 36, 0, 36]


def test_text_photo_keeps_its_lines():
    page, ph, q = RC.text_photo()
    got = R.find_page_quad(ph)
    assert got[:8].tolist() == q and got[11] == 1
    rect = R.rectify(ph, q)
    n_page, n_rect = S.segment_page(page)[1][1], S.segment_page(rect)[1][1]
    assert n_page == n_rect == 3
    words = S.segment_page(rect, **RC.TEXT_SEGMENT)[1]
    assert words[1] == S.segment_page(page, **RC.TEXT_SEGMENT)[1][1] == 3 and words[0] > 20
    n_photo = S.segment_page(ph)[1][1]
    print(f"[rectify] lines: page {n_page}, rectified {n_rect}, the photograph as it is {n_photo}")


def test_c_plan_matches_the_restatement_exactly():
    import aocr
    for q in _all_quads() + list(BAD_QUADS.values()) + [[0, 0, 16384, 0, 16384, 100, 0, 100]]:
        for Wo_in, Ho_in in ((0, 0), (37, 0), (0, 1), (1, 1), (640, 480)):
            qa, size, coef = (C.c_int32 * 8)(*q), (C.c_int32 * 2)(-5, -5), (C.c_double * 9)(*([-5.0] * 9))
            st = aocr.lib.aocr_rectify_plan(qa, Wo_in, Ho_in, size, coef)
            try:
                (Wo, Ho), c = R.rectify_plan(q, Wo_in, Ho_in)
            except ValueError:
                assert st != 0 and aocr.last_error(), q
                assert list(size) == [-5, -5] and list(coef) == [-5.0] * 9                    # an error leaves the outputs untouched
                continue
            assert st == 0, (q, aocr.last_error())
            assert list(size) == [Wo, Ho], q
            assert np.array(list(coef)).tobytes() == c.tobytes(), (q, list(coef), c.tolist())      # bit for bit, the sign of a zero included
            (s2, c2) = aocr.rectify_plan(q, Wo_in, Ho_in)
            assert s2 == (Wo, Ho) and c2.tobytes() == c.tobytes()
    assert aocr.lib.aocr_rectify_plan(None, 0, 0, size, coef) != 0
    with pytest.raises(ValueError, match="16385"):
        aocr.rectify_plan([0, 0, 16384, 0, 16384, 100, 0, 100])
    with pytest.raises(ValueError):
        aocr.rectify_plan(BAD_QUADS["bow_tie"])
    X, Y = aocr.warp_points(c, np.arange(5), np.arange(5))
    Xr, Yr, _ = R.warp_points(c, np.arange(5), np.arange(5))
    assert X.tobytes() == Xr.tobytes() and Y.tobytes() == Yr.tobytes()
