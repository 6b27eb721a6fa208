"""CPU: the numpy restatement of aocr_estimate_curl / aocr_dewarp_page (tests/curl_ref.py) on planted pages -- it finds the curl, and taking
it out gives the row profiles their lines back -- its edge cases, and the host helpers of aocr.page against it.  test_curl_gpu.py holds the
kernels to the same restatement, byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import curl_ref as K
import segment_ref as R
from curl_cases import GATED, PLANTED, PLANTED_AMPS, SEGMENT, TIE, curled_page, gated_page, planted_page, planted_truth, tie_page

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("amp", PLANTED_AMPS)
def test_planted_curl_is_found_and_removed(amp):
    straight, _ = planted_page(0)
    page = curled_page(amp)
    _, c0 = R.segment_page(straight, **SEGMENT)
    assert c0[1] == 15
    if amp == 20:
        _, cc = R.segment_page(page, **SEGMENT)
        assert cc[1] == 1, "the curled page's row profile still shows its lines"
    for group in (2, 3, 4):
        params = dict(PLANTED, group=group)
        curl, s, scores = K.estimate_curl(page, **params)
        ng, jc = len(s), len(s) >> 1
        assert curl[0] == ng == K.n_groups(800, group) and curl[1] == np.abs(s).max() and curl[2] == 128
        out = K.dewarp(page, s, group)
        if amp == 0:
            assert not s.any() and curl[3] == 0 and np.array_equal(out, page)
        else:
            sign = 1 if amp > 0 else -1
            assert (sign * s[:jc] >= 0).all() and (sign * s[jc:] >= 0).all() and sign * s[0] > 0 and sign * s[-1] > 0
        _, cd = R.segment_page(out, **SEGMENT)
        assert cd[1] == 15, (amp, group, cd)
        inked = K.group_ink(page, 128, 0, group) >= params["min_ink"]
        err = int(np.abs(s - planted_truth(amp, group))[inked].max())
        print(f"[curl] amp {amp} group {group}: shifts {s.tolist()}, max |s - truth| over inked groups {err}, pairs moved {curl[3]}")


def test_tie_goes_to_the_negative_shift():
    curl, s, scores = K.estimate_curl(tie_page(), **TIE)
    D = TIE["max_shift"]
    assert scores.shape == (1, 2 * D + 1) and scores[0, D - 1] == scores[0, D + 1] == 32 * 32 and np.delete(scores[0], [D - 1, D + 1]).max() == 0
    assert s.tolist() == [1, 0] and curl.tolist() == [2, 1, 128, 1]              # delta_0 = -1; jc = 1: s[0] = s[1] - delta_0
    assert np.array_equal(K.estimate_curl(tie_page()[:, ::-1], **TIE)[1], [1, 0])    # mirrored: rows 11 and 13 against row 12, still -1


def test_gated_pair_gets_shift_zero_and_keeps_its_scores():
    curl, s, scores = K.estimate_curl(gated_page(), **GATED)
    D = GATED["max_shift"]
    assert K.group_ink(gated_page(), 128, 0, 1).tolist() == [32, 32, 3]
    assert scores[0, D + 2] == 32 * 32 and scores[1, D + 3] == 32 * 3 and scores[1].argmax() == D + 3
    assert s.tolist() == [-2, 0, 0] and curl.tolist() == [3, 2, 128, 1]
    open_gate = dict(GATED, min_ink=3)
    assert K.estimate_curl(gated_page(), **open_gate)[1].tolist() == [-2, 0, 3]


def test_degenerate_pages():
    one = K.estimate_curl(np.zeros((40, 32), np.uint8), threshold=128, group=1, max_shift=8, min_ink=0)       # ng == 1
    assert one[0].tolist() == [1, 0, 128, 0] and one[1].tolist() == [0] and one[2].shape == (0, 17)
    assert K.estimate_curl(np.zeros((40, 500), np.uint8), threshold=128, group=16, max_shift=8, min_ink=0)[1].tolist() == [0]
    assert np.array_equal(K.dewarp(tie_page()[:, :32], [5], 1, 0)[:-5], tie_page()[5:, :32])                # one group: a rigid move
    # D >= H: the shifts that leave the page score 0
    page = gated_page()[8:14]                                                      # H = 6: rows 2 and 4 inked
    curl, s, scores = K.estimate_curl(page, threshold=128, group=1, max_shift=8, min_ink=1)
    assert scores.shape == (2, 17) and not scores[:, :8 - 5].any() and not scores[:, 8 + 6:].any() and s.tolist() == [-2, 0, 0]
    # no ink, and one gray value under Otsu
    for pg, thr, want in ((np.full((30, 100), 255, np.uint8), 128, 128), (np.full((30, 100), 77, np.uint8), -1, -1)):
        curl, s, scores = K.estimate_curl(pg, threshold=thr, group=1, max_shift=3, min_ink=0)
        assert curl.tolist() == [4, 0, want, 0] and not s.any() and not scores.any()


def test_shift_formula_edges():
    g = 2                                                                          # w = 64, h = 32: centres 32, 96, 160
    s = [4, -3, 10]
    assert K.shift_q8(0, s, g) == K.shift_q8(32, s, g) == 1024                     # flat up to and at c_0
    assert K.shift_q8(160, s, g) == K.shift_q8(191, s, g) == 2560                  # flat from c_{ng-1} on
    assert K.shift_q8(96, s, g) == -768                                            # a centre carries its own shift: t = 0, floor(h / w) = 0
    # ds = -7, t = 1: (-7*256 + 32) / 64 = -27.5 -> floor -28 (truncation would give -27)
    assert K.shift_q8(33, s, g) == 1024 - 28
    # ds = +13, t = 63: (13*63*256 + 32) // 64 = 3276
    assert K.shift_q8(159, s, g) == -768 + 3276
    # a narrow last group: W = 130 with group 2 has ng = 3 and its last centre, 160, beyond the page: the last columns still interpolate
    assert K.n_groups(130, g) == 3 and K.shift_q8(129, s, g) == -768 + (13 * 33 * 256 + 32) // 64
    # clamped like the device clamps them
    assert K.shift_q8(0, [70000, 0], 1) == 256 * 16384 and K.shift_q8(99, [0, -70000], 1) == -256 * 16384
    assert K.shift_q8(17, [16384, -16384], 1) == 256 * 16384 + (-32768 * 256 + 16) // 32
    q = K.curl_shift_q8(np.arange(200), s, g)
    assert q.dtype == np.int64 and (np.diff(q[32:97]) <= 0).all() and (np.diff(q[96:161]) >= 0).all()


def test_dewarp_blends_two_rows_and_fills():
    page = np.arange(8 * 64, dtype=np.int64).reshape(8, 64).astype(np.uint8)
    assert np.array_equal(K.dewarp(page, [0, 0], 1), page)
    out = K.dewarp(page, [1, 2], 1, fill=7)
    assert np.array_equal(out[:-1, :17], page[1:, :17]) and (out[-1, :17] == 7).all()       # x <= c_0: one whole row up
    assert np.array_equal(out[:-2, 48:], page[2:, 48:]) and (out[-2:, 48:] == 7).all()
    x, y = 32, 3                                                                   # t = 16: q = 256 + (16*256 + 16) // 32 = 384: rows 4 and 5, half each
    assert K.shift_q8(x, [1, 2], 1) == 384
    assert out[y, x] == (int(page[4, x]) * 128 + int(page[5, x]) * 128 + 128) >> 8
    up = K.dewarp(page, [-3, -3], 1, fill=200)
    assert (up[:3] == 200).all() and np.array_equal(up[3:], page[:-3])


def test_curl_params_layout_matches_the_header():
    import aocr
    hdr = open(os.path.join(ROOT, "include", "aocr.h")).read()
    body = re.search(r"typedef struct aocr_curl_params \{(.*?)\} aocr_curl_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(1), int(m.group(2) or 1)) for m in re.finditer(r"int32_t\s+(\w+)(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("threshold", 1), ("light_text", 1), ("group", 1), ("max_shift", 1), ("min_ink", 1), ("reserved", 3)]
    got = [(n, C.sizeof(t) // 4) for n, t in aocr.CurlParams._fields_]
    assert got == fields and C.sizeof(aocr.CurlParams) == 32
    off = 0
    for n, words in fields:
        assert getattr(aocr.CurlParams, n).offset == off
        off += 4 * words
    p = aocr.CurlParams()
    assert (p.threshold, p.light_text, p.group, p.max_shift, p.min_ink, list(p.reserved)) == (-1, 0, 4, 8, 64, [0, 0, 0])
    p = aocr.CurlParams(threshold=100, light_text=1, group=2, max_shift=12, min_ink=5)
    assert (p.threshold, p.light_text, p.group, p.max_shift, p.min_ink) == (100, 1, 2, 12, 5)


def test_host_helpers_equal_the_restatement():
    import aocr
    rng = np.random.default_rng(7)
    for W, group in ((800, 4), (130, 2), (31, 1), (333, 3), (16384, 16), (64, 16)):
        ng = K.n_groups(W, group)
        for s in (rng.integers(-40, 41, ng), rng.integers(-70000, 70001, ng), np.zeros(ng, np.int64)):
            x = np.arange(W)
            want = K.curl_shift_q8(x, s, group)
            got = aocr.page.curl_shift_q8(x, s, group)
            assert got.dtype == np.int64 and np.array_equal(got, want), (W, group)
            xs = rng.integers(0, W, (5, 4))
            ys = rng.integers(0, 600, (5, 4))
            ux, uy = aocr.uncurl_points(xs, ys, s, group)
            wx, wy = K.uncurl_points(xs, ys, s, group)
            assert ux.dtype == uy.dtype == np.float64 and np.array_equal(ux, wx) and np.array_equal(uy, wy)
    assert aocr.curl_shift_q8 is aocr.page.curl_shift_q8 and int(aocr.curl_shift_q8(5, [3], 1)) == 768


def test_source_points_is_source_corners_point_by_point():
    import aocr
    import skew_ref as S
    boxes = np.array([[10, 20, 110, 45, 0, 9], [300, 400, 420, 431, 7, 3], [0, 0, 1, 1, 0, 0]], np.int32)
    for slope in (0, 2560, -4096, 70000):
        want = S.source_corners(boxes, slope, 600, 800)
        assert np.array_equal(aocr.page.source_corners(boxes, slope, 600, 800), want)
        x, y = aocr.page.box_corners(boxes)
        sx, sy = aocr.source_points(x, y, slope, 600, 800)
        assert np.array_equal(np.stack([sx, sy], axis=2), want)
