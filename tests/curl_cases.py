"""Pages for the dewarp tests, shared by test_curl_cpu.py (the restatement alone) and test_curl_gpu.py (the kernels against it)."""
import numpy as np

from skew_cases import PLANTED_SHAPE, SEGMENT, noise_page, planted_page, text_page  # noqa: F401  (re-exported for the two test files)

PLANTED_AMPS = (0, 6, 12, -12, 20)              # rows of sag at the page's left and right edge
PLANTED = dict(threshold=128, light_text=0, group=4, max_shift=8, min_ink=64)


def sag(x, amp, W):
    """rows by which column x of a curled page lies below the page's middle column: round(amp * ((x - W/2) / (W/2))^2), halves rounded up
    (floor(v + 0.5))."""
    u = (np.asarray(x, np.float64) - W / 2) / (W / 2)
    return np.floor(amp * u * u + 0.5).astype(np.int64)


_curled = {}


def curled_page(amp):
    """the straight planted 600 x 800 page of skew_cases with column x moved down by sag(x) rows (paper moves in): computed once per amp."""
    if amp not in _curled:
        straight, _ = planted_page(0)
        H, W = straight.shape
        out = np.full((H, W), 255, np.uint8)
        for x, d in enumerate(sag(np.arange(W), amp, W).tolist()):
            if d >= 0:
                out[d:, x] = straight[:H - d, x]
            else:
                out[:H + d, x] = straight[-d:, x]
        _curled[amp] = out
    return _curled[amp]


def planted_truth(amp, group):
    """s[j] as planted: the sag at the centre column of group j (the page's last column for a centre beyond it) minus that of group ng >> 1."""
    H, W = PLANTED_SHAPE
    w, h = 32 * group, 16 * group
    ng = -(-((W + 31) // 32) // group)
    c = np.minimum(np.arange(ng) * w + h, W - 1)
    s = sag(c, amp, W)
    return s - s[ng >> 1]


def tie_page():
    """Two 32-column groups (group = 1), symmetric under the sign of d: group 0 inked on row 12, group 1 on rows 11 and 13.  C(-1) = C(+1) =
    32 * 32, every other score is 0: the order 0, -1, +1, ... makes -1 the winner, s = [+1, 0]."""
    page = np.full((24, 64), 255, np.uint8)
    page[12, 0:32] = 0
    page[11, 32:64] = 0
    page[13, 32:64] = 0
    return page


TIE = dict(threshold=128, light_text=0, group=1, max_shift=4, min_ink=1)


def gated_page():
    """Three 32-column groups (group = 1): group 0 inked on row 10, group 1 on row 12 (delta_0 = +2), group 2 holds 3 ink pixels on row 15:
    with min_ink = 8 the pair (1, 2) is gated to 0 although its scores peak at +3; s = [-2, 0, 0]."""
    page = np.full((24, 96), 255, np.uint8)
    page[10, 0:32] = 0
    page[12, 32:64] = 0
    page[15, 70:73] = 0
    return page


GATED = dict(threshold=128, light_text=0, group=1, max_shift=4, min_ink=8)
