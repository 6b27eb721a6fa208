"""Plain numpy restatement of aocr_estimate_curl, aocr_dewarp_page (include/aocr.h) and of aocr.page.curl_shift_q8 / uncurl_points: loops over
pairs, shifts and columns, Python integers (`//` floors, `>>` is an arithmetic shift).  Test infrastructure: it does not import the product."""
import numpy as np

from skew_ref import ink_mask, strip_counts

SHIFT_MAX = 16384


def n_groups(W, group):
    nb = (W + 31) // 32
    return (nb + group - 1) // group


def group_profiles(ink, group):
    """G (ng, H) int64: ink pixels of row y inside the columns [j * 32 * group, (j + 1) * 32 * group)."""
    R = strip_counts(ink)
    nb = R.shape[0]
    ng = (nb + group - 1) // group
    G = np.zeros((ng, ink.shape[0]), np.int64)
    for j in range(ng):
        for b in range(j * group, min((j + 1) * group, nb)):
            G[j] += R[b]
    return G


def pair_score(Ga, Gb, d):
    """sum over y of Ga[y] * Gb[y + d], rows outside [0, H) contributing nothing; a Python int."""
    H = len(Ga)
    lo, hi = max(0, -d), min(H, H - d)                  # the rows y with 0 <= y + d < H
    if hi <= lo:
        return 0
    return int(np.dot(Ga[lo:hi], Gb[lo + d:hi + d]))    # int64: at most 16384 * 512^2 = 2^32


def estimate_curl(page, threshold=-1, light_text=0, group=4, max_shift=8, min_ink=64):
    """(curl (4) int32: ng, max |s|, threshold used, pairs with a non-zero shift; shifts (ng) int32; scores (ng - 1, 2D + 1) uint64)."""
    assert 1 <= group <= 16 and 0 <= max_shift <= 64 and 0 <= min_ink <= 1 << 20
    ink, thr = ink_mask(page, threshold, light_text)
    G = group_profiles(ink, group)
    ng, D = G.shape[0], max_shift
    I = [int(G[j].sum()) for j in range(ng)]
    scores = np.zeros((ng - 1, 2 * D + 1), np.uint64)
    delta = []
    for j in range(ng - 1):
        for d in range(-D, D + 1):
            scores[j, d + D] = pair_score(G[j], G[j + 1], d)
        best_d, best = 0, int(scores[j, D])
        for a in range(1, D + 1):
            for d in (-a, a):
                if int(scores[j, d + D]) > best:
                    best_d, best = d, int(scores[j, d + D])
        delta.append(0 if I[j] < min_ink or I[j + 1] < min_ink else best_d)
    jc = ng >> 1
    s = [0] * ng
    for j in range(jc, ng - 1):
        s[j + 1] = s[j] + delta[j]
    for j in range(jc - 1, -1, -1):
        s[j] = s[j + 1] - delta[j]
    curl = [ng, max(abs(v) for v in s), thr, sum(1 for v in delta if v != 0)]
    return np.array(curl, np.int32), np.array(s, np.int32), scores


def group_ink(page, threshold=-1, light_text=0, group=4):
    """I_j per group, for the tests that look at the gate."""
    ink, _ = ink_mask(page, threshold, light_text)
    return group_profiles(ink, group).sum(axis=1)


def shift_q8(x, shifts, group):
    """q(x) of aocr_dewarp_page for one column, a Python int."""
    s = [min(max(int(v), -SHIFT_MAX), SHIFT_MAX) for v in shifts]
    ng, w, h = len(s), 32 * group, 16 * group
    if x <= h:
        return 256 * s[0]
    if x >= (ng - 1) * w + h:
        return 256 * s[ng - 1]
    j = (x - h) // w
    t = x - (j * w + h)
    return 256 * s[j] + ((s[j + 1] - s[j]) * t * 256 + h) // w


def curl_shift_q8(x, shifts, group):
    x = np.asarray(x)
    return np.array([shift_q8(int(v), shifts, group) for v in x.reshape(-1)], np.int64).reshape(x.shape)


def uncurl_points(x, y, shifts, group):
    x = np.asarray(x)
    return x.astype(np.float64), np.asarray(y, np.float64) + curl_shift_q8(x, shifts, group) / 256.0


def dewarp(page, shifts, group, fill=255):
    """out[y][x] = the two rows p >> 8 and (p >> 8) + 1 of column x blended by p & 255, p = 256 * y + q(x); `fill` outside the page."""
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim == 2
    H, W = page.shape
    assert len(shifts) == n_groups(W, group)
    out = np.empty((H, W), np.uint8)
    y = np.arange(H, dtype=np.int64)
    for x in range(W):
        p = 256 * y + shift_q8(x, shifts, group)
        sy, f = p >> 8, p & 255
        col = page[:, x].astype(np.int64)
        a = np.where((sy >= 0) & (sy < H), col[np.clip(sy, 0, H - 1)], fill)
        b = np.where((sy + 1 >= 0) & (sy + 1 < H), col[np.clip(sy + 1, 0, H - 1)], fill)
        out[:, x] = (a * (256 - f) + b * f + 128) >> 8
    return out
