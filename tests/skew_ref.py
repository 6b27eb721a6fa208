"""Plain numpy restatement of aocr_estimate_skew and aocr_deskew_page (include/aocr.h): loops over candidates and strips, Python and int64
integers, `>>` an arithmetic shift.  Test infrastructure: it does not import the product."""
import numpy as np

from segment_ref import otsu

SLOPE_MAX = 16384


def ink_mask(page, threshold=-1, light_text=0):
    """(ink (H, W) bool, the threshold used): steps 1-2 of aocr_segment_page."""
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim == 2
    thr = threshold
    if thr < 0:
        thr = otsu(np.bincount(page.reshape(-1), minlength=256))
    if thr < 0:
        return np.zeros(page.shape, bool), thr
    return (page > thr) if light_text else (page <= thr), thr


def strip_counts(ink):
    """R (nb, H): ink pixels of row y inside the 32-column strip b."""
    H, W = ink.shape
    nb = (W + 31) // 32
    R = np.zeros((nb, H), np.int64)
    for b in range(nb):
        R[b] = ink[:, 32 * b:32 * b + 32].sum(axis=1)
    return R


def offsets(W, slope):
    nb = (W + 31) // 32
    cx = W >> 1
    return [((32 * b + 16 - cx) * slope + 32768) >> 16 for b in range(nb)]


def profile(R, H, W, slope):
    """P[r] for r in [-D, H + D), as an array of H + 2D entries."""
    off = offsets(W, slope)
    D = max(abs(o) for o in off)
    P = np.zeros(H + 2 * D, np.int64)
    for b, o in enumerate(off):
        # source row y = r + o  <=>  r = y - o, at index r + D
        P[D - o:D - o + H] += R[b]
    return P


def estimate_skew(page, threshold=-1, light_text=0, step_q16=64, n_steps=96):
    """(skew (4) int32: k, k * step_q16, threshold used, 0; scores (2K+1) uint64, k = -K first)."""
    assert 1 <= step_q16 <= 4096 and 0 <= n_steps <= 256 and n_steps * step_q16 <= SLOPE_MAX
    ink, thr = ink_mask(page, threshold, light_text)
    H, W = ink.shape
    R = strip_counts(ink)
    K = n_steps
    scores = []
    for k in range(-K, K + 1):
        P = profile(R, H, W, k * step_q16)
        assert int(P.sum()) == int(ink.sum())
        scores.append(sum(int(v) * int(v) for v in P))
    best_k, best = 0, scores[K]
    for a in range(1, K + 1):
        for k in (-a, a):
            if scores[k + K] > best:
                best_k, best = k, scores[k + K]
    return np.array([best_k, best_k * step_q16, thr, 0], np.int32), np.array(scores, np.uint64)


def deskew(page, slope_q16, fill=255):
    """out[y][x] = page[sy][sx] or fill: the shear of aocr_deskew_page."""
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim == 2
    H, W = page.shape
    s = min(max(int(slope_q16), -SLOPE_MAX), SLOPE_MAX)
    cx, cy = W >> 1, H >> 1
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    sy = y + (((x - cx) * s + 32768) >> 16)
    sx = x - (((y - cy) * s + 32768) >> 16)
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    out = np.full((H, W), fill, np.uint8)
    out[inside] = page[np.broadcast_to(sy, (H, W))[inside], np.broadcast_to(sx, (H, W))[inside]]
    return out


def source_corners(boxes, slope_q16, H, W):
    """(n, 4, 2): source-page (x, y) of the corner pixels (x0,y0) (x1-1,y0) (x1-1,y1-1) (x0,y1-1) of every box, by the two formulas."""
    s = min(max(int(slope_q16), -SLOPE_MAX), SLOPE_MAX)
    cx, cy = W >> 1, H >> 1
    out = []
    for bx in np.asarray(boxes).reshape(-1, np.asarray(boxes).shape[-1] if np.asarray(boxes).ndim > 1 else 4):
        x0, y0, x1, y1 = (int(v) for v in bx[:4])
        out.append([[x - (((y - cy) * s + 32768) >> 16), y + (((x - cx) * s + 32768) >> 16)]
                    for x, y in ((x0, y0), (x1 - 1, y0), (x1 - 1, y1 - 1), (x0, y1 - 1))])
    return np.array(out, np.int64).reshape(-1, 4, 2)
