"""Plain integer restatement of aocr_estimate_slant and of the virtual rectangle of aocr_crop_lines_slanted (include/aocr.h).  Python ints
and int64 throughout; Python's >> floors like the header's arithmetic shift.  `estimate_slant(..., plain=True)` is the specification
written out pixel by pixel; the default gathers the ink pixels of a box once and counts their profile columns with np.bincount, which
tests/test_slant_cpu.py holds against the plain loops.  Nothing here imports the library."""
import numpy as np

MAX_H = 256                                    # AOCR_SLANT_MAX_H
S_MAX = 65536                                  # what aocr_crop_lines_slanted clamps a slant to


def clamp_box(box, H, W):
    x0, y0, x1, y1 = (int(v) for v in box[:4])
    return min(max(x0, 0), W), min(max(y0, 0), H), min(max(x1, 0), W), min(max(y1, 0), H)


def off(cy, y, s):
    """off(y) of the header; y an int or an int64 array"""
    return ((cy - y) * s + 32768) >> 16


def extent(y0, y1, s):
    """max over y in [y0, y1) of |off(y)|, by looking at every row"""
    cy = (y0 + y1) >> 1
    return max(abs(off(cy, y, s)) for y in range(y0, y1))


def ink_mask(page, threshold, light_text):
    if threshold < 0:
        return np.zeros(page.shape, bool)
    return page > threshold if light_text else page <= threshold


def _scores_plain(I, x0, y0, x1, y1, step, K):
    cy = (y0 + y1) >> 1
    out = []
    for k in range(-K, K + 1):
        s = k * step
        D = extent(y0, y1, s)
        total = 0
        for c in range(x0 - D, x1 + D):
            P = 0
            for y in range(y0, y1):
                x = c + off(cy, y, s)
                if x0 <= x < x1 and I[y, x]:
                    P += 1
            total += P * P
        out.append(total)
    return out


def _scores_fast(I, x0, y0, x1, y1, step, K):
    cy = (y0 + y1) >> 1
    ys, xs = np.nonzero(I[y0:y1, x0:x1])
    ys, xs = ys.astype(np.int64) + y0, xs.astype(np.int64) + x0
    out = []
    for k in range(-K, K + 1):
        c = xs - off(cy, ys, k * step)         # the one profile column an ink pixel lands in: c + off(y) = x
        P = np.bincount(c - (x0 - MAX_H), minlength=1).astype(np.int64) if len(c) else np.zeros(1, np.int64)
        out.append(int((P * P).sum()))
    return out


def pick(scores, K):
    """0, -1, +1, -2, +2, ...: the first with the strictly largest score"""
    best, bk = scores[K], 0
    for a in range(1, K + 1):
        for k in (-a, a):
            if scores[K + k] > best:
                best, bk = scores[K + k], k
    return bk


def estimate_slant(page, boxes, n, threshold=128, light_text=0, step_q16=4096, n_steps=12, plain=False):
    """(slant (n, 4) int32: k, k * step_q16, flag, ink; scores (n, 2 * n_steps + 1) uint64) for the first n boxes.  threshold: the value
    in use (a device word's value where the call reads one; -1: nothing is ink)."""
    H, W = page.shape
    K = int(n_steps)
    I = ink_mask(page, int(threshold), int(light_text))
    slant = np.zeros((n, 4), np.int32)
    scores = np.zeros((n, 2 * K + 1), np.uint64)
    for i in range(n):
        x0, y0, x1, y1 = clamp_box(boxes[i], H, W)
        if x1 <= x0 or y1 <= y0:
            slant[i] = (0, 0, 2, 0)
            continue
        ink = int(I[y0:y1, x0:x1].sum())
        if y1 - y0 > MAX_H:
            slant[i] = (0, 0, 1, ink)
            continue
        sc = (_scores_plain if plain else _scores_fast)(I, x0, y0, x1, y1, int(step_q16), K)
        k = pick(sc, K)
        slant[i] = (k, k * int(step_q16), 0, ink)
        scores[i] = np.array(sc, np.uint64)
    return slant, scores


def slant_view(page, box, s, fill):
    """V of aocr_crop_lines_slanted: (h, w + 2D) uint8, None for a box that is empty after clamping"""
    H, W = page.shape
    x0, y0, x1, y1 = clamp_box(box, H, W)
    if x1 <= x0 or y1 <= y0:
        return None
    s = min(max(int(s), -S_MAX), S_MAX)
    cy = (y0 + y1) >> 1
    D = max(abs(off(cy, y0, s)), abs(off(cy, y1 - 1, s)))
    V = np.full((y1 - y0, x1 - x0 + 2 * D), fill, np.uint8)
    for r in range(y1 - y0):
        for c in range(V.shape[1]):
            sx = x0 - D + c + off(cy, y0 + r, s)
            if x0 <= sx < x1:
                V[r, c] = page[y0 + r, sx]
    return V


def slant_extent(boxes, slant_q16):
    """aocr.page.slant_extent as a loop"""
    out = []
    for b, s in zip(boxes, slant_q16):
        x0, y0, x1, y1 = (int(v) for v in b[:4])
        s = min(max(int(s), -S_MAX), S_MAX)
        out.append(extent(y0, y1, s) if x1 > x0 and y1 > y0 else 0)
    return np.array(out, np.int32)
