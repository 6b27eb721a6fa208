"""Plain numpy restatement of aocr_binarize_page (include/aocr.h), written from the header's text: the clipped window sums of v and v*v
(differences of cumulative sums, one axis after the other: the same number as the header's double loop), D = n*S2 - S1*S1, its exact integer
square root, the Sauvola threshold T and the two output forms, all in int64 with floor division.  Test infrastructure: it does not import
the product."""
import math

import numpy as np

from flatten_ref import window_sum

DEFAULTS = dict(radius=20, k_q8=51, range=128, light_text=0, hard=0)


def isqrt(D):
    """floor(sqrt(D)) of a non-negative int64 array, exactly: the float estimate stepped until q*q <= D < (q+1)*(q+1) everywhere."""
    D = np.asarray(D, np.int64)
    assert int(D.min()) >= 0
    q = np.floor(np.sqrt(D.astype(np.float64))).astype(np.int64)
    while True:
        high, low = q * q > D, (q + 1) * (q + 1) <= D
        if not (high.any() or low.any()):
            return q
        q = q - high + low


def thresholds(v, radius, k_q8, range):
    """T of the header for an int64 page v (the bright side is paper)."""
    s1, nx = window_sum(v, radius, 1)
    s1, ny = window_sum(s1, radius, 0)
    s2, _ = window_sum(v * v, radius, 1)
    s2, _ = window_sum(s2, radius, 0)
    n = (ny[:, None] * nx[None, :]).astype(np.int64)
    D = n * s2 - s1 * s1
    assert int(D.max()) < 1 << 43
    q = isqrt(D)
    num = s1 * ((256 - k_q8) * range * n + k_q8 * q)
    assert int(num.max()) < 1 << 53
    return num // (256 * range * n * n)


def binarize(page, radius=20, k_q8=51, range=128, light_text=0, hard=0):
    """(out uint8 page, counts [ink pixels, min T, max T, 0] int32)."""
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim == 2 and 1 <= radius <= 63 and 0 <= k_q8 <= 255 and 1 <= range <= 255
    v = page.astype(np.int64)
    if light_text:
        v = 255 - v
    T = thresholds(v, radius, k_q8, range)
    ink = v <= T
    if hard:
        out = np.where(ink, 0, 255)
    else:
        out = np.where(ink, (v * 127) // np.maximum(T, 1), np.minimum(255, 128 + ((v - T - 1) * 127) // np.maximum(254 - T, 1)))
    if light_text:
        out = 255 - out
    return out.astype(np.uint8), np.array([int(ink.sum()), int(T.min()), int(T.max()), 0], np.int32)


def threshold_at(page, x, y, radius, k_q8=51, range=128):
    """T of one pixel by the header's double loop and math.isqrt: what `thresholds` must equal."""
    H, W = page.shape
    win = page[max(y - radius, 0):min(y + radius, H - 1) + 1, max(x - radius, 0):min(x + radius, W - 1) + 1].astype(np.int64)
    n, S1, S2 = int(win.size), int(win.sum()), int((win * win).sum())
    q = math.isqrt(n * S2 - S1 * S1)
    return (S1 * ((256 - k_q8) * range * n + k_q8 * q)) // (256 * range * n * n)
