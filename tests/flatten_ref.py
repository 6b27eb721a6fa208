"""Plain numpy restatement of aocr_flatten_page (include/aocr.h): the windowed max, the rounded windowed mean and the division, in int64
integers with floor division.  A max and a sum over a rectangle are taken one axis after the other (shifted slices for the max, differences of
cumulative sums for the sum), which is the same number as the header's double loop.  Test infrastructure: it does not import the product."""
import numpy as np


def window_max(v, r, axis):
    """out[i] = max of v[max(i-r,0) .. min(i+r,n-1)] along `axis`."""
    v = np.moveaxis(v, axis, 0)
    n = v.shape[0]
    out = v.copy()
    for d in range(1, min(r, n - 1) + 1):
        out[:n - d] = np.maximum(out[:n - d], v[d:])       # the element d further on
        out[d:] = np.maximum(out[d:], v[:n - d])           # the element d before
    return np.moveaxis(out, 0, axis)


def window_sum(v, r, axis):
    """(sums, counts): the sum of v[max(i-r,0) .. min(i+r,n-1)] along `axis`, and how many elements that is, per i."""
    v = np.moveaxis(v, axis, 0)
    n = v.shape[0]
    c = np.concatenate([np.zeros((1,) + v.shape[1:], np.int64), np.cumsum(v, axis=0, dtype=np.int64)])
    i = np.arange(n)
    lo, hi = np.maximum(i - r, 0), np.minimum(i + r, n - 1)
    return np.moveaxis(c[hi + 1] - c[lo], 0, axis), hi - lo + 1


def background(v, r):
    """(M, B) of the header for an int64 page v."""
    M = window_max(window_max(v, r, 1), r, 0)
    s, nx = window_sum(M, r, 1)
    s, ny = window_sum(s, r, 0)
    n = ny[:, None] * nx[None, :]
    assert int(s.max()) < 1 << 24
    return M, (s + (n >> 1)) // n


def flatten(page, radius=16, light_text=0):
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim == 2 and 1 <= radius <= 127
    v = page.astype(np.int64)
    if light_text:
        v = 255 - v
    _, B = background(v, radius)
    Bc = np.maximum(B, 1)
    out = np.minimum(255, (v * 255 + (Bc >> 1)) // Bc)
    if light_text:
        out = 255 - out
    return out.astype(np.uint8)
