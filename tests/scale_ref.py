"""Plain restatement of aocr_estimate_glyph_size and aocr_resize_page (include/aocr.h) in numpy int64.  The estimator goes on
components_ref.label_components (a flood fill); the resize is separable through prefix sums: with P the running sum of a row and
F(x*Wo + r) = Wo*P[x] + r*v[x] the sum of the row up to position x*Wo + r of the common axis, the horizontal sum for output pixel X is
F((X+1)*W) - F(X*W).  Test infrastructure: it does not import the product."""
import numpy as np

import components_ref as CR

GLYPH_DEFAULTS = dict(threshold=-1, light_text=0, connectivity=8, min_size=2, max_size=512, max_aspect=8)
SCALE_DEFAULTS = dict(target=16, tolerance=1.25, min_glyphs=8)


def glyph_sizes(page, **kw):
    """(the ascending list of a = min(w, h) over the qualifying components, info of label_components)."""
    p = dict(GLYPH_DEFAULTS)
    p.update(kw)
    assert 1 <= p["min_size"] <= p["max_size"] <= 1024 and p["max_aspect"] >= 1
    page = np.asarray(page)
    _, comps, info = CR.label_components(page, p["threshold"], p["light_text"], p["connectivity"], max_components=page.size)
    sizes = []
    for x0, y0, x1, y1, _, _ in comps.tolist():
        w, h = x1 - x0, y1 - y0
        a, b = min(w, h), max(w, h)
        if p["min_size"] <= a <= p["max_size"] and b <= p["max_aspect"] * a:
            sizes.append(a)
    return sorted(sizes), info


def estimate_glyph_size(page, **kw):
    """glyph (8) int32: q_2, q_1, q_3, n, components found, the threshold used, the total ink, 0."""
    sizes, info = glyph_sizes(page, **kw)
    n = len(sizes)
    q = [sizes[k * (n - 1) // 4] if n else 0 for k in (1, 2, 3)]
    return np.array([q[1], q[0], q[2], n, info[2], info[0], info[1], 0], np.int32)


def _axis_sums(v, Lo):
    """v (..., L) int64 -> (..., Lo): sum over x of w(x, X) * v[..., x], w as include/aocr.h defines it."""
    L = v.shape[-1]
    P = np.concatenate([np.zeros(v.shape[:-1] + (1,), np.int64), np.cumsum(v, axis=-1)], axis=-1)       # P[x] = v[0] + .. + v[x-1]
    vp = np.concatenate([v, np.zeros(v.shape[:-1] + (1,), np.int64)], axis=-1)                           # v[L] = 0: only met with r == 0
    pos = np.arange(Lo + 1, dtype=np.int64) * L                                                        # X*L on the axis of L*Lo units
    x, r = pos // Lo, pos % Lo
    F = Lo * P[..., x] + r * vp[..., x]
    return F[..., 1:] - F[..., :-1]


def resize_page(page, Ho, Wo):
    """(Ho, Wo) uint8: floor((S + floor(H*W / 2)) / (H*W)), S the area-weighted sum."""
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim == 2
    H, W = page.shape
    assert W <= 8 * Wo and Wo <= 8 * W and H <= 8 * Ho and Ho <= 8 * H
    h = _axis_sums(page.astype(np.int64), Wo)                                  # (H, Wo)
    S = _axis_sums(np.ascontiguousarray(h.T), Ho).T                            # (Ho, Wo)
    return ((S + (H * W) // 2) // (H * W)).astype(np.uint8)


def resize_direct(page, Ho, Wo):
    """the definition itself, weight by weight: for small pages, to check the prefix-sum form."""
    page = np.asarray(page).astype(np.int64)
    H, W = page.shape

    def weights(L, Lo):
        x, X = np.arange(L, dtype=np.int64)[:, None], np.arange(Lo, dtype=np.int64)[None, :]
        return np.maximum(0, np.minimum((x + 1) * Lo, (X + 1) * L) - np.maximum(x * Lo, X * L))        # (L, Lo)

    S = weights(H, Ho).T @ page @ weights(W, Wo)
    return ((S + (H * W) // 2) // (H * W)).astype(np.uint8)


def scale_plan(size, n, H, W, **kw):
    """(Wo, Ho) or None, as aocr.scale_plan; the product clamp (Ho*Wo <= 2^26) is not restated: the tests that meet it check the limits."""
    p = dict(SCALE_DEFAULTS)
    p.update(kw)
    if n < p["min_glyphs"] or size <= 0:
        return None
    t = p["target"]
    if t <= p["tolerance"] * size and size <= p["tolerance"] * t:
        return None
    side = lambda L: min(max(min(max((2 * L * t + size) // (2 * size), -(-L // 8)), 8 * L), 1), 16384)
    return side(W), side(H)


def unscale(x, y, H, W, Ho, Wo):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return (x + 0.5) * W / Wo - 0.5, (y + 0.5) * H / Ho - 0.5
