"""Plain numpy restatement of aocr_remove_rules (include/aocr.h), written from its definitions, twice.  remove_rules measures the run of every
pixel -- the columns [c, d) of its row run and the rows [a, b) of its column run as four arrays -- and applies the three erasure classes
to them as the header states them.  remove_rules_by_runs is independent of it: it lists the runs of every row and column (segment_ref.runs),
takes the two openings from the lists and walks every thin run pixel by pixel.  Integers only.  Test infrastructure: it does not import the
product."""
import numpy as np

from components_ref import ink_mask
from segment_ref import runs

DEFAULTS = dict(threshold=-1, light_text=0, axes=3, min_len=100, max_thick=6, edge=1)


def check_params(p):
    assert -1 <= p["threshold"] <= 254 and p["axes"] in (1, 2, 3)
    assert 1 <= p["max_thick"] <= 16 and p["max_thick"] < p["min_len"] <= 16384 and 0 <= p["edge"] <= 4


def run_extents(ink):
    """(c, d): per pixel the half-open columns of the maximal ink run of its row through it (meaningless on paper)."""
    H, W = ink.shape
    x = np.broadcast_to(np.arange(W), (H, W))
    c = np.maximum.accumulate(np.where(ink, 0, x + 1), axis=1)                   # behind the last paper pixel at or left of x
    d = np.minimum.accumulate(np.where(ink, W, x)[:, ::-1], axis=1)[:, ::-1]     # the first paper pixel at or right of x
    return c, d


def _result(page, ink, thr, hc, vc, cross, by_h, by_v, light_text):
    erased = cross | by_h | by_v
    out = page.copy()
    out[erased] = 0 if light_text else 255
    n_h = by_h & ~cross
    counts = [thr, ink.sum(), erased.sum(), cross.sum(), n_h.sum(), (by_v & ~cross & ~n_h).sum(), ((hc | vc) & ~erased).sum(), 0]
    return out, np.array([int(v) for v in counts], np.int32)


def remove_rules(page, **kw):
    """(out (H, W) uint8, counts (8) int32)."""
    p = dict(DEFAULTS)
    p.update(kw)
    check_params(p)
    page = np.asarray(page)
    ink, thr = ink_mask(page, p["threshold"], p["light_text"])
    H, W = ink.shape
    L, T, e = p["min_len"], p["max_thick"], p["edge"]
    c, d = run_extents(ink)
    a, b = (v.T for v in run_extents(ink.T))
    hc = ink & (d - c >= L) if p["axes"] & 1 else np.zeros((H, W), bool)
    vc = ink & (b - a >= L) if p["axes"] & 2 else np.zeros((H, W), bool)
    ys, xs = np.mgrid[0:H, 0:W]
    by_h, by_v = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for k in range(-e, e + 1):
        y2 = ys + k                                                               # y' in [max(a, y - e), min(b - 1, y + e)]
        ok = ink & (b - a <= T) & (y2 >= a) & (y2 < b)
        by_h |= ok & hc[np.clip(y2, 0, H - 1), xs]
        x2 = xs + k
        ok = ink & (d - c <= T) & (x2 >= c) & (x2 < d)
        by_v |= ok & vc[ys, np.clip(x2, 0, W - 1)]
    return _result(page, ink, thr, hc, vc, hc & vc, by_h, by_v, p["light_text"])


def _opening(ink, L):
    """per row: the pixels of the runs of at least L."""
    out = np.zeros(ink.shape, bool)
    for y in range(ink.shape[0]):
        for s, t in runs(ink[y]):
            if t - s >= L:
                out[y, s:t] = True
    return out


def _thin_hits(ink, cand, T, e):
    """per column: the pixels of runs of at most T rows that have a candidate within e rows inside the run."""
    out = np.zeros(ink.shape, bool)
    for x in range(ink.shape[1]):
        for a, b in runs(ink[:, x]):
            if b - a > T:
                continue
            for y in range(a, b):
                out[y, x] = cand[max(a, y - e):min(b - 1, y + e) + 1, x].any()
    return out


def remove_rules_by_runs(page, **kw):
    """the same result from run lists: the second formulation."""
    p = dict(DEFAULTS)
    p.update(kw)
    check_params(p)
    page = np.asarray(page)
    ink, thr = ink_mask(page, p["threshold"], p["light_text"])
    L, T, e = p["min_len"], p["max_thick"], p["edge"]
    hc = _opening(ink, L) if p["axes"] & 1 else np.zeros(ink.shape, bool)
    vc = _opening(ink.T, L).T if p["axes"] & 2 else np.zeros(ink.shape, bool)
    by_h = _thin_hits(ink, hc, T, e)
    by_v = _thin_hits(ink.T, vc.T, T, e).T
    return _result(page, ink, thr, hc, vc, hc & vc, by_h, by_v, p["light_text"])
