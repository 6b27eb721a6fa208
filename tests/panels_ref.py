"""Plain restatement of aocr_invert_panels (include/aocr.h) on top of components_ref: the candidates among the components in label order, the
row spans of every examined candidate, the two percent tests, and 255 - v inside the spans of the accepted ones.  Loops over candidates and
rows, Python integers.  Test infrastructure: it does not import the product."""
import numpy as np

import components_ref as CR

DEFAULTS = dict(threshold=-1, light_text=0, connectivity=8, min_w=64, min_h=24, fill_percent=60, min_inside_percent=2)
HULL_CAP = 2 ** 31 - 1


def spans_of(labels, comp):
    """[(y, lo, hi)] for every row of the component's box: the smallest column with the component's label, the largest plus one."""
    x0, y0, x1, y1, label, _ = (int(v) for v in comp)
    rows = []
    for y in range(y0, y1):
        xs = np.nonzero(labels[y, x0:x1] == label)[0]
        assert len(xs), "a connected component has a pixel in every row of its box"
        rows.append((y, x0 + int(xs[0]), x0 + int(xs[-1]) + 1))
    return rows


def is_panel(area, hull, fill_percent, min_inside_percent):
    return area * 100 >= fill_percent * hull and (hull - area) * 100 >= min_inside_percent * hull


def invert_panels(page, max_panels=256, **kw):
    """(out (H, W) uint8, panels (examined, 8) int32 rows x0 y0 x1 y1 label area hull accepted, counts (8) int32)."""
    p = dict(DEFAULTS)
    p.update(kw)
    assert p["connectivity"] in (4, 8) and p["min_w"] >= 1 and p["min_h"] >= 1 and 1 <= max_panels <= 1024
    assert 1 <= p["fill_percent"] <= 100 and 0 <= p["min_inside_percent"] <= 99 and p["fill_percent"] + p["min_inside_percent"] <= 100
    page = np.asarray(page)
    labels, comps, info = CR.label_components(page, p["threshold"], p["light_text"], p["connectivity"], max_components=page.size)
    cands = [c for c in comps if c[2] - c[0] >= p["min_w"] and c[3] - c[1] >= p["min_h"]]        # comps are in label order
    out = page.copy()
    rows, inverted, hull_sum = [], 0, 0
    for c in cands[:max_panels]:
        spans = spans_of(labels, c)
        area, hull = int(c[5]), sum(hi - lo for _, lo, hi in spans)
        ok = is_panel(area, hull, p["fill_percent"], p["min_inside_percent"])
        rows.append([int(v) for v in c[:5]] + [area, hull, int(ok)])
        if ok:
            inverted, hull_sum = inverted + 1, hull_sum + hull
            for y, lo, hi in spans:
                out[y, lo:hi] = 255 - page[y, lo:hi]                  # from the page, never from out: an overlap is inverted once
    counts = [int(info[2]), len(cands), len(rows), inverted, int(info[0]), int(info[1]), min(hull_sum, HULL_CAP), 0]
    return out, np.array(rows, np.int32).reshape(-1, 8), np.array(counts, np.int32)
