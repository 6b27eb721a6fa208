"""Plain restatement of aocr_label_components and aocr_clean_page (include/aocr.h): a flood fill over the ink mask in raster order, so the
first pixel met of every component is its smallest y*W + x.  Loops and integers.  Test infrastructure: it does not import the product."""
import numpy as np

from segment_ref import otsu

DEFAULTS = dict(threshold=-1, light_text=0, connectivity=8, min_area=6, max_w=0, max_h=200)
N4 = ((0, -1), (-1, 0), (1, 0), (0, 1))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def ink_mask(page, threshold=-1, light_text=0):
    """(mask, the threshold used)."""
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim == 2
    thr = threshold
    if thr < 0:
        thr = otsu(np.bincount(page.reshape(-1), minlength=256))
    if thr < 0:
        return np.zeros(page.shape, bool), thr
    return (page > thr) if light_text else (page <= thr), thr


def label_components(page, threshold=-1, light_text=0, connectivity=8, max_components=4096):
    """(labels (H, W) int32, comps (n_written, 6) int32 rows x0 y0 x1 y1 label area, info (4) int32)."""
    assert connectivity in (4, 8)
    ink, thr = ink_mask(page, threshold, light_text)
    H, W = ink.shape
    nb = N8 if connectivity == 8 else N4
    labels = np.full((H, W), -1, np.int32)
    comps = []
    for y, x in zip(*np.nonzero(ink)):                         # raster order
        if labels[y, x] >= 0:
            continue
        first = int(y) * W + int(x)
        labels[y, x] = first
        stack = [(int(y), int(x))]
        x0, y0, x1, y1, area = W, H, -1, -1, 0
        while stack:
            cy, cx = stack.pop()
            area += 1
            x0, y0, x1, y1 = min(x0, cx), min(y0, cy), max(x1, cx), max(y1, cy)
            for dy, dx in nb:
                ny, nx = cy + dy, cx + dx
                if 0 <= ny < H and 0 <= nx < W and ink[ny, nx] and labels[ny, nx] < 0:
                    labels[ny, nx] = first
                    stack.append((ny, nx))
        comps.append((x0, y0, x1 + 1, y1 + 1, first, area))
    info = np.array([thr, int(ink.sum()), len(comps), 0], np.int32)
    return labels, np.array(comps[:max_components], np.int32).reshape(-1, 6), info


def classify(comp, min_area, max_w, max_h):
    """0: stays, 1: a speck, 2: a rule.  Specks first."""
    x0, y0, x1, y1, _, area = (int(v) for v in comp)
    if area < min_area:
        return 1
    if (max_w > 0 and x1 - x0 > max_w) or (max_h > 0 and y1 - y0 > max_h):
        return 2
    return 0


def clean_page(page, **kw):
    """(out (H, W) uint8, counts (8) int32)."""
    p = dict(DEFAULTS)
    p.update(kw)
    assert p["min_area"] >= 1 and p["max_w"] >= 0 and p["max_h"] >= 0
    page = np.asarray(page)
    labels, comps, info = label_components(page, p["threshold"], p["light_text"], p["connectivity"], max_components=page.size)
    out = page.copy()
    fill = 0 if p["light_text"] else 255
    specks = rules = removed = 0
    for c in comps:
        k = classify(c, p["min_area"], p["max_w"], p["max_h"])
        if k == 0:
            continue
        specks += k == 1
        rules += k == 2
        removed += int(c[5])
        out[labels == c[4]] = fill
    return out, np.array([len(comps), specks, rules, info[0], info[1], removed, 0, 0], np.int32)
