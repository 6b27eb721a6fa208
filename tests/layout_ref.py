"""Plain numpy restatement of aocr_ink_integral and aocr_layout_blocks (include/aocr.h): the summed-area table of the ink mask as a double
cumsum, and the recursive XY cut as plain loops over level lists.  Written from the header text.  Test infrastructure: it does not import
the product."""
import numpy as np

import segment_ref as R

DEFAULTS = dict(min_ink=1, gap_x=24, gap_y=30, max_depth=8, min_block_w=8, min_block_h=8, min_block_ink=16)


def ink_mask(page, threshold=-1, light_text=0):
    """(mask (H, W) bool, the threshold used)."""
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim == 2
    thr = threshold
    if thr < 0:
        thr = R.otsu(np.bincount(page.reshape(-1), minlength=256))
    if thr < 0:
        return np.zeros(page.shape, bool), thr
    return (page > thr) if light_text else (page <= thr), thr


def ink_integral(page, threshold=-1, light_text=0):
    """(S (H+1, W+1) int64 with a zero row 0 and column 0, info (4) int32: threshold, total ink, 0, 0)."""
    mask, thr = ink_mask(page, threshold, light_text)
    H, W = mask.shape
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = mask.astype(np.int64).cumsum(axis=0).cumsum(axis=1)
    return S, np.array([thr, S[H, W], 0, 0], np.int32)


def rect(S, x0, y0, x1, y1):
    return int(S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0])


def pieces(occupied, gap):
    """maximal runs of occupied elements, runs with fewer than `gap` unoccupied elements between them merged (chaining): half-open pairs."""
    out = []
    for s, e in R.runs(occupied):
        if out and s - out[-1][1] < gap:
            out[-1] = (out[-1][0], e)
        else:
            out.append((s, e))
    return out


def tighten(S, reg, min_ink):
    x0, y0, x1, y1 = reg
    cols = [x for x in range(x0, x1) if rect(S, x, y0, x + 1, y1) >= min_ink]
    if not cols:
        return None
    x0, x1 = cols[0], cols[-1] + 1
    rows = [y for y in range(y0, y1) if rect(S, x0, y, x1, y + 1) >= min_ink]
    if not rows:
        return None
    return (x0, rows[0], x1, rows[-1] + 1)


def layout_blocks(S, max_blocks=256, info=None, **kw):
    """(blocks (n_written, 6) int32 rows x0 y0 x1 y1 depth ink, counts (4) int32: written, levels kept, dropped by size, overflow).
    info: a dict that receives the final list before the size filter."""
    p = dict(DEFAULTS)
    p.update(kw)
    H, W = S.shape[0] - 1, S.shape[1] - 1
    first = tighten(S, (0, 0, W, H), p["min_ink"])
    level = [dict(box=first, depth=0, leaf=False)] if first else []
    levels = overflow = 0
    for d in range(p["max_depth"]):
        nxt, cut_any = [], False
        for reg in level:
            if reg["leaf"]:
                nxt.append(reg)
                continue
            x0, y0, x1, y1 = reg["box"]
            ps = pieces([rect(S, x, y0, x + 1, y1) >= p["min_ink"] for x in range(x0, x1)], p["gap_x"])
            if len(ps) >= 2:
                kids = [(x0 + s, y0, x0 + e, y1) for s, e in ps]
            else:
                ps = pieces([rect(S, x0, y, x1, y + 1) >= p["min_ink"] for y in range(y0, y1)], p["gap_y"])
                kids = [(x0, y0 + s, x1, y0 + e) for s, e in ps] if len(ps) >= 2 else None
            if kids is None:
                nxt.append(dict(reg, leaf=True))
                continue
            cut_any = True
            for k in kids:
                t = tighten(S, k, p["min_ink"])
                if t is not None:
                    nxt.append(dict(box=t, depth=d + 1, leaf=False))
        if len(nxt) > max_blocks:
            overflow = 1
            break
        if not cut_any:
            break
        level = nxt
        levels += 1
    if info is not None:
        info.update(final=[r["box"] + (r["depth"],) for r in level])
    out = []
    for reg in level:
        x0, y0, x1, y1 = reg["box"]
        ink = rect(S, x0, y0, x1, y1)
        if x1 - x0 >= p["min_block_w"] and y1 - y0 >= p["min_block_h"] and ink >= p["min_block_ink"]:
            out.append((x0, y0, x1, y1, reg["depth"], ink))
    counts = np.array([len(out), levels, len(level) - len(out), overflow], np.int32)
    return np.array(out, np.int32).reshape(-1, 6), counts


def layout_page(page, threshold=-1, light_text=0, max_blocks=256, **kw):
    """(blocks, counts, info) of a page: both calls in a row."""
    S, info = ink_integral(page, threshold, light_text)
    blocks, counts = layout_blocks(S, max_blocks, **kw)
    return blocks, counts, info


def segment_blocks(page, blocks, max_boxes=1024, **seg):
    """aocr_segment_page block by block, as Model.recognize_page(layout=...) does it: every block is a page of its own (padding clamps to the
    block), its boxes are shifted to page coordinates and its line numbers continue after the previous block's.  seg must carry a fixed
    threshold (the page's).  (boxes (n, 6) int32, block id (n), lines, found, truncated)."""
    rows, ids = [], []
    lines = found = 0
    truncated = False
    for b, (x0, y0, x1, y1) in enumerate(np.asarray(blocks)[:, :4].tolist()):
        bx, c = R.segment_page(np.ascontiguousarray(page[y0:y1, x0:x1]), max_boxes=max_boxes, **seg)
        bx = bx.astype(np.int64)
        bx[:, [0, 2]] += x0
        bx[:, [1, 3]] += y0
        bx[:, 4] += lines
        rows.append(bx)
        ids += [b] * len(bx)
        lines += int(c[1])
        found += int(c[0])
        truncated |= bool(c[0] > max_boxes)
    boxes = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 6), np.int32)
    return boxes, np.array(ids, np.int32), lines, found, truncated
