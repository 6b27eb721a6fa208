"""Plain numpy restatement of aocr_segment_page (include/aocr.h, steps 1-7): projection-profile page segmentation.  Loops, integers, and the
Otsu scores in np.float64 scalars in the stated order.  Test infrastructure: it does not import the product."""
import numpy as np

DEFAULTS = dict(threshold=-1, light_text=0, min_row_ink=1, merge_gap=2, min_line_h=8, word_gap=12, min_word_w=4, pad_x=2, pad_y=2)


def otsu(hist):
    """the first t in 0..254 with the strictly largest between-class score; -1 when no t splits the page into two non-empty classes."""
    h = [int(v) for v in hist]
    N = sum(h)
    S = sum(v * h[v] for v in range(256))
    n0 = s0 = 0
    best, best_t = np.float64(-1.0), -1
    for t in range(255):
        n0 += h[t]
        s0 += t * h[t]
        n1 = N - n0
        if n0 == 0 or n1 == 0:
            continue
        d = np.float64(s0) * np.float64(n1) - np.float64(S - s0) * np.float64(n0)
        score = (d * d) / (np.float64(n0) * np.float64(n1))
        if score > best:
            best, best_t = score, t
    return best_t


def runs(flags):
    """maximal runs of set elements as half-open (start, end) pairs."""
    out, start = [], None
    for i, f in enumerate(list(flags) + [False]):
        if f and start is None:
            start = i
        elif not f and start is not None:
            out.append((start, i))
            start = None
    return out


def segment_page(page, max_boxes=1024, info=None, **kw):
    """(boxes (n_written, 6) int32 rows x0 y0 x1 y1 line ink, counts (4) int32).  info: a dict that receives what happened on the way
    (row runs, bands before and after the height filter, words before and after the width filter), for tests that must see every branch taken."""
    p = dict(DEFAULTS)
    p.update(kw)
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim == 2
    H, W = page.shape
    thr = p["threshold"]
    if thr < 0:
        thr = otsu(np.bincount(page.reshape(-1), minlength=256))
    if thr < 0:
        ink = np.zeros((H, W), bool)
    elif p["light_text"]:
        ink = page > thr
    else:
        ink = page <= thr
    row_ink = ink.sum(axis=1)
    bands = []
    row_runs = runs(row_ink >= p["min_row_ink"])
    for y0, y1 in row_runs:
        if bands and y0 - bands[-1][1] <= p["merge_gap"]:      # the gap to the previous ORIGINAL run, which ends where the merged band ends
            bands[-1] = (bands[-1][0], y1)
        else:
            bands.append((y0, y1))
    merged = len(bands)
    bands = [b for b in bands if b[1] - b[0] >= p["min_line_h"]]
    boxes = []
    col_runs = words_merged = 0
    for line, (y0, y1) in enumerate(bands):
        col_ink = ink[y0:y1].sum(axis=0)
        cr = runs(col_ink >= 1)
        words = []
        if p["word_gap"] == 0:
            if cr:
                words = [(cr[0][0], cr[-1][1])]
        else:
            for x0, x1 in cr:
                if words and x0 - words[-1][1] < p["word_gap"]:
                    words[-1] = (words[-1][0], x1)
                else:
                    words.append((x0, x1))
        col_runs += len(cr)
        words_merged += len(words)
        for x0, x1 in words:
            if x1 - x0 < p["min_word_w"]:
                continue
            boxes.append((max(0, x0 - p["pad_x"]), max(0, y0 - p["pad_y"]), min(W, x1 + p["pad_x"]), min(H, y1 + p["pad_y"]), line,
                          int(col_ink[x0:x1].sum())))
    if info is not None:
        info.update(row_runs=len(row_runs), bands_merged=merged, lines=len(bands), col_runs=col_runs, words_merged=words_merged, boxes=len(boxes),
                    max_boxes_per_line=max(np.bincount([b[4] for b in boxes]).tolist()) if boxes else 0)
    counts = np.array([len(boxes), len(bands), thr, 0], np.int32)
    return np.array(boxes[:max_boxes], np.int32).reshape(-1, 6), counts
