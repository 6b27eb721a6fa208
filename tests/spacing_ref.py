"""Plain numpy restatement of aocr_segment_page_spaced (include/aocr.h): aocr_segment_page with step 5 taking one word gap per band,
estimated from the band's own gaps between ink-column runs.  Loops and integers; the split is segment_ref.otsu, the function of step 2, on
the 256-bin histogram of clipped gap lengths.  Test infrastructure: it does not import the product."""
import numpy as np

from segment_ref import DEFAULTS, otsu, runs

SPACING = dict(min_gaps=4, lo_percent=25, hi_percent=80, default_percent=40, ratio_percent=150)       # the defaults of aocr.SpacingParams


def band_gap(flags, h, min_gaps, lo_percent, hi_percent, default_percent, ratio_percent):
    """the spacing row of one band without its trailing zeros: [gap used, flags, gaps counted m, a, c, band height].  flags: the ink-column
    flags of the band, h its height."""
    cr = runs(flags)
    m = max(len(cr) - 1, 0)
    lo = max(1, h * lo_percent // 100)
    hi = max(lo, h * hi_percent // 100)
    clip = min(hi, 255)
    hist = [0] * 256
    for j in range(1, len(cr)):
        hist[min(cr[j][0] - cr[j - 1][1], clip)] += 1
    t = otsu(hist)
    a = c = 0
    if t >= 0:
        a = max(v for v in range(t + 1) if hist[v])
        c = min(v for v in range(t + 1, 256) if hist[v])
    if m < min_gaps:
        flag = 1
    elif t < 0:
        flag = 2
    elif c * 100 < a * ratio_percent:
        flag = 3
    else:
        flag = 0
    est = (a + c + 1) >> 1 if flag == 0 else max(1, h * default_percent // 100)
    gap = min(max(est, lo), hi)
    if gap != est:
        flag += 4
    return [gap, flag, m, a, c, h]


def segment_page_spaced(page, max_boxes=1024, spacing=None, max_lines=None, **kw):
    """(boxes (n_written, 6) int32 rows x0 y0 x1 y1 line ink, counts (4) int32, rows (min(lines, max_lines), 8) int32: gap used, flags, gaps
    counted, a, c, band height, 0, 0).  Steps 1-4, 6 and 7 are those of segment_ref.segment_page; kw are its parameters (word_gap is not
    read, but 0 is an error as in the library)."""
    p = dict(DEFAULTS)
    p.update(kw)
    sp = dict(SPACING)
    sp.update(spacing or {})
    assert p["word_gap"] != 0
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
    for y0, y1 in runs(row_ink >= p["min_row_ink"]):
        if bands and y0 - bands[-1][1] <= p["merge_gap"]:
            bands[-1] = (bands[-1][0], y1)
        else:
            bands.append((y0, y1))
    bands = [b for b in bands if b[1] - b[0] >= p["min_line_h"]]
    boxes, rows = [], []
    for line, (y0, y1) in enumerate(bands):
        col_ink = ink[y0:y1].sum(axis=0)
        row = band_gap(col_ink >= 1, y1 - y0, **sp)
        rows.append(row + [0, 0])
        words = []
        for x0, x1 in runs(col_ink >= 1):
            if words and x0 - words[-1][1] < row[0]:
                words[-1] = (words[-1][0], x1)
            else:
                words.append((x0, x1))
        for x0, x1 in words:
            if x1 - x0 < p["min_word_w"]:
                continue
            boxes.append((max(0, x0 - p["pad_x"]), max(0, y0 - p["pad_y"]), min(W, x1 + p["pad_x"]), min(H, y1 + p["pad_y"]), line,
                          int(col_ink[x0:x1].sum())))
    counts = np.array([len(boxes), len(bands), thr, 0], np.int32)
    if max_lines is not None:
        rows = rows[:max_lines]
    return np.array(boxes[:max_boxes], np.int32).reshape(-1, 6), counts, np.array(rows, np.int32).reshape(-1, 8)
