"""Plain numpy restatement of aocr_rotate_page and aocr_estimate_orientation (include/aocr.h).  Test infrastructure: it does not import the
product."""
import numpy as np

from skew_ref import ink_mask


def rotate(page, q):
    """the page turned by q clockwise quarter turns."""
    return np.ascontiguousarray(np.rot90(np.asarray(page), -(int(q) & 3)))


def effective_quarter(quarter, orient_word=None):
    """q of aocr_rotate_page: the host's quarter plus the half-turn bit of orient_dev[0]."""
    return (int(quarter) + ((int(orient_word) & 2) if orient_word is not None else 0)) & 3


def run_starts(ink):
    """(N_h, N_v): ink pixels whose left / upper neighbour is paper or off the page."""
    ink = np.asarray(ink, bool)
    left = np.zeros_like(ink)
    left[:, 1:] = ink[:, :-1]
    up = np.zeros_like(ink)
    up[1:, :] = ink[:-1, :]
    return int((ink & ~left).sum()), int((ink & ~up).sum())


def estimate_orientation(page, threshold=-1, light_text=0):
    """orient (8) int32: axis, N_h, N_v, the threshold used, the total ink, 0, 0, 0."""
    ink, thr = ink_mask(page, threshold, light_text)
    nh, nv = run_starts(ink)
    return np.array([1 if nv > nh else 0, nh, nv, thr, int(ink.sum()), 0, 0, 0], np.int32)


def unrotate_boxes(boxes, quarter, H, W):
    """half-open boxes x0 y0 x1 y1 on rotate(page, quarter) -> boxes on the (H, W) page, by the mapping of aocr_rotate_page."""
    out = []
    q = int(quarter) & 3
    for x0, y0, x1, y1 in np.asarray(boxes, np.int64).reshape(-1, 4).tolist():
        out.append({0: [x0, y0, x1, y1], 1: [y0, H - x1, y1, H - x0], 2: [W - x1, H - y1, W - x0, H - y0], 3: [W - y1, x0, W - y0, x1]}[q])
    return np.array(out, np.int64).reshape(-1, 4)
