"""Pages for the deskew tests, shared by test_skew_cpu.py (the restatement alone) and test_skew_gpu.py (the kernels against it)."""
import numpy as np

import skew_ref as S

PLANTED_SHAPE = (600, 800)
PLANTED_K0 = (0, 5, -17, 40, -64, 96)           # planted slopes, in steps of 64 / 65536 rows per column
PLANTED = dict(step_q16=64, n_steps=100, threshold=128)
SEGMENT = dict(threshold=128)                   # segment_ref parameters for the planted pages (the rest: its defaults)


def text_page(H, W, seed, light=False, margin=40, line_h=20, pitch=34):
    """paper 255 (0 with light), lines line_h rows high every `pitch` rows, words 30..120 columns wide at 45 % ink density with gaps of 14..25
    columns, inside `margin`.  Pages too small for the margin shrink it, and the first word of a line is cut to the page."""
    rng = np.random.default_rng(seed)
    paper, ink = (0, 255) if light else (255, 0)
    page = np.full((H, W), paper, np.uint8)
    margin = min(margin, H // 8, W // 8)
    y = margin
    while y + line_h <= H - margin:
        x = margin
        while True:
            w = int(rng.integers(30, 121))
            if x == margin:
                w = min(w, W - 2 * margin)                  # a narrow page still gets one word per line
            if x + w > W - margin or w < 1:
                break
            page[y:y + line_h, x:x + w] = np.where(rng.random((line_h, w)) < 0.45, ink, paper)
            x += w + int(rng.integers(14, 26))
        y += pitch
    return page


_planted = {}


def planted_page(k0):
    """(the straight 600 x 800 page, the page skewed so that the text lines have slope k0 * 64 / 65536): each computed once."""
    if "straight" not in _planted:
        _planted["straight"] = text_page(*PLANTED_SHAPE, seed=600800)
    if k0 not in _planted:
        _planted[k0] = S.deskew(_planted["straight"], -k0 * 64)
    return _planted["straight"], _planted[k0]


def noise_page(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


def tie_page():
    """Symmetric under the shear sign: W = 64 (cx = 32, strip centres 16 and 48), strip 0 inked on rows 10 and 14, strip 1 on row 12.  With
    step 4096 the offsets of k = +1 are (-1, +1) and those of k = -1 are (+1, -1): one aligns row 12 with row 14, the other with row 10, both
    score 64^2 + 32^2 = 5120 against 3 * 32^2 = 3072 for every other candidate.  The order 0, -1, +1, ... makes -1 the winner."""
    page = np.full((24, 64), 255, np.uint8)
    page[10, 0:32] = 0
    page[14, 0:32] = 0
    page[12, 32:64] = 0
    return page
