"""Pages for the flattening tests, shared by test_flatten_cpu.py (the restatement alone) and test_flatten_gpu.py (the kernels against it).
Every expected page of CASES was written down by hand from the three steps of the header, not computed."""
import numpy as np

from skew_cases import planted_page, text_page


def _a(rows):
    return np.array(rows, np.uint8)


_INK = np.full((5, 5), 100, np.uint8)
_INK[2, 2] = 40
_INK_OUT = np.full((5, 5), 255, np.uint8)
_INK_OUT[2, 2] = 102
_CORNER = np.full((3, 3), 120, np.uint8)
_CORNER[0, 0] = 60
_CORNER_OUT = np.full((3, 3), 255, np.uint8)
_CORNER_OUT[0, 0] = 128

# name, page, radius, light_text, expected
CASES = [
    ("constant", np.full((7, 9), 93, np.uint8), 2, 0, np.full((7, 9), 255, np.uint8)),
    ("constant_1", np.full((4, 3), 1, np.uint8), 1, 0, np.full((4, 3), 255, np.uint8)),
    ("constant_0", np.zeros((6, 5), np.uint8), 3, 0, np.zeros((6, 5), np.uint8)),
    ("one_pixel", _a([[77]]), 1, 0, _a([[255]])),
    ("one_pixel_r127", _a([[77]]), 127, 0, _a([[255]])),
    # every 3 x 3 window holds paper: M = B = 100; paper (100*255 + 50) / 100 = 255, ink (40*255 + 50) / 100 = 10250 / 100 = 102
    ("ink_pixel", _INK, 1, 0, _INK_OUT),
    # every clipped window of a 3 x 3 page holds a 120: M = B = 120; the corner (60*255 + 60) / 120 = 128
    ("corner_pixel", _CORNER, 1, 0, _CORNER_OUT),
    # columns 100 100 200 200, three rows.  M = 100 200 200 200 in every row.  Row sums of M over the clipped window: 300 (2 columns), 500 (3),
    # 600 (3), 400 (2); rows 0 and 2 see 2 rows, row 1 sees 3.  B at x = 0: n = 4: (600 + 2) / 4 = 150, n = 6: (900 + 3) / 6 = 150;
    # x = 1: n = 6: (1000 + 3) / 6 = 167, n = 9: (1500 + 4) / 9 = 167; x = 2: 200; x = 3: n = 4: (800 + 2) / 4 = 200.
    # out: (100*255 + 75) / 150 = 170, (100*255 + 83) / 167 = 153, (200*255 + 100) / 200 = 255
    ("step_edge", _a([[100, 100, 200, 200]] * 3), 1, 0, _a([[170, 153, 255, 255]] * 3)),
    ("step_edge_down", _a([[100, 100, 200, 200]] * 3).T.copy(), 1, 0, _a([[170, 153, 255, 255]] * 3).T.copy()),
    # the mirror image of ink_pixel: light ink 215 on dark paper 155; the result is 255 - (255, 102)
    ("light_ink_pixel", (255 - _INK).astype(np.uint8), 1, 1, (255 - _INK_OUT).astype(np.uint8)),
    ("light_constant", np.full((5, 4), 200, np.uint8), 2, 1, np.zeros((5, 4), np.uint8)),
    ("light_constant_255", np.full((5, 4), 255, np.uint8), 2, 1, np.full((5, 4), 255, np.uint8)),
]

LIT_SHAPE = (600, 800)
LIT_SEED = 600800
LIT_FLOORS = (110, 90, 70)            # the multiplier at the dim edge of the page, of 256


def repaint(page, ink=40, paper=230):
    """a 0 / 255 page as ink 40 on paper 230."""
    return np.where(page < 128, ink, paper).astype(np.uint8)


def light(gray, floor=110):
    """lit = (gray * L) >> 8 with L(x, y) = 256 - ((256-floor)*x)//(W-1) - (20*y)//(H-1): bright at the left edge, `floor`/256 at the right."""
    H, W = gray.shape
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    L = 256 - ((256 - floor) * x) // max(W - 1, 1) - (20 * y) // max(H - 1, 1)
    return ((gray.astype(np.int64) * L) >> 8).astype(np.uint8)


_lit = {}


def lit_page(floor=110, k0=0):
    """(the straight clean 600 x 800 page of skew_cases, that page sheared by k0 steps, repainted and lit): each computed once."""
    straight, skewed = planted_page(k0)
    if (floor, k0) not in _lit:
        _lit[(floor, k0)] = light(repaint(skewed), floor)
    return straight, _lit[(floor, k0)]


def clean_page():
    return text_page(*LIT_SHAPE, seed=LIT_SEED)
