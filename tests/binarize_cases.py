"""Pages for the binarisation tests, shared by test_binarize_cpu.py (the restatement alone) and test_binarize_gpu.py (the kernel against it).
Every expected page of CASES was written down by hand from the steps of the header, not computed."""
import numpy as np

from flatten_cases import clean_page


def _a(rows):
    return np.array(rows, np.uint8)


_DOT = np.full((3, 3), 200, np.uint8)
_DOT[1, 1] = 20

# name, page, params (radius, k_q8, range), expected gray output (hard = 0, dark text); the hard output is 0 where that is <= 127, else 255
CASES = [
    # q = 0: T = (93 * 205) / 256 = 74; paper: 128 + ((93 - 74 - 1) * 127) / (254 - 74) = 128 + 2286 / 180 = 140
    ("constant", np.full((7, 9), 93, np.uint8), (2, 51, 128), np.full((7, 9), 140, np.uint8)),
    # c = 1: T = 205 / 256 = 0; paper: 128 + ((1 - 0 - 1) * 127) / 254 = 128
    ("constant_1", np.full((4, 3), 1, np.uint8), (1, 51, 128), np.full((4, 3), 128, np.uint8)),
    # c = 0: T = 0, v <= T: ink, (0 * 127) / max(0, 1) = 0
    ("constant_0", np.zeros((6, 5), np.uint8), (3, 51, 128), np.zeros((6, 5), np.uint8)),
    # n = 1, D = 0: T = (77 * 205) / 256 = 61; paper: 128 + (15 * 127) / 193 = 128 + 9
    ("one_pixel", _a([[77]]), (1, 51, 128), _a([[137]])),
    ("one_pixel_r63", _a([[77]]), (63, 51, 128), _a([[137]])),
    # a dark pixel 20 in the middle of 3 x 3 paper at 200, r = 1: the windows hold 9, 6 (edges) and 4 (corners) pixels, all with the dot.
    # centre: S1 = 1620, S2 = 320400, D = 9 * 320400 - 1620^2 = 259200, q = 509; T = 1620 * (205*128*9 + 51*509) / (256*128*81)
    #         = 1620 * 262119 / 2654208 = 159; ink: (20 * 127) / 159 = 15
    # edge:   S1 = 1020, S2 = 200400, D = 162000, q = 402; T = 1020 * (157440 + 20502) / 1179648 = 153; paper: 128 + (46 * 127) / 101 = 185
    # corner: S1 = 620, S2 = 120400, D = 97200, q = 311; T = 620 * (104960 + 15861) / 524288 = 142; paper: 128 + (57 * 127) / 112 = 192
    ("dark_pixel", _DOT, (1, 51, 128), _a([[192, 185, 192], [185, 15, 185], [192, 185, 192]])),
    # k = 0: T is the floored mean of the window.  Columns 100 100 200 200, r = 1: the means are 100, 400 / 3 = 133, 500 / 3 = 166, 200.
    # x = 0: v = T: ink, 127;  x = 1: ink, 12700 / 133 = 95;  x = 2: paper, 128 + (33 * 127) / 88 = 175;  x = 3: v = T: ink, 127
    ("step_edge_mean", _a([[100, 100, 200, 200]] * 3), (1, 0, 128), _a([[127, 95, 175, 127]] * 3)),
    ("step_edge_mean_down", _a([[100, 100, 200, 200]] * 3).T.copy(), (1, 0, 77), _a([[127, 95, 175, 127]] * 3).T.copy()),
    # the same edge with k = 51 / 256, R = 128, r = 1 (every window spans the three rows: D carries the factor 9 or 4 of the row count).
    # x = 0: n = 6 (rows clipped: 4), flat 100: T = (100 * 205) / 256 = 80; paper: 128 + (19 * 127) / 174 = 141
    # x = 1, middle row: n = 9, S1 = 1200, S2 = 180000, D = 180000, q = 424; T = 1200 * (236160 + 21624) / 2654208 = 116;
    #        ink: 12700 / 116 = 109.  Rows 0 and 2: n = 6, S1 = 800, S2 = 120000, D = 80000, q = 282; T = 800 * (157440 + 14382) / 1179648
    #        = 116 as well
    # x = 2, middle row: S1 = 1500, S2 = 270000, D = 180000, q = 424; T = 1500 * 257784 / 2654208 = 145; paper: 128 + (54 * 127) / 109 = 190.
    #        Rows 0 and 2: S1 = 1000, S2 = 180000, D = 80000, q = 282; T = 1000 * 171822 / 1179648 = 145
    # x = 3: flat 200: T = (200 * 205) / 256 = 160; paper: 128 + (39 * 127) / 94 = 180
    ("step_edge", _a([[100, 100, 200, 200]] * 3), (1, 51, 128), _a([[141, 109, 190, 180]] * 3)),
]


def hard_of(gray):
    return np.where(gray <= 127, 0, 255).astype(np.uint8)


# ---- the stained, faded page -----------------------------------------------------------------------------------------------------------------
# The clean 600 x 800 word page of flatten_cases (15 lines at rows 40 + 34 i, 20 rows high, 109 words), painted with these levels:
PAPER = 235
INK = 40                  # strong print: the top half of the page
FADED = 175               # the print of every line from FADED_ROW down: its ink is lighter than the stain's paper
FADED_ROW = 300
STAIN = 140               # the stain's paper at its core, darker than the faded ink: no global threshold keeps both
STAIN_CORE = (100, 180, 120, 520)     # y0, y1, x0, x1: the core covers lines 2, 3 and 4 (rows 108..196) in part or whole
STAIN_RAMP = 48           # the stain fades out linearly over this many pixels around the core.
# Levels chosen, and why the edge is a ramp.  Sauvola's T at a pixel just inside a SHARP edge between paper b and stain d, with the fraction
# f of the window on the bright side, is about (d + (b-d) f) (1 - k + k (b-d) sqrt(f (1-f)) / R): with b = 235, d = 140, k = 0.2, R = 128 and
# f = 0.5 that is 164 > 140, so a rim some 0.27 (2r+1) pixels wide inside the stain is read as ink and joins the lines it crosses.  That is the method, not
# the kernel (include/aocr.h lists it among the limits), so the fixture's stain has an edge wider than the window (48 > 41): on a linear ramp
# the pixel is the window's mean and T is about 0.83 of it.  Faded ink at 175 on paper 235 is found with the default k: over a line 20 rows
# high at 45 % density the window holds about 22 % ink, the mean is about 222, the deviation about 25 and T about 186 >= 175; a lone
# faded pixel sees T = (235 * 205) / 256 = 188.

_pages = {}


def stain_level():
    """the paper level under the stain, (600, 800) int64: STAIN inside the core, PAPER from STAIN_RAMP pixels outside it, linear between
    (the Chebyshev distance to the core: rectangular contours)."""
    H, W = clean_page().shape
    y0, y1, x0, x1 = STAIN_CORE
    y = np.arange(H, dtype=np.int64)[:, None]
    x = np.arange(W, dtype=np.int64)[None, :]
    dy = np.maximum(np.maximum(y0 - y, y - (y1 - 1)), 0)
    dx = np.maximum(np.maximum(x0 - x, x - (x1 - 1)), 0)
    d = np.minimum(np.maximum(dy, dx), STAIN_RAMP)
    return PAPER - ((PAPER - STAIN) * (STAIN_RAMP - d)) // STAIN_RAMP


def stained_page():
    """(the clean 0 / 255 page, the stained and faded gray page): each computed once."""
    if "stained" not in _pages:
        clean = clean_page()
        ink = clean < 128
        gray = np.full(clean.shape, PAPER, np.int64)
        gray[ink] = INK
        faded = ink.copy()
        faded[:FADED_ROW] = False
        gray[faded] = FADED
        _pages["clean"] = clean
        _pages["stained"] = ((gray * stain_level()) // PAPER).astype(np.uint8)
    return _pages["clean"], _pages["stained"]
