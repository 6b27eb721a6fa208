"""Pages for the slant tests, shared by test_slant_cpu.py (the restatement alone) and test_slant_gpu.py (the kernels against it): bar words
whose slant is known by construction, the hand-written 5 x 7 stroke, words rendered from the shipped glyph atlas (aocr/glyph_atlas.txt read
as text by orient_cases.atlas, drawn by synth_ref.synth) and sheared by a known candidate, and one seeded page with every kind of box."""
import numpy as np

import slant_ref as R
import synth_ref as Y
from orient_cases import atlas

DEFAULTS = dict(threshold=128, light_text=0, step_q16=4096, n_steps=12)
PLANTED_K = (-12, -3, 0, 5, 12)


def shear_into(page, ink, x0, y0, s):
    """paints the ink mask (h, w) dark into the page, row y0 + r moved along x by off(y0 + r) about the mask's middle row: pixel (r, c) of
    the upright mask lands on column x0 + c + off -- the spec's own offsets, so candidate s reads the mask back upright."""
    h, w = ink.shape
    cy = (y0 + y0 + h) >> 1
    for r in range(h):
        o = R.off(cy, y0 + r, s)
        cols = np.flatnonzero(ink[r]) + x0 + o
        assert cols.size == 0 or (cols.min() >= 0 and cols.max() < page.shape[1])
        page[y0 + r, cols] = 0


def bar_word(k, h=40, bars=(0, 9, 14, 27, 33), step_q16=4096):
    """(page, box): full-height vertical bars two pixels wide at the upright columns `bars`, leaning by candidate k.  The box is the whole
    sheared word.  At candidate k every profile column is 0 or h, so its score 2 * len(bars) * h^2 is the largest a box with this much ink
    can have, and any other candidate breaks a column."""
    assert h >= 32
    ink = np.zeros((h, max(bars) + 2), bool)
    for c in bars:
        ink[:, c:c + 2] = True
    D = R.extent(8, 8 + h, k * step_q16)
    page = np.full((h + 16, ink.shape[1] + 2 * D + 24), 255, np.uint8)
    x0 = 12 + D
    shear_into(page, ink, x0, 8, k * step_q16)
    return page, np.array([x0 - D, 8, x0 + ink.shape[1] + D, 8 + h, 0, 0], np.int32)


def bar_page(ks=PLANTED_K, h=40):
    """the bar words of `ks` next to each other on one page: (page, boxes (n, 6), the planted k of every box)"""
    words = [bar_word(k, h) for k in ks]
    W = sum(p.shape[1] for p, _ in words)
    page = np.full((h + 16, W), 255, np.uint8)
    boxes, x = [], 0
    for p, b in words:
        page[:, x:x + p.shape[1]] = p
        boxes.append(b + np.array([x, 0, x, 0, 0, 0], np.int32))
        x += p.shape[1]
    return page, np.stack(boxes), np.array(ks, np.int32)


def stroke_5x7(right=True):
    """a one-pixel stroke through a 5 x 7 page at 45 degrees, from (row 0, column 5) to (row 4, column 1) when `right`, mirrored otherwise.
    With step_q16 = 8192 and n_steps = 8 the offsets of candidate 8 (s = 65536, cy = 2) are +2 +1 0 -1 -2 for rows 0..4, and those of
    candidate 7 round to the same."""
    page = np.full((5, 7), 255, np.uint8)
    for y in range(5):
        page[y, 5 - y if right else 1 + y] = 0
    return page


STROKE = dict(threshold=128, light_text=0, step_q16=8192, n_steps=8)

# ---- glyph words ---------------------------------------------------------------------------------------------------------------------------------
# (word, face, planted k): the committed list on which the restatement lands within one step at the defaults (test_slant_cpu.py asserts it;
# DESIGN.md section 22 says how many of the words tried do)
GLYPH_WORDS = [("hill", 0, 6), ("milk", 0, -4), ("built", 0, 8), ("fifth", 0, 3), ("until", 0, -7), ("limit", 0, 10), ("thin", 0, 0),
               ("hill", 1, 5), ("milk", 1, -6), ("fifth", 1, 9), ("limit", 1, -3), ("built", 2, 4), ("until", 2, -9), ("thin", 2, 7),
               ("width", 0, -10), ("think", 1, 2), ("little", 2, -5), ("1411", 0, 6), ("hundred", 1, -8), ("filled", 0, 11)]
# every word tried for DESIGN.md's count: the committed ones and those that miss
GLYPH_TRIED = ["hill", "milk", "built", "fifth", "until", "limit", "thin", "width", "think", "little", "1411", "hundred", "filled", "soon",
               "access", "zero", "wavy", "ox", "808", "cocoa", "seas", "sway", "eve", "swam"]

_words = {}


def upright_word(word, face):
    """the ink mask (32, w) of a word drawn by synth_ref.synth from the shipped atlas at its native size, dark where the coverage is at
    least half"""
    if (word, face) not in _words:
        pixels, advance = atlas()
        ids = [4 + (int(c) if c.isdigit() else 10 + ord(c) - ord("a")) for c in word]
        W = int(sum(int(advance[face, i - 4]) for i in ids)) + pixels.shape[3]
        img = Y.synth(Y.pack([ids], 16), pixels, advance.astype(np.uint8), Y.style_records([(0, face, 0.0, 1.0, 1.0, 0.0, 0.0, 255.0, 0.0)]),
                      pixels.shape[2], W)[0, 0]
        ink = img >= 128
        cols = np.flatnonzero(ink.any(axis=0))
        _words[(word, face)] = ink[:, cols[0]:cols[-1] + 1]
    return _words[(word, face)]


def glyph_word(word, face, k, step_q16=4096):
    """(page, box): the word leaning by candidate k, the box two pixels around the ink rows and the sheared columns"""
    ink = upright_word(word, face)
    rows = np.flatnonzero(ink.any(axis=1))
    ink = ink[rows[0]:rows[-1] + 1]
    h, w = ink.shape
    D = R.extent(4, 4 + h, k * step_q16)
    page = np.full((h + 8, w + 2 * D + 8), 255, np.uint8)
    shear_into(page, ink, 4 + D, 4, k * step_q16)
    ys, xs = np.nonzero(page < 128)
    return page, np.array([xs.min() - 2, ys.min() - 2, xs.max() + 3, ys.max() + 3, 0, 0], np.int32)


# ---- the seeded page -------------------------------------------------------------------------------------------------------------------------------
SEEDED_SHAPE = (300, 1300)
SPECIAL_BOXES = [
    (10, 10, 11, 11),            # 1 x 1
    (20, 5, 120, 261),           # h = 256: the tallest box that is estimated
    (130, 5, 200, 262),          # h = 257: flag 1
    (-20, 50, 30, 90),           # over the left edge
    (1280, 40, 1400, 100),       # over the right edge
    (300, -30, 380, 20),         # over the top
    (400, 280, 500, 400),        # over the bottom
    (-5, -5, 40, 30),            # over a corner
    (100, 100, 1250, 140),       # 1150 columns: more than four column chunks of 256
    (0, 20, 700, 276),           # h = 256 and three chunks: the widest halo
    (700, 0, 1290, 300),         # the page's full height: flag 1, its ink counted over several chunks
    (500, 50, 620, 100),         # two boxes that overlap
    (560, 60, 700, 120),
    (50, 20, 40, 10),            # inverted: flag 2
    (2000, 10, 2100, 40),        # wholly outside: flag 2
    (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1),      # the whole page after clamping: flag 1
]

_seeded = {}


def seeded_page():
    """(page (300, 1300) uint8, boxes (n, 6) int32): sparse random ink (one pixel in six is dark, gray levels on both sides of 128), bar
    words planted in three places, the special boxes and 26 random ones"""
    if "p" not in _seeded:
        rng = np.random.default_rng(3001300)
        H, W = SEEDED_SHAPE
        page = rng.integers(129, 256, size=(H, W), dtype=np.uint8)
        dark = rng.random((H, W)) < 1 / 6
        page[dark] = rng.integers(0, 129, size=int(dark.sum()), dtype=np.uint8)
        boxes = [b + (0, 0) for b in SPECIAL_BOXES]
        for i, k in enumerate((7, -11, 2)):
            p, b = bar_word(k)
            y, x = 120 + 50 * i, 60 + 400 * i
            page[y:y + p.shape[0], x:x + p.shape[1]] = p
            boxes.append(tuple(int(v) for v in b + np.array([x, y, x, y, 0, 0])))
        for _ in range(26):
            w, h = int(rng.integers(4, 300)), int(rng.integers(3, 90))
            x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
            boxes.append((x, y, x + w, y + h, 0, 0))
        _seeded["p"] = (page, np.array(boxes, np.int64).astype(np.int32))
    return _seeded["p"]
