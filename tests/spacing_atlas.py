"""Glyph-atlas pages for the spacing tests and for choosing the defaults of aocr_spacing_params: words of the shipped
atlas pasted on white as tests/test_segment_gpu.py::_atlas_page pastes them, one face per page, enlarged 1, 2 and 3 times with np.kron.  The
atlas is read as text (orient_cases.atlas): no device and no product import."""
import numpy as np

from orient_cases import atlas

CHARS = "0123456789abcdefghijklmnopqrstuvwxyz"
SPACE = 14               # columns between the last ink column of a word and the first of the next, at 1x
# a line of four words and more, a one-word line, a two-word line, and a line with a one-letter word and the widest letter gaps of the atlas
TEXT = [["hello", "w0rld", "42", "page"], ["segment"], ["kilo", "byte5"], ["minimum", "x", "jazzy", "illinois"], ["0123456789"]]
LINE_PITCH = 44
SCALES = (1, 2, 3)


def atlas_word(word, face):
    """coverage bitmap (gh, w) of a word: glyphs pasted at their pens, overlaps by maximum, cut behind the last ink column."""
    pixels, advance = atlas()
    gw = pixels.shape[3]
    gi = [CHARS.index(c) for c in word]
    adv = [int(advance[face, g]) for g in gi]
    out = np.zeros((pixels.shape[2], sum(adv) + gw), np.uint8)
    pen = 0
    for g, a in zip(gi, adv):
        out[:, pen:pen + gw] = np.maximum(out[:, pen:pen + gw], pixels[face, g])
        pen += a
    return out[:, :int(np.nonzero(out.any(axis=0))[0].max()) + 1]


def atlas_page(face, scale=1, text=TEXT, space=SPACE, thr=128):
    """(page, words): the text in one face, enlarged `scale` times; words: per line the (x0, x1) of every placed word's ink at threshold
    thr, in page columns."""
    lines = []
    for ln, ws in enumerate(text):
        x, placed = 16, []                                      # the first ink column of the next word
        for w in ws:
            bm = atlas_word(w, face)
            cols = np.nonzero(((255 - bm) <= thr).any(axis=0))[0]
            assert cols.min() <= x
            placed.append((x - int(cols.min()), bm))
            x += int(cols.max()) + 1 - int(cols.min()) + space
        lines.append(placed)
    W = max(x + bm.shape[1] for placed in lines for x, bm in placed) + 3
    page = np.full((4 + LINE_PITCH * len(text), W), 255, np.uint8)
    words = []
    for ln, placed in enumerate(lines):
        y, row = 4 + LINE_PITCH * ln, []
        for x, bm in placed:
            view = page[y:y + bm.shape[0], x:x + bm.shape[1]]
            view[:] = np.minimum(view, 255 - bm)
            cols = np.nonzero(((255 - bm) <= thr).any(axis=0))[0]
            row.append(((x + int(cols.min())) * scale, (x + int(cols.max()) + 1) * scale))
        words.append(row)
    return np.kron(page, np.ones((scale, scale), np.uint8)), words


def stacked_page():
    """the 131 x 470 page of tests/test_segment_gpu.py (its three lines, the faces taking turns) above its own 3x enlargement: body text and
    a headline on one page.  (page, words per line at threshold 128)"""
    lines = [(4, [(3, "hello"), (150, "w0rld"), (300, "42")]), (50, [(20, "page"), (170, "segment"), (380, "x")]), (97, [(0, "kilo"), (200, "byte5")])]
    page = np.full((131, 470), 255, np.uint8)
    words, i = [], 0
    for y, ws in lines:
        row = []
        for x, w in ws:
            bm = atlas_word(w, i % 3)
            i += 1
            view = page[y:y + bm.shape[0], x:x + bm.shape[1]]
            view[:] = np.minimum(view, 255 - bm)
            cols = np.nonzero(((255 - bm) <= 128).any(axis=0))[0]
            row.append((x + int(cols.min()), x + int(cols.max()) + 1))
        words.append(row)
    big = np.kron(page, np.ones((3, 3), np.uint8))
    out = np.full((131 + big.shape[0], big.shape[1]), 255, np.uint8)
    out[:131, :470] = page
    out[131:] = big
    return out, words + [[(3 * a, 3 * b) for a, b in row] for row in words]
