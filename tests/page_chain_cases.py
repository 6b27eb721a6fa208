"""One planted photograph on which every stage of Model.recognize_page has work to do, shared by test_page_chain_cpu.py (the numpy chain
alone) and test_page_chain_gpu.py (recognize_page against it).  Test infrastructure: numpy and the other case builders, no product import.

The page at its normalised size (302 x 480, glyphs of the shipped atlas at their native 32 rows):
  - a headline across the page: a word leaning by slant candidate 6 (slant_cases.glyph_word) and two upright ones, 30 columns apart;
  - a reversed-out header slab, 44 rows high, with three light words on it;
  - two columns of three lines each with a gutter of 36 columns, their words 10 columns apart: no fixed word_gap cuts both the headline
    and the body; the right column is faded print;
  - a form rule, two rows thick, through the last rows of the stems of both columns' first line and across the gutter: with it the
    line is one word, and the XY cut finds no gutter;
  - a red stroke that joins two words of the right column;
  - specks of 1 and 4 pixels in the margins and the gutter.
It is then curled (curl_cases.sag, 5 rows), sheared (skew_ref.deskew, -17 steps of 64 / 65536), turned upside down, doubled (np.kron),
stained (binarize_cases' ramped stain: its paper is darker than the faded print) and lit by a ramp, tinted (the paper is yellowish) and
photographed with rectify_ref.make_photo's keystone on a desk: 664 x 1040 x 3, under the 1260 x 1680 of test_recognize_gpu.py's page."""
import numpy as np

import rectify_ref as RR
import skew_ref as SK
from curl_cases import sag
from slant_cases import glyph_word
from spacing_atlas import atlas_word

H1, W1 = 302, 480
PAPER, INK, FADED, STAIN, STAIN_RAMP, DESK = 235, 40, 165, 140, 48, 50
HEADLINE_Y, SLAB = 10, (12, 78, 468, 122)                   # x0 y0 x1 y1
BODY_Y, PITCH, COLUMNS, COLUMN_W = 158, 44, (14, 258), 208
HEAD_SPACE, BODY_SPACE = 30, 10
SAG, SHEAR = 5, -17 * 64
HUE_RED = 0                                                 # AOCR_HUE_RED
BODY = [[["pump", "hunk", "x"], ["bunk", "42", "nun"], ["dumb", "x", "hub"]],
        [["numb", "punk"], ["mud", "bump", "x"], ["dunk", "hmm"]]]
SLAB_WORDS = ["hundred", "pump", "808"]
STAIN_CORE = (150, 215, 30, 190)                            # y0 y1 x0 x1 at the normalised size: over the left column's second line
SPECKS = [(296, 40, 1), (296, 100, 2), (150, 238, 2), (200, 240, 1), (70, 6, 2), (296, 300, 2), (296, 420, 1), (230, 474, 2)]   # y, x, side

SEGMENT = dict(threshold=-1)                                # Otsu: binarize puts 127 in its place
LAYOUT_MAX_BOXES = 64
_made = {}


def _paste(cover, y, x, bm):
    view = cover[y:y + bm.shape[0], x:x + bm.shape[1]]
    view[:] = np.maximum(view, bm)


def _line(cover, y, x, words, space, limit):
    """pastes the words from column x on, `space` columns between one word's last ink column and the next word's first."""
    for w in words:
        bm = atlas_word(w, 0)
        cols = np.nonzero((bm >= 128).any(axis=0))[0]
        _paste(cover, y, x - int(cols.min()), bm)
        x += int(cols.max()) + 1 - int(cols.min()) + space
    assert x - space <= limit, (words, x - space, limit)
    return x - space


def straight_page():
    """(gray (H1, W1) uint8, red (H1, W1) bool): the normalised page before it is bent, and the pixels of the red stroke."""
    strong, faded = np.zeros((H1, W1), np.uint8), np.zeros((H1, W1), np.uint8)             # ink coverage 0..255
    word, _ = glyph_word("hill", 0, 6)
    _paste(strong, HEADLINE_Y, 20, 255 - word)
    _line(strong, HEADLINE_Y, 20 + word.shape[1] + HEAD_SPACE, ["dump", "hub"], HEAD_SPACE, W1 - 12)
    on_slab = np.zeros((H1, W1), np.uint8)
    _line(on_slab, SLAB[1] + 6, SLAB[0] + 14, SLAB_WORDS, 14, SLAB[2] - 8)
    strong[SLAB[1]:SLAB[3], SLAB[0]:SLAB[2]] = 255 - on_slab[SLAB[1]:SLAB[3], SLAB[0]:SLAB[2]]
    ends = {}
    for c, x0 in enumerate(COLUMNS):
        for ln, words in enumerate(BODY[c]):
            ends[c, ln] = _line(faded if c else strong, BODY_Y + PITCH * ln, x0, words, BODY_SPACE, x0 + COLUMN_W)
    strong[BODY_Y + 23:BODY_Y + 25, COLUMNS[0] - 4:COLUMNS[1] + COLUMN_W] = 255                 # the form rule, across the gutter
    for y, x, s in SPECKS:
        strong[y:y + s, x:x + s] = 255
    gray = PAPER - (strong.astype(np.int64) * (PAPER - INK) + faded.astype(np.int64) * (PAPER - FADED)) // 255
    red = np.zeros((H1, W1), bool)
    y, x1 = BODY_Y + 2 * PITCH + 12, ends[1, 2]
    red[y:y + 3, COLUMNS[1] + 20:x1 - 20] = True                                            # through both words of the right column's last line
    return gray.astype(np.uint8), red


def _bend(img, fill):
    """curled, sheared, turned upside down and doubled."""
    H, W = img.shape
    out = np.full((H, W), fill, img.dtype)
    for x, d in enumerate(sag(np.arange(W), SAG, W).tolist()):
        out[d:, x] = img[:H - d, x]
    out = SK.deskew(out, SHEAR, fill)
    return np.kron(np.ascontiguousarray(out[::-1, ::-1]), np.ones((2, 2), np.uint8))


def _light(H, W):
    """the light on the doubled, turned page as a fraction of 1024: a ramp from 840 at the left to 1024 at the right, times the stain."""
    y0, y1, x0, x1 = STAIN_CORE
    y0, y1, x0, x1 = 2 * (H1 - y1), 2 * (H1 - y0), 2 * (W1 - x1), 2 * (W1 - x0)                # where the half turn and the doubling take it
    y = np.arange(H, dtype=np.int64)[:, None]
    x = np.arange(W, dtype=np.int64)[None, :]
    d = np.minimum(np.maximum(np.maximum(np.maximum(y0 - y, y - (y1 - 1)), 0), np.maximum(np.maximum(x0 - x, x - (x1 - 1)), 0)), STAIN_RAMP)
    stain = PAPER - ((PAPER - STAIN) * (STAIN_RAMP - d)) // STAIN_RAMP
    return ((840 + (184 * x) // (W - 1)) * stain) // PAPER


def planted_photo():
    """(photo (H, W, 3) uint8 RGB, corners: the sheet's four (x, y) TL TR BR BL on it)."""
    if "photo" not in _made:
        gray, red = straight_page()
        page = _bend(gray, PAPER).astype(np.int64)
        mark = _bend(red.astype(np.uint8) * 255, 0) > 0
        Hp, Wp = page.shape
        lit = _light(Hp, Wp)
        r = (page * lit) >> 10
        rgb = np.stack([r, (r * 246) >> 8, (r * 218) >> 8], axis=2)                          # yellowish paper
        rgb[mark] = np.stack([(200 * lit) >> 10, (40 * lit) >> 10, (40 * lit) >> 10], axis=2)[mark]
        H, W = Hp + 60, Wp + 80
        quad = [31, 22, W - 44, 14, W - 25, H - 16, 12, H - 25]
        photo = np.stack([RR.make_photo(rgb[:, :, c].astype(np.uint8), quad, H, W, DESK) for c in range(3)], axis=2)
        _made["photo"] = (np.ascontiguousarray(photo), [tuple(quad[2 * i:2 * i + 2]) for i in range(4)])
    return _made["photo"]


def gray_photo():
    """the photograph as a gray page (the luma of its pixels), for the runs without the colour stage."""
    photo, corners = planted_photo()
    p = photo.astype(np.int64)
    return ((77 * p[:, :, 0] + 150 * p[:, :, 1] + 29 * p[:, :, 2] + 128) >> 8).astype(np.uint8), corners


def options_given():
    """every stage on, every estimate that would cost a sync given by value; True wherever the defaults serve, so that what the stages
    inherit from the segment parameters (the 127 behind binarize, light_text, the paper fill) is part of what is checked."""
    _, corners = planted_photo()
    return dict(colour=dict(drop=1 << HUE_RED, fill=255), rectify=corners, flatten=True, binarize=True, scale=0.5, panels=True, clean=True,
                orient=2, deskew=True, dewarp=True, rules=True, deslant=True, spacing=True)


def options_estimated():
    """the same with the three estimating forms."""
    return dict(options_given(), rectify=True, scale=True, orient=True)
