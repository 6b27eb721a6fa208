"""Hand-drawn pages with hand answers for aocr_remove_rules, the seeded pages and the form page of the motive, shared by test_rules_cpu.py (the
restatements) and test_rules_gpu.py (the kernels).  Every expected page below was drawn by hand, not computed: '#' is ink, '.' paper."""
import numpy as np

from segment_cases import seeded_page
from spacing_atlas import atlas_word

BASE = dict(threshold=128, light_text=0, axes=3, min_len=5, max_thick=2, edge=0)


def art(rows, light=False):
    ink = np.array([[ch == "#" for ch in r] for r in rows])
    assert ink.ndim == 2
    return np.where(ink, 255 if light else 0, 0 if light else 255).astype(np.uint8)


def case(name, page, out, counts, light=False, **kw):
    p = dict(BASE)
    p.update(kw)
    p["light_text"] = int(light)
    page, out = (v if isinstance(v, np.ndarray) else art(v, light) for v in (page, out))
    assert page.shape == out.shape
    return dict(name=name, page=page, out=out, params=p, counts=np.array(counts, np.int32))


_LEN = ["........",
        ".####...",            # L - 1 = 4: stays
        "........",
        ".#####..",            # L = 5: goes
        "........"]
_LEN_OUT = ["........",
            ".####...",
            "........",
            "........",
            "........"]
_THICK = [".......",
          "#####..",           # T = 2 rows thick: goes
          "#####..",
          ".......",
          "#####..",           # T + 1 = 3 rows thick: stays, every pixel a candidate kept
          "#####..",
          "#####..",
          "......."]
_THICK_OUT = ["......."] * 4 + ["#####.."] * 3 + ["......."]
_RAGGED = [".......",
           "..##...",           # two pixels on top of the rule: their row run is no candidate
           "######.",
           "......."]
_RAGGED_E0 = [".......",
              "..##...",
              ".......",
              "......."]
_BLANK4 = ["......."] * 4
_STEM = ["...#....",
         "...#....",
         "########",            # the underline; the stem's column run is 4 > T
         "...#...."]
_STEM_OUT = ["...#....",
             "...#....",
             "...#....",
             "...#...."]
_O = ["..####...",
      "..#..#...",
      "..#..#...",
      "..####...",             # the bottom of the o sits on the rule
      "#########"]
_O_E0 = ["..####...",
         "..#..#...",
         "..#..#...",
         "..####...",             # e = 0: the bottom stroke stays, the rule under it goes (a column run of 2 = T)
         "..#..#..."]             # under the stems the column run is longer than T: the rule's pixels stay there
_O_E1 = ["..####...",
         "..#..#...",
         "..#..#...",
         "..#..#...",            # e = 1 takes the bottom stroke between the stems as well: one row, the edge
         "..#..#..."]
_PLUS = ["...#...",
         "...#...",
         "...#...",
         "#######",
         "...#...",
         "...#...",
         "...#..."]
_PLUS_H = ["...#..."] * 7       # axes = 1: the row goes, the column stays whole
_PLUS_V = ["......."] * 3 + ["#######"] + ["......."] * 3
_BLOCK = ["......",
          ".####.",             # 4 wide (< L), 7 high: too thick for a vertical rule, too short for a horizontal one
          ".####.",
          ".####.",
          ".####.",
          ".####.",
          ".####.",
          ".####."]
_FRAME = ["#####",
          "#...#",
          "#...#",
          "#...#",
          "#####"]

CASES = [
    case("run_of_L", _LEN, _LEN_OUT, [128, 9, 5, 0, 5, 0, 0, 0]),
    case("thickness_T", _THICK, _THICK_OUT, [128, 25, 10, 0, 10, 0, 15, 0]),
    case("edge_0_keeps_ragged", _RAGGED, _RAGGED_E0, [128, 8, 6, 0, 6, 0, 0, 0]),
    case("edge_1_takes_ragged", _RAGGED, _BLANK4, [128, 8, 8, 0, 8, 0, 0, 0], edge=1),
    case("stem_through_underline", _STEM, _STEM_OUT, [128, 11, 7, 0, 7, 0, 1, 0], edge=1),
    case("o_on_rule_edge_0", _O, _O_E0, [128, 21, 7, 0, 7, 0, 2, 0], min_len=9),
    case("o_on_rule_edge_1", _O, _O_E1, [128, 21, 9, 0, 9, 0, 2, 0], min_len=9, edge=1),
    case("crossing", _PLUS, ["......."] * 7, [128, 13, 13, 1, 6, 6, 0, 0], max_thick=1),
    case("axes_1", _PLUS, _PLUS_H, [128, 13, 6, 0, 6, 0, 1, 0], max_thick=1, axes=1),
    case("axes_2", _PLUS, _PLUS_V, [128, 13, 6, 0, 0, 6, 1, 0], max_thick=1, axes=2),
    case("filled_block", _BLOCK, _BLOCK, [128, 28, 0, 0, 0, 0, 28, 0]),
    case("page_edges", _FRAME, ["....."] * 5, [128, 16, 16, 4, 6, 6, 0, 0], max_thick=1),
    case("light_text", _LEN, _LEN_OUT, [128, 9, 5, 0, 5, 0, 0, 0], light=True),
    case("one_gray", np.full((6, 9), 93, np.uint8), np.full((6, 9), 93, np.uint8), [-1, 0, 0, 0, 0, 0, 0, 0], threshold=-1),
    case("nothing", _LEN[:3], _LEN[:3], [128, 4, 0, 0, 0, 0, 0, 0]),
]

# ---- seeded pages: segment_cases.seeded_page with rules, strokes across them and ragged pixels on them ---------------------------------------
SEEDED = dict(min_len=4, max_thick=2, edge=1)              # small, so that the text rectangles themselves are rules, blocks and strokes
# H, W, pitch, base offset in bytes, seed: the shapes of segment_cases.SEEDED_SHAPES that can hold a crossing (1 x 1 has its own test)
SEEDED_SHAPES = [(9, 37, 37, 0, 9037), (40, 100, 112, 0, 3), (70, 257, 257, 3, 70257), (300, 700, 704, 0, 300700)]


def ruled_page(H, W, seed, light=False):
    """seeded_page plus, from the seed: a horizontal and a vertical rule of 1 or 2 pixels across the page, strokes of 3 pixels across both,
    and single pixels on their edges.  Ink values are drawn from 0..80 like the text's."""
    page = seeded_page(H, W, seed)
    rng = np.random.default_rng(seed + 1)
    y, x = int(rng.integers(1, H - 2)), int(rng.integers(1, W - 2))
    ty, tx = int(rng.integers(1, 3)), int(rng.integers(1, 3))

    def ink(shape):
        return rng.integers(0, 81, shape).astype(np.uint8)
    page[max(y - 1, 0):y + ty + 1, :] = 255                                       # a clear row above and below the rule
    page[:, max(x - 1, 0):x + tx + 1] = 255
    page[y:y + ty, :] = ink((ty, W))
    page[:, x:x + tx] = ink((H, tx))
    for _ in range(max(2, W // 40)):                                              # strokes across the horizontal rule, 3 wide, and ragged pixels
        sx = int(rng.integers(0, W - 3))
        page[max(y - 1, 0):y + ty + 1, sx:sx + 3] = ink((min(y, 1) + ty + 1 - max(y + ty + 1 - H, 0), 3))
        page[max(y - 1, 0), int(rng.integers(0, W))] = 40
    for _ in range(max(2, H // 40)):
        sy = int(rng.integers(0, H - 3))
        page[sy:sy + 3, max(x - 1, 0):x + tx + 1] = ink((3, min(x, 1) + tx + 1 - max(x + tx + 1 - W, 0)))
        page[int(rng.integers(0, H)), max(x - 1, 0)] = 40
    return (255 - page).astype(np.uint8) if light else page


# ---- the motive: a form ------------------------------------------------------------------------------------------------------------------------
MOTIVE_SEG = dict(threshold=128, light_text=0, min_row_ink=1, merge_gap=2, min_line_h=8, word_gap=12, min_word_w=4, pad_x=2, pad_y=2)
MOTIVE_RULES = dict(threshold=128, light_text=0, axes=3, min_len=40, max_thick=2, edge=1)
# y, x, word.  Glyphs are 32 rows: stems from row 0, the baseline's last row is 24, descenders reach row 31; strokes are 3 pixels
MOTIVE_WORDS = [(4, 16, "pump"), (4, 150, "min"), (52, 16, "hill"), (52, 110, "min"), (106, 20, "42"), (106, 147, "hill"), (152, 20, "page"), (152, 160, "x")]
# y0, y1, x0, x1 of every rule, 2 pixels thick (= max_thick):
#   the underline runs through the descenders of "pump" (the hook of a j would stand on it), two rows below the bottoms of u and m, and on under "min";
#   the form line lies in the last two rows of the stems of "hill" and "min";
#   the grid is a frame with one inner vertical and one inner horizontal rule; the stem of the h of the second "hill" stands on the inner
#   vertical rule (its 3 columns cover the rule's 2).
MOTIVE_RULE_RECTS = [(30, 32, 8, 230), (75, 77, 8, 230),
                     (100, 102, 8, 290), (144, 146, 8, 290), (190, 192, 8, 290), (100, 192, 8, 10), (100, 192, 150, 152), (100, 192, 288, 290)]
# What had to be avoided for the page without rules and the page with its rules removed to be equal pixel for pixel: a stroke that meets a
# rule at a slant (the descender of y) or side on (the bar of the 4 against a vertical rule) makes the rule's run across longer than T right
# next to it, and those pixels of the rule stay as a stub on the letter; a letter whose bottom is a curve or a bar (u, e, a) lying on the
# rule is thin there and goes with it.  So: only upright stems cross or stand in the rules, and every other glyph keeps a clear row.


def motive_page(rules=True):
    page = np.full((200, 300), 255, np.uint8)
    for y, x, w in MOTIVE_WORDS:
        bm = atlas_word(w, 0)
        view = page[y:y + bm.shape[0], x:x + bm.shape[1]]
        view[:] = np.minimum(view, 255 - bm)
    if rules:
        for y0, y1, x0, x1 in MOTIVE_RULE_RECTS:
            page[y0:y1, x0:x1] = 0
    return page
