"""Pages and shapes for the scale tests, shared by test_scale_cpu.py (the restatement alone) and test_scale_gpu.py (the kernels against it):
hand-painted pages with hand-written glyph words, the resize shapes, and a page of atlas words for the motive."""
import numpy as np

import orient_cases as OC
from segment_cases import paint


def squares(sizes, bg=255, fg=0, gap=3):
    """squares of the given sides from left to right, `gap` columns of paper between them and around them."""
    H, W = max(sizes) + 2 * gap, sum(sizes) + gap * (len(sizes) + 1)
    rects, x = [], gap
    for s in sizes:
        rects.append((gap, gap + s, x, x + s))
        x += s + gap
    return paint(H, W, rects, bg=bg, fg=fg)


def case(name, page, want, **params):
    """want: q_2, q_1, q_3, n, components found, the threshold used, the total ink, 0 -- written down from the rectangles, not computed."""
    p = dict(threshold=128)
    p.update(params)
    return dict(name=name, page=page, params=p, want=np.array(want, np.int32))


HAND = [
    case("n0", np.full((9, 11), 255, np.uint8), [0, 0, 0, 0, 0, 128, 0, 0]),
    # 3 rows x 5 columns: a = 3
    case("n1", paint(9, 11, [(2, 5, 3, 8)]), [3, 3, 3, 1, 1, 128, 15, 0]),
    # n = 4: the indices floor(k * 3 / 4) are 0, 1, 2
    case("n4", squares([2, 4, 6, 8]), [4, 2, 6, 4, 4, 128, 4 + 16 + 36 + 64, 0]),
    # n = 5: the indices floor(k * 4 / 4) are 1, 2, 3
    case("n5", squares([8, 2, 10, 4, 6]), [6, 4, 8, 5, 5, 128, 64 + 4 + 100 + 16 + 36, 0]),
    # 2 x 6 has b == max_aspect * a and counts, 2 x 7 does not
    case("aspect_edge", paint(8, 20, [(2, 4, 2, 8), (2, 4, 11, 18)]), [2, 2, 2, 1, 2, 128, 12 + 14, 0], max_aspect=3),
    # the same turned: 6 x 2 and 7 x 2
    case("aspect_edge_tall", paint(20, 8, [(2, 8, 2, 4), (11, 18, 2, 4)]), [2, 2, 2, 1, 2, 128, 12 + 14, 0], max_aspect=3),
    # sides 2, 3, 5, 6 with min_size 3 and max_size 5: 3 and 5 count; n = 2: every index is 0
    case("size_edges", squares([2, 3, 5, 6]), [3, 3, 3, 2, 4, 128, 4 + 9 + 25 + 36, 0], min_size=3, max_size=5),
    # min(w, h): 6 wide x 3 high and 3 wide x 7 high are both 3
    case("min_side", paint(12, 16, [(2, 5, 2, 8), (2, 9, 11, 14)]), [3, 3, 3, 2, 2, 128, 18 + 21, 0]),
    case("light_text", squares([4], bg=0, fg=255), [4, 4, 4, 1, 1, 128, 16, 0], light_text=1),
    # one gray value: Otsu has no threshold, nothing is ink
    case("one_gray", np.full((9, 11), 200, np.uint8), [0, 0, 0, 0, 0, -1, 0, 0], threshold=-1),
    # Otsu on two levels a < b takes a (segment_cases.otsu_two_level)
    case("otsu_two_level", squares([3, 5, 5], bg=200, fg=50), [5, 3, 5, 3, 3, 50, 9 + 25 + 25, 0], threshold=-1),
    # two 2 x 2 squares that touch at a corner: one 4 x 4 box with 8 neighbours, two of 2 x 2 with 4
    case("diagonal_8", paint(8, 8, [(2, 4, 2, 4), (4, 6, 4, 6)]), [4, 4, 4, 1, 1, 128, 8, 0], connectivity=8),
    case("diagonal_4", paint(8, 8, [(2, 4, 2, 4), (4, 6, 4, 6)]), [2, 2, 2, 2, 2, 128, 8, 0], connectivity=4),
    # a component of side 1 is below min_size 2; with min_size 1 it counts
    case("dot_out", squares([1, 3]), [3, 3, 3, 1, 2, 128, 10, 0]),
    case("dot_in", squares([1, 3]), [1, 1, 1, 2, 2, 128, 10, 0], min_size=1),
]

# source (H, W, pitch, offset in bytes) -> (Ho, Wo), output (pitch or None: Wo, offset in bytes)
RESIZE_SHAPES = [
    ((1, 1, 1, 0), (1, 1), (None, 0)),                  # the smallest page
    ((1, 7, 7, 0), (1, 3), (None, 0)),                  # a single row, shrink in x
    ((7, 1, 1, 0), (15, 1), (None, 0)),                 # a single column, grow in y
    ((33, 65, 65, 0), (33, 65), (None, 0)),             # a copy
    ((64, 64, 64, 0), (8, 8), (None, 0)),               # 8x shrink
    ((8, 8, 8, 0), (64, 64), (None, 0)),                # 8x grow
    ((63, 129, 129, 0), (47, 100), (107, 5)),           # ratios in lowest terms on both axes; an unaligned output base and a wider pitch
    ((257, 129, 134, 3), (300, 97), (101, 1)),          # up in y, down in x, misaligned; the same on the output
    ((130, 1100, 1100, 0), (61, 1009), (None, 0)),      # more than one wave chunk per row
    ((2048, 8192, 8192, 0), (256, 1024), (None, 0)),    # bytes 254 and 255 only: the divisor is 2^24, the numerator near its top
    # output rows around one 16-byte store at an unaligned base: a row that is all head, a head and a tail, one and two whole stores
    ((7, 3, 3, 0), (5, 1), (8, 5)),
    ((7, 29, 29, 0), (5, 15), (22, 5)),
    ((7, 16, 16, 0), (5, 16), (23, 5)),
    ((7, 23, 23, 0), (5, 17), (24, 5)),
    ((7, 20, 20, 0), (8, 33), (40, 5)),
]


def resize_source(H, W):
    rng = np.random.default_rng(1000 * H + W)
    if H * W >= 1 << 24:
        return rng.integers(254, 256, (H, W), dtype=np.uint8)
    return rng.integers(0, 256, (H, W), dtype=np.uint8)


# ---- the motive: a page of atlas words whose spaces the default segment parameters separate at the atlas size ------------------------------
WORD_GAP = 18                                   # columns of paper between words: the narrow end of tools/segment_prof.py's 18..30
MOTIVE_COUNTS = (24, 9, 24)                     # words found at the native size, on the page shrunk 2x, and after estimate + plan + resize


def word_page(face=0, gap=WORD_GAP, n_lines=4, per_line=6):
    """(page, words): dark text on white paper, n_lines lines of per_line words of orient_cases.TEXT from one face of the atlas at its native
    size, `gap` columns between the advance boxes of neighbouring words, a margin of one glyph height all round."""
    glyphs, adv = OC.shrunk(face, 1)
    gh, gw = glyphs.shape[1:]
    ids = lambda w: [int(c) if c.isdigit() else 10 + ord(c) - ord("a") for c in w]
    rows = [OC.TEXT[i * per_line:(i + 1) * per_line] for i in range(n_lines)]
    width = max(sum(int(adv[i]) for w in r for i in ids(w)) + gap * (len(r) - 1) for r in rows)
    pitch, m = gh + gh // 2, gh
    H, W = 2 * m + pitch * (n_lines - 1) + gh, 2 * m + width + gw
    cover = np.zeros((H, W), np.uint8)
    for li, r in enumerate(rows):
        y, x = m + li * pitch, m
        for w in r:
            for i in ids(w):
                box = cover[y:y + gh, x:x + gw]
                np.maximum(box, glyphs[i], out=box)
                x += int(adv[i])
            x += gap
    return (255 - cover).astype(np.uint8), n_lines * per_line


_text = {}


def text_page(face, scale):
    """orient_cases.text_page, rendered once."""
    if (face, scale) not in _text:
        _text[(face, scale)] = OC.text_page(face, scale)
    return _text[(face, scale)]


ATLAS_MEDIAN = {(1, 0): 15, (1, 1): 16, (1, 2): 15, (2, 0): 8, (2, 1): 8, (2, 2): 7}       # (scale, face): q_2 at threshold 128
