"""Hand-painted pages with hand answers for aocr_ink_integral + aocr_layout_blocks, shared by test_layout_cpu.py (the restatement) and
test_layout_gpu.py (the kernels), and the seeded two-column page both use.  Every expected block list below was written down from the
rectangles, not computed: block rows are x0 y0 x1 y1 depth ink; counts are written, levels, dropped by size, overflow; info is threshold,
total ink, 0, 0."""
import numpy as np

from segment_cases import paint
from skew_cases import text_page

BASE = dict(min_ink=1, gap_x=4, gap_y=4, max_depth=8, min_block_w=1, min_block_h=1, min_block_ink=1)


def case(name, page, blocks, counts, info, threshold=128, light_text=0, max_blocks=16, **kw):
    p = dict(BASE)
    p.update(kw)
    return dict(name=name, page=page, threshold=threshold, light_text=light_text, max_blocks=max_blocks, params=p,
                blocks=np.array(blocks, np.int32).reshape(-1, 6), counts=np.array(counts, np.int32), info=np.array(info, np.int32))


_GRID = paint(24, 24, [(2, 8, 2, 8), (2, 8, 14, 20), (14, 20, 2, 8), (14, 20, 14, 20)])
# two 8 x 16 columns; the gutter is columns 10..17 (8 wide) with a speck in column 14: 4 clear columns to its left, 3 to its right
_SPECK_WIDE = paint(20, 30, [(2, 18, 2, 10), (2, 18, 18, 26), (9, 10, 14, 15)])
# the gutter is columns 10..16 (7 wide) with a speck in column 13: 3 clear columns on either side
_SPECK_MID = paint(20, 30, [(2, 18, 2, 10), (2, 18, 17, 25), (9, 10, 13, 14)])
# a 6 x 6 square, and 4 columns to its right one column with two pixels on different rows
_LONE = paint(12, 20, [(2, 8, 2, 8), (3, 4, 12, 13), (6, 7, 12, 13)])
# 10 x 10 (ink 100), 2 wide x 10 high (ink 20), 10 wide x 2 high (ink 20), 3 x 3 (ink 9), 6 clear columns between neighbours
_SIZES = paint(20, 50, [(2, 12, 2, 12), (2, 12, 18, 20), (2, 4, 26, 36), (2, 5, 42, 45)])
_BIG, _NARROW, _SHORT, _SPARSE = [2, 2, 12, 12, 1, 100], [18, 2, 20, 12, 1, 20], [26, 2, 36, 4, 1, 20], [42, 2, 45, 5, 1, 9]

CASES = [
    case("empty", paint(10, 12, []), [], [0, 0, 0, 0], [128, 0, 0, 0]),
    # one gray value: Otsu has no threshold, nothing is ink
    case("constant_otsu", np.full((9, 11), 200, np.uint8), [], [0, 0, 0, 0], [-1, 0, 0, 0], threshold=-1),
    case("one_rect", paint(12, 16, [(3, 8, 4, 11)]), [[4, 3, 11, 8, 0, 35]], [1, 0, 0, 0], [128, 35, 0, 0]),
    case("all_four_edges", paint(6, 7, [(0, 6, 0, 7)]), [[0, 0, 7, 6, 0, 42]], [1, 0, 0, 0], [128, 42, 0, 0]),
    # columns 4, 5, 6 clear: gap_x - 1, one block; columns 4..7 clear: gap_x, two
    case("gap_x_minus_1", paint(8, 12, [(2, 6, 1, 4), (2, 6, 7, 10)]), [[1, 2, 10, 6, 0, 24]], [1, 0, 0, 0], [128, 24, 0, 0]),
    case("gap_x", paint(8, 12, [(2, 6, 1, 4), (2, 6, 8, 11)]), [[1, 2, 4, 6, 1, 12], [8, 2, 11, 6, 1, 12]], [2, 1, 0, 0], [128, 24, 0, 0]),
    # rows 3, 4, 5 clear: gap_y - 1, one block; rows 3..6 clear: gap_y, two
    case("gap_y_minus_1", paint(11, 9, [(1, 3, 2, 7), (6, 9, 2, 7)]), [[2, 1, 7, 9, 0, 25]], [1, 0, 0, 0], [128, 25, 0, 0]),
    case("gap_y", paint(12, 9, [(1, 3, 2, 7), (7, 10, 2, 7)]), [[2, 1, 7, 3, 1, 10], [2, 7, 7, 10, 1, 15]], [2, 1, 0, 0], [128, 25, 0, 0]),
    # the headline covers the gutter's columns: level 0 cuts rows (headline | body), level 1 cuts the body's columns; every child is tightened
    case("headline_two_columns", paint(30, 40, [(2, 5, 3, 37), (10, 26, 3, 17), (12, 28, 23, 37)]),
         [[3, 2, 37, 5, 1, 102], [3, 10, 17, 26, 2, 224], [23, 12, 37, 28, 2, 224]], [3, 2, 0, 0], [128, 550, 0, 0]),
    # columns first: top left, bottom left, top right, bottom right
    case("grid_column_major", _GRID, [[2, 2, 8, 8, 2, 36], [2, 14, 8, 20, 2, 36], [14, 2, 20, 8, 2, 36], [14, 14, 20, 20, 2, 36]],
         [4, 2, 0, 0], [128, 144, 0, 0]),
    # min_ink 1: the speck is an occupied column 3 < gap_x columns from the right column: it joins it, and the block starts at the speck
    case("speck_widens_a_block", _SPECK_WIDE, [[2, 2, 10, 18, 1, 128], [14, 2, 26, 18, 1, 129]], [2, 1, 0, 0], [128, 257, 0, 0]),
    # min_ink 1: the speck halves the gutter into two gaps of 3 < gap_x: no column cut, and every row is occupied: one block
    case("speck_blocks_the_gutter", _SPECK_MID, [[2, 2, 25, 18, 0, 257]], [1, 0, 0, 0], [128, 257, 0, 0]),
    # min_ink 2: a column with one pixel is not occupied
    case("speck_ignored_wide", _SPECK_WIDE, [[2, 2, 10, 18, 1, 128], [18, 2, 26, 18, 1, 128]], [2, 1, 0, 0], [128, 257, 0, 0], min_ink=2),
    case("speck_ignored_mid", _SPECK_MID, [[2, 2, 10, 18, 1, 128], [17, 2, 25, 18, 1, 128]], [2, 1, 0, 0], [128, 257, 0, 0], min_ink=2),
    # min_ink 2: column 12 holds two pixels and is a piece of its own, but none of its rows holds two: the child is empty and dropped;
    # the level still cut something and was kept
    case("empty_child_dropped", _LONE, [[2, 2, 8, 8, 1, 36]], [1, 1, 0, 0], [128, 38, 0, 0], min_ink=2),
    case("max_depth_1", _GRID, [[2, 2, 8, 20, 1, 72], [14, 2, 20, 20, 1, 72]], [2, 1, 0, 0], [128, 144, 0, 0], max_depth=1),
    # three pieces do not fit max_blocks 2: the level is discarded, the list stays [the tightened page], the flag is set
    case("overflow", paint(10, 30, [(2, 6, 1, 5), (2, 6, 11, 15), (2, 6, 21, 25)]), [[1, 2, 25, 6, 0, 48]], [1, 0, 0, 1], [128, 48, 0, 0],
         max_blocks=2),
    case("exactly_max_blocks", paint(10, 30, [(2, 6, 1, 5), (2, 6, 11, 15), (2, 6, 21, 25)]),
         [[1, 2, 5, 6, 1, 16], [11, 2, 15, 6, 1, 16], [21, 2, 25, 6, 1, 16]], [3, 1, 0, 0], [128, 48, 0, 0], max_blocks=3),
    case("min_block_w", _SIZES, [_BIG, _SHORT, _SPARSE], [3, 1, 1, 0], [128, 149, 0, 0], min_block_w=3),
    case("min_block_h", _SIZES, [_BIG, _NARROW, _SPARSE], [3, 1, 1, 0], [128, 149, 0, 0], min_block_h=3),
    case("min_block_ink", _SIZES, [_BIG, _NARROW, _SHORT], [3, 1, 1, 0], [128, 149, 0, 0], min_block_ink=10),
    case("min_block_all", _SIZES, [_BIG], [1, 1, 3, 0], [128, 149, 0, 0], min_block_w=3, min_block_h=3, min_block_ink=10),
    case("light_text", paint(12, 16, [(3, 8, 4, 11)], bg=0, fg=255), [[4, 3, 11, 8, 0, 35]], [1, 0, 0, 0], [128, 35, 0, 0], light_text=1),
]


# ---- the two-column page: 900 x 1000, dark text ------------------------------------------------------------------------------------------
TWO_COL_SHAPE = (900, 1000)
TWO_COL = dict(gap_x=24, gap_y=30)              # threshold 128; the rest: layout_ref.DEFAULTS
GUTTER = (480, 530)                             # columns; the speck sits at (row 400, column 505): 25 and 24 clear columns around it
SPECK = (400, 505)
# (name, y0, y1, x0, x1) of the painted text areas: the headline, then per column a top and a bottom paragraph 40 rows apart
# (heights are 34 k + 20: whole lines)
AREAS = [("headline", 30, 60, 150, 834), ("left_top", 100, 392, 40, 480), ("left_bottom", 432, 826, 40, 480),
         ("right_top", 110, 538, 530, 970), ("right_bottom", 578, 836, 530, 970)]
_two_col = {}


def two_column_page():
    """computed once; the caller must not write to it.  Lines are 20 rows high every 34 (14 clear rows < gap_y), words 30..120 columns with
    gaps of 14..25; the right column starts 10 rows lower than the left, so the bands of the two columns overlap on the whole page."""
    if "page" not in _two_col:
        H, W = TWO_COL_SHAPE
        page = np.full((H, W), 255, np.uint8)
        for i, (name, y0, y1, x0, x1) in enumerate(AREAS):
            if name == "headline":                          # one line of 84-column words 16 columns apart: no word gap reaches gap_x
                rng = np.random.default_rng(9001000)
                for x in range(x0, x1, 100):
                    page[y0:y1, x:x + 84] = np.where(rng.random((y1 - y0, 84)) < 0.45, 0, 255)
            else:
                page[y0:y1, x0:x1] = text_page(y1 - y0, x1 - x0, 9001000 + i, margin=0)
        page[SPECK] = 0
        page.setflags(write=False)
        _two_col["page"] = page
    return _two_col["page"]
