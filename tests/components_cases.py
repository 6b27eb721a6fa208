"""Hand-painted pages with hand answers for aocr_label_components and aocr_clean_page, shared by test_components_cpu.py (the restatement)
and test_components_gpu.py (the kernels); the page the calls exist for (two lines of three words with dust, a margin rule and an underline);
and the pages whose shape follows the kernels' tile, as functions of the tile size.  Every expected label map, component list and count
below was written down from the painting, not computed.  Component rows are x0 y0 x1 y1 label area."""
import numpy as np

from segment_cases import paint

X = -1                                                                         # paper, in the label maps below


def _page(rows, ink=0, paper=255):
    """a page from strings: '#' is ink."""
    return np.array([[ink if c == "#" else paper for c in r] for r in rows], np.uint8)


def case(name, page, connectivity, labels, comps, info, threshold=128, light_text=0):
    return dict(name=name, page=page, threshold=threshold, light_text=light_text, connectivity=connectivity,
                labels=np.array(labels, np.int32).reshape(page.shape), comps=np.array(comps, np.int32).reshape(-1, 6), info=np.array(info, np.int32))


_DIAG = _page(["#...",
               ".#..",
               "..##"])
_U = _page(["#.#",
            "#.#",
            "###"])
_RING = _page(["####",
               "#..#",
               "#.##",
               "####"])
_TWO_LEVEL = np.array([[50, 200, 50], [200, 200, 200], [50, 50, 200]], np.uint8)

LABEL_CASES = [
    # a diagonal chain is one component at 8-connectivity and three at 4 (the last two pixels touch by an edge)
    case("diag_8", _DIAG, 8, [[0, X, X, X], [X, 0, X, X], [X, X, 0, 0]], [[0, 0, 4, 3, 0, 4]], [128, 4, 1, 0]),
    case("diag_4", _DIAG, 4, [[0, X, X, X], [X, 5, X, X], [X, X, 10, 10]], [[0, 0, 1, 1, 0, 1], [1, 1, 2, 2, 5, 1], [2, 2, 4, 3, 10, 2]],
         [128, 4, 3, 0]),
    # the right arm starts a component of its own (pixel 2) that the bottom row joins to the left arm: everything is label 0
    case("u", _U, 4, [[0, X, 0], [0, X, 0], [0, 0, 0]], [[0, 0, 3, 3, 0, 7]], [128, 7, 1, 0]),
    # a ring: the hole is paper, the box is the whole page
    case("ring", _RING, 4, [[0, 0, 0, 0], [0, X, X, 0], [0, X, 0, 0], [0, 0, 0, 0]], [[0, 0, 4, 4, 0, 13]], [128, 13, 1, 0]),
    # components come out in the raster order of their first pixels: (0,3) = 3 before (1,0) = 5
    case("order", _page(["...##", "#....", "#..#."]), 4, [[X, X, X, 3, 3], [5, X, X, X, X], [5, X, X, 13, X]],
         [[3, 0, 5, 1, 3, 2], [0, 1, 1, 3, 5, 2], [3, 2, 4, 3, 13, 1]], [128, 5, 3, 0]),
    case("light_text", _page(["##.", "...", ".#."], ink=255, paper=0), 8, [[0, 0, X], [X, X, X], [X, 7, X]],
         [[0, 0, 2, 1, 0, 2], [1, 2, 2, 3, 7, 1]], [128, 3, 2, 0], light_text=1),
    # Otsu on two levels 50 < 200: the threshold is 50 (segment_cases: otsu_two_level); (0,0) and (0,2) are apart, the bottom pair is one
    case("otsu", _TWO_LEVEL, 8, [[0, X, 2], [X, X, X], [6, 6, X]], [[0, 0, 1, 1, 0, 1], [2, 0, 3, 1, 2, 1], [0, 2, 2, 3, 6, 2]], [50, 4, 3, 0],
         threshold=-1),
    # one gray value: no threshold, nothing is ink
    case("constant", np.full((3, 4), 90, np.uint8), 8, [[X] * 4] * 3, [], [-1, 0, 0, 0], threshold=-1),
    case("all_ink", np.zeros((3, 5), np.uint8), 4, [[0] * 5] * 3, [[0, 0, 5, 3, 0, 15]], [128, 15, 1, 0]),
    case("one_pixel", np.zeros((1, 1), np.uint8), 8, [[0]], [[0, 0, 1, 1, 0, 1]], [128, 1, 1, 0]),
]


# ---- aocr_clean_page: a 12 x 20 page with one component per rule of the call --------------------------------------------------------------------
#   A  a 3 x 3 block (area 9)          rows 1..3, columns 1..3     stays under every setting below
#   B  a 1 x 5 dash (area 5, w 5)      row 1, columns 8..12
#   C  a 6 x 1 bar (area 6, h 6)       rows 5..10, column 16
#   D  one pixel                       row 10, column 2
#   E  a 2 x 2 block (area 4)          rows 7..8, columns 6..7
_CLEAN_RECTS = dict(A=(1, 4, 1, 4), B=(1, 2, 8, 13), C=(5, 11, 16, 17), D=(10, 11, 2, 3), E=(7, 9, 6, 8))
CLEAN_PAGE = paint(12, 20, list(_CLEAN_RECTS.values()))
CLEAN_INK = 9 + 5 + 6 + 1 + 4


def clean_case(name, gone, specks, rules, removed, page=None, light_text=0, **kw):
    """gone: the letters of the components that are painted over."""
    p = dict(threshold=128, light_text=light_text, connectivity=8, min_area=1, max_w=0, max_h=0)
    p.update(kw)
    src = CLEAN_PAGE if page is None else page
    fg, bg = (255, 0) if light_text else (0, 255)
    if light_text:
        src = (255 - src).astype(np.uint8)
    out = src.copy()
    for g in gone:
        y0, y1, x0, x1 = _CLEAN_RECTS[g]
        out[y0:y1, x0:x1] = bg
    return dict(name=name, page=src, params=p, out=out, counts=np.array([5, specks, rules, 128, CLEAN_INK, removed, 0, 0], np.int32))


CLEAN_CASES = [
    clean_case("nothing", "", 0, 0, 0),                                          # min_area 1 and both limits off: bit for bit
    clean_case("min_area_at_boundary", "D", 1, 0, 1, min_area=4),                # E has area 4 = min_area: it stays
    clean_case("min_area_above", "DE", 2, 0, 5, min_area=5),                     # B has area 5 = min_area: it stays
    clean_case("max_w_at_boundary", "", 0, 0, 0, max_w=5),                       # B is 5 wide = max_w: it stays
    clean_case("max_w_below", "B", 0, 1, 5, max_w=4),
    clean_case("max_h_at_boundary", "", 0, 0, 0, max_h=6),                       # C is 6 high = max_h: it stays
    clean_case("max_h_below", "C", 0, 1, 6, max_h=5),
    clean_case("speck_before_rule", "BCDE", 3, 1, 16, min_area=6, max_w=4, max_h=5),   # B (area 5 < 6) counts as a speck though it is too wide; C as a rule
    clean_case("everything", "ABCDE", 5, 0, 25, min_area=10),
    clean_case("light_text", "DE", 2, 0, 5, light_text=1, min_area=5),           # removed pixels become 0
]


# ---- the page the calls exist for: 60 x 120, two lines of three 22 x 12 words -----------------------------------------------------------------
MOTIVE_SEG = dict(threshold=128, light_text=0, min_row_ink=1, merge_gap=2, min_line_h=8, word_gap=8, min_word_w=4, pad_x=0, pad_y=0)
MOTIVE_CLEAN = dict(threshold=128, light_text=0, connectivity=8, min_area=6, max_w=40, max_h=20)
_WORD_X = (10, 44, 78)                                                         # 22 wide, 12 columns apart
_LINE_Y = (8, 34)                                                              # 12 high
MOTIVE_BOXES = [[x, y, x + 22, y + 12, l, 22 * 12] for l, y in enumerate(_LINE_Y) for x in _WORD_X]
MOTIVE_SPECKS = ((12, 37), (14, 38), (26, 60), (28, 90))                       # (row, column): two in the gap of words 1 and 2 of line 0, two between the lines
MOTIVE_VRULE = (2, 58, 4)                                                      # rows [2, 58) of column 4
MOTIVE_HRULE = (22, 6, 112)                                                    # row 22, columns [6, 112)


def motive_page(specks=False, vrule=False, hrule=False):
    page = paint(60, 120, [(y, y + 12, x, x + 22) for y in _LINE_Y for x in _WORD_X])
    if specks:
        for y, x in MOTIVE_SPECKS:
            page[y, x] = 0
    if vrule:
        page[MOTIVE_VRULE[0]:MOTIVE_VRULE[1], MOTIVE_VRULE[2]] = 0
    if hrule:
        page[MOTIVE_HRULE[0], MOTIVE_HRULE[1]:MOTIVE_HRULE[2]] = 0
    return page


# ---- pages whose shape follows the tile of csrc/components.hip (TH rows x TW columns) ---------------------------------------------------------
def checkerboard(H, W):
    """ink where x + y is even: every ink pixel is its own component at 4-connectivity, the page is one component at 8."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy + xx) % 2 == 0, 0, 255).astype(np.uint8)


def corner_diagonals(TH, TW):
    """2 TH x 2 TW: two pixels that touch only across the corner where four tiles meet, on the main diagonal; and, far from them, two on the
    anti-diagonal of the same kind of corner would need a second corner, so the page is 2 TH x 3 TW with the second pair at the second corner."""
    page = np.full((2 * TH, 3 * TW), 255, np.uint8)
    page[TH - 1, TW - 1] = page[TH, TW] = 0                                    # main diagonal, corner (TH, TW)
    page[TH - 1, 2 * TW] = page[TH, 2 * TW - 1] = 0                            # anti-diagonal, corner (TH, 2 TW)
    return page


def border_crossers(TH, TW):
    """2 TH + 3 x 2 TW + 5: a vertical bar over rows TH-1, TH; a horizontal bar over columns TW-1, TW; an L that crosses both borders."""
    page = np.full((2 * TH + 3, 2 * TW + 5), 255, np.uint8)
    page[TH - 1:TH + 1, 3] = 0
    page[2, TW - 1:TW + 1] = 0
    page[TH - 3:TH + 4, TW + 7] = 0
    page[TH + 3, TW - 6:TW + 8] = 0
    return page


def u_shape(TH, TW):
    """2 TH x 2 TW: two arms that start in the two upper tiles and meet only in a bar along the bottom row, inside the lower tiles.  The
    right arm's pixels can reach the smallest index (the left arm's top) only through that bar."""
    page = np.full((2 * TH, 2 * TW), 255, np.uint8)
    page[1:, 2] = 0
    page[3:, TW + 5] = 0
    page[2 * TH - 1, 2:TW + 6] = 0
    return page


def serpentine(TH, TW, ty=3, tx=3):
    """ty TH x tx TW + 1: a one-pixel line that runs right along row 0, down two rows at the right edge, left along row 2, down at the left
    edge, and so on to the bottom: every second row is ink from edge to edge, the turns alternate sides.  One component at either connectivity,
    and the longest chain of parents a page of this size can make."""
    H, W = ty * TH, tx * TW + 1
    page = np.full((H, W), 255, np.uint8)
    for k, y in enumerate(range(0, H, 2)):
        page[y, :] = 0
        if y + 1 < H and y + 2 < H:
            page[y + 1, W - 1 if k % 2 == 0 else 0] = 0
    return page


def framed_text(TH, TW):
    """a frame one pixel wide around a (2 TH + 5) x (2 TW + 9) page with words inside that do not touch it."""
    H, W = 2 * TH + 5, 2 * TW + 9
    page = paint(H, W, [(y, y + 5, x, x + 9) for y in range(3, H - 8, 8) for x in range(3, W - 12, 13)])
    page[0, :] = page[H - 1, :] = 0
    page[:, 0] = page[:, W - 1] = 0
    return page
