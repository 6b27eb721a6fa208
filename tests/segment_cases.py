"""Hand-painted pages with hand answers for aocr_segment_page, shared by test_segment_cpu.py (the restatement) and test_segment_gpu.py (the
kernels).  Every expected box list below was written down from the rectangles, not computed: box rows are x0 y0 x1 y1 line ink."""
import numpy as np

BASE = dict(threshold=128, light_text=0, min_row_ink=1, merge_gap=2, min_line_h=3, word_gap=4, min_word_w=2, pad_x=0, pad_y=0)


def paint(H, W, rects, bg=255, fg=0):
    """rects: (y0, y1, x0, x1) half-open, filled with fg on a bg page."""
    page = np.full((H, W), bg, np.uint8)
    for y0, y1, x0, x1 in rects:
        page[y0:y1, x0:x1] = fg
    return page


def case(name, page, boxes, counts, **kw):
    p = dict(BASE)
    p.update(kw)
    return dict(name=name, page=page, params=p, boxes=np.array(boxes, np.int32).reshape(-1, 6), counts=np.array(counts, np.int32))


_WORDS = paint(8, 20, [(2, 6, 1, 4), (2, 6, 7, 10), (2, 6, 14, 17)])          # column gaps of 3 = word_gap-1 and 4 = word_gap
_TIE = np.full((6, 8), 20, np.uint8)                                           # 12 pixels of 10, 24 of 20, 12 of 30: t = 10 and t = 20 tie
_TIE[0:3, 0:4] = 10
_TIE[3:6, 4:8] = 30

CASES = [
    # a run at row 0 and one ending at row H-1
    case("edge_rows", paint(20, 30, [(0, 3, 5, 10), (17, 20, 0, 4)]), [[5, 0, 10, 3, 0, 15], [0, 17, 4, 20, 1, 12]], [2, 2, 128, 0]),
    # runs merge_gap apart are one band, merge_gap+1 apart two
    case("merge_gap", paint(20, 12, [(2, 5, 4, 9), (7, 10, 4, 9), (13, 16, 4, 9)]), [[4, 2, 9, 10, 0, 30], [4, 13, 9, 16, 1, 15]], [2, 2, 128, 0]),
    # three runs of height 2, each merge_gap from the next: one band (and it is the merged height that min_line_h sees)
    case("chain", paint(14, 8, [(1, 3, 2, 6), (5, 7, 2, 6), (9, 11, 2, 6)]), [[2, 1, 6, 11, 0, 24]], [1, 1, 128, 0]),
    # merge_gap = 0 never merges: runs one row apart stay two bands
    case("merge_gap_0", paint(12, 8, [(1, 4, 2, 6), (5, 8, 2, 6)]), [[2, 1, 6, 4, 0, 12], [2, 5, 6, 8, 1, 12]], [2, 2, 128, 0], merge_gap=0),
    # a band of height min_line_h-1 is dropped, one of height min_line_h kept (and becomes line 0)
    case("min_line_h", paint(14, 10, [(1, 3, 3, 8), (8, 11, 3, 8)]), [[3, 8, 8, 11, 0, 15]], [1, 1, 128, 0]),
    # 3 empty columns: one word; 4: two
    case("word_gap", _WORDS, [[1, 2, 10, 6, 0, 24], [14, 2, 17, 6, 0, 12]], [2, 1, 128, 0]),
    case("word_gap_0", _WORDS, [[1, 2, 17, 6, 0, 36]], [1, 1, 128, 0], word_gap=0),
    # a word of width min_word_w-1 is dropped
    case("min_word_w", paint(8, 16, [(2, 6, 3, 4), (2, 6, 10, 12)]), [[10, 2, 12, 6, 0, 8]], [1, 1, 128, 0]),
    # a band that loses all its words keeps its line number
    case("empty_line", paint(16, 10, [(1, 5, 5, 6), (10, 14, 2, 6)]), [[2, 10, 6, 14, 1, 16]], [1, 2, 128, 0]),
    # padding clamped at all four edges; ink is that of the unpadded box
    case("pad_clamp", paint(12, 14, [(1, 11, 1, 13)]), [[0, 0, 14, 12, 0, 120]], [1, 1, 128, 0], pad_x=3, pad_y=3),
    case("pad_inside", paint(20, 20, [(8, 12, 7, 13)]), [[5, 7, 15, 13, 0, 24]], [1, 1, 128, 0], pad_x=2, pad_y=1),
    case("light_text", paint(8, 12, [(2, 6, 3, 9)], bg=0, fg=255), [[3, 2, 9, 6, 0, 24]], [1, 1, 128, 0], light_text=1),
    # min_row_ink: rows with fewer ink pixels are not text rows (the 1-pixel rows 1 and 2 are not; rows 3..6 are)
    case("min_row_ink", paint(10, 12, [(1, 3, 4, 5), (3, 7, 2, 8)]), [[2, 3, 8, 7, 0, 24]], [1, 1, 128, 0], min_row_ink=2),
    # one gray value: Otsu has no threshold, nothing is ink
    case("constant", np.full((9, 11), 200, np.uint8), [], [0, 0, -1, 0], threshold=-1),
    case("constant_light", np.full((9, 11), 200, np.uint8), [], [0, 0, -1, 0], threshold=-1, light_text=1),
    case("all_ink", np.zeros((10, 12), np.uint8), [[0, 0, 12, 10, 0, 120]], [1, 1, 128, 0]),
    # Otsu on two levels a < b: every t in a..b-1 scores the same, the first wins: a
    case("otsu_two_level", paint(8, 12, [(2, 6, 3, 9)], bg=200, fg=50), [[3, 2, 9, 6, 0, 24]], [1, 1, 50, 0], threshold=-1),
    # Otsu tie between the splits {10 | 20 30} and {10 20 | 30}: the lowest t, 10; the ink is the 3 x 4 block of 10s
    case("otsu_tie", _TIE, [[0, 0, 4, 3, 0, 12]], [1, 1, 10, 0], threshold=-1),
]


# ---- seeded pages for the kernel-against-restatement tests: ink rectangles laid out as lines of words, plus counter-based speckle ----------
SEEDED = dict(min_row_ink=2, merge_gap=2, min_line_h=5, word_gap=4, min_word_w=3, pad_x=1, pad_y=1)      # threshold / light_text per test
# H, W, pitch, base offset in bytes, page seed (chosen so that the restatement's result takes every branch: test_segment_gpu.py asserts it)
SEEDED_SHAPES = [(1, 1, 1, 0, 1), (9, 37, 37, 0, 9037), (40, 100, 112, 0, 3), (70, 257, 257, 3, 70257), (300, 700, 704, 0, 300700)]


def _mix(v):
    """splitmix64 finaliser on uint64 arrays: the speckle is a function of (seed, pixel index), not of a generator's call order."""
    v = (v + np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    v = (v ^ (v >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    v = (v ^ (v >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return v ^ (v >> np.uint64(31))


def seeded_page(H, W, seed, light=False):
    """Dark text (0..80) on light paper (175..255): lines 5-11 rows high, some cut by a blank row or two (they merge), some too low (dropped);
    words 1-20 columns wide with gaps of 1-9 columns (they merge, split, or are too narrow); about one pixel every other row is speckle.  light: inverted."""
    rng = np.random.default_rng(seed)
    with np.errstate(over="ignore"):
        r = _mix(np.arange(H * W, dtype=np.uint64) + _mix(np.uint64(seed) * np.ones(1, np.uint64))[0]).reshape(H, W)
    page = (175 + (r >> np.uint64(8)) % np.uint64(81)).astype(np.uint8)
    inkv = ((r >> np.uint64(20)) % np.uint64(81)).astype(np.uint8)
    mask = (r % np.uint64(2 * W + 50)) == 0                                              # speckle: a pixel every other row
    y = int(rng.integers(0, 3))
    while y < H:
        h = int(rng.choice([2, 3, 5, 6, 8, 11]))
        cut = int(rng.choice([0, 0, 1, 2, 3])) if h >= 5 else 0                          # blank rows inside the line: <= merge_gap merges
        x = int(rng.integers(0, 4))
        while x < W:
            w = int(rng.choice([1, 2, 3, 5, 9, 14, 20]))
            mask[y:y + h, x:x + w] = True
            if cut:
                mask[y + h // 2:y + h // 2 + cut, :] = False
            x += w + int(rng.choice([1, 2, 3, 4, 6, 9]))
        y += h + int(rng.choice([1, 3, 4, 7]))
    page = np.where(mask, inkv, page).astype(np.uint8)
    return (255 - page).astype(np.uint8) if light else page
