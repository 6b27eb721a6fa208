"""Hand-painted pages with hand answers for aocr_segment_page_spaced, shared by test_spacing_cpu.py (the restatement) and
test_spacing_gpu.py (the kernels).  Every expected gap, flag and box below was written down from the bars, not computed.  Box rows are
x0 y0 x1 y1 line ink; spacing rows are gap used, flags, gaps counted m, a, c, band height, 0, 0.  The spacing parameters are HAND (round
numbers for sums done by hand, not the library's defaults) unless a case says otherwise."""
import numpy as np

from segment_cases import paint

HAND = dict(min_gaps=4, lo_percent=10, hi_percent=80, default_percent=25, ratio_percent=150)
BASE = dict(threshold=128, light_text=0, min_row_ink=1, merge_gap=2, min_line_h=3, word_gap=4, min_word_w=2, pad_x=0, pad_y=0)


def bars(y0, h, x0, w, gaps):
    """rects of len(gaps) + 1 bars of width w and height h, the first at x0, `gaps` empty columns between neighbours."""
    out, x = [(y0, y0 + h, x0, x0 + w)], x0 + w
    for g in gaps:
        out.append((y0, y0 + h, x + g, x + g + w))
        x += g + w
    return out


def case(name, page, boxes, counts, rows, spacing=None, **kw):
    p = dict(BASE)
    p.update(kw)
    return dict(name=name, page=page, params=p, spacing=dict(HAND, **(spacing or {})), boxes=np.array(boxes, np.int32).reshape(-1, 6),
                counts=np.array(counts, np.int32), rows=np.array(rows, np.int32).reshape(-1, 8))


# Line A: rows 2..12 (h 10), bars 3 wide, letter gaps 1, word gaps 4: words [2,13) [17,28) [32,43).  lo 1, hi 8; hist[1] = 6, hist[4] = 2;
# two lengths: every t in 1..3 ties and the first wins, t = 1, a = 1, c = 4, est = (1 + 4 + 1) >> 1 = 3.  A fixed word_gap cuts it right in 2..4.
# Line B: rows 20..50 (h 30), bars 8 wide, letter gaps 5, word gaps 14: words [2,36) [50,84) [98,132).  lo 3, hi 24; hist[5] = 6,
# hist[14] = 2, t = 5, a = 5, c = 14, est = 10.  A fixed word_gap cuts it right in 6..14: no value serves both lines.
TWO_LINES = paint(54, 140, bars(2, 10, 2, 3, [1, 1, 4, 1, 1, 4, 1, 1]) + bars(20, 30, 2, 8, [5, 5, 14, 5, 5, 14, 5, 5]))
TWO_LINES_WORDS = 6

CASES = [
    case("two_lines", TWO_LINES,
         [[2, 2, 13, 12, 0, 90], [17, 2, 28, 12, 0, 90], [32, 2, 43, 12, 0, 90],
          [2, 20, 36, 50, 1, 720], [50, 20, 84, 50, 1, 720], [98, 20, 132, 50, 1, 720]], [6, 2, 128, 0],
         [[3, 0, 8, 1, 4, 10, 0, 0], [10, 0, 8, 5, 14, 30, 0, 0]]),
    # flag 1: two gaps (1 and 6) are fewer than min_gaps; the split is still reported (t = 1, a = 1, c = 6); the default 10 * 25 / 100 = 2
    # merges the gap of 1 and keeps the gap of 6
    case("too_few_gaps", paint(14, 22, bars(2, 10, 2, 3, [1, 6])), [[2, 2, 9, 12, 0, 60], [15, 2, 18, 12, 0, 30]], [2, 1, 128, 0],
         [[2, 1, 2, 1, 6, 10, 0, 0]]),
    # flag 2: five gaps, all 3 columns: no split (t = -1, a = c = 0); the default 2 keeps all six bars apart
    case("one_gap_length", paint(14, 36, bars(2, 10, 1, 3, [3, 3, 3, 3, 3])),
         [[1, 2, 4, 12, 0, 30], [7, 2, 10, 12, 0, 30], [13, 2, 16, 12, 0, 30], [19, 2, 22, 12, 0, 30], [25, 2, 28, 12, 0, 30], [31, 2, 34, 12, 0, 30]],
         [6, 1, 128, 0], [[2, 2, 5, 0, 0, 10, 0, 0]]),
    # flag 3: gaps 4 5 4 5 4: t = 4, a = 4, c = 5, and 5 * 100 < 4 * 150: the classes are not separated; the default 2
    case("not_separated", paint(14, 37, bars(2, 10, 1, 2, [4, 5, 4, 5, 4])),
         [[1, 2, 3, 12, 0, 20], [7, 2, 9, 12, 0, 20], [14, 2, 16, 12, 0, 20], [20, 2, 22, 12, 0, 20], [27, 2, 29, 12, 0, 20], [33, 2, 35, 12, 0, 20]],
         [6, 1, 128, 0], [[2, 3, 5, 4, 5, 10, 0, 0]]),
    # adjacent bins, and the ratio met with equality: gaps 2 2 3 2 2: t = 2, a = 2, c = 3, 3 * 100 >= 2 * 150, est = (2 + 3 + 1) >> 1 = 3 = c
    case("adjacent_bins", paint(14, 26, bars(2, 10, 1, 2, [2, 2, 3, 2, 2])), [[1, 2, 11, 12, 0, 60], [14, 2, 24, 12, 0, 60]], [2, 1, 128, 0],
         [[3, 0, 5, 2, 3, 10, 0, 0]]),
    # the clamp at lo: h 40, lo 4, hi 32; gaps 1 1 3 1 1: a = 1, c = 3, est = 2 < lo: gap 4 (flag 0 + 4), and every gap merges: one word
    case("clamp_lo", paint(44, 30, bars(2, 40, 2, 3, [1, 1, 3, 1, 1])), [[2, 2, 27, 42, 0, 720]], [1, 1, 128, 0], [[4, 4, 5, 1, 3, 40, 0, 0]]),
    # hi: h 10, hi = clip = 8; gaps 2 2 20 2 2: the gutter of 20 counts in bin 8, a = 2, c = 8, est = (2 + 8 + 1) >> 1 = 5 (unclipped it
    # would be 11, above hi).  est <= c <= clip <= hi, and the default is at most hi too: the upper clamp itself never changes a value
    case("clip_at_hi", paint(14, 44, bars(2, 10, 1, 2, [2, 2, 20, 2, 2])), [[1, 2, 11, 12, 0, 60], [31, 2, 41, 12, 0, 60]], [2, 1, 128, 0],
         [[5, 0, 5, 2, 8, 10, 0, 0]]),
    # hi_percent 50: hi = clip = 5, the same bars: a = 2, c = 5, est = 4
    case("clip_at_hi_50", paint(14, 44, bars(2, 10, 1, 2, [2, 2, 20, 2, 2])), [[1, 2, 11, 12, 0, 60], [31, 2, 41, 12, 0, 60]], [2, 1, 128, 0],
         [[4, 0, 5, 2, 5, 10, 0, 0]], spacing=dict(hi_percent=50)),
    # a gutter wider than 255 columns: h 320, lo 32, hi 256, clip 255; gaps 40 40 300 40 40: the gutter counts in bin 255, a = 40,
    # c = 255, est = (40 + 255 + 1) >> 1 = 148
    case("gutter_over_255", paint(324, 530, bars(2, 320, 5, 10, [40, 40, 300, 40, 40])),
         [[5, 2, 115, 322, 0, 9600], [415, 2, 525, 322, 0, 9600]], [2, 1, 128, 0], [[148, 0, 5, 40, 255, 320, 0, 0]]),
    # a band that loses all its words to min_word_w (three bars one column wide, gaps 5 5: flag 1, one length, the default 2) keeps its
    # line number and its spacing row; the line below has one word and no gap: h 5, lo 1, hi 4, the default max(1, 5 * 25 / 100) = 1
    case("no_words_left", paint(24, 16, bars(2, 10, 1, 1, [5, 5]) + bars(16, 5, 4, 6, [])), [[4, 16, 10, 21, 1, 30]], [1, 2, 128, 0],
         [[2, 1, 2, 0, 0, 10, 0, 0], [1, 1, 0, 0, 0, 5, 0, 0]]),
    # min_gaps 2 turns the estimate on for too_few_gaps' bars: a = 1, c = 6, est = 4
    case("min_gaps_2", paint(14, 22, bars(2, 10, 2, 3, [1, 6])), [[2, 2, 9, 12, 0, 60], [15, 2, 18, 12, 0, 30]], [2, 1, 128, 0],
         [[4, 0, 2, 1, 6, 10, 0, 0]], spacing=dict(min_gaps=2)),
]
