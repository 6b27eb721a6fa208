"""Shapes and pages shared by tests/test_colour_cpu.py and tests/test_colour_gpu.py."""
import numpy as np

from components_cases import MOTIVE_BOXES, MOTIVE_SEG, _LINE_Y, _WORD_X, motive_page
from segment_cases import _mix

# raw calls: 3W crosses empty and non-empty heads, whole vectors and tails; 1025 is one pixel more than a wave's segment
WIDTHS = (1, 5, 6, 21, 22, 43, 342, 1025)
HEIGHTS = (1, 3, 70)
OFFSETS = (0, 1, 3, 13)                        # source base, bytes
PITCH_EXTRA = (0, 1, 5)                        # source pitch = 3W + this; + 1: a channel phase taken from the address goes wrong on every row
OUTS = ((0, 0), (5, 3))                        # (out_pitch - W, out base offset)
MERGE_SHAPE = (300, 700)                       # several workgroups merge their histograms

PAPER_TINT = (250, 240, 200)
RED_INK, YELLOW_INK, BLUE_INK = (230, 20, 20), (250, 230, 40), (30, 40, 220)


def random_rgb(H, W, seed):
    """every byte a function of (seed, index); a third of the pixels near gray, so that both sides of chroma_min are populated."""
    with np.errstate(over="ignore"):
        r = _mix(np.arange(H * W * 3, dtype=np.uint64) + _mix(np.uint64(seed) * np.ones(1, np.uint64))[0]).reshape(H, W, 3)
    rgb = (r >> np.uint64(8)).astype(np.uint8)
    grayish = ((r[:, :, 0] >> np.uint64(40)) % np.uint64(3)) == 0
    base = rgb[:, :, :1].astype(np.int64) + ((r >> np.uint64(20)) % np.uint64(7)).astype(np.int64) - 3
    return np.where(grayish[:, :, None], np.clip(base, 0, 255).astype(np.uint8), rgb)


def paper_rgb(H, W, seed, tint=PAPER_TINT, low=False):
    """tinted paper with a little noise and some dark pixels; low: everything below 100."""
    rgb = random_rgb(H, W, seed).astype(np.int64)
    noise = rgb % 5 - 2
    page = np.clip(np.array(tint, np.int64)[None, None, :] + noise, 0, 255)
    page[rgb[:, :, 0] < 40] = 20
    if low:
        page = page * 99 // 255
    return page.astype(np.uint8)


# ---- the page the stage exists for: components_cases' two lines of three words, black on tinted paper ------------------------------------------
MARKED_DROP = (1 << 0) | (1 << 1) | (1 << 4)   # RED | YELLOW | BLUE
MARKED_SEG = MOTIVE_SEG
MARKED_BOXES = MOTIVE_BOXES
RULE_X = 40                                    # a vertical red rule, one pixel wide, through the gap of words 0 and 1 and through both lines
BAND = (6, 22, 42, 70)                         # y0, y1, x0, x1: a yellow highlighter band over word 1 of line 0 (the text stays black)
SPECK = (38, 40, 72, 75)                       # a blue speck in the gap of words 1 and 2 of line 1


def marked_page(marks=True, tint=PAPER_TINT):
    """(60, 120, 3): the unmarked page in black on tinted paper; with marks a red rule that joins the two lines, a yellow band over one
    word and a blue speck in a word gap."""
    gray = motive_page()
    rgb = np.where(gray[:, :, None] == 0, np.uint8(0), np.array(tint, np.uint8)[None, None, :]).astype(np.uint8)
    if marks:
        ink = gray == 0
        y0, y1, x0, x1 = BAND
        band = np.zeros_like(ink)
        band[y0:y1, x0:x1] = True
        rgb[band & ~ink] = YELLOW_INK
        rgb[2:58, RULE_X] = RED_INK
        y0, y1, x0, x1 = SPECK
        rgb[y0:y1, x0:x1] = BLUE_INK
    return rgb


def all_paper(H=60, W=120, tint=PAPER_TINT):
    return np.broadcast_to(np.array(tint, np.uint8), (H, W, 3)).copy()


__all__ = ["WIDTHS", "HEIGHTS", "OFFSETS", "PITCH_EXTRA", "OUTS", "MERGE_SHAPE", "PAPER_TINT", "MARKED_DROP", "MARKED_SEG", "MARKED_BOXES",
           "random_rgb", "paper_rgb", "marked_page", "all_paper", "_LINE_Y", "_WORD_X"]
