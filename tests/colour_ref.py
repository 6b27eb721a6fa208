"""numpy restatement of aocr_estimate_page_colour and aocr_gray_page (include/aocr.h), for tests/test_colour_cpu.py and test_colour_gpu.py.
Integer arithmetic only, vectorised over the page: every expression below is the header's, in the header's order."""
import numpy as np

RED, YELLOW, GREEN, CYAN, BLUE, MAGENTA = range(6)
LUMA = (77, 150, 29)
DEFAULTS = dict(weights=LUMA, mode=0, balance=1, paper=None, paper_min=128, chroma_min=64, drop=0, fill=255)

# what each call writes: (name, words)
ESTIMATE_WORDS = (("paper", 3), ("estimated", 1), ("zero", 12))
GRAY_WORDS = (("paper", 3), ("estimated", 1), ("hues", 6), ("dropped", 1), ("zero", 5))


def histograms(rgb):
    """(3, 256) int64: hist[c][v] = the pixels whose channel c is v."""
    return np.stack([np.bincount(rgb[:, :, c].reshape(-1), minlength=256) for c in range(3)]).astype(np.int64)


def window_mode(hist, paper_min):
    """the v >= paper_min with the largest hist[v-2] + ... + hist[v+2] (bins outside 0..255 are 0), the larger v on a tie; 255 when no
    bin >= paper_min holds a pixel."""
    hist = np.asarray(hist, np.int64)
    if hist[paper_min:].sum() == 0:
        return 255
    padded = np.concatenate([np.zeros(2, np.int64), hist, np.zeros(2, np.int64)])
    best, best_v = -1, 255
    for v in range(paper_min, 256):
        s = int(padded[v:v + 5].sum())
        if s >= best:
            best, best_v = s, v
    return best_v


def estimate_paper(rgb, paper_min=128):
    """the 16 words of aocr_estimate_page_colour."""
    h = histograms(rgb)
    return np.array([window_mode(h[c], paper_min) for c in range(3)] + [1] + [0] * 12, np.int32)


def lut(p):
    """(256) int64: min(255, (v * 255 + p // 2) // p)."""
    v = np.arange(256, dtype=np.int64)
    return np.minimum(255, (v * 255 + p // 2) // p)


def hue_class(r, g, b):
    """(class, chroma) of balanced channels, int64 arrays."""
    r, g, b = (np.asarray(v, np.int64) for v in (r, g, b))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    c = mx - mn
    red = np.where(2 * (g - b) >= c, YELLOW, np.where(2 * (b - g) > c, MAGENTA, RED))
    green = np.where(2 * (r - b) > c, YELLOW, np.where(2 * (b - r) >= c, CYAN, GREEN))
    blue = np.where(2 * (g - r) > c, CYAN, np.where(2 * (r - g) >= c, MAGENTA, BLUE))
    return np.where(mx == r, red, np.where(mx == g, green, blue)), c


def gray_page(rgb, words_in=None, weights=LUMA, mode=0, balance=1, paper=None, paper_min=128, chroma_min=64, drop=0, fill=255):
    """(gray (H, W) uint8, the 16 words of colour_out_dev).  words_in: colour_in_dev (its paper is clamped to 1..255), or None: `paper`, or
    (255, 255, 255) without balance.  paper None with balance and no words_in is the caller's error."""
    if words_in is not None:
        p, est = [min(max(int(v), 1), 255) for v in words_in[:3]], int(words_in[3] != 0)
    elif balance:
        assert paper is not None
        p, est = [int(v) for v in paper], 0
    else:
        p, est = [255, 255, 255], 0
    r, g, b = (lut(p[c])[rgb[:, :, c]] for c in range(3))
    cls, c = hue_class(r, g, b)
    coloured = c >= chroma_min
    dropped = coloured & (((drop >> cls) & 1) == 1)
    if mode == 0:
        gray = (weights[0] * r + weights[1] * g + weights[2] * b + 128) >> 8
    else:
        gray = np.minimum(r, np.minimum(g, b))
    out = np.where(dropped, fill, gray).astype(np.uint8)
    hues = [int((coloured & (cls == k)).sum()) for k in range(6)]
    return out, np.array(p + [est] + hues + [int(dropped.sum())] + [0] * 5, np.int32)


def gray(rgb, **kw):
    """the gray page of recognize_page(colour=...): the estimate, when the params ask for one, then the gray rule."""
    p = dict(DEFAULTS)
    p.update(kw)
    words = estimate_paper(rgb, p["paper_min"]) if p["balance"] and p["paper"] is None else None
    return gray_page(rgb, words, **p)
