"""Shapes, quads and coefficients for the rectification tests, shared by test_rectify_cpu.py (the restatement alone, and the host-only
aocr_rectify_plan) and test_rectify_gpu.py (the kernels against the restatement)."""
import numpy as np

import rectify_ref as R
from orient_cases import text_page
from segment_cases import seeded_page

# ---- aocr_warp_page --------------------------------------------------------------------------------------------------------------------------
# H, W, pitch, base offset in bytes
WARP_SHAPES = [(1, 1, 1, 0), (1, 7, 7, 0), (7, 1, 1, 0), (33, 65, 65, 0), (64, 64, 64, 0), (63, 129, 129, 0), (257, 129, 134, 3)]
NAN = float("nan")


def image_quad(H, W):
    return [0, 0, W - 1, 0, W - 1, H - 1, 0, H - 1]


def warp_cases(H, W):
    """[(name, coef (9) float64, Ho, Wo)] for an H x W source: the identity, a sub-rectangle copy, 2x up and 1/2x down, a strong keystone, a
    quad partly off the page (fill taps and fill pixels), a denominator that changes sign inside the output, and coefficients holding a
    NaN.  Planned from quads where the source has a quad (H, W >= 2), hand-made otherwise -- and the hand-made ones always."""
    f = lambda *c: np.array(c, np.float64)
    out = [("identity_hand", f(1, 0, 0, 0, 1, 0, 0, 0, 1), H, W),
           ("copy_hand", f(1, 0, W // 4, 0, 1, H // 4, 0, 0, 1), max(1, H // 2), max(1, W // 2)),
           ("up2_hand", f(1, 0, 0, 0, 1, 0, 0, 0, 2), 2 * H, 2 * W),
           ("down2_hand", f(2, 0, 0.5, 0, 2, 0.5, 0, 0, 1), (H + 1) // 2, (W + 1) // 2),
           ("keystone_hand", f(1, 0.125, 0, 0.0625, 1, 0, 0.1, 0.05, 1), H + 1, W + 2),
           ("off_page_hand", f(1, 0, -3, 0, 1, -2.5, 0, 0, 1), H + 5, W + 6),
           ("sign_change", f(1, 0.25, 0.5, 0.125, 1, 0.25, -2.0 / (W + 3), 0.0, 1.0), H + 2, W + 3),
           ("sign_change_y", f(1, 0, 0, 0, 1, 0, 0.0, -1.0 / (H + 1), 0.5), H + 2, W),
           ("nan_num", f(1, NAN, 0, 0, 1, 0, 0, 0, 1), H, W),
           ("nan_den", f(1, 0, 0, 0, 1, 0, NAN, 0, 1), H, W),
           ("inf_num", f(float("inf"), 0, 0, 0, 1, 0, 0, 0, 1), H, W)]
    if H >= 2 and W >= 2:
        plan = lambda name, quad, Wo=0, Ho=0: (lambda s, c: (name, c, s[1], s[0]))(*R.rectify_plan(quad, Wo, Ho))
        x0, y0 = W // 4, H // 4
        out += [plan("identity", image_quad(H, W), W, H),
                plan("copy", [x0, y0, x0 + W // 2, y0, x0 + W // 2, y0 + H // 2, x0, y0 + H // 2]),
                plan("up2", image_quad(H, W), 2 * W, 2 * H),
                plan("down2", image_quad(H, W), (W + 1) // 2, (H + 1) // 2),
                plan("keystone", [W // 3, 0, W - 1 - W // 3, 1, W - 1, H - 1, 0, H - 2]),
                plan("off_page", [-(W // 3), -(H // 4), W + W // 5, H // 6, W - 1, H + H // 3, W // 5, H - 1])]
    return out


# ---- aocr_find_page_quad ---------------------------------------------------------------------------------------------------------------------
def _rect(H, W, y0, y1, x0, x1, bg=40, fg=220):
    p = np.full((H, W), bg, np.uint8)
    p[y0:y1, x0:x1] = fg
    return p


def _two(H, W, a, b, bg=40, fg=220):
    p = np.full((H, W), bg, np.uint8)
    for y0, y1, x0, x1 in (a, b):
        p[y0:y1, x0:x1] = fg
    return p


# quads (TL, TR, BR, BL) whose corners are the unique extremes of x+y and x-y over the polygon: test_rectify_cpu.py checks that
PHOTO_QUADS = {
    "keystone": dict(quad=[22, 14, 131, 9, 148, 101, 9, 108], H=120, W=160, page=(80, 100)),
    "turned": dict(quad=[30, 6, 120, 25, 104, 110, 12, 88], H=118, W=131, page=(70, 64)),
    "w63": dict(quad=[5, 4, 57, 7, 60, 70, 2, 66], H=75, W=63, page=(50, 40)),
    "w64": dict(quad=[5, 4, 58, 7, 61, 70, 2, 66], H=75, W=64, page=(50, 40)),
    "w65": dict(quad=[5, 4, 59, 7, 63, 70, 2, 66], H=75, W=65, page=(50, 40)),
    "wide": dict(quad=[12, 9, 290, 4, 297, 52, 3, 49], H=57, W=300, page=(40, 200)),
}

_photos = {}


def photo(name):
    """(photograph, quad) of PHOTO_QUADS[name]: a seeded text-like page with a clean margin of 6 pixels, on a desk of gray 60."""
    if name not in _photos:
        c = PHOTO_QUADS[name]
        page = np.pad(seeded_page(c["page"][0] - 12, c["page"][1] - 12, 7 * c["H"] + c["W"]), 6, constant_values=235)
        _photos[name] = (R.make_photo(page, c["quad"], c["H"], c["W"], 60), list(c["quad"]))
    return _photos[name]


def quad_cases():
    """[dict(name, page, threshold, dark_paper)]: what the issue lists, at widths 63, 64 and 65 and one wider than a workgroup."""
    out = []
    add = lambda name, page, threshold=-1, dark_paper=0: out.append(dict(name=name, page=page, threshold=threshold, dark_paper=dark_paper))
    add("one_gray", np.full((20, 64), 200, np.uint8))                                          # Otsu -1: nothing is paper
    add("one_gray_fixed", np.full((20, 65), 200, np.uint8), 128)                               # everything is paper: the image corners
    add("one_pixel", _rect(20, 63, 7, 8, 31, 32), 128)                                         # all four corners are the pixel: valid 0
    add("one_row", _rect(20, 65, 7, 8, 3, 60), 128)                                            # a line has no area: valid 0
    for W in (63, 64, 65):
        add(f"rect_w{W}", _rect(40, W, 5, 33, 4, W - 3))
        add(f"rect_fixed_w{W}", _rect(40, W, 5, 33, 4, W - 3), 100)
        add(f"rect_dark_paper_w{W}", _rect(40, W, 5, 33, 4, W - 3, bg=220, fg=40), -1, 1)
        add(f"all_borders_w{W}", _rect(37, W, 0, 37, 0, W), 128)
    add("larger_wins", _two(50, 130, (3, 20, 4, 40), (22, 48, 50, 125)))
    add("larger_wins_first", _two(50, 130, (3, 40, 4, 80), (42, 48, 90, 125)))
    add("equal_smaller_label", _two(50, 130, (10, 30, 70, 100), (12, 32, 5, 35)))              # the right one starts in an earlier row
    add("equal_same_row", _two(50, 130, (10, 30, 70, 100), (10, 30, 5, 35)))                   # the left one comes first in raster order
    add("touching_diagonally", _two(50, 130, (5, 20, 5, 40), (20, 45, 40, 120)))               # 8-connected: one sheet
    speckled = np.where(seeded_page(60, 140, 5) < 100, 230, 30).astype(np.uint8)                # a dark desk with bright specks and strokes
    speckled[10:50, 20:120] = 255
    add("speckled_desk", speckled, 128)
    add("tall", _rect(300, 70, 9, 290, 6, 66))
    for name in PHOTO_QUADS:
        add(f"photo_{name}", photo(name)[0])
        add(f"photo_{name}_fixed", photo(name)[0], 128)
    add("photo_dark_paper", (255 - photo("keystone")[0]).astype(np.uint8), -1, 1)
    return out


# ---- the text page for Model.recognize_page(rectify=...) -------------------------------------------------------------------------------------
TEXT_SEGMENT = dict(threshold=128, word_gap=4, merge_gap=0, min_line_h=6)      # segment params that cut the text page into words: 3 lines


def text_photo():
    """(page, photo, quad): three lines of atlas text, and its photograph on a dark desk with a mild keystone."""
    if "text" not in _photos:
        page = text_page(0, 2, 3)
        Hp, Wp = page.shape
        H, W = Hp + 60, Wp + 80
        quad = [31, 22, W - 44, 14, W - 25, H - 16, 12, H - 25]
        _photos["text"] = (page, R.make_photo(page, quad, H, W, 50), quad)
    return _photos["text"]
