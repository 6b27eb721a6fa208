"""Hand pages for aocr_invert_panels with their answers written out (out, the panels rows, the eight counts), and the seeded page with
reversed-out bands that the motive tests and the GPU tests share.  Test infrastructure: numpy only."""
import numpy as np

from segment_cases import seeded_page

SMALL = dict(threshold=128, light_text=0, connectivity=8, min_w=8, min_h=4, fill_percent=60, min_inside_percent=2)
SEEDED = dict(connectivity=8, min_w=40, min_h=10, fill_percent=40, min_inside_percent=2)       # the seeded lines are about 60 % text
SEEDED_SHAPES = ((300, 700, 700, 0, 11), (300, 700, 731, 5, 11), (61, 257, 263, 3, 5))        # H, W, pitch, offset, seed


def _paper(H=12, W=80):
    return np.full((H, W), 255, np.uint8)


def _inverted(page, *rects):
    out = page.copy()
    for x0, y0, x1, y1 in rects:
        out[y0:y1, x0:x1] = 255 - page[y0:y1, x0:x1]
    return out


def _slab():
    """a 40 x 8 slab with two `words` of 4 x 2 and 8 x 2 light pixels on it, and a 3 x 3 glyph beside it"""
    page = _paper()
    page[2:10, 10:50] = 0
    page[4:6, 14:18] = 255
    page[4:6, 22:30] = 255
    page[3:6, 60:63] = 0
    return page


def _bar():
    page = _paper()
    page[2:10, 10:50] = 0
    return page


def _u_shape():
    """a U of two 4-wide posts and a 2-high foot, fill 144 / 400, and a 20 x 5 panel with four light pixels between the posts"""
    page = _paper()
    page[1:11, 5:9] = 0
    page[1:11, 41:45] = 0
    page[9:11, 5:45] = 0
    page[3:8, 15:35] = 0
    page[5, [18, 19, 25, 26]] = 255
    return page


def _glyph():
    page = _paper()
    page[3:6, 60:63] = 0
    return page


def _case(name, page, params, out, panels, counts):
    return dict(name=name, page=page, params=params, out=out, panels=np.array(panels, np.int32).reshape(-1, 8), counts=np.array(counts, np.int32))


CASES = [
    # the slab's label is the index of its first pixel, 2 * 80 + 10; 24 of its 320 hull pixels are light
    _case("slab", _slab(), SMALL, _inverted(_slab(), (10, 2, 50, 10)), [[10, 2, 50, 10, 170, 296, 320, 1]], [2, 1, 1, 1, 128, 305, 320, 0]),
    _case("slab_light", 255 - _slab(), dict(SMALL, light_text=1), 255 - _inverted(_slab(), (10, 2, 50, 10)), [[10, 2, 50, 10, 170, 296, 320, 1]],
          [2, 1, 1, 1, 128, 305, 320, 0]),
    # nothing written on it: examined and turned down, the page comes back as it is
    _case("solid_bar", _bar(), SMALL, _bar(), [[10, 2, 50, 10, 170, 320, 320, 0]], [1, 1, 1, 0, 128, 320, 0, 0]),
    _case("solid_bar_inside_0", _bar(), dict(SMALL, min_inside_percent=0), _inverted(_bar(), (10, 2, 50, 10)), [[10, 2, 50, 10, 170, 320, 320, 1]],
          [1, 1, 1, 1, 128, 320, 320, 0]),
    # the U's spans run from post to post and cover the small panel: every pixel between the posts is inverted once
    _case("u_shape_over_a_panel", _u_shape(), dict(SMALL, fill_percent=30), _inverted(_u_shape(), (5, 1, 45, 11)),
          [[5, 1, 45, 11, 85, 144, 400, 1], [15, 3, 35, 8, 255, 96, 100, 1]], [2, 2, 2, 2, 128, 240, 500, 0]),
    # at fill 60 the U is a figure, not a panel: only the small panel is inverted
    _case("u_shape_rejected", _u_shape(), SMALL, _inverted(_u_shape(), (15, 3, 35, 8)),
          [[5, 1, 45, 11, 85, 144, 400, 0], [15, 3, 35, 8, 255, 96, 100, 1]], [2, 2, 2, 1, 128, 240, 100, 0]),
    _case("no_candidate", _glyph(), SMALL, _glyph(), [], [1, 0, 0, 0, 128, 9, 0, 0]),
    _case("one_gray", np.full((12, 80), 77, np.uint8), dict(SMALL, threshold=-1), np.full((12, 80), 77, np.uint8), [], [0, 0, 0, 0, -1, 0, 0, 0]),
]


def panel_page(H, W, seed, light=False):
    """(painted, plain, rects): `plain` is segment_cases.seeded_page with a text-free frame around every rectangle of `rects` (x0, y0, x1, y1):
    the rectangle's own outermost rows and columns, the row above, the row below, and the band's rows outside the rectangle, so that the
    slab touches no other ink, reaches its box in every row, and stands alone in its rows; `painted` is `plain` with every rectangle
    replaced by 255 - v: a dark slab (a light one with `light`) that carries the band's words reversed out."""
    plain = seeded_page(H, W, seed, light).copy()
    rng = np.random.default_rng(seed + 977)
    blank = 55 if light else 200
    xa = 3 + int(rng.integers(0, 4))
    xb = W - 3 - int(rng.integers(0, 4))
    rects, y = [], 3 + int(rng.integers(0, 6))
    while True:
        h = int(rng.integers(14, 34))
        if y + h + 2 > H:
            break
        rects.append((xa, y, xb, y + h))
        y += h + int(rng.integers(12, 40))
    for x0, y0, x1, y1 in rects:
        plain[y0 - 1:y1 + 1, :x0 + 1] = blank
        plain[y0 - 1:y1 + 1, x1 - 1:] = blank
        plain[[y0 - 1, y0, y1 - 1, y1], :] = blank
    painted = plain.copy()
    for x0, y0, x1, y1 in rects:
        painted[y0:y1, x0:x1] = 255 - plain[y0:y1, x0:x1]
    return painted, plain, rects


def rotated_slab(H, W, c=10, s=1, light=False):
    """a slab turned by atan(s / c) (a few degrees) about the page's middle, with a dotted light line along its long axis: its hull is smaller
    than its box, and none of the box's corners is part of it"""
    yy, xx = np.mgrid[:H, :W]
    dx, dy = xx - W // 2, yy - H // 2
    u, v = dx * c + dy * s, dy * c - dx * s
    a, b = (W // 2 - 8) * c, (H // 2 - 5) * c
    page = np.where((np.abs(u) <= a) & (np.abs(v) <= b), 0, 255).astype(np.uint8)
    page[(np.abs(v) <= c // 2) & (np.abs(u) <= a - 6 * c) & (xx % 2 == 0)] = 255
    return (255 - page).astype(np.uint8) if light else page


def diamond(R):
    """a filled diamond |dx| + |dy| <= R with a light stripe across its middle row, on a (2R + 5) square page"""
    n = 2 * R + 5
    yy, xx = np.mgrid[:n, :n]
    page = np.where(np.abs(yy - n // 2) + np.abs(xx - n // 2) <= R, 0, 255).astype(np.uint8)
    page[n // 2, n // 2 - R + 2:n // 2 + R - 1:2] = 255
    return page
