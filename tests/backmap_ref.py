"""The corner fields of Model.recognize_page written out field by field from the public point functions of aocr.page, as its docstring
describes them: what test_page_backmap_cpu.py holds aocr.page.backmap_corners to, and what the combined recognize_page cases of
test_recognize_gpu.py expect.  The arguments are backmap_corners' own: None for a stage that did not run, () for a resize or a warp that
left the page alone."""
import numpy as np

from aocr import page as P


def corner_fields(boxes, curl=None, skew=None, turn=None, resize=None, warp=None):
    want = {}
    cx, cy = P.box_corners(boxes)
    if curl is not None:
        ux, uy = P.uncurl_points(cx, cy, *curl)
        want["uncurled_corners"] = np.stack([ux, uy], axis=2)
        rx, ry = ux.astype(np.int64), np.floor(uy + 0.5).astype(np.int64)               # y rounded half up
    if turn is not None:
        want["source_boxes"] = P.unrotate_boxes(boxes, *turn)
    if skew is not None:
        sx, sy = P.source_points(*((rx, ry) if curl is not None else (cx, cy)), *skew)
        if turn is not None:
            sx, sy = P.unrotate_points(sx, sy, *turn)
        want["source_corners"] = np.stack([sx, sy], axis=2)
    if resize is None and warp is None:
        return want
    if skew is not None:
        px, py = sx, sy
    elif curl is not None:
        px, py = P.unrotate_points(rx, ry, *turn) if turn is not None else (rx, ry)     # the corner POINTS, un-rotated
    elif turn is not None:
        px, py = P.box_corners(want["source_boxes"])                                    # the corners of the un-rotated BOX
    else:
        px, py = cx, cy
    px, py = px.astype(np.float64), py.astype(np.float64)
    if resize is not None:
        if len(resize):
            px, py = P.unscale_points(px, py, *resize)
        want["unscaled_corners"] = np.stack([px, py], axis=2)
    if warp is not None:
        if len(warp):
            px, py = P.warp_points(warp, px, py)
        want["photo_corners"] = np.stack([px, py], axis=2)
    return want
