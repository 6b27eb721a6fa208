"""Page segmentation on the device: `aocr_segment_page` (word boxes of a gray page by projection profiles) and `aocr_crop_lines` (the boxes
cut out and scaled like `aocr_preprocess_lines`), the stage in front of `Model.recognize`.  Both calls only enqueue; nothing is read back
here.  Projection profiles assume horizontal lines in one column: a skewed page goes through `estimate_skew_device` and `deskew_page_device`
(`aocr_estimate_skew`, `aocr_deskew_page`: a sweep of sheared profiles, then a shear) first; a multi-column page is first cut into blocks by
`layout_page_device` (`aocr_ink_integral`, `aocr_layout_blocks`: a summed-area table of the ink, then a recursive XY cut) and each block is
segmented as a view of the page.  A profile cannot tell a word from a speck or a ruled line: `clean_page_device` (`aocr_clean_page`: connected
components of the ink, `label_components_device`) paints over the components that cannot be text before any profile is taken.  One global threshold assumes paper of one brightness: an unevenly lit page goes through `flatten_page_device` (`aocr_flatten_page`) before all of them.  All of them assume that the lines run along x, the right way up: a page
fed sideways goes through `estimate_orientation_device` (`aocr_estimate_orientation`: where ink runs start along x and along y) and
`rotate_page_device` (`aocr_rotate_page`: quarter turns) before the deskew; `unrotate_boxes` takes boxes back to the page as given.  A
photographed page, a quadrilateral on a desk seen in perspective, goes through `find_page_quad_device` (`aocr_find_page_quad`: the corners
of the largest paper component), `rectify_plan` (`aocr_rectify_plan`, host only) and `warp_page_device` (`aocr_warp_page`: the projective
resample) before all of them; `warp_points` takes points of the rectified page back to the photograph.  Every one of them counts in
pixels of text at 300 dpi: a page scanned at another resolution goes through `estimate_glyph_size_device` (`aocr_estimate_glyph_size`: the
median of min(w, h) over the component boxes), `scale_plan` (host only) and `resize_page_device` (`aocr_resize_page`: exact area
resampling) after the flattening; `unscale_points` takes points back to the page before resizing.  A shear takes out one slope: the
curved lines of a page bending into a book's gutter go through `estimate_curl_device` (`aocr_estimate_curl`: the row shift between
neighbouring column groups by correlation) and `dewarp_page_device` (`aocr_dewarp_page`: every column moved by its shift) after the
deskew; `uncurl_points` takes points back to the page before it.  All of them read a gray page: a colour page, (H, W, 3) RGB, goes through
`estimate_page_colour_device` (`aocr_estimate_page_colour`: the paper colour, the mode of every channel) and `gray_page_device`
(`aocr_gray_page`: the paper divided out, a weighted sum or the darkest channel, and the coloured pixels of chosen hue classes -- a red
form rule, a highlighter stroke, a stamp -- turned into paper) before any of them; the shape does not change, so no box needs a way back.
None of them straightens the writing inside a box: italic print and handwriting go through `estimate_slant_device` (`aocr_estimate_slant`:
one slant per box from a sweep of sheared column profiles) after the segmentation, and `crop_lines_slanted_device`
(`aocr_crop_lines_slanted`: the crops with every row moved back along x) takes the place of `crop_lines_device`; `slant_extent` is how far
such a crop reaches beyond its box on either side.  The boxes do not move.  One `word_gap` cuts every line of the page into words; a page
whose lines are set in different sizes goes through `segment_page_spaced_device` (`aocr_segment_page_spaced`: the gap of every line
estimated from the line's own gaps) in place of `segment_page_device`.  A form or a table is text that touches rules, one component with
them: `remove_rules_device` (`aocr_remove_rules`: run lengths per pixel) takes out what is long one way and thin the other and leaves the
strokes that cross it, after the deskew and before layout and segmentation.  The boxes do not move.  Faded print beside strong print, a
stain, show-through: no single threshold is right everywhere even on evenly lit paper; `binarize_page_device` (`aocr_binarize_page`: a
Sauvola threshold per pixel from the window's mean and standard deviation) writes a page on which the fixed threshold 127 is the local
decision, behind `flatten_page_device` and in front of everything that thresholds.  A table header row or a section bar
is light text on a dark slab, one component that holds no readable crop: `invert_panels_device` (`aocr_invert_panels`) finds such slabs
among the components and inverts the bytes inside their row spans, in front of `clean_page_device`.  The boxes do not move."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from ._lib import BinarizeParams, Box, CleanParams, ColourParams, CurlParams, FlattenParams, GlyphParams, LayoutParams, PanelParams, RectifyParams, RuleParams, ScaleParams, SegmentParams, SkewParams, SlantParams, SpacingParams, check, lib, ptr

IMG_H = 32
MIN_ASPECT = 0.5


def _stream(stream, device):
    s = stream if stream is not None else torch.cuda.current_stream(device).cuda_stream
    return s if isinstance(s, C.c_void_p) else C.c_void_p(s)


def _page_view(page_dev):
    """a 2-D uint8 device tensor whose rows are contiguous (a view of a larger image is taken as it is: its row stride is the pitch)."""
    if not (isinstance(page_dev, torch.Tensor) and page_dev.dim() == 2 and page_dev.dtype == torch.uint8):
        raise ValueError("page must be a 2-D uint8 tensor (H, W): colour pages are out of scope")
    if not page_dev.is_cuda:
        raise ValueError("page must be on the device")
    H, W = page_dev.shape
    if H < 1 or W < 1:
        raise ValueError(f"empty page {tuple(page_dev.shape)}")
    if W > 1 and page_dev.stride(1) != 1:
        page_dev = page_dev.contiguous()
    pitch = page_dev.stride(0) if H > 1 else W
    if pitch < W:                                            # an expanded (stride 0) view
        page_dev = page_dev.contiguous()
        pitch = W
    return page_dev, int(pitch)


def _rgb_view(rgb_dev):
    """`_page_view` for a colour page: an (H, W, 3) uint8 device tensor whose pixels are contiguous (3 bytes, channel stride 1, pixel stride
    3); a view of a wider image is taken as it is: its row stride is the pitch."""
    if not (isinstance(rgb_dev, torch.Tensor) and rgb_dev.dim() == 3 and rgb_dev.shape[2] == 3 and rgb_dev.dtype == torch.uint8):
        raise ValueError("page must be a 3-D uint8 tensor (H, W, 3)")
    if not rgb_dev.is_cuda:
        raise ValueError("page must be on the device")
    H, W, _ = rgb_dev.shape
    if H < 1 or W < 1:
        raise ValueError(f"empty page {tuple(rgb_dev.shape)}")
    if rgb_dev.stride(2) != 1 or (W > 1 and rgb_dev.stride(1) != 3):
        rgb_dev = rgb_dev.contiguous()
    pitch = rgb_dev.stride(0) if H > 1 else 3 * W
    if pitch < 3 * W:                                        # an expanded (stride 0) view
        rgb_dev = rgb_dev.contiguous()
        pitch = 3 * W
    return rgb_dev, int(pitch)


def _scratch(query, dev, *args):
    """the int64 scratch tensor of a call on `dev`: lib.<query>(*args) bytes, rounded up to whole words.  A size of 0 is the library turning
    the arguments down: raised through `check` under the query's name."""
    need = int(getattr(lib, query)(*args))
    if need == 0:
        check(1, query)
    return torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)


def segment_page_device(page_dev, params=None, max_boxes=1024, stream=None):
    """(boxes (max_boxes, 6) int32 rows x0 y0 x1 y1 line ink, counts (4) int32: boxes found, lines, threshold, 0) as device tensors.
    Rows of boxes beyond min(counts[0], max_boxes) are not written (they hold zeros).  Enqueues only.
    stream: the raw handle of the CURRENT torch stream of the page's device (None takes it): the scratch and the outputs come from torch's
    caching allocator, which orders the reuse of a freed block on the current stream only, and the scratch is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else SegmentParams()
    dev = page_dev.device
    scratch = _scratch("aocr_segment_scratch_bytes", dev, H, W, max_boxes)
    boxes = torch.zeros((max_boxes, 6), dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    check(lib.aocr_segment_page(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), ptr(scratch), max_boxes, ptr(boxes),
                                ptr(counts)), "aocr_segment_page")
    return boxes, counts


def segment_page_spaced_device(page_dev, params=None, spacing=None, max_boxes=1024, stream=None, max_lines=None):
    """`segment_page_device` with one word gap per line, estimated on the device from the line's own gaps (`aocr_segment_page_spaced`):
    (boxes, counts, spacing_rows (max_lines, 8) int32: gap used, flags (0 estimated, 1 too few gaps, 2 one gap length, 3 classes not
    separated; + 4 clamped), gaps counted, the two occupied gap lengths around the split, band height, 0, 0) as device tensors.  Rows of
    spacing_rows beyond min(counts[1], max_lines) are not written (they hold zeros).  params.word_gap is not read, but 0 is an error.
    spacing: a `SpacingParams` (default: its defaults).  max_lines None: (H + 1) // 2, every line a page of H rows can have.  Enqueues
    only.  stream: as for `segment_page_device`."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else SegmentParams()
    spacing = spacing if spacing is not None else SpacingParams()
    max_lines = (H + 1) // 2 if max_lines is None else int(max_lines)
    dev = page_dev.device
    scratch = _scratch("aocr_segment_spaced_scratch_bytes", dev, H, W, max_boxes)
    boxes = torch.zeros((max_boxes, 6), dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    rows = torch.zeros((max(max_lines, 0), 8), dtype=torch.int32, device=dev)
    check(lib.aocr_segment_page_spaced(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), C.byref(spacing), ptr(scratch), max_boxes,
                                       ptr(boxes), ptr(counts), max_lines, ptr(rows) if max_lines > 0 else None), "aocr_segment_page_spaced")
    return boxes, counts, rows


def crop_lines_device(page_dev, boxes, counts, out_w, out_h=IMG_H, stream=None):
    """(n_boxes, 1, out_h, out_w) fp32 device tensor: row i < min(n_boxes, counts[0]) is box i of the page scaled as `aocr_preprocess_lines`
    scales it; the other rows are paper (255).  boxes (n_boxes, 6) int32 and counts (>= 1) int32 device tensors as `segment_page_device`
    returns them; counts None: every row of boxes is cropped.  Enqueues only.  stream: as for `segment_page_device`, the current torch stream
    (the call reads boxes and counts, which the caller may drop right after it)."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    assert boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.dtype == torch.int32 and boxes.device == dev
    boxes = boxes.contiguous()
    n = int(boxes.shape[0])
    if counts is not None:
        assert counts.dtype == torch.int32 and counts.device == dev and counts.numel() >= 1
        counts = counts.contiguous()
    out = torch.full((n, 1, int(out_h), int(out_w)), 255.0, dtype=torch.float32, device=dev)
    if n:
        check(lib.aocr_crop_lines(_stream(stream, dev), ptr(page_dev), pitch, H, W, ptr(boxes), ptr(counts), n, int(out_h), int(out_w),
                                  ptr(out)), "aocr_crop_lines")
    return out


def estimate_skew_device(page_dev, params=None, stream=None, scores=False):
    """skew (4) int32 device tensor: the winning candidate k, its slope k * step_q16 (rows per column, Q16), the threshold used, 0; with
    scores=True (skew, scores (2 * n_steps + 1) int64: the score of every candidate, k = -n_steps first).  params: a `SkewParams` (default:
    Otsu, +-96 steps of 1/1024 row per column).  Enqueues only.  stream: as for `segment_page_device`, the current torch stream."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else SkewParams()
    dev = page_dev.device
    scratch = _scratch("aocr_skew_scratch_bytes", dev, H, W, params.n_steps)
    skew = torch.zeros(4, dtype=torch.int32, device=dev)
    sc = torch.zeros(2 * params.n_steps + 1, dtype=torch.int64, device=dev) if scores else None
    check(lib.aocr_estimate_skew(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), ptr(scratch), ptr(skew), ptr(sc)),
          "aocr_estimate_skew")
    return (skew, sc) if scores else skew


def deskew_page_device(page_dev, skew, fill=255, stream=None):
    """a new (H, W) uint8 device tensor: the page with the slope taken out by `aocr_deskew_page` (shear, nearest neighbour; `fill` where the
    source is outside the page).  skew: the device tensor of `estimate_skew_device` (its slope is read on the device: no host sync), or a
    Python int slope in Q16 rows per column.  Enqueues only.  stream: as for `segment_page_device`."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    skew_dev, slope = None, 0
    if isinstance(skew, torch.Tensor):
        assert skew.dtype == torch.int32 and skew.device == dev and skew.numel() >= 2
        skew_dev = skew.contiguous()
    else:
        slope = int(skew)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    check(lib.aocr_deskew_page(_stream(stream, dev), ptr(page_dev), pitch, H, W, ptr(skew_dev), slope, int(fill), ptr(out), W), "aocr_deskew_page")
    return out


def flatten_page_device(page_dev, params=None, stream=None):
    """a new (H, W) uint8 device tensor: the page with its background divided out by `aocr_flatten_page` (the paper brightness near every
    pixel, a windowed max then a windowed mean, becomes 255).  params: a `FlattenParams` (default: radius 16, dark text).  Enqueues only.
    stream: as for `segment_page_device`, the current torch stream; the scratch is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else FlattenParams()
    dev = page_dev.device
    scratch = _scratch("aocr_flatten_scratch_bytes", dev, H, W, params.radius)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    check(lib.aocr_flatten_page(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), ptr(scratch), ptr(out), W), "aocr_flatten_page")
    return out


def binarize_page_device(page_dev, params=None, stream=None, counts=False):
    """a new (H, W) uint8 device tensor: the page binarised locally by `aocr_binarize_page` (a Sauvola threshold per pixel from the mean and
    the standard deviation of the window around it): on it the fixed threshold 127 is the local decision, ink 0..127 and paper 128..255
    (0 and 255 with params.hard; mirrored with params.light_text).  params: a `BinarizeParams` (default: radius 20, k = 51 / 256, R = 128,
    dark text, gray output).  counts=True: (out, counts (4) int32 on the device: ink pixels, the smallest T, the largest T, 0).  Enqueues
    only.  stream: as for `segment_page_device`, the current torch stream; the scratch is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else BinarizeParams()
    dev = page_dev.device
    scratch = _scratch("aocr_binarize_scratch_bytes", dev, H, W, params.radius)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    words = torch.zeros(4, dtype=torch.int32, device=dev) if counts else None
    check(lib.aocr_binarize_page(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), ptr(scratch), ptr(out), W, ptr(words)),
          "aocr_binarize_page")
    return (out, words) if counts else out


def _ink_integral(page_dev, pitch, threshold, light_text, stream):
    H, W = page_dev.shape
    dev = page_dev.device
    scratch = _scratch("aocr_integral_scratch_bytes", dev, H, W)
    sat_pitch = (W + 1 + 3) & ~3                             # rows of whole 16-byte words
    sat = torch.empty((H + 1, sat_pitch), dtype=torch.int32, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    check(lib.aocr_ink_integral(_stream(stream, dev), ptr(page_dev), pitch, H, W, int(threshold), int(light_text), ptr(scratch), ptr(sat),
                                sat_pitch, ptr(info)), "aocr_ink_integral")
    return sat, info


def ink_integral_device(page_dev, threshold=-1, light_text=0, stream=None):
    """(sat, info): sat an (H+1, W+1) int32 view of a table whose rows are `sat.stride(0)` elements apart -- sat[y+1, x+1] is the number of
    ink pixels in [0,x] x [0,y], row 0 and column 0 are zero (counts are at most 2^26: int32 holds them) -- and info (4) int32: the threshold
    used, the total ink, 0, 0 (`aocr_ink_integral`).  threshold -1: Otsu.  Enqueues only.  stream: as for `segment_page_device`, the current
    torch stream; the scratch is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    sat, info = _ink_integral(page_dev, pitch, threshold, light_text, stream)
    return sat[:, :page_dev.shape[1] + 1], info


def layout_page_device(page_dev, params=None, threshold=-1, light_text=0, max_blocks=256, stream=None):
    """(blocks (max_blocks, 6) int32 rows x0 y0 x1 y1 depth ink in reading order, counts (4) int32: blocks written, levels cut, regions
    dropped by size, overflow flag, info (4) int32: threshold, total ink, 0, 0) as device tensors: the page's ink table (`aocr_ink_integral`)
    and the recursive XY cut on it (`aocr_layout_blocks`).  Rows of blocks beyond counts[0] are not written (they hold zeros).  params: a
    `LayoutParams` (default: gaps of 24 columns and 30 rows).  Enqueues only.  stream: as for `segment_page_device`; the table and the scratch
    are freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else LayoutParams()
    dev = page_dev.device
    scratch = _scratch("aocr_layout_scratch_bytes", dev, H, W, max_blocks)        # checked before the ink table is built
    sat, info = _ink_integral(page_dev, pitch, threshold, light_text, stream)
    blocks = torch.zeros((max_blocks, 6), dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    check(lib.aocr_layout_blocks(_stream(stream, dev), ptr(sat), sat.stride(0), H, W, C.byref(params), ptr(scratch), max_blocks, ptr(blocks),
                                 ptr(counts)), "aocr_layout_blocks")
    return blocks, counts, info


def label_components_device(page_dev, threshold=-1, light_text=0, connectivity=8, max_components=4096, stream=None):
    """(labels (H, W) int32: -1 on paper, on ink the smallest y*W + x of the pixel's connected component; comps (max_components, 6) int32 rows
    x0 y0 x1 y1 label area in ascending label order, the box half-open and tight; info (4) int32: threshold, total ink, components found, 0)
    as device tensors (`aocr_label_components`).  Rows of comps beyond min(info[2], max_components) are not written (they hold zeros).
    threshold -1: Otsu; connectivity 4 or 8.  Enqueues only.  stream: as for `segment_page_device`, the current torch stream; the scratch is
    freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    scratch = _scratch("aocr_components_scratch_bytes", dev, H, W)
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    comps = torch.zeros((max(int(max_components), 1), 6), dtype=torch.int32, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    check(lib.aocr_label_components(_stream(stream, dev), ptr(page_dev), pitch, H, W, int(threshold), int(light_text), int(connectivity),
                                    ptr(scratch), ptr(labels), W, int(max_components), ptr(comps), ptr(info)), "aocr_label_components")
    return labels, comps, info


def clean_page_device(page_dev, params=None, stream=None):
    """(out, counts): out a new (H, W) uint8 device tensor, the page with its specks and rules painted over by `aocr_clean_page` (every other
    byte copied), and counts (8) int32: components, specks removed, rules removed, threshold, total ink, ink pixels removed, 0, 0.  params: a
    `CleanParams` (default: Otsu, 8-connectivity, specks under 6 pixels, rules higher than 200 rows).  Enqueues only.  stream: as for
    `segment_page_device`, the current torch stream; the scratch (about 12 bytes per pixel) is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else CleanParams()
    dev = page_dev.device
    scratch = _scratch("aocr_clean_scratch_bytes", dev, H, W)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)
    check(lib.aocr_clean_page(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), ptr(scratch), ptr(out), W, ptr(counts)),
          "aocr_clean_page")
    return out, counts


def remove_rules_device(page_dev, params=None, stream=None):
    """(out, counts): out a new (H, W) uint8 device tensor, the page with its rules painted over by `aocr_remove_rules` and the strokes that
    cross them kept (every other byte copied), and counts (8) int32: threshold, total ink, pixels erased, of them at crossings of two rules,
    of them of horizontal rules, of them of vertical rules, candidate pixels kept, 0.  params: a `RuleParams` (default: Otsu, both axes, runs
    of 100 pixels, 6 thick, edge 1).  Enqueues only.  stream: as for `segment_page_device`, the current torch stream; the scratch (7 / 16 of
    a byte per pixel) is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else RuleParams()
    dev = page_dev.device
    scratch = _scratch("aocr_rules_scratch_bytes", dev, H, W)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)
    check(lib.aocr_remove_rules(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), ptr(scratch), ptr(out), W, ptr(counts)),
          "aocr_remove_rules")
    return out, counts


def invert_panels_device(page_dev, params=None, max_panels=256, stream=None):
    """(out, panels, counts): out a new (H, W) uint8 device tensor, the page with its reversed-out panels inverted by `aocr_invert_panels`
    (255 - v inside the row spans of every dark slab that carries light text, every other byte copied); panels (max_panels, 8) int32, one
    row x0 y0 x1 y1 label area hull accepted per examined candidate in label order (the rows behind them are 0); counts (8) int32:
    components, candidates found, candidates examined (min(found, max_panels)), panels inverted, threshold, total ink, the sum of the
    inverted panels' hulls, 0.  params: a `PanelParams` (default: Otsu, boxes of at least 64 x 24, 60 % filled, 2 % inside).  Enqueues only.
    stream: as for `segment_page_device`, the current torch stream; the scratch (a little over 4 bytes per pixel and 8 bytes per candidate
    and row) is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else PanelParams()
    dev = page_dev.device
    scratch = _scratch("aocr_panels_scratch_bytes", dev, H, W, int(max_panels))
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    panels = torch.zeros((int(max_panels), 8), dtype=torch.int32, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)
    check(lib.aocr_invert_panels(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), ptr(scratch), ptr(out), W, int(max_panels),
                                 ptr(panels), ptr(counts)), "aocr_invert_panels")
    return out, panels, counts


def rotate_page_device(page_dev, quarter, orient_dev=None, stream=None):
    """a new uint8 device tensor: the page turned by `aocr_rotate_page`, numpy.rot90(page, -q) with q = (quarter + (orient_dev[0] & 2)) & 3
    clockwise quarter turns: (H, W) for an even `quarter`, (W, H) for an odd one.  quarter: a Python int 0..3 (it sets the shape).  orient_dev:
    None, or an int32 device tensor whose first word may add a half turn (bit 1; read on the device: no host sync; the odd bit is ignored).
    Enqueues only.  stream: as for `segment_page_device`."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    quarter = int(quarter)
    if not 0 <= quarter <= 3:
        raise ValueError(f"quarter={quarter}: 0..3")
    if orient_dev is not None:
        assert orient_dev.dtype == torch.int32 and orient_dev.device == dev and orient_dev.numel() >= 1
        orient_dev = orient_dev.contiguous()
    Ho, Wo = (W, H) if quarter & 1 else (H, W)
    out = torch.empty((Ho, Wo), dtype=torch.uint8, device=dev)
    check(lib.aocr_rotate_page(_stream(stream, dev), ptr(page_dev), pitch, H, W, ptr(orient_dev), quarter, ptr(out), Wo), "aocr_rotate_page")
    return out


def estimate_orientation_device(page_dev, threshold=-1, light_text=0, stream=None):
    """orient (8) int32 device tensor: axis, N_h, N_v, the threshold used, the total ink, 0, 0, 0 (`aocr_estimate_orientation`).  N_h / N_v:
    the ink pixels whose left / upper neighbour is paper; axis = 1 when N_v > N_h: the lines run along y and the page wants one clockwise
    quarter turn (or three: the counts cannot tell up from down).  threshold -1: Otsu.  Enqueues only.  stream: as for
    `segment_page_device`, the current torch stream; the scratch is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    scratch = _scratch("aocr_orient_scratch_bytes", dev, H, W)
    orient = torch.zeros(8, dtype=torch.int32, device=dev)
    check(lib.aocr_estimate_orientation(_stream(stream, dev), ptr(page_dev), pitch, H, W, int(threshold), int(light_text), ptr(scratch),
                                        ptr(orient)), "aocr_estimate_orientation")
    return orient


def unrotate_points(x, y, quarter, H, W):
    """pixel (x, y) of the page turned by `quarter` clockwise quarter turns -> the pixel (x, y) of the (H, W) page it came from
    (`aocr_rotate_page`'s mapping); numpy arrays or ints."""
    q = int(quarter) & 3
    if q == 1:
        return y, H - 1 - x
    if q == 2:
        return W - 1 - x, H - 1 - y
    if q == 3:
        return W - 1 - y, x
    return x, y


def unrotate_boxes(boxes, quarter, H, W):
    """(n, 4) int64: half-open boxes x0 y0 x1 y1 on the page turned by `quarter` clockwise quarter turns (`aocr_rotate_page`), mapped back
    to the page as given; H, W: the shape of the page as given.  Host numpy."""
    b = np.asarray(boxes, np.int64)
    b = b.reshape(-1, b.shape[-1] if b.ndim > 1 else 4)[:, :4]
    x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    q = int(quarter) & 3
    H, W = int(H), int(W)
    if q == 1:
        out = [y0, H - x1, y1, H - x0]
    elif q == 2:
        out = [W - x1, H - y1, W - x0, H - y0]
    elif q == 3:
        out = [W - y1, x0, W - y0, x1]
    else:
        out = [x0, y0, x1, y1]
    return np.stack(out, axis=1).reshape(-1, 4)


def source_corners(boxes, slope_q16, H, W):
    """(n, 4, 2) int64: for every box (x0 y0 x1 y1, half-open, deskewed-page coordinates) the source-page (x, y) of its corner pixels
    (x0, y0), (x1-1, y0), (x1-1, y1-1), (x0, y1-1) under `aocr_deskew_page`'s mapping with slope_q16 (clamped like the device clamps it).
    Host numpy; the corners of a box near the rim may lie outside the source page."""
    x, y = box_corners(boxes)
    sx, sy = source_points(x, y, slope_q16, H, W)
    return np.stack([sx, sy], axis=2)


def box_corners(boxes):
    """(x, y), each (n, 4) int64: the corner pixels (x0, y0), (x1-1, y0), (x1-1, y1-1), (x0, y1-1) of half-open boxes x0 y0 x1 y1."""
    b = np.asarray(boxes, np.int64)
    b = b.reshape(-1, b.shape[-1] if b.ndim > 1 else 4)[:, :4]
    x = np.stack([b[:, 0], b[:, 2] - 1, b[:, 2] - 1, b[:, 0]], axis=1)
    y = np.stack([b[:, 1], b[:, 1], b[:, 3] - 1, b[:, 3] - 1], axis=1)
    return x, y


def source_points(x, y, slope_q16, H, W):
    """(sx, sy) int64: the source-page pixel of pixel (x, y) of the deskewed page under `aocr_deskew_page`'s mapping with slope_q16 (clamped
    like the device clamps it): `source_corners` point by point.  Integer arrays; host numpy."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    s = min(max(int(slope_q16), -16384), 16384)
    cx, cy = int(W) >> 1, int(H) >> 1
    sy = y + (((x - cx) * s + 32768) >> 16)
    sx = x - (((y - cy) * s + 32768) >> 16)
    return sx, sy


def estimate_curl_device(page_dev, params=None, stream=None, scores=False):
    """(curl (4) int32: ng, max |shift|, the threshold used, pairs with a non-zero shift; shifts (ng) int32: the rows by which the text of
    every group of 32 * group columns sits below that of the middle group) as device tensors (`aocr_estimate_curl`); with scores=True also
    scores (ng - 1, 2 * max_shift + 1) int64: every pair's correlation at every candidate shift, -max_shift first.  params: a `CurlParams`
    (default: Otsu, groups of 128 columns, shifts up to 8 rows).  Enqueues only.  stream: as for `segment_page_device`, the current torch
    stream; the scratch is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else CurlParams()
    dev = page_dev.device
    scratch = _scratch("aocr_curl_scratch_bytes", dev, H, W, params.group, params.max_shift)
    ng = -(-((W + 31) // 32) // params.group)
    curl = torch.zeros(4, dtype=torch.int32, device=dev)
    shifts = torch.zeros(ng, dtype=torch.int32, device=dev)
    sc = torch.zeros((ng - 1, 2 * params.max_shift + 1), dtype=torch.int64, device=dev) if scores else None
    check(lib.aocr_estimate_curl(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), ptr(scratch), ptr(curl), ptr(shifts),
                                 ptr(sc) if scores and sc.numel() else None), "aocr_estimate_curl")
    return (curl, shifts, sc) if scores else (curl, shifts)


def dewarp_page_device(page_dev, shifts, group, fill=255, stream=None):
    """a new (H, W) uint8 device tensor: every column of the page moved along y by its shift (`aocr_dewarp_page`: the shifts interpolated
    between the group centres in Q8, two source rows blended; `fill` where a source row is outside the page).  shifts: the (ng) int32 device
    tensor of `estimate_curl_device` (read on the device: no host sync) for the same `group`.  Enqueues only.  stream: as for
    `segment_page_device`."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    group = int(group)
    if not 1 <= group <= 16:
        raise ValueError(f"group={group}: 1..16")
    ng = -(-((W + 31) // 32) // group)
    assert isinstance(shifts, torch.Tensor) and shifts.dtype == torch.int32 and shifts.device == dev and shifts.numel() == ng, \
        f"shifts must be {ng} int32 words on the page's device"
    shifts = shifts.contiguous()
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    check(lib.aocr_dewarp_page(_stream(stream, dev), ptr(page_dev), pitch, H, W, group, ptr(shifts), int(fill), ptr(out), W), "aocr_dewarp_page")
    return out


def curl_shift_q8(x, shifts, group):
    """q(x) int64: the row shift of column x in Q8 as `aocr_dewarp_page` takes it from the group shifts (clamped to +-16384 like the device
    clamps them): flat up to the first group centre and from the last one on, between two centres interpolated with a floor division.
    x: an int array or int; host numpy."""
    s = np.clip(np.asarray(shifts, np.int64).reshape(-1), -16384, 16384)
    x = np.asarray(x, np.int64)
    group, ng = int(group), len(s)
    w, h = 32 * group, 16 * group
    j = np.clip((x - h) // w, 0, max(ng - 2, 0))
    j1 = np.minimum(j + 1, ng - 1)
    t = x - (j * w + h)
    q = 256 * s[j] + ((s[j1] - s[j]) * t * 256 + h) // w        # numpy's // floors
    q = np.where(x <= h, 256 * s[0], q)
    return np.where(x >= (ng - 1) * w + h, 256 * s[ng - 1], q)


def uncurl_points(x, y, shifts, group):
    """(x, y + q(x) / 256) float64: where `aocr_dewarp_page` with these shifts samples the page for the pixel (x, y) of the dewarped page.
    x: integer columns.  Host numpy."""
    x = np.asarray(x, np.int64)
    return x.astype(np.float64), np.asarray(y, np.float64) + curl_shift_q8(x, shifts, group) / 256.0


def estimate_page_colour_device(rgb_dev, params=None, stream=None):
    """colour (16) int32 device tensor: the paper colour p_R, p_G, p_B of an (H, W, 3) uint8 RGB page, 1, then zeros
    (`aocr_estimate_page_colour`): for every channel the value >= params.paper_min whose five-bin window of the channel's histogram holds
    the most pixels.  params: a `ColourParams` (default: paper_min 128).  Enqueues only.  stream: as for `segment_page_device`, the current
    torch stream; the scratch is freed when this returns."""
    rgb_dev, pitch = _rgb_view(rgb_dev)
    H, W, _ = rgb_dev.shape
    params = params if params is not None else ColourParams()
    dev = rgb_dev.device
    scratch = _scratch("aocr_colour_scratch_bytes", dev, H, W)
    colour = torch.zeros(16, dtype=torch.int32, device=dev)
    check(lib.aocr_estimate_page_colour(_stream(stream, dev), ptr(rgb_dev), pitch, H, W, C.byref(params), ptr(scratch), ptr(colour)),
          "aocr_estimate_page_colour")
    return colour


def gray_page_device(rgb_dev, params=None, colour=None, stream=None, counts=False):
    """a new (H, W) uint8 device tensor: the (H, W, 3) uint8 RGB page reduced to gray by `aocr_gray_page` (the paper divided out, the
    weighted sum or the darkest channel, the coloured pixels of the classes in params.drop replaced by params.fill); with counts=True
    (gray, words (16) int32: the paper used, whether it was estimated, the coloured pixels of the six hue classes, the pixels dropped, zeros).
    params: a `ColourParams` (default: luma weights, balanced, nothing dropped).  colour: the device tensor of `estimate_page_colour_device`
    (its paper is read on the device: no host sync); None: the paper of params, or, when params asks for an estimate, the estimate is
    enqueued here first.  Enqueues only.  stream: as for `segment_page_device`."""
    rgb_dev, pitch = _rgb_view(rgb_dev)
    H, W, _ = rgb_dev.shape
    params = params if params is not None else ColourParams()
    dev = rgb_dev.device
    if colour is None and params.balance and params.paper[0] < 0:
        colour = estimate_page_colour_device(rgb_dev, params, stream)
    if colour is not None:
        assert isinstance(colour, torch.Tensor) and colour.dtype == torch.int32 and colour.device == dev and colour.numel() >= 16, \
            "colour must be 16 int32 words on the page's device"
        colour = colour.contiguous()
    words = torch.empty(16, dtype=torch.int32, device=dev) if counts else None
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    check(lib.aocr_gray_page(_stream(stream, dev), ptr(rgb_dev), pitch, H, W, C.byref(params), ptr(colour), ptr(words), ptr(out), W),
          "aocr_gray_page")
    return (out, words) if counts else out


def find_page_quad_device(page_dev, threshold=-1, dark_paper=0, stream=None):
    """quad (16) int32 device tensor: x y of the corners TL, TR, BR, BL of the paper, the threshold used, the sheet's area, components found,
    valid, 0, 0, 0, 0 (`aocr_find_page_quad`): the extremes along the diagonals of the largest 8-connected component of (v > threshold), or
    of (v <= threshold) with dark_paper.  threshold -1: Otsu.  Enqueues only.  stream: as for `segment_page_device`, the current torch
    stream; the scratch (about 12 bytes per pixel) is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    scratch = _scratch("aocr_quad_scratch_bytes", dev, H, W)
    quad = torch.zeros(16, dtype=torch.int32, device=dev)
    check(lib.aocr_find_page_quad(_stream(stream, dev), ptr(page_dev), pitch, H, W, int(threshold), int(dark_paper), ptr(scratch), ptr(quad)),
          "aocr_find_page_quad")
    return quad


def rectify_plan(quad, width=0, height=0):
    """((Wo, Ho), coef (9) float64) of `aocr_rectify_plan` for the corners TL, TR, BR, BL: quad is eight ints x0 y0 .. x3 y3 or a (4, 2)
    array.  width / height 0: the lengths of the quad's longer sides.  Host only.  A quad that is not convex and clockwise, or an output
    that would be too large, raises ValueError."""
    q = np.asarray(quad).reshape(-1)
    if q.size != 8 or not np.all(q == np.round(q)) or np.any(np.abs(q) > (1 << 20)):
        raise ValueError(f"quad must be four integer (x, y) corners within +-2^20, got {quad!r}")
    q = (C.c_int32 * 8)(*[int(v) for v in q])
    size, coef = (C.c_int32 * 2)(), (C.c_double * 9)()
    if lib.aocr_rectify_plan(q, int(width), int(height), size, coef) != 0:
        from ._lib import last_error
        raise ValueError(f"aocr_rectify_plan: {last_error()}")
    return (int(size[0]), int(size[1])), np.array(list(coef), np.float64)


def warp_page_device(page_dev, coef, size, fill=255, stream=None):
    """a new (Ho, Wo) uint8 device tensor, size = (Wo, Ho): the page resampled by `aocr_warp_page` through the nine coefficients of
    `rectify_plan` (a host array: they travel in the kernel's arguments); `fill` where the source is outside the page.  Enqueues only.
    stream: as for `segment_page_device`."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    c = np.ascontiguousarray(np.asarray(coef, np.float64).reshape(-1))
    if c.size != 9:
        raise ValueError("coef must hold nine doubles")
    Wo, Ho = int(size[0]), int(size[1])
    if Wo < 1 or Ho < 1:
        raise ValueError(f"bad output size {size!r}")
    out = torch.empty((Ho, Wo), dtype=torch.uint8, device=dev)
    check(lib.aocr_warp_page(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.c_void_p(c.ctypes.data), int(fill), ptr(out), Wo, Ho, Wo),
          "aocr_warp_page")
    return out


def warp_points(coef, x, y):
    """(X, Y) float64: where `aocr_warp_page` with these coefficients samples the photograph for the pixel (x, y) of the rectified page -- the
    same expression, one numpy operation per operation (no range test: the caller sees infinities and NaNs as they come).  Host numpy."""
    c = np.asarray(coef, np.float64).reshape(-1)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        nx = (c[0] * x + c[1] * y) + c[2]
        ny = (c[3] * x + c[4] * y) + c[5]
        dn = (c[6] * x + c[7] * y) + c[8]
        return nx / dn, ny / dn


def estimate_glyph_size_device(page_dev, params=None, stream=None):
    """glyph (8) int32 device tensor: the median q_2 of min(w, h) over the tight boxes of the components that qualify as glyphs, the
    quartiles q_1 and q_3, how many qualified, components found, the threshold used, the total ink, 0 (`aocr_estimate_glyph_size`).  params:
    a `GlyphParams` (default: Otsu, dark text, 8-connectivity, sizes 2..512, aspect up to 8).  Enqueues only.  stream: as for
    `segment_page_device`, the current torch stream; the scratch (about 12 bytes per pixel) is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    params = params if params is not None else GlyphParams()
    dev = page_dev.device
    scratch = _scratch("aocr_glyph_scratch_bytes", dev, H, W)
    glyph = torch.zeros(8, dtype=torch.int32, device=dev)
    check(lib.aocr_estimate_glyph_size(_stream(stream, dev), ptr(page_dev), pitch, H, W, C.byref(params), ptr(scratch), ptr(glyph)),
          "aocr_estimate_glyph_size")
    return glyph


def resize_page_device(page_dev, size, stream=None):
    """a new (Ho, Wo) uint8 device tensor, size = (Wo, Ho): the page resampled by exact pixel areas (`aocr_resize_page`); each axis may
    shrink or grow by a factor of up to 8.  Enqueues only.  stream: as for `segment_page_device`."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    Wo, Ho = int(size[0]), int(size[1])
    if Wo < 1 or Ho < 1:
        raise ValueError(f"bad output size {size!r}")
    out = torch.empty((Ho, Wo), dtype=torch.uint8, device=dev)
    check(lib.aocr_resize_page(_stream(stream, dev), ptr(page_dev), pitch, H, W, ptr(out), Wo, Ho, Wo), "aocr_resize_page")
    return out


def scale_plan(size, n, H, W, params=None):
    """(Wo, Ho), the size to resample an H x W page to so that glyphs of `size` pixels (`estimate_glyph_size_device`'s first word, from `n`
    qualifying components) come out at params.target pixels; None when the page is to be left alone: n < params.min_glyphs, size == 0, or
    target / size within [1 / tolerance, tolerance].  Wo = round(W * target / size) in integers, (2*W*target + size) // (2*size), and Ho
    likewise; both are then clamped to what `aocr_resize_page` takes: a factor of 8 either way, 1..16384, and Ho*Wo <= 2^26 (both sides are
    shrunk by the same factor).  params: a `ScaleParams`.  Host only."""
    params = params if params is not None else ScaleParams()
    size, n, H, W = int(size), int(n), int(H), int(W)
    if n < params.min_glyphs or size <= 0:
        return None
    t = params.target
    if t <= params.tolerance * size and size <= params.tolerance * t:
        return None

    def side(L):
        v = (2 * L * t + size) // (2 * size)
        v = min(max(v, -(-L // 8)), 8 * L)
        return min(max(v, 1), 16384)

    Wo, Ho = side(W), side(H)
    if Ho * Wo > 1 << 26:
        f = math.sqrt((1 << 26) / (Ho * Wo))
        Wo, Ho = max(int(Wo * f), -(-W // 8)), max(int(Ho * f), -(-H // 8))
        while Ho * Wo > 1 << 26:                             # only when a lower bound lifted one side: take it off the longer one
            if Ho >= Wo:
                Ho -= 1
            else:
                Wo -= 1
    return Wo, Ho


def unscale_points(x, y, H, W, Ho, Wo):
    """(xs, ys) float64: the centre of pixel (x, y) of the Ho x Wo page `aocr_resize_page` made, on the H x W page it was made from:
    xs = (x + 0.5) * W / Wo - 0.5, and likewise for y.  Host numpy."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return (x + 0.5) * W / Wo - 0.5, (y + 0.5) * H / Ho - 0.5


def backmap_corners(boxes, curl=None, skew=None, turn=None, resize=None, warp=None):
    """The corner fields of `Model.recognize_page`: the corner pixels of the final page's boxes carried back through every stage that ran,
    in the one order the stages have: curl, shear, quarter turn, resize, perspective warp.  Host numpy; a dict of (n, 4, 2) arrays
    ((n, 4) for source_boxes) holding only the fields of the stages given.  boxes: (n, >= 4) x0 y0 x1 y1, half-open.  Each stage is None when
    it was not asked for, else what it left behind:
    curl = (shifts, group): uncurled_corners, float64 `uncurl_points` of `box_corners(boxes)`; the later stages go on from them as int64
    with y rounded half up, floor(y + 0.5).
    skew = (slope_q16, H, W), H x W the final page: source_corners, int64 `source_points` of those corners, with a turn carried through
    `unrotate_points` afterwards.
    turn = (quarter, H0, W0), H0 x W0 the page before the turn: source_boxes, `unrotate_boxes(boxes, ...)`, which ignores shear and curl.
    resize = (H, W, Ho, Wo), the page before and after `aocr_resize_page`, or () when the plan left the page alone: unscaled_corners,
    float64 `unscale_points` of the incoming corners (() : the incoming corners).
    warp = the nine coefficients of `rectify_plan`, or () when no sheet was used: photo_corners, float64 `warp_points` of the corners
    that the resize put out (() : those corners).
    The corners entering resize and warp are source_corners with skew; otherwise, with curl, the rounded uncurled corners carried through
    `unrotate_points`; otherwise the corner pixels of source_boxes (of boxes without a turn).  The last case takes the corners of the
    un-rotated BOX, the one before un-rotates the corner POINTS: for an odd quarter turn the two list the same four pixels in a different
    order.  That is how recognize_page has always published them, and it is kept."""
    out = {}
    x, y = box_corners(boxes)
    if curl is not None:
        ux, uy = uncurl_points(x, y, *curl)
        out["uncurled_corners"] = np.stack([ux, uy], axis=2)
        x, y = ux.astype(np.int64), np.floor(uy + 0.5).astype(np.int64)
    if skew is not None:
        x, y = source_points(x, y, *skew)
    if turn is not None:
        out["source_boxes"] = unrotate_boxes(boxes, *turn)
        x, y = unrotate_points(x, y, *turn) if curl is not None or skew is not None else box_corners(out["source_boxes"])
    if skew is not None:
        out["source_corners"] = np.stack([x, y], axis=2)
    if resize is not None or warp is not None:
        x, y = x.astype(np.float64), y.astype(np.float64)
    if resize is not None:
        if len(resize):
            x, y = unscale_points(x, y, *resize)
        out["unscaled_corners"] = np.stack([x, y], axis=2)
    if warp is not None:
        if len(warp):
            x, y = warp_points(warp, x, y)
        out["photo_corners"] = np.stack([x, y], axis=2)
    return out


def estimate_slant_device(page_dev, boxes, counts, params=None, threshold_dev=None, stream=None, scores=False):
    """slant (n_boxes, 4) int32 device tensor: for every box the winning candidate k, its slant k * step_q16 (columns per row, Q16; positive:
    the strokes lean to the right), a flag (0 estimated, 1 taller than 256 rows and left alone, 2 empty) and the ink pixels of the box
    (`aocr_estimate_slant`); with scores=True (slant, scores (n_boxes, 2 * n_steps + 1) int64: every candidate's score, k = -n_steps
    first).  Rows >= min(n_boxes, counts[0]) are not written (they hold zeros).  boxes (n_boxes, 6) int32 and counts (>= 1) int32 device
    tensors as `segment_page_device` returns them; counts None: every row of boxes.  params: a `SlantParams` (default: +-12 steps of 1/16
    column per row); with threshold -1 the threshold is read on the device from threshold_dev[0], and threshold_dev None then takes
    counts[2:3], the word `aocr_segment_page` left there.  Enqueues only.  stream: as for `segment_page_device`, the current torch stream;
    the scratch is freed when this returns."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    params = params if params is not None else SlantParams()
    assert boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.dtype == torch.int32 and boxes.device == dev
    boxes = boxes.contiguous()
    n = int(boxes.shape[0])
    if counts is not None:
        assert counts.dtype == torch.int32 and counts.device == dev and counts.numel() >= 1
        counts = counts.contiguous()
    if threshold_dev is None and params.threshold < 0:
        if counts is None or counts.numel() < 3:
            raise ValueError("threshold -1 needs threshold_dev, or the counts of segment_page_device")
        threshold_dev = counts[2:3]
    if threshold_dev is not None:
        assert threshold_dev.dtype == torch.int32 and threshold_dev.device == dev and threshold_dev.numel() >= 1
        threshold_dev = threshold_dev.contiguous()
    nc = 2 * params.n_steps + 1
    slant = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    sc = torch.zeros((n, nc), dtype=torch.int64, device=dev) if scores else None
    scratch = _scratch("aocr_slant_scratch_bytes", dev, n, params.n_steps)
    check(lib.aocr_estimate_slant(_stream(stream, dev), ptr(page_dev), pitch, H, W, ptr(boxes), ptr(counts), n, C.byref(params), ptr(threshold_dev),
                                  ptr(scratch), ptr(slant), ptr(sc) if scores and n else None), "aocr_estimate_slant")
    return (slant, sc) if scores else slant


def crop_lines_slanted_device(page_dev, boxes, counts, slant, out_w, out_h=IMG_H, fill=255, stream=None):
    """`crop_lines_device` with the slant taken out (`aocr_crop_lines_slanted`): row i is box i of the page, every row of the box moved along x
    by its offset, widened by `slant_extent` on either side and filled with `fill` where the source column is outside the box, scaled as
    `aocr_preprocess_lines` scales it.  slant: the (n_boxes, 4) int32 device tensor of `estimate_slant_device` (word 1 of every row is read
    on the device: no host sync), or None: the plain crops, bit for bit.  Enqueues only.  stream: as for `segment_page_device`."""
    page_dev, pitch = _page_view(page_dev)
    H, W = page_dev.shape
    dev = page_dev.device
    assert boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.dtype == torch.int32 and boxes.device == dev
    boxes = boxes.contiguous()
    n = int(boxes.shape[0])
    if counts is not None:
        assert counts.dtype == torch.int32 and counts.device == dev and counts.numel() >= 1
        counts = counts.contiguous()
    if slant is not None:
        assert slant.dtype == torch.int32 and slant.device == dev and tuple(slant.shape) == (n, 4), f"slant must be ({n}, 4) int32 on the page's device"
        slant = slant.contiguous()
    out = torch.full((n, 1, int(out_h), int(out_w)), 255.0, dtype=torch.float32, device=dev)
    if n:
        check(lib.aocr_crop_lines_slanted(_stream(stream, dev), ptr(page_dev), pitch, H, W, ptr(boxes), ptr(counts), n, ptr(slant), int(fill),
                                          int(out_h), int(out_w), ptr(out)), "aocr_crop_lines_slanted")
    return out


def slant_extent(boxes, slant_q16):
    """D (n) int32: how many columns `aocr_crop_lines_slanted` adds on either side of every box, max(|off(y0)|, |off(y1 - 1)|) with
    off(y) = ((cy - y) * s + 32768) >> 16, cy = (y0 + y1) >> 1 and s the slant clamped to +-65536; 0 for an empty box.  boxes (n, >= 4)
    x0 y0 x1 y1 inside the page (what `aocr_segment_page` writes); host numpy."""
    b = np.asarray(boxes, np.int64)
    b = b.reshape(-1, b.shape[-1] if b.ndim > 1 else 4)
    s = np.clip(np.asarray(slant_q16, np.int64).reshape(-1), -65536, 65536)
    y0, y1 = b[:, 1], b[:, 3]
    cy = (y0 + y1) >> 1
    d = np.maximum(np.abs(((cy - y0) * s + 32768) >> 16), np.abs(((cy - (y1 - 1)) * s + 32768) >> 16))
    return np.where((y1 > y0) & (b[:, 2] > b[:, 0]), d, 0).astype(np.int32)


def bucket_width(w, h, max_img_w, width_step=32, max_aspect=None):
    """DataGen's width rule for a w x h box, ceil(clamp(w/h, 0.5, max_aspect) * 32), rounded up to a multiple of width_step and capped at
    max_img_w.  max_aspect None: max_img_w / 32."""
    max_aspect = max_aspect if max_aspect is not None else max_img_w / IMG_H
    aspect = max(min(w / h, max_aspect), MIN_ASPECT)
    img_w = int(math.ceil(aspect * IMG_H))
    img_w = -(-img_w // width_step) * width_step
    return min(img_w, int(max_img_w))


__all__ = ["backmap_corners", "SpacingParams", "segment_page_spaced_device", "SlantParams", "estimate_slant_device", "crop_lines_slanted_device", "slant_extent", "ColourParams", "estimate_page_colour_device", "gray_page_device", "CurlParams", "estimate_curl_device", "dewarp_page_device", "curl_shift_q8", "uncurl_points", "source_points", "box_corners", "GlyphParams", "ScaleParams", "estimate_glyph_size_device", "resize_page_device", "scale_plan", "unscale_points", "RectifyParams", "find_page_quad_device", "rectify_plan", "warp_page_device", "warp_points", "SegmentParams", "SkewParams", "FlattenParams", "LayoutParams", "CleanParams", "Box", "label_components_device", "clean_page_device", "segment_page_device", "crop_lines_device",
           "estimate_skew_device", "deskew_page_device", "flatten_page_device", "BinarizeParams", "binarize_page_device", "ink_integral_device", "layout_page_device", "source_corners",
           "rotate_page_device", "estimate_orientation_device", "unrotate_boxes", "unrotate_points", "bucket_width"]
