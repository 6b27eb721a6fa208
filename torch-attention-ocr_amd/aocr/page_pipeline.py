"""The stage chain of `Model.recognize_page` in front of the recogniser, as plain functions of the page: colour, rectify, flatten, binarize, scale, panels,
clean and the quarter turn (one function each, in that order), then `page_boxes`: deskew, dewarp, rule removal, layout and segmentation down to
the boxes on the host.  Every function takes the page on the device, the raw handle of the current torch stream and the page's resolved `SegmentParams`,
enqueues on that stream, and returns the page with a small record of what it did (None when the stage was not asked for).  What needs a
model -- the which-way-up probe, the crop-and-recognise loop, the lexicon -- stays in `Model`; the way back from box corners to the page as
given is `aocr.page.backmap_corners`."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .page import (binarize_page_device, clean_page_device, invert_panels_device, deskew_page_device, estimate_slant_device, dewarp_page_device, estimate_curl_device, estimate_glyph_size_device,
                   estimate_orientation_device, gray_page_device, estimate_skew_device, find_page_quad_device, flatten_page_device, layout_page_device,
                   rectify_plan, remove_rules_device, resize_page_device, rotate_page_device, scale_plan, segment_page_device, segment_page_spaced_device, warp_page_device)

MAX_BLOCKS = 256
MAX_PANELS = 256


def asked(option):
    """whether a stage option of recognize_page asks for its stage: anything but None and False."""
    return option is not None and option is not False


def paper(seg):
    """the gray level of paper, what a resampling stage fills with outside the page."""
    return 0 if seg.light_text else 255


def read_named(pieces):
    """One readback of many small results: `pieces` maps names to int32 device tensors, lists of them, or None.  The pieces that are not
    None are flattened and joined in the mapping's order by ONE torch.cat(...).cpu() -- one sync -- and come back as a dict from name to
    numpy view (a list's tensors as one view, end to end); names given as None are absent."""
    parts = {k: [t.reshape(-1) for t in (v if isinstance(v, (list, tuple)) else [v])] for k, v in pieces.items() if v is not None}
    host = torch.cat([t for ts in parts.values() for t in ts]).cpu().numpy()
    out, at = {}, 0
    for k, ts in parts.items():
        n = sum(t.numel() for t in ts)
        out[k], at = host[at:at + n], at + n
    return out


def colour_stage(page, stream, seg, colour):
    """(gray page, the sixteen colour words on the device: they come back with the boxes' readback, the ColourParams used) of an (H, W, 3) RGB
    page.  colour True:
    the defaults, filled with paper; with light text the page is not balanced (its most frequent colour is no paper to divide by)."""
    if not asked(colour):
        return page, None, None
    cp = colour if isinstance(colour, _lib.ColourParams) else _lib.ColourParams(fill=paper(seg), balance=0 if seg.light_text else 1)
    return gray_page_device(page, cp, None, stream, counts=True) + (cp,)


def rectify_stage(page, stream, seg, rectify):
    """(page, rect): rect.used, quad, size, area as recognize_page publishes them; rect.warp the nine coefficients, () when no sheet was used."""
    if not asked(rectify):
        return page, None
    rect = SimpleNamespace(used=False, quad=None, size=None, area=None, warp=())
    if rectify is True or isinstance(rectify, _lib.RectifyParams):
        rp = rectify if isinstance(rectify, _lib.RectifyParams) else _lib.RectifyParams(dark_paper=seg.light_text)
        words = find_page_quad_device(page, rp.threshold, rp.dark_paper, stream).cpu().numpy()         # the additional sync
        rect.area = int(words[9])
        if rect.area > 0:
            rect.quad = words[:8].reshape(4, 2).astype(np.int64)
        rect.used = bool(words[11]) and rect.area * 100 >= rp.min_area_percent * int(page.shape[0]) * int(page.shape[1])
    else:
        rp = _lib.RectifyParams(dark_paper=seg.light_text)
        q = np.asarray(rectify)
        if q.shape != (4, 2) or not np.all(q == np.round(q)):
            raise ValueError(f"rectify={rectify!r}: None, False, True, an aocr.RectifyParams or four integer (x, y) corners TL, TR, BR, BL")
        rect.quad, rect.used = q.astype(np.int64), True
    if rect.used:
        rect.size, rect.warp = rectify_plan(rect.quad, rp.width, rp.height)
        page = warp_page_device(page, rect.warp, rect.size, rp.fill if rp.fill is not None else paper(seg), stream)
    return page, rect


def flatten_stage(page, stream, seg, flatten):
    """(page, the FlattenParams used)."""
    if not asked(flatten):
        return page, None
    flat = flatten if isinstance(flatten, _lib.FlattenParams) else _lib.FlattenParams(light_text=seg.light_text)
    return flatten_page_device(page, flat, stream), flat


def binarize_stage(page, stream, seg, binarize):
    """(page, the BinarizeParams used, the four count words on the device: they come back with the boxes' readback).  Directly after the
    flatten stage, which takes strong shading out first, and before the scale stage: the pixel values change and no geometry does, so
    there is nothing to map back.  binarize True: the defaults with the light_text of the segment params."""
    if not asked(binarize):
        return page, None, None
    if isinstance(binarize, _lib.BinarizeParams):
        bp = binarize
    elif binarize is True:
        bp = _lib.BinarizeParams(light_text=seg.light_text)
    else:
        raise ValueError(f"binarize={binarize!r}: None, False, True or an aocr.BinarizeParams")
    page, counts_dev = binarize_page_device(page, bp, stream, counts=True)
    return page, bp, counts_dev


def binarized_params(seg):
    """the segment params of the stages behind binarize_stage: a copy, with the fixed threshold 127 -- the local decision on the binarised
    page -- in the place of Otsu (-1), which could land below 127 on the output and drop faint ink.  A fixed threshold is the caller's."""
    if seg.threshold >= 0:
        return seg
    fixed = _lib.SegmentParams(*[getattr(seg, f) for f, _ in seg._fields_][:9])
    fixed.threshold = 127
    return fixed


def scale_stage(page, stream, seg, scale):
    """(page, scl): scl.shape, size, quartiles, glyphs as recognize_page publishes them; scl.resize (H, W, Ho, Wo), the page before and
    after, () when the page was left alone."""
    if not asked(scale):
        return page, None
    H, W = int(page.shape[0]), int(page.shape[1])
    scl = SimpleNamespace(shape=None, size=None, quartiles=None, glyphs=None, resize=())
    if scale is True or isinstance(scale, _lib.ScaleParams):
        sp = scale if isinstance(scale, _lib.ScaleParams) else _lib.ScaleParams(_lib.GlyphParams(threshold=seg.threshold, light_text=seg.light_text))
        words = estimate_glyph_size_device(page, sp.glyph, stream).cpu().numpy()                      # the additional sync
        scl.size, scl.quartiles, scl.glyphs = int(words[0]), (int(words[1]), int(words[2])), int(words[3])
        scl.shape = scale_plan(scl.size, scl.glyphs, H, W, sp)
    else:
        ok = isinstance(scale, (int, float, np.integer, np.floating)) and not isinstance(scale, bool)
        if not (ok and math.isfinite(float(scale)) and float(scale) > 0):
            raise ValueError(f"scale={scale!r}: None, False, True, an aocr.ScaleParams or a positive ratio")
        scl.shape = (max(int(math.floor(W * float(scale) + 0.5)), 1), max(int(math.floor(H * float(scale) + 0.5)), 1))
    if scl.shape is not None:
        page, scl.resize = resize_page_device(page, scl.shape, stream), (H, W, scl.shape[1], scl.shape[0])
    return page, scl


def panels_stage(page, stream, seg, panels):
    """(page, [the eight panel counts, the MAX_PANELS panel rows] on the device: they come back with the boxes' readback).  After the scale
    stage (min_w and min_h are pixels at the normalised size) and before the clean stage, which then sees the text of an inverted slab
    and not the slab, a figure to paint over.  panels True: the defaults with the threshold and light_text of the segment params."""
    if not asked(panels):
        return page, None
    if isinstance(panels, _lib.PanelParams):
        pp = panels
    elif panels is True:
        pp = _lib.PanelParams(threshold=seg.threshold, light_text=seg.light_text)
    else:
        raise ValueError(f"panels={panels!r}: None, False, True or an aocr.PanelParams")
    page, rows_dev, counts_dev = invert_panels_device(page, pp, MAX_PANELS, stream)
    return page, [counts_dev, rows_dev]


def clean_stage(page, stream, seg, clean):
    """(page, the eight clean counts on the device: they come back with the boxes' readback)."""
    if not asked(clean):
        return page, None
    cp = clean if isinstance(clean, _lib.CleanParams) else _lib.CleanParams(threshold=seg.threshold, light_text=seg.light_text)
    return clean_page_device(page, cp, stream)


def orient_stage(page, stream, seg, orient):
    """(page, quarter, runs): the clockwise quarter turns applied, and (N_h, N_v) when they were estimated (orient=True)."""
    if not asked(orient):
        return page, None, None
    runs = None
    if orient is True:
        words = estimate_orientation_device(page, seg.threshold, seg.light_text, stream).cpu().numpy()    # the additional sync
        quarter, runs = int(words[0]), (int(words[1]), int(words[2]))
    else:
        quarter = int(orient)
        if not 0 <= quarter <= 3:
            raise ValueError(f"orient={orient!r}: None, False, True or 0..3 clockwise quarter turns")
    return rotate_page_device(page, quarter, None, stream), quarter, runs


def slant_params(seg, deslant, threshold=-1):
    """the SlantParams of recognize_page(deslant=...): True takes the defaults with the light_text of the segment params; `threshold` replaces
    a params' -1 where the page threshold is already on the host (the layout path)."""
    if isinstance(deslant, _lib.SlantParams):
        sp = _lib.SlantParams(deslant.threshold, deslant.light_text, deslant.step_q16, deslant.n_steps)
    elif deslant is True:
        sp = _lib.SlantParams(light_text=seg.light_text)
    else:
        raise ValueError(f"deslant={deslant!r}: None, False, True or an aocr.SlantParams")
    if sp.threshold < 0:
        sp.threshold = int(threshold)
    return sp


def spacing_params(spacing):
    """the SpacingParams of recognize_page(spacing=...): True takes the defaults."""
    if isinstance(spacing, _lib.SpacingParams):
        return spacing
    if spacing is True:
        return _lib.SpacingParams()
    raise ValueError(f"spacing={spacing!r}: None, False, True or an aocr.SpacingParams")


def rule_params(seg, rules):
    """the RuleParams of recognize_page(rules=...): True takes the defaults with the threshold and light_text of the segment params."""
    if isinstance(rules, _lib.RuleParams):
        return rules
    if rules is True:
        return _lib.RuleParams(threshold=seg.threshold, light_text=seg.light_text)
    raise ValueError(f"rules={rules!r}: None, False, True or an aocr.RuleParams")


def page_boxes(page, stream, seg, max_boxes, deskew, dewarp, layout, clean_dev, colour_dev=None, deslant=None, spacing=None, rules=None, panels_dev=None,
               binarize_dev=None):
    """the middle of recognize_page, from the deskew to the boxes on the host: everything that reads the page in its final orientation and
    has to be redone when recognize_page(orient=True) turns the page by another half turn.  Returns a namespace: page, boxes_dev, rows, counts,
    n, truncated; skew, cleaned, curl, colour (the words read back, None without the stage), curl_group; lay, blocks, block_id, nb, lcounts
    (None without layout); slant (n, 4) and slant_dev, the words of aocr_estimate_slant for the boxes kept (None without deslant).  The
    slant estimate is enqueued right after the segmentation, on the page that was segmented, and its words come back with the boxes: no
    readback of its own.  spacing (n_lines, 8): the rows of aocr_segment_page_spaced, which then takes the place of aocr_segment_page (None
    without spacing); they too come back with the boxes.  rules: aocr_remove_rules after the deskew and the dewarp (a rule is a pure row run
    only on a straight page) and before layout and segmentation (a column-separator rule sits in the gutter the XY cut looks for); st.page
    is then the page with the rules taken out, st.rules its eight counts, which ride with the first readback (None without rules).
    panels_dev: what panels_stage left on the device, one more rider of the first readback; st.panels is then its words end to end, the
    eight counts and the MAX_PANELS rows of eight (None without the stage).  binarize_dev: the four count words binarize_stage left on the
    device, another rider of the first readback; st.binarize is then those words (None without the stage)."""
    st = SimpleNamespace(curl_group=None, lay=None, blocks=None, block_id=None, nb=None, lcounts=None, slant=None, slant_dev=None, spacing=None)
    skew_dev = curl_dev = rules_dev = None
    ruled = rule_params(seg, rules) if asked(rules) else None
    spaced = spacing_params(spacing) if asked(spacing) else None

    def segment(view, params):
        """(boxes, counts, spacing rows or None) of a page or a block"""
        if spaced is None:
            return segment_page_device(view, params, max_boxes, stream) + (None,)
        return segment_page_spaced_device(view, params, spaced, max_boxes, stream)
    if asked(deskew):
        sp = deskew if isinstance(deskew, _lib.SkewParams) else _lib.SkewParams(threshold=seg.threshold, light_text=seg.light_text)
        skew_dev = estimate_skew_device(page, sp, stream)
        page = deskew_page_device(page, skew_dev, paper(seg), stream)
    if asked(dewarp):
        cp = dewarp if isinstance(dewarp, _lib.CurlParams) else _lib.CurlParams(threshold=seg.threshold, light_text=seg.light_text)
        words_dev, shifts_dev = estimate_curl_device(page, cp, stream)
        page = dewarp_page_device(page, shifts_dev, cp.group, paper(seg), stream)
        curl_dev, st.curl_group = [words_dev, shifts_dev], int(cp.group)      # the four curl words, then the ng group shifts
    if ruled is not None:
        page, rules_dev = remove_rules_device(page, ruled, stream)
    st.page = page
    riders = dict(skew=skew_dev, cleaned=clean_dev, curl=curl_dev, colour=colour_dev, rules=rules_dev, panels=panels_dev, binarize=binarize_dev)            # what comes back with the first readback, whichever it is
    if asked(layout):
        st.lay = layout if isinstance(layout, _lib.LayoutParams) else _lib.LayoutParams()
        blocks_dev, lcounts_dev, info_dev = layout_page_device(page, st.lay, seg.threshold, seg.light_text, MAX_BLOCKS, stream)
        got = read_named(dict(lcounts=lcounts_dev, info=info_dev, **riders, blocks=blocks_dev))             # the first sync
        st.lcounts, info = got["lcounts"], got["info"]
        st.nb = nb = int(st.lcounts[0])
        st.blocks = got["blocks"].reshape(MAX_BLOCKS, 6)[:nb]
        block_seg = _lib.SegmentParams(*[getattr(seg, f) for f, _ in seg._fields_][:9])
        block_seg.threshold = int(info[0])                        # the page's threshold: every block thresholds like the whole page
        per = [segment(page[b[1]:b[3], b[0]:b[2]], block_seg) for b in st.blocks.tolist()]
        if nb:
            all_boxes = torch.stack([bx for bx, _, _ in per])                       # (nb, max_boxes, 6)
            all_counts = torch.stack([c for _, c, _ in per])                        # (nb, 4)
            all_boxes[:, :, :4] += blocks_dev[:nb][:, [0, 1, 0, 1]][:, None, :]
            lines_dev = all_counts[:, 1]
            all_boxes[:, :, 4] += (torch.cumsum(lines_dev, 0) - lines_dev).to(torch.int32)[:, None]
            slants = []
            if asked(deslant):                                  # per block, its boxes in page coordinates against the whole page
                sp = slant_params(seg, deslant, int(info[0]))
                slants = [estimate_slant_device(page, all_boxes[b], all_counts[b], sp, None, stream).reshape(-1) for b in range(nb)]
            all_boxes = all_boxes.reshape(-1, 6)
            gaps = [r.reshape(-1) for _, _, r in per] if spaced is not None else []     # per block (block height + 1) // 2 rows of 8
            back = torch.cat([all_counts.reshape(-1), all_boxes.reshape(-1)] + slants + gaps).cpu().numpy()     # the second sync
            bcounts = back[:4 * nb].reshape(nb, 4)
            taken = np.minimum(bcounts[:, 0], max_boxes)
            keep = np.concatenate([b * max_boxes + np.arange(t) for b, t in enumerate(taken.tolist())]).astype(np.int64)
            st.rows = back[4 * nb:4 * nb + 6 * nb * max_boxes].reshape(-1, 6)[keep]
            keep_dev = torch.from_numpy(keep).to(page.device)
            st.boxes_dev = all_boxes[keep_dev]
            if slants:
                st.slant = back[4 * nb + 6 * nb * max_boxes:4 * nb + 10 * nb * max_boxes].reshape(-1, 4)[keep]
                st.slant_dev = torch.cat(slants).reshape(-1, 4)[keep_dev]
            if gaps:                                            # the lines of the blocks end to end, as the line numbers run
                tail = back[len(back) - sum(g.numel() for g in gaps):].reshape(-1, 8)
                starts = np.cumsum([0] + [g.numel() // 8 for g in gaps[:-1]])
                st.spacing = np.concatenate([tail[s0:s0 + n] for s0, n in zip(starts.tolist(), bcounts[:, 1].tolist())])
            st.block_id = np.repeat(np.arange(nb, dtype=np.int32), taken)
        else:
            bcounts = np.zeros((0, 4), np.int32)
            st.rows, st.block_id = np.zeros((0, 6), np.int32), np.zeros(0, np.int32)
            st.boxes_dev = torch.zeros((0, 6), dtype=torch.int32, device=page.device)
            if asked(deslant):
                slant_params(seg, deslant)
                st.slant, st.slant_dev = np.zeros((0, 4), np.int32), torch.zeros((0, 4), dtype=torch.int32, device=page.device)
            if spaced is not None:
                st.spacing = np.zeros((0, 8), np.int32)
        st.n = len(st.rows)
        st.counts = np.array([bcounts[:, 0].sum(), bcounts[:, 1].sum(), info[0], 0], np.int64)
        st.truncated = bool((bcounts[:, 0] > max_boxes).any())
    else:
        st.boxes_dev, counts_dev, gaps_dev = segment(page, seg)
        if asked(deslant):                                      # the threshold is the device word counts_dev[2] unless the params fix one
            st.slant_dev = estimate_slant_device(page, st.boxes_dev, counts_dev, slant_params(seg, deslant), counts_dev[2:3], stream)
        if all(v is None for v in riders.values()):
            got = dict(counts=counts_dev.cpu().numpy())           # nothing rides along: the counts as they are, no torch.cat
        else:
            got = read_named(dict(counts=counts_dev, **riders))
        st.counts = got["counts"]
        st.n = int(min(st.counts[0], max_boxes))
        if st.slant_dev is None and gaps_dev is None:
            st.rows = st.boxes_dev[:st.n].cpu().numpy()
        else:                                                   # the slant words and the spacing rows ride with the boxes
            lines = int(st.counts[1])
            parts = [st.boxes_dev[:st.n].reshape(-1)]
            if st.slant_dev is not None:
                st.slant_dev = st.slant_dev[:st.n]
                parts.append(st.slant_dev.reshape(-1))
            if gaps_dev is not None:
                parts.append(gaps_dev[:lines].reshape(-1))
            back = torch.cat(parts).cpu().numpy()
            st.rows, at = back[:6 * st.n].reshape(-1, 6), 6 * st.n
            if st.slant_dev is not None:
                st.slant, at = back[at:at + 4 * st.n].reshape(-1, 4), at + 4 * st.n
            if gaps_dev is not None:
                st.spacing = back[at:at + 8 * lines].reshape(-1, 8)
        st.truncated = bool(st.counts[0] > max_boxes)
    st.skew, st.cleaned, st.curl, st.colour, st.rules = got.get("skew"), got.get("cleaned"), got.get("curl"), got.get("colour"), got.get("rules")
    st.panels, st.binarize = got.get("panels"), got.get("binarize")
    return st
