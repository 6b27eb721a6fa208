"""The stage chain of Model.recognize_page in numpy, written from its docstring on top of the stage restatements of this directory
(tests/*_ref.py): colour, rectify, flatten, binarize, scale, panels, clean, the quarter turn, deskew, dewarp, rules, layout, segmentation,
slant.  No device, no torch, and it does not import aocr.page_pipeline; the corner fields come from tests/backmap_ref.py, which is imported
only when they are asked for.

Options are plain values: None / False (the stage is off), True (the stage's defaults, resolved from the segment parameters as the
docstring says) or a dict of the stage's parameters, which is then used as given (what it leaves out takes the restatement's defaults, the
library's own).  rectify also takes four (x, y) corners, scale a positive ratio, orient 0..3 quarter turns.  `seg` is a dict of
segment_ref's parameters.  Two options are not stages: max_boxes (1024) and half_turn (False): with orient=True, the further half turn
that recognize_page takes when its recogniser scores the flipped crops higher -- the pages up to `clean` are kept and everything behind
the quarter turn is done on the page turned by estimate + 2."""
import math
from types import SimpleNamespace

import numpy as np

import binarize_ref as BR
import colour_ref as CO
import components_ref as CC
import curl_ref as CU
import flatten_ref as FL
import layout_ref as LA
import orient_ref as OR
import panels_ref as PA
import rectify_ref as RE
import rules_ref as RU
import scale_ref as SC
import segment_ref as SG
import skew_ref as SK
import slant_ref as SL
import spacing_ref as SP

STAGES = ("colour", "rectify", "flatten", "binarize", "scale", "panels", "clean", "orient", "deskew", "dewarp", "rules")
MAX_BLOCKS = 256
MAX_PANELS = 256
RECTIFY = dict(threshold=-1, dark_paper=0, width=0, height=0, min_area_percent=10, fill=None)        # aocr.RectifyParams
SKEW = dict(threshold=-1, light_text=0, step_q16=64, n_steps=96)                                     # aocr.SkewParams
CURL = dict(threshold=-1, light_text=0, group=4, max_shift=8, min_ink=64)                            # aocr.CurlParams
SLANT = dict(threshold=-1, light_text=0, step_q16=4096, n_steps=12)                                  # aocr.SlantParams


def asked(option):
    return option is not None and option is not False


def _given(option, defaults, **inherited):
    """a dict is used as given over the defaults; True takes the defaults with what the stage inherits from the segment parameters."""
    p = dict(defaults)
    p.update(option if isinstance(option, dict) else inherited)
    return p


def read_page_ref(page, seg, options):
    """Returns a namespace: pages (stage name -> the page after it, in the order the stages ran; "final" is the page that was segmented),
    words (stage name -> the words the stage reports), rows (n, 6) int32 x0 y0 x1 y1 line ink, counts (found, lines, threshold),
    truncated, blocks (nb, 6) / block_id / lcounts / n_block_lines (None without layout), slant (n, 4) and extent (n) (None without
    deslant), spacing (n_lines, 8) in line order across the blocks (None without spacing), quarter, turn, resize, warp, shape, size, quad,
    area, rectified, and corners(), the corner fields of the boxes."""
    o = dict(options)
    seg = dict(SG.DEFAULTS, **seg)
    light = int(seg["light_text"])
    paper = 0 if light else 255
    max_boxes = int(o.get("max_boxes", 1024))
    r = SimpleNamespace(pages={}, words={}, blocks=None, block_id=None, lcounts=None, n_block_lines=None, slant=None, extent=None, spacing=None,
                        quarter=None, turn=None, resize=None, warp=None, shape=None, size=None, quad=None, area=None, rectified=None,
                        curl_group=None, params={})
    page = np.asarray(page)
    # 1. colour
    if asked(o.get("colour")):
        assert page.ndim == 3 and page.shape[2] == 3 and page.dtype == np.uint8
        cp = _given(o["colour"], CO.DEFAULTS, fill=paper, balance=0 if light else 1)
        page, r.words["colour"] = CO.gray(page, **cp)
        r.pages["colour"], r.params["colour"] = page, cp
    assert page.ndim == 2 and page.dtype == np.uint8
    # 2. rectify
    rect = o.get("rectify")
    if asked(rect):
        r.rectified, r.warp = False, ()
        if rect is True or isinstance(rect, dict):
            rp = _given(rect, RECTIFY, dark_paper=light)
            words = RE.find_page_quad(page, rp["threshold"], rp["dark_paper"])
            r.words["rectify"], r.area = words, int(words[9])
            if r.area > 0:
                r.quad = words[:8].reshape(4, 2).astype(np.int64)
            r.rectified = bool(words[11]) and r.area * 100 >= rp["min_area_percent"] * page.shape[0] * page.shape[1]
        else:
            rp = dict(RECTIFY, dark_paper=light)
            r.quad, r.rectified = np.asarray(rect).astype(np.int64).reshape(4, 2), True
        if r.rectified:
            r.size, r.warp = RE.rectify_plan(r.quad, rp["width"], rp["height"])
            page = RE.warp_page(page, r.warp, rp["fill"] if rp["fill"] is not None else paper, r.size[1], r.size[0])
        r.pages["rectify"] = page
    # 3. flatten
    if asked(o.get("flatten")):
        fp = _given(o["flatten"], dict(radius=16, light_text=0), light_text=light)
        page = FL.flatten(page, **fp)
        r.pages["flatten"], r.params["flatten"] = page, fp
    # 4. binarize, then the fixed threshold of its output in the place of Otsu
    if asked(o.get("binarize")):
        bp = _given(o["binarize"], BR.DEFAULTS, light_text=light)
        page, r.words["binarize"] = BR.binarize(page, **bp)
        r.pages["binarize"], r.params["binarize"] = page, bp
        if seg["threshold"] < 0:
            seg = dict(seg, threshold=127)
    thr = int(seg["threshold"])
    # 5. scale
    scale = o.get("scale")
    if asked(scale):
        H, W = page.shape
        r.resize = ()
        if scale is True or isinstance(scale, dict):
            sp = dict(scale) if isinstance(scale, dict) else {}
            glyph = dict(SC.GLYPH_DEFAULTS, **sp.pop("glyph")) if "glyph" in sp else dict(SC.GLYPH_DEFAULTS, threshold=thr, light_text=light)
            words = SC.estimate_glyph_size(page, **glyph)
            r.words["scale"] = words
            r.shape = SC.scale_plan(int(words[0]), int(words[3]), H, W, **sp)
        else:
            r.shape = (max(int(math.floor(W * float(scale) + 0.5)), 1), max(int(math.floor(H * float(scale) + 0.5)), 1))
        if r.shape is not None:
            page, r.resize = SC.resize_page(page, r.shape[1], r.shape[0]), (H, W, r.shape[1], r.shape[0])
        r.pages["scale"] = page
    # 6. panels
    if asked(o.get("panels")):
        pp = _given(o["panels"], PA.DEFAULTS, threshold=thr, light_text=light)
        page, rows, counts = PA.invert_panels(page, MAX_PANELS, **pp)
        r.words["panels"], r.words["panel_rows"] = counts, rows
        r.pages["panels"] = page
    # 7. clean
    if asked(o.get("clean")):
        cp = _given(o["clean"], CC.DEFAULTS, threshold=thr, light_text=light)
        page, r.words["clean"] = CC.clean_page(page, **cp)
        r.pages["clean"] = page
    page0 = page
    # 8. the quarter turn
    orient = o.get("orient")
    if asked(orient):
        if orient is True:
            words = OR.estimate_orientation(page, thr, light)
            r.words["orient"] = words
            r.quarter = (int(words[0]) + (2 if o.get("half_turn") else 0)) & 3
        else:
            r.quarter = int(orient)
            assert 0 <= r.quarter <= 3
        r.turn = (r.quarter, page0.shape[0], page0.shape[1])
        page = OR.rotate(page0, r.quarter)
        r.pages["orient"] = page
    # 9. deskew
    if asked(o.get("deskew")):
        kp = _given(o["deskew"], SKEW, threshold=thr, light_text=light)
        r.words["deskew"], _ = SK.estimate_skew(page, **kp)
        page = SK.deskew(page, int(r.words["deskew"][1]), paper)
        r.pages["deskew"] = page
    # 10. dewarp
    if asked(o.get("dewarp")):
        up = _given(o["dewarp"], CURL, threshold=thr, light_text=light)
        r.words["dewarp"], r.words["curl_shifts"], _ = CU.estimate_curl(page, **up)
        r.curl_group = int(up["group"])
        page = CU.dewarp(page, r.words["curl_shifts"], r.curl_group, paper)
        r.pages["dewarp"] = page
    # 11. rules
    if asked(o.get("rules")):
        lp = _given(o["rules"], RU.DEFAULTS, threshold=thr, light_text=light)
        page, r.words["rules"] = RU.remove_rules(page, **lp)
        r.pages["rules"] = page
    r.pages["final"] = page
    # 12. layout, then the segmentation of every block or of the page, spaced or plain
    spaced = None
    if asked(o.get("spacing")):
        spaced = _given(o["spacing"], SP.SPACING)
        assert seg["word_gap"] != 0

    def segment(view, params):
        if spaced is None:
            return SG.segment_page(view, max_boxes, **params) + (None,)
        return SP.segment_page_spaced(view, max_boxes, spaced, **params)
    if asked(o.get("layout")):
        yp = _given(o["layout"], LA.DEFAULTS)
        r.blocks, r.lcounts, info = LA.layout_page(page, thr, light, MAX_BLOCKS, **yp)
        page_thr = int(info[0])
        block_seg = dict(seg, threshold=page_thr)
        rows, ids, gaps, found, lines, r.n_block_lines, r.block_found = [], [], [], 0, 0, [], []
        r.truncated = False
        for b, (x0, y0, x1, y1) in enumerate(r.blocks[:, :4].tolist()):
            bx, c, g = segment(np.ascontiguousarray(page[y0:y1, x0:x1]), block_seg)
            bx = bx.astype(np.int64)
            bx[:, [0, 2]] += x0
            bx[:, [1, 3]] += y0
            bx[:, 4] += lines
            rows.append(bx)
            ids += [b] * len(bx)
            if g is not None:
                gaps.append(g[:int(c[1])])
            found, lines = found + int(c[0]), lines + int(c[1])
            r.n_block_lines.append(int(c[1]))
            r.block_found.append(int(c[0]))
            r.truncated |= bool(c[0] > max_boxes)
        r.rows = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 6), np.int32)
        r.block_id = np.array(ids, np.int32)
        if spaced is not None:
            r.spacing = np.concatenate(gaps) if gaps else np.zeros((0, 8), np.int32)
        r.counts = (found, lines, page_thr)
    else:
        r.rows, counts, r.spacing = segment(page, seg)
        r.counts = tuple(int(v) for v in counts[:3])
        page_thr = r.counts[2]
        r.truncated = bool(counts[0] > max_boxes)
        if r.spacing is not None:
            r.spacing = r.spacing[:r.counts[1]]
    # 13. the slant of every box kept, on the page that was segmented, at the threshold the segmentation used
    if asked(o.get("deslant")):
        tp = _given(o["deslant"], SLANT, light_text=light)
        if tp["threshold"] < 0:
            tp["threshold"] = page_thr
        r.slant, _ = SL.estimate_slant(page, r.rows, len(r.rows), **tp)
        r.extent = SL.slant_extent(r.rows, r.slant[:, 1])
    r.paper, r.seg, r.max_boxes = paper, seg, max_boxes

    def corners():
        from backmap_ref import corner_fields
        curl = (r.words["curl_shifts"], r.curl_group) if "dewarp" in r.words else None
        skew = (int(r.words["deskew"][1]), page.shape[0], page.shape[1]) if "deskew" in r.words else None
        return corner_fields(r.rows[:, :4], curl, skew, r.turn, r.resize, r.warp)
    r.corners = corners
    return r
