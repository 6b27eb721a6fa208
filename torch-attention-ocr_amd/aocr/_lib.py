"""ctypes binding of libaocr.so (the C ABI declared in include/aocr.h).

There is NO fallback: if the HIP library is missing or a symbol is absent this
module raises at import time, and every entry point raises ``AocrError`` on a
non-zero status.  Nothing here touches ``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  -- BEFORE libaocr.so: the process must end up with ONE HIP runtime, the one PyTorch loads.  Loading
#                libaocr.so first pulls in /opt/rocm's libamdhip64 next to PyTorch's own copy, and the library then sees no device

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AOCR_LIB") or os.path.join(_HERE, "libaocr.so")     # AOCR_LIB: another build of the SAME library (debug stamps), as in lua/aocr_ffi.lua

NUM_GROUPS = 5
COMPUTE_F32, COMPUTE_BF16 = 0, 1
PROF_FAMILIES = ["other", "conv_fwd", "conv_dgrad", "conv_wgrad", "bn", "pool_conv1", "encoder_seq", "rnn_gemm", "decoder_fwd",
                 "decoder_bwd", "sgd", "decode_chain"]          # AOCR_PROF_* of include/aocr.h


class AocrError(RuntimeError):
    pass


class TrieDesc(C.Structure):
    """mirror of `aocr_trie` (include/aocr.h)."""
    _fields_ = [("child_mask_dev", C.c_void_p), ("child_base_dev", C.c_void_p), ("child_dev", C.c_void_p),
                ("n_nodes", C.c_int32), ("n_edges", C.c_int32)]


class LexiconDesc(C.Structure):
    """mirror of `aocr_lexicon` (include/aocr.h)."""
    _fields_ = [("words_dev", C.c_void_p), ("n_words", C.c_int32), ("stride", C.c_int32)]


class GlyphAtlasDesc(C.Structure):
    """mirror of `aocr_glyph_atlas` (include/aocr.h)."""
    _fields_ = [("pixels_dev", C.c_void_p), ("advance_dev", C.c_void_p), ("n_faces", C.c_int32), ("n_glyphs", C.c_int32),
                ("gh", C.c_int32), ("gw", C.c_int32)]


class SynthStyle(C.Structure):
    """mirror of `aocr_synth_style` (include/aocr.h)."""
    _fields_ = [("word", C.c_int32), ("face", C.c_int32)] + [(n, C.c_float) for n in ("spacing", "sx", "sy", "x0", "y0", "fg", "bg")]


class AdamParams(C.Structure):
    """mirror of `aocr_adam_params` (include/aocr.h): AdamW's step size, the two decay rates of the moment estimates, the denominator's eps,
    the decoupled weight decay and the per-group gradient-norm clip (0: no clip).  The constructor raises ValueError for what the library
    would turn down."""
    _fields_ = [(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "clip")] + [("reserved", C.c_int32 * 2)]

    def __init__(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip=0.0):
        b1, b2 = (float(b) for b in betas)
        lr, eps, weight_decay, clip = float(lr), float(eps), float(weight_decay), float(clip)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas={betas!r}: each in [0, 1)")
        if not (0.0 < eps < float("inf")):
            raise ValueError(f"eps={eps}: finite and > 0")
        for name, v in (("lr", lr), ("weight_decay", weight_decay), ("clip", clip)):
            if not (0.0 <= v < float("inf")):
                raise ValueError(f"{name}={v}: finite and >= 0")
        super().__init__(lr, b1, b2, eps, weight_decay, clip, (C.c_int32 * 2)(0, 0))


class SegmentParams(C.Structure):
    """mirror of `aocr_segment_params` (include/aocr.h): how `aocr_segment_page` finds lines and words.  threshold -1: Otsu."""
    _fields_ = [(n, C.c_int32) for n in ("threshold", "light_text", "min_row_ink", "merge_gap", "min_line_h", "word_gap", "min_word_w",
                                         "pad_x", "pad_y", "reserved")]

    def __init__(self, threshold=-1, light_text=0, min_row_ink=1, merge_gap=2, min_line_h=8, word_gap=12, min_word_w=4, pad_x=2, pad_y=2):
        super().__init__(int(threshold), int(light_text), int(min_row_ink), int(merge_gap), int(min_line_h), int(word_gap), int(min_word_w),
                         int(pad_x), int(pad_y), 0)


class SpacingParams(C.Structure):
    """mirror of `aocr_spacing_params` (include/aocr.h): how `aocr_segment_page_spaced` estimates the word gap of every line from the line's
    own gaps.  The percents are of the band height: the estimate is clamped to lo..hi, and a line with fewer than min_gaps gaps, one gap
    length, or two classes closer than ratio_percent / 100 takes default_percent.  How the defaults were chosen: DESIGN.md section 23."""
    _fields_ = [(n, C.c_int32) for n in ("min_gaps", "lo_percent", "hi_percent", "default_percent", "ratio_percent")] + [("reserved", C.c_int32 * 3)]

    def __init__(self, min_gaps=4, lo_percent=25, hi_percent=80, default_percent=40, ratio_percent=150):
        super().__init__(int(min_gaps), int(lo_percent), int(hi_percent), int(default_percent), int(ratio_percent), (C.c_int32 * 3)(0, 0, 0))


class SkewParams(C.Structure):
    """mirror of `aocr_skew_params` (include/aocr.h): the candidates of `aocr_estimate_skew`, k = -n_steps..n_steps at k * step_q16 / 65536 rows
    per column.  threshold -1: Otsu.  The defaults sweep +-5.4 degrees in steps of 0.056."""
    _fields_ = [(n, C.c_int32) for n in ("threshold", "light_text", "step_q16", "n_steps")]

    def __init__(self, threshold=-1, light_text=0, step_q16=64, n_steps=96):
        super().__init__(int(threshold), int(light_text), int(step_q16), int(n_steps))


class FlattenParams(C.Structure):
    """mirror of `aocr_flatten_params` (include/aocr.h): the window radius of `aocr_flatten_page`.  The radius must exceed the stroke width
    (solid ink wider than 2 * radius + 1 is read as dark paper); at 300 dpi 16 to 32 is typical."""
    _fields_ = [("radius", C.c_int32), ("light_text", C.c_int32), ("reserved", C.c_int32 * 2)]

    def __init__(self, radius=16, light_text=0):
        super().__init__(int(radius), int(light_text), (C.c_int32 * 2)(0, 0))


class BinarizeParams(C.Structure):
    """mirror of `aocr_binarize_params` (include/aocr.h): the window radius, Sauvola's k (k_q8 / 256) and the dynamic range R of
    `aocr_binarize_page`.  hard 0 writes a gray page on which the fixed threshold 127 is the local decision (ink 0..127, paper 128..255, the
    anti-aliasing kept); hard 1 writes ink 0 and paper 255.  The window must be wider than a stroke (a wider stroke is hollowed out); the
    defaults are a judgement for text at 300 dpi and nobody has tuned them on real scans."""
    _fields_ = [(n, C.c_int32) for n in ("radius", "k_q8", "range", "light_text", "hard")] + [("reserved", C.c_int32 * 3)]

    def __init__(self, radius=20, k_q8=51, range=128, light_text=0, hard=0):
        super().__init__(int(radius), int(k_q8), int(range), int(light_text), int(hard), (C.c_int32 * 3)(0, 0, 0))


class LayoutParams(C.Structure):
    """mirror of `aocr_layout_params` (include/aocr.h): the recursive XY cut of `aocr_layout_blocks`.  gap_x is what a gutter must exceed and a
    word gap must not; gap_y what a paragraph gap must exceed and a line gap must not."""
    _fields_ = [(n, C.c_int32) for n in ("min_ink", "gap_x", "gap_y", "max_depth", "min_block_w", "min_block_h", "min_block_ink", "reserved")]

    def __init__(self, min_ink=1, gap_x=24, gap_y=30, max_depth=8, min_block_w=8, min_block_h=8, min_block_ink=16):
        super().__init__(int(min_ink), int(gap_x), int(gap_y), int(max_depth), int(min_block_w), int(min_block_h), int(min_block_ink), 0)


class CleanParams(C.Structure):
    """mirror of `aocr_clean_params` (include/aocr.h): which connected components `aocr_clean_page` paints over.  A component with fewer than
    min_area pixels is a speck; one that is no speck and whose box is wider than max_w or higher than max_h is a rule (0: that test is off).
    threshold -1: Otsu.  The defaults are a judgement for text at 300 dpi -- dust is a few pixels, an i-dot a dozen or more, no glyph is 200
    rows high, and a long word can be as wide as a short rule, so the width test is off -- and nobody has tuned them on real scans."""
    _fields_ = [(n, C.c_int32) for n in ("threshold", "light_text", "connectivity", "min_area", "max_w", "max_h")] + [("reserved", C.c_int32 * 2)]

    def __init__(self, threshold=-1, light_text=0, connectivity=8, min_area=6, max_w=0, max_h=200):
        super().__init__(int(threshold), int(light_text), int(connectivity), int(min_area), int(max_w), int(max_h), (C.c_int32 * 2)(0, 0))


class RuleParams(C.Structure):
    """mirror of `aocr_rule_params` (include/aocr.h): which pixels `aocr_remove_rules` paints over.  A run of at least min_len ink pixels along
    a row (axes & 1) or a column (axes & 2) is a rule candidate; of it go the pixels whose run across the rule is at most max_thick long,
    the ragged pixels within `edge` of it, and the crossings of two rules; a stroke that crosses a rule is thicker and stays whole.
    threshold -1: Otsu.  The defaults are a judgement for text at 300 dpi -- a third of an inch is longer than any stroke of body text, half a
    millimetre thicker than a form line -- and nobody has tuned them on real scans.  The constructor raises ValueError for what the library
    would turn down."""
    _fields_ = [(n, C.c_int32) for n in ("threshold", "light_text", "axes", "min_len", "max_thick", "edge")] + [("reserved", C.c_int32 * 2)]

    def __init__(self, threshold=-1, light_text=0, axes=3, min_len=100, max_thick=6, edge=1):
        threshold, light_text, axes, min_len, max_thick, edge = (int(v) for v in (threshold, light_text, axes, min_len, max_thick, edge))
        if not -1 <= threshold <= 254:
            raise ValueError(f"threshold={threshold}: 0..254, or -1 for Otsu")
        if axes not in (1, 2, 3):
            raise ValueError(f"axes={axes}: 1 horizontal rules, 2 vertical rules, 3 both")
        if not 1 <= max_thick <= 16:
            raise ValueError(f"max_thick={max_thick}: 1..16")
        if not max_thick < min_len <= 16384:
            raise ValueError(f"min_len={min_len}: max_thick={max_thick} < min_len <= 16384")
        if not 0 <= edge <= 4:
            raise ValueError(f"edge={edge}: 0..4")
        super().__init__(threshold, light_text, axes, min_len, max_thick, edge, (C.c_int32 * 2)(0, 0))


class PanelParams(C.Structure):
    """mirror of `aocr_panel_params` (include/aocr.h): which connected components `aocr_invert_panels` takes for reversed-out panels -- dark
    slabs that carry light text -- and inverts inside their row spans.  A component whose tight box is at least min_w x min_h is a candidate;
    it is a panel when its ink fills at least fill_percent of its row-convex hull (glyphs, figures and photographs do not) and at least
    min_inside_percent of the hull is not ink (something is written on it; 0 takes solid bars too).  threshold -1: Otsu.  The defaults are a
    judgement for text at 300 dpi -- a slab holds at least one line of body text and a short word -- and nobody has tuned them on real scans.
    The constructor raises ValueError for what the library would turn down."""
    _fields_ = [(n, C.c_int32) for n in ("threshold", "light_text", "connectivity", "min_w", "min_h", "fill_percent", "min_inside_percent", "reserved")]

    def __init__(self, threshold=-1, light_text=0, connectivity=8, min_w=64, min_h=24, fill_percent=60, min_inside_percent=2):
        threshold, light_text, connectivity, min_w, min_h, fill_percent, min_inside_percent = (
            int(v) for v in (threshold, light_text, connectivity, min_w, min_h, fill_percent, min_inside_percent))
        if not -1 <= threshold <= 254:
            raise ValueError(f"threshold={threshold}: 0..254, or -1 for Otsu")
        if connectivity not in (4, 8):
            raise ValueError(f"connectivity={connectivity}: 4 or 8")
        if min_w < 1 or min_h < 1:
            raise ValueError(f"min_w={min_w} min_h={min_h} must be >= 1")
        if not 1 <= fill_percent <= 100:
            raise ValueError(f"fill_percent={fill_percent}: 1..100")
        if not 0 <= min_inside_percent <= 99:
            raise ValueError(f"min_inside_percent={min_inside_percent}: 0..99")
        if fill_percent + min_inside_percent > 100:
            raise ValueError(f"fill_percent={fill_percent} + min_inside_percent={min_inside_percent} is more than 100")
        super().__init__(threshold, light_text, connectivity, min_w, min_h, fill_percent, min_inside_percent, 0)


class RectifyParams:
    """how `Model.recognize_page(rectify=...)` finds and straightens a photographed page (`aocr_find_page_quad`, `aocr_rectify_plan`,
    `aocr_warp_page`; plain Python: there is no C struct behind it).  threshold -1: Otsu; dark_paper 1: the paper is the dark side of the threshold
    (rectify=True takes the segment params' light_text for it); width / height 0: the lengths of the quad's longer sides; the quad is used only when it is valid and the sheet covers at least
    min_area_percent of the photograph; fill None: the paper colour, as for deskew."""

    def __init__(self, threshold=-1, dark_paper=0, width=0, height=0, min_area_percent=10, fill=None):
        self.threshold, self.dark_paper = int(threshold), int(dark_paper)
        self.width, self.height, self.min_area_percent = int(width), int(height), int(min_area_percent)
        self.fill = None if fill is None else int(fill)


class GlyphParams(C.Structure):
    """mirror of `aocr_glyph_params` (include/aocr.h): which connected components `aocr_estimate_glyph_size` counts as glyphs.  The size of a
    component is a = min(w, h) of its tight box; it counts when min_size <= a <= max_size and max(w, h) <= max_aspect * a (rules and the
    stems of l and 1 do not).  threshold -1: Otsu."""
    _fields_ = [(n, C.c_int32) for n in ("threshold", "light_text", "connectivity", "min_size", "max_size", "max_aspect")] + [("reserved", C.c_int32 * 2)]

    def __init__(self, threshold=-1, light_text=0, connectivity=8, min_size=2, max_size=512, max_aspect=8):
        super().__init__(int(threshold), int(light_text), int(connectivity), int(min_size), int(max_size), int(max_aspect), (C.c_int32 * 2)(0, 0))


class CurlParams(C.Structure):
    """mirror of `aocr_curl_params` (include/aocr.h): how `aocr_estimate_curl` measures page curl.  Columns are taken in groups of 32 * group;
    neighbouring groups are tried at row shifts -max_shift..max_shift (keep it below half the line pitch); a pair with a group of fewer than
    min_ink ink pixels gets shift 0.  threshold -1: Otsu."""
    _fields_ = [(n, C.c_int32) for n in ("threshold", "light_text", "group", "max_shift", "min_ink")] + [("reserved", C.c_int32 * 3)]

    def __init__(self, threshold=-1, light_text=0, group=4, max_shift=8, min_ink=64):
        super().__init__(int(threshold), int(light_text), int(group), int(max_shift), int(min_ink), (C.c_int32 * 3)(0, 0, 0))


SLANT_MAX_H = 256                                                               # AOCR_SLANT_MAX_H of include/aocr.h


class SlantParams(C.Structure):
    """mirror of `aocr_slant_params` (include/aocr.h): the candidates of `aocr_estimate_slant`, k = -n_steps..n_steps at k * step_q16 / 65536
    columns per row (n_steps * step_q16 <= 65536, 45 degrees).  threshold -1: the device word given with the call (the threshold that
    `aocr_segment_page` wrote to its counts).  The defaults sweep +-36.9 degrees in steps of 1/16 column per row."""
    _fields_ = [(n, C.c_int32) for n in ("threshold", "light_text", "step_q16", "n_steps")] + [("reserved", C.c_int32 * 4)]

    def __init__(self, threshold=-1, light_text=0, step_q16=4096, n_steps=12):
        super().__init__(int(threshold), int(light_text), int(step_q16), int(n_steps), (C.c_int32 * 4)(0, 0, 0, 0))


HUE_RED, HUE_YELLOW, HUE_GREEN, HUE_CYAN, HUE_BLUE, HUE_MAGENTA = range(6)      # AOCR_HUE_* of include/aocr.h: the bits of ColourParams.drop


class ColourParams(C.Structure):
    """mirror of `aocr_colour_params` (include/aocr.h): how `aocr_gray_page` turns an RGB page into the gray page the other stages read.
    weights: (w_R, w_G, w_B), each >= 0 and 256 in sum ((77, 150, 29): luma; (256, 0, 0): the red channel); mode 0: the weighted sum, 1: the
    smallest balanced channel; balance 1: the paper colour is divided out; paper: (p_R, p_G, p_B) in 1..255, None: estimated on the device
    (`aocr_estimate_page_colour`, which takes the most frequent value >= paper_min of every channel); a pixel is coloured when the spread
    of its balanced channels reaches chroma_min; drop: a sum of 1 << HUE_*, the classes whose coloured pixels become `fill`.  The
    constructor raises ValueError for what the library would turn down."""
    _fields_ = [("weights", C.c_int32 * 3), ("mode", C.c_int32), ("balance", C.c_int32), ("paper", C.c_int32 * 3)] + \
               [(n, C.c_int32) for n in ("paper_min", "chroma_min", "drop", "fill")]

    def __init__(self, weights=(77, 150, 29), mode=0, balance=1, paper=None, paper_min=128, chroma_min=64, drop=0, fill=255):
        w = [int(v) for v in weights]
        if len(w) != 3 or min(w) < 0 or sum(w) != 256:
            raise ValueError(f"weights={weights!r}: three integers >= 0 that sum to 256")
        p = [-1, -1, -1] if paper is None else [int(v) for v in paper]
        if len(p) != 3 or (paper is not None and not all(1 <= v <= 255 for v in p)):
            raise ValueError(f"paper={paper!r}: None or three integers in 1..255")
        mode, balance, paper_min, chroma_min, drop, fill = int(mode), int(balance), int(paper_min), int(chroma_min), int(drop), int(fill)
        if mode not in (0, 1) or balance not in (0, 1):
            raise ValueError(f"mode={mode} balance={balance}: 0 or 1 each")
        if not (1 <= paper_min <= 255 and 1 <= chroma_min <= 255):
            raise ValueError(f"paper_min={paper_min} chroma_min={chroma_min}: 1..255 each")
        if not 0 <= drop <= 63:
            raise ValueError(f"drop={drop}: 0..63, a sum of 1 << HUE_*")
        if not 0 <= fill <= 255:
            raise ValueError(f"fill={fill}: 0..255")
        super().__init__((C.c_int32 * 3)(*w), mode, balance, (C.c_int32 * 3)(*p), paper_min, chroma_min, drop, fill)


class ScaleParams:
    """how `Model.recognize_page(scale=...)` brings the text of a page to the size the other stages' defaults were written for
    (`aocr_estimate_glyph_size`, `aocr.scale_plan`, `aocr_resize_page`; plain Python: there is no C struct behind it).  glyph: the
    `GlyphParams` of the estimate; target: the glyph size to resample to (16: what the estimate reads on the glyph atlas at its native size,
    the size every default was judged on); the page is left alone when target / size lies within [1 / tolerance, tolerance], or when fewer
    than min_glyphs components qualified."""

    def __init__(self, glyph=None, target=16, tolerance=1.25, min_glyphs=8):
        self.glyph = glyph if glyph is not None else GlyphParams()
        self.target, self.tolerance, self.min_glyphs = int(target), float(tolerance), int(min_glyphs)


class Box(C.Structure):
    """mirror of `aocr_box` (include/aocr.h): half-open [x0,x1) x [y0,y1), line number, ink pixels."""
    _fields_ = [(n, C.c_int32) for n in ("x0", "y0", "x1", "y1", "line", "ink")]


class Config(C.Structure):
    """mirror of `aocr_config` (include/aocr.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "batch_size", "img_h", "max_img_w", "enc_hidden", "enc_layers", "dec_layers", "vocab", "emb",
        "input_feed", "max_decoder_l", "max_beam", "compute")]


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `make -C torch-attention-ocr_amd/csrc` "
        "(or __graft_entry__.build()); there is no CPU fallback for the hot path")

lib = C.CDLL(LIB_PATH)

_vp, _i32, _i64, _f32, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
_cfgp = C.POINTER(Config)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, _vp, _vp, _i64, _i32, _vp)     # aocr_allreduce_fn of include/aocr.h

# name -> (restype, argtypes); every symbol declared in include/aocr.h
SIGNATURES = {
    "aocr_last_error": (C.c_char_p, []),
    "aocr_version": (C.c_int, []),
    "aocr_param_counts": (C.c_int, [_cfgp, C.POINTER(_i64)]),
    "aocr_param_entry": (C.c_int, [_cfgp, _i32, C.c_char_p, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i64)]),
    "aocr_bn_state_count": (_i64, []),
    "aocr_workspace_bytes": (_sz, [_cfgp]),
    "aocr_model_create": (C.c_int, [_cfgp, _vp, _vp, _vp, _vp, _sz, _vp, C.POINTER(_vp)]),
    "aocr_model_destroy": (C.c_int, [_vp]),
    "aocr_model_set_stream": (C.c_int, [_vp, _vp]),
    "aocr_train_forward_backward": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "aocr_set_dropout": (C.c_int, [_vp, C.c_double, C.c_uint64, C.c_uint64]),
    "aocr_cluster_status": (C.c_int, [_vp, C.POINTER(_i32)]),
    "aocr_grad_buckets": (C.c_int, [_cfgp, C.POINTER(_i64), C.POINTER(_i64)]),
    "aocr_stream_wait_grads": (C.c_int, [_vp, _i32, _vp]),
    "aocr_comm_unique_id": (C.c_int, [C.c_char_p]),
    "aocr_comm_init_rank": (C.c_int, [_vp, C.c_char_p, _i32, _i32, _i32]),
    "aocr_comm_set_callback": (C.c_int, [_vp, _vp, _vp, _i32, _i32]),
    "aocr_allreduce_grads": (C.c_int, [_vp, _vp]),
    "aocr_comm_destroy": (C.c_int, [_vp]),
    "aocr_comm_exposed_ms": (C.c_int, [_vp, C.POINTER(_f32)]),
    "aocr_comm_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "aocr_sgd_step": (C.c_int, [_vp, _f32, _f32, _vp]),
    "aocr_adadelta_step": (C.c_int, [_vp, _f32, _f32, _f32, _vp]),
    "aocr_adam_state_bytes": (_sz, [_i64]),
    "aocr_adam_scratch_bytes": (_sz, []),
    "aocr_adam_update": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(AdamParams), _vp, _vp, _vp]),
    "aocr_adam_step": (C.c_int, [_vp, C.POINTER(AdamParams), _vp, _vp]),
    "aocr_forward_logits": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "aocr_decode": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "aocr_decode_dict": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "aocr_recognize": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "aocr_get_tensor": (C.c_int, [_vp, C.c_char_p, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i64)]),
    "aocr_profile_kernel": (C.c_int, [_vp, _i32, _i32, C.POINTER(_f32), C.POINTER(C.c_double)]),
    "aocr_profile_enable": (C.c_int, [_vp, _i32]),
    "aocr_profile_read": (C.c_int, [_vp, C.POINTER(_f32), C.POINTER(_i32)]),
    "aocr_gemm": (C.c_int, [_vp, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _i32, _i32, _vp, _i32]),
    "aocr_conv2d_forward": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp] + [_i32] * 9),
    "aocr_conv2d_backward_data": (C.c_int, [_vp, _i32, _vp, _vp, _vp] + [_i32] * 7),
    "aocr_conv2d_backward_filter": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp] + [_i32] * 7),
    "aocr_unpool_relu_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp] + [_i32] * 5),
    "aocr_conv1_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32]),
    "aocr_conv1_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32]),
    "aocr_batchnorm_relu_forward": (C.c_int, [_vp] * 9 + [_i64, _i32, _i32, _i32, _i32]),
    "aocr_batchnorm_relu_backward": (C.c_int, [_vp] * 10 + [_i64, _i32, _i32]),
    "aocr_lstm_cell_forward": (C.c_int, [_vp, _i32, _vp, _i32] + [_vp] * 9 + [_i32, _i32]),
    "aocr_lstm_cell_forward_zx": (C.c_int, [_vp, _i32, _vp, _i64] + [_vp] * 6 + [_i32, _i32]),
    "aocr_lstm_cell_backward": (C.c_int, [_vp] * 8 + [_i32, _i32]),
    "aocr_attention_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "aocr_attention_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _i32, _i32]),
    "aocr_pointwise": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i64]),
    "aocr_lookup_forward": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32]),
    "aocr_lookup_backward": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32]),
    "aocr_logsoftmax_nll": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _f32]),
    "aocr_beam_select_dict": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "aocr_edit_distance": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "aocr_lexicon_scratch_bytes": (_sz, [_i32, _i32]),
    "aocr_lexicon_nearest": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "aocr_preprocess_lines": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "aocr_augment_lines": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, C.c_uint64, C.c_uint64, _vp]),
    "aocr_degrade_lines": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, C.c_uint64, C.c_uint64, _vp]),
    "aocr_synth_lines": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "aocr_segment_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "aocr_segment_page": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "aocr_segment_spaced_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "aocr_segment_page_spaced": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "aocr_crop_lines": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp]),
    "aocr_skew_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "aocr_estimate_skew": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "aocr_deskew_page": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _i32, _i32, _vp, C.c_int64]),
    "aocr_flatten_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "aocr_flatten_page": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, C.c_int64]),
    "aocr_binarize_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "aocr_binarize_page": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, C.c_int64, _vp]),
    "aocr_integral_scratch_bytes": (C.c_size_t, [_i32, _i32]),
    "aocr_ink_integral": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _i32, _i32, _vp, _vp, C.c_int64, _vp]),
    "aocr_layout_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "aocr_layout_blocks": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "aocr_components_scratch_bytes": (C.c_size_t, [_i32, _i32]),
    "aocr_label_components": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, C.c_int64, _i32, _vp, _vp]),
    "aocr_clean_scratch_bytes": (C.c_size_t, [_i32, _i32]),
    "aocr_clean_page": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, C.c_int64, _vp]),
    "aocr_rules_scratch_bytes": (C.c_size_t, [_i32, _i32]),
    "aocr_remove_rules": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, C.c_int64, _vp]),
    "aocr_panels_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "aocr_invert_panels": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, C.c_int64, _i32, _vp, _vp]),
    "aocr_rotate_page": (C.c_int,[_vp, _vp, C.c_int64, _i32, _i32, _vp, _i32, _vp, C.c_int64]),
    "aocr_orient_scratch_bytes": (C.c_size_t, [_i32, _i32]),
    "aocr_estimate_orientation": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "aocr_quad_scratch_bytes": (C.c_size_t, [_i32, _i32]),
    "aocr_find_page_quad": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "aocr_rectify_plan": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "aocr_warp_page": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _i32, _vp, C.c_int64, _i32, _i32]),
    "aocr_glyph_scratch_bytes": (C.c_size_t, [_i32, _i32]),
    "aocr_estimate_glyph_size": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp]),
    "aocr_resize_page": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, C.c_int64, _i32, _i32]),
    "aocr_curl_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32]),
    "aocr_estimate_curl": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "aocr_dewarp_page": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _i32, _vp, _i32, _vp, C.c_int64]),
    "aocr_colour_scratch_bytes": (C.c_size_t, [_i32, _i32]),
    "aocr_estimate_page_colour": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp]),
    "aocr_gray_page": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, _vp, C.c_int64]),
    "aocr_slant_scratch_bytes": (C.c_size_t, [_i32, _i32]),
    "aocr_estimate_slant": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "aocr_crop_lines_slanted": (C.c_int, [_vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp]),
    "aocr_beam_select": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)          # AttributeError here = library/header mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


def last_error() -> str:
    return (lib.aocr_last_error() or b"").decode()


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise AocrError(f"{what}: {last_error()}" if what else last_error())


def ptr(t):
    """device (or host) address of a torch tensor / None."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def param_table(cfg: Config):
    """[(name, group, offset, shape)] + per-group counts, straight from the library."""
    counts = (_i64 * NUM_GROUPS)()
    check(lib.aocr_param_counts(C.byref(cfg), counts), "aocr_param_counts")
    out = []
    i = 0
    while True:
        name = C.create_string_buffer(64)
        g, nd, off = _i32(), _i32(), _i64()
        shape = (_i64 * 4)()
        rc = lib.aocr_param_entry(C.byref(cfg), i, name, C.byref(g), C.byref(off), C.byref(nd), shape)
        if rc == 1:
            break
        if rc != 0:
            raise AocrError(last_error())
        out.append((name.value.decode(), g.value, off.value, tuple(shape[k] for k in range(nd.value))))
        i += 1
    return out, [counts[k] for k in range(NUM_GROUPS)]
