"""aocr -- host side of the MI355X-native attention-OCR hot path.

`aocr.Model` mirrors the reference's Lua `Model` class (src/model/model.lua) on top of
the C ABI in include/aocr.h (libaocr.so, hand-written HIP for gfx950).  Importing this
package loads the shared library and fails loudly if it is missing.
"""
from . import _lib                      # noqa: F401  (raises ImportError when libaocr.so is absent)
from ._lib import HUE_RED, HUE_YELLOW, HUE_GREEN, HUE_CYAN, HUE_BLUE, HUE_MAGENTA, AdamParams, AocrError, Config, COMPUTE_BF16, COMPUTE_F32, lib, last_error, check, ptr, param_table
from .model import Model, eval_word_err_rate, numlist2str, encoder_columns, GROUPS
from . import synth
from . import data
from .data import DataGen
from . import degrade
from .degrade import Degrader
from . import augment
from .augment import Augmenter
from . import synth_lines
from .synth_lines import GlyphAtlas, SynthGen
from . import page
from .page import SegmentParams, SkewParams, FlattenParams, LayoutParams, CleanParams, label_components_device, clean_page_device, ink_integral_device, layout_page_device, segment_page_device, crop_lines_device, estimate_skew_device, deskew_page_device, flatten_page_device, source_corners, rotate_page_device, estimate_orientation_device, unrotate_boxes, RectifyParams, find_page_quad_device, rectify_plan, warp_page_device, warp_points, GlyphParams, ScaleParams, estimate_glyph_size_device, resize_page_device, scale_plan, unscale_points, CurlParams, estimate_curl_device, dewarp_page_device, curl_shift_q8, uncurl_points, source_points, ColourParams, estimate_page_colour_device, gray_page_device, SlantParams, estimate_slant_device, crop_lines_slanted_device, slant_extent, SpacingParams, segment_page_spaced_device, RuleParams, remove_rules_device, PanelParams, invert_panels_device, BinarizeParams, binarize_page_device
from . import dictionary
from . import t7, checkpoint
from .dictionary import Trie, load_dictionary, build_trie, levenshtein, Lexicon, load_lexicon

__all__ = ["Model", "DataGen", "Augmenter", "augment", "Degrader", "degrade", "GlyphAtlas", "SynthGen", "synth_lines", "page", "SegmentParams", "segment_page_device", "crop_lines_device", "SkewParams", "estimate_skew_device", "deskew_page_device", "FlattenParams", "flatten_page_device", "LayoutParams", "ink_integral_device", "layout_page_device", "CleanParams", "label_components_device", "clean_page_device", "source_corners", "rotate_page_device", "estimate_orientation_device", "unrotate_boxes", "RectifyParams", "find_page_quad_device", "rectify_plan", "warp_page_device", "warp_points", "GlyphParams", "ScaleParams", "estimate_glyph_size_device", "resize_page_device", "scale_plan", "unscale_points", "CurlParams", "estimate_curl_device", "dewarp_page_device", "curl_shift_q8", "uncurl_points", "source_points", "ColourParams", "estimate_page_colour_device", "gray_page_device", "SlantParams", "estimate_slant_device", "crop_lines_slanted_device", "slant_extent", "SpacingParams", "segment_page_spaced_device", "RuleParams", "remove_rules_device", "PanelParams", "invert_panels_device", "BinarizeParams", "binarize_page_device", "HUE_RED", "HUE_YELLOW", "HUE_GREEN", "HUE_CYAN", "HUE_BLUE", "HUE_MAGENTA", "data", "dictionary", "t7", "checkpoint", "Trie", "load_dictionary", "build_trie", "levenshtein", "Lexicon", "load_lexicon", "AdamParams", "AocrError", "Config", "COMPUTE_F32", "COMPUTE_BF16", "lib", "last_error", "check", "ptr",
           "param_table", "eval_word_err_rate", "numlist2str", "encoder_columns", "GROUPS", "synth"]
