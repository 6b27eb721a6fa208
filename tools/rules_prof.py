"""ms per call of aocr_remove_rules (the defaults, Otsu) next to aocr_clean_page (the defaults) and aocr_segment_page on the same page in the
same process: the seeded A4 page of tools/segment_prof.py (3508 x 2480) with a table grid and an underline under every fourth line drawn
on it, 3 pixels thick.  `--baseline PATH` loads another build of libaocr.so (the parent commit's) next to the package's and times its
aocr_clean_page and aocr_segment_page in the same windows, interleaved with this build's: the stage that rule removal complements, and
whether aocr_segment_page itself moved.  HIP events, warm-up calls, then medians over windows, as tools/segment_prof.py times its calls.
The byte floor is the page read once and written once and the three bit planes written once and read once (the apply pass reads 2T + 2e + 8
words per word from the cache, not from memory).  Prints one JSON line and writes it to profiles/rules_prof.json."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import HBM_BYTES_PER_S, WINDOWS, a4_page, emit, time_rows   # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

MAX_BOXES = 4096


def form_page():
    page, n_words = a4_page()
    H, W = page.shape
    for y in range(190, H - 150, 4 * 48):                                       # underlines
        page[y:y + 3, 150:W - 150] = 0
    for y in range(100, H - 90, 330):                                           # the grid
        page[y:y + 3, 100:W - 100] = 0
    for x in range(100, W - 90, 570):
        page[100:H - 100, x:x + 3] = 0
    return page, n_words


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = form_page()
    H, W = page_h.shape
    page = torch.from_numpy(page_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    seg, cp, rp = aocr.SegmentParams(), aocr.CleanParams(), aocr.RuleParams()
    need = max(int(aocr.lib.aocr_clean_scratch_bytes(H, W)), int(aocr.lib.aocr_segment_scratch_bytes(H, W, MAX_BOXES)),
               int(aocr.lib.aocr_rules_scratch_bytes(H, W)))
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    boxes = torch.zeros((MAX_BOXES, 6), dtype=torch.int32, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)

    def segment_of(lib):
        fn = lib.aocr_segment_page
        fn.restype, fn.argtypes = aocr._lib.SIGNATURES["aocr_segment_page"]
        return lambda: aocr.check(fn(st, aocr.ptr(page), W, H, W, C.byref(seg), aocr.ptr(scratch), MAX_BOXES, aocr.ptr(boxes), aocr.ptr(counts)), "segment")

    def clean_of(lib):
        fn = lib.aocr_clean_page
        fn.restype, fn.argtypes = aocr._lib.SIGNATURES["aocr_clean_page"]
        return lambda: aocr.check(fn(st, aocr.ptr(page), W, H, W, C.byref(cp), aocr.ptr(scratch), aocr.ptr(out), W, aocr.ptr(counts)), "clean")

    def rules():
        aocr.check(aocr.lib.aocr_remove_rules(st, aocr.ptr(page), W, H, W, C.byref(rp), aocr.ptr(scratch), aocr.ptr(out), W, aocr.ptr(counts)), "rules")

    rules()
    got = counts.cpu().numpy().copy()
    w64 = (W + 63) // 64
    floor_bytes = 2 * H * W + 2 * 3 * H * w64 * 8
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS, rules_scratch_bytes=int(aocr.lib.aocr_rules_scratch_bytes(H, W)),
               clean_scratch_bytes=int(aocr.lib.aocr_clean_scratch_bytes(H, W)), min_len=rp.min_len, max_thick=rp.max_thick, edge=rp.edge,
               counts=[int(v) for v in got], floor_bytes=floor_bytes, floor_ms=floor_bytes / HBM_BYTES_PER_S * 1e3)
    fns = [("rules", rules, 50), ("clean", clean_of(aocr.lib), 20), ("segment", segment_of(aocr.lib), 50)]
    if "--baseline" in sys.argv:
        base = C.CDLL(sys.argv[sys.argv.index("--baseline") + 1])
        fns += [("clean_baseline", clean_of(base), 20), ("segment_baseline", segment_of(base), 50)]
    time_rows(row, fns + [(name + "_again", fn, iters) for name, fn, iters in fns])          # a second pass: drift between passes is the noise floor
    row["rules_over_floor"] = row["rules_ms"] / row["floor_ms"]
    row["rules_over_clean"] = row["rules_ms"] / row["clean_ms"]
    if "--baseline" in sys.argv:
        row["rules_over_clean_baseline"] = row["rules_ms"] / row["clean_baseline_ms"]
        row["segment_over_baseline"] = row["segment_ms"] / row["segment_baseline_ms"]
        row["segment_over_baseline_again"] = row["segment_again_ms"] / row["segment_baseline_again_ms"]
    emit(row, "rules")


if __name__ == "__main__":
    main()
