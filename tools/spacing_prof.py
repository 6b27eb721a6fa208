"""ms per call of aocr_segment_page_spaced (the defaults) next to aocr_segment_page (Otsu, word_gap 12) on the same page in the same process:
the seeded A4 page of tools/segment_prof.py (3508 x 2480).  The difference is what the first find_runs, the gap histogram and the Otsu wave
cost per call.  `--baseline PATH` loads another build of libaocr.so (the parent commit's) next to the package's and times its
aocr_segment_page in the same windows, interleaved with this build's: whether aocr_segment_page itself moved.  HIP events, warm-up calls,
then medians over windows, as tools/segment_prof.py times its calls.  Prints one JSON line and writes it to profiles/spacing_prof.json."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import WINDOWS, a4_page, emit, time_rows                    # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

MAX_BOXES = 4096


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = a4_page()
    H, W = page_h.shape
    page = torch.from_numpy(page_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    seg, sp = aocr.SegmentParams(), aocr.SpacingParams()
    scratch = torch.empty((int(aocr.lib.aocr_segment_spaced_scratch_bytes(H, W, MAX_BOXES)) + 7) // 8, dtype=torch.int64, device=dev)
    boxes = torch.zeros((MAX_BOXES, 6), dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    max_lines = (H + 1) // 2
    rows = torch.zeros((max_lines, 8), dtype=torch.int32, device=dev)

    def segment_of(lib):
        fn = lib.aocr_segment_page
        fn.restype, fn.argtypes = aocr._lib.SIGNATURES["aocr_segment_page"]

        def call():
            aocr.check(fn(st, aocr.ptr(page), W, H, W, C.byref(seg), aocr.ptr(scratch), MAX_BOXES, aocr.ptr(boxes), aocr.ptr(counts)), "segment")
        return call

    def spaced():
        aocr.check(aocr.lib.aocr_segment_page_spaced(st, aocr.ptr(page), W, H, W, C.byref(seg), C.byref(sp), aocr.ptr(scratch), MAX_BOXES,
                                                     aocr.ptr(boxes), aocr.ptr(counts), max_lines, aocr.ptr(rows)), "spaced")

    segment = segment_of(aocr.lib)
    segment()
    fixed = counts.cpu().numpy().copy()
    spaced()
    got = counts.cpu().numpy().copy()
    lines = int(got[1])
    r = rows[:lines].cpu().numpy()
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS, lines=lines, boxes_fixed_gap_12=int(fixed[0]), boxes_spaced=int(got[0]),
               gaps_counted_median=float(np.median(r[:, 2])), gap_histogram={int(k): int(v) for k, v in zip(*np.unique(r[:, 0], return_counts=True))},
               flags={int(k): int(v) for k, v in zip(*np.unique(r[:, 1], return_counts=True))},
               min_gaps=sp.min_gaps, lo_percent=sp.lo_percent, hi_percent=sp.hi_percent, default_percent=sp.default_percent, ratio_percent=sp.ratio_percent)
    fns = [("segment", segment, 50), ("spaced", spaced, 50)]
    if "--baseline" in sys.argv:
        fns.insert(0, ("segment_baseline", segment_of(C.CDLL(sys.argv[sys.argv.index("--baseline") + 1])), 50))
    time_rows(row, fns + [(name + "_again", fn, iters) for name, fn, iters in fns])          # a second pass: drift between passes is the noise floor
    row["spaced_minus_segment_ms"] = row["spaced_ms"] - row["segment_ms"]
    row["spaced_over_segment"] = row["spaced_ms"] / row["segment_ms"]
    if "--baseline" in sys.argv:
        row["segment_over_baseline"] = row["segment_ms"] / row["segment_baseline_ms"]
        row["segment_over_baseline_again"] = row["segment_again_ms"] / row["segment_baseline_again_ms"]
    emit(row, "spacing")


if __name__ == "__main__":
    main()
