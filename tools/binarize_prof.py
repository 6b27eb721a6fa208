"""microseconds per call of aocr_binarize_page at r = 20 and r = 63 on the two-column A4 page of tools/layout_prof.py (3508 x 2480, 300 dpi), next
to aocr_flatten_page (radius 16), an existing windowed stage, on the same page in the same process.  HIP events, warm-up calls, then medians
over windows, as tools/segment_prof.py times its calls; every call is timed in two passes.  Effective GB/s is counted at 2 bytes per pixel:
one page read, one written, the least any such stage can move.  No gate.  Prints one JSON line and writes it to profiles/binarize_prof.json."""
import ctypes as C
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import H, W, HBM_BYTES_PER_S, WINDOWS, emit, time_rows      # noqa: E402  (also puts the package on sys.path)
from layout_prof import two_column_a4                                         # noqa: E402
import aocr                                                                   # noqa: E402


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = two_column_a4()
    page = torch.from_numpy(page_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    fp = aocr.FlattenParams(radius=16)
    b20, b63 = aocr.BinarizeParams(radius=20), aocr.BinarizeParams(radius=63)
    need = max(int(aocr.lib.aocr_flatten_scratch_bytes(H, W, 16)), int(aocr.lib.aocr_binarize_scratch_bytes(H, W, 63)))
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)

    def binarize(bp, words):
        def call():
            aocr.check(aocr.lib.aocr_binarize_page(st, aocr.ptr(page), W, H, W, C.byref(bp), aocr.ptr(scratch), aocr.ptr(out), W, words), "binarize")
        return call

    def flatten():
        aocr.check(aocr.lib.aocr_flatten_page(st, aocr.ptr(page), W, H, W, C.byref(fp), aocr.ptr(scratch), aocr.ptr(out), W), "flatten")

    binarize(b20, aocr.ptr(counts))()
    got = counts.cpu().numpy().copy()
    floor_bytes = 2 * H * W
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS, form="fused: one launch, vertical sums in registers",
               binarize_scratch_bytes=int(aocr.lib.aocr_binarize_scratch_bytes(H, W, 63)),
               flatten_scratch_bytes=int(aocr.lib.aocr_flatten_scratch_bytes(H, W, 16)), counts_r20=[int(v) for v in got],
               floor_bytes=floor_bytes, floor_us=floor_bytes / HBM_BYTES_PER_S * 1e6)
    fns = [("binarize_r20", binarize(b20, None), 20), ("binarize_r20_counts", binarize(b20, aocr.ptr(counts)), 20),
           ("binarize_r63", binarize(b63, None), 20), ("flatten_r16", flatten, 20)]
    time_rows(row, fns + [(name + "_again", fn, iters) for name, fn, iters in fns])          # a second pass: drift between passes is the noise floor
    for name in ("binarize_r20", "binarize_r20_counts", "binarize_r63", "flatten_r16"):
        row[name + "_us"] = row[name + "_ms"] * 1e3
        row[name + "_gbps"] = floor_bytes / (row[name + "_ms"] * 1e-3) / 1e9
    row["binarize_r20_over_flatten"] = row["binarize_r20_ms"] / row["flatten_r16_ms"]
    row["binarize_r63_over_flatten"] = row["binarize_r63_ms"] / row["flatten_r16_ms"]
    emit(row, "binarize")


if __name__ == "__main__":
    main()
