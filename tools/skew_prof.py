"""ms per call of aocr_estimate_skew (the defaults: Otsu, 193 candidates; and with a fixed threshold), of aocr_deskew_page and, as the
yardstick in the same process, of aocr_segment_page with Otsu, on the seeded 3508 x 2480 page of tools/segment_prof.py (A4 at 300 dpi),
skewed by one degree.  HIP events, warm-up calls, then medians over windows, as tools/segment_prof.py times its calls; next to the floors:
one page read for the estimate, one page read and one page write for the deskew, at the HBM rate.  Prints one JSON line and writes it to
profiles/skew_prof.json.
`skew_prof.py --trace N` instead runs N estimate calls and N deskew calls and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/skew_prof.py --trace 300`."""
import ctypes as C
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import H, W, HBM_BYTES_PER_S, WINDOWS, a4_page, emit, time_rows     # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

SLOPE = 1144                                   # atan(1144 / 65536) = 1.0 degree: 18 steps of the default sweep


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = a4_page()
    straight = torch.from_numpy(page_h).to(dev)
    page = aocr.deskew_page_device(straight, -SLOPE)                          # the lines now rise by SLOPE
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    otsu, fixed = aocr.SkewParams(), aocr.SkewParams(threshold=128)
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS, candidates=2 * otsu.n_steps + 1, planted_slope_q16=SLOPE,
               scratch_bytes=int(aocr.lib.aocr_skew_scratch_bytes(H, W, otsu.n_steps)), strips=(W + 31) // 32)
    scratch = torch.empty((row["scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    skew = torch.zeros(4, dtype=torch.int32, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)

    def est(p):
        aocr.check(aocr.lib.aocr_estimate_skew(st, aocr.ptr(page), W, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(skew), None), "estimate")

    def desk():
        aocr.check(aocr.lib.aocr_deskew_page(st, aocr.ptr(page), W, H, W, aocr.ptr(skew), 0, 255, aocr.ptr(out), W), "deskew")

    max_boxes = 4096
    seg_scratch = torch.empty((int(aocr.lib.aocr_segment_scratch_bytes(H, W, max_boxes)) + 7) // 8, dtype=torch.int64, device=dev)
    boxes = torch.zeros((max_boxes, 6), dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    seg_p = aocr.SegmentParams()

    def seg(pg):
        aocr.check(aocr.lib.aocr_segment_page(st, aocr.ptr(pg), W, H, W, C.byref(seg_p), aocr.ptr(seg_scratch), max_boxes, aocr.ptr(boxes), aocr.ptr(counts)), "seg")

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        for _ in range(int(sys.argv[2])):
            est(otsu)
            desk()
        torch.cuda.synchronize()
        return
    est(otsu)
    desk()
    row["skew"] = skew.cpu().numpy().tolist()
    seg(page)
    row["lines_skewed"], row["boxes_skewed"] = int(counts[1]), int(counts[0])
    seg(out)
    row["lines_deskewed"], row["boxes_deskewed"] = int(counts[1]), int(counts[0])
    seg(straight)
    row["lines_straight"], row["boxes_straight"] = int(counts[1]), int(counts[0])
    time_rows(row, [("estimate_otsu", lambda: est(otsu), 50), ("estimate_fixed", lambda: est(fixed), 50), ("deskew", desk, 50),
                    ("segment_otsu", lambda: seg(out), 50)])
    row["read_floor_ms"] = H * W / HBM_BYTES_PER_S * 1e3                      # the estimate's floor: one read of the page
    row["deskew_floor_ms"] = 2 * H * W / HBM_BYTES_PER_S * 1e3                # one read and one write
    row["sweep_byte_adds"] = row["candidates"] * row["strips"] * H
    row["estimate_over_segment"] = row["estimate_otsu_ms"] / row["segment_otsu_ms"]
    emit(row, "skew")


if __name__ == "__main__":
    main()
