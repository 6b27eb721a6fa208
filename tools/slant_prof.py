"""ms per call of aocr_estimate_slant (the defaults: 25 candidates, the threshold read from the segmentation's device word) and of
aocr_crop_lines_slanted at 32 x 100 and, as the yardsticks in the same process on the same page, of aocr_segment_page (Otsu) and of
aocr_crop_lines, on the seeded A4 page of tools/segment_prof.py (3508 x 2480, about a thousand word boxes).  The boxes are the
segmentation's own, on the device.  HIP events, warm-up calls, then medians over windows, as tools/segment_prof.py times its calls.
Prints one JSON line and writes it to profiles/slant_prof.json."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import WINDOWS, a4_page, emit, time_rows                    # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

MAX_BOXES, OUT_H, OUT_W = 4096, 32, 100


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = a4_page()
    H, W = page_h.shape
    page = torch.from_numpy(page_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    seg, p = aocr.SegmentParams(), aocr.SlantParams()
    seg_scratch = torch.empty((int(aocr.lib.aocr_segment_scratch_bytes(H, W, MAX_BOXES)) + 7) // 8, dtype=torch.int64, device=dev)
    boxes = torch.zeros((MAX_BOXES, 6), dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)

    def segment():
        aocr.check(aocr.lib.aocr_segment_page(st, aocr.ptr(page), W, H, W, C.byref(seg), aocr.ptr(seg_scratch), MAX_BOXES, aocr.ptr(boxes),
                                              aocr.ptr(counts)), "segment")

    segment()
    n = int(min(int(counts[0]), MAX_BOXES))
    rows = boxes[:n].cpu().numpy()
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, boxes=n, windows=WINDOWS, step_q16=p.step_q16, n_steps=p.n_steps,
               out_h=OUT_H, out_w=OUT_W, box_w_median=float(np.median(rows[:, 2] - rows[:, 0])), box_h_median=float(np.median(rows[:, 3] - rows[:, 1])),
               scratch_bytes=int(aocr.lib.aocr_slant_scratch_bytes(n, p.n_steps)))
    scratch = torch.empty((row["scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    slant = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    out = torch.empty((n, 1, OUT_H, OUT_W), dtype=torch.float32, device=dev)
    thr = counts[2:3]

    def estimate():
        aocr.check(aocr.lib.aocr_estimate_slant(st, aocr.ptr(page), W, H, W, aocr.ptr(boxes), aocr.ptr(counts), n, C.byref(p), aocr.ptr(thr),
                                                aocr.ptr(scratch), aocr.ptr(slant), None), "estimate")

    def crop_slanted():
        aocr.check(aocr.lib.aocr_crop_lines_slanted(st, aocr.ptr(page), W, H, W, aocr.ptr(boxes), aocr.ptr(counts), n, aocr.ptr(slant), 255, OUT_H, OUT_W,
                                                    aocr.ptr(out)), "crop_slanted")

    def crop():
        aocr.check(aocr.lib.aocr_crop_lines(st, aocr.ptr(page), W, H, W, aocr.ptr(boxes), aocr.ptr(counts), n, OUT_H, OUT_W, aocr.ptr(out)), "crop")

    estimate()
    words = slant.cpu().numpy()
    row["slant_histogram"] = {int(k): int(v) for k, v in zip(*np.unique(words[:, 0], return_counts=True))}
    row["flags"] = [int((words[:, 2] == f).sum()) for f in range(3)]
    time_rows(row, [("segment_otsu", segment, 50), ("estimate", estimate, 50), ("crop", crop, 50), ("crop_slanted", crop_slanted, 50)])
    row["estimate_over_segment"] = row["estimate_ms"] / row["segment_otsu_ms"]
    row["crop_slanted_over_crop"] = row["crop_slanted_ms"] / row["crop_ms"]
    emit(row, "slant")


if __name__ == "__main__":
    main()
