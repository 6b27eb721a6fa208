"""ms per call of aocr_estimate_curl (the defaults: Otsu, groups of 128 columns, 17 shifts), of aocr_dewarp_page and, as the yardstick in
the same process on the same page, of aocr_deskew_page, on a 3300 x 2550 page (US letter at 300 dpi): the seeded page of
tools/segment_prof.py cut to 3300 rows and widened with paper, its columns sagging by up to 20 rows toward both edges.  HIP events,
warm-up calls, then medians over windows, as tools/segment_prof.py times its calls.  Prints one JSON line and writes it to
profiles/curl_prof.json.
`curl_prof.py --trace N` instead runs N estimate calls, N dewarp calls and N deskew calls and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/curl_prof.py --trace 300` (profiles/curl_kernel_stats.csv)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import HBM_BYTES_PER_S, WINDOWS, a4_page, emit, time_rows   # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

H, W = 3300, 2550
AMP = 20                                       # rows of sag at the left and right edge
SLOPE = 655                                    # the yardstick's shear: 0.01 rows per column


def letter_page():
    a4, n_words = a4_page()
    flat = np.full((H, W), 255, np.uint8)
    flat[:, 35:35 + a4.shape[1]] = a4[:H]
    page = np.full((H, W), 255, np.uint8)
    for x in range(W):
        d = int(np.floor(AMP * ((x - W / 2) / (W / 2)) ** 2 + 0.5))
        page[d:, x] = flat[:H - d, x]
    return flat, page, n_words


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    flat_h, page_h, n_words = letter_page()
    page = torch.from_numpy(page_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = aocr.CurlParams()
    ng = -(-((W + 31) // 32) // p.group)
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS, group=p.group, max_shift=p.max_shift, groups=ng, planted_amp=AMP,
               scratch_bytes=int(aocr.lib.aocr_curl_scratch_bytes(H, W, p.group, p.max_shift)))
    scratch = torch.empty((row["scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    curl = torch.zeros(4, dtype=torch.int32, device=dev)
    shifts = torch.zeros(ng, dtype=torch.int32, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)

    def est():
        aocr.check(aocr.lib.aocr_estimate_curl(st, aocr.ptr(page), W, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(curl), aocr.ptr(shifts), None), "estimate")

    def dewarp():
        aocr.check(aocr.lib.aocr_dewarp_page(st, aocr.ptr(page), W, H, W, p.group, aocr.ptr(shifts), 255, aocr.ptr(out), W), "dewarp")

    def deskew():
        aocr.check(aocr.lib.aocr_deskew_page(st, aocr.ptr(page), W, H, W, None, SLOPE, 255, aocr.ptr(out), W), "deskew")

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        for _ in range(int(sys.argv[2])):
            est()
            dewarp()
            deskew()
        torch.cuda.synchronize()
        return
    est()
    row["curl"], row["shifts"] = curl.cpu().numpy().tolist(), shifts.cpu().numpy().tolist()
    seg = aocr.SegmentParams()
    dewarp()
    row["lines_flat"] = int(aocr.segment_page_device(torch.from_numpy(flat_h).to(dev), seg, 4096)[1][1])
    row["lines_curled"] = int(aocr.segment_page_device(page, seg, 4096)[1][1])
    row["lines_dewarped"] = int(aocr.segment_page_device(out, seg, 4096)[1][1])
    time_rows(row, [("estimate_otsu", est, 50), ("dewarp", dewarp, 50), ("deskew", deskew, 50)])
    row["copy_floor_ms"] = 2 * H * W / HBM_BYTES_PER_S * 1e3                  # one read and one write of the page
    row["dewarp_over_deskew"] = row["dewarp_ms"] / row["deskew_ms"]
    emit(row, "curl")


if __name__ == "__main__":
    main()
