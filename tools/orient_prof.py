"""ms per call of aocr_rotate_page (q = 1, 2, 3) and of aocr_estimate_orientation (fixed threshold and Otsu) on the seeded 3508 x 2480 page
(A4 at 300 dpi) of tools/segment_prof.py.  As the yardstick, in the same process and on the same page, aocr_deskew_page at slope 0.01: the
other page kernel that reads and writes one byte per pixel.  HIP events, warm-up calls, then medians over windows, as tools/segment_prof.py
times its calls; next to the byte floor at the HBM rate: 2 bytes per pixel for the rotation, 1 for the estimate.  The page and its copy
(17 MB) fit in the Infinity Cache, so a call may beat that floor.  Prints one JSON line and writes it to profiles/orient_prof.json.
`orient_prof.py --trace N` instead runs N quarter turns (q = 1) and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/orient_prof.py --trace 300`."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import H, W, HBM_BYTES_PER_S, WINDOWS, a4_page, emit, time_rows     # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = a4_page()
    page = torch.from_numpy(page_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS, orient_scratch_bytes=int(aocr.lib.aocr_orient_scratch_bytes(H, W)))
    out = torch.empty(H * W, dtype=torch.uint8, device=dev)
    scratch = torch.empty((row["orient_scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    words = torch.zeros(8, dtype=torch.int32, device=dev)

    def rotate(q):
        aocr.check(aocr.lib.aocr_rotate_page(st, aocr.ptr(page), W, H, W, None, q, aocr.ptr(out), H if q & 1 else W), "rotate")

    def estimate(thr):
        aocr.check(aocr.lib.aocr_estimate_orientation(st, aocr.ptr(page), W, H, W, thr, 0, aocr.ptr(scratch), aocr.ptr(words)), "estimate")

    def deskew():
        aocr.check(aocr.lib.aocr_deskew_page(st, aocr.ptr(page), W, H, W, None, 655, 255, aocr.ptr(out), W), "deskew")

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        for _ in range(int(sys.argv[2])):
            rotate(1)
        torch.cuda.synchronize()
        return
    for q in (1, 2, 3):                                                       # what is timed is also right
        rotate(q)
        shape = (W, H) if q & 1 else (H, W)
        row[f"rotate_q{q}_matches_rot90"] = bool(np.array_equal(out.cpu().numpy().reshape(shape), np.rot90(page_h, -q)))
    estimate(-1)
    row["orient_words"] = words.cpu().tolist()
    time_rows(row, [("rotate_q1", lambda: rotate(1), 50), ("rotate_q2", lambda: rotate(2), 50), ("rotate_q3", lambda: rotate(3), 50),
                    ("estimate_fixed", lambda: estimate(128), 50), ("estimate_otsu", lambda: estimate(-1), 50), ("deskew", deskew, 50)])
    row["rotate_floor_ms"] = 2 * H * W / HBM_BYTES_PER_S * 1e3                # one read and one write of the page
    row["estimate_floor_ms"] = H * W / HBM_BYTES_PER_S * 1e3                  # one read
    for q in (1, 2, 3):
        row[f"rotate_q{q}_over_deskew"] = row[f"rotate_q{q}_ms"] / row["deskew_ms"]
        row[f"rotate_q{q}_over_floor"] = row[f"rotate_q{q}_ms"] / row["rotate_floor_ms"]
    row["estimate_fixed_over_floor"] = row["estimate_fixed_ms"] / row["estimate_floor_ms"]
    row["estimate_otsu_over_floor"] = row["estimate_otsu_ms"] / row["estimate_floor_ms"]
    row["estimate_otsu_over_deskew"] = row["estimate_otsu_ms"] / row["deskew_ms"]
    emit(row, "orient")


if __name__ == "__main__":
    main()
