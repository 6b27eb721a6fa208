"""ms per call of aocr_find_page_quad (Otsu and a fixed threshold) and of aocr_warp_page on a 3508 x 2480 photograph (A4 at 300 dpi): the
seeded page of tools/segment_prof.py with everything outside a keystone quad painted as a dark desk.  As yardsticks, in the same process
and on the same page, aocr_deskew_page at slope 0.01 (the same bytes in and out, also a gather) and aocr_rotate_page (q = 1).  HIP events,
warm-up calls, then medians over windows, as tools/segment_prof.py times its calls; GB/s counts one read and one write of a page-sized
image for the warp, the deskew and the rotation, and one read of the page for the quad (its scratch traffic is several times that).  No
pass/fail gate.  Prints one JSON line and writes it to profiles/rectify_prof.json."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import H, W, WINDOWS, a4_page, emit, time_rows             # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

QUAD = [150, 100, W - 200, 60, W - 80, H - 90, 60, H - 150]                   # TL, TR, BR, BL


def photograph():
    page, n_words = a4_page()
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    paper = np.ones((H, W), bool)
    for i in range(4):
        ax, ay, bx, by = QUAD[2 * i], QUAD[2 * i + 1], QUAD[(2 * i + 2) % 8], QUAD[(2 * i + 3) % 8]
        paper &= (bx - ax) * (y - ay) - (by - ay) * (x - ax) >= 0
    return np.where(paper, page, 40).astype(np.uint8), n_words


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    photo_h, n_words = photograph()
    page = torch.from_numpy(photo_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS, quad=QUAD,
               quad_scratch_bytes=int(aocr.lib.aocr_quad_scratch_bytes(H, W)))
    scratch = torch.empty((row["quad_scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    words = torch.zeros(16, dtype=torch.int32, device=dev)

    def find(thr):
        aocr.check(aocr.lib.aocr_find_page_quad(st, aocr.ptr(page), W, H, W, thr, 0, aocr.ptr(scratch), aocr.ptr(words)), "find_page_quad")

    find(-1)
    row["quad_words"] = words.cpu().tolist()
    row["quad_found"] = row["quad_words"][:8] == QUAD
    (Wo, Ho), coef = aocr.rectify_plan(row["quad_words"][:8])
    row["Wo"], row["Ho"] = Wo, Ho
    cc = (C.c_double * 9)(*coef.tolist())
    out = torch.empty(max(H * W, Ho * Wo), dtype=torch.uint8, device=dev)

    def warp():
        aocr.check(aocr.lib.aocr_warp_page(st, aocr.ptr(page), W, H, W, cc, 255, aocr.ptr(out), Wo, Ho, Wo), "warp_page")

    def deskew():
        aocr.check(aocr.lib.aocr_deskew_page(st, aocr.ptr(page), W, H, W, None, 655, 255, aocr.ptr(out), W), "deskew")

    def rotate():
        aocr.check(aocr.lib.aocr_rotate_page(st, aocr.ptr(page), W, H, W, None, 1, aocr.ptr(out), H), "rotate")

    time_rows(row, [("find_quad_otsu", lambda: find(-1), 20), ("find_quad_fixed", lambda: find(128), 20), ("warp", warp, 50),
                    ("deskew", deskew, 50), ("rotate_q1", rotate, 50)])
    row["warp_gb_s"] = (H * W + Ho * Wo) / row["warp_ms"] * 1e-6
    row["deskew_gb_s"] = 2 * H * W / row["deskew_ms"] * 1e-6
    row["rotate_q1_gb_s"] = 2 * H * W / row["rotate_q1_ms"] * 1e-6
    row["find_quad_otsu_gb_s"] = H * W / row["find_quad_otsu_ms"] * 1e-6
    row["find_quad_fixed_gb_s"] = H * W / row["find_quad_fixed_ms"] * 1e-6
    row["warp_over_deskew"] = row["warp_ms"] / row["deskew_ms"]
    row["warp_ns_per_pixel"] = row["warp_ms"] * 1e6 / (Ho * Wo)
    row["find_quad_otsu_over_deskew"] = row["find_quad_otsu_ms"] / row["deskew_ms"]
    emit(row, "rectify")


if __name__ == "__main__":
    main()
