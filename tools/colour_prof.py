"""ms per call of aocr_estimate_page_colour and of aocr_gray_page on a 3508 x 2480 x 3 page (A4 at 300 dpi): the two-column seeded page of
tools/layout_prof.py as black text on paper tinted (250, 240, 200) with its speckle kept, a red rule down the gutter, a yellow band over
the headline and a blue stamp.  As the yardstick, in the same process, the only way to gray on the device without the stage: the torch
expression (rgb.to(float32) * w).sum(-1) rounded to uint8.  HIP events, warm-up calls, then medians over windows, as
tools/segment_prof.py times its calls; next to the floors at the HBM rate: 3 bytes per pixel for the estimate, 4 for the gray pass.  Prints
one JSON line and writes it to profiles/colour_prof.json.
`colour_prof.py --trace N` instead runs N estimates and N gray passes and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/colour_prof.py --trace 300`."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import H, W, HBM_BYTES_PER_S, WINDOWS, emit, time_rows     # noqa: E402  (also puts the package on sys.path)
from layout_prof import GUTTER, HEADLINE_ROWS, two_column_a4                  # noqa: E402
import aocr                                                                   # noqa: E402

TINT = (250, 240, 200)


def colour_a4():
    gray, n_words = two_column_a4()
    rgb = (gray[:, :, None].astype(np.uint32) * np.array(TINT, np.uint32)[None, None, :] // 255).astype(np.uint8)
    band = np.zeros(gray.shape, bool)
    band[40:HEADLINE_ROWS - 40, 200:W - 200] = True
    rgb[band & (gray > 128)] = (250, 230, 40)
    rgb[400:, (GUTTER[0] + GUTTER[1]) // 2] = (230, 20, 20)
    rgb[3000:3200, 1800:2300][gray[3000:3200, 1800:2300] > 128] = (30, 40, 220)
    return rgb, n_words


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    rgb_h, n_words = colour_a4()
    rgb = torch.from_numpy(rgb_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    row = dict(H=H, W=W, page_bytes=3 * H * W, words_pasted=n_words, windows=WINDOWS,
               colour_scratch_bytes=int(aocr.lib.aocr_colour_scratch_bytes(H, W)))
    scratch = torch.empty((row["colour_scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    words = torch.zeros(16, dtype=torch.int32, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    cp = aocr.ColourParams(drop=(1 << aocr.HUE_RED) | (1 << aocr.HUE_YELLOW) | (1 << aocr.HUE_BLUE))
    luma = torch.tensor([0.299, 0.587, 0.114], dtype=torch.float32, device=dev)

    def estimate():
        aocr.check(aocr.lib.aocr_estimate_page_colour(st, aocr.ptr(rgb), 3 * W, H, W, C.byref(cp), aocr.ptr(scratch), aocr.ptr(words)), "estimate")

    def gray():
        aocr.check(aocr.lib.aocr_gray_page(st, aocr.ptr(rgb), 3 * W, H, W, C.byref(cp), aocr.ptr(words), aocr.ptr(words), aocr.ptr(out), W), "gray")

    def torch_luma():
        return ((rgb.to(torch.float32) * luma).sum(-1) + 0.5).to(torch.uint8)

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        for _ in range(int(sys.argv[2])):
            estimate()
        for _ in range(int(sys.argv[2])):
            gray()
        torch.cuda.synchronize()
        return
    estimate()
    gray()
    w = words.cpu().tolist()
    row["paper"], row["hues"], row["dropped"] = w[:3], w[4:10], w[10]
    row["paper_pixels_are_white"] = bool(int((out == 255).sum()) > H * W // 2)
    time_rows(row, [("estimate", estimate, 50), ("gray", gray, 50), ("torch_luma", torch_luma, 20)])
    row["estimate_floor_ms"] = 3 * H * W / HBM_BYTES_PER_S * 1e3                # one read of the page
    row["gray_floor_ms"] = 4 * H * W / HBM_BYTES_PER_S * 1e3                    # one read of the page and one write of the gray page
    row["estimate_over_floor"] = row["estimate_ms"] / row["estimate_floor_ms"]
    row["gray_over_floor"] = row["gray_ms"] / row["gray_floor_ms"]
    row["torch_luma_over_gray"] = row["torch_luma_ms"] / row["gray_ms"]
    emit(row, "colour")


if __name__ == "__main__":
    main()
