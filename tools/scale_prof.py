"""ms per call of aocr_resize_page (to 1/2 and to 2x) and of aocr_estimate_glyph_size (Otsu) on the seeded 3508 x 2480 page (A4 at 300 dpi)
of tools/segment_prof.py.  As yardsticks, in the same process and on the same page, aocr_deskew_page at slope 0.01 (one read and one write
of the page, also a gather) and aocr_label_components with Otsu (what the estimate runs first).  HIP events, warm-up calls, then medians
over windows, as tools/segment_prof.py times its calls; GB/s counts the bytes each call must move: H*W + Ho*Wo for the resize, 2*H*W for
the deskew, one read of the page for the estimate and the labelling (their scratch traffic is several times that).  No pass/fail gate.
Prints one JSON line and writes it to profiles/scale_prof.json."""
import ctypes as C
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import H, W, WINDOWS, a4_page, emit, time_rows             # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = a4_page()
    page = torch.from_numpy(page_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS,
               glyph_scratch_bytes=int(aocr.lib.aocr_glyph_scratch_bytes(H, W)))
    scratch = torch.empty((row["glyph_scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    words = torch.zeros(8, dtype=torch.int32, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    gp = aocr.GlyphParams()
    sizes = {"half": (W // 2, H // 2), "twice": (2 * W, 2 * H)}
    out = torch.empty(4 * H * W, dtype=torch.uint8, device=dev)

    def resize(name):
        Wo, Ho = sizes[name]
        aocr.check(aocr.lib.aocr_resize_page(st, aocr.ptr(page), W, H, W, aocr.ptr(out), Wo, Ho, Wo), "resize_page")

    def glyph():
        aocr.check(aocr.lib.aocr_estimate_glyph_size(st, aocr.ptr(page), W, H, W, C.byref(gp), aocr.ptr(scratch), aocr.ptr(words)), "glyph_size")

    def label():
        aocr.check(aocr.lib.aocr_label_components(st, aocr.ptr(page), W, H, W, -1, 0, 8, aocr.ptr(scratch), aocr.ptr(labels), W, 1, None,
                                                  aocr.ptr(info)), "label_components")

    def deskew():
        aocr.check(aocr.lib.aocr_deskew_page(st, aocr.ptr(page), W, H, W, None, 655, 255, aocr.ptr(out), W), "deskew")

    glyph()
    row["glyph_words"] = words.cpu().tolist()
    row["plan_native"] = aocr.scale_plan(row["glyph_words"][0], row["glyph_words"][3], H, W)
    time_rows(row, [("resize_half", lambda: resize("half"), 50), ("resize_twice", lambda: resize("twice"), 50), ("glyph_otsu", glyph, 20),
                    ("label_otsu", label, 20), ("deskew", deskew, 50)])
    for name in sizes:
        Wo, Ho = sizes[name]
        row[f"resize_{name}_gb_s"] = (H * W + Ho * Wo) / row[f"resize_{name}_ms"] * 1e-6
        row[f"resize_{name}_ns_per_out_pixel"] = row[f"resize_{name}_ms"] * 1e6 / (Ho * Wo)
    row["deskew_gb_s"] = 2 * H * W / row["deskew_ms"] * 1e-6
    row["glyph_otsu_gb_s"] = H * W / row["glyph_otsu_ms"] * 1e-6
    row["label_otsu_gb_s"] = H * W / row["label_otsu_ms"] * 1e-6
    for name in sizes:
        row[f"resize_{name}_over_deskew"] = row[f"resize_{name}_ms"] / row["deskew_ms"]
        row[f"resize_{name}_per_byte_over_deskew"] = row["deskew_gb_s"] / row[f"resize_{name}_gb_s"]
    row["glyph_over_label"] = row["glyph_otsu_ms"] / row["label_otsu_ms"]
    emit(row, "scale")


if __name__ == "__main__":
    main()
