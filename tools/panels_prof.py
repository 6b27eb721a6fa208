"""ms per call of aocr_invert_panels (the defaults, Otsu) next to aocr_label_components and aocr_clean_page on the same page in the same
process: the seeded A4 page of tools/segment_prof.py (3508 x 2480) with four bands of lines reversed out (a dark slab across the text
block, its words light).  The new call shares the two yardsticks' labelling, so what it costs beyond aocr_label_components is the cost of
the new kernels.  HIP events, warm-up calls, then medians over windows, as tools/segment_prof.py times its calls; every call is timed in two
passes.  The byte floor is one page read and one page written.  Prints one JSON line and writes it to profiles/panels_prof.json.
`panels_prof.py --trace N` instead runs N calls of aocr_invert_panels and nothing else: under
`rocprofv3 --kernel-trace --stats -- python tools/panels_prof.py --trace 100` the pn_* rows of the stats file are the new kernels alone
(profiles/panels_kernel_stats.csv)."""
import ctypes as C
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import HBM_BYTES_PER_S, WINDOWS, a4_page, emit, time_rows   # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

MAX_PANELS = 256
BANDS = ((400, 520), (1200, 1290), (2000, 2260), (3000, 3060))                # rows of the slabs


def panel_page():
    page, n_words = a4_page()
    H, W = page.shape
    for y0, y1 in BANDS:
        page[y0:y1, 120:W - 120] = 255 - page[y0:y1, 120:W - 120]
    return page, n_words


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = panel_page()
    H, W = page_h.shape
    page = torch.from_numpy(page_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cp, pp = aocr.CleanParams(), aocr.PanelParams()
    need = max(int(aocr.lib.aocr_clean_scratch_bytes(H, W)), int(aocr.lib.aocr_components_scratch_bytes(H, W)),
               int(aocr.lib.aocr_panels_scratch_bytes(H, W, MAX_PANELS)))
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    rows = torch.zeros((MAX_PANELS, 8), dtype=torch.int32, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)

    def panels():
        aocr.check(aocr.lib.aocr_invert_panels(st, aocr.ptr(page), W, H, W, C.byref(pp), aocr.ptr(scratch), aocr.ptr(out), W, MAX_PANELS, aocr.ptr(rows),
                                               aocr.ptr(counts)), "panels")

    def label():
        aocr.check(aocr.lib.aocr_label_components(st, aocr.ptr(page), W, H, W, -1, 0, 8, aocr.ptr(scratch), aocr.ptr(labels), W, 1, None, aocr.ptr(info)),
                   "label")

    def clean():
        aocr.check(aocr.lib.aocr_clean_page(st, aocr.ptr(page), W, H, W, C.byref(cp), aocr.ptr(scratch), aocr.ptr(out), W, aocr.ptr(counts)), "clean")

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        for _ in range(int(sys.argv[2])):
            panels()
        torch.cuda.synchronize()
        return
    panels()
    got, got_rows = counts.cpu().numpy().copy(), rows.cpu().numpy().copy()
    floor_bytes = 2 * H * W
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS, max_panels=MAX_PANELS, bands=len(BANDS),
               panels_scratch_bytes=int(aocr.lib.aocr_panels_scratch_bytes(H, W, MAX_PANELS)),
               clean_scratch_bytes=int(aocr.lib.aocr_clean_scratch_bytes(H, W)), counts=[int(v) for v in got],
               accepted=[[int(v) for v in r] for r in got_rows[:int(got[2])] if r[7]], floor_bytes=floor_bytes,
               floor_ms=floor_bytes / HBM_BYTES_PER_S * 1e3)
    fns = [("panels", panels, 20), ("label", label, 20), ("clean", clean, 20)]
    time_rows(row, fns + [(name + "_again", fn, iters) for name, fn, iters in fns])          # a second pass: drift between passes is the noise floor
    row["panels_over_clean"] = row["panels_ms"] / row["clean_ms"]
    row["panels_over_label"] = row["panels_ms"] / row["label_ms"]
    row["new_kernels_ms"] = row["panels_ms"] - row["label_ms"]
    row["new_kernels_over_floor"] = row["new_kernels_ms"] / row["floor_ms"]
    emit(row, "panels")


if __name__ == "__main__":
    main()
