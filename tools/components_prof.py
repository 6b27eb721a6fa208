"""ms per call of aocr_label_components (with the component list) and of aocr_clean_page on a 3508 x 2480 page (A4 at 300 dpi), for three
contents: `text`, the two-column page of tests/layout_cases.py scaled up three times and cut to the sheet (the rows below it take the top of
the same page again); `noise`, the same with 0.1 % of the pixels set to ink at seeded places; `checker`, ink where x + y is even, labelled at
4-connectivity: every ink pixel is a component of its own, the largest number of components a page can hold (at 8-connectivity, also timed,
the same page is one component).  HIP events, warm-up calls, then medians over windows, as tools/segment_prof.py times its calls; next to
the byte floor of each call at the HBM rate: the page read (1 byte per pixel), the labels written and read (4 + 4), and for the cleaning the
output written (1).  As the yardsticks, in the same process, aocr_ink_integral with a fixed threshold and aocr_segment_page with Otsu on the
text page.  Prints one JSON line and writes it to profiles/components_prof.json.
`components_prof.py --trace N CONTENT` instead runs N labelling calls and N cleaning calls on one content (checker: 4-connectivity) and
nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/components_prof.py --trace 100 text`."""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from segment_prof import H, W, HBM_BYTES_PER_S, WINDOWS, emit, time_rows, windows     # noqa: E402  (also puts the package on sys.path)
from layout_cases import two_column_page                                      # noqa: E402
import aocr                                                                   # noqa: E402

MAX_COMPONENTS = 65536


def text_a4():
    big = np.kron(two_column_page(), np.ones((3, 3), np.uint8))               # 2700 x 3000
    page = np.full((H, W), 255, np.uint8)
    page[:big.shape[0]] = big[:, :W]
    page[big.shape[0]:] = big[:H - big.shape[0], :W]
    return page


def pages():
    text = text_a4()
    noise = text.copy()
    rng = np.random.default_rng(35082480)
    idx = rng.choice(H * W, size=H * W // 1000, replace=False)
    noise.reshape(-1)[idx] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    checker = np.where((yy + xx) % 2 == 0, 0, 255).astype(np.uint8)
    return dict(text=(text, 8), noise=(noise, 8), checker=(checker, 4), checker8=(checker, 8))


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    row = dict(H=H, W=W, page_bytes=H * W, windows=WINDOWS, components_scratch_bytes=int(aocr.lib.aocr_components_scratch_bytes(H, W)),
               clean_scratch_bytes=int(aocr.lib.aocr_clean_scratch_bytes(H, W)))
    scratch = torch.empty((row["clean_scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    comps = torch.zeros((MAX_COMPONENTS, 6), dtype=torch.int32, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)

    def label(page, conn):
        aocr.check(aocr.lib.aocr_label_components(st, aocr.ptr(page), W, H, W, 128, 0, conn, aocr.ptr(scratch), aocr.ptr(labels), W, MAX_COMPONENTS,
                                                  aocr.ptr(comps), aocr.ptr(info)), "label")

    def clean(page, conn):
        p = aocr.CleanParams(threshold=128, connectivity=conn)
        aocr.check(aocr.lib.aocr_clean_page(st, aocr.ptr(page), W, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(out), W, aocr.ptr(counts)), "clean")

    content = pages()
    if len(sys.argv) > 3 and sys.argv[1] == "--trace":
        page_h, conn = content[sys.argv[3]]
        page = torch.from_numpy(page_h).to(dev)
        for _ in range(int(sys.argv[2])):
            label(page, conn)
        for _ in range(int(sys.argv[2])):
            clean(page, conn)
        torch.cuda.synchronize()
        return
    row["label_floor_ms"] = 9 * H * W / HBM_BYTES_PER_S * 1e3                 # page read, labels written and read
    row["clean_floor_ms"] = 10 * H * W / HBM_BYTES_PER_S * 1e3                # and the output written
    for name, (page_h, conn) in content.items():
        page = torch.from_numpy(page_h).to(dev)
        label(page, conn)
        clean(page, conn)
        row[name + "_info"], row[name + "_counts"] = info.cpu().tolist(), counts.cpu().tolist()
        iters = 20 if name.startswith("checker") else 50
        for call, fn in (("label", label), ("clean", clean)):
            k = f"{name}_{call}"
            time_rows(row, [(k, lambda: fn(page, conn), iters)])
            row[k + "_over_floor"] = row[k + "_ms"] / row[call + "_floor_ms"]
    page = torch.from_numpy(content["text"][0]).to(dev)
    sat_pitch = (W + 1 + 3) & ~3
    sat = torch.empty((H + 1, sat_pitch), dtype=torch.int32, device=dev)
    iscratch = torch.empty((int(aocr.lib.aocr_integral_scratch_bytes(H, W)) + 7) // 8, dtype=torch.int64, device=dev)
    max_boxes = 4096
    sscratch = torch.empty((int(aocr.lib.aocr_segment_scratch_bytes(H, W, max_boxes)) + 7) // 8, dtype=torch.int64, device=dev)
    boxes = torch.zeros((max_boxes, 6), dtype=torch.int32, device=dev)
    seg_counts = torch.zeros(4, dtype=torch.int32, device=dev)
    seg_p = aocr.SegmentParams()

    def table():
        aocr.check(aocr.lib.aocr_ink_integral(st, aocr.ptr(page), W, H, W, 128, 0, aocr.ptr(iscratch), aocr.ptr(sat), sat_pitch, aocr.ptr(info)), "table")

    def seg():
        aocr.check(aocr.lib.aocr_segment_page(st, aocr.ptr(page), W, H, W, C.byref(seg_p), aocr.ptr(sscratch), max_boxes, aocr.ptr(boxes),
                                              aocr.ptr(seg_counts)), "seg")

    row["integral_fixed_ms"] = statistics.median(windows(table, 50))
    row["segment_otsu_ms"] = statistics.median(windows(seg, 50))
    row["checker_label_over_text_label"] = row["checker_label_ms"] / row["text_label_ms"]
    row["text_label_over_segment"] = row["text_label_ms"] / row["segment_otsu_ms"]
    emit(row, "components")


if __name__ == "__main__":
    main()
