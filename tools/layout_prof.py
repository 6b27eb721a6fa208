"""ms per call of aocr_ink_integral (Otsu and fixed threshold) and of aocr_layout_blocks on a two-column 3508 x 2480 page (A4 at 300 dpi)
made of the seeded page of tools/segment_prof.py: its first lines stay as a headline across the page, a band of clear rows follows, and below
it an 80-column gutter is cleared down the middle.  As the yardstick, in the same process, aocr_segment_page with Otsu on the same page.
HIP events, warm-up calls, then medians over windows, as tools/segment_prof.py times its calls; next to the floor: one page read and one
table write (5 bytes per pixel) at the HBM rate.  Prints one JSON line and writes it to profiles/layout_prof.json.
`layout_prof.py --trace N` instead runs N table calls (Otsu) and N cuts and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/layout_prof.py --trace 300`."""
import ctypes as C
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import H, W, HBM_BYTES_PER_S, WINDOWS, a4_page, emit, time_rows     # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

HEADLINE_ROWS, BODY_ROW, GUTTER = 330, 400, (1200, 1280)


def two_column_a4():
    page, n_words = a4_page()
    page = page.copy()
    page[HEADLINE_ROWS:BODY_ROW, :] = 255
    page[BODY_ROW:, GUTTER[0]:GUTTER[1]] = 255
    return page, n_words


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = two_column_a4()
    page = torch.from_numpy(page_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    max_blocks, max_boxes = 256, 4096
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS,
               integral_scratch_bytes=int(aocr.lib.aocr_integral_scratch_bytes(H, W)),
               layout_scratch_bytes=int(aocr.lib.aocr_layout_scratch_bytes(H, W, max_blocks)))
    scratch = torch.empty((row["integral_scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    lscratch = torch.empty((row["layout_scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    sat_pitch = (W + 1 + 3) & ~3
    sat = torch.empty((H + 1, sat_pitch), dtype=torch.int32, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    blocks = torch.zeros((max_blocks, 6), dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    lp = aocr.LayoutParams(gap_x=40)

    def table(thr):
        aocr.check(aocr.lib.aocr_ink_integral(st, aocr.ptr(page), W, H, W, thr, 0, aocr.ptr(scratch), aocr.ptr(sat), sat_pitch, aocr.ptr(info)), "table")

    def cut():
        aocr.check(aocr.lib.aocr_layout_blocks(st, aocr.ptr(sat), sat_pitch, H, W, C.byref(lp), aocr.ptr(lscratch), max_blocks, aocr.ptr(blocks),
                                               aocr.ptr(counts)), "cut")

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        for _ in range(int(sys.argv[2])):
            table(-1)
        for _ in range(int(sys.argv[2])):
            cut()
        torch.cuda.synchronize()
        return
    seg_scratch = torch.empty((int(aocr.lib.aocr_segment_scratch_bytes(H, W, max_boxes)) + 7) // 8, dtype=torch.int64, device=dev)
    boxes = torch.zeros((max_boxes, 6), dtype=torch.int32, device=dev)
    seg_counts = torch.zeros(4, dtype=torch.int32, device=dev)
    seg_p = aocr.SegmentParams()

    def seg():
        aocr.check(aocr.lib.aocr_segment_page(st, aocr.ptr(page), W, H, W, C.byref(seg_p), aocr.ptr(seg_scratch), max_boxes, aocr.ptr(boxes),
                                              aocr.ptr(seg_counts)), "seg")

    table(-1)
    cut()
    row["threshold"], row["ink"] = int(info[0]), int(info[1])
    row["table_total_matches_mask"] = bool(int(info[1]) == int((page <= int(info[0])).sum()))
    row["layout_counts"] = counts.cpu().tolist()
    row["blocks"] = blocks[:int(counts[0])].cpu().tolist()
    time_rows(row, [("integral_otsu", lambda: table(-1), 50), ("integral_fixed", lambda: table(128), 50), ("layout_blocks", cut, 20),
                    ("segment_otsu", seg, 50)])
    row["floor_ms"] = 5 * H * W / HBM_BYTES_PER_S * 1e3                       # one read of the page and one write of the table
    row["integral_fixed_over_floor"] = row["integral_fixed_ms"] / row["floor_ms"]
    row["integral_otsu_over_floor"] = row["integral_otsu_ms"] / row["floor_ms"]
    row["integral_otsu_over_segment"] = row["integral_otsu_ms"] / row["segment_otsu_ms"]
    row["layout_blocks_over_segment"] = row["layout_blocks_ms"] / row["segment_otsu_ms"]
    emit(row, "layout")


if __name__ == "__main__":
    main()
