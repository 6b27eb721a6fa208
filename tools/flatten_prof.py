"""ms per call of aocr_flatten_page at radius 16 and 48 on the seeded 3508 x 2480 page of tools/segment_prof.py (A4 at 300 dpi) repainted
as ink 40 on paper 230 under a lighting gradient that falls to 110/256 at the right edge, and, as yardsticks in the same process, of
aocr_segment_page and aocr_estimate_skew (both with Otsu) on the flattened page.  HIP events, warm-up calls, then medians over windows, as
tools/segment_prof.py times its calls; next to the floor: one page read and one page write at the HBM rate.  Prints one JSON line and
writes it to profiles/flatten_prof.json.
`flatten_prof.py --trace N [radius]` instead runs N flatten calls and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/flatten_prof.py --trace 300`."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import H, W, HBM_BYTES_PER_S, WINDOWS, a4_page, emit, time_rows     # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

FLOOR = 110


def lit_a4():
    page, n_words = a4_page()
    gray = (40 + (page.astype(np.int64) * 190) // 255)                        # ink 40, paper 230, the glyph edges in between
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    L = 256 - ((256 - FLOOR) * x) // (W - 1) - (20 * y) // (H - 1)
    return ((gray * L) >> 8).astype(np.uint8), page, n_words


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    lit_h, clean_h, n_words = lit_a4()
    page = torch.from_numpy(lit_h).to(dev)
    clean = torch.from_numpy(clean_h).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, windows=WINDOWS, floor=FLOOR,
               scratch_bytes=int(aocr.lib.aocr_flatten_scratch_bytes(H, W, 16)))
    scratch = torch.empty((row["scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)

    def flat(r, pg=page):
        p = aocr.FlattenParams(radius=r)
        aocr.check(aocr.lib.aocr_flatten_page(st, aocr.ptr(pg), W, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(out), W), "flatten")

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        r = int(sys.argv[3]) if len(sys.argv) > 3 else 16
        for _ in range(int(sys.argv[2])):
            flat(r)
        torch.cuda.synchronize()
        return
    max_boxes = 4096
    seg_scratch = torch.empty((int(aocr.lib.aocr_segment_scratch_bytes(H, W, max_boxes)) + 7) // 8, dtype=torch.int64, device=dev)
    boxes = torch.zeros((max_boxes, 6), dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    seg_p, skew_p = aocr.SegmentParams(), aocr.SkewParams()
    skew_scratch = torch.empty((int(aocr.lib.aocr_skew_scratch_bytes(H, W, skew_p.n_steps)) + 7) // 8, dtype=torch.int64, device=dev)
    skew = torch.zeros(4, dtype=torch.int32, device=dev)

    def seg(pg):
        aocr.check(aocr.lib.aocr_segment_page(st, aocr.ptr(pg), W, H, W, C.byref(seg_p), aocr.ptr(seg_scratch), max_boxes, aocr.ptr(boxes), aocr.ptr(counts)), "seg")

    def est(pg):
        aocr.check(aocr.lib.aocr_estimate_skew(st, aocr.ptr(pg), W, H, W, C.byref(skew_p), aocr.ptr(skew_scratch), aocr.ptr(skew), None), "estimate")

    seg(clean)
    row["lines_clean"], row["boxes_clean"] = int(counts[1]), int(counts[0])
    seg(page)
    row["lines_lit"], row["boxes_lit"], row["threshold_lit"] = int(counts[1]), int(counts[0]), int(counts[2])
    for r in (16, 48):
        flat(r)
        seg(out)
        row[f"lines_flat_r{r}"], row[f"boxes_flat_r{r}"], row[f"threshold_flat_r{r}"] = int(counts[1]), int(counts[0]), int(counts[2])
    flat(16, clean)
    row["clean_page_unchanged"] = bool(torch.equal(out, clean))
    flat(16)
    time_rows(row, [("flatten_r16", lambda: flat(16), 50), ("flatten_r48", lambda: flat(48), 50), ("flatten_r127", lambda: flat(127), 50),
                    ("segment_otsu", lambda: seg(out), 50), ("estimate_otsu", lambda: est(out), 50)])
    row["floor_ms"] = 2 * H * W / HBM_BYTES_PER_S * 1e3                       # one read and one write of the page
    row["r48_over_r16"] = row["flatten_r48_ms"] / row["flatten_r16_ms"]
    row["flatten_r16_over_floor"] = row["flatten_r16_ms"] / row["floor_ms"]
    row["flatten_r16_over_segment"] = row["flatten_r16_ms"] / row["segment_otsu_ms"]
    emit(row, "flatten")


if __name__ == "__main__":
    main()
