"""ms per call of aocr_segment_page (Otsu and fixed threshold) and of aocr_crop_lines on a seeded 3508 x 2480 page (A4 at 300 dpi) assembled
from GlyphAtlas.default() words, timed with HIP events in one process (as tools/lexicon_prof.py times its calls), next to the floor: the
page's bytes over the HBM rate.  The whole call is timed in three variants: Otsu, fixed threshold (no histogram and no Otsu launch) and a
fixed threshold on a page of paper (the row profile reads the page, the later kernels find nothing).  Every window is warmed up and
repeated; the JSON line carries the median and the spread.
`segment_prof.py --trace N` instead runs N Otsu calls and N crop calls on the text page and nothing else: under
`rocprofv3 --kernel-trace --stats -- python tools/segment_prof.py --trace 300` the per-kernel averages of the stats file are those of one
kind of call, not a mixture (profiles/segment_kernel_stats.csv)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torch-attention-ocr_amd"))
import aocr

H, W = 3508, 2480
WINDOWS, WARMUP = int(os.environ.get("WINDOWS", "7")), 10
HBM_BYTES_PER_S = 6.3e12                                  # what a streaming copy reaches on one MI355X (8 TB/s on paper)
CHARS = "0123456789abcdefghijklmnopqrstuvwxyz"


def windows(fn, iters):
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def time_rows(row, named_fns):
    """row[name + "_ms"], "_ms_min" and "_ms_max": the median, least and greatest window of fn, for every (name, fn, iters), in that order."""
    for name, fn, iters in named_fns:
        t = windows(fn, iters)
        row[name + "_ms"], row[name + "_ms_min"], row[name + "_ms_max"] = statistics.median(t), min(t), max(t)


def emit(row, stage):
    """the row as one JSON line, floats rounded to 5 places: printed, and written to profiles/<stage>_prof.json."""
    line = json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()})
    print(line, flush=True)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", stage + "_prof.json"), "w") as f:
        f.write(line + "\n")


def a4_page(seed=300):
    """lines of atlas words at 40..56 px pitch with 18..30 px between words, 150 px margins; glyphs at their atlas size (32 px high)."""
    atlas = aocr.GlyphAtlas.default()
    rng = np.random.default_rng(seed)
    page = np.full((H, W), 255, np.uint8)
    y, n_words = 150, 0
    while y + atlas.gh < H - 150:
        x = 150 + int(rng.integers(0, 60))
        face = int(rng.integers(0, atlas.n_faces))
        while True:
            gi = rng.integers(0, len(CHARS), size=int(rng.integers(2, 11)))
            adv = [int(atlas.advance[face, g]) for g in gi]
            if x + sum(adv) + atlas.gw >= W - 150:
                break
            pen = x
            for g, a in zip(gi, adv):
                page[y:y + atlas.gh, pen:pen + atlas.gw] = np.minimum(page[y:y + atlas.gh, pen:pen + atlas.gw], 255 - atlas.pixels[face, g])
                pen += a
            x = pen + int(rng.integers(18, 31))
            n_words += 1
        y += atlas.gh + int(rng.integers(8, 25))
    return page, n_words


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    page_h, n_words = a4_page()
    page = torch.from_numpy(page_h).to(dev)
    max_boxes = 4096
    row = dict(H=H, W=W, page_bytes=H * W, words_pasted=n_words, max_boxes=max_boxes, windows=WINDOWS,
               scratch_bytes=int(aocr.lib.aocr_segment_scratch_bytes(H, W, max_boxes)))
    otsu, fixed = aocr.SegmentParams(), aocr.SegmentParams(threshold=128)
    boxes, counts = aocr.segment_page_device(page, otsu, max_boxes)
    c = counts.cpu().numpy()
    row["boxes_found"], row["lines"], row["threshold"] = int(c[0]), int(c[1]), int(c[2])
    # the Python wrapper allocates its scratch and outputs per call (torch's caching allocator: no device allocation after the first);
    # the C call is timed on its own with everything preallocated
    import ctypes as C
    scratch = torch.empty((row["scratch_bytes"] + 7) // 8, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def seg(p, pg=page):
        aocr.check(aocr.lib.aocr_segment_page(st, aocr.ptr(pg), W, H, W, C.byref(p), aocr.ptr(scratch), max_boxes, aocr.ptr(boxes), aocr.ptr(counts)), "seg")

    out = torch.empty((max_boxes, 1, 32, 100), dtype=torch.float32, device=dev)

    def crop():
        aocr.check(aocr.lib.aocr_crop_lines(st, aocr.ptr(page), W, H, W, aocr.ptr(boxes), aocr.ptr(counts), max_boxes, 32, 100, aocr.ptr(out)), "crop")

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        for _ in range(int(sys.argv[2])):
            seg(otsu)
            crop()
        torch.cuda.synchronize()
        return
    time_rows(row, [("segment_otsu", lambda: seg(otsu), 50), ("segment_fixed", lambda: seg(fixed), 50)])
    blank = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
    t = windows(lambda: seg(fixed, blank), 50)                  # no ink: the row profile reads the page, every later kernel finds nothing to do
    row["segment_fixed_blank_page_ms"] = statistics.median(t)
    t = windows(lambda: aocr.segment_page_device(page, otsu, max_boxes), 50)
    row["segment_page_device_ms"] = statistics.median(t)
    seg(otsu)
    n = int(min(c[0], max_boxes))
    t = windows(crop, 50)
    row["crop_ms"], row["crop_ms_min"], row["crop_ms_max"], row["crops"] = statistics.median(t), min(t), max(t), n
    row["hbm_floor_ms"] = H * W / HBM_BYTES_PER_S * 1e3         # one read of the page
    row["segment_otsu_page_reads"] = 3                          # histogram, row profile, column profiles (the last one only inside the bands)
    row["segment_otsu_over_floor"] = row["segment_otsu_ms"] / (3 * row["hbm_floor_ms"])
    row["crop_out_bytes"] = n * 32 * 100 * 4
    print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
