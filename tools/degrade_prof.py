"""ms per launch of aocr_degrade_lines (every stage on, and the identity record) next to aocr_augment_lines on the same tensor -- the parent
of this kernel has no such stage, so the neighbouring data stage is the yardstick -- for the C3 batch (256 x 32 x 256) and c5's (16 x 128 x
1024).  HIP events on the current stream, warm-up launches of every call, then WINDOWS windows of ITERS launches per call in alternation,
median and spread; next to the floor: one read and one write of the batch at the HBM rate a streaming copy reaches.  Prints one JSON line
and writes it to profiles/degrade_prof.json.
`degrade_prof.py --trace N` instead runs N degrade launches per shape and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/degrade_prof.py --trace 300`."""
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from segment_prof import HBM_BYTES_PER_S                                      # noqa: E402  (also puts the package on sys.path)
import aocr                                                                   # noqa: E402

SHAPES = {"c3": (256, 32, 256), "c5": (16, 128, 1024)}
ITERS, WINDOWS, WARMUP = int(os.environ.get("ITERS", "2000")), int(os.environ.get("WINDOWS", "7")), 20


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev).cuda_stream
    D = aocr.Degrader(blur_sigma=1.5, thickness=0.8, elastic=(2.0, 1.5), pitch=8)
    A = aocr.Augmenter(rotate_deg=8, shear=0.2, scale=1.2, translate=(6, 2), contrast=1.5, brightness=20, noise=12)
    up = lambda rec: torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    row = dict(launches_per_window=ITERS, windows=WINDOWS, hbm_bytes_per_s=HBM_BYTES_PER_S)
    for name, (B, H, W) in SHAPES.items():
        images = torch.randint(0, 256, (B, 1, H, W), device=dev).float()
        out = torch.empty_like(images)
        rec, ident, warp = up(D.params(B, H, W, 0)), up(aocr.Degrader().params(B, H, W, 0)), up(A.params(B, H, W, 0))
        calls = {
            "degrade": lambda: aocr.check(aocr.lib.aocr_degrade_lines(st, aocr.ptr(images), aocr.ptr(rec), B, H, W, D.seed, 0, aocr.ptr(out))),
            "degrade_identity": lambda: aocr.check(aocr.lib.aocr_degrade_lines(st, aocr.ptr(images), aocr.ptr(ident), B, H, W, D.seed, 0, aocr.ptr(out))),
            "augment": lambda: aocr.check(aocr.lib.aocr_augment_lines(st, aocr.ptr(images), aocr.ptr(warp), B, H, W, A.seed, 0, aocr.ptr(out))),
        }
        if len(sys.argv) > 2 and sys.argv[1] == "--trace":
            for _ in range(int(sys.argv[2])):
                calls["degrade"]()
            torch.cuda.synchronize()
            continue
        calls["degrade_identity"]()
        identity_ok = bool(torch.equal(out, images))
        for fn in calls.values():
            for _ in range(WARMUP):
                fn()
        ms = {k: [] for k in calls}
        for _ in range(WINDOWS):
            for k, fn in calls.items():
                ms[k].append(window(fn))
        r = dict(shape=[B, 1, H, W], identity_returns_input=identity_ok, floor_ms=2 * B * H * W * 4 / HBM_BYTES_PER_S * 1e3)
        for k, v in ms.items():
            r[k + "_ms"], r[k + "_ms_min"], r[k + "_ms_max"] = statistics.median(v), min(v), max(v)
        r["degrade_over_augment"] = r["degrade_ms"] / r["augment_ms"]
        r["degrade_over_floor"] = r["degrade_ms"] / r["floor_ms"]
        r["augment_over_floor"] = r["augment_ms"] / r["floor_ms"]
        row[name] = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items()}
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        return
    line = json.dumps(row)
    print(line, flush=True)
    with open(os.path.join(HERE, "..", "profiles", "degrade_prof.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
