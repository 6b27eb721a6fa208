"""ms per launch of aocr_augment_lines against aocr_preprocess_lines for the same output shape: the C3 batch (256 x 32 x 256; the
preprocess call scales 48x384x3 sources, as bench.py's data-path leg does), HIP events on the current stream, ITERS launches per
window after warm-up, REPEATS windows of each call in alternation.  Prints one JSON line."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torch-attention-ocr_amd"))
import aocr
from aocr.data import ImageDesc

B, H, W, SH, SW = 256, 32, 256, 48, 384
ITERS, REPEATS, WARMUP = int(os.environ.get("ITERS", "200")), int(os.environ.get("REPEATS", "5")), 10


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev).cuda_stream
src = torch.randint(0, 256, (B * SH * SW * 3,), dtype=torch.uint8, device=dev)
desc = (ImageDesc * B)(*[ImageDesc(i * SH * SW * 3, SH, SW, 3, 0) for i in range(B)])
dsc = torch.from_numpy(np.frombuffer(bytes(desc), np.uint8).copy()).to(dev)
images = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
out = torch.empty_like(images)
A = aocr.Augmenter(rotate_deg=8, shear=0.2, scale=1.2, translate=(6, 2), contrast=1.5, brightness=20, noise=12)
warp = torch.from_numpy(A.params(B, H, W, 0).view(np.uint8).copy()).to(dev)
ident = torch.from_numpy(aocr.Augmenter().params(B, H, W, 0).view(np.uint8).copy()).to(dev)

calls = {
    "preprocess": lambda: aocr.check(aocr.lib.aocr_preprocess_lines(st, aocr.ptr(src), aocr.ptr(dsc), B, H, W, aocr.ptr(images))),
    "augment": lambda: aocr.check(aocr.lib.aocr_augment_lines(st, aocr.ptr(images), aocr.ptr(warp), B, H, W, A.seed, 0, aocr.ptr(out))),
    "augment_identity": lambda: aocr.check(aocr.lib.aocr_augment_lines(st, aocr.ptr(images), aocr.ptr(ident), B, H, W, A.seed, 0, aocr.ptr(out))),
}
for fn in calls.values():
    for _ in range(WARMUP):
        fn()
ms = {k: [] for k in calls}
for _ in range(REPEATS):
    for k, fn in calls.items():
        ms[k].append(window(fn))
res = {"shape": [B, 1, H, W], "launches_per_window": ITERS, "windows": REPEATS}
for k, v in ms.items():
    res[k] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
res["augment"]["GBps"] = 2 * B * H * W * 4 / (res["augment"]["ms_median"] * 1e-3) / 1e9          # one read + one write of the batch
print(json.dumps(res))
