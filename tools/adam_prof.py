"""us per call of the three optimizer tails at the C3 model's parameter count (12.18 M), timed with HIP events in one process: AdamW as the leaf
(aocr_adam_update on the model's vectors) and through the model (aocr_adam_step: + the time-out latch and the restore launch), clipped SGD
(aocr_sgd_step = sgd_clip_update on the model's vectors) and Adadelta (aocr_adadelta_step).  7 windows of 50 calls after 10 warm-up calls each;
the JSON carries the median, the spread, and bytes moved over the median time against the 6.3 TB/s the project takes as achievable.
Bytes per parameter: AdamW 8 (norm pass: w, g) + 16 read + 12 written = 36; Adadelta one pass, 16 + 12 = 28; SGD 8 + 8 + 4 = 20.
Writes the row to --out (default profiles/adam_prof.json) and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "torch-attention-ocr_amd"))
import aocr
from aocr import lib, ptr

WINDOWS, CALLS, WARMUP = 7, 50, 10
HBM_BYTES_PER_S = 6.3e12
BYTES = dict(adam=36, adadelta=28, sgd=20)


def windows(fn):
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_prof.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    m = aocr.Model().create(dict(encoder_num_hidden=256, encoder_num_layers=1, decoder_num_layers=2, input_feed=True, batch_size=256, max_img_w=256,
                                 max_decoder_l=24, max_beam=5, compute="bf16", learning_rate=0.1, seed=910820))
    n = m.num_params
    m.grad_params.normal_(0.0, 1e-3, generator=torch.Generator(device=dev).manual_seed(1))
    aocr.check(lib.aocr_model_set_stream(m._h, m._stream()))
    p = aocr.AdamParams(lr=1e-5, clip=5.0)
    off = (C.c_int64 * 6)(*[int(o) for o in m.group_offsets])
    state = torch.zeros(lib.aocr_adam_state_bytes(n) // 8, dtype=torch.int64, device=dev)
    scratch = torch.zeros(lib.aocr_adam_scratch_bytes() // 8, dtype=torch.int64, device=dev)
    norms = torch.zeros(16, dtype=torch.float32, device=dev)
    ada = torch.zeros(2 * n, dtype=torch.float32, device=dev)

    def adam_leaf():
        aocr.check(lib.aocr_adam_update(m._stream(), ptr(m.params), ptr(m.grad_params), ptr(state), off, C.byref(p), None, ptr(scratch), ptr(norms)), "aocr_adam_update")

    def adam_model():
        aocr.check(lib.aocr_adam_step(m._h, C.byref(p), ptr(state), ptr(norms)), "aocr_adam_step")

    def sgd():
        aocr.check(lib.aocr_sgd_step(m._h, 1e-5, 5.0, ptr(norms)), "aocr_sgd_step")

    def adadelta():
        aocr.check(lib.aocr_adadelta_step(m._h, 0.9, 1e-6, 0.0, ptr(ada)), "aocr_adadelta_step")

    row = dict(n=n, windows=WINDOWS, calls=CALLS, warmup=WARMUP, compute_units=torch.cuda.get_device_properties(dev).multi_processor_count,
               v_offset_mod_4=n % 4)
    for name, fn, kind in (("adam_update", adam_leaf, "adam"), ("adam_step", adam_model, "adam"), ("adadelta_step", adadelta, "adadelta"), ("sgd_step", sgd, "sgd"),
                           ("adam_update_again", adam_leaf, "adam")):
        t = windows(fn)
        med = statistics.median(t)
        row[name + "_us"], row[name + "_us_min"], row[name + "_us_max"] = med, min(t), max(t)
        row[name + "_bytes"] = BYTES[kind] * n
        row[name + "_TBps"] = BYTES[kind] * n / (med * 1e-6) / 1e12
        row[name + "_of_6.3TBps"] = BYTES[kind] * n / (med * 1e-6) / HBM_BYTES_PER_S
    m.check_health()
    row["adam_steps_applied"] = int(state[n + 2].item())
    row["adam_over_adadelta"] = row["adam_update_us"] / row["adadelta_step_us"]
    row["byte_ratio_prediction"] = BYTES["adam"] / BYTES["adadelta"]
    row["adam_over_prediction"] = row["adam_over_adadelta"] / row["byte_ratio_prediction"]
    m.shutdown()
    line = json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
