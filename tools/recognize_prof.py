"""ms per call of aocr_decode against aocr_recognize (without and with both optional outputs) at C3 and at the reference's default shape,
greedy and beam 5, timed with HIP events on the model's stream (as tools/decode_prof.py runs the decode loop).  Prints one JSON line per cell."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torch-attention-ocr_amd"))
import aocr

SHAPES = {"c3": dict(B=256, W=256, He=256), "ref": dict(B=400, W=100, He=512)}
ITERS, WARMUP = int(os.environ.get("ITERS", "10")), 3


def timed(fn):
    for _ in range(WARMUP):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


for name in (sys.argv[1:] or list(SHAPES)):
    s = SHAPES[name]
    B, W = s["B"], s["W"]
    m = aocr.Model().create(dict(encoder_num_hidden=s["He"], encoder_num_layers=1, decoder_num_layers=2, input_feed=True, batch_size=B,
                                 max_img_w=W, max_decoder_l=50, max_beam=5, compute="bf16", learning_rate=0.1, seed=910820))
    img, tgt, tge, nnz = aocr.synth.synth_batch(B, W, seed=1234, max_len=23)
    dev = m.device
    images = torch.from_numpy(img).to(device=dev, dtype=torch.float32)
    targets, targets_eval = torch.from_numpy(tgt).to(dev), torch.from_numpy(tge).to(dev)
    for beam in (1, 5):
        row = dict(shape=name, B=B, W=W, beam=beam, iters=ITERS)
        row["decode_ms"] = timed(lambda: m.decode_device(images, targets, targets_eval, beam))
        row["recognize_ms"] = timed(lambda: m.recognize_device(images, beam))
        row["recognize_outputs_ms"] = timed(lambda: m.recognize_device(images, beam, attention=True, char_scores=True))
        m.check_health()
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    m.shutdown()
