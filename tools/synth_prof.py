"""Rates of the synthetic word-line generator (aocr_synth_lines, aocr.SynthGen) at the two headline batch shapes, 256 x 32 x 256 (C3) and
400 x 32 x 100 (the reference's defaults), next to what it has to keep pace with and what it replaces:

  * the kernel alone and the kernel + aocr_augment_lines, timed with HIP events on the current stream (ITERS launches per window after
    warm-up, WINDOWS windows of each in alternation): ms, image-lines/s, bytes written per ms, share of the achievable HBM rate;
  * SynthGen.next_device end to end (style draw on the host, upload, launch), host clock around a window that ends in a synchronise;
  * the host DataGen path on the same batch sizes in the same run: PNG files (Pillow; .npy when it is missing) of the same crops decoded on
    the host, uploaded and scaled by aocr_preprocess_lines -- the first pass decodes, the second reads DataGen's cache;
  * the train step's rate, quoted from README.md (not measured here);
  * the loss of a tiny model over 200 steps on SynthGen batches: evidence that the crops can be learnt, reported and not asserted.

Prints one JSON line per shape and one for the loss curve."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torch-attention-ocr_amd"))
import aocr
from aocr.synth_lines import synth_lines

SHAPES = ((256, 32, 256), (400, 32, 100))
ITERS, WINDOWS, WARMUP = int(os.environ.get("ITERS", "200")), int(os.environ.get("WINDOWS", "5")), 10
HBM_BYTES_PER_S = 6.3e12                       # achievable HBM rate of one MI355X (float4 copy)
README_TRAIN_LINES_PER_S = {(256, 32, 256): "53.0-54.9 k (C3)", (400, 32, 100): "49.3-51.3 k (ref)"}
CHARS = "0123456789abcdefghijklmnopqrstuvwxyz"


def words(n, seed, lo=3, hi=12):
    """n seeded words of lo..hi characters over 0-9 a-z."""
    lens = lo + np.floor(aocr.synth.counter_uniform(seed, 1, n) * (hi - lo + 1)).astype(np.int64)
    pick = np.floor(aocr.synth.counter_uniform(seed, 2, n * hi) * len(CHARS)).astype(np.int64).reshape(n, hi)
    return ["".join(CHARS[c] for c in pick[i, :lens[i]]) for i in range(n)]


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def host_datagen(images_u8, labels, B, W, dev):
    """lines/s of aocr.DataGen over files holding `images_u8`: (first pass: decode + upload + scale, second pass: cached + upload + scale)."""
    try:
        from PIL import Image
        ext = "png"
    except ImportError:
        Image, ext = None, "npy"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "list.txt"), "w") as f:
            for i, (im, lab) in enumerate(zip(images_u8, labels)):
                name = f"{i}.{ext}"
                if Image is not None:
                    Image.fromarray(im).save(os.path.join(d, name))
                else:
                    np.save(os.path.join(d, name), im)
                f.write(f"{name} {lab or 'a'}\n")
        gen = aocr.DataGen(d, "list.txt", 8.0, force_width=W, device=dev)
        rates = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            while True:
                b = gen.nextBatch(B)
                if b is None:
                    break
                n += b[0].shape[0]
            torch.cuda.synchronize()
            rates.append(n / (time.perf_counter() - t0))
    return ext, rates


def shape_row(B, H, W, lex, atlas, dev):
    gen = aocr.SynthGen(lex, atlas, width=W, seed=1, epoch_size=1 << 40, device=dev)
    gen._device()
    style = gen.params(B, 0)
    L = int(gen._n_ids[style["word"]].max()) + 1
    st = torch.cuda.current_stream(dev).cuda_stream
    sd = torch.from_numpy(style.view(np.uint8).copy()).to(dev)
    ld, ad = lex.desc(), atlas.desc()
    out, aug = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev), torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    tg, te = torch.empty((B, L), dtype=torch.int32, device=dev), torch.empty((B, L), dtype=torch.int32, device=dev)
    A = aocr.Augmenter(rotate_deg=3, scale=1.1, translate=(4, 2), contrast=1.3, noise=8)
    warp = torch.from_numpy(A.params(B, H, W, 0).view(np.uint8).copy()).to(dev)
    import ctypes as C

    def render():
        aocr.check(aocr.lib.aocr_synth_lines(st, C.byref(ld), C.byref(ad), aocr.ptr(sd), B, H, W, L, aocr.ptr(out), aocr.ptr(tg), aocr.ptr(te)))

    def render_augment():
        render()
        aocr.check(aocr.lib.aocr_augment_lines(st, aocr.ptr(out), aocr.ptr(warp), B, H, W, A.seed, 0, aocr.ptr(aug)))

    calls = {"render": render, "render_augment": render_augment}
    for fn in calls.values():
        for _ in range(WARMUP):
            fn()
    ms = {k: [] for k in calls}
    for _ in range(WINDOWS):
        for k, fn in calls.items():
            ms[k].append(window(fn))
    row = {"shape": [B, 1, H, W], "L": L, "launches_per_window": ITERS, "windows": WINDOWS}
    written = B * H * W * 4 + 2 * B * L * 4                                      # the images and the two target arrays
    for k, v in ms.items():
        med = statistics.median(v)
        row[k] = {"ms_median": med, "ms_min": min(v), "ms_max": max(v), "lines_per_s": B / (med * 1e-3)}
    row["render"]["bytes_written_per_ms"] = written / row["render"]["ms_median"]
    row["render"]["share_of_hbm_rate"] = written / (row["render"]["ms_median"] * 1e-3) / HBM_BYTES_PER_S
    # end to end through the Python class: style draw, upload, launch
    for _ in range(3):
        gen.next_device(B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        gen.next_device(B)
    torch.cuda.synchronize()
    row["synthgen_next_device_lines_per_s"] = 50 * B / (time.perf_counter() - t0)
    # the host path on the same batch size: files of the same crops
    images_u8 = out[:, 0].clamp(0, 255).to(torch.uint8).cpu().numpy()
    n_files = 4 * B
    ext, rates = host_datagen([images_u8[i % B] for i in range(n_files)], [lex.words[w] for w in np.resize(style["word"], n_files)], B, W, dev)
    row["host_datagen"] = {"files": ext, "n": n_files, "first_pass_lines_per_s": rates[0], "cached_pass_lines_per_s": rates[1]}
    row["train_step_lines_per_s_readme"] = README_TRAIN_LINES_PER_S[(B, H, W)]
    return row


def loss_curve(atlas, dev, steps=200, B=32, W=100):
    lex = aocr.Lexicon(words(50, 7, 3, 6), device=dev)
    gen = aocr.SynthGen(lex, atlas, width=W, seed=3, epoch_size=1 << 40, device=dev)
    m = aocr.Model().create(dict(encoder_num_hidden=64, encoder_num_layers=1, decoder_num_layers=2, input_feed=True, batch_size=B, max_img_w=W,
                                 max_decoder_l=8, max_beam=1, learning_rate=0.1, seed=1))
    per_char = []
    for _ in range(steps):
        images, tg, te, nnz, _ = gen.nextBatch(B)
        loss, _ = m.step([images, tg, te, nnz, None], forward_only=False)
        per_char.append(loss / nnz)
    m.shutdown()
    return {"tiny_model_loss_per_char": {str(k): round(float(np.mean(per_char[k:k + 10])), 4) for k in range(0, steps, 20)},
            "last_10_mean": round(float(np.mean(per_char[-10:])), 4), "steps": steps, "batch": B, "lexicon_words": 50}


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    atlas = aocr.GlyphAtlas.default().to(dev)
    lex = aocr.Lexicon(words(10000, 90), device=dev)
    rnd = lambda o: {k: rnd(v) for k, v in o.items()} if isinstance(o, dict) else (round(o, 5) if isinstance(o, float) else o)
    for B, H, W in SHAPES:
        print(json.dumps(rnd(shape_row(B, H, W, lex, atlas, dev))), flush=True)
    print(json.dumps(loss_curve(atlas, dev)), flush=True)


if __name__ == "__main__":
    main()
