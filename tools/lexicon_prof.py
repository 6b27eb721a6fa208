"""ms per call of aocr_lexicon_nearest at B = 256, L = 50 against a seeded synthetic lexicon of 90 000 words of 2-16 ids, next to the ms of the
beam-1 recognize_device call at C3 that it follows, both timed with HIP events in one process (as tools/recognize_prof.py times the decode loop).
Every window is warmed up, long enough to be well above the event resolution, and repeated; the JSON line carries the median and the spread."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torch-attention-ocr_amd"))
import aocr

B, L, N_WORDS, STRIDE = 256, 50, 90000, 32          # 16 ids and their 0 need the second 16-byte chunk
WINDOWS, WARMUP = int(os.environ.get("WINDOWS", "7")), 10
INT_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9           # 256 CUs x 4 SIMDs x 32 lanes at the 2.4 GHz peak clock: the chip's 32-bit integer rate


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


def synthetic(seed=90000):
    """the lexicon (ids 4..39: the 36 characters of the default vocabulary) and B predictions: lexicon words with up to two edits."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, 17, size=N_WORDS)
    words = np.zeros((N_WORDS, STRIDE), np.uint8)
    for n in range(2, 17):
        rows = np.nonzero(lens == n)[0]
        words[rows, :n] = rng.integers(4, 40, size=(rows.size, n))
    labels = np.full((B, L), 3, np.int32)
    for b in range(B):
        w = words[rng.integers(0, N_WORDS)]
        ids = [int(v) for v in w[w != 0]]
        for _ in range(int(rng.integers(0, 3))):
            ids[int(rng.integers(0, len(ids)))] = int(rng.integers(4, 40))
        labels[b, :len(ids)] = ids
    return words, labels, int(lens.sum())


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    words, labels, n_ids = synthetic()
    lex = aocr.Lexicon([aocr.numlist2str(w[w != 0].tolist()) for w in words], device=dev)
    assert np.array_equal(lex.array, words) and not lex.skipped
    labels_dev = torch.from_numpy(labels).to(dev)
    row = dict(B=B, L=L, n_words=N_WORDS, stride=STRIDE, pairs=B * N_WORDS, mean_word_ids=round(n_ids / N_WORDS, 3), windows=WINDOWS)
    t = windows(lambda: lex.nearest(labels_dev), 200)
    row["lexicon_ms"], row["lexicon_ms_min"], row["lexicon_ms_max"] = statistics.median(t), min(t), max(t)
    rows = torch.arange(B + 1, dtype=torch.int32, device=dev) * 50          # the 50-word lexicon per image of IIIT5K / SVT
    t = windows(lambda: lex.nearest(labels_dev, rows), 200)
    row["lexicon_50_per_image_ms"] = statistics.median(t)

    m = aocr.Model().create(dict(encoder_num_hidden=256, encoder_num_layers=1, decoder_num_layers=2, input_feed=True, batch_size=B, max_img_w=256,
                                 max_decoder_l=50, max_beam=5, compute="bf16", learning_rate=0.1, seed=910820))
    img, _, _, _ = aocr.synth.synth_batch(B, 256, seed=1234, max_len=23)
    images = torch.from_numpy(img).to(device=dev, dtype=torch.float32)
    t = windows(lambda: m.recognize_device(images, 1), 20)
    m.check_health()
    row["recognize_ms"], row["recognize_ms_min"], row["recognize_ms_max"] = statistics.median(t), min(t), max(t)
    t = windows(lambda: lex.nearest(m.recognize_device(images, 1)[0]), 20)
    row["recognize_then_lexicon_ms"] = statistics.median(t)
    m.shutdown()

    row["lexicon_over_recognize"] = row["lexicon_ms"] / row["recognize_ms"]
    est_ops = B * n_ids * 15.0                                              # pairs x ids per word x ~15 integer operations per id
    row["est_int_ops"] = est_ops
    row["fraction_of_int_rate"] = est_ops / (row["lexicon_ms"] * 1e-3) / INT_LANE_OPS_PER_S
    print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
