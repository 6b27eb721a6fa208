"""aocr_profile_kernel's replays run from the same stage view and launch functions as the training step (csrc/cnn.h): each is the
launch the step makes, on the buffers the step left, with the step's own partial-sum slab.

Shape: bf16, 32 x 128 crops, B = 32.  The conv5 / conv6 maps have 32 * 4 * 32 = 4096 pixels (a multiple of 256, 16 statistics
chunks); the gradient-map scratch G0 holds 32 * 16 * 64 * 128 = 4.19 M floats: at least conv6's 512 x 4608 filter gradient and the
4096 x 640 of conv1's backward scratch, and fewer than eight 4 Mi-float slabs -- so every replay must put its partial sums at the
start of G0, where the step puts them at this size, and not at a slab offset past its end."""
import os

import pytest
import torch

from cdecl import defines
from model_harness import make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relnorm(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_replays_run_the_steps_launches(cuda):
    from aocr._lib import check, lib, ptr
    pk = {k: int(v) for k, v in defines(open(os.path.join(ROOT, "include", "aocr.h")).read()).items() if k.startswith("AOCR_PK_")}
    m, O, ocfg, P, st, batch = make(dict(enc_hidden=256, enc_layers=1, dec_layers=2, input_feed=True), B=32, W=128, maxlen=11, compute="bf16",
                                    max_decoder_l=12, max_beam=1)
    images, targets, targets_eval = m._upload(batch)          # kept alive: the conv1 replays read the step's image buffer

    def step():
        check(lib.aocr_model_set_stream(m._h, m._stream()))
        check(lib.aocr_train_forward_backward(m._h, ptr(images), ptr(targets), ptr(targets_eval), 32, 128, targets.shape[1], 1.0 / 32,
                                              ptr(m._scal[0:1])), "aocr_train_forward_backward")
        torch.cuda.synchronize()
        return m.grad_params.clone()

    g_first = step()
    taps = {n: m.get_tensor(n) for n in ("conv6", "idx6", "conv1", "conv5")}
    assert taps["conv5"].shape == (32, 4, 32, 512) and taps["conv6"].shape == (32, 2, 32, 512) and taps["conv1"].shape == (32, 16, 64, 64)

    def replay(name):
        ms, _ = m.profile_kernel(pk[name], 1)
        assert ms > 0.0, (name, ms)

    # the forward replays rewrite the same outputs from the same inputs
    for name in ("AOCR_PK_CONV6_FWD", "AOCR_PK_CONV1_FWD", "AOCR_PK_BN_FWD"):
        replay(name)
    for n, want in taps.items():
        assert torch.equal(m.get_tensor(n), want), n
    for name in ("AOCR_PK_CONV6_WGRAD", "AOCR_PK_CONV1_BWD", "AOCR_PK_BN_BWD", "AOCR_PK_UNPOOL", "AOCR_PK_SPLITK"):
        replay(name)
    torch.cuda.synchronize()
    assert m.cluster_status() == 0
    # nothing the next step reads was damaged: the same batch gives the same gradient vector, up to the order in which split-K partial sums meet
    # (the bound of test_side_stream_overlaps_match_in_line_order)
    rel = relnorm(step(), g_first)
    print(f"[replay] gradient vector of the step after the replays vs the step before them: {rel:.2e}")
    assert rel < 1e-5
    assert m.cluster_status() == 0
    m.shutdown()
