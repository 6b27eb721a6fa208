"""GPU: AdamW through the model (aocr_adam_step, Model.adam_step, optimizer="adam") on the tiny model of tests/test_train_gpu.py: the loop learns,
the model-level call is the leaf op on the model's vectors, and the optimizer state survives a checkpoint."""
import ctypes as C
import math
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

B, W, L = 16, 64, 5
ADAM = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip=5.0)


def tiny(compute="f32", **extra):
    return dict(encoder_num_hidden=64, encoder_num_layers=1, decoder_num_layers=2, input_feed=True, batch_size=B, max_img_w=W, max_decoder_l=8,
                max_beam=3, compute=compute, learning_rate=0.1, seed=3, **extra)


def fixed_batch():
    import oracle_torch as O
    img, tgt, tge, nnz = O.synth_batch(B, W, max_len=L - 1, min_len=2, seed=7)
    return [img, tgt, tge, nnz, [f"img{i}" for i in range(B)]], nnz


def train(m, batch, nnz):
    """tests/test_train_gpu.py's stopping rule: 40 steps in a row under 0.02 loss / token, within 3000 steps"""
    first, per_tok, calm, steps = None, None, 0, 0
    while steps < 3000 and calm < 40:
        loss, _ = m.step(batch, False)
        per_tok = loss / nnz
        first = per_tok if first is None else first
        calm = calm + 1 if per_tok < 0.02 else 0
        steps += 1
    return first, per_tok, calm, steps


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_adam_overfits_a_fixed_batch(cuda, compute):
    """Nothing is asserted about the step counts: nobody has measured them.  They are printed side by side."""
    import aocr
    batch, nnz = fixed_batch()
    res = {}
    for opt in ("adam", "sgd"):
        m = aocr.Model().create(tiny(compute, optimizer=opt, adam=ADAM))
        res[opt] = train(m, batch, nnz)
        if opt == "adam":
            assert m.adam_steps() == res[opt][3] and m.last_norms is None and m.last_norms_adam.shape == (15,)
            for beam in (1, 3):
                _, (n, correct) = m.step(batch, True, beam)
                print(f"[adam-train] {compute}: forward_only beam {beam}: {correct:.0f}/{B} words right")
                assert correct >= B - 2
        else:
            assert m.adam_state is None and m.last_norms is not None
        m.shutdown()
    (first, per_tok, calm, steps), sgd = res["adam"], res["sgd"]
    print(f"[adam-train] {compute}: AdamW {ADAM['lr']:g}: loss/token {first:.3f} -> {per_tok:.4f} after {steps} steps; "
          f"SGD 0.1: {sgd[0]:.3f} -> {sgd[1]:.4f} after {sgd[3]} steps")
    assert abs(first - math.log(39)) < 0.6
    assert calm >= 40 and math.isfinite(per_tok), (steps, per_tok)
    assert sgd[2] >= 40, sgd


def test_unknown_optimizer_raises(cuda):
    import aocr
    with pytest.raises(ValueError, match="optimizer"):
        aocr.Model().create(tiny(optimizer="adagrad"))


def test_model_step_is_the_leaf_on_the_models_vectors(cuda):
    import aocr
    batch, _ = fixed_batch()
    m = aocr.Model().create(tiny("bf16"))                # bf16: the model has a time-out word, so the call latches it and reads the latch as its skip word
    m.train_forward_backward(batch)
    n = m.num_params
    w, g = m.params.clone(), m.grad_params.clone()
    p = aocr.AdamParams(**ADAM)
    state = torch.zeros(aocr.lib.aocr_adam_state_bytes(n) // 8, dtype=torch.int64, device=m.device)
    scratch = torch.zeros(aocr.lib.aocr_adam_scratch_bytes() // 8, dtype=torch.int64, device=m.device)
    norms = torch.zeros(15, device=m.device)
    off = (C.c_int64 * 6)(*[int(o) for o in m.group_offsets])
    for _ in range(2):                                   # the second step starts from a state that is not zero
        m.adam_step(**ADAM)
        aocr.check(aocr.lib.aocr_adam_update(m._stream(), aocr.ptr(w), aocr.ptr(g), aocr.ptr(state), off, C.byref(p), None, aocr.ptr(scratch), aocr.ptr(norms)),
                   "aocr_adam_update")
    torch.cuda.synchronize()
    assert torch.equal(g, m.grad_params), "aocr_adam_step modified the gradients"
    assert torch.equal(m.params.view(torch.int32), w.view(torch.int32)) and not torch.equal(m.params, torch.zeros_like(w))
    assert torch.equal(m.adam_state, state.view(torch.uint8)) and torch.equal(m.last_norms_adam.view(torch.int32), norms.view(torch.int32))
    assert m.adam_steps() == 2 and m.cluster_status() == 0
    m.shutdown()


def test_checkpoint_round_trip(cuda, tmp_path):
    import aocr
    batch, _ = fixed_batch()
    m1 = aocr.Model().create(tiny(optimizer="adam", adam=ADAM))
    for _ in range(3):
        m1.step(batch, False)
    path = str(tmp_path / "adam.pt")
    m1.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["adam_state"].dtype == torch.uint8 and ck["adam_state"].numel() == 8 * m1.num_params + 32
    m2 = aocr.Model().load(path, dict(optimizer="adam", adam=ADAM, batch_size=B, max_img_w=W, max_decoder_l=8, max_beam=3))
    assert m2.optimizer == "adam" and m2.adam_steps() == 3 and torch.equal(m2.adam_state, m1.adam_state) and torch.equal(m2.params, m1.params)
    # the fourth step on both, from ONE gradient vector: two backward passes need not agree in the last bit (split-K sums), the optimizer must
    m1.train_forward_backward(batch)
    m2.grad_params.copy_(m1.grad_params)
    m1.adam_step(**ADAM); m2.adam_step(**ADAM)
    assert m1.adam_steps() == 4 and m2.adam_steps() == 4
    assert torch.equal(m1.params.view(torch.int32), m2.params.view(torch.int32)) and torch.equal(m1.adam_state, m2.adam_state)
    # a checkpoint written by an SGD model carries no optimizer state and loads as before
    m3 = aocr.Model().create(tiny())
    m3.step(batch, False)
    sgd_path = str(tmp_path / "sgd.pt")
    m3.save(sgd_path)
    assert "adam_state" not in torch.load(sgd_path, map_location="cpu", weights_only=True)
    m4 = aocr.Model().load(sgd_path, dict(batch_size=B, max_img_w=W, max_decoder_l=8, max_beam=3))
    assert m4.adam_state is None and m4.optimizer == "sgd" and torch.equal(m4.params, m3.params)
    for m in (m1, m2, m3, m4):
        m.shutdown()


def test_t7_save_warns_that_the_state_stays_behind(cuda, tmp_path):
    import aocr
    batch, _ = fixed_batch()
    m = aocr.Model().create(tiny(optimizer="adam", adam=ADAM))
    m.step(batch, False)
    path = str(tmp_path / "x.t7")
    with pytest.warns(UserWarning, match="AdamW state"):
        m.save(path)
    with warnings.catch_warnings(record=True) as rec:           # once per model, not once per call
        warnings.simplefilter("always")
        m.save(path)
    assert not [r for r in rec if "AdamW state" in str(r.message)]
    m2 = aocr.Model().load(path, dict(batch_size=B, max_img_w=W, max_decoder_l=8, max_beam=3))
    assert m2.adam_state is None and torch.equal(m2.params, m.params)
    m.shutdown(); m2.shutdown()
