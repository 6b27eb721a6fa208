"""CPU: tests/enc_seq_ref.py (the float64 restatement the encoder whole-sequence kernels are held to in tests/test_encoder_seq_kernels_gpu.py)
against independent statements of the same recurrence: oracle_torch's encoder LSTM with operand rounding switched off (forward) and torch
autograd in float64 (backward), both directions, T = 1 included; and the condition the GPU test's operand generators must meet, on every shape
the GPU test uses."""
import types

import pytest
import torch

import enc_seq_ref as R
import oracle_torch as O

F64 = torch.float64
TOL_CELL = 2e-5                      # tests/kernel_harness.py


@pytest.mark.parametrize("B,T,He", [(3, 1, 8), (4, 5, 16), (2, 2, 8)])
def test_forward_matches_the_oracle_encoder(B, T, He):
    D = 12
    g = torch.Generator().manual_seed(5 + T)
    P = {}
    for pre in ("enc_fw", "enc_bw"):
        P[f"{pre}.l1.i2h.w"] = torch.randn(4 * He, D, generator=g, dtype=F64) * 0.5
        P[f"{pre}.l1.i2h.b"] = torch.randn(4 * He, generator=g, dtype=F64) * 0.3
        P[f"{pre}.l1.h2h.w"] = torch.randn(4 * He, He, generator=g, dtype=F64) * 0.5
        P[f"{pre}.l1.h2h.b"] = torch.randn(4 * He, generator=g, dtype=F64) * 0.3
    feats = torch.randn(B, T, D, generator=g, dtype=F64)
    with O.operand_rounding(None):
        ctx, traces = O.encoder_forward(P, types.SimpleNamespace(enc_hidden=He, enc_layers=1), feats)
    hs = {}
    for pre, rev in (("enc_fw", False), ("enc_bw", True)):
        zx = torch.einsum("btd,gd->tbg", feats, P[f"{pre}.l1.i2h.w"]) + P[f"{pre}.l1.i2h.b"] + P[f"{pre}.l1.h2h.b"]
        r = R.forward(zx, P[f"{pre}.l1.h2h.w"], rev, round=False)
        hs[pre] = r["hs"]
        last = T if not rev else 1                                   # the slot of the last processed step
        assert (r["cs"][last] - traces[pre][1]).abs().max() < 1e-12 and (r["hs"][last] - traces[pre][2]).abs().max() < 1e-12
        assert r["cs"][0].abs().max() == 0 and r["cs"][T + 1].abs().max() == 0 and r["hs"][0].abs().max() == 0 and r["hs"][T + 1].abs().max() == 0
        # the saved gates of every step are the oracle's cache (i, f, o, g), in both layouts
        for t in range(T):
            i, f, o, gg, _ = traces[pre][0][t][0][3]
            want = torch.stack([i, f, o, gg], 1)
            assert (r["gates"][t] - want).abs().max() < 1e-12
            for layout in ("seq", "cl"):
                flat = R.gates_layout(r["gates"][t], layout)
                assert torch.equal(R.gates_unlayout(flat, He, layout), r["gates"][t])
            assert torch.equal(R.gates_layout(r["gates"][t], "seq")[:, He:2 * He], r["gates"][t][:, 1])
            assert torch.equal(R.gates_layout(r["gates"][t], "cl")[:, 4 * 3 + 2], r["gates"][t][:, 2, 3])
    assert (R.context(hs["enc_fw"], hs["enc_bw"]) - ctx).abs().max() < 1e-12


@pytest.mark.parametrize("forward_dir", [1, 0])
@pytest.mark.parametrize("B,T,He", [(3, 1, 8), (4, 5, 8), (2, 2, 16)])
def test_backward_matches_autograd(B, T, He, forward_dir):
    g = torch.Generator().manual_seed(11 * T + forward_dir)
    W = (torch.randn(4 * He, He, generator=g, dtype=F64) * 0.5).requires_grad_(False)
    zx = (torch.randn(T, B, 4 * He, generator=g, dtype=F64)).requires_grad_(True)
    dh1, dh2, dc0 = (torch.randn(*s, generator=g, dtype=F64) for s in ((T, B, He), (B, He), (B, He)))
    reverse = not forward_dir
    # the forward pass as an autograd graph: lists, no slots
    c0 = torch.zeros(B, He, dtype=F64, requires_grad=True)
    c, h, hs_t, saved = c0, torch.zeros(B, He, dtype=F64), {}, {}
    order = R.steps(T, reverse)
    for t in order:
        c, h, gates = R.cell((zx[t] + h @ W.t()).view(B, 4, He), c)
        hs_t[t], saved[t] = h, (gates.detach(), c.detach())
    # BPTT enters at the LAST forward step: d h = dh1(t) there plus dh2, d c = dc0
    loss = sum((dh1[t] * hs_t[t]).sum() for t in order) + (dh2 * hs_t[order[-1]]).sum() + (dc0 * c).sum()
    loss.backward()
    fw = R.forward(zx.detach(), W, reverse, round=False)
    r = R.backward(W, fw["gates"], fw["cs"], dh1, dh2, dc0, forward_dir, round=False)
    assert (r["dz"].reshape(T, B, 4 * He) - zx.grad).abs().max() < 1e-12
    assert (r["db"].reshape(-1) - zx.grad.sum(dim=(0, 1))).abs().max() < 1e-12
    assert (r["dc"] - c0.grad).abs().max() < 1e-12
    # chunks: [0, k) then [k, T), the second one device-fed (every step takes the d z of the step before from the given tensor), carry d c and give the same
    for k in range(1, T):
        a = R.backward(W, fw["gates"], fw["cs"], dh1, dh2, dc0, forward_dir, round=False, it1=k)
        b = R.backward(W, fw["gates"], fw["cs"], dh1, dh2, a["dc"], forward_dir, round=False, fed_dzb=r["dz"].reshape(T, B, 4 * He), it0=k)
        assert (a["dz"] + b["dz"] - r["dz"]).abs().max() < 1e-12 and (b["dc"] - r["dc"]).abs().max() < 1e-12
        assert (a["db"] + b["db"] - r["db"]).abs().max() < 1e-12


def test_device_fed_forward_is_the_free_running_one_on_its_own_state():
    """fed with its own (rounded) state the device-fed mode reproduces the free-running reference, chunk by chunk"""
    B, T, He = 3, 5, 16
    W, zx = R.weights(He, 1), R.inputs(T, B, He, 2)
    for rev in (False, True):
        free = R.forward(zx, W, rev)
        fed = R.forward(zx, W, rev, fed=dict(hsb=R.rne(free["hs"]), cs=free["cs"]))
        part = R.forward(zx, W, rev, fed=dict(hsb=R.rne(free["hs"]), cs=free["cs"]), it0=2, it1=4)
        assert torch.equal(fed["cs"], free["cs"]) and torch.equal(fed["gates"], free["gates"])
        for t in R.steps(T, rev, 2, 4):
            assert torch.equal(part["cs"][t + 1], free["cs"][t + 1])
        exact = R.forward(zx, W, rev, round=False)
        assert 0 < (exact["hs"] - free["hs"]).abs().max() < 0.05       # the rounding is there, and small


@pytest.mark.parametrize("B,T,He", sorted(set(R.SEQ_SHAPES + R.CL_SHAPES)))
def test_operand_generators_keep_the_gates_sensitive(B, T, He):
    """At least 90 % of the free-running reference's pre-activations lie inside |z| <= 4 (tanh'(4) q: one wrong product moves a gate by several
    tolerances there), W is exact in bf16, and the state a step reads differs from its neighbours' -- by row, by step and by direction -- by far more
    than a tolerance in z: a read from the wrong row, slot or direction cannot pass."""
    hb = {}
    for d, rev in enumerate((False, True)):
        W, zx = R.weights(He, 100 + d), R.inputs(T, B, He, 200 + d)
        assert torch.equal(W.to(torch.bfloat16).float(), W) and W.abs().max() <= R.W_INT * R.Q
        r = R.forward(zx, W, rev)
        assert R.z_share(r["z"]) >= 0.9, f"share of |z| <= 4 is {R.z_share(r['z']):.3f}"
        h = R.rne(r["hs"][1:-1])                                      # [T][B][He]
        hb[d] = (h, W.double())
        dz_rows = ((h - h.roll(1, dims=1)) @ W.double().t()).abs().amax(dim=2) if B > 1 else None
        assert dz_rows is None or dz_rows.min() > 100 * TOL_CELL, "two neighbouring rows give the same product"
        if T > 1:
            dz_steps = ((h - h.roll(1, dims=0)) @ W.double().t()).abs().amax(dim=2)
            assert dz_steps.min() > 100 * TOL_CELL, "two neighbouring steps give the same product"
    dz_dir = ((hb[0][0] - hb[1][0]) @ hb[0][1].t()).abs().amax(dim=2)
    assert dz_dir.min() > 100 * TOL_CELL, "the two directions give the same product"
