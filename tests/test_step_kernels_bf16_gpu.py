"""GPU: every branch of the bf16 fused recurrent-step launchers (csrc/ops_gemm.hip: launch_small_gates_fwd_hh/_h, launch_small_hh/_h,
launch_small_gates_bwd_hh/_h, gates_elem_bwd, big_step_store, big_step_gates_fwd) against an exact reference, called directly through
tests/libkprobe.so.  Method of tests/test_kernels_bf16_gpu.py, helpers of tests/kernel_harness.py: sentinel tails (and here the padding columns of every strided
buffer) must survive every call, and every case asserts the kernel it reached from the AOCR_TRACE dispatch line.

Operands.  A-side values are small integers, B-side values small integers times a power of two q: all exact in bf16, every product and
partial sum a multiple of q below 2^20 q, so the fp32 product part is exact in ANY summation order and the reference forms it in float64.
An _hh launcher reads A from its bf16 shadow, an _h launcher the fp32 A.  K is one segment or two ([p0 | p1], different row strides), and
every operand and output is a window of a wider buffer (row stride > row length).

Plain products (EpStore): bit-exact (bias + bias2, ReLU, accumulate onto a non-zero buffer, the C1 / N0 column split, the bf16 shadow =
RNE, the tanh-backward fusion with dout in {0, +-0.5}); EP_TANH within 2e-5 of float64 tanh.
Gate forward (EpGatesFwd): float64 LSTM cell (LSTM.lua:79-105) on the exact pre-activation; c, h and the saved gates within 2e-5 (the
exact-fp32 cell's tolerance, test_ops_gpu.py::test_lstm_cell).  q = 2^-4 and at least 90 % of the reference pre-activations inside
|z| <= 4 (asserted), so ONE wrong product moves a gate by >= q tanh'(4) ~ 8e-5 = four tolerances.  Exact parts: hb = RNE of the device's
own h, h_out2 = h times oracle_torch.dropout_mask at row H + j + off, hb2 = RNE of that, token rows from table row tok - 1.
Gate backward (EpGatesBwd): float64 of EpGatesBwd::quad's formulas on the exact product; 5e-5 max(1, max |dh|) with |dh| <= 4
(asserted); dzb = RNE of the device's own dz.
Random operands (already rounded to bf16), a few per function: plain outputs within bound(|A| |B|, K), gate outputs within
2e-5 + 2 bound (every cell derivative with respect to z is <= 1.5 for |c_prev| <= 1, <= 1.75 for h).

Branches (M, H or N, K; function = launch_small_bf16_hh for _hh, launch_small_bf16 for _h):
  gates_fwd_hh  gemm_step_kernel[2,2,w8]      33, 64, 64 and 70, 64, 64 + 128
  gates_fwd_hh  gemm_step_kernel[2,2,w4]      the same, AOCR_STEP_WAVES4=1
  gates_fwd_hh  gemm_step_kernel[4,1,w4]      33, 32, 64, AOCR_NO_HALF_TILES=1
  gates_fwd_hh  gemm_step_kernel[4,1,w4,mt2]  770, 512, 64, AOCR_NO_HALF_TILES=1 (16 x 13 = 208 >= 200 workgroups)
  gates_fwd_hh  gemm_stepl_kernel[gates]      70, 64, 128 and 64, 64, 64 + 64, AOCR_STEPL_MIN_WGS=1; once with ldh % 4 != 0 (scalar epilogue)
  hh / gates_bwd_hh  gemm_step_kernel[1,0,w8 | w4 | w16]   33, 32, 64 (w4: AOCR_STEP_WAVES4=1); w16: 33, 64, 1024, AOCR_STEP_WAVES16=1
  hh            gemm_step_kernel[1,0,w8,mt2]  400, 1024, 64, AOCR_STEP_MT2_MINK=64
  hh / gates_bwd_hh  gemm_stepl_kernel[plain] 70, 128, 128, AOCR_STEPL_MIN_WGS=1, nz = 1 and 3
  gates_fwd_h / h / gates_bwd_h  staged       33, 64, 64: gemm_step_kernel[2,2,w8] ([4,1,w4] without half tiles) / [1,0,w8] / [1,0,w8]
  gates_fwd_h / h / gates_bwd_h  non-staged   37, 40, 96: gemm_small_kernel[bf16,4,gates] / [bf16,1,plain]
  big_step_store / big_step_gates_fwd         AOCR_BIG_STEP=1, AOCR_BIG_STEP_MIN_ROWS=128: 130, 1024, 64 / 130, 256, 64 + 64 -> gemm_dma128_kernel[8,8]
                                              (+ gates_elem_fwd_kernel[]); taken == 0 without the switch
  gates_elem_bwd  gates_elem_bwd_kernel[]     33, 40
(A gate-backward launch is a plain product for the dispatch: GATES kind 0 in its trace line.)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module (tests/test_kernel_harness_cpu.py checks it)
from kernel_harness import (EP_ACCUM, EP_RELU, EP_TANH, SENT, TOL_BWD, TOL_CELL, Buf, Drop, GatesBwd, GatesFwd, Mat, Store, bf, bound, call, expect,
                            ints, no_drop, operand, out, ratio, rb, rnd, setenv, trace_of, vp)

pytestmark = pytest.mark.gpu

Q = 2.0 ** -4                       # B-side quantum of the gate cases
HH, HF = "launch_small_bf16_hh", "launch_small_bf16"


def drop_spec(p, seed, step, site, off, n):
    """(Drop, the n mask values as float32) of oracle_torch.dropout_mask"""
    import oracle_torch as O
    with np.errstate(over="ignore"):
        stream = np.uint64(step) * np.uint64(64) + np.uint64(site)
        base = O._splitmix64(np.array([np.uint64(seed) ^ (stream * np.uint64(0xD1342543DE82EF95))], dtype=np.uint64))[0]
    d = Drop(int(base), int(math.ceil(p * 9007199254740992.0)), 1.0 / (1.0 - p), off)
    return d, torch.from_numpy(O.dropout_mask(p, seed, step, site, off, n)).float()


# ------------------------------------------------------------------------------------------------------------------------------
# gate forward
# ------------------------------------------------------------------------------------------------------------------------------
def gf_problem(M, H, segs, opts, seed, a_dtype, random=False):
    """One problem of a gate-forward launch: the ctypes struct, its buffers and the float64 reference.
    opts: zx | tok (token table), bias, drop, h2 (second copy, another stride), hb, hb2, nogates, misalign (ldh % 4 != 0)."""
    K = sum(segs)
    if random:
        A, B = rb(rnd(M, K, seed=seed)), rb(rnd(4 * H, K, seed=seed + 1) * (2.0 / K ** 0.5))
    else:
        A, B = ints(M, K, seed=seed, lo=-2, hi=2), ints(4 * H, K, seed=seed + 1, lo=-1, hi=1) * Q
    p, keep = GatesFwd(), []
    p.a, ka = operand(A, segs, a_dtype, vary=seed % 2)
    p.b, kb = operand(B, segs, torch.bfloat16, vary=(seed + 1) % 2)
    prod = A.double() @ B.double().t()
    z, mag = prod, A.double().abs() @ B.double().abs().t()
    if "bias" in opts:
        b1, b2 = (ints(4 * H, seed=seed + 2, lo=-8, hi=8) * Q, ints(4 * H, seed=seed + 3, lo=-8, hi=8) * Q) if not random else \
                 ((rnd(4 * H, seed=seed + 2) * 0.5).float(), (rnd(4 * H, seed=seed + 3) * 0.5).float())
        m1, m2 = Buf(b1), Buf(b2)
        p.b1, p.b2 = m1.full.data_ptr(), m2.full.data_ptr()
        z = z + (b1.double() + b2.double())
        keep += [m1, m2]
    if "zx" in opts or "tok" in opts:
        rows = 11 if "tok" in opts else M                                    # tok: an 11-row per-token table
        zx = ints(rows, 4 * H, seed=seed + 4, lo=-8, hi=8) * Q if not random else (rnd(rows, 4 * H, seed=seed + 4) * 0.5).float()
        mz = Mat(rows, 4 * H, data=zx, pad=4)
        p.zx, p.ldzx = mz.addr, mz.ld
        keep.append(mz)
        if "tok" in opts:
            tok = torch.randint(1, rows + 1, (M,), generator=torch.Generator().manual_seed(seed + 5))
            mt = Buf(torch.stack([tok, torch.full_like(tok, 99)], 1), torch.int32)          # stride 2; the other column is never a valid row
            p.zx_tok, p.zx_tok_stride = mt.full.data_ptr(), 2
            keep.append(mt)
            zx = zx[tok - 1]
        z = z + zx.double()
    cp = rnd(M, H, seed=seed + 6).float()
    mcp = Mat(M, H, data=cp, pad=4)
    p.c_prev, p.ldcp = mcp.addr, mcp.ld
    o = dict(c=out(M, H, pad=4), h=out(M, H, pad=6 if "misalign" in opts else 8))
    p.c_out, p.ldc, p.h_out, p.ldh = o["c"].addr, o["c"].ld, o["h"].addr, o["h"].ld
    if "h2" in opts:
        o["h2"] = out(M, H, pad=12, off=4)
        p.h_out2, p.ldh2 = o["h2"].addr, o["h2"].ld
    if "nogates" not in opts:
        o["gates"] = out(M, 4 * H, pad=4)
        p.gates, p.ldg = o["gates"].addr, o["gates"].ld
    if "hb" in opts:
        o["hb"] = out(M, H, torch.bfloat16, pad=8)
        p.hb, p.ldhb = o["hb"].addr, o["hb"].ld
    if "hb2" in opts:
        o["hb2"] = out(M, H, torch.bfloat16, pad=4, off=4)
        p.hb2, p.ldhb2 = o["hb2"].addr, o["hb2"].ld
    mask = None
    p.drop = no_drop()
    if "drop" in opts:
        p.drop, mask = drop_spec(0.25, 77 + seed, 3, 2, 1000 * seed + 5, M * H)
        mask = mask.view(M, H)
    zz = z.view(M, 4, H)
    ig, fg, og, gg = torch.sigmoid(zz[:, 0]), torch.sigmoid(zz[:, 1]), torch.sigmoid(zz[:, 2]), torch.tanh(zz[:, 3])
    c = fg * cp.double() + ig * gg
    ref = dict(c=c, h=og * torch.tanh(c), gates=torch.cat([ig, fg, og, gg], 1), z=z, prod=prod, mag=mag, mask=mask)
    return p, o, ref, keep + ka + kb + [mcp]


def gf_check(o, ref, K, what, random=False):
    """-> largest error / tolerance over c, h and the gates; the exact parts are asserted here"""
    for k, m in o.items():
        m.check(f"{what} {k}")
    H = o["c"].cols
    if random:
        b = bound(ref["mag"], K)
        unit = b.view(-1, 4, H).max(dim=1).values
        tols = dict(c=TOL_CELL + 2 * unit, h=TOL_CELL + 2 * unit, gates=TOL_CELL + 2 * b)
    else:
        tols = dict(c=TOL_CELL, h=TOL_CELL, gates=TOL_CELL)
    worst = 0.0
    for k in ("c", "h", "gates"):
        if k in o:
            r = ratio(o[k].win(), ref[k], tols[k])
            assert r <= 1.0, f"{what}: {k} error / tolerance = {r:.3f}"
            worst = max(worst, r)
    h = o["h"].win()
    h2 = h * ref["mask"] if ref["mask"] is not None else h
    if "hb" in o:
        assert torch.equal(o["hb"].win().view(torch.int16), bf(h)), f"{what}: hb is not the RNE of the kernel's own h"
    if "h2" in o:
        assert torch.equal(o["h2"].win(), h2), f"{what}: h_out2 is not h times the dropout mask"
    if "hb2" in o:
        assert torch.equal(o["hb2"].win().view(torch.int16), bf(h2)), f"{what}: hb2 is not the RNE of the (masked) second copy"
    return worst


def z_share(refs):
    z = torch.cat([r["z"].reshape(-1) for r in refs])
    return (z.abs() <= 4).double().mean().item()


ALL = {"zx", "bias", "drop", "h2", "hb", "hb2"}
NH, W4, ST = {"AOCR_NO_HALF_TILES": "1"}, {"AOCR_STEP_WAVES4": "1"}, {"AOCR_STEPL_MIN_WGS": "1"}
BIG = {"AOCR_BIG_STEP": "1", "AOCR_BIG_STEP_MIN_ROWS": "128"}
# (name, launcher, M, H, K segments, switches, trace function, kernel[instantiation], options per problem (nz = their number))
GF_CASES = [
    ("half_w8", "hh", 33, 64, (64,), {}, HH, "gemm_step_kernel[2,2,w8]", [{"zx", "bias", "hb"}]),
    ("half_w8_2seg", "hh", 70, 64, (64, 128), {}, HH, "gemm_step_kernel[2,2,w8]", [{"tok", "drop", "h2", "hb2"}, {"bias", "nogates"}]),
    ("half_w4", "hh", 33, 64, (64,), W4, HH, "gemm_step_kernel[2,2,w4]", [{"bias", "nogates"}, {"zx", "h2"}, ALL]),
    ("half_w4_2seg", "hh", 70, 64, (64, 128), W4, HH, "gemm_step_kernel[2,2,w4]", [{"zx", "bias", "drop", "h2", "hb", "hb2"}]),
    ("tile_w4", "hh", 33, 32, (64,), NH, HH, "gemm_step_kernel[4,1,w4]", [{"zx", "drop", "h2", "hb2"}, {"tok", "bias", "hb"}]),
    ("tile_mt2", "hh", 770, 512, (64,), NH, HH, "gemm_step_kernel[4,1,w4,mt2]", [{"zx", "bias", "drop", "h2", "hb", "hb2"}]),
    ("stepl", "hh", 70, 64, (128,), ST, HH, "gemm_stepl_kernel[gates]", [ALL, {"tok", "bias", "hb"}, {"bias", "nogates"}]),
    ("stepl_2seg", "hh", 64, 64, (64, 64), ST, HH, "gemm_stepl_kernel[gates]", [{"tok", "drop", "h2", "hb2"}, {"zx"}]),
    ("stepl_scalar_ep", "hh", 70, 64, (128,), ST, HH, "gemm_stepl_kernel[gates]", [ALL | {"misalign"}]),
    ("h_staged", "h", 33, 64, (64,), {}, HF, "gemm_step_kernel[2,2,w8]", [ALL, {"tok", "bias", "nogates"}]),
    ("h_staged_2seg", "h", 33, 64, (64, 64), NH, HF, "gemm_step_kernel[4,1,w4]", [{"zx", "bias", "hb"}, {"tok", "drop", "h2", "hb2"}, {"bias"}]),
    ("h_small", "h", 37, 40, (96,), {}, HF, "gemm_small_kernel[bf16,4,gates]", [ALL, {"tok", "bias", "nogates"}]),
    ("h_small_2seg", "h", 37, 40, (48, 48), {}, HF, "gemm_small_kernel[bf16,4,gates]", [{"zx", "drop", "h2", "hb2"}]),
]


def run_gf(case, capfd, random=False):
    name, which, M, H, segs, env, fn, kernel, optsets = case
    a_dtype = torch.bfloat16 if which == "hh" else torch.float32
    probs = [gf_problem(M, H, segs, o, 100 + 10 * i, a_dtype, random) for i, o in enumerate(optsets)]
    arr = (GatesFwd * len(probs))(*[p[0] for p in probs])
    capfd.readouterr()
    call(f"kp_small_gates_fwd_{which}", len(probs), C.cast(arr, vp), M, H)
    torch.cuda.synchronize()
    expect(capfd, fn, kernel)
    worst = max(gf_check(o, ref, sum(segs), f"{name} problem {i}", random) for i, (_, o, ref, _) in enumerate(probs))
    return worst, z_share([p[2] for p in probs])


@pytest.mark.parametrize("case", GF_CASES, ids=[c[0] for c in GF_CASES])
def test_gates_fwd_exact(case, monkeypatch, capfd):
    setenv(monkeypatch, case[5])
    worst, share = run_gf(case, capfd)
    print(f"[step-kernels] gates_fwd {case[0]} {case[7]}: largest error / tolerance = {worst:.3f}, share of |z| <= 4 = {share:.3f}")
    assert share >= 0.9, "the operand ranges leave too many saturated pre-activations for the 2e-5 bound to see one wrong product"


@pytest.mark.parametrize("name", ["half_w8_2seg", "stepl", "h_staged", "h_small"])
def test_gates_fwd_random(name, monkeypatch, capfd):
    case = next(c for c in GF_CASES if c[0] == name)
    setenv(monkeypatch, case[5])
    worst, _ = run_gf(case, capfd, random=True)
    print(f"[step-kernels] gates_fwd random {name} {case[7]}: largest error / (2e-5 + 2 bound) = {worst:.3f}")


def test_big_step_gates_fwd(monkeypatch, capfd):
    M, H, segs = 130, 256, (64, 64)
    p, o, ref, keep = gf_problem(M, H, segs, {"tok", "bias", "drop", "h2", "hb", "hb2"}, 140, torch.bfloat16)
    zbuf = Buf((M * 4 * H,), fill=SENT)
    taken = C.c_int(-1)
    capfd.readouterr()
    call("kp_big_step_gates_fwd", C.byref(p), M, H, zbuf.ptr(), M * 4 * H, C.byref(taken))
    torch.cuda.synchronize()
    assert taken.value == 0 and not trace_of(capfd, "big_step_gates_fwd"), "taken without AOCR_BIG_STEP=1"
    assert torch.equal(o["c"].win(), torch.full((M, H), SENT))
    setenv(monkeypatch, BIG)
    call("kp_big_step_gates_fwd", C.byref(p), M, H, zbuf.ptr(), M * 4 * H - 1, C.byref(taken))
    assert taken.value == 0, "taken with a scratch one float short"
    capfd.readouterr()
    call("kp_big_step_gates_fwd", C.byref(p), M, H, zbuf.ptr(), M * 4 * H, C.byref(taken))
    torch.cuda.synchronize()
    assert taken.value == 1
    lines = trace_of(capfd, "big_step_gates_fwd")
    assert len(lines) == 2 and ": gemm_dma128_kernel[8,8] 130 1024 128" in lines[0] and ": gates_elem_fwd_kernel[] 130 256 0" in lines[1], lines
    zbuf.check_tail("zbuf")
    assert torch.equal(zbuf.cpu().double().view(M, 4 * H), ref["prod"]), "the scratch z is not the exact product"
    worst, share = gf_check(o, ref, sum(segs), "big_step_gates_fwd"), z_share([ref])
    print(f"[step-kernels] big_step_gates_fwd: largest error / tolerance = {worst:.3f}, share of |z| <= 4 = {share:.3f}")
    assert share >= 0.9


# ------------------------------------------------------------------------------------------------------------------------------
# plain products (EpStore)
# ------------------------------------------------------------------------------------------------------------------------------
QP = 2.0 ** -3                      # B-side quantum of the plain cases
VARIANTS = ("shadow", "bias_relu", "accum", "split", "tanh_bwd", "tanh")


def st_problem(M, N, segs, variant, seed, a_dtype, random=False):
    K = sum(segs)
    if random:
        A, B = rb(rnd(M, K, seed=seed)), rb(rnd(N, K, seed=seed + 1))
    else:
        A, B = ints(M, K, seed=seed, lo=-2, hi=2), ints(N, K, seed=seed + 1, lo=-2, hi=2) * QP
    p, keep = Store(), []
    p.a, ka = operand(A, segs, a_dtype, vary=seed % 2)
    p.b, kb = operand(B, segs, torch.bfloat16, vary=(seed + 1) % 2)
    x = A.double() @ B.double().t()
    mag = A.double().abs() @ B.double().abs().t()
    o = {}
    if variant in ("bias_relu", "accum", "split"):
        b1, b2 = ints(N, seed=seed + 2), ints(N, seed=seed + 3) * QP
        m1, m2 = Buf(b1), Buf(b2)
        keep += [m1, m2]
        p.bias = m1.full.data_ptr()
        x = x + b1.double()
        if variant != "accum":
            p.bias2 = m2.full.data_ptr()
            x = x + b2.double()
    if variant == "bias_relu":
        p.flags = EP_RELU
        x = x.clamp(min=0)
    if variant == "tanh":
        p.flags = EP_TANH
        x = torch.tanh(x)
    if variant == "tanh_bwd":
        dg = ints(M, N, seed=seed + 4, lo=-6, hi=6)
        dout = ints(M, N, seed=seed + 5, lo=-1, hi=1) * 0.5
        md = Mat(M, N, data=dg, pad=4), Mat(M, N, data=dout, pad=4)
        keep += md
        p.dg, p.dout, p.ldd = md[0].addr, md[1].addr, md[0].ld
        x = (x + dg.double()) * (1 - dout.double() ** 2)
    N0 = N
    if variant == "accum":
        c0 = ints(M, N, seed=seed + 6, lo=-30, hi=30)
        o["C"] = Mat(M, N, data=c0, pad=8)
        p.flags = EP_ACCUM
        x = c0.double() + x
    else:
        o["C"] = out(M, N, pad=8)
    if variant == "split":
        N0 = N - 24                                                       # the second destination takes the last 24 columns
        o["C1"] = out(M, N - N0, pad=4, off=4)
        p.C1, p.ldc1, p.N0 = o["C1"].addr, o["C1"].ld, N0
    if variant in ("shadow", "split"):
        o["Cb"] = out(M, N, torch.bfloat16, pad=8)
        p.Cb, p.ldcb = o["Cb"].addr, o["Cb"].ld
    p.C, p.ldc = o["C"].addr, o["C"].ld
    return p, o, dict(x=x, mag=mag, N0=N0, variant=variant), keep + ka + kb


def st_check(o, ref, K, what, random=False):
    for k, m in o.items():
        m.check(f"{what} {k}")
    x, N0, N = ref["x"], ref["N0"], ref["x"].shape[1]
    got = o["C"].win()
    worst = 0.0
    if random:
        worst = ratio(got, x, bound(ref["mag"], K) + 1e-30)
        assert worst <= 1.0, f"{what}: error / bound = {worst:.3f}"
    elif ref["variant"] == "tanh":
        worst = ratio(got, x, TOL_CELL)
        assert worst <= 1.0, f"{what}: tanh error / 2e-5 = {worst:.3f}"
    else:
        assert torch.equal(got[:, :N0].double(), x[:, :N0]), f"{what}: C (max diff {(got[:, :N0].double() - x[:, :N0]).abs().max().item()})"
        if N0 < N:
            assert torch.equal(got[:, N0:], torch.full((got.shape[0], N - N0), SENT)), f"{what}: C written past N0"
            assert torch.equal(o["C1"].win().double(), x[:, N0:]), f"{what}: C1"
    if "Cb" in o:
        cb = o["Cb"].win()
        assert torch.equal(cb[:, :N0].view(torch.int16), bf(got[:, :N0])), f"{what}: Cb is not the RNE of C"
        assert torch.equal(cb[:, N0:], torch.full((cb.shape[0], N - N0), -3.0, dtype=torch.bfloat16)), f"{what}: Cb written past N0"
    return worst


W16, MK = {"AOCR_STEP_WAVES16": "1"}, {"AOCR_STEP_MT2_MINK": "64"}
# (name, launcher, M, N, K segments, switches, trace function, kernel[instantiation], nz)
ST_CASES = [
    ("w8", "hh", 33, 32, (64,), {}, HH, "gemm_step_kernel[1,0,w8]", 2),
    ("w4", "hh", 33, 32, (64,), W4, HH, "gemm_step_kernel[1,0,w4]", 1),
    ("w16", "hh", 33, 64, (1024,), W16, HH, "gemm_step_kernel[1,0,w16]", 1),
    ("w8_2seg", "hh", 70, 96, (64, 128), {}, HH, "gemm_step_kernel[1,0,w8]", 3),
    ("mt2", "hh", 400, 1024, (64,), MK, HH, "gemm_step_kernel[1,0,w8,mt2]", 1),
    ("stepl", "hh", 70, 128, (128,), ST, HH, "gemm_stepl_kernel[plain]", 1),
    ("stepl_nz3", "hh", 70, 128, (128,), ST, HH, "gemm_stepl_kernel[plain]", 3),
    ("stepl_2seg", "hh", 64, 128, (64, 64), ST, HH, "gemm_stepl_kernel[plain]", 2),
    ("h_staged", "h", 33, 64, (64,), {}, HF, "gemm_step_kernel[1,0,w8]", 2),
    ("h_staged_w4_2seg", "h", 33, 64, (64, 64), W4, HF, "gemm_step_kernel[1,0,w4]", 1),
    ("h_staged_w16", "h", 33, 64, (1024,), W16, HF, "gemm_step_kernel[1,0,w16]", 1),
    ("h_small", "h", 37, 40, (96,), {}, HF, "gemm_small_kernel[bf16,1,plain]", 3),
    ("h_small_2seg", "h", 37, 40, (48, 48), {}, HF, "gemm_small_kernel[bf16,1,plain]", 1),
]


def run_st(case, variants, capfd, random=False):
    name, which, M, N, segs, env, fn, kernel, nz = case
    a_dtype = torch.bfloat16 if which == "hh" else torch.float32
    worst = 0.0
    for v, variant in enumerate(variants):
        probs = [st_problem(M, N, segs, variant, 300 + 20 * v + 7 * i, a_dtype, random) for i in range(nz)]
        arr = (Store * nz)(*[p[0] for p in probs])
        capfd.readouterr()
        call(f"kp_small_{which}", nz, C.cast(arr, vp), M, N)
        torch.cuda.synchronize()
        expect(capfd, fn, kernel)
        worst = max([worst] + [st_check(o, ref, sum(segs), f"{name} {variant} problem {i}", random) for i, (_, o, ref, _) in enumerate(probs)])
    return worst


@pytest.mark.parametrize("case", ST_CASES, ids=[c[0] for c in ST_CASES])
def test_store_exact(case, monkeypatch, capfd):
    setenv(monkeypatch, case[5])
    worst = run_st(case, VARIANTS, capfd)
    print(f"[step-kernels] store {case[0]} {case[7]}: bit-exact; EP_TANH largest error / 2e-5 = {worst:.3f}")


@pytest.mark.parametrize("name", ["w8_2seg", "stepl", "h_small"])
def test_store_random(name, monkeypatch, capfd):
    case = next(c for c in ST_CASES if c[0] == name)
    setenv(monkeypatch, case[5])
    worst = run_st(case, ("shadow",), capfd, random=True)
    print(f"[step-kernels] store random {name} {case[7]}: largest error / bound = {worst:.3f}")


def test_big_step_store(monkeypatch, capfd):
    M, N, segs = 130, 1024, (64,)
    taken = C.c_int(-1)
    p, o, ref, keep = st_problem(M, N, segs, "shadow", 400, torch.bfloat16)
    capfd.readouterr()
    call("kp_big_step_store", C.byref(p), M, N, C.byref(taken))
    torch.cuda.synchronize()
    assert taken.value == 0 and not trace_of(capfd, "big_step_store"), "taken without AOCR_BIG_STEP=1"
    assert torch.equal(o["C"].win(), torch.full((M, N), SENT))
    setenv(monkeypatch, BIG)
    worst = 0.0
    for v, variant in enumerate(VARIANTS):
        p, o, ref, keep = st_problem(M, N, segs, variant, 400 + 20 * v, torch.bfloat16)
        capfd.readouterr()
        call("kp_big_step_store", C.byref(p), M, N, C.byref(taken))
        torch.cuda.synchronize()
        assert taken.value == 1
        expect(capfd, "big_step_store", "gemm_dma128_kernel[8,8] 130 1024 64")
        worst = max(worst, st_check(o, ref, sum(segs), f"big_step_store {variant}"))
    print(f"[step-kernels] big_step_store gemm_dma128_kernel[8,8]: bit-exact; EP_TANH largest error / 2e-5 = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# gate backward
# ------------------------------------------------------------------------------------------------------------------------------
def gb_problem(M, H, segs, opts, seed, a_dtype, random=False):
    """opts: dh1, dh2, dh3, dc, drop, gil (gates [m][j][4]), dzb, alias (dc_out = dc_in, as the decoder's BPTT runs it), noprod (gates_elem_bwd)."""
    K = sum(segs)
    p, keep = GatesBwd(), []
    P = torch.zeros(M, H, dtype=torch.float64)
    mag = torch.zeros(M, H, dtype=torch.float64)
    if "noprod" not in opts:
        q = 2.0 ** -4 if K <= 64 else 2.0 ** -5 if K <= 256 else 2.0 ** -6      # keeps |dh| <= 4: the product's standard deviation stays near 0.6
        if random:
            A, B = rb(rnd(M, K, seed=seed)), rb(rnd(H, K, seed=seed + 1) * (1.0 / K ** 0.5))
        else:
            A, B = ints(M, K, seed=seed, lo=-2, hi=2), ints(H, K, seed=seed + 1, lo=-1, hi=1) * q
        p.a, ka = operand(A, segs, a_dtype, vary=seed % 2)
        p.b, kb = operand(B, segs, torch.bfloat16, vary=(seed + 1) % 2)
        keep += ka + kb
        P, mag = A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t()
    p.drop = no_drop()
    if "drop" in opts:
        p.drop, mask = drop_spec(0.25, 55 + seed, 2, 3, 77 * seed + 3, M * H)
        P, mag = P * mask.view(M, H).double(), mag * mask.view(M, H).double()
    dh = P.clone()
    for i, k in enumerate(("dh1", "dh2", "dh3")):
        if k in opts:
            t = (rnd(M, H, seed=seed + 10 + i) * 0.5).float()
            m = Mat(M, H, data=t, pad=4 + 4 * i, off=4 * i)
            setattr(p, k, m.addr); setattr(p, f"ld{i + 1}", m.ld)
            keep.append(m)
            dh = dh + t.double()
    g = rnd(M, 4, H, seed=seed + 20) * 2
    gates = torch.cat([torch.sigmoid(g[:, :3]), torch.tanh(g[:, 3:])], 1).float()            # [M][4][H]
    if "gil" in opts:
        mg = Mat(M, 4 * H, data=gates.permute(0, 2, 1).reshape(M, 4 * H), pad=4)
        p.gil = 1
    else:
        mg = Mat(M, 4 * H, data=gates.reshape(M, 4 * H), pad=12)                             # ldg > 4 H
    p.gates, p.ldg = mg.addr, mg.ld
    c, cp = (rnd(M, H, seed=seed + 21) * 1.5).float(), rnd(M, H, seed=seed + 22).float()
    mc, mcp = Mat(M, H, data=c, pad=4), Mat(M, H, data=cp, pad=8)
    p.c, p.ldcc, p.c_prev, p.ldcp = mc.addr, mc.ld, mcp.addr, mcp.ld
    o = dict(dz=out(M, 4 * H, pad=4))
    p.dz, p.lddz = o["dz"].addr, o["dz"].ld
    dcin = None
    if "dc" in opts:
        dcin = (rnd(M, H, seed=seed + 23) * 0.5).float()
        mdc = Mat(M, H, data=dcin, pad=4)
        p.dc_in, p.lddc = mdc.addr, mdc.ld
        keep.append(mdc)
    if "alias" in opts:
        o["dc_out"] = mdc
    else:
        o["dc_out"] = out(M, H, pad=4)
    p.dc_out, p.lddco = o["dc_out"].addr, o["dc_out"].ld
    if "dzb" in opts:
        o["dzb"] = out(M, 4 * H, torch.bfloat16, pad=8)
        p.dzb, p.lddzb = o["dzb"].addr, o["dzb"].ld
    ig, fg, og, gg = (gates[:, i].double() for i in range(4))
    tc = torch.tanh(c.double())
    dc = dh * og * (1 - tc * tc) + (dcin.double() if dcin is not None else 0)
    d_o, di, dg, df = dh * tc, dc * gg, dc * ig, dc * cp.double()
    dz = torch.cat([di * ig * (1 - ig), df * fg * (1 - fg), d_o * og * (1 - og), dg * (1 - gg * gg)], 1)
    return p, o, dict(dz=dz, dc_out=dc * fg, dh=dh, mag=mag), keep + [mg, mc, mcp]


def gb_check(o, ref, K, what, random=False):
    for k, m in o.items():
        m.check(f"{what} {k}")
    dhmax = ref["dh"].abs().max().item()
    if random:
        b = bound(ref["mag"], K)
        tols = dict(dz=TOL_CELL + 2 * torch.cat([b] * 4, 1), dc_out=TOL_CELL + 2 * b)
    else:
        assert dhmax <= 4.0, f"{what}: |dh| reaches {dhmax}: rescale the operands"
        tols = dict(dz=TOL_BWD * max(1.0, dhmax), dc_out=TOL_BWD * max(1.0, dhmax))
    worst = 0.0
    for k in ("dz", "dc_out"):
        r = ratio(o[k].win(), ref[k], tols[k])
        assert r <= 1.0, f"{what}: {k} error / tolerance = {r:.3f}"
        worst = max(worst, r)
    if "dzb" in o:
        assert torch.equal(o["dzb"].win().view(torch.int16), bf(o["dz"].win())), f"{what}: dzb is not the RNE of the kernel's own dz"
    return worst


FULL = {"dh1", "dh2", "dc", "drop", "dzb"}
# (name, launcher, M, H, K segments, switches, trace function, kernel[instantiation], options per problem)
GB_CASES = [
    ("w8", "hh", 33, 32, (64,), {}, HH, "gemm_step_kernel[1,0,w8]", [FULL, {"dh2", "dc", "gil", "dzb", "alias"}]),
    ("w4", "hh", 33, 32, (64,), W4, HH, "gemm_step_kernel[1,0,w4]", [{"dh1", "dh2", "dh3", "dc", "gil"}, set()]),
    ("w16", "hh", 33, 64, (1024,), W16, HH, "gemm_step_kernel[1,0,w16]", [FULL | {"gil"}]),
    ("stepl", "hh", 70, 128, (128,), ST, HH, "gemm_stepl_kernel[plain]", [FULL]),
    ("stepl_nz3", "hh", 70, 128, (128,), ST, HH, "gemm_stepl_kernel[plain]", [{"dh2", "dc", "gil", "dzb", "alias"}, {"dh1"}, {"dh1", "dh2", "dh3", "drop"}]),
    ("h_staged", "h", 33, 64, (64,), {}, HF, "gemm_step_kernel[1,0,w8]", [FULL, {"dh2", "gil"}]),
    ("h_small", "h", 37, 40, (96,), {}, HF, "gemm_small_kernel[bf16,1,plain]", [FULL, {"dh1", "dh2", "dh3", "dc", "gil", "dzb", "alias"}]),
]


def run_gb(case, capfd, random=False):
    name, which, M, H, segs, env, fn, kernel, optsets = case
    a_dtype = torch.bfloat16 if which == "hh" else torch.float32
    probs = [gb_problem(M, H, segs, o, 500 + 10 * i, a_dtype, random) for i, o in enumerate(optsets)]
    arr = (GatesBwd * len(probs))(*[p[0] for p in probs])
    capfd.readouterr()
    call(f"kp_small_gates_bwd_{which}", len(probs), C.cast(arr, vp), M, H)
    torch.cuda.synchronize()
    expect(capfd, fn, kernel)
    return max(gb_check(o, ref, sum(segs), f"{name} problem {i}", random) for i, (_, o, ref, _) in enumerate(probs))


@pytest.mark.parametrize("case", GB_CASES, ids=[c[0] for c in GB_CASES])
def test_gates_bwd_exact(case, monkeypatch, capfd):
    setenv(monkeypatch, case[5])
    worst = run_gb(case, capfd)
    print(f"[step-kernels] gates_bwd {case[0]} {case[7]}: largest error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("name", ["w8", "stepl", "h_small"])
def test_gates_bwd_random(name, monkeypatch, capfd):
    case = next(c for c in GB_CASES if c[0] == name)
    setenv(monkeypatch, case[5])
    worst = run_gb(case, capfd, random=True)
    print(f"[step-kernels] gates_bwd random {name} {case[7]}: largest error / (2e-5 + 2 bound) = {worst:.3f}")


@pytest.mark.parametrize("opts", [{"dh1", "dh2", "dh3", "dc", "gil", "dzb", "alias"}, {"dh1", "dzb"}], ids=["chain_top_cell", "dh1_only"])
def test_gates_elem_bwd(opts, capfd):
    M, H = 33, 40
    p, o, ref, keep = gb_problem(M, H, (0,), opts | {"noprod"}, 600, torch.bfloat16)
    capfd.readouterr()
    call("kp_gates_elem_bwd", C.byref(p), M, H)
    torch.cuda.synchronize()
    expect(capfd, "gates_elem_bwd", "gates_elem_bwd_kernel[] 33 40 0")
    worst = gb_check(o, ref, 0, "gates_elem_bwd")
    print(f"[step-kernels] gates_elem_bwd: largest error / tolerance = {worst:.3f}")
