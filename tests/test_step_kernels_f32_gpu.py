"""GPU: every branch of the exact-fp32 recurrent-step launchers (csrc/ops_gemm.hip: launch_small_gates_fwd, launch_small_kk, launch_small_kmn,
launch_small_gates_bwd_kk, launch_small_gates_bwd with bf16 = false) against an exact reference, called directly through tests/libkprobe.so
(kp_small_f32_*).  Structure of tests/test_step_kernels_bf16_gpu.py, operands of tests/test_kernels_f32_gpu.py, helpers of
tests/kernel_harness.py: strided windows of junk-filled buffers with sentinel tails, nz = 1..3 problems per launch, one- and two-segment A
(and K-contiguous B) operands, and the kernel of every launch asserted from its AOCR_TRACE line.

Operands.  One side of every product is wide integers (|v| <= 300, at least half of them outside bf16), the other small integers; one side
carries a power-of-two quantum where the epilogue is nonlinear, so every product and partial sum stays exact in fp32 in ANY order.
Plain products (EpStore, kk and kmn): bit-exact (bias + bias2, ReLU, accumulate onto a non-zero buffer, the C1 / N0 split); EP_TANH within
TOL_CELL of float64 tanh.  Gate forward: the float64 LSTM cell on the exact pre-activation, c / h / saved gates within TOL_CELL, at least
90 % of the pre-activations inside |z| <= 4 (asserted).  Gate backward: float64 of EpGatesBwd's formulas on the exact product, within
TOL_BWD max(1, max |dh|) with |dh| <= 4 (asserted); dh1..dh3 and dc_in present and absent.  Random operands: plain outputs within
bound(|A| |B|, K), gate outputs within TOL_CELL + 2 bound.

Branches (function launch_small):
  gates_fwd   gemm_step_f32_kernel[gates]            33, 8, 32 and 33, 64, 32 + 32
  gates_fwd   gemm_small_kernel[f32,quarter]         AOCR_NO_STEP_F32=1; K = 40 with no switch
  gates_fwd   gemm_small_kernel[f32,4,gates,w8|w4]   + AOCR_NO_QUARTER_TILES=1 (+ AOCR_STEP_WAVES4=1); H = 12 with no switch
  kk          gemm_step_f32_kernel[plain,w8|w16]     33, 32, 64; 32, 64, 2048 with AOCR_STEP_F32_W16=1
  kk          gemm_small_kernel[f32,1,plain,w8]      N = 40
  kmn / gates_bwd (LoadMN B)  gemm_small_kernel[f32,1,plain,w8|w4]
  gates_bwd_kk                gemm_step_f32_kernel[plain,w8]; gemm_small_kernel[f32,1,plain,w8] with AOCR_NO_STEP_F32=1"""
import ctypes as C

import pytest
import torch

from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module (tests/test_kernel_harness_cpu.py checks it)
from kernel_harness import (ST_VARIANTS, TOL_BWD, TOL_CELL, WIDE, Buf, GatesBwd, GatesFwd, Mat, Store, assert_exact_range, bound, call, expect, ints, no_drop,
                            operand, out, ratio, rnd, setenv, store_check, store_problem, vp, wide_ints)

pytestmark = pytest.mark.gpu

FN = "launch_small"
STEP_G, STEP_P8, STEP_P16 = "gemm_step_f32_kernel[gates]", "gemm_step_f32_kernel[plain,w8]", "gemm_step_f32_kernel[plain,w16]"
QUARTER, FULL8, FULL4 = "gemm_small_kernel[f32,quarter]", "gemm_small_kernel[f32,4,gates,w8]", "gemm_small_kernel[f32,4,gates,w4]"
PLAIN8, PLAIN4 = "gemm_small_kernel[f32,1,plain,w8]", "gemm_small_kernel[f32,1,plain,w4]"
NS, NQ, W4 = {"AOCR_NO_STEP_F32": "1"}, {"AOCR_NO_STEP_F32": "1", "AOCR_NO_QUARTER_TILES": "1"}, {"AOCR_NO_STEP_F32": "1", "AOCR_NO_QUARTER_TILES": "1", "AOCR_STEP_WAVES4": "1"}


def quantum(K, target, sd):
    """the power of two q with sqrt(K) sd q closest below `target`: the standard deviation the product is scaled to"""
    q = 1.0
    while (K ** 0.5) * sd * q > target:
        q /= 2
    return q


def scaled_pair(M, N, K, seed, wide_a, target):
    """A [M][K], B [N][K]: wide integers x (small integers times a power of two), every product exact; the product's deviation near `target`"""
    if wide_a:
        A, B = wide_ints(M, K, seed=seed), ints(N, K, seed=seed + 1, lo=-1, hi=1)
        q = quantum(K, target, 200.0 * 0.82)
    else:
        A, B = ints(M, K, seed=seed, lo=-2, hi=2), wide_ints(N, K, seed=seed + 1)
        q = quantum(K, target, 200.0 * 1.42)
    assert_exact_range(K, WIDE, 2)
    return A, B * q


def b_operand(p, B, segs, b_mn, seed):
    """B [cols][K]: K-contiguous in one or two segments (LoadK), or ONE segment stored [K][cols] (LoadMN)"""
    if b_mn:
        mb = Mat(B.shape[1], B.shape[0], data=B.t(), pad=8, off=4)
        p.b.p0, p.b.ld0, p.b.K0, p.b.rows = mb.addr, mb.ld, B.shape[1], B.shape[0]
        return [mb]
    p.b, kb = operand(B, segs, torch.float32, vary=(seed + 1) % 2)
    return kb


# ------------------------------------------------------------------------------------------------------------------------------
# gate forward
# ------------------------------------------------------------------------------------------------------------------------------
def gf_problem(M, H, segs, opts, seed, random=False):
    """opts: zx | tok (token table), bias, h2 (second copy, another stride), nogates"""
    K = sum(segs)
    if random:
        A, B = rnd(M, K, seed=seed).float(), (rnd(4 * H, K, seed=seed + 1) * (2.0 / K ** 0.5)).float()
    else:
        A, B = scaled_pair(M, 4 * H, K, seed, seed % 20 == 0, 1.0)
    p, keep = GatesFwd(), []
    p.a, ka = operand(A, segs, torch.float32, vary=seed % 2)
    keep += ka + b_operand(p, B, segs, False, seed)
    z, mag = A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t()
    if "bias" in opts:
        b1, b2 = ints(4 * H, seed=seed + 2, lo=-8, hi=8) / 16, ints(4 * H, seed=seed + 3, lo=-8, hi=8) / 16
        m1, m2 = Buf(b1), Buf(b2)
        p.b1, p.b2 = m1.full.data_ptr(), m2.full.data_ptr()
        z = z + (b1.double() + b2.double())
        keep += [m1, m2]
    if "zx" in opts or "tok" in opts:
        rows = 11 if "tok" in opts else M                                    # tok: an 11-row per-token table
        zx = ints(rows, 4 * H, seed=seed + 4, lo=-8, hi=8) / 16
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
    o = dict(c=out(M, H, pad=4), h=out(M, H, pad=8))
    p.c_out, p.ldc, p.h_out, p.ldh = o["c"].addr, o["c"].ld, o["h"].addr, o["h"].ld
    if "h2" in opts:
        o["h2"] = out(M, H, pad=12, off=4)
        p.h_out2, p.ldh2 = o["h2"].addr, o["h2"].ld
    if "nogates" not in opts:
        o["gates"] = out(M, 4 * H, pad=4)
        p.gates, p.ldg = o["gates"].addr, o["gates"].ld
    p.drop = no_drop()
    zz = z.view(M, 4, H)
    ig, fg, og, gg = torch.sigmoid(zz[:, 0]), torch.sigmoid(zz[:, 1]), torch.sigmoid(zz[:, 2]), torch.tanh(zz[:, 3])
    c = fg * cp.double() + ig * gg
    return p, o, dict(c=c, h=og * torch.tanh(c), gates=torch.cat([ig, fg, og, gg], 1), z=z, mag=mag), keep + [mcp]


def gf_check(o, ref, K, what, random=False):
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
    if "h2" in o:
        assert torch.equal(o["h2"].win(), o["h"].win()), f"{what}: h_out2 is not h"
    return worst


# (name, M, H, K segments, switches, kernel[instantiation], options per problem (nz = their number))
GF_CASES = [
    ("step_h8", 33, 8, (32,), {}, STEP_G, [{"zx", "bias"}]),
    ("step_2seg", 33, 64, (32, 32), {}, STEP_G, [{"tok", "bias", "h2"}, {"bias", "nogates"}, {"zx"}]),
    ("quarter", 33, 64, (32, 32), NS, QUARTER, [{"zx", "bias", "h2"}, {"tok", "nogates"}]),
    ("full_w8", 33, 64, (32, 32), NQ, FULL8, [{"zx", "bias"}, {"tok", "bias", "h2"}, {"bias", "nogates"}]),
    ("full_w4", 33, 64, (64,), W4, FULL4, [{"zx", "bias", "h2"}]),
    ("k40_quarter", 33, 8, (40,), {}, QUARTER, [{"zx", "bias"}, {"bias"}]),
    ("h12_full", 33, 12, (32,), {}, FULL8, [{"zx", "bias", "h2"}]),
]


def run_gf(case, capfd, random=False):
    name, M, H, segs, env, kernel, optsets = case
    probs = [gf_problem(M, H, segs, o, 3000 + 10 * i, random) for i, o in enumerate(optsets)]
    arr = (GatesFwd * len(probs))(*[p[0] for p in probs])
    capfd.readouterr()
    call("kp_small_f32_gates_fwd", len(probs), C.cast(arr, vp), M, H)
    torch.cuda.synchronize()
    expect(capfd, FN, kernel)
    worst = max(gf_check(o, ref, sum(segs), f"{name} problem {i}", random) for i, (_, o, ref, _) in enumerate(probs))
    z = torch.cat([p[2]["z"].reshape(-1) for p in probs])
    return worst, (z.abs() <= 4).double().mean().item()


@pytest.mark.parametrize("case", GF_CASES, ids=[c[0] for c in GF_CASES])
def test_gates_fwd_exact(case, monkeypatch, capfd):
    setenv(monkeypatch, case[4])
    worst, share = run_gf(case, capfd)
    print(f"[step-kernels-f32] gates_fwd {case[0]} {case[5]}: largest error / tolerance = {worst:.3f}, share of |z| <= 4 = {share:.3f}")
    assert share >= 0.9, "the operand ranges leave too many saturated pre-activations for the 2e-5 bound to see one wrong product"


@pytest.mark.parametrize("name", ["step_2seg", "quarter", "full_w8"])
def test_gates_fwd_random(name, monkeypatch, capfd):
    case = next(c for c in GF_CASES if c[0] == name)
    setenv(monkeypatch, case[4])
    worst, _ = run_gf(case, capfd, random=True)
    print(f"[step-kernels-f32] gates_fwd random {name} {case[5]}: largest error / (2e-5 + 2 bound) = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# plain products (EpStore): kk (B K-contiguous) and kmn (B stored [K][N])
# ------------------------------------------------------------------------------------------------------------------------------
# (name, wrapper, M, N, K segments, switches, kernel[instantiation], nz)
ST_CASES = [
    ("kk_w8", "kk", 33, 32, (64,), {}, STEP_P8, 2),
    ("kk_w8_2seg", "kk", 33, 64, (32, 32), {}, STEP_P8, 3),
    ("kk_w16", "kk", 32, 64, (2048,), {"AOCR_STEP_F32_W16": "1"}, STEP_P16, 1),
    ("kk_w16_off", "kk", 32, 64, (2048,), {}, STEP_P8, 1),
    ("kk_n40", "kk", 33, 40, (64,), {}, PLAIN8, 2),
    ("kk_no_step", "kk", 33, 32, (32, 32), NS, PLAIN8, 1),
    ("kk_no_step_w4", "kk", 33, 32, (64,), {"AOCR_NO_STEP_F32": "1", "AOCR_STEP_WAVES4": "1"}, PLAIN4, 1),
    ("kmn", "kmn", 33, 32, (64,), {}, PLAIN8, 3),
    ("kmn_ragged", "kmn", 33, 40, (32, 40), {}, PLAIN8, 1),
    ("kmn_w4", "kmn", 33, 32, (64,), {"AOCR_STEP_WAVES4": "1"}, PLAIN4, 1),
]


def run_st(case, variants, capfd, random=False):
    name, which, M, N, segs, env, kernel, nz = case
    worst = 0.0
    for v, variant in enumerate(variants):
        probs = [store_problem(M, N, segs, variant, 3300 + 20 * v + 7 * i, (v + i) % 2 == 0, random, b_mn=which == "kmn") for i in range(nz)]
        arr = (Store * nz)(*[p[0] for p in probs])
        capfd.readouterr()
        call(f"kp_small_f32_{which}", nz, C.cast(arr, vp), M, N)
        torch.cuda.synchronize()
        expect(capfd, FN, kernel)
        worst = max([worst] + [store_check(o, ref, sum(segs), f"{name} {variant} problem {i}", random, tanh_tol=TOL_CELL) for i, (_, o, ref, _) in enumerate(probs)])
    return worst


@pytest.mark.parametrize("case", ST_CASES, ids=[c[0] for c in ST_CASES])
def test_store_exact(case, monkeypatch, capfd):
    setenv(monkeypatch, case[5])
    worst = run_st(case, ST_VARIANTS, capfd)
    print(f"[step-kernels-f32] store {case[0]} {case[6]}: bit-exact; EP_TANH largest error = {worst:.2e}")


@pytest.mark.parametrize("name", ["kk_w8_2seg", "kk_n40", "kmn"])
def test_store_random(name, monkeypatch, capfd):
    case = next(c for c in ST_CASES if c[0] == name)
    setenv(monkeypatch, case[5])
    worst = run_st(case, ("plain",), capfd, random=True)
    print(f"[step-kernels-f32] store random {name} {case[6]}: largest error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# gate backward: gates_bwd_kk (B K-contiguous: the transposed weights) and gates_bwd (B stored [K][H])
# ------------------------------------------------------------------------------------------------------------------------------
def gb_problem(M, H, segs, opts, seed, b_mn, random=False):
    """opts: dh1, dh2, dh3, dc, gil (gates [m][j][4]), alias (dc_out = dc_in, as the decoder's BPTT runs it)"""
    K = sum(segs)
    p, keep = GatesBwd(), []
    if random:
        A, B = rnd(M, K, seed=seed).float(), (rnd(H, K, seed=seed + 1) * (1.0 / K ** 0.5)).float()
    else:
        A, B = scaled_pair(M, H, K, seed, seed % 20 == 0, 0.5)                # keeps |dh| <= 4
    p.a, ka = operand(A, segs, torch.float32, vary=seed % 2)
    keep += ka + b_operand(p, B, segs, b_mn, seed)
    P, mag = A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t()
    p.drop = no_drop()
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
    o["dc_out"] = mdc if "alias" in opts else out(M, H, pad=4)
    p.dc_out, p.lddco = o["dc_out"].addr, o["dc_out"].ld
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
    return worst


ALL = {"dh1", "dh2", "dh3", "dc"}
# (name, wrapper, M, H, K segments, switches, kernel[instantiation], options per problem)
GB_CASES = [
    ("kk_step", "gates_bwd_kk", 33, 32, (64,), {}, STEP_P8, [ALL, {"dh2", "dc", "gil", "alias"}, set()]),
    ("kk_step_2seg", "gates_bwd_kk", 33, 32, (32, 32), {}, STEP_P8, [{"dh1", "dc"}, ALL | {"gil"}]),
    ("kk_small", "gates_bwd_kk", 33, 32, (64,), NS, PLAIN8, [ALL, {"dh1"}]),
    ("mn", "gates_bwd", 33, 32, (128,), {}, PLAIN8, [ALL, {"dh2", "dc", "gil", "alias"}, set()]),
    ("mn_w4", "gates_bwd", 33, 32, (128,), {"AOCR_STEP_WAVES4": "1"}, PLAIN4, [ALL | {"gil"}, {"dh1"}]),
]


def run_gb(case, capfd, random=False):
    name, which, M, H, segs, env, kernel, optsets = case
    probs = [gb_problem(M, H, segs, o, 3600 + 10 * i, which == "gates_bwd", random) for i, o in enumerate(optsets)]
    arr = (GatesBwd * len(probs))(*[p[0] for p in probs])
    capfd.readouterr()
    call(f"kp_small_f32_{which}", len(probs), C.cast(arr, vp), M, H)
    torch.cuda.synchronize()
    expect(capfd, FN, kernel)
    return max(gb_check(o, ref, sum(segs), f"{name} problem {i}", random) for i, (_, o, ref, _) in enumerate(probs))


@pytest.mark.parametrize("case", GB_CASES, ids=[c[0] for c in GB_CASES])
def test_gates_bwd_exact(case, monkeypatch, capfd):
    setenv(monkeypatch, case[5])
    worst = run_gb(case, capfd)
    print(f"[step-kernels-f32] gates_bwd {case[0]} {case[6]}: largest error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("name", ["kk_step", "mn"])
def test_gates_bwd_random(name, monkeypatch, capfd):
    case = next(c for c in GB_CASES if c[0] == name)
    setenv(monkeypatch, case[5])
    worst = run_gb(case, capfd, random=True)
    print(f"[step-kernels-f32] gates_bwd random {name} {case[6]}: largest error / (2e-5 + 2 bound) = {worst:.3f}")
