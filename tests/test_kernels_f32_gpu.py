"""GPU: every exact-fp32 (compute="f32") conv / GEMM kernel branch against an exact reference, called directly through tests/libkprobe.so:
gemm_f32t_kernel (three tiles), gemm_lds_f32_kernel, gemm_f32w_kernel (both stagers) and gemm_big_kernel<false>, through aocr::gemm,
launch_big_kk (two-segment operands), grouped_wgrad and the three conv entry points with no bf16 shadow.  Method of
tests/test_kernels_bf16_gpu.py, helpers of tests/kernel_harness.py.

Wide-integer operands (the main method): ONE operand of every product is drawn from the integers in [-300, 300] with at least half of them
odd magnitudes above 256 -- not representable in bf16 --, the other from [-4, 4]; which side is wide alternates between the cases.
assert_exact_range holds K max|a| max|b| + |what the epilogue adds| below 2^24, so every partial sum is an exact fp32 integer in ANY order
(MFMA, split-K atomics, wave reductions), the reference is float64 on the CPU cast to fp32, and outputs are compared BIT for bit.  The
bf16 files use |v| <= 4, which a bf16 demotion of an operand would pass; these inputs fail on one.

Random operands (a few per launcher): the error against float64 stays within bound(|A| |B|, K) = BOUND_C sqrt(K) 2^-24 (|A| |B|);
tests/test_f32_bound_cpu.py checks BOUND_C = 4 against a float32 restatement of a sequential fused-multiply-add chain at these K.  With
ksplit = 1 gemm_f32t_kernel (every tile), gemm_lds_f32_kernel and gemm_big_kernel<false> share the k order per output element, and their
outputs on the same random inputs are asserted bit-identical to one another.

Every case asserts the kernel it reached from the AOCR_TRACE line; operands are windows of wider buffers filled with junk, every buffer
has a sentinel tail, accumulating outputs start non-zero."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module (tests/test_kernel_harness_cpu.py checks it)
from kernel_harness import (EP_ACCUM, EP_RELU, EP_TANH, SENT, ST_VARIANTS, TQ, WIDE, Buf, Mat, assert_exact_range, bound, call, check_exact, eq_bits, expect,
                            ints, nhwc, out, pair, ratio, rnd, setenv, store_check, store_problem, trace_of, vp, wide_ints)

pytestmark = pytest.mark.gpu

EP_ATOMIC = 8
F32T, LDS, F32W, BIG = "gemm_f32t_kernel[", "gemm_lds_f32_kernel[]", "gemm_f32w_kernel[]", "gemm_big_kernel[f32]"


# ------------------------------------------------------------------------------------------------------------------------------
# aocr::gemm (kp_gemm, bf16 = 0): C [M][N] = A B^T with A [M][K] (k-major) or [K][M], B [N][K] (k-major) or [K][N]
# ------------------------------------------------------------------------------------------------------------------------------
def run_gemm(A, Bm, layout, flags=0, bias=None, bias2=None, C0=None, pad=8, off=0, pad_b=None):
    """A [M][K], Bm [N][K] as values; layout kk | kmn | mnmn says how they lie in memory.  -> the output window"""
    M, K = A.shape
    N = Bm.shape[0]
    a_k, b_k = layout in ("kk", "kmn"), layout == "kk"
    am = Mat(M, K, data=A, pad=pad, off=off) if a_k else Mat(K, M, data=A.t(), pad=pad, off=off)
    pad_b = pad if pad_b is None else pad_b
    bm = Mat(N, K, data=Bm, pad=pad_b, off=off) if b_k else Mat(K, N, data=Bm.t(), pad=pad_b, off=off)
    cm = Mat(M, N, data=C0, pad=8) if C0 is not None else out(M, N)
    keep = [Buf(b) if b is not None else None for b in (bias, bias2)]
    rc = C.c_int(-1)
    call("kp_gemm", 0, vp(am.addr), am.ld, int(a_k), vp(bm.addr), bm.ld, int(b_k), vp(cm.addr), cm.ld, M, N, K,
         keep[0].ptr() if keep[0] else None, keep[1].ptr() if keep[1] else None, flags, C.byref(rc))
    torch.cuda.synchronize()
    assert rc.value == 0
    cm.check("C")
    return cm.win()


NO_T, NO_L = {"AOCR_NO_F32T": "1"}, {"AOCR_NO_LDS_F32": "1"}
# (name, layout, M, N, K, switches, kernel[instantiation], operand window (pad, off[, pad of B]))
GEMM_CASES = [
    ("kk_thresholds", "kk", 96, 16, 32, {}, F32T + "64x64]", (8, 0)),
    ("kk_ragged", "kk", 97, 39, 40, {}, F32T + "64x64]", (8, 4)),
    ("kk_ragged_tile1", "kk", 130, 200, 72, {"AOCR_F32T_TILE": "1"}, F32T + "128x128]", (8, 4)),
    ("kk_ragged_tile2", "kk", 130, 200, 72, {"AOCR_F32T_TILE": "2"}, F32T + "64x128]", (8, 4)),
    ("kk_auto_64x128", "kk", 16384, 256, 32, {}, F32T + "64x128]", (8, 0)),
    ("kk_auto_128x128", "kk", 32768, 256, 32, {}, F32T + "128x128]", (8, 0)),
    ("kk_no_f32t", "kk", 97, 100, 40, NO_T, LDS, (8, 4)),
    ("kk_k36", "kk", 96, 64, 36, {}, LDS, (8, 0)),
    ("kk_ld47", "kk", 96, 64, 40, {}, LDS, (7, 0)),
    ("kk_m95", "kk", 95, 80, 64, {}, BIG, (8, 0)),
    ("kk_n15", "kk", 96, 15, 64, {}, BIG, (8, 0)),
    ("kk_k31", "kk", 96, 80, 31, {}, BIG, (8, 0)),
    ("kk_projector", "kk", 39, 300, 777, {}, BIG, (8, 4)),
    ("kk_no_lds_f32", "kk", 97, 100, 40, NO_L, BIG, (8, 4)),
    ("kmn", "kmn", 100, 70, 50, {}, BIG, (8, 4)),
    ("mnmn_thresholds", "mnmn", 64, 64, 64, {}, F32W, (8, 0)),
    ("mnmn_ragged", "mnmn", 68, 132, 70, {}, F32W, (8, 4)),
    ("mnmn_rows66", "mnmn", 66, 64, 64, {}, BIG, (6, 0, 8)),          # both strides multiples of 4: only rows % 4 keeps it off gemm_f32w_kernel
    ("mnmn_k63", "mnmn", 64, 64, 63, {}, BIG, (8, 0)),
    ("mnmn_no_f32w", "mnmn", 68, 132, 70, {"AOCR_NO_F32W": "1"}, BIG, (8, 4)),
]


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_exact(case, monkeypatch, capfd):
    name, layout, M, N, K, env, kernel, win = case
    setenv(monkeypatch, env)
    A, Bm = pair(M, N, K, 1000 + 2 * GEMM_CASES.index(case), wide_a=GEMM_CASES.index(case) % 2 == 0)
    assert_exact_range(K, WIDE, 4)
    capfd.readouterr()
    got = run_gemm(A, Bm, layout, pad=win[0], off=win[1], pad_b=win[2] if len(win) > 2 else None)
    expect(capfd, "gemm", kernel)
    eq_bits(got, A.double() @ Bm.double().t(), name)


# split-K: EP_ATOMIC into a non-zero C, K = 200 -> three k ranges of 96, 96 and 8 (the ragged last one)
@pytest.mark.parametrize("name,env,kernel", [("f32t", {}, F32T), ("lds_f32", NO_T, LDS), ("big", NO_L, BIG)])
def test_gemm_kk_split_k_exact(name, env, kernel, monkeypatch, capfd):
    M, N, K = 130, 130, 200
    setenv(monkeypatch, env)
    A, Bm = pair(M, N, K, 1100, wide_a=name != "lds_f32")
    C0 = ints(M, N, seed=1102, lo=-1000, hi=1000)
    assert_exact_range(K, WIDE, 4, 1000)
    capfd.readouterr()
    got = run_gemm(A, Bm, "kk", flags=EP_ATOMIC, C0=C0)
    expect(capfd, "gemm", kernel)
    eq_bits(got, C0.double() + A.double() @ Bm.double().t(), name)


@pytest.mark.parametrize("mink,split", [("32", 3), (None, 1)], ids=["mink32", "default"])
def test_gemm_mnmn_split_exact(mink, split, monkeypatch, capfd):
    """gemm_f32w_kernel's split: the caller's 3 ranges stand with AOCR_F32W_MINK=32 and are clamped to 1 by the default of 192"""
    M, N, K = 68, 132, 200
    if mink:
        monkeypatch.setenv("AOCR_F32W_MINK", mink)
    A, Bm = pair(M, N, K, 1110, wide_a=split == 1)
    C0 = ints(M, N, seed=1112, lo=-1000, hi=1000)
    assert_exact_range(K, WIDE, 4, 1000)
    capfd.readouterr()
    got = run_gemm(A, Bm, "mnmn", flags=EP_ATOMIC, C0=C0, off=4)
    lines = trace_of(capfd, "gemm")
    assert len(lines) == 1 and lines[0].endswith(f": gemm_f32w_kernel[] {M} {N} {K} {split}"), lines
    eq_bits(got, C0.double() + A.double() @ Bm.double().t(), f"mnmn split {split}")


# ------------------------------------------------------------------------------------------------------------------------------
# launch_big_kk (kp_big_kk_f32): two-segment LoadK operands and the whole EpStore
# ------------------------------------------------------------------------------------------------------------------------------
def run_big_kk(M, N, segs, variant, seed, wide_a, capfd, kernel, ksplit=1, random=False):
    p, o, ref, keep = store_problem(M, N, segs, variant, seed, wide_a, random)
    capfd.readouterr()
    call("kp_big_kk_f32", C.byref(p), M, N, ksplit)
    torch.cuda.synchronize()
    expect(capfd, "launch_big_kk", kernel)
    return store_check(o, ref, sum(segs), f"{kernel} {variant}", random), o


# (name, M, N, K segments, switches, kernel)
KK_CASES = [
    ("f32t_2seg", 100, 70, (16, 24), {}, F32T + "64x64]"),
    ("lds_f32_2seg_novec", 100, 70, (8, 32), {}, LDS),
    ("f32t_tile1", 130, 200, (72,), {"AOCR_F32T_TILE": "1"}, F32T + "128x128]"),
    ("f32t_tile2", 130, 200, (32, 40), {"AOCR_F32T_TILE": "2"}, F32T + "64x128]"),
    ("lds_f32", 97, 100, (40,), NO_T, LDS),
    ("big", 97, 100, (16, 24), NO_L, BIG),
]


@pytest.mark.parametrize("case", KK_CASES, ids=[c[0] for c in KK_CASES])
def test_big_kk_epilogues_exact(case, monkeypatch, capfd):
    name, M, N, segs, env, kernel = case
    setenv(monkeypatch, env)
    for v, variant in enumerate(ST_VARIANTS):
        run_big_kk(M, N, segs, variant, 1200 + 10 * v, v % 2 == 0, capfd, kernel)


def test_f32_kernels_bit_identical_on_random_operands(monkeypatch, capfd):
    """ksplit = 1: gemm_f32t_kernel (every tile), gemm_lds_f32_kernel and gemm_big_kernel<false> sum every output element's products in
    the same order (chunk c, MFMA s: k = 8 c + s, then 8 c + 4 + s) -- the kernel-level form of test_f32t_kernel_matches_lds_f32_kernel."""
    M, N, segs = 130, 200, (32, 40)
    wins = {}
    for name, env, kernel in (("t64x64", {"AOCR_F32T_TILE": "3"}, F32T + "64x64]"), ("t64x128", {"AOCR_F32T_TILE": "2"}, F32T + "64x128]"),
                              ("t128x128", {"AOCR_F32T_TILE": "1"}, F32T + "128x128]"), ("lds", NO_T, LDS), ("big", NO_L, BIG)):
        with monkeypatch.context() as mp:
            setenv(mp, env)
            r, o = run_big_kk(M, N, segs, "plain", 1300, True, capfd, kernel, random=True)
        print(f"[f32-kernels] launch_big_kk random {kernel}: largest error / bound = {r:.3f}")
        wins[name] = o["C"].win()
    for name, w in wins.items():
        assert torch.equal(w.view(torch.int32), wins["big"].view(torch.int32)), f"{name} differs from gemm_big_kernel<false> in {(w != wins['big']).sum().item()} elements"


@pytest.mark.parametrize("layout,M,N,K,kernel", [("mnmn", 68, 132, 70, F32W), ("kmn", 100, 70, 50, BIG)])
def test_gemm_random(layout, M, N, K, kernel, capfd):
    A, Bm = rnd(M, K, seed=1400).float(), rnd(N, K, seed=1401).float()
    capfd.readouterr()
    got = run_gemm(A, Bm, layout, off=4)
    expect(capfd, "gemm", kernel)
    r = ratio(got, A.double() @ Bm.double().t(), bound(A.double().abs() @ Bm.double().abs().t(), K) + 1e-30)
    print(f"[f32-kernels] gemm random {layout} {kernel}: largest error / bound = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("flags", [0, EP_RELU, EP_ACCUM, EP_TANH], ids=["bias2", "relu", "accum", "tanh"])
def test_gemm_mnmn_epilogues_exact(flags, capfd):
    """gemm_f32w_kernel's epilogues (aocr::gemm has no split output)"""
    M, N, K = 68, 132, 70
    A, Bm = pair(M, N, K, 1500 + flags, wide_a=flags in (0, EP_ACCUM))
    if flags == EP_TANH:
        Bm = Bm * TQ
    b1, b2, C0 = ints(N, seed=1510, lo=-500, hi=500), ints(N, seed=1511, lo=-500, hi=500), ints(M, N, seed=1512, lo=-1000, hi=1000)
    assert_exact_range(K, WIDE, 4, 2000)
    x = A.double() @ Bm.double().t() + (0 if flags == EP_TANH else b1.double() + b2.double())
    x = x.clamp(min=0) if flags == EP_RELU else torch.tanh(x) if flags == EP_TANH else C0.double() + x if flags == EP_ACCUM else x
    capfd.readouterr()
    got = run_gemm(A, Bm, "mnmn", flags=flags, bias=None if flags == EP_TANH else b1, bias2=None if flags == EP_TANH else b2,
                   C0=C0 if flags == EP_ACCUM else None, off=4)
    expect(capfd, "gemm", F32W)
    if flags == EP_TANH:
        assert (got.double() - x).abs().max().item() <= 1e-5
    else:
        eq_bits(got, x, f"mnmn flags {flags}")


# ------------------------------------------------------------------------------------------------------------------------------
# grouped_wgrad (bf16 = 0): one aocr::gemm per problem, C_i [M_i][N_i] += A_i^T B_i
# ------------------------------------------------------------------------------------------------------------------------------
def test_grouped_wgrad_exact(capfd):
    problems = [(128, 64, 100, F32W), (96, 40, 77, BIG), (68, 132, 200, F32W)]            # (M, N, K, kernel)
    n, keep, refs = len(problems), [], []
    cols = {k: [] for k in ("A", "lda", "B", "ldb", "C", "ldc", "M", "N", "K")}
    for i, (M, N, K, _) in enumerate(problems):
        a, b = pair(M, N, K, 1600 + 3 * i, wide_a=i % 2 == 0)                                # a [M][K], b [N][K] as values
        c0 = ints(M, N, seed=1602 + 3 * i, lo=-1000, hi=1000)
        assert_exact_range(K, WIDE, 4, 1000)
        am, bm, cm = Mat(K, M, data=a.t(), pad=4, off=4), Mat(K, N, data=b.t(), pad=8), Mat(M, N, data=c0, pad=4)
        keep += [am, bm, cm]
        for k, v in (("A", am.addr), ("B", bm.addr), ("C", cm.addr), ("lda", am.ld), ("ldb", bm.ld), ("ldc", cm.ld), ("M", M), ("N", N), ("K", K)):
            cols[k].append(v)
        refs.append((cm, c0.double() + a.double() @ b.double().t()))
    P, L, I = (lambda k: (C.c_void_p * n)(*cols[k])), (lambda k: (C.c_int64 * n)(*cols[k])), (lambda k: (C.c_int * n)(*cols[k]))
    nul = (C.c_void_p * n)()
    capfd.readouterr()
    call("kp_grouped_wgrad", 0, n, P("A"), L("lda"), P("B"), L("ldb"), P("C"), L("ldc"), I("M"), I("N"), I("K"), nul, nul, None, 0)
    torch.cuda.synchronize()
    lines = trace_of(capfd, "grouped_wgrad")
    assert len(lines) == n, lines
    for (M, N, K, kernel), ln, (cm, ref) in zip(problems, lines, refs):
        assert f": {kernel} {M} {N} {K}" in ln, (kernel, ln)
        cm.check(f"C {M}x{N}")
        eq_bits(cm.win(), ref, f"grouped problem {M}x{N}x{K}")


# ------------------------------------------------------------------------------------------------------------------------------
# conv_forward (bf16 = 0, no shadows): LoadConvK x LoadK, EpConv (bias, ReLU, the two poolings and their arg-max)
# ------------------------------------------------------------------------------------------------------------------------------
T1, T2 = {"AOCR_F32T_TILE": "1"}, {"AOCR_F32T_TILE": "2"}
# (name, B, H, W, Cin, Cout, ks, pad, switches, kernel)
FWD_CASES = [
    ("base", 1, 4, 25, 32, 64, 3, 1, {}, F32T + "64x64]"),
    ("tile1", 2, 4, 25, 32, 128, 3, 1, T1, F32T + "128x128]"),           # a pool window's four rows meet the 128-row tile seam and a ragged last tile
    ("tile2", 2, 4, 25, 32, 128, 3, 1, T2, F32T + "64x128]"),            # ... and the 64-row seams
    ("conv7", 2, 2, 50, 32, 64, 2, 0, {}, F32T + "64x64]"),
    ("cin16", 2, 4, 25, 16, 64, 3, 1, {}, LDS),
    ("small", 1, 2, 9, 32, 64, 3, 1, {}, BIG),                            # rows < 96
]


def conv_operands(B, H, W, Cin, Cout, ks, seed, wide_x):
    x = wide_ints(B, Cin, H, W, seed=seed) if wide_x else ints(B, Cin, H, W, seed=seed)
    w = ints(Cout, Cin, ks, ks, seed=seed + 1) if wide_x else wide_ints(Cout, Cin, ks, ks, seed=seed + 1)
    assert_exact_range(ks * ks * Cin, WIDE, 4, 1000)
    return x, w, ints(Cout, seed=seed + 2, lo=-1000, hi=1000)


def run_forward(x, w, b, ks, pad, relu, pool):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    oshape = (B, Ho, Wo, Cout) if pool == 0 else (B, Ho // 2, Wo // 2, Cout) if pool == 1 else (B, Ho // 2, Wo, Cout)
    xd, wd, bd = Buf(nhwc(x)), Buf(w.permute(0, 2, 3, 1)), Buf(b)
    y = Buf(oshape, fill=SENT)
    idx = Buf(oshape, torch.uint8, fill=0x77) if pool else None
    call("kp_conv_forward", 0, xd.ptr(), wd.ptr(), bd.ptr(), y.ptr(), idx.ptr() if idx else None, B, H, W, Cin, Cout, ks, pad, relu, pool,
         None, None, None, None, None, None, None, None)
    torch.cuda.synchronize()
    y.check_tail("y")
    if idx:
        idx.check_tail("idx")
    return dict(y=y, yb=None, idx=idx)


@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_conv_forward_exact(case, monkeypatch, capfd):
    name, B, H, W, Cin, Cout, ks, pad, env, kernel = case
    setenv(monkeypatch, env)
    x, w, b = conv_operands(B, H, W, Cin, Cout, ks, 2000, wide_x=FWD_CASES.index(case) % 2 == 0)
    z0 = F.conv2d(x.double(), w.double(), b.double(), padding=pad).float()          # exact: integers below 2^24
    pools = (0, 1, 2) if z0.shape[2] >= 2 else (0,)
    for relu in (0, 1):
        z = F.relu(z0) if relu else z0
        for pool in pools:
            capfd.readouterr()
            res = run_forward(x, w, b, ks, pad, relu, pool)
            # a pooled launch of the small case has fewer rows still; every launch of a case names the same kernel
            expect(capfd, "conv_forward", kernel)
            check_exact(res, z, pool, f"{name} relu={relu} pool={pool}")


@pytest.mark.parametrize("name", ["base", "cin16", "small"])
def test_conv_forward_random(name, monkeypatch, capfd):
    _, B, H, W, Cin, Cout, ks, pad, env, kernel = next(c for c in FWD_CASES if c[0] == name)
    setenv(monkeypatch, env)
    x, w, b = rnd(B, Cin, H, W, seed=2100).float(), (rnd(Cout, Cin, ks, ks, seed=2101) / (ks * ks * Cin) ** 0.5).float(), (rnd(Cout, seed=2102) * 0.1).float()
    ref = nhwc(F.conv2d(x.double(), w.double(), b.double(), padding=pad))
    mag = nhwc(F.conv2d(x.double().abs(), w.double().abs(), None, padding=pad) + b.double().abs().view(1, -1, 1, 1))
    capfd.readouterr()
    res = run_forward(x, w, b, ks, pad, 0, 0)
    expect(capfd, "conv_forward", kernel)
    r = ratio(res["y"].cpu(), ref, bound(mag, ks * ks * Cin) + 2.0 ** -24 * ref.abs())
    print(f"[f32-kernels] conv_forward random {name} {kernel}: largest error / bound = {r:.3f}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# conv_backward_data: the model's path (re-laid taps wtf -> LoadConvK x LoadK) and the LoadConvWT path of a null wtf
# ------------------------------------------------------------------------------------------------------------------------------
# (name, B, H, W, Cin, Cout, ks, pad, switches, kernel with wtf)
DGRAD_CASES = [
    ("base", 1, 4, 25, 32, 64, 3, 1, {}, F32T + "64x64]"),
    ("tile1", 2, 4, 25, 32, 128, 3, 1, T1, F32T + "128x128]"),
    ("tile2", 2, 4, 25, 32, 128, 3, 1, T2, F32T + "64x128]"),
    ("conv7", 2, 2, 50, 32, 64, 2, 0, {}, F32T + "64x64]"),
    ("cin16", 2, 4, 25, 16, 64, 3, 1, {}, F32T + "64x64]"),
    ("cin40", 1, 4, 25, 40, 64, 3, 1, {}, F32T + "64x64]"),                # the N edge: 40 of a 64-column tile
    ("small", 1, 2, 9, 32, 64, 3, 1, {}, BIG),                            # rows < 96
]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_conv_backward_data_exact(case, monkeypatch, capfd):
    name, B, H, W, Cin, Cout, ks, pad, env, kernel = case
    setenv(monkeypatch, env)
    Ho, Wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    wide_dy = DGRAD_CASES.index(case) % 2 == 0
    dy = wide_ints(B, Cout, Ho, Wo, seed=2200) if wide_dy else ints(B, Cout, Ho, Wo, seed=2200)
    w = ints(Cout, Cin, ks, ks, seed=2201) if wide_dy else wide_ints(Cout, Cin, ks, ks, seed=2201)
    assert_exact_range(ks * ks * Cout, WIDE, 4)
    ref = nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), w.double(), dy.double(), padding=pad))
    dyd, wd = Buf(nhwc(dy)), Buf(w.permute(0, 2, 3, 1))
    wtf = Buf((Cin, ks * ks, Cout), fill=SENT)
    call("kp_conv_weight_transpose_f32", wd.ptr(), wtf.ptr(), Cout, ks * ks, Cin)
    torch.cuda.synchronize()
    wtf.check_tail("wtf")
    eq_bits(wtf.cpu(), w.permute(1, 2, 3, 0).reshape(Cin, ks * ks, Cout).double(), f"{name}: wtf")
    dx = Buf((B, H, W, Cin), fill=SENT)
    capfd.readouterr()
    call("kp_conv_backward_data_f32", dyd.ptr(), wd.ptr(), wtf.ptr(), dx.ptr(), B, H, W, Cin, Cout, ks, pad)
    torch.cuda.synchronize()
    expect(capfd, "conv_backward_data", kernel)
    dx.check_tail("dx")
    eq_bits(dx.cpu(), ref, f"{name}: dx (wtf)")
    # a null wtf: LoadConvWT is neither 8-k-chunked nor K-contiguous -> the fragment-from-global kernel, on every run
    for _ in range(2):
        dx = Buf((B, H, W, Cin), fill=SENT)
        capfd.readouterr()
        call("kp_conv_backward_data", 0, dyd.ptr(), wd.ptr(), dx.ptr(), B, H, W, Cin, Cout, ks, pad, None, None, None)
        torch.cuda.synchronize()
        expect(capfd, "conv_backward_data", BIG)
        dx.check_tail("dx")
        eq_bits(dx.cpu(), ref, f"{name}: dx (LoadConvWT)")


def test_conv_backward_data_random(capfd):
    _, B, H, W, Cin, Cout, ks, pad, _, kernel = DGRAD_CASES[0]
    w, dy = (rnd(Cout, Cin, ks, ks, seed=2300) / 17.0).float(), rnd(B, Cout, H, W, seed=2301).float()
    ref = nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), w.double(), dy.double(), padding=pad))
    mag = nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), w.double().abs(), dy.double().abs(), padding=pad))
    dyd, wd, wtf, dx = Buf(nhwc(dy)), Buf(w.permute(0, 2, 3, 1)), Buf((Cin, ks * ks, Cout), fill=SENT), Buf((B, H, W, Cin), fill=SENT)
    call("kp_conv_weight_transpose_f32", wd.ptr(), wtf.ptr(), Cout, ks * ks, Cin)
    capfd.readouterr()
    call("kp_conv_backward_data_f32", dyd.ptr(), wd.ptr(), wtf.ptr(), dx.ptr(), B, H, W, Cin, Cout, ks, pad)
    torch.cuda.synchronize()
    expect(capfd, "conv_backward_data", kernel)
    r = ratio(dx.cpu(), ref, bound(mag, ks * ks * Cout) + 1e-30)
    print(f"[f32-kernels] conv_backward_data random {kernel}: largest error / bound = {r:.3f}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# conv_backward_filter (bf16 = 0): LoadMN x LoadConvXcol, EP_ATOMIC: dw and dbias accumulate
# ------------------------------------------------------------------------------------------------------------------------------
M32 = {"AOCR_F32W_MINK": "32"}
# (name, B, H, W, Cin, Cout, ks, pad, switches, kernel, split note of gemm_f32w_kernel's line or None)
WGRAD_CASES = [
    ("wo8", 2, 4, 8, 32, 64, 3, 1, {}, F32W, 1),
    ("wo9", 2, 4, 9, 32, 64, 3, 1, {}, F32W, 1),
    ("wo25", 1, 4, 25, 32, 64, 3, 1, {}, F32W, 1),
    ("k2p0", 5, 3, 9, 32, 64, 2, 0, {}, F32W, 1),     # Ho = 2, Wo = 8: row-end and image-end pointer steps non-zero, 16 pixels per image: images wrap inside a 32-k tile
    ("split", 2, 4, 25, 32, 64, 3, 1, M32, F32W, 3),  # P = 200
    ("wo7", 3, 4, 7, 32, 64, 3, 1, {}, BIG, None),
    ("cin6", 2, 4, 9, 6, 64, 3, 1, {}, BIG, None),
    ("cout60", 2, 4, 9, 32, 60, 3, 1, {}, BIG, None),
]


def run_wgrad(x, dy, dw0, db0, ks, pad):
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    xd, dyd, dw, db = Buf(nhwc(x)), Buf(nhwc(dy)), Buf(dw0), Buf(db0)
    call("kp_conv_backward_filter", 0, xd.ptr(), dyd.ptr(), dw.ptr(), db.ptr(), B, H, W, Cin, Cout, ks, pad, None, None, None, 0)
    torch.cuda.synchronize()
    dw.check_tail("dw"); db.check_tail("db")
    return dw, db


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv_backward_filter_exact(case, monkeypatch, capfd):
    name, B, H, W, Cin, Cout, ks, pad, env, kernel, split = case
    setenv(monkeypatch, env)
    Ho, Wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    wide_x = WGRAD_CASES.index(case) % 2 == 0
    x = wide_ints(B, Cin, H, W, seed=2400) if wide_x else ints(B, Cin, H, W, seed=2400)
    dy = ints(B, Cout, Ho, Wo, seed=2401) if wide_x else wide_ints(B, Cout, Ho, Wo, seed=2401)
    P = B * Ho * Wo
    assert_exact_range(P, WIDE, 4, 1000)
    dw0, db0 = ints(Cout, ks, ks, Cin, seed=2402, lo=-1000, hi=1000), ints(Cout, seed=2403, lo=-1000, hi=1000)     # accumulated onto
    ref_dw = dw0.double() + torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, ks, ks), dy.double(), padding=pad).permute(0, 2, 3, 1)
    ref_db = db0.double() + dy.double().sum(dim=(0, 2, 3))
    capfd.readouterr()
    dw, db = run_wgrad(x, dy, dw0, db0, ks, pad)
    lines = trace_of(capfd, "conv_backward_filter")
    want = f": {kernel} {Cout} {ks * ks * Cin} {P}" + (f" {split}" if split else "")
    assert len(lines) == 1 and lines[0].endswith(want), (want, lines)
    eq_bits(dw.cpu(), ref_dw, f"{name}: dw")
    eq_bits(db.cpu(), ref_db, f"{name}: dbias")


@pytest.mark.parametrize("name", ["wo25", "k2p0"])
def test_conv_backward_filter_random(name, monkeypatch, capfd):
    _, B, H, W, Cin, Cout, ks, pad, env, kernel, _ = next(c for c in WGRAD_CASES if c[0] == name)
    Ho, Wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    x, dy = rnd(B, Cin, H, W, seed=2500).float(), rnd(B, Cout, Ho, Wo, seed=2501).float()
    ref = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, ks, ks), dy.double(), padding=pad).permute(0, 2, 3, 1)
    mag = torch.nn.grad.conv2d_weight(x.double().abs(), (Cout, Cin, ks, ks), dy.double().abs(), padding=pad).permute(0, 2, 3, 1)
    capfd.readouterr()
    dw, db = run_wgrad(x, dy, torch.zeros(Cout, ks, ks, Cin), torch.zeros(Cout), ks, pad)
    expect(capfd, "conv_backward_filter", kernel)
    K = B * Ho * Wo
    r = ratio(dw.cpu(), ref, bound(mag, K) + 1e-30)
    print(f"[f32-kernels] conv_backward_filter random {name} {kernel}: largest error / bound = {r:.3f}")
    assert r <= 1.0
    assert ((db.cpu().double() - dy.double().sum(dim=(0, 2, 3))).abs() <= bound(dy.double().abs().sum(dim=(0, 2, 3)), K)).all()
