"""GPU: every bf16-source conv / GEMM kernel branch against an exact reference, called directly through tests/libkprobe.so
(extern "C" wrappers of csrc/ops.h's launchers, given the bf16 shadows the model passes).

Exact-integer operands (the main method): operands and biases are small integers (|v| <= 4), exact in bf16; every product and
partial sum is an integer below 2^20, so fp32 accumulation is exact in ANY order -- across MFMA, split-K slabs, atomics and
splitk_reduce.  The reference is torch on the CPU in fp32 (exact for these data) and the assertions are bit-exact: outputs equal the
reference, bf16 output shadows equal its RNE conversion, the pooling arg-max is the FIRST maximum of its window in EpConv's order
(strict > over i = 0..3 with i = 2 dy + dx, LoadConvK's pooled row mapping; (2,1) windows: i = dy), and accumulating outputs start
from a non-zero buffer.

Random operands (a few cases per function): operand shadows equal torch's RNE, output shadows equal the RNE of the GPU's own fp32
output, and the error against float64 on the bf16-rounded operands stays within BOUND_C * sqrt(K) * 2^-24 * (|A| |B|) per element
(fp32 accumulation of K exact bf16 x bf16 products; tests/tol.py holds the model-level bounds).

Each case asserts the kernel it reached from the AOCR_TRACE dispatch line ("[aocr] <function>: <kernel>[<instantiation>] M N K"),
so a moved threshold cannot silently send a case to another kernel.  Every device buffer has a sentinel-filled tail that must survive.
The helpers the other kernel-level files share with this one (Buf, the operand generators, the trace assertions, the shim's handle) are in
tests/kernel_harness.py."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module (tests/test_kernel_harness_cpu.py checks it)
from kernel_harness import EP_ACCUM, EP_RELU, EP_TANH, SENT, Buf, bf, bits, bound, call, check_exact, expect, ints, kp, nhwc, rnd, setenv, trace_of

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------------
# conv_forward (bf16 shadows xb / wb)
# ------------------------------------------------------------------------------------------------------------------------------
# (name, B, H, W, Cin, Cout, ks, pad, switches, kernel[instantiation])
FWD_CASES = [
    ("halo4_w32", 2, 8, 32, 32, 256, 3, 1, {"AOCR_FORCE_DMA": "1"}, "gemm_halo4_bf16_kernel[fwd]"),
    ("halo4_w64", 2, 4, 64, 32, 256, 3, 1, {"AOCR_FORCE_DMA": "1"}, "gemm_halo4_bf16_kernel[fwd]"),
    ("halo4_w128", 1, 4, 128, 32, 256, 3, 1, {"AOCR_FORCE_DMA": "1"}, "gemm_halo4_bf16_kernel[fwd]"),
    ("halo8_w64", 2, 4, 64, 32, 256, 3, 1, {"AOCR_FORCE_DMA": "1", "AOCR_HALO8": "1"}, "gemm_halo_bf16_kernel[fwd]"),
    ("dma_w40", 1, 8, 40, 32, 256, 3, 1, {"AOCR_FORCE_DMA": "1"}, "gemm_dma_bf16_kernel[]"),
    ("dma_k2p0", 2, 3, 65, 32, 256, 2, 0, {"AOCR_FORCE_DMA": "1"}, "gemm_dma_bf16_kernel[]"),
    ("narrow_c128", 1, 8, 40, 32, 128, 3, 1, {"AOCR_FORCE_DMA": "1"}, "gemm_dma_narrow_kernel[2]"),
    ("narrow_c64", 1, 8, 40, 32, 64, 3, 1, {"AOCR_FORCE_DMA": "1"}, "gemm_dma_narrow_kernel[1]"),
    ("mid_c384", 2, 68, 128, 32, 384, 3, 1, {}, "gemm_dma_narrow_kernel[2]"),
    ("dma128_88", 1, 6, 50, 32, 256, 3, 1, {}, "gemm_dma128_kernel[8,8]"),
    ("dma128_84", 1, 6, 50, 32, 256, 3, 1, {"AOCR_DMA128_W4": "1"}, "gemm_dma128_kernel[8,4]"),
    ("dma128_44", 1, 130, 258, 32, 128, 3, 1, {}, "gemm_dma128_kernel[4,4]"),
    ("lds_cin48", 1, 6, 10, 48, 128, 3, 1, {}, "gemm_lds_bf16_kernel[32]"),
    ("lds_cin16", 2, 4, 9, 16, 128, 3, 1, {}, "gemm_lds_bf16_kernel[32]"),
    ("h1_b1", 1, 1, 300, 32, 256, 3, 1, {}, "gemm_dma128_kernel[8,8]"),
    ("h2_b1", 1, 2, 150, 32, 256, 3, 1, {}, "gemm_dma128_kernel[8,8]"),
]


def conv_operands(B, H, W, Cin, Cout, ks, seed):
    return ints(B, Cin, H, W, seed=seed), ints(Cout, Cin, ks, ks, seed=seed + 1), ints(Cout, seed=seed + 2)


def run_forward(x, w, b, ks, pad, relu, pool, out, bn=None, bn_part=None):
    """x NCHW, w OIHW, b: CPU tensors.  out: "y", "y+yb" or "yb" (the destinations given).  Returns the buffers."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    oshape = (B, Ho, Wo, Cout) if pool == 0 else (B, Ho // 2, Wo // 2, Cout) if pool == 1 else (B, Ho // 2, Wo, Cout)
    xd, wd, bd, xb = Buf(nhwc(x)), Buf(w.permute(0, 2, 3, 1)), Buf(b), Buf(nhwc(x), torch.bfloat16)
    wb, wtb = Buf((Cout, ks, ks, Cin), torch.bfloat16, fill=0), Buf((Cin, ks * ks, Cout), torch.bfloat16, fill=0)
    call("kp_conv_weight_shadows", wd.ptr(), wb.ptr(), wtb.ptr(), Cout, ks * ks, Cin)
    dst = out.split("+")
    y = Buf(oshape, fill=SENT) if "y" in dst else None
    yb = Buf(oshape, torch.bfloat16, fill=0) if "yb" in dst else None
    idx = Buf(oshape, torch.uint8, fill=0x77) if pool else None
    chunks = C.c_int(-1)
    bnp = (None, None, None) if bn is None else tuple(t.ptr() for t in bn)
    call("kp_conv_forward", 1, xd.ptr(), wd.ptr(), bd.ptr(), y.ptr() if y else None, idx.ptr() if idx else None, B, H, W, Cin, Cout, ks, pad,
         relu, pool, xb.ptr(), wb.ptr(), yb.ptr() if yb else None, *bnp,
         C.c_void_p(bn_part.data_ptr()) if bn_part is not None else None, C.byref(chunks) if bn_part is not None else None)
    torch.cuda.synchronize()
    for t, nm in ((y, "y"), (yb, "yb"), (idx, "idx"), (wb, "wb"), (wtb, "wtb")):
        if t is not None:
            t.check_tail(nm)
    return dict(y=y, yb=yb, idx=idx, wb=wb, wtb=wtb, xb=xb, chunks=chunks.value)


@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_conv_forward_exact(case, monkeypatch, capfd):
    name, B, H, W, Cin, Cout, ks, pad, env, kernel = case
    setenv(monkeypatch, env)
    x, w, b = conv_operands(B, H, W, Cin, Cout, ks, seed=11)
    z0 = F.conv2d(x, w, b, padding=pad)                                     # exact (integers, fp32)
    pools = (0, 1, 2) if z0.shape[2] >= 2 else (0,)
    stageds = tuple(str(i) for i in range(8)) if name in ("halo4_w64", "dma_w40") else (None,)     # AOCR_HALO4_STAGED = 0..7
    for staged in stageds:
        if staged is not None:
            monkeypatch.setenv("AOCR_HALO4_STAGED", staged)
        for relu in (0, 1):
            z = F.relu(z0) if relu else z0
            for pool in pools:
                for out in ("y", "y+yb", "yb"):
                    capfd.readouterr()
                    res = run_forward(x, w, b, ks, pad, relu, pool, out)
                    expect(capfd, "conv_forward", kernel)
                    check_exact(res, z, pool, f"{name} staged={staged} relu={relu} pool={pool} out={out}")
    assert torch.equal(bits(res["wb"]), bf(w.permute(0, 2, 3, 1)))
    assert torch.equal(bits(res["wtb"]), bf(w.permute(1, 2, 3, 0).reshape(Cin, ks * ks, Cout)))


@pytest.mark.parametrize("name", ["halo4_w64", "halo8_w64", "dma_w40", "narrow_c128", "mid_c384", "dma128_88", "lds_cin48"])
def test_conv_forward_random(name, monkeypatch, capfd):
    _, B, H, W, Cin, Cout, ks, pad, env, kernel = next(c for c in FWD_CASES if c[0] == name)
    setenv(monkeypatch, env)
    x, w, b = rnd(B, Cin, H, W, seed=3).float(), (rnd(Cout, Cin, ks, ks, seed=4) / (ks * ks * Cin) ** 0.5).float(), (rnd(Cout, seed=5) * 0.1).float()
    xq, wq = x.to(torch.bfloat16).double(), w.to(torch.bfloat16).double()
    ref = nhwc(F.conv2d(xq, wq, b.double(), padding=pad))
    mag = nhwc(F.conv2d(xq.abs(), wq.abs(), None, padding=pad) + b.double().abs().view(1, -1, 1, 1))
    capfd.readouterr()
    res = run_forward(x, w, b, ks, pad, 0, 0, "y+yb")
    expect(capfd, "conv_forward", kernel)
    assert torch.equal(bits(res["xb"]), bf(nhwc(x))) and torch.equal(bits(res["wb"]), bf(w.permute(0, 2, 3, 1)))
    y = res["y"].cpu()
    assert torch.equal(bits(res["yb"]), bf(y)), "yb is not the RNE of the kernel's own fp32 output"
    r = ((y.double() - ref).abs() / (bound(mag, ks * ks * Cin) + 2.0 ** -24 * ref.abs())).max().item()
    print(f"[bf16-kernels] conv_forward {name}: largest error / bound = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("out", ["y", "yb"])
def test_conv_forward_folded_bn_random(out, monkeypatch, capfd):
    """Evaluation-mode BatchNorm + ReLU folded into the epilogue (bn_save from bn_eval_prepare): yb alone takes the staged bf16 tile,
    y the quad epilogue."""
    B, H, W, Cin, Cout = 2, 4, 64, 32, 256
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    x, w, b = rnd(B, Cin, H, W, seed=6).float(), (rnd(Cout, Cin, 3, 3, seed=7) / 17.0).float(), (rnd(Cout, seed=8) * 0.1).float()
    rm, rv = (rnd(Cout, seed=9) * 0.2).float(), (rnd(Cout, seed=10).abs() + 0.5).float()
    bw, bb = (rnd(Cout, seed=12).abs() + 0.2).float(), (rnd(Cout, seed=13) * 0.3).float()
    rmd, rvd, save, bwd, bbd = Buf(rm), Buf(rv), Buf((2 * Cout,), fill=0.0), Buf(bw), Buf(bb)
    call("kp_bn_eval_prepare", rmd.ptr(), rvd.ptr(), save.ptr(), Cout)
    xq, wq = x.to(torch.bfloat16).double(), w.to(torch.bfloat16).double()
    z = F.conv2d(xq, wq, b.double(), padding=1)
    mag = F.conv2d(xq.abs(), wq.abs(), None, padding=1) + b.double().abs().view(1, -1, 1, 1)
    col = lambda t: t.double().view(1, -1, 1, 1)
    scale = col(bw) / torch.sqrt(col(rv) + 1e-5)
    for relu in (0, 1):
        zz = F.relu(z) if relu else z
        ref = F.relu((zz - col(rm)) * scale + col(bb))
        lim = scale.abs() * (bound(mag, 9 * Cin) + 2.0 ** -22 * (zz.abs() + col(rm).abs())) + 2.0 ** -22 * (ref.abs() + col(bb).abs())
        capfd.readouterr()
        res = run_forward(x, w, b, 3, 1, relu, 0, out, bn=(save, bwd, bbd))
        expect(capfd, "conv_forward", "gemm_halo4_bf16_kernel[fwd]")
        ref, lim = nhwc(ref), nhwc(lim)
        if out == "y":
            err = (res["y"].cpu().double() - ref).abs()
        else:
            err = ((res["yb"].cpu().double() - ref).abs() - 2.0 ** -8 * ref.abs()).clamp(min=0)        # + one bf16 rounding
        r = (err / lim).max().item()
        print(f"[bf16-kernels] conv_forward folded BatchNorm relu={relu} out={out}: largest error / bound = {r:.3f}")
        assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# conv_backward_data (dyb / wtb): the same kernel set with SGN = -1 (the loader's channels are Cout, the output columns Cin)
# ------------------------------------------------------------------------------------------------------------------------------
DGRAD_CASES = [
    ("halo4_w32", 2, 8, 32, 256, 32, {"AOCR_FORCE_DMA": "1"}, "gemm_halo4_bf16_kernel[dgrad]"),
    ("halo4_w64", 2, 4, 64, 256, 32, {"AOCR_FORCE_DMA": "1"}, "gemm_halo4_bf16_kernel[dgrad]"),
    ("halo4_w128", 1, 4, 128, 256, 32, {"AOCR_FORCE_DMA": "1"}, "gemm_halo4_bf16_kernel[dgrad]"),
    ("halo8_w64", 2, 4, 64, 256, 32, {"AOCR_FORCE_DMA": "1", "AOCR_HALO8": "1"}, "gemm_halo_bf16_kernel[dgrad]"),
    ("dma_w40", 1, 8, 40, 256, 32, {"AOCR_FORCE_DMA": "1"}, "gemm_dma_bf16_kernel[]"),
    ("dma_w64_nohalo", 2, 4, 64, 256, 32, {"AOCR_FORCE_DMA": "1", "AOCR_NO_HALO": "1"}, "gemm_dma_bf16_kernel[]"),
    ("narrow_c128", 1, 8, 40, 128, 32, {"AOCR_FORCE_DMA": "1"}, "gemm_dma_narrow_kernel[2]"),
    ("narrow_c64", 1, 8, 40, 64, 32, {"AOCR_FORCE_DMA": "1"}, "gemm_dma_narrow_kernel[1]"),
    ("dma128_88", 1, 6, 50, 256, 32, {}, "gemm_dma128_kernel[8,8]"),
    ("dma128_84", 1, 6, 50, 256, 32, {"AOCR_DMA128_W4": "1"}, "gemm_dma128_kernel[8,4]"),
    ("dma128_44", 1, 130, 258, 128, 32, {}, "gemm_dma128_kernel[4,4]"),
    ("lds_cout48", 1, 6, 10, 128, 48, {}, "gemm_lds_bf16_kernel[32]"),
    ("h1_b1", 1, 1, 300, 256, 32, {}, "gemm_dma128_kernel[8,8]"),
]


def run_dgrad(dy, w, B, H, W, dx16=False):
    Cout, Cin = w.shape[0], w.shape[1]
    dyd, dyb, wd = Buf(nhwc(dy)), Buf(nhwc(dy), torch.bfloat16), Buf(w.permute(0, 2, 3, 1))
    wb, wtb = Buf((Cout, 9, Cin), torch.bfloat16, fill=0), Buf((Cin, 9, Cout), torch.bfloat16, fill=0)
    call("kp_conv_weight_shadows", wd.ptr(), wb.ptr(), wtb.ptr(), Cout, 9, Cin)
    dx = Buf((B, H, W, Cin), fill=SENT)
    flag = C.c_int(-1)
    call("kp_conv_backward_data", 1, dyd.ptr(), wd.ptr(), dx.ptr(), B, H, W, Cin, Cout, 3, 1, dyb.ptr(), wtb.ptr(), C.byref(flag) if dx16 else None)
    torch.cuda.synchronize()
    dx.check_tail("dx")
    assert torch.equal(bits(dyb), bf(nhwc(dy)))
    return dx, flag.value


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_conv_backward_data_exact(case, monkeypatch, capfd):
    name, B, H, W, Cin, Cout, env, kernel = case
    setenv(monkeypatch, env)
    w, dy = ints(Cout, Cin, 3, 3, seed=22), ints(B, Cout, H, W, seed=24)
    ref = nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), w, dy, padding=1))
    capfd.readouterr()
    dx, _ = run_dgrad(dy, w, B, H, W)
    expect(capfd, "conv_backward_data", kernel)
    assert torch.equal(dx.cpu(), ref), f"{name}: max diff {(dx.cpu() - ref).abs().max().item()}"


@pytest.mark.parametrize("name", ["halo4_w64", "dma_w64_nohalo"])
def test_conv_backward_data_dx16_exact(name, monkeypatch, capfd):
    """AOCR_DX16=1: the data gradient as bf16 into the first half of the same buffer (staged 256 x 256 tile)."""
    _, B, H, W, Cin, Cout, env, kernel = next(c for c in DGRAD_CASES if c[0] == name)
    setenv(monkeypatch, env)
    monkeypatch.setenv("AOCR_DX16", "1")
    w, dy = ints(Cout, Cin, 3, 3, seed=32), ints(B, Cout, H, W, seed=34)
    ref = nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), w, dy, padding=1))
    capfd.readouterr()
    dx, flag = run_dgrad(dy, w, B, H, W, dx16=True)
    expect(capfd, "conv_backward_data", kernel)
    assert flag == 1, "dx16 path not taken"
    assert torch.equal(dx.full.view(torch.int16)[:dx.n].cpu(), bf(ref).reshape(-1)), name


@pytest.mark.parametrize("name", ["halo4_w64", "narrow_c128", "dma128_88", "lds_cout48"])
def test_conv_backward_data_random(name, monkeypatch, capfd):
    _, B, H, W, Cin, Cout, env, kernel = next(c for c in DGRAD_CASES if c[0] == name)
    setenv(monkeypatch, env)
    w, dy = (rnd(Cout, Cin, 3, 3, seed=41) / 17.0).float(), rnd(B, Cout, H, W, seed=42).float()
    wq, dyq = w.to(torch.bfloat16).double(), dy.to(torch.bfloat16).double()
    ref = nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), wq, dyq, padding=1))
    mag = nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), wq.abs(), dyq.abs(), padding=1))
    capfd.readouterr()
    dx, _ = run_dgrad(dy, w, B, H, W)
    expect(capfd, "conv_backward_data", kernel)
    r = ((dx.cpu().double() - ref).abs() / (bound(mag, 9 * Cout) + 1e-30)).max().item()
    print(f"[bf16-kernels] conv_backward_data {name}: largest error / bound = {r:.3f}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# conv_backward_filter (xb / dyb / part): dw and dbias ACCUMULATE on every path
# ------------------------------------------------------------------------------------------------------------------------------
PART_BIG = 4 << 20
F1 = {"AOCR_FORCE_DMA": "1"}
NOMID = {"AOCR_FORCE_DMA": "1", "AOCR_NO_WGRAD_ISSUE_MID": "1"}
# (name, B, H, W, Cin, Cout, switches, part floats: None = PART_BIG, 0 = no scratch, -1 = one short of the halo kernel's, kernel[instantiation])
WGRAD_CASES = [
    ("halo_w32", 2, 4, 32, 32, 256, F1, None, "conv_wgrad_halo_kernel[256,whole,issue_mid]"),
    ("halo_w64", 2, 4, 64, 32, 256, F1, None, "conv_wgrad_halo_kernel[256,whole,issue_mid]"),
    ("halo_w96", 1, 4, 96, 32, 256, F1, None, "conv_wgrad_halo_kernel[256,whole,issue_mid]"),
    ("halo_w64_nomid", 2, 4, 64, 32, 256, NOMID, None, "conv_wgrad_halo_kernel[256,whole,no_issue_mid]"),
    ("halo_w64_c128", 2, 4, 64, 64, 128, F1, None, "conv_wgrad_halo_kernel[128,whole,issue_mid]"),
    ("halo_w64_c128_nomid", 2, 4, 64, 64, 128, NOMID, None, "conv_wgrad_halo_kernel[128,whole,no_issue_mid]"),
    ("halo_w24", 2, 4, 24, 32, 256, F1, None, "conv_wgrad_halo_kernel[256,ragged,issue_mid]"),
    ("halo_w25", 2, 4, 25, 32, 256, F1, None, "conv_wgrad_halo_kernel[256,ragged,issue_mid]"),
    ("halo_w72", 1, 4, 72, 32, 256, F1, None, "conv_wgrad_halo_kernel[256,ragged,issue_mid]"),
    ("halo_w97", 1, 3, 97, 32, 256, F1, None, "conv_wgrad_halo_kernel[256,ragged,issue_mid]"),
    ("halo_w97_nomid", 1, 3, 97, 32, 256, NOMID, None, "conv_wgrad_halo_kernel[256,ragged,no_issue_mid]"),
    ("halo_w25_c128", 2, 4, 25, 32, 128, F1, None, "conv_wgrad_halo_kernel[128,ragged,issue_mid]"),
    ("halo_w25_c128_nomid", 2, 4, 25, 32, 128, NOMID, None, "conv_wgrad_halo_kernel[128,ragged,no_issue_mid]"),
    ("w33_falls_back", 2, 4, 33, 32, 256, F1, None, "conv_wgrad_dma_kernel[slab]"),
    ("halo_part_short", 2, 4, 64, 32, 256, F1, -1, "conv_wgrad_dma_kernel["),
    ("dma_slab", 2, 4, 64, 32, 256, {"AOCR_FORCE_DMA": "1", "AOCR_NO_WGRAD_HALO": "1"}, None, "conv_wgrad_dma_kernel[slab]"),
    ("dma_atomic", 2, 4, 64, 32, 256, {"AOCR_FORCE_DMA": "1", "AOCR_WGRAD_ATOMIC": "1"}, None, "conv_wgrad_dma_kernel[atomic]"),
    ("tr_slab", 2, 4, 64, 32, 128, {"AOCR_NO_WGRAD_HALO": "1"}, None, "conv_wgrad_tr_kernel[slab]"),
    ("tr_atomic", 2, 4, 64, 32, 128, {"AOCR_WGRAD_ATOMIC": "1"}, None, "conv_wgrad_tr_kernel[atomic]"),
    ("tr_nopart", 1, 6, 50, 48, 64, {}, 0, "conv_wgrad_tr_kernel[atomic]"),
]


def halo_part_floats(B, H, W, Cin, Cout):
    """conv_backward_filter's own k split of the halo kernel (no AOCR_WGRAD_HALO_MINSTEPS): needs Cout * 9 Cin * ksh floats."""
    hmt = 256 if Cout % 256 == 0 else 128
    htiles = (Cin // 32) * (Cout // hmt)
    S = B * H * ((W + 31) // 32)
    ksh = min(1 if htiles >= 256 else 256 // htiles, S)
    per = -(-S // ksh)
    return Cout * 9 * Cin * (-(-S // per))


def run_wgrad(x, dy, dw0, db0, part_n):
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    part = Buf((part_n,), fill=SENT) if part_n else None
    xd, xb, dyd, dyb = Buf(nhwc(x)), Buf(nhwc(x), torch.bfloat16), Buf(nhwc(dy)), Buf(nhwc(dy), torch.bfloat16)
    dw, db = Buf(dw0), Buf(db0)
    call("kp_conv_backward_filter", 1, xd.ptr(), dyd.ptr(), dw.ptr(), db.ptr(), B, H, W, Cin, Cout, 3, 1, xb.ptr(), dyb.ptr(),
         part.ptr() if part else None, part_n)
    torch.cuda.synchronize()
    dw.check_tail("dw"); db.check_tail("db")
    if part:
        part.check_tail("part")
    assert torch.equal(bits(xb), bf(nhwc(x))) and torch.equal(bits(dyb), bf(nhwc(dy)))
    return dw, db


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv_backward_filter_exact(case, monkeypatch, capfd):
    name, B, H, W, Cin, Cout, env, part_n, kernel = case
    setenv(monkeypatch, env)
    x, dy = ints(B, Cin, H, W, seed=51), ints(B, Cout, H, W, seed=52)
    dw0, db0 = ints(Cout, 3, 3, Cin, seed=53, lo=-50, hi=50), ints(Cout, seed=54, lo=-50, hi=50)     # accumulated onto
    ref_dw = dw0 + torch.nn.grad.conv2d_weight(x, (Cout, Cin, 3, 3), dy, padding=1).permute(0, 2, 3, 1)
    ref_db = db0 + dy.sum(dim=(0, 2, 3))
    part_n = PART_BIG if part_n is None else halo_part_floats(B, H, W, Cin, Cout) - 1 if part_n == -1 else part_n
    capfd.readouterr()
    dw, db = run_wgrad(x, dy, dw0, db0, part_n)
    expect(capfd, "conv_backward_filter", kernel)
    assert torch.equal(dw.cpu(), ref_dw), f"{name}: dw (max diff {(dw.cpu() - ref_dw).abs().max().item()})"
    assert torch.equal(db.cpu(), ref_db), f"{name}: dbias"


@pytest.mark.parametrize("name", ["halo_w64", "halo_w25", "dma_slab", "tr_slab"])
def test_conv_backward_filter_random(name, monkeypatch, capfd):
    _, B, H, W, Cin, Cout, env, _, kernel = next(c for c in WGRAD_CASES if c[0] == name)
    setenv(monkeypatch, env)
    x, dy = rnd(B, Cin, H, W, seed=61).float(), rnd(B, Cout, H, W, seed=62).float()
    xq, dyq = x.to(torch.bfloat16).double(), dy.to(torch.bfloat16).double()
    ref = torch.nn.grad.conv2d_weight(xq, (Cout, Cin, 3, 3), dyq, padding=1).permute(0, 2, 3, 1)
    mag = torch.nn.grad.conv2d_weight(xq.abs(), (Cout, Cin, 3, 3), dyq.abs(), padding=1).permute(0, 2, 3, 1)
    capfd.readouterr()
    dw, db = run_wgrad(x, dy, torch.zeros(Cout, 3, 3, Cin), torch.zeros(Cout), PART_BIG)
    expect(capfd, "conv_backward_filter", kernel)
    K = B * H * W
    r = ((dw.cpu().double() - ref).abs() / (bound(mag, K) + 1e-30)).max().item()
    print(f"[bf16-kernels] conv_backward_filter {name}: largest error / bound = {r:.3f}")
    assert r <= 1.0
    dbr = dy.double().sum(dim=(0, 2, 3))                       # the bias gradient reads the fp32 d y
    assert ((db.cpu().double() - dbr).abs() <= bound(dy.double().abs().sum(dim=(0, 2, 3)), K)).all()


def test_splitk_reduce_exact():
    ks, n = 5, 4096
    part, out = Buf(ints(ks, n, seed=71)), Buf(ints(n, seed=72, lo=-100, hi=100))
    ref = out.cpu() + part.cpu().sum(0)
    call("kp_splitk_reduce", part.ptr(), ks, n, out.ptr())
    torch.cuda.synchronize()
    out.check_tail("out")
    assert torch.equal(out.cpu(), ref)


# ------------------------------------------------------------------------------------------------------------------------------
# gemm_hh / gemm_hh_shadow / gemm_hh_cat: C = A B^T (+ bias + bias2, flags); A [M][K], B [N][K] bf16
# ------------------------------------------------------------------------------------------------------------------------------
HH_CASES = [
    ("narrow_full", 25600, 256, 64, {}, "gemm_dma_narrow_kernel[2]"),
    ("narrow_ragged", 25500, 256, 64, {}, "gemm_dma_narrow_kernel[2]"),
    ("narrow_full_only", 25500, 256, 64, {"AOCR_HH_NARROW_FULL_ONLY": "1"}, "gemm_dma128_kernel[4,4]"),
    ("dma128_44", 33000, 128, 64, {}, "gemm_dma128_kernel[4,4]"),
    ("dma128_88", 300, 256, 96, {}, "gemm_dma128_kernel[8,8]"),
    ("dma128_84", 300, 256, 96, {"AOCR_DMA128_W4": "1"}, "gemm_dma128_kernel[8,4]"),
    ("lds_n100", 300, 100, 64, {}, "gemm_lds_bf16_kernel[32]"),
    ("lds_k48", 200, 128, 48, {}, "gemm_lds_bf16_kernel[32]"),
]


@pytest.mark.parametrize("case", HH_CASES, ids=[c[0] for c in HH_CASES])
def test_gemm_hh_exact(case, monkeypatch, capfd):
    name, M, N, K, env, kernel = case
    setenv(monkeypatch, env)
    A, Bm = ints(M, K, seed=81), ints(N, K, seed=82)
    Ab, Bb = Buf(A, torch.bfloat16), Buf(Bm, torch.bfloat16)
    prod = A @ Bm.t()
    bias, bias2 = ints(N, seed=83), ints(N, seed=84)
    bd, bd2 = Buf(bias), Buf(bias2)
    C0 = ints(M, N, seed=85, lo=-30, hi=30)
    for flags in (0, EP_RELU, EP_ACCUM, EP_RELU | EP_ACCUM, EP_TANH):
        for nb in (0, 1, 2):
            ref = prod + (bias if nb >= 1 else 0) + (bias2 if nb == 2 else 0)
            if flags & EP_RELU:
                ref = ref.clamp(min=0)
            if flags & EP_TANH:
                ref = torch.tanh(ref.double())
            if flags & EP_ACCUM:
                ref = C0 + ref
            Cd = Buf(C0) if flags & EP_ACCUM else Buf((M, N), fill=SENT)
            capfd.readouterr()
            call("kp_gemm_hh", Ab.ptr(), K, Bb.ptr(), K, Cd.ptr(), N, M, N, K, bd.ptr() if nb >= 1 else None, bd2.ptr() if nb == 2 else None, flags)
            torch.cuda.synchronize()
            expect(capfd, "gemm_hh", kernel)
            Cd.check_tail("C")
            if flags & EP_TANH:                                      # the kernel's own tanh: not exact
                e = (Cd.cpu().double() - ref).abs().max().item()
                assert e <= 1e-5, (name, flags, nb, e)
            else:
                assert torch.equal(Cd.cpu(), ref), (name, flags, nb, (Cd.cpu() - ref).abs().max().item())


SHADOW_CASES = [c for c in HH_CASES if c[0] in ("narrow_full", "narrow_ragged", "dma128_88", "lds_n100")]


@pytest.mark.parametrize("case", SHADOW_CASES, ids=[c[0] for c in SHADOW_CASES])
@pytest.mark.parametrize("staged", ["1", "0"])
def test_gemm_hh_shadow_exact(case, staged, monkeypatch, capfd):
    """Cb is always written.  C only where the code writes it: the staged narrow path leaves C untouched on purpose (every reader takes
    Cb); AOCR_NO_NARROW_STAGED=1 and the other kernels write both."""
    name, M, N, K, env, kernel = case
    setenv(monkeypatch, env)
    if staged == "0":
        monkeypatch.setenv("AOCR_NO_NARROW_STAGED", "1")
    A, Bm = ints(M, K, seed=91), ints(N, K, seed=92)
    ref = A @ Bm.t()
    Ab, Bb, Cd, Cb = Buf(A, torch.bfloat16), Buf(Bm, torch.bfloat16), Buf((M, N), fill=SENT), Buf((M, N), torch.bfloat16, fill=0)
    capfd.readouterr()
    call("kp_gemm_hh_shadow", Ab.ptr(), K, Bb.ptr(), K, Cd.ptr(), N, Cb.ptr(), N, M, N, K)
    torch.cuda.synchronize()
    expect(capfd, "gemm_hh_shadow", kernel)
    Cd.check_tail("C"); Cb.check_tail("Cb")
    assert torch.equal(bits(Cb), bf(ref)), name
    if kernel.startswith("gemm_dma_narrow_kernel") and staged == "1":
        assert torch.equal(Cd.cpu(), torch.full((M, N), SENT)), "the staged narrow path must leave C untouched"
    else:
        assert torch.equal(Cd.cpu(), ref), name


@pytest.mark.parametrize("M", [25600, 25500])
def test_gemm_hh_cat_exact(M, monkeypatch, capfd):
    N, K0, K1 = 256, 64, 96
    A0, B0, A1, B1 = ints(M, K0, seed=101), ints(N, K0, seed=102), ints(M, K1, seed=103), ints(N, K1, seed=104)
    ref = A0 @ B0.t() + A1 @ B1.t()
    # both halves share one leading dimension (K1): A0 / B0 live in the first K0 columns of K1-wide rows
    a0, a1 = Buf(torch.cat([A0, ints(M, K1 - K0, seed=105)], 1), torch.bfloat16), Buf(A1, torch.bfloat16)
    b0, b1 = Buf(torch.cat([B0, ints(N, K1 - K0, seed=106)], 1), torch.bfloat16), Buf(B1, torch.bfloat16)
    Cd = Buf((M, N), fill=SENT)
    taken = C.c_int(-1)
    capfd.readouterr()
    call("kp_gemm_hh_cat", a0.ptr(), a1.ptr(), K1, b0.ptr(), b1.ptr(), K1, Cd.ptr(), N, M, N, K0, K1, C.byref(taken))
    torch.cuda.synchronize()
    assert taken.value == 1
    expect(capfd, "gemm_hh_cat", "gemm_dma_narrow_kernel[2]")
    Cd.check_tail("C")
    assert torch.equal(Cd.cpu(), ref)
    monkeypatch.setenv("AOCR_NO_HH_CAT", "1")
    call("kp_gemm_hh_cat", a0.ptr(), a1.ptr(), K1, b0.ptr(), b1.ptr(), K1, Cd.ptr(), N, M, N, K0, K1, C.byref(taken))
    assert taken.value == 0


@pytest.mark.parametrize("name", ["narrow_full", "dma128_44", "lds_n100"])
def test_gemm_hh_random(name, monkeypatch, capfd):
    _, M, N, K, env, kernel = next(c for c in HH_CASES if c[0] == name)
    setenv(monkeypatch, env)
    monkeypatch.setenv("AOCR_NO_NARROW_STAGED", "1")               # C written on every path
    A, Bm = rnd(M, K, seed=111).float(), rnd(N, K, seed=112).float()
    Aq, Bq = A.to(torch.bfloat16).double(), Bm.to(torch.bfloat16).double()
    ref, mag = Aq @ Bq.t(), Aq.abs() @ Bq.abs().t()
    Ab, Bb = Buf(A, torch.bfloat16), Buf(Bm, torch.bfloat16)
    Cd, Cb = Buf((M, N), fill=SENT), Buf((M, N), torch.bfloat16, fill=0)
    capfd.readouterr()
    call("kp_gemm_hh_shadow", Ab.ptr(), K, Bb.ptr(), K, Cd.ptr(), N, Cb.ptr(), N, M, N, K)
    torch.cuda.synchronize()
    expect(capfd, "gemm_hh_shadow", kernel)
    got = Cd.cpu()
    assert torch.equal(bits(Cb), bf(got)), "Cb is not the RNE of the kernel's own fp32 output"
    r = ((got.double() - ref).abs() / (bound(mag, K) + 1e-30)).max().item()
    print(f"[bf16-kernels] gemm_hh_shadow {name}: largest error / bound = {r:.3f}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# grouped_wgrad (bf16): C_i [M_i][N_i] += A_i^T B_i with A_i [K_i][M_i], B_i [K_i][N_i]
# ------------------------------------------------------------------------------------------------------------------------------
DEEP, SHALLOW, PLAIN = (256, 256, 2048, True), (128, 64, 100, True), (96, 40, 77, False)     # (M, N, K, bf16 shadows given)


def run_grouped(problems, part_floats, capfd):
    n = len(problems)
    keep, cols = [], {k: [] for k in ("A", "lda", "B", "ldb", "C", "ldc", "M", "N", "K", "Ab", "Bb")}
    refs = []
    for i, (M, N, K, sh) in enumerate(problems):
        a, b, c0 = ints(K, M, seed=200 + 3 * i), ints(K, N, seed=201 + 3 * i), ints(M, N, seed=202 + 3 * i, lo=-40, hi=40)
        ad, bd, cd = Buf(a), Buf(b), Buf(c0)
        abd, bbd = (Buf(a, torch.bfloat16), Buf(b, torch.bfloat16)) if sh else (None, None)
        keep += [ad, bd, cd, abd, bbd]
        for k, v in (("A", ad.full.data_ptr()), ("B", bd.full.data_ptr()), ("C", cd.full.data_ptr()), ("lda", M), ("ldb", N), ("ldc", N),
                     ("M", M), ("N", N), ("K", K), ("Ab", abd.full.data_ptr() if sh else None), ("Bb", bbd.full.data_ptr() if sh else None)):
            cols[k].append(v)
        refs.append((cd, c0 + a.t() @ b))
    part = Buf((part_floats,), fill=SENT) if part_floats else None
    P, L, I = (lambda k: (C.c_void_p * n)(*cols[k])), (lambda k: (C.c_int64 * n)(*cols[k])), (lambda k: (C.c_int * n)(*cols[k]))
    capfd.readouterr()
    call("kp_grouped_wgrad", 1, n, P("A"), L("lda"), P("B"), L("ldb"), P("C"), L("ldc"), I("M"), I("N"), I("K"), P("Ab"), P("Bb"),
         part.ptr() if part else None, part_floats)
    torch.cuda.synchronize()
    lines = trace_of(capfd, "grouped_wgrad")
    for i, (cd, ref) in enumerate(refs):
        cd.check_tail(f"C{i}")
        assert torch.equal(cd.cpu(), ref), f"problem {i} {problems[i]}: max diff {(cd.cpu() - ref).abs().max().item()}"
    if part:
        part.check_tail("part")
    return lines


@pytest.mark.parametrize("name,problems,part,expected", [
    ("deep", [DEEP], 8 << 20, ["wgrad_dma_grouped_kernel"]),
    ("shallow_shadowed", [SHALLOW], 8 << 20, ["wgrad_tr_grouped_kernel"]),
    ("unshadowed", [PLAIN], 8 << 20, ["gemm_lds_grouped_kernel"]),
    ("mix", [DEEP, SHALLOW, PLAIN, (512, 256, 2080, True)], 8 << 20,
     ["wgrad_dma_grouped_kernel", "wgrad_tr_grouped_kernel", "gemm_lds_grouped_kernel", "wgrad_dma_grouped_kernel"]),
    ("ten_problems", [(64 + 8 * i, 32 + 8 * i, 40 + 3 * i, i != 4) for i in range(10)], 8 << 20,
     ["gemm_lds_grouped_kernel" if i == 4 else "wgrad_tr_grouped_kernel" for i in range(10)]),
    ("part_too_small", [DEEP, SHALLOW], 65536 - 1, ["wgrad_tr_grouped_kernel", "wgrad_tr_grouped_kernel"]),
    ("no_part", [DEEP], 0, ["wgrad_tr_grouped_kernel"]),
])
def test_grouped_wgrad_exact(name, problems, part, expected, capfd):
    lines = run_grouped(problems, part, capfd)
    got = sorted((tuple(int(v) for v in ln.split()[-3:]), ln.split(": ", 1)[1].split("[")[0]) for ln in lines)
    want = sorted((p[:3], k) for p, k in zip(problems, expected))
    assert got == want, (name, lines)


# ------------------------------------------------------------------------------------------------------------------------------
# fused BatchNorm statistics: conv_forward's epilogue leaves the partial sums, bn_relu_forward(stats_chunks = n) reads them
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env,kernel", [("halo4", {}, "gemm_halo4_bf16_kernel[fwd]"), ("dma", {"AOCR_NO_HALO": "1"}, "gemm_dma_bf16_kernel[]")])
def test_conv_forward_bn_stats_fused(name, env, kernel, monkeypatch, capfd):
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    setenv(monkeypatch, env)
    B, H, W, Cin, Cout = 2, 4, 64, 32, 256
    x, w, b = conv_operands(B, H, W, Cin, Cout, 3, seed=131)
    z = nhwc(F.conv2d(x, w, b, padding=1)).reshape(-1, Cout).double()           # exact
    rows = z.shape[0]
    scratch = torch.zeros(kp().kp_bn_scratch_bytes(Cout) // 8 + 8, dtype=torch.float64, device="cuda")
    capfd.readouterr()
    res = run_forward(x, w, b, 3, 1, 0, 0, "y", bn_part=scratch)
    expect(capfd, "conv_forward", kernel)
    assert res["chunks"] == rows // 256 and res["chunks"] > 0, f"fused statistics not taken (*bn_chunks = {res['chunks']})"
    assert torch.equal(res["y"].cpu().double().reshape(rows, Cout), z)
    bw, bb = (rnd(Cout, seed=132).abs() + 0.2).float(), (rnd(Cout, seed=133) * 0.3).float()
    rm0, rv0 = (rnd(Cout, seed=134) * 0.1).float(), (rnd(Cout, seed=135).abs() + 0.5).float()
    out, rmd, rvd, save, bwd, bbd = Buf((rows, Cout), fill=SENT), Buf(rm0), Buf(rv0), Buf((2 * Cout,), fill=0.0), Buf(bw), Buf(bb)
    call("kp_bn_relu_forward", res["y"].ptr(), out.ptr(), bwd.ptr(), bbd.ptr(), rmd.ptr(), rvd.ptr(), save.ptr(), C.c_void_p(scratch.data_ptr()),
         rows, Cout, 1, 1, res["chunks"])
    torch.cuda.synchronize()
    out.check_tail("y")
    mean, var = z.mean(0), z.var(0, unbiased=False)
    inv = 1.0 / torch.sqrt(var + 1e-5)
    ref = F.relu((z - mean) * inv * bw.double() + bb.double())
    e = (out.cpu().double() - ref).abs().max().item()
    print(f"[bf16-kernels] fused BatchNorm statistics ({name}): max-abs error {e:.2e}")
    assert e <= 2e-5 * max(1.0, ref.abs().max().item())
    sv = save.cpu().double()
    assert ((sv[:Cout] - mean).abs() <= 1e-6 * mean.abs().clamp(min=1)).all(), "saved mean"
    assert ((sv[Cout:] - inv).abs() <= 1e-5 * inv).all(), "saved inverse std"
    rm_ref = 0.9 * rm0.double() + 0.1 * mean
    rv_ref = 0.9 * rv0.double() + 0.1 * z.var(0, unbiased=True)
    assert ((rmd.cpu().double() - rm_ref).abs() <= 1e-5 * rm_ref.abs().clamp(min=1)).all(), "running mean"
    assert ((rvd.cpu().double() - rv_ref).abs() <= 1e-5 * rv_ref.abs().clamp(min=1)).all(), "running var"
