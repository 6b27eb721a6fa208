"""GPU: every BatchNorm, un-pool, conv1 and column-sum kernel variant (csrc/ops_misc.hip) against a float64 / exact-integer reference
(tests/cnn_elementwise_ref.py), called directly through tests/libkprobe.so with the optional arguments the bf16 train step passes.
Helpers and fixture of tests/kernel_harness.py: every device buffer has a sentinel tail that must survive, partial slabs and
scratch are allocated at exactly the size csrc/ops.h documents, accumulating outputs start from non-zero integers, and every case
asserts the AOCR_TRACE line(s) of the launch decision it reached.

Exact data (most cases, bit-exact assertions).
  conv1: pixels 0..255 normalise to multiples of 2^-7, weights are integers in [-2, 2], the bias an integer: every conv value is exact,
    ties and exact zeros are frequent and pin the routing rule (first strict maximum above the ReLU floor, order (0,0),(0,1),(1,0),
    (1,1); exactly 0 routes nothing).  d(pooled) integers in [-4, 4]: every dw / db partial is a multiple of 2^-7 and the test asserts
    sum |term| < 2^17 per channel, so the sums are exact through atomics, slabs and column sums in any order.
  un-pool: pure selection; integer gradients make the bias sums exact.
  BatchNorm: integer x gives exact fp64 sums, so save / running statistics are the float64 formula to 1 fp32 ulp and db is exact; the ReLU
    mask is the y / yb the test supplies.
Handed-over decisions are made to differ from what the launcher would compute itself: stats_chunks / sums_chunks hold the sums of ANOTHER map, xh / dAh
  / dpooled16 come with a decoy fp32 map, and the routed conv1 backward also gets a route the test makes up -- the values, not only the trace, show what was read.
Random operands (a few cases per family) keep the rounding honest: bf16 shadows must be the RNE of the fp32 value, fp32 sums stay within one rounding per addition.
Non-exact values are compared with float64 evaluated on the device's own `save`, per element, within c * 2^-24 * (sum of the magnitudes
of the terms), c = fp32 roundings on the value's path + 1, derived at the constants below.

measured on MI355X (largest error / bound per test function over its cases; the bf16-only outputs reach 1 because the bound is then half a bf16 ulp):
  test_bn_forward: y 0.41  yb-only 1
  test_bn_backward: dw 0.21  dx 0.27  conv_dbias 0.021  dxb-only 1
  test_bn_random: y 0.41  yb-only 0.99  dw 0.13  dx 0.26  conv_dbias 0.0062  dxb-only 0.99
  test_conv1_random: y 0.42  dw 0.0023  db 0.0015
  test_unpool_random: dbias 0.13
  test_colsum_random: accum 0.054  jobs 0.054
"""
import ctypes as C

import pytest
import torch

import cnn_elementwise_ref as R
from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module (tests/test_kernel_harness_cpu.py checks it)
from kernel_harness import SENT, Buf, bf, bits, call, expect, i32, i64, ints, kp, rnd, setenv, trace_of, vp

pytestmark = pytest.mark.gpu
U = R.U

# ---- bounds: c = fp32 roundings + 1, from the kernels' expressions
# bn_apply_relu_kernel: (x - m) [1] * iv [1] * w [1] + b [1]                                            -> 4 roundings
C_Y = 5
# bn_bwd_apply_kernel: gx = (d - (float)fin0 [1] - xh * (float)fin1) * inv * w with xh = (x - m) [1] * inv [1], (float)fin1 [1] whose fp64
# sum holds fp32 xhat terms [2, against mean |d xhat|], the product [1], two subtractions [2], * inv [1], * w [1]  -> 11 roundings
C_DX = 12
# dw: sum in fp64 of d * fp32((x - m) * inv) [2 per term], then (float)ss [1] and dw += [1], both against sum |term| + |dw0|   -> 4 roundings
C_DW = 5
# conv_dbias: fp32 sum of `rows` values of gx per channel in some order: the per-term error C_DX plus at most one rounding per addition,
# each against sum |gx| (thread partial, LDS tree, column sum, atomics: fewer than `rows` additions on any path)      -> C_DX + rows
# conv1 forward: bias + nine FMAs                                                                        -> 9 roundings
C_CONV = 10
BF = 2.0 ** -8                      # RNE to bf16 (8 significant bits): half an ulp is at most 2^-8 of the value


def P(b):
    return b.ptr() if b is not None else None


def lines(capfd, fn, kernels):
    """the trace lines of one launch of `fn`, in order: exactly these kernels"""
    got = trace_of(capfd, fn)
    assert len(got) == len(kernels) and all(f": {k} " in ln for k, ln in zip(kernels, got)), (fn, kernels, got)


def tails(what, **bufs):
    for nm, b in bufs.items():
        if b is not None:
            b.check_tail(f"{what}: {nm}")


def within(what, got, ref, bound, worst, key):
    ratio = ((got.double() - ref).abs() / bound.clamp(min=1e-300)).max().item() if ref.numel() else 0.0
    worst[key] = max(worst.get(key, 0.0), ratio)
    assert ratio <= 1.0, f"{what}: {key} error / bound = {ratio:.3g}"


def report(name, worst):
    print(f"{name}: " + "  ".join(f"{k} {v:.2g}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------------------
# conv1
# ------------------------------------------------------------------------------------------------------------------------------
def conv1_scratch_floats(B, H, W):                                   # csrc/ops.h: min(ceil(strips / 4), 2048) * 640, strips = B (H/2) ceil((W/2) / 32)
    strips = B * (H // 2) * ((W // 2 + 31) // 32)
    return min((strips + 3) // 4, 2048) * 640


def decode_route(words, B, H, W):
    """route words (four 4-bit codes per word, one word per channel and four consecutive windows of a 32-window strip) -> (B,Hp,Wp,64) in -1..3"""
    Hp, Wp = H // 2, W // 2
    spr = (Wp + 31) // 32
    w = (words.cpu().to(torch.int32) & 0xFFFF).view(B, Hp, spr, 8, 1, 64)
    codes = torch.cat([(w >> (4 * u)) & 15 for u in range(4)], dim=4)              # (B,Hp,spr,8,4,64): window = 32 sp + 4 word + u
    return codes.reshape(B, Hp, spr * 32, 64)[:, :, :Wp].to(torch.int64) - 1


def encode_route(r, B, H, W):
    """the inverse of decode_route: (B,Hp,Wp,64) decisions in -1..3 -> a route buffer"""
    Hp, Wp = H // 2, W // 2
    spr = (Wp + 31) // 32
    codes = torch.zeros(B, Hp, spr * 32, 64, dtype=torch.int32)
    codes[:, :, :Wp] = (r + 1).to(torch.int32)
    codes = codes.view(B, Hp, spr, 8, 4, 64)
    words = sum(codes[:, :, :, :, u] << (4 * u) for u in range(4))
    return Buf(words.reshape(-1), torch.int16)


def conv1_fwd(xd, wd, bd, B, H, W, out, with_route, capfd, what):
    Hp, Wp = H // 2, W // 2
    dst = out.split("+")
    y = Buf((B, Hp, Wp, 64), fill=SENT) if "y" in dst else None
    yb = Buf((B, Hp, Wp, 64), torch.bfloat16, fill=0) if "yb" in dst else None
    route = Buf((kp().kp_conv1_route_elems(B, H, W),), torch.int16, fill=0x7777) if with_route else None
    capfd.readouterr()
    call("kp_conv1_forward", xd.ptr(), wd.ptr(), bd.ptr(), P(y), B, H, W, P(yb), P(route))
    torch.cuda.synchronize()
    expect(capfd, "conv1_forward", f"conv1_fwd_kernel[{int(with_route)}]")
    tails(what, y=y, yb=yb, route=route)
    return y, yb, route


def conv1_bwd(xd, wd, bd, gd, dw0, db0, B, H, W, kernel, finish, route, monkeypatch, capfd, what):
    if kernel == "scalar":
        monkeypatch.setenv("AOCR_CONV1_SCALAR", "1")
    else:
        monkeypatch.delenv("AOCR_CONV1_SCALAR", raising=False)
    dw, db = Buf(dw0), Buf(db0)
    scratch = Buf((conv1_scratch_floats(B, H, W),), fill=SENT) if finish != "atomic" else None
    capfd.readouterr()
    call("kp_conv1_backward", xd.ptr(), wd.ptr(), bd.ptr(), gd.ptr(), dw.ptr(), db.ptr(), B, H, W, P(scratch), int(finish == "defer"),
         P(route) if kernel == "routed" else None)
    torch.cuda.synchronize()
    expect(capfd, "conv1_backward", {"scalar": "conv1_bwd_kernel[]", "packed": "conv1_bwd_pk_kernel[0]", "routed": "conv1_bwd_pk_kernel[1]"}[kernel])
    tails(what, dw=dw, db=db, scratch=scratch)
    return dw.cpu(), db.cpu()


# (name, B, H, W): Wp = 3, 32, 33 (a second strip with one window), 50 (Wp % 4 != 0); odd W (the last column is a real tap), odd H;
# strips / 4 above the grid caps: 1024 workgroups without scratch (4400 strips), 2048 with scratch (8400), 4096 forward (16800: forward only)
CONV1_CASES = [("wp3", 2, 4, 6), ("wp32", 1, 6, 64), ("wp33", 2, 4, 66), ("wp50", 1, 4, 100), ("odd_w", 2, 6, 67), ("odd_h", 2, 7, 13),
               ("wrap1024", 1100, 8, 6), ("wrap2048", 2100, 8, 6), ("wrap4096_fwd", 4200, 8, 6)]


def conv1_exact_operands(B, H, W):
    x = ints(B, H, W, seed=5, lo=0, hi=255)
    # a flat mid-grey corner (normalised 0, like the padding): every conv value of its windows is the bias -- an exact zero or a four-way tie
    x[:, :H // 2 + 1, :max(4, W // 4)] = 128.0
    return x, ints(64, 3, 3, seed=6, lo=-2, hi=2), ints(64, seed=7, lo=-1, hi=1)


@pytest.mark.parametrize("case", CONV1_CASES, ids=[c[0] for c in CONV1_CASES])
def test_conv1_exact(case, monkeypatch, capfd):
    name, B, H, W = case
    x, w, b = conv1_exact_operands(B, H, W)
    v, _, xn = R.conv1_windows(x, w, b)
    rref, yref = R.conv1_route(v)
    assert (rref == -1).any() and (v.max(-1).values == 0).any(), "the case has no window at the ReLU floor"
    sv = v.sort(dim=-1, descending=True).values
    assert ((sv[..., 0] == sv[..., 1]) & (sv[..., 0] > 0)).any(), "the case has no tie above the ReLU floor"
    xd, wd, bd = Buf(x), Buf(w), Buf(b)
    route = None
    for out in ("y", "y+yb", "yb"):
        for with_route in (False, True):
            what = f"{name} forward {out} route={with_route}"
            y, yb, rt = conv1_fwd(xd, wd, bd, B, H, W, out, with_route, capfd, what)
            if y is not None:
                assert torch.equal(y.cpu(), yref.float()), what + ": y"
            if yb is not None:
                assert torch.equal(bits(yb), bf(yref)), what + ": yb"
            if rt is not None:
                bad = decode_route(rt.t, B, H, W) != rref
                assert not bad.any(), f"{what}: {bad.sum().item()} of {bad.numel()} route codes differ from the first strict maximum above 0"
                route = rt
    if name.endswith("_fwd"):
        return
    g = ints(B, H // 2, W // 2, 64, seed=8)
    dwr, dbr, _, gsum = R.conv1_grads(xn, rref, g)
    dw0, db0 = ints(64, 9, seed=9, lo=1, hi=4), ints(64, seed=10, lo=1, hi=4)
    assert gsum.max().item() + 4 < 2 ** 17, "sum |term| must stay below 2^17 for multiples of 2^-7 to add exactly in fp32"
    gd = Buf(g)
    # "foreign": a route the test makes up (any of nothing / the four positions per window), NOT what re-evaluation decides -- the routed kernel must follow it
    rfor = ints(B, H // 2, W // 2, 64, seed=12, lo=-1, hi=3).long()
    assert (rfor != rref).float().mean().item() > 0.5
    assert (decode_route(encode_route(rref, B, H, W).t, B, H, W) == rref).all()
    dwf, dbf, _, gsumf = R.conv1_grads(xn, rfor, g)
    assert gsumf.max().item() + 4 < 2 ** 17
    foreign = encode_route(rfor, B, H, W)
    for kernel in ("scalar", "packed", "routed", "foreign"):
        for finish in ("atomic", "scratch", "defer"):
            what = f"{name} backward {kernel} {finish}"
            dw, db = conv1_bwd(xd, wd, bd, gd, dw0, db0, B, H, W, "routed" if kernel == "foreign" else kernel, finish, foreign if kernel == "foreign" else route,
                               monkeypatch, capfd, what)
            edw, edb = (dwf, dbf) if kernel == "foreign" else (dwr, dbr)
            assert torch.equal(dw.double(), dw0.double() + edw), f"{what}: dw (max diff {(dw.double() - dw0.double() - edw).abs().max().item()})"
            assert torch.equal(db.double(), db0.double() + edb), f"{what}: db"
            if kernel == "foreign":
                foreign.check_tail(what + ": route")


CONV1_RANDOM = [("wp33", 2, 8, 66, 31), ("wrap2048", 2100, 8, 6, 32)]


def conv1_random_operands(B, H, W, seed):
    """the first seed (from `seed` up) whose float64 reference has at most 0.1 % of windows with its two largest values closer than 2^-18"""
    for sd in range(seed, seed + 20):
        x = ints(B, H, W, seed=sd, lo=0, hi=255)
        w, b = rnd(64, 3, 3, seed=sd + 100).float(), (rnd(64, seed=sd + 200) * 0.5).float()
        v, a, xn = R.conv1_windows(x, w, b)
        top = torch.cat([v, torch.zeros_like(v[..., :1])], dim=-1).sort(dim=-1, descending=True).values     # the ReLU floor competes too
        near = (top[..., 0] - top[..., 1]) < 2.0 ** -18
        if near.float().mean().item() <= 1e-3:
            return x, w, b, v, a, xn, near
    raise AssertionError("no seed within the near-tie cap")


@pytest.mark.parametrize("case", CONV1_RANDOM, ids=[c[0] for c in CONV1_RANDOM])
def test_conv1_random(case, monkeypatch, capfd):
    name, B, H, W, seed = case
    worst = {}
    x, w, b, v, a, xn, near = conv1_random_operands(B, H, W, seed)
    rref, yref = R.conv1_route(v)
    xd, wd, bd = Buf(x), Buf(w), Buf(b)
    y, yb, rt = conv1_fwd(xd, wd, bd, B, H, W, "y+yb", True, capfd, name)
    within(name, y.cpu(), yref, C_CONV * U * a.max(dim=-1).values, worst, "y")
    assert torch.equal(bits(yb), bf(y.cpu())), name + ": yb is not the RNE of the device's y"
    rdev = decode_route(rt.t, B, H, W)
    bad = (rdev != rref) & ~near
    assert not bad.any(), f"{name}: {bad.sum().item()} route codes differ from float64 outside near-ties"
    g = rnd(B, H // 2, W // 2, 64, seed=seed + 1).float()
    dwr, dbr, mag, gsum = R.conv1_grads(xn, rdev, g)                                # routed as the DEVICE decided
    dw0, db0 = ints(64, 9, seed=9, lo=1, hi=4), ints(64, seed=10, lo=1, hi=4)
    n = B * (H // 2) * (W // 2)                                                      # fp32 sums of n terms: at most one rounding per addition, against sum |term|
    gd = Buf(g)
    for kernel, finish in (("scalar", "atomic"), ("packed", "scratch"), ("routed", "defer")):
        what = f"{name} backward {kernel} {finish}"
        dw, db = conv1_bwd(xd, wd, bd, gd, dw0, db0, B, H, W, kernel, finish, rt, monkeypatch, capfd, what)
        within(what, dw, dw0.double() + dwr, (n + 1) * U * (mag + dw0.double()), worst, "dw")
        within(what, db, db0.double() + dbr, (n + 1) * U * (gsum + db0.double()), worst, "db")
    print(f"test_conv1_random[{name}]: {near.sum().item()} of {near.numel()} windows left out of the route check (near-ties < 2^-18)")
    report(f"test_conv1_random[{name}]", worst)


# ------------------------------------------------------------------------------------------------------------------------------
# un-pool + ReLU backward
# ------------------------------------------------------------------------------------------------------------------------------
# (name, B, Ho, Wo, C, pool): pool 1 = (2,2), 2 = (2,1); odd Ho / Wo leave a zero row / column; C = 96: 256 % (C/4) != 0 (the plain kernel even
# with a slab); C = 1024: C/4 = 256; big: 8300 windows x 64 eight-channel items > 2048 * 256 (the grid-stride loop repeats)
UNPOOL_CASES = [("c8_p22", 2, 4, 6, 8, 1), ("c64_p22_odd", 1, 5, 7, 64, 1), ("c96_p21_oddh", 2, 5, 3, 96, 2), ("c96_p22", 1, 4, 4, 96, 1),
                ("c128_p21", 2, 6, 5, 128, 2), ("c512_p22", 1, 4, 6, 512, 1), ("c1024_p22", 1, 4, 4, 1024, 1), ("c1024_p21_oddh", 1, 3, 2, 1024, 2),
                ("c512_p21_big", 1, 166, 100, 512, 2), ("c64_p22_big4", 1, 2, 2 * 33000, 64, 1)]


@pytest.mark.parametrize("case", UNPOOL_CASES, ids=[c[0] for c in UNPOOL_CASES])
def test_unpool_exact(case, monkeypatch, capfd):
    name, B, Ho, Wo, Cc, pool = case
    Hp, Wp = Ho // 2, (Wo // 2 if pool == 1 else Wo)
    g = ints(B, Hp, Wp, Cc, seed=21)
    pooled = ints(B, Hp, Wp, Cc, seed=22, lo=-2, hi=3).clamp(min=0)                 # post-ReLU values: half of them exactly 0 (no gradient)
    idx = ints(B, Hp, Wp, Cc, seed=23, lo=0, hi=3 if pool == 1 else 1)
    dyr, dbr = R.unpool(g, pooled, idx, Ho, Wo, pool)
    db0 = ints(Cc, seed=24, lo=1, hi=4)
    gd, g16, pd, pbd, idxd = Buf(g), Buf(g, torch.bfloat16), Buf(pooled), Buf(pooled, torch.bfloat16), Buf(idx, torch.uint8)
    decoy = Buf(torch.zeros_like(g))                                                # a valid fp32 map the launcher must not prefer over dpooled16 / pooledb
    fusable = 256 % (Cc // 4) == 0
    # (label, switches, dy, dyb, bias slab, mask, gradient, kernel)
    variants = []
    if fusable:
        if Cc % 8 == 0:
            variants += [("unpool8 f32 grad", {}, 0, 1, 1, "pooledb", "f32", "unpool8_kernel[]"), ("unpool8 bf16 grad", {}, 0, 1, 1, "pooledb", "bf16", "unpool8_kernel[]")]
        variants += [("unpool4 shadow only", {"AOCR_UNPOOL4": "1"}, 0, 1, 1, "pooledb", "f32", "unpool_kernel[0,1]"),
                     ("shadow only, fp32 mask", {}, 0, 1, 1, "pooled", "f32", "unpool_kernel[0,1]"),
                     ("f32 + shadow + bias", {}, 1, 1, 1, "pooledb", "f32", "unpool_kernel[1,1]")]
    else:
        variants += [("slab offered, C not fusable", {}, 1, 1, 1, "pooledb", "f32", "unpool_kernel[1,0]")]
    variants += [("plain, fp32 mask", {}, 1, 0, 0, "pooled", "f32", "unpool_kernel[1,0]"), ("plain, bf16 mask", {}, 1, 1, 0, "pooledb", "f32", "unpool_kernel[1,0]")]
    for label, env, want_dy, want_dyb, want_bias, mask, grad, kernel in variants:
        for defer in ((0, 1) if want_bias and fusable else (0,)):
            what = f"{name}: {label} defer={defer}"
            monkeypatch.delenv("AOCR_UNPOOL4", raising=False)
            setenv(monkeypatch, env)
            dy = Buf((B, Ho, Wo, Cc), fill=SENT) if want_dy else None
            dyb = Buf((B, Ho, Wo, Cc), torch.bfloat16, fill=7) if want_dyb else None
            dbias = Buf(db0) if want_bias else None
            partial = Buf((2048 * Cc,), fill=SENT) if want_bias else None        # csrc/ops.h: >= 2048*C floats
            capfd.readouterr()
            call("kp_unpool_relu_backward", (decoy if grad == "bf16" else gd).ptr(), (pd if mask == "pooled" else decoy).ptr(), idxd.ptr(), P(dy), B, Ho, Wo, Cc, pool,
                 P(dyb), P(dbias), P(partial), pbd.ptr() if mask == "pooledb" else None, defer, g16.ptr() if grad == "bf16" else None)
            torch.cuda.synchronize()
            expect(capfd, "unpool_relu_backward", kernel)
            tails(what, dy=dy, dyb=dyb, dbias=dbias, partial=partial)
            if dy is not None:
                assert torch.equal(dy.cpu(), dyr), what + ": dy"
            if dyb is not None:
                assert torch.equal(bits(dyb), bf(dyr)), what + ": dyb"
            if dbias is not None:
                assert torch.equal(dbias.cpu(), db0 + dbr if kernel != "unpool_kernel[1,0]" else db0), what + ": dbias"


# random gradients: dy is still pure selection (bit-equal), dyb must ROUND the fp32 value to nearest even (integers cannot tell that from truncation), and the fused
# bias gradient sums non-integers in fp32 through the thread partial, the LDS reduction, the slab and the column sum: at most one rounding per addition, fewer than
# n additions on any path for n windows per channel, each against sum |g mask|  ->  n * 2^-24 * (sum |g mask| + |dbias0|)
UNPOOL_RANDOM = [("c64_p22_odd", 2, 5, 7, 64, 1), ("c128_p21", 2, 6, 5, 128, 2), ("c512_p21_big", 1, 166, 100, 512, 2), ("c1024_p22", 1, 6, 8, 1024, 1)]


@pytest.mark.parametrize("case", UNPOOL_RANDOM, ids=[c[0] for c in UNPOOL_RANDOM])
def test_unpool_random(case, monkeypatch, capfd):
    name, B, Ho, Wo, Cc, pool = case
    worst = {}
    Hp, Wp = Ho // 2, (Wo // 2 if pool == 1 else Wo)
    g32 = (rnd(B, Hp, Wp, Cc, seed=25) * 3).float()
    gbf = g32.to(torch.bfloat16).float()                                            # what a producer that wrote d(pooled) as bf16 left
    assert (bf(g32).view(torch.bfloat16).float() != g32).float().mean().item() > 0.9, "the gradients must need rounding"
    pooled = rnd(B, Hp, Wp, Cc, seed=26).clamp(min=0).float()                       # half of them exactly 0
    idx = ints(B, Hp, Wp, Cc, seed=23, lo=0, hi=3 if pool == 1 else 1)
    db0 = ints(Cc, seed=24, lo=1, hi=4)
    pd, pbd, idxd = Buf(pooled), Buf(pooled, torch.bfloat16), Buf(idx, torch.uint8)
    n = B * Hp * Wp
    # (label, switches, dy, mask, gradient, kernel, defer)
    variants = [("unpool8 f32 grad", {}, 0, "pooledb", "f32", "unpool8_kernel[]", 0), ("unpool8 bf16 grad", {}, 0, "pooledb", "bf16", "unpool8_kernel[]", 1),
                ("unpool4 shadow only", {"AOCR_UNPOOL4": "1"}, 0, "pooledb", "f32", "unpool_kernel[0,1]", 1),
                ("shadow only, fp32 mask", {}, 0, "pooled", "f32", "unpool_kernel[0,1]", 0), ("f32 + shadow + bias", {}, 1, "pooled", "f32", "unpool_kernel[1,1]", 1)]
    keep = (pooled > 0).double()
    refs = {k: (R.unpool(t, pooled, idx, Ho, Wo, pool)[0], (t.double() * keep).sum(dim=(0, 1, 2)), (t.double().abs() * keep).sum(dim=(0, 1, 2)))
            for k, t in (("f32", g32), ("bf16", gbf))}
    for label, env, want_dy, mask, grad, kernel, defer in variants:
        what = f"{name}: {label} defer={defer}"
        monkeypatch.delenv("AOCR_UNPOOL4", raising=False)
        setenv(monkeypatch, env)
        g = gbf if grad == "bf16" else g32
        dyr, dbr, dba = refs[grad]
        gd = Buf(torch.zeros_like(g)) if grad == "bf16" else Buf(g)                 # bf16 gradient: the fp32 map is a decoy
        g16 = Buf(g, torch.bfloat16) if grad == "bf16" else None
        dy = Buf((B, Ho, Wo, Cc), fill=SENT) if want_dy else None
        dyb, dbias, partial = Buf((B, Ho, Wo, Cc), torch.bfloat16, fill=7), Buf(db0), Buf((2048 * Cc,), fill=SENT)
        capfd.readouterr()
        call("kp_unpool_relu_backward", gd.ptr(), pd.ptr(), idxd.ptr(), P(dy), B, Ho, Wo, Cc, pool, dyb.ptr(), dbias.ptr(), partial.ptr(),
             pbd.ptr() if mask == "pooledb" else None, defer, P(g16))
        torch.cuda.synchronize()
        expect(capfd, "unpool_relu_backward", kernel)
        tails(what, dy=dy, dyb=dyb, dbias=dbias, partial=partial)
        if dy is not None:
            assert torch.equal(dy.cpu(), dyr), what + ": dy"
        assert torch.equal(bits(dyb), bf(dyr)), what + ": dyb is not the RNE of the selected fp32 value"
        within(what, dbias.cpu(), db0.double() + dbr, n * U * (dba + db0.double()), worst, "dbias")
    report(f"test_unpool_random[{name}]", worst)


# ------------------------------------------------------------------------------------------------------------------------------
# BatchNorm (+ ReLU)
# ------------------------------------------------------------------------------------------------------------------------------
# (name, rows, C, tb_rows).  C = 4: 1024 row groups; 192 (C/4 = 48) and 2048 (C/4 > 256): the generic partial kernel, and 256 % 48 != 0 leaves the bias
# unfused; 1024: 4 row groups (RP = 4: 63 = 3 * 4 RP + 15, 65 -> two chunks of 33 = 2 * 4 RP + 1).  Chunk counts ceil(rows / 64) = 1, 17, 113, 129 (the edges of
# bn_reduce_partials' eight-load loop) and the 512 cap.  8200 x 256: rows C / 4 >= 2048 * 256 -- the fused-bias apply loop iterates and the slab is at its maximum.
BN_CASES = [("r1_c4", 1, 4, 0), ("r63_c4", 63, 4, 0), ("r65_c64", 65, 64, 0), ("r63_c192", 63, 192, 0), ("r65_c192", 65, 192, 0), ("r65_c256", 65, 256, 0),
            ("r1080_c64", 1080, 64, 0), ("r7200_c64", 7200, 64, 0), ("r8200_c256", 8200, 256, 0), ("r33000_c64", 33000, 64, 0), ("r63_c1024", 63, 1024, 0),
            ("r65_c1024", 65, 1024, 0), ("r70_c2048", 70, 2048, 0), ("tb_t7_b9_c256", 63, 256, 9), ("tb_t13_b5_c1024", 65, 1024, 5), ("tb_t9_b7_c192", 63, 192, 7)]
BN_IDS = [c[0] for c in BN_CASES]


def partial4_ok(Cc, old):
    c4 = Cc // 4
    return c4 <= 256 and c4 & (c4 - 1) == 0 and not old


def bn_scratch(Cc, chunks=None):
    """bn_relu_*'s scratch (bn_scratch_bytes(C) bytes of doubles), optionally holding `chunks` (n, C, 2) partial sums; the rest is junk the launcher must not read"""
    nd = kp().kp_bn_scratch_bytes(Cc) // 8
    s = Buf((nd,), torch.float64, fill=1e30)
    if chunks is not None:
        s.t[:chunks.numel()] = chunks.reshape(-1).cuda()
    return s


def chunk_sums(a, b, n):
    """(n, C, 2): the sums of a and b (rows, C) over n interleaved row classes -- an arbitrary partition, as a producing conv's epilogue would leave it"""
    return torch.stack([torch.stack([a[k::n].sum(0), b[k::n].sum(0)], dim=-1) if k < a.shape[0] else torch.zeros(a.shape[1], 2, dtype=a.dtype)
                        for k in range(n)])


def bn_params(Cc):
    return (rnd(Cc, seed=41) * 0.5 + 1.0).float(), rnd(Cc, seed=42).float(), ints(Cc, seed=43, lo=-2, hi=2) / 4, ints(Cc, seed=44, lo=1, hi=8) / 4


def bn_forward_run(name, x, Cc, tb, w, b, rm0, rv0, v, worst, monkeypatch, capfd):
    """v: dict(old, out, training, update, sync, chunks, xh)"""
    rows = x.shape[0]
    what = f"{name}: {v}"
    monkeypatch.delenv("AOCR_BN_PARTIAL_OLD", raising=False)
    if v["old"]:
        monkeypatch.setenv("AOCR_BN_PARTIAL_OLD", "1")
    xd = Buf(x + 1.0) if v["xh"] else Buf(x)                                        # with xh the fp32 map is a decoy (shifted by one)
    xh = Buf(x, torch.bfloat16) if v["xh"] else None
    dst = v["out"].split("+")
    y = Buf((rows, Cc), fill=SENT) if "y" in dst else None
    yb = Buf((rows, Cc), torch.bfloat16, fill=7) if "yb" in dst else None
    wd, bd, rm, rv, save = Buf(w), Buf(b), Buf(rm0), Buf(rv0), Buf((2 * Cc,), fill=SENT)
    # stats_chunks: the chunks hold the sums of ANOTHER map, so a launcher that ran its own pass over x (or xh) gives other statistics
    xs = ints(rows, Cc, seed=47, lo=-3, hi=5) if v["chunks"] else x
    xx = xs.double()
    scratch = bn_scratch(Cc, chunk_sums(xx, xx * xx, v["chunks"]) if v["chunks"] else None)
    capfd.readouterr()
    call("kp_bn_relu_forward2", xd.ptr(), P(y), wd.ptr(), bd.ptr(), rm.ptr(), rv.ptr(), save.ptr(), scratch.ptr(), rows, Cc, v["training"], v["update"], tb,
         P(yb), v["sync"], v["chunks"], P(xh))
    torch.cuda.synchronize()
    if v["training"]:
        expect(capfd, "bn_relu_forward", f"chunks[{v['chunks']}]" if v["chunks"] else "bn_partial4_kernel[0]" if partial4_ok(Cc, v["old"]) else "bn_partial_kernel[0]")
    else:
        assert not trace_of(capfd, "bn_relu_forward"), what + ": evaluation mode makes no partial-sum decision"
    tails(what, y=y, yb=yb, rm=rm, rv=rv, save=save, scratch=scratch)
    mean, inv, rmr, rvr = R.bn_stats(xs, rm0, rv0)
    if not v["training"]:
        mean, inv = rm0.double(), 1.0 / torch.sqrt(rv0.double() + 1e-5)
    sv = save.cpu()
    assert R.ulps(sv[:Cc], mean) <= 1 and R.ulps(sv[Cc:], inv) <= 1, f"{what}: save {R.ulps(sv[:Cc], mean)} / {R.ulps(sv[Cc:], inv)} ulp"
    if v["training"] and v["update"]:
        assert R.ulps(rm.cpu(), rmr) <= 1 and R.ulps(rv.cpu(), rvr) <= 1, f"{what}: running statistics {R.ulps(rm.cpu(), rmr)} / {R.ulps(rv.cpu(), rvr)} ulp"
    else:
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0), what + ": running statistics moved"
    yr, mag = R.bn_fwd(x, sv, w, b)
    if tb:
        yr, mag = R.to_tb(yr, rows // tb, tb), R.to_tb(mag, rows // tb, tb)
    if y is not None:
        within(what, y.cpu(), yr, C_Y * U * mag, worst, "y")
        if yb is not None:
            assert torch.equal(bits(yb), bf(y.cpu())), what + ": yb is not the RNE of the device's y"
    else:
        within(what, yb.cpu().float(), yr, C_Y * U * mag + BF * yr.abs(), worst, "yb-only")


@pytest.mark.parametrize("case", BN_CASES, ids=BN_IDS)
def test_bn_forward(case, monkeypatch, capfd):
    name, rows, Cc, tb = case
    worst = {}
    x = ints(rows, Cc, seed=40)
    w, b, rm0, rv0 = bn_params(Cc)
    base = dict(old=0, out="y+yb", training=1, update=1, sync=0, chunks=0, xh=0)
    variants = [base, dict(base, old=1, out="y"), dict(base, out="yb", update=0), dict(base, sync=1), dict(base, training=0, out="y"),
                dict(base, chunks=17), dict(base, chunks=113, sync=1, out="yb"), dict(base, chunks=129, old=1), dict(base, chunks=1), dict(base, chunks=512)]
    if partial4_ok(Cc, 0):
        variants += [dict(base, xh=1), dict(base, xh=1, chunks=17, out="yb"), dict(base, xh=1, training=0)]
    for v in variants:
        bn_forward_run(name, x, Cc, tb, w, b, rm0, rv0, v, worst, monkeypatch, capfd)
    report(f"test_bn_forward[{name}]", worst)


def bn_partial_floats(rows, Cc):                                     # csrc/ops.h: min(ceil(rows*C/4 / 256), 2048) * 1024 floats
    return min((rows * (Cc // 4) + 255) // 256, 2048) * 1024


def bn_backward_run(name, x, mask, dA, save, w, Cc, tb, ref, v, worst, monkeypatch, capfd):
    """v: dict(old, mask, apply, defer, sync, chunks, h); mask / dA are in the output's row order ((T, B) with tb)"""
    rows = x.shape[0]
    what = f"{name}: {v}"
    monkeypatch.delenv("AOCR_BN_PARTIAL_OLD", raising=False)
    if v["old"]:
        monkeypatch.setenv("AOCR_BN_PARTIAL_OLD", "1")
    p4 = partial4_ok(Cc, v["old"])
    fused = v["apply"] != "1,0" and 256 % (Cc // 4) == 0
    xd, dAd = (Buf(x + 1.0), Buf(dA + 1.0)) if v["h"] else (Buf(x), Buf(dA))      # with xh / dAh the fp32 maps are decoys
    xh, dAh = (Buf(x, torch.bfloat16), Buf(dA, torch.bfloat16)) if v["h"] else (None, None)
    yd = Buf(mask) if v["mask"] == "y" else Buf(torch.zeros_like(mask))
    ybd = Buf(mask, torch.bfloat16) if v["mask"] == "yb" else None
    dw0, db0, cb0 = ints(Cc, seed=51, lo=1, hi=4), ints(Cc, seed=52, lo=1, hi=4), ints(Cc, seed=53, lo=1, hi=4)
    dw, db, wd, sd = Buf(dw0), Buf(db0), Buf(w), Buf(save)
    want_dx = v["apply"] in ("1,0", "1,1") or not fused
    dx = Buf((rows, Cc), fill=SENT) if want_dx else None
    dxb = Buf((rows, Cc), torch.bfloat16, fill=7) if v["apply"] != "1,0" or v["mask"] == "yb" else None
    cdb = Buf(cb0) if v["apply"] != "1,0" else None
    partial = Buf((bn_partial_floats(rows, Cc),), fill=SENT) if v["apply"] != "1,0" else None
    if v["chunks"]:                                                                 # the sums of ANOTHER d A were handed over (ref["chunked"]): running the launcher's own pass changes every result
        scratch = bn_scratch(Cc, chunk_sums(ref["d2"], ref["d2"] * ref["xhat32"], v["chunks"]))
        ref = ref["chunked"]
    else:
        scratch = bn_scratch(Cc)
    capfd.readouterr()
    call("kp_bn_relu_backward", xd.ptr(), yd.ptr(), dAd.ptr(), wd.ptr(), sd.ptr(), P(dx), dw.ptr(), db.ptr(), scratch.ptr(), rows, Cc, tb, P(dxb), P(ybd),
         P(cdb), P(partial), v["sync"], v["defer"], P(xh), P(dAh), v["chunks"])
    torch.cuda.synchronize()
    lines(capfd, "bn_relu_backward", [f"chunks[{v['chunks']}]" if v["chunks"] else "bn_partial4_kernel[1]" if p4 else "bn_partial_kernel[1]",
                                      f"bn_bwd_apply_kernel[{v['apply'] if fused else '1,0'}]"])
    tails(what, dx=dx, dxb=dxb, dw=dw, db=db, conv_dbias=cdb, partial=partial, scratch=scratch)
    assert torch.equal(db.cpu().double(), db0.double() + ref["db"]), what + ": db"
    within(what, dw.cpu(), dw0.double() + ref["dw"], C_DW * U * (ref["dwmag"] + dw0.double()), worst, "dw")
    if dx is not None:
        within(what, dx.cpu(), ref["dx"], C_DX * U * ref["dxmag"], worst, "dx")
        if dxb is not None:
            assert torch.equal(bits(dxb), bf(dx.cpu())), what + ": dxb is not the RNE of the device's dx"
    else:
        within(what, dxb.cpu().float(), ref["dx"], C_DX * U * ref["dxmag"] + BF * ref["dx"].abs(), worst, "dxb-only")
    if cdb is not None and fused:
        within(what, cdb.cpu(), cb0.double() + ref["dx"].sum(0), (C_DX + rows) * U * (ref["dxmag"].sum(0) + cb0.double()), worst, "conv_dbias")
    elif cdb is not None:
        assert torch.equal(cdb.cpu(), cb0), what + ": conv_dbias must stay untouched where the bias gradient is not fused"
    return partial


def bn_backward_operands(rows, Cc, tb, x, dA, mask):
    w, _, rm0, rv0 = bn_params(Cc)
    mean, inv, _, _ = R.bn_stats(x, rm0, rv0)
    save = torch.cat([mean, inv]).float()
    mx, dAx = (R.to_tb(mask, tb, rows // tb), R.to_tb(dA, tb, rows // tb)) if tb else (mask, dA)      # (T, B) rows -> x's (B, T) order
    ref = R.bn_bwd(x, mx, dAx, save, w)
    # what a producing epilogue leaves as per-chunk sums holds the fp32 xhat, as the kernels compute it
    ref["xhat32"] = ((x - save[:Cc]) * save[Cc:]).double()
    # sums_chunks: the producer's sums are those of another integer d A (same mask); d x of the live d A is then taken against THOSE sums
    r2 = R.bn_bwd(x, mx, ints(rows, Cc, seed=48, lo=-3, hi=5), save, w)
    ref["d2"] = r2["d"]
    ref["chunked"] = R.bn_bwd(x, mx, dAx, save, w, sums=(r2["db"], r2["dw"], r2["dwmag"]))
    return w, save, ref


@pytest.mark.parametrize("case", BN_CASES, ids=BN_IDS)
def test_bn_backward(case, monkeypatch, capfd):
    name, rows, Cc, tb = case
    worst = {}
    x, dA = ints(rows, Cc, seed=40), ints(rows, Cc, seed=45)
    mask = ints(rows, Cc, seed=46, lo=-1, hi=2).clamp(min=0)                        # post-ReLU values: half of them exactly 0
    w, save, ref = bn_backward_operands(rows, Cc, tb, x, dA, mask)
    base = dict(old=0, mask="y", apply="1,0", defer=0, sync=0, chunks=0, h=0)
    variants = [base, dict(base, old=1), dict(base, mask="yb"), dict(base, sync=1), dict(base, chunks=17), dict(base, chunks=129, sync=1, mask="yb"),
                dict(base, apply="1,1", mask="yb"), dict(base, apply="1,1", defer=1), dict(base, apply="0,1", mask="yb"),
                dict(base, apply="0,1", mask="yb", defer=1, old=1), dict(base, apply="0,1", chunks=113, mask="yb", sync=1)]
    if partial4_ok(Cc, 0):
        variants += [dict(base, h=1), dict(base, h=1, apply="0,1", mask="yb", defer=1), dict(base, h=1, apply="1,1", chunks=17)]
    for v in variants:
        partial = bn_backward_run(name, x, mask, dA, save, w, Cc, tb, ref, v, worst, monkeypatch, capfd)
        if name == "r8200_c256" and partial is not None:
            assert partial.n == 2048 * 1024 and not (partial.cpu() == SENT).any(), "the maximum slab (2048 * 1024 floats) is written to its last element"
    report(f"test_bn_backward[{name}]", worst)


BN_RANDOM = [("r257_c64", 257, 64, 0), ("r130_c192", 130, 192, 0), ("tb_t9_b8_c512", 72, 512, 8)]


@pytest.mark.parametrize("case", BN_RANDOM, ids=[c[0] for c in BN_RANDOM])
def test_bn_random(case, monkeypatch, capfd):
    name, rows, Cc, tb = case
    worst = {}
    x, dA = (rnd(rows, Cc, seed=60) * 3).float(), rnd(rows, Cc, seed=61).float()
    w, b, rm0, rv0 = bn_params(Cc)
    base = dict(old=0, out="y+yb", training=1, update=1, sync=0, chunks=0, xh=0)
    for v in (base, dict(base, old=1, sync=1), dict(base, out="yb")):
        # random x: the fp64 sums of fp32 values are exact to ~2^-53 relative, far inside the 1-ulp fp32 assertion on save
        bn_forward_run(name, x, Cc, tb, w, b, rm0, rv0, v, worst, monkeypatch, capfd)
    mask = rnd(rows, Cc, seed=62).clamp(min=0).float()
    # db: a fp64 sum of fp32 terms, rounded once and added once -- compared as dw is (bn_backward_run asserts bit-equality, so integer db0 is subtracted there):
    # make the sum itself an integer by rounding d A to multiples of 2^-10 (exact in fp64 sums, and (float) of the sum is then exact below 2^14)
    dA = (dA * 1024).round() / 1024
    w, save, ref = bn_backward_operands(rows, Cc, tb, x, dA, mask)
    bvar = dict(old=0, mask="y", apply="1,0", defer=0, sync=0, chunks=0, h=0)
    for v in (bvar, dict(bvar, apply="1,1", mask="yb", defer=1), dict(bvar, apply="0,1", mask="yb", old=1, sync=1)):
        bn_backward_run(name, x, mask, dA, save, w, Cc, tb, ref, v, worst, monkeypatch, capfd)
    report(f"test_bn_random[{name}]", worst)


# ------------------------------------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------------------------------------
def colsum_operand(rows, N, ld, offset, seed):
    """A (rows, ld) integers inside a buffer that starts `offset` floats earlier; columns N.. of every row are junk the sum must not read"""
    a = ints(rows, ld, seed=seed)
    a[:, N:] = 1000.0
    flat = torch.cat([torch.full((offset,), 1000.0), a.reshape(-1)])
    return a, Buf(flat)


COLSUM_N = (3, 39, 64, 576, 2048)
COLSUM_ROWS = (1, 15, 16, 17, 129, 5000)


@pytest.mark.parametrize("N", COLSUM_N)
def test_colsum_accum(N, monkeypatch, capfd):
    for rows in COLSUM_ROWS:
        # ld a multiple of 4 on an aligned base (16-byte loads); ld % 4 != 0; a base one float off 16 bytes (both: the scalar branch)
        for ld, offset in (((N + 3) // 4 * 4 + 4, 0), ((N + 3) // 4 * 4 + 1, 0), ((N + 3) // 4 * 4, 1)):
            for with_out2 in (0, 1):
                what = f"N={N} rows={rows} ld={ld} offset={offset} out2={with_out2}"
                a, ad = colsum_operand(rows, N, ld, offset, seed=70 + rows)
                o0, p0 = ints(N, seed=71, lo=1, hi=4), ints(N, seed=72, lo=5, hi=9)
                out, out2 = Buf(o0), Buf(p0) if with_out2 else None
                call("kp_colsum_accum", C.c_void_p(ad.full.data_ptr() + 4 * offset), ld, rows, N, out.ptr(), P(out2))
                torch.cuda.synchronize()
                tails(what, out=out, out2=out2, A=ad)
                s = a[:, :N].sum(0)                                                   # integers below 2^24: exact; rows = 5000 takes the atomic form (ny > 1)
                assert torch.equal(out.cpu(), o0 + s), what + ": out"
                if out2 is not None:
                    assert torch.equal(out2.cpu(), p0 + s), what + ": out2"


# (rows, N, ld, offset, out2) per job
JOBS8 = [(5000, 576, 640, 0, 0), (129, 64, 640, 0, 0), (17, 39, 41, 0, 1), (1, 3, 4, 0, 0), (2048, 512, 512, 0, 0), (16, 2048, 2048, 1, 1), (15, 64, 64, 0, 0),
         (600, 1024, 1024, 0, 0)]


@pytest.mark.parametrize("njobs", (1, 8, 9))
def test_colsum_jobs(njobs, monkeypatch, capfd):
    jobs = (JOBS8 + [(33, 64, 64, 0, 1)])[:njobs]
    ops, outs, out2s, refs = [], [], [], []
    for i, (rows, N, ld, offset, with_out2) in enumerate(jobs):
        a, ad = colsum_operand(rows, N, ld, offset, seed=80 + i)
        o0, p0 = ints(N, seed=90 + i, lo=1, hi=4), ints(N, seed=95 + i, lo=5, hi=9)
        ops.append(ad); outs.append(Buf(o0)); out2s.append(Buf(p0) if with_out2 else None); refs.append((o0, p0, a[:, :N].sum(0)))
    n = len(jobs)
    A = (vp * n)(*[ad.full.data_ptr() + 4 * j[3] for ad, j in zip(ops, jobs)])
    O = (vp * n)(*[o.full.data_ptr() for o in outs])
    O2 = (vp * n)(*[o.full.data_ptr() if o is not None else None for o in out2s])
    ld = (i64 * n)(*[j[2] for j in jobs]); rows = (i64 * n)(*[j[0] for j in jobs]); N = (i32 * n)(*[j[1] for j in jobs])
    dropped = i32(-1)
    call("kp_colsum_jobs", n, A, ld, rows, N, O, O2, C.byref(dropped))
    torch.cuda.synchronize()
    assert dropped.value == max(0, n - 8), f"{dropped.value} jobs dropped"
    for i, (o0, p0, s) in enumerate(refs):
        tails(f"job {i}", out=outs[i], out2=out2s[i], A=ops[i])
        taken = i < 8                                                               # the table holds 8: a 9th deferred job is not run and its outputs stay as they were
        assert torch.equal(outs[i].cpu(), o0 + s if taken else o0), f"job {i} of {n}: out"
        if out2s[i] is not None:
            assert torch.equal(out2s[i].cpu(), p0 + s if taken else p0), f"job {i} of {n}: out2"


# random operands: fp32 sums of `rows` non-integers per column in some order (lane partial, LDS tree, one atomic per row chunk): at most one rounding per addition,
# fewer than `rows` additions on any path, each against sum |A| + |out0|  ->  rows * 2^-24 * (sum |A| + |out0|)
# (rows, N, ld, offset): the atomic form on 16-byte loads; the scalar branch (ld % 4 != 0); a base one float off 16 bytes with the eight-row loop
COLSUM_RANDOM = [(5000, 576, 640, 0), (17, 39, 41, 0), (129, 2048, 2048, 1)]


def colsum_random_operand(rows, N, ld, offset, seed):
    a = rnd(rows, ld, seed=seed).float()
    a[:, N:] = 1000.0
    return a, Buf(torch.cat([torch.full((offset,), 1000.0), a.reshape(-1)]))


def test_colsum_random(monkeypatch, capfd):
    worst = {}
    ops = [colsum_random_operand(*c, seed=75 + i) for i, c in enumerate(COLSUM_RANDOM)]
    o0 = [ints(c[1], seed=76, lo=1, hi=4) for c in COLSUM_RANDOM]
    ref = [o.double() + a[:, :c[1]].double().sum(0) for (a, _), o, c in zip(ops, o0, COLSUM_RANDOM)]
    bnd = [c[0] * U * (a[:, :c[1]].double().abs().sum(0) + o.double()) for (a, _), o, c in zip(ops, o0, COLSUM_RANDOM)]
    for i, (rows, N, ld, offset) in enumerate(COLSUM_RANDOM):
        what = f"rows={rows} N={N} ld={ld} offset={offset}"
        out, out2 = Buf(o0[i]), Buf(o0[i])
        call("kp_colsum_accum", C.c_void_p(ops[i][1].full.data_ptr() + 4 * offset), ld, rows, N, out.ptr(), out2.ptr())
        torch.cuda.synchronize()
        tails(what, out=out, out2=out2, A=ops[i][1])
        within(what, out.cpu(), ref[i], bnd[i], worst, "accum")
        assert torch.equal(out2.cpu(), out.cpu()) or rows > 512, what + ": out2 is the same sum (ny == 1: the same value)"
        within(what, out2.cpu(), ref[i], bnd[i], worst, "accum")
    n = len(COLSUM_RANDOM)                                                           # the same three sums as deferred jobs behind one flush
    outs = [Buf(o) for o in o0]
    A = (vp * n)(*[ad.full.data_ptr() + 4 * c[3] for (_, ad), c in zip(ops, COLSUM_RANDOM)])
    O = (vp * n)(*[o.full.data_ptr() for o in outs])
    O2 = (vp * n)(*[None] * n)
    ld = (i64 * n)(*[c[2] for c in COLSUM_RANDOM]); rows = (i64 * n)(*[c[0] for c in COLSUM_RANDOM]); N = (i32 * n)(*[c[1] for c in COLSUM_RANDOM])
    dropped = i32(-1)
    call("kp_colsum_jobs", n, A, ld, rows, N, O, O2, C.byref(dropped))
    torch.cuda.synchronize()
    assert dropped.value == 0
    for i in range(n):
        tails(f"job {i}", out=outs[i])
        within(f"job {i}", outs[i].cpu(), ref[i], bnd[i], worst, "jobs")
    report("test_colsum_random", worst)
