"""GPU: every attention kernel instantiation (csrc/ops_misc.hip: attn_launch behind attention_forward / attention_backward, the two
attention_*_dual launchers, attention_dctx) against a float64 reference, called directly through tests/libkprobe.so.  Method
of tests/test_kernels_bf16_gpu.py and tests/test_step_kernels_bf16_gpu.py, helpers of tests/kernel_harness.py: every output is a window of a wider buffer or has a sentinel
tail, nothing outside the window may change, and every case asserts the kernel it reached from the AOCR_TRACE dispatch line
("[aocr] <function>: <kernel>[<instantiation>] B T Hd").

Operands.  Context values are integers in [-2, 2] times 2^-2 (exact in bf16; given as fp32 ctx AND as the bf16 shadow ctxb), u (the query, or
d c for the backward pass) integers in [-2, 2] times 2^-3.  Every score is a sum of multiples of 2^-5 far below 2^20 quanta: exact in fp32 in any
summation order, and the float64 reference has it exactly.  ONE wrong, missing or doubled product moves a score by >= 2^-5 = 0.03, which moves
any probability in (1e-3, 0.999) by more than 3e-5.
Edge rows.  Rows 0, T - 1 and the last / first row on both sides of every 64-row boundary (the streamed 16-wave forms' and beam<1,8,5>'s chunk; also
used for the register forms and the 4-wave kernels) or 32-row boundary (the 8-wave and beam<2,4,5> forms) each get a batch row of their own, in
which the first n columns of that context row are overwritten with 0.5 sign(u_b) (still exact).  n grows until the float64 reference gives the row a probability >= 0.05 in
its batch row (asserted on the reference), so a kernel that drops, doubles or misplaces an edge row misses every tolerance.  With ctx_div = k the
context belongs to the image and the edge is checked in one of its hypotheses; the beam cases use as many images as it takes to give every edge
a row (at least 2).
Forward: a within 2e-5 of softmax(ctx u), c within 5e-5 max|ctx| of a^T ctx (the tolerances of test_ops_gpu.py::test_attention), the bf16
shadow cb = RNE of the device's own c, bit for bit.  Backward: a = float32 of the reference probabilities of a forward problem with another u;
d a = ctx d c, d s = a (d a - sum a d a) within 5e-5 max(1, max|d a|), d q = d s^T ctx within 1e-4 max(1, max|d a|) max|ctx|, dqb = RNE of the
device's d q; the one-pass streamed form gets cfwd = float32(a^T ctx) as a window with ldcf = 2 Hd.  DUAL forms: a second, independent integer
context ctxab -- forward scores from ctxab and weighted sum from ctx; backward d a, d s, d q from ctx and dh_attn = d s^T ctxab at d q's tolerance.
Random operands (one case per kernel family): context rounded to bf16, fp32 u scaled to a score deviation of about 2; a within
2e-5 + bound(|ctx| |u|, Hd), c within 5e-5 + 2 bound (an error e in every score moves sum_t |a_t| by <= 2 e); d s and d q the same way on top of
their integer-case tolerances.
attn_dctx_kernel: a, d s integers times 2^-3, d c, q integers times 2^-2: every sum is exact and dctx equals float64 bit for bit.

Instantiations asserted (their union is every launch statement of attn_launch and of both dual launchers):
  attn_reg_h512_kernel[w16]                  512: T = 1, 15, 16, 17, 63, 64; ctx_div = 3; also what AOCR_NO_ATTN_BF16=1 reaches at T <= 64 (the switch
                                             does not cover this branch: its condition is ctxb && ldu % 4 == 0)
  attn_bf16_kernel[1,8,reg,w16]              512: 65, 128            attn_bf16_kernel[1,16,reg,w16]   512: 129, 256
  attn_bf16_kernel[1,4,stream,w16,onepass]   512: 257, 320, 321 (forward; backward with cfwd)   ...,twopass]: backward, AOCR_ATTN_BWD_TWO_PASS=1
  attn_bf16_kernel[2,4,reg,w8]               1024: 1, 7, 8, 9, 24, 32
  attn_bf16_kernel[2,4,reg,w16]              1024: 33, 64; 24 with AOCR_ATTN_NW16=1
  attn_bf16_kernel[2,8,reg,w16]              1024: 65, 128
  attn_bf16_kernel[2,4,stream,w16,onepass | twopass]   1024: 129, 192, 200
  attn_bf16_kernel[2,4,reg,w8,dual]          1024: 1, 24, 32        attn_bf16_kernel[2,4,reg,w16,dual]   1024: 33, 64   (forward ctx_div 1, 2; backward)
  attn_bf16_beam_kernel[1,8,5]               512: 65, 128, 130, k = 2, 3, 5    attn_bf16_beam_kernel[2,4,5]   1024: 65, 96, 100, k = 2, 5
                                             (AOCR_NO_ATTN_BEAM_GROUP=1: the per-row attn_bf16_kernel, same tolerances)
  attn_reg_kernel[2,f32] / [1,f32]           512 / 256: 1, 63, 64, no ctxb
  attn_core_kernel[]                         (32, 8), (768, 65), (512, 300), no ctxb; (512, 65) with ctxb under AOCR_NO_ATTN_BF16=1
  attn_dctx_kernel[]                         (L, T, Hd) = (1, 1, 32), (32, 64, 96), (33, 65, 96), (70, 130, 512)

measured (largest error / tolerance per test, MI355X):
  test_attention_exact[h512-T1]: a 0  c 0  ds 0  dq 0
  test_attention_exact[h512-T15]: a 0.0021  c 0.0026  ds 0.00049  dq 0.00048
  test_attention_exact[h512-T16]: a 0.0022  c 0.003  ds 0.00077  dq 0.00069
  test_attention_exact[h512-T17]: a 0.0075  c 0.0052  ds 0.00032  dq 0.00036
  test_attention_exact[h512-T63]: a 0.0043  c 0.0036  ds 0.00025  dq 0.00043
  test_attention_exact[h512-T64]: a 0.0022  c 0.0024  ds 0.00022  dq 0.00029
  test_attention_exact[bf16_1_8_reg-T65]: a 0.0066  c 0.0048  ds 0.00058  dq 0.00038
  test_attention_exact[bf16_1_8_reg-T128]: a 0.0032  c 0.0037  ds 0.00025  dq 0.00014
  test_attention_exact[bf16_1_16_reg-T129]: a 0.0045  c 0.0047  ds 0.0002  dq 0.00026
  test_attention_exact[bf16_1_16_reg-T256]: a 0.0013  c 0.0046  ds 0.00049  dq 0.00044
  test_attention_exact[bf16_1_4_stream-T257]: a 0.0089  c 0.0083  ds 0.0033  dq 0.0057
  test_attention_exact[bf16_1_4_stream-T320]: a 0.0073  c 0.0076  ds 0.00025  dq 0.00042
  test_attention_exact[bf16_1_4_stream-T321]: a 0.008  c 0.011  ds 0.00094  dq 0.0017
  test_attention_exact[bf16_2_4_reg_w8-T1]: a 0  c 0  ds 0  dq 0
  test_attention_exact[bf16_2_4_reg_w8-T7]: a 0.0065  c 0.0038  ds 0.0002  dq 0.00022
  test_attention_exact[bf16_2_4_reg_w8-T8]: a 0.0047  c 0.0036  ds 8.1e-05  dq 0.00012
  test_attention_exact[bf16_2_4_reg_w8-T9]: a 0.0074  c 0.0048  ds 0.0011  dq 0.00059
  test_attention_exact[bf16_2_4_reg_w8-T24]: a 0.0033  c 0.0045  ds 0.00058  dq 0.00037
  test_attention_exact[bf16_2_4_reg_w8-T32]: a 0.0011  c 0.0028  ds 0.00012  dq 0.00041
  test_attention_exact[bf16_2_4_reg_w16-T33]: a 0.0045  c 0.0042  ds 0.001  dq 0.00072
  test_attention_exact[bf16_2_4_reg_w16-T64]: a 0.0046  c 0.0043  ds 0.00014  dq 0.00011
  test_attention_exact[bf16_2_4_reg_w16_nw16-T24]: a 0.0033  c 0.0046  ds 0.00058  dq 0.0004
  test_attention_exact[bf16_2_8_reg-T65]: a 0.0053  c 0.0052  ds 0.00013  dq 0.00029
  test_attention_exact[bf16_2_8_reg-T128]: a 0.0014  c 0.0028  ds 0.00032  dq 0.00021
  test_attention_exact[bf16_2_4_stream-T129]: a 0.0045  c 0.0064  ds 0.00016  dq 0.00056
  test_attention_exact[bf16_2_4_stream-T192]: a 0.0087  c 0.0068  ds 0.00016  dq 0.00066
  test_attention_exact[bf16_2_4_stream-T200]: a 0.02  c 0.012  ds 0.00085  dq 0.0014
  test_attention_exact[reg_2_f32-T1]: a 0  c 0  ds 0  dq 0
  test_attention_exact[reg_2_f32-T63]: a 0.0043  c 0.006  ds 0.00025  dq 0.00039
  test_attention_exact[reg_2_f32-T64]: a 0.0022  c 0.0025  ds 0.00022  dq 0.00028
  test_attention_exact[reg_1_f32-T1]: a 0  c 0  ds 0  dq 0
  test_attention_exact[reg_1_f32-T63]: a 0.0047  c 0.0062  ds 0.00024  dq 0.00016
  test_attention_exact[reg_1_f32-T64]: a 0.0039  c 0.0039  ds 0.0011  dq 0.00079
  test_attention_exact[core_h32-T8]: a 0.0014  c 0.002  ds 0.00037  dq 0.00054
  test_attention_exact[core_h768-T65]: a 0.0017  c 0.0076  ds 0.00038  dq 0.00022
  test_attention_exact[core_h512-T300]: a 0.0019  c 0.014  ds 0.00072  dq 0.00052
  test_attention_exact[no_attn_bf16_h512-T24]: a 0.002  c 0.0033  ds 0.00015  dq 0.00027
  test_attention_exact[no_attn_bf16_h512-T64]: a 0.0022  c 0.0024  ds 0.00022  dq 0.00029
  test_attention_exact[no_attn_bf16_core-T65]: a 0.0024  c 0.0085  ds 0.00015  dq 0.00021
  test_attention_h512_ctx_div[17]: a 0.0014  c 0.0023
  test_attention_h512_ctx_div[64]: a 0.0046  c 0.0038
  test_attention_dual[1]: a 0  c 0  ds 0  dq 0  dh_attn 0
  test_attention_dual[24]: a 0.0072  c 0.0047  ds 0.00014  dq 0.00056  dh_attn 0.0005
  test_attention_dual[32]: a 0.0029  c 0.0033  ds 0.00063  dq 0.00053  dh_attn 0.00053
  test_attention_dual[33]: a 0.0032  c 0.0034  ds 0.00013  dq 0.00039  dh_attn 0.00023
  test_attention_dual[64]: a 0.0038  c 0.0049  ds 0.00031  dq 0.0006  dh_attn 0.00052
  test_attention_beam[beam_1_8_5-T65]: a 0.0092  c 0.007
  test_attention_beam[beam_1_8_5-T128]: a 0.011  c 0.0096
  test_attention_beam[beam_1_8_5-T130]: a 0.015  c 0.011
  test_attention_beam[beam_2_4_5-T65]: a 0.0083  c 0.009
  test_attention_beam[beam_2_4_5-T96]: a 0.016  c 0.0098
  test_attention_beam[beam_2_4_5-T100]: a 0.015  c 0.011
  test_attention_random[h512]: a 0.00034  c 0.00032  ds 0.00012  dq 0.0002
  test_attention_random[bf16_reg]: a 0.00013  c 0.0002  ds 5.7e-05  dq 9.7e-05
  test_attention_random[bf16_stream]: a 0.00024  c 0.00032  ds 5.1e-05  dq 0.00013
  test_attention_random[beam]: a 0.00014  c 0.00022
  test_attention_random[core]: a 0.00036  c 0.00035  ds 0.00029  dq 0.00035
  test_attention_dctx_exact[1-1-32]: 0 of 96 elements differ from float64
  test_attention_dctx_exact[32-64-96]: 0 of 18432 elements differ from float64
  test_attention_dctx_exact[33-65-96]: 0 of 18720 elements differ from float64
  test_attention_dctx_exact[70-130-512]: 0 of 199680 elements differ from float64
"""
import math

import pytest
import torch

from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module (tests/test_kernel_harness_cpu.py checks it)
from kernel_harness import SENT, TOL_A, TOL_C, TOL_DQ, TOL_DS, Buf, Mat, bf, bound, call, expect, ints, kp, out, ratio, rnd, setenv, vp

pytestmark = pytest.mark.gpu

P_EDGE = 0.05                       # least reference probability of a planted edge row in its batch row
QC, QU = 2.0 ** -2, 2.0 ** -3       # quanta of the context and of u


def edges(T, chunk):
    e = {0, T - 1}
    for c in range(chunk, T, chunk):
        e |= {c - 1, c}
    return sorted(e)


def softmax_ref(ctx, u, k):
    """float64: scores of batch row b against the context of image b // k"""
    img = torch.arange(u.shape[0]) // k
    return torch.softmax(torch.einsum("btj,bj->bt", ctx[img], u), dim=1)


def wsum_ref(p, ctx, k):
    img = torch.arange(p.shape[0]) // k
    return torch.einsum("bt,btj->bj", p, ctx[img])


class Problem:
    """Exact-integer context [nimg][T][Hd] and u [nimg k][Hd] with every edge row of `chunk` planted in a batch row of its own."""

    def __init__(self, Hd, T, chunk, k=1, nimg=None, seed=0):
        ed = edges(T, chunk)
        if nimg is None:
            nimg = max(-(-4 // k), -(-len(ed) // k))
        B = nimg * k
        assert len(ed) <= B
        self.B, self.T, self.Hd, self.k, self.nimg, self.ed = B, T, Hd, k, nimg, ed
        plant, seen = [], set()                                        # (batch row, its edge row): every edge once, and again in the other images
        for r in range(B):
            t = ed[r % len(ed)]
            if (r // k, t) not in seen:
                seen.add((r // k, t))
                plant.append((r, t))
        base = ints(nimg, T, Hd, seed=seed, lo=-2, hi=2).double() * QC
        self.u = ints(B, Hd, seed=seed + 1, lo=-2, hi=2).double() * QU
        # a planted row scores about 0.075 n (E|u| = 0.15) against ln(sum e^s) ~ ln T + var(s) / 2 with var(s) = Hd / 256
        n = min(Hd, math.ceil((math.log(T) + Hd / 512.0 + 1.0) / 0.075))
        while True:
            ctx = base.clone()
            for b, t in plant:
                ctx[b // k, t, :n] = 0.5 * torch.sign(self.u[b, :n])
            a = softmax_ref(ctx, self.u, k)
            self.p_edge = min(a[b, t].item() for b, t in plant)
            if self.p_edge >= P_EDGE or n >= Hd:
                break
            n = min(Hd, n + 16)
        assert self.p_edge >= P_EDGE, f"edge rows carry too little weight in the reference ({self.p_edge:.3g}, n = {n})"
        self.ctx, self.a, self.n = ctx, a, n
        self.c = wsum_ref(a, ctx, k)


def plain_ctx(nimg, T, Hd, seed):
    return ints(nimg, T, Hd, seed=seed, lo=-2, hi=2).double() * QC


def b16(t):
    return t.contiguous().view(torch.int16)


def run_forward(ctx, u, k, shadow=True, ctxab=None):
    """ctx [nimg][T][Hd], u [B][Hd] (float64 CPU, exact in their device types).  ctxab: the DUAL launcher (scores from ctxab).  Returns (a, c) of the device."""
    nimg, T, Hd = ctx.shape
    B = u.shape[0]
    ctxd, ctxb = Buf(ctx), Buf(ctx, torch.bfloat16) if shadow else None
    a, c, cb = Buf((B, T), fill=SENT), out(B, Hd, pad=Hd), out(B, Hd, torch.bfloat16, pad=Hd)
    if ctxab is None:
        ud = Buf(u)
        call("kp_attention_forward", ctxd.ptr(), ud.ptr(), a.ptr(), vp(c.addr), c.ld, B, T, Hd, k, vp(cb.addr), cb.ld, ctxb.ptr() if shadow else None)
    else:
        ud, cab = Mat(B, Hd, data=u, pad=8), Buf(ctxab, torch.bfloat16)
        call("kp_attention_forward_dual", vp(ud.addr), ud.ld, a.ptr(), vp(c.addr), c.ld, B, T, k, vp(cb.addr), cb.ld, ctxb.ptr(), cab.ptr())
    torch.cuda.synchronize()
    a.check_tail("a"); c.check("c"); cb.check("cb")
    assert torch.equal(b16(cb.win()), bf(c.win())), "cb is not the RNE of the kernel's own c"
    return a.cpu(), c.win()


def check_forward(got, ref_a, ref_c, maxctx, extra=0.0):
    """-> (a, c) error / tolerance.  extra: the random cases' score bound per batch row ([B][1])"""
    return ratio(got[0], ref_a, TOL_A + extra), ratio(got[1], ref_c, TOL_C * maxctx + 2 * extra)


def backward_ref(ctx, a32, dc, ctxab=None):
    """float64 of LSTM.lua's attention backward on the inputs as given (a32: the float32 probabilities)"""
    a = a32.double()
    da = torch.einsum("btj,bj->bt", ctx, dc)
    ds = a * (da - (a * da).sum(1, keepdim=True))
    r = dict(da=da, ds=ds, dq=torch.einsum("bt,btj->bj", ds, ctx), cfwd=torch.einsum("bt,btj->bj", a, ctx).float())
    if ctxab is not None:
        r["dh"] = torch.einsum("bt,btj->bj", ds, ctxab)
    return r


def run_backward(ctx, a32, dc, ref, shadow=True, cfwd=False, ctxab=None):
    """ctx [B][T][Hd]; d c is the first half of a [B][2 Hd] buffer (junk in the other half).  Returns the device's (ds, dq, dh_attn or None)."""
    B, T, Hd = ctx.shape
    ctxd, ctxb = Buf(ctx), Buf(ctx, torch.bfloat16) if shadow else None
    ad, dcd = Buf(a32), Mat(B, Hd, data=dc, pad=Hd)
    ds, dq, dqb = Buf((B, T), fill=SENT), Buf((B, Hd), fill=SENT), Buf((B, Hd), torch.bfloat16, fill=-3.0)
    dh = None
    if ctxab is None:
        cf = Mat(B, Hd, data=ref["cfwd"], pad=Hd) if cfwd else None
        call("kp_attention_backward", ctxd.ptr(), ad.ptr(), vp(dcd.addr), dcd.ld, ds.ptr(), dq.ptr(), B, T, Hd, dqb.ptr(),
             ctxb.ptr() if shadow else None, vp(cf.addr) if cf else None, cf.ld if cf else 0)
    else:
        dh, cab = Buf((B, Hd), fill=SENT), Buf(ctxab, torch.bfloat16)
        call("kp_attention_backward_dual", ad.ptr(), vp(dcd.addr), dcd.ld, ds.ptr(), dq.ptr(), dqb.ptr(), dh.ptr(), B, T, ctxb.ptr(), cab.ptr())
    torch.cuda.synchronize()
    ds.check_tail("ds"); dq.check_tail("dq"); dqb.check_tail("dqb")
    assert torch.equal(b16(dqb.cpu()), bf(dq.cpu())), "dqb is not the RNE of the kernel's own dq"
    if dh is not None:
        dh.check_tail("dh_attn")
    return ds.cpu(), dq.cpu(), dh.cpu() if dh is not None else None


def check_backward(got, ref, maxctx, extra=0.0):
    """-> (ds, dq[, dh_attn]) error / tolerance"""
    m = max(1.0, ref["da"].abs().max().item())
    r = [ratio(got[0], ref["ds"], TOL_DS * m + extra), ratio(got[1], ref["dq"], TOL_DQ * m * maxctx + 2 * extra)]
    if got[2] is not None:
        r.append(ratio(got[2], ref["dh"], TOL_DQ * m * maxctx + 2 * extra))
    return r


_WORST = {}


@pytest.fixture(autouse=True)
def _record(request):
    """one "[attn-kernels] <test id>: ..." line per test: its largest error / tolerance per output over everything it ran"""
    _WORST.clear()
    yield
    if _WORST:
        print(f"[attn-kernels] {request.node.name}: " + "  ".join(f"{n} {r:.2g}" for n, r in _WORST.items()))


def report(what, names, rs):
    for n, r in zip(names, rs):
        _WORST[n] = max(_WORST.get(n, 0.0), r)
    assert all(r <= 1.0 for r in rs), (what, [f"{n} error / tolerance = {r:.3f}" for n, r in zip(names, rs)])


def fwd_bwd(name, Hd, T, chunk, capfd, monkeypatch, fwd_kernel, bwd_kernels, shadow=True, seed=0):
    """One planted forward problem and one planted backward problem; bwd_kernels: [(kernel, cfwd given, switches)]."""
    p = Problem(Hd, T, chunk, seed=seed)
    capfd.readouterr()
    got = run_forward(p.ctx, p.u, 1, shadow)
    expect(capfd, "attention_forward", fwd_kernel)
    report(f"{name} T={T} forward (B={p.B}, n={p.n}, edge p>={p.p_edge:.2f})", ("a", "c"), check_forward(got, p.a, p.c, 0.5))
    q = Problem(Hd, T, chunk, seed=seed + 10)                          # its a: the probabilities the backward pass is given
    dc = ints(q.B, Hd, seed=seed + 20, lo=-2, hi=2).double() * QU
    a32 = q.a.float()
    ref = backward_ref(q.ctx, a32, dc)
    for kernel, cfwd, env in bwd_kernels:
        setenv(monkeypatch, env)
        capfd.readouterr()
        gb = run_backward(q.ctx, a32, dc, ref, shadow, cfwd)
        expect(capfd, "attention_backward", kernel)
        report(f"{name} T={T} backward {kernel}", ("ds", "dq"), check_backward(gb, ref, 0.5))


# (name, Hd, Ts, chunk, switches, forward kernel, backward: None = the same kernel, "stream" = one-pass with cfwd and two-pass, ctxb given)
CASES = [
    ("h512", 512, (1, 15, 16, 17, 63, 64), 64, {}, "attn_reg_h512_kernel[w16]", None, True),
    ("bf16_1_8_reg", 512, (65, 128), 64, {}, "attn_bf16_kernel[1,8,reg,w16]", None, True),
    ("bf16_1_16_reg", 512, (129, 256), 64, {}, "attn_bf16_kernel[1,16,reg,w16]", None, True),
    ("bf16_1_4_stream", 512, (257, 320, 321), 64, {}, "attn_bf16_kernel[1,4,stream,w16", "stream", True),
    ("bf16_2_4_reg_w8", 1024, (1, 7, 8, 9, 24, 32), 32, {}, "attn_bf16_kernel[2,4,reg,w8]", None, True),
    ("bf16_2_4_reg_w16", 1024, (33, 64), 64, {}, "attn_bf16_kernel[2,4,reg,w16]", None, True),
    ("bf16_2_4_reg_w16_nw16", 1024, (24,), 64, {"AOCR_ATTN_NW16": "1"}, "attn_bf16_kernel[2,4,reg,w16]", None, True),
    ("bf16_2_8_reg", 1024, (65, 128), 64, {}, "attn_bf16_kernel[2,8,reg,w16]", None, True),
    ("bf16_2_4_stream", 1024, (129, 192, 200), 64, {}, "attn_bf16_kernel[2,4,stream,w16", "stream", True),
    ("reg_2_f32", 512, (1, 63, 64), 64, {}, "attn_reg_kernel[2,f32]", None, False),
    ("reg_1_f32", 256, (1, 63, 64), 64, {}, "attn_reg_kernel[1,f32]", None, False),
    ("core_h32", 32, (8,), 64, {}, "attn_core_kernel[]", None, False),
    ("core_h768", 768, (65,), 64, {}, "attn_core_kernel[]", None, False),
    ("core_h512", 512, (300,), 64, {}, "attn_core_kernel[]", None, False),
    # what the switch reaches: not the fp32-context kernel at (Hd = 512, T <= 64) -- that branch does not test it -- and the generic kernel beyond
    ("no_attn_bf16_h512", 512, (24, 64), 64, {"AOCR_NO_ATTN_BF16": "1"}, "attn_reg_h512_kernel[w16]", None, True),
    ("no_attn_bf16_core", 512, (65,), 64, {"AOCR_NO_ATTN_BF16": "1"}, "attn_core_kernel[]", None, True),
]
FLAT = [(c, T) for c in CASES for T in c[2]]


@pytest.mark.parametrize("case,T", FLAT, ids=[f"{c[0]}-T{T}" for c, T in FLAT])
def test_attention_exact(case, T, monkeypatch, capfd):
    name, Hd, _, chunk, env, kernel, bwd, shadow = case
    setenv(monkeypatch, env)
    if bwd == "stream":
        fwd_kernel = kernel + ",onepass]"
        bwds = [(kernel + ",onepass]", True, {}), (kernel + ",twopass]", True, {"AOCR_ATTN_BWD_TWO_PASS": "1"}), ]
    else:
        fwd_kernel, bwds = kernel, [(kernel, False, {})]
    fwd_bwd(name, Hd, T, chunk, capfd, monkeypatch, fwd_kernel, bwds, shadow, seed=1000 + T)


@pytest.mark.parametrize("T", [17, 64])
def test_attention_h512_ctx_div(T, capfd):
    """ctx_div = 3: batch rows 3 i .. 3 i + 2 read the context of image i (B = 6)."""
    p = Problem(512, T, 64, k=3, nimg=2, seed=2000 + T)
    capfd.readouterr()
    got = run_forward(p.ctx, p.u, 3)
    expect(capfd, "attention_forward", "attn_reg_h512_kernel[w16]")
    report(f"h512 ctx_div=3 T={T} forward", ("a", "c"), check_forward(got, p.a, p.c, 0.5))


# ------------------------------------------------------------------------------------------------------------------------------
# the two-context (DUAL) launchers: Hd = 1024, T <= 64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 24, 32, 33, 64])
def test_attention_dual(T, capfd):
    Hd, chunk = 1024, 32 if T <= 32 else 64
    kernel = "attn_bf16_kernel[2,4,reg,w8,dual]" if T <= 32 else "attn_bf16_kernel[2,4,reg,w16,dual]"
    for k in (1, 2):
        p = Problem(Hd, T, chunk, k=k, seed=3000 + T + 100 * k)           # p.ctx: the planted context the SCORES come from (ctxab)
        ctx = plain_ctx(p.nimg, T, Hd, seed=3500 + T + k)                  # the weighted sum's context
        capfd.readouterr()
        got = run_forward(ctx, p.u, k, ctxab=p.ctx)
        expect(capfd, "attention_forward_dual", kernel)
        report(f"dual T={T} ctx_div={k} forward", ("a", "c"), check_forward(got, p.a, wsum_ref(p.a, ctx, k), 0.5))
    q = Problem(Hd, T, chunk, seed=3700 + T)
    dc, ctxab = ints(q.B, Hd, seed=3800 + T, lo=-2, hi=2).double() * QU, plain_ctx(q.B, T, Hd, seed=3900 + T)
    a32 = q.a.float()
    ref = backward_ref(q.ctx, a32, dc, ctxab)
    capfd.readouterr()
    gb = run_backward(q.ctx, a32, dc, ref, ctxab=ctxab)
    expect(capfd, "attention_backward_dual", kernel)
    report(f"dual T={T} backward", ("ds", "dq", "dh_attn"), check_backward(gb, ref, 0.5))


def test_attention_dual_ok(monkeypatch):
    ok = kp().kp_attention_dual_ok
    x = Buf((8,), torch.bfloat16, fill=0)
    assert ok(64, 1024, x.ptr(), x.ptr()) == 1 and ok(1, 1024, x.ptr(), x.ptr()) == 1
    assert ok(65, 1024, x.ptr(), x.ptr()) == 0
    assert ok(24, 512, x.ptr(), x.ptr()) == 0
    assert ok(24, 1024, x.ptr(), None) == 0 and ok(24, 1024, None, x.ptr()) == 0
    monkeypatch.setenv("AOCR_NO_CHAIN_CTXA", "1")
    assert ok(24, 1024, x.ptr(), x.ptr()) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# beam decode: one workgroup per image, its k hypotheses share every context row that is loaded
# ------------------------------------------------------------------------------------------------------------------------------
BEAM = [("beam_1_8_5", 512, 64, (65, 128, 130), (2, 3, 5), "attn_bf16_beam_kernel[1,8,5]"),
        ("beam_2_4_5", 1024, 32, (65, 96, 100), (2, 5), "attn_bf16_beam_kernel[2,4,5]")]
BEAM_FLAT = [(c, T) for c in BEAM for T in c[3]]


@pytest.mark.parametrize("case,T", BEAM_FLAT, ids=[f"{c[0]}-T{T}" for c, T in BEAM_FLAT])
def test_attention_beam(case, T, monkeypatch, capfd):
    name, Hd, chunk, _, ks, kernel = case
    for k in ks:
        p = Problem(Hd, T, chunk, k=k, nimg=max(2, -(-len(edges(T, chunk)) // k)), seed=4000 + T + 10 * k)
        for env, kern in (({}, kernel), ({"AOCR_NO_ATTN_BEAM_GROUP": "1"}, "attn_bf16_kernel[")):
            setenv(monkeypatch, env)
            capfd.readouterr()
            got = run_forward(p.ctx, p.u, k)
            expect(capfd, "attention_forward", kern)
            report(f"{name} T={T} k={k} images={p.nimg} {'per-row' if env else 'grouped'} forward", ("a", "c"), check_forward(got, p.a, p.c, 0.5))
        monkeypatch.delenv("AOCR_NO_ATTN_BEAM_GROUP")


# ------------------------------------------------------------------------------------------------------------------------------
# random operands: one case per kernel family (guards against the integer data hiding a rounding-order bug)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Hd,T,k,shadow,fwd_kernel,bwd_kernel", [
    ("h512", 512, 63, 1, True, "attn_reg_h512_kernel[w16]", "attn_reg_h512_kernel[w16]"),
    ("bf16_reg", 1024, 100, 1, True, "attn_bf16_kernel[2,8,reg,w16]", "attn_bf16_kernel[2,8,reg,w16]"),
    ("bf16_stream", 512, 300, 1, True, "attn_bf16_kernel[1,4,stream,w16,onepass]", "attn_bf16_kernel[1,4,stream,w16,onepass]"),
    ("beam", 1024, 100, 5, True, "attn_bf16_beam_kernel[2,4,5]", None),
    ("core", 768, 65, 1, False, "attn_core_kernel[]", "attn_core_kernel[]"),
], ids=["h512", "bf16_reg", "bf16_stream", "beam", "core"])
def test_attention_random(name, Hd, T, k, shadow, fwd_kernel, bwd_kernel, capfd):
    nimg = 4 if k == 1 else 2
    B = nimg * k
    ctx = rnd(nimg, T, Hd, seed=5000).float().to(torch.bfloat16).double()
    u = (rnd(B, Hd, seed=5001) * (6.0 / Hd ** 0.5)).float().double()        # var(score) = Hd / 3 * var(u) = 4
    a = softmax_ref(ctx, u, k)
    img = torch.arange(B) // k
    eb = bound(torch.einsum("btj,bj->bt", ctx[img].abs(), u.abs()), Hd).max(1, keepdim=True).values
    capfd.readouterr()
    got = run_forward(ctx, u, k, shadow)
    expect(capfd, "attention_forward", fwd_kernel)
    report(f"random {name} forward", ("a", "c"), check_forward(got, a, wsum_ref(a, ctx, k), ctx.abs().max().item(), eb))
    if bwd_kernel is None:
        return
    dc = (rnd(B, Hd, seed=5002) * (6.0 / Hd ** 0.5)).float().double()
    a32 = softmax_ref(ctx, (rnd(B, Hd, seed=5003) * (6.0 / Hd ** 0.5)).float().double(), 1).float()
    ref = backward_ref(ctx, a32, dc)
    eb = bound(torch.einsum("btj,bj->bt", ctx.abs(), dc.abs()), Hd).max(1, keepdim=True).values
    capfd.readouterr()
    gb = run_backward(ctx, a32, dc, ref, shadow, cfwd=True)
    expect(capfd, "attention_backward", bwd_kernel)
    report(f"random {name} backward", ("ds", "dq"), check_backward(gb, ref, ctx.abs().max().item(), eb))


# ------------------------------------------------------------------------------------------------------------------------------
# attn_dctx_kernel: d(ctx)[b,t,j] = sum_l a[l,b,t] dc[l,b,j] + ds[l,b,t] q[l,b,j]
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,T,Hd", [(1, 1, 32), (32, 64, 96), (33, 65, 96), (70, 130, 512)])
def test_attention_dctx_exact(L, T, Hd, capfd):
    B = 3
    a, ds = ints(L, B, T, seed=6000 + L, lo=-2, hi=2).double() * QU, ints(L, B, T, seed=6001 + L, lo=-2, hi=2).double() * QU
    dc, q = ints(L, B, Hd, seed=6002 + L, lo=-2, hi=2).double() * QC, ints(L, B, Hd, seed=6003 + L, lo=-2, hi=2).double() * QC
    ref = torch.einsum("lbt,lbj->btj", a, dc) + torch.einsum("lbt,lbj->btj", ds, q)
    ad, dsd, qd = Buf(a), Buf(ds), Buf(q)
    dcd = Mat(L * B, Hd, data=dc.reshape(L * B, Hd), pad=Hd)                # the first half of [L][B][2 Hd], junk in the other
    dctx = Buf((B, T, Hd), fill=SENT)
    capfd.readouterr()
    call("kp_attention_dctx", ad.ptr(), dsd.ptr(), vp(dcd.addr), dcd.ld, qd.ptr(), dctx.ptr(), L, B, T, Hd)
    torch.cuda.synchronize()
    expect(capfd, "attention_dctx", "attn_dctx_kernel[]")
    dctx.check_tail("dctx")
    got = dctx.cpu().double()
    bad = got != ref
    print(f"[attn-kernels] test_attention_dctx_exact[{L}-{T}-{Hd}]: {int(bad.sum())} of {bad.numel()} elements differ from float64")
    assert not bad.any(), f"dctx differs from the exact sum at {int(bad.sum())} elements (max {(got - ref).abs().max().item()})"
