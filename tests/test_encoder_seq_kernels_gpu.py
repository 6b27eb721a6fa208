"""GPU: the whole-sequence encoder kernels of the default configuration -- enc_seq_fwd_kernel / enc_seq_bwd_kernel (csrc/rnn_seq.hip) and
enc_cl_fwd_kernel / enc_cl_bwd_kernel (csrc/rnn_cluster.hip) -- called directly through tests/libkprobe.so and held, step by step, to the float64
restatement of tests/enc_seq_ref.py (itself checked on the CPU in tests/test_enc_seq_ref_cpu.py).  Method of
tests/test_kernels_bf16_gpu.py / tests/test_step_kernels_bf16_gpu.py, helpers of tests/kernel_harness.py: sentinel-filled outputs with sentinel tails, JUNK around every strided window,
the configuration each call reached asserted from its AOCR_TRACE line, err[0] == 0 after every cluster call.

DEVICE-FED comparison.  Step t of the reference is computed from the device's OWN saved hsb(t') and cs(t') (backward: from the device's own dzb of the
step processed before), so nothing compounds and every step is a one-step problem: W_h2h entries are integers in [-2, 2] times q = 2^-4 (exact in
bf16), zx is random fp32, >= 90 % of the pre-activations lie inside |z| <= 4 (asserted on the device-fed reference; on the free-running one in the
CPU test), and the states differ by row, step and direction by far more than a tolerance (CPU test).
  forward   c(t), the saved gates and -- where the fp32 h is visible: hs of rnn_seq.hip, ctx of a top layer, hs of a cluster launch's last step --
            h(t) within TOL_CELL + bound(|W| |h_b|, He); hsb(t) bit-exactly the RNE of the device's own fp32 h, or, where that is not visible,
            inside [RNE(h64 - tol), RNE(h64 + tol)].  Initial-state slots, the steps not run yet and every tail keep their sentinels.
  backward  dz (rnn_seq.hip) within TOL_BWD max(1, max |dh|) + bound(|dzb| |W|, 4He) =: tol_step; dzb bit-exactly the RNE of the device's dz, or
            (cluster: no fp32 dz) inside the RNE range of the reference.
  d c       The running d c is not saved per step; the reference carries its own.  Per step d c' = f (dh o (1 - tanh^2 c) + d c) with a forget gate
            f < 1 and every factor of dh at most 1: an error e in d c becomes at most f e < e, and the step adds at most the error of dh (the fp32
            product: bound(...)) plus the cell's own evaluation error, together tol_step.  After n steps |d c - ref| <= n tol_step, which is what the
            final d c is asserted against (the measured worst case is printed).
  bias      dbi / dbh start from a NON-ZERO accumulator a0 and gain the sum of dz over the B valid rows and the n steps.  Every term is within its
            tol_step of the reference's, and the B n + 1 fp32 additions (lane sums, shuffles, atomics, in any order) each round a partial sum of
            magnitude at most S = |a0| + sum |dz|:  |db - ref| <= B n max tol_step + (B n + 1) 2^-23 S.
The free-running distance of the final context (compounded bf16 noise, bounded by nobody) is printed as a [parity] number only.

Branches (B, T, He; the cluster's G = He / 64):
  rnn_seq.hip  (16,1,64) ctx  (32,2,128)  (16,5,256) ctx  (32,5,64)  (16,2,256)  (32,1,128) ctx -- both directions are in every launch
  cluster      G = 1, 2, 4, 8; B = 5 (one ragged group, rh = 16), B = 16 at rh = 8 (two full half-groups), B = 21 ragged at rh = 8 and rh = 16,
               B = 40 with AOCR_ENC_RT2=1 (RT = 2) at G = 2 and 4; T = 1, 2, 3 (first reuse of a parity slot), 7; gslot > 0 at rh = 16 and rh = 8;
               He = 512, B = 70, T = 2 with the compute units reserved down to 64: 8 gids per pass, two launches;
               T = 7 as chunks [0,3) + [3,7) and [0,1) + [1,7) with consecutive epochs, checked as they land and bit for bit against one launch
               (backward: dc_in, the decoder's [B][2 He] layout, given to both chunks and used by the first only);
               AOCR_CL_REMOTE=1 bit-identical to the local exchange, then a second call on the same exchange buffers with epoch + 1 (stale tags);
               rh = 8 against rh = 16 on the same operands: c, hsb, gates, ctx / dzb, final dc bit-identical, bias sums within their bound."""
import ctypes as C
import re

import pytest
import torch

import enc_seq_ref as R
from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module (tests/test_kernel_harness_cpu.py checks it)
from kernel_harness import JUNK, SENT, TOL_BWD, TOL_CELL, Buf, bound, i32, i64, kp, launch, ratio, setenv, sz, trace_of, vp

pytestmark = pytest.mark.gpu

SENT_B = -3.0                       # sentinel of the bf16 outputs (exact in bf16)
ERR_INTS = 16 + 256 * 8 + 4096      # model.hip: cl_err
KNOBS = ("AOCR_ENC_RT2", "AOCR_ENC_RH16", "AOCR_ENC_BWD_RH", "AOCR_CL_REMOTE", "AOCR_SEQ_ABL", "AOCR_SEQ_STAMP")
KP_ENC_UNSUPPORTED, KP_ENC_PLAN_MISMATCH, KP_ENC_BUF_SMALL, KP_ENC_XTAB_SMALL, KP_ENC_ERR_SMALL, KP_ENC_BAD_ARGS = range(2001, 2007)


class EncDir(C.Structure):
    _fields_ = [("w", vp), ("zx", vp), ("hs", vp), ("cs", vp), ("hsb", vp), ("gates", vp), ("ctx", vp), ("reverse", i32)]


class EncBwdDir(C.Structure):
    _fields_ = [("wt", vp), ("dh1", vp), ("dh1_row", i64), ("dh1_t", i64), ("dh2", vp), ("dh2_row", i64), ("dc", vp), ("dc_in", vp), ("dc_in_row", i64),
                ("gates", vp), ("cs", vp), ("dz", vp), ("dzb", vp), ("dbi", vp), ("dbh", vp), ("forward_dir", i32)]


class EncSeqFwd(C.Structure):
    _fields_ = [("d", EncDir * 2), ("B", i32), ("T", i32), ("He", i32), ("Hd", i32)]


class EncSeqBwd(C.Structure):
    _fields_ = [("d", EncBwdDir * 2), ("B", i32), ("T", i32), ("He", i32)]


class EncCl(C.Structure):
    _fields_ = [("B", i32), ("T", i32), ("He", i32), ("Hd", i32), ("groups", i32), ("epoch", C.c_uint), ("it0", i32), ("it1", i32), ("gslot", i32),
                ("buf", vp), ("buf_bytes", sz), ("xtab", vp), ("xtab_bytes", sz), ("err", vp), ("err_ints", sz), ("layers", i32),
                ("G", i32), ("RT", i32), ("reserve_cus", i32), ("concurrent", i32)]


class EncClFwd(C.Structure):
    _fields_ = [("d", EncDir * 2), ("c", EncCl)]


class EncClBwd(C.Structure):
    _fields_ = [("d", EncBwdDir * 2), ("c", EncCl)]


@pytest.fixture(autouse=True)
def _knobs(monkeypatch, _switches):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def config_of(capfd, fn):
    """the one trace line of the call -> its line and its name=value fields"""
    lines = trace_of(capfd, fn)
    assert len(lines) == 1, f"{fn}: expected one dispatch trace line (AOCR_TRACE), got {lines}"
    return lines[0], {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[0])}


def same_bits(a, b):
    if a.dtype == torch.bfloat16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def is_sentinel(t):
    return bool((t == (SENT_B if t.dtype == torch.bfloat16 else SENT)).all())


def in_rne_range(got_b, ref, tol):
    """got (bf16) inside the closed range [RNE(ref - tol), RNE(ref + tol)]"""
    g = got_b.float().double()
    return bool(((g >= R.rne(ref - tol)) & (g <= R.rne(ref + tol))).all())


# ------------------------------------------------------------------------------------------------------------------------------
# problems
# ------------------------------------------------------------------------------------------------------------------------------
class Fwd:
    """One layer, both directions (dir 0 walks t = 0..T-1, dir 1 is `reverse`); layout "seq" | "cl" (saved gates); ctx: the top layer's context."""

    def __init__(self, B, T, He, layout, ctx, seed=0):
        self.B, self.T, self.He, self.layout, self.has_ctx = B, T, He, layout, ctx
        self.W = [R.weights(He, 100 + seed + d) for d in range(2)]
        self.zx = [R.inputs(T, B, He, 200 + seed + d) for d in range(2)]
        self.Wd = [Buf(w, torch.bfloat16) for w in self.W]
        self.zxd = [Buf(z) for z in self.zx]
        self.fresh()

    def fresh(self):
        B, T, He = self.B, self.T, self.He
        self.hs = [Buf((T + 2, B, He), fill=SENT) for _ in range(2)]
        self.cs = [Buf((T + 2, B, He), fill=SENT) for _ in range(2)]
        self.hsb = [Buf((T + 2, B, He), torch.bfloat16, fill=SENT_B) for _ in range(2)]
        self.gates = [Buf((T, B, 4 * He), fill=SENT) for _ in range(2)]
        self.ctx = Buf((B, T, 2 * He), fill=SENT) if self.has_ctx else None

    def dirs(self):
        d = (EncDir * 2)()
        for k in range(2):
            d[k].w, d[k].zx, d[k].hs, d[k].cs = self.Wd[k].full.data_ptr(), self.zxd[k].full.data_ptr(), self.hs[k].full.data_ptr(), self.cs[k].full.data_ptr()
            d[k].hsb, d[k].gates, d[k].reverse = self.hsb[k].full.data_ptr(), self.gates[k].full.data_ptr(), k
            d[k].ctx = self.ctx.full.data_ptr() + k * self.He * 4 if self.ctx else None
        return d

    def outputs(self):
        o = {f"{n}{k}": getattr(self, n)[k].cpu().clone() for n in ("hs", "cs", "hsb", "gates") for k in range(2)}
        if self.ctx:
            o["ctx"] = self.ctx.cpu().clone()
        return o

    def check(self, it0, it1, what, hs_its, untouched_from=None):
        """Device-fed check of iterations [it0, it1) of both directions; hs_its: the iterations whose fp32 h was written to the state slots.
        Everything of the iterations >= untouched_from (default it1), the initial-state slots and the tails must hold their sentinels.
        -> (largest error / tolerance, share of |z| <= 4)"""
        B, T, He = self.B, self.T, self.He
        worst, zs = 0.0, []
        ctx = self.ctx.cpu() if self.ctx else None
        for k in range(2):
            cs, hs, hsb, gates = self.cs[k].cpu(), self.hs[k].cpu(), self.hsb[k].cpu(), self.gates[k].cpu()
            ref = R.forward(self.zx[k], self.W[k], bool(k), fed=dict(hsb=hsb.float(), cs=cs), it0=it0, it1=it1)
            for it, t in zip(range(it0, it1), R.steps(T, bool(k), it0, it1)):
                b = bound(ref["mag"][t], He)
                tol_g, tol_u = TOL_CELL + b, TOL_CELL + b.amax(dim=1)
                w = f"{what} dir {k} step {t}"
                r = max(ratio(cs[t + 1], ref["cs"][t + 1], tol_u), ratio(R.gates_unlayout(gates[t], He, self.layout), ref["gates"][t], tol_g))
                assert r <= 1.0, f"{w}: c / saved gates error / tolerance = {r:.3f}"
                seen = []
                if it in hs_its:
                    seen.append(hs[t + 1])
                else:
                    assert is_sentinel(hs[t + 1]), f"{w}: fp32 h written to a slot the kernel does not own"
                if ctx is not None:
                    seen.append(ctx[:, t, k * He:(k + 1) * He])
                for h in seen:
                    rh = ratio(h, ref["hs"][t + 1], tol_u)
                    assert rh <= 1.0, f"{w}: h error / tolerance = {rh:.3f}"
                    assert same_bits(hsb[t + 1], h.to(torch.bfloat16)), f"{w}: hsb is not the RNE of the kernel's own fp32 h"
                    r = max(r, rh)
                if not seen:
                    assert in_rne_range(hsb[t + 1], ref["hs"][t + 1], tol_u), f"{w}: hsb outside [RNE(h - tol), RNE(h + tol)]"
                worst = max(worst, r)
                zs.append(ref["z"][t].reshape(-1))
            done = {t + 1 for t in R.steps(T, bool(k), 0, it1 if untouched_from is None else untouched_from)}
            for s in range(T + 2):
                if s not in done:
                    assert is_sentinel(cs[s]) and is_sentinel(hs[s]) and is_sentinel(hsb[s]), f"{what} dir {k}: state slot {s} is not this launch's to write"
                    if 1 <= s <= T:
                        assert is_sentinel(gates[s - 1]), f"{what} dir {k}: gates of step {s - 1} written early"
                        assert ctx is None or is_sentinel(ctx[:, s - 1, k * He:(k + 1) * He]), f"{what} dir {k}: context of step {s - 1} written early"
            for nm in ("hs", "cs", "hsb", "gates"):
                getattr(self, nm)[k].check_tail(f"{what} {nm}{k}")
        if self.ctx:
            self.ctx.check_tail(f"{what} ctx")
        share = (torch.cat(zs).abs() <= 4).double().mean().item()
        assert share >= 0.9, f"{what}: only {share:.3f} of the device-fed pre-activations inside |z| <= 4"
        return worst, share

    def parity(self):
        """free-running distance of the final context / h (compounded bf16 noise: a number, not an assertion)"""
        worst = 0.0
        for k in range(2):
            ref = R.forward(self.zx[k], self.W[k], bool(k))
            if self.ctx:
                got = self.ctx.cpu()[:, :, k * self.He:(k + 1) * self.He].transpose(0, 1).double()
            else:
                got = self.hsb[k].cpu()[1:-1].float().double()
                ref["hs"] = R.rne(ref["hs"])
            worst = max(worst, (got - ref["hs"][1:-1]).abs().max().item())
        return worst


class Bwd:
    """BPTT of one layer, both directions (dir 0: forward_dir = 1).  Saved gates and cell states are the fp32 images of the free-running float64
    forward reference.  dh1 is a window of a [B][T][2 He + 8] buffer (two strides), dh2 of a [B][2 He + 8] one, dc_in of a [B][2 He] one."""

    def __init__(self, B, T, He, layout, seed=0, dh2=True, dc_in=False, acc=False):
        self.B, self.T, self.He, self.layout = B, T, He, layout
        Hp = 2 * He + 8
        self.W = [R.weights(He, 300 + seed + d) for d in range(2)]
        fw = [R.forward(R.inputs(T, B, He, 400 + seed + d), self.W[d], bool(d)) for d in range(2)]
        self.g32 = [f["gates"].float() for f in fw]
        self.c32 = [f["cs"].float() for f in fw]
        self.Wt = [Buf(w.t().contiguous(), torch.bfloat16) for w in self.W]
        self.gd = [Buf(R.gates_layout(g, layout)) for g in self.g32]
        self.cd = [Buf(c) for c in self.c32]
        self.dh1 = [R.uniform((T, B, He), 0.5, 500 + seed + d) for d in range(2)]
        host = torch.full((B, T, Hp), JUNK)
        for d in range(2):
            host[:, :, d * He:(d + 1) * He] = self.dh1[d].transpose(0, 1)
        self.dh1d, self.dh1_row, self.dh1_t = Buf(host), T * Hp, Hp
        self.dh2 = self.dh2d = None
        if dh2:                                                      # |dh2| in [2, 3]: added at any other step, or left out, it is 10^4 tolerances
            self.dh2 = [R.uniform((B, He), 0.5, 600 + seed + d) + 2.5 * torch.sign(R.uniform((B, He), 1.0, 610 + seed + d)) for d in range(2)]
            host = torch.full((B, Hp), JUNK)
            for d in range(2):
                host[:, d * He:(d + 1) * He] = self.dh2[d]
            self.dh2d = Buf(host)
        self.dc0 = [R.uniform((B, He), 0.5, 700 + seed + d) for d in range(2)]
        self.dc_ind = Buf(torch.cat(self.dc0, 1)) if dc_in else None          # the decoder's [B][2 He] initial-state gradient
        self.acc0 = [R.uniform((4 * He,), 1.0, 800 + seed + d) for d in range(2)] if acc else None
        self.fresh()

    def fresh(self):
        B, T, He = self.B, self.T, self.He
        self.dc = [Buf((B, He), fill=SENT) if self.dc_ind else Buf(self.dc0[d]) for d in range(2)]
        self.dz = [Buf((T, B, 4 * He), fill=SENT) for _ in range(2)] if self.layout == "seq" else None
        self.dzb = [Buf((T, B, 4 * He), torch.bfloat16, fill=SENT_B) for _ in range(2)]
        self.dbi = [Buf(a) for a in self.acc0] if self.acc0 else None
        self.dbh = [Buf(a) for a in self.acc0] if self.acc0 else None

    def dirs(self):
        d = (EncBwdDir * 2)()
        for k in range(2):
            d[k].wt, d[k].dh1, d[k].dh1_row, d[k].dh1_t = self.Wt[k].full.data_ptr(), self.dh1d.full.data_ptr() + k * self.He * 4, self.dh1_row, self.dh1_t
            if self.dh2d:
                d[k].dh2, d[k].dh2_row = self.dh2d.full.data_ptr() + k * self.He * 4, 2 * self.He + 8
            d[k].dc = self.dc[k].full.data_ptr()
            if self.dc_ind:
                d[k].dc_in, d[k].dc_in_row = self.dc_ind.full.data_ptr() + k * self.He * 4, 2 * self.He
            d[k].gates, d[k].cs, d[k].dzb, d[k].forward_dir = self.gd[k].full.data_ptr(), self.cd[k].full.data_ptr(), self.dzb[k].full.data_ptr(), 1 - k
            if self.dz:
                d[k].dz = self.dz[k].full.data_ptr()
            if self.dbi:
                d[k].dbi, d[k].dbh = self.dbi[k].full.data_ptr(), self.dbh[k].full.data_ptr()
        return d

    def outputs(self):
        o = {f"{n}{k}": getattr(self, n)[k].cpu().clone() for n in ("dc", "dzb") for k in range(2)}
        if self.dbi:
            o.update({f"{n}{k}": getattr(self, n)[k].cpu().clone() for n in ("dbi", "dbh") for k in range(2)})
        return o

    def check(self, it0, it1, what, dc_start=None, acc_start=None):
        """Device-fed check of iterations [it0, it1).  dc_start: the d c entering iteration it0 (default: dc0, the sequence's); acc_start: the bias
        accumulators before this launch, {"dbi": [dir 0, dir 1], "dbh": ...} (default: acc0).  -> dict of the largest error / tolerance per quantity (+ the raw d c drift)"""
        B, T, He = self.B, self.T, self.He
        n = it1 - it0
        out = dict(dz=0.0, dc=0.0, dc_abs=0.0, db=0.0)
        for k in range(2):
            fd = 1 - k
            dzb = self.dzb[k].cpu()
            ref = R.backward(self.W[k], self.g32[k], self.c32[k], self.dh1[k], self.dh2[k] if self.dh2 else None,
                             self.dc0[k] if dc_start is None else dc_start[k], fd, fed_dzb=dzb.float(), it0=it0, it1=it1)
            ts = R.steps(T, bool(fd), it0, it1)
            dhmax = max(1.0, ref["dh"][ts].abs().max().item())
            tol_step = TOL_BWD * dhmax + bound(ref["mag"], 4 * He)                    # [T][B][He]
            for t in ts:
                w = f"{what} dir {k} step {t}"
                tol = tol_step[t].unsqueeze(1).expand(B, 4, He)
                if self.dz:
                    dz = self.dz[k].cpu()[t]
                    r = ratio(dz.view(B, 4, He), ref["dz"][t], tol)
                    assert r <= 1.0, f"{w}: dz error / tolerance = {r:.3f}"
                    out["dz"] = max(out["dz"], r)
                    assert same_bits(dzb[t], dz.to(torch.bfloat16)), f"{w}: dzb is not the RNE of the kernel's own dz"
                else:
                    assert in_rne_range(dzb[t].view(B, 4, He), ref["dz"][t], tol), f"{w}: dzb outside [RNE(dz - tol), RNE(dz + tol)]"
            for t in range(T):
                if t not in R.steps(T, bool(fd), 0, it1):
                    assert is_sentinel(dzb[t]) and (not self.dz or is_sentinel(self.dz[k].cpu()[t])), f"{what} dir {k}: d z of step {t} written early"
            tmax = tol_step[ts].max().item()
            dc = self.dc[k].cpu()
            out["dc_abs"] = max(out["dc_abs"], (dc.double() - ref["dc"]).abs().max().item())
            r = ratio(dc, ref["dc"], n * tmax)
            assert r <= 1.0, f"{what} dir {k}: final dc error / (n tol_step) = {r:.3f}"
            out["dc"] = max(out["dc"], r)
            if self.dbi:
                for nm in ("dbi", "dbh"):
                    a0 = (self.acc0[k] if acc_start is None else acc_start[nm][k]).double()
                    want = a0 + ref["db"].reshape(-1)
                    S = a0.abs() + ref["dz"][ts].abs().sum(dim=(0, 1)).reshape(-1)
                    tol_b = B * n * tmax + (B * n + 1) * 2.0 ** -23 * S
                    r = ratio(getattr(self, nm)[k].cpu(), want, tol_b)
                    assert r <= 1.0, f"{what} dir {k}: {nm} error / bound = {r:.3f}"
                    out["db"] = max(out["db"], r)
                    getattr(self, nm)[k].check_tail(f"{what} {nm}{k}")
            for nm in ("dc", "dzb") + (("dz",) if self.dz else ()):
                getattr(self, nm)[k].check_tail(f"{what} {nm}{k}")
        return out


class Exchange:
    """The exchange buffers of the cluster kernels, sized as model.hip sizes them for `layers` layers, and the plan of the shape."""

    def __init__(self, B, T, He, kind, layers=1, reserve=0):
        G, RT, groups = C.c_int(0), C.c_int(0), C.c_int(0)
        assert kp().kp_enc_cluster_plan(B, He, T, reserve, C.byref(G), C.byref(RT), C.byref(groups)) == 1, "the cluster kernels do not take this shape here"
        self.G, self.RT, self.groups, self.layers, self.reserve = G.value, RT.value, groups.value, layers, reserve
        per = kp().kp_enc_cluster_xbuf_bytes(B, He) if kind == "x" else kp().kp_enc_cluster_pbuf_bytes(B, He)
        self.buf = Buf((layers * per // 8,), torch.int64, fill=0)
        self.xtab = Buf((layers * 4 * ((B + 15) // 16) * 8 + 64,), torch.int64, fill=0)
        self.err = Buf((ERR_INTS,), torch.int32, fill=0)
        self.epoch = 0

    def fill(self, c, p, it0, it1, gslot, concurrent):
        self.epoch += 1
        c.B, c.T, c.He, c.Hd, c.groups, c.epoch, c.it0, c.it1, c.gslot = p.B, p.T, p.He, 2 * p.He, self.groups, self.epoch, it0, it1, gslot
        c.buf, c.buf_bytes, c.xtab, c.xtab_bytes = self.buf.full.data_ptr(), self.buf.n * 8, self.xtab.full.data_ptr(), self.xtab.n * 8
        c.err, c.err_ints, c.layers, c.G, c.RT, c.reserve_cus, c.concurrent = self.err.full.data_ptr(), self.err.n, self.layers, self.G, self.RT, self.reserve, concurrent

    def ok(self, what):
        err = self.err.cpu()
        assert int(err[0]) == 0, f"{what}: a cluster kernel timed out: err = {err[:5].tolist()}"
        for b, nm in ((self.buf, "exchange buffer"), (self.xtab, "xtab"), (self.err, "err")):
            b.check_tail(f"{what} {nm}")


def cl_run(p, ex, capfd, it0=0, it1=0, gslot=0, concurrent=1):
    """one cluster launch of p (Fwd or Bwd) -> the configuration its trace line states"""
    fwd = isinstance(p, Fwd)
    a = EncClFwd() if fwd else EncClBwd()
    a.d = p.dirs()
    ex.fill(a.c, p, it0, it1, gslot, concurrent)
    capfd.readouterr()
    rc = launch("kp_enc_cluster_forward" if fwd else "kp_enc_cluster_backward", a)
    assert rc == 0, f"wrapper / hipGetLastError() = {rc}"
    torch.cuda.synchronize()
    line, cfg = config_of(capfd, "enc_cluster_forward" if fwd else "enc_cluster_backward")
    ex.ok(line)
    kernel = f": enc_cl_fwd_kernel[{ex.G},{ex.RT}{',ctx' if p.has_ctx else ''}] " if fwd else f": enc_cl_bwd_kernel[{ex.G},{ex.RT}] "
    assert kernel in line and f" {p.B} {p.T} {p.He} " in line, line
    return cfg


def expect_cfg(cfg, ex, rh, groups, passes, remote=0):
    assert cfg == dict(G=ex.G, RT=ex.RT, rh=rh, groups=groups, passes=passes, remote=remote), cfg


# ------------------------------------------------------------------------------------------------------------------------------
# rnn_seq.hip
# ------------------------------------------------------------------------------------------------------------------------------
SEQ_CASES = [(16, 1, 64, True), (32, 2, 128, False), (16, 5, 256, True), (32, 5, 64, False), (16, 2, 256, False), (32, 1, 128, True)]
assert {c[:3] for c in SEQ_CASES} <= set(R.SEQ_SHAPES)


@pytest.mark.parametrize("B,T,He,ctx", SEQ_CASES)
def test_seq_forward(B, T, He, ctx, capfd):
    assert kp().kp_enc_seq_supported(B, He) == 1
    p = Fwd(B, T, He, "seq", ctx, seed=B + T)
    a = EncSeqFwd()
    a.d, a.B, a.T, a.He, a.Hd = p.dirs(), B, T, He, 2 * He
    capfd.readouterr()
    assert launch("kp_enc_seq_forward", a) == 0
    torch.cuda.synchronize()
    line, _ = config_of(capfd, "enc_seq_forward")
    assert f": enc_seq_fwd_kernel[{He // 32}{',ctx' if ctx else ''}] {B} {T} {He}" in line, line
    worst, share = p.check(0, T, line, hs_its=set(range(T)))
    print(f"[enc-kernels] {line[7:]}: largest error / tolerance = {worst:.3f}, share of |z| <= 4 = {share:.3f}")
    print(f"[parity] enc_seq_forward B={B} T={T} He={He}: free-running distance of the final {'context' if ctx else 'hsb'} = {p.parity():.3e}")


@pytest.mark.parametrize("B,T,He,dh2", [c[:3] + (i % 2 == 0,) for i, c in enumerate(SEQ_CASES)])
def test_seq_backward(B, T, He, dh2, capfd):
    p = Bwd(B, T, He, "seq", seed=B + T, dh2=dh2)
    a = EncSeqBwd()
    a.d, a.B, a.T, a.He = p.dirs(), B, T, He
    capfd.readouterr()
    assert launch("kp_enc_seq_backward", a) == 0
    torch.cuda.synchronize()
    line, _ = config_of(capfd, "enc_seq_backward")
    assert f": enc_seq_bwd_kernel[{He // 32}] {B} {T} {He}" in line, line
    r = p.check(0, T, line)
    print(f"[enc-kernels] {line[7:]}: dz error / tolerance = {r['dz']:.3f}, final dc drift = {r['dc_abs']:.3e} = {r['dc']:.3f} of its bound")


def test_seq_wrappers_refuse_what_the_model_would_not_launch():
    assert kp().kp_enc_seq_supported(21, 256) == 0 and kp().kp_enc_seq_supported(16, 512) == 0
    p = Fwd(16, 1, 64, "seq", False)
    a = EncSeqFwd()
    a.d, a.B, a.T, a.He, a.Hd = p.dirs(), 21, 1, 64, 128
    assert launch("kp_enc_seq_forward", a) == KP_ENC_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(is_sentinel(v) for v in p.outputs().values())


# ------------------------------------------------------------------------------------------------------------------------------
# rnn_cluster.hip
# ------------------------------------------------------------------------------------------------------------------------------
RH16, BWD8, BWD16, RT2 = {"AOCR_ENC_RH16": "1"}, {"AOCR_ENC_BWD_RH": "8"}, {"AOCR_ENC_BWD_RH": "16"}, {"AOCR_ENC_RT2": "1"}
# (name, B, T, He, ctx, half tiles asked for, switches, rh, groups, layers, layer of the call)
CL_CASES = [
    ("g1_ragged_t1", 5, 1, 64, True, True, {}, 16, 1, 1, 0),
    ("g2_ragged_t3", 5, 3, 128, False, True, {}, 16, 1, 1, 0),
    ("g4_half_t2", 16, 2, 256, True, True, {}, 8, 2, 1, 0),
    ("g4_half_ragged_t7", 21, 7, 256, False, True, {}, 8, 3, 1, 0),
    ("g1_full_ragged_t7", 21, 7, 64, False, False, {}, 16, 2, 1, 0),
    ("g2_rt2_t3", 40, 3, 128, True, True, RT2, 16, 2, 1, 0),
    ("g4_rt2_t2", 40, 2, 256, False, True, RT2, 16, 2, 1, 0),
    ("g8_half_ragged_t3", 21, 3, 512, True, True, {}, 8, 3, 1, 0),
    ("g8_gslot_t7", 5, 7, 512, False, True, {}, 16, 1, 2, 1),
    ("g4_half_gslot_t2", 16, 2, 256, False, True, {}, 8, 2, 2, 1),
]
assert {c[1:4] for c in CL_CASES} <= set(R.CL_SHAPES)


def cl_env(monkeypatch, half, env, fwd):
    setenv(monkeypatch, env)
    setenv(monkeypatch, (RH16 if not half else {}) if fwd else (BWD8 if half else BWD16))


@pytest.mark.parametrize("case", CL_CASES, ids=[c[0] for c in CL_CASES])
def test_cluster_forward(case, monkeypatch, capfd):
    name, B, T, He, ctx, half, env, rh, groups, layers, layer = case
    cl_env(monkeypatch, half, env, True)
    p, ex = Fwd(B, T, He, "cl", ctx, seed=B + T), Exchange(B, T, He, "x", layers)
    assert (ex.G, ex.RT) == (He // 64, 2 if env is RT2 else 1)
    cfg = cl_run(p, ex, capfd, gslot=layer * 2 * ex.groups, concurrent=layers)
    expect_cfg(cfg, ex, rh, groups, 1)
    worst, share = p.check(0, T, name, hs_its={T - 1})
    print(f"[enc-kernels] enc_cluster_forward {name} {cfg}: largest error / tolerance = {worst:.3f}, share of |z| <= 4 = {share:.3f}")
    print(f"[parity] enc_cluster_forward {name}: free-running distance of the final {'context' if ctx else 'hsb'} = {p.parity():.3e}")


@pytest.mark.parametrize("case", CL_CASES, ids=[c[0] for c in CL_CASES])
def test_cluster_backward(case, monkeypatch, capfd):
    name, B, T, He, _, half, env, rh, groups, layers, layer = case
    cl_env(monkeypatch, half, env, False)
    p, ex = Bwd(B, T, He, "cl", seed=B + T, dh2=T != 3, dc_in=T != 2, acc=True), Exchange(B, T, He, "p", layers)
    cfg = cl_run(p, ex, capfd, gslot=layer * 2 * ex.groups, concurrent=layers)
    expect_cfg(cfg, ex, rh, groups, 1)
    r = p.check(0, T, name)
    print(f"[enc-kernels] enc_cluster_backward {name} {cfg}: final dc drift = {r['dc_abs']:.3e} = {r['dc']:.3f} of its bound, "
          f"bias sums error / bound = {r['db']:.2e}")


def two_pass_exchange(kind):
    """He = 512, B = 70, T = 2 with all but 64 compute units reserved: 8 gids per pass, the 10 gids of 16-row groups run as two launches"""
    ex = Exchange(70, 2, 512, kind, reserve=cus() - 64)
    assert (ex.G, ex.RT, ex.groups) == (8, 1, 5)
    return ex


def test_cluster_forward_two_passes(capfd):
    p, ex = Fwd(70, 2, 512, "cl", True, seed=9), two_pass_exchange("x")
    expect_cfg(cl_run(p, ex, capfd), ex, 16, 5, 2)
    worst, share = p.check(0, 2, "two passes", hs_its={1})
    print(f"[enc-kernels] enc_cluster_forward two passes: largest error / tolerance = {worst:.3f}")


def test_cluster_backward_two_passes(capfd):
    p, ex = Bwd(70, 2, 512, "cl", seed=9, dc_in=True, acc=True), two_pass_exchange("p")
    expect_cfg(cl_run(p, ex, capfd), ex, 16, 5, 2)
    r = p.check(0, 2, "two passes")
    print(f"[enc-kernels] enc_cluster_backward two passes: final dc drift = {r['dc_abs']:.3e}, bias sums error / bound = {r['db']:.2e}")


@pytest.mark.parametrize("cut", [3, 1])
def test_cluster_forward_chunks(cut, capfd):
    """T = 7 as [0, cut) + [cut, 7): consecutive epochs, each chunk checked as it lands, the whole bit for bit against one launch"""
    B, T, He = 16, 7, 128
    p, ex = Fwd(B, T, He, "cl", True, seed=3), Exchange(B, T, He, "x")
    expect_cfg(cl_run(p, ex, capfd), ex, 8, 2, 1)
    p.check(0, T, "one launch", hs_its={T - 1})
    whole = p.outputs()
    p.fresh()
    cl_run(p, ex, capfd, 0, cut)
    p.check(0, cut, f"chunk [0,{cut})", hs_its={cut - 1})
    cl_run(p, ex, capfd, cut, T)
    worst, _ = p.check(cut, T, f"chunk [{cut},{T})", hs_its={cut - 1, T - 1})
    parts = p.outputs()
    for k, v in whole.items():
        if k.startswith("hs") and k[2] != "b":                       # the fp32 h of each launch's last step: the chunked run has one more
            t_last = [T, 1][int(k[2])]
            assert same_bits(v[t_last], parts[k][t_last]), k
        else:
            assert same_bits(v, parts[k]), f"{k}: the chunked run differs from the one launch"
    print(f"[enc-kernels] enc_cluster_forward chunks [0,{cut}) + [{cut},{T}): bit-identical to one launch; largest error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("cut", [3, 1])
def test_cluster_backward_chunks(cut, monkeypatch, capfd):
    B, T, He = 16, 7, 128
    setenv(monkeypatch, BWD8)
    p, ex = Bwd(B, T, He, "cl", seed=3, dc_in=True, acc=True), Exchange(B, T, He, "p")
    expect_cfg(cl_run(p, ex, capfd), ex, 8, 2, 1)
    rw = p.check(0, T, "one launch")
    whole = p.outputs()
    p.fresh()
    cl_run(p, ex, capfd, 0, cut)
    p.check(0, cut, f"chunk [0,{cut})")
    mid = p.outputs()
    cl_run(p, ex, capfd, cut, T)                                       # dc_in is still given: only the first chunk may use it
    p.check(cut, T, f"chunk [{cut},{T})", dc_start=[mid["dc0"], mid["dc1"]], acc_start={nm: [mid[nm + "0"], mid[nm + "1"]] for nm in ("dbi", "dbh")})
    parts = p.outputs()
    for k in ("dzb0", "dzb1", "dc0", "dc1"):
        assert same_bits(whole[k], parts[k]), f"{k}: the chunked run differs from the one launch"
    print(f"[enc-kernels] enc_cluster_backward chunks [0,{cut}) + [{cut},{T}): dzb and final dc bit-identical to one launch "
          f"(one launch: dc drift {rw['dc_abs']:.3e}, bias sums error / bound {rw['db']:.2e})")


def test_cluster_forward_remote_and_stale_tags(monkeypatch, capfd):
    B, T, He = 21, 7, 256
    p, ex = Fwd(B, T, He, "cl", True, seed=5), Exchange(B, T, He, "x")
    expect_cfg(cl_run(p, ex, capfd), ex, 8, 3, 1, remote=0)
    p.check(0, T, "local", hs_its={T - 1})
    local = p.outputs()
    for what, env in (("stale tags, epoch + 1", {}), ("remote", {"AOCR_CL_REMOTE": "1"})):
        setenv(monkeypatch, env)
        p.fresh()
        expect_cfg(cl_run(p, ex, capfd), ex, 8, 3, 1, remote=1 if env else 0)     # the same exchange buffers: the tags of the call before are in place
        p.check(0, T, what, hs_its={T - 1})
        now = p.outputs()
        assert all(same_bits(local[k], now[k]) for k in local), f"{what}: differs from the first local run"
    print("[enc-kernels] enc_cluster_forward: epoch + 1 on used exchange buffers and AOCR_CL_REMOTE=1 bit-identical to the local exchange")


def test_cluster_backward_remote_and_stale_tags(monkeypatch, capfd):
    B, T, He = 21, 7, 256
    setenv(monkeypatch, BWD8)
    p, ex = Bwd(B, T, He, "cl", seed=5, acc=True), Exchange(B, T, He, "p")
    expect_cfg(cl_run(p, ex, capfd), ex, 8, 3, 1, remote=0)
    p.check(0, T, "local")
    local = p.outputs()
    for what, env in (("stale tags, epoch + 1", {}), ("remote", {"AOCR_CL_REMOTE": "1"})):
        setenv(monkeypatch, env)
        p.fresh()
        expect_cfg(cl_run(p, ex, capfd), ex, 8, 3, 1, remote=1 if env else 0)
        p.check(0, T, what)
        now = p.outputs()
        assert all(same_bits(local[k], now[k]) for k in ("dzb0", "dzb1", "dc0", "dc1")), f"{what}: differs from the first local run"
    print("[enc-kernels] enc_cluster_backward: epoch + 1 on used exchange buffers and AOCR_CL_REMOTE=1 bit-identical to the local exchange")


@pytest.mark.parametrize("B,T,He", [(21, 7, 256), (21, 3, 512)])
def test_cluster_half_tiles_match_full_tiles(B, T, He, monkeypatch, capfd):
    """rh = 8 against rh = 16 on the same operands: the same arithmetic per row"""
    got = {}
    for rh, groups, fenv, benv in ((8, (B + 7) // 8, {}, BWD8), (16, (B + 15) // 16, RH16, BWD16)):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        setenv(monkeypatch, fenv)
        setenv(monkeypatch, benv)
        f, fx = Fwd(B, T, He, "cl", True, seed=7), Exchange(B, T, He, "x")
        expect_cfg(cl_run(f, fx, capfd), fx, rh, groups, 1)
        f.check(0, T, f"forward rh={rh}", hs_its={T - 1})
        b, bx = Bwd(B, T, He, "cl", seed=7, dc_in=True, acc=True), Exchange(B, T, He, "p")
        expect_cfg(cl_run(b, bx, capfd), bx, rh, groups, 1)
        r = b.check(0, T, f"backward rh={rh}")                          # (the bias sums: each within its bound)
        got[rh] = (f.outputs(), b.outputs(), r)
    for k, v in got[8][0].items():
        assert same_bits(v, got[16][0][k]), f"forward {k}: 8-row groups differ from 16-row groups"
    for k in ("dzb0", "dzb1", "dc0", "dc1"):
        assert same_bits(got[8][1][k], got[16][1][k]), f"backward {k}: 8-row groups differ from 16-row groups"
    print(f"[enc-kernels] cluster rh=8 vs rh=16 B={B} T={T} He={He}: c, h, hsb, gates, ctx / dzb, dc bit-identical; bias sums error / bound = "
          f"{got[8][2]['db']:.2e} / {got[16][2]['db']:.2e}")


def test_cluster_wrappers_refuse_what_the_model_would_not_launch(capfd):
    """every refusal has its own code and launches nothing (the outputs keep their sentinels, no trace line)"""
    B, T, He = 21, 2, 128
    p, ex = Fwd(B, T, He, "cl", False), Exchange(B, T, He, "x")

    def refused(code, **change):
        a = EncClFwd()
        a.d = p.dirs()
        ex.fill(a.c, p, 0, 0, 0, 1)
        for k, v in change.items():
            setattr(a.c, k, v)
        capfd.readouterr()
        assert launch("kp_enc_cluster_forward", a) == code, change
        assert not trace_of(capfd, "enc_cluster_forward")

    refused(KP_ENC_UNSUPPORTED, He=192)
    refused(KP_ENC_UNSUPPORTED, reserve_cus=cus() - 8)                 # fewer than 8 G compute units left
    refused(KP_ENC_PLAN_MISMATCH, G=ex.G * 2)
    refused(KP_ENC_PLAN_MISMATCH, RT=3 - ex.RT)
    refused(KP_ENC_PLAN_MISMATCH, groups=ex.groups + 1)
    refused(KP_ENC_BUF_SMALL, buf_bytes=ex.buf.n * 8 - 8)
    refused(KP_ENC_BUF_SMALL, layers=2, gslot=2 * ex.groups)
    refused(KP_ENC_XTAB_SMALL, xtab_bytes=ex.xtab.n * 8 - 8)
    refused(KP_ENC_ERR_SMALL, err_ints=16 + 256 * 4)
    refused(KP_ENC_BAD_ARGS, gslot=1)
    refused(KP_ENC_BAD_ARGS, it0=2)
    refused(KP_ENC_BAD_ARGS, reserve_cus=-1)
    refused(KP_ENC_BAD_ARGS, epoch=0)
    torch.cuda.synchronize()
    assert all(is_sentinel(v) for v in p.outputs().values())
    b, bx = Bwd(B, T, He, "cl", acc=True), Exchange(B, T, He, "p")
    a = EncClBwd()
    a.d = b.dirs()
    bx.fill(a.c, b, 0, 0, 0, 1)
    a.c.buf_bytes -= 8
    assert launch("kp_enc_cluster_backward", a) == KP_ENC_BUF_SMALL
    torch.cuda.synchronize()
    assert is_sentinel(b.dzb[0].cpu())
