"""GPU: aocr_adam_update (include/aocr.h; csrc/optim.hip) through ctypes, held bit for bit to the numpy restatement tests/adam_ref.py.

Every device buffer is a kernel_harness.Buf of bytes (sentinel tail behind it) with guard bytes in front, so that the operand starts where the
case wants it: the float vectors 4 bytes past a 16-byte boundary, the state and the scratch block 8 bytes past one.  Bit equality is the check
wherever the arithmetic is the element update's (float32, every operation rounded on its own: csrc/Makefile builds optim.hip without
contraction); the norms are sums in the kernel's order and are held to float64 norms within 2^-22 relative (one double-to-float rounding, one
divide and as much again for the order of the sum), and the update is then held to the restatement GIVEN the reported scales."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as R
from kernel_harness import Buf
from page_harness import csrc_constants

pytestmark = pytest.mark.gpu

OFF = [0, 5, 5, 7, 1030, 5001]            # tests/test_tail_kernels_gpu.py's: an empty group, two groups inside one 16-byte block, unaligned heads and tails
N_BUF = 5010                              # the vectors are longer than the last offset: the elements behind it must not move
GUARD = 0x5A
REL = 2.0 ** -22


class Place:
    """`raw` bytes on the device, `lead` guard bytes past a 512-byte aligned allocation, a sentinel tail behind them."""

    def __init__(self, raw, lead):
        host = np.concatenate([np.full(lead, GUARD, np.uint8), np.frombuffer(bytes(raw), np.uint8)])
        self.buf, self.lead, self.nbytes = Buf(torch.from_numpy(host), torch.uint8), lead, len(raw)
        assert self.buf.full.data_ptr() % 16 == 0
        self.addr = self.buf.full.data_ptr() + lead

    def ptr(self, shift=0):
        return C.c_void_p(self.addr + shift)

    def raw(self):
        return self.buf.cpu().numpy()[self.lead:].tobytes()

    def f32(self):
        return np.frombuffer(self.raw(), np.float32)

    def check(self, what):
        self.buf.check_tail(what)
        assert (self.buf.full[:self.lead].cpu().numpy() == GUARD).all(), f"{what}: write in front of the buffer"


def vec(a):
    return Place(np.asarray(a, np.float32).tobytes(), 4)


def values(n, seed, lo=-20, hi=4, zeros=0.05):
    """sign * 2^uniform(lo, hi), a few exact zeros: no intermediate of the update is denormal (a long vector repeats its first 2^20 + 1 values)"""
    if n > 2 ** 20 + 1:
        return np.resize(values(2 ** 20 + 1, seed, lo, hi, zeros), n)
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 2.0 ** rng.uniform(lo, hi, n)
    v[rng.random(n) < zeros] = 0.0
    v = v.astype(np.float32)
    assert np.all((v == 0) | ((np.abs(v) >= 2.0 ** -20) & (np.abs(v) <= 2.0 ** 4)))
    return v


def hyper(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, clip=0.0):
    import aocr
    return aocr.AdamParams(lr, (beta1, beta2), eps, wd, clip)


def ref_kw(p):
    return dict(lr=p.lr, beta1=p.beta1, beta2=p.beta2, eps=p.eps, wd=p.weight_decay)


class Run:
    """one optimizer: parameters, state, scratch and norms on the device; step(g) is one aocr_adam_update"""

    def __init__(self, w0, off, state=None):
        import aocr
        self.lib, self.off, self.n = aocr.lib, list(off), off[5]
        self.w = vec(w0)
        nbytes = self.lib.aocr_adam_state_bytes(self.n)
        assert nbytes == 8 * self.n + 32
        self.state = Place(bytes(nbytes) if state is None else state, 8)
        self.scratch = Place(bytes([0xEE]) * self.lib.aocr_adam_scratch_bytes(), 8)
        self.norms = Place(np.full(15, -12345.0, np.float32).tobytes(), 4)
        self.skip = Place(np.zeros(1, np.int32).tobytes(), 4)

    def call(self, g, p, over=None):
        a = dict(w=self.w.ptr(), g=g.ptr(), state=self.state.ptr(), off=(C.c_int64 * 6)(*self.off), p=None if p is None else C.byref(p), skip=self.skip.ptr(),
                 scratch=self.scratch.ptr(), norms=self.norms.ptr())
        a.update(over or {})
        rc = self.lib.aocr_adam_update(C.c_void_p(torch.cuda.current_stream().cuda_stream), a["w"], a["g"], a["state"], a["off"], a["p"], a["skip"],
                                       a["scratch"], a["norms"])
        torch.cuda.synchronize()
        return rc

    def step(self, g, p):
        import aocr
        g0 = g.raw()
        assert self.call(g, p) == 0, aocr.last_error()
        for b, what in ((self.w, "params"), (g, "grads"), (self.state, "state"), (self.scratch, "scratch"), (self.norms, "norms"), (self.skip, "skip")):
            b.check(what)
        assert g.raw() == g0, "grads were modified"

    def set_skip(self, word):
        self.skip.buf.full[self.skip.lead:self.skip.lead + 4] = torch.from_numpy(np.frombuffer(np.int32(word).tobytes(), np.uint8).copy()).cuda()

    def reported(self):
        nr = self.norms.f32()
        return nr[0:5], nr[5:10], nr[10:15]


def same_as_ref(run, w_ref, st, what):
    w = run.w.f32()
    assert np.array_equal(w[:run.n].view(np.int32), w_ref[:run.n].view(np.int32)), \
        f"{what}: params differ in {(w[:run.n] != w_ref[:run.n]).sum()} elements, max |diff| {np.abs(w[:run.n].astype(np.float64) - w_ref[:run.n]).max():.3e}"
    assert np.array_equal(w[run.n:].view(np.int32), w_ref[run.n:].view(np.int32)), f"{what}: elements behind the last offset moved"
    got, ref = run.state.raw(), st.to_bytes()
    n4 = 4 * run.n
    assert got[:n4] == ref[:n4], f"{what}: m differs"
    assert got[n4:2 * n4] == ref[n4:2 * n4], f"{what}: v differs"
    assert got[2 * n4:] == ref[2 * n4:], f"{what}: tail {np.frombuffer(got[2 * n4:2 * n4 + 16], np.float64)} {np.frombuffer(got[2 * n4 + 16:], np.int64)} != {st.p1, st.p2, st.steps}"


def check_norms(run, w, g, off, clip, what):
    """the reported norms against float64; returns the reported scales"""
    pn, gn, sc = run.reported()
    pn64, gn64 = R.norms64(w[:off[5]], g[:off[5]], off)
    for k in range(5):
        assert abs(pn[k] - pn64[k]) <= REL * pn64[k] and abs(gn[k] - gn64[k]) <= REL * gn64[k], (what, k, pn[k], pn64[k], gn[k], gn64[k])
        if clip > 0 and gn64[k] > clip * (1 + REL):
            assert abs(sc[k] - clip / gn64[k]) <= REL * clip / gn64[k], (what, k, sc[k], clip / gn64[k])
        elif clip == 0 or gn64[k] < clip * (1 - REL):
            assert sc[k] == 1.0, (what, k, sc[k])
    return sc


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_ragged_offsets_three_steps_bit_equal(cuda, wd):
    p = hyper(lr=2.0 ** -6, wd=wd)
    w0 = values(N_BUF, 1)
    run, st, w_ref = Run(w0, OFF), R.State(OFF[5]), w0.copy()
    for t in (1, 2, 3):
        g0 = values(N_BUF, 10 + t)
        run.step(vec(g0), p)
        w_ref[:OFF[5]] = R.step(w_ref[:OFF[5]], g0[:OFF[5]], st, OFF, [1.0] * 5, **ref_kw(p))
        same_as_ref(run, w_ref, st, f"step {t}")
        sc = check_norms(run, w0 if t == 1 else w_prev, g0, OFF, 0.0, f"step {t}")
        assert list(sc) == [1.0] * 5 and run.reported()[0][1] == 0.0 and run.reported()[1][1] == 0.0       # the empty group: norms 0, scale 1
        w_prev = w_ref.copy()
    assert st.steps == 3


def test_grid_stride_seam(cuda):
    """one element more than 16 x threads x workgroups of the launch, all of it in group 3: every workgroup goes round its loop more than once and the
    last block is ragged"""
    k = csrc_constants("optim.hip", ("ADAM_THREADS", "ADAM_WGS_PER_CU", "ADAM_MAX_WGS"))
    wgs = min(torch.cuda.get_device_properties(0).multi_processor_count * k["ADAM_WGS_PER_CU"], k["ADAM_MAX_WGS"])
    n = 16 * k["ADAM_THREADS"] * wgs + 1
    off = [0, 0, 0, 0, n, n]
    p = hyper(lr=2.0 ** -6)
    w0, g0 = values(n, 2), values(n, 3)
    run, st = Run(w0, off), R.State(n)
    run.step(vec(g0), p)
    w_ref = R.step(w0, g0, st, off, [1.0] * 5, **ref_kw(p))
    same_as_ref(run, w_ref, st, "seam")
    pn, gn, sc = run.reported()
    pn64, gn64 = R.norms64(w0, g0, off)
    assert abs(pn[3] - pn64[3]) <= REL * pn64[3] and abs(gn[3] - gn64[3]) <= REL * gn64[3]
    assert [pn[k_] for k_ in (0, 1, 2, 4)] == [0.0] * 4 and list(sc) == [1.0] * 5


def test_clip_both_sides(cuda):
    clip = 1.0
    p = hyper(lr=2.0 ** -6, clip=clip)
    w0, g0 = values(N_BUF, 4), values(N_BUF, 5, lo=-6, hi=2, zeros=0.0)
    for k, want in ((0, 0.5), (2, 0.25), (3, 3.0), (4, 7.0)):             # groups 0 and 2 below the clip, 3 and 4 above it (1 is empty)
        seg = slice(OFF[k], OFF[k + 1])
        g0[seg] = (g0[seg] * (want / np.sqrt((g0[seg].astype(np.float64) ** 2).sum()))).astype(np.float32)
    assert np.all((np.abs(g0[:OFF[5]]) >= 2.0 ** -20) & (np.abs(g0[:OFF[5]]) <= 2.0 ** 4))
    run, st, w_ref = Run(w0, OFF), R.State(OFF[5]), w0.copy()
    for t in (1, 2):
        run.step(vec(g0), p)
        sc = check_norms(run, w_ref, g0, OFF, clip, f"step {t}")
        assert [float(s) == 1.0 for s in sc] == [True, True, True, False, False]
        w_ref[:OFF[5]] = R.step(w_ref[:OFF[5]], g0[:OFF[5]], st, OFF, sc, **ref_kw(p))
        same_as_ref(run, w_ref, st, f"step {t}")


def test_skip_word(cuda):
    p = hyper(lr=2.0 ** -6, clip=1.0)
    w0, g1, g2 = values(N_BUF, 6), values(N_BUF, 7), values(N_BUF, 8)
    run, st, w_ref = Run(w0, OFF), R.State(OFF[5]), w0.copy()
    run.step(vec(g1), p)
    w_ref[:OFF[5]] = R.step(w_ref[:OFF[5]], g1[:OFF[5]], st, OFF, run.reported()[2], **ref_kw(p))
    same_as_ref(run, w_ref, st, "step 1")
    w_img, st_img = run.w.raw(), run.state.raw()
    run.norms = Place(np.full(15, -12345.0, np.float32).tobytes(), 4)
    run.set_skip(7)
    g = vec(g2)
    run.step(g, p)
    assert run.w.raw() == w_img and run.state.raw() == st_img, "a skipped step wrote parameters or state"
    sc = check_norms(run, w_ref, g2, OFF, 1.0, "skipped step")              # ... but its norms
    run.set_skip(0)
    run.step(g, p)
    w_ref[:OFF[5]] = R.step(w_ref[:OFF[5]], g2[:OFF[5]], st, OFF, sc, **ref_kw(p))
    same_as_ref(run, w_ref, st, "the step after the skipped one")
    assert st.steps == 2


def test_two_runs_agree_bit_for_bit(cuda):
    n = 300001
    off = [0, 1001, 70003, 70003, 250000, n]
    p = hyper(lr=2.0 ** -6, wd=0.01, clip=2.0)
    w0, g0 = values(n, 9), values(n, 10, lo=-8, hi=0)
    out = []
    for _ in range(2):
        run = Run(w0, off)
        g = vec(g0)
        run.step(g, p); run.step(g, p)
        out.append((run.w.raw(), run.state.raw(), run.norms.raw()))
    assert out[0] == out[1]
    assert sum(float(s) != 1.0 for s in np.frombuffer(out[0][2], np.float32)[10:]) >= 3, "the case must clip"


def test_rejected_arguments(cuda):
    import aocr
    w0, g0 = values(N_BUF, 11), values(N_BUF, 12)
    run, g = Run(w0, OFF, state=bytes([0xA5]) * (8 * OFF[5] + 32)), vec(g0)
    before = (run.w.raw(), run.state.raw(), run.norms.raw(), run.scratch.raw())

    def bad(**fields):
        p = hyper()
        for k, v in fields.items():
            if k == "reserved":
                p.reserved[1] = v
            else:
                setattr(p, k, v)
        return dict(p=p)

    cases = {"beta1 = 1": bad(beta1=1.0), "eps = 0": bad(eps=0.0), "negative clip": bad(clip=-1.0), "NaN lr": bad(lr=float("nan")),
             "reserved word": bad(reserved=1), "decreasing offsets": dict(off=(C.c_int64 * 6)(0, 5, 4, 7, 1030, 5001)),
             "first offset not 0": dict(off=(C.c_int64 * 6)(1, 5, 5, 7, 1030, 5001)), "misaligned state": dict(state=run.state.ptr(4)),
             "NULL params": dict(w=None), "NULL grads": dict(g=None), "NULL state": dict(state=None), "NULL offsets": dict(off=None),
             "NULL hyperparameters": dict(p=None), "NULL scratch": dict(scratch=None)}
    for what, over in cases.items():
        over = dict(over)
        p = over.pop("p") if "p" in over else hyper()
        assert run.call(g, p, over) != 0, f"{what}: accepted"
        assert aocr.last_error(), f"{what}: no message"
        assert (run.w.raw(), run.state.raw(), run.norms.raw(), run.scratch.raw()) == before, f"{what}: an output was written"
    assert Run(w0, OFF).call(g, hyper(), dict(skip=None, norms=None)) == 0, aocr.last_error()            # the two optional pointers
