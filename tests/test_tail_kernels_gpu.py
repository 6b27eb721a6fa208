"""GPU: the loss, token-sum, optimizer, weight-shadow, beam-search and small elementwise kernels (csrc/ops_misc.hip; project_loss_kernel of
csrc/ops_gemm.hip) against the references of tests/tail_ref.py (checked on the CPU by tests/test_tail_ref_cpu.py), called directly through
tests/libkprobe.so.  Method of tests/test_kernels_bf16_gpu.py and tests/test_step_kernels_bf16_gpu.py, helpers of tests/kernel_harness.py
(call_sync: every call is followed by a device synchronisation): every output and every
+= target has a sentinel tail, every strided buffer padding columns, and both must survive each call; accumulating outputs start from a
non-zero buffer.

Exact cases: operands are small integers (times a power of two), the reference asserts that every partial sum stays below 2^24, so fp32
sums are exact in ANY order (atomics included) and the assertions are bit-exact.  Loss: the tolerances of test_ops_gpu.py::test_logsoftmax_nll
(logp, nll 1e-5; d logits 1e-6 at scale 1/64).  Selection: two candidates of a row are exactly equal by construction or >= 1e-3 apart in
float64 (asserted by the reference), so tokens and parents are asserted equal; scores within the 1e-5 of test_ops_gpu.py::test_beam_select.

Branches and the shapes that reach them:
  token_sort_kernel          rows > 8192 (the two extra loops)                     (L, B) = (9, 1033): 9297 rows
  segsum_sorted_kernel       tokens with 0, 1, 16, 17, 48, 49, 96 rows; PAD with thousands (full chunks, 16-row groups, scalar remainder)
                             second column block: ncols = 1028; V = 2 / E = 4; token strides (1, L) and (B, 1)
  segsum_bias / dlookup / dw accumulate onto non-zero buffers; db2 null; dW a window of ldw = E + 8 columns
  emb_scatter_kernel         2047 rows (one slice, plain +=) / 2048 rows (8 slices, atomics); E = 20, 256 (one row lane), 3 (255 of 256 threads)
  lsm_nll_wave_kernel        V = 39 / ld 40, V = 64 / ld 64, V = 2 / ld 40;  lsm_nll_kernel: V = 65 / ld 72 (two workgroups), V = 200
  project_loss_kernel        rows = 1045 (last tile 21 rows), V = 2 / 39 / 40 (the min(k, V - 1) clamp), Hd = 64 (two column tiles) / 128, PAD rows
  sgd_sumsq / sgd_update     group offsets {0, 5, 5, 7, 1030, 5001}: empty group, 2 elements inside one 16-byte block, unaligned heads and tails
  skip path                  err[0] = 7: sgd_clip_update, adadelta_update, step_snapshot
  shadow_jobs_kernel         64 x 64 (vector), 33 x 70 ld 72 (ragged tiles, scalar), 5 x 3 (scalar), 96 x 32 from a pointer offset by 4 bytes
                             (scalar by misalignment); whole and split in two by tile_off
  beam_select_kernel (logp / fused logits), project_select_kernel   V = 39 / 64 / 2, (kin, kout) = (1,1) (1,5) (5,5) (8,8), Hd = 4 / 260 / 512
                             with ldh = Hd + 4; ties, finished beams, trie (2 children for 5 beams, a node that admits nothing, bit 63), -inf / NaN rows
  gather_rows_many_kernel    width 64, n = 1 / 5 / 8, kin = 1 / k, dstb; fallback gather_rows_kernel + copy2d_bf16_kernel: width 6
  token_rows_kernel          width 8, token stride 3
  backtrace / recognize_gather   Lt = 6, B = 5, k = 1 / 3, T = 70 (two passes of 64 lanes), EOS at step 2, tied final scores, greedy (hist_par null)
  dec_init_kernel            B = 3, He = 8, Hd = 16 / 24, Ld = 2, copy_h 0 / 1, with and without shadows
  zero_many_kernel           0, 5, 16, 4099 bytes and 1 MB in one call
  copy2d_bf16x4_kernel / copy2d_bf16_kernel   cols 64 / 6
  dropout_apply / dropout_apply_b / dpre_kernel   n = 1000 (four workgroups, the last partial), DropSpec.off = 12345
(edit_distance's raised dynamic-LDS limit: tests/test_dict_gpu.py::test_edit_distance_kernel, (B, L) = (3, 300).)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import tail_ref as R
from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module (tests/test_kernel_harness_cpu.py checks it)
from kernel_harness import SENT, Buf, Drop, Mat, bf, bound, call_sync, i32, i64, ints, kp, rnd, sz, vp

pytestmark = pytest.mark.gpu

TOL_LOGP, TOL_NLL, TOL_DLOGITS, LOSS_SCALE = 1e-5, 1e-5, 1e-6, 1.0 / 64      # test_ops_gpu.py::test_logsoftmax_nll
TOL_SCORE = 1e-5                                                              # test_ops_gpu.py::test_beam_select
ISENT = -7


class Trie(C.Structure):
    _fields_ = [("mask", vp), ("base", vp), ("child", vp), ("loc_in", vp), ("loc_out", vp)]


class DecInit(C.Structure):
    _fields_ = [("c0", vp * 4), ("h0", vp * 4), ("hb", vp * 4), ("feed0", vp), ("outb", vp), ("cfw", vp), ("cbw", vp), ("hfw", vp), ("hbw", vp),
                ("B", i32), ("He", i32), ("Hd", i32), ("Ld", i32), ("copy_h", i32)]


_KEEP = []


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    del _KEEP[:]


def P(x):
    """device address of a Buf / Mat / tensor, or null.  The object is kept until the test ends: the address of a temporary would let the caching
    allocator hand its block to the next upload before the kernel has run."""
    if x is None:
        return None
    _KEEP.append(x)
    if isinstance(x, Mat):
        return vp(x.addr)
    if isinstance(x, Buf):
        return x.ptr()
    return vp(x.data_ptr())


def ibuf(t):
    return Buf(torch.as_tensor(t).reshape(-1), torch.int32)


def iout(n):
    return Buf((n,), torch.int32, fill=ISENT)


def same(got, ref, what):
    """bit-exact: fp32 results against a float64 reference that is exact in fp32"""
    assert torch.equal(ref.double().float().double(), ref.double()), f"{what}: the reference is not exact in fp32"
    assert torch.equal(got.float().view(torch.int32), ref.float().view(torch.int32)), f"{what}: max |diff| {(got.double() - ref.double()).abs().max().item()}"


def close(got, ref, tol, what):
    err = (got.double() - ref.double()).abs().max().item()
    print(f"[tail] {what}: max-abs err {err:.3e} (tol {tol:.1e})")
    assert err <= tol, f"{what}: {err} > {tol}"


def layout(tok_rows, L, B, model):
    """tokens of rows r = t * B + b -> (stored tensor, st, sb): [B][L] with strides (1, L) as the model passes them, or [L][B] with (B, 1)"""
    tl = torch.as_tensor(tok_rows).reshape(L, B)
    return (tl.t().contiguous(), 1, L) if model else (tl, B, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# sums by token, lookup-table scatter / gather
# ------------------------------------------------------------------------------------------------------------------------------
def counted_tokens(rows, V, counts, seed):
    """`counts` {token: rows}; every other row is PAD; shuffled"""
    toks = [t for t, c in counts.items() for _ in range(c)]
    assert len(toks) <= rows and all(2 <= t <= V for t in counts)
    toks += [R.PAD] * (rows - len(toks))
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(seed))
    return torch.tensor(toks)[perm]


@pytest.mark.parametrize("L,B,ncols,V,E,counts", [
    (9, 1033, 8, 39, 20, {3: 1, 4: 16, 5: 17, 6: 48, 7: 49, 8: 96, 9: 47, 39: 95, 20: 144, 21: 3}),      # token 2: no row; PAD: 8781
    (7, 11, 1028, 64, 128, {3: 1, 5: 16, 64: 17}),
    (5, 13, 64, 2, 4, {2: 17}),                                                                            # PAD: exactly 48
])
@pytest.mark.parametrize("model_strides", [True, False])
@pytest.mark.parametrize("with_db2", [True, False])
def test_segsum_by_token(L, B, ncols, V, E, counts, model_strides, with_db2):
    rows = L * B
    assert kp().kp_segsum_supported(ncols, V, E) == 1
    tok = counted_tokens(rows, V, counts, seed=L)
    hist = torch.bincount(tok, minlength=V + 1)
    assert all(int(hist[t]) == c for t, c in counts.items())
    stored, st, sb = layout(tok, L, B, model_strides)
    assert torch.equal(R.targets_at(stored, st, sb, L, B), tok)
    dz = ints(rows, ncols, seed=1, lo=-2, hi=2)
    W, lookup = ints(ncols, E, seed=2, lo=-2, hi=2), ints(V, E, seed=3, lo=-2, hi=2)
    init = [ints(ncols, seed=4), ints(ncols, seed=5), ints(V, E, seed=6), ints(ncols, E, seed=7)]
    S_ref = R.token_sums(dz, tok, V)
    db_ref, dlk_ref, dW_ref = R.token_sum_products(S_ref, W, lookup, E)
    dzm, Wm, lk = Mat(rows, ncols, data=dz), Mat(ncols, E, data=W, pad=8), Buf(lookup)
    S, index = Buf((V, ncols), fill=SENT), iout(kp().kp_segsum_index_ints(rows, V))
    db1, db2, dlk = Buf(init[0]), Buf(init[1]), Buf(init[2])
    dW = Mat(ncols, E, pad=8)
    dW.buf.t[:, :E] = init[3].cuda()
    dW.init = dW.buf.cpu().clone()
    assert dW.ld == Wm.ld > E
    call_sync("kp_segsum_by_token", P(dzm), dzm.ld, P(ibuf(stored)), st, sb, L, B, ncols, V, P(S), P(index), P(db1), P(db2) if with_db2 else None, P(Wm),
              Wm.ld, P(lk), E, P(dlk), P(dW))
    for b, nm in ((S, "S"), (index, "index"), (db1, "db1"), (db2, "db2"), (dlk, "dlookup")):
        b.check_tail(nm)
    dW.check("dW")
    same(S.cpu(), S_ref, "S")
    same(db1.cpu(), init[0] + db_ref, "db1")
    same(db2.cpu(), init[1] + (db_ref if with_db2 else 0), "db2")
    same(dlk.cpu(), init[2] + dlk_ref, "dlookup")
    same(dW.win(), init[3] + dW_ref, "dW")
    order = index.cpu()[:rows].long()
    assert torch.equal(order.sort().values, torch.arange(rows)), "order is not a permutation of the rows"
    assert torch.equal(tok[order], tok.sort().values), "order is not grouped by token"


@pytest.mark.parametrize("L,B", [(23, 89), (32, 64)])                # 2047 rows: one slice; 2048: eight slices
@pytest.mark.parametrize("E", [20, 256, 3])
def test_embedding_scatter_and_gather(L, B, E):
    rows, V = L * B, 39
    assert rows in (2047, 2048)
    tok = torch.randint(1, V + 1, (rows,), generator=torch.Generator().manual_seed(E))
    tok[tok == 17] = 1                                               # a row of the table nobody uses
    stored, st, sb = layout(tok, L, B, E != 256)
    demb, init, table = ints(rows, E, seed=1, lo=-2, hi=2), ints(V, E, seed=2), ints(V, E, seed=3)
    d, dt, tokd = Buf(demb), Buf(init), ibuf(stored)
    call_sync("kp_embedding_scatter_accum", P(d), P(tokd), st, sb, P(dt), L, B, E, V)
    dt.check_tail("dtable")
    same(dt.cpu(), init + R.embedding_scatter(demb, tok, V), "dtable")
    out = Buf((rows, E), fill=SENT)
    call_sync("kp_embedding_gather", P(Buf(table)), P(tokd), st, sb, P(out), L, B, E)
    out.check_tail("embedding_gather")
    same(out.cpu(), R.token_rows(table, tok), "embedding_gather")


# ------------------------------------------------------------------------------------------------------------------------------
# beam bookkeeping
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("kin_is_k", [False, True])
@pytest.mark.parametrize("width", [64, 6])
def test_gather_beam_rows_many(n, kin_is_k, width):
    B, k = 3, 4
    kin = k if kin_is_k else 1
    parents = torch.tensor([[2, 2, 0, 3], [3, 1, 1, 0], [0, 0, 0, 0]])                    # repeated and out-of-order rows
    ld = width + (8 if width % 4 == 0 else 3)
    srcs = [Mat(B * kin, width, data=ints(B * kin, width, seed=10 + i, lo=-99, hi=99) + 0.5 * 2.0 ** -8, pad=ld - width) for i in range(n)]
    dsts = [Mat(B * k, width, pad=ld - width) for _ in range(n)]
    dstb = [Mat(B * k, width, torch.bfloat16, pad=ld - width, fill=-3.0) if i % 2 == 0 else None for i in range(n)]
    arr = lambda ms: (vp * n)(*[m.addr if m is not None else None for m in ms])
    call_sync("kp_gather_beam_rows_many", n, arr(srcs), arr(dsts), ld, P(ibuf(parents)), B, kin, k, width, arr(dstb))
    for i in range(n):
        ref = R.gather_rows(srcs[i].win(), parents, B, kin, k)
        dsts[i].check(f"dst {i}")
        assert torch.equal(dsts[i].win(), ref), f"tensor {i}"
        if dstb[i] is not None:
            dstb[i].check(f"dstb {i}")
            assert torch.equal(dstb[i].win().view(torch.int16), bf(ref)), f"bf16 copy {i}"
    one = Mat(B * k, width, pad=5)                                                          # the single-tensor form, another destination stride
    call_sync("kp_gather_beam_rows", P(srcs[0]), ld, P(one), one.ld, P(ibuf(parents)), B, kin, k, width)
    one.check("gather_beam_rows")
    assert torch.equal(one.win(), R.gather_rows(srcs[0].win(), parents, B, kin, k))


def test_token_rows():
    V, width, Rr, stride = 39, 8, 301, 3
    table = ints(V, width, seed=1, lo=-99, hi=99)
    tok = torch.randint(1, V + 1, (Rr,), generator=torch.Generator().manual_seed(2))
    spaced = torch.full((Rr, stride), 99, dtype=torch.int64)
    spaced[:, 0] = tok
    dst = Buf((Rr, width), fill=SENT)
    call_sync("kp_token_rows", P(Buf(table)), P(ibuf(spaced)), stride, P(dst), Rr, width)
    dst.check_tail("token_rows")
    same(dst.cpu(), R.token_rows(table, tok), "token_rows")


def history(Lt, B, k, T):
    """a search history in which the winner changes parent at every step"""
    g = torch.Generator().manual_seed(k)
    hist_tok = torch.randint(4, 39, (Lt, B, k), generator=g)
    hist_par = torch.zeros(Lt, B, k, dtype=torch.int64)
    for t in range(1, Lt):
        for b in range(B):
            for i in range(k):
                hist_par[t, b, i] = (i + 1 + (b + t) % max(k - 1, 1)) % k                  # a shift by 1 .. k - 1: never the same beam twice in a row (k > 1)
    sc_hist = -(torch.arange(1, Lt + 1).double().reshape(Lt, 1, 1) + torch.rand(Lt, B, k, generator=g, dtype=torch.float64)).float().double()
    final = sc_hist[Lt - 1].clone()
    if k > 1:
        final[1, :] = final[1, 1]                                                         # image 1: all tied -> the first
        final[2, k - 1] = final[2].max() + 1.0                                            # image 2: the last beam wins
    attn_hist = ints(Lt, B * k, T, seed=3, lo=0, hi=50).double()
    return hist_tok, hist_par, sc_hist, final, attn_hist


@pytest.mark.parametrize("k", [1, 3])
def test_backtrace_and_recognize_gather(k):
    Lt, B, T = 6, 5, 70
    hist_tok, hist_par, sc_hist, final, attn_hist = history(Lt, B, k, T)
    labels_ref, scores_ref = R.backtrace(hist_tok, hist_par, final)
    if k > 1:
        w = R.winner(final[0])[0]
        chain = [w]
        for t in range(Lt - 1, 0, -1):
            chain.append(int(hist_par[t, 0, chain[-1]]))
        assert all(a != b for a, b in zip(chain, chain[1:])), "the winner does not change parent at every step"
        assert R.winner(final[1])[0] == 0 and R.winner(final[2])[0] == k - 1
    labels, scores = iout(B * Lt), Buf((B,), fill=SENT)
    ht, hp, fs = ibuf(hist_tok), ibuf(hist_par), Buf(final)
    call_sync("kp_beam_backtrace", P(ht), P(hp), P(fs), P(labels), P(scores), Lt, B, k)
    labels.check_tail("labels"); scores.check_tail("scores")
    assert torch.equal(labels.cpu().long().reshape(B, Lt), labels_ref)
    same(scores.cpu(), scores_ref, "scores")
    lab = labels_ref.clone()
    lab[3, 2] = R.EOS                                                                     # image 3 ends at step 2
    lab[4, 0] = R.PAD
    for par in ((hp, hist_par), (None, None))[:1 if k > 1 else 2]:                          # greedy (k = 1): also with hist_par null
        cl_ref, at_ref = R.recognize_gather(lab, par[1], final, sc_hist, attn_hist)
        assert float(cl_ref[3, 3:].abs().max()) == 0.0 and float(at_ref[3, 3:].abs().max()) == 0.0 and float(at_ref[3, 2].abs().max()) > 0
        cl, at = Buf((B, Lt), fill=SENT), Buf((B, Lt, T), fill=SENT)
        call_sync("kp_recognize_gather", P(ibuf(lab)), P(par[0]), P(fs), P(Buf(sc_hist)), P(Buf(attn_hist)), P(cl), P(at), Lt, B, k, T)
        cl.check_tail("char_logp"); at.check_tail("attn")
        same(at.cpu(), at_ref, "attn")
        close(cl.cpu(), cl_ref, 2e-6, "char_logp")                                        # one fp32 subtraction of scores below 8
        only = Buf((B, Lt, T), fill=SENT)
        call_sync("kp_recognize_gather", P(ibuf(lab)), P(par[0]), P(fs), P(Buf(sc_hist)), P(Buf(attn_hist)), None, P(only), Lt, B, k, T)
        same(only.cpu(), at_ref, "attn alone")


# ------------------------------------------------------------------------------------------------------------------------------
# weight shadows, initial decoder state, zero list, bf16 copies, dropout
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_shadow_jobs(split):
    pieces = [(64, 64, 0, 0), (33, 70, 2, 0), (5, 3, 1, 0), (96, 32, 8, 1)]               # (R, C, pad of w, offset of w in floats)
    ws, wbs, wts, keep = [], [], [], []
    for i, (Rr, Cc, pad, off) in enumerate(pieces):
        w = ints(Rr, Cc, seed=20 + i, lo=-200, hi=200) * (1.0 + 2.0 ** -9)                # needs rounding: not exact in bf16
        raw = Buf(torch.full((Rr * (Cc + pad) + off,), 7.0))
        view = raw.full[off:off + Rr * (Cc + pad)].view(Rr, Cc + pad)
        view[:, :Cc] = w.cuda()
        keep.append(raw)
        ws.append((raw.full.data_ptr() + 4 * off, Cc + pad, w.float()))
        wbs.append(Mat(Rr, Cc, torch.bfloat16, pad=4, fill=-3.0))
        wts.append(Mat(Cc, Rr, torch.bfloat16, pad=4 if i != 2 else 1, fill=-3.0))
    assert ws[3][0] % 16 == 4
    n = len(pieces)
    jobs = Buf((n * kp().kp_shadow_job_bytes(),), torch.uint8, fill=0)
    A = lambda vals, t=vp: (t * n)(*vals)
    args = [n, A([w[0] for w in ws]), A([m.addr for m in wbs]), A([m.addr for m in wts]), A([w[1] for w in ws], i64), A([m.ld for m in wbs], i64),
            A([m.ld for m in wts], i64), A([p[0] for p in pieces], i32), A([p[1] for p in pieces], i32), P(jobs)]
    total = i32(-1)
    tiles = sum(math.ceil(p[0] / 32) * math.ceil(p[1] / 32) for p in pieces)
    if split:
        call_sync("kp_shadow_jobs", *args, 0, 5, C.byref(total))                               # 4 tiles of piece 0 + the first of piece 1
        call_sync("kp_shadow_jobs", *args, 5, -1, C.byref(total))
    else:
        call_sync("kp_shadow_jobs", *args, 0, -1, C.byref(total))
    assert total.value == tiles == 4 + 6 + 1 + 3
    jobs.check_tail("job table")
    for i in range(n):
        wb_ref, wtb_ref = R.shadow(ws[i][2])
        wbs[i].check(f"wb {i}"); wts[i].check(f"wtb {i}")
        assert torch.equal(wbs[i].win().view(torch.int16), bf(wb_ref)), f"wb {i}"
        assert torch.equal(wts[i].win().view(torch.int16), bf(wtb_ref)), f"wtb {i}"
        assert not torch.equal(wb_ref, ws[i][2]), "the piece does not exercise rounding"
        keep[i].check_tail(f"w {i}")


@pytest.mark.parametrize("Hd", [16, 24])
@pytest.mark.parametrize("copy_h", [0, 1])
@pytest.mark.parametrize("shadows", [False, True])
def test_dec_init(Hd, copy_h, shadows):
    B, He, Ld = 3, 8, 2
    src = [ints(B, He, seed=30 + i, lo=-99, hi=99) + 2.0 ** -9 for i in range(4)]         # cfw, cbw, hfw, hbw
    c0, h0 = [Buf((B, Hd), fill=SENT) for _ in range(Ld)], [Buf((B, Hd), fill=SENT) for _ in range(Ld)]
    hb = [Buf((B, Hd), torch.bfloat16, fill=-3.0) if shadows else None for _ in range(Ld)]
    feed, outb = Buf((B, Hd), fill=SENT), Buf((B, Hd), torch.bfloat16, fill=-3.0) if shadows else None
    sb = [Buf(s) for s in src]
    a = DecInit()
    for l in range(Ld):
        a.c0[l], a.h0[l], a.hb[l] = c0[l].full.data_ptr(), h0[l].full.data_ptr(), hb[l].full.data_ptr() if shadows else None
    a.feed0, a.outb = feed.full.data_ptr(), outb.full.data_ptr() if shadows else None
    a.cfw, a.cbw, a.hfw, a.hbw = (s.full.data_ptr() for s in sb)
    a.B, a.He, a.Hd, a.Ld, a.copy_h = B, He, Hd, Ld, copy_h
    call_sync("kp_dec_init", C.byref(a))
    c_ref, h_ref = R.dec_init(*[s.float() for s in src], Hd, Ld, copy_h)
    for l in range(Ld):
        for b, nm in ((c0[l], "c0"), (h0[l], "h0"), (hb[l], "hb")):
            if b is not None:
                b.check_tail(nm)
        same(c0[l].cpu(), c_ref[l], f"c0[{l}]"); same(h0[l].cpu(), h_ref[l], f"h0[{l}]")
        if shadows:
            assert torch.equal(hb[l].cpu().view(torch.int16), bf(h_ref[l])), f"hb[{l}]"
    feed.check_tail("feed0")
    assert float(feed.cpu().abs().max()) == 0.0
    if shadows:
        outb.check_tail("outb")
        assert float(outb.cpu().float().abs().max()) == 0.0
    if Hd > 2 * He:
        assert float(c0[0].cpu()[:, 2 * He:].abs().max()) == 0.0


def test_zero_many():
    sizes = [0, 5, 16, 4099, 1 << 20]
    gap = 64                                                                              # 16-byte aligned starts, untouched bytes between the regions
    starts, pos = [], 0
    for s in sizes:
        starts.append(pos); pos += (s + gap + 15) // 16 * 16
    buf = Buf((pos,), torch.uint8, fill=0xA5)
    base = buf.full.data_ptr()
    assert base % 16 == 0
    n = len(sizes)
    call_sync("kp_zero_many", n, (vp * n)(*[base + s for s in starts]), (sz * n)(*sizes))
    buf.check_tail("zero_many")
    ref = torch.full((pos,), 0xA5, dtype=torch.uint8)
    for s, b in zip(starts, sizes):
        ref[s:s + b] = 0
    assert torch.equal(buf.cpu(), ref)


@pytest.mark.parametrize("cols", [64, 6])
def test_copy2d_bf16(cols):
    rows = 37
    src = Mat(rows, cols, data=ints(rows, cols, seed=1, lo=-200, hi=200) * (1.0 + 2.0 ** -9), pad=4)
    dst = Mat(rows, cols, torch.bfloat16, pad=8 if cols == 64 else 3, fill=-3.0)
    call_sync("kp_copy2d_bf16", P(src), src.ld, P(dst), dst.ld, rows, cols)
    dst.check("copy2d_bf16")
    assert torch.equal(dst.win().view(torch.int16), bf(src.win()))


def test_dropout_kernels():
    n, off, p = 1000, 12345, 0.5
    base, thr = R.drop_base_thr(p, 99, 4, 16)
    d = Drop(base, thr, 1.0 / (1.0 - p), off)
    mk = R.drop_mask(p, 99, 4, 16, off, n)
    assert 300 < int((mk != 0).sum()) < 700 and not torch.equal(mk, R.drop_mask(p, 99, 4, 16, 0, n))
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0])
    x = vals[torch.randint(0, 5, (n,), generator=torch.Generator().manual_seed(1))]
    ref = x.double() * mk
    dst, dstb = Buf((n,), fill=SENT), Buf((n,), torch.bfloat16, fill=-3.0)
    call_sync("kp_dropout_apply", P(Buf(x)), P(dst), P(dstb), n, C.byref(d))
    dst.check_tail("dropout dst"); dstb.check_tail("dropout dstb")
    same(dst.cpu(), ref, "dropout_apply")
    assert torch.equal(dstb.cpu().view(torch.int16), bf(ref))
    dst2, dstb2 = Buf((n,), fill=SENT), Buf((n,), torch.bfloat16, fill=-3.0)
    call_sync("kp_dropout_apply_b", P(Buf(x, torch.bfloat16)), P(dst2), P(dstb2), n, C.byref(d))
    dst2.check_tail("dropout_b dst"); dstb2.check_tail("dropout_b dstb")
    same(dst2.cpu(), ref, "dropout_apply_b")
    assert torch.equal(dstb2.cpu().view(torch.int16), bf(ref))
    only_b = Buf((n,), torch.bfloat16, fill=-3.0)
    call_sync("kp_dropout_apply", P(Buf(x)), None, P(only_b), n, C.byref(d))
    assert torch.equal(only_b.cpu().view(torch.int16), bf(ref))
    # d pre: `out` holds the masked value (0, +-1, +-2 -> unmasked 0, +-0.5, +-1); every result is exact
    g1, g2 = ints(n, seed=2, lo=-3, hi=3), ints(n, seed=3, lo=-3, hi=3)
    half = vals[torch.randint(0, 5, (n,), generator=torch.Generator().manual_seed(4))]
    out = (half.double() * mk).float()
    for second in (g2, None):
        ref_d = R.dpre(g1, second, out, mk)
        dp, dpb = Buf((n,), fill=SENT), Buf((n,), torch.bfloat16, fill=-3.0)
        call_sync("kp_dpre_tanh", P(Buf(g1)), P(Buf(second)) if second is not None else None, P(Buf(out)), P(dp), n, P(dpb), C.byref(d))
        dp.check_tail("dpre"); dpb.check_tail("dpreb")
        same(dp.cpu(), ref_d, "dpre_tanh with a mask")
        assert torch.equal(dpb.cpu().view(torch.int16), bf(ref_d))
    plain = Buf((n,), fill=SENT)
    call_sync("kp_dpre_tanh", P(Buf(g1)), P(Buf(g2)), P(Buf(half)), P(plain), n, None, None)
    same(plain.cpu(), R.dpre(g1, g2, half), "dpre_tanh")


# ------------------------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------------------------
def loss_targets(L, Bt, V, seed):
    y = torch.randint(1, V + 1, (L * Bt,), generator=torch.Generator().manual_seed(seed))
    y[::7] = R.PAD
    return y


@pytest.mark.parametrize("L,Bt,V,ld", [(37, 9, 39, 40), (7, 1, 64, 64), (1, 5, 2, 40), (20, 15, 65, 72), (3, 3, 200, 200)])
@pytest.mark.parametrize("model_strides", [True, False])
def test_logsoftmax_nll(L, Bt, V, ld, model_strides):
    rows = L * Bt
    assert rows in (333, 7, 5, 300, 9)
    x = (rnd(rows, V, seed=1) * 3).float().double()
    x[rows // 2, 0], x[rows // 2, 1] = 80.0, -80.0                                          # no NaN from the exponentials
    y = loss_targets(L, Bt, V, 2)
    y[rows // 2] = 2
    stored, st, sb = layout(y, L, Bt, model_strides)
    lp_ref, nll_ref, dl_ref = R.lsm_nll(x, y, LOSS_SCALE)
    xm = Mat(rows, V, data=x, pad=ld - V)
    assert xm.ld == ld
    tok = ibuf(stored)
    for skip in (None, "logp", "dlogits", "nll"):
        lp, dl, nll = Buf((rows, V), fill=SENT), Buf((rows, ld), fill=SENT), Buf((rows,), fill=SENT)
        call_sync("kp_logsoftmax_nll", P(xm), ld, P(tok), st, sb, Bt, P(lp) if skip != "logp" else None, P(dl) if skip != "dlogits" else None,
                  P(nll) if skip != "nll" else None, rows, V, LOSS_SCALE)
        for b, nm in ((lp, "logp"), (dl, "dlogits"), (nll, "nll")):
            b.check_tail(nm)
            if skip == nm:
                assert float((b.cpu() - SENT).abs().max()) == 0.0, f"{nm} written although null was passed"
        if skip != "logp":
            close(lp.cpu(), lp_ref, TOL_LOGP, "logp")
        if skip != "nll":
            close(nll.cpu(), nll_ref, TOL_NLL, "nll")
            assert float(nll.cpu()[y == R.PAD].abs().max()) == 0.0
        if skip != "dlogits":
            d = dl.cpu()
            assert torch.isfinite(d).all()
            close(d[:, :V], dl_ref, TOL_DLOGITS, "dlogits")
            if ld > V:
                assert float(d[:, V:].abs().max()) == 0.0
            assert float(d[y == R.PAD].abs().max()) == 0.0
    nl = Buf(nll_ref.reshape(L, Bt))
    total, gold = Buf((1,), fill=SENT), Buf((Bt,), fill=SENT)
    call_sync("kp_sum_to_scalar", P(nl), rows, P(total))
    call_sync("kp_gold_scores", P(nl), P(gold), L, Bt)
    total.check_tail("sum"); gold.check_tail("gold")
    f = nl.cpu().double()
    close(total.cpu(), f.sum().reshape(1), 1e-6 * max(1.0, float(f.sum())), "sum_to_scalar")          # fp64 sum, one rounding to fp32
    close(gold.cpu(), -f.sum(0), 2.0 ** -22 * L * max(1.0, float(f.sum(0).max())), "gold_scores")    # L fp32 additions


@pytest.mark.parametrize("V", [2, 39, 40])
@pytest.mark.parametrize("Hd", [64, 128])
def test_project_loss(V, Hd):
    k = kp()
    assert k.kp_project_loss_ok(1045, V, Hd) == 1
    assert k.kp_project_loss_ok(1045, 41, Hd) == 0 and k.kp_project_loss_ok(1045, V, 96) == 0 and k.kp_project_loss_ok(1023, V, Hd) == 0
    Bt, L, ld, rows_alloc = 11, 95, 40, 1056
    rows = L * Bt
    assert rows == 1045 and rows % 32 != 0
    out = ints(rows, Hd, seed=1, lo=-1, hi=1)
    wo, bo = ints(V, Hd, seed=2, lo=-2, hi=2) * 2.0 ** -3, ints(V, seed=3, lo=-8, hi=8) * 2.0 ** -3
    y = loss_targets(L, Bt, V, 4)
    stored, st, sb = layout(y, L, Bt, V != 39)
    logits_ref = out.double() @ wo.double().t() + bo.double()
    lp_ref, nll_ref, dl_ref = R.lsm_nll(logits_ref, y, LOSS_SCALE)
    om, wod, bod, tok = Mat(rows, Hd, data=out), Buf(wo), Buf(bo), ibuf(stored)

    def outputs():
        return Mat(rows_alloc, V, pad=ld - V), Mat(rows_alloc, ld, pad=0), Buf((rows_alloc,), fill=SENT), Buf((rows_alloc, Hd), fill=SENT)
    logits, dlog, nll, dout = outputs()
    call_sync("kp_project_loss", P(om), om.ld, P(wod), P(bod), P(logits), P(dlog), ld, P(nll), P(dout), P(tok), st, sb, Bt, rows, V, Hd, LOSS_SCALE)
    logits.check("logits"); dlog.check("dlogits"); nll.check_tail("nll"); dout.check_tail("dout")
    for t, nm in ((logits.win(), "logits"), (dlog.win(), "dlogits"), (dout.cpu(), "dout"), (nll.cpu(), "nll")):
        assert float((t[rows:] - SENT).abs().max()) == 0.0, f"{nm}: rows past the end written"
    same(logits.win()[:rows], logits_ref, "logits")
    close(nll.cpu()[:rows], nll_ref, TOL_NLL, "nll")
    d = dlog.win()[:rows]
    close(d[:, :V], dl_ref, TOL_DLOGITS, "dlogits")
    assert V == ld or float(d[:, V:].abs().max()) == 0.0
    assert float(d[y == R.PAD].abs().max()) == 0.0 and float(nll.cpu()[:rows][y == R.PAD].abs().max()) == 0.0
    dq = R.rne(d[:, :V]).double()                                                          # the product reads d logits as bf16; wo is exact in bf16
    ref_dout = dq @ wo.double()
    mag = dq.abs() @ wo.double().abs()
    err = ((dout.cpu()[:rows].double() - ref_dout).abs() - bound(mag, V)).max().item()
    print(f"[tail] project_loss dout: max (err - bound) {err:.3e}")
    assert err <= 0.0
    # the contract of ops.h: bit-identical to gemm + logsoftmax_nll + gemm on the same operands
    l2, d2, n2, o2 = outputs()
    rc = i32(-1)
    call_sync("kp_gemm", 1, P(om), om.ld, 1, P(wod), Hd, 1, P(l2), ld, rows, V, Hd, P(bod), None, 0, C.byref(rc))
    assert rc.value == 0
    call_sync("kp_logsoftmax_nll", P(l2), ld, P(tok), st, sb, Bt, None, P(d2), P(n2), rows, V, LOSS_SCALE)
    call_sync("kp_gemm", 1, P(d2), ld, 1, P(wod), Hd, 0, P(o2), Hd, rows, Hd, V, None, None, 0, C.byref(rc))
    assert rc.value == 0
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(logits.win()[:rows]), bits(l2.win()[:rows])), "logits differ from gemm"
    assert torch.equal(bits(nll.cpu()[:rows]), bits(n2.cpu()[:rows])), "nll differs from logsoftmax_nll"
    assert torch.equal(bits(dlog.win()[:rows]), bits(d2.win()[:rows])), "dlogits differ from logsoftmax_nll"
    assert torch.equal(bits(dout.cpu()[:rows]), bits(o2.cpu()[:rows])), "dout differs from gemm"


# ------------------------------------------------------------------------------------------------------------------------------
# optimizer
# ------------------------------------------------------------------------------------------------------------------------------
OFF = [0, 5, 5, 7, 1030, 5001]
N_PARAMS = 5010


def sgd_call(p, g, lr, clip, err=None, bn=None, snap=None, bn_n=0, norms=None):
    scratch = Buf((kp().kp_sgd_scratch_bytes(),), torch.uint8, fill=0)
    call_sync("kp_sgd_clip_update", P(p), P(g), (i64 * 6)(*OFF), lr, clip, P(norms), P(scratch), P(err), P(bn), P(snap), bn_n)
    scratch.check_tail("sgd scratch")


def test_sgd_clip_update_exact():
    lr, clip = 2.0 ** -3, 5.0
    p0 = ints(N_PARAMS, seed=1, lo=-64, hi=64) * 2.0 ** -4
    sign = ints(N_PARAMS, seed=2, lo=0, hi=1) * 2 - 1
    g0 = sign * 2.0 ** -4                                                                 # groups 3, 4: norms sqrt(1023) / 16 and sqrt(3971) / 16 < clip
    g0[0:5] = torch.tensor([1.0, -0.5, 0.25, 0.0, -1.0])
    g0[5:7] = torch.tensor([12.0, -16.0])                                                 # |g|^2 = 400 = (4 clip)^2: scale exactly 0.25
    p, g, norms = Buf(p0), Buf(g0), Buf((10,), fill=SENT)
    sgd_call(p, g, lr, clip, norms=norms)
    p.check_tail("params"); g.check_tail("grads"); norms.check_tail("norms")
    ref, nr = R.sgd_groups(p0, g0, OFF, lr, clip)
    assert nr[2][1] == 20.0 and nr[1] == (0.0, 0.0) and all(n[1] < clip for i, n in enumerate(nr) if i != 2)
    assert torch.equal(ref[5:7], p0[5:7].double() - lr * 0.25 * g0[5:7].double()) and torch.equal(ref[OFF[5]:], p0[OFF[5]:].double())
    same(p.cpu(), ref, "params")
    same(g.cpu(), g0, "grads")
    same(norms.cpu(), torch.tensor([v for n in nr for v in n], dtype=torch.float64).float(), "norms")


def test_sgd_clip_update_random():
    lr, clip = 0.1, 5.0
    p0, g0 = rnd(N_PARAMS, seed=3).float(), (rnd(N_PARAMS, seed=4) * 0.3).float()
    g0[5:7] *= 40.0
    p, g = Buf(p0), Buf(g0)
    sgd_call(p, g, lr, clip)
    ref, nr = R.sgd_groups(p0, g0, OFF, lr, clip)
    assert [n[1] > clip for n in nr] == [False, False, False, True, True]                     # both sides of the clip
    tol = 2.0 ** -22 * (p0.double().abs() + lr * g0.double().abs())                         # three fp32 roundings, with or without contraction
    worst = ((p.cpu().double() - ref).abs() / tol.clamp_min(1e-30)).max().item()
    print(f"[tail] sgd random: worst err / tol {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(p.cpu()[OFF[5]:], p0[OFF[5]:])


@pytest.mark.parametrize("opt", ["sgd", "adadelta"])
def test_optimizer_skip_path(opt):
    latch, sticky, bn_n = kp().kp_cl_err_latch(), kp().kp_cl_err_sticky(), 300
    p0, g0 = rnd(N_PARAMS, seed=5).float(), (rnd(N_PARAMS, seed=6) * 0.3).float()
    var0, acc0 = rnd(N_PARAMS, seed=7).abs().float(), rnd(N_PARAMS, seed=8).abs().float()
    bn0, snap0 = rnd(bn_n, seed=9).float(), rnd(bn_n, seed=10).float()
    p, g, var, acc, bn, snap = Buf(p0), Buf(g0), Buf(var0), Buf(acc0), Buf(bn0), Buf(snap0)
    words = torch.zeros(64, dtype=torch.int32)
    words[0] = 7
    err = ibuf(words)

    def step():
        if opt == "sgd":
            sgd_call(p, g, 0.1, 5.0, err, bn, snap, bn_n)
        else:
            call_sync("kp_adadelta_update", P(p), P(g), P(var), P(acc), N_PARAMS, 0.9, 1e-6, 0.0, P(err), P(bn), P(snap), bn_n)
        for b, nm in ((p, "params"), (g, "grads"), (var, "var"), (acc, "acc"), (bn, "bn_state"), (snap, "bn_snap"), (err, "err")):
            b.check_tail(nm)

    step()
    e0, l, s, skip = R.skip_rule(7, 0)
    assert skip
    for b, ref, nm in ((p, p0, "params"), (g, g0, "grads"), (var, var0, "var"), (acc, acc0, "acc"), (bn, snap0, "bn_state"), (snap, snap0, "bn_snap")):
        assert torch.equal(b.cpu().view(torch.int32), ref.view(torch.int32)), f"skipped step: {nm}"
    w = err.cpu()
    assert (int(w[0]), int(w[latch]), int(w[sticky])) == (e0, l, s) == (0, 7, 7)
    assert int(w.abs().sum()) == 14, "another word of the block changed"
    bn.t.copy_(bn0.cuda())                                                                 # the next step moves the statistics again ...
    step()                                                                                 # ... and its update goes through
    e0, l, s, skip = R.skip_rule(0, 7)
    w = err.cpu()
    assert not skip and (int(w[0]), int(w[latch]), int(w[sticky])) == (e0, l, s) == (0, 0, 7)
    assert torch.equal(bn.cpu(), bn0), "bn_state restored although the step was not skipped"
    if opt == "sgd":
        ref, _ = R.sgd_groups(p0, g0, OFF, 0.1, 5.0)
        assert ((p.cpu().double() - ref).abs() <= 2.0 ** -22 * (p0.double().abs() + 0.1 * g0.double().abs())).all()
        assert not torch.equal(p.cpu()[:OFF[5]], p0[:OFF[5]])
    else:
        assert (p.cpu() != p0).float().mean().item() > 0.99 and not torch.equal(var.cpu(), var0) and not torch.equal(acc.cpu(), acc0)


def test_step_snapshot():
    sticky, bn_n = kp().kp_cl_err_sticky(), 300
    bn0 = rnd(bn_n, seed=11).float()
    for code in (0, 5):
        bn, snap = Buf(bn0), Buf((bn_n,), fill=SENT)
        words = torch.zeros(64, dtype=torch.int32)
        words[0], words[sticky] = code, 9
        err = ibuf(words)
        call_sync("kp_step_snapshot", P(bn), P(snap), bn_n, P(err))
        snap.check_tail("bn_snap"); err.check_tail("err")
        assert torch.equal(snap.cpu(), bn0) and torch.equal(bn.cpu(), bn0)
        e0, s = R.snapshot_rule(code, 9)
        w = err.cpu()
        assert (int(w[0]), int(w[sticky])) == (e0, s) and int(w.abs().sum()) == s
    snap = Buf((bn_n,), fill=SENT)
    call_sync("kp_step_snapshot", P(Buf(bn0)), P(snap), bn_n, None)                              # without the word block
    assert torch.equal(snap.cpu(), bn0)


# ------------------------------------------------------------------------------------------------------------------------------
# selection
# ------------------------------------------------------------------------------------------------------------------------------
D_GRID, U_GRID = 2.0 ** -5, 2.0 ** -8             # logits are multiples of D_GRID; beam j's offset is j * U_GRID: candidates of two beams are >= U_GRID apart


def make_trie(V):
    leaf, dead = {}, {}
    if V == 2:
        return {2: {2: dead}}
    a = {R.EOS: leaf, V: None}
    c = {R.EOS: leaf, 9: a}
    a[7], a[V] = c, c
    return {5: a, V: dead}                                                                 # two first tokens; id V = bit V - 1 (bit 63 at V = 64)


def selection_case(B, V, kin, Hd, use_trie):
    """operands whose logits are exact multiples of D_GRID, running scores that put beam j of an image on the grid + j U_GRID, duplicated classes
    and beams (exact ties), finished beams; the first seed whose rows keep the reference's gap (a finished beam's PAD sits off the grid)"""
    trie = None
    if use_trie:
        mask, base, child, _ = R.flat_trie(make_trie(V))
        trie = (mask, base, child)
    for seed in range(400):
        h, wo = ints(B * kin, Hd, seed=seed, lo=-2, hi=2), ints(V, Hd, seed=seed + 1000, lo=-2, hi=2) * D_GRID
        bo = ints(V, seed=seed + 2000, lo=-8, hi=8) * D_GRID
        if V >= 4:
            wo[V - 1], bo[V - 1] = wo[2], bo[2]                                            # class V ties with class 3 in every row
        rows = torch.arange(B * kin).reshape(B, kin)
        if kin >= 3:
            h[rows[:, 2]] = h[rows[:, 0]]                                                  # beam 2 = beam 0
        logits = h.double() @ wo.double().t() + bo.double()
        assert torch.equal(logits.float().double(), logits)
        prev = loc_in = None
        bs = torch.zeros(B, kin)
        if kin > 1:
            lse = torch.logsumexp(logits, 1).reshape(B, kin)
            j = torch.arange(kin).double().repeat(B, 1)
            m = ints(B, kin, seed=seed + 3000, lo=-3, hi=3).double()
            if kin >= 3:
                j[:, 2], m[:, 2] = j[:, 0], m[:, 0]
            bs = (lse + m * D_GRID + j * U_GRID).float()
            prev = torch.full((B, kin), 5)
            prev[1, 1], prev[3, 0] = R.PAD, R.EOS
            if kin >= 3:
                prev[3, 2] = R.EOS
            prev = prev.reshape(-1)
            if use_trie:
                loc_in = (torch.arange(B * kin) % len(trie[0])).reshape(B, kin)
                if kin >= 3:
                    loc_in[:, 2] = loc_in[:, 0]
                loc_in = loc_in.reshape(-1)
        tot = R.beam_totals(torch.log_softmax(logits, 1), prev, bs, B, kin, V, trie, loc_in)
        if min(R.min_gap(r.tolist()) for r in tot) >= R.GAP:
            return dict(h=h, wo=wo, bo=bo, logits=logits, prev=prev, bs=bs, trie=trie, loc_in=loc_in)
    raise AssertionError("no seed keeps the gap")


def run_selection(form, case, B, V, kin, kout, Hd):
    prev, trie = case["prev"], case["trie"]
    n = B * max(kin, kout)
    scores = Buf(torch.cat([case["bs"].reshape(-1), torch.full((n - B * kin,), SENT)]))
    toks, pars, sc_out, loc_out = iout(B * kout), iout(B * kout), Buf((B, kout), fill=SENT), iout(B * kout)
    keep = [ibuf(prev) if prev is not None else None]
    tv = None
    if trie is not None:
        keep += [Buf(torch.from_numpy(trie[0].astype(np.int64)), torch.int64), ibuf(torch.from_numpy(trie[1])), ibuf(torch.from_numpy(trie[2])),
                 ibuf(case["loc_in"]) if case["loc_in"] is not None else None]
        tv = Trie(keep[1].full.data_ptr(), keep[2].full.data_ptr(), keep[3].full.data_ptr(), keep[4].full.data_ptr() if keep[4] else None,
                  loc_out.full.data_ptr())
    tvp = C.byref(tv) if tv is not None else None
    if form == "logp":
        lp = Buf(case["logp"] if "logp" in case else torch.log_softmax(case["logits"], 1))
        call_sync("kp_beam_select", P(lp), P(keep[0]), P(scores), P(toks), P(pars), B, kin, kout, V, None, 0, tvp, P(sc_out))
    elif form == "logits":
        lg = Mat(B * kin, V, data=case["logits"], pad=3)
        call_sync("kp_beam_select", None, P(keep[0]), P(scores), P(toks), P(pars), B, kin, kout, V, P(lg), lg.ld, tvp, P(sc_out))
    else:
        hm = Mat(B * kin, Hd, data=case["h"], pad=4)
        assert hm.ld == Hd + 4
        call_sync("kp_project_select", P(hm), hm.ld, P(Buf(case["wo"])), P(Buf(case["bo"])), Hd, P(keep[0]), P(scores), P(toks), P(pars), B, kin, kout, V, tvp,
                  P(sc_out))
    for b, nm in ((scores, "beam_scores"), (toks, "tokens"), (pars, "parents"), (sc_out, "sc_out"), (loc_out, "loc_out")):
        b.check_tail(nm)
    return toks.cpu().long().reshape(B, kout), pars.cpu().long().reshape(B, kout), scores.cpu()[:B * kout].reshape(B, kout), sc_out.cpu(), \
        loc_out.cpu().long().reshape(B, kout), scores.cpu()[B * kout:]


@pytest.mark.parametrize("V", [39, 64, 2])
@pytest.mark.parametrize("kin,kout", [(1, 1), (1, 5), (5, 5), (8, 8)])
@pytest.mark.parametrize("Hd", [4, 260, 512])
@pytest.mark.parametrize("use_trie", [False, True])
def test_selection(V, kin, kout, Hd, use_trie):
    B = 5
    case = selection_case(B, V, kin, Hd, use_trie)
    t_ref, p_ref, v_ref, l_ref = R.beam_step(torch.log_softmax(case["logits"], 1), case["prev"], case["bs"], B, kin, kout, V, case["trie"], case["loc_in"])
    if use_trie and kout == 5 and kin == 1 and V > 2:
        assert all(len(set(r)) == 2 and r[2:] == [r[0]] * 3 for r in t_ref.tolist()), "two admissible first tokens: the best is repeated"
    if use_trie and V == 64 and (kin, kout) == (1, 5):
        assert (t_ref == 64).all(1).logical_not().all() and (t_ref == 64).any(), "no selected child on bit 63"
    if kin >= 3 and not use_trie:
        tied = sum(1 for b in range(B) for i in range(kout - 1) if float(v_ref[b, i]) == float(v_ref[b, i + 1]))
        assert tied > 0, "no exact tie among the selected candidates"
    for form in ("logp", "logits", "project"):
        toks, pars, sc, sc2, loc, rest = run_selection(form, case, B, V, kin, kout, Hd)
        assert torch.equal(toks, t_ref), (form, toks, t_ref)
        assert torch.equal(pars, p_ref), (form, pars, p_ref)
        close(sc, v_ref, TOL_SCORE, f"{form} scores")
        assert torch.equal(sc2.view(torch.int32), sc.view(torch.int32)), f"{form}: sc_out is not a copy of the new scores"
        if use_trie:
            assert torch.equal(loc, l_ref), (form, loc, l_ref)
        else:
            assert int((loc - ISENT).abs().max()) == 0
        if len(rest):
            assert float((rest - SENT).abs().max()) == 0.0


@pytest.mark.parametrize("form", ["logp", "logits", "project"])
def test_selection_inf_and_nan_rows(form):
    B, V, kin, kout, Hd = 5, 39, 2, 3, 8
    case = selection_case(B, V, kin, Hd, False)
    lg, h = case["logits"].clone(), case["h"].clone()
    lg[2:4], lg[4:6] = -math.inf, math.nan
    h[2:4], h[4:6] = math.inf, math.nan                                                    # project: inf * weights of both signs = NaN logits
    lp = torch.log_softmax(case["logits"], 1)
    lp[2:4], lp[4:6] = -math.inf, math.nan                                                 # image 1: all -inf, image 2: all NaN
    bad = dict(case, logits=lg, h=h, logp=lp)
    toks, pars, sc, sc2, loc, rest = run_selection(form, bad, B, V, kin, kout, Hd)
    assert int(toks.min()) >= 1 and int(toks.max()) <= V and int(pars.min()) >= 0 and int(pars.max()) < kin
    good = R.beam_step(torch.log_softmax(case["logits"][:2], 1), case["prev"][:2], case["bs"][:1], 1, kin, kout, V)
    assert torch.equal(toks[:1], good[0]) and torch.equal(pars[:1], good[1])                # the healthy image is unaffected
