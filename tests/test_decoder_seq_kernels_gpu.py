"""GPU: the whole-sequence decoder kernels of the default configuration -- dec_ch_fwd_kernel / dec_ch_bwd_kernel (csrc/dec_chain.hip) and
dec_cl_fwd_kernel / dec_cl_bwd_kernel (csrc/dec_cluster.hip) -- called directly through tests/libkprobe.so (the PUBLIC launchers: AOCR_NO_DEC_CHAINS*
choose the kernel as in the model) and held, step by step, to the float64 restatement of tests/dec_seq_ref.py (itself held to oracle_torch and
autograd on the CPU in tests/test_dec_seq_ref_cpu.py).  Method of tests/test_encoder_seq_kernels_gpu.py, helpers of tests/kernel_harness.py: outputs
sentinel-filled with sentinel tails, the token table read through a strided window with JUNK around it, err[0] == 0 and untouched exchange / xtab / err
tails after every call, the kernel, instantiation, groups and passes of every call asserted from its AOCR_TRACE line (per_pass from the device's
compute-unit count, as the launchers compute it).

DEVICE-FED comparison.  Every stage of step t of the reference takes the device's OWN saved inputs of that stage, so nothing compounds:
  forward   layer 1 from out_b[t], hsb[l][t], cs[l][t]; layer 2 from the device's hsb[0][t+1]; the attention from the device's hsb[1][t+1]; out from the
            device's cat_b[t].  c1, c2 and the saved gates within TOL_CELL + bound(|W| |x|, 1024); hsb inside [RNE(h - tol), RNE(h + tol)]; a_all within
            TOL_A + bound(|ctxa| |h2|, 512); the c half of cat_b in the RNE range of TOL_C max|ctx| + 2 bound, its h2 half bit-equal to hsb[1]; out within
            TOL_CELL + bound(|W_c| |cat_b|, 1024); out_b bit-equal to the RNE of the device's own out.  Slot 0 keeps the initial state (out: its
            sentinel), gates == nullptr (the gold pass) changes no other output, chain and cluster kernels agree bit for bit.
  backward  saved gates, cs, a_all, out = the fp32 images of the free-running float64 forward reference; every carry but d c is a product of the device's
            own dzb(t+1), which the reference takes as input.  tol_step = TOL_BWD max(1, max |dh|) + bound(|dzb| |W|, 2048): dpre, dz[l] and the c half
            of dcat at tol_step (its h half keeps the sentinel); dpre_b, dzb[l], dq_b bit-equal to the RNE of the device's fp32 value; ds_all / dq at the
            attention test's TOL_DS / TOL_DQ scaling plus the bound of d a; dc_st[l] within L tol_step (the d c argument of the encoder test: the forget
            gate damps an error in d c, every step adds at most tol_step); dh_rec[l], dfeed within tol_step of the products of the device's own step-0 dzb.
The free-running distance of the final out is printed as a [parity] number only.

Shapes (B, T, L): (1,1,1) (7,15,2) (16,16,3: the second chain wholly beyond B) (17,17,3) (32,64,2) (33,65,3: two groups, ctx W_a tile not resident)
(45,5,5) (5,256,2) (32 per_pass + 4, 3, 2: two passes); zx1 as the [L][B][4Hd] tensor for every other shape and as the per-token table read through
token strides for the rest, (17,17,3) both ways bit-identically; AOCR_CH_NO_RES=1 at T = 16, 64; AOCR_CL_REMOTE=1 and epoch + 1 on used buffers.

Dropout (cluster kernels only, (45,5,3) at p = 0.25): masks from tail_ref.drop_mask (the restatement of DropSpec); out and hm_b are exactly zero where
the mask drops; hm_b lies in the RNE range of mask x the float64 h1 and within one bf16 rounding of mask x the device's hsb[0] (a bit-exact statement is
not possible: the kernel rounds 4/3 x the fp32 h1, which is saved only as bf16); the trace shows dec_cl_*_kernel[...,drop] although the chains are enabled.
Greedy decode (DEC, HIST; (45,5,12) and (33,65,6), seeds chosen with the free-running CPU reference): stage 1 -- the teacher-forced kernel on greedy's own
tokens gives bit-identical hsb / out_b up to each row's last live step (measured mismatch share: 0); stage 2 -- every label in the reference's arg-max set
{logp >= max - 2 tol} (cut by the trie node's child mask with a dictionary), margins > 2 tol except the planted twin classes, which go to the lower id,
scores = the running sum within (t + 1) tol, PAD at no cost after EOS / PAD; AOCR_NO_DEC_EARLY=1 bit-identical; chain and AOCR_NO_DEC_CHAINS_GREEDY=1;
sc_hist bit-equal to the final score at the row's last live step; tok0 / labels are windows of row stride L + 3 with JUNK / sentinels around them.
dh_rec / dfeed use TOL_BWD max(1, max |product|) + bound, dc_st one scalar L max tol_step: the step's tol_step with the quantity that is visible there.

Measured on an MI355X (256 compute units: per_pass = 8), largest error / tolerance; chain and cluster kernels give the same figures (bit-identical outputs):
  forward (B-T-L)   c      gates  a      out    [parity] final out      backward   dpre   dcat   ds     dq     dz     dc     rec
  1-1-1             0.001  0.001  0.000  0.001  9.2e-08                            0.000  0.000  0.000  0.000  0.000  0.000  0.000
  7-15-2            0.001  0.001  0.000  0.002  3.4e-07                            0.001  0.000  0.004  0.003  0.000  0.000  0.001
  16-16-3           0.001  0.001  0.000  0.002  3.7e-03                            0.001  0.001  0.004  0.003  0.001  0.000  0.001
  17-17-3           0.001  0.001  0.001  0.002  3.5e-03                            0.001  0.001  0.003  0.004  0.001  0.000  0.001
  32-64-2           0.001  0.002  0.000  0.002  1.3e-03                            0.001  0.000  0.001  0.002  0.000  0.000  0.001
  33-65-3           0.002  0.001  0.000  0.002  2.5e-03                            0.001  0.000  0.002  0.002  0.001  0.000  0.001
  45-5-5            0.002  0.001  0.001  0.001  6.4e-03                            0.001  0.000  0.009  0.006  0.001  0.000  0.001
  5-256-2           0.001  0.001  0.000  0.002  2.3e-04                            0.000  0.001  0.000  0.001  0.000  0.000  0.001
  260-3-2 (2 passes) 0.002 0.002  0.001  0.001  4.6e-03                            0.000  0.001  0.010  0.008  0.000  0.000  0.001
(The tolerances are those of the per-step kernel tests, whose constants bound the transcendental functions of any fp32 cell; a one-step fp32 product is far
inside them.  A swapped f / o gate in the reference fails every forward and backward case.)
  dropout 45-5-3    forward c 0.002  gates 0.001  a 0.001  out 0.001  [parity] 6.2e-03;  backward dpre 0.001  dcat 0.000  ds 0.009  dq 0.007  dz 0.001  dc 0.000  rec 0.001
  greedy 45-5-12    stage 1 mismatch share 0;  final score error / (n tol) 0.000;  planted ties won 48;  hist: running score 0.002, a_all 0.000;
                    dictionary: score 0.003, 142 steps with the free arg-max masked   (chain [dec,res(,hist)] and cluster [dec(,hist)] alike)
  greedy 33-65-6    stage 1 mismatch share 0;  score 0.001;  ties won 5;  hist: running score 0.002, a_all 0.000;  dictionary: score 0.002, 79 steps masked
Beam search (dec_chain_beam_forward: DEC + BEAM [+ HIST] through kp_dec_chain_beam_forward; cases R.BEAM_CASES + the XCD-cap shape, seeds chosen with the free-running
CPU reference R.beam).  Buffers as above plus hist_tok / hist_par / beam_scores / sc_hist / the [L][B k][T] attention history, all sentinel-filled; pbuf / xtab sized
for max(B, 32 group_cap) rows as in model.hip.  labels / scores KEEP their sentinel: the beam launcher does not write them (model.hip's back-trace does), and so do
out, the gates, cs behind slot 0 and everything of hsb / out_b / cat_b behind the initial rows and the four rolling step slots.  Stage 1 -- the hypothesis tree is
rebuilt from the device's own hist_tok / hist_par and every distinct maximal token prefix runs as one row of the teacher-forced kernel (rp.check applied; the XCD-cap
case replays group by group and applies rp.check to the first and last image of each pass only): the HIST attention rows (row image * kin + hypothesis, kin = 1 at step
0, the other rows sentinel) and the surviving rolling slots of the last min(4, L) steps (hsb[0], hsb[1], out_b, the h half of cat_b; groups of the last pass) are
BIT-EQUAL to the replay: product_sum adds the four partial tiles in product's order (mismatch shares 0 in every case).  Stage 2 -- tail_ref.beam_totals of the float64
logprobs of the replay's fp32 out, the device's own previous sc_hist row, tokens and trie nodes, tol = TOL_CELL + bound(|out| . |W_o|, 512) of the parent row: every
pick >= the k-th best - 2 tol, scores non-increasing, exact ties in index order, score within tol of the picked candidate's total, PAD after a finished parent at the
parent's score bits, the repeat-the-best fallback bit for bit, and every DECIDED rank (no other candidate value within 2 tol above or below) equal to the reference's;
undecided ranks (next value below within 2 tol) <= 2 % of a case.  beam_scores = sc_hist[L-1] in bits; no-history, AOCR_CL_REMOTE=1, AOCR_CH_NO_RES=1 (T <= 64) and a
second call on the used buffers (epoch advanced by the pass count) give bit-identical histories; kp_beam_backtrace = tail_ref.backtrace; recognize_gather finite and
summing to sc_hist on the winner.
  beam (B-T-L-k)       groups/passes  replay rows  a_all  a_all / slot mismatch share  score increment  undecided (loose)  ties won  fallback selections  steps masked
  16-5-8-2             1/1            64           0.000  0 / 0                        0.006            0.0078 (0.0156)    3         0                    0
  5-17-26-3            1/1            53           0.000  0 / 0                        0.004            0.0077 (0.0154)    2         0                    0
  11-16-12-3           2/2            90           0.000  0 / 0                        0.007            0.0000 (0.0000)    1         0                    0
  11-16-24-3           2/1            129          0.000  0 / 0                        0.004            0.0025 (0.0051)    1         0                    0
  7-65-20-5            2/2            145          0.000  0 / 0                        0.004            0.0029 (0.0043)    2         0                    0
  9-64-16-7            3/3            215          0.000  0 / 0                        0.004            0.0050 (0.0089)    5         0                    0
  11-16-12-3 dict-6ga  2/2            80           0.000  0 / 0                        0.009            0.0051 (0.0126)    90        11                   127
  9-64-16-7 dict-6g    3/3            132          0.000  0 / 0                        0.010            0.0069 (0.0069)    711       9                    144
  11-16-12-3 eos       2/2            81           0.000  0 / 0                        0.004            0.0000 (0.0000)    1         0                    0
  33-5-32-8 (cap 8)    9/2            1287         0.000  0 / 0                        0.006            0.0049 (0.0089)    19        0                    0
(loose: the share of ranks that get the membership check only -- the undecided ones and those whose next value ABOVE is within 2 tol, which the device may have
swapped with an undecided neighbour; the 2 % cap is on the undecided share.)  The "dict" cases are word lists (R.beam_words: R.words over a small alphabet behind
the two twin characters) through dict_oracle.load_dictionary and tail_ref.flat_trie, ~20000 nodes; the test requires that the hypotheses of an image sit at nodes
with different child sets after at least a quarter of the selections, so that a node taken from the wrong slot, a wrong trie_base or a wrong child offset shows in
the admissibility of later picks.  The XCD-cap case takes its 33 images as rows of a 256-image batch of the same generator (R.BEAM_CAP_ROWS).
Before `#pragma clang fp contract(off)` in the forward cell bodies the cluster kernel's DEC instantiation differed from the teacher-forced kernels (f c + i g
contracted differently): 18372 of 772608 bf16 trajectory values at 45-5-12 (one-ulp flips, compounded along the row), 2 of 251904 at 33-65-6; now 0.
Before `#pragma clang fp contract(off)` in the two cell_bwd bodies the BPTT kernels differed: at 45-5-5, 4559 of 92160 d z values per step by one fp32 ulp and
1 of 92160 dzb values, from which a whole row of dpre of the next step differed; now 0.
"""
import ctypes as C
import re

import pytest
import torch

import dec_seq_ref as R
import tail_ref as TR
from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module (tests/test_kernel_harness_cpu.py checks it)
from kernel_harness import (JUNK, SENT, TOL_A, TOL_BWD, TOL_C, TOL_CELL, TOL_DQ, TOL_DS, Buf, Drop, bound, i32, i64, kp, launch, ratio, setenv, sz, vp)

pytestmark = pytest.mark.gpu

H, V = R.H, R.V
SENT_B = -3.0                       # sentinel of the bf16 outputs (exact in bf16)
ERR_INTS = 16 + 256 * 8 + 4096      # model.hip: cl_err
KP_DEC_UNSUPPORTED, KP_DEC_XBUF_SMALL, KP_DEC_PBUF_SMALL, KP_DEC_XTAB_SMALL, KP_DEC_ERR_SMALL, KP_DEC_BAD_ARGS = range(2101, 2107)
CLUSTER = {"AOCR_NO_DEC_CHAINS": "1"}


class DecFwd(C.Structure):
    _fields_ = [("B", i32), ("T", i32), ("L", i32), ("Hd", i32), ("epoch", C.c_uint), ("greedy", i32),
                ("w1i", vp), ("w1h", vp), ("w2i", vp), ("w2h", vp), ("wc", vp), ("b2i", vp), ("b2h", vp), ("zx1", vp), ("ctxb", vp), ("ctxa", vp),
                ("cs", vp * 2), ("hsb", vp * 2), ("gates", vp * 2), ("a_all", vp), ("out", vp), ("cat_b", vp), ("out_b", vp),
                ("xbuf", vp), ("xbuf_bytes", sz), ("xtab", vp), ("xtab_bytes", sz), ("err", vp), ("err_ints", sz),
                ("tok0", vp), ("tok0_stride", i32), ("wo", vp), ("bo", vp), ("V", i32), ("pbuf", vp), ("pbuf_bytes", sz), ("labels", vp), ("scores", vp),
                ("trie_mask", vp), ("trie_base", vp), ("trie_child", vp), ("drop_h", Drop), ("drop_out", Drop), ("hm_b", vp),
                ("zx_tok", vp), ("zx_st", i64), ("zx_sb", i64), ("sc_hist", vp)]


class DecBwd(C.Structure):
    _fields_ = [("B", i32), ("T", i32), ("L", i32), ("Hd", i32), ("epoch", C.c_uint),
                ("w2i_t", vp), ("w2h_t", vp), ("w1h_t", vp), ("w1f_t", vp), ("wc_t", vp), ("wa_t", vp), ("dout_proj", vp), ("out", vp), ("a_all", vp),
                ("ctxb", vp), ("cs", vp * 2), ("gates", vp * 2),
                ("dpre", vp), ("dpre_b", vp), ("dcat", vp), ("ds_all", vp), ("dq", vp), ("dq_b", vp), ("dz", vp * 2), ("dzb", vp * 2), ("dc_st", vp * 2),
                ("dh_rec", vp * 2), ("dfeed", vp),
                ("xbuf", vp), ("xbuf_bytes", sz), ("xtab", vp), ("xtab_bytes", sz), ("err", vp), ("err_ints", sz), ("drop_h", Drop), ("drop_out", Drop)]


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def per_pass():
    return R.per_pass(cus())


def config_of(capfd, fn, others=()):
    """the one trace line of the call -> its line and its name=value fields; no line of the launchers in `others`"""
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if ln.startswith(f"[aocr] {fn}: ")]
    assert len(lines) == 1, f"{fn}: expected one dispatch trace line (AOCR_TRACE), got {lines}"
    for o in others:
        assert not [ln for ln in err.splitlines() if ln.startswith(f"[aocr] {o}: ")], f"a line of {o} beside {lines[0]}"
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


def d64(t):
    return t.float().double()


class Exchange:
    """exchange, xtab and err buffers sized as model.hip sizes them for B rows; kind "f": dec_cluster_xbuf_bytes, "b": dec_cluster_bwd_xbuf_bytes"""

    def __init__(self, B, kind, tab_rows=None):
        n = kp().kp_dec_cluster_xbuf_bytes(B) if kind == "f" else kp().kp_dec_cluster_bwd_xbuf_bytes(B)
        self.xbuf = Buf(((n + 7) // 8,), torch.int64, fill=0)
        self.xtab = Buf(((kp().kp_dec_cluster_xtab_bytes(tab_rows or B) + 7) // 8,), torch.int64, fill=0)      # (beam search: the model's max(B, 32 group_cap) rows)
        self.err = Buf((ERR_INTS,), torch.int32, fill=0)
        self.epoch = 0

    def fill(self, a, epochs=1):
        """the next epoch; a beam launch takes `epochs` consecutive ones (one per pass)"""
        a.epoch = self.epoch + 1
        self.epoch += epochs
        a.xbuf, a.xbuf_bytes, a.xtab, a.xtab_bytes = self.xbuf.full.data_ptr(), self.xbuf.n * 8, self.xtab.full.data_ptr(), self.xtab.n * 8
        a.err, a.err_ints = self.err.full.data_ptr(), self.err.n

    def ok(self, what):
        err = self.err.cpu()
        assert int(err[0]) == 0, f"{what}: a decoder kernel timed out: err = {err[:5].tolist()}"
        for b, nm in ((self.xbuf, "exchange buffer"), (self.xtab, "xtab"), (self.err, "err")):
            b.check_tail(f"{what} {nm}")


class Common:
    def __init__(self, B, T, L, seed, o=None):
        self.B, self.T, self.L = B, T, L
        self.o = R.operands(B, T, seed) if o is None else o            # o: explicit operands (R.take_rows: the context and initial state of chosen rows)
        self.w = R.weights_of(self.o)
        self.maxctx = self.o["ctx"].abs().max().item()
        self.ctxb = Buf(self.o["ctx"], torch.bfloat16)
        self.mask_h = self.mask_out = None

    def set_drop(self, drop):
        """drop = (p, seed, train step): the masks of sites 2 (layer 2's input) and 16 (attention output), flat index step B H + row H + unit"""
        p, seed, step = drop
        n = self.L * self.B * H
        self.mask_h, self.mask_out = (TR.drop_mask(p, seed, step, site, 0, n).view(self.L, self.B, H) for site in (2, 16))
        self.scale = 1.0 / (1.0 - p)
        self.specs = [Drop(*TR.drop_base_thr(p, seed, step, site), self.scale, 0) for site in (2, 16)]


# ------------------------------------------------------------------------------------------------------------------------------
# teacher-forced forward
# ------------------------------------------------------------------------------------------------------------------------------
class Fwd(Common):
    """table: zx1 is the per-token table [V][4H] and the tokens are a strided window (token of (t, b) at 1 + 2 t + (2 L + 3) b) with JUNK around it"""

    def __init__(self, B, T, L, table, seed, zx=None, drop=None, o=None, lean=False):
        super().__init__(B, T, L, seed, o)
        self.lean = lean                                               # no saved gates (one row each): the beam tests' replays and the beam problem itself
        if drop:
            self.set_drop(drop)
        self.table = table
        self.zx1, self.tok = R.gate_inputs(L, B, seed, table) if zx is None else zx
        o = self.o
        self.wd = {n: Buf(o[n], torch.bfloat16) for n in ("W1i", "W1h", "W2i", "W2h", "Wc")}
        self.b2i, self.b2h, self.zxd, self.ctxa = Buf(o["b2i"]), Buf(o["b2h"]), Buf(self.zx1), Buf(o["ctxa"], torch.bfloat16)
        self.tokd = None
        if self.tok is not None:
            self.st, self.sb = 2, 2 * L + 3
            host = torch.full((B * self.sb + 8,), int(JUNK), dtype=torch.int32)
            idx = 1 + self.st * torch.arange(L).view(L, 1) + self.sb * torch.arange(B).view(1, B)
            host[idx.reshape(-1)] = self.tok.reshape(-1)
            self.tokd = Buf(host, torch.int32)
        self.fresh()

    def fresh(self):
        B, T, L, o = self.B, self.T, self.L, self.o
        self.cs = [Buf((L + 1, B, H), fill=SENT) for _ in range(2)]
        self.hsb = [Buf((L + 1, B, H), torch.bfloat16, fill=SENT_B) for _ in range(2)]
        self.out, self.out_b = Buf((L + 1, B, H), fill=SENT), Buf((L + 1, B, H), torch.bfloat16, fill=SENT_B)
        for l in range(2):
            self.cs[l].t[0] = o["c0"][l].cuda()
            self.hsb[l].t[0] = o["h0"][l].to(torch.bfloat16).cuda()
        self.out_b.t[0] = o["feed0"].to(torch.bfloat16).cuda()
        self.gates = [Buf((1, 1, 4 * H) if self.lean else (L, B, 4 * H), fill=SENT) for _ in range(2)]
        self.a_all, self.cat_b = Buf((L, B, T), fill=SENT), Buf((L, B, 2 * H), torch.bfloat16, fill=SENT_B)
        self.hm_b = Buf((L, B, H), torch.bfloat16, fill=SENT_B) if self.mask_h is not None else None

    NAMES = ("cs0", "cs1", "hsb0", "hsb1", "out", "out_b", "gates0", "gates1", "a_all", "cat_b")

    def bufs(self):
        return dict(cs0=self.cs[0], cs1=self.cs[1], hsb0=self.hsb[0], hsb1=self.hsb[1], out=self.out, out_b=self.out_b, gates0=self.gates[0],
                    gates1=self.gates[1], a_all=self.a_all, cat_b=self.cat_b, **({"hm_b": self.hm_b} if self.hm_b else {}))

    def outputs(self):
        return {k: v.cpu().clone() for k, v in self.bufs().items()}

    def args(self, gates=True):
        a = DecFwd()
        a.B, a.T, a.L, a.Hd = self.B, self.T, self.L, H
        p = lambda b: b.full.data_ptr()
        a.w1i, a.w1h, a.w2i, a.w2h, a.wc = (p(self.wd[n]) for n in ("W1i", "W1h", "W2i", "W2h", "Wc"))
        a.b2i, a.b2h, a.zx1, a.ctxb, a.ctxa = p(self.b2i), p(self.b2h), p(self.zxd), p(self.ctxb), p(self.ctxa)
        for l in range(2):
            a.cs[l], a.hsb[l] = p(self.cs[l]), p(self.hsb[l])
            a.gates[l] = p(self.gates[l]) if gates else None
        a.a_all, a.out, a.cat_b, a.out_b = p(self.a_all), p(self.out), p(self.cat_b), p(self.out_b)
        if self.tokd is not None:
            a.zx_tok, a.zx_st, a.zx_sb, a.V = p(self.tokd) + 4, self.st, self.sb, V
        if self.hm_b:
            a.drop_h, a.drop_out, a.hm_b = self.specs[0], self.specs[1], p(self.hm_b)
        return a

    def check(self, what, gates=True, rows=None):
        """device-fed check of every step -> dict of the largest error / tolerance per quantity.  rows: only these batch rows (the outputs are [step][row][..])"""
        B, L, w, o = self.B, self.L, self.w, self.o
        d = self.outputs()
        if rows is not None:
            rows = torch.as_tensor(rows).long()
            B, o, w = len(rows), R.take_rows(o, rows), R.weights_of(R.take_rows(o, rows))
            d = {k: v if k.startswith("gates") and self.lean else v[:, rows] for k, v in d.items()}
        tok_ = self.tok if rows is None or self.tok is None else self.tok[:, rows]
        worst = dict(c=0.0, gates=0.0, a=0.0, out=0.0)
        zs = []
        assert same_bits(d["cs0"][0], o["c0"][0]) and same_bits(d["cs1"][0], o["c0"][1]), f"{what}: slot 0 of cs changed"
        assert same_bits(d["hsb0"][0], o["h0"][0].to(torch.bfloat16)) and same_bits(d["hsb1"][0], o["h0"][1].to(torch.bfloat16)), f"{what}: slot 0 of hsb changed"
        assert same_bits(d["out_b"][0], o["feed0"].to(torch.bfloat16)) and is_sentinel(d["out"][0]), f"{what}: slot 0 of out / out_b changed"
        for t in range(L):
            h1b, h2b, cat_b = d64(d["hsb0"][t + 1]), d64(d["hsb1"][t + 1]), d64(d["cat_b"][t])
            s = R.step_fed(w, R.zx_at(self.zx1, tok_, t), d64(d["out_b"][t]), d64(d["hsb0"][t]), d64(d["hsb1"][t]), d["cs0"][t].double(),
                           d["cs1"][t].double(), h1b, h2b, cat_b, x2b=d64(d["hm_b"][t]) if self.hm_b else None)
            zs.append(s["z"].reshape(-1))
            wt = f"{what} step {t}"
            for l, (c, h, g, m) in enumerate((("c1", "h1", "g1", "m1"), ("c2", "h2", "g2", "m2"))):
                bg = bound(s[m], 1024).view(B, 4, H)
                tol_g, tol_u = TOL_CELL + bg, TOL_CELL + bg.amax(dim=1)
                r = ratio(d[f"cs{l}"][t + 1], s[c], tol_u)
                assert r <= 1.0, f"{wt}: c{l + 1} error / tolerance = {r:.3f}"
                worst["c"] = max(worst["c"], r)
                if gates:
                    r = ratio(R.unil(d[f"gates{l}"][t]), s[g], tol_g)
                    assert r <= 1.0, f"{wt}: saved gates of layer {l + 1} error / tolerance = {r:.3f}"
                    worst["gates"] = max(worst["gates"], r)
                assert in_rne_range(d[f"hsb{l}"][t + 1], s[h], tol_u), f"{wt}: hsb[{l}] outside [RNE(h - tol), RNE(h + tol)]"
            bs = bound(s["ms"].amax(dim=1, keepdim=True), 512)
            r = ratio(d["a_all"][t], s["a"], TOL_A + bs)
            assert r <= 1.0, f"{wt}: a_all error / tolerance = {r:.3f}"
            worst["a"] = max(worst["a"], r)
            assert in_rne_range(d["cat_b"][t][:, :H], s["c"], TOL_C * self.maxctx + 2 * bs), f"{wt}: c half of cat_b outside its RNE range"
            assert same_bits(d["cat_b"][t][:, H:], d["hsb1"][t + 1]), f"{wt}: h2 half of cat_b is not hsb[1]"
            ref_out, tol_out = s["out"], TOL_CELL + bound(s["mo"], 1024)
            if self.hm_b:                                              # nn.Dropout on the attention output and on layer 2's input: value and bound times the mask
                ref_out, tol_out = ref_out * self.mask_out[t], tol_out * self.scale
                mk, hm = self.mask_h[t], d["hm_b"][t]
                tol_h = (TOL_CELL + bound(s["m1"], 1024).view(B, 4, H).amax(dim=1)) * self.scale
                assert bool((hm.float()[mk == 0] == 0).all()), f"{wt}: hm_b is not zero where the mask drops"
                assert bool((d["out"][t + 1][self.mask_out[t] == 0] == 0).all()), f"{wt}: out is not zero where the mask drops"
                assert in_rne_range(hm, s["h1"] * mk, tol_h), f"{wt}: hm_b outside the RNE range of mask x h1"
                # mask x the device's own bf16 h1: hm_b is the RNE of mask x the fp32 h1, whose bf16 image is hsb[0] -- within one rounding of h1 each
                assert in_rne_range(hm, h1b * mk, h1b.abs() * mk * 2.0 ** -8 + 1e-30), f"{wt}: hm_b is not mask x the device's h1"
            r = ratio(d["out"][t + 1], ref_out, tol_out)
            assert r <= 1.0, f"{wt}: out error / tolerance = {r:.3f}"
            worst["out"] = max(worst["out"], r)
            assert same_bits(d["out_b"][t + 1], d["out"][t + 1].to(torch.bfloat16)), f"{wt}: out_b is not the RNE of the kernel's own out"
        if not gates:
            assert is_sentinel(d["gates0"]) and is_sentinel(d["gates1"]), f"{what}: gates written by the gold pass"
        for k, b in self.bufs().items():
            b.check_tail(f"{what} {k}")                                # rows >= B of the last group appear in no output
        share = R.z_share(torch.cat(zs))
        assert share >= 0.9, f"{what}: only {share:.3f} of the device-fed pre-activations inside |z| <= 4"
        return worst

    def parity(self):
        f = R.forward(self.w, self.zx1, self.o["c0"], self.o["h0"], self.o["feed0"], self.L, tok=self.tok, mask_h=self.mask_h, mask_out=self.mask_out)
        return (self.out.cpu()[self.L].double() - f["out"][self.L]).abs().max().item()


def expect_trace(line, cfg, kernel, p, remote=0):
    groups = (p.B + 31) // 32
    assert f": {kernel} {p.B} {p.T} {p.L} " in line, line
    assert cfg == dict(groups=groups, passes=(groups + per_pass() - 1) // per_pass(), remote=remote), (cfg, per_pass())


def run_fwd(p, ex, capfd, monkeypatch, env, gates=True, remote=0, res=True, drop=False):
    """one forward call under the switches `env` -> its trace line; trace, err and the exchange tails asserted"""
    setenv(monkeypatch, env)
    a = p.args(gates)
    ex.fill(a)
    capfd.readouterr()
    rc = launch("kp_dec_cluster_forward", a)
    assert rc == 0, f"wrapper / hipGetLastError() = {rc}"
    torch.cuda.synchronize()
    if "AOCR_NO_DEC_CHAINS" in env or drop:                           # dropout: the cluster kernel although the chains are enabled
        line, cfg = config_of(capfd, "dec_cluster_forward", others=("dec_chain_forward",))
        expect_trace(line, cfg, "dec_cl_fwd_kernel[tf,drop]" if drop else "dec_cl_fwd_kernel[tf]", p, remote)
    else:
        line, cfg = config_of(capfd, "dec_chain_forward", others=("dec_cluster_forward",))
        expect_trace(line, cfg, "dec_ch_fwd_kernel[tf,res]" if p.T <= 64 and res else "dec_ch_fwd_kernel[tf]", p, remote)
    for k in env:
        monkeypatch.delenv(k)
    ex.ok(line)
    return line


def tf_shapes():
    return R.TF_SHAPES + [(32 * per_pass() + 4, 3, 2)]


TF_IDS = [f"{b}-{t}-{l}" for b, t, l in R.TF_SHAPES] + ["two-passes"]


def fmt(w):
    return "  ".join(f"{k} {v:.3f}" for k, v in w.items())


@pytest.mark.parametrize("i", range(len(TF_IDS)), ids=TF_IDS)
def test_forward(i, cuda, capfd, monkeypatch):
    B, T, L = tf_shapes()[i]
    p, ex = Fwd(B, T, L, table=i % 2 == 1, seed=B + T + L), Exchange(B, "f")
    got, report = {}, []                                               # (printed at the end: capfd.readouterr() of a later call would swallow the lines)
    for name, env in (("chain", {}), ("cluster", CLUSTER)):
        p.fresh()
        line = run_fwd(p, ex, capfd, monkeypatch, env)
        worst = p.check(f"{name} {B}-{T}-{L}")
        got[name] = p.outputs()
        report.append(f"[dec-kernels] {line[7:]} ({'token table' if p.table else 'zx tensor'}): {fmt(worst)}")
        report.append(f"[parity] {name} B={B} T={T} L={L}: free-running distance of the final out = {p.parity():.3e}")
        p.fresh()
        run_fwd(p, ex, capfd, monkeypatch, env, gates=False)       # the gold pass: no gates, every other output bit-identical
        gold = p.outputs()
        assert is_sentinel(gold["gates0"]) and is_sentinel(gold["gates1"]), f"{name}: the gold pass wrote gates"
        for k in Fwd.NAMES:
            if not k.startswith("gates"):
                assert same_bits(gold[k], got[name][k]), f"{name}: {k} of the gold pass (gates == nullptr) differs from the saved-gates run"
    for k in Fwd.NAMES:
        assert same_bits(got["chain"][k], got["cluster"][k]), f"{k}: the chain kernel differs from the cluster kernel"
    print("\n".join(report))


def test_forward_table_and_tensor_agree(cuda, capfd, monkeypatch):
    B, T, L = 17, 17, 3
    pt = Fwd(B, T, L, table=True, seed=B + T + L)
    zx = pt.zx1[pt.tok.long() - 1].contiguous()                        # [L][B][4H]: the rows the table run gathers
    pz = Fwd(B, T, L, table=False, seed=B + T + L, zx=(zx, None))
    for env in ({}, CLUSTER):
        outs = []
        for p in (pt, pz):
            p.fresh()
            run_fwd(p, Exchange(B, "f"), capfd, monkeypatch, env)
            outs.append(p.outputs())
        for k in Fwd.NAMES:
            assert same_bits(outs[0][k], outs[1][k]), f"{k}: the per-token table and the [L][B][4Hd] tensor give different results ({env})"
    pz.check("zx tensor")
    print("[dec-kernels] forward 17-17-3: per-token table (strided tokens) and zx tensor bit-identical on chain and cluster")


@pytest.mark.parametrize("B,T,L", [(16, 16, 3), (32, 64, 2)])
def test_forward_chain_without_resident_tile(B, T, L, cuda, capfd, monkeypatch):
    p, ex = Fwd(B, T, L, table=T == 64, seed=B + T + L), Exchange(B, "f")
    line = run_fwd(p, ex, capfd, monkeypatch, {})
    assert "[tf,res]" in line
    res = p.outputs()
    p.fresh()
    line = run_fwd(p, ex, capfd, monkeypatch, {"AOCR_CH_NO_RES": "1"}, res=False)
    assert "dec_ch_fwd_kernel[tf]" in line
    p.check("AOCR_CH_NO_RES=1")
    now = p.outputs()
    for k in Fwd.NAMES:
        assert same_bits(res[k], now[k]), f"{k}: AOCR_CH_NO_RES=1 differs from the resident form"
    print(f"[dec-kernels] {line[7:]}: bit-identical to [tf,res]")


@pytest.mark.parametrize("kernel", ["chain", "cluster"])
def test_forward_remote_and_stale_epoch(kernel, cuda, capfd, monkeypatch):
    B, T, L = 45, 5, 5
    env = CLUSTER if kernel == "cluster" else {}
    p, ex = Fwd(B, T, L, table=True, seed=7), Exchange(B, "f")
    run_fwd(p, ex, capfd, monkeypatch, env)
    p.check("local")
    local = p.outputs()
    for what, extra, remote in (("epoch + 1 on used exchange buffers", {}, 0), ("AOCR_CL_REMOTE=1", {"AOCR_CL_REMOTE": "1"}, 1)):
        p.fresh()
        run_fwd(p, ex, capfd, monkeypatch, {**env, **extra}, remote=remote)
        now = p.outputs()
        for k in Fwd.NAMES:
            assert same_bits(local[k], now[k]), f"{kernel} {what}: {k} differs from the first local run"
    print(f"[dec-kernels] forward {kernel} 45-5-5: epoch + 1 on used exchange buffers and AOCR_CL_REMOTE=1 bit-identical to the local exchange")


# ------------------------------------------------------------------------------------------------------------------------------
# BPTT
# ------------------------------------------------------------------------------------------------------------------------------
class Bwd(Common):
    def __init__(self, B, T, L, seed, drop=None):
        super().__init__(B, T, L, seed)
        if drop:
            self.set_drop(drop)
        o, w = self.o, self.w
        zx1, tok = R.gate_inputs(L, B, seed, table=False)
        f = R.forward(w, zx1, o["c0"], o["h0"], o["feed0"], L, mask_h=self.mask_h, mask_out=self.mask_out)
        self.f32 = dict(cs=f["cs"].float(), gates=f["gates"].float(), a=f["a"].float(), out=f["out"].float())
        self.dout = R.uniform((L, B, H), 0.5, seed * 16 + 14)
        tr = lambda t: Buf(t.t().contiguous(), torch.bfloat16)
        self.wt = dict(w2i_t=tr(o["W2i"]), w2h_t=tr(o["W2h"]), w1h_t=tr(o["W1h"]), w1f_t=tr(o["W1i"]), wc_t=tr(o["Wc"]), wa_t=tr(o["Wa"]))
        self.doutd, self.outd, self.ad = Buf(self.dout), Buf(self.f32["out"]), Buf(self.f32["a"])
        self.csd = [Buf(self.f32["cs"][l]) for l in range(2)]
        self.gd = [Buf(R.il(self.f32["gates"][l])) for l in range(2)]
        self.fresh()

    def fresh(self):
        B, T, L = self.B, self.T, self.L
        f = lambda *s: Buf(s, fill=SENT)
        fb = lambda *s: Buf(s, torch.bfloat16, fill=SENT_B)
        self.b = dict(dpre=f(L, B, H), dpre_b=fb(L, B, H), dcat=f(L, B, 2 * H), ds_all=f(L, B, T), dq=f(L, B, H), dq_b=fb(L, B, H),
                      dz0=f(L, B, 4 * H), dz1=f(L, B, 4 * H), dzb0=fb(L, B, 4 * H), dzb1=fb(L, B, 4 * H), dc_st0=f(B, H), dc_st1=f(B, H),
                      dh_rec0=f(B, H), dh_rec1=f(B, H), dfeed=f(B, H))

    BF = ("dpre_b", "dq_b", "dzb0", "dzb1")

    def outputs(self):
        return {k: v.cpu().clone() for k, v in self.b.items()}

    def args(self):
        a = DecBwd()
        a.B, a.T, a.L, a.Hd = self.B, self.T, self.L, H
        p = lambda b: b.full.data_ptr()
        for k, v in self.wt.items():
            setattr(a, k, p(v))
        a.dout_proj, a.out, a.a_all, a.ctxb = p(self.doutd), p(self.outd), p(self.ad), p(self.ctxb)
        b = self.b
        for l in range(2):
            a.cs[l], a.gates[l], a.dz[l], a.dzb[l] = p(self.csd[l]), p(self.gd[l]), p(b[f"dz{l}"]), p(b[f"dzb{l}"])
            a.dc_st[l], a.dh_rec[l] = p(b[f"dc_st{l}"]), p(b[f"dh_rec{l}"])
        a.dpre, a.dpre_b, a.dcat, a.ds_all, a.dq, a.dq_b, a.dfeed = (p(b[k]) for k in ("dpre", "dpre_b", "dcat", "ds_all", "dq", "dq_b", "dfeed"))
        if self.mask_h is not None:
            a.drop_h, a.drop_out = self.specs[0], self.specs[1]
        return a

    def check(self, what):
        B, L, w = self.B, self.L, self.w
        d = self.outputs()
        f = {k: v.double() for k, v in self.f32.items()}
        worst = dict(dpre=0.0, dcat=0.0, ds=0.0, dq=0.0, dz=0.0, dc=0.0, rec=0.0)
        zero = torch.zeros(B, 4 * H, dtype=torch.float64)
        dc1 = dc2 = torch.zeros(B, H, dtype=torch.float64)
        tmax = 0.0

        def upd(k, r, wt, name):
            assert r <= 1.0, f"{wt}: {name} error / tolerance = {r:.3f}"
            worst[k] = max(worst[k], r)

        for t in range(L - 1, -1, -1):
            n1, n2 = (d64(d["dzb0"][t + 1]), d64(d["dzb1"][t + 1])) if t < L - 1 else (zero, zero)
            fed = dict(dpre_b=d64(d["dpre_b"][t]), dcat_c=d["dcat"][t][:, :H].double(), dq_b=d64(d["dq_b"][t]), dzb2=d64(d["dzb1"][t]))
            s = R.bwd_step_fed(w, R.saved_step(f, t), self.dout[t].double(), n1, n2, dc1, dc2, fed=fed,
                               mask_h=None if self.mask_h is None else self.mask_h[t], mask_out=None if self.mask_out is None else self.mask_out[t])
            dc1, dc2 = s["dc1"], s["dc2"]
            wt = f"{what} step {t}"
            base = TOL_BWD * max(1.0, s["dh"]) * (self.scale if self.mask_h is not None else 1.0)      # (dropout: d h passes the mask, a factor 1 / (1 - p))
            tol = lambda m: base + bound(m, 2048)
            tmax = max(tmax, tol(torch.maximum(s["m_z1"], s["m_z2"])).max().item(), tol(s["m_pre"]).max().item())
            upd("dpre", ratio(d["dpre"][t], s["dpre"], tol(s["m_pre"])), wt, "dpre")
            assert same_bits(d["dpre_b"][t], d["dpre"][t].to(torch.bfloat16)), f"{wt}: dpre_b is not the RNE of the kernel's own dpre"
            upd("dcat", ratio(d["dcat"][t][:, :H], s["dcat_c"], tol(s["m_cat"])), wt, "c half of dcat")
            assert is_sentinel(d["dcat"][t][:, H:]), f"{wt}: h half of dcat written"
            m = max(1.0, s["da"].abs().max().item())
            extra = bound(s["m_da"].amax(dim=1, keepdim=True), 512)
            upd("ds", ratio(d["ds_all"][t], s["ds"], TOL_DS * m + extra), wt, "ds_all")
            upd("dq", ratio(d["dq"][t], s["dq"], TOL_DQ * m * self.maxctx + 2 * extra), wt, "dq")
            assert same_bits(d["dq_b"][t], d["dq"][t].to(torch.bfloat16)), f"{wt}: dq_b is not the RNE of the kernel's own dq"
            for l, (k, mk) in enumerate((("dz1", "m_z1"), ("dz2", "m_z2"))):
                tz = tol(s[mk]).unsqueeze(1).expand(B, 4, H).reshape(B, 4 * H)
                upd("dz", ratio(d[f"dz{l}"][t], s[k], tz), wt, f"dz[{l}]")
                assert same_bits(d[f"dzb{l}"][t], d[f"dz{l}"][t].to(torch.bfloat16)), f"{wt}: dzb[{l}] is not the RNE of the kernel's own dz"
        upd("dc", ratio(d["dc_st0"], dc1, L * tmax), what, "dc_st[0]")
        upd("dc", ratio(d["dc_st1"], dc2, L * tmax), what, "dc_st[1]")
        z1, z2 = d64(d["dzb0"][0]), d64(d["dzb1"][0])
        for k, prod, mag in (("dh_rec0", z1 @ w.W1h, z1.abs() @ w.W1h.abs()), ("dh_rec1", z2 @ w.W2h, z2.abs() @ w.W2h.abs()),
                             ("dfeed", z1 @ w.W1i, z1.abs() @ w.W1i.abs())):
            upd("rec", ratio(d[k], prod, TOL_BWD * max(1.0, prod.abs().max().item()) + bound(mag, 2048)), what, k)
        for k, b in self.b.items():
            b.check_tail(f"{what} {k}")
        return worst


def run_bwd(p, ex, capfd, monkeypatch, env, remote=0, drop=False):
    setenv(monkeypatch, env)
    a = p.args()
    ex.fill(a)
    capfd.readouterr()
    rc = launch("kp_dec_cluster_backward", a)
    assert rc == 0, f"wrapper / hipGetLastError() = {rc}"
    torch.cuda.synchronize()
    if "AOCR_NO_DEC_CHAINS" in env or "AOCR_NO_DEC_CHAINS_BWD" in env or drop:
        line, cfg = config_of(capfd, "dec_cluster_backward", others=("dec_chain_backward",))
        expect_trace(line, cfg, "dec_cl_bwd_kernel[bptt,drop]" if drop else "dec_cl_bwd_kernel[bptt]", p, remote)
    else:
        line, cfg = config_of(capfd, "dec_chain_backward", others=("dec_cluster_backward",))
        expect_trace(line, cfg, "dec_ch_bwd_kernel[bptt]", p, remote)
    for k in env:
        monkeypatch.delenv(k)
    ex.ok(line)
    return line


@pytest.mark.parametrize("i", range(len(TF_IDS)), ids=TF_IDS)
def test_backward(i, cuda, capfd, monkeypatch):
    B, T, L = tf_shapes()[i]
    assert kp().kp_dec_cluster_bwd_supported(H, 2, 1, T, L) == 1
    p, ex = Bwd(B, T, L, seed=B + T + L), Exchange(B, "b")
    got, report = {}, []
    for name, env in (("chain", {}), ("cluster", {"AOCR_NO_DEC_CHAINS_BWD": "1"} if i % 2 else CLUSTER)):
        p.fresh()
        line = run_bwd(p, ex, capfd, monkeypatch, env)
        worst = p.check(f"{name} {B}-{T}-{L}")
        got[name] = p.outputs()
        report.append(f"[dec-kernels] {line[7:]}: {fmt(worst)}")
    print("\n".join(report))
    for k in Bwd.BF:
        assert same_bits(got["chain"][k], got["cluster"][k]), f"{k}: the chain kernel differs from the cluster kernel"


@pytest.mark.parametrize("kernel", ["chain", "cluster"])
def test_backward_remote_and_stale_epoch(kernel, cuda, capfd, monkeypatch):
    B, T, L = 45, 5, 5
    env = CLUSTER if kernel == "cluster" else {}
    p, ex = Bwd(B, T, L, seed=7), Exchange(B, "b")
    run_bwd(p, ex, capfd, monkeypatch, env)
    p.check("local")
    local = p.outputs()
    for what, extra, remote in (("epoch + 1 on used exchange buffers", {}, 0), ("AOCR_CL_REMOTE=1", {"AOCR_CL_REMOTE": "1"}, 1)):
        p.fresh()
        run_bwd(p, ex, capfd, monkeypatch, {**env, **extra}, remote=remote)
        now = p.outputs()
        for k in local:
            assert same_bits(local[k], now[k]), f"{kernel} {what}: {k} differs from the first local run"
    print(f"[dec-kernels] backward {kernel} 45-5-5: epoch + 1 on used exchange buffers and AOCR_CL_REMOTE=1 bit-identical to the local exchange")


# ------------------------------------------------------------------------------------------------------------------------------
# nn.Dropout(0.25): the cluster kernels only
# ------------------------------------------------------------------------------------------------------------------------------
DROP = (0.25, 99, 4)                # p, seed, train step


def test_dropout_forward(cuda, capfd, monkeypatch):
    B, T, L = R.DROP_SHAPE
    p, ex = Fwd(B, T, L, table=True, seed=11, drop=DROP), Exchange(B, "f")
    kept = (p.mask_h != 0).double().mean().item()
    assert 0.70 < kept < 0.80 and not torch.equal(p.mask_h, p.mask_out) and not torch.equal(p.mask_h[0], p.mask_h[1])
    line = run_fwd(p, ex, capfd, monkeypatch, {}, drop=True)           # chains enabled: the trace must still show the cluster kernel
    worst = p.check("dropout")
    print(f"[dec-kernels] {line[7:]} p=0.25: {fmt(worst)}")
    print(f"[parity] dropout B={B} T={T} L={L}: free-running distance of the final out = {p.parity():.3e}")


def test_dropout_backward(cuda, capfd, monkeypatch):
    B, T, L = R.DROP_SHAPE
    p, ex = Bwd(B, T, L, seed=11, drop=DROP), Exchange(B, "b")
    line = run_bwd(p, ex, capfd, monkeypatch, {}, drop=True)
    worst = p.check("dropout")
    print(f"[dec-kernels] {line[7:]} p=0.25: {fmt(worst)}")


# ------------------------------------------------------------------------------------------------------------------------------
# greedy decode (DEC, HIST)
# ------------------------------------------------------------------------------------------------------------------------------
class Greedy:
    """The DEC problem on the operands of Fwd(B, T, L, table=True, seed): GO tokens in column 1 of a [B][L + 3] window with JUNK around it
    (tok0_stride = L + 3, which is the row stride of labels too), W_o with the planted twin classes, optional flat trie, optional sc_hist."""

    def __init__(self, B, T, L, seed, trie=None):
        self.B, self.T, self.L, self.seed = B, T, L, seed
        self.p = Fwd(B, T, L, table=True, seed=seed)
        self.wo, self.bo = R.projector(seed)
        self.wod, self.bod = Buf(self.wo), Buf(self.bo)
        self.stride = L + 3
        host = torch.full((B * self.stride + 8,), int(JUNK), dtype=torch.int32)
        host[1 + self.stride * torch.arange(B)] = R.GO
        self.tok0 = Buf(host, torch.int32)
        self.pbuf = Buf(((kp().kp_dec_cluster_pbuf_bytes(B) + 3) // 4,), fill=0.0)
        self.trie = trie
        self.tried = [Buf(torch.from_numpy(t.astype("int64") if i == 0 else t), torch.int64 if i == 0 else torch.int32) for i, t in enumerate(trie)] if trie else None

    def run(self, ex, capfd, monkeypatch, env, hist=False):
        p, B, L = self.p, self.B, self.L
        p.fresh()
        self.labels = Buf((B * self.stride + 8,), torch.int32, fill=0x5B)
        self.scores, self.sc_hist = Buf((B,), fill=SENT), Buf((L, B), fill=SENT) if hist else None
        setenv(monkeypatch, env)
        a = p.args(gates=False)
        a.zx_tok, a.greedy, a.V = None, 1, V
        a.tok0, a.tok0_stride, a.wo, a.bo = self.tok0.full.data_ptr() + 4, self.stride, self.wod.full.data_ptr(), self.bod.full.data_ptr()
        a.pbuf, a.pbuf_bytes, a.labels, a.scores = self.pbuf.full.data_ptr(), self.pbuf.n * 4, self.labels.full.data_ptr() + 4, self.scores.full.data_ptr()
        if hist:
            a.sc_hist = self.sc_hist.full.data_ptr()
        if self.tried:
            a.trie_mask, a.trie_base, a.trie_child = (b.full.data_ptr() for b in self.tried)
        ex.fill(a)
        capfd.readouterr()
        rc = launch("kp_dec_cluster_forward", a)
        assert rc == 0, f"wrapper / hipGetLastError() = {rc}"
        torch.cuda.synchronize()
        cluster = "AOCR_NO_DEC_CHAINS" in env or "AOCR_NO_DEC_CHAINS_GREEDY" in env
        inst = "dec" + (",res" if self.T <= 64 and not cluster else "") + (",hist" if hist else "")
        if cluster:
            line, cfg = config_of(capfd, "dec_cluster_forward", others=("dec_chain_forward",))
            expect_trace(line, cfg, f"dec_cl_fwd_kernel[{inst}]", p)
        else:
            line, cfg = config_of(capfd, "dec_chain_forward", others=("dec_cluster_forward",))
            expect_trace(line, cfg, f"dec_ch_fwd_kernel[{inst}]", p)
        for k in env:
            monkeypatch.delenv(k)
        ex.ok(line)
        for b, nm in ((self.labels, "labels"), (self.scores, "scores"), (self.pbuf, "pbuf"), (self.tok0, "tok0")) + (((self.sc_hist, "sc_hist"),) if hist else ()):
            b.check_tail(f"{line} {nm}")
        full = self.labels.cpu()
        win = full[1:1 + B * self.stride].view(B, self.stride)
        assert bool((win[:, L:] == 0x5B).all()) and int(full[0]) == 0x5B, f"{line}: labels written outside their [B][L] window"
        return dict(line=line, labels=win[:, :L].clone().long(), scores=self.scores.cpu().clone(), hsb0=p.hsb[0].cpu().clone(), hsb1=p.hsb[1].cpu().clone(),
                    out_b=p.out_b.cpu().clone(), a_all=p.a_all.cpu().clone(), sc_hist=self.sc_hist.cpu().clone() if hist else None)

    def verify(self, g, capfd, monkeypatch, what):
        """stage 1: the teacher-forced kernel (verified above) on greedy's own tokens reproduces its bf16 trajectories bit for bit up to each row's last
        live step; stage 2: labels, scores, PAD after EOS against the float64 projector + LogSoftMax of the replay's fp32 out.  -> figures"""
        B, T, L = self.B, self.T, self.L
        lab = g["labels"]
        assert bool(((lab >= 1) & (lab <= V)).all()), f"{what}: labels outside 1..V"
        tok = torch.cat([torch.full((B, 1), R.GO, dtype=torch.int64), lab[:, :-1]], 1).t().contiguous().int()         # [L][B]
        rp = Fwd(B, T, L, table=True, seed=self.seed, zx=(self.p.zx1, tok))
        run_fwd(rp, Exchange(B, "f"), capfd, monkeypatch, {})
        rp.check(f"{what} replay", gates=True)
        r = rp.outputs()
        e = R.end_step(lab)                                            # the row's last live step: it emits EOS (or PAD); PAD at no cost from then on
        diff = total = 0
        for b in range(B):
            n = min(int(e[b]) + 1, L)                                  # live steps of the row
            for k in ("hsb0", "hsb1", "out_b"):
                x, y = g[k][1:n + 1, b].view(torch.int16), r[k][1:n + 1, b].view(torch.int16)
                diff += int((x != y).sum()); total += x.numel()
        assert diff == 0, f"{what}: {diff} of {total} bf16 values of the greedy trajectory differ from the teacher-forced replay"
        worst, ties, masked, node = 0.0, 0, 0, [0] * B
        run = torch.zeros(B, dtype=torch.float64)
        for t in range(L):
            lp, mag = R.logprobs(r["out"][t + 1], self.wo, self.bo)
            tol = TOL_CELL + bound(mag.amax(dim=1), 512)                # [B]
            for b in range(B):
                v = int(lab[b, t])
                if t > int(e[b]):
                    assert v == R.PAD, f"{what}: row {b} step {t}: label {v} after EOS / PAD"
                    continue
                row = lp[b].clone()
                free = int(row.argmax()) + 1
                if self.trie:
                    row[~R.admissible(self.trie, node[b], t)] = -float("inf")
                    masked += int(row[free - 1] == -float("inf"))
                    node[b] = R.trie_step(self.trie, node[b], v, t)
                best = row.max().item()
                top = row.topk(3).values
                twin = int(row.argmax()) + 1 == R.TIE[0] and row[R.TIE[1] - 1] == best
                margin = (top[0] - top[2 if twin else 1]).item()
                assert margin > 2 * tol[b].item(), f"{what}: row {b} step {t}: the reference's margin {margin:.2e} is inside 2 tol"
                assert row[v - 1].item() >= best - 2 * tol[b].item(), f"{what}: row {b} step {t}: label {v} is not in the reference's arg-max set"
                if twin:
                    ties += 1
                    assert v == R.TIE[0], f"{what}: row {b} step {t}: the tie between the twin classes went to {v}"
                run[b] += row[v - 1]
                if g["sc_hist"] is not None:
                    rr = abs(g["sc_hist"][t, b].item() - run[b].item()) / ((t + 1) * tol[b].item())
                    assert rr <= 1.0, f"{what}: row {b} step {t}: running score error / tolerance = {rr:.3f}"
                    worst = max(worst, rr)
        n_live = torch.clamp(e + 1, max=L).double()
        tolmax = TOL_CELL + bound(R.logprobs(r["out"][1:].reshape(L * B, H), self.wo, self.bo)[1].amax(), 512).item()
        rs = ((g["scores"].double() - run).abs() / (n_live * tolmax)).max().item()
        assert rs <= 1.0, f"{what}: final score error / (n tol) = {rs:.3f}"
        if g["sc_hist"] is not None:
            h = g["sc_hist"]                                          # (steps behind a group's early exit are not run: their entries keep the sentinel)
            for b in range(B):
                last = min(int(e[b]), L - 1)
                assert same_bits(h[last, b], g["scores"][b]), f"{what}: row {b}: sc_hist at the row's last live step is not the final score"
                later = h[last + 1:, b]
                assert bool(((later == SENT) | (later.view(torch.int32) == h[last, b].view(torch.int32))).all()), f"{what}: row {b}: the score moves after EOS"
        if self.trie:
            assert masked >= 1, f"{what}: the dictionary never masks the unconstrained arg-max"
        else:
            assert ties >= 1, f"{what}: no step at which the planted twin classes win"
        return dict(score=max(worst, rs), ties=ties, masked=masked, eos=e, replay=r)


@pytest.mark.parametrize("B,T,L,seed", R.GREEDY_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in R.GREEDY_CASES])
def test_greedy(B, T, L, seed, cuda, capfd, monkeypatch):
    q, ex = Greedy(B, T, L, seed), Exchange(B, "f")
    report, got = [], {}
    for name, env in (("chain", {}), ("cluster", {"AOCR_NO_DEC_CHAINS_GREEDY": "1"})):
        g = q.run(ex, capfd, monkeypatch, env)
        ok, txt = R.greedy_conditions(g["labels"], B)
        assert ok, f"{name}: the case lost its conditions: {txt}"
        v = q.verify(g, capfd, monkeypatch, name)
        got[name] = g
        report.append(f"[dec-kernels] {g['line'][7:]}: stage 1 mismatch share 0, final score error / (n tol) = {v['score']:.3f}, planted ties won {v['ties']}")
        ne = q.run(ex, capfd, monkeypatch, {**env, "AOCR_NO_DEC_EARLY": "1"})
        assert torch.equal(ne["labels"], g["labels"]) and same_bits(ne["scores"], g["scores"]), f"{name}: AOCR_NO_DEC_EARLY=1 changes labels or scores"
    assert torch.equal(got["chain"]["labels"], got["cluster"]["labels"]) and same_bits(got["chain"]["scores"], got["cluster"]["scores"]), "chain and cluster greedy differ"
    print("\n".join(report))


@pytest.mark.parametrize("B,T,L,seed", R.GREEDY_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in R.GREEDY_CASES])
def test_greedy_history(B, T, L, seed, cuda, capfd, monkeypatch):
    q, ex = Greedy(B, T, L, seed), Exchange(B, "f")
    report = []
    for name, env in (("chain", {}), ("cluster", {"AOCR_NO_DEC_CHAINS_GREEDY": "1"})):
        g = q.run(ex, capfd, monkeypatch, env, hist=True)
        assert ",hist]" in g["line"]
        v = q.verify(g, capfd, monkeypatch, f"{name} hist")
        worst = 0.0
        for b in range(B):                                             # the attention rows of the live steps against the replay's (verified above), at the attention tolerance
            n = min(int(v["eos"][b]) + 1, L)
            worst = max(worst, ratio(g["a_all"][:n, b], v["replay"]["a_all"][:n, b].double(), TOL_A))
        assert worst <= 1.0, f"{name}: a_all of the hist run error / tolerance = {worst:.3f}"
        report.append(f"[dec-kernels] {g['line'][7:]}: running score error / ((t+1) tol) = {v['score']:.3f}, a_all {worst:.3f}")
    print("\n".join(report))


@pytest.mark.parametrize("B,T,L,seed", R.GREEDY_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in R.GREEDY_CASES])
def test_greedy_dictionary(B, T, L, seed, cuda, capfd, monkeypatch):
    import dict_oracle as DO
    trie = TR.flat_trie(DO.load_dictionary(R.words(seed)))[:3]
    q, ex = Greedy(B, T, L, seed, trie=trie), Exchange(B, "f")
    report = []
    for name, env in (("chain", {}), ("cluster", {"AOCR_NO_DEC_CHAINS_GREEDY": "1"})):
        g = q.run(ex, capfd, monkeypatch, env)
        v = q.verify(g, capfd, monkeypatch, f"{name} trie")
        report.append(f"[dec-kernels] {g['line'][7:]} dictionary: final score error / (n tol) = {v['score']:.3f}, steps with the free arg-max masked {v['masked']}")
    print("\n".join(report))


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_what_the_model_would_not_launch(cuda, capfd):
    """every KP_DEC_* code once: nothing is launched (the outputs keep their sentinels, no trace line)"""
    assert kp().kp_dec_cluster_supported(H, 2, 1, 16, 3) == 1 and kp().kp_dec_cluster_supported(1024, 2, 1, 16, 3) == 0
    assert kp().kp_dec_cluster_supported(H, 2, 1, 257, 3) == 0 and kp().kp_dec_cluster_supported(H, 3, 1, 16, 3) == 0
    assert kp().kp_dec_cluster_supported(H, 2, 0, 16, 3) == 0
    assert kp().kp_dec_cluster_supported(H, 2, 1, 16, 600) == 1 and kp().kp_dec_cluster_bwd_supported(H, 2, 1, 16, 600) == 0
    B, T, L = 7, 15, 2
    p, ex = Fwd(B, T, L, table=True, seed=1), Exchange(B, "f")
    pbuf = Buf(((kp().kp_dec_cluster_pbuf_bytes(B) + 3) // 4,), fill=0.0)
    lab, sc = Buf((B, L), torch.int32, fill=0x5B), Buf((B,), fill=SENT)

    def refused(code, greedy=False, **change):
        a = p.args()
        ex.fill(a)
        if greedy:                                                    # a complete greedy problem, so that only `change` is wrong
            a.greedy, a.tok0, a.tok0_stride, a.wo, a.bo, a.V = 1, p.tokd.full.data_ptr(), L, p.zxd.full.data_ptr(), p.b2i.full.data_ptr(), V
            a.pbuf, a.pbuf_bytes, a.labels, a.scores = pbuf.full.data_ptr(), pbuf.n * 4, lab.full.data_ptr(), sc.full.data_ptr()
        for k, v in change.items():
            setattr(a, k, v)
        capfd.readouterr()
        assert launch("kp_dec_cluster_forward", a) == code, change
        err = capfd.readouterr().err
        assert "[aocr] dec_" not in err, err

    refused(KP_DEC_UNSUPPORTED, Hd=1024)
    refused(KP_DEC_UNSUPPORTED, T=257)
    refused(KP_DEC_XBUF_SMALL, xbuf_bytes=ex.xbuf.n * 8 - 8)
    refused(KP_DEC_PBUF_SMALL, greedy=True, pbuf_bytes=pbuf.n * 4 - 8)
    refused(KP_DEC_XTAB_SMALL, xtab_bytes=ex.xtab.n * 8 - 8)
    refused(KP_DEC_ERR_SMALL, err_ints=16 + 256 * 4)
    refused(KP_DEC_BAD_ARGS, epoch=0)
    refused(KP_DEC_BAD_ARGS, V=41)
    refused(KP_DEC_BAD_ARGS, greedy=True, tok0_stride=L - 1)
    torch.cuda.synchronize()
    d = p.outputs()
    assert all(is_sentinel(d[k][1:]) for k in ("cs0", "cs1", "hsb0", "hsb1", "out_b")) and all(is_sentinel(d[k]) for k in ("out", "gates0", "gates1", "a_all", "cat_b"))
    assert bool((lab.cpu() == 0x5B).all()) and is_sentinel(sc.cpu())
    b, bx = Bwd(B, T, L, seed=1), Exchange(B, "b")
    for code, change in ((KP_DEC_UNSUPPORTED, dict(L=600)), (KP_DEC_XBUF_SMALL, dict(xbuf_bytes=bx.xbuf.n * 8 - 8)), (KP_DEC_XTAB_SMALL, dict(xtab_bytes=8)),
                         (KP_DEC_ERR_SMALL, dict(err_ints=16)), (KP_DEC_BAD_ARGS, dict(epoch=0))):
        a = b.args()
        bx.fill(a)
        for k, v in change.items():
            setattr(a, k, v)
        capfd.readouterr()
        assert launch("kp_dec_cluster_backward", a) == code, change
        assert "[aocr] dec_" not in capfd.readouterr().err
    torch.cuda.synchronize()
    assert all(is_sentinel(v) for v in b.outputs().values())


# ------------------------------------------------------------------------------------------------------------------------------
# beam search (DEC + BEAM, HIST): dec_chain_beam_forward
# ------------------------------------------------------------------------------------------------------------------------------
class DecBeam(C.Structure):
    _fields_ = [("f", DecFwd), ("beam", i32), ("hist_tok", vp), ("hist_par", vp), ("beam_scores", vp)]


def beam_cases():
    return R.BEAM_CASES + [R.beam_cap_case(kp().kp_dec_chain_beam_group_cap())]


BEAM_IDS = [f"{c[0]}-{c[1]}-{c[2]}-{c[3]}{'-' + c[5] if c[5] else ''}" for c in R.BEAM_CASES] + ["xcd-cap"]
I16 = lambda t: t.contiguous().view(torch.int16)


class Beam:
    """The BEAM problem on the operands of Fwd(B, T, L, table=True, seed): GO tokens in column 1 of a [B][L + 3] window with JUNK around it, R.beam_projector
    (the planted twin classes; "eos": a boosted EOS bias), optional flat trie; pbuf / xtab sized for max(B, 32 group_cap) rows as in model.hip."""

    def __init__(self, B, T, L, k, seed, flags):
        self.B, self.T, self.L, self.k, self.seed = B, T, L, k, seed
        self.p = Fwd(B, T, L, table=True, seed=seed, lean=True, o=R.beam_operands(B, T, seed, flags))
        self.wo, self.bo = R.beam_projector(seed, flags)
        self.wod, self.bod = Buf(self.wo), Buf(self.bo)
        self.stride = L + 3
        host = torch.full((B * self.stride + 8,), int(JUNK), dtype=torch.int32)
        host[1 + self.stride * torch.arange(B)] = R.GO
        self.tok0 = Buf(host, torch.int32)
        self.cap = kp().kp_dec_chain_beam_group_cap()
        assert self.cap == per_pass(), f"dec_chain_beam_group_cap() = {self.cap}, from the compute units: {per_pass()}"
        rows = max(B, 32 * self.cap)
        self.pbuf = Buf(((kp().kp_dec_cluster_pbuf_bytes(rows) + 3) // 4,), fill=0.0)
        self.ex = Exchange(B, "f", tab_rows=rows)
        self.trie = R.beam_trie(seed, flags, L)
        self.tried = [Buf(torch.from_numpy(t.astype("int64") if i == 0 else t), torch.int64 if i == 0 else torch.int32) for i, t in enumerate(self.trie)] if self.trie else None
        ipg = 2 * (16 // k)
        self.groups = (B + ipg - 1) // ipg
        self.per = min(self.cap, self.groups, L * B // 128)                # dec_chain.hip: beam_pass_groups
        self.passes = (self.groups + self.per - 1) // self.per
        assert kp().kp_dec_chain_beam_supported(B, L, k, V) == 1 and kp().kp_dec_chain_beam_passes(B, L, k) == self.passes

    def args(self, hist):
        p, B, L, k = self.p, self.B, self.L, self.k
        p.fresh()
        self.hist_tok, self.hist_par = Buf((L, B, k), torch.int32, fill=0x5B), Buf((L, B, k), torch.int32, fill=0x5B)
        self.beam_scores, self.sc_hist = Buf((B, k), fill=SENT), Buf((L, B, k), fill=SENT)
        self.a_hist = Buf((L, B * k, self.T), fill=SENT)
        self.labels, self.scores = Buf((B * self.stride + 8,), torch.int32, fill=0x5B), Buf((B,), fill=SENT)
        a = DecBeam()
        a.f = p.args(gates=False)
        f = a.f
        f.zx_tok, f.greedy, f.V = None, 0, V
        f.tok0, f.tok0_stride, f.wo, f.bo = self.tok0.full.data_ptr() + 4, self.stride, self.wod.full.data_ptr(), self.bod.full.data_ptr()
        f.pbuf, f.pbuf_bytes, f.labels, f.scores = self.pbuf.full.data_ptr(), self.pbuf.n * 4, self.labels.full.data_ptr() + 4, self.scores.full.data_ptr()
        if hist:
            f.sc_hist, f.a_all = self.sc_hist.full.data_ptr(), self.a_hist.full.data_ptr()
        if self.tried:
            f.trie_mask, f.trie_base, f.trie_child = (b.full.data_ptr() for b in self.tried)
        a.beam, a.hist_tok, a.hist_par, a.beam_scores = k, self.hist_tok.full.data_ptr(), self.hist_par.full.data_ptr(), self.beam_scores.full.data_ptr()
        self.ex.fill(f, epochs=self.passes)
        return a

    def outputs_untouched(self, what, d, hist):
        """what the beam launcher must not write: labels / scores (the model's back-trace fills them from the history; dec_chain_beam_forward itself leaves
        them alone), the fp32 out, the gates, the cell-state slots, everything of hsb / out_b / cat_b outside the initial rows and the four rolling slots"""
        B, L, o, Rs = self.B, self.L, self.p.o, 32 * self.per
        assert bool((self.labels.cpu() == 0x5B).all()) and is_sentinel(self.scores.cpu()), f"{what}: labels / scores written by the beam launcher"
        assert all(is_sentinel(d[n]) for n in ("out", "gates0", "gates1")) and (hist or is_sentinel(d["a_all"])), f"{what}: out, gates or a_all written"
        assert is_sentinel(self.p.a_all.cpu()), f"{what}: the [L][B][T] attention buffer of the other kernels written"
        for l in range(2):
            assert same_bits(d[f"cs{l}"][0], o["c0"][l]) and is_sentinel(d[f"cs{l}"][1:]), f"{what}: cs[{l}] written"
        for n, init in (("hsb0", o["h0"][0]), ("hsb1", o["h0"][1]), ("out_b", o["feed0"])):
            flat = d[n].view(-1, H)
            assert same_bits(flat[:B], init.to(torch.bfloat16)), f"{what}: the initial rows of {n} changed"
            assert is_sentinel(flat[B + 4 * Rs:]), f"{what}: {n} written behind the four rolling step slots"
        assert is_sentinel(d["cat_b"].view(-1, 2 * H)[4 * Rs:]), f"{what}: cat_b written behind the four rolling step slots"

    def run(self, capfd, monkeypatch, env, hist):
        p, B, L, k = self.p, self.B, self.L, self.k
        setenv(monkeypatch, env)
        a = self.args(hist)
        capfd.readouterr()
        rc = launch("kp_dec_chain_beam_forward", a)
        assert rc == 0, f"wrapper / hipGetLastError() = {rc}"
        torch.cuda.synchronize()
        line, cfg = config_of(capfd, "dec_chain_beam_forward", others=("dec_cluster_forward", "dec_chain_forward"))
        inst = "dec" + (",res" if self.T <= 64 and "AOCR_CH_NO_RES" not in env else "") + ",beam" + (",hist" if hist else "")
        assert f": dec_ch_fwd_kernel[{inst}] {B} {self.T} {L} " in line, line
        assert cfg == dict(groups=self.groups, passes=self.passes, remote=1 if "AOCR_CL_REMOTE" in env else 0), (line, self.groups, self.passes)
        for n in env:
            monkeypatch.delenv(n)
        self.ex.ok(line)
        bufs = dict(hist_tok=self.hist_tok, hist_par=self.hist_par, beam_scores=self.beam_scores, sc_hist=self.sc_hist, a_hist=self.a_hist, labels=self.labels,
                    scores=self.scores, pbuf=self.pbuf, tok0=self.tok0, **p.bufs())
        for n, b in bufs.items():
            b.check_tail(f"{line} {n}")
        d = p.outputs()
        g = dict(line=line, hist_tok=self.hist_tok.cpu().clone().long(), hist_par=self.hist_par.cpu().clone().long(), beam_scores=self.beam_scores.cpu().clone(),
                 sc_hist=self.sc_hist.cpu().clone(), a_hist=self.a_hist.cpu().clone(), hsb0=d["hsb0"], hsb1=d["hsb1"], out_b=d["out_b"], cat_b=d["cat_b"])
        d["a_all"] = g["a_hist"]
        self.outputs_untouched(line, d, hist)
        if not hist:
            assert is_sentinel(g["sc_hist"]) and is_sentinel(g["a_hist"]), f"{line}: search history written without sc_hist"
        return g

    # ---- stage 1: the hypothesis tree of the device's own history, replayed by the teacher-forced kernel
    def prefixes(self, g):
        """pre[t][b][j]: the token prefix (GO, x_1 .. x_t) of the hypothesis in slot j of image b that ENTERS step t (kin = 1 at step 0)"""
        L, B, k = self.L, self.B, self.k
        ht, hp = g["hist_tok"], g["hist_par"]
        assert bool(((ht >= 1) & (ht <= V)).all()), "tokens outside 1..V"
        assert bool((hp[0] == 0).all()) and bool(((hp >= 0) & (hp < k)).all()), "parents outside the beam (step 0: one hypothesis per image)"
        pre = [[[(R.GO,)] for _ in range(B)]]
        for t in range(1, L):
            pre.append([[pre[t - 1][b][int(hp[t - 1, b, j])] + (int(ht[t - 1, b, j]),) for j in range(k)] for b in range(B)])
        return pre

    def replay(self, g, pre, images, check_images, capfd, monkeypatch, what, acc):
        """every distinct maximal prefix of `images` as one row of the teacher-forced kernel (context and initial state of the row's image); rp.check on the
        rows of check_images.  acc[name][t][b kin + j] <- the replay's values of the hypothesis that entered step t"""
        L, k, T = self.L, self.k, self.T
        allp = {(b, q) for t in range(L) for b in images for q in pre[t][b]}
        inner = {(b, q[:-1]) for b, q in allp if len(q) > 1}
        rows = sorted(allp - inner)
        at = {}
        for r, (b, q) in enumerate(rows):
            for n in range(1, len(q) + 1):
                at[(b, q[:n])] = r
        tok = torch.full((L, len(rows)), R.PAD, dtype=torch.int32)
        for r, (b, q) in enumerate(rows):
            tok[:len(q), r] = torch.tensor(q, dtype=torch.int32)
        rp = Fwd(len(rows), T, L, table=True, seed=self.seed, zx=(self.p.zx1, tok), o=R.take_rows(self.p.o, [b for b, _ in rows]), lean=True)
        run_fwd(rp, Exchange(len(rows), "f"), capfd, monkeypatch, {}, gates=False)
        crow = [r for r, (b, _) in enumerate(rows) if b in check_images]
        if crow:
            rp.check(f"{what} replay", gates=False, rows=None if len(crow) == len(rows) else crow)
        r = rp.outputs()
        for t in range(L):
            kin = 1 if t == 0 else k
            for b in images:
                for j in range(kin):
                    row = at[(b, pre[t][b][j])]
                    acc["out"][t][b * kin + j] = r["out"][t + 1, row]
                    acc["a"][t][b * kin + j] = r["a_all"][t, row]
                    if t >= L - 4:
                        for n in ("hsb0", "hsb1", "out_b"):
                            acc[n][t][b * kin + j] = r[n][t + 1, row]
                        acc["cat_h"][t][b * kin + j] = r["cat_b"][t, row, H:]
        return len(rows)

    def verify(self, g, capfd, monkeypatch, what, chunks=None, check_images=None):
        B, T, L, k = self.B, self.T, self.L, self.k
        pre = self.prefixes(g)
        kin_of = lambda t: 1 if t == 0 else k
        acc = dict(out=[torch.zeros(B * kin_of(t), H) for t in range(L)], a=[torch.zeros(B * kin_of(t), T) for t in range(L)])
        for n in ("hsb0", "hsb1", "out_b", "cat_h"):
            acc[n] = [torch.zeros(B * kin_of(t), H, dtype=torch.bfloat16) for t in range(L)]
        nrows = 0
        for images in (chunks or [list(range(B))]):
            nrows += self.replay(g, pre, images, set(range(B)) if check_images is None else check_images, capfd, monkeypatch, what, acc)
        fig = dict(rows=nrows)
        # HIST attention rows: [L][B k][T], row image * kin + hypothesis, kin = 1 at step 0; everything else keeps the sentinel
        worst = diff = total = 0
        for t in range(L):
            kin = kin_of(t)
            at = torch.tensor([b * kin + j for b in range(B) for j in range(kin)])                  # the history's row of (image, hypothesis)
            rest = torch.ones(B * k, dtype=torch.bool)
            rest[at] = False
            dev = g["a_hist"][t][at]
            worst = max(worst, ratio(dev, acc["a"][t].double(), TOL_A))
            diff += int((dev.view(torch.int32) != acc["a"][t].view(torch.int32)).sum()); total += dev.numel()
            assert is_sentinel(g["a_hist"][t][rest]), f"{what}: step {t}: attention rows other than image * kin + hypothesis written"
        assert worst <= 1.0, f"{what}: a_all error / tolerance = {worst:.3f}"
        assert diff == 0, f"{what}: {diff} of {total} a_all values differ in bits from the teacher-forced replay"
        fig.update(a=worst, a_share=diff / total)
        # the rolling slots of the last min(4, L) steps, groups of the last pass
        Rs, ipc, g0 = 32 * self.per, 16 // k, (self.passes - 1) * self.per
        diff = total = 0
        for t in range(max(0, L - 4), L):
            kin = kin_of(t)
            for gl in range(self.groups - g0):
                for c in range(2):
                    for lr in range(ipc * k):
                        b, j = ((g0 + gl) * 2 + c) * ipc + lr // k, lr % k
                        if b >= B:
                            continue
                        src = b * kin + (j if kin > 1 else 0)
                        row = gl * 32 + 16 * c + lr
                        for n in ("hsb0", "hsb1", "out_b"):
                            x = g[n].view(-1, H)[B + ((t + 1) & 3) * Rs + row]
                            diff += int((I16(x) != I16(acc[n][t][src])).sum()); total += H
                        x = g["cat_b"].view(-1, 2 * H)[(t & 3) * Rs + row, H:]
                        diff += int((I16(x) != I16(acc["cat_h"][t][src])).sum()); total += H
        assert diff == 0, f"{what}: {diff} of {total} bf16 values of the surviving step slots differ from the teacher-forced replay"
        fig.update(slot_share=diff / total)
        fig.update(self.selection(g, acc, what))
        return fig

    # ---- stage 2: every selection against tail_ref.beam_totals of the replay's out, the device's own previous scores, tokens and trie nodes
    def selection(self, g, acc, what):
        B, L, k, trie = self.B, self.L, self.k, self.trie
        ht, hp, sc = g["hist_tok"], g["hist_par"], g["sc_hist"]
        bits32 = lambda x: int(x.view(torch.int32))
        node = [[0] for _ in range(B)]
        totals, frees = [], []
        n = dict(picks=0, undecided=0, loose=0, ties=0, fallback=0, split=0, worst=0.0)
        for t in range(L):
            kin, first = (1 if t == 0 else k), t == 0
            lp, mag = R.logprobs(acc["out"][t], self.wo, self.bo)
            tolr = TOL_CELL + bound(mag.amax(dim=1), 512)                       # [B kin]: per parent row
            prev, psc = (None, None) if first else (ht[t - 1].reshape(-1), sc[t - 1].double())
            loc = None if trie is None else [x for b in range(B) for x in node[b]]
            tot = TR.beam_totals(lp, prev, psc, B, kin, V, trie, loc)
            totals.append(tot)
            frees.append(TR.beam_totals(lp, prev, psc, B, kin, V) if trie is not None else tot)
            tolc = tolr.view(B, kin, 1).expand(B, kin, V).reshape(B, kin * V)
            for b in range(B):
                wt = f"{what}: step {t} image {b}"
                c = R.pick_classes(tot[b], tolc[b], k)
                idx = [int(hp[t, b, i]) * V + int(ht[t, b, i]) - 1 for i in range(k)]
                assert all(int(hp[t, b, i]) < kin for i in range(k)), f"{wt}: a parent outside the {kin} hypotheses that entered the step"
                for i in range(k):
                    v, tl = tot[b, idx[i]].item(), tolc[b, idx[i]].item()
                    assert v >= c["kth"] - 2 * tl, f"{wt}: pick {i} (token {int(ht[t, b, i])} of parent {int(hp[t, b, i])}) has the reference total {v:.5f}, the k-th best is {c['kth']:.5f}"
                    e = abs(sc[t, b, i].item() - v) / tl
                    assert e <= 1.0, f"{wt}: pick {i}: score error / tolerance = {e:.3f}"
                    n["worst"] = max(n["worst"], e)
                    if i > 0:
                        assert sc[t, b, i].item() <= sc[t, b, i - 1].item(), f"{wt}: the scores increase from slot {i - 1} to slot {i}"
                    if i in c["fallback"]:
                        assert idx[i] == idx[0] and bits32(sc[t, b, i]) == bits32(sc[t, b, 0]), f"{wt}: pick {i} does not repeat pick 0 (fewer than {k} admissible)"
                        continue
                    assert idx[i] not in idx[:i], f"{wt}: candidate {idx[i]} chosen twice"
                    if i > 0 and tot[b, idx[i]] == tot[b, idx[i - 1]]:
                        assert idx[i - 1] < idx[i], f"{wt}: exactly tied candidates {idx[i - 1]}, {idx[i]} not in index order"
                    if not c["loose"][i]:
                        assert idx[i] == c["ref"][i], f"{wt}: pick {i} is candidate {idx[i]}, the reference's (decided) is {c['ref'][i]}"
                    if not first and int(ht[t, b, i]) == R.PAD and int(ht[t - 1, b, int(hp[t, b, i])]) in (R.PAD, R.EOS):
                        assert bits32(sc[t, b, i]) == bits32(sc[t - 1, b, int(hp[t, b, i])]), f"{wt}: pick {i}: PAD after a finished parent changes the score bits"
                n["picks"] += k; n["undecided"] += sum(c["undecided"]); n["loose"] += sum(c["loose"]); n["fallback"] += int(bool(c["fallback"]))
                n["ties"] += sum(1 for i in c["ties"] if idx[i] == c["ref"][i] and idx[i + 1] == c["ref"][i + 1])
                if trie is not None:
                    node[b] = [TR.trie_next(trie[0], trie[1], trie[2], node[b][int(hp[t, b, i])], int(ht[t, b, i]), first) for i in range(k)]
                    n["split"] += int(len({int(trie[0][x]) for x in node[b]}) > 1)
        share = n["undecided"] / n["picks"]
        assert share <= 0.02, f"{what}: the case lost its conditions: {share:.4f} of the picks are undecided"
        ok, txt, cnt = R.beam_conditions(ht, hp, totals, frees, k, trie is not None)
        assert ok, f"{what}: the case lost its conditions: {txt}"
        # (the nodes are checked through the admissibility of every later pick: that only bites where the hypotheses of an image sit at nodes with different children)
        assert trie is None or n["split"] >= L * B // 4, f"{what}: the case lost its conditions: only {n['split']} selections leave an image's hypotheses at nodes with different child sets"
        assert same_bits(g["beam_scores"], sc[L - 1]), f"{what}: beam_scores is not sc_hist of the last step"
        return dict(score=n["worst"], undecided=share, loose=n["loose"] / n["picks"], ties=n["ties"], fallback=n["fallback"], masked=cnt["masked"])

    def tail(self, g, what):
        """kp_beam_backtrace on the device's history against tail_ref.backtrace; tail_ref.recognize_gather of it finite and consistent with sc_hist"""
        B, L, k = self.B, self.L, self.k
        lab, scr = Buf((B, L), torch.int32, fill=0x5B), Buf((B,), fill=SENT)
        rc = getattr(kp(), "kp_beam_backtrace")(C.c_void_p(torch.cuda.current_stream().cuda_stream), self.hist_tok.ptr(), self.hist_par.ptr(), self.beam_scores.ptr(),
                                                lab.ptr(), scr.ptr(), L, B, k)
        torch.cuda.synchronize()
        assert rc == 0, f"kp_beam_backtrace: {rc}"
        labels, scores = TR.backtrace(g["hist_tok"], g["hist_par"], g["beam_scores"].double())
        assert torch.equal(lab.cpu().long(), labels) and same_bits(scr.cpu(), scores.float()), f"{what}: beam_backtrace differs from tail_ref.backtrace"
        cl, at = TR.recognize_gather(labels, g["hist_par"], g["beam_scores"].double(), g["sc_hist"].double(), g["a_hist"])
        assert bool(torch.isfinite(cl).all()) and bool(torch.isfinite(at).all()), f"{what}: recognize_gather of the history is not finite"
        for b in range(B):
            tend = next((t for t in range(L) if int(labels[b, t]) in (R.PAD, R.EOS)), L - 1)
            idx = TR.winner(g["beam_scores"][b].double())[0]
            for t in range(L - 1, tend, -1):
                idx = int(g["hist_par"][t, b, idx])
            assert abs(cl[b, :tend + 1].sum().item() - g["sc_hist"][tend, b, idx].item()) <= 1e-4, f"{what}: image {b}: per-character scores do not sum to sc_hist on the winner"
            assert bool(((at[b, :tend + 1].sum(1) - 1).abs() <= 1e-4).all()), f"{what}: image {b}: an attention row of the winner does not sum to 1"


def same_history(a, b):
    return torch.equal(a["hist_tok"], b["hist_tok"]) and torch.equal(a["hist_par"], b["hist_par"]) and same_bits(a["beam_scores"], b["beam_scores"])


@pytest.mark.parametrize("i", range(len(BEAM_IDS)), ids=BEAM_IDS)
def test_beam(i, cuda, capfd, monkeypatch):
    """Measured on an MI355X (group cap 8), per case: see the module docstring's table"""
    B, T, L, k, seed, flags = beam_cases()[i]
    q = Beam(B, T, L, k, seed, flags)
    g = q.run(capfd, monkeypatch, {}, hist=True)
    chunks = check_images = None
    if i == len(BEAM_IDS) - 1:                                         # the XCD-cap case: selection on all images, replay group by group, rp.check on the first and last image of each pass
        chunks = [list(range(b, min(b + 4, B))) for b in range(0, B, 4)]
        check_images = {0, 4 * q.per - 1, 4 * q.per, B - 1}
    fig = q.verify(g, capfd, monkeypatch, BEAM_IDS[i], chunks, check_images)
    q.tail(g, BEAM_IDS[i])
    report = [f"[dec-kernels] {g['line'][7:]}: replay rows {fig['rows']}, a_all {fig['a']:.3f} (mismatch share {fig['a_share']:.0f}), slot mismatch share {fig['slot_share']:.0f}, "
              f"score increment {fig['score']:.3f}, undecided {fig['undecided']:.4f} (membership check only, with their upper neighbours: {fig['loose']:.4f}), ties won {fig['ties']}, fallback selections {fig['fallback']}, steps masked {fig['masked']}"]
    runs = [("no history", {}), ("AOCR_CL_REMOTE=1", {"AOCR_CL_REMOTE": "1"})] + ([("AOCR_CH_NO_RES=1", {"AOCR_CH_NO_RES": "1"})] if T <= 64 else [])
    for name, env in runs:                                             # each on the used buffers, the epoch advanced by the pass count
        h = q.run(capfd, monkeypatch, env, hist=False)
        assert same_history(g, h), f"{name}: hist_tok / hist_par / beam_scores differ from the first [.., hist] run"
        report.append(f"[dec-kernels] {h['line'][7:]} ({name}): bit-identical history")
    h = q.run(capfd, monkeypatch, {}, hist=True)
    assert same_history(g, h) and same_bits(g["sc_hist"], h["sc_hist"]) and same_bits(g["a_hist"], h["a_hist"]), "a second [.., hist] call on the used buffers differs"
    print("\n".join(report))


def test_beam_switch_and_refusals(cuda, capfd, monkeypatch):
    """AOCR_NO_DEC_CHAINS_BEAM=1 and every refusal of kp_dec_chain_beam_forward: its code, no trace line, every buffer still all-sentinel"""
    B, T, L, k, seed, flags = R.BEAM_CASES[2]
    assert k == 3
    q = Beam(B, T, L, k, seed, flags)
    rows = max(B, 32 * q.cap)
    bad, tok0 = [], q.tok0.cpu().clone()

    def refused(code, env=None, **change):
        setenv(monkeypatch, env or {})
        a = q.args(hist=True)
        for n, v in change.items():
            setattr(a if n in ("beam", "hist_tok", "hist_par", "beam_scores") else a.f, n, v)
        capfd.readouterr()
        rc = launch("kp_dec_chain_beam_forward", a)
        torch.cuda.synchronize()
        for n in (env or {}):
            monkeypatch.delenv(n)
        assert rc == code, (change, env, rc)
        assert "[aocr] dec_" not in capfd.readouterr().err, change
        d = q.p.outputs()
        ok = all(is_sentinel(d[n].view(-1, H)[B:]) for n in ("hsb0", "hsb1", "out_b")) and all(is_sentinel(d[n]) for n in ("out", "cat_b", "a_all", "gates0", "gates1"))
        ok = ok and all(bool((b.cpu() == 0x5B).all()) for b in (q.hist_tok, q.hist_par, q.labels)) and all(is_sentinel(b.cpu()) for b in (q.beam_scores, q.sc_hist, q.a_hist, q.scores))
        ok = ok and all(bool((b.cpu() == 0).all()) for b in (q.pbuf, q.ex.xbuf, q.ex.xtab, q.ex.err)) and torch.equal(q.tok0.cpu(), tok0)
        ok = ok and all(same_bits(d[f"cs{l}"][0], q.p.o["c0"][l]) and is_sentinel(d[f"cs{l}"][1:]) for l in range(2))
        ok = ok and all(same_bits(d[n].view(-1, H)[:B], init.to(torch.bfloat16)) for n, init in (("hsb0", q.p.o["h0"][0]), ("hsb1", q.p.o["h0"][1]), ("out_b", q.p.o["feed0"])))
        if not ok:
            bad.append((change, env))

    monkeypatch.setenv("AOCR_NO_DEC_CHAINS_BEAM", "1")
    assert kp().kp_dec_chain_beam_supported(B, L, k, V) == 0
    monkeypatch.delenv("AOCR_NO_DEC_CHAINS_BEAM")
    refused(KP_DEC_UNSUPPORTED, env={"AOCR_NO_DEC_CHAINS_BEAM": "1"})
    refused(KP_DEC_UNSUPPORTED, env={"AOCR_NO_DEC_CHAINS": "1"})
    assert kp().kp_dec_chain_beam_supported(B, L, 1, V) == 0 and kp().kp_dec_chain_beam_supported(B, L, 9, V) == 0 and kp().kp_dec_chain_beam_supported(B, L, k, 41) == 0
    assert kp().kp_dec_chain_beam_supported(B, 128 // B, k, V) == 0 and kp().kp_dec_chain_beam_passes(B, 128 // B, k) == 0      # L B < 128: no group fits the four slots
    refused(KP_DEC_UNSUPPORTED, beam=1)
    refused(KP_DEC_UNSUPPORTED, beam=9)
    refused(KP_DEC_UNSUPPORTED, V=41)
    refused(KP_DEC_UNSUPPORTED, L=128 // B)                            # !dec_chain_beam_supported
    refused(KP_DEC_UNSUPPORTED, Hd=1024)                               # !dec_cluster_supported
    refused(KP_DEC_UNSUPPORTED, T=257)
    refused(KP_DEC_BAD_ARGS, epoch=0)
    refused(KP_DEC_BAD_ARGS, epoch=(1 << 20) - q.passes)
    refused(KP_DEC_BAD_ARGS, hist_tok=None)
    refused(KP_DEC_BAD_ARGS, hist_par=None)
    refused(KP_DEC_BAD_ARGS, beam_scores=None)
    refused(KP_DEC_BAD_ARGS, tok0_stride=L - 1)
    refused(KP_DEC_XBUF_SMALL, xbuf_bytes=q.ex.xbuf.n * 8 - 8)
    refused(KP_DEC_PBUF_SMALL, pbuf_bytes=kp().kp_dec_cluster_pbuf_bytes(rows) - 4)
    refused(KP_DEC_PBUF_SMALL, pbuf_bytes=kp().kp_dec_cluster_pbuf_bytes(B))          # sized for B rows as for the greedy kernel: below the launch's group cap
    refused(KP_DEC_XTAB_SMALL, xtab_bytes=kp().kp_dec_cluster_xtab_bytes(rows) - 8)
    refused(KP_DEC_XTAB_SMALL, xtab_bytes=kp().kp_dec_cluster_xtab_bytes(B))
    refused(KP_DEC_ERR_SMALL, err_ints=16 + 256 * 4)
    assert not bad, f"a refused call wrote a buffer: {bad}"
