"""Float64 restatement of ONE step of the attention decoder and of its backward step, as the whole-sequence decoder kernels run them
(csrc/dec_cluster.hip, csrc/dec_chain.hip; model.lua:553-568 teacher-forced loop, :643-661 BPTT; cell LSTM.lua:79-105, attention LSTM.lua:124-162),
written from oracle/oracle_torch.py (decoder_step_fwd, attn_fwd / attn_bwd, lstm_cell_bwd) and the header of dec_cluster.hip.
Used by tests/test_dec_seq_ref_cpu.py (held there to oracle_torch and torch autograd) and tests/test_decoder_seq_kernels_gpu.py.

Conventions (csrc/ops.h: DecClFwdArgs / DecClBwdArgs; H = Hd = 512, two layers, input feed):
  W1i, W1h, W2i, W2h  [4H][H]   gate-major rows [in, forget, out, g]; W1i is the FEED part of layer 1's W_i2h (columns E..E+H)
  zx1     [L][B][4H]            the embedding part of layer 1's pre-activation incl. both biases, or a per-token table [V][4H] + tokens [L][B]
  b2      [4H]                  b2_i2h + b2_h2h
  Wa [H][H], Wc [H][2H]         q = Wa h2;  out = tanh(Wc [c ; h2])
  ctx     [B][T][H]             bf16-exact;  ctxa = RNE(ctx Wa): s = ctxa . h2 = ctx . (Wa h2)
  slots   cs[l], hs[l], out: [L+1][B][H], slot t+1 holds step t, slot 0 the initial state (out slot 0 = the initial feed)
  gates   [L][B][4][H] here;  the kernels save them INTERLEAVED per unit, [L][B][H][4] (il / unil below);  d z is gate-major [L][B][4H]

Where the kernels exchange bf16, the reference rounds (RNE of the fp32 image): h1, h2, the c half of [c ; h2], out (as the feed and as the bf16 copy), and in
the backward pass d z, d pre and d q as the operands of the products that follow.  round=False switches every rounding off (the exact recurrence, which
the CPU test holds to oracle_torch).

Two modes.  FREE-RUNNING (forward, backward): the recurrence on its own state.  FED (step_fed, bwd_step_fed): every stage of step t from the DEVICE's saved
inputs of that stage, so nothing compounds: a stage is an independent one-step problem whose noise is its fp32 product and its transcendental functions."""
import torch

F64 = torch.float64
H = 512
V = 39


def rne(x):
    """bf16 image (round to nearest even) of the fp32 image of x, as float64"""
    return x.float().to(torch.bfloat16).to(F64)


def il(g):
    """gates [..., 4, H] -> the kernels' interleaved layout, flat [..., 4H] = [unit][i, f, o, g]"""
    return g.transpose(-1, -2).reshape(*g.shape[:-2], -1)


def unil(flat, Hn=H):
    """inverse of il: [..., 4H] -> [..., 4, H]"""
    return flat.reshape(*flat.shape[:-1], Hn, 4).transpose(-1, -2)


def cell(z, c_prev):
    """z [B][4H] gate-major -> c, h, gates [B][4][H]"""
    B = z.shape[0]
    z = z.view(B, 4, -1)
    i, f, o, g = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.sigmoid(z[:, 2]), torch.tanh(z[:, 3])
    c = f * c_prev + i * g
    return c, o * torch.tanh(c), torch.stack([i, f, o, g], 1)


def cell_backward(dh, dc_in, gates, c, c_prev):
    """gates [B][4][H] -> d z [B][4H] gate-major, the d c that leaves the step"""
    i, f, o, g = gates[:, 0], gates[:, 1], gates[:, 2], gates[:, 3]
    tc = torch.tanh(c)
    dc = dh * o * (1 - tc * tc) + dc_in
    dz = torch.stack([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dh * tc * o * (1 - o), dc * i * (1 - g * g)], 1)
    return dz.reshape(dz.shape[0], -1), dc * f


def attention(h2b, ctx, ctxa):
    """-> a [B][T], c [B][H], |ctxa| . |h2| [B][T]"""
    s = torch.einsum("btj,bj->bt", ctxa, h2b)
    a = torch.softmax(s, dim=1)
    return a, torch.einsum("bt,btj->bj", a, ctx), torch.einsum("btj,bj->bt", ctxa.abs(), h2b.abs())


class Weights:
    """float64 views of one problem's operands (all exact in their device types)"""

    def __init__(self, W1i, W1h, W2i, W2h, b2, Wa, Wc, ctx, ctxa=None):
        d = lambda t: t.to(F64)
        self.W1i, self.W1h, self.W2i, self.W2h, self.b2, self.Wa, self.Wc, self.ctx = d(W1i), d(W1h), d(W2i), d(W2h), d(b2), d(Wa), d(Wc), d(ctx)
        self.ctxa = d(ctxa) if ctxa is not None else self.ctx @ self.Wa


def zx_at(zx1, tok, t):
    """the gate input of step t: a row block of the [L][B][4H] tensor, or the table rows of the step's tokens (1-based, clamped as the kernels clamp)"""
    if tok is None:
        return zx1[t].to(F64)
    return zx1.to(F64)[tok[t].long().clamp(1, zx1.shape[0]) - 1]


def forward(w, zx1, c0, h0, feed0, L, tok=None, round=True, mask_h=None, mask_out=None):
    """free-running.  c0, h0: [2][B][H]; feed0 [B][H]; masks [L][B][H] (nn.Dropout on layer 2's input and on the attention output) or None.
    -> dict of float64 tensors: cs, hs [2][L+1][B][H]; out [L+1][B][H]; gates [2][L][B][4][H]; z [2][L][B][4H]; pre [L][B][H]; a [L][B][T]; c [L][B][H]"""
    r = rne if round else (lambda x: x)
    B, T = w.ctx.shape[0], w.ctx.shape[1]
    cs, hs = torch.zeros(2, L + 1, B, H, dtype=F64), torch.zeros(2, L + 1, B, H, dtype=F64)
    out = torch.zeros(L + 1, B, H, dtype=F64)
    gates, z = torch.zeros(2, L, B, 4, H, dtype=F64), torch.zeros(2, L, B, 4 * H, dtype=F64)
    pre, a_all, c_all = torch.zeros(L, B, H, dtype=F64), torch.zeros(L, B, T, dtype=F64), torch.zeros(L, B, H, dtype=F64)
    cs[:, 0], hs[:, 0], out[0] = c0.to(F64), h0.to(F64), feed0.to(F64)
    for t in range(L):
        z[0, t] = zx_at(zx1, tok, t) + r(out[t]) @ w.W1i.t() + r(hs[0, t]) @ w.W1h.t()
        cs[0, t + 1], hs[0, t + 1], gates[0, t] = cell(z[0, t], cs[0, t])
        x2 = hs[0, t + 1] if mask_h is None else hs[0, t + 1] * mask_h[t]
        z[1, t] = w.b2 + r(x2) @ w.W2i.t() + r(hs[1, t]) @ w.W2h.t()
        cs[1, t + 1], hs[1, t + 1], gates[1, t] = cell(z[1, t], cs[1, t])
        h2b = r(hs[1, t + 1])
        a_all[t], c_all[t], _ = attention(h2b, w.ctx, w.ctxa)
        pre[t] = torch.cat([r(c_all[t]), h2b], 1) @ w.Wc.t()
        out[t + 1] = torch.tanh(pre[t]) if mask_out is None else torch.tanh(pre[t]) * mask_out[t]
    return dict(cs=cs, hs=hs, out=out, gates=gates, z=z, pre=pre, a=a_all, c=c_all)


def step_fed(w, zx_t, feed_b, h1p, h2p, c1p, c2p, h1b, h2b, cat_b, x2b=None):
    """step t, every stage from the device's own inputs (bf16 tensors as float64): feed_b = out_b[t], h1p / h2p = hsb[l][t], c1p / c2p = cs[l][t];
    h1b / h2b = the device's hsb[l][t+1] (operands of layer 2 and of the attention; x2b: the masked copy under dropout), cat_b = the device's [c ; h2].
    -> dict: c1, h1, g1, c2, h2, g2, a, c, out (before any dropout mask) and the magnitudes m1, m2 [B][4H], ms [B][T], mo [B][H] their fp32 products scale with"""
    z1 = zx_t + feed_b @ w.W1i.t() + h1p @ w.W1h.t()
    c1, h1, g1 = cell(z1, c1p)
    x2 = h1b if x2b is None else x2b
    z2 = w.b2 + x2 @ w.W2i.t() + h2p @ w.W2h.t()
    c2, h2, g2 = cell(z2, c2p)
    a, c, ms = attention(h2b, w.ctx, w.ctxa)
    pre = cat_b @ w.Wc.t()
    return dict(c1=c1, h1=h1, g1=g1, c2=c2, h2=h2, g2=g2, a=a, c=c, out=torch.tanh(pre), z=torch.cat([z1, z2, pre], 1),
                m1=feed_b.abs() @ w.W1i.abs().t() + h1p.abs() @ w.W1h.abs().t(), m2=x2.abs() @ w.W2i.abs().t() + h2p.abs() @ w.W2h.abs().t(),
                ms=ms, mo=cat_b.abs() @ w.Wc.abs().t())


def attention_backward(ctx, a, dc):
    da = torch.einsum("btj,bj->bt", ctx, dc)
    ds = a * (da - (a * da).sum(1, keepdim=True))
    return da, ds, torch.einsum("bt,btj->bj", ds, ctx)


def bwd_step_fed(w, s, dout_t, dz1n, dz2n, dc1, dc2, fed=None, round=True, mask_h=None, mask_out=None):
    """backward step t.  s: the saved forward state of the step, dict(out [B][H] (= out slot t+1, masked under dropout), a [B][T], g1, g2 [B][4][H],
    c1, c1p, c2, c2p [B][H]).  dz1n, dz2n: d z of step t+1 ([B][4H], zeros at t = L-1) as the products read them -- the device's own bf16 in the fed mode.
    dc1, dc2: the d c entering the step.  fed: the device's dpre_b, dcat_c (fp32 c half of d cat), dq_b, dzb2 of THIS step (None: the reference's own, rounded).
    -> dict: dpre, dcat_c, da, ds, dq, dz2, dz1, dc1, dc2, dh (the largest |d h| of the step) and the magnitudes m_pre, m_cat, m_da, m_z2, m_z1"""
    r = rne if round else (lambda x: x)
    dfeed, dh1rec, dh2rec = dz1n @ w.W1i, dz1n @ w.W1h, dz2n @ w.W2h
    if mask_out is None:
        dpre = (dout_t + dfeed) * (1 - s["out"] ** 2)
    else:
        o = torch.where(mask_out != 0, s["out"] / torch.where(mask_out != 0, mask_out, torch.ones_like(mask_out)), torch.zeros_like(s["out"]))
        dpre = (dout_t + dfeed) * mask_out * (1 - o * o)
    dpre_b = fed["dpre_b"] if fed else r(dpre)
    dcat = dpre_b @ w.Wc
    dcat_c = fed["dcat_c"] if fed else dcat[:, :H]
    da, ds, dq = attention_backward(w.ctx, s["a"], dcat_c)
    dq_b = fed["dq_b"] if fed else r(dq)
    dh2 = dq_b @ w.Wa + dcat[:, H:] + dh2rec
    dz2, dc2o = cell_backward(dh2, dc2, s["g2"], s["c2"], s["c2p"])
    dzb2 = fed["dzb2"] if fed else r(dz2)
    dx2 = dzb2 @ w.W2i
    dh1 = (dx2 if mask_h is None else dx2 * mask_h) + dh1rec
    dz1, dc1o = cell_backward(dh1, dc1, s["g1"], s["c1"], s["c1p"])
    A = torch.abs
    return dict(dpre=dpre, dcat_c=dcat[:, :H], da=da, ds=ds, dq=dq, dz2=dz2, dz1=dz1, dc1=dc1o, dc2=dc2o,
                dh=max((dout_t + dfeed).abs().max().item(), dh2.abs().max().item(), dh1.abs().max().item()),
                m_pre=A(dz1n) @ A(w.W1i), m_cat=A(dpre_b) @ A(w.Wc)[:, :H], m_da=torch.einsum("btj,bj->bt", A(w.ctx), A(dcat_c)),
                m_z2=A(dq_b) @ A(w.Wa) + A(dpre_b) @ A(w.Wc)[:, H:] + A(dz2n) @ A(w.W2h), m_z1=A(dzb2) @ A(w.W2i) + A(dz1n) @ A(w.W1h))


def saved_step(f, t):
    """the saved state of step t of a forward dict (free-running reference, or its fp32 images as float64)"""
    return dict(out=f["out"][t + 1], a=f["a"][t], g1=f["gates"][0, t], g2=f["gates"][1, t], c1=f["cs"][0, t + 1], c1p=f["cs"][0, t],
                c2=f["cs"][1, t + 1], c2p=f["cs"][1, t])


def backward(w, f, dout, round=True, mask_h=None, mask_out=None):
    """free-running BPTT over a forward dict.  dout [L][B][H].  -> dict(dpre, dq [L][B][H], ds [L][B][T], dcat_c, dz [2][L][B][4H], dc_st [2][B][H],
    dh_rec [2][B][H], dfeed [B][H])"""
    L, B = dout.shape[0], dout.shape[1]
    r = rne if round else (lambda x: x)
    zero = torch.zeros(B, 4 * H, dtype=F64)
    dz = torch.zeros(2, L, B, 4 * H, dtype=F64)
    o = dict(dpre=torch.zeros(L, B, H, dtype=F64), dq=torch.zeros(L, B, H, dtype=F64), dcat_c=torch.zeros(L, B, H, dtype=F64),
             ds=torch.zeros(L, B, w.ctx.shape[1], dtype=F64))
    dc1 = dc2 = torch.zeros(B, H, dtype=F64)
    for t in range(L - 1, -1, -1):
        n1, n2 = (r(dz[0, t + 1]), r(dz[1, t + 1])) if t < L - 1 else (zero, zero)
        st = bwd_step_fed(w, saved_step(f, t), dout[t].to(F64), n1, n2, dc1, dc2, round=round, mask_h=None if mask_h is None else mask_h[t],
                          mask_out=None if mask_out is None else mask_out[t])
        dz[0, t], dz[1, t], dc1, dc2 = st["dz1"], st["dz2"], st["dc1"], st["dc2"]
        for k in ("dpre", "dq", "dcat_c", "ds"):
            o[k][t] = st[k]
    z1, z2 = r(dz[0, 0]), r(dz[1, 0])
    o.update(dz=dz, dc_st=torch.stack([dc1, dc2]), dh_rec=torch.stack([z1 @ w.W1h, z2 @ w.W2h]), dfeed=z1 @ w.W1i)
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# operand generators of the GPU test (here, so that the CPU test can assert their conditions on every shape the GPU test uses)
# ------------------------------------------------------------------------------------------------------------------------------
Q = 2.0 ** -4                       # gate weights and W_c: integers in [-2, 2] times Q, exact in bf16.  With |h| < 1 a K = 1024 product has a standard
W_INT = 2                           # deviation of ~sqrt(1024 * 2) * 0.3 / 16 = 0.85; with zx uniform in [-2, 2] well over 90 % of |z| stays inside 4
QA = 2.0 ** -6                      # W_a quantum: ctx W_a has a standard deviation of sqrt(512 * 2 * 2) / 256 = 0.18, the scores of ~1
QC = 2.0 ** -2                      # context: integers in [-2, 2] times QC
ZX_SCALE = 2.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, q, seed):
    return torch.randint(-W_INT, W_INT + 1, shape, generator=_gen(seed)).float() * q


def uniform(shape, scale, seed):
    return ((torch.rand(*shape, generator=_gen(seed), dtype=F64) * 2 - 1) * scale).float()


def operands(B, T, seed):
    """-> dict of float32 tensors exact in their device types: W1i, W1h, W2i, W2h [4H][H], Wa [H][H], Wc [H][2H] (bf16-exact), b2i, b2h [4H],
    ctx [B][T][H] (bf16-exact), ctxa = RNE(ctx Wa), c0 [2][B][H], h0 [2][B][H] and feed0 [B][H] (bf16-exact)"""
    o = {n: _ints((4 * H, H), Q, seed * 16 + i) for i, n in enumerate(("W1i", "W1h", "W2i", "W2h"))}
    o["Wa"], o["Wc"] = _ints((H, H), QA, seed * 16 + 4), _ints((H, 2 * H), Q, seed * 16 + 5)
    o["b2i"], o["b2h"] = uniform((4 * H,), 0.5, seed * 16 + 6), uniform((4 * H,), 0.5, seed * 16 + 7)
    o["ctx"] = _ints((B, T, H), QC, seed * 16 + 8)
    o["ctxa"] = rne(o["ctx"].double() @ o["Wa"].double()).float()            # the product is exact in float64 (multiples of 2^-8 below 2^45)
    o["c0"] = uniform((2, B, H), 0.5, seed * 16 + 9)
    o["h0"] = rne(uniform((2, B, H), 0.5, seed * 16 + 10)).float()
    o["feed0"] = rne(uniform((B, H), 0.5, seed * 16 + 11)).float()
    return o


def weights_of(o):
    return Weights(o["W1i"], o["W1h"], o["W2i"], o["W2h"], o["b2i"].double() + o["b2h"].double(), o["Wa"], o["Wc"], o["ctx"], o["ctxa"])


def gate_inputs(L, B, seed, table):
    """-> (zx1, tok): random fp32 [L][B][4H] and None, or the per-token table [V][4H] and tokens [L][B] in 1..V"""
    if not table:
        return uniform((L, B, 4 * H), ZX_SCALE, seed * 16 + 12), None
    return uniform((V, 4 * H), ZX_SCALE, seed * 16 + 12), torch.randint(1, V + 1, (L, B), generator=_gen(seed * 16 + 13), dtype=torch.int32)


def z_share(z):
    """share of the pre-activations inside |z| <= 4"""
    return (z.abs() <= 4).double().mean().item()


def per_pass(cus):
    """groups of 32 rows one launch holds (dec_cluster.hip / dec_chain.hip: 32 compute units per group, whole sets of 8 groups)"""
    return max(8, cus // (8 * 32) * 8)


# (B, T, L) of the teacher-forced forward / backward problems of tests/test_decoder_seq_kernels_gpu.py; the two-pass shape depends on the device
# (32 per_pass + 4 rows) and is added there -- the CPU test takes it at per_pass = 8
TF_SHAPES = [(1, 1, 1), (7, 15, 2), (16, 16, 3), (17, 17, 3), (32, 64, 2), (33, 65, 3), (45, 5, 5), (5, 256, 2)]
DROP_SHAPE = (45, 5, 3)


# ------------------------------------------------------------------------------------------------------------------------------
# greedy decode (the kernels' DEC instantiations; model.lua:376-536 at beam 1, the selection of project_select_kernel)
# ------------------------------------------------------------------------------------------------------------------------------
PAD, GO, EOS = 1, 2, 3
TIE = (10, 20)                      # two classes with identical W_o rows and biases: their logits are bit-equal whatever out is; the lower id wins a tie
WO_SCALE = 40.0                     # test_greedy_decode_cluster_kernel_matches_launch_chain: the arg-max is not a coin toss between 39 near-equal classes
# (B, T, L, seed) of the greedy cases: seeds picked with the free-running reference below so that >= 3 rows emit EOS before step L, one never does,
# and at B = 33 the one-row second group finishes early while the first does not (tests/test_dec_seq_ref_cpu.py asserts it)
GREEDY_CASES = [(45, 5, 12, 27), (33, 65, 6, 75)]


def projector(seed):
    """-> W_o [V][H], b_o [V] float32 with the planted twin classes"""
    wo = uniform((V, H), WO_SCALE / H ** 0.5, seed * 16 + 15)
    bo = uniform((V,), 0.5, seed * 16 + 3)
    wo[TIE[1] - 1], bo[TIE[1] - 1] = wo[TIE[0] - 1], bo[TIE[0] - 1]
    return wo, bo


def logprobs(out, wo, bo):
    """float64 projector + LogSoftMax of out [B][H] -> (logp [B][V], |out| . |W_o| [B][V])"""
    x = out.to(F64) @ wo.to(F64).t() + bo.to(F64)
    return torch.log_softmax(x, dim=1), out.to(F64).abs() @ wo.to(F64).abs().t()


def admissible(trie, node, t):
    """bool [V]: the classes the row's trie node continues; PAD is always admissible after the first step (model.lua:413,469)"""
    ok = torch.tensor([bool((int(trie[0][node]) >> v) & 1) for v in range(V)])
    if t > 0:
        ok[PAD - 1] = True
    return ok


def trie_step(trie, node, label, t):
    """PAD keeps the node, any other admissible token moves to the child (model.lua:499-507)"""
    mask, base, child = trie
    m = int(mask[node])
    if (t > 0 and label == PAD) or not (m >> (label - 1)) & 1:
        return node
    return int(child[int(base[node]) + bin(m & ((1 << (label - 1)) - 1)).count("1")])


def greedy(w, table, wo, bo, c0, h0, feed0, L, trie=None):
    """free-running greedy decode from GO -> dict(labels [B][L] int64, logp [L][B][V] (the rule's totals BEFORE the running score is added; -inf where the
    trie forbids), scores [L][B] running, out [L+1][B][H])"""
    B = c0.shape[1]
    cs, hs, out = [c0[0].to(F64), c0[1].to(F64)], [h0[0].to(F64), h0[1].to(F64)], feed0.to(F64)
    tok = torch.full((B,), GO, dtype=torch.int64)
    labels, lps, scores, outs = torch.zeros(B, L, dtype=torch.int64), [], [], [out]
    score, node = torch.zeros(B, dtype=F64), [0] * B
    for t in range(L):
        z1 = table.to(F64)[tok - 1] + rne(out) @ w.W1i.t() + rne(hs[0]) @ w.W1h.t()
        cs[0], hs[0], _ = cell(z1, cs[0])
        z2 = w.b2 + rne(hs[0]) @ w.W2i.t() + rne(hs[1]) @ w.W2h.t()
        cs[1], hs[1], _ = cell(z2, cs[1])
        h2b = rne(hs[1])
        _, c, _ = attention(h2b, w.ctx, w.ctxa)
        out = torch.tanh(torch.cat([rne(c), h2b], 1) @ w.Wc.t())
        lp, _ = logprobs(out.float(), wo, bo)                          # (the projector reads the fp32 out)
        if t > 0:
            done = (tok == PAD) | (tok == EOS)
            lp[done, PAD - 1] = 0.0
        if trie is not None:
            for b in range(B):
                lp[b, ~admissible(trie, node[b], t)] = -float("inf")
        tok = lp.argmax(dim=1) + 1                                     # (first maximum: ties -> the lowest id)
        score = score + lp[torch.arange(B), tok - 1]
        if trie is not None:
            node = [trie_step(trie, node[b], int(tok[b]), t) for b in range(B)]
        labels[:, t] = tok
        lps.append(lp); scores.append(score.clone()); outs.append(out)
    return dict(labels=labels, logp=torch.stack(lps), scores=torch.stack(scores), out=torch.stack(outs))


def eos_step(labels):
    """per row: the step that emits EOS (L if none)"""
    L = labels.shape[1]
    return torch.tensor([next((t for t in range(L) if int(r[t]) == EOS), L) for r in labels])


def end_step(labels):
    """per row: the first step that emits EOS or PAD (L if none): from the next step on the rule selects PAD at no cost (model.lua:448-449)"""
    L = labels.shape[1]
    return torch.tensor([next((t for t in range(L) if int(r[t]) in (EOS, PAD)), L) for r in labels])


def greedy_conditions(labels, B):
    """the conditions on a greedy case's inputs -> (ok, text)"""
    L = labels.shape[1]
    e = eos_step(labels)
    early = int((e < L - 1).sum())
    ok = early >= 3 and bool((e == L).any())
    if B == 33:
        ok = ok and int(e[32]) < L - 2 and bool((e[:32] >= L - 1).any())
    return ok, f"EOS steps {e.tolist()}"


def words(seed, n=25, alphabet="abcdefghij0123", lo=1, hi=4):
    """a small word list in the style of tests/test_dict_gpu.py's"""
    g = _gen(seed)
    pick = lambda k: int(torch.randint(0, k, (1,), generator=g))
    return ["".join(alphabet[pick(len(alphabet))] for _ in range(lo + pick(hi - lo + 1))) for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------------------------
# beam search (the kernels' BEAM instantiations; model.lua:360-536, the rule of tail_ref.beam_step / select_topk / gather_rows)
# ------------------------------------------------------------------------------------------------------------------------------
EOS_BOOST = 6.0                     # flag "eos": added to the EOS bias, so that hypotheses finish early and compete with live ones
# (B, T, L, k, seed, flags) of the beam cases of tests/test_decoder_seq_kernels_gpu.py; flags: "" / "dict-<alphabet>" (beam_words) / "eos" / "pool".  Seeds picked with the
# free-running reference below so that beam_conditions holds (tests/test_dec_seq_ref_cpu.py asserts it).  The XCD-cap shape depends on the device
# (beam_cap_case) and is added there -- the CPU test takes it at a cap of 8 groups.
BEAM_CASES = [(16, 5, 8, 2, 104, ""), (5, 17, 26, 3, 151, ""), (11, 16, 12, 3, 122, ""), (11, 16, 24, 3, 50, ""), (7, 65, 20, 5, 35, ""), (9, 64, 16, 7, 87, ""),
              (11, 16, 12, 3, 51, "dict-6ga"), (9, 64, 16, 7, 52, "dict-6g"), (11, 16, 12, 3, 50, "eos")]
BEAM_CAP_SEED = 62
# The XCD-cap case ("pool"): a search of 32 steps at k = 8 keeps hypotheses that differ in one early token and end within fp32 rounding of each other, more of
# them than the near-tie cap allows in a batch taken as generated.  The images of a batch do not interact, so the case takes its images (context, ctx W_a,
# initial state) as rows of a larger batch of `operands` with the case's seed -- weights, token table and projector are the seed's as in every other case.  The
# rows are those with the fewest near-tied picks in the free-running reference at a cap of 8 groups (33 images); another cap takes further rows in order, and
# tests/test_dec_seq_ref_cpu.py checks the conditions at 8 only.
BEAM_CAP_POOL = 256
BEAM_CAP_ROWS = [6, 13, 17, 20, 25, 35, 46, 73, 81, 95, 99, 100, 106, 109, 112, 119, 123, 125, 129, 132, 138, 145, 152, 156, 170, 183, 185, 195, 197, 203, 208, 218, 251]


def beam_cap_case(cap):
    """the smallest two-pass shape of the one-group-per-XCD cap at k = 8 (4 images per group): 4 cap + 1 images, L the smallest with L B >= 128 cap"""
    B = 4 * cap + 1
    return (B, 5, -(-128 * cap // B), 8, BEAM_CAP_SEED, "pool")


def beam_operands(B, T, seed, flags):
    """`operands` of a beam case; "pool": the images are rows of a larger batch of the same generator (BEAM_CAP_ROWS, then the pool's other rows in order)"""
    if "pool" not in flags:
        return operands(B, T, seed)
    rows = BEAM_CAP_ROWS + [r for r in range(BEAM_CAP_POOL) if r not in BEAM_CAP_ROWS]
    return take_rows(operands(max(BEAM_CAP_POOL, B), T, seed), (rows + list(range(BEAM_CAP_POOL, B)))[:B])


def beam_projector(seed, flags):
    wo, bo = projector(seed)
    if "eos" in flags:
        bo[EOS - 1] += EOS_BOOST
    return wo, bo


BEAM_WORDS = 6000


def beam_words(seed, L, alphabet):
    """the word list of a "dict-<alphabet>" case: words(seed) over `alphabet`, 1 .. L + 2 characters, each behind one of the two planted twin classes as a
    character ("6" = 10, "g" = 20).  The start node so has TWO children, fewer than any beam used with it: an exact tie, then the repeat-the-best fallback.  The
    alphabet is small and the list long so that the tree stays dense down to depth ~L: where a node has one child, PAD (always admissible) enters the beam and no
    image is left without a finished hypothesis."""
    return ["6g"[i % 2] + w for i, w in enumerate(words(seed, n=BEAM_WORDS, alphabet=alphabet, lo=1, hi=L + 2))]


def beam_trie(seed, flags, L):
    """the flat trie (mask, base, child) of the case's word list (dict_oracle.load_dictionary, tail_ref.flat_trie), or None"""
    if "dict" not in flags:
        return None
    import dict_oracle as DO
    import tail_ref as TR
    return TR.flat_trie(DO.load_dictionary(beam_words(seed, L, flags.split("dict-")[1])))[:3]


def take_rows(o, rows):
    """the operands of `operands` with the per-image ones (context, ctx W_a, initial state) replaced by those of the images `rows` (repeats allowed)"""
    rows = torch.as_tensor(rows).long()
    return {**o, "ctx": o["ctx"][rows].contiguous(), "ctxa": o["ctxa"][rows].contiguous(), "c0": o["c0"][:, rows].contiguous(),
            "h0": o["h0"][:, rows].contiguous(), "feed0": o["feed0"][rows].contiguous()}


def beam(w, table, wo, bo, c0, h0, feed0, L, k, trie=None, round=True):
    """free-running beam search from GO: greedy's step arithmetic on the rows image * kin + hypothesis (kin = 1 at step 0; the context is not replicated),
    tail_ref.beam_step's selection, tail_ref.gather_rows' state gather by parent.  -> dict(hist_tok, hist_par [L][B][k] int64, scores [L][B][k] running,
    totals: per step [B][kin V] (the candidates the selection saw, -inf = inadmissible), free: the same without the dictionary, out: per step
    [B kin][H] and a: per step [B kin][T] of the rows that ENTERED the step, tol_mag: per step [B kin] = max_v |out| . |W_o|)"""
    import tail_ref as TR
    r = rne if round else (lambda x: x)
    B = c0.shape[1]
    cs, hs, out = [c0[0].to(F64), c0[1].to(F64)], [h0[0].to(F64), h0[1].to(F64)], feed0.to(F64)
    tok, scores, loc = torch.full((B,), GO, dtype=torch.int64), None, None
    res = dict(hist_tok=[], hist_par=[], scores=[], totals=[], free=[], out=[], a=[], tol_mag=[])
    for t in range(L):
        kin = 1 if t == 0 else k
        img = torch.arange(B).repeat_interleave(kin)
        z1 = table.to(F64)[tok - 1] + r(out) @ w.W1i.t() + r(hs[0]) @ w.W1h.t()
        cs[0], hs[0], _ = cell(z1, cs[0])
        z2 = w.b2 + r(hs[0]) @ w.W2i.t() + r(hs[1]) @ w.W2h.t()
        cs[1], hs[1], _ = cell(z2, cs[1])
        h2b = r(hs[1])
        a, c, _ = attention(h2b, w.ctx[img], w.ctxa[img])
        out = torch.tanh(torch.cat([r(c), h2b], 1) @ w.Wc.t())
        lp, mag = logprobs(out.float() if round else out, wo, bo)      # (the projector reads the fp32 out)
        prev = None if t == 0 else tok
        res["free"].append(TR.beam_totals(lp, prev, scores, B, kin, lp.shape[1]))
        res["totals"].append(TR.beam_totals(lp, prev, scores, B, kin, lp.shape[1], trie, loc) if trie is not None else res["free"][-1])
        toks, pars, vals, locs = TR.beam_step(lp, prev, scores, B, kin, k, lp.shape[1], trie, loc, check_gap=False)
        res["hist_tok"].append(toks); res["hist_par"].append(pars); res["scores"].append(vals)
        res["out"].append(out); res["a"].append(a); res["tol_mag"].append(mag.amax(dim=1))
        cs = [TR.gather_rows(x, pars, B, kin, k) for x in cs]
        hs = [TR.gather_rows(x, pars, B, kin, k) for x in hs]
        out = TR.gather_rows(out, pars, B, kin, k)
        tok, scores, loc = toks.reshape(-1), vals, (locs.reshape(-1) if trie is not None else None)
    for n in ("hist_tok", "hist_par", "scores"):
        res[n] = torch.stack(res[n])
    return res


def pick_classes(tot, tol, k):
    """One selection against its reference candidates.  tot: [n] float64 reference totals, tol: [n] the tolerance of every candidate (its parent row's).
    Reference order = tail_ref.select_topk (descending, ties -> lowest index, the best repeated when fewer than k are admissible).  Rank i is UNDECIDED
    when the next distinct candidate value BELOW the reference's rank-i value lies within 2 tol of it (exact ties, the planted twins', are not distinct
    values), and LOOSE when it is undecided or the next distinct value ABOVE it lies within 2 tol (the device may have swapped it with the undecided pick
    above).  -> dict(ref: the reference indices, kth: the reference's k-th best value, undecided, loose: [k] bool, fallback: the ranks that repeat the best,
    ties: the ranks whose successor has exactly the same value)"""
    import tail_ref as TR
    vals = [float(v) for v in tot]
    ref, rv = TR.select_topk(vals, k)
    nfin = sum(1 for v in vals if v > -float("inf"))
    fin = tot[torch.isfinite(tot)]
    und, loose, ties = [], [], []
    for i in range(k):
        if i >= nfin:
            und.append(False); loose.append(False)
            continue
        lo, hi = fin[fin < rv[i]], fin[fin > rv[i]]
        t2 = 2 * float(tol[ref[i]])
        und.append(bool(len(lo)) and rv[i] - lo.max().item() <= t2)
        loose.append(und[-1] or (bool(len(hi)) and hi.min().item() - rv[i] <= t2))
        if i + 1 < min(k, nfin) and rv[i + 1] == rv[i]:
            ties.append(i)
    return dict(ref=ref, kth=rv[min(k, nfin) - 1] if nfin else -float("inf"), undecided=und, loose=loose,
                fallback=list(range(max(nfin, 1), k)) if nfin < k else [], ties=ties)


def beam_conditions(hist_tok, hist_par, totals, free, k, dictionary):
    """the conditions on a beam case (of the free-running reference, or of the device's own history with the reference totals of stage 2) -> (ok, text, counts)"""
    L, B = hist_tok.shape[0], hist_tok.shape[1]
    fin = (hist_tok == PAD) | (hist_tok == EOS)                         # [L][B][k]: the hypothesis is finished after the step
    n = dict(eos=int((hist_tok[:L - 1] == EOS).sum()), mixed=int((fin.any(2) & ~fin.all(2)).any(0).sum()), never=int((~fin.any(2).any(0)).sum()),
             moved=0, twice=0, ties=0, few=0, masked=0)
    own = torch.arange(k).view(1, 1, k)
    n["moved"] = int((hist_par[1:] != own).sum())
    n["twice"] = sum(int(len(set(hist_par[t, b].tolist())) < k) for t in range(1, L) for b in range(B))
    for t in range(L):
        V = totals[t].shape[1] // (1 if t == 0 else k)
        for b in range(B):
            tk, pr = hist_tok[t, b].tolist(), hist_par[t, b].tolist()
            row = totals[t][b]
            for i in range(k - 1):
                if (tk[i], tk[i + 1]) == TIE and pr[i] == pr[i + 1] and row[pr[i] * V + tk[i] - 1] == row[pr[i + 1] * V + tk[i + 1] - 1]:
                    n["ties"] += 1
            if dictionary:
                n["few"] += int(int(torch.isfinite(row).sum()) < k)
                top = torch.sort(free[t][b], descending=True, stable=True).indices[:k]
                n["masked"] += int(bool((row[top] == -float("inf")).any()))
    ok = n["eos"] >= 3 and n["mixed"] >= 1 and n["never"] >= 1 and n["moved"] >= 1 and n["twice"] >= 1 and n["ties"] >= 1
    if dictionary:
        ok = ok and n["few"] >= 1 and n["masked"] >= 1
    return ok, ", ".join(f"{a} {v}" for a, v in n.items()), n


def beam_undecided_share(ref, k, tol_of, factor):
    """share of the ranks of every selection of a free-running reference that are undecided at `factor` / 2 times the 2 tol of pick_classes"""
    und = total = 0
    for t, tot in enumerate(ref["totals"]):
        kin = 1 if t == 0 else k
        tol = tol_of(ref["tol_mag"][t]).view(-1, kin, 1).expand(-1, kin, tot.shape[1] // kin).reshape(tot.shape) * (factor / 2.0)
        for b in range(tot.shape[0]):
            c = pick_classes(tot[b], tol[b], k)
            und += sum(c["undecided"]); total += k
    return und / total
