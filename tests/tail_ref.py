"""Plain float64 / integer restatements of the operations behind the loss, token-sum, optimizer, weight-shadow, beam-search and small
elementwise kernels (csrc/ops_misc.hip, project_loss_kernel of csrc/ops_gemm.hip), written from the Lua lines the kernels cite.  No GPU:
tests/test_tail_ref_cpu.py checks them against oracle_torch / dict_oracle / torch autograd, tests/test_tail_kernels_gpu.py checks the
kernels against them.  Ids are 1-based as in the reference (PAD = 1, GO = 2, EOS = 3)."""
import math

import numpy as np
import torch

PAD, GO, EOS = 1, 2, 3
EXACT = float(2 ** 24)          # integers below this are exact in fp32, so a sum that stays below it is exact in any order
GAP = 1e-3                      # two candidates of a selection row are exactly equal or at least this far apart (asserted)


# ---- LogSoftMax + weighted ClassNLL (output_projector.lua:6, criterion.lua:3-8, model.lua:644-648)
def targets_at(tgt, st, sb, L, Bt):
    """the 1-based target of row r = t * Bt + b: tgt.flat[t * st + b * sb]"""
    flat = torch.as_tensor(tgt).reshape(-1).long()
    t, b = torch.arange(L).unsqueeze(1), torch.arange(Bt).unsqueeze(0)
    return flat[(t * st + b * sb).reshape(-1)]


def lsm_nll(x, y, scale):
    """x [rows][V] float64 logits, y [rows] 1-based targets -> (logp, nll [rows], d logits); PAD rows carry weight 0 (criterion.lua:5)."""
    x = x.double()
    lp = x - torch.logsumexp(x, 1, keepdim=True)
    w = (y != PAD).double()
    rows = torch.arange(x.shape[0])
    nll = -w * lp[rows, y - 1]
    onehot = torch.zeros_like(x)
    onehot[rows, y - 1] = 1.0
    return lp, nll, scale * w.unsqueeze(1) * (lp.exp() - onehot)


# ---- sums of d z by token and the three products hanging off them (LSTM.lua:55-56 nn.LookupTable accGradParameters; model.lua:643-661)
def token_sums(dz, tok, V):
    """S [V][ncols] = rows of dz summed by their (1-based) token.  Asserts that every partial sum is exact in fp32."""
    dz, idx = dz.double(), torch.as_tensor(tok).long() - 1
    assert int(idx.min()) >= 0 and int(idx.max()) < V
    S = torch.zeros(V, dz.shape[1], dtype=torch.float64).index_add_(0, idx, dz)
    mag = torch.zeros(V, dz.shape[1], dtype=torch.float64).index_add_(0, idx, dz.abs())
    assert float(mag.max()) < EXACT and float(mag.sum(0).max()) < EXACT, "token sums leave the exact range of fp32"
    assert torch.equal(dz, dz.round()), "exact operands are integers"
    return S


def token_sum_products(S, W, lookup, E):
    """(d b = column totals, d lookup [V][E] = S W[:, :E], d W[:, :E] = S^T lookup); W [ncols][>= E].  Exactness asserted."""
    S, W, lookup = S.double(), W.double()[:, :E], lookup.double()
    assert float((S.abs() @ W.abs()).max()) < EXACT and float((S.abs().t() @ lookup.abs()).max()) < EXACT
    return S.sum(0), S @ W, S.t() @ lookup


def embedding_scatter(demb, tok, V):
    """d table [V][E] = rows of demb summed by token (exactness asserted)"""
    return token_sums(demb, tok, V)


# ---- optim.sgd_list (optim_sgd.lua:38-95): per group, clip the gradient's L2 norm, then w -= lr * g
def sgd_groups(p, g, off, lr, clip):
    """p, g flat float64; off: group offsets (len = groups + 1).  Returns (new p, [(param norm, grad norm)] per group); elements
    outside [off[0], off[-1]) are returned unchanged."""
    p, g = p.double().clone(), g.double()
    norms = []
    for a, b in zip(off[:-1], off[1:]):
        gn = math.sqrt(float((g[a:b] ** 2).sum()))
        pn = math.sqrt(float((p[a:b] ** 2).sum()))
        sc = clip / gn if gn > clip else 1.0                        # optim_sgd.lua:50-52
        p[a:b] = p[a:b] - lr * (g[a:b] * sc)                        # :90
        norms.append((pn, gn))
    return p, norms


# ---- the time-out word (include/aocr.h: aocr_cluster_status): word 0 = code of the step in flight, latch = what this optimizer
# call acts on, sticky = the last code the host has not read
def skip_rule(err0, sticky):
    """an optimizer call: -> (err0, latch, sticky, skip).  skip: no update, BatchNorm state <- snapshot."""
    return (0, err0, err0, True) if err0 != 0 else (0, 0, sticky, False)


def snapshot_rule(err0, sticky):
    """the start of a step: a code no optimizer call consumed moves to the sticky word -> (err0, sticky)"""
    return (0, err0) if err0 != 0 else (0, sticky)


# ---- bf16 weight shadows
def rne(t):
    """round-to-nearest-even bf16 image, as float32"""
    return t.float().to(torch.bfloat16).float()


def shadow(w):
    """(bf16(w), bf16(w)^T) as float32"""
    r = rne(w)
    return r, r.t().contiguous()


# ---- flat dictionary trie (utils.lua:177-218 -> include/aocr.h): node n has a child for id v iff bit v - 1 of mask[n]; its children
# are child[base[n] ..] in ascending v; node 0 is the start node
def flat_trie(root):
    """nested dicts {id: node} (dict_oracle.load_dictionary's shape; shared / cyclic nodes allowed) -> (mask uint64, base, child int32, node index by id())"""
    index, order, todo = {id(root): 0}, [root], [root]
    while todo:
        node = todo.pop(0)
        for v in sorted(node):
            ch = node[v]
            if id(ch) not in index:
                index[id(ch)] = len(order); order.append(ch); todo.append(ch)
    mask, base, child = np.zeros(len(order), dtype=np.uint64), np.zeros(len(order), dtype=np.int32), []
    for n, node in enumerate(order):
        base[n] = len(child)
        for v in sorted(node):
            assert 1 <= v <= 64
            mask[n] |= np.uint64(1) << np.uint64(v - 1)
            child.append(index[id(node[v])])
    return mask, base, np.array(child if child else [0], dtype=np.int32), index


def trie_admits(mask, node, v, first):
    """candidate id v (1-based) at a node: a child, or -- after the first step -- PAD (model.lua:413,469)"""
    return (not first and v == PAD) or bool((int(mask[node]) >> (v - 1)) & 1)


def trie_next(mask, base, child, node, v, first):
    """PAD keeps the node, any other token moves to the child (model.lua:499-507)"""
    if not first and v == PAD:
        return node
    m = int(mask[node])
    if not (m >> (v - 1)) & 1:
        return node
    return int(child[int(base[node]) + bin(m & ((1 << (v - 1)) - 1)).count("1")])


# ---- one beam-search step (model.lua:399-404, 446-458, 516): top-k over the kin * V candidates of every image
def select_topk(row, k):
    """row: float64 scores (-inf = inadmissible).  Descending score, ties to the lowest index; fewer admissible than k: the best one is
    repeated (model.lua:419-433); none: index 0.  -> (indices, scores)"""
    row = [float(v) for v in row]
    order = sorted((i for i in range(len(row)) if row[i] > -math.inf), key=lambda i: (-row[i], i))[:k]
    if not order:
        return [0] * k, [-math.inf] * k
    order = order + [order[0]] * (k - len(order))
    return order, [row[i] for i in order]


def min_gap(row):
    """the smallest distance between two different finite scores of a row (inf: all equal)"""
    v = np.unique(np.asarray([x for x in row if x > -math.inf], dtype=np.float64))
    return float(np.diff(v).min()) if len(v) > 1 else math.inf


def beam_totals(logp, prev_tok, beam_scores, B, kin, V, trie=None, loc_in=None):
    """[B][kin * V] float64 candidate scores: finished beams (previous token PAD / EOS) continue with PAD at zero cost (model.lua:448-449),
    the running score is added (:450), what the dictionary does not admit is -inf.  prev_tok None: the first step."""
    first = prev_tok is None
    tot = logp.double().reshape(B, kin, V).clone()
    if not first:
        fin = ((torch.as_tensor(prev_tok) == PAD) | (torch.as_tensor(prev_tok) == EOS)).reshape(B, kin)
        tot[:, :, 0] = torch.where(fin, torch.zeros((), dtype=torch.float64), tot[:, :, 0])
        tot = tot + beam_scores.double().reshape(B, kin, 1)
    if trie is not None:
        for b in range(B):
            for j in range(kin):
                node = 0 if first else int(loc_in[b * kin + j])
                for v in range(1, V + 1):
                    if not trie_admits(trie[0], node, v, first):
                        tot[b, j, v - 1] = -math.inf
    return tot.reshape(B, kin * V)


def beam_step(logp, prev_tok, beam_scores, B, kin, kout, V, trie=None, loc_in=None, check_gap=True):
    """-> (tokens [B][kout] 1-based, parents [B][kout], scores [B][kout] float64, next nodes [B][kout] or None)"""
    first = prev_tok is None
    tot = beam_totals(logp, prev_tok, beam_scores, B, kin, V, trie, loc_in)
    toks, pars, vals, locs = [], [], [], []
    for b in range(B):
        if check_gap:
            assert min_gap(tot[b].tolist()) >= GAP, f"row {b}: two candidates closer than {GAP} but not equal"
        idx, sc = select_topk(tot[b].tolist(), kout)
        toks.append([i % V + 1 for i in idx]); pars.append([i // V for i in idx]); vals.append(sc)
        if trie is not None:
            locs.append([trie_next(trie[0], trie[1], trie[2], 0 if first else int(loc_in[b * kin + i // V]), i % V + 1, first) for i in idx])
    return (torch.tensor(toks), torch.tensor(pars), torch.tensor(vals, dtype=torch.float64), torch.tensor(locs) if trie is not None else None)


# ---- beam bookkeeping (model.lua:521-535, 573-585)
def gather_rows(src, parents, B, kin, kout):
    """dst[b * kout + i] = src[kin == 1 ? b : b * kin + parents[b][i]]"""
    par = torch.as_tensor(parents).long().reshape(B, kout)
    rows = torch.arange(B).unsqueeze(1).expand(B, kout) if kin == 1 else torch.arange(B).unsqueeze(1) * kin + par
    return src[rows.reshape(-1)]


def token_rows(table, tok):
    return table[torch.as_tensor(tok).long() - 1]


def winner(beam_scores):
    """torch.max over the final scores of an image: the FIRST maximum"""
    best, bi = float(beam_scores[0]), 0
    for i in range(1, len(beam_scores)):
        if float(beam_scores[i]) > best:
            best, bi = float(beam_scores[i]), i
    return bi, best


def backtrace(hist_tok, hist_par, beam_scores):
    """hist_tok / hist_par [Lt][B][k], beam_scores [B][k] -> (labels [B][Lt], scores [B]): the winner walked back through its parents"""
    Lt, B, k = hist_tok.shape
    labels, scores = torch.zeros(B, Lt, dtype=torch.int64), torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        idx, scores[b] = winner(beam_scores[b])
        for t in range(Lt - 1, -1, -1):
            labels[b, t] = int(hist_tok[t, b, idx])
            idx = int(hist_par[t, b, idx])
    return labels, scores


def recognize_gather(labels, hist_par, beam_scores, sc_hist, attn_hist):
    """labels [B][Lt]; hist_par [Lt][B][k] or None (greedy); sc_hist [Lt][B][k]; attn_hist [Lt][B k][T] with row b * kin + hypothesis
    (kin = 1 at step 0).  -> (char_logp [B][Lt] = the winner's score differences, attn [B][Lt][T] = its attention rows); steps after the
    first EOS / PAD of labels are 0."""
    Lt, B, k = sc_hist.shape
    T = attn_hist.shape[-1]
    cl, at = torch.zeros(B, Lt, dtype=torch.float64), torch.zeros(B, Lt, T, dtype=torch.float64)
    for b in range(B):
        tend = next((t for t in range(Lt) if int(labels[b, t]) in (PAD, EOS)), Lt - 1)
        idx = winner(beam_scores[b])[0] if k > 1 else 0
        for t in range(Lt - 1, -1, -1):
            kin = 1 if t == 0 else k
            par = int(hist_par[t, b, idx]) if (k > 1 and hist_par is not None) else 0
            if t <= tend:
                cl[b, t] = float(sc_hist[t, b, idx]) - (float(sc_hist[t - 1, b, par]) if t > 0 else 0.0)
                at[b, t] = attn_hist[t].reshape(-1, T)[b * kin + par].double()
            idx = par
    return cl, at


# ---- decoder initial state (model.lua:541-552)
def dec_init(cfw, cbw, hfw, hbw, Hd, Ld, copy_h):
    """-> (c0 [Ld][B][Hd], h0 [Ld][B][Hd]): layer 0 = [fw ; bw] in the first 2 He columns (h only when copy_h), everything else 0"""
    B, He = cfw.shape
    c0, h0 = torch.zeros(Ld, B, Hd, dtype=torch.float64), torch.zeros(Ld, B, Hd, dtype=torch.float64)
    c0[0, :, :He], c0[0, :, He:2 * He] = cfw.double(), cbw.double()
    if copy_h:
        h0[0, :, :He], h0[0, :, He:2 * He] = hfw.double(), hbw.double()
    return c0, h0


# ---- nn.Dropout masks (LSTM.lua:68-69,116-118) and the tanh backward that divides them out again
def drop_mask(p, seed, step, site, off, n):
    import oracle_torch as O
    return torch.from_numpy(O.dropout_mask(p, seed, step, site, off, n))


def drop_base_thr(p, seed, step, site):
    """(base, thr) of the device's DropSpec for the same stream"""
    import oracle_torch as O
    with np.errstate(over="ignore"):
        stream = np.uint64(step) * np.uint64(64) + np.uint64(site)
        base = O._splitmix64(np.array([np.uint64(seed) ^ (stream * np.uint64(0xD1342543DE82EF95))], dtype=np.uint64))[0]
    return int(base), int(math.ceil(p * 9007199254740992.0))


def dpre(g1, g2, out, mask=None):
    """d pre-activation of out = tanh(pre) (model.lua:649,654-657): (g1 + g2) (1 - out^2); with a dropout mask `out` holds the MASKED value"""
    g = g1.double() + (g2.double() if g2 is not None else 0.0)
    o = out.double()
    if mask is not None:
        o = torch.where(mask != 0, o / torch.where(mask != 0, mask, torch.ones_like(mask)), torch.zeros_like(o))
        g = g * mask
    return g * (1.0 - o * o)
