"""CPU: the references of tests/tail_ref.py against independent statements of the same operations -- oracle_torch, dict_oracle, torch
autograd and hand-written examples -- so that tests/test_tail_kernels_gpu.py compares the kernels with something shown to be right."""
import math

import pytest
import torch
import torch.nn.functional as F

import dict_oracle as D
import oracle_torch as O
import tail_ref as R


def rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def ints(*shape, seed, lo=-4, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def test_lsm_nll_matches_autograd():
    rows, V = 23, 11
    x = (rnd(rows, V, seed=1) * 3).requires_grad_(True)
    y = torch.randint(1, V + 1, (rows,), generator=torch.Generator().manual_seed(2))
    y[::5] = R.PAD
    w = torch.ones(V, dtype=torch.float64); w[0] = 0
    loss = F.nll_loss(torch.log_softmax(x, 1), y - 1, weight=w, reduction="sum")
    loss.backward()
    lp, nll, dl = R.lsm_nll(x.detach(), y, 0.25)
    assert torch.allclose(lp, torch.log_softmax(x.detach(), 1), atol=1e-14)
    assert abs(float(nll.sum()) - loss.item()) < 1e-12
    assert torch.allclose(dl, 0.25 * x.grad, atol=1e-14)
    assert float(nll[::5].abs().max()) == 0.0 and float(dl[::5].abs().max()) == 0.0


def test_targets_at_both_layouts():
    L, B = 3, 4
    tb = torch.arange(1, L * B + 1).reshape(B, L)                  # stored [B][L]: strides (1, L), as the model passes them
    assert R.targets_at(tb, 1, L, L, B).tolist() == [int(tb[b, t]) for t in range(L) for b in range(B)]
    tl = tb.t().contiguous()                                       # stored [L][B]: strides (B, 1)
    assert R.targets_at(tl, B, 1, L, B).tolist() == R.targets_at(tb, 1, L, L, B).tolist()


def test_token_sums_match_autograd_through_embedding_and_linear():
    """z = embedding(tok) W[:, :E]^T + b: autograd's d lookup, d W and d b for an upstream gradient dz are the three products of the sums by token"""
    rows, V, E, ncols, ldw = 61, 7, 5, 12, 9
    tok = torch.randint(1, V + 1, (rows,), generator=torch.Generator().manual_seed(3))
    tok[tok == 4] = 5                                              # a token without rows
    lookup = ints(V, E, seed=4).requires_grad_(True)
    W = ints(ncols, ldw, seed=5).requires_grad_(True)
    b = torch.zeros(ncols, dtype=torch.float64, requires_grad=True)
    dz = ints(rows, ncols, seed=6)
    z = F.linear(F.embedding(tok - 1, lookup), W[:, :E], b)
    z.backward(dz)
    S = R.token_sums(dz, tok, V)
    assert float(S[3].abs().max()) == 0.0
    db, dlk, dW = R.token_sum_products(S, W.detach(), lookup.detach(), E)
    assert torch.equal(db, b.grad) and torch.equal(dlk, lookup.grad) and torch.equal(dW, W.grad[:, :E])
    assert float(W.grad[:, E:].abs().max()) == 0.0
    assert torch.equal(R.embedding_scatter(dz, tok, V), torch.zeros(V, ncols, dtype=torch.float64).index_add_(0, tok - 1, dz))
    with pytest.raises(AssertionError):
        R.token_sums(dz * 2.0 ** 22, tok, V)                      # the exactness guard fires


def test_sgd_groups_match_oracle_sgd_list():
    cfg = O.OcrConfig(enc_hidden=8, enc_layers=1, dec_layers=1, input_feed=True)
    P = O.init_params(cfg, 5)
    G = {k: rnd(*v.shape, seed=10 + i) * (3.0 if O.group_of(k) in (0, 3) else 0.01) for i, (k, v) in enumerate(P.items())}
    newP, norms = O.sgd_list(P, G, 0.1, 5.0)
    keys = sorted(P, key=O.group_of)                               # stable: the groups in order
    off = [0]
    for gi in range(len(O.GROUPS)):
        off.append(off[-1] + sum(P[k].numel() for k in keys if O.group_of(k) == gi))
    flat = lambda d: torch.cat([d[k].reshape(-1) for k in keys])
    got, gn = R.sgd_groups(flat(P), flat(G), off, 0.1, 5.0)
    assert torch.allclose(got, flat(newP), rtol=0, atol=1e-14)
    assert any(n[1] > 5.0 for n in norms) and any(n[1] < 5.0 for n in norms)          # both sides of the clip
    for a, b in zip(gn, norms):
        assert abs(a[0] - b[0]) < 1e-9 and abs(a[1] - b[1]) < 1e-9
    # offsets that do not start at 0 / end at n, an empty group
    p, g = rnd(40, seed=1), rnd(40, seed=2)
    q, nn = R.sgd_groups(p, g, [3, 3, 10, 37], 0.5, 1e9)
    assert torch.equal(q[:3], p[:3]) and torch.equal(q[37:], p[37:]) and torch.allclose(q[3:37], p[3:37] - 0.5 * g[3:37])
    assert nn[0] == (0.0, 0.0)


def test_skip_rule():
    assert R.skip_rule(7, 0) == (0, 7, 7, True)
    assert R.skip_rule(0, 7) == (0, 0, 7, False)                   # a following call updates and leaves the sticky word alone
    assert R.snapshot_rule(5, 0) == (0, 5) and R.snapshot_rule(0, 9) == (0, 9)


def test_shadow_is_rne():
    w = torch.tensor([[1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], [-(1.0 + 2.0 ** -8), 3.0, 1.0 + 2.0 ** -9]])
    wb, wtb = R.shadow(w)
    # ties go to the even mantissa: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6; below half an ulp -> down
    assert wb.tolist() == [[1.0, 1.0, 1.0 + 2.0 ** -6], [-1.0, 3.0, 1.0]]
    assert torch.equal(wtb, wb.t())


def test_select_topk_matches_topk_sorted():
    tot = ints(6, 40, seed=7, lo=-3, hi=3)                        # many exact ties
    for k in (1, 5, 8):
        vals, idx = O._topk_sorted(tot, k)
        for b in range(6):
            gi, gv = R.select_topk(tot[b].tolist(), k)
            assert gi == idx[b].tolist() and gv == vals[b].tolist()
    assert R.select_topk([-math.inf, 2.0, -math.inf, 2.0, 1.0], 4) == ([1, 3, 4, 1], [2.0, 2.0, 1.0, 2.0])       # repeat the best
    assert R.select_topk([-math.inf] * 3, 2) == ([0, 0], [-math.inf, -math.inf])
    assert R.min_gap([1.0, 1.0, -math.inf, 1.5, 3.0]) == 0.5 and R.min_gap([2.0, 2.0]) == math.inf


def _trie():
    return D.load_dictionary(["ab", "abc", "b0", "c"])


def test_flat_trie_and_beam_step_match_dict_oracle():
    root = _trie()
    mask, base, child, index = R.flat_trie(root)
    assert index[id(root)] == 0
    a, b_, c = D.char_id(ord("a")), D.char_id(ord("b")), D.char_id(ord("c"))
    assert int(mask[0]) == (1 << (a - 1)) | (1 << (b_ - 1)) | (1 << (c - 1))
    assert R.trie_next(mask, base, child, 0, b_, True) == index[id(root[b_])]
    assert not R.trie_admits(mask, 0, R.PAD, True) and R.trie_admits(mask, 0, R.PAD, False)
    V, k = 39, 5
    # first step: 3 admissible tokens for 5 beams -> the best one is repeated
    lp = torch.log_softmax(rnd(2, V, seed=8) * 3, 1)
    toks, pars, vals, locs = R.beam_step(lp, None, None, 2, 1, k, V, (mask, base, child), None, check_gap=False)
    nodes_of = []
    for b in range(2):
        t, s, nodes = D.select_first(lp[b].tolist(), root, k)
        assert toks[b].tolist() == t and vals[b].tolist() == s and pars[b].tolist() == [0] * k
        assert locs[b].tolist() == [index[id(n)] for n in nodes]
        assert len(set(t)) == 3
        nodes_of.append(nodes)
    # next step from those nodes; beam 0 of image 1 finished with EOS
    lp2 = torch.log_softmax(rnd(2 * k, V, seed=9) * 3, 1)
    prev = toks.reshape(-1).clone()
    prev[k] = R.EOS
    loc_in = locs.reshape(-1)
    t2, p2, v2, l2 = R.beam_step(lp2, prev, vals, 2, k, k, V, (mask, base, child), loc_in, check_gap=False)
    for b in range(2):
        l = lp2[b * k:(b + 1) * k].clone()
        fin = (prev[b * k:(b + 1) * k] == R.PAD) | (prev[b * k:(b + 1) * k] == R.EOS)
        l[fin, 0] = 0.0
        tot = (l + vals[b].unsqueeze(1)).reshape(-1).tolist()
        t, raws, s, nodes = D.select_next(tot, nodes_of[b], k, V)
        assert t2[b].tolist() == t and p2[b].tolist() == [c_ // V for c_ in raws] and v2[b].tolist() == s
        assert l2[b].tolist() == [index[id(n)] for n in nodes]
    # without a dictionary: oracle_torch's sorted top-k of the same totals
    t3, p3, v3, _ = R.beam_step(lp2, prev, vals, 2, k, k, V, check_gap=False)
    tot = R.beam_totals(lp2, prev, vals, 2, k, V)
    ov, oi = O._topk_sorted(tot, k)
    assert torch.equal(t3, oi % V + 1) and torch.equal(p3, oi // V) and torch.equal(v3, ov)
    with pytest.raises(AssertionError):
        R.beam_step(torch.tensor([[0.0, -0.5, -0.5004]]), None, None, 1, 1, 1, 3)      # the gap guard fires


def test_trie_bit_63_and_shared_nodes():
    root = {64: {R.EOS: {}}, 5: {}}
    root[5][64] = root[64]                                         # a shared node
    mask, base, child, index = R.flat_trie(root)
    assert len(mask) == 4 and int(mask[0]) == (1 << 63) | (1 << 4)
    assert R.trie_next(mask, base, child, 0, 64, True) == index[id(root[64])] == R.trie_next(mask, base, child, index[id(root[5])], 64, False)
    assert int(mask[index[id(root[64][R.EOS])]]) == 0               # a node that admits nothing: only PAD continues it
    lp = torch.full((1, 64), -5.0, dtype=torch.float64)
    t, p, v, l = R.beam_step(lp, torch.tensor([9]), torch.zeros(1, 1), 1, 1, 3, 64, (mask, base, child), torch.tensor([index[id(root[64][R.EOS])]]),
                             check_gap=False)
    assert t.tolist() == [[1, 1, 1]] and l.tolist() == [[index[id(root[64][R.EOS])]] * 3]


def test_backtrace_then_recognize_gather_hand_example():
    """3 steps, 1 image, 2 beams.  Final scores (-1.0, -0.5): beam 1 wins.  Step 2: beam 1 = token 3 (EOS) from parent 0; step 1: beam 0 = token 7
    from parent 1; step 0: beam 1 = token 9.  Labels 9 7 3."""
    hist_tok = torch.tensor([[[8, 9]], [[7, 6]], [[5, 3]]])
    hist_par = torch.tensor([[[0, 0]], [[1, 0]], [[1, 0]]])
    sc_hist = torch.tensor([[[-0.1, -0.2]], [[-0.3, -0.6]], [[-1.0, -0.5]]], dtype=torch.float64)
    final = sc_hist[2]
    labels, scores = R.backtrace(hist_tok, hist_par, final)
    assert labels.tolist() == [[9, 7, 3]] and scores.tolist() == [-0.5]
    T = 2
    attn_hist = torch.zeros(3, 2, T, dtype=torch.float64)
    attn_hist[0, 0] = torch.tensor([1.0, 2.0])                     # step 0: one row per image (kin = 1)
    attn_hist[1] = torch.tensor([[3.0, 4.0], [5.0, 6.0]])          # step t > 0: row = the PARENT hypothesis the step ran on
    attn_hist[2] = torch.tensor([[7.0, 8.0], [9.0, 10.0]])
    cl, at = R.recognize_gather(labels, hist_par, final, sc_hist, attn_hist)
    assert torch.allclose(cl, torch.tensor([[-0.2, -0.3 + 0.2, -0.5 + 0.3]], dtype=torch.float64))
    assert at.tolist() == [[[1.0, 2.0], [5.0, 6.0], [7.0, 8.0]]]
    assert abs(float(cl.sum()) - float(scores[0])) < 1e-15         # the per-character scores add up to the winner's score
    # EOS at step 1: everything later is 0; tied final scores: the first maximum wins
    labels2, _ = R.backtrace(hist_tok, hist_par, torch.tensor([[-0.5, -0.5]]))
    assert labels2.tolist() == [[8, 6, 5]]                         # beam 0: token 5 from parent 1 = token 6 from parent 0 = token 8
    cl2, at2 = R.recognize_gather(torch.tensor([[9, 3, 5]]), hist_par, torch.tensor([[-0.5, -0.5]]), sc_hist, attn_hist)
    assert float(cl2[0, 2]) == 0.0 and float(at2[0, 2].abs().max()) == 0.0 and float(cl2[0, 1]) == -0.6 + 0.1
    # greedy: no parents
    cl3, at3 = R.recognize_gather(torch.tensor([[9, 7, 4]]), None, None, sc_hist[:, :, :1], attn_hist[:, :1])
    assert torch.allclose(cl3, torch.tensor([[-0.1, -0.2, -0.7]], dtype=torch.float64)) and at3[0, 2].tolist() == [7.0, 8.0]


def test_gather_and_dec_init_and_dpre():
    src = torch.arange(12.0).reshape(6, 2)
    assert R.gather_rows(src, torch.tensor([[2, 0, 2], [1, 1, 0]]), 2, 3, 3).tolist() == [[4, 5], [0, 1], [4, 5], [8, 9], [8, 9], [6, 7]]
    assert R.gather_rows(src[:2], torch.tensor([[5, 5], [5, 5]]), 2, 1, 2).tolist() == [[0, 1], [0, 1], [2, 3], [2, 3]]
    assert R.token_rows(src, torch.tensor([3, 1])).tolist() == [[4, 5], [0, 1]]
    cfw, cbw, hfw, hbw = (torch.full((2, 3), float(v)) for v in (1, 2, 3, 4))
    c0, h0 = R.dec_init(cfw, cbw, hfw, hbw, 8, 2, 1)
    assert c0[0, 0].tolist() == [1, 1, 1, 2, 2, 2, 0, 0] and h0[0, 1].tolist() == [3, 3, 3, 4, 4, 4, 0, 0]
    assert float(c0[1].abs().max()) == 0.0 and float(h0[1].abs().max()) == 0.0
    assert float(R.dec_init(cfw, cbw, hfw, hbw, 8, 2, 0)[1].abs().max()) == 0.0
    mk = R.drop_mask(0.5, 11, 3, 16, 40, 200)
    assert set(mk.tolist()) == {0.0, 2.0} and torch.equal(mk[10:], R.drop_mask(0.5, 11, 3, 16, 50, 190))
    pre = rnd(200, seed=3)
    g = rnd(200, seed=4)
    out = torch.tanh(pre)
    ref = g * mk * (1 - out * out)                                 # d/d pre of mask * tanh(pre), upstream g
    assert torch.allclose(R.dpre(g, None, out * mk, mk), ref, atol=1e-15)
    assert torch.allclose(R.dpre(g, g, out), 2 * g * (1 - out * out), atol=1e-15)
