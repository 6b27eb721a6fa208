"""CPU: tests/dec_seq_ref.py, the float64 restatement the decoder kernel tests compare with (tests/test_decoder_seq_kernels_gpu.py), against
oracle/oracle_torch.py's decoder and torch autograd in pure float64 (bf16 rounding off), its layout helpers, the fed mode against the free-running
one, and the conditions of its operand generators on every shape the GPU test uses."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import dec_seq_ref as R  # noqa: E402
import oracle_torch as O  # noqa: E402

F64, H = torch.float64, R.H


def _oracle_problem(B, T, L, seed=3):
    cfg = O.OcrConfig(enc_hidden=H // 2, enc_layers=1, dec_layers=2, input_feed=True)
    g = torch.Generator().manual_seed(seed)
    P = {k: v.clone() for k, v in O.init_params(cfg, 77).items() if k.startswith("dec.")}
    for k in P:                                                      # larger than the initialisation: every path carries gradient well above rounding
        if k.endswith(".w") or k.startswith("dec.attn"):
            P[k] = P[k] * 2.0
    ctx = torch.rand(B, T, H, generator=g, dtype=F64) - 0.5
    tok = torch.randint(1, cfg.vocab + 1, (L, B), generator=g)
    c0, h0 = torch.rand(2, B, H, generator=g, dtype=F64) - 0.5, torch.rand(2, B, H, generator=g, dtype=F64) - 0.5
    feed0, dout = torch.rand(B, H, generator=g, dtype=F64) - 0.5, torch.rand(L, B, H, generator=g, dtype=F64) - 0.5
    return cfg, P, ctx, tok, c0, h0, feed0, dout


def test_reference_matches_oracle_decoder_and_autograd():
    B, T, L = 3, 4, 3
    cfg, P, ctx, tok, c0, h0, feed0, dout = _oracle_problem(B, T, L)
    E = cfg.emb
    leaves = dict(c0=c0.clone().requires_grad_(), h0=h0.clone().requires_grad_(), feed0=feed0.clone().requires_grad_())
    Pg = {k: v.clone().requires_grad_() for k, v in P.items()}
    c, h, feed = [leaves["c0"][0], leaves["c0"][1]], [leaves["h0"][0], leaves["h0"][1]], leaves["feed0"]
    outs, hs, cs, aa = [], [], [], []
    for t in range(L):
        c, h, feed, (_, acache) = O.decoder_step_fwd(Pg, cfg, tok[t], ctx, feed, c, h, t)
        outs.append(feed); hs.append(torch.stack(h)); cs.append(torch.stack(c)); aa.append(acache[1])
    (torch.stack(outs) * dout).sum().backward()

    Wi1 = P["dec.l1.i2h.w"]
    zx1 = P["dec.lookup"][tok.long() - 1] @ Wi1[:, :E].t() + P["dec.l1.i2h.b"] + P["dec.l1.h2h.b"]
    w = R.Weights(Wi1[:, E:], P["dec.l1.h2h.w"], P["dec.l2.i2h.w"], P["dec.l2.h2h.w"], P["dec.l2.i2h.b"] + P["dec.l2.h2h.b"], P["dec.attn.wa"],
                  P["dec.attn.wc"], ctx)
    f = R.forward(w, zx1, c0, h0, feed0, L, round=False)
    close = lambda a, b, what: torch.testing.assert_close(a, b.detach(), rtol=1e-10, atol=1e-12, msg=lambda m: f"{what}: {m}")
    close(f["out"][1:], torch.stack(outs), "out")
    close(f["hs"][:, 1:], torch.stack(hs, 1), "h")
    close(f["cs"][:, 1:], torch.stack(cs, 1), "c")
    close(f["a"], torch.stack(aa), "a")
    # the same through the per-token table
    table = P["dec.lookup"] @ Wi1[:, :E].t() + P["dec.l1.i2h.b"] + P["dec.l1.h2h.b"]
    ft = R.forward(w, table, c0, h0, feed0, L, tok=tok.int(), round=False)
    close(ft["out"], f["out"], "out through the token table")

    b = R.backward(w, f, dout, round=False)
    close(b["dc_st"], leaves["c0"].grad, "d c of the initial state")
    close(b["dh_rec"], leaves["h0"].grad, "d h of the initial state")
    close(b["dfeed"], leaves["feed0"].grad, "d feed")
    close(b["dz"][0].sum((0, 1)), Pg["dec.l1.h2h.b"].grad, "sum of d z1")
    close(b["dz"][1].sum((0, 1)), Pg["dec.l2.i2h.b"].grad, "sum of d z2")
    cat = torch.cat([f["c"], f["hs"][1, 1:]], 2)
    close(torch.einsum("tbi,tbj->ij", b["dpre"], cat), Pg["dec.attn.wc"].grad, "d W_c (d pre)")
    close(torch.einsum("tbi,tbj->ij", b["dq"], f["hs"][1, 1:]), Pg["dec.attn.wa"].grad, "d W_a (d q)")
    close(torch.einsum("tbi,tbj->ij", b["dz"][0], f["out"][:-1]), Pg["dec.l1.i2h.w"].grad[:, E:], "d W1_i2h feed part (d z1)")
    close(torch.einsum("tbi,tbj->ij", b["dz"][1], f["hs"][0, 1:]), Pg["dec.l2.i2h.w"].grad, "d W2_i2h (d z2)")


def test_gate_layout_round_trips():
    g = torch.arange(2 * 3 * 4 * 8, dtype=F64).view(2, 3, 4, 8)
    flat = R.il(g)
    assert flat.shape == (2, 3, 32)
    assert flat[1, 2, 4 * 5 + 2] == g[1, 2, 2, 5]                      # [unit][gate]
    assert torch.equal(R.unil(flat, 8), g)
    assert torch.equal(R.il(R.unil(flat, 8)), flat)


def _problem(B, T, L, table, seed):
    o = R.operands(B, T, seed)
    zx1, tok = R.gate_inputs(L, B, seed, table)
    return o, R.weights_of(o), zx1, tok


def test_fed_steps_reproduce_the_free_running_reference():
    """fed with the free-running reference's own (rounded) state, every stage of step_fed / bwd_step_fed returns that reference exactly"""
    B, T, L = 5, 7, 3
    o, w, zx1, tok = _problem(B, T, L, True, 1)
    f = R.forward(w, zx1, o["c0"], o["h0"], o["feed0"], L, tok=tok)
    for t in range(L):
        h1b, h2b = R.rne(f["hs"][0, t + 1]), R.rne(f["hs"][1, t + 1])
        s = R.step_fed(w, R.zx_at(zx1, tok, t), R.rne(f["out"][t]), R.rne(f["hs"][0, t]), R.rne(f["hs"][1, t]), f["cs"][0, t], f["cs"][1, t], h1b, h2b,
                       torch.cat([R.rne(f["c"][t]), h2b], 1))
        for k, ref in (("c1", f["cs"][0, t + 1]), ("c2", f["cs"][1, t + 1]), ("h2", f["hs"][1, t + 1]), ("out", f["out"][t + 1]), ("a", f["a"][t]),
                       ("g1", f["gates"][0, t])):
            assert torch.equal(s[k], ref), (t, k)
    dout = R.uniform((L, B, H), 0.5, 9).double()
    b = R.backward(w, f, dout)
    t = 0
    fed = dict(dpre_b=R.rne(b["dpre"][t]), dcat_c=b["dcat_c"][t], dq_b=R.rne(b["dq"][t]), dzb2=R.rne(b["dz"][1, t]))
    # the d c entering step 0 is not an output of `backward`: redo the carry
    dc1 = dc2 = torch.zeros(B, H, dtype=F64)
    zero = torch.zeros(B, 4 * H, dtype=F64)
    for tt in range(L - 1, 0, -1):
        n1, n2 = (R.rne(b["dz"][0, tt + 1]), R.rne(b["dz"][1, tt + 1])) if tt < L - 1 else (zero, zero)
        st = R.bwd_step_fed(w, R.saved_step(f, tt), dout[tt], n1, n2, dc1, dc2)
        dc1, dc2 = st["dc1"], st["dc2"]
    st = R.bwd_step_fed(w, R.saved_step(f, 0), dout[0], R.rne(b["dz"][0, 1]), R.rne(b["dz"][1, 1]), dc1, dc2, fed=fed)
    assert torch.equal(st["dz1"], b["dz"][0, 0]) and torch.equal(st["dz2"], b["dz"][1, 0]) and torch.equal(st["dc1"], b["dc_st"][0])


SHAPES = R.TF_SHAPES + [(32 * 8 + 4, 3, 2), R.DROP_SHAPE]


@pytest.mark.parametrize("B,T,L", SHAPES)
def test_generators_keep_their_conditions(B, T, L):
    for table in (False, True):
        o, w, zx1, tok = _problem(B, T, L, table, seed=B + T + L)
        for k in ("W1i", "W1h", "W2i", "W2h", "Wa", "Wc", "ctx", "ctxa", "h0", "feed0"):
            assert torch.equal(R.rne(o[k]).float(), o[k]), f"{k} is not exact in bf16"
        f = R.forward(w, zx1, o["c0"], o["h0"], o["feed0"], L, tok=tok)
        share = R.z_share(torch.cat([f["z"].reshape(-1), f["pre"].reshape(-1)]))
        assert share >= 0.9, f"only {share:.3f} of the free-running pre-activations inside |z| <= 4"
        # rows and steps differ by far more than any tolerance (1e-2 is 500 TOL_CELL): a row or step mix-up cannot pass
        for name, x in (("h1", f["hs"][0, 1:]), ("h2", f["hs"][1, 1:]), ("out", f["out"][1:]), ("c1", f["cs"][0, 1:]), ("c2", f["cs"][1, 1:])):
            flat = x.reshape(L * B, H)
            if L * B > 1:
                d = torch.cdist(flat, flat, p=float("inf")) + torch.eye(L * B, dtype=F64)
                assert d.min().item() > 1e-2, f"{name}: two (step, row) states are closer than 1e-2"
        if T > 1:
            assert (f["a"].max(2).values < 1 - 1e-3).all(), "an attention row is one-hot: the context sum would not see a wrong row"


@pytest.mark.parametrize("B,T,L,seed", R.GREEDY_CASES)
def test_greedy_cases_keep_their_conditions(B, T, L, seed):
    """the free-running greedy reference on the GPU test's inputs: EOS rows, a row that never ends, the early group, planted ties that win, margins"""
    o, w, table, _ = _problem(B, T, L, True, seed)
    wo, bo = R.projector(seed)
    assert torch.equal(wo[R.TIE[0] - 1], wo[R.TIE[1] - 1]) and bo[R.TIE[0] - 1] == bo[R.TIE[1] - 1]
    g = R.greedy(w, table, wo, bo, o["c0"], o["h0"], o["feed0"], L)
    ok, txt = R.greedy_conditions(g["labels"], B)
    assert ok, txt
    lab = g["labels"]
    assert (lab == R.TIE[0]).any() and not (lab == R.TIE[1]).any(), "the planted tie never wins, or the higher id won it"
    e = R.eos_step(lab)
    for b in range(B):
        assert (lab[b, int(e[b]) + 1:] == R.PAD).all(), "a label after EOS is not PAD"
        if int(e[b]) < L:
            assert torch.equal(g["scores"][int(e[b]):, b], g["scores"][int(e[b]), b].expand(L - int(e[b]))), "the score moves after EOS"
    top = g["logp"].topk(3, dim=2).values
    live = torch.stack([torch.arange(L) <= e[b] for b in range(B)], 1)                    # [L][B]
    gap = torch.where(lab.t() == R.TIE[0], top[:, :, 0] - top[:, :, 2], top[:, :, 0] - top[:, :, 1])
    from kernel_harness import TOL_CELL, bound
    tol = TOL_CELL + bound(R.logprobs(g["out"][1:].reshape(L * B, R.H).float(), wo, bo)[1].amax(1).view(L, B), 512)
    assert (gap > 2 * tol)[live].all(), f"best-to-second margin {gap[live].min().item():.2e} against 2 tol = {2 * tol.max().item():.2e}"
    # with the dictionary: some step's unconstrained arg-max is forbidden
    import dict_oracle as DO
    import tail_ref as TR
    trie = TR.flat_trie(DO.load_dictionary(R.words(seed)))[:3]
    gt = R.greedy(w, table, wo, bo, o["c0"], o["h0"], o["feed0"], L, trie=trie)
    free = R.logprobs(gt["out"][1:].reshape(L * B, R.H).float(), wo, bo)[0].argmax(1).view(L, B) + 1
    assert ((free != gt["labels"].t()) & (gt["labels"].t() != R.PAD)).any(), "the dictionary never masks the unconstrained arg-max"


# ------------------------------------------------------------------------------------------------------------------------------
# beam search
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,with_trie", [(3, False), (4, True)])
def test_beam_reference_matches_oracle_decode_beam(k, with_trie, monkeypatch):
    """R.beam (rounding off) against oracle_torch.decode_beam on the same decoder: the CNN, the encoder and the initial state of the oracle are replaced by
    the problem's context and state, so both run the same free-running search; history, labels and scores after the back-trace must agree"""
    import dict_oracle as DO
    import tail_ref as TR
    B, T, L = 4, 5, 7
    cfg, P, ctx, _, c0, h0, _, _ = _oracle_problem(B, T, L, seed=5)
    g = torch.Generator().manual_seed(11)
    P["proj.w"] = (torch.rand(cfg.vocab, H, generator=g, dtype=F64) * 2 - 1) * 1.5
    P["proj.b"] = torch.rand(cfg.vocab, generator=g, dtype=F64) - 0.5
    P["proj.b"][R.EOS - 1] += 2.0                                     # some hypotheses finish inside L steps
    monkeypatch.setattr(O, "cnn_forward", lambda P_, st, images, training, **kw: images)
    monkeypatch.setattr(O, "encoder_forward", lambda P_, cfg_, feats: (ctx, None))
    monkeypatch.setattr(O, "decoder_init_state", lambda cfg_, traces, B_, like: ([c0[0], c0[1]], [h0[0], h0[1]]))
    root = DO.load_dictionary(R.words(3)) if with_trie else None
    tgt = torch.full((B, L), R.PAD, dtype=torch.int64); tgt[:, 0] = R.GO
    ref = O.decode_beam(P, None, cfg, torch.zeros(B, 1, dtype=F64), tgt, tgt, beam=k, max_decoder_l=L, trie=root)
    E, Wi1 = cfg.emb, P["dec.l1.i2h.w"]
    table = P["dec.lookup"] @ Wi1[:, :E].t() + P["dec.l1.i2h.b"] + P["dec.l1.h2h.b"]
    w = R.Weights(Wi1[:, E:], P["dec.l1.h2h.w"], P["dec.l2.i2h.w"], P["dec.l2.h2h.w"], P["dec.l2.i2h.b"] + P["dec.l2.h2h.b"], P["dec.attn.wa"],
                  P["dec.attn.wc"], ctx)
    trie = TR.flat_trie(root)[:3] if with_trie else None
    r = R.beam(w, table, P["proj.w"], P["proj.b"], c0, h0, torch.zeros(B, H, dtype=F64), L, k, trie=trie, round=False)
    assert torch.equal(r["hist_tok"], ref["hist_tok"]) and torch.equal(r["hist_par"], ref["hist_par"])
    labels, scores = TR.backtrace(r["hist_tok"], r["hist_par"], r["scores"][L - 1])
    assert torch.equal(labels, ref["labels"])
    torch.testing.assert_close(scores, ref["scores"], rtol=1e-10, atol=1e-12)
    assert ((r["hist_tok"] == R.EOS).any() and (r["hist_par"][1:] != torch.arange(k)).any()), "the anchor problem is trivial: no EOS, or no hypothesis changes its slot"


def test_pick_classes_hand_cases():
    inf = float("inf")
    tol = torch.full((6,), 0.01, dtype=F64)
    c = R.pick_classes(torch.tensor([1.0, 5.0, 5.0, 3.0, 2.985, -inf], dtype=F64), tol, 3)
    assert c["ref"] == [1, 2, 3] and c["ties"] == [0] and c["undecided"] == [False, False, True] and c["fallback"] == [] and c["kth"] == 3.0
    c = R.pick_classes(torch.tensor([-inf, 4.0, -inf, 1.0, -inf, -inf], dtype=F64), tol, 3)
    assert c["ref"] == [1, 3, 1] and c["fallback"] == [2] and c["undecided"] == [False, False, False] and c["kth"] == 1.0


def _beam_cases():
    return R.BEAM_CASES + [R.beam_cap_case(8)]


@pytest.mark.parametrize("B,T,L,k,seed,flags", _beam_cases(), ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}{'-' + c[5] if c[5] else ''}" for c in _beam_cases()])
def test_beam_cases_keep_their_conditions(B, T, L, k, seed, flags):
    """the free-running beam reference on the GPU test's inputs: hypotheses that end, finished beside live ones, an image that never ends, picks that change
    slot, parents chosen twice, planted ties inside a selection; with a dictionary the repeat-the-best fallback and masked free picks; near-ties within 1 %.
    The XCD-cap shape draws its images from a pool: R.BEAM_CAP_ROWS."""
    from kernel_harness import TOL_CELL, bound
    assert L * B >= 128 and 2 <= k <= 8
    o = R.beam_operands(B, T, seed, flags)
    w, (table, _) = R.weights_of(o), R.gate_inputs(L, B, seed, True)
    wo, bo = R.beam_projector(seed, flags)
    trie = R.beam_trie(seed, flags, L)
    r = R.beam(w, table, wo, bo, o["c0"], o["h0"], o["feed0"], L, k, trie=trie)
    ok, txt, _ = R.beam_conditions(r["hist_tok"], r["hist_par"], r["totals"], r["free"], k, trie is not None)
    assert ok, txt
    share = R.beam_undecided_share(r, k, lambda mag: TOL_CELL + bound(mag, 512), 4.0)
    assert share <= 0.01, f"{share:.4f} of the picks have another candidate value within 4 tol"
