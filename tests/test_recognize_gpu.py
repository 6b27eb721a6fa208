"""Label-free recognition (include/aocr.h aocr_recognize) on every path decode_beam takes: the bf16 decoder chain kernel (greedy and beam 5),
the greedy decoder cluster kernel (AOCR_NO_DEC_CHAINS=1) and the per-step launch chain (fp32: greedy and beam 5).

1. labels / scores are bit-equal to aocr_decode / aocr_decode_dict on the same images, with and without a dictionary, and asking for the
   optional outputs does not change them;
2. the attention rows are the fp64 oracle's, teacher-forced with [GO, labels[:, :-1]] (a hypothesis' state depends on its tokens only, so
   this replays the winning beam too); rows sum to 1 up to the first EOS and are 0 after it;
3. char_logp is the oracle's log-probability of each emitted token (0 on the PAD-at-no-cost steps) and sums to the score;
4. Model.recognize reads a list of uint8 images without labels and returns what step(forward_only=True) reads;
5. Model.recognize_page with every optional stage on at once, as one column and with layout=True, reads what the public stage functions
   called one after the other read, publishes the corner fields of tests/backmap_ref.py and makes no read of its own per stage.
Weights are sharpened (oracle_torch.sharpen_params) and the BatchNorm statistics calibrated, so that the attention is peaked and a mis-indexed
row shows."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from model_harness import make

pytestmark = pytest.mark.gpu

C2 = dict(enc_hidden=256, enc_layers=1, dec_layers=2, input_feed=True)       # Hd = 512, two layers, input feed: the whole-sequence kernels
SMALL = dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True)
# Stated bounds (next to tol.py's).  Attention weights are probabilities.  fp32: 1e-4 max-abs against the fp64 oracle.  bf16: against the
# oracle with bf16-rounded operands (oracle_torch.operand_rounding, the arithmetic the kernels implement); the scores are 512-term products and
# softmax turns a score error d into a factor e^d, so the bound is a few percent of a peak (test_sharp_gpu.py: the bf16 logits hold 5 %).
F32_ATTN_TOL, BF16_ATTN_TOL = 1e-4, 6e-2          # measured: fp32 1.4e-6, bf16 3.2e-2 (B = 32, W = 100, 12 steps)
F32_LOGP_TOL, BF16_LOGP_TOL = 1e-3, 3e-2          # measured: fp32 2.5e-6, bf16 1.1e-2

# path -> (config, compute, beam, environment)
PATHS = {
    "chain_greedy_bf16": (C2, "bf16", 1, {}),
    "chain_beam5_bf16": (C2, "bf16", 5, {}),
    "cluster_greedy_bf16": (C2, "bf16", 1, {"AOCR_NO_DEC_CHAINS": "1"}),
    "launch_greedy_f32": (SMALL, "f32", 1, {}),
    "launch_beam5_f32": (SMALL, "f32", 5, {}),
}
B, W, LT = 32, 100, 12
_CACHE, _BN = {}, {}


def _words():
    rng = random.Random(5)
    return ["".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(rng.randint(2, 8))) for _ in range(3000)]


def _first_end(row):
    for t, v in enumerate(row):
        if v in (1, 3):
            return t
    return len(row) - 1


def _bn_state(O, P, batch):
    """Evaluation-mode BatchNorm statistics that normalise this batch (oracle_torch.calibrated_bn_state): with the initial 0 / 1 the CNN is not
    normalised, the LSTMs saturate and the attention is uniform.  The CNN's seeded weights do not depend on the configuration and are untouched
    by the sharpening, and every model here sees the same images: one calibration serves all (20 iterations leave 0.9^20 = 12 % of the initial
    statistics -- normalised enough for a peaked attention)."""
    key = float(P["cnn.conv1.w"].sum()), float(P["cnn.conv7.w"].sum())
    if key not in _BN:
        _BN[key] = O.calibrated_bn_state(P, torch.from_numpy(np.asarray(batch[0])).double(), iters=20)
    return {k: v.clone() for k, v in _BN[key].items()}


def _run(path, cuda, monkeypatch):
    """One model per path: decode, recognize (with and without the optional outputs, with and without a trie), the oracle replay."""
    if path in _CACHE:
        return _CACHE[path]
    import aocr
    cfgkw, compute, beam, env = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, O, ocfg, P0, _, batch = make(cfgkw, B=B, W=W, maxlen=8, compute=compute, max_decoder_l=LT, max_beam=max(beam, 1))
    P = O.sharpen_params(P0)
    st = _bn_state(O, P0, batch)
    m.set_parameters(P, st)
    images, targets, targets_eval = m._upload(batch)
    trie = aocr.build_trie(_words()).to(cuda)
    out = {}
    for tname, tr in (("none", None), ("trie", trie)):
        lab_d, sc_d, _, _ = m.decode_device(images, targets, targets_eval, beam, tr)
        lab_d, sc_d = lab_d.clone(), sc_d.clone()
        lab_0, sc_0, _, _ = m.recognize_device(images, beam, tr)
        lab_0, sc_0 = lab_0.clone(), sc_0.clone()
        lab, sc, clp, att = m.recognize_device(images, beam, tr, attention=True, char_scores=True)
        torch.cuda.synchronize()
        m.check_health()
        out[tname] = dict(dec=(lab_d.cpu(), sc_d.cpu()), plain=(lab_0.cpu(), sc_0.cpu()), full=(lab.cpu(), sc.cpu(), clp.cpu(), att.cpu()))
    # the oracle, teacher-forced with the recognised tokens (no dictionary run: the labels of the plain search)
    lab = out["none"]["full"][0]
    img = torch.from_numpy(np.asarray(batch[0]))
    go = torch.full((B, 1), 2, dtype=torch.int32)
    tin = torch.cat([go, lab[:, :-1]], 1)
    with torch.no_grad(), O.operand_rounding("bf16" if compute == "bf16" else "none"):
        r = O.forward_train(P, {k: v.clone() for k, v in st.items()}, ocfg, img, tin, lab, training=False, update_running=False)
    a_ref = torch.stack([tr[3][1][1] for tr in r["dec_tr"]], 1)             # (B, Lt, T): acache = (q, a, c, cat)
    logp = r["logp"]                                                         # (Lt, B, V)
    m.shutdown()
    for k in env:
        monkeypatch.delenv(k, raising=False)
    _CACHE[path] = (out, a_ref, logp, compute, beam)
    return _CACHE[path]


@pytest.mark.parametrize("path", list(PATHS))
def test_recognize_equals_decode(cuda, monkeypatch, path):
    out = _run(path, cuda, monkeypatch)[0]
    for tname in ("none", "trie"):
        (ld, sd), (l0, s0), (l1, s1, _, _) = out[tname]["dec"], out[tname]["plain"], out[tname]["full"]
        assert torch.equal(ld, l0) and torch.equal(ld, l1), (path, tname, "labels")
        assert torch.equal(sd.view(torch.int32), s0.view(torch.int32)) and torch.equal(sd.view(torch.int32), s1.view(torch.int32)), (path, tname, "scores")
        print(f"[recognize] {path} trie={tname}: labels and scores bit-equal to decode; rows ending in EOS {(ld == 3).any(1).float().mean():.2f}")


@pytest.mark.parametrize("path", list(PATHS))
def test_recognize_attention_against_oracle(cuda, monkeypatch, path):
    out, a_ref, _, compute, _ = _run(path, cuda, monkeypatch)
    lab, _, _, att = out["none"]["full"]
    T = W // 4 - 1
    assert att.shape == (B, LT, T)
    err, n_on = 0.0, 0
    for b in range(B):
        e = _first_end(lab[b].tolist())
        on = att[b, :e + 1].double()
        assert (on.sum(1) - 1.0).abs().max().item() < 1e-5, (path, b)
        assert (att[b, e + 1:] == 0).all(), (path, b, "after the first EOS")
        err = max(err, (on - a_ref[b, :e + 1]).abs().max().item()); n_on += e + 1
    ent = -(a_ref.clamp_min(1e-30) * a_ref.clamp_min(1e-30).log()).sum(-1).mean().item()
    tol = F32_ATTN_TOL if compute == "f32" else BF16_ATTN_TOL
    print(f"[recognize] {path}: attention max-abs vs the oracle {err:.3e} over {n_on} steps (bound {tol:g}); oracle entropy {ent:.3f} nat (ln T = {np.log(T):.3f})")
    assert ent < 0.9 * np.log(T)                                               # peaked: a row of another step or image would not match
    assert err < tol, (path, err, tol)


@pytest.mark.parametrize("path", list(PATHS))
def test_recognize_char_scores_against_oracle(cuda, monkeypatch, path):
    out, _, logp, compute, _ = _run(path, cuda, monkeypatch)
    err = 0.0
    for tname in ("none", "trie"):
        lab, sc, clp, _ = out[tname]["full"]
        for b in range(B):
            e = _first_end(lab[b].tolist())
            assert (clp[b, e + 1:] == 0).all(), (path, tname, b)
            s = clp[b].double().sum().item()
            bound = LT * 2.0 ** -22 * (1.0 + np.abs(np.cumsum(clp[b].double().numpy())).max())
            assert abs(s - float(sc[b])) <= bound, (path, tname, b, s, float(sc[b]), bound)
            if tname == "none":                                              # the oracle replays the unconstrained search
                for t in range(e + 1):
                    prev = 2 if t == 0 else int(lab[b, t - 1])
                    ref = 0.0 if (t > 0 and prev in (1, 3)) else logp[t, b, int(lab[b, t]) - 1].item()
                    err = max(err, abs(float(clp[b, t]) - ref))
    tol = F32_LOGP_TOL if compute == "f32" else BF16_LOGP_TOL
    print(f"[recognize] {path}: char_logp max-abs vs the oracle {err:.3e} (bound {tol:g}); sums match the scores")
    assert err < tol, (path, err, tol)


def test_recognize_unlabeled_images(cuda):
    """Model.recognize on a list of uint8 images (what load_image returns) reads what step(forward_only=True) reads from the same batch."""
    import aocr
    from aocr.data import preprocess_batch
    m, O, ocfg, P0, _, batch = make(C2, B=B, W=W, maxlen=8, compute="bf16", max_decoder_l=LT, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), _bn_state(O, P0, batch))
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, size=(32, int(w)), dtype=np.uint8) for w in rng.integers(60, 160, size=B)]
    imgs[1] = np.stack([imgs[1]] * 3, -1)                                      # an RGB one
    for beam in (1, 5):
        res = m.recognize(imgs, beam_size=beam, attention=True, width=W)
        images = preprocess_batch(imgs, W, cuda)
        m.step([images, batch[1], batch[2], batch[3], batch[4]], True, beam)
        _, ref, _ = aocr.eval_word_err_rate(m._dec_out.labels, m._dec_out.labels, True)     # rows cut at the first EOS, as text is
        assert res.text == ref, beam
        assert np.array_equal(res.labels, m._dec_out.labels) and np.array_equal(res.scores, m._dec_out.scores)
        assert res.attention.shape == (B, LT, W // 4 - 1) and res.char_logp.shape == (B, LT)
        assert np.array_equal(res.columns, aocr.encoder_columns(W))
        print(f"[recognize] unlabeled uint8 batch, beam {beam}: e.g. {res.text[:3]}; {len(ref)} rows")
    m.shutdown()


def test_recognize_rejects_bad_arguments(cuda):
    import aocr
    m, O, ocfg, P0, st, batch = make(SMALL, B=4, W=36, maxlen=4, compute="f32", max_decoder_l=6, max_beam=2)
    images, _, _ = m._upload(batch)
    labels = torch.empty((8, 6), dtype=torch.int32, device=cuda)
    scores = torch.empty(8, dtype=torch.float32, device=cuda)
    for Bb, Ww, beam, what in ((0, 36, 1, "B="), (5, 36, 1, "B="), (4, 4, 1, "W="), (4, 200, 1, "W="), (4, 36, 0, "beam="), (4, 36, 3, "beam=")):
        rc = aocr.lib.aocr_recognize(m._h, aocr.ptr(images), Bb, Ww, beam, None, aocr.ptr(labels), aocr.ptr(scores), None, None)
        assert rc != 0 and what in aocr.last_error(), (Bb, Ww, beam, aocr.last_error())
    rc = aocr.lib.aocr_recognize(m._h, aocr.ptr(images), 4, 36, 1, None, None, aocr.ptr(scores), None, None)
    assert rc != 0 and "NULL" in aocr.last_error()
    m.shutdown()


# ---- Model.recognize_page with every stage at once -------------------------------------------------------------------------------------------
# The planted 600 x 800 page of curl_cases, curled (20 rows of sag) and then skewed (17 steps of 64 / 65536), doubled, turned upside down and
# photographed on a desk with rectify_cases.text_photo's keystone: rectify (four corners given), flatten, scale=0.5, clean, orient=2, deskew
# and dewarp each have something to do, and every estimate that would cost a sync is given by value.  What is expected is computed here from
# the public stage functions in the documented order, once for both tests; the corner fields by tests/backmap_ref.py.
PAGE_B = 32


@pytest.fixture(scope="module")
def staged(cuda):
    import math
    import aocr
    import rectify_ref as RR
    import skew_ref as SK
    from curl_cases import SEGMENT, curled_page
    m, O, ocfg, P0, st, _ = make(SMALL, B=PAGE_B, W=100, maxlen=8, compute="f32", max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    given = np.ascontiguousarray(np.kron(SK.deskew(curled_page(20), -17 * 64), np.ones((2, 2), np.uint8))[::-1, ::-1])
    Hp, Wp = given.shape
    H, W = Hp + 60, Wp + 80
    quad = [31, 22, W - 44, 14, W - 25, H - 16, 12, H - 25]
    photo = RR.make_photo(given, quad, H, W, 50)
    corners = [tuple(quad[2 * i:2 * i + 2]) for i in range(4)]
    params = aocr.SegmentParams(**SEGMENT)
    skew_p, group = aocr.SkewParams(threshold=128, n_steps=32), 4
    s = SimpleNamespace(m=m, photo=photo, params=params, group=group)
    s.options = dict(rectify=corners, flatten=True, scale=0.5, clean=True, orient=2, deskew=skew_p, dewarp=True)
    s.size, s.coef = aocr.rectify_plan(np.array(corners))
    page = aocr.warp_page_device(torch.from_numpy(photo).to(cuda), s.coef, s.size, 255)
    page = aocr.flatten_page_device(page, aocr.FlattenParams(light_text=0))
    H1, W1 = page.shape
    s.shape = (max(int(math.floor(W1 * 0.5 + 0.5)), 1), max(int(math.floor(H1 * 0.5 + 0.5)), 1))
    s.resize = (H1, W1, s.shape[1], s.shape[0])
    page = aocr.resize_page_device(page, s.shape)
    page, cleaned = aocr.clean_page_device(page, aocr.CleanParams(threshold=128, light_text=0))
    s.turn = (2, page.shape[0], page.shape[1])
    page = aocr.rotate_page_device(page, 2)
    skew = aocr.estimate_skew_device(page, skew_p)
    page = aocr.deskew_page_device(page, skew, 255)
    curl, shifts = aocr.estimate_curl_device(page, aocr.CurlParams(threshold=128, light_text=0))
    s.final = aocr.dewarp_page_device(page, shifts, group, 255)
    s.cleaned, s.skew, s.curl, s.shifts = cleaned.cpu().numpy(), skew.cpu().numpy(), curl.cpu().numpy(), shifts.cpu().numpy()
    print(f"[recognize_page every stage] photo {photo.shape} -> {s.size} -> {s.shape}; skew {s.skew.tolist()}, curl {s.curl.tolist()} {s.shifts.tolist()}, "
          f"cleaned {s.cleaned.tolist()}")
    assert s.skew[1] != 0 and s.curl[1] > 0                                    # the shear and the curl are there to be taken out
    yield s
    m.check_health()
    m.shutdown()


def _read_page(s, monkeypatch, **kw):
    """(the namespace, the elements of every Tensor.cpu() of the call before its first recognize_device, those after it)."""
    reads = []
    real_cpu, real_rec = torch.Tensor.cpu, s.m.recognize_device
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (reads.append(t.numel()), real_cpu(t, *a, **k))[1])
        mp.setattr(s.m, "recognize_device", lambda *a, **k: (reads.append("loop"), real_rec(*a, **k))[1])
        res = s.m.recognize_page(s.photo, s.params, width=100, **s.options, **kw)
    at = reads.index("loop")
    return res, reads[:at], [r for r in reads[at:] if r != "loop"]


def _check_staged(s, res, rows, cuda):
    """everything but the layout fields: `rows` (n, 6) are the boxes expected on s.final."""
    import math
    import aocr
    from backmap_ref import corner_fields
    n = len(rows)
    assert n > PAGE_B and res.n_found == n and not res.truncated and res.threshold == 128
    np.testing.assert_array_equal(res.boxes, rows[:, :4])
    np.testing.assert_array_equal(res.line, rows[:, 4])
    np.testing.assert_array_equal(res.ink, rows[:, 5])
    boxes_dev = torch.from_numpy(np.ascontiguousarray(rows)).to(cuda)
    for c0 in range(0, n, PAGE_B):
        ref = s.m.recognize(aocr.crop_lines_device(s.final, boxes_dev[c0:c0 + PAGE_B], None, 100))
        np.testing.assert_array_equal(res.labels[c0:c0 + PAGE_B], ref.labels)
        np.testing.assert_array_equal(res.scores[c0:c0 + PAGE_B], ref.scores)
        assert res.text[c0:c0 + PAGE_B] == ref.text
    assert (res.widths == 100).all() and res.flatten_radius == 16
    assert (res.clean_components, res.clean_specks, res.clean_rules, res.clean_ink_removed) == tuple(int(s.cleaned[i]) for i in (0, 1, 2, 5))
    assert (res.orientation, res.orient_runs, res.orient_scores) == (2, None, None)
    assert (res.skew_steps, res.skew_slope_q16) == (int(s.skew[0]), int(s.skew[1])) and res.skew_deg == math.degrees(math.atan(int(s.skew[1]) / 65536.0))
    np.testing.assert_array_equal(res.curl_shifts, s.shifts)
    assert res.curl_shifts.dtype == np.int32 and (res.curl_group, res.curl_max, res.curl_pairs) == (s.group, int(s.curl[1]), int(s.curl[3]))
    assert (res.scaled, res.scale_size, res.scale_quartiles, res.scale_glyphs, res.scale_shape) == (True, None, None, None, s.shape)
    assert (res.rectified, res.rectify_size, res.rectify_area) == (True, s.size, None)
    np.testing.assert_array_equal(res.rectify_quad, np.array(s.options["rectify"]))
    want = corner_fields(rows[:, :4], (s.shifts, s.group), (int(s.skew[1]), s.final.shape[0], s.final.shape[1]), s.turn, s.resize, s.coef)
    assert sorted(want) == ["photo_corners", "source_boxes", "source_corners", "uncurled_corners", "unscaled_corners"]
    for k, v in want.items():
        got = getattr(res, k)
        assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v), k
    layout = {"block", "blocks", "block_depth", "n_blocks", "layout_overflow"}
    assert set(vars(res)) - layout == {
        "boxes", "line", "ink", "text", "labels", "scores", "widths", "threshold", "n_found", "n_lines", "truncated", "flatten_radius",
        "clean_components", "clean_specks", "clean_rules", "clean_ink_removed", "curl_shifts", "curl_group", "curl_max", "curl_pairs",
        "skew_steps", "skew_slope_q16", "skew_deg", "orientation", "orient_runs", "orient_scores", "scaled", "scale_size", "scale_quartiles",
        "scale_glyphs", "scale_shape", "rectified", "rectify_quad", "rectify_size", "rectify_area"} | set(want)


def test_recognize_page_every_stage_single_column(cuda, staged, monkeypatch):
    import aocr
    s = staged
    res, before, after = _read_page(s, monkeypatch)
    boxes_dev, counts_dev = aocr.segment_page_device(s.final, s.params)
    counts = counts_dev.cpu().numpy()
    rows = boxes_dev[:int(counts[0])].cpu().numpy()
    assert (res.n_found, res.n_lines, res.threshold) == tuple(int(v) for v in counts[:3])
    _check_staged(s, res, rows, cuda)
    assert not hasattr(res, "blocks") and not hasattr(res, "block")
    # one read brings every word back -- counts 4, skew 4, clean 8, curl 4 + ng: no stage adds a sync of its own -- and the boxes follow it
    n = len(rows)
    assert before == [4 + 4 + 8 + 4 + len(s.shifts), 6 * n], before
    assert len(after) == 2 * -(-n // PAGE_B)                                 # labels and scores of every chunk
    print(f"[recognize_page every stage] {n} boxes in {res.n_lines} lines; reads {before} then {len(after)} in the loop")


def test_recognize_page_every_stage_layout(cuda, staged, monkeypatch):
    import layout_ref as L
    import segment_ref as R
    from curl_cases import SEGMENT
    s = staged
    res, before, after = _read_page(s, monkeypatch, layout=True)
    final = s.final.cpu().numpy()
    want_blocks, want_counts, info = L.layout_page(final, 128, 0)
    rows, ids, lines, found, truncated = L.segment_blocks(final, want_blocks, **dict(R.DEFAULTS, **SEGMENT))
    nb = len(want_blocks)
    assert nb >= 1 and res.n_blocks == nb == want_counts[0] and res.layout_overflow == bool(want_counts[3]) and info[0] == 128
    np.testing.assert_array_equal(res.blocks, want_blocks[:, :4])
    np.testing.assert_array_equal(res.block_depth, want_blocks[:, 4])
    np.testing.assert_array_equal(res.block, ids)
    assert res.block.dtype == np.int32 and (res.n_found, res.n_lines, res.truncated) == (found, lines, truncated)
    _check_staged(s, res, rows, cuda)
    # two reads: the layout's counts 4, info 4 and 256 blocks with skew 4, clean 8, curl 4 + ng; then every block's counts and boxes
    assert before == [4 + 4 + 4 + 8 + 4 + len(s.shifts) + 6 * 256, nb * (4 + 6 * 1024)], before
    assert len(after) == 2 * -(-len(rows) // PAGE_B)
    print(f"[recognize_page every stage, layout] {len(rows)} boxes in {lines} lines of {nb} blocks; reads {before}")
