"""GPU: aocr_remove_rules against the restatement (tests/rules_ref.py) and against hand answers, and Model.recognize_page(rules=...) against
the restatement's rule removal followed by its segmentation.  Raw ABI calls through page_harness; every comparison is exact equality of the
whole poisoned output buffer (the padding between W and out_pitch and the tail included), of the counts over sentinels, over garbage-filled
scratch, at odd pitches and unaligned bases.  The shapes are built from the RULES_ constants of csrc/rules.hip, read from its source: they
are the smallest at which each seam of the kernels is crossed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import components_ref as CR
import rules_ref as RR
import segment_ref as R
from page_harness import csrc_constants, expect_placed, garbage_scratch, guarded_words, place, poisoned
from rules_cases import CASES, MOTIVE_RULES, MOTIVE_SEG, SEEDED, SEEDED_SHAPES, motive_page, ruled_page
from segment_cases import seeded_page

pytestmark = pytest.mark.gpu

SENTINEL = -7
OUT_FILL = 0x5A          # the poison of the output buffer
OUT_TAIL = 16            # bytes of that buffer behind the last row's pitch
SMALL = dict(threshold=128, light_text=0, axes=3, min_len=5, max_thick=2, edge=1)


def _consts():
    return csrc_constants("rules.hip", ("RULES_WORD", "RULES_CHUNK", "RULES_ROWS", "RULES_LANE_WORDS", "RULES_MAX_T"))


def _remove(cuda, page, params, pitch=None, offset=0, op=None, shape=None, out=True, counts=True, no_scratch=False, reserved=0, raw=None):
    """raw aocr_remove_rules: (the whole output buffer (H, op) plus OUT_TAIL bytes, counts, status)."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=255 if params.get("light_text") else 0)
    op = op or page.shape[1]
    o = poisoned(cuda, page.shape[0] * op + OUT_TAIL, OUT_FILL)
    cnt = guarded_words(cuda, 8, 0, SENTINEL, torch.int32)
    p = aocr.RuleParams()
    for k, v in dict(params, **(raw or {})).items():                            # field by field: the constructor turns bad values down
        setattr(p, k, v)
    p.reserved[0] = reserved
    sc = garbage_scratch(cuda, aocr.lib.aocr_rules_scratch_bytes(*page.shape), 1 << 12)
    st = aocr.lib.aocr_remove_rules(None, C.c_void_p(addr), pitch, H, W, C.byref(p), None if no_scratch else aocr.ptr(sc), aocr.ptr(o) if out else None,
                                    op, aocr.ptr(cnt) if counts else None)
    torch.cuda.synchronize()
    return o.cpu().numpy(), cnt.cpu().numpy(), st


def _check(cuda, page, params, what, pitch=None, offset=0, op=None, want=None):
    want_out, want_counts = want if want is not None else RR.remove_rules(page, **params)
    out, counts, st = _remove(cuda, page, params, pitch, offset, op)
    assert st == 0, what
    np.testing.assert_array_equal(counts, want_counts, err_msg=str(what))
    np.testing.assert_array_equal(out, expect_placed(want_out, op, 0, poison=OUT_FILL, tail=OUT_TAIL), err_msg=str(what))
    return want_counts


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_cases(cuda, case):
    H, W = case["page"].shape
    for pitch, offset, op in ((W, 0, W), (W + 7, 5, W + 3)):
        _check(cuda, case["page"], case["params"], case["name"], pitch, offset, op, want=(case["out"], case["counts"]))


@functools.lru_cache(maxsize=None)
def _seeded_ref(shape, thr, light, axes):
    H, W, _, _, seed = shape
    page = ruled_page(H, W, seed, bool(light))
    page.setflags(write=False)
    return page, RR.remove_rules(page, threshold=thr, light_text=light, axes=axes, **SEEDED)


@pytest.mark.parametrize("axes", [1, 2, 3])
@pytest.mark.parametrize("thr,light", [(128, 0), (-1, 0), (128, 1), (-1, 1)], ids=["fixed", "otsu", "fixed_light", "otsu_light"])
@pytest.mark.parametrize("shape", SEEDED_SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SEEDED_SHAPES])
def test_matches_restatement_on_seeded_pages(cuda, shape, thr, light, axes):
    H, W, pitch, offset, _ = shape
    k = _consts()
    if (H, W) == (300, 700):
        assert H > 4 * k["RULES_CHUNK"] and W > 10 * k["RULES_WORD"]
    page, want = _seeded_ref(shape, thr, light, axes)
    if axes == 3:
        assert min(want[1][3:7]) > 0                                             # every class and kept candidates (test_rules_cpu.py: the condition)
    params = dict(threshold=thr, light_text=light, axes=axes, **SEEDED)
    for op in (W, W + 3):
        _check(cuda, page, params, (shape, op), pitch, offset, op, want=want)


@pytest.mark.parametrize("T", range(1, 17))
def test_every_thickness(cuda, T):
    """one kernel instance per max_thick; e = 4 with T = 1 is the case of the edge reaching past the run"""
    assert _consts()["RULES_MAX_T"] == 16
    H, W, pitch, offset, seed = SEEDED_SHAPES[2]
    page = ruled_page(H, W, seed)
    big = np.kron(page[:40, :120], np.ones((2, 5), np.uint8))                    # thicker strokes for the larger T
    for pg, L, e in ((page, T + 1, 4), (big, 3 * T + 2, T % 5)):
        counts = _check(cuda, pg, dict(threshold=128, light_text=0, axes=3, min_len=L, max_thick=T, edge=e), (T, L, e), pg.shape[1] + 5, 3, pg.shape[1] + 1)
        assert counts[2] > 0 or pg is big                                         # the page's own rules are at most 2 thick and cross it


def test_smallest_pages(cuda):
    for page in (np.zeros((1, 1), np.uint8), np.full((1, 1), 255, np.uint8), np.zeros((1, 9), np.uint8), np.zeros((9, 1), np.uint8),
                 np.zeros((1, 3), np.uint8), np.zeros((2, 2), np.uint8)):
        for axes in (1, 2, 3):
            H, W = page.shape
            _check(cuda, page, dict(SMALL, axes=axes), (page.shape, axes), W + 2, 1, W + 1)
    _check(cuda, np.zeros((1, 1), np.uint8), dict(SMALL, threshold=-1), "1x1 otsu")


def _runs_page(H, W, row_runs=(), col_runs=()):
    """paper with horizontal runs (y, x0, x1) and vertical runs (x, y0, y1), half-open, one pixel thick"""
    page = np.full((H, W), 255, np.uint8)
    for y, x0, x1 in row_runs:
        page[y, x0:x1] = 0
    for x, y0, y1 in col_runs:
        page[y0:y1, x] = 0
    return page


@pytest.mark.parametrize("L", [5, 64, 70, 130, 200])
def test_runs_at_word_and_chunk_seams(cuda, L):
    k = _consts()
    S, CH = k["RULES_WORD"], k["RULES_CHUNK"]
    assert S == 64 and CH == 64
    W = H = 5 * S + 7
    # exactly L: starting one pixel before a seam, ending on a seam, starting on a seam; L - 1 next to each: they stay
    starts = (S - 1, 2 * S - L if L <= 2 * S else 0, S)
    rows = [(2 + 4 * i, x0, x0 + L) for i, x0 in enumerate(starts)] + [(4 + 4 * i, x0, x0 + L - 1) for i, x0 in enumerate(starts)]
    cols = [(2 + 4 * i, y0, y0 + L) for i, y0 in enumerate(starts)] + [(4 + 4 * i, y0, y0 + L - 1) for i, y0 in enumerate(starts)]
    if L == 70:
        assert starts[0] < S and 2 * S < starts[0] + L < 3 * S                    # three words / chunks, the middle one full
    for name, page in (("rows", _runs_page(40, W, row_runs=rows)), ("cols", _runs_page(H, 40, col_runs=cols))):
        params = dict(threshold=128, light_text=0, axes=3, min_len=L, max_thick=1, edge=0)
        want = RR.remove_rules(page, **params)
        assert want[1][2] == 3 * L and want[1][1] == 3 * L + 3 * (L - 1), name      # the three runs of L go, the three of L - 1 stay
        _check(cuda, page, params, (name, L), page.shape[1] + 3, 1, page.shape[1] + 2, want=want)


def test_runs_through_the_whole_page(cuda):
    k = _consts()
    CH, S = k["RULES_CHUNK"], k["RULES_WORD"]
    H, W = 3 * CH + 5, S + 6
    page = _runs_page(H, W, col_runs=[(0, 0, H), (S - 1, 0, H), (S, 0, H), (W - 1, 0, H), (7, 0, H - 1), (9, 1, H)])
    page[2 * CH, 9] = 255                                                         # column 9: cut at a chunk seam
    want = RR.remove_rules(page, threshold=128, axes=3, min_len=H, max_thick=2, edge=0)     # columns S - 1 and S: a rule 2 thick over a seam
    assert want[1][2] == 4 * H
    _check(cuda, page, dict(threshold=128, light_text=0, axes=3, min_len=H, max_thick=2, edge=0), "columns", want=want)
    wide = _runs_page(3, S * 64 * 2 + 70, row_runs=[(0, 0, S * 64 * 2 + 70), (2, 0, S * 64 * 2 + 69)])      # a lane owns 3 words of the row
    Lw = wide.shape[1]
    want = RR.remove_rules(wide, threshold=128, axes=3, min_len=Lw, max_thick=1, edge=0)
    assert want[1][2] == Lw and (want[0][2, :-1] == 0).all()
    _check(cuda, wide, dict(threshold=128, light_text=0, axes=3, min_len=Lw, max_thick=1, edge=0), "row", want=want)


def test_widest_and_highest_pages(cuda):
    k = _consts()
    assert k["RULES_WORD"] * k["RULES_LANE_WORDS"] * 64 == 16384
    rng = np.random.default_rng(16384)
    for shape in ((2, 16384), (16384, 2)):
        page = np.where(rng.random(shape) < 0.02, 255, 0).astype(np.uint8)        # runs of about 50 between single paper pixels
        page[0, :] = 0                                                            # and one run through the whole page
        page[:, 0] = 0
        params = dict(threshold=128, light_text=0, axes=3, min_len=100, max_thick=2, edge=1)
        want = RR.remove_rules(page, **params)
        assert want[1][2] > 16384
        _check(cuda, page, params, shape, want=want)


def test_halo_reads_at_the_page_edges(cuda):
    """T + e rows and columns around every pixel are looked at: on pages smaller than that, and with rules lying in the edge rows and columns"""
    for H, W in ((3, 40), (40, 3), (5, 5), (18, 70)):
        page = seeded_page(H, W, 7 * H + W)
        page[0, :] = 0
        page[-1, :] = 0
        page[:, 0] = 0
        page[:, -1] = 0
        for T, e in ((16, 4), (1, 4), (2, 0)):
            L = max(T + 1, min(H, W))
            _check(cuda, page, dict(threshold=128, light_text=0, axes=3, min_len=L, max_thick=T, edge=e), (H, W, T, e), W + 1, 1, W + 1)


def test_null_counts_reused_scratch_and_a_second_call(cuda):
    import aocr
    H, W, pitch, offset, seed = SEEDED_SHAPES[2]
    page = ruled_page(H, W, seed)
    params = dict(threshold=-1, light_text=0, axes=3, **SEEDED)
    want_out, want_counts = RR.remove_rules(page, **params)
    out, counts, st = _remove(cuda, page, params, counts=False)
    assert st == 0 and (counts == SENTINEL).all()
    np.testing.assert_array_equal(out, expect_placed(want_out, None, 0, poison=OUT_FILL, tail=OUT_TAIL))
    dev = torch.from_numpy(page).to(cuda)
    a, ca = aocr.remove_rules_device(dev, aocr.RuleParams(**params))
    b, cb = aocr.remove_rules_device(dev[:, 3:200], aocr.RuleParams(**params))   # a view: pitch 257, an odd base
    np.testing.assert_array_equal(a.cpu().numpy(), want_out)
    np.testing.assert_array_equal(ca.cpu().numpy(), want_counts)
    wb = RR.remove_rules(page[:, 3:200], **params)
    np.testing.assert_array_equal(b.cpu().numpy(), wb[0])
    np.testing.assert_array_equal(cb.cpu().numpy(), wb[1])
    clean = motive_page(False)                                                    # nothing to erase: bit for bit
    same, cs = aocr.remove_rules_device(torch.from_numpy(clean).to(cuda), aocr.RuleParams(**MOTIVE_RULES))
    np.testing.assert_array_equal(same.cpu().numpy(), clean)
    assert cs.cpu().tolist()[2:] == [0, 0, 0, 0, 0, 0]


def test_invalid_arguments_leave_the_outputs_untouched(cuda):
    import aocr
    page = seeded_page(40, 100, 3)
    for kw, word in ((dict(raw=dict(axes=0)), "axes"), (dict(raw=dict(axes=4)), "axes"), (dict(raw=dict(max_thick=0)), "max_thick"),
                     (dict(raw=dict(max_thick=17, min_len=40)), "max_thick"), (dict(raw=dict(min_len=2)), "min_len"),
                     (dict(raw=dict(min_len=16385)), "min_len"), (dict(raw=dict(edge=5)), "edge"), (dict(raw=dict(edge=-1)), "edge"),
                     (dict(raw=dict(threshold=255)), "threshold"), (dict(raw=dict(threshold=-2)), "threshold"), (dict(reserved=1), "reserved"),
                     (dict(out=False), "NULL"), (dict(no_scratch=True), "NULL"), (dict(op=99), "out_pitch"), (dict(shape=(40, 101)), "pitch"),
                     (dict(shape=(0, 100)), "page size"), (dict(shape=(16384, 4097), pitch=100), "page size")):
        a = dict(op=100)
        a.update(kw)
        out, counts, st = _remove(cuda, page, dict(SMALL), **a)
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (out == OUT_FILL).all() and (counts == SENTINEL).all(), kw
    assert aocr.lib.aocr_rules_scratch_bytes(0, 10) == 0 and aocr.lib.aocr_rules_scratch_bytes(16384, 4097) == 0
    need = aocr.lib.aocr_rules_scratch_bytes(40, 100)
    assert 0 < need and need + (1 << 15) <= 1 << 17
    arena = torch.full(((1 << 17) // 8,), -1, dtype=torch.int64, device=cuda)          # every address below lies inside it
    base = arena.data_ptr()
    arena.view(torch.uint8)[:4000] = torch.from_numpy(page.reshape(-1)).to(cuda)
    cnt = torch.full((8,), SENTINEL, dtype=torch.int32, device=cuda)
    before = arena.clone()
    p = aocr.RuleParams(**SMALL)
    for out_at, sc_at, cnt_at in ((2000, 1 << 15, None), ((1 << 15) + 64, 1 << 15, None), (1 << 14, 2048, None), (1 << 14, 1 << 15, 100),
                                  (1 << 14, 1 << 15, (1 << 14) + 8), (1 << 14, 1 << 15, (1 << 15) + 8)):
        st = aocr.lib.aocr_remove_rules(None, C.c_void_p(base), 100, 40, 100, C.byref(p), C.c_void_p(base + sc_at), C.c_void_p(base + out_at), 100,
                                        aocr.ptr(cnt) if cnt_at is None else C.c_void_p(base + cnt_at))
        assert st != 0 and "overlap" in aocr.last_error(), (out_at, sc_at, cnt_at)
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and (cnt.cpu().numpy() == SENTINEL).all()
    with pytest.raises(aocr.AocrError):
        aocr.remove_rules_device(torch.from_numpy(page).to(cuda), _bad_params(aocr))


def _bad_params(aocr):
    p = aocr.RuleParams()
    p.min_len = 3
    return p


def test_recognize_page_rules(cuda, monkeypatch):
    import aocr
    from model_harness import make
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=32, W=100, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    plain, form = motive_page(False), motive_page(True)
    params = aocr.SegmentParams(**MOTIVE_SEG)
    rp = aocr.RuleParams(**MOTIVE_RULES)
    want_out, want_counts = RR.remove_rules(form, **MOTIVE_RULES)
    want_boxes, want_seg = R.segment_page(want_out, **MOTIVE_SEG)
    before = m.recognize_page(form, params)                                       # today's path, before any rules call
    assert (before.n_found, before.n_lines) != (8, 4)

    res = m.recognize_page(form, params, rules=rp)
    assert (res.n_found, res.n_lines, res.threshold, res.truncated) == (8, 4, 128, False)
    np.testing.assert_array_equal(res.boxes, want_boxes[:, :4])
    np.testing.assert_array_equal(res.line, want_boxes[:, 4])
    np.testing.assert_array_equal(res.ink, want_boxes[:, 5])
    np.testing.assert_array_equal(res.rules_counts, want_counts)
    assert res.rules_counts.dtype == np.int64 and (res.rules_erased, res.rules_kept) == (int(want_counts[2]), int(want_counts[6]))
    assert np.array_equal(want_out <= 128, plain <= 128)                          # the ink of the page drawn without rules
    ref = m.recognize_page(want_out, params)                                      # the crops are cut from the page without its rules
    np.testing.assert_array_equal(res.boxes, ref.boxes)
    np.testing.assert_array_equal(res.labels, ref.labels)
    assert res.text == ref.text

    # clean=True alone loses what touches a rule, or keeps the rules: neither reads the underlined word or the word on the grid
    cleaned = m.recognize_page(form, params, clean=aocr.CleanParams(threshold=128, max_w=150))
    assert cleaned.clean_rules == 3 and cleaned.n_found == 6 and cleaned.n_lines == 3
    assert not any((cleaned.boxes == b).all(axis=1).any() for b in ref.boxes[[0, 2, 3, 5]])
    dflt = m.recognize_page(form, params, clean=True)
    assert dflt.clean_rules == 0 and dflt.n_found < 8 and dflt.n_lines < 4
    both = m.recognize_page(form, params, clean=aocr.CleanParams(threshold=128, max_h=0), rules=rp)       # the pairing for forms
    np.testing.assert_array_equal(both.boxes, ref.boxes)
    np.testing.assert_array_equal(both.labels, ref.labels)
    assert both.clean_rules == 0 and both.rules_erased == res.rules_erased

    true_res = m.recognize_page(form, params, rules=True)                         # the defaults with the threshold and light_text of params
    d_out, d_counts = RR.remove_rules(form, **dict(RR.DEFAULTS, threshold=128))
    d_boxes, d_seg = R.segment_page(d_out, **MOTIVE_SEG)
    np.testing.assert_array_equal(true_res.rules_counts, d_counts)
    np.testing.assert_array_equal(true_res.boxes, d_boxes[:, :4])
    lay = m.recognize_page(form, params, rules=rp, deskew=aocr.SkewParams(threshold=128, n_steps=4), layout=aocr.LayoutParams(gap_x=400, gap_y=400))
    assert lay.skew_steps == 0 and lay.n_found == 8                               # the counts ride with the skew and the layout readback
    np.testing.assert_array_equal(lay.rules_counts, want_counts)
    with pytest.raises(ValueError, match="RuleParams"):
        m.recognize_page(form, params, rules=3)

    for off in (None, False):                                                     # rules=None is the call as it was
        b = m.recognize_page(form, params, rules=off)
        assert sorted(vars(before)) == sorted(vars(b)) and not hasattr(b, "rules_counts")
        for k, v in vars(before).items():
            assert np.array_equal(v, getattr(b, k)) if isinstance(v, np.ndarray) else v == getattr(b, k), k

    reads = []
    real_cpu = torch.Tensor.cpu
    real_boxes = m._page_boxes

    def counted(*a, **k):
        monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *aa, **kk: (reads.append(t.numel()), real_cpu(t, *aa, **kk))[1])
        try:
            return real_boxes(*a, **k)
        finally:
            monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)

    monkeypatch.setattr(m, "_page_boxes", counted)
    for layout in (None, aocr.LayoutParams(gap_x=400, gap_y=400)):
        reads[:] = []
        m.recognize_page(form, params, layout=layout)
        without, reads[:] = list(reads), []
        m.recognize_page(form, params, layout=layout, rules=rp)
        assert len(reads) == len(without) == 2 and reads[0] == without[0] + 8, (layout, without, reads)
    m.check_health()
    m.shutdown()
