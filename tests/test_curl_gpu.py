"""GPU: aocr_estimate_curl and aocr_dewarp_page against the numpy restatement (tests/curl_ref.py), and Model.recognize_page(dewarp=...)
against the pieces it is made of.  Everything is exact equality: the header, every shift and every one of the (ng-1)(2D+1) scores of the
estimate, every byte of the dewarped page and of the buffer around it.  tests/test_curl_cpu.py shows on the restatement alone that the
planted pages used here are found and removed."""
import ctypes as C

import numpy as np
import pytest
import torch

import curl_ref as K
import segment_ref as R
from curl_cases import GATED, PLANTED, SEGMENT, TIE, curled_page, gated_page, noise_page, planted_page, text_page, tie_page
from page_harness import expect_placed, garbage_scratch, guarded_words, place, poisoned

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD = 4                # entries beyond shifts_dev's ng and scores_dev's (ng-1)(2D+1) that every raw call gets: they must keep their sentinel
POISON = 0xAB
TAIL = 32                # bytes of the dewarped page's buffer behind the last row's pitch


def _estimate(cuda, page, params, pitch=None, offset=0, scores=True, shape=None):
    """raw aocr_estimate_curl: (curl (4), shifts (ng) then GUARD sentinels, scores then GUARD sentinels, status); the scratch holds garbage."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset)
    p = aocr.CurlParams(**{k: v for k, v in params.items() if k != "reserved"})
    if "reserved" in params:
        p.reserved[1] = params["reserved"]
    g, D = min(max(p.group, 1), 16), min(max(p.max_shift, 0), 64)
    ng = K.n_groups(max(W, 1), g)
    need = aocr.lib.aocr_curl_scratch_bytes(H, W, p.group, p.max_shift)
    scratch = garbage_scratch(cuda, need, 1 << 16)
    curl = guarded_words(cuda, 4, 0, SENTINEL, torch.int32)
    sh = guarded_words(cuda, ng, GUARD, SENTINEL, torch.int32)
    sc = guarded_words(cuda, (ng - 1) * (2 * D + 1), GUARD, SENTINEL, torch.int64)
    st = aocr.lib.aocr_estimate_curl(None, C.c_void_p(addr), pitch, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(curl), aocr.ptr(sh),
                                     aocr.ptr(sc) if scores else None)
    torch.cuda.synchronize()
    return curl.cpu().numpy(), sh.cpu().numpy(), sc.cpu().numpy(), st


def _check(got, page, params, what):
    curl, sh, sc, st = got
    ref_curl, ref_s, ref_sc = K.estimate_curl(page, **params)
    assert st == 0, what
    ng, n = len(ref_s), ref_sc.size
    np.testing.assert_array_equal(curl, ref_curl, err_msg=str(what))
    np.testing.assert_array_equal(sh[:ng], ref_s, err_msg=str(what))
    np.testing.assert_array_equal(sc[:n].view(np.uint64), ref_sc.reshape(-1), err_msg=str(what))
    assert (sh[ng:] == SENTINEL).all() and (sc[n:] == SENTINEL).all(), what
    return ref_curl, ref_s, ref_sc


def _dewarp(cuda, page, shifts, group, fill, out_pitch, out_offset, pitch=None, offset=0):
    """raw aocr_dewarp_page into a poisoned buffer: (the whole buffer as the device left it, status)."""
    import aocr
    H, W = page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=99)
    buf = poisoned(cuda, out_offset + H * out_pitch + TAIL, POISON)
    sh = torch.tensor([int(v) for v in shifts], dtype=torch.int32, device=cuda)
    st = aocr.lib.aocr_dewarp_page(None, C.c_void_p(addr), pitch, H, W, group, aocr.ptr(sh), fill, C.c_void_p(buf.data_ptr() + out_offset), out_pitch)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st


def _expect(page, shifts, group, fill, out_pitch, out_offset):
    return expect_placed(K.dewarp(page, shifts, group, fill), out_pitch, out_offset, poison=POISON, tail=TAIL)


# H, W, kind; every shape runs at pitch = W, offset 0 and at pitch = W + 5, offset 3.  (64, 129): a one-column last group with group = 1
SHAPES = [(64, 97, "text"), (40, 31, "noise"), (9, 33, "noise"), (1, 1, "noise"), (1, 70, "noise"), (70, 1, "noise"), (64, 129, "text"),
          (300, 333, "text")]
MODES = [(128, 0), (-1, 0), (128, 1)]


def _page(H, W, kind, light):
    """a text page whose columns sag by up to 5 rows toward the right edge, or noise"""
    if kind == "noise":
        return noise_page(H, W, 31 * H + W)
    page = text_page(H, W, 31 * H + W, bool(light))
    out = np.full_like(page, 0 if light else 255)
    for x in range(W):
        d = (5 * x) // W
        out[d:, x] = page[:H - d, x]
    return out


@pytest.mark.parametrize("group,D", [(1, 5), (3, 0), (3, 64), (16, 5)], ids=["g1D5", "g3D0", "g3D64", "g16D5"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}{s[2]}" for s in SHAPES])
def test_estimate_and_dewarp_match_restatement(cuda, shape, group, D):
    H, W, kind = shape
    moved = 0
    for (thr, light), (dp, off) in zip(MODES + MODES[:1], ((0, 0), (5, 3), (5, 3), (5, 3))):
        page = _page(H, W, kind, light)
        params = dict(threshold=thr, light_text=light, group=group, max_shift=D, min_ink=4)
        ref_curl, ref_s, _ = _check(_estimate(cuda, page, params, W + dp, off), page, params, (shape, params, dp))
        moved += int(ref_curl[3])
        # the estimate's shifts through the dewarp, every byte of the output buffer
        fill = 0 if light else 255
        got, st = _dewarp(cuda, page, ref_s, group, fill, W + dp + 2, off, W + dp, off)
        assert st == 0
        np.testing.assert_array_equal(got, _expect(page, ref_s, group, fill, W + dp + 2, off), err_msg=str((shape, params)))
    if kind == "text" and W >= 129 and D >= 5 and K.n_groups(W, group) > 1:       # (64, 97) with group 3: the second group is one margin column
        assert moved > 0, "no pair saw the planted sag"


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_dewarp_hand_made_shifts(cuda, shape):
    """every byte of the output buffer -- the page's bytes, and the poison before the base, between W and the pitch and behind the last row --
    for shifts of every size: fractions of a row between the centres, whole pages (+-16384, and beyond the clamp), and none (a copy)."""
    H, W, _ = shape
    page = noise_page(H, W, 7 * H + W)
    rng = np.random.default_rng(H * W)
    for group in (1, 3, 16):
        ng = K.n_groups(W, group)
        small = rng.integers(-9, 10, ng)
        large = rng.integers(-H - 2, H + 3, ng)
        edge = np.where(np.arange(ng) % 2 == 0, 16384, -16384)
        beyond = np.where(np.arange(ng) % 3 == 0, 70000, -2 ** 31)
        for shifts, fill, (out_pitch, out_offset), (pitch, offset) in ((small, 255, (W, 0), (W, 0)), (small, 0, (W + 7, 5), (W + 5, 3)),
                                                                       (large, 0, (W + 7, 5), (W + 5, 3)), (edge, 255, (W + 7, 5), (W, 0)),
                                                                       (beyond, 7, (W, 0), (W + 5, 3)), (np.zeros(ng, int), 0, (W + 7, 5), (W + 5, 3))):
            got, st = _dewarp(cuda, page, shifts, group, fill, out_pitch, out_offset, pitch, offset)
            assert st == 0
            np.testing.assert_array_equal(got, _expect(page, shifts, group, fill, out_pitch, out_offset), err_msg=str((shape, group, shifts[:4])))
    assert np.array_equal(K.dewarp(page, np.zeros(K.n_groups(W, 3), int), 3, 0), page)


@pytest.mark.parametrize("amp", [12, 20])
def test_planted_pages(cuda, amp):
    page = curled_page(amp)
    ref_curl, ref_s, _ = _check(_estimate(cuda, page, PLANTED), page, PLANTED, amp)
    assert ref_curl[3] >= 4 and ref_s[0] > 0 and ref_s[-1] > 0
    got, st = _dewarp(cuda, page, ref_s, PLANTED["group"], 255, 800, 0)
    assert st == 0
    np.testing.assert_array_equal(got, _expect(page, ref_s, PLANTED["group"], 255, 800, 0))
    if amp == 20:
        otsu = dict(PLANTED, threshold=-1, group=2)
        _check(_estimate(cuda, page, otsu, 805, 3), page, otsu, "otsu")
        got = _estimate(cuda, page, PLANTED, scores=False)                      # scores_dev = NULL: the same shifts
        assert got[3] == 0 and np.array_equal(got[0], ref_curl) and np.array_equal(got[1][:len(ref_s)], ref_s) and (got[2] == SENTINEL).all()
        again = _estimate(cuda, page, PLANTED, 1024, 16)                        # and the same bits from another placement
        assert all(np.array_equal(a, b) for a, b in zip(again[:3], _estimate(cuda, page, PLANTED)[:3]))


def test_tie_gate_and_pages_without_ink(cuda):
    for pitch, offset in ((None, 0), (71, 3)):
        got = _estimate(cuda, tie_page(), TIE, pitch, offset)
        _check(got, tie_page(), TIE, "tie")
        assert got[1][:2].tolist() == [1, 0] and got[0].tolist() == [2, 1, 128, 1]
    got = _estimate(cuda, gated_page(), GATED, 101, 3)
    _, _, ref_sc = _check(got, gated_page(), GATED, "gated")
    assert got[1][:3].tolist() == [-2, 0, 0] and ref_sc[1].max() == 96          # the gated pair's scores are written all the same
    open_gate = dict(GATED, min_ink=3)
    assert _check(_estimate(cuda, gated_page(), open_gate), gated_page(), open_gate, "gate open")[1].tolist() == [-2, 0, 3]
    for page, params, thr in ((np.full((40, 70), 255, np.uint8), dict(threshold=128, light_text=0, group=1, max_shift=9, min_ink=0), 128),
                              (np.full((40, 70), 77, np.uint8), dict(threshold=-1, light_text=0, group=1, max_shift=9, min_ink=0), -1),
                              (np.full((40, 70), 77, np.uint8), dict(threshold=-1, light_text=1, group=1, max_shift=9, min_ink=64), -1)):
        got = _estimate(cuda, page, params)
        _check(got, page, params, params)
        assert got[0].tolist() == [3, 0, thr, 0] and not got[1][:3].any() and not got[2][:2 * 19].any()
    # D >= H, many row chunks per pair, and the widest page: 512 strips in 32 groups
    short = gated_page()[8:14]
    params = dict(threshold=128, light_text=0, group=1, max_shift=64, min_ink=1)
    _check(_estimate(cuda, short, params, 99, 1), short, params, "D >= H")
    tall = noise_page(1100, 70, 11)
    params = dict(threshold=60, light_text=0, group=1, max_shift=64, min_ink=0)
    _check(_estimate(cuda, tall, params, 75, 1), tall, params, "tall")
    wide = noise_page(16, 16384, 16)
    params = dict(threshold=40, light_text=0, group=16, max_shift=3, min_ink=0)
    _check(_estimate(cuda, wide, params, 16384, 5), wide, params, "wide")


def test_invalid_arguments_leave_the_outputs_untouched(cuda):
    import aocr
    page = text_page(40, 100, 3)
    good = dict(threshold=128, light_text=0, group=2, max_shift=8, min_ink=16)
    for bad, word in ((dict(threshold=255), "threshold"), (dict(threshold=-2), "threshold"), (dict(group=0), "group"), (dict(group=17), "group"),
                      (dict(max_shift=-1), "max_shift"), (dict(max_shift=65), "max_shift"), (dict(min_ink=-1), "min_ink"),
                      (dict(min_ink=(1 << 20) + 1), "min_ink"), (dict(reserved=1), "reserved")):
        curl, sh, sc, st = _estimate(cuda, page, dict(good, **bad))
        assert st != 0 and word in aocr.last_error(), (bad, aocr.last_error())
        assert (curl == SENTINEL).all() and (sh == SENTINEL).all() and (sc == SENTINEL).all(), bad
    for H, W, pit, word in ((0, 100, 100, "page size"), (40, 0, 100, "page size"), (16385, 100, 100, "page size"), (40, 16385, 16385, "page size"),
                            (16384, 4097, 4097, "page size"), (40, 100, 99, "pitch")):
        curl, sh, sc, st = _estimate(cuda, page, good, pit, 0, shape=(H, W))
        assert st != 0 and word in aocr.last_error(), (H, W, pit, aocr.last_error())
        assert (curl == SENTINEL).all() and (sh == SENTINEL).all() and (sc == SENTINEL).all()
    for args in ((0, 100, 2, 8), (40, 0, 2, 8), (16384, 4097, 2, 8), (40, 100, 0, 8), (40, 100, 17, 8), (40, 100, 2, -1), (40, 100, 2, 65)):
        assert aocr.lib.aocr_curl_scratch_bytes(*args) == 0 and "bad sizes" in aocr.last_error(), args
    need = aocr.lib.aocr_curl_scratch_bytes(40, 100, 2, 8)
    assert need > 0 and need % 256 == 0
    dev, addr, pitch = place(cuda, page)
    p = aocr.CurlParams(**good)
    scratch = torch.empty(1 << 16, dtype=torch.int64, device=cuda)
    curl = torch.full((4,), SENTINEL, dtype=torch.int32, device=cuda)
    sh = torch.full((2,), SENTINEL, dtype=torch.int32, device=cuda)
    call = aocr.lib.aocr_estimate_curl
    assert call(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), None, aocr.ptr(curl), aocr.ptr(sh), None) != 0
    assert call(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), aocr.ptr(scratch), None, aocr.ptr(sh), None) != 0
    assert call(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), aocr.ptr(scratch), aocr.ptr(curl), None, None) != 0
    assert call(None, C.c_void_p(addr), pitch, 40, 100, None, aocr.ptr(scratch), aocr.ptr(curl), aocr.ptr(sh), None) != 0
    assert call(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), aocr.ptr(scratch), aocr.ptr(curl), C.c_void_p(addr + 48), None) != 0
    assert "overlap" in aocr.last_error()
    out = poisoned(cuda, 40 * 100, POISON)
    for args, word in (((0, aocr.ptr(sh), 255, aocr.ptr(out), 100), "group"), ((17, aocr.ptr(sh), 255, aocr.ptr(out), 100), "group"),
                       ((2, None, 255, aocr.ptr(out), 100), "shifts_dev"), ((2, aocr.ptr(sh), 256, aocr.ptr(out), 100), "fill"),
                       ((2, aocr.ptr(sh), -1, aocr.ptr(out), 100), "fill"), ((2, aocr.ptr(sh), 255, aocr.ptr(out), 99), "out_pitch"),
                       ((2, aocr.ptr(sh), 255, None, 100), "out_dev"), ((2, aocr.ptr(sh), 255, C.c_void_p(addr + 50), 100), "overlap")):
        st = aocr.lib.aocr_dewarp_page(None, C.c_void_p(addr), pitch, 40, 100, *args)
        assert st != 0 and word in aocr.last_error(), (word, aocr.last_error())
    assert aocr.lib.aocr_dewarp_page(None, C.c_void_p(addr), pitch, 16384, 4097, 2, aocr.ptr(sh), 255, aocr.ptr(out), 4097) != 0
    torch.cuda.synchronize()
    assert (curl == SENTINEL).all() and (sh == SENTINEL).all() and (out == POISON).all()
    assert np.array_equal(dev.cpu().numpy()[:4000].reshape(40, 100), page)


def test_python_surface_estimate_then_dewarp_on_a_view(cuda):
    """estimate_curl_device and dewarp_page_device on a non-contiguous view; the shifts go from one to the other on the device."""
    import aocr
    page = curled_page(20)
    H, W = page.shape
    big = torch.zeros((H + 9, W + 30), dtype=torch.uint8, device=cuda)
    big[4:4 + H, 11:11 + W] = torch.from_numpy(page).to(cuda)
    view = big[4:4 + H, 11:11 + W]
    assert not view.is_contiguous()
    p = aocr.CurlParams(**PLANTED)
    curl, shifts, scores = aocr.estimate_curl_device(view, p, scores=True)
    ref_curl, ref_s, ref_sc = K.estimate_curl(page, **PLANTED)
    assert np.array_equal(curl.cpu().numpy(), ref_curl) and np.array_equal(shifts.cpu().numpy(), ref_s)
    assert scores.shape == ref_sc.shape and np.array_equal(scores.cpu().numpy().view(np.uint64), ref_sc)
    only = aocr.estimate_curl_device(view, p)
    assert len(only) == 2 and torch.equal(only[0], curl) and torch.equal(only[1], shifts)
    out = aocr.dewarp_page_device(view, shifts, p.group)
    assert out.shape == (H, W) and out.is_contiguous() and np.array_equal(out.cpu().numpy(), K.dewarp(page, ref_s, 4))
    assert np.array_equal(aocr.dewarp_page_device(view, shifts, 4, fill=0).cpu().numpy(), K.dewarp(page, ref_s, 4, 0))
    d = aocr.estimate_curl_device(torch.from_numpy(page).to(cuda))               # the defaults: Otsu, 4, 8, 64
    assert np.array_equal(d[1].cpu().numpy(), K.estimate_curl(page)[1])
    narrow = aocr.estimate_curl_device(view[:, :100], aocr.CurlParams(threshold=128, group=4), scores=True)      # ng == 1: no scores
    assert narrow[1].tolist() == [0] and narrow[2].shape == (0, 17) and narrow[0].tolist() == [1, 0, 128, 0]
    with pytest.raises(AssertionError):
        aocr.dewarp_page_device(view, shifts[:3], 4)


# ---- Model.recognize_page(dewarp=...) --------------------------------------------------------------------------------------------------------
def test_recognize_page_dewarp(cuda, monkeypatch):
    import aocr
    import skew_ref as S
    from model_harness import make
    B, W = 32, 100
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=W, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    straight, _ = planted_page(0)
    page = curled_page(20)
    H, PW = page.shape
    params = aocr.SegmentParams(**SEGMENT)
    ref_curl, ref_s, _ = K.estimate_curl(page, **PLANTED)                        # dewarp=True: the defaults with the segment threshold
    flat = K.dewarp(page, ref_s, 4, 255)
    want, want_counts = R.segment_page(flat, **SEGMENT)
    plain = m.recognize_page(straight, params, width=100)
    assert want_counts[1] == 15 == plain.n_lines

    for dewarp in (True, aocr.CurlParams(**PLANTED)):
        res = m.recognize_page(page, params, width=100, dewarp=dewarp)
        np.testing.assert_array_equal(res.curl_shifts, ref_s)
        assert res.curl_shifts.dtype == np.int32 and (res.curl_group, res.curl_max, res.curl_pairs) == (4, int(ref_curl[1]), int(ref_curl[3]))
        assert res.n_found == want_counts[0] and res.n_lines == plain.n_lines and res.threshold == 128 and not res.truncated
        np.testing.assert_array_equal(res.boxes, want[:, :4])
        np.testing.assert_array_equal(res.line, want[:, 4])
        np.testing.assert_array_equal(res.ink, want[:, 5])
        cx, cy = aocr.page.box_corners(want)
        ux, uy = K.uncurl_points(cx, cy, ref_s, 4)
        assert res.uncurled_corners.dtype == np.float64
        np.testing.assert_array_equal(res.uncurled_corners, np.stack([ux, uy], axis=2))
        assert not hasattr(res, "source_corners") and not hasattr(res, "skew_steps")
        n = len(want)
        flat_dev = torch.from_numpy(flat).to(cuda)
        boxes_dev = torch.from_numpy(np.ascontiguousarray(want)).to(cuda)
        for c0 in range(0, n, B):
            crops = aocr.crop_lines_device(flat_dev, boxes_dev[c0:c0 + B], None, 100)
            ref = m.recognize(crops)
            np.testing.assert_array_equal(res.labels[c0:c0 + B], ref.labels)
            np.testing.assert_array_equal(res.scores[c0:c0 + B], ref.scores)
            assert res.text[c0:c0 + B] == ref.text
    print(f"[recognize_page dewarp] shifts {res.curl_shifts.tolist()}, {n} boxes in {res.n_lines} lines")

    curled = m.recognize_page(page, params, width=100)                           # no dewarp: the lines run into each other
    assert curled.n_lines < 15 and not hasattr(curled, "curl_shifts") and not hasattr(curled, "uncurled_corners")
    b = m.recognize_page(straight, params, width=100, dewarp=None)               # dewarp=None is the call as it was
    assert sorted(vars(plain)) == sorted(vars(b))
    for k, v in vars(plain).items():
        assert np.array_equal(v, getattr(b, k)) if isinstance(v, np.ndarray) else v == getattr(b, k), k

    # with deskew as well: the skew words, the curl words and the shifts come back in the counts' one readback, and source_corners starts from
    # the uncurled corners with y rounded half up
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
    m.recognize_page(page, params, width=100, deskew=True)
    without, reads[:] = list(reads), []
    both = m.recognize_page(page, params, width=100, deskew=True, dewarp=True)
    assert len(reads) == len(without) == 2 and reads[0] == without[0] + 4 + len(ref_s), (without, reads)     # counts + words, then the boxes
    ref_skew, _ = S.estimate_skew(page, threshold=128, light_text=0, step_q16=64, n_steps=96)
    sheared = S.deskew(page, int(ref_skew[1]), 255)
    _, s2, _ = K.estimate_curl(sheared, **PLANTED)
    want2, _ = R.segment_page(K.dewarp(sheared, s2, 4, 255), **SEGMENT)
    np.testing.assert_array_equal(both.curl_shifts, s2)
    np.testing.assert_array_equal(both.boxes, want2[:, :4])
    assert both.skew_slope_q16 == int(ref_skew[1])
    ux, uy = K.uncurl_points(*aocr.page.box_corners(want2), s2, 4)
    np.testing.assert_array_equal(both.uncurled_corners, np.stack([ux, uy], axis=2))
    sx, sy = aocr.source_points(ux.astype(np.int64), np.floor(uy + 0.5).astype(np.int64), int(ref_skew[1]), H, PW)
    np.testing.assert_array_equal(both.source_corners, np.stack([sx, sy], axis=2))
    empty = m.recognize_page(np.full((40, 60), 255, np.uint8), dewarp=True)
    assert empty.boxes.shape == (0, 4) and empty.curl_shifts.tolist() == [0] and empty.uncurled_corners.shape == (0, 4, 2) and empty.threshold == -1
    m.check_health()
    m.shutdown()
