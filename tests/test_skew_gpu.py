"""GPU: aocr_estimate_skew and aocr_deskew_page against the numpy restatement (tests/skew_ref.py), and Model.recognize_page(deskew=...)
against the pieces it is made of.  Everything is exact equality: the winner, its slope, the threshold and every one of the 2K+1 scores of
the estimate, every byte of the deskewed page.  tests/test_skew_cpu.py shows on the restatement alone that the planted pages used here are
found and removed."""
import ctypes as C

import numpy as np
import pytest
import torch

import segment_ref as R
import skew_ref as S
from page_harness import expect_placed, garbage_scratch, guarded_words, place, poisoned
from skew_cases import PLANTED, PLANTED_K0, SEGMENT, noise_page, planted_page, text_page, tie_page

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD = 4                # entries of scores_dev beyond 2K+1 that every raw call gets: they must keep their sentinel
POISON = 0xAB
TAIL = 32                # bytes of the deskewed page's buffer behind the last row's pitch


def _estimate(cuda, page, params, pitch=None, offset=0, scores=True, shape=None):
    """raw aocr_estimate_skew: (skew (4), scores (2K+1) uint64 then GUARD sentinels, status); the scratch holds garbage."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset)
    p = aocr.SkewParams(**params)
    need = aocr.lib.aocr_skew_scratch_bytes(H, W, p.n_steps)
    scratch = garbage_scratch(cuda, need, 1 << 16)
    skew = guarded_words(cuda, 4, 0, SENTINEL, torch.int32)
    sc = guarded_words(cuda, 2 * max(p.n_steps, 0) + 1, GUARD, SENTINEL, torch.int64)
    st = aocr.lib.aocr_estimate_skew(None, C.c_void_p(addr), pitch, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(skew), aocr.ptr(sc) if scores else None)
    torch.cuda.synchronize()
    return skew.cpu().numpy(), sc.cpu().numpy(), st


def _check(got, page, params, what):
    skew, sc, st = got
    ref_skew, ref_sc = S.estimate_skew(page, **params)
    assert st == 0, what
    n = len(ref_sc)
    np.testing.assert_array_equal(skew, ref_skew, err_msg=str(what))
    np.testing.assert_array_equal(sc[:n].view(np.uint64), ref_sc, err_msg=str(what))
    assert (sc[n:] == SENTINEL).all(), what
    return ref_skew, ref_sc


# H, W, pitch, offset, kind, sweep
SHAPES = [(64, 97, 97, 0, "text", dict(step_q16=512, n_steps=16)), (64, 97, 102, 3, "text", dict(step_q16=512, n_steps=16)),
          (40, 31, 31, 0, "noise", dict(step_q16=1024, n_steps=8)), (40, 31, 36, 3, "text", dict(step_q16=1024, n_steps=8)),
          (9, 33, 33, 0, "noise", dict(step_q16=4096, n_steps=4)), (9, 33, 38, 3, "noise", dict(step_q16=4096, n_steps=4)),
          (1, 1, 1, 0, "noise", dict(step_q16=64, n_steps=3)), (1, 70, 75, 3, "noise", dict(step_q16=4096, n_steps=4)),
          (70, 1, 6, 3, "noise", dict(step_q16=4096, n_steps=4)), (300, 333, 333, 0, "text", dict(step_q16=64, n_steps=96)),
          (300, 333, 338, 3, "text", dict(step_q16=64, n_steps=96))]


@pytest.mark.parametrize("thr,light", [(128, 0), (-1, 0), (128, 1), (-1, 1)], ids=["fixed", "otsu", "fixed_light", "otsu_light"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}{s[4]}" for s in SHAPES])
def test_estimate_matches_restatement(cuda, shape, thr, light):
    H, W, pitch, offset, kind, sweep = shape
    page = text_page(H, W, 31 * H + W, bool(light)) if kind == "text" else noise_page(H, W, 31 * H + W)
    if kind == "text" and H >= 40:
        page = S.deskew(page, 1500, fill=0 if light else 255)                 # lines at a slope inside every sweep above
    params = dict(sweep, threshold=thr, light_text=light)
    ref_skew, ref_sc = _check(_estimate(cuda, page, params, pitch, offset), page, params, shape)
    print(f"[skew] {H}x{W} pitch {pitch} offset {offset} {kind} thr {thr} light {light}: {ref_skew.tolist()} scores {int(ref_sc.min())}..{int(ref_sc.max())}")
    if kind == "text" and H >= 64:
        assert ref_skew[0] < 0 and len(set(ref_sc.tolist())) >= 8, "the sweep saw nothing"


@pytest.mark.parametrize("k0", PLANTED_K0)
def test_planted_pages(cuda, k0):
    _, skewed = planted_page(k0)
    ref_skew, _ = _check(_estimate(cuda, skewed, PLANTED), skewed, PLANTED, k0)
    assert abs(int(ref_skew[0]) - k0) <= 1
    if k0 == 40:
        otsu = dict(PLANTED, threshold=-1)
        _check(_estimate(cuda, skewed, otsu, 805, 3), skewed, otsu, "otsu")
        got = _estimate(cuda, skewed, PLANTED, scores=False)                  # scores_dev = NULL: the same winner
        assert got[2] == 0 and np.array_equal(got[0], ref_skew) and (got[1] == SENTINEL).all()


def test_pages_without_ink(cuda):
    for page, params, thr in ((np.full((40, 70), 255, np.uint8), dict(threshold=128, light_text=0, step_q16=64, n_steps=9), 128),
                              (np.full((40, 70), 77, np.uint8), dict(threshold=-1, light_text=0, step_q16=64, n_steps=9), -1),
                              (np.full((40, 70), 77, np.uint8), dict(threshold=-1, light_text=1, step_q16=64, n_steps=9), -1)):
        skew, sc, st = _estimate(cuda, page, params)
        _check((skew, sc, st), page, params, params)
        assert skew.tolist() == [0, 0, thr, 0] and not sc[:19].any()


def test_parameter_edges(cuda):
    page = S.deskew(text_page(64, 97, 5), -2000)
    for sweep in (dict(step_q16=64, n_steps=0), dict(step_q16=64, n_steps=256), dict(step_q16=4096, n_steps=4), dict(step_q16=1, n_steps=256)):
        params = dict(sweep, threshold=128, light_text=0)
        _check(_estimate(cuda, page, params, 104, 1), page, params, sweep)
    # the largest products: W = 16384 at slope 0.25; strip 0 has c_b - cx = 16 - 8192: D_k = |(-8176 * 16384 + 32768) >> 16| = 2044
    wide = noise_page(16, 16384, 16)
    params = dict(threshold=40, light_text=0, step_q16=4096, n_steps=4)
    assert max(abs(o) for o in S.offsets(16384, 16384)) == 2044
    _check(_estimate(cuda, wide, params, 16384, 5), wide, params, "wide")
    # the long row axis, many row chunks per candidate: one strip (every candidate scores the same: k = 0), and a full strip plus a narrow one
    params = dict(threshold=128, light_text=0, step_q16=4096, n_steps=4)
    for W in (16, 40):
        tall = noise_page(8300, W, 83)
        ref_skew, ref_sc = _check(_estimate(cuda, tall, params, W, 1), tall, params, ("tall", W))
        assert (len(set(ref_sc.tolist())) == 1) == (W == 16)


def test_planted_tie_goes_to_the_negative_candidate(cuda):
    params = dict(threshold=128, light_text=0, step_q16=4096, n_steps=4)
    ref_skew, ref_sc = S.estimate_skew(tie_page(), **params)
    assert ref_sc[3] == ref_sc[5] == ref_sc.max() and (np.delete(ref_sc, [3, 5]) < ref_sc.max()).all()     # the restatement shows the tie
    for pitch, offset in ((None, 0), (71, 3)):
        skew, sc, st = _estimate(cuda, tie_page(), params, pitch, offset)
        _check((skew, sc, st), tie_page(), params, "tie")
        assert skew.tolist() == [-1, -4096, 128, 0]


def test_bit_identical_between_calls_and_pitches(cuda):
    _, skewed = planted_page(-17)
    params = dict(PLANTED, threshold=-1)
    a = _estimate(cuda, skewed, params)
    for other in (_estimate(cuda, skewed, params), _estimate(cuda, skewed, params, 837, 5), _estimate(cuda, skewed, params, 1024, 16)):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1])
    assert a[0][0] == -17


def test_invalid_arguments_leave_the_outputs_untouched(cuda):
    import aocr
    page = text_page(40, 100, 3)
    good = dict(threshold=128, light_text=0, step_q16=64, n_steps=8)
    for bad, word in ((dict(threshold=255), "threshold"), (dict(threshold=-2), "threshold"), (dict(step_q16=0), "step_q16"),
                      (dict(step_q16=4097), "step_q16"), (dict(n_steps=-1), "n_steps"), (dict(n_steps=257), "n_steps"),
                      (dict(step_q16=4096, n_steps=5), "16384")):
        skew, sc, st = _estimate(cuda, page, dict(good, **bad))
        assert st != 0 and word in aocr.last_error(), (bad, aocr.last_error())
        assert (skew == SENTINEL).all() and (sc == SENTINEL).all(), bad
    for H, W, pit, word in ((0, 100, 100, "page size"), (40, 0, 100, "page size"), (16385, 100, 100, "page size"), (40, 16385, 16385, "page size"),
                            (16384, 4097, 4097, "page size"), (40, 100, 99, "pitch")):
        skew, sc, st = _estimate(cuda, page, good, pit, 0, shape=(H, W))
        assert st != 0 and word in aocr.last_error(), (H, W, pit, aocr.last_error())
        assert (skew == SENTINEL).all() and (sc == SENTINEL).all()
    dev, addr, pitch = place(cuda, page)
    p = aocr.SkewParams(**good)
    scratch = torch.empty(1 << 16, dtype=torch.int64, device=cuda)
    skew = torch.full((4,), SENTINEL, dtype=torch.int32, device=cuda)
    assert aocr.lib.aocr_estimate_skew(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), None, aocr.ptr(skew), None) != 0
    assert aocr.lib.aocr_estimate_skew(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), aocr.ptr(scratch), None, None) != 0
    assert aocr.lib.aocr_estimate_skew(None, C.c_void_p(addr), pitch, 40, 100, None, aocr.ptr(scratch), aocr.ptr(skew), None) != 0
    out = poisoned(cuda, 40 * 100, POISON)
    for args, word in (((None, 0, 256, aocr.ptr(out), 100), "fill"), ((None, 0, -1, aocr.ptr(out), 100), "fill"), ((None, 0, 255, aocr.ptr(out), 99), "out_pitch"),
                       ((None, 0, 255, None, 100), "out_dev"), ((None, 0, 255, C.c_void_p(addr + 50), 100), "overlap")):
        st = aocr.lib.aocr_deskew_page(None, C.c_void_p(addr), pitch, 40, 100, *args)
        assert st != 0 and word in aocr.last_error(), (word, aocr.last_error())
    torch.cuda.synchronize()
    assert (skew == SENTINEL).all() and (out == POISON).all() and np.array_equal(dev.cpu().numpy()[:4000].reshape(40, 100), page)


# ---- aocr_deskew_page ----------------------------------------------------------------------------------------------------------------------
def _deskew(cuda, page, slope, fill, out_pitch, out_offset, skew_words=None, pitch=None, offset=0):
    """raw aocr_deskew_page into a poisoned buffer: (the whole buffer as the device left it, status)."""
    import aocr
    H, W = page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=99)
    buf = poisoned(cuda, out_offset + H * out_pitch + TAIL, POISON)
    sk = torch.tensor(skew_words, dtype=torch.int32, device=cuda) if skew_words is not None else None
    st = aocr.lib.aocr_deskew_page(None, C.c_void_p(addr), pitch, H, W, aocr.ptr(sk), slope, fill, C.c_void_p(buf.data_ptr() + out_offset), out_pitch)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st


def _expect(page, slope, fill, out_pitch, out_offset):
    return expect_placed(S.deskew(page, slope, fill), out_pitch, out_offset, poison=POISON, tail=TAIL)


@pytest.mark.parametrize("W", [1, 15, 16, 17, 333])
def test_deskew_matches_restatement(cuda, W):
    """every byte of the output buffer: the page's bytes, and the poison everywhere else (before the base, between W and the pitch, behind the
    last row).  Output rows aligned (pitch 16k at base 0 for W = 16), and unaligned (pitch W + 7 at base 5): heads, tails and rows shorter
    than one 16-byte store."""
    H = 41
    page = noise_page(H, W, 100 + W)
    for slope in (0, 64, -64, 4096, -4096, 16384, -16384):
        for fill, (out_pitch, out_offset), (pitch, offset) in ((255, (W, 0), (W, 0)), (0, (W + 7, 5), (W + 5, 3))):
            got, st = _deskew(cuda, page, slope, fill, out_pitch, out_offset, None, pitch, offset)
            assert st == 0
            np.testing.assert_array_equal(got, _expect(page, slope, fill, out_pitch, out_offset), err_msg=str((W, slope, fill, out_pitch)))
    assert np.array_equal(S.deskew(page, 0), page)
    # the slope from the device, the by-value argument ignored; and clamped on the device
    got, st = _deskew(cuda, page, 12345, 255, W + 7, 5, [9, -4096, 128, 0])
    np.testing.assert_array_equal(got, _expect(page, -4096, 255, W + 7, 5))
    got, st = _deskew(cuda, page, 0, 7, W + 7, 5, [0, 70000, 0, 0])
    np.testing.assert_array_equal(got, _expect(page, 16384, 7, W + 7, 5))
    got, st = _deskew(cuda, page, -2 ** 31, 7, W, 0)
    np.testing.assert_array_equal(got, _expect(page, -16384, 7, W, 0))


def test_python_surface_estimate_then_deskew_on_a_view(cuda):
    """estimate_skew_device and deskew_page_device on a non-contiguous view; the slope goes from one to the other on the device."""
    import aocr
    _, skewed = planted_page(40)
    H, W = skewed.shape
    big = torch.zeros((H + 9, W + 30), dtype=torch.uint8, device=cuda)
    big[4:4 + H, 11:11 + W] = torch.from_numpy(skewed).to(cuda)
    view = big[4:4 + H, 11:11 + W]
    assert not view.is_contiguous()
    p = aocr.SkewParams(threshold=128, step_q16=64, n_steps=100)
    skew, scores = aocr.estimate_skew_device(view, p, scores=True)
    ref_skew, ref_sc = S.estimate_skew(skewed, **PLANTED)
    assert np.array_equal(skew.cpu().numpy(), ref_skew) and np.array_equal(scores.cpu().numpy().view(np.uint64), ref_sc)
    only = aocr.estimate_skew_device(view, p)
    assert torch.equal(only, skew)
    out = aocr.deskew_page_device(view, skew)
    want = S.deskew(skewed, int(ref_skew[1]))
    assert out.shape == (H, W) and out.is_contiguous() and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(aocr.deskew_page_device(view, int(ref_skew[1]), fill=255).cpu().numpy(), want)
    assert np.array_equal(aocr.deskew_page_device(view, -320, fill=0).cpu().numpy(), S.deskew(skewed, -320, 0))
    d = aocr.estimate_skew_device(torch.from_numpy(skewed).to(cuda))             # the defaults: Otsu, 64, 96
    assert np.array_equal(d.cpu().numpy(), S.estimate_skew(skewed)[0])


# ---- Model.recognize_page(deskew=...) --------------------------------------------------------------------------------------------------------
def test_recognize_page_deskew(cuda):
    import aocr
    from model_harness import make
    B, W = 32, 100
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=W, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    straight, skewed = planted_page(40)
    H, PW = skewed.shape
    params = aocr.SegmentParams(**SEGMENT)
    ref_skew, _ = S.estimate_skew(skewed, threshold=128, light_text=0, step_q16=64, n_steps=96)   # deskew=True: the default sweep, the segment threshold
    flat = S.deskew(skewed, int(ref_skew[1]), 255)
    want, want_counts = R.segment_page(flat, **SEGMENT)
    assert abs(int(ref_skew[0]) - 40) <= 1 and want_counts[1] == 15

    for deskew in (True, aocr.SkewParams(threshold=128, step_q16=64, n_steps=96)):
        res = m.recognize_page(skewed, params, width=100, deskew=deskew)
        assert (res.skew_steps, res.skew_slope_q16) == (int(ref_skew[0]), int(ref_skew[1]))
        assert res.skew_deg == pytest.approx(np.degrees(np.arctan(int(ref_skew[1]) / 65536.0)), rel=1e-12)
        assert res.n_found == want_counts[0] and res.n_lines == 15 and res.threshold == 128 and not res.truncated
        np.testing.assert_array_equal(res.boxes, want[:, :4])
        np.testing.assert_array_equal(res.line, want[:, 4])
        np.testing.assert_array_equal(res.ink, want[:, 5])
        np.testing.assert_array_equal(res.source_corners, S.source_corners(want, int(ref_skew[1]), H, PW))
        n = len(want)
        assert res.labels.shape == (n, 12) and len(res.text) == n
        flat_dev = torch.from_numpy(flat).to(cuda)
        boxes_dev = torch.from_numpy(np.ascontiguousarray(want)).to(cuda)
        for c0 in range(0, n, B):
            crops = aocr.crop_lines_device(flat_dev, boxes_dev[c0:c0 + B], None, 100)
            ref = m.recognize(crops)
            np.testing.assert_array_equal(res.labels[c0:c0 + B], ref.labels)
            np.testing.assert_array_equal(res.scores[c0:c0 + B], ref.scores)
            assert res.text[c0:c0 + B] == ref.text
    print(f"[recognize_page deskew] skew {res.skew_steps} steps = {res.skew_deg:.3f} deg, {n} boxes in {res.n_lines} lines")

    plain = m.recognize_page(skewed, params, width=100)                          # no deskew: the lines run into each other
    assert plain.n_lines < 15 and not hasattr(plain, "skew_steps") and not hasattr(plain, "source_corners")
    a = m.recognize_page(straight, params, width=100)                            # deskew=None is the call as it was
    b = m.recognize_page(straight, params, width=100, deskew=None)
    assert a.n_lines == 15 and sorted(vars(a)) == sorted(vars(b))
    for k, v in vars(a).items():
        assert np.array_equal(v, getattr(b, k)) if isinstance(v, np.ndarray) else v == getattr(b, k), k
    light = m.recognize_page(255 - skewed, aocr.SegmentParams(threshold=128, light_text=1), width=100, deskew=True)   # fill 0: paper is dark
    assert light.skew_steps == int(ref_skew[0]) and light.n_lines == 15
    np.testing.assert_array_equal(light.boxes, want[:, :4])
    empty = m.recognize_page(np.full((40, 60), 255, np.uint8), deskew=True)
    assert empty.boxes.shape == (0, 4) and empty.skew_steps == 0 and empty.source_corners.shape == (0, 4, 2) and empty.threshold == -1
    m.check_health()
    m.shutdown()
