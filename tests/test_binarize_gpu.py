"""GPU: aocr_binarize_page against the numpy restatement (tests/binarize_ref.py), and Model.recognize_page(binarize=...).  Every comparison
is exact byte equality, of the whole output buffer: the binarised page, and the guard pattern everywhere else.  tests/test_binarize_cpu.py
shows on the restatement alone that the stained page used here cannot be segmented with any global threshold and can after the stage."""
import ctypes as C

import numpy as np
import pytest
import torch

import binarize_ref as B
import flatten_ref as F
import segment_ref as R
import skew_ref as S
from binarize_cases import CASES, hard_of, stained_page
from page_harness import csrc_constants, expect_placed, garbage_scratch, guarded_words, place, poisoned
from segment_cases import SEEDED_SHAPES, seeded_page

pytestmark = pytest.mark.gpu

POISON = 0xAB
AROUND = 99              # the bytes around every placed page: neither paper nor ink
TAIL = 32                # bytes of the output buffer behind the last row's pitch
SENTINEL = -77           # the count words before the call, and the guard words behind them ever after


def _binarize(cuda, page, radius=20, k_q8=51, rng=128, light_text=0, hard=0, pitch=None, offset=0, out_pitch=None, out_offset=0, shape=None,
              reserved=(0, 0, 0), scratch=True, counts=True):
    """raw aocr_binarize_page into a poisoned buffer over garbage scratch: (the whole output buffer as the device left it, status, the four
    count words and their four guard words, or None)."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=AROUND)
    out_pitch = out_pitch or page.shape[1]
    buf = poisoned(cuda, out_offset + page.shape[0] * out_pitch + TAIL, POISON)
    p = aocr.BinarizeParams(radius, k_q8, rng, light_text, hard)
    p.reserved[0], p.reserved[1], p.reserved[2] = reserved
    sc = garbage_scratch(cuda, aocr.lib.aocr_binarize_scratch_bytes(H, W, radius), 1 << 12)
    words = guarded_words(cuda, 4, 4, SENTINEL, torch.int32) if counts else None
    st = aocr.lib.aocr_binarize_page(None, C.c_void_p(addr), pitch, H, W, C.byref(p), aocr.ptr(sc) if scratch else None,
                                     C.c_void_p(buf.data_ptr() + out_offset), out_pitch, aocr.ptr(words))
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st, (words.cpu().numpy() if counts else None)


def _expect(want, out_pitch=None, out_offset=0):
    return expect_placed(want, out_pitch, out_offset, poison=POISON, tail=TAIL)


def _tiling():
    """the tile sizes of csrc/binarize.hip."""
    return csrc_constants("binarize.hip", ("BIN_EW", "BIN_TH", "BIN_RMAX"))


@pytest.mark.parametrize("light_text", [0, 1], ids=["dark", "light"])
@pytest.mark.parametrize("hard", [0, 1], ids=["gray", "hard"])
@pytest.mark.parametrize("shape", SEEDED_SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SEEDED_SHAPES])
def test_seeded_pages_match_restatement(cuda, shape, hard, light_text):
    """a seeded page at its offset and pitch; the output at an odd offset with a pitch > W: every byte around the page keeps its poison."""
    H, W, pitch, offset, seed = shape
    page = seeded_page(H, W, seed, light=bool(light_text))
    for r in (1, 3, 20) + ((63,) if H * W <= 70 * 257 else ()):
        want, want_counts = B.binarize(page, r, 51, 128, light_text, hard)
        for out_pitch, out_offset in ((W, 0), (W + 7, 5)):
            got, st, words = _binarize(cuda, page, r, 51, 128, light_text, hard, pitch, offset, out_pitch, out_offset)
            assert st == 0
            np.testing.assert_array_equal(got, _expect(want, out_pitch, out_offset), err_msg=str((shape, r, light_text, hard, out_pitch)))
            assert words.tolist() == want_counts.tolist() + [SENTINEL] * 4, (shape, r)
    if H >= 40:
        assert 0 < want_counts[0] < H * W and want_counts[1] < want_counts[2]     # ink and paper, and more than one threshold


@pytest.mark.parametrize("shape", [(8, 4100), (4100, 8)], ids=["wide", "tall"])
def test_long_axis_pages_cross_every_seam(cuda, shape):
    H, W = shape
    t = _tiling()
    assert len(t) == 3 and t["BIN_RMAX"] == 63 and t["BIN_EW"] - 2 * t["BIN_RMAX"] >= 1
    page = seeded_page(H, W, 4100 + H)
    for r in (3, 20, 63):
        tw = t["BIN_EW"] - 2 * r                                  # the output columns of a workgroup
        if W > H:      # many column tiles of one row tile; the last tile is ragged and its halo leaves the page
            assert W > 4 * tw and W % tw != 0 and H < t["BIN_TH"]
        else:          # many row tiles of one column tile narrower than its halo; the last one is ragged
            assert H > 4 * t["BIN_TH"] and H % t["BIN_TH"] != 0 and W < tw
        want, want_counts = B.binarize(page, r)
        got, st, words = _binarize(cuda, page, r, pitch=W + 3, offset=1, out_pitch=W + 9, out_offset=3)
        assert st == 0
        np.testing.assert_array_equal(got, _expect(want, W + 9, 3), err_msg=str(r))
        assert words[:4].tolist() == want_counts.tolist()


def test_tile_seams_in_both_axes_and_every_parameter(cuda):
    """a page of several tiles each way (the seams of rows and columns meet), with k, R and the radius away from their defaults."""
    t = _tiling()
    H, W = 2 * t["BIN_TH"] + 9, 2 * t["BIN_EW"] + 45
    page = seeded_page(H, W, H * 1000 + W)
    for r, k, rng, light_text, hard in ((20, 51, 128, 0, 0), (63, 255, 255, 0, 0), (7, 0, 1, 1, 0), (2, 128, 1, 0, 1), (31, 1, 64, 1, 1)):
        src = (255 - page).astype(np.uint8) if light_text else page
        want, want_counts = B.binarize(src, r, k, rng, light_text, hard)
        got, st, words = _binarize(cuda, src, r, k, rng, light_text, hard, pitch=W + 5, offset=7, out_pitch=W + 1, out_offset=1)
        assert st == 0
        np.testing.assert_array_equal(got, _expect(want, W + 1, 1), err_msg=str((r, k, rng, light_text, hard)))
        assert words[:4].tolist() == want_counts.tolist()


def test_page_smaller_than_the_window(cuda):
    rng = np.random.default_rng(11)
    for H, W, r in ((5, 9, 20), (3, 100, 63), (90, 2, 63), (1, 1, 63), (41, 41, 20), (40, 42, 20)):
        page = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
        want, want_counts = B.binarize(page, r)
        got, st, words = _binarize(cuda, page, r, pitch=W + 2, offset=3)
        assert st == 0
        np.testing.assert_array_equal(got, _expect(want), err_msg=str((H, W, r)))
        assert words[:4].tolist() == want_counts.tolist()


def test_hand_cases_determinism_and_null_counts(cuda):
    for name, page, (r, k, rng), want in CASES:
        got, st, _ = _binarize(cuda, page, r, k, rng)
        assert st == 0
        np.testing.assert_array_equal(got, _expect(want), err_msg=name)
        got, st, words = _binarize(cuda, page, r, k, rng, hard=1, counts=False)             # counts_dev NULL
        assert st == 0 and words is None
        np.testing.assert_array_equal(got, _expect(hard_of(want)), err_msg=name)
        got, st, _ = _binarize(cuda, (255 - page).astype(np.uint8), r, k, rng, light_text=1)
        assert st == 0
        np.testing.assert_array_equal(got, _expect(255 - want), err_msg=name)
    _, stained = stained_page()
    want, want_counts = B.binarize(stained)
    a, st, words = _binarize(cuda, stained)
    assert st == 0 and words.tolist() == want_counts.tolist() + [SENTINEL] * 4
    np.testing.assert_array_equal(a, _expect(want))
    for pitch, offset in ((None, 0), (837, 5), (1024, 16)):                     # two calls, three pitches
        b, st, w2 = _binarize(cuda, stained, pitch=pitch, offset=offset)
        assert st == 0 and np.array_equal(a, b) and np.array_equal(words, w2)


def test_invalid_arguments_leave_the_output_untouched(cuda):
    import aocr
    page = seeded_page(40, 100, 3)
    for kw, word in ((dict(radius=0), "radius"), (dict(radius=64), "radius"), (dict(k_q8=256), "k_q8"), (dict(k_q8=-1), "k_q8"),
                     (dict(rng=0), "range"), (dict(rng=256), "range"), (dict(reserved=(1, 0, 0)), "reserved"),
                     (dict(reserved=(0, 0, -1)), "reserved"), (dict(shape=(0, 100)), "page size"), (dict(shape=(40, 101)), "pitch"),
                     (dict(shape=(16384, 4097), pitch=100), "page size"), (dict(scratch=False), "NULL"), (dict(out_pitch=99), "out_pitch")):
        got, st, words = _binarize(cuda, page, **kw)
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (got == POISON).all() and (words == SENTINEL).all(), kw
    dev, addr, pitch = place(cuda, page, fill=AROUND)
    p = aocr.BinarizeParams()
    sc = torch.empty(1 << 14, dtype=torch.int64, device=cuda)
    for out in (addr + 50, addr - 50, addr):                                    # an output that overlaps the page
        assert aocr.lib.aocr_binarize_page(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), aocr.ptr(sc), C.c_void_p(out), 100, None) != 0
        assert "overlap" in aocr.last_error()
    assert aocr.lib.aocr_binarize_page(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), aocr.ptr(sc), C.c_void_p(addr + 8000), 100,
                                       C.c_void_p(addr + 16)) != 0 and "overlap" in aocr.last_error()       # counts inside the page
    assert aocr.lib.aocr_binarize_page(None, None, pitch, 40, 100, C.byref(p), aocr.ptr(sc), C.c_void_p(addr + 8000), 100, None) != 0
    assert aocr.lib.aocr_binarize_page(None, C.c_void_p(addr), pitch, 40, 100, None, aocr.ptr(sc), C.c_void_p(addr + 8000), 100, None) != 0
    assert aocr.lib.aocr_binarize_page(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), aocr.ptr(sc), None, 100, None) != 0
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy()[:4000].reshape(40, 100), page)
    for H, W, r in ((0, 10, 20), (10, 0, 20), (16385, 10, 20), (16384, 4097, 20), (10, 10, 0), (10, 10, 64), (10, 10, -1)):
        assert aocr.lib.aocr_binarize_scratch_bytes(H, W, r) == 0 and "bad sizes" in aocr.last_error()
    assert aocr.lib.aocr_binarize_scratch_bytes(16384, 4096, 63) > 0


def test_python_surface_on_a_view(cuda):
    import aocr
    _, stained = stained_page()
    H, W = stained.shape
    big = torch.zeros((H + 9, W + 30), dtype=torch.uint8, device=cuda)
    big[4:4 + H, 11:11 + W] = torch.from_numpy(stained).to(cuda)
    view = big[4:4 + H, 11:11 + W]
    assert not view.is_contiguous()
    out = aocr.binarize_page_device(view)                                       # the defaults: radius 20, k 51 / 256, R 128, dark, gray
    assert out.shape == (H, W) and out.is_contiguous() and out.dtype == torch.uint8
    want, want_counts = B.binarize(stained)
    assert np.array_equal(out.cpu().numpy(), want)
    out7, words = aocr.page.binarize_page_device(view, aocr.BinarizeParams(radius=7, hard=1), counts=True)
    want7, want7_counts = B.binarize(stained, 7, hard=1)
    assert np.array_equal(out7.cpu().numpy(), want7) and words.cpu().numpy().tolist() == want7_counts.tolist()
    inv = aocr.binarize_page_device(255 - view, aocr.BinarizeParams(light_text=1))
    assert np.array_equal(inv.cpu().numpy(), 255 - want)
    assert np.array_equal(big.cpu().numpy()[4:4 + H, 11:11 + W], stained)
    with pytest.raises(aocr.AocrError):
        aocr.binarize_page_device(view, aocr.BinarizeParams(radius=64))


def test_recognize_page_binarize(cuda):
    import aocr
    from model_harness import make
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=32, W=100, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    clean, stained = stained_page()
    want, want_counts = R.segment_page(clean)
    assert want_counts[0] == 109 and want_counts[1] == 15
    _, ref_counts = B.binarize(stained)

    seg = aocr.SegmentParams()
    res = m.recognize_page(stained, seg, width=100, binarize=True)
    assert seg.threshold == -1                                                  # the caller's params are not modified
    assert res.n_lines == 15 and res.n_found == 109 and res.threshold == 127
    assert res.binarize_radius == 20 and res.binarize_ink == ref_counts[0] and res.binarize_threshold_range == (ref_counts[1], ref_counts[2])
    np.testing.assert_array_equal(res.boxes, want[:, :4])
    np.testing.assert_array_equal(res.line, want[:, 4])
    res7 = m.recognize_page(stained, width=100, binarize=aocr.BinarizeParams(radius=15, hard=1))
    _, ref15 = B.binarize(stained, 15, hard=1)
    assert res7.binarize_radius == 15 and res7.n_lines == 15 and res7.binarize_ink == ref15[0]
    np.testing.assert_array_equal(res7.boxes, want[:, :4])

    plain = m.recognize_page(stained, width=100)                                # one threshold: lines lost or merged
    assert plain.n_lines < 15 and not hasattr(plain, "binarize_radius")
    off = m.recognize_page(stained, width=100, binarize=False)
    assert sorted(vars(plain)) == sorted(vars(off)) and not any(k.startswith("binarize") for k in vars(off))
    for k, v in vars(plain).items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(v, getattr(off, k), err_msg=k)
        else:
            assert v == getattr(off, k), k
    with pytest.raises(ValueError, match="BinarizeParams"):
        m.recognize_page(stained, width=100, binarize=3)

    skewed = S.deskew(stained, -17 * 64, 235)                                   # the stained page sheared by 17 steps, paper filled in
    both = m.recognize_page(skewed, width=100, flatten=True, binarize=True, deskew=True)
    chain, _ = B.binarize(F.flatten(skewed, 16))
    ref_skew, _ = S.estimate_skew(chain, threshold=127)
    assert (both.skew_steps, both.skew_slope_q16) == (int(ref_skew[0]), int(ref_skew[1])) and both.flatten_radius == 16
    flat, flat_counts = R.segment_page(S.deskew(chain, int(ref_skew[1]), 255), threshold=127)
    assert both.n_lines == flat_counts[1] and both.n_found == flat_counts[0]
    np.testing.assert_array_equal(both.boxes, flat[:, :4])

    light_res = m.recognize_page(255 - stained, aocr.SegmentParams(light_text=1), width=100, binarize=True)
    assert light_res.n_lines == 15 and light_res.binarize_ink == ref_counts[0]
    np.testing.assert_array_equal(light_res.boxes, want[:, :4])
    print(f"[recognize_page binarize] {res.n_found} boxes in {res.n_lines} lines, T {res.binarize_threshold_range}; "
          f"without: {plain.n_found} in {plain.n_lines}")
    m.check_health()
    m.shutdown()
