"""GPU: aocr_resize_page and aocr_estimate_glyph_size against the numpy restatement (tests/scale_ref.py) through the C ABI, and
Model.recognize_page(scale=...) against the call on the page at its native size.  Everything is exact equality: every byte of the output
buffer (the resized page, and the poison everywhere else), every word of the estimate."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_cases as CC
import scale_cases as SC
import scale_ref as S
from page_harness import corner_pixels, expect_placed, garbage_scratch, guarded_words, place, poisoned, same_reading
from rectify_cases import TEXT_SEGMENT

pytestmark = pytest.mark.gpu

SENTINEL = -7
POISON = 0xAB


# ---- aocr_resize_page ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SC.RESIZE_SHAPES, ids=[f"{s[0][0]}x{s[0][1]}p{s[0][2]}o{s[0][3]}_to_{s[1][0]}x{s[1][1]}" for s in SC.RESIZE_SHAPES])
def test_resize_matches_restatement(cuda, shape):
    """every byte of the output buffer: the resized page, and the poison before the base, between Wo and the pitch and behind the last row.
    The bytes around the source are 99: a read beside the page changes a sum."""
    import aocr
    (H, W, pitch, offset), (Ho, Wo), (out_pitch, out_offset) = shape
    page = SC.resize_source(H, W)
    out_pitch = out_pitch or Wo
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=99)
    want_img = S.resize_page(page, Ho, Wo)
    want = expect_placed(want_img, out_pitch, out_offset, poison=POISON, tail=32)
    buf = poisoned(cuda, len(want), POISON)
    st = aocr.lib.aocr_resize_page(None, C.c_void_p(addr), pitch, H, W, C.c_void_p(buf.data_ptr() + out_offset), out_pitch, Ho, Wo)
    assert st == 0, aocr.last_error()
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=str(shape))
    if (Ho, Wo) == (H, W):
        np.testing.assert_array_equal(want_img, page)
    if H * W >= 1 << 24:                                    # the block means lie strictly between 254 and 255: both roundings occur
        assert set(np.unique(want_img).tolist()) == {254, 255}


def test_resize_identities_and_python_surface(cuda):
    """an integer shrink is the rounded block mean, an integer growth is numpy.kron, a constant page stays constant; a non-contiguous view is
    taken with its stride as the pitch."""
    import aocr
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, (48, 120), dtype=np.uint8)
    big = torch.full((60, 140), 9, dtype=torch.uint8, device=cuda)
    big[4:52, 6:126] = torch.from_numpy(page).to(cuda)
    view = big[4:52, 6:126]
    for k in (2, 3, 8):
        mean = (page.astype(np.int64).reshape(48 // k, k, 120 // k, k).sum(axis=(1, 3)) + k * k // 2) // (k * k)
        np.testing.assert_array_equal(aocr.resize_page_device(view, (120 // k, 48 // k)).cpu().numpy(), mean)
        np.testing.assert_array_equal(aocr.resize_page_device(view, (120 * k, 48 * k)).cpu().numpy(), np.kron(page, np.ones((k, k), np.uint8)))
    np.testing.assert_array_equal(aocr.resize_page_device(view, (120, 48)).cpu().numpy(), page)
    for v in (0, 1, 254, 255):
        flat = torch.full((13, 29), v, dtype=torch.uint8, device=cuda)
        assert (aocr.resize_page_device(flat, (10, 31)) == v).all() and (aocr.resize_page_device(flat, (57, 5)) == v).all()
    with pytest.raises(ValueError):
        aocr.resize_page_device(view, (0, 10))


def test_resize_invalid_arguments_leave_the_output_untouched(cuda):
    import aocr
    page = SC.resize_source(63, 129)
    f = aocr.lib.aocr_resize_page
    for kw, word in ((dict(out=(63, 16)), "ratio"), (dict(out=(7, 129)), "ratio"), (dict(shape=(2, 100), out=(17, 100)), "ratio"),
                     (dict(shape=(63, 2), pitch=129, out=(63, 17)), "ratio"), (dict(shape=(0, 129)), "page size"),
                     (dict(shape=(63, 16385), pitch=16385), "page size"), (dict(pitch=128), "pitch"), (dict(out=(0, 129)), "output size"),
                     (dict(out=(63, 0)), "output size"), (dict(out=(16385, 129)), "output size"),
                     (dict(shape=(4096, 4096), pitch=4096, out=(16384, 4097)), "output size"), (dict(out_pitch=128), "out_pitch")):
        dev, addr, p = place(cuda, page)
        H, W = kw.get("shape", page.shape)
        Ho, Wo = kw.get("out", page.shape)
        buf = poisoned(cuda, 63 * 129 + 32, POISON)
        st = f(None, C.c_void_p(addr), kw.get("pitch", p), H, W, aocr.ptr(buf), kw.get("out_pitch", max(Wo, 1)), Ho, Wo)
        torch.cuda.synchronize()
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (buf == POISON).all(), kw
    dev, addr, p = place(cuda, page)
    buf = poisoned(cuda, 63 * 129 + 32, POISON)
    assert f(None, C.c_void_p(addr), p, 63, 129, None, 129, 63, 129) != 0 and "out_dev" in aocr.last_error()
    assert f(None, None, p, 63, 129, aocr.ptr(buf), 129, 63, 129) != 0 and "page_dev" in aocr.last_error()
    assert f(None, C.c_void_p(addr), p, 63, 129, C.c_void_p(addr + 100), 129, 20, 129) != 0 and "overlap" in aocr.last_error()
    torch.cuda.synchronize()
    assert (buf == POISON).all()
    assert np.array_equal(dev.cpu().numpy()[:63 * 129].reshape(63, 129), page)


# ---- aocr_estimate_glyph_size ----------------------------------------------------------------------------------------------------------------
def _glyph(cuda, page, params=None, pitch=None, offset=0, shape=None, around=255, **kw):
    """raw aocr_estimate_glyph_size: (glyph (8) then 4 sentinels, status); the scratch holds garbage."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=around)
    p = params if params is not None else aocr.GlyphParams(**kw)
    need = aocr.lib.aocr_glyph_scratch_bytes(max(min(H, 16384), 1), max(min(W, 4096), 1))
    scratch = garbage_scratch(cuda, need, 1 << 12)
    out = guarded_words(cuda, 8, 4, SENTINEL, torch.int32)
    st = aocr.lib.aocr_estimate_glyph_size(None, C.c_void_p(addr), pitch, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy(), st


@pytest.mark.parametrize("case", SC.HAND, ids=[c["name"] for c in SC.HAND])
def test_glyph_hand_cases(cuda, case):
    """all 8 words, twice (the same words), then with a wider pitch at an odd base whose surrounding bytes are ink: a read beside the page
    changes a box."""
    light = case["params"].get("light_text", 0)
    W = case["page"].shape[1]
    for pitch, offset in ((None, 0), (None, 0), (W + 7, 5)):
        got, st = _glyph(cuda, case["page"], None, pitch, offset, around=255 if light else 0, **case["params"])
        assert st == 0, case["name"]
        np.testing.assert_array_equal(got[:8], case["want"], err_msg=str((case["name"], pitch, offset)))
        assert (got[8:] == SENTINEL).all()


_ATLAS = [(face, scale, quarter) for face in (0, 1, 2) for scale in (1, 2) for quarter in (0, 1)]


@pytest.mark.parametrize("face,scale,quarter", _ATLAS, ids=[f"face{f}_scale{s}_q{q}" for f, s, q in _ATLAS])
def test_glyph_atlas_pages(cuda, face, scale, quarter):
    """Otsu on the upright pages, a fixed threshold on the turned ones; the median is the one the CPU tests pin."""
    page = np.ascontiguousarray(np.rot90(SC.text_page(face, scale), -quarter))
    thr = 128 if quarter else -1
    want = S.estimate_glyph_size(page, threshold=thr)
    got, st = _glyph(cuda, page, threshold=thr)
    assert st == 0
    np.testing.assert_array_equal(got[:8], want)
    assert (got[8:] == SENTINEL).all() and want[3] >= 300
    if thr == 128:
        assert want[0] == SC.ATLAS_MEDIAN[(scale, face)]
    print(f"[glyph size] face {face} scale {scale} quarter {quarter}: {want.tolist()}")


def test_glyph_component_across_tile_borders(cuda):
    """a frame one pixel wide around a 37 x 137 page crosses every tile border and is one component with the box 137 x 37: it counts under the
    default max_aspect 8 (41 of 41 components), not under 3 (40 of 41).  The 40 words are 9 x 5 boxes: the size is 5."""
    page = CC.framed_text(16, 64)
    assert page.shape == (37, 137)
    for kw, n in ((dict(threshold=128), 41), (dict(threshold=-1), 41), (dict(threshold=128, max_aspect=3), 40),
                  (dict(threshold=128, connectivity=4, min_size=1), 41)):
        got, st = _glyph(cuda, page, **kw)
        want = S.estimate_glyph_size(page, **kw)
        assert st == 0
        np.testing.assert_array_equal(got[:8], want, err_msg=str(kw))
        assert want[:5].tolist() == [5, 5, 5, n, 41]


def test_glyph_python_surface(cuda):
    import aocr
    page = SC.text_page(1, 2)
    big = torch.full((page.shape[0] + 9, page.shape[1] + 20), 0, dtype=torch.uint8, device=cuda)
    big[4:4 + page.shape[0], 11:11 + page.shape[1]] = torch.from_numpy(page).to(cuda)
    words = aocr.estimate_glyph_size_device(big[4:4 + page.shape[0], 11:11 + page.shape[1]]).cpu().numpy()
    np.testing.assert_array_equal(words, S.estimate_glyph_size(page))
    inv = torch.from_numpy((255 - page).astype(np.uint8)).to(cuda)
    np.testing.assert_array_equal(aocr.estimate_glyph_size_device(inv, aocr.GlyphParams(threshold=126, light_text=1)).cpu().numpy(),
                                  S.estimate_glyph_size(255 - page, threshold=126, light_text=1))


def test_glyph_invalid_arguments_leave_the_output_untouched(cuda):
    import aocr
    page = SC.text_page(0, 2)
    H, W = page.shape
    bad = [(dict(threshold=255), "threshold"), (dict(threshold=-2), "threshold"), (dict(connectivity=6), "connectivity"), (dict(min_size=0), "min_size"),
           (dict(min_size=9, max_size=8), "max_size"), (dict(max_size=1025), "max_size"), (dict(max_aspect=0), "max_aspect")]
    for kw, word in bad:
        got, st = _glyph(cuda, page, **kw)
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (got == SENTINEL).all()
    for i in (0, 1):
        p = aocr.GlyphParams()
        p.reserved[i] = 1
        got, st = _glyph(cuda, page, p)
        assert st != 0 and "reserved" in aocr.last_error() and (got == SENTINEL).all()
    for shape, pitch, word in (((0, W), None, "page size"), ((H, 16385), 16385, "page size"), (None, W - 1, "pitch")):
        got, st = _glyph(cuda, page, None, pitch, 0, shape)
        assert st != 0 and word in aocr.last_error() and (got == SENTINEL).all()
    assert aocr.lib.aocr_glyph_scratch_bytes(0, 5) == 0 and aocr.lib.aocr_glyph_scratch_bytes(16384, 4097) == 0
    assert aocr.lib.aocr_glyph_scratch_bytes(16384, 4096) % 16 == 0 and aocr.lib.aocr_glyph_scratch_bytes(1, 1) > 0
    dev, addr, pt = place(cuda, page)
    out = torch.full((8,), SENTINEL, dtype=torch.int32, device=cuda)
    need = aocr.lib.aocr_glyph_scratch_bytes(H, W)
    scratch = torch.empty((need + 7) // 8 + 8, dtype=torch.int64, device=cuda)
    f, p = aocr.lib.aocr_estimate_glyph_size, aocr.GlyphParams()
    assert f(None, C.c_void_p(addr), pt, H, W, None, aocr.ptr(scratch), aocr.ptr(out)) != 0
    assert f(None, C.c_void_p(addr), pt, H, W, C.byref(p), None, aocr.ptr(out)) != 0
    assert f(None, C.c_void_p(addr), pt, H, W, C.byref(p), aocr.ptr(scratch), None) != 0
    assert f(None, None, pt, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(out)) != 0
    assert f(None, C.c_void_p(addr), pt, H, W, C.byref(p), C.c_void_p(scratch.data_ptr() + 8), aocr.ptr(out)) != 0 and "aligned" in aocr.last_error()
    assert f(None, C.c_void_p(addr), pt, H, W, C.byref(p), aocr.ptr(scratch), C.c_void_p(scratch.data_ptr() + 64)) != 0 and "overlap" in aocr.last_error()
    assert f(None, C.c_void_p(addr), pt, H, W, C.byref(p), aocr.ptr(scratch), C.c_void_p(addr + 64)) != 0 and "overlap" in aocr.last_error()
    assert f(None, C.c_void_p(scratch.data_ptr() + 1024), W, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(out)) != 0 and "overlap" in aocr.last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert np.array_equal(dev.cpu().numpy()[:H * W].reshape(H, W), page)


# ---- Model.recognize_page(scale=...) ---------------------------------------------------------------------------------------------------------
NEW_FIELDS = ("scaled", "scale_size", "scale_quartiles", "scale_glyphs", "scale_shape", "unscaled_corners")


def test_recognize_page_scale(cuda):
    import aocr
    from model_harness import make
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=32, W=100, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    p = SC.text_page(0, 1)
    H, W = p.shape
    twice = np.kron(p, np.ones((2, 2), np.uint8))
    params = aocr.SegmentParams(**TEXT_SEGMENT)
    base = m.recognize_page(p, params, width=100)
    assert base.n_lines == 12 and len(base.text) == len(base.boxes) > 50
    for k in NEW_FIELDS:
        assert not hasattr(base, k)
    for none in (None, False):                                                               # scale=None is the call as it was
        same = m.recognize_page(p, params, width=100, scale=none)
        assert sorted(vars(same)) == sorted(vars(base))
        same_reading(same, base)

    # a ratio given: the 2x page halved is p exactly, so the reading is that of p, and the corners map back onto the 2x page
    half = m.recognize_page(twice, params, width=100, scale=0.5)
    same_reading(half, base)
    np.testing.assert_array_equal(half.scores, base.scores)
    assert half.scaled is True and half.scale_shape == (W, H) and half.scale_size is None and half.scale_quartiles is None and half.scale_glyphs is None
    cx, cy = corner_pixels(base.boxes)
    ux, uy = S.unscale(cx, cy, 2 * H, 2 * W, H, W)
    assert half.unscaled_corners.shape == (len(base.boxes), 4, 2) and half.unscaled_corners.dtype == np.float64
    np.testing.assert_array_equal(half.unscaled_corners, np.stack([ux, uy], 2))
    np.testing.assert_array_equal(half.unscaled_corners, np.stack([2 * cx + 0.5, 2 * cy + 0.5], 2))

    # scale=True on the native page: 15 pixels is within the tolerance of 16, nothing is resized
    want = S.estimate_glyph_size(p, threshold=params.threshold)
    for how in (True, aocr.ScaleParams(aocr.GlyphParams(threshold=params.threshold))):
        auto = m.recognize_page(p, params, width=100, scale=how)
        same_reading(auto, base)
        assert auto.scaled is False and auto.scale_shape is None and auto.scale_size == want[0] == 15
        assert auto.scale_quartiles == (int(want[1]), int(want[2])) and auto.scale_glyphs == want[3]
        np.testing.assert_array_equal(auto.unscaled_corners, np.stack([cx, cy], 2))

    # scale=True on the 2x page: 30 pixels, planned down to 16 / 30
    want2 = S.estimate_glyph_size(twice, threshold=params.threshold)
    big = m.recognize_page(twice, params, width=100, scale=True)
    plan = aocr.scale_plan(30, int(want2[3]), 2 * H, 2 * W)
    assert big.scaled is True and big.scale_size == want2[0] == 30 and big.scale_glyphs == want2[3]
    assert big.scale_shape == plan == S.scale_plan(30, int(want2[3]), 2 * H, 2 * W)
    assert big.n_lines == 12
    bx, by = corner_pixels(big.boxes)
    ux, uy = S.unscale(bx, by, 2 * H, 2 * W, plan[1], plan[0])
    np.testing.assert_array_equal(big.unscaled_corners, np.stack([ux, uy], 2))

    # with rectify, photo_corners goes through the scale map first: the image corners as the quad make the warp a copy
    quad = [(0, 0), (2 * W - 1, 0), (2 * W - 1, 2 * H - 1), (0, 2 * H - 1)]
    both = m.recognize_page(twice, params, width=100, rectify=quad, scale=0.5)
    same_reading(both, base)
    np.testing.assert_array_equal(both.photo_corners, half.unscaled_corners)
    np.testing.assert_array_equal(both.unscaled_corners, half.unscaled_corners)

    for bad in ("x", -1.0, 0, float("nan"), [0.5]):
        with pytest.raises(ValueError):
            m.recognize_page(p, params, width=100, scale=bad)
    print(f"[recognize_page scale] {len(base.text)} boxes in {base.n_lines} lines; 2x page: size {big.scale_size}, shape {big.scale_shape}")
    m.check_health()
    m.shutdown()
