"""GPU: aocr_warp_page and aocr_find_page_quad against the numpy restatement (tests/rectify_ref.py) through the C ABI, and
Model.recognize_page(rectify=...) against the call on the reference-rectified page.  Everything is exact equality: every byte of the output
buffer (the warped page, and the poison everywhere else), every word of the quad."""
import ctypes as C

import numpy as np
import pytest
import torch

import rectify_cases as RC
import rectify_ref as R
from page_harness import corner_pixels, expect_placed, garbage_scratch, guarded_words, place, poisoned, same_reading
from segment_cases import seeded_page

pytestmark = pytest.mark.gpu

SENTINEL = -7
POISON = 0xAB


def _coef(c):
    return (C.c_double * 9)(*[float(v) for v in c])


_pages = {}


def _seeded(H, W):
    if (H, W) not in _pages:
        _pages[(H, W)] = seeded_page(H, W, 17 * H + W)
    return _pages[(H, W)]


# ---- aocr_warp_page --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RC.WARP_SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in RC.WARP_SHAPES])
def test_warp_matches_restatement(cuda, shape):
    """every byte of the output buffer: the warped page, and the poison before the base, between Wo and the pitch and behind the last row.  A
    tight output at the buffer's base, and one with a wider pitch at an odd base.  The bytes around the source are neither fill nor page."""
    import aocr
    H, W, pitch, offset = shape
    page = _seeded(H, W)
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=99)
    n_fill = n_page = 0
    for name, coef, Ho, Wo in RC.warp_cases(H, W):
        for fill, (out_pitch, out_offset) in ((255, (Wo, 0)), (7, (Wo + 5, 3))):
            want_img = R.warp_page(page, coef, fill, Ho, Wo)
            want = expect_placed(want_img, out_pitch, out_offset, poison=POISON, tail=32)
            buf = poisoned(cuda, len(want), POISON)
            st = aocr.lib.aocr_warp_page(None, C.c_void_p(addr), pitch, H, W, _coef(coef), fill, C.c_void_p(buf.data_ptr() + out_offset), out_pitch,
                                         Ho, Wo)
            assert st == 0, (name, aocr.last_error())
            np.testing.assert_array_equal(buf.cpu().numpy(), want, err_msg=str((shape, name, out_pitch)))
            n_fill += int((want_img == fill).sum())
            n_page += int((want_img != fill).sum())
        if name in ("identity", "identity_hand"):
            np.testing.assert_array_equal(want_img, page)
        if name.startswith(("nan", "inf")):
            assert (want_img == fill).all()
    assert n_fill > 0 and n_page > 0


def test_warp_python_surface_and_views(cuda):
    import aocr
    page = _seeded(63, 129)
    big = torch.full((70, 140), 9, dtype=torch.uint8, device=cuda)
    big[4:67, 6:135] = torch.from_numpy(page).to(cuda)
    view = big[4:67, 6:135]                                                                  # a non-contiguous view: its stride is the pitch
    quad = [40, 0, 90, 1, 128, 62, 0, 61]
    size, coef = aocr.rectify_plan(quad)
    (Wo, Ho), cr = R.rectify_plan(quad)
    assert size == (Wo, Ho) and coef.tobytes() == cr.tobytes()
    out = aocr.warp_page_device(view, coef, size, 200)
    assert out.shape == (Ho, Wo)
    np.testing.assert_array_equal(out.cpu().numpy(), R.warp_page(page, cr, 200, Ho, Wo))
    x0, y0, w, h = 10, 5, 100, 40                                                            # the consequence: a rectangle is a copy
    size, coef = aocr.rectify_plan([x0, y0, x0 + w, y0, x0 + w, y0 + h, x0, y0 + h])
    np.testing.assert_array_equal(aocr.warp_page_device(view, coef, size).cpu().numpy(), page[y0:y0 + h + 1, x0:x0 + w + 1])


def test_warp_invalid_arguments_leave_the_output_untouched(cuda):
    import aocr
    page = _seeded(63, 129)
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    for kw, word in ((dict(fill=256), "fill"), (dict(fill=-1), "fill"), (dict(shape=(0, 129)), "page size"), (dict(shape=(63, 16385), pitch=16385), "page size"),
                     (dict(pitch=128), "pitch"), (dict(out=(0, 129)), "output size"), (dict(out=(63, 0)), "output size"),
                     (dict(out=(16385, 4)), "output size"), (dict(out=(16384, 4097)), "output size"), (dict(out_pitch=128), "out_pitch")):
        dev, addr, p = place(cuda, page)
        H, W = kw.get("shape", page.shape)
        Ho, Wo = kw.get("out", page.shape)
        buf = poisoned(cuda, 63 * 129 + 32, POISON)
        st = aocr.lib.aocr_warp_page(None, C.c_void_p(addr), kw.get("pitch", p), H, W, _coef(ident), kw.get("fill", 255), aocr.ptr(buf),
                                     kw.get("out_pitch", max(Wo, 1)), Ho, Wo)
        torch.cuda.synchronize()
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (buf == POISON).all(), kw
    dev, addr, p = place(cuda, page)
    buf = poisoned(cuda, 63 * 129 + 32, POISON)
    assert aocr.lib.aocr_warp_page(None, C.c_void_p(addr), p, 63, 129, None, 255, aocr.ptr(buf), 129, 63, 129) != 0 and "coef" in aocr.last_error()
    assert aocr.lib.aocr_warp_page(None, C.c_void_p(addr), p, 63, 129, _coef(ident), 255, None, 129, 63, 129) != 0 and "out_dev" in aocr.last_error()
    assert aocr.lib.aocr_warp_page(None, None, p, 63, 129, _coef(ident), 255, aocr.ptr(buf), 129, 63, 129) != 0
    assert aocr.lib.aocr_warp_page(None, C.c_void_p(addr), p, 63, 129, _coef(ident), 255, C.c_void_p(addr + 100), 129, 20, 129) != 0
    assert "overlap" in aocr.last_error()
    torch.cuda.synchronize()
    assert (buf == POISON).all()
    assert np.array_equal(dev.cpu().numpy()[:63 * 129].reshape(63, 129), page)


# ---- aocr_find_page_quad ---------------------------------------------------------------------------------------------------------------------
def _quad(cuda, page, threshold, dark, pitch=None, offset=0, shape=None, around=0):
    """raw aocr_find_page_quad: (quad (16) then 4 sentinels, status); the scratch holds garbage."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=around)
    need = aocr.lib.aocr_quad_scratch_bytes(max(min(H, 16384), 1), max(min(W, 4096), 1))
    scratch = garbage_scratch(cuda, need, 1 << 12)
    out = guarded_words(cuda, 16, 4, SENTINEL, torch.int32)
    st = aocr.lib.aocr_find_page_quad(None, C.c_void_p(addr), pitch, H, W, threshold, dark, aocr.ptr(scratch), aocr.ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy(), st


_QUAD_CASES = RC.quad_cases()


@pytest.mark.parametrize("case", _QUAD_CASES, ids=[c["name"] for c in _QUAD_CASES])
def test_quad_matches_restatement(cuda, case):
    """all 16 words, twice (the same words), then with a wider pitch at an odd base whose surrounding bytes are what the threshold takes for
    paper: a read beside the page changes the sheet."""
    page, thr, dark = case["page"], case["threshold"], case["dark_paper"]
    want = R.find_page_quad(page, thr, dark)
    W = page.shape[1]
    for pitch, offset in ((None, 0), (None, 0), (W + 7, 5), (W + 1, 1)):
        got, st = _quad(cuda, page, thr, dark, pitch, offset, around=0 if dark else 255)
        assert st == 0, case["name"]
        np.testing.assert_array_equal(got[:16], want, err_msg=str((case["name"], pitch, offset)))
        assert (got[16:] == SENTINEL).all()
    print(f"[quad] {case['name']}: {want[:12].tolist()}")


def test_quad_fixed_threshold_against_otsu(cuda):
    """a photograph whose paper is 235, desk 60 and ink dark: Otsu and any fixed threshold between desk and paper find the same corners; a
    threshold below the desk takes the whole frame for the sheet."""
    ph, q = RC.photo("keystone")
    otsu, _ = _quad(cuda, ph, -1, 0)
    fixed, _ = _quad(cuda, ph, 128, 0)
    low, _ = _quad(cuda, ph, 40, 0)
    assert otsu[:8].tolist() == fixed[:8].tolist() == q and otsu[11] == fixed[11] == 1 and fixed[8] == 128 and otsu[8] != 128
    H, W = ph.shape
    assert low[:8].tolist() == [0, 0, W - 1, 0, W - 1, H - 1, 0, H - 1] and low[8] == 40
    np.testing.assert_array_equal(low[:16], R.find_page_quad(ph, 40, 0))


def test_quad_python_surface(cuda):
    import aocr
    ph, q = RC.photo("turned")
    big = torch.full((ph.shape[0] + 9, ph.shape[1] + 20), 255, dtype=torch.uint8, device=cuda)
    big[4:4 + ph.shape[0], 11:11 + ph.shape[1]] = torch.from_numpy(ph).to(cuda)
    words = aocr.find_page_quad_device(big[4:4 + ph.shape[0], 11:11 + ph.shape[1]]).cpu().numpy()
    np.testing.assert_array_equal(words, R.find_page_quad(ph))
    assert words[:8].tolist() == q
    np.testing.assert_array_equal(aocr.find_page_quad_device(torch.from_numpy((255 - ph).astype(np.uint8)).to(cuda), -1, 1).cpu().numpy()[:8], q)


def test_quad_invalid_arguments_leave_the_output_untouched(cuda):
    import aocr
    page = _seeded(70, 257)
    for thr, shape, pitch, word in ((255, None, None, "threshold"), (-2, None, None, "threshold"), (128, (0, 257), None, "page size"),
                                    (128, (70, 16385), 16385, "page size"), (128, None, 256, "pitch")):
        got, st = _quad(cuda, page, thr, 0, pitch, 0, shape)
        assert st != 0 and word in aocr.last_error(), (thr, shape, pitch, aocr.last_error())
        assert (got == SENTINEL).all()
    assert aocr.lib.aocr_quad_scratch_bytes(0, 5) == 0 and aocr.lib.aocr_quad_scratch_bytes(16384, 4097) == 0
    assert aocr.lib.aocr_quad_scratch_bytes(16384, 4096) % 16 == 0 and aocr.lib.aocr_quad_scratch_bytes(1, 1) > 0
    dev, addr, p = place(cuda, page)
    out = torch.full((16,), SENTINEL, dtype=torch.int32, device=cuda)
    need = aocr.lib.aocr_quad_scratch_bytes(70, 257)
    scratch = torch.empty((need + 7) // 8 + 8, dtype=torch.int64, device=cuda)
    f = aocr.lib.aocr_find_page_quad
    assert f(None, C.c_void_p(addr), p, 70, 257, 128, 0, None, aocr.ptr(out)) != 0
    assert f(None, C.c_void_p(addr), p, 70, 257, 128, 0, aocr.ptr(scratch), None) != 0
    assert f(None, None, p, 70, 257, 128, 0, aocr.ptr(scratch), aocr.ptr(out)) != 0
    assert f(None, C.c_void_p(addr), p, 70, 257, 128, 0, C.c_void_p(scratch.data_ptr() + 8), aocr.ptr(out)) != 0 and "aligned" in aocr.last_error()
    assert f(None, C.c_void_p(addr), p, 70, 257, 128, 0, aocr.ptr(scratch), C.c_void_p(scratch.data_ptr() + 64)) != 0 and "overlap" in aocr.last_error()
    assert f(None, C.c_void_p(addr), p, 70, 257, 128, 0, aocr.ptr(scratch), C.c_void_p(addr + 64)) != 0 and "overlap" in aocr.last_error()
    assert f(None, C.c_void_p(scratch.data_ptr() + 1024), 257, 70, 257, 128, 0, aocr.ptr(scratch), aocr.ptr(out)) != 0 and "overlap" in aocr.last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert np.array_equal(dev.cpu().numpy()[:70 * 257].reshape(70, 257), page)


# ---- Model.recognize_page(rectify=...) -------------------------------------------------------------------------------------------------------
NEW_FIELDS = ("rectified", "rectify_quad", "rectify_size", "rectify_area", "photo_corners")


def test_recognize_page_rectify(cuda):
    import aocr
    from model_harness import make
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=32, W=100, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    page, photo, quad = RC.text_photo()
    (Wo, Ho), coef = R.rectify_plan(quad)
    upright = R.warp_page(photo, coef, 255, Ho, Wo)                                          # what the device must produce and then read
    params = aocr.SegmentParams(**RC.TEXT_SEGMENT)
    base = m.recognize_page(upright, params, width=100)
    assert base.n_lines == 3 and len(base.text) == len(base.boxes) > 20
    for k in NEW_FIELDS:
        assert not hasattr(base, k)
    for none in (None, False):                                                               # rectify=None is the call as it was
        same = m.recognize_page(upright, params, width=100, rectify=none)
        assert sorted(vars(same)) == sorted(vars(base))
        same_reading(same, base)

    area = int(R.find_page_quad(photo)[9])
    for how in (True, aocr.RectifyParams(), [tuple(quad[2 * i:2 * i + 2]) for i in range(4)], np.array(quad).reshape(4, 2)):
        res = m.recognize_page(photo, params, width=100, rectify=how)
        same_reading(res, base)
        np.testing.assert_array_equal(res.scores, base.scores)
        assert res.rectified is True and res.rectify_size == (Wo, Ho)
        np.testing.assert_array_equal(res.rectify_quad, np.array(quad).reshape(4, 2))
        assert res.rectify_area == (area if how is True or isinstance(how, aocr.RectifyParams) else None)
        cx, cy = corner_pixels(res.boxes)
        X, Y, _ = R.warp_points(coef, cx, cy)
        assert res.photo_corners.shape == (len(res.boxes), 4, 2) and res.photo_corners.dtype == np.float64
        np.testing.assert_array_equal(res.photo_corners, np.stack([X, Y], 2))
        inside = R.inside_quad(quad, *photo.shape)                                           # every box lies on the paper of the photograph
        pc = np.floor(res.photo_corners + 0.5).astype(np.int64)
        assert inside[pc[:, :, 1], pc[:, :, 0]].all()
    sized = m.recognize_page(photo, params, width=100, rectify=aocr.RectifyParams(width=Wo + 10, height=Ho))
    assert sized.rectified and sized.rectify_size == (Wo + 10, Ho) and sized.n_lines == 3
    with pytest.raises(ValueError):
        m.recognize_page(photo, params, width=100, rectify=[(0, 0), (0, 50), (50, 50), (50, 0)])      # counter-clockwise
    with pytest.raises(ValueError):
        m.recognize_page(photo, params, width=100, rectify=[(0, 0), (50, 0), (50, 50)])

    # a sheet too small to be the page: the photograph is read as it is
    small = m.recognize_page(photo, params, width=100, rectify=aocr.RectifyParams(min_area_percent=99))
    plain = m.recognize_page(photo, params, width=100)
    same_reading(small, plain)
    assert small.rectified is False and small.rectify_size is None and small.rectify_area == area
    cx, cy = corner_pixels(small.boxes)
    np.testing.assert_array_equal(small.photo_corners, np.stack([cx, cy], 2))

    # a page without a desk: one component fills the frame, the quad is the image corners, rectification is a copy
    H, W = page.shape
    filled = page                                                                            # its margins are paper all round
    nodesk = m.recognize_page(filled, params, width=100, rectify=True)
    np.testing.assert_array_equal(nodesk.rectify_quad, [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]])
    assert nodesk.rectified and nodesk.rectify_size == (W, H)
    same_reading(nodesk, m.recognize_page(filled, params, width=100))

    # with deskew and orient the corners start from source_corners: slope 0 and no turn here, so they are the corner pixels again
    both = m.recognize_page(photo, params, width=100, rectify=True, orient=0, deskew=aocr.SkewParams(n_steps=0))
    same_reading(both, base)
    cx, cy = corner_pixels(both.boxes)
    X, Y, _ = R.warp_points(coef, cx, cy)
    np.testing.assert_array_equal(both.photo_corners, np.stack([X, Y], 2))
    turned = m.recognize_page(photo, params, width=100, rectify=True, orient=2)
    cx, cy = corner_pixels(turned.source_boxes)
    X, Y, _ = R.warp_points(coef, cx, cy)
    np.testing.assert_array_equal(turned.photo_corners, np.stack([X, Y], 2))
    print(f"[recognize_page rectify] quad {quad} -> {Wo} x {Ho}, sheet {area} pixels, {len(base.text)} boxes in {base.n_lines} lines")
    m.check_health()
    m.shutdown()
