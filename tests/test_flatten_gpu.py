"""GPU: aocr_flatten_page against the numpy restatement (tests/flatten_ref.py), and Model.recognize_page(flatten=...).  Every comparison is
exact byte equality, of the whole output buffer: the flattened page, and the guard pattern everywhere else.  tests/test_flatten_cpu.py shows
on the restatement alone that the lit pages used here cannot be segmented before flattening and can after it."""
import ctypes as C

import numpy as np
import pytest
import torch

import flatten_ref as F
import segment_ref as R
import skew_ref as S
from flatten_cases import CASES, clean_page, light, lit_page
from page_harness import csrc_constants, expect_placed, garbage_scratch, place, poisoned
from segment_cases import SEEDED_SHAPES, seeded_page

pytestmark = pytest.mark.gpu

POISON = 0xAB
AROUND = 99              # the bytes around every placed page: neither paper nor ink
TAIL = 32                # bytes of the output buffer behind the last row's pitch


def _flatten(cuda, page, radius, light_text=0, pitch=None, offset=0, out_pitch=None, out_offset=0, shape=None, reserved=(0, 0), scratch=True):
    """raw aocr_flatten_page into a poisoned buffer over garbage scratch: (the whole output buffer as the device left it, status)."""
    import aocr
    H, W = shape or page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=AROUND)
    out_pitch = out_pitch or page.shape[1]
    buf = poisoned(cuda, out_offset + page.shape[0] * out_pitch + TAIL, POISON)
    p = aocr.FlattenParams(radius, light_text)
    p.reserved[0], p.reserved[1] = reserved
    need = aocr.lib.aocr_flatten_scratch_bytes(H, W, radius)
    sc = garbage_scratch(cuda, need, 1 << 12)
    st = aocr.lib.aocr_flatten_page(None, C.c_void_p(addr), pitch, H, W, C.byref(p), aocr.ptr(sc) if scratch else None,
                                    C.c_void_p(buf.data_ptr() + out_offset), out_pitch)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st


def _expect(want, out_pitch=None, out_offset=0):
    return expect_placed(want, out_pitch, out_offset, poison=POISON, tail=TAIL)


def _tiling():
    """the tile sizes of csrc/flatten.hip."""
    return csrc_constants("flatten.hip", ("HSEG", "HROWS", "VT_COLS", "VT_ROWS", "VS_WORDS", "VS_ROWS"))


@pytest.mark.parametrize("light_text", [0, 1], ids=["dark", "light"])
@pytest.mark.parametrize("shape", SEEDED_SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SEEDED_SHAPES])
def test_seeded_pages_match_restatement(cuda, shape, light_text):
    """a seeded page under a lighting gradient; the output at an odd offset with a pitch > W: every byte around the page keeps its poison."""
    H, W, pitch, offset, seed = shape
    page = light(seeded_page(H, W, seed), 110)
    if light_text:
        page = (255 - page).astype(np.uint8)
    for r in (1, 3, 16) + ((127,) if H * W <= 40 * 100 else ()):
        want = F.flatten(page, r, light_text)
        for out_pitch, out_offset in ((W, 0), (W + 7, 5)):
            got, st = _flatten(cuda, page, r, light_text, pitch, offset, out_pitch, out_offset)
            assert st == 0
            np.testing.assert_array_equal(got, _expect(want, out_pitch, out_offset), err_msg=str((shape, r, light_text, out_pitch)))
    if H >= 40:
        assert len(np.unique(want)) > 50 and not np.array_equal(want, page)     # the page really changed


@pytest.mark.parametrize("shape", [(8, 4100), (4100, 8)], ids=["wide", "tall"])
def test_long_axis_pages_cross_every_seam(cuda, shape):
    H, W = shape
    t = _tiling()
    assert len(t) == 6
    if W > H:      # more than one segment of the row kernels, one tile of the column max, one workgroup of the column sum
        assert W > 4 * t["HSEG"] and W > t["VT_COLS"] and W > 4 * t["VS_WORDS"]
    else:          # more than one workgroup of rows in every kernel, and more than one band per thread column
        assert H > t["HROWS"] and H > t["VT_ROWS"] and H > 4 * t["VS_ROWS"]
    page = light(seeded_page(H, W, 4100 + H), 110)
    got, st = _flatten(cuda, page, 16, 0, W + 3, 1, W + 9, 3)
    assert st == 0
    np.testing.assert_array_equal(got, _expect(F.flatten(page, 16), W + 9, 3))


def test_hand_cases_determinism_and_identity(cuda):
    for name, page, r, light_text, want in CASES:
        got, st = _flatten(cuda, page, r, light_text)
        assert st == 0
        np.testing.assert_array_equal(got, _expect(want), err_msg=name)
    _, lit = lit_page(110)
    a, st = _flatten(cuda, lit, 16)
    assert st == 0
    np.testing.assert_array_equal(a, _expect(F.flatten(lit, 16)))
    for pitch, offset in ((None, 0), (837, 5), (1024, 16)):                     # two calls, three pitches
        b, st = _flatten(cuda, lit, 16, 0, pitch, offset)
        assert st == 0 and np.array_equal(a, b)
    clean = clean_page()
    got, st = _flatten(cuda, clean, 16)
    assert st == 0 and np.array_equal(got, _expect(clean))


def test_invalid_arguments_leave_the_output_untouched(cuda):
    import aocr
    page = light(seeded_page(40, 100, 3), 110)
    for kw, word in ((dict(radius=0), "radius"), (dict(radius=128), "radius"), (dict(radius=16, reserved=(1, 0)), "reserved"),
                     (dict(radius=16, reserved=(0, -1)), "reserved"), (dict(radius=16, shape=(0, 100)), "page size"),
                     (dict(radius=16, shape=(40, 101)), "pitch"), (dict(radius=16, shape=(16384, 4097), pitch=100), "page size"),
                     (dict(radius=16, scratch=False), "NULL"), (dict(radius=16, out_pitch=99), "out_pitch")):
        got, st = _flatten(cuda, page, **kw)
        assert st != 0 and word in aocr.last_error(), (kw, aocr.last_error())
        assert (got == POISON).all(), kw
    dev, addr, pitch = place(cuda, page, fill=AROUND)
    p = aocr.FlattenParams()
    sc = torch.empty(1 << 14, dtype=torch.int64, device=cuda)
    for out in (addr + 50, addr - 50, addr):                                    # an output that overlaps the page
        assert aocr.lib.aocr_flatten_page(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), aocr.ptr(sc), C.c_void_p(out), 100) != 0
        assert "overlap" in aocr.last_error()
    assert aocr.lib.aocr_flatten_page(None, C.c_void_p(addr), pitch, 40, 100, None, aocr.ptr(sc), C.c_void_p(addr + 8000), 100) != 0
    assert aocr.lib.aocr_flatten_page(None, C.c_void_p(addr), pitch, 40, 100, C.byref(p), aocr.ptr(sc), None, 100) != 0
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy()[:4000].reshape(40, 100), page)
    for H, W, r in ((0, 10, 16), (10, 0, 16), (16385, 10, 16), (16384, 4097, 16), (10, 10, 0), (10, 10, 128), (10, 10, -1)):
        assert aocr.lib.aocr_flatten_scratch_bytes(H, W, r) == 0 and "bad sizes" in aocr.last_error()
    assert aocr.lib.aocr_flatten_scratch_bytes(16384, 4096, 127) > 0


def test_python_surface_on_a_view(cuda):
    import aocr
    _, lit = lit_page(110)
    H, W = lit.shape
    big = torch.zeros((H + 9, W + 30), dtype=torch.uint8, device=cuda)
    big[4:4 + H, 11:11 + W] = torch.from_numpy(lit).to(cuda)
    view = big[4:4 + H, 11:11 + W]
    assert not view.is_contiguous()
    out = aocr.flatten_page_device(view)                                        # the defaults: radius 16, dark text
    assert out.shape == (H, W) and out.is_contiguous() and out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), F.flatten(lit, 16))
    out4 = aocr.page.flatten_page_device(view, aocr.FlattenParams(radius=4))
    assert np.array_equal(out4.cpu().numpy(), F.flatten(lit, 4))
    inv = aocr.flatten_page_device(255 - view, aocr.FlattenParams(light_text=1))
    assert np.array_equal(inv.cpu().numpy(), 255 - F.flatten(lit, 16))
    assert np.array_equal(big.cpu().numpy()[4:4 + H, 11:11 + W], lit)
    with pytest.raises(aocr.AocrError):
        aocr.flatten_page_device(view, aocr.FlattenParams(radius=200))


def test_recognize_page_flatten(cuda):
    import aocr
    from model_harness import make
    B = 32
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=100, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    straight, lit = lit_page(110)
    want, want_counts = R.segment_page(straight)
    assert want_counts[0] == 109 and want_counts[1] == 15

    res = m.recognize_page(lit, width=100, flatten=True)
    assert res.n_lines == 15 and res.n_found == 109 and res.flatten_radius == 16
    np.testing.assert_array_equal(res.boxes, want[:, :4])
    np.testing.assert_array_equal(res.line, want[:, 4])
    res4 = m.recognize_page(lit, width=100, flatten=aocr.FlattenParams(radius=4))
    assert res4.flatten_radius == 4 and res4.n_lines == 15
    np.testing.assert_array_equal(res4.boxes, want[:, :4])
    plain = m.recognize_page(lit, width=100)                                    # one threshold: the dim half of the paper is all ink
    assert plain.n_lines == 1 and not hasattr(plain, "flatten_radius")
    assert sorted(vars(plain)) == sorted(vars(m.recognize_page(lit, width=100, flatten=False)))

    a = m.recognize_page(straight, width=100, flatten=True)                     # a clean page comes back bit for bit
    b = m.recognize_page(straight, width=100, flatten=None)
    np.testing.assert_array_equal(a.boxes, b.boxes)
    np.testing.assert_array_equal(a.labels, b.labels)
    assert a.text == b.text and a.n_lines == 15

    _, lit_skewed = lit_page(110, 17)
    ref_skew, _ = S.estimate_skew(F.flatten(lit_skewed, 16))
    assert ref_skew[0] == 17
    both = m.recognize_page(lit_skewed, width=100, flatten=True, deskew=True)
    assert (both.skew_steps, both.skew_slope_q16) == (17, 17 * 64) and both.flatten_radius == 16
    flat, flat_counts = R.segment_page(S.deskew(F.flatten(lit_skewed, 16), 17 * 64, 255))
    assert both.n_lines == flat_counts[1] == 15
    np.testing.assert_array_equal(both.boxes, flat[:, :4])
    light_res = m.recognize_page(255 - lit, aocr.SegmentParams(light_text=1), width=100, flatten=True)
    assert light_res.n_lines == 15
    np.testing.assert_array_equal(light_res.boxes, want[:, :4])
    print(f"[recognize_page flatten] {res.n_found} boxes in {res.n_lines} lines, threshold {res.threshold}; without: {plain.n_found} in {plain.n_lines}")
    m.check_health()
    m.shutdown()
