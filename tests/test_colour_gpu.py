"""GPU: aocr_estimate_page_colour and aocr_gray_page against the numpy restatement (tests/colour_ref.py), through the C ABI and through the
host wrappers, and Model.recognize_page(colour=...) against the call on the reference's gray page.  Everything is exact equality: every
byte of the poisoned output buffer, every one of the sixteen words and the sentinels behind them.  tests/test_colour_cpu.py checks the
restatement itself and the premise of the marked page."""
import ctypes as C

import numpy as np
import pytest
import torch

import colour_ref as K
import segment_ref as R
from colour_cases import (HEIGHTS, MARKED_BOXES, MARKED_DROP, MARKED_SEG, MERGE_SHAPE, OFFSETS, OUTS, PITCH_EXTRA, WIDTHS, all_paper, marked_page,
                          paper_rgb, random_rgb)
from page_harness import expect_placed, garbage_scratch, guarded_words, place, poisoned

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD = 4                # words behind the sixteen that every raw call gets: they must keep their sentinel
POISON = 0xAB
TAIL = 32                # bytes of the gray page's buffer behind the last row's pitch
AROUND = 99              # the bytes around a placed RGB page, where a test does not say otherwise: neither paper nor ink


def _params(**kw):
    import aocr
    return aocr.ColourParams(**kw)


def _gray(cuda, rgb, params, words_in=None, alias=False, counts=True, pitch=None, offset=0, out_extra=0, out_offset=0):
    """raw aocr_gray_page into a poisoned buffer: (the whole buffer, the 16 words and GUARD sentinels or None, status)."""
    import aocr
    H, W, _ = rgb.shape
    dev, addr, pitch = place(cuda, rgb, pitch, offset, fill=AROUND, elem=3)
    out_pitch = W + out_extra
    buf = poisoned(cuda, out_offset + H * out_pitch + TAIL, POISON)
    win = None
    if words_in is not None:
        win = torch.tensor([int(v) for v in words_in] + [SENTINEL] * GUARD, dtype=torch.int32, device=cuda)
    wout = win if alias else (guarded_words(cuda, 16, GUARD, SENTINEL, torch.int32) if counts else None)
    st = aocr.lib.aocr_gray_page(None, C.c_void_p(addr), pitch, H, W, C.byref(params), aocr.ptr(win), aocr.ptr(wout),
                                 C.c_void_p(buf.data_ptr() + out_offset), out_pitch)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), None if wout is None else wout.cpu().numpy(), st


def _expect(gray, out_extra, out_offset):
    return expect_placed(gray, gray.shape[1] + out_extra, out_offset, poison=POISON, tail=TAIL)


_pages = {}


def _random(H, W):
    if (H, W) not in _pages:
        _pages[(H, W)] = random_rgb(H, W, 31 * H + W)
    return _pages[(H, W)]


# the ways a gray call is asked: (params, colour_in_dev words or None, colour_out_dev is colour_in_dev)
VARIANTS = [
    (dict(paper=(250, 240, 200)), None, False),                                                         # paper in params, luma, nothing dropped
    (dict(mode=1, balance=0, drop=1 << K.YELLOW, chroma_min=1, fill=3), None, False),                   # the identity, the darkest channel
    (dict(weights=(256, 0, 0), drop=63, chroma_min=255, fill=0), [200, 180, 255, 1] + [11] * 12, False),   # paper from device words, red channel
    (dict(drop=63, fill=7), [251, 243, 190, 0] + [5] * 12, True),                                       # the words overwritten in place
]


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("H", HEIGHTS)
def test_gray_matches_restatement(cuda, H, W):
    rgb = _random(H, W)
    i = 0
    for offset in OFFSETS:
        for extra in PITCH_EXTRA:
            kw, words_in, alias = VARIANTS[i % len(VARIANTS)]
            out_extra, out_offset = OUTS[(i // len(VARIANTS) + i) % len(OUTS)]
            i += 1
            want, want_words = K.gray_page(rgb, words_in, **{**K.DEFAULTS, **kw})
            buf, words, st = _gray(cuda, rgb, _params(**kw), words_in, alias, True, 3 * W + extra, offset, out_extra, out_offset)
            what = (H, W, offset, extra, kw, out_extra, out_offset)
            assert st == 0, what
            np.testing.assert_array_equal(buf, _expect(want, out_extra, out_offset), err_msg=str(what))
            np.testing.assert_array_equal(words[:16], want_words, err_msg=str(what))
            assert (words[16:] == SENTINEL).all(), what


def test_gray_without_counts_and_twice_on_the_same_words(cuda):
    rgb = _random(70, 342)
    kw = dict(paper=(250, 240, 200), drop=1 << K.RED)
    want, want_words = K.gray_page(rgb, None, **{**K.DEFAULTS, **kw})
    buf, words, st = _gray(cuda, rgb, _params(**kw), counts=False)
    assert st == 0 and words is None
    np.testing.assert_array_equal(buf, _expect(want, 0, 0))
    # overwritten, not accumulated: the output words of one call as the input words of the next give the same counts again
    first = _gray(cuda, rgb, _params(**kw), [250, 240, 200, 1] + [0] * 12, True)[1][:16]
    second = _gray(cuda, rgb, _params(**kw), first, True)[1][:16]
    np.testing.assert_array_equal(first, second)
    np.testing.assert_array_equal(first[4:], want_words[4:])
    assert first[3] == 1 and want_words[4:11].sum() > 0


# ---- aocr_estimate_page_colour -------------------------------------------------------------------------------------------------------------------
def _estimate(cuda, rgb, paper_min=128, pitch=None, offset=0, scratch=None):
    """raw aocr_estimate_page_colour: (the 16 words and GUARD sentinels, status, the scratch tensor); the scratch holds poison."""
    import aocr
    H, W, _ = rgb.shape
    dev, addr, pitch = place(cuda, rgb, pitch, offset, fill=255, elem=3)
    need = aocr.lib.aocr_colour_scratch_bytes(H, W)
    if scratch is None:
        scratch = garbage_scratch(cuda, need, 0)                                      # no floor: exactly the queried size
    out = guarded_words(cuda, 16, GUARD, SENTINEL, torch.int32)
    st = aocr.lib.aocr_estimate_page_colour(None, C.c_void_p(addr), pitch, H, W, C.byref(_params(paper_min=paper_min)), aocr.ptr(scratch),
                                            aocr.ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy(), st, scratch


def _check_estimate(cuda, rgb, paper_min=128, pitch=None, offset=0, what=""):
    want = K.estimate_paper(rgb, paper_min)
    scratch = None
    for _ in range(2):                                                            # twice on the same scratch: the same words
        got, st, scratch = _estimate(cuda, rgb, paper_min, pitch, offset, scratch)
        assert st == 0, what
        np.testing.assert_array_equal(got[:16], want, err_msg=str(what))
        assert (got[16:] == SENTINEL).all(), what
    return want


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("H", HEIGHTS)
def test_estimate_matches_restatement(cuda, H, W):
    for i, (offset, extra) in enumerate((o, e) for o in OFFSETS for e in PITCH_EXTRA):
        rgb = _random(H, W) if i % 2 else paper_rgb(H, W, 31 * H + W + i)
        _check_estimate(cuda, rgb, (128, 1, 200)[i % 3], 3 * W + extra, offset, (H, W, offset, extra))


def test_estimate_special_pages(cuda):
    want = _check_estimate(cuda, all_paper(9, 37), what="constant")
    assert want[:4].tolist() == [252, 242, 202, 1]                                # a constant channel: the windows tie, the largest v
    want = _check_estimate(cuda, paper_rgb(40, 100, 5, low=True), what="below paper_min")
    assert want[:4].tolist() == [255, 255, 255, 1]
    H, W = MERGE_SHAPE
    want = _check_estimate(cuda, paper_rgb(H, W, 300700), pitch=3 * W + 7, offset=5, what="several workgroups")
    assert all(abs(int(v) - t) <= 2 for v, t in zip(want[:3], (250, 240, 200)))
    _check_estimate(cuda, _random(H, W), pitch=3 * W + 1, offset=1, what="several workgroups, noise")


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_everything_untouched(cuda):
    import aocr
    rgb = _random(70, 43)
    H, W, _ = rgb.shape
    dev, addr, pitch = place(cuda, rgb, fill=AROUND, elem=3)
    good = dict(paper=(250, 240, 200))

    def raw(**fields):
        """a ColourParams with fields the constructor would turn down"""
        p = _params(**good)
        for k, v in fields.items():
            if k in ("weights", "paper"):
                for j, x in enumerate(v):
                    getattr(p, k)[j] = x
            else:
                setattr(p, k, v)
        return p

    bad_params = [(raw(weights=(77, 150, 30)), "weights"), (raw(weights=(-1, 228, 29)), "weights"), (raw(mode=2), "mode"), (raw(mode=-1), "mode"),
                  (raw(drop=64), "drop"), (raw(drop=-1), "drop"), (raw(chroma_min=0), "chroma_min"), (raw(chroma_min=256), "chroma_min"),
                  (raw(paper_min=0), "paper_min"), (raw(paper_min=256), "paper_min"), (raw(paper=(0, 240, 200)), "paper"),
                  (raw(paper=(250, 240, 256)), "paper"), (raw(fill=-1), "fill"), (raw(fill=256), "fill")]
    out = poisoned(cuda, H * W + 64, POISON)
    words = torch.full((16,), SENTINEL, dtype=torch.int32, device=cuda)
    scratch = torch.full((aocr.lib.aocr_colour_scratch_bytes(H, W) // 8,), -1, dtype=torch.int64, device=cuda)
    src, ok = C.c_void_p(addr), _params(**good)
    gray_calls = [((None, src, pitch, H, W, C.byref(p), None, aocr.ptr(words), aocr.ptr(out), W), word) for p, word in bad_params] + [
        ((None, None, pitch, H, W, C.byref(ok), None, aocr.ptr(words), aocr.ptr(out), W), "rgb_dev"),
        ((None, src, pitch, H, W, None, None, aocr.ptr(words), aocr.ptr(out), W), "params"),
        ((None, src, pitch, H, W, C.byref(ok), None, aocr.ptr(words), None, W), "out_dev"),
        ((None, src, pitch, H, W, C.byref(_params()), None, aocr.ptr(words), aocr.ptr(out), W), "colour_in_dev"),      # an estimate asked, none given
        ((None, src, 3 * W - 1, H, W, C.byref(ok), None, aocr.ptr(words), aocr.ptr(out), W), "pitch"),
        ((None, src, pitch, H, W, C.byref(ok), None, aocr.ptr(words), aocr.ptr(out), W - 1), "out_pitch"),
        ((None, src, pitch, 0, W, C.byref(ok), None, aocr.ptr(words), aocr.ptr(out), W), "page size"),
        ((None, src, pitch, H, 16385, C.byref(ok), None, aocr.ptr(words), aocr.ptr(out), 16385), "page size"),
        ((None, src, pitch, H, W, C.byref(ok), None, aocr.ptr(words), C.c_void_p(addr + 100), W), "overlaps"),
        ((None, src, pitch, H, W, C.byref(ok), None, C.c_void_p(addr + 8), aocr.ptr(out), W), "overlaps"),
        ((None, src, pitch, H, W, C.byref(ok), None, C.c_void_p(out.data_ptr() + 16), aocr.ptr(out), W), "overlaps"),
    ]
    for args, word in gray_calls:
        assert aocr.lib.aocr_gray_page(*args) != 0 and word in aocr.last_error(), (word, aocr.last_error())
    est_calls = [((None, src, pitch, H, W, C.byref(p), aocr.ptr(scratch), aocr.ptr(words)), word) for p, word in bad_params] + [
        ((None, None, pitch, H, W, C.byref(ok), aocr.ptr(scratch), aocr.ptr(words)), "rgb_dev"),
        ((None, src, pitch, H, W, None, aocr.ptr(scratch), aocr.ptr(words)), "params"),
        ((None, src, pitch, H, W, C.byref(ok), None, aocr.ptr(words)), "scratch_dev"),
        ((None, src, pitch, H, W, C.byref(ok), aocr.ptr(scratch), None), "colour_dev"),
        ((None, src, 3 * W - 1, H, W, C.byref(ok), aocr.ptr(scratch), aocr.ptr(words)), "pitch"),
        ((None, src, pitch, H, 0, C.byref(ok), aocr.ptr(scratch), aocr.ptr(words)), "page size"),
        ((None, src, pitch, H, W, C.byref(ok), aocr.ptr(scratch), C.c_void_p(addr + 8)), "overlaps"),
        ((None, src, pitch, H, W, C.byref(ok), aocr.ptr(scratch), C.c_void_p(scratch.data_ptr() + 64)), "overlaps"),
        ((None, src, pitch, H, W, C.byref(ok), C.c_void_p(addr + 16 - addr % 16), aocr.ptr(words)), "overlaps"),
    ]
    for args, word in est_calls:
        assert aocr.lib.aocr_estimate_page_colour(*args) != 0 and word in aocr.last_error(), (word, aocr.last_error())
    torch.cuda.synchronize()
    assert (out == POISON).all() and (words == SENTINEL).all() and (scratch == -1).all()
    np.testing.assert_array_equal(dev.cpu().numpy()[:H * 3 * W].reshape(H, W, 3), rgb)


# ---- the host wrappers -----------------------------------------------------------------------------------------------------------------------------
def test_host_wrappers_take_a_view_and_chain_on_the_device(cuda, monkeypatch):
    import aocr
    wide = paper_rgb(70, 150, 70150)
    wide[:, :, :][random_rgb(70, 150, 1)[:, :, 0] < 30] = (230, 20, 20)
    wide_dev = torch.from_numpy(wide).to(cuda)
    view, ref = wide_dev[3:64, 7:140], np.ascontiguousarray(wide[3:64, 7:140])
    assert not view.is_contiguous()
    params = aocr.ColourParams(drop=1 << aocr.HUE_RED, fill=200)
    reads = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (reads.append(t.numel()), real_cpu(t, *a, **k))[1])
    words_dev = aocr.estimate_page_colour_device(view, params)
    gray_dev, out_dev = aocr.gray_page_device(view, params, words_dev, counts=True)
    auto_dev = aocr.gray_page_device(view, params)                                 # the estimate enqueued by the wrapper itself
    assert reads == []                                                             # nothing was read back in between
    monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
    want_words = K.estimate_paper(ref)
    want, want_out = K.gray_page(ref, want_words, **{**K.DEFAULTS, "drop": 1 << K.RED, "fill": 200})
    np.testing.assert_array_equal(words_dev.cpu().numpy(), want_words)
    np.testing.assert_array_equal(gray_dev.cpu().numpy(), want)
    np.testing.assert_array_equal(out_dev.cpu().numpy(), want_out)
    np.testing.assert_array_equal(auto_dev.cpu().numpy(), want)
    assert want_out[4 + K.RED] > 0 and want_out[10] == want_out[4 + K.RED]
    np.testing.assert_array_equal(wide_dev.cpu().numpy(), wide)
    with pytest.raises(ValueError):
        aocr.gray_page_device(wide_dev[:, :, 0])
    with pytest.raises(ValueError):
        aocr.gray_page_device(torch.zeros((4, 4, 4), dtype=torch.uint8, device=cuda))


# ---- Model.recognize_page(colour=...) --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(cuda):
    from model_harness import make
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=32, W=100, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    return m


def _same(a, b, skip=()):
    assert sorted(k for k in vars(a) if k not in skip) == sorted(k for k in vars(b) if k not in skip)
    for k, v in vars(a).items():
        if k not in skip:
            assert np.array_equal(v, getattr(b, k)) if isinstance(v, np.ndarray) else v == getattr(b, k), k


COLOUR_FIELDS = ("colour_paper", "colour_balanced", "colour_hues", "colour_dropped")


def test_recognize_page_colour(cuda, model, monkeypatch):
    import aocr
    m = model
    seg = aocr.SegmentParams(**MARKED_SEG)
    rgb = marked_page()
    cp = aocr.ColourParams(drop=MARKED_DROP)
    gray, words = K.gray(rgb, drop=MARKED_DROP)

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
    ref = m.recognize_page(gray, seg, width=100)
    on_gray, reads[:] = list(reads), []
    res = m.recognize_page(rgb, seg, width=100, colour=cp)
    assert len(reads) == len(on_gray) == 2 and reads[0] == on_gray[0] + 16 and reads[1] == on_gray[1], (on_gray, reads)
    monkeypatch.setattr(m, "_page_boxes", real_boxes)

    np.testing.assert_array_equal(ref.boxes, np.array(MARKED_BOXES, np.int32)[:, :4])
    assert ref.n_lines == 2 and not any(hasattr(ref, k) for k in COLOUR_FIELDS)
    _same(ref, res, skip=COLOUR_FIELDS)                                            # boxes, line, ink, labels, scores, text and the rest
    assert res.colour_paper == tuple(int(v) for v in words[:3]) and res.colour_balanced is True
    assert res.colour_hues.dtype == np.int64
    np.testing.assert_array_equal(res.colour_hues, words[4:10])
    assert res.colour_dropped == int(words[10]) > 0
    as_tensor = m.recognize_page(torch.from_numpy(rgb), seg, width=100, colour=cp)  # a tensor is taken like an array
    _same(res, as_tensor)

    luma = m.recognize_page(rgb, seg, width=100, colour=True)                      # nothing dropped: the rule joins the lines
    _same(m.recognize_page(K.gray(rgb)[0], seg, width=100), luma, skip=COLOUR_FIELDS)
    assert luma.colour_dropped == 0 and (luma.n_lines < 2 or len(luma.boxes) < len(MARKED_BOXES))

    # colour=None is the call as it was
    _same(ref, m.recognize_page(gray, seg, width=100, colour=None))
    for off in (None, False):
        with pytest.raises(ValueError, match="colour pages are out of scope"):
            m.recognize_page(rgb, seg, width=100, colour=off)
    for bad in (gray, np.zeros((60, 120, 4), np.uint8), rgb.astype(np.float32), torch.zeros((60, 120), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            m.recognize_page(bad, seg, width=100, colour=True)
    with pytest.raises(ValueError):
        m.recognize_page(rgb, seg, width=100, colour="red")


def test_recognize_page_colour_composes_and_reads_an_empty_page(cuda, model):
    import aocr
    m = model
    seg = aocr.SegmentParams(**MARKED_SEG)
    rgb = marked_page()
    cp = aocr.ColourParams(drop=MARKED_DROP)
    gray, _ = K.gray(rgb, drop=MARKED_DROP)
    corners = [(1, 1), (118, 2), (117, 58), (2, 57)]
    kw = dict(width=100, rectify=corners, deskew=True)
    _same(m.recognize_page(gray, seg, **kw), m.recognize_page(rgb, seg, colour=cp, **kw), skip=COLOUR_FIELDS)

    empty = m.recognize_page(all_paper(), seg, width=100, colour=True)
    assert empty.boxes.shape == (0, 4) and empty.text == [] and empty.n_found == 0
    assert empty.colour_hues.tolist() == [0] * 6 and empty.colour_dropped == 0 and empty.colour_paper == (252, 242, 202)
    light = m.recognize_page(255 - all_paper(), aocr.SegmentParams(**{**MARKED_SEG, "light_text": 1}), width=100, colour=True)
    assert light.colour_paper == (255, 255, 255) and light.colour_balanced is False and light.boxes.shape == (0, 4)
