"""GPU: aocr_estimate_slant and aocr_crop_lines_slanted against the restatement (tests/slant_ref.py), and Model.recognize_page(deslant=...)
against the pieces it is made of.  Everything is exact equality: every word of slant_dev and scores_dev and of the poison around them,
every float of the crops.  tests/test_slant_cpu.py shows on the restatement alone that planted slants are found.
The estimate's column chunk is 256 profile columns (SLANT_CHUNK in csrc/slant.hip): the seeded page's widest boxes have 1150 and 700
columns, above twice that."""
import ctypes as C

import numpy as np
import pytest
import torch

import slant_ref as R
from page_harness import garbage_scratch, guarded_words, place
from slant_cases import DEFAULTS, PLANTED_K, STROKE, bar_page, bar_word, seeded_page, stroke_5x7

pytestmark = pytest.mark.gpu

CHUNK = 256
SENTINEL = -7
GUARD = 3                # rows beyond n_boxes that every raw call's outputs get: they must keep their sentinel


def _estimate(cuda, page, boxes, params, count=None, word=None, pitch=None, offset=0, scores=True, shape=None, n_boxes=None):
    """raw aocr_estimate_slant over poison: (slant (n + GUARD, 4), scores (n + GUARD, 2K + 1), status).  count: the device word count_dev[0]
    (None: count_dev = NULL); word: the device word threshold_dev[0] (None: threshold_dev = NULL); the scratch holds garbage."""
    import aocr
    H, W = shape or page.shape
    dev, addr, placed = place(cuda, page, max(pitch or 0, page.shape[1]), offset, fill=131)      # `pitch` below the page's width is only passed on
    pitch = pitch or placed
    p = aocr.SlantParams(**{k: v for k, v in params.items() if k != "reserved"})
    if "reserved" in params:
        p.reserved[2] = params["reserved"]
    bx = torch.from_numpy(np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 6))).to(cuda)
    n = len(bx) if n_boxes is None else n_boxes
    K = min(max(p.n_steps, 0), 64)
    need = aocr.lib.aocr_slant_scratch_bytes(min(max(n, 0), 65535), K)
    scratch = garbage_scratch(cuda, need, 1 << 12)
    sl = guarded_words(cuda, max(n, 0), GUARD, SENTINEL, torch.int32, width=4)
    sc = guarded_words(cuda, max(n, 0), GUARD, SENTINEL, torch.int64, width=2 * K + 1)
    cnt = torch.tensor([count, 9, 9, 9], dtype=torch.int32, device=cuda) if count is not None else None
    thr = torch.tensor([word], dtype=torch.int32, device=cuda) if word is not None else None
    st = aocr.lib.aocr_estimate_slant(None, C.c_void_p(addr), pitch, H, W, aocr.ptr(bx), aocr.ptr(cnt), n, C.byref(p), aocr.ptr(thr),
                                      aocr.ptr(scratch), aocr.ptr(sl), aocr.ptr(sc) if scores else None)
    torch.cuda.synchronize()
    return sl.cpu().numpy(), sc.cpu().numpy(), st


def _expect(page, boxes, n, params, threshold=None):
    """the whole of both buffers: the restatement's rows, then sentinels"""
    p = dict(params)
    if threshold is not None:
        p["threshold"] = threshold
    ref_sl, ref_sc = R.estimate_slant(page, boxes, n, **p)
    rows, K = len(boxes) + GUARD, p["n_steps"]
    sl = np.full((rows, 4), SENTINEL, np.int32)
    sc = np.full((rows, 2 * K + 1), SENTINEL, np.int64)
    sl[:n], sc[:n] = ref_sl, ref_sc.view(np.int64)
    return sl, sc


def _check(got, want, what):
    sl, sc, st = got
    assert st == 0, what
    np.testing.assert_array_equal(sl, want[0], err_msg=str(what))
    np.testing.assert_array_equal(sc, want[1], err_msg=str(what))


def test_hand_cases(cuda):
    for right in (True, False):
        page = stroke_5x7(right)
        got = _estimate(cuda, page, [(0, 0, 7, 5, 0, 0)], STROKE, pitch=9, offset=1)
        _check(got, _expect(page, [(0, 0, 7, 5, 0, 0)], 1, STROKE), right)
        assert got[0][0].tolist() == [7 if right else -7, 57344 if right else -57344, 0, 5]
    page, boxes, ks = bar_page()
    got = _estimate(cuda, page, boxes, DEFAULTS)
    _check(got, _expect(page, boxes, len(boxes), DEFAULTS), "bars")
    assert got[0][:len(ks), 0].tolist() == list(PLANTED_K)
    blank = np.full((20, 30), 255, np.uint8)
    dot = blank.copy()
    dot[7, 11] = 0
    for page, ink in ((blank, 0), (dot, 1)):
        got = _estimate(cuda, page, [(2, 2, 28, 18, 0, 0)], DEFAULTS, pitch=37, offset=3)
        _check(got, _expect(page, [(2, 2, 28, 18, 0, 0)], 1, DEFAULTS), ink)
        assert got[0][0].tolist() == [0, 0, 0, ink]


SETTINGS = [
    ("defaults", DEFAULTS, {}),
    ("odd_base", DEFAULTS, dict(pitch=1311, offset=3)),
    ("light_text", dict(DEFAULTS, light_text=1, threshold=100), dict(pitch=1301, offset=1)),
    ("K0", dict(DEFAULTS, n_steps=0), {}),
    ("K64", dict(DEFAULTS, n_steps=64, step_q16=1024), dict(pitch=1305, offset=5)),
    ("K8_45deg", dict(DEFAULTS, n_steps=8, step_q16=8192), {}),
    ("device_word", dict(DEFAULTS, threshold=-1), dict(word=77)),
    ("device_word_none", dict(DEFAULTS, threshold=-1, light_text=1), dict(word=-1)),
    ("fixed_beats_word", DEFAULTS, dict(word=3)),
]


@pytest.mark.parametrize("name,params,how", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_seeded_page_matches_restatement(cuda, name, params, how):
    page, boxes = seeded_page()
    n = len(boxes)
    assert page.shape == (300, 1300) and 40 <= n <= 50 and max(int(b[2] - b[0]) for b in boxes[8:10]) > 2 * CHUNK
    thr = how["word"] if params["threshold"] < 0 else None
    want = _expect(page, boxes, n, params, thr)
    _check(_estimate(cuda, page, boxes, params, **how), want, name)
    flags = want[0][:n, 2]
    assert (flags == 1).sum() == 3 and (flags == 2).sum() == 2
    if name == "defaults":
        assert want[0][16:19, 0].tolist() == [7, -11, 2]                               # the bar words planted in the noise
        # count_dev: above n_boxes, below it (the rows beyond keep their sentinel), zero and negative; n_boxes below the rows
        _check(_estimate(cuda, page, boxes, params, count=n + 9), want, "count above")
        for count in (20, 1, 0, -4):
            _check(_estimate(cuda, page, boxes, params, count=count), _expect(page, boxes, max(count, 0), params), count)
        _check(_estimate(cuda, page, boxes[:12], params, count=30), _expect(page, boxes[:12], 12, params), "n_boxes below count")
        sl, sc, st = _estimate(cuda, page, boxes, params, scores=False)                # scores_dev = NULL: the same slants
        assert st == 0 and np.array_equal(sl, want[0]) and (sc == SENTINEL).all()
        sl, sc, st = _estimate(cuda, page, boxes, params, n_boxes=0)                   # n_boxes = 0: a no-op
        assert st == 0 and (sl == SENTINEL).all() and (sc == SENTINEL).all()
    if name == "device_word_none":
        assert not want[0][:n, 3].any() and not want[1][:n].any()


# ---- aocr_crop_lines_slanted ----------------------------------------------------------------------------------------------------------------
CROP_BOXES = [
    (0, 0, 100, 32), (5, 3, 41, 35), (10, 10, 30, 20), (0, 0, 128, 64), (3, 1, 120, 9), (60, 2, 70, 62), (7, 5, 60, 6), (9, 2, 10, 50), (4, 4, 5, 5),
    (-5, -3, 40, 20), (100, 50, 140, 80), (200, 10, 230, 40), (50, 20, 40, 10), (2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1),
]
CROP_SLANTS = [28672, -45056, 65536, 4096, -65536, 12288, 30000, 65536, -20000, -8192, 49152, 4096, 4096, 4096]
_crop_ref = {}


def _crop_setup(cuda):
    rng = np.random.default_rng(64128)
    page = rng.integers(0, 256, size=(64, 128), dtype=np.uint8)
    bx = np.zeros((len(CROP_BOXES), 6), np.int32)
    bx[:, :4] = np.array(CROP_BOXES, np.int64).astype(np.int32)
    return page, bx


def _crop_reference(cuda, page, slants, fill, out_w):
    """aocr_preprocess_lines on slant_view built on the host; paper for the empty boxes.  Computed once per setting."""
    from aocr.data import preprocess_batch
    key = (tuple(slants), fill, out_w)
    if key not in _crop_ref:
        ref = torch.full((len(CROP_BOXES), 1, 32, out_w), 255.0, dtype=torch.float32, device=cuda)
        views = [R.slant_view(page, b, s, fill) for b, s in zip(CROP_BOXES, slants)]
        rows = [i for i, v in enumerate(views) if v is not None]
        ref[rows] = preprocess_batch([np.ascontiguousarray(views[i]) for i in rows], out_w, cuda)
        assert len(rows) == len(CROP_BOXES) - 3
        _crop_ref[key] = ref.cpu().numpy()
    return _crop_ref[key]


def _crop(cuda, page, bx, slants, fill, out_w, pitch=None, offset=0, count=None, n_boxes=None, plain=False):
    import aocr
    n = len(bx)
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=99)
    boxes = torch.from_numpy(bx).to(cuda)
    out = torch.full((n, 1, 32, out_w), float(SENTINEL), dtype=torch.float32, device=cuda)
    cnt = torch.tensor([count, 0, 0, 0], dtype=torch.int32, device=cuda) if count is not None else None
    sl = None
    if slants is not None:
        words = np.full((n, 4), 12345, np.int32)                                       # only word 1 of a row is read
        words[:, 1] = slants
        sl = torch.from_numpy(words).to(cuda)
    nb = n if n_boxes is None else n_boxes
    if plain:
        st = aocr.lib.aocr_crop_lines(None, C.c_void_p(addr), pitch, 64, 128, aocr.ptr(boxes), aocr.ptr(cnt), nb, 32, out_w, aocr.ptr(out))
    else:
        st = aocr.lib.aocr_crop_lines_slanted(None, C.c_void_p(addr), pitch, 64, 128, aocr.ptr(boxes), aocr.ptr(cnt), nb, aocr.ptr(sl), fill, 32, out_w,
                                              aocr.ptr(out))
    torch.cuda.synchronize()
    assert st == 0, aocr.last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("out_w", [100, 32])
def test_slanted_crops_equal_preprocess_lines_on_the_view(cuda, out_w):
    page, bx = _crop_setup(cuda)
    n = len(bx)
    for (pitch, offset), fill in (((128, 0), 255), ((141, 3), 0), ((141, 3), 77)):
        ref = _crop_reference(cuda, page, CROP_SLANTS, fill, out_w)
        np.testing.assert_array_equal(_crop(cuda, page, bx, CROP_SLANTS, fill, out_w, pitch, offset), ref)
        np.testing.assert_array_equal(_crop(cuda, page, bx, CROP_SLANTS, fill, out_w, pitch, offset, count=n + 5), ref)
        part = _crop(cuda, page, bx, CROP_SLANTS, fill, out_w, pitch, offset, count=5)
        np.testing.assert_array_equal(part[:5], ref[:5])
        assert (part[5:] == SENTINEL).all()
    assert (_crop(cuda, page, bx, CROP_SLANTS, 255, out_w, count=0) == SENTINEL).all()
    assert (_crop(cuda, page, bx, CROP_SLANTS, 255, out_w, count=-3) == SENTINEL).all()
    assert (_crop(cuda, page, bx, CROP_SLANTS, 255, out_w, n_boxes=0) == SENTINEL).all()
    few = _crop(cuda, page, bx, CROP_SLANTS, 255, out_w, n_boxes=3)
    ref = _crop_reference(cuda, page, CROP_SLANTS, 255, out_w)
    np.testing.assert_array_equal(few[:3], ref[:3])
    assert (few[3:] == SENTINEL).all()
    assert (ref[11:] == 255.0).all() and not (ref[9] == 255.0).all()
    # slants beyond +-65536 are clamped
    beyond = [70000, -10 ** 6, 2 ** 31 - 1, -2 ** 31] * 4
    clamped = [65536, -65536, 65536, -65536] * 4
    np.testing.assert_array_equal(_crop(cuda, page, bx, beyond[:n], 9, out_w), _crop_reference(cuda, page, clamped[:n], 9, out_w))


@pytest.mark.parametrize("out_w", [100, 32])
def test_no_slant_is_the_plain_crop(cuda, out_w):
    page, bx = _crop_setup(cuda)
    for pitch, offset in ((128, 0), (141, 3)):
        plain = _crop(cuda, page, bx, None, 0, out_w, pitch, offset, plain=True)
        np.testing.assert_array_equal(_crop(cuda, page, bx, None, 7, out_w, pitch, offset), plain)              # slant_dev = NULL
        np.testing.assert_array_equal(_crop(cuda, page, bx, [0] * len(bx), 7, out_w, pitch, offset), plain)     # every s = 0
    assert not (plain == SENTINEL).any()


def test_invalid_arguments_leave_the_outputs_untouched(cuda):
    import aocr
    page, boxes = seeded_page()
    boxes = boxes[:6]
    for bad, word in ((dict(threshold=255), "threshold"), (dict(threshold=-2), "threshold"), (dict(step_q16=0), "step_q16"),
                      (dict(step_q16=8193), "step_q16"), (dict(n_steps=-1), "n_steps"), (dict(n_steps=65), "n_steps"),
                      (dict(n_steps=17), "n_steps"), (dict(reserved=1), "reserved"), (dict(threshold=-1), "threshold_dev")):
        sl, sc, st = _estimate(cuda, page, boxes, dict(DEFAULTS, **bad))
        assert st != 0 and word in aocr.last_error(), (bad, aocr.last_error())
        assert (sl == SENTINEL).all() and (sc == SENTINEL).all(), bad
    for H, W, pit, word in ((0, 100, 100, "page size"), (40, 0, 100, "page size"), (16385, 100, 100, "page size"), (40, 16385, 16385, "page size"),
                            (16384, 4097, 4097, "page size"), (300, 1300, 1299, "pitch")):
        sl, sc, st = _estimate(cuda, page, boxes, DEFAULTS, pitch=pit, shape=(H, W))
        assert st != 0 and word in aocr.last_error(), (H, W, pit, aocr.last_error())
        assert (sl == SENTINEL).all() and (sc == SENTINEL).all()
    for nb in (-1, 65536):
        sl, sc, st = _estimate(cuda, page, boxes, DEFAULTS, n_boxes=nb)
        assert st != 0 and "n_boxes" in aocr.last_error() and (sl == SENTINEL).all() and (sc == SENTINEL).all()
    dev, addr, pitch = place(cuda, page)
    p = aocr.SlantParams(**DEFAULTS)
    bx = torch.from_numpy(np.ascontiguousarray(boxes)).to(cuda)
    scratch = torch.empty(1 << 12, dtype=torch.int64, device=cuda)
    sl = torch.full((6, 4), SENTINEL, dtype=torch.int32, device=cuda)
    out = torch.full((6, 1, 32, 40), float(SENTINEL), dtype=torch.float32, device=cuda)
    call, pg = aocr.lib.aocr_estimate_slant, C.c_void_p(addr)
    for args, word in (((None, pitch, 300, 1300, aocr.ptr(bx), None, 6, C.byref(p), None, aocr.ptr(scratch), aocr.ptr(sl), None), "page_dev"),
                       ((pg, pitch, 300, 1300, None, None, 6, C.byref(p), None, aocr.ptr(scratch), aocr.ptr(sl), None), "boxes_dev"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, None, None, aocr.ptr(scratch), aocr.ptr(sl), None), "params"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, C.byref(p), None, None, aocr.ptr(sl), None), "NULL"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, C.byref(p), None, aocr.ptr(scratch), None, None), "slant_dev"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, C.byref(p), None, aocr.ptr(scratch), C.c_void_p(addr + 48), None), "overlap"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, C.byref(p), None, aocr.ptr(scratch), aocr.ptr(sl), C.c_void_p(addr + 64)), "overlap")):
        assert call(None, *args) != 0 and word in aocr.last_error(), (word, aocr.last_error())
    crop = aocr.lib.aocr_crop_lines_slanted
    for args, word in (((None, pitch, 300, 1300, aocr.ptr(bx), None, 6, aocr.ptr(sl), 255, 32, 40, aocr.ptr(out)), "page_dev"),
                       ((pg, 1299, 300, 1300, aocr.ptr(bx), None, 6, aocr.ptr(sl), 255, 32, 40, aocr.ptr(out)), "pitch"),
                       ((pg, pitch, 300, 1300, None, None, 6, aocr.ptr(sl), 255, 32, 40, aocr.ptr(out)), "boxes_dev"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, aocr.ptr(sl), 255, 32, 40, None), "out_dev"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, aocr.ptr(sl), 256, 32, 40, aocr.ptr(out)), "fill"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, aocr.ptr(sl), -1, 32, 40, aocr.ptr(out)), "fill"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 65536, aocr.ptr(sl), 255, 32, 40, aocr.ptr(out)), "n_boxes"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, aocr.ptr(sl), 255, 0, 40, aocr.ptr(out)), "out_h"),
                       ((pg, pitch, 300, 1300, aocr.ptr(bx), None, 6, aocr.ptr(sl), 255, 32, 0, aocr.ptr(out)), "out_w")):
        assert crop(None, *args) != 0 and word in aocr.last_error(), (word, aocr.last_error())
    torch.cuda.synchronize()
    assert (sl == SENTINEL).all() and (out == SENTINEL).all()
    assert np.array_equal(dev.cpu().numpy()[:300 * 1300].reshape(300, 1300), page)


def test_python_surface_on_a_view(cuda):
    """estimate_slant_device and crop_lines_slanted_device on a non-contiguous view; the slants go from one to the other on the device."""
    import aocr
    page, boxes, ks = bar_page()
    H, W = page.shape
    big = torch.full((H + 9, W + 30), 255, dtype=torch.uint8, device=cuda)
    big[4:4 + H, 11:11 + W] = torch.from_numpy(page).to(cuda)
    view = big[4:4 + H, 11:11 + W]
    assert not view.is_contiguous()
    bx = torch.from_numpy(boxes).to(cuda)
    n = len(boxes)
    counts = torch.tensor([n - 1, 1, 128, 0], dtype=torch.int32, device=cuda)
    ref_sl, ref_sc = R.estimate_slant(page, boxes, n, **DEFAULTS)
    slant, scores = aocr.estimate_slant_device(view, bx, None, aocr.SlantParams(**DEFAULTS), scores=True)
    assert slant.shape == (n, 4) and scores.shape == (n, 25)
    assert np.array_equal(slant.cpu().numpy(), ref_sl) and np.array_equal(scores.cpu().numpy().view(np.uint64), ref_sc)
    d = aocr.estimate_slant_device(view, bx, counts)                                   # the defaults: the threshold is counts[2] on the device
    assert np.array_equal(d[:n - 1].cpu().numpy(), ref_sl[:n - 1]) and not d[n - 1].any()
    w = aocr.estimate_slant_device(view, bx, counts, threshold_dev=torch.tensor([-1], dtype=torch.int32, device=cuda))
    assert not w[:, [0, 1, 3]].any()
    with pytest.raises(ValueError):
        aocr.estimate_slant_device(view, bx, None)
    crops = aocr.crop_lines_slanted_device(view, bx, None, slant, 64)
    assert crops.shape == (n, 1, 32, 64)
    from aocr.data import preprocess_batch
    want = preprocess_batch([R.slant_view(page, b, s, 255) for b, s in zip(boxes, ref_sl[:, 1])], 64, cuda)
    assert torch.equal(crops, want)
    assert torch.equal(aocr.crop_lines_slanted_device(view, bx, None, None, 64), aocr.crop_lines_device(view, bx, None, 64))
    part = aocr.crop_lines_slanted_device(view, bx, counts, slant, 64, fill=0)
    assert (part[n - 1] == 255.0).all() and torch.equal(part[0], preprocess_batch([R.slant_view(page, boxes[0], ref_sl[0, 1], 0)], 64, cuda)[0])
    with pytest.raises(AssertionError):
        aocr.crop_lines_slanted_device(view, bx, None, slant[:2], 64)
    empty = aocr.estimate_slant_device(view, bx[:0], None, aocr.SlantParams(**DEFAULTS), scores=True)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 25) and aocr.crop_lines_slanted_device(view, bx[:0], None, empty[0], 64).shape == (0, 1, 32, 64)


# ---- Model.recognize_page(deslant=...) -------------------------------------------------------------------------------------------------------
def _word_page():
    """two text lines of bar words leaning by known candidates, in two columns with a gutter of 90 columns: (page, the planted k in reading
    order of the one-column path)"""
    ks = [[6, -9, 3], [-4, 11, 0]]
    rows = []
    for line in ks:
        words = [bar_word(k)[0] for k in line]
        gap = np.full((words[0].shape[0], 90), 255, np.uint8)
        rows.append(np.concatenate([words[0], words[1], gap, words[2]], axis=1))
    W = max(r.shape[1] for r in rows)
    rows = [np.concatenate([r, np.full((r.shape[0], W - r.shape[1]), 255, np.uint8)], axis=1) for r in rows]
    margin = np.full((20, W), 255, np.uint8)
    return np.concatenate([margin, rows[0], margin, rows[1], margin], axis=0), [k for line in ks for k in line]


def test_recognize_page_deslant(cuda, monkeypatch):
    import aocr
    from model_harness import make
    B = 32
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=100, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    page, planted = _word_page()
    params = aocr.SegmentParams(threshold=128)
    page_dev = torch.from_numpy(page).to(cuda)
    plain = m.recognize_page(page, params)
    assert len(plain.boxes) == 6 and plain.n_lines == 2

    def check(res, deslant_params):
        n = len(res.boxes)
        rows = np.concatenate([res.boxes, np.zeros((n, 2), np.int32)], axis=1)
        ref_sl, _ = R.estimate_slant(page, rows, n, **deslant_params)
        np.testing.assert_array_equal(res.slant_q16, ref_sl[:, 1])
        np.testing.assert_array_equal(res.slant_flags, ref_sl[:, 2])
        np.testing.assert_array_equal(res.slant_extent, R.slant_extent(rows, ref_sl[:, 1]))
        assert res.slant_q16.dtype == res.slant_flags.dtype == res.slant_extent.dtype == np.int32 and res.slant_deg.dtype == np.float64
        np.testing.assert_array_equal(res.slant_deg, np.degrees(np.arctan(ref_sl[:, 1] / 65536.0)))
        want_w = [aocr.page.bucket_width(int(b[2] - b[0]) + 2 * int(d), int(b[3] - b[1]), m.max_img_w, 32) for b, d in zip(res.boxes, res.slant_extent)]
        assert res.widths.tolist() == want_w
        boxes_dev, slant_dev = torch.from_numpy(rows).to(cuda), torch.from_numpy(ref_sl).to(cuda)
        for w in sorted(set(want_w)):
            idx = np.flatnonzero(np.array(want_w) == w)
            sel = torch.from_numpy(idx).to(cuda)
            ref = m.recognize(aocr.crop_lines_slanted_device(page_dev, boxes_dev[sel], None, slant_dev[sel], w, fill=255))
            np.testing.assert_array_equal(res.labels[idx], ref.labels)
            np.testing.assert_array_equal(res.scores[idx], ref.scores)
            assert [res.text[i] for i in idx] == ref.text
        return ref_sl

    res = m.recognize_page(page, params, deslant=True)
    ref_sl = check(res, DEFAULTS)
    assert ref_sl[:, 0].tolist() == planted and (res.slant_extent > 0).sum() == 5                # pad_y is the same above and below: cy stays
    np.testing.assert_array_equal(res.boxes, plain.boxes)                                         # the boxes do not move
    custom = aocr.SlantParams(threshold=-1, step_q16=2048, n_steps=24)
    check(m.recognize_page(page, params, deslant=custom), dict(threshold=128, light_text=0, step_q16=2048, n_steps=24))
    lay = m.recognize_page(page, params, layout=True, deslant=True)
    check(lay, DEFAULTS)
    assert lay.n_blocks >= 2 and np.abs(np.sort(lay.slant_q16) - np.sort(4096 * np.array(planted))).max() <= 4096
    with pytest.raises(ValueError):
        m.recognize_page(page, params, deslant=3)

    for off in (None, False):                                                                     # deslant=None is the call as it was
        b = m.recognize_page(page, params, deslant=off)
        assert sorted(vars(plain)) == sorted(vars(b)) and not hasattr(b, "slant_q16")
        for k, v in vars(plain).items():
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
    for layout in (None, True):
        reads[:] = []
        m.recognize_page(page, params, layout=layout)
        without, reads[:] = list(reads), []
        m.recognize_page(page, params, layout=layout, deslant=True)
        assert len(reads) == len(without) == 2 and reads[0] == without[0] and reads[1] > without[1], (layout, without, reads)
    empty = m.recognize_page(np.full((40, 60), 255, np.uint8), deslant=True)
    assert empty.boxes.shape == (0, 4) and empty.slant_q16.shape == (0,) and empty.slant_deg.shape == (0,) and empty.slant_extent.shape == (0,)
    m.check_health()
    m.shutdown()
