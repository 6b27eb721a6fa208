"""GPU: aocr_segment_page against the numpy restatement (tests/segment_ref.py) and against hand answers, aocr_crop_lines against
aocr_preprocess_lines on contiguous copies, and Model.recognize_page against Model.recognize on the numpy slices.  Everything here is exact:
the segmentation is integer arithmetic (the Otsu scores are doubles computed operation for operation as the restatement computes them) and
the crops repeat aocr_preprocess_lines' single-precision operations."""
import ctypes as C

import numpy as np
import pytest
import torch

import segment_ref as R
from page_harness import garbage_scratch, guarded_words, place
from segment_cases import CASES, SEEDED, SEEDED_SHAPES, seeded_page

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD_ROWS = 4           # rows of boxes_dev beyond max_boxes that every raw call gets: they must keep their sentinel
CHARS = "0123456789abcdefghijklmnopqrstuvwxyz"


def _segment(cuda, page, params, max_boxes=64, pitch=None, offset=0):
    """raw aocr_segment_page: (boxes (max_boxes + GUARD_ROWS, 6) with SENTINEL in the rows that were not written, counts, status).  The
    tensor is longer than max_boxes, so that a write past the cut lands in rows the caller checks, not in the allocator's slack."""
    import aocr
    H, W = page.shape
    dev, addr, pitch = place(cuda, page, pitch, offset, fill=0)           # the bytes around the page are ink, were they read
    p = aocr.SegmentParams(**params)
    need = aocr.lib.aocr_segment_scratch_bytes(H, W, max_boxes)
    assert need > 0
    scratch = garbage_scratch(cuda, need, 0)                              # exactly the queried size: the call must not rely on zeroed scratch
    boxes = guarded_words(cuda, max_boxes, GUARD_ROWS, SENTINEL, torch.int32, width=6)
    counts = guarded_words(cuda, 4, 0, SENTINEL, torch.int32)
    st = aocr.lib.aocr_segment_page(None, C.c_void_p(addr), pitch, H, W, C.byref(p), aocr.ptr(scratch), max_boxes, aocr.ptr(boxes), aocr.ptr(counts))
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), counts.cpu().numpy(), st


def _check(got_boxes, got_counts, ref_boxes, ref_counts, what):
    np.testing.assert_array_equal(got_counts, ref_counts, err_msg=str(what))
    n = len(ref_boxes)
    np.testing.assert_array_equal(got_boxes[:n], ref_boxes, err_msg=str(what))
    assert (got_boxes[n:] == SENTINEL).all(), what


@pytest.mark.parametrize("thr,light", [(128, 0), (-1, 0), (128, 1), (-1, 1)], ids=["fixed", "otsu", "fixed_light", "otsu_light"])
@pytest.mark.parametrize("shape", SEEDED_SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}o{s[3]}" for s in SEEDED_SHAPES])
def test_matches_restatement_on_seeded_pages(cuda, shape, thr, light):
    H, W, pitch, offset, seed = shape
    page = seeded_page(H, W, seed, bool(light))
    params = dict(SEEDED, threshold=thr, light_text=light)
    info = {}
    ref_boxes, ref_counts = R.segment_page(page, max_boxes=512, info=info, **params)
    # a page that takes no branch must not pass silently
    if H >= 40:
        assert info["row_runs"] > info["bands_merged"], "no row runs merged"
        assert info["bands_merged"] > info["lines"] >= 2, "no band dropped"
        assert info["col_runs"] > info["words_merged"], "no column runs merged"
        assert info["words_merged"] > info["boxes"], "no word dropped"
        assert info["max_boxes_per_line"] >= 2, "no band split"
    elif H == 9:
        assert info["boxes"] >= 2 and info["col_runs"] > info["words_merged"]
    if thr < 0 and H > 1:
        assert 0 <= ref_counts[2] <= 254
    boxes, counts, st = _segment(cuda, page, params, 512, pitch, offset)
    assert st == 0
    print(f"[segment] {H}x{W} pitch {pitch} offset {offset} thr {thr} light {light}: counts {counts.tolist()} events {info}")
    _check(boxes, counts, ref_boxes, ref_counts, shape)


@pytest.mark.parametrize("H,W,pitch", [(40, 2100, 2100), (1100, 40, 48), (8300, 16, 16)])
def test_long_axes(cuda, H, W, pitch):
    """the sizes at which the kernels change path: more than 1024 columns / rows (several elements per thread in the run finder), more than
    8192 rows (the row kernels' grid-stride loop) and more than 128 bands (the band loops of the column and word kernels)."""
    page = seeded_page(H, W, 7 * H + W)
    params = dict(SEEDED, threshold=-1, light_text=0)
    info = {}
    ref_boxes, ref_counts = R.segment_page(page, max_boxes=4096, info=info, **params)
    assert info["boxes"] >= 20 and (H < 8300 or info["lines"] > 128), info
    boxes, counts, st = _segment(cuda, page, params, 4096, pitch, 1)
    assert st == 0
    print(f"[segment] {H}x{W}: counts {counts.tolist()} events {info}")
    _check(boxes, counts, ref_boxes, ref_counts, (H, W))


def test_one_pixel_pages(cuda):
    """H = W = 1: ink or paper under a fixed threshold, and no Otsu threshold at all."""
    for v, thr, light, want in ((0, 128, 0, 1), (255, 128, 0, 0), (255, 128, 1, 1), (128, 128, 0, 1), (129, 128, 0, 0), (7, -1, 0, 0)):
        params = dict(R.DEFAULTS, threshold=thr, light_text=light, min_line_h=1, min_word_w=1, pad_x=0, pad_y=0)
        boxes, counts, st = _segment(cuda, np.full((1, 1), v, np.uint8), params, 4)
        assert st == 0 and counts.tolist() == [want, want, thr if thr >= 0 else -1, 0], (v, thr, light, counts)
        if want:
            assert boxes[0].tolist() == [0, 0, 1, 1, 0, 1]
        assert (boxes[want:] == SENTINEL).all()


def test_truncation(cuda):
    page = np.full((8, 40), 255, np.uint8)
    for k in range(5):
        page[2:6, 8 * k:8 * k + 3] = 0
    params = dict(R.DEFAULTS, threshold=128, min_line_h=3, word_gap=4, min_word_w=2, pad_x=0, pad_y=0)
    boxes, counts, st = _segment(cuda, page, params, 3)
    assert st == 0 and counts.tolist() == [5, 1, 128, 0]                            # the true number, not 3
    assert boxes.shape == (3 + GUARD_ROWS, 6)
    np.testing.assert_array_equal(boxes[:3], [[0, 2, 3, 6, 0, 12], [8, 2, 11, 6, 0, 12], [16, 2, 19, 6, 0, 12]])
    assert (boxes[3:] == SENTINEL).all(), boxes[3:]                                 # boxes 4 and 5 exist and were not written anywhere
    big, counts2, _ = _segment(cuda, page, params, 8)                               # and with room: the sentinel after the five
    assert counts2.tolist() == [5, 1, 128, 0] and (big[5:] == SENTINEL).all() and big[4].tolist() == [32, 2, 35, 6, 0, 12]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_painted_pages(cuda, case):
    boxes, counts, st = _segment(cuda, case["page"], case["params"], 16)
    assert st == 0
    _check(boxes, counts, case["boxes"], case["counts"], case["name"])


def _atlas_word(atlas, word, face):
    """coverage bitmap (gh, sum of advances) of a word: glyphs pasted at their pens, overlaps by maximum."""
    gi = [CHARS.index(c) for c in word]
    adv = [int(atlas.advance[face, g]) for g in gi]
    out = np.zeros((atlas.gh, sum(adv) + atlas.gw), np.uint8)
    pen = 0
    for g, a in zip(gi, adv):
        out[:, pen:pen + atlas.gw] = np.maximum(out[:, pen:pen + atlas.gw], atlas.pixels[face, g])
        pen += a
    return out[:, :max(1, int(np.nonzero(out.any(axis=0))[0].max()) + 1)]


def _atlas_page(H, W, lines, face_of=lambda i: i % 3):
    """(page, placements): words pasted on white at known positions; placements: (line, x, y, bitmap)."""
    import aocr
    atlas = aocr.GlyphAtlas.default()
    page = np.full((H, W), 255, np.uint8)
    placed, i = [], 0
    for ln, (y, words) in enumerate(lines):
        for x, w in words:
            bm = _atlas_word(atlas, w, face_of(i))
            i += 1
            assert y + bm.shape[0] <= H and x + bm.shape[1] <= W, (w, x, y, bm.shape)
            page[y:y + bm.shape[0], x:x + bm.shape[1]] = np.minimum(page[y:y + bm.shape[0], x:x + bm.shape[1]], 255 - bm)
            placed.append((ln, x, y, bm))
    return page, placed


def _atlas_expected(placed, H, W, thr, params):
    """the boxes from the atlas bitmaps alone: per line the rows first-to-last that hold ink of any of its words, per word its own first and
    last ink column, then the padding.  The preconditions that make this the answer (no gap inside a word reaches word_gap, words are at
    least word_gap apart, lines more than merge_gap apart, no blank row run inside a line above merge_gap) are asserted."""
    out = []
    n_lines = max(p[0] for p in placed) + 1
    prev_y1 = None
    for ln in range(n_lines):
        ws = [p for p in placed if p[0] == ln]
        rows = np.zeros(H, bool)
        for _, x, y, bm in ws:
            rows[y:y + bm.shape[0]] |= ((255 - bm) <= thr).any(axis=1)
        ys = np.nonzero(rows)[0]
        y0, y1 = int(ys.min()), int(ys.max()) + 1
        assert np.diff(ys).max() - 1 <= params["merge_gap"] and y1 - y0 >= params["min_line_h"]
        assert prev_y1 is None or y0 - prev_y1 > params["merge_gap"]
        prev_y1 = y1
        prev_x1 = None
        for _, x, y, bm in sorted(ws, key=lambda p: p[1]):
            cols = np.nonzero(((255 - bm) <= thr).any(axis=0))[0]
            x0, x1 = x + int(cols.min()), x + int(cols.max()) + 1
            assert np.diff(cols).max() - 1 < params["word_gap"] and x1 - x0 >= params["min_word_w"]
            assert prev_x1 is None or x0 - prev_x1 >= params["word_gap"]
            prev_x1 = x1
            out.append([max(0, x0 - params["pad_x"]), max(0, y0 - params["pad_y"]), min(W, x1 + params["pad_x"]), min(H, y1 + params["pad_y"]), ln,
                        int(((255 - bm) <= thr).sum())])
    return np.array(out, np.int32), n_lines


ATLAS_LINES = [(4, [(3, "hello"), (150, "w0rld"), (300, "42")]), (50, [(20, "page"), (170, "segment"), (380, "x")]), (97, [(0, "kilo"), (200, "byte5")])]


def test_glyph_atlas_page(cuda):
    H, W = 131, 470
    page, placed = _atlas_page(H, W, ATLAS_LINES)
    params = dict(R.DEFAULTS, threshold=128, min_word_w=2)
    want, n_lines = _atlas_expected(placed, H, W, 128, params)
    boxes, counts, st = _segment(cuda, page, params, 32)
    assert st == 0 and counts.tolist() == [len(want), n_lines, 128, 0]
    np.testing.assert_array_equal(boxes[:len(want)], want)
    ob, oc, _ = _segment(cuda, page, dict(params, threshold=-1), 32)                 # Otsu on anti-aliased glyphs: the restatement's answer
    rb, rc = R.segment_page(page, max_boxes=32, **dict(params, threshold=-1))
    _check(ob, oc, rb, rc, "atlas otsu")


def test_bit_identical_between_calls_and_pitches(cuda):
    H, W, _, _, seed = SEEDED_SHAPES[-1]
    page = seeded_page(H, W, seed)
    params = dict(SEEDED, threshold=-1, light_text=0)
    a = _segment(cuda, page, params, 512)
    b = _segment(cuda, page, params, 512)
    c = _segment(cuda, page, params, 512, pitch=W + 37, offset=5)
    d = _segment(cuda, page, params, 512, pitch=1024, offset=16)
    for other in (b, c, d):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1])
    assert a[1][0] > 100


def test_python_surface_takes_a_view(cuda):
    """segment_page_device on a non-contiguous view (a rectangle of a larger image): the row stride is the pitch, no copy."""
    import aocr
    H, W, _, _, seed = SEEDED_SHAPES[3]
    page = seeded_page(H, W, seed)
    big = torch.zeros((H + 9, W + 30), dtype=torch.uint8, device=cuda)
    big[4:4 + H, 11:11 + W] = torch.from_numpy(page).to(cuda)
    view = big[4:4 + H, 11:11 + W]
    assert not view.is_contiguous()
    p = aocr.SegmentParams(**dict(SEEDED, threshold=-1))
    boxes, counts = aocr.segment_page_device(view, p, max_boxes=64)
    rb, rc = R.segment_page(page, max_boxes=64, **dict(SEEDED, threshold=-1))
    assert np.array_equal(counts.cpu().numpy(), rc) and np.array_equal(boxes.cpu().numpy()[:len(rb)], rb)
    crops = aocr.crop_lines_device(view, boxes, counts, 100)
    assert crops.shape == (64, 1, 32, 100)
    from aocr.data import preprocess_batch
    ref = preprocess_batch([np.ascontiguousarray(page[b[1]:b[3], b[0]:b[2]]) for b in rb], 100, cuda)
    assert torch.equal(crops[:len(rb)], ref) and (crops[len(rb):] == 255.0).all()


def test_invalid_arguments_leave_the_outputs_untouched(cuda):
    import aocr
    page = seeded_page(40, 100, 3)
    good = dict(SEEDED, threshold=128, light_text=0)
    for field, v in (("threshold", 255), ("threshold", -2), ("min_row_ink", 0), ("min_line_h", 0), ("min_word_w", 0), ("merge_gap", -1),
                     ("word_gap", -3), ("pad_x", -1), ("pad_y", -1)):
        boxes, counts, st = _segment(cuda, page, dict(good, **{field: v}), 16)
        assert st != 0 and field in aocr.last_error(), (field, aocr.last_error())
        assert (boxes == SENTINEL).all() and (counts == SENTINEL).all(), field
    dev, addr, pitch = place(cuda, page)
    p = aocr.SegmentParams(**good)
    boxes = torch.full((16, 6), SENTINEL, dtype=torch.int32, device=cuda)
    counts = torch.full((4,), SENTINEL, dtype=torch.int32, device=cuda)
    scratch = torch.empty(1 << 16, dtype=torch.int64, device=cuda)
    for H, W, pit, mb, word in ((0, 100, 100, 16, "page size"), (40, 0, 100, 16, "page size"), (16385, 100, 100, 16, "page size"),
                                (40, 16385, 16385, 16, "page size"), (16384, 4097, 4097, 16, "page size"), (40, 100, 99, 16, "pitch"),
                                (40, 100, 100, 0, "max_boxes"), (40, 100, 100, 4097, "max_boxes")):
        st = aocr.lib.aocr_segment_page(None, C.c_void_p(addr), pit, H, W, C.byref(p), aocr.ptr(scratch), mb, aocr.ptr(boxes), aocr.ptr(counts))
        assert st != 0 and word in aocr.last_error(), (H, W, pit, mb, aocr.last_error())
    torch.cuda.synchronize()
    assert (boxes == SENTINEL).all() and (counts == SENTINEL).all()


# ---- aocr_crop_lines ---------------------------------------------------------------------------------------------------------------------
CROP_BOXES = [
    (0, 0, 100, 32),        # out_w = 100: the same size in both directions
    (5, 3, 41, 35),         # out_w = 36: the same size in both directions
    (10, 10, 30, 20),       # enlarges in both
    (0, 0, 128, 64),        # shrinks in both (the whole page)
    (3, 1, 120, 9),         # shrinks in x (for both widths), enlarges in y
    (60, 2, 70, 62),        # enlarges in x, shrinks in y
    (7, 5, 60, 6),          # height 1
    (9, 2, 10, 50),         # width 1
    (4, 4, 5, 5),           # one pixel
    (-5, -3, 40, 20),       # partly outside, top left: clamped to (0, 0, 40, 20)
    (100, 50, 140, 80),     # partly outside, bottom right: (100, 50, 128, 64)
    (200, 10, 230, 40),     # wholly outside: paper
    (50, 20, 40, 10),       # inverted: empty, paper
    (2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1),   # garbage: empty after clamping, paper
]


def _crop_reference(cuda, page, out_w):
    from aocr.data import preprocess_batch
    H, W = page.shape
    ref = torch.full((len(CROP_BOXES), 1, 32, out_w), 255.0, dtype=torch.float32, device=cuda)
    rows, imgs = [], []
    for i, (x0, y0, x1, y1) in enumerate(CROP_BOXES):
        x0, x1, y0, y1 = min(max(x0, 0), W), min(max(x1, 0), W), min(max(y0, 0), H), min(max(y1, 0), H)
        if x1 > x0 and y1 > y0:
            rows.append(i)
            imgs.append(np.ascontiguousarray(page[y0:y1, x0:x1]))
    ref[rows] = preprocess_batch(imgs, out_w, cuda)
    assert len(rows) == len(CROP_BOXES) - 3
    return ref


@pytest.mark.parametrize("out_w", [100, 36])
def test_crop_lines_equals_preprocess_lines(cuda, out_w):
    import aocr
    rng = np.random.default_rng(64128)
    page = rng.integers(0, 256, size=(64, 128), dtype=np.uint8)
    ref = _crop_reference(cuda, page, out_w).cpu().numpy()
    n = len(CROP_BOXES)
    bx = np.zeros((n, 6), np.int32)
    bx[:, :4] = np.array(CROP_BOXES, np.int64).astype(np.int32)
    boxes = torch.from_numpy(bx).to(cuda)
    for pitch, offset in ((128, 0), (141, 3)):
        dev, addr, pitch = place(cuda, page, pitch, offset, fill=99)

        def crop(count, n_boxes):
            out = torch.full((n, 1, 32, out_w), float(SENTINEL), dtype=torch.float32, device=cuda)
            cnt = torch.tensor([count, 0, 0, 0], dtype=torch.int32, device=cuda) if count is not None else None
            st = aocr.lib.aocr_crop_lines(None, C.c_void_p(addr), pitch, 64, 128, aocr.ptr(boxes), aocr.ptr(cnt), n_boxes, 32, out_w, aocr.ptr(out))
            torch.cuda.synchronize()
            assert st == 0, aocr.last_error()
            return out.cpu().numpy()

        np.testing.assert_array_equal(crop(None, n), ref)                            # count_dev = NULL: every box
        np.testing.assert_array_equal(crop(n + 5, n), ref)                           # a count above n_boxes: n_boxes
        part = crop(5, n)                                                            # a count below: the rows beyond it keep their sentinel
        np.testing.assert_array_equal(part[:5], ref[:5])
        assert (part[5:] == SENTINEL).all()
        assert (crop(0, n) == SENTINEL).all() and (crop(-3, n) == SENTINEL).all()
        assert (crop(None, 0) == SENTINEL).all()                                     # n_boxes = 0: a no-op
        few = crop(None, 3)
        np.testing.assert_array_equal(few[:3], ref[:3])
        assert (few[3:] == SENTINEL).all()
    assert (ref[11:] == 255.0).all() and not (ref[9] == 255.0).all()


# ---- Model.recognize_page ------------------------------------------------------------------------------------------------------------------
def _first_eos_text(aocr, labels):
    out = []
    for row in labels:
        ids = []
        for v in row:
            if v == 3:
                break
            ids.append(int(v))
        out.append(aocr.numlist2str(ids))
    return out


def test_recognize_page(cuda):
    import aocr
    from model_harness import make
    B, W = 32, 100
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=W, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    H, PW = 131, 470
    page, placed = _atlas_page(H, PW, ATLAS_LINES)
    params = aocr.SegmentParams(threshold=128, min_word_w=2)
    want, n_lines = _atlas_expected(placed, H, PW, 128, dict(R.DEFAULTS, threshold=128, min_word_w=2))
    lex = aocr.Lexicon([w for _, ws in ATLAS_LINES for _, w in ws] + ["zebra", "a1"])

    for width in (100, None):
        res = m.recognize_page(page, params, width=width, lexicon=lex)
        n = len(want)
        assert res.n_found == n and res.n_lines == n_lines and res.threshold == 128 and not res.truncated
        np.testing.assert_array_equal(res.boxes, want[:, :4])
        np.testing.assert_array_equal(res.line, want[:, 4])
        np.testing.assert_array_equal(res.ink, want[:, 5])
        order = [(int(l), int(b[0])) for l, b in zip(res.line, res.boxes)]
        assert order == sorted(order)                                                # reading order: line, then x
        assert res.labels.shape == (n, 12) and res.labels.dtype == np.int32 and res.scores.shape == (n,) and len(res.text) == n
        if width is not None:
            assert (res.widths == 100).all()
        else:
            exp_w = [min(-(-int(np.ceil(max(min((b[2] - b[0]) / (b[3] - b[1]), W / 32), 0.5) * 32)) // 32) * 32, W) for b in want]
            assert res.widths.tolist() == exp_w and len(set(exp_w)) >= 2, exp_w      # more than one bucket, or this checks nothing
        for w in sorted(set(res.widths.tolist())):
            idx = np.nonzero(res.widths == w)[0]
            slices = [np.ascontiguousarray(page[b[1]:b[3], b[0]:b[2]]) for b in res.boxes[idx]]
            ref = m.recognize(slices, width=int(w))
            np.testing.assert_array_equal(res.labels[idx], ref.labels)
            np.testing.assert_array_equal(res.scores[idx], ref.scores)
            assert [res.text[i] for i in idx] == ref.text
        assert res.text == _first_eos_text(aocr, res.labels)
        wi, wd = lex.nearest(torch.from_numpy(res.labels).to(cuda))
        np.testing.assert_array_equal(res.word_index, wi.cpu().numpy())
        np.testing.assert_array_equal(res.word_distance, wd.cpu().numpy())
        assert res.word == [lex.words[i] for i in res.word_index]
        print(f"[recognize_page] width {width}: {n} boxes, widths {sorted(set(res.widths.tolist()))}, e.g. {res.text[:3]} -> {res.word[:3]}")

    plain = m.recognize_page(torch.from_numpy(page), params, width=100, beam_size=5)
    assert not hasattr(plain, "word") and plain.labels.shape == (len(want), 12)
    cut = m.recognize_page(page, params, width=100, max_boxes=3)                     # truncated: the first three in reading order
    assert cut.truncated and cut.n_found == len(want) and len(cut.text) == 3
    np.testing.assert_array_equal(cut.boxes, want[:3, :4])

    empty = m.recognize_page(np.full((40, 60), 255, np.uint8), lexicon=lex)          # no ink: the empty result, not an error
    assert empty.boxes.shape == (0, 4) and empty.labels.shape == (0, 12) and empty.scores.shape == (0,) and empty.text == [] and empty.word == []
    assert empty.n_found == 0 and empty.threshold == -1 and not empty.truncated and empty.line.shape == (0,) and empty.ink.shape == (0,)
    with pytest.raises(ValueError):
        m.recognize_page(np.zeros((10, 10, 3), np.uint8))
    with pytest.raises(ValueError):
        m.recognize_page(np.zeros((10, 10), np.float32))
    m.check_health()
    m.shutdown()


def test_recognize_page_in_chunks(cuda):
    """a bucket with more boxes than batch_size: the 8 boxes of the atlas page at one width through a batch_size-3 model, three chunks
    (3, 3, 2), scattered back in reading order; and bucketed widths, where a bucket of 3 is one full chunk."""
    import aocr
    from model_harness import make
    B, W = 3, 100
    m, O, ocfg, P0, st, _ = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=W, maxlen=8, compute="f32",
                                 max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    page, placed = _atlas_page(131, 470, ATLAS_LINES)
    params = aocr.SegmentParams(threshold=128, min_word_w=2)
    want, _ = _atlas_expected(placed, 131, 470, 128, dict(R.DEFAULTS, threshold=128, min_word_w=2))
    lex = aocr.Lexicon([w for _, ws in ATLAS_LINES for _, w in ws])
    for width in (100, None):
        res = m.recognize_page(page, params, width=width, lexicon=lex)
        assert len(res.text) == len(want) == 8 and len(want) > 2 * B
        np.testing.assert_array_equal(res.boxes, want[:, :4])
        n_chunks = 0
        for w in sorted(set(res.widths.tolist())):
            members = np.nonzero(res.widths == w)[0]
            for c0 in range(0, len(members), B):
                idx = members[c0:c0 + B]
                n_chunks += 1
                ref = m.recognize([np.ascontiguousarray(page[b[1]:b[3], b[0]:b[2]]) for b in res.boxes[idx]], width=int(w), lexicon=lex)
                np.testing.assert_array_equal(res.labels[idx], ref.labels)
                np.testing.assert_array_equal(res.scores[idx], ref.scores)
                assert [res.text[i] for i in idx] == ref.text
                np.testing.assert_array_equal(res.word_index[idx], ref.word_index)
                np.testing.assert_array_equal(res.word_distance[idx], ref.word_distance)
        assert n_chunks == (3 if width else 4), (width, n_chunks, res.widths.tolist())
    m.check_health()
    m.shutdown()
