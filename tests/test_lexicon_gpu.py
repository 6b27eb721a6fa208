"""aocr_lexicon_nearest (include/aocr.h) on the device against the tests' numpy reference (lexicon_ref.nearest: the classic DP and
argmin's first minimum).  Every comparison is exact equality of index and dist.  The shapes are the smallest at which the kernel can
go wrong: every pattern length around the 32- and 64-bit column widths, word lists that are no multiple of a wave or a workgroup,
one slice per row and many, ranges that start and end anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import lexicon_ref as R

pytestmark = pytest.mark.gpu


def _pack(words, stride):
    a = np.zeros((len(words), stride), np.uint8)
    for i, w in enumerate(words):
        assert len(w) < stride
        a[i, :len(w)] = w
    return a


def _rows(pats, L, tail=None):
    """(B, L) int32: every pattern, its EOS (when it fits), then `tail` values (default: more EOS)."""
    lab = np.full((len(pats), L), 3, np.int32)
    for b, p in enumerate(pats):
        lab[b, :len(p)] = p
        if tail is not None and len(p) + 1 < L:
            lab[b, len(p) + 1:] = tail[b][:L - len(p) - 1]
    return lab


def _nearest(cuda, labels, words_u8, row_begin=None, out=None):
    """aocr_lexicon_nearest through the raw ABI on uploaded copies; returns (index, dist) as numpy."""
    import aocr
    from aocr._lib import LexiconDesc
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    B, L = labels.shape
    n, stride = words_u8.shape
    lab_d = torch.from_numpy(labels).to(cuda)
    words_d = torch.from_numpy(np.ascontiguousarray(words_u8) if n else np.zeros((1, stride), np.uint8)).to(cuda)
    rb_d = None if row_begin is None else torch.from_numpy(np.ascontiguousarray(row_begin, dtype=np.int32)).to(cuda)
    index, dist = out if out is not None else (torch.full((B,), -7, dtype=torch.int32, device=cuda), torch.full((B,), -7, dtype=torch.int32, device=cuda))
    need = aocr.lib.aocr_lexicon_scratch_bytes(B, n)
    scratch = torch.empty(need // 8, dtype=torch.int64, device=cuda) if need else None
    desc = LexiconDesc(aocr.ptr(words_d), n, stride)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    aocr.check(aocr.lib.aocr_lexicon_nearest(stream, aocr.ptr(lab_d), B, L, C.byref(desc), aocr.ptr(rb_d), aocr.ptr(scratch), aocr.ptr(index),
                                             aocr.ptr(dist)), "aocr_lexicon_nearest")
    torch.cuda.synchronize()
    return index.cpu().numpy(), dist.cpu().numpy()


def _check(cuda, labels, words_u8, row_begin=None, what=""):
    got_i, got_d = _nearest(cuda, labels, words_u8, row_begin)
    ref_i, ref_d = R.nearest(labels, words_u8, row_begin)
    assert np.array_equal(got_d, ref_d), (what, "dist", got_d.tolist(), ref_d.tolist())
    assert np.array_equal(got_i, ref_i), (what, "index", got_i.tolist(), ref_i.tolist())
    return got_i, got_d


def _mutate(rng, w, edits, lo=1, hi=255):
    w = list(w)
    for _ in range(edits):
        k = int(rng.integers(0, 3))
        if k == 0 and w:
            w[int(rng.integers(0, len(w)))] = int(rng.integers(lo, hi + 1))
        elif k == 1 and w:
            del w[int(rng.integers(0, len(w)))]
        else:
            w.insert(int(rng.integers(0, len(w) + 1)), int(rng.integers(lo, hi + 1)))
    return [v if v != 3 else 4 for v in w]


M_CASES = (0, 1, 2, 31, 32, 33, 63, 64)


def test_pattern_lengths(cuda):
    """L = 64, cut lengths on both sides of the 32- and 64-bit columns (m = 64: a row without any EOS), ids up to 255 on both sides;
    257 words of 0..63 ids at stride 64 with the empty word and, for each m, the row itself with one id changed (for m = 64, which no
    word of this stride can hold, its first 63 ids with one changed)."""
    rng = np.random.default_rng(64)
    ids = [v for v in range(1, 256) if v != 3]
    pats = [[int(v) for v in rng.choice(ids, size=m)] for m in M_CASES]
    for p in pats[3:]:
        p[0], p[-1] = 255, 254
    words = [[]]
    for p in pats:
        w = list(p[:63])
        if w:
            k = int(rng.integers(0, len(w)))
            w[k] = 255 if w[k] != 255 else 1
        words.append(w)
        words.append(list(p[:63]))                                       # and the row itself where it fits (distance 0 for m <= 63)
    while len(words) < 257:
        src = pats[int(rng.integers(0, len(pats)))]
        if rng.integers(0, 3) == 0:
            words.append([int(v) for v in rng.choice(ids, size=int(rng.integers(0, 64)))])
        else:
            words.append(_mutate(rng, src, int(rng.integers(1, 9)))[:63])
    order = rng.permutation(257)
    words = [words[i] for i in order]
    packed = _pack(words, 64)
    assert set(R.word_lengths(packed).tolist()) >= {0, 1, 2, 31, 32, 33, 63}
    labels = _rows(pats, 64)
    assert [len(R.cut(r)) for r in labels] == list(M_CASES)
    _, d = _check(cuda, labels, packed, what="with the rows themselves")
    assert d.tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    keep = [i for i, w in enumerate(words) if all(w != p[:63] for p in pats)]          # without the exact copies: distances >= 1
    _, d = _check(cuda, labels, packed[keep], what="one id changed")
    assert d.tolist()[1:7] == [1] * 6 and d[0] >= 1 and d[7] in (1, 2)


def test_cut_rule(cuda):
    """Ids behind the first EOS are garbage (> 255, 0, negative) and do not matter; a PAD (1) before the EOS is an ordinary symbol;
    aocr_edit_distance of the same rows against the winning words gives the same distances."""
    import aocr
    from aocr.dictionary import edit_distance_device
    rng = np.random.default_rng(2)
    L, B = 24, 16
    ids = [1, 2] + list(range(4, 12))
    pats = [[int(v) for v in rng.choice(ids, size=int(rng.integers(0, 16)))] for _ in range(B)]
    pats[1] = [1, 1, 5, 1]
    pats[2] = [1]
    words = [[1, 5, 1], [1, 1, 5], [5], [1, 1], [], [1, 1, 5, 1, 1]] + [_mutate(rng, pats[int(rng.integers(0, B))], int(rng.integers(1, 4)), 1, 11)[:15]
                                                                        for _ in range(300)]
    packed = _pack(words, 16)
    garbage = [rng.choice(np.array([0, -1, -2 ** 31, 256, 300, 2 ** 31 - 1, 3, 1, 7], np.int64), size=L) for _ in range(B)]
    labels = _rows(pats, L, tail=garbage)
    gi, gd = _check(cuda, labels, packed, what="garbage behind the EOS")
    gi2, gd2 = _nearest(cuda, _rows(pats, L), packed)
    assert np.array_equal(gi, gi2) and np.array_equal(gd, gd2)
    targets = _rows([words[i] for i in gi], L)
    d_dev, _ = edit_distance_device(torch.from_numpy(labels).to(cuda), torch.from_numpy(targets).to(cuda))
    assert np.array_equal(d_dev.cpu().numpy(), gd)
    # ids outside 1..255 BEFORE the EOS match nothing, and index nothing
    odd = [[5, 300, 6], [-1, 5], [256 + 5, 5], [0, 5, 0], [2 ** 31 - 1], [-2 ** 31, 7, 7]]
    _check(cuda, _rows(odd, L), packed, what="ids outside 1..255 before the EOS")


TIE_N, TIE_STRIDE = 70001, 32
_TIES = {}


def _tie_case():
    """70 001 words at stride 32, B = 5: copies of each row's best word at indices that fall into different lanes, waves and workgroups of
    any slicing (row r: 7, 63, 64, 4 097, 40 000 and 69 999 counted from the far end, each moved by 300 r), and a word of EQUAL distance
    but DIFFERENT length in front of the lowest copy (rows 0 and 2) or right behind it (rows 1 and 3)."""
    if _TIES:
        return _TIES
    rng = np.random.default_rng(70001)
    words = [[int(v) for v in rng.integers(4, 40, size=int(rng.integers(2, 17)))] for _ in range(TIE_N)]
    pats = [[int(v) for v in rng.integers(40, 60, size=m)] for m in (6, 9, 12, 20, 40)]      # ids the filler words do not use
    expect = []
    for r, p in enumerate(pats):
        best = list(p[:31])
        if len(p) <= 31:
            best[len(p) // 2] = 39                                       # distance 1 (m = 40: the 31-id prefix, distance 9)
        spots = [7 + 300 * r, 63 + 300 * r, 64 + 300 * r, 4097 + 300 * r, 40000 + 300 * r, 69999 - 300 * r]
        for i in spots:
            words[i] = list(best)
        if r < 4:
            other = list(p[:-1]) if r % 2 == 0 else list(p) + [39]       # one id less / one more: distance 1 too
            at = r if r % 2 == 0 else spots[0] + 1
            words[at] = other
            expect.append(at if at < spots[0] else spots[0])
        else:
            expect.append(spots[0])
    packed = _pack(words, TIE_STRIDE)
    labels = _rows(pats, 64)
    _TIES.update(labels=labels, packed=packed, expect=expect, ref=R.nearest(labels, packed))
    return _TIES


def test_ties_lowest_index_wins(cuda):
    import aocr
    t = _tie_case()
    assert aocr.lib.aocr_lexicon_scratch_bytes(5, TIE_N) > 0            # more than one workgroup per row: the second reduction level runs
    ref_i, ref_d = t["ref"]
    assert ref_i.tolist() == t["expect"] and ref_d.tolist() == [1, 1, 1, 1, 9]
    i1, d1 = _nearest(cuda, t["labels"], t["packed"])
    i2, d2 = _nearest(cuda, t["labels"], t["packed"])
    assert np.array_equal(d1, ref_d) and np.array_equal(i1, ref_i), (i1.tolist(), d1.tolist(), ref_i.tolist(), ref_d.tolist())
    assert i1.tobytes() == i2.tobytes() and d1.tobytes() == d2.tobytes()


def test_per_row_ranges(cuda):
    rng = np.random.default_rng(4)
    n, B, L = 1000, 12, 20
    words = [[int(v) for v in rng.integers(4, 10, size=int(rng.integers(0, 16)))] for _ in range(n)]
    packed = _pack(words, 16)
    pats = [[int(v) for v in rng.integers(4, 10, size=int(rng.integers(0, 16)))] for _ in range(B)]
    labels = _rows(pats, L)
    # empty at the first, a middle and the last row; one-word ranges; bounds off every multiple of 64
    rb = [0, 0, 1, 2, 65, 67, 67, 190, 321, 322, 707, 999, 999]
    i, d = _check(cuda, labels, packed, rb, what="ranges")
    assert [b for b in range(B) if i[b] == -1] == [0, 5, 11] and (d[i == -1] == -1).all()
    assert i[1] == 0 and i[2] == 1 and i[8] == 321
    # a table that leaves [0, n] on both sides: the device clamps, the expectation is computed on the clamped table
    rb = [-5, -1, 3, 3, 64, 130, 131, 500, 500, 901, 1000, 1007, 2 ** 31 - 1]
    i, d = _check(cuda, labels, packed, rb, what="clamped")
    assert i[0] == -1 and i[11] == -1 and 0 <= i[1] < 3 and 901 <= i[9] < 1000 and i[10] == -1
    # several workgroups per row (n_words beyond one slice) with narrow ranges
    big = np.concatenate([packed] * 9)[:8200]
    rb = [0, 0, 5, 300, 4095, 4097, 4097, 4200, 8000, 8191, 8192, 8200, 8200]
    _check(cuda, labels, big, rb, what="ranges over several slices")
    # no table = every row searches the whole list: the same list repeated once per row, with row b searching copy b
    i0, d0 = _check(cuda, labels, packed, None, what="no table")
    rep = np.concatenate([packed] * B)
    i1, d1 = _nearest(cuda, labels, rep, [b * n for b in range(B + 1)])
    assert np.array_equal(d1, d0) and np.array_equal(i1 - n * np.arange(B), i0)


def test_shapes(cuda):
    rng = np.random.default_rng(5)
    words = [[int(v) for v in rng.integers(4, 9, size=int(rng.integers(0, 16)))] for _ in range(130)]
    pats = [[int(v) for v in rng.integers(4, 9, size=int(rng.integers(0, 20)))] for _ in range(300)]
    _check(cuda, _rows(pats[:1], 20), _pack(words, 16), what="B = 1")
    i, d = _check(cuda, _rows(pats, 20), _pack(words[7:8], 16), what="B = 300, one word")
    assert (i == 0).all()
    i, d = _check(cuda, _rows(pats[:3], 20), np.zeros((0, 16), np.uint8), what="no words")
    assert i.tolist() == [-1] * 3 and d.tolist() == [-1] * 3
    i, d = _check(cuda, _rows(pats[:3], 20), np.zeros((0, 16), np.uint8), [0, 0, 0, 0], what="no words, a table")
    assert i.tolist() == [-1] * 3
    out = (torch.full((4,), 77, dtype=torch.int32, device=cuda), torch.full((4,), 78, dtype=torch.int32, device=cuda))
    i, d = _nearest(cuda, np.zeros((0, 20), np.int32), _pack(words, 16), out=out)                # B = 0: nothing is written
    assert i.tolist() == [77] * 4 and d.tolist() == [78] * 4
    for stride in (16, 256):
        ws = [[int(v) for v in rng.integers(1, 256, size=int(rng.integers(0, stride)))] for _ in range(129)] + [[], [9] * (stride - 1)]
        ws = [[v if v != 3 else 4 for v in w] for w in ws]
        ps = [_mutate(rng, ws[int(rng.integers(0, len(ws)))][:60], 3) for _ in range(7)] + [[], [9] * 64]
        _check(cuda, _rows(ps, 64), _pack(ws, stride), what=f"stride {stride}")
    with pytest.raises(Exception, match="scratch_dev is NULL"):
        import aocr
        from aocr._lib import LexiconDesc
        w = torch.zeros((5000, 16), dtype=torch.uint8, device=cuda)
        lab = torch.full((2, 8), 3, dtype=torch.int32, device=cuda)
        o = torch.zeros(2, dtype=torch.int32, device=cuda)
        aocr.check(aocr.lib.aocr_lexicon_nearest(None, aocr.ptr(lab), 2, 8, C.byref(LexiconDesc(aocr.ptr(w), 5000, 16)), None, None, aocr.ptr(o),
                                                 aocr.ptr(o)))


def test_lexicon_class_on_device(cuda):
    """aocr.Lexicon.nearest: the packed list of the class, its own scratch (grown and reused), a host row_begin table."""
    import aocr
    rng = np.random.default_rng(6)
    abc = "abcdefghijklmnopqrstuvwxyz0123456789"
    words = ["".join(rng.choice(list(abc), size=int(rng.integers(1, 9)))) for _ in range(5000)]
    lex = aocr.Lexicon(words, device=cuda)
    assert lex.n_words == 5000 and lex.stride == 16
    pats = [list(lex.array[int(rng.integers(0, 5000))][:int(rng.integers(1, 6))]) + [int(v) for v in rng.integers(4, 40, size=2)] for _ in range(9)]
    labels = _rows(pats, 12)
    lab_d = torch.from_numpy(labels).to(cuda)
    for rb in (None, np.arange(10) * 555):
        i, d = lex.nearest(lab_d, rb)
        torch.cuda.synchronize()
        ref_i, ref_d = R.nearest(labels, lex.array, rb)
        assert np.array_equal(i.cpu().numpy(), ref_i) and np.array_equal(d.cpu().numpy(), ref_d)
    scratch = lex._scratch
    lex.nearest(lab_d[:4])
    assert lex._scratch is scratch                                       # a smaller batch reuses it
    with pytest.raises(ValueError):
        lex.nearest(lab_d, [0, 1, 2])


def test_through_the_model(cuda):
    """Model.recognize(images, lexicon=...) on the small fp32 configuration of test_recognize_gpu.py: the snapped words are the reference's
    for the labels the call returns, and labels / scores / text are those of the same call without a lexicon."""
    import aocr
    from model_harness import make
    B, W = 32, 100
    m, O, ocfg, P0, st, batch = make(dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True), B=B, W=W, maxlen=8, compute="f32",
                                     max_decoder_l=12, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    rng = np.random.default_rng(8)
    abc = list("abcdefghijklmnopqrstuvwxyz0123456789")
    words = ["".join(rng.choice(abc, size=int(rng.integers(1, 9)))) for _ in range(B * 50)] + ["not-a-word"]
    lex = aocr.Lexicon(words)
    assert lex.n_words == B * 50 and lex.skipped == ["not-a-word"]
    images = torch.from_numpy(np.asarray(batch[0]))
    for beam in (1, 5):
        plain = m.recognize(images, beam_size=beam)
        assert not hasattr(plain, "word") and not hasattr(plain, "word_index")
        res = m.recognize(images, beam_size=beam, lexicon=lex)
        assert np.array_equal(res.labels, plain.labels) and np.array_equal(res.scores, plain.scores) and res.text == plain.text
        ref_i, ref_d = R.nearest(res.labels, lex.array)
        assert res.word_index.dtype == np.int32 and res.word_distance.dtype == np.int32
        assert np.array_equal(res.word_index, ref_i) and np.array_equal(res.word_distance, ref_d)
        assert res.word == [lex.words[i] for i in ref_i]
        rows = np.arange(B + 1, dtype=np.int32) * 50                     # every image its own 50 words
        per = m.recognize(images, beam_size=beam, lexicon=lex, lexicon_rows=rows)
        ref_i, ref_d = R.nearest(per.labels, lex.array, rows)
        assert np.array_equal(per.labels, plain.labels)
        assert np.array_equal(per.word_index, ref_i) and np.array_equal(per.word_distance, ref_d)
        assert all(50 * b <= per.word_index[b] < 50 * (b + 1) for b in range(B))
        assert per.word == [lex.words[i] for i in ref_i]
        print(f"[lexicon] beam {beam}: e.g. {res.text[:3]} -> {res.word[:3]} at {res.word_distance[:3].tolist()} edits")
    none = m.recognize(images, lexicon=lex, lexicon_rows=np.full(B + 1, 7))      # empty ranges: no word
    assert none.word == [None] * B and (none.word_index == -1).all() and (none.word_distance == -1).all()
    with pytest.raises(ValueError):
        m.recognize(images, lexicon_rows=np.arange(B + 1))
    m.shutdown()
