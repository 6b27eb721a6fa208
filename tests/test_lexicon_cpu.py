"""Lexicon snapping (include/aocr.h aocr_lexicon_nearest) without a GPU: the tests' numpy reference against the host Levenshtein
restatement, the packing of `aocr.Lexicon`, and the argument checks of the ABI (which happen before any device call)."""
import ctypes as C

import numpy as np
import pytest

import lexicon_ref as R


def _pack(words, stride):
    a = np.zeros((len(words), stride), np.uint8)
    for i, w in enumerate(words):
        a[i, :len(w)] = w
    return a


def test_reference_equals_host_levenshtein_pair_by_pair():
    from aocr.dictionary import levenshtein
    rng = np.random.default_rng(11)
    words = [[]] + [rng.integers(1, 6, size=int(rng.integers(0, 16))).tolist() for _ in range(39)]     # small alphabet: many matches
    packed = _pack(words, 16)
    pats = [[]] + [rng.integers(1, 6, size=int(rng.integers(0, 20))).tolist() for _ in range(9)]
    pats = [[v if v != 3 else 7 for v in p] for p in pats]                                             # 3 would cut the row
    n = 0
    for p in pats:
        d = R.distances(p, packed)
        for w, got in zip(words, d):
            assert got == levenshtein(p, w), (p, w, got)
            n += 1
    assert n == 400
    labels = np.full((len(pats), 24), 3, np.int32)
    for b, p in enumerate(pats):
        labels[b, :len(p)] = p
        labels[b, len(p) + 1:] = 1000 + b                           # behind the EOS: ignored
    index, dist = R.nearest(labels, packed)
    for b, p in enumerate(pats):
        all_d = [levenshtein(p, w) for w in words]
        assert dist[b] == min(all_d) and index[b] == all_d.index(min(all_d))      # list.index: the first minimum
    assert index[0] == 0 and dist[0] == 0                                         # empty row, empty word
    index, dist = R.nearest(labels, packed, [-2, 0, 3, 4, 7, 7, 7, 30, 40, 90, 90])   # -2 clamps to 0, 90 to 40: rows 0, 8, 9 search nothing
    assert [b for b in range(10) if index[b] == -1] == [0, 4, 5, 8, 9] and (dist[index == -1] == -1).all()
    assert index[2] == 3 and 4 <= index[3] < 7 and 7 <= index[6] < 30 and 30 <= index[7] < 40
    for b in (1, 3, 6, 7):
        assert dist[b] == R.distances(R.cut(labels[b]), packed)[index[b]]


def test_lexicon_packing():
    import aocr
    from aocr.dictionary import char_id
    lex = aocr.Lexicon(["abc", " 42 \n", "", "x" * 15, "a-b", "Z9"])
    assert lex.words == ["abc", "42", "", "x" * 15, "Z9"] and lex.skipped == ["a-b"]          # '-' maps to id 1
    assert lex.stride == 16 and lex.array.shape == (5, 16) and lex.array.dtype == np.uint8 and lex.n_words == 5
    assert lex.array[0].tolist() == [char_id(c) for c in b"abc"] + [0] * 13 == [14, 15, 16] + [0] * 13
    assert lex.array[1].tolist() == [8, 6] + [0] * 14
    assert not lex.array[2].any()
    assert lex.array[3].tolist() == [char_id(ord("x"))] * 15 + [0]                            # 15 ids + the 0 fit stride 16
    assert lex.array[4].tolist() == [char_id(ord("Z")), 13] + [0] * 14
    assert R.word_lengths(lex.array).tolist() == [3, 2, 0, 15, 2]
    lex = aocr.Lexicon(["abc", "y" * 16])
    assert lex.stride == 32 and lex.words == ["abc", "y" * 16] and lex.array[1, 15] != 0 and lex.array[1, 16] == 0      # 16 ids force 32
    lex = aocr.Lexicon(["abc", "y" * 16, "a-b", "z" * 15], stride=16)
    assert lex.stride == 16 and lex.words == ["abc", "z" * 15] and lex.skipped == ["y" * 16, "a-b"]
    lex = aocr.Lexicon(["\xff\xfe", "q" * 300, "ok"])                                        # bytes 255, 254 -> ids 172, 171; 300 ids never fit
    assert lex.words == ["\xff\xfe", "ok"] and lex.array[0, :3].tolist() == [172, 171, 0] and lex.skipped == ["q" * 300]
    assert aocr.Lexicon([]).stride == 16 and aocr.Lexicon([]).n_words == 0
    for bad in (8, 24, 272):
        with pytest.raises(ValueError):
            aocr.Lexicon(["a"], stride=bad)
    with pytest.raises(RuntimeError):
        aocr.Lexicon(["a"]).desc()                                                            # not uploaded


def test_load_lexicon(tmp_path):
    import aocr
    p = tmp_path / "lexicon.txt"
    p.write_bytes(b"hello\nworld \nfoo-bar\n\xe9t\xe9\n")
    lex = aocr.load_lexicon(str(p))
    assert lex.words == ["hello", "world", "\xe9t\xe9"] and lex.skipped == ["foo-bar"] and lex.stride == 16
    with pytest.raises(FileNotFoundError, match="Error: Data file .* not found"):
        aocr.load_lexicon(str(tmp_path / "missing.txt"))
    with pytest.raises(FileNotFoundError, match="Error: Data file .* not found"):
        aocr.load_dictionary(str(tmp_path / "missing.txt"))                                   # the shape it mirrors


def test_abi_symbols_and_argument_checks():
    """No device is touched: aocr_lexicon_scratch_bytes is host arithmetic, and every bad call fails on its arguments."""
    import aocr
    from aocr._lib import LexiconDesc
    raw = C.CDLL(aocr._lib.LIB_PATH)
    assert hasattr(raw, "aocr_lexicon_scratch_bytes") and hasattr(raw, "aocr_lexicon_nearest")
    sb = aocr.lib.aocr_lexicon_scratch_bytes
    assert sb(0, 1000) == 0 and sb(256, 0) == 0
    assert sb(256, 90000) % 8 == 0 and sb(256, 90000) == 2 * sb(128, 90000)                   # one 64-bit key per row and slice, if any
    labels = np.full((4, 64), 3, np.int32)
    words = np.zeros((8, 16 + 16), np.uint8)
    words = words.reshape(-1)[(-words.ctypes.data) % 16:][:8 * 16].reshape(8, 16)             # a 16-byte aligned host view
    out_i, out_d = np.zeros(4, np.int32), np.zeros(4, np.int32)
    lp, ip, dp = (C.c_void_p(a.ctypes.data) for a in (labels, out_i, out_d))

    def call(L=64, stride=16, lex=True, index=ip, dist=dp, n_words=8, scratch=None, lab=lp):
        d = LexiconDesc(C.c_void_p(words.ctypes.data), n_words, stride)
        return aocr.lib.aocr_lexicon_nearest(None, lab, 4, L, C.byref(d) if lex else None, None, scratch, index, dist)

    for kw, what in ((dict(L=65), "L=65"), (dict(L=0), "L=0"), (dict(stride=24), "stride 24"), (dict(stride=0), "stride 0"),
                     (dict(stride=272), "stride 272"), (dict(lex=False), "lexicon is NULL"), (dict(index=None), "NULL"),
                     (dict(dist=None), "NULL"), (dict(lab=None), "NULL"), (dict(n_words=-1), "n_words=-1"),
                     (dict(n_words=90000), "scratch_dev is NULL")):
        assert call(**kw) != 0, kw
        assert what in aocr.last_error(), (kw, aocr.last_error())
    assert sb(4, 90000) > 0
    assert (out_i == 0).all() and (out_d == 0).all()
    d = LexiconDesc(C.c_void_p(words.ctypes.data), 8, 16)
    assert aocr.lib.aocr_lexicon_nearest(None, lp, 0, 64, C.byref(d), None, None, ip, dp) == 0          # B == 0: a no-op, no launch
