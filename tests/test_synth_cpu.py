"""Synthetic word lines (include/aocr.h aocr_synth_lines) without a GPU: the numpy restatement tests/synth_ref.py against hand answers
that do not use it, the targets rows, the style draw of aocr.SynthGen, the shipped atlas, the host targets against DataGen's rule, and the
argument checks of the ABI (which happen before any device call)."""
import ctypes as C

import numpy as np
import pytest

import synth_ref as R

F = np.float32
GH, GW = R.BLIT_GH, R.BLIT_GW


_pack, _blit_atlas, _side_by_side = R.pack, R.blit_atlas, R.side_by_side


def test_identity_blits_the_glyphs_side_by_side():
    pixels, advance = _blit_atlas()
    words = _pack([[4, 5, 6, 8], [7, 7, 4], [8]])
    for W in (24, 9):                                                 # 3 + 0 + 5 + 2 = 10 columns of word 0: once inside, once cut by W
        got = R.synth(words, pixels, advance, R.style_records([R.identity(w) for w in range(3)]), GH, W)
        for w, ids in enumerate(([4, 5, 6, 8], [7, 7, 4], [8])):
            np.testing.assert_array_equal(got[w, 0], _side_by_side(pixels, advance, ids, W), err_msg=f"word {w} W {W}")
    assert not got[0, 0, :, 3 + 5 + 2:].any() and got[0, 0, :, :3].any()                 # 0 after the last pen (W = 9: column 9 is none)


def test_integer_shift_blits_over_the_paper():
    pixels, advance = _blit_atlas()
    words = _pack([[6, 4]])
    H, W = GH + 3, 16
    got = R.synth(words, pixels, advance, R.style_records([(0, 0, 0.0, 1.0, 1.0, 3.0, 2.0, 200.0, 40.0)]), H, W)
    ink = np.zeros((H, W), bool)
    ink[2:2 + GH, 3:3 + 5] = pixels[0, 2, :, :5] == 255
    ink[2:2 + GH, 8:8 + 3] = pixels[0, 0, :, :3] == 255
    np.testing.assert_array_equal(got[0, 0], np.where(ink, F(200), F(40)))
    # one extra pixel of spacing moves the second glyph by one column
    got = R.synth(words, pixels, advance, R.style_records([(0, 0, 1.0, 1.0, 1.0, 3.0, 2.0, 200.0, 40.0)]), H, W)
    ink[:, 8:] = False
    ink[2:2 + GH, 9:9 + 3] = pixels[0, 0, :, :3] == 255
    np.testing.assert_array_equal(got[0, 0], np.where(ink, F(200), F(40)))


def test_half_steps_average_the_neighbours():
    pixels, advance = _blit_atlas()
    words = _pack([[7]])                                                          # glyph 3: advance 6 = gw, ink in every column
    got = R.synth(words, pixels, advance, R.style_records([(0, 0, 0.0, 0.5, 0.5, 0.0, 0.0, 255.0, 0.0)]), 2 * GH, 2 * GW)
    P = np.pad(pixels[0, 3].astype(np.float64), ((0, 1), (0, 1)))                  # 0 outside the bitmap
    want = np.empty((2 * GH, 2 * GW))
    for y in range(2 * GH):
        for x in range(2 * GW):
            r, c = y // 2, x // 2
            want[y, x] = (P[r, c] + P[r, c + x % 2] + P[r + y % 2, c] + P[r + y % 2, c + x % 2]) / 4.0
    assert set(np.unique(want)) <= {0.0, 63.75, 127.5, 191.25, 255.0} and len(np.unique(want)) >= 4
    np.testing.assert_array_equal(got[0, 0], want.astype(F))                      # quarters of 255 divide and multiply back exactly


def test_bad_records_draw_paper_and_unknown_ids_draw_nothing():
    pixels, advance = _blit_atlas()
    words = _pack([[4, 6], [3, 4, 200, 6]])
    rec = [(-1, 0, 0, 1, 1, 0, 0, 255, 7), (2, 0, 0, 1, 1, 0, 0, 255, 7), (0, 1, 0, 1, 1, 0, 0, 255, 7), (0, 0, 0, 1, 1, np.nan, 0, 255, 7),
           (0, 0, np.nan, 1, 1, 0, 0, 255, 7), (0, 0, -5.0, 1, 1, 0, 0, 255, 7), (1, 0, 0, 1, 1, 0, 0, 255, 0)]
    got = R.synth(words, pixels, advance, R.style_records(rec), GH, 12)
    for i in range(4):
        assert (got[i] == 7).all(), i                                             # word -1, word n_words, face 1 of 1, NaN x0
    plain = R.synth(words, pixels, advance, R.style_records([(0, 0, 0, 1, 1, 0, 0, 255, 7)]), GH, 12)
    np.testing.assert_array_equal(got[4], plain[0]); np.testing.assert_array_equal(got[5], plain[0])      # NaN, negative spacing: 0
    np.testing.assert_array_equal(got[6, 0], _side_by_side(pixels, advance, [4, 6], 12))                 # ids 3 and 200 take no room


def test_targets_rows():
    words = _pack([[], [9], [4, 5, 6, 7, 8]])
    st = R.style_records([R.identity(0), R.identity(1), R.identity(2), R.identity(3), R.identity(2, face=9)])
    tg, te = R.targets(words, st, 1, 6)
    assert tg.dtype == np.int32 and te.dtype == np.int32
    assert tg.tolist() == [[2, 1, 1, 1, 1, 1], [2, 9, 1, 1, 1, 1], [2, 4, 5, 6, 7, 8], [2, 1, 1, 1, 1, 1], [2, 1, 1, 1, 1, 1]]
    assert te.tolist() == [[3, 1, 1, 1, 1, 1], [9, 3, 1, 1, 1, 1], [4, 5, 6, 7, 8, 3], [3, 1, 1, 1, 1, 1], [3, 1, 1, 1, 1, 1]]
    tg, te = R.targets(words, st, 1, 3)                                           # L = 3 cuts the five-id word: no EOS is left
    assert tg.tolist() == [[2, 1, 1], [2, 9, 1], [2, 4, 5], [2, 1, 1], [2, 1, 1]]
    assert te.tolist() == [[3, 1, 1], [9, 3, 1], [4, 5, 6], [3, 1, 1], [3, 1, 1]]
    tg, te = R.targets(words, st, 1, 1)
    assert tg.tolist() == [[2]] * 5 and te.tolist() == [[3], [9], [4], [3], [3]]


def test_default_atlas():
    import aocr
    a = aocr.GlyphAtlas.default()
    assert a.n_glyphs == 36 and 1 <= a.n_faces <= 3 and a.gh == 32 and 1 <= a.gw <= 64
    assert a.pixels.dtype == np.uint8 and a.advance.dtype == np.uint8 and a.advance.shape == (a.n_faces, 36)
    assert a.advance.min() >= 1 and a.advance.max() <= a.gw
    assert len(a.names) == a.n_faces and all(a.names)                              # the fonts it was made from are recorded
    assert a.pixels.reshape(a.n_faces * 36, -1).max(axis=1).min() >= 128           # every glyph has ink
    import os
    assert os.path.getsize(aocr.synth_lines.DEFAULT_ATLAS) <= 64 * 1024
    with open(aocr.synth_lines.DEFAULT_ATLAS, "rb") as f:
        assert all(c == 10 or 32 <= c < 127 for c in f.read())                     # the shipped atlas is plain text
    with pytest.raises(RuntimeError):
        a.desc()                                                                   # not uploaded
    with pytest.raises(ValueError):
        aocr.GlyphAtlas(np.zeros((1, 2, 65, 4), np.uint8), np.zeros((1, 2), np.uint8))
    with pytest.raises(ValueError):
        aocr.GlyphAtlas(np.zeros((1, 2, 4, 4), np.float32), np.zeros((1, 2), np.uint8))


def test_atlas_text_form_round_trips(tmp_path):
    """save rounds the coverage to 16 levels (17 l: 0 and 255 exact, any other value moves by at most 8) and leaves trailing paper off;
    load returns exactly the rounded atlas, and a second save writes the same bytes."""
    import aocr
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (2, 3, 7, 5), dtype=np.uint8)
    px[0, 1] = 0                                                                   # a blank glyph: rows of '|' alone
    px[1, 2, :, 3:] = 0                                                            # trailing paper
    px[1, 0, 0] = [0, 255, 8, 9, 247]                                              # 8 rounds down to paper, 9 up to level 1, 247 up to 255
    adv = rng.integers(0, 6, (2, 3), dtype=np.uint8)
    aocr.GlyphAtlas(px, adv, ["one face", "another"]).save(tmp_path / "a.txt")
    b = aocr.GlyphAtlas.load(tmp_path / "a.txt")
    want = ((px.astype(np.int32) * 15 + 127) // 255 * 17).astype(np.uint8)
    np.testing.assert_array_equal(b.pixels, want)
    np.testing.assert_array_equal(b.advance, adv)
    assert b.names == ["one face", "another"]
    assert b.pixels[1, 0, 0].tolist() == [0, 255, 0, 17, 255] and np.abs(want.astype(int) - px).max() <= 8
    assert ((want == 0) == (px <= 8)).all() and ((want == 255) == (px >= 247)).all()
    b.save(tmp_path / "b.txt")
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()
    (tmp_path / "c.txt").write_text("not an atlas\n")
    with pytest.raises(ValueError):
        aocr.GlyphAtlas.load(tmp_path / "c.txt")


WORDS = ["a", "hello", "w0rld", "mmmmmmmmmmmmmmmmmmmmmmm", "", "il1", "quick", "zebra9"]


@pytest.mark.parametrize("fill_width", [True, False])
@pytest.mark.parametrize("width", [100, 37, 256])
def test_params_are_counter_based_and_keep_the_text_box_inside(width, fill_width):
    """The box edges are recomputed in float64 from the fp32 records.  The records are float64 values cast once to fp32 (relative error
    2^-24 each) and an edge combines three of them, so an edge may pass the image's by 3 * 2^-24 of its size: the slack is 1e-6 of it."""
    import aocr
    lex, atlas = aocr.Lexicon(WORDS), aocr.GlyphAtlas.default()
    g = aocr.SynthGen(lex, atlas, width=width, seed=77, fill_width=fill_width, stretch=1.5)
    a, b = g.params(64, 5), g.params(64, 5)
    assert a.dtype == aocr.synth_lines.STYLE_DTYPE == R.STYLE_DTYPE and a.tobytes() == b.tobytes()
    assert a.tobytes() != g.params(64, 6).tobytes()
    assert a.tobytes() != aocr.SynthGen(lex, atlas, width=width, seed=78, fill_width=fill_width, stretch=1.5).params(64, 5).tobytes()
    np.testing.assert_array_equal(g.params(16, 5), a[:16])                         # image i draws its own nine uniforms
    assert set(a["word"]) <= set(range(len(WORDS))) and len(set(a["word"])) > 4 and set(a["face"]) == set(range(atlas.n_faces))
    filled = 0
    for st in a:
        ids = R.word_of(lex.array, lex.stride, st, atlas.n_faces)
        assert st["spacing"] >= 0 and st["sx"] > 0 and st["sy"] > 0
        total = float(sum(int(atlas.advance[st["face"], v - 4]) for v in ids)) + max(len(ids) - 1, 0) * float(st["spacing"])
        tw, th = total / float(st["sx"]), atlas.gh / float(st["sy"])
        assert st["x0"] >= 0 and st["y0"] >= 0
        assert float(st["x0"]) + tw <= width * (1 + 1e-6) and float(st["y0"]) + th <= 32 * (1 + 1e-6), st
        assert 0.6 * 32 * (1 - 1e-6) <= th
        if len(ids):
            if fill_width:
                assert abs(tw - width) <= 1e-6 * width and st["x0"] == 0
            else:
                assert tw == pytest.approx(width, rel=1e-6) or 1 / 1.5 * (1 - 1e-6) <= float(st["sx"]) / float(st["sy"]) <= 1.5 * (1 + 1e-6)
            filled += abs(tw - width) <= 1e-6 * width
    assert filled > 0


def test_host_targets_follow_datagens_rule():
    import aocr
    from aocr.data import str2numlist
    from aocr.synth_lines import host_targets
    lex = aocr.Lexicon(WORDS)
    pick = [3, 0, 4, 1, 1, 7]
    tg, te, nnz = host_targets(lex.array[pick])
    lists = [str2numlist(lex.words[w]) for w in pick]                               # DataGen._emit, written out
    max_len = max(len(l) for l in lists)
    want_t, want_e, want_n = np.ones((len(pick), max_len - 1), np.int32), np.ones((len(pick), max_len - 1), np.int32), 0
    for i, l in enumerate(lists):
        want_n += len(l) - 1
        want_t[i, :len(l) - 1] = l[:-1]
        want_e[i, :len(l) - 1] = l[1:]
    np.testing.assert_array_equal(tg, want_t); np.testing.assert_array_equal(te, want_e)
    assert nnz == want_n and tg.dtype == np.int32 and te.dtype == np.int32
    st = R.style_records([R.identity(w) for w in pick])
    rt, re_ = R.targets(lex.array, st, 1, tg.shape[1])                              # and the kernel's rows are the same rows
    np.testing.assert_array_equal(rt, tg); np.testing.assert_array_equal(re_, te)


def test_from_font_needs_pillow_only_when_called(monkeypatch):
    import sys
    import aocr
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError, match="Pillow"):
        aocr.GlyphAtlas.from_font(["/nonexistent.ttf"])
    assert aocr.GlyphAtlas.default().n_glyphs == 36                                # the library side does not


def test_abi_symbol_and_argument_checks():
    """No device is touched: every bad call fails on its arguments, and n_images == 0 launches nothing."""
    import aocr
    from aocr._lib import GlyphAtlasDesc, LexiconDesc, SynthStyle
    raw = C.CDLL(aocr._lib.LIB_PATH)
    assert hasattr(raw, "aocr_synth_lines")
    assert C.sizeof(SynthStyle) == 36 == R.STYLE_DTYPE.itemsize and C.sizeof(GlyphAtlasDesc) == 32
    words = np.zeros((8, 16 + 16), np.uint8)
    words = words.reshape(-1)[(-words.ctypes.data) % 16:][:8 * 16].reshape(8, 16)             # a 16-byte aligned host view
    pix, adv = np.zeros((1, 2, 4, 4), np.uint8), np.ones((1, 2), np.uint8)
    style, out = np.zeros(2, R.STYLE_DTYPE), np.full((2, 1, 4, 4), 5, F)
    tg, te = np.full((2, 3), 9, np.int32), np.full((2, 3), 9, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(n=2, H=4, W=4, L=3, stride=16, n_words=8, lex=True, atlas=True, faces=1, glyphs=2, gh=4, gw=4, pixels=p(pix), advance=p(adv),
             sty=p(style), o=p(out), t=p(tg), e=p(te), wptr=words.ctypes.data):
        ld = LexiconDesc(C.c_void_p(wptr), n_words, stride)
        ad = GlyphAtlasDesc(pixels, advance, faces, glyphs, gh, gw)
        return aocr.lib.aocr_synth_lines(None, C.byref(ld) if lex else None, C.byref(ad) if atlas else None, sty, n, H, W, L, o, t, e)

    for kw, what in ((dict(H=0), "H=0"), (dict(W=0), "W=0"), (dict(L=0), "L=0"), (dict(n=-1), "n_images=-1"), (dict(n=65536), "65535"),
                     (dict(stride=24), "stride 24"), (dict(stride=0), "stride 0"), (dict(stride=272), "stride 272"),
                     (dict(wptr=words.ctypes.data + 1), "16-byte aligned"), (dict(n_words=-1), "n_words=-1"),
                     (dict(lex=False), "lexicon is NULL"), (dict(atlas=False), "atlas is NULL"), (dict(faces=0), "n_faces=0"),
                     (dict(glyphs=0), "n_glyphs=0"), (dict(glyphs=253), "n_glyphs=253"), (dict(gh=0), "gh=0"), (dict(gh=65), "gh=65"),
                     (dict(gw=0), "gw=0"), (dict(gw=65), "gw=65"), (dict(pixels=None), "pixels_dev"), (dict(advance=None), "advance_dev"),
                     (dict(sty=None), "NULL"), (dict(o=None), "NULL"), (dict(t=None), "together"), (dict(e=None), "together")):
        assert call(**kw) != 0, kw
        assert what in aocr.last_error(), (kw, aocr.last_error())
    assert (out == 5).all() and (tg == 9).all() and (te == 9).all()
    assert call(n=0) == 0 and call(n=0, t=None, e=None) == 0                       # n_images == 0: a no-op, no launch
