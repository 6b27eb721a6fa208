"""Synthetic word lines, GPU side: aocr_synth_lines against the numpy restatement tests/synth_ref.py bit for bit (every float op of the
kernel is one rounded single-precision op in the restatement's order), against hand answers that do not use the restatement, the no-op
and NULL-target conventions, reproducibility, and aocr.SynthGen end to end through a train step."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
N_GLYPHS = 9                                                    # ids 4..12 have a glyph, id 13 is beyond the atlas
WORDS = ["a", "hello", "w0rld", "il1", "quick", "zebra9", "m", "0123456"]


def _run(words, pixels, advance, style, H, W, L=None, n=None, out=None, tg=None, te=None):
    """aocr_synth_lines on host arrays; returns (images, targets, targets_eval) as numpy (targets None without L)."""
    import aocr
    from aocr._lib import GlyphAtlasDesc, LexiconDesc
    n = len(style) if n is None else n
    wd, pd, ad = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (words, pixels, advance))
    sd = torch.from_numpy(style.view(np.uint8).copy()).cuda()
    out = torch.full((len(style), 1, H, W), -7.0, device="cuda") if out is None else out
    if L is not None and tg is None:
        tg, te = torch.full((len(style), L), -7, dtype=torch.int32, device="cuda"), torch.full((len(style), L), -7, dtype=torch.int32, device="cuda")
    ld = LexiconDesc(aocr.ptr(wd), words.shape[0], words.shape[1])
    gd = GlyphAtlasDesc(aocr.ptr(pd), aocr.ptr(ad), *pixels.shape)
    st = torch.cuda.current_stream().cuda_stream
    aocr.check(aocr.lib.aocr_synth_lines(st, C.byref(ld), C.byref(gd), aocr.ptr(sd), n, H, W, L or 1, aocr.ptr(out), aocr.ptr(tg), aocr.ptr(te)),
               "aocr_synth_lines")
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if tg is None else tg.cpu().numpy(), None if te is None else te.cpu().numpy()


def _case(H, W, gh, gw, stride):
    """lexicon, atlas and the 8 records of one case: together they take every branch of the kernel."""
    pixels, advance = R.counter_atlas(2, N_GLYPHS, gh, gw, seed=H + W + stride)
    assert (advance == 0).any() and (advance > 0).any()
    full = [4 + k % N_GLYPHS for k in range(stride - 1)]                                      # stride-1 ids: no 0 before the row's last byte
    words = R.pack([[], [5], full, [4, 4 + N_GLYPHS, 3, 6, 200, 8], [7, 8, 9, 10]], stride)
    ry = gh / H
    style = R.style_records([
        (0, 0, 0.5, 1.0, ry, 0.0, 0.0, 10.0, 240.0),                                           # the empty row
        (1, 1, -3.0, 0.3, 0.4 * ry, W / 2 + 0.25, -1.5, 30.0, 220.0),                          # one id, enlarged, runs past W; spacing < 0
        (2, 0, np.nan, 3.0, 0.9 * ry, 1.5, 0.75, 0.0, 255.0),                                  # stride-1 ids, shrunk; NaN spacing
        (3, 1, 1.5, 0.77, 1.3 * ry, -7.5, 1.5, 250.0, 20.0),                                   # ids beyond the atlas and below 4; starts left of 0
        (-1, 0, 0.0, 1.0, ry, 0.0, 0.0, 0.0, 200.0),                                           # word = -1
        (5, 0, 0.0, 1.0, ry, 0.0, 0.0, 0.0, 190.0),                                            # word = n_words
        (4, 2, 0.0, 1.0, ry, 0.0, 0.0, 0.0, 180.0),                                            # face out of range
        (4, 1, 0.0, 1.0, ry, np.nan, 0.0, 0.0, 170.0),                                         # NaN x0
    ])
    return words, pixels, advance, style


@pytest.mark.parametrize("stride", [16, 32])
@pytest.mark.parametrize("gh,gw", [(32, 24), (8, 5)])
@pytest.mark.parametrize("H,W", [(32, 100), (32, 37), (8, 5)])
def test_synth_matches_restatement_bitwise(cuda, H, W, gh, gw, stride):
    words, pixels, advance, style = _case(H, W, gh, gw, stride)
    ref = R.synth(words, pixels, advance, style, H, W)
    for L in (stride, 3):                                                                     # n_max + 1, and one that cuts words
        got, tg, te = _run(words, pixels, advance, style, H, W, L)
        np.testing.assert_array_equal(got, ref)
        rt, re_ = R.targets(words, style, 2, L)
        np.testing.assert_array_equal(tg, rt); np.testing.assert_array_equal(te, re_)
    assert rt[2].tolist() == [2, 4, 5] and re_[1].tolist() == [5, 3, 1] and re_[6].tolist() == [3, 1, 1]
    for i, bg in ((0, 240), (4, 200), (5, 190), (6, 180), (7, 170)):
        assert (got[i] == bg).all(), i                                                        # paper only
    for i in (1, 2, 3):
        assert len(np.unique(got[i])) > 2, i                                                  # ink, blended
    print(f"[parity] synth {H}x{W} atlas {gh}x{gw} stride {stride}: 8 images and 2 x 2 target arrays bit-identical to the restatement")


def test_identity_and_shift_known_answers(cuda):
    pixels, advance = R.blit_atlas()
    gh = R.BLIT_GH
    lists = [[4, 5, 6, 8], [7, 7, 4], [8]]
    words = R.pack(lists)
    for W in (24, 9):
        got, _, _ = _run(words, pixels, advance, R.style_records([R.identity(w) for w in range(3)]), gh, W)
        for w, ids in enumerate(lists):
            np.testing.assert_array_equal(got[w, 0], R.side_by_side(pixels, advance, ids, W), err_msg=f"word {w} W {W}")
    # more than one workgroup per image, a width that is no multiple of anything: H * W = 40 * 37 > 1024
    got, _, _ = _run(words, pixels, advance, R.style_records([R.identity(1)]), 40, 37)
    np.testing.assert_array_equal(got[0, 0], R.side_by_side(pixels, advance, lists[1], 37, H=40))
    H, W = gh + 3, 16
    got, _, _ = _run(R.pack([[6, 4]]), pixels, advance, R.style_records([(0, 0, 1.0, 1.0, 1.0, 3.0, 2.0, 200.0, 40.0)]), H, W)
    ink = np.zeros((H, W), bool)
    ink[2:2 + gh, 3:3 + 5] = pixels[0, 2, :, :5] == 255
    ink[2:2 + gh, 9:9 + 3] = pixels[0, 0, :, :3] == 255                                       # 3 + 5 + one pixel of spacing
    np.testing.assert_array_equal(got[0, 0], np.where(ink, F(200), F(40)))


def test_empty_batch_and_null_targets_leave_buffers_untouched(cuda):
    words, pixels, advance, style = _case(8, 5, 8, 5, 16)
    out = torch.full((8, 1, 8, 5), 3.0, device="cuda")
    tg, te = torch.full((8, 4), 11, dtype=torch.int32, device="cuda"), torch.full((8, 4), 12, dtype=torch.int32, device="cuda")
    _run(words, pixels, advance, style, 8, 5, 4, n=0, out=out, tg=tg, te=te)
    assert (out == 3.0).all() and (tg == 11).all() and (te == 12).all()
    got, none_t, none_e = _run(words, pixels, advance, style, 8, 5, out=out)                  # NULL targets: only the images are written
    assert none_t is None and none_e is None and (tg == 11).all() and (te == 12).all()
    np.testing.assert_array_equal(got, R.synth(words, pixels, advance, style, 8, 5))


def test_two_calls_return_identical_bits(cuda):
    words, pixels, advance, style = _case(32, 100, 32, 24, 32)
    a, b = _run(words, pixels, advance, style, 32, 100, 32), _run(words, pixels, advance, style, 32, 100, 32)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_synthgen_end_to_end(cuda):
    import aocr
    from aocr.data import str2numlist
    lex, atlas = aocr.Lexicon(WORDS), aocr.GlyphAtlas.default()
    A = aocr.Augmenter(seed=31, rotate_deg=4, scale=1.1, translate=(3, 1), contrast=1.3, noise=6)
    g, h = aocr.SynthGen(lex, atlas, width=100, seed=5, epoch_size=8), aocr.SynthGen(lex, atlas, width=100, seed=5, epoch_size=8)
    a = aocr.SynthGen(lex, atlas, width=100, seed=5, epoch_size=8, augment=A)
    assert g.size() == 8
    first = g.nextBatch(4)
    images, tg, te, nnz, words = first
    assert images.shape == (4, 1, 32, 100) and images.dtype == torch.float32 and images.is_cuda
    img = images.cpu().numpy()
    assert img.min() >= 0 and img.max() <= 255 and all(len(np.unique(i)) > 8 for i in img)    # anti-aliased ink on paper
    lists = [str2numlist(w) for w in words]                                                   # DataGen._emit's rule for these words
    assert nnz == sum(len(l) - 1 for l in lists) and tg.shape == te.shape == (4, max(len(l) for l in lists) - 1)
    for i, l in enumerate(lists):
        assert tg[i, :len(l) - 1].tolist() == l[:-1] and te[i, :len(l) - 1].tolist() == l[1:]
        assert (tg[i, len(l) - 1:] == 1).all() and (te[i, len(l) - 1:] == 1).all()
    dev = h.next_device(4)                                                                    # same (seed, counter): same batch, device targets
    assert torch.equal(dev[0], images)
    np.testing.assert_array_equal(dev[1].cpu().numpy(), tg); np.testing.assert_array_equal(dev[2].cpu().numpy(), te)
    assert dev[1].dtype == torch.int32 and dev[1].is_cuda
    second = g.nextBatch(4)
    assert not torch.equal(second[0], images)                                                 # another counter: other pixels
    assert g.nextBatch(4) is None and g.synth_counter == 2
    g.synth_counter = 0                                                                       # a resumed run sets the counter
    again = g.nextBatch(4)
    assert torch.equal(again[0], images) and again[4] == words
    for k, plain in enumerate((first, second)):                                               # augment=A: A.apply(plain, counter)
        b = a.nextBatch(4)
        assert torch.equal(b[0], A.apply(plain[0], k)) and not torch.equal(b[0], plain[0])
        np.testing.assert_array_equal(b[1], plain[1]); assert b[3] == plain[3] and b[4] == plain[4]
    assert a.augment_counter == 2 and g.augment_counter == 0
    m = aocr.Model().create(dict(encoder_num_hidden=32, encoder_num_layers=1, decoder_num_layers=2, input_feed=True, batch_size=4,
                                 max_img_w=100, max_decoder_l=8, max_beam=1, learning_rate=0.1, seed=1))
    loss, stats = m.step(first, forward_only=False)
    assert np.isfinite(loss) and stats[0] == first[3]
    m.shutdown()
