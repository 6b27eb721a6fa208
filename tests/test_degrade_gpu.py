"""Scan degradation, GPU side: aocr_degrade_lines against the numpy restatement tests/degrade_ref.py bit for bit (every float op of the
kernel is one rounded single-precision op in the restatement's order; the restatement works on whole images, so a tile seam or a border
handled differently by a tile shows), the identity, the empty batch, reproducibility, the bad record, and the stage inside
aocr.Augmenter(degrade=...) and aocr.SynthGen."""
import numpy as np
import pytest
import torch

import augment_ref as AR
import degrade_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
EVERYTHING = dict(blur_sigma=1.4, thickness=0.9, elastic=(2.5, 1.5), pitch=8, fill=240.0)


def _image(n, H, W, seed):
    """dark strokes on light paper with some texture: every stage has something to act on."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(200, 255, (n, 1, H, W))
    x[rng.uniform(size=x.shape) < 0.2] = 20.0
    x[..., H // 3, :] = 0.0
    x[..., :, W // 2] = 5.0
    return x.astype(F)


def _run(x, rec, seed=0, counter=0):
    """aocr_degrade_lines on a host (n,1,H,W) float32 array and a structured array of aocr_degrade records."""
    import aocr
    n, _, H, W = x.shape
    xd = torch.from_numpy(x).cuda()
    rd = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    out = torch.full_like(xd, -7.0)
    st = torch.cuda.current_stream().cuda_stream
    aocr.check(aocr.lib.aocr_degrade_lines(st, aocr.ptr(xd), aocr.ptr(rd), n, H, W, seed, counter, aocr.ptr(out)), "aocr_degrade_lines")
    return out.cpu().numpy()


def _same(got, ref, what):
    bad = got != ref
    print(f"[parity] degrade {what}: {got.shape}, {int(bad.sum())} of {bad.size} values differ"
          + (f", max |diff| {np.abs(got - ref).max():.3g} first at {tuple(np.argwhere(bad)[0])}" if bad.any() else ""))
    assert np.array_equal(got, ref), what


def test_one_stage_per_image_matches_restatement_bitwise(cuda):
    x = _image(3, 32, 100, 1)
    rec = R.records([R.record(amp=(3.0, 2.0), pitch=8, fill=128.0), R.record(thick=0.7), R.record(taps=R.gauss_taps(1.3))])
    got, ref = _run(x, rec, seed=77, counter=2), R.degrade(x, rec, seed=77, counter=2)
    _same(got, ref, "elastic | stroke | blur")
    assert all(not np.array_equal(got[i], x[i]) for i in range(3))


def test_everything_on_odd_sizes_matches_restatement_bitwise(cuda):
    """37 x 131: two tiles down and three across, neither a multiple of the tile; image 1 thins."""
    x = _image(2, 37, 131, 2)
    rec = R.records([R.record(amp=(2.5, 1.5), pitch=8, thick=0.6, taps=R.gauss_taps(1.5), fill=240.0),
                     R.record(amp=(1.0, 3.0), pitch=5, thick=-0.8, taps=R.gauss_taps(0.8), fill=10.0)])
    _same(_run(x, rec, seed=5, counter=9), R.degrade(x, rec, seed=5, counter=9), "everything on")


def test_image_smaller_than_a_cell_and_than_the_halo(cuda):
    x = _image(1, 5, 7, 3)
    rec = R.records([R.record(amp=(1.5, 1.0), pitch=8, thick=0.5, taps=R.gauss_taps(1.2), fill=200.0)])
    _same(_run(x, rec, seed=1, counter=1), R.degrade(x, rec, seed=1, counter=1), "5 x 7")


@pytest.mark.parametrize("pitch", [2, 13])
def test_smallest_pitch_and_one_that_divides_nothing(cuda, pitch):
    x = _image(1, 32, 64, 4)
    rec = R.records([R.record(amp=(2.0, 2.0), pitch=pitch, thick=-0.4, taps=R.gauss_taps(1.0))])
    _same(_run(x, rec, seed=8, counter=pitch), R.degrade(x, rec, seed=8, counter=pitch), f"pitch {pitch}")


def test_identity_returns_the_input_bitwise(cuda):
    x = np.random.default_rng(1).uniform(0, 255, (3, 1, 32, 256)).astype(F)
    got = _run(x, R.records([R.record(fill=9.0), R.record(pitch=2), R.record(pitch=13)]), seed=11, counter=5)
    np.testing.assert_array_equal(got, x)


def test_empty_batch_is_a_no_op(cuda):
    import aocr
    xd = torch.zeros(16, device="cuda")
    out = torch.full((16,), 3.0, device="cuda")
    rd = torch.zeros(44, dtype=torch.uint8, device="cuda")
    assert aocr.lib.aocr_degrade_lines(None, aocr.ptr(xd), aocr.ptr(rd), 0, 4, 4, 0, 0, aocr.ptr(out)) == 0
    torch.cuda.synchronize()
    assert (out == 3.0).all()


def test_same_seed_and_counter_same_pixels(cuda):
    import aocr
    D = aocr.Degrader(seed=99, **EVERYTHING)
    x = torch.from_numpy(_image(4, 32, 100, 5)).cuda()
    a = D.apply(x, 0)
    assert torch.equal(D.apply(x, 0), a)
    assert not torch.equal(D.apply(x, 1), a)
    assert not torch.equal(aocr.Degrader(seed=100, **EVERYTHING).apply(x, 0), a)
    assert torch.equal(aocr.Degrader().apply(x, 0), x)                          # the default is the identity
    rec = D.params(4, 32, 100, 0)
    # the same records under another counter of the device field alone: only the elastic stage reads (seed, counter) on the device
    b, c = _run(x.cpu().numpy(), rec, seed=99, counter=0), _run(x.cpu().numpy(), rec, seed=99, counter=1)
    np.testing.assert_array_equal(b, a.cpu().numpy())
    assert not np.array_equal(b, c)


def test_bad_pitch_is_an_error_and_launches_nothing(cuda):
    """pitch is part of the record, and the record is device memory by the time the C call runs: the host wrapper every record goes through
    refuses it before anything is uploaded or enqueued, bad sizes fail in the C call itself, and a record that reaches the kernel all the same
    leaves its image unwritten."""
    import aocr
    x = _image(2, 8, 16, 6)
    xd = torch.from_numpy(x).cuda()
    for pitch in (1, 0, -3):
        rec = R.records([R.record(), R.record()])
        rec["pitch"][1] = pitch
        with pytest.raises(ValueError, match="pitch"):
            aocr.degrade.degrade_lines(xd, rec, 0, 0)
        got = _run(x, rec)                                                      # _run pre-fills the output with -7
        np.testing.assert_array_equal(got[0], x[0])
        assert (got[1] == -7.0).all()
    with pytest.raises(ValueError, match="pitch"):
        aocr.Degrader(pitch=1)
    out = torch.full_like(xd, -7.0)
    rd = torch.from_numpy(R.records([R.record()] * 2).view(np.uint8).copy()).cuda()
    assert aocr.lib.aocr_degrade_lines(None, aocr.ptr(xd), aocr.ptr(rd), 2, 0, 16, 0, 0, aocr.ptr(out)) != 0 and "bad sizes" in aocr.last_error()
    assert aocr.lib.aocr_degrade_lines(None, aocr.ptr(xd), aocr.ptr(rd), 2, 8, 16, 0, 0, aocr.ptr(xd)) != 0 and "alias" in aocr.last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all()


def test_augmenter_runs_the_degrader_first(cuda):
    import aocr
    D = aocr.Degrader(seed=21, **EVERYTHING)
    jitter = dict(rotate_deg=6, shear=0.1, scale=1.15, translate=(4, 2), contrast=1.4, brightness=10, noise=9, seed=31)
    A, plain = aocr.Augmenter(degrade=D, **jitter), aocr.Augmenter(**jitter)
    x = _image(4, 32, 100, 7)
    xd = torch.from_numpy(x).cuda()
    warp = plain.params(4, 32, 100, 3)
    assert A.params(4, 32, 100, 3).tobytes() == warp.tobytes()                  # the warp records do not know about the degrader
    got = A.apply(xd, 3).cpu().numpy()
    ref = AR.augment(R.degrade(x, D.params(4, 32, 100, 3), seed=21, counter=3), warp, seed=31, counter=3)
    _same(got, ref, "Augmenter(degrade=)")
    # without degrade: the bits of before
    _same(plain.apply(xd, 3).cpu().numpy(), AR.augment(x, warp, seed=31, counter=3), "Augmenter()")
    assert not np.array_equal(got, plain.apply(xd, 3).cpu().numpy())


def test_synthgen_with_a_degrader_is_reproducible(cuda):
    import aocr
    lex, atlas = aocr.Lexicon(["a", "hello", "w0rld", "il1", "quick", "zebra9", "m", "0123456"]), aocr.GlyphAtlas.default()
    A = aocr.Augmenter(seed=31, noise=6, degrade=aocr.Degrader(seed=4, **EVERYTHING))
    g = aocr.SynthGen(lex, atlas, width=100, seed=5, epoch_size=64, augment=A)
    p = aocr.SynthGen(lex, atlas, width=100, seed=5, epoch_size=64, augment=aocr.Augmenter(seed=31, noise=6))
    first, second, plain = g.next_device(4), g.next_device(4), p.next_device(4)
    assert first[0].shape == (4, 1, 32, 100) and g.augment_counter == 2
    assert not torch.equal(first[0], second[0]) and not torch.equal(first[0], plain[0])
    assert torch.equal(first[1], plain[1])                                      # the targets do not move
    g.synth_counter = g.augment_counter = 0                                     # a resumed run restores the counters
    again = g.next_device(4)
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    img = first[0].cpu().numpy()
    assert img.min() >= 0 and img.max() <= 255
