"""Training augmentation, GPU side: aocr_augment_lines against the numpy restatement tests/augment_ref.py bit for bit (every float
op of the kernel is one rounded single-precision op in the restatement's order), against hand answers that do not use the
restatement, the statistics and the reproducibility of the noise field, and aocr.DataGen(augment=...) end to end."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
JITTER = dict(rotate_deg=8, shear=0.2, scale=1.2, translate=(6, 2), contrast=1.5, brightness=20, noise=12)


def _run(x, warp, seed=0, counter=0):
    """aocr_augment_lines on a host (n,1,H,W) float32 array and a structured array of aocr_warp records."""
    import aocr
    n, _, H, W = x.shape
    xd = torch.from_numpy(x).cuda()
    wd = torch.from_numpy(warp.view(np.uint8).copy()).cuda()
    out = torch.full_like(xd, -7.0)
    st = torch.cuda.current_stream().cuda_stream
    aocr.check(aocr.lib.aocr_augment_lines(st, aocr.ptr(xd), aocr.ptr(wd), n, H, W, seed, counter, aocr.ptr(out)), "aocr_augment_lines")
    return out.cpu().numpy()


@pytest.mark.parametrize("H,W", [(32, 32), (32, 100), (8, 5)])
def test_augment_matches_restatement_bitwise(cuda, H, W):
    import aocr
    A = aocr.Augmenter(seed=4242, **JITTER)
    x = np.random.default_rng(H * 1000 + W).integers(0, 256, (8, 1, H, W)).astype(F)
    warp = A.params(8, H, W, counter=3)
    # image 6: a NaN matrix entry in the x row; its y row is the identity, so that the y interpolation is 1*fill + 0*fill
    warp[6]["m00"] = np.nan
    warp[6]["m10"], warp[6]["m11"], warp[6]["m12"] = 0.0, 1.0, 0.0
    # image 7: maps entirely outside the source
    warp[7]["m00"], warp[7]["m01"], warp[7]["m02"] = 1.0, 0.0, W + 3.5
    got = _run(x, warp, seed=A.seed, counter=3)
    ref = R.augment(x, warp, seed=A.seed, counter=3)
    np.testing.assert_array_equal(got, ref)
    assert not np.array_equal(got[:6], x[:6])
    tri = R.noise_field(8, H, W, A.seed, 3)
    for i in (6, 7):
        w = warp[i]
        flat = np.clip((w["gain"] * w["fill"] + w["offset"]) + w["noise"] * tri[i], F(0), F(255))
        assert flat.dtype == np.float32
        if i == 6:
            np.testing.assert_array_equal(got[i, 0], flat, err_msg="NaN record")
        else:       # its y row still blends fill with fill at a fractional weight: three roundings at 255 (ulp 1.5e-5), times gain <= 1.5
            np.testing.assert_allclose(got[i, 0], flat, rtol=0, atol=1e-4, err_msg="outside record")
    print(f"[parity] augment {H}x{W}: 8 images bit-identical to the restatement")


def test_identity_returns_the_input_bitwise(cuda):
    x = np.random.default_rng(1).uniform(0, 255, (3, 1, 32, 256)).astype(F)
    got = _run(x, R.warp_records([R.identity(9.0)] * 3), seed=11, counter=5)
    np.testing.assert_array_equal(got, x)


def test_integer_shift_known_answer(cuda):
    x = np.random.default_rng(2).integers(0, 256, (2, 1, 6, 11)).astype(F)
    got = _run(x, R.warp_records([(1, 0, 3, 0, 1, 0, 1, 0, 200.0, 0)] * 2))
    want = np.full_like(x, 200.0)
    want[..., :-3] = x[..., 3:]
    np.testing.assert_array_equal(got, want)
    # a vertical shift the other way, more than one block per image, a width that is no multiple of the block
    x = np.random.default_rng(3).integers(0, 256, (2, 1, 32, 37)).astype(F)
    got = _run(x, R.warp_records([(1, 0, 0, 0, 1, -2, 1, 0, 17.0, 0)] * 2))
    want = np.full_like(x, 17.0)
    want[..., 2:, :] = x[..., :-2, :]
    np.testing.assert_array_equal(got, want)


def test_empty_batch_is_a_no_op(cuda):
    import aocr
    xd = torch.zeros(16, device="cuda")
    out = torch.full((16,), 3.0, device="cuda")
    wd = torch.zeros(40, dtype=torch.uint8, device="cuda")
    assert aocr.lib.aocr_augment_lines(None, aocr.ptr(xd), aocr.ptr(wd), 0, 4, 4, 0, 0, aocr.ptr(out)) == 0
    torch.cuda.synchronize()
    assert (out == 3.0).all()


def test_noise_statistics_and_reproducibility(cuda):
    import aocr
    A = aocr.Augmenter(noise=20, seed=99)
    x = torch.full((8, 1, 32, 128), 128.0, device="cuda")
    a = A.apply(x, 0).cpu().numpy().astype(np.float64)
    assert a.min() > 128 - 20 and a.max() < 128 + 20                            # nothing clamps
    mean, var = a.mean(), a.var(ddof=1)
    print(f"[noise] mean {mean:.4f} (128), variance {var:.3f} ({400 / 6:.3f})")
    assert abs(mean - 128.0) < 0.5
    assert abs(var - 400.0 / 6.0) < 0.05 * 400.0 / 6.0
    b = A.apply(x, 1).cpu().numpy()
    assert not np.array_equal(a, b)
    np.testing.assert_array_equal(A.apply(x, 0).cpu().numpy(), a.astype(F))
    assert not np.array_equal(aocr.Augmenter(noise=20, seed=100).apply(x, 0).cpu().numpy(), a.astype(F))


def test_apply_rejects_host_tensors(cuda):
    import aocr
    with pytest.raises(ValueError, match="device tensor"):
        aocr.Augmenter().apply(torch.zeros(1, 1, 32, 32), 0)


def test_datagen_augments_every_batch(cuda, tmp_path):
    import aocr
    rng = np.random.default_rng(5)
    with open(tmp_path / "l.txt", "w") as f:
        for i in range(8):
            np.save(tmp_path / f"a{i}.npy", rng.integers(0, 256, (32, 120), dtype=np.uint8))
            f.write(f"a{i}.npy ab{i}\n")
    A = aocr.Augmenter(seed=31, **JITTER)
    g = aocr.DataGen(str(tmp_path), "l.txt", 8.0, augment=A)
    p = aocr.DataGen(str(tmp_path), "l.txt", 8.0)
    seen = []
    for epoch in range(2):
        for k in range(2):
            b, r = g.nextBatch(4), p.nextBatch(4)
            counter = 2 * epoch + k
            assert b[0].shape == r[0].shape == (4, 1, 32, 100)
            assert torch.equal(b[0], A.apply(r[0], counter)), f"batch {counter}"
            assert not torch.equal(b[0], r[0])
            np.testing.assert_array_equal(b[1], r[1]); np.testing.assert_array_equal(b[2], r[2])
            assert b[3] == r[3] and b[4] == r[4]
            seen.append(b)
        assert g.nextBatch(4) is None and p.nextBatch(4) is None
    assert g.augment_counter == 4 and p.augment_counter == 0
    assert not torch.equal(seen[0][0], seen[2][0]) and not torch.equal(seen[1][0], seen[3][0])      # second pass: other pixels
    g.augment_counter = 1                                                        # a resumed run sets the counter
    assert torch.equal(g.nextBatch(4)[0], A.apply(p.nextBatch(4)[0], 1))
    m = aocr.Model().create(dict(encoder_num_hidden=32, encoder_num_layers=1, decoder_num_layers=2, input_feed=True, batch_size=4,
                                 max_img_w=100, max_decoder_l=8, max_beam=1, learning_rate=0.1, seed=1))
    loss, stats = m.step(seen[0], forward_only=False)
    assert np.isfinite(loss) and stats[0] == seen[0][3]
    m.shutdown()
