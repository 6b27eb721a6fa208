"""Scan degradation, host side: known answers of the numpy restatement tests/degrade_ref.py (what the GPU tests compare the kernel with),
the records aocr.Degrader draws, and the argument errors of the C call that need no device."""
import ctypes as C

import numpy as np
import pytest

import degrade_ref as R

F = np.float32


def _dot(H=11, W=13, y=5, x=6, paper=255.0, ink=0.0):
    img = np.full((1, 1, H, W), paper, F)
    img[0, 0, y, x] = ink
    return img


def test_ref_identity_record_returns_the_input():
    x = np.random.default_rng(0).uniform(0, 255, (2, 1, 9, 21)).astype(F)
    np.testing.assert_array_equal(R.degrade(x, R.records([R.record(fill=3.0), R.record(pitch=2)]), seed=5, counter=7), x)


def test_ref_impulse_under_blur_is_the_outer_product_of_the_taps():
    taps = R.gauss_taps(1.2)
    img = _dot(paper=0.0, ink=1.0)                                              # far enough from every edge: nothing clamps
    got = R.degrade(img, R.records([R.record(taps=taps)]))[0, 0]
    full = np.array(taps[:0:-1] + taps, F)                                      # w4..w1 w0 w1..w4
    want = np.zeros_like(got)
    want[1:10, 2:11] = np.outer(full, full)                                     # (w_j * 1) * w_i: one rounded product each, as the two passes form it
    np.testing.assert_array_equal(got, want)
    assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-6


def test_ref_stroke_weight_known_answers():
    thick = R.degrade(_dot(), R.records([R.record(thick=1.0)]))[0, 0]
    want = np.full((11, 13), 255.0, F)
    want[4:7, 5:8] = 0.0                                                        # one dark pixel becomes a 3x3 block
    np.testing.assert_array_equal(thick, want)
    thin = R.degrade(_dot(), R.records([R.record(thick=-1.0)]))[0, 0]
    np.testing.assert_array_equal(thin, np.full((11, 13), 255.0, F))            # and vanishes under the maximum
    half = R.degrade(_dot(), R.records([R.record(thick=0.5)]))[0, 0]
    assert half[5, 6] == 0.0 and half[4, 5] == 127.5 and half[3, 6] == 255.0


@pytest.mark.parametrize("pitch", [2, 3, 8, 13, 1000])
def test_ref_zero_amplitude_is_the_identity_at_any_pitch(pitch):
    x = np.random.default_rng(pitch).uniform(0, 255, (1, 1, 17, 29)).astype(F)
    np.testing.assert_array_equal(R.degrade(x, R.records([R.record(pitch=pitch)]), seed=1, counter=2), x)


def test_ref_elastic_moves_pixels_by_at_most_the_amplitude_and_is_seeded():
    x = np.zeros((1, 1, 32, 64), F)
    x[0, 0, :, 32:] = 255.0                                                     # a vertical edge: only dx shows
    rec = R.records([R.record(amp=(2.0, 0.0), pitch=8)])
    a = R.degrade(x, rec, seed=3, counter=0)[0, 0]
    assert not np.array_equal(a, x[0, 0])
    # |dx| <= 2 and one more pixel of bilinear support; a blend of 255 with 255 at a fractional weight is three roundings at 255 (ulp 1.5e-5)
    # (columns within 3 of the left border may pull in `fill`)
    assert (a[:, 3:29] == 0).all() and (np.abs(a[:, 35:] - 255.0) < 1e-4).all()
    np.testing.assert_array_equal(R.degrade(x, rec, seed=3, counter=0)[0, 0], a)
    assert not np.array_equal(R.degrade(x, rec, seed=3, counter=1)[0, 0], a)
    dx, _ = R.node_field(0, 32, 64, 8, 2.0, 0.0, 3, 0)
    assert dx.shape == (5, 9) and np.abs(dx).max() <= 2.0 and len(np.unique(dx)) > 40


def test_degrader_default_is_the_identity_record():
    import aocr
    p = aocr.Degrader().params(3, 32, 100, counter=4)
    assert p.dtype == R.DEGRADE_DTYPE and p.dtype.itemsize == 44 == C.sizeof(aocr.degrade.Degrade)
    assert p.tobytes() == R.records([R.record()] * 3).tobytes()
    assert not np.signbit(p["thick"]).any()
    for name in p.dtype.names:                                                  # the ctypes mirror and the dtype lay the record out alike
        assert getattr(aocr.degrade.Degrade, name).offset == p.dtype.fields[name][1], name


def test_degrader_params_are_a_pure_function_of_seed_and_counter():
    import aocr
    kw = dict(blur_sigma=1.5, thickness=0.8, elastic=(2.0, 1.0), pitch=6, fill=200.0)
    a = aocr.Degrader(seed=7, **kw).params(16, 32, 100, 3)
    assert a.tobytes() == aocr.Degrader(seed=7, **kw).params(16, 32, 100, 3).tobytes()
    assert a.tobytes() != aocr.Degrader(seed=7, **kw).params(16, 32, 100, 4).tobytes()
    assert a.tobytes() != aocr.Degrader(seed=8, **kw).params(16, 32, 100, 3).tobytes()
    assert a[:8].tobytes() == aocr.Degrader(seed=7, **kw).params(8, 64, 9, 3).tobytes()         # image i's record: its own four uniforms only
    u = aocr.synth.counter_uniform(7, aocr.degrade.PARAM_STREAM + 3, 64).reshape(16, 4)
    np.testing.assert_array_equal(a["thick"], ((2 * u[:, 1] - 1) * 0.8).astype(F))
    np.testing.assert_array_equal(a["amp_x"], (u[:, 2] * 2.0).astype(F))
    np.testing.assert_array_equal(a["amp_y"], (u[:, 3] * 1.0).astype(F))
    assert (a["pitch"] == 6).all() and (a["inv_pitch"] == F(1.0 / 6)).all() and (a["fill"] == 200).all()
    assert (np.abs(a["thick"]) <= 0.8).all() and (a["thick"] > 0).any() and (a["thick"] < 0).any()
    sigma = u[:, 0] * 1.5
    for i in range(16):
        k = np.arange(5, dtype=np.float64)
        w = np.exp(-k * k / (2 * sigma[i] ** 2))
        np.testing.assert_array_equal(a["taps"][i], (w / (w[0] + 2 * w[1:].sum())).astype(F))


def test_degrader_taps_sum_to_one():
    import aocr
    p = aocr.Degrader(blur_sigma=1.5, seed=11).params(256, 32, 100, 0)
    t = p["taps"].astype(np.float64)
    s = t[:, 0] + 2.0 * t[:, 1:].sum(axis=1)
    assert np.abs(s - 1.0).max() <= 2.0 ** -23                                  # the float64 sum is 1; five casts move it by less than one fp32 ulp
    assert (np.diff(p["taps"], axis=1) <= 0).all() and (p["taps"] >= 0).all()
    np.testing.assert_array_equal(aocr.degrade.blur_taps([0.0, 5e-324])[:, :], [[1, 0, 0, 0, 0]] * 2)


def test_degrader_stream_is_not_the_augmenters():
    import aocr
    assert aocr.degrade.PARAM_STREAM != aocr.augment.PARAM_STREAM
    for counter in (0, 1, 12345):
        d = aocr.synth.counter_uniform(9, aocr.degrade.PARAM_STREAM + counter, 64)
        a = aocr.synth.counter_uniform(9, aocr.augment.PARAM_STREAM + counter, 64)
        assert not np.intersect1d(d, a).size


def test_degrader_argument_errors():
    import aocr
    with pytest.raises(ValueError, match="four taps"):
        aocr.Degrader(blur_sigma=1.6)
    for bad in (dict(blur_sigma=-0.1), dict(thickness=1.01), dict(thickness=-1.01), dict(thickness=float("nan")), dict(pitch=1), dict(pitch=0),
                dict(pitch=2.5), dict(elastic=(-1, 0)), dict(elastic=(0, -0.5))):
        with pytest.raises(ValueError):
            aocr.Degrader(**bad)
    aocr.Degrader(blur_sigma=1.5, thickness=-1, pitch=2, elastic=(0, 3))
    with pytest.raises(TypeError):
        aocr.Augmenter(degrade="blur")
    assert aocr.Augmenter().degrade is None


def test_c_call_rejects_bad_arguments_before_any_launch():
    """sizes, NULL and aliasing go through the usual error path: a status, a message, nothing enqueued (there is no device here to enqueue on)."""
    import aocr
    a, b, r = (C.c_float * 4)(), (C.c_float * 4)(), (C.c_char * 44)()
    pa, pb, pr = C.addressof(a), C.addressof(b), C.addressof(r)
    call = aocr.lib.aocr_degrade_lines
    assert call(None, pa, pr, 1, 0, 4, 0, 0, pb) != 0 and "bad sizes" in aocr.last_error()
    assert call(None, pa, pr, 1, 4, 0, 0, 0, pb) != 0 and "bad sizes" in aocr.last_error()
    assert call(None, pa, pr, -1, 2, 2, 0, 0, pb) != 0 and "bad sizes" in aocr.last_error()
    assert call(None, pa, pr, 1, 16385, 2, 0, 0, pb) != 0 and "bad sizes" in aocr.last_error()
    assert call(None, pa, pr, 65536, 2, 2, 0, 0, pb) != 0 and "65535" in aocr.last_error()
    assert call(None, pa, pr, 1, 2, 2, 0, 0, pa) != 0 and "alias" in aocr.last_error()
    assert call(None, None, pr, 1, 2, 2, 0, 0, pb) != 0 and "NULL" in aocr.last_error()
    assert call(None, pa, None, 1, 2, 2, 0, 0, pb) != 0 and "NULL" in aocr.last_error()
    assert call(None, pa, pr, 0, 2, 2, 0, 0, pb) == 0                           # an empty batch: a no-op, not an error


def test_apply_rejects_host_tensors():
    import torch
    import aocr
    with pytest.raises(ValueError, match="device tensor"):
        aocr.Degrader().apply(torch.zeros(1, 1, 8, 8), 0)
    with pytest.raises(ValueError, match="device tensor"):
        aocr.Augmenter(degrade=aocr.Degrader()).apply(torch.zeros(1, 1, 8, 8), 0)
