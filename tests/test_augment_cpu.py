"""CPU: training augmentation (include/aocr.h aocr_augment_lines, aocr/augment.py) without a device -- hand answers for the
numpy restatement tests/augment_ref.py (the yardstick of tests/test_augment_gpu.py), the host-side parameter draw of
aocr.Augmenter, the record layout, and the argument checks of the entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _ints(n, H, W, seed=1, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (n, 1, H, W)).astype(F)


# ---- the restatement against answers worked out by hand

def test_ref_identity_returns_the_input():
    x = _ints(3, 8, 5)
    np.testing.assert_array_equal(R.augment(x, R.warp_records([R.identity(7.0)] * 3), seed=5, counter=9), x)


def test_ref_integer_shift():
    x = _ints(2, 6, 11)
    got = R.augment(x, R.warp_records([(1, 0, 3, 0, 1, 0, 1, 0, 200.0, 0)] * 2))
    want = np.full_like(x, 200.0)
    want[..., :-3] = x[..., 3:]
    np.testing.assert_array_equal(got, want)


def test_ref_half_pixel_is_the_mean_of_neighbours():
    x = _ints(1, 4, 9, hi=64)                                                   # small integers: every op below is exact
    got = R.augment(x, R.warp_records([(1, 0, 0.5, 0, 1, 0, 1, 0, 10.0, 0)]))
    right = np.concatenate([x[..., 1:], np.full_like(x[..., :1], 10.0)], axis=-1)
    np.testing.assert_array_equal(got, (x + right) / F(2))


def test_ref_gain_offset_and_clamps():
    x = np.arange(256, dtype=F).reshape(1, 1, 8, 32)
    got = R.augment(x, R.warp_records([(1, 0, 0, 0, 1, 0, 2, -128, 255.0, 0)]))
    want = np.clip(2.0 * np.arange(256) - 128.0, 0.0, 255.0).astype(F).reshape(1, 1, 8, 32)
    np.testing.assert_array_equal(got, want)
    assert got.min() == 0.0 and got.max() == 255.0 and (got == 0).sum() == 65 and (got == 255).sum() == 64


def test_ref_noise_is_triangular_on_the_open_interval():
    t = R.noise_field(4, 16, 64, seed=3, counter=1)
    assert t.dtype == np.float32 and -1.0 <= t.min() and t.max() < 1.0
    assert abs(float(t.mean())) < 0.03 and abs(float(t.var()) * 6.0 - 1.0) < 0.1      # 4096 samples: sd 0.0064 / 0.0185, over 4 sigma each
    assert not np.array_equal(t, R.noise_field(4, 16, 64, seed=3, counter=2))


# ---- aocr.Augmenter.params

def test_params_defaults_are_the_identity_record():
    import aocr
    p = aocr.Augmenter(fill=200.0).params(5, 32, 100, counter=3)
    assert p.dtype == R.WARP_DTYPE and p.shape == (5,)
    assert p.tobytes() == R.warp_records([R.identity(200.0)] * 5).tobytes()


def test_params_are_a_function_of_seed_and_counter():
    import aocr
    kw = dict(rotate_deg=5, shear=0.1, scale=1.25, translate=(4, 2), contrast=1.4, brightness=10, noise=3)
    a = aocr.Augmenter(**kw).params(6, 32, 100, 7)
    assert a.tobytes() == aocr.Augmenter(**kw).params(6, 32, 100, 7).tobytes()
    assert a.tobytes() != aocr.Augmenter(**kw).params(6, 32, 100, 8).tobytes()
    assert a.tobytes() != aocr.Augmenter(seed=1, **kw).params(6, 32, 100, 7).tobytes()
    assert a[:4].tobytes() == aocr.Augmenter(**kw).params(4, 32, 100, 7).tobytes()          # image i draws uniforms 8i .. 8i+7


def test_params_stay_inside_the_configured_ranges():
    import aocr
    H, W = 32, 100
    A = aocr.Augmenter(rotate_deg=5, scale=1.25, translate=(6, 2), contrast=1.5, brightness=20, noise=12, fill=250)
    p = A.params(256, H, W, 0)
    m = {k: p[k].astype(np.float64) for k in R.FIELDS}
    # det(R S D) = 1 / (sx sy); the entries were rounded to fp32 once: four relative errors of 2^-24 in the two products
    eps = 8 * 2.0 ** -24
    det = m["m00"] * m["m11"] - m["m01"] * m["m10"]
    assert (det >= 1.25 ** -2 * (1 - eps)).all() and (det <= 1.25 ** 2 * (1 + eps)).all()
    assert det.max() / det.min() > 1.5                                           # and the range is used
    # translation: where the centre lands, minus the centre
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    tx = m["m00"] * cx + m["m01"] * cy + m["m02"] - cx
    ty = m["m10"] * cx + m["m11"] * cy + m["m12"] - cy
    tol = 64 * 2.0 ** -24 * W                                                    # fp32 rounding of entries of magnitude <= W
    assert np.abs(tx).max() <= 6 + tol and np.abs(ty).max() <= 2 + tol
    assert np.abs(tx).max() > 3 and np.abs(ty).max() > 1
    assert (m["gain"] >= 1 / 1.5 * (1 - eps)).all() and (m["gain"] <= 1.5 * (1 + eps)).all()
    b = m["offset"] - 128.0 * (1.0 - m["gain"])
    assert np.abs(b).max() <= 20 + 1e-3
    assert (p["fill"] == 250).all() and (p["noise"] == 12).all()


def test_params_match_the_documented_composition():
    """one image recomputed from the docstring's formulas, scalar by scalar."""
    import math
    import aocr
    A = aocr.Augmenter(rotate_deg=8, shear=0.2, scale=1.2, translate=(6, 2), contrast=1.5, brightness=20, noise=12, seed=77)
    n, H, W, counter, i = 4, 32, 100, 5, 2
    u = aocr.synth.counter_uniform(77, 0x41554700 + counter, 8 * n)[8 * i:8 * i + 8]
    j = [2 * float(v) - 1 for v in u]
    th, k = math.radians(j[0] * 8), j[1] * 0.2
    sx, sy = math.exp(j[2] * math.log(1.2)), math.exp(j[3] * math.log(1.2))
    tx, ty, g, b = j[4] * 6, j[5] * 2, math.exp(j[6] * math.log(1.5)), j[7] * 20
    a00, a01 = math.cos(th) / sx, (k * math.cos(th) - math.sin(th)) / sy
    a10, a11 = math.sin(th) / sx, (k * math.sin(th) + math.cos(th)) / sy
    cx, cy = (W - 1) / 2, (H - 1) / 2
    want = [a00, a01, cx + tx - (a00 * cx + a01 * cy), a10, a11, cy + ty - (a10 * cx + a11 * cy), g, 128 * (1 - g) + b, 255.0, 12.0]
    got = [float(v) for v in A.params(n, H, W, counter)[i]]
    np.testing.assert_allclose(got, want, rtol=2.0 ** -22, atol=2.0 ** -22)     # float64 composition, one cast to fp32


# ---- ABI and errors

def test_warp_record_layout_is_the_headers():
    import aocr
    assert C.sizeof(aocr.augment.Warp) == 40 and aocr.augment.WARP_DTYPE.itemsize == 40
    hdr = open(os.path.join(ROOT, "include", "aocr.h")).read()
    body = re.search(r"typedef struct aocr_warp \{(.*?)\} aocr_warp;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in body.split(";") for f in decl.replace("float", "").split(",") if f.strip()]
    assert fields == [n for n, _ in aocr.augment.Warp._fields_] == list(R.FIELDS) == list(aocr.augment.WARP_DTYPE.names)
    assert all(t is C.c_float for _, t in aocr.augment.Warp._fields_)
    res, args = aocr._lib.SIGNATURES["aocr_augment_lines"]
    assert res is C.c_int and len(args) == 9 and args[6] is C.c_uint64 and args[7] is C.c_uint64


def test_augment_lines_rejects_bad_arguments():
    import aocr
    buf = np.zeros(64, F)
    out = np.zeros(64, F)
    w = R.warp_records([R.identity()])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = aocr.lib.aocr_augment_lines
    for args in ((None, p(w), p(out)), (p(buf), None, p(out)), (p(buf), p(w), None)):
        assert call(None, args[0], args[1], 1, 8, 8, 0, 0, args[2]) != 0
        assert "NULL" in aocr.last_error()
    assert call(None, p(buf), p(w), 1, 8, 8, 0, 0, p(buf)) != 0
    assert "alias" in aocr.last_error()
    for n, H, W in ((-1, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert call(None, p(buf), p(w), n, H, W, 0, 0, p(out)) != 0
        assert "bad sizes" in aocr.last_error()
    assert call(None, p(buf), p(w), 65536, 8, 8, 0, 0, p(out)) != 0
    assert "65535" in aocr.last_error()
    with pytest.raises(aocr.AocrError, match="aocr_augment_lines"):
        aocr.check(call(None, None, None, 1, 8, 8, 0, 0, None), "aocr_augment_lines")


def test_datagen_takes_an_augmenter(tmp_path):
    import aocr
    (tmp_path / "l.txt").write_text("a.npy ab\n")
    A = aocr.Augmenter(noise=2)
    g = aocr.DataGen(str(tmp_path), "l.txt", 8.0, augment=A)
    assert g.augment is A and g.augment_counter == 0
    assert aocr.DataGen(str(tmp_path), "l.txt", 8.0).augment is None
