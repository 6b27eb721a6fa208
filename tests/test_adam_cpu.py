"""CPU: tests/adam_ref.py (the float32 restatement the GPU tests hold aocr_adam_update to, bit for bit) against AdamW written out in float64,
and the new declarations of lua/aocr_ffi.lua and aocr/_lib.py against include/aocr.h."""
import ctypes as C
import os

import numpy as np

import adam_ref as R
import cdecl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aocr_adam_state_bytes", "aocr_adam_scratch_bytes", "aocr_adam_update", "aocr_adam_step")


def test_ref_follows_float64_adamw_over_20_steps():
    """Gradients keep their sign per element with 0.5 <= |g| <= 1, so m and v are sums of same-signed terms and relative errors add up instead of
    being amplified by cancellation.  With e = 2^-24 (float32 unit round-off), to first order in e:
      m_t, v_t: each step adds at most 2e to the relative error (the scaled product, then the sum)            -> 2t e
      m_t / c1 and v_t / c2: + e for c1 / c2 (one double-to-float rounding), + e for the divide               -> (2t + 2) e
      sqrt halves it, + e for its own rounding, + e for adding eps > 0                                         -> (t + 3) e
      u = quotient                                                                                            -> (3t + 6) e relative, |u| <= U = 1 / 0.5
      w' = w - lr (u + wd w): wd w (e), the sum s (e), lr s (e), the difference (e), with |s| <= S = U + wd W, |w| <= W
         abs error added by step t <= e (lr (U (3t + 6) + wd W + 2 S) + W); what earlier steps left is carried with factor 1 - lr wd <= 1.
    The bound is the sum over t = 1..20, times 1.01 for the terms of second order and the float64 reference's own rounding (beta^t by pow
    against running products: ~2^-52 relative).  The float64 side uses the float32 VALUES of lr, betas, eps, wd; 1 - beta is exact for both betas."""
    T, n = 20, 4096
    rng = np.random.default_rng(20)
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in (1e-2, 0.9, 0.999, 1e-8, 0.01))
    assert float(np.float32(1.0) - np.float32(b1)) == 1.0 - b1 and float(np.float32(1.0) - np.float32(b2)) == 1.0 - b2
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    grads = [(sign * rng.uniform(0.5, 1.0, n)).astype(np.float32) for _ in range(T)]
    w0 = rng.uniform(-2.0, 2.0, n).astype(np.float32)
    ref = R.adamw64(w0, grads, lr, b1, b2, eps, wd)
    off = [0, 5, 5, 7, 1030, n]
    st, w = R.State(n), w0
    e, U = 2.0 ** -24, 2.0
    W = max(np.abs(r).max() for r in ref) * (1 + 2.0 ** -10)
    S = U + wd * W
    bound = 0.0
    for t in range(1, T + 1):
        w = R.step(w, grads[t - 1], st, off, [1.0] * 5, lr, b1, b2, eps, wd)
        bound += 1.01 * e * (lr * (U * (3 * t + 6) + wd * W + 2 * S) + W)
        err = np.abs(w.astype(np.float64) - ref[t - 1]).max()
        print(f"[adam] step {t:2d}: max |float32 ref - float64 AdamW| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (t, err, bound)
    q1 = 1.0
    for _ in range(T):
        q1 *= b1
    assert st.steps == T and st.p1 == q1 and abs(st.p2 - b2 ** T) <= 1e-15
    assert np.abs(w.astype(np.float64) - w0).min() > 10 * bound, "the trajectory must move by much more than the bound"


def test_ref_scale_and_fresh_state():
    """scale enters as g * scale[group]; an all-zero state reads p1 = p2 = 1, so step 1 has c1 = 1 - beta1, c2 = 1 - beta2 and |u| = |g| / (|g| + eps)."""
    off = [0, 2, 2, 3, 5, 6]
    g = np.array([1.0, -2.0, 4.0, 0.5, 0.0, -8.0], np.float32)
    w0 = np.zeros(6, np.float32)
    st = R.State(6)
    w = R.step(w0, g, st, off, [1.0, 1.0, 0.5, 1.0, 0.25], lr=0.5, beta1=0.5, beta2=0.75, eps=2.0 ** -20)
    gs = np.array([1.0, -2.0, 2.0, 0.5, 0.0, -2.0])
    np.testing.assert_array_equal(st.m, (0.5 * gs).astype(np.float32))
    np.testing.assert_array_equal(st.v, (0.25 * gs * gs).astype(np.float32))
    np.testing.assert_array_equal(w, (-0.5 * gs / (np.abs(gs) + 2.0 ** -20)).astype(np.float32))
    assert (st.p1, st.p2, st.steps) == (0.5, 0.75, 1) and w[4] == 0.0
    img = st.to_bytes()
    assert len(img) == 8 * 6 + 32 and np.frombuffer(img[48:64], np.float64).tolist() == [0.5, 0.75] and np.frombuffer(img[64:], np.int64).tolist() == [1, 0]


def _decls():
    hdr = open(os.path.join(ROOT, "include", "aocr.h")).read()
    lua = open(os.path.join(ROOT, "lua", "aocr_ffi.lua")).read()
    return cdecl.parse(hdr), cdecl.parse(cdecl.lua_cdef_blocks(lua), macros=cdecl.defines(hdr))


def test_header_declares_the_adam_entry_points():
    h, _ = _decls()
    f = h["functions"]
    assert f["aocr_adam_state_bytes"] == ("size_t", ["int64_t"]) and f["aocr_adam_scratch_bytes"] == ("size_t", ["void"])
    assert f["aocr_adam_update"] == ("int", ["void*", "float*", "const float*", "void*", "const int64_t[6]", "const aocr_adam_params*", "const int32_t*",
                                             "void*", "float*"])
    assert f["aocr_adam_step"] == ("int", ["aocr_model*", "const aocr_adam_params*", "void*", "float*"])
    assert [n for _, n in h["structs"]["aocr_adam_params"]][:6] == ["lr", "beta1", "beta2", "eps", "weight_decay", "clip"]
    assert all(t == "float" for t, _ in h["structs"]["aocr_adam_params"][:6])


def test_lua_cdef_matches_the_header():
    h, l = _decls()
    for n in NAMES:
        assert l["functions"].get(n) == h["functions"][n], (n, l["functions"].get(n), h["functions"][n])
    assert l["structs"].get("aocr_adam_params") == h["structs"]["aocr_adam_params"]


def test_ctypes_signatures_match_the_header():
    import aocr
    from aocr import _lib
    h, _ = _decls()
    ctype = {"void*": C.c_void_p, "float*": C.c_void_p, "const float*": C.c_void_p, "const int32_t*": C.c_void_p, "aocr_model*": C.c_void_p,
             "int64_t": C.c_int64, "const int64_t[6]": C.POINTER(C.c_int64), "const aocr_adam_params*": C.POINTER(_lib.AdamParams)}
    res = {"int": C.c_int, "size_t": C.c_size_t}
    for n in NAMES:
        ret, params = h["functions"][n]
        want = [] if params == ["void"] else [ctype[p] for p in params]
        assert _lib.SIGNATURES[n] == (res[ret], want), (n, _lib.SIGNATURES[n], ret, params)
        assert getattr(aocr.lib, n).argtypes == want
    fields = _lib.AdamParams._fields_
    assert [(nm, t) for nm, t in fields[:6]] == [(nm, C.c_float) for _, nm in h["structs"]["aocr_adam_params"][:6]]
    assert fields[6][0] == "reserved" and C.sizeof(fields[6][1]) == 8 and C.sizeof(_lib.AdamParams) == 32
    assert aocr.AdamParams is _lib.AdamParams


def test_sizes_and_host_side_checks():
    import aocr
    import pytest
    assert aocr.lib.aocr_adam_state_bytes(0) == 32 and aocr.lib.aocr_adam_state_bytes(12178995) == 8 * 12178995 + 32
    assert aocr.lib.aocr_adam_scratch_bytes() % 8 == 0 and aocr.lib.aocr_adam_scratch_bytes() > 0
    p = aocr.AdamParams()
    assert (p.lr, p.beta1, p.beta2, p.eps, p.weight_decay, p.clip) == tuple(float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0))
    for bad in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=0.0), dict(lr=float("nan")), dict(clip=-1.0), dict(weight_decay=float("inf"))):
        with pytest.raises(ValueError):
            aocr.AdamParams(**bad)
    m = aocr.Model()
    with pytest.raises(ValueError, match="optimizer"):
        m._set_optimizer(dict(optimizer="rmsprop"))
    with pytest.raises(ValueError, match="unknown"):
        m._set_optimizer(dict(optimizer="adam", adam=dict(beta=0.9)))
    m._set_optimizer({})
    assert m.optimizer == "sgd" and m.adam_state is None and m.adam_steps() == 0
    m._set_optimizer(dict(optimizer="adam", adam=dict(lr=3e-4, clip=5.0)))
    assert m.optimizer == "adam" and m.adam_opts == dict(lr=3e-4, clip=5.0)
    # the library's own checks run before anything is enqueued, so they answer without a device
    off = (C.c_int64 * 6)(0, 1, 2, 3, 4, 5)
    one = C.c_void_p(64)
    assert aocr.lib.aocr_adam_update(None, one, one, one, off, None, None, one, None) != 0 and "NULL" in aocr.last_error()
    assert aocr.lib.aocr_adam_update(None, one, one, C.c_void_p(68), off, C.byref(p), None, one, None) != 0 and "aligned" in aocr.last_error()
