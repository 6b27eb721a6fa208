"""CPU: label-free recognition (include/aocr.h aocr_recognize) -- the entry point is exported and bound, a bad call fails loudly, and the
image column of every encoder step follows from the CNN's geometry (cnn.lua).  The calls that need a model handle run in
tests/test_recognize_gpu.py (creating a model needs a device)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# cnn.lua:12-40, along the width only: (kernel, stride, pad).  3x3 / pad 1 convolutions keep the width, the two 2x2 / stride 2 pools halve it,
# the (1,2) pools have a width kernel of 1 (stride 1), conv7 is 2x2 without padding.
CNN_WIDTH = [(3, 1, 1), (2, 2, 0), (3, 1, 1), (2, 2, 0), (3, 1, 1), (3, 1, 1), (1, 1, 0), (3, 1, 1), (3, 1, 1), (1, 1, 0), (2, 1, 0)]


def _out_width(W):
    for k, s, p in CNN_WIDTH:
        W = (W + 2 * p - k) // s + 1
    return W


def _receptive_field(t):
    """image columns [lo, hi] (inclusive, padding included) that encoder step t reads."""
    lo, hi = t, t
    for k, s, p in reversed(CNN_WIDTH):
        lo, hi = lo * s - p, hi * s - p + k - 1
    return lo, hi


def test_recognize_exported_and_bound():
    import aocr
    hdr = open(os.path.join(ROOT, "include", "aocr.h")).read()
    assert re.search(r"^int aocr_recognize\(", hdr, re.M)
    raw = C.CDLL(aocr._lib.LIB_PATH)
    assert hasattr(raw, "aocr_recognize")
    res, args = aocr._lib.SIGNATURES["aocr_recognize"]
    assert res is C.c_int and len(args) == 10
    assert aocr.lib.aocr_recognize.argtypes is not None


def test_recognize_rejects_null_model():
    import aocr
    labels = np.zeros((2, 4), np.int32)
    scores = np.zeros(2, np.float32)
    rc = aocr.lib.aocr_recognize(None, None, 2, 100, 1, None, labels.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p), None, None)
    assert rc != 0
    assert "NULL" in aocr.last_error()


def test_encoder_columns():
    import aocr
    for W in (100, 256, 36, 1024):
        T = W // 4 - 1
        assert _out_width(W) == T
        cols = aocr.encoder_columns(W)
        assert cols.shape == (T,)
        for t in (0, T // 2, T - 1):
            lo, hi = _receptive_field(t)
            assert cols[t] == (lo + hi + 1) / 2.0          # centre of the symmetric receptive field, column k spanning [k, k + 1)
    assert np.array_equal(aocr.encoder_columns(100), 4.0 * np.arange(24) + 4.0)
    c256 = aocr.encoder_columns(256)
    assert len(c256) == 63 and c256[0] == 4.0 and c256[-1] == 252.0
