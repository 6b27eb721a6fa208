"""No device: the numpy half of tests/page_harness.py, which the page-stage GPU tests build their inputs and expected buffers with."""
import numpy as np
import pytest

from page_harness import csrc_constants, expect_placed, placed_bytes

FLATTEN_TILING = ("HSEG", "HROWS", "VT_COLS", "VT_ROWS", "VS_WORDS", "VS_ROWS")


@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("extra", [0, 7])
@pytest.mark.parametrize("shape,elem", [((1, 1), 1), ((3, 5), 1), ((3, 5), 3)], ids=["1x1", "3x5", "3x5rgb"])
def test_placed_bytes(shape, elem, extra, offset):
    H, W = shape
    rng = np.random.default_rng(H * W + elem)
    page = rng.integers(1, 99, shape + ((elem,) if elem > 1 else ()), dtype=np.uint8)       # no byte of it is the fill
    row, fill, tail = W * elem, 99, 16
    pitch = row + extra
    for given in ((pitch,) if extra else (pitch, None)):                                      # pitch=None is the tight pitch
        buf = placed_bytes(page, given, offset, fill, tail, elem)
        assert buf.dtype == np.uint8 and len(buf) == offset + H * pitch + tail
        inside = np.zeros(len(buf), bool)
        for y in range(H):
            inside[offset + y * pitch:offset + y * pitch + row] = True
        np.testing.assert_array_equal(buf[inside].reshape(page.shape), page)
        assert (buf[~inside] == fill).all() and (~inside).sum() == offset + H * extra + tail


def test_expect_placed_is_placed_bytes_with_the_poison():
    want = np.arange(15, dtype=np.uint8).reshape(3, 5)
    for out_pitch, out_offset, poison, tail in ((None, 0, 0xAB, 32), (12, 5, 0xAB, 32), (8, 0, 0x5A, 16)):
        np.testing.assert_array_equal(expect_placed(want, out_pitch, out_offset, poison=poison, tail=tail),
                                      placed_bytes(want, out_pitch, out_offset, fill=poison, tail=tail))
    with pytest.raises(TypeError):
        expect_placed(want)                                                                   # the poison and the tail have no default


def test_csrc_constants():
    t = csrc_constants("flatten.hip", FLATTEN_TILING)
    assert sorted(t) == sorted(FLATTEN_TILING) and all(isinstance(v, int) and v > 0 for v in t.values())
    with pytest.raises(KeyError):
        csrc_constants("flatten.hip", FLATTEN_TILING + ("NO_SUCH_TILE",))
