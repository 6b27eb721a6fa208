"""CPU: the numpy restatement of aocr_flatten_page (tests/flatten_ref.py) alone: the hand answers, the identity on a clean page, and the
result the call exists for -- an unevenly lit page that one global threshold cannot segment segments like the clean page once flattened."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flatten_ref as F
import segment_ref as R
import skew_ref as S
from flatten_cases import CASES, LIT_FLOORS, clean_page, lit_page

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases(case):
    _, page, r, light, want = case
    np.testing.assert_array_equal(F.flatten(page, r, light), want)
    if not light:                                                            # light_text is the mirror image of the dark case
        np.testing.assert_array_equal(F.flatten((255 - page).astype(np.uint8), r, 1), 255 - want)


def test_step_edge_sees_every_clipped_window():
    """the step-edge case really has windows of 4, 6 and 9 pixels, and its B is the one written down in flatten_cases.py."""
    page = CASES[[c[0] for c in CASES].index("step_edge")][1]
    M, B = F.background(page.astype(np.int64), 1)
    assert M.tolist() == [[100, 200, 200, 200]] * 3 and B.tolist() == [[150, 167, 200, 200]] * 3
    _, nx = F.window_sum(M, 1, 1)
    _, ny = F.window_sum(M, 1, 0)
    assert sorted(set((ny[:, None] * nx[None, :]).reshape(-1).tolist())) == [4, 6, 9]


def test_radius_beyond_the_page_is_the_whole_page():
    rng = np.random.default_rng(3)
    page = rng.integers(0, 256, size=(5, 9), dtype=np.uint8)
    want = F.flatten(page, 9)
    assert np.array_equal(F.flatten(page, 127), want)
    Bc = max(int(page.max()), 1)                                             # M is the page's max everywhere, and so is its mean
    assert np.array_equal(want, np.minimum(255, (page.astype(np.int64) * 255 + (Bc >> 1)) // Bc))


def test_clean_page_comes_back_unchanged():
    page = clean_page()
    assert np.array_equal(F.flatten(page, 16), page) and np.array_equal(F.flatten(page, 4), page)
    assert np.array_equal(F.flatten((255 - page).astype(np.uint8), 16, 1), 255 - page)


@pytest.mark.parametrize("floor", LIT_FLOORS)
def test_lit_page_segments_like_the_clean_page_once_flattened(floor):
    straight, lit = lit_page(floor)
    want, c0 = R.segment_page(straight)
    assert c0[0] == 109 and c0[1] == 15
    _, c = R.segment_page(lit)
    print(f"[flatten ref] floor {floor}: lit page {c.tolist()}")
    assert c[0] == 1 and c[1] == 1                                           # the dim half of the paper is all ink
    for r in (16, 4):
        got, c = R.segment_page(F.flatten(lit, r))
        assert c[0] == 109 and c[1] == 15, (r, c)
        np.testing.assert_array_equal(got[:, :5], want[:, :5])


def test_skew_estimate_on_the_lit_sheared_page():
    """the 600 x 800 page sheared by 17 steps, repainted and lit at floor 110.  skew_ref.estimate_skew with its defaults returns
    [17, 1088, 125, 0] before flattening -- at Otsu's 125 the dim half is one block of ink whose sheared edge still votes for 17 -- and
    [17, 1088, 44, 0] after it, where the threshold separates ink from paper over the whole page."""
    _, lit = lit_page(110, 17)
    before, _ = S.estimate_skew(lit)
    after, _ = S.estimate_skew(F.flatten(lit, 16))
    print(f"[flatten ref] skew before {before.tolist()} after {after.tolist()}")
    assert after[0] == 17 and after[1] == 17 * 64
    _, c = R.segment_page(S.deskew(F.flatten(lit, 16), int(after[1])))
    assert c[1] == 15 and c[0] == 109


def test_params_struct_and_exports():
    import aocr
    p = aocr.FlattenParams()
    assert (p.radius, p.light_text, list(p.reserved)) == (16, 0, [0, 0]) and C.sizeof(p) == 16
    q = aocr.FlattenParams(radius=32, light_text=1)
    assert (q.radius, q.light_text) == (32, 1)
    hdr = open(os.path.join(ROOT, "include", "aocr.h")).read()
    body = re.search(r"typedef struct aocr_flatten_params \{(.*?)\} aocr_flatten_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(1), int(m.group(2) or 1)) for m in re.finditer(r"int32_t\s+(\w+)(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("radius", 1), ("light_text", 1), ("reserved", 2)]
    assert [(n, C.sizeof(t) // 4) for n, t in aocr.FlattenParams._fields_] == fields
    for n in ("aocr_flatten_scratch_bytes", "aocr_flatten_page"):
        assert n in aocr._lib.SIGNATURES
    for n in ("FlattenParams", "flatten_page_device"):
        assert n in aocr.__all__ and n in aocr.page.__all__ and hasattr(aocr, n)
    assert aocr.lib.aocr_flatten_scratch_bytes(3508, 2480, 16) > 0
    for H, W, r in ((0, 10, 16), (10, 16385, 16), (16384, 4097, 16), (10, 10, 0), (10, 10, 128)):
        assert aocr.lib.aocr_flatten_scratch_bytes(H, W, r) == 0 and "bad sizes" in aocr.last_error()
