"""CPU: the numpy restatements of aocr_ink_integral and aocr_layout_blocks (tests/layout_ref.py) alone: the hand answers, and the result the
calls exist for -- a two-column page whose lines aocr_segment_page interleaves across the gutter reads column by column once it is cut into
blocks.  Plus the host mirror of the params struct, the exports and the argument checks that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import layout_ref as L
import segment_ref as R
from layout_cases import AREAS, CASES, GUTTER, SPECK, TWO_COL, TWO_COL_SHAPE, two_column_page

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_cases(case):
    S, info = L.ink_integral(case["page"], case["threshold"], case["light_text"])
    np.testing.assert_array_equal(info, case["info"])
    blocks, counts = L.layout_blocks(S, case["max_blocks"], **case["params"])
    np.testing.assert_array_equal(blocks, case["blocks"])
    np.testing.assert_array_equal(counts, case["counts"])


def test_table_is_the_rectangle_count():
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, size=(13, 17), dtype=np.uint8)
    S, info = L.ink_integral(page, 100)
    assert S.shape == (14, 18) and (S[0] == 0).all() and (S[:, 0] == 0).all() and info.tolist() == [100, int((page <= 100).sum()), 0, 0]
    for x0, y0, x1, y1 in ((0, 0, 17, 13), (3, 2, 9, 11), (16, 12, 17, 13), (5, 5, 5, 9)):
        assert L.rect(S, x0, y0, x1, y1) == int((page[y0:y1, x0:x1] <= 100).sum())
    Sl, _ = L.ink_integral(page, 100, 1)
    assert np.array_equal(S + Sl, np.outer(np.arange(14), np.arange(18)))           # every pixel is ink in exactly one of the two


def test_pieces_chain_and_ignore_the_rim():
    f = [0, 1, 1, 0, 0, 1, 0, 0, 0, 1, 0]
    assert L.pieces(f, 3) == [(1, 6), (9, 10)] and L.pieces(f, 4) == [(1, 10)] and L.pieces(f, 1) == [(1, 3), (5, 6), (9, 10)]
    assert L.pieces([0, 0, 0], 2) == []


def _inside(block, area):
    _, y0, y1, x0, x1 = area
    return x0 <= block[0] < block[2] <= x1 and y0 <= block[1] < block[3] <= y1


def test_two_column_page_cuts_into_reading_order():
    page = two_column_page()
    assert page.shape == TWO_COL_SHAPE
    blocks, counts, info = L.layout_page(page, 128, 0, min_ink=2, **TWO_COL)
    print(f"[layout ref] min_ink 2: counts {counts.tolist()} info {info.tolist()}\n{blocks}")
    assert counts.tolist() == [5, 3, 0, 0]
    for b, area in zip(blocks, AREAS):                                               # headline, left top, left bottom, right top, right bottom
        assert _inside(b, area), (b, area)
        assert b[2] - b[0] > 0.8 * (area[4] - area[3]) and b[1] == area[1] and b[3] == area[2]
    assert blocks[:, 4].tolist() == [1, 3, 3, 3, 3]
    assert int(blocks[:, 5].sum()) == int(info[1]) - 1                              # all the ink but the speck

    lst = {}
    S, _ = L.ink_integral(page, 128)
    blocks1, counts1 = L.layout_blocks(S, info=lst, **dict(TWO_COL, min_ink=1))
    print(f"[layout ref] min_ink 1: counts {counts1.tolist()}")
    assert counts1.tolist() == [5, 3, 1, 0]                                          # the same, plus the speck as a 1 x 1 block that is dropped
    assert lst["final"][3] == (SPECK[1], SPECK[0], SPECK[1] + 1, SPECK[0] + 1, 2) and len(lst["final"]) == 6
    np.testing.assert_array_equal(blocks1[:, :4], blocks[:, :4])


def test_whole_page_interleaves_the_columns_and_blocks_do_not():
    page = two_column_page()
    seg = dict(threshold=128)
    whole, wc = R.segment_page(page, **seg)
    mid = (GUTTER[0] + GUTTER[1]) // 2
    body = AREAS[0][2]                                                               # below the headline, which spans the gutter by design
    both = [l for l in range(int(wc[1])) if {bool(b[0] >= mid) for b in whole if b[4] == l and b[1] >= body} == {False, True}]
    assert both, "no line of the whole page has boxes on both sides of the gutter"
    blocks, _, _ = L.layout_page(page, 128, 0, min_ink=2, **TWO_COL)
    boxes, ids, lines, found, truncated = L.segment_blocks(page, blocks, **seg)
    assert not truncated and found == len(boxes) and len(boxes) > 100
    for l in range(lines):
        sides = {bool(b[0] >= mid) for b in boxes if b[4] == l and b[1] >= body}
        assert len(sides) <= 1, l
    assert (np.diff(ids) >= 0).all() and (np.diff(boxes[:, 4]) >= 0).all()         # reading order: block, then line
    print(f"[layout ref] whole page: {int(wc[0])} boxes in {int(wc[1])} lines, {len(both)} of them on both sides; by blocks: {found} in {lines}")


def test_params_struct_exports_and_argument_checks():
    import aocr
    p = aocr.LayoutParams()
    assert [getattr(p, n) for n, _ in p._fields_] == [1, 24, 30, 8, 8, 8, 16, 0] and C.sizeof(p) == 32
    hdr = open(os.path.join(ROOT, "include", "aocr.h")).read()
    body = re.search(r"typedef struct aocr_layout_params \{(.*?)\} aocr_layout_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"int32_t\s+([^;]+);", body) for n in decl.split(",")]
    assert fields == [n for n, _ in aocr.LayoutParams._fields_]
    for n in ("aocr_integral_scratch_bytes", "aocr_ink_integral", "aocr_layout_scratch_bytes", "aocr_layout_blocks"):
        assert n in aocr._lib.SIGNATURES
    for n in ("LayoutParams", "ink_integral_device", "layout_page_device"):
        assert n in aocr.__all__ and n in aocr.page.__all__ and hasattr(aocr, n)
    assert aocr.lib.aocr_integral_scratch_bytes(3508, 2480) > 0 and aocr.lib.aocr_layout_scratch_bytes(3508, 2480, 1024) > 0
    for H, W in ((0, 10), (10, 16385), (16384, 4097)):
        assert aocr.lib.aocr_integral_scratch_bytes(H, W) == 0 and "bad sizes" in aocr.last_error()
    for H, W, mb in ((0, 10, 8), (16384, 4097, 8), (10, 10, 0), (10, 10, 1025)):
        assert aocr.lib.aocr_layout_scratch_bytes(H, W, mb) == 0 and "bad sizes" in aocr.last_error()
    # the checks come before any device work: host addresses are enough to see them refuse
    sat = np.zeros((11, 12), np.uint32)
    out, counts, sc = np.zeros((4, 6), np.int32), np.zeros(4, np.int32), np.zeros(4096, np.int64)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for kw, word in ((dict(max_depth=0), "max_depth"), (dict(max_depth=17), "max_depth"), (dict(gap_x=0), "gap_x"), (dict(min_ink=0), "min_ink"),
                     (dict(min_block_ink=0), "min_block")):
        assert aocr.lib.aocr_layout_blocks(None, vp(sat), 12, 10, 11, C.byref(aocr.LayoutParams(**kw)), vp(sc), 4, vp(out), vp(counts)) != 0
        assert word in aocr.last_error()
    q = aocr.LayoutParams()
    q.reserved = 1
    assert aocr.lib.aocr_layout_blocks(None, vp(sat), 12, 10, 11, C.byref(q), vp(sc), 4, vp(out), vp(counts)) != 0 and "reserved" in aocr.last_error()
    assert aocr.lib.aocr_layout_blocks(None, vp(sat), 11, 10, 11, C.byref(p), vp(sc), 4, vp(out), vp(counts)) != 0 and "sat_pitch" in aocr.last_error()
    assert aocr.lib.aocr_layout_blocks(None, None, 12, 10, 11, C.byref(p), vp(sc), 4, vp(out), vp(counts)) != 0 and "NULL" in aocr.last_error()
