"""CPU: the flood-fill restatement of aocr_label_components and aocr_clean_page (tests/components_ref.py) alone: against a second,
independent labelling (a two-pass union-find over row runs written here), against the hand answers, and the result the calls exist for -- a
page with dust, a margin rule and an underline segments wrongly as it is and exactly like the clean page once it is cleaned.  Plus the host
mirror of the params struct, the exports and the argument checks that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import components_ref as CR
import segment_ref as R
from components_cases import (CLEAN_CASES, LABEL_CASES, MOTIVE_BOXES, MOTIVE_CLEAN, MOTIVE_SEG, border_crossers, checkerboard, corner_diagonals,
                              framed_text, motive_page, serpentine, u_shape)
from segment_cases import SEEDED_SHAPES, seeded_page

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def two_pass(ink, connectivity):
    """(labels, {label: [x0, y0, x1, y1, label, area]}): the classic two-pass labelling.  Pass 1 gives every horizontal run a provisional
    number and records which runs of neighbouring rows touch in a union-find over run numbers; pass 2 maps every run to the smallest first
    pixel of its class.  Shares nothing with the flood fill: no stack, no pixel neighbourhoods."""
    H, W = ink.shape
    parent, first, runs_of_row = [], [], []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for y in range(H):
        runs = []
        for x0, x1 in R.runs(ink[y]):
            k = len(parent)
            parent.append(k)
            first.append(y * W + x0)
            runs.append((x0, x1, k))
            reach = 1 if connectivity == 8 else 0
            for px0, px1, pk in (runs_of_row[-1] if y else []):
                if px0 < x1 + reach and x0 - reach < px1:
                    a, b = find(k), find(pk)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
        runs_of_row.append(runs)
    best = {}
    for k in range(len(parent)):
        r = find(k)
        best[r] = min(best.get(r, first[k]), first[k])
    labels = np.full((H, W), -1, np.int32)
    comps = {}
    for y, runs in enumerate(runs_of_row):
        for x0, x1, k in runs:
            l = best[find(k)]
            labels[y, x0:x1] = l
            c = comps.setdefault(l, [W, H, 0, 0, l, 0])
            c[0], c[1], c[2], c[3], c[5] = min(c[0], x0), min(c[1], y), max(c[2], x1), max(c[3], y + 1), c[5] + x1 - x0
    return labels, comps


def _pages():
    for H, W, _, _, seed in SEEDED_SHAPES:
        yield f"seeded{H}x{W}", seeded_page(H, W, seed)
    for name, fn in (("checker", lambda: checkerboard(9, 14)), ("corner", lambda: corner_diagonals(4, 6)), ("cross", lambda: border_crossers(4, 6)),
                     ("u", lambda: u_shape(4, 6)), ("serpentine", lambda: serpentine(4, 6)), ("frame", lambda: framed_text(8, 16))):
        yield name, fn()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_flood_fill_agrees_with_two_pass_union_find(connectivity):
    for name, page in _pages():
        labels, comps, info = CR.label_components(page, 128, 0, connectivity, max_components=page.size)
        want, want_comps = two_pass(page <= 128, connectivity)
        np.testing.assert_array_equal(labels, want, err_msg=name)
        np.testing.assert_array_equal(comps, np.array([want_comps[k] for k in sorted(want_comps)], np.int32).reshape(-1, 6), err_msg=name)
        assert info.tolist() == [128, int((page <= 128).sum()), len(want_comps), 0], name
        ink = labels >= 0                                                        # the label is the first pixel of its own component
        flat = labels.reshape(-1)
        assert (flat[flat[ink.reshape(-1)]] == flat[ink.reshape(-1)]).all() and (flat[ink.reshape(-1)] <= np.nonzero(ink.reshape(-1))[0]).all(), name


@pytest.mark.parametrize("case", LABEL_CASES, ids=[c["name"] for c in LABEL_CASES])
def test_label_hand_cases(case):
    labels, comps, info = CR.label_components(case["page"], case["threshold"], case["light_text"], case["connectivity"])
    np.testing.assert_array_equal(labels, case["labels"])
    np.testing.assert_array_equal(comps, case["comps"])
    np.testing.assert_array_equal(info, case["info"])


@pytest.mark.parametrize("case", CLEAN_CASES, ids=[c["name"] for c in CLEAN_CASES])
def test_clean_hand_cases(case):
    out, counts = CR.clean_page(case["page"], **case["params"])
    np.testing.assert_array_equal(out, case["out"])
    np.testing.assert_array_equal(counts, case["counts"])


def test_shape_pages_have_the_components_they_are_built_for():
    for conn, n in ((4, 63), (8, 1)):
        assert CR.label_components(checkerboard(9, 14), 128, 0, conn)[2][2] == n
    for conn, n in ((4, 4), (8, 2)):
        labels, comps, info = CR.label_components(corner_diagonals(4, 6), 128, 0, conn)
        assert info[2] == n and (conn == 4 or comps[:, 5].tolist() == [2, 2])
    assert CR.label_components(border_crossers(4, 6), 128, 0, 4)[2][2] == 3
    labels, comps, info = CR.label_components(u_shape(4, 6), 128, 0, 4)
    assert info[2] == 1 and comps[0, 4] == 1 * 12 + 2 and labels[3, 11] == 14     # the right arm carries the left arm's first pixel
    for conn in (4, 8):
        page = serpentine(4, 6)
        labels, comps, info = CR.label_components(page, 128, 0, conn)
        assert info[2] == 1 and comps[0].tolist() == [0, 0, 19, 11, 0, int((page == 0).sum())]
    labels, comps, info = CR.label_components(framed_text(8, 16), 128, 0, 8)
    assert info[2] == 1 + 2 * 2 and comps[0].tolist()[:5] == [0, 0, 41, 21, 0] and (comps[1:, 5] == 45).all()


def test_dirty_page_segments_wrongly_and_the_cleaned_page_like_the_clean_one():
    clean = motive_page()
    boxes, counts = R.segment_page(clean, **MOTIVE_SEG)
    np.testing.assert_array_equal(boxes, np.array(MOTIVE_BOXES, np.int32))
    assert counts.tolist() == [6, 2, 128, 0]
    # each defect alone: what the issue's table says
    b, c = R.segment_page(motive_page(specks=True), **MOTIVE_SEG)
    assert c[:2].tolist() == [5, 2] and b[0, :4].tolist() == [10, 8, 66, 20] and b[1, 0] == 78
    b, c = R.segment_page(motive_page(vrule=True), **MOTIVE_SEG)
    assert c[:2].tolist() == [3, 1] and (b[:, 1] == 2).all() and (b[:, 3] == 58).all()
    b, c = R.segment_page(motive_page(hrule=True), **MOTIVE_SEG)
    assert c[:2].tolist() == [4, 2] and b[0, :4].tolist() == [6, 8, 112, 23]
    dirty = motive_page(True, True, True)
    b, c = R.segment_page(dirty, **MOTIVE_SEG)
    assert c[:2].tolist() != [6, 2]
    print(f"[components ref] dirty page: {int(c[0])} boxes in {int(c[1])} lines")
    out, counts = CR.clean_page(dirty, **MOTIVE_CLEAN)
    np.testing.assert_array_equal(out, clean)
    assert counts.tolist() == [6 + 4 + 2, 4, 2, 128, 6 * 264 + 4 + 56 + 106, 4 + 56 + 106, 0, 0]
    b, c = R.segment_page(out, **MOTIVE_SEG)
    np.testing.assert_array_equal(b, np.array(MOTIVE_BOXES, np.int32))
    assert c.tolist() == [6, 2, 128, 0]
    same, counts = CR.clean_page(clean, **MOTIVE_CLEAN)                         # nothing to remove: bit for bit
    np.testing.assert_array_equal(same, clean)
    assert counts.tolist() == [6, 0, 0, 128, 6 * 264, 0, 0, 0]


def test_params_struct_exports_and_argument_checks():
    import aocr
    p = aocr.CleanParams()
    assert [getattr(p, n) for n, _ in p._fields_][:6] == [-1, 0, 8, 6, 0, 200] and list(p.reserved) == [0, 0] and C.sizeof(p) == 32
    hdr = open(os.path.join(ROOT, "include", "aocr.h")).read()
    body = re.search(r"typedef struct aocr_clean_params \{(.*?)\} aocr_clean_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"int32_t\s+([^;]+);", body) for n in decl.split(",")]
    assert fields == ["threshold", "light_text", "connectivity", "min_area", "max_w", "max_h", "reserved[2]"]
    assert [n for n, _ in aocr.CleanParams._fields_] == [f.split("[")[0] for f in fields]
    lib = C.CDLL(aocr._lib.LIB_PATH)
    for n in ("aocr_components_scratch_bytes", "aocr_label_components", "aocr_clean_scratch_bytes", "aocr_clean_page"):
        assert n in aocr._lib.SIGNATURES and getattr(lib, n) is not None and re.search(r"\b%s\(" % n, hdr)
    for n in ("CleanParams", "label_components_device", "clean_page_device"):
        assert n in aocr.__all__ and n in aocr.page.__all__ and hasattr(aocr, n)
    a4 = aocr.lib.aocr_components_scratch_bytes(3508, 2480), aocr.lib.aocr_clean_scratch_bytes(3508, 2480)
    assert 0 < a4[0] < a4[1] and a4[1] - a4[0] >= 4 * 3508 * 2480              # the labels live in the clean call's scratch
    assert aocr.lib.aocr_clean_scratch_bytes(8192, 8192) < 1 << 30
    for fn in (aocr.lib.aocr_components_scratch_bytes, aocr.lib.aocr_clean_scratch_bytes):
        for H, W in ((0, 10), (10, 16385), (16384, 4097)):
            assert fn(H, W) == 0 and "bad sizes" in aocr.last_error()
    # the checks come before any device work: host addresses are enough to see them refuse
    page, out = np.zeros((10, 12), np.uint8), np.full((10, 12), 7, np.uint8)
    labels, comps = np.full((10, 12), -7, np.int32), np.full((4, 6), -7, np.int32)
    info, counts, sc = np.full(4, -7, np.int32), np.full(8, -7, np.int32), np.zeros(1 << 13, np.int64)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def label(**kw):
        a = dict(page=vp(page), pitch=12, H=10, W=12, thr=128, light=0, conn=8, sc=vp(sc), labels=vp(labels), lp=12, mc=4, comps=vp(comps), info=vp(info))
        a.update(kw)
        return aocr.lib.aocr_label_components(None, a["page"], a["pitch"], a["H"], a["W"], a["thr"], a["light"], a["conn"], a["sc"], a["labels"],
                                              a["lp"], a["mc"], a["comps"], a["info"])

    for kw, word in ((dict(conn=6), "connectivity"), (dict(conn=0), "connectivity"), (dict(thr=255), "threshold"), (dict(thr=-2), "threshold"),
                     (dict(mc=0), "max_components"), (dict(mc=65537), "max_components"), (dict(lp=11), "labels_pitch"), (dict(pitch=11), "pitch"),
                     (dict(H=0), "page size"), (dict(page=None), "NULL"), (dict(sc=None), "NULL"), (dict(labels=None), "NULL"), (dict(info=None), "NULL"),
                     (dict(labels=C.c_void_p(labels.ctypes.data + 2)), "aligned"), (dict(labels=vp(sc)), "overlaps the scratch"),
                     (dict(labels=vp(page), H=2, W=2, pitch=2, lp=2), "overlaps the page")):
        assert label(**kw) != 0 and word in aocr.last_error(), (kw, aocr.last_error())
    assert (labels == -7).all() and (comps == -7).all() and (info == -7).all()

    def clean(params=None, **kw):
        a = dict(page=vp(page), pitch=12, H=10, W=12, sc=vp(sc), out=vp(out), op=12, counts=vp(counts))
        a.update(kw)
        q = aocr.CleanParams(**(params or {}))
        q.reserved[1] = a.pop("reserved", 0)
        return aocr.lib.aocr_clean_page(None, a["page"], a["pitch"], a["H"], a["W"], None if a.get("null_params") else C.byref(q), a["sc"], a["out"],
                                        a["op"], a["counts"])

    for params, kw, word in ((dict(connectivity=5), {}, "connectivity"), (dict(min_area=0), {}, "min_area"), (dict(max_w=-1), {}, "max_w"),
                             (dict(max_h=-1), {}, "max_h"), (dict(threshold=255), {}, "threshold"), ({}, dict(reserved=1), "reserved"),
                             ({}, dict(null_params=1), "NULL"), ({}, dict(out=None), "NULL"), ({}, dict(counts=None), "NULL"), ({}, dict(sc=None), "NULL"),
                             ({}, dict(op=11), "out_pitch"), ({}, dict(W=13), "pitch"), ({}, dict(out=vp(page)), "overlaps the page"),
                             ({}, dict(out=vp(sc)), "overlaps the scratch")):
        assert clean(params, **kw) != 0 and word in aocr.last_error(), (params, kw, aocr.last_error())
    assert (out == 7).all() and (counts == -7).all()
