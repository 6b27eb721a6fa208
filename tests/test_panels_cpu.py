"""CPU: the restatement of aocr_invert_panels (tests/panels_ref.py) against the hand answers, the motive on the restatements alone (the
words on a reversed-out slab are lost by segmentation and by cleaning, and come back after the stage), the boundary of every condition
and one pixel past it, and the readback of page_boxes with the new rider left out.  No device."""
import numpy as np
import pytest
import torch

import components_ref as CR
import panels_ref as PR
import segment_ref as R
from panels_cases import CASES, SEEDED, SMALL, diamond, panel_page, rotated_slab

MOTIVE = (120, 300, 21)                  # H, W, seed
SEG = dict(threshold=128, min_line_h=4, word_gap=3, min_word_w=2, pad_x=0, pad_y=0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_cases(case):
    out, panels, counts = PR.invert_panels(case["page"], **case["params"])
    np.testing.assert_array_equal(out, case["out"])
    np.testing.assert_array_equal(panels, case["panels"])
    np.testing.assert_array_equal(counts, case["counts"])


def _inside(box, rect):
    return rect[0] <= box[0] and box[2] <= rect[2] and rect[1] <= box[1] and box[3] <= rect[3]


@pytest.mark.parametrize("light", [0, 1])
def test_motive_words_on_a_slab_are_lost_and_come_back(light):
    H, W, seed = MOTIVE
    painted, plain, rects = panel_page(H, W, seed, bool(light))
    assert len(rects) >= 2
    seg = dict(SEG, light_text=light)
    plain_boxes, plain_counts = R.segment_page(plain, **seg)
    on_slab = [b for b in plain_boxes if any(_inside(b, r) for r in rects)]
    assert len(on_slab) >= 4 * len(rects)                                       # the words the slabs carry
    # segmentation alone: one box per slab, and none of the words on it
    boxes, _ = R.segment_page(painted, **seg)
    for r in rects:
        in_rows = [b for b in boxes if b[1] < r[3] and b[3] > r[1]]
        assert len(in_rows) == 1 and in_rows[0][0] <= r[0] and in_rows[0][2] >= r[2] and in_rows[0][1] <= r[1] and in_rows[0][3] >= r[3]
    assert not any((boxes[:, :4] == b[:4]).all(axis=1).any() for b in on_slab)
    # cleaning: the slab is wider than max_w and goes as a rule, the words on it with it
    cleaned, ccounts = CR.clean_page(painted, threshold=128, light_text=light, max_w=150)
    assert ccounts[2] == len(rects)
    paper_side = (cleaned <= 128) if light else (cleaned > 128)
    for x0, y0, x1, y1 in rects:
        assert paper_side[y0:y1, x0:x1].all()
    cboxes, _ = R.segment_page(cleaned, **seg)
    assert not any(_inside(b, r) for b in cboxes for r in rects)
    # the stage: byte for byte the page before the slabs were painted, and its boxes row for row
    for thr in (128, -1):
        out, panels, counts = PR.invert_panels(painted, threshold=thr, light_text=light, **SEEDED)
        np.testing.assert_array_equal(out, plain)
        assert counts[3] == len(rects) and [tuple(p[:4]) for p in panels if p[7]] == rects
        assert counts[6] == sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in rects)
        got_boxes, got_counts = R.segment_page(out, **seg)
        np.testing.assert_array_equal(got_boxes, plain_boxes)
        np.testing.assert_array_equal(got_counts, plain_counts)
    again, _, _ = PR.invert_panels(plain, threshold=128, light_text=light, **SEEDED)              # a page without panels comes back identical
    np.testing.assert_array_equal(again, plain)


def _bar(w, h, holes=0, H=20, W=60):
    """a w x h bar at (5, 3) with `holes` light pixels in its second row, from its second column on, every other column"""
    page = np.full((H, W), 255, np.uint8)
    page[3:3 + h, 5:5 + w] = 0
    page[4, 6:6 + 2 * holes:2] = 255
    return page


def test_box_size_at_and_under_the_minimum():
    for w, h, found in ((8, 4, 1), (7, 4, 0), (8, 3, 0), (9, 5, 1)):
        _, panels, counts = PR.invert_panels(_bar(w, h, 1), **SMALL)
        assert counts[1] == found and len(panels) == found, (w, h)


def test_fill_percent_at_the_boundary_and_one_pixel_past_it():
    # hull 20 x 5 = 100: 60 ink pixels pass fill_percent 60, 59 do not
    for holes, ok in ((40, 1), (41, 0)):
        page = np.full((12, 40), 255, np.uint8)
        page[3:8, 5:25] = 0
        cut = [(y, x) for y in (4, 5, 6) for x in range(6, 24)][:holes]        # never the box's outermost rows and columns
        for y, x in cut:
            page[y, x] = 255
        out, panels, counts = PR.invert_panels(page, **SMALL)
        assert panels[0].tolist() == [5, 3, 25, 8, 3 * 40 + 5, 100 - holes, 100, ok] and counts[3] == ok
        assert (out != page).any() == bool(ok)


def test_min_inside_percent_at_the_boundary_and_one_pixel_past_it():
    # hull 25 x 8 = 200: 4 light pixels are 2 %, 3 are not
    for holes, ok in ((4, 1), (3, 0)):
        page = _bar(25, 8, holes)
        _, panels, counts = PR.invert_panels(page, **SMALL)
        assert panels[0].tolist()[5:] == [200 - holes, 200, ok], holes
    _, panels, _ = PR.invert_panels(_bar(25, 8, 0), **dict(SMALL, min_inside_percent=0))
    assert panels[0].tolist()[5:] == [200, 200, 1]


def test_hull_not_box_for_a_diamond_and_a_rotated_slab():
    for page in (diamond(12), rotated_slab(30, 90)):
        out, panels, counts = PR.invert_panels(page, **dict(SMALL, fill_percent=80))
        x0, y0, x1, y1, _, area, hull, ok = panels[0].tolist()
        assert ok == 1 and counts[3] == 1 and hull < (x1 - x0) * (y1 - y0)
        changed = out != page
        assert changed.sum() == hull and not changed[y0, x0] and not changed[y1 - 1, x1 - 1] and not changed[y0, x1 - 1] and not changed[y1 - 1, x0]
        np.testing.assert_array_equal(out[changed], 255 - page[changed])


def test_diagonal_touch_under_both_connectivities():
    page = np.full((14, 40), 255, np.uint8)
    page[1:6, 2:14] = 0
    page[6:11, 14:26] = 0                                                        # touches the first at one corner only
    page[3, 4:10:2] = 255
    page[8, 16:22:2] = 255
    _, p4, c4 = PR.invert_panels(page, **dict(SMALL, connectivity=4, fill_percent=40))
    _, p8, c8 = PR.invert_panels(page, **dict(SMALL, connectivity=8, fill_percent=40))
    assert c4[:4].tolist() == [2, 2, 2, 2] and c8[:4].tolist() == [1, 1, 1, 1]
    assert p8[0].tolist()[:4] == [2, 1, 26, 11] and p8[0][6] == p4[0][6] + p4[1][6]


def test_max_panels_cuts_the_list():
    page = np.full((40, 40), 255, np.uint8)
    for i in range(3):
        page[2 + 12 * i:10 + 12 * i, 4:30] = 0
        page[5 + 12 * i, 6:20:2] = 255
    out, panels, counts = PR.invert_panels(page, max_panels=2, **SMALL)
    assert counts[1:4].tolist() == [3, 2, 2] and len(panels) == 2
    np.testing.assert_array_equal(out[26:], page[26:])                           # the third slab is copied as it is
    assert (out[2:10, 4:30] == 255 - page[2:10, 4:30]).all()


def test_bad_params_are_turned_down_by_the_mirror():
    import aocr
    for kw in (dict(fill_percent=0), dict(fill_percent=101), dict(min_inside_percent=-1), dict(min_inside_percent=100),
               dict(fill_percent=60, min_inside_percent=41), dict(min_w=0), dict(min_h=0), dict(connectivity=6), dict(threshold=255)):
        with pytest.raises(ValueError):
            aocr.PanelParams(**kw)
    p = aocr.PanelParams()
    assert [getattr(p, f) for f, _ in p._fields_] == [-1, 0, 8, 64, 24, 60, 2, 0]
    assert {k: getattr(p, k) for k in PR.DEFAULTS} == PR.DEFAULTS


def test_page_boxes_without_the_rider_reads_back_what_it_did(monkeypatch):
    """page_boxes with panels_dev left at None: the same calls of read_named and Tensor.cpu as before the argument existed; with the rider the
    same number of them, the first longer by the rider's words"""
    import aocr
    from aocr import page_pipeline as PP
    boxes = torch.arange(24, dtype=torch.int32).reshape(4, 6)
    counts = torch.tensor([3, 2, 128, 0], dtype=torch.int32)
    clean = torch.arange(8, dtype=torch.int32)
    monkeypatch.setattr(PP, "segment_page_device", lambda view, params, max_boxes, stream: (boxes, counts))
    named, reads = [], []
    real_named, real_cpu = PP.read_named, torch.Tensor.cpu
    monkeypatch.setattr(PP, "read_named", lambda pieces: (named.append({k: v for k, v in pieces.items() if v is not None}), real_named(pieces))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (reads.append(t.numel()), real_cpu(t, *a, **k))[1])
    page = torch.zeros((10, 20), dtype=torch.uint8)
    seg = aocr.SegmentParams()
    bare = PP.page_boxes(page, None, seg, 4, None, None, None, None)
    assert named == [] and reads == [4, 18] and bare.panels is None              # nothing rides: the counts as they are, then the boxes
    reads[:] = []
    old = PP.page_boxes(page, None, seg, 4, None, None, None, clean)
    new = PP.page_boxes(page, None, seg, 4, None, None, None, clean, None, None, None, None, None)
    assert len(named) == 2 and list(named[0]) == list(named[1]) == ["counts", "cleaned"] and reads == [12, 18, 12, 18]
    assert new.panels is None and sorted(vars(old)) == sorted(vars(new))
    rider = [torch.arange(8, dtype=torch.int32), torch.arange(16, dtype=torch.int32).reshape(2, 8)]
    reads[:] = []
    st = PP.page_boxes(page, None, seg, 4, None, None, None, clean, panels_dev=rider)
    assert list(named[2]) == ["counts", "cleaned", "panels"] and reads == [12 + 24, 18]
    np.testing.assert_array_equal(st.panels, np.concatenate([np.arange(8), np.arange(16)]))
    np.testing.assert_array_equal(st.cleaned, np.arange(8))
    np.testing.assert_array_equal(st.rows, boxes[:3].numpy())
