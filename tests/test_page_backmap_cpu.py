"""CPU: aocr.page.backmap_corners -- the way from the final page's boxes back through curl, shear, quarter turn, resize and perspective warp
that Model.recognize_page publishes as its corner fields -- against the same maps composed by hand from the public point functions
(tests/backmap_ref.py, and written out in a straight line below), over all 32 on/off combinations of the five stages; and
aocr.page_pipeline.read_named, the one-sync readback, on CPU tensors.  No device and no model.  Everything is exact equality."""
import itertools

import numpy as np
import pytest
import torch

from aocr import page as P
from aocr.page_pipeline import read_named
from backmap_ref import corner_fields

H, W = 60, 90                                    # the final page: the one that was segmented
# a one-pixel box, a box in the page's last rows and columns, one whose shear source falls outside the page, the whole page, an inner box
BOXES = np.array([[10, 10, 11, 11], [80, 50, 90, 60], [0, 0, 5, 3], [0, 0, 90, 60], [33, 20, 64, 29]], np.int32)
SHIFTS, GROUP = np.array([-3, 0, 5], np.int32), 1                    # ng = 3 groups of 32 columns: both signs
SLOPES = (40000, -3000)                          # beyond the +-16384 clamp, and inside it
COEF = np.array([1.1, 0.05, 3.0, -0.02, 0.95, 2.0, 1e-3, 2e-3, 1.0])  # the denominator runs from 1 to about 1.3 over the page
FIELDS = ("uncurled_corners", "source_corners", "source_boxes", "unscaled_corners", "photo_corners")
DTYPES = dict(uncurled_corners=np.float64, source_corners=np.int64, source_boxes=np.int64, unscaled_corners=np.float64, photo_corners=np.float64)


def stages(on, quarter, slope, resized=True, sheet=True):
    """backmap_corners' arguments for the stages switched on; the page before the turn is (H0, W0), before the resize 70 x 200."""
    dewarp, deskew, orient, scale, rectify = on
    H0, W0 = (W, H) if quarter & 1 else (H, W)
    return dict(curl=(SHIFTS, GROUP) if dewarp else None, skew=(slope, H, W) if deskew else None,
                turn=(quarter, H0, W0) if orient else None,
                resize=((70, 200, H0, W0) if resized else ()) if scale else None,          # 70/H0 != 200/W0: the aspect changes
                warp=(COEF if sheet else ()) if rectify else None)


def same(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype == DTYPES[k] and got[k].shape == v.shape and np.array_equal(got[k], v), k


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("quarter", (1, 2))
@pytest.mark.parametrize("on", list(itertools.product((0, 1), repeat=5)), ids=lambda on: "".join(map(str, on)))
def test_every_combination_of_stages(on, quarter, slope):
    kw = stages(on, quarter, slope)
    got = P.backmap_corners(BOXES, **kw)
    assert sorted(got) == sorted(f for f, o in zip(FIELDS, on) if o)                     # each field with its own stage, and only then
    same(got, corner_fields(BOXES, **kw))
    n = len(BOXES)
    assert all(v.shape == ((n, 4) if k == "source_boxes" else (n, 4, 2)) for k, v in got.items())
    empty = P.backmap_corners(np.zeros((0, 4), np.int32), **kw)
    same(empty, corner_fields(np.zeros((0, 4), np.int32), **kw))
    assert all(v.shape == ((0, 4) if k == "source_boxes" else (0, 4, 2)) for k, v in empty.items())
    rows = np.concatenate([BOXES, np.full((n, 2), 7, np.int32)], axis=1)                 # (n, 6) rows x0 y0 x1 y1 line ink: the first four count
    same(P.backmap_corners(rows, **kw), got)


@pytest.mark.parametrize("quarter,slope", [(1, 40000), (3, -3000), (2, 40000), (0, 123)])
def test_every_stage_on_in_a_straight_line(quarter, slope):
    """all five stages, with no branch in the expectation: each map applied to the output of the one before."""
    H0, W0 = (W, H) if quarter & 1 else (H, W)
    got = P.backmap_corners(BOXES, (SHIFTS, GROUP), (slope, H, W), (quarter, H0, W0), (70, 200, H0, W0), COEF)
    cx, cy = P.box_corners(BOXES)
    ux, uy = P.uncurl_points(cx, cy, SHIFTS, GROUP)
    assert np.array_equal(ux, cx) and np.array_equal(uy, cy + P.curl_shift_q8(cx, SHIFTS, GROUP) / 256.0)
    assert (uy < cy).any() and (uy > cy).any()                                           # shifts of both signs are met
    sx, sy = P.source_points(ux.astype(np.int64), np.floor(uy + 0.5).astype(np.int64), slope, H, W)
    if abs(slope) > 16384:
        assert np.array_equal(sx, P.source_points(ux.astype(np.int64), np.floor(uy + 0.5).astype(np.int64), 16384, H, W)[0])   # the clamp
        assert (sy[2] < 0).any() or (sy[2] >= H).any()                                   # box 2's source is outside the page
    tx, ty = P.unrotate_points(sx, sy, quarter, H0, W0)
    vx, vy = P.unscale_points(tx, ty, 70, 200, H0, W0)
    px, py = P.warp_points(COEF, vx, vy)
    same(got, dict(uncurled_corners=np.stack([ux, uy], 2), source_corners=np.stack([tx, ty], 2), source_boxes=P.unrotate_boxes(BOXES, quarter, H0, W0),
                   unscaled_corners=np.stack([vx, vy], 2), photo_corners=np.stack([px, py], 2)))
    assert not np.array_equal(got["unscaled_corners"], got["source_corners"])
    dn = COEF[6] * vx + COEF[7] * vy + COEF[8]
    assert (np.abs(dn - 1) > 0.1).sum() > dn.size // 2                                   # a warp whose denominator is not 1


@pytest.mark.parametrize("on", list(itertools.product((0, 1), repeat=3)), ids=lambda on: "".join(map(str, on)))
def test_resize_and_warp_that_left_the_page_alone(on):
    """scale whose plan left the page alone, rectify that found no sheet: the fields are there and equal the corners that came in."""
    kw = stages(on + (1, 1), 3, -3000, resized=False, sheet=False)
    got = P.backmap_corners(BOXES, **kw)
    same(got, corner_fields(BOXES, **kw))
    coming = corner_fields(BOXES, **dict(kw, resize=(70, 200, 70, 200), warp=None))["unscaled_corners"]      # the identity resize
    assert np.array_equal(got["unscaled_corners"], coming) and np.array_equal(got["photo_corners"], coming)
    only_warp = P.backmap_corners(BOXES, **dict(kw, resize=None, warp=COEF))
    assert "unscaled_corners" not in only_warp
    assert np.array_equal(only_warp["photo_corners"], np.stack(P.warp_points(COEF, coming[:, :, 0], coming[:, :, 1]), 2))


def test_corner_order_of_an_odd_turn_without_and_with_dewarp():
    """orient=1 with rectify: without dewarp (and without deskew) the corners that go on are those of the un-rotated BOX, TL TR BR BL on the
    page as given; with dewarp they are the un-rotated corner POINTS, which start at the given page's BL.  The same four pixels, listed from
    another corner: recognize_page has always published them so, and backmap_corners keeps it."""
    flat = np.zeros(3, np.int32)                                                         # a dewarp that found no curl: the points do not move
    turn = (1, W, H)
    off = P.backmap_corners(BOXES, turn=turn, warp=COEF)["photo_corners"]
    on = P.backmap_corners(BOXES, curl=(flat, GROUP), turn=turn, warp=COEF)["photo_corners"]
    bx, by = P.box_corners(P.unrotate_boxes(BOXES, *turn))
    assert np.array_equal(off, np.stack(P.warp_points(COEF, bx.astype(np.float64), by.astype(np.float64)), 2))
    qx, qy = P.unrotate_points(*P.box_corners(BOXES), *turn)
    assert np.array_equal(on, np.stack(P.warp_points(COEF, qx.astype(np.float64), qy.astype(np.float64)), 2))
    assert not np.array_equal(on[1:], off[1:]) and np.array_equal(on, np.roll(off, 1, axis=1))     # (box 0 is one pixel: all four the same)
    even = (2, H, W)                                                                     # a half turn: the lists start two corners apart
    off2 = P.backmap_corners(BOXES, turn=even, warp=COEF)["photo_corners"]
    on2 = P.backmap_corners(BOXES, curl=(flat, GROUP), turn=even, warp=COEF)["photo_corners"]
    assert np.array_equal(on2, np.roll(off2, 2, axis=1))


def test_read_named(monkeypatch):
    a = torch.arange(4, dtype=torch.int32)
    b = torch.arange(10, 18, dtype=torch.int32)
    c = [torch.arange(20, 24, dtype=torch.int32), torch.arange(30, 33, dtype=torch.int32)]
    d = torch.arange(40, 52, dtype=torch.int32).reshape(2, 6)
    cats, reads = [], []
    real_cat, real_cpu = torch.cat, torch.Tensor.cpu
    monkeypatch.setattr(torch, "cat", lambda ts, *aa, **kk: (cats.append(len(ts)), real_cat(ts, *aa, **kk))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *aa, **kk: (reads.append(t.numel()), real_cpu(t, *aa, **kk))[1])
    got = read_named(dict(counts=a, skew=None, cleaned=b, curl=c, blocks=d))
    assert cats == [5] and reads == [4 + 8 + 7 + 12]                                     # one cat of the five pieces, one read of all words
    assert list(got) == ["counts", "cleaned", "curl", "blocks"] and got.get("skew") is None
    assert got["counts"].tolist() == [0, 1, 2, 3] and got["cleaned"].tolist() == list(range(10, 18))
    assert got["curl"].tolist() == [20, 21, 22, 23, 30, 31, 32]                          # a list comes back end to end under its one name
    assert got["blocks"].tolist() == list(range(40, 52)) and all(v.dtype == np.int32 for v in got.values())
    base = got["counts"].base
    assert base is not None and all(v.base is base for v in got.values())                # views of the one array that was read
    cats[:], reads[:] = [], []
    one = read_named(dict(counts=a, skew=None))
    assert list(one) == ["counts"] and cats == [1] and reads == [4]
