"""CPU: the numpy restatement of aocr_segment_page (tests/segment_ref.py) against hand answers that do not use it (tests/segment_cases.py),
the ctypes mirrors of the two structs, and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import segment_ref as R
from segment_cases import CASES


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_hand_answers(case):
    boxes, counts = R.segment_page(case["page"], **case["params"])
    np.testing.assert_array_equal(counts, case["counts"])
    np.testing.assert_array_equal(boxes, case["boxes"])


def test_hand_cases_cover_the_listed_events():
    names = {c["name"] for c in CASES}
    assert {"edge_rows", "merge_gap", "chain", "min_line_h", "word_gap", "word_gap_0", "min_word_w", "empty_line", "pad_clamp", "light_text",
            "constant", "all_ink", "otsu_two_level", "otsu_tie"} <= names


def test_otsu_by_hand():
    h = np.zeros(256, np.int64)
    h[50], h[200] = 24, 72
    assert R.otsu(h) == 50                                   # two levels a < b: a
    h = np.zeros(256, np.int64)
    h[10], h[20], h[30] = 12, 24, 12                         # both splits score 5760^2 / 432 = 76800 exactly
    assert R.otsu(h) == 10
    h = np.zeros(256, np.int64)
    h[7] = 99
    assert R.otsu(h) == -1                                   # one gray value: no split
    h = np.zeros(256, np.int64)
    h[254], h[255] = 3, 5
    assert R.otsu(h) == 254                                  # the last admissible t
    h = np.zeros(256, np.int64)
    h[0], h[1], h[255] = 100, 100, 1                         # the far outlier decides: {0,1 | 255}
    assert R.otsu(h) == 1


def test_truncation_keeps_the_true_count():
    page = np.full((8, 40), 255, np.uint8)
    for k in range(5):
        page[2:6, 8 * k:8 * k + 3] = 0                       # five words, 5 columns apart
    boxes, counts = R.segment_page(page, max_boxes=3, threshold=128, min_line_h=3, word_gap=4, min_word_w=2, pad_x=0, pad_y=0)
    assert counts.tolist() == [5, 1, 128, 0]
    np.testing.assert_array_equal(boxes, [[0, 2, 3, 6, 0, 12], [8, 2, 11, 6, 0, 12], [16, 2, 19, 6, 0, 12]])


def test_struct_mirrors():
    import aocr
    p = aocr.SegmentParams()
    assert C.sizeof(p) == 40 and C.sizeof(aocr._lib.Box) == 24
    assert (p.threshold, p.light_text, p.min_row_ink, p.merge_gap, p.min_line_h, p.word_gap, p.min_word_w, p.pad_x, p.pad_y, p.reserved) == \
        (-1, 0, 1, 2, 8, 12, 4, 2, 2, 0)
    assert {k: getattr(p, k) for k in R.DEFAULTS} == R.DEFAULTS
    q = aocr.SegmentParams(threshold=100, word_gap=0, pad_y=5)
    assert (q.threshold, q.word_gap, q.pad_y, q.merge_gap) == (100, 0, 5, 2)


def test_scratch_bytes_and_size_errors():
    import aocr
    f = aocr.lib.aocr_segment_scratch_bytes
    assert 0 < f(1, 1, 1) < 1 << 16
    a4 = f(3508, 2480, 1024)
    assert 3508 * 2480 < a4 < 4 * 3508 * 2480                # the per-band column profiles dominate
    assert f(16384, 4096, 4096) > 0
    for bad in ((0, 10, 10), (10, 0, 10), (16385, 1, 10), (1, 16385, 10), (16384, 4097, 10), (10, 10, 0), (10, 10, 4097)):
        assert f(*bad) == 0 and "bad sizes" in aocr.last_error(), bad


def test_entry_points_reject_bad_arguments_before_touching_the_device():
    """NULL pointers and bad sizes are refused on the host: nothing is enqueued, so this runs without a GPU."""
    import aocr
    p = aocr.SegmentParams()
    one = C.c_void_p(16)                                     # never dereferenced: every call below fails its checks first
    assert aocr.lib.aocr_segment_page(None, None, 10, 10, 10, C.byref(p), one, 4, one, one) != 0 and "NULL" in aocr.last_error()
    assert aocr.lib.aocr_segment_page(None, one, 9, 10, 10, C.byref(p), one, 4, one, one) != 0 and "pitch" in aocr.last_error()
    assert aocr.lib.aocr_segment_page(None, one, 10, 10, 10, C.byref(p), one, 5000, one, one) != 0 and "max_boxes" in aocr.last_error()
    for field, v in (("threshold", 255), ("threshold", -2), ("min_row_ink", 0), ("min_line_h", 0), ("min_word_w", 0), ("merge_gap", -1),
                     ("word_gap", -1), ("pad_x", -1), ("pad_y", -1)):
        q = aocr.SegmentParams()
        setattr(q, field, v)
        assert aocr.lib.aocr_segment_page(None, one, 10, 10, 10, C.byref(q), one, 4, one, one) != 0, field
        assert field in aocr.last_error(), (field, aocr.last_error())
    assert aocr.lib.aocr_crop_lines(None, one, 10, 10, 10, one, None, -1, 32, 100, one) != 0 and "n_boxes" in aocr.last_error()
    assert aocr.lib.aocr_crop_lines(None, one, 10, 10, 20000, one, None, 1, 32, 100, one) != 0 and "page size" in aocr.last_error()
    assert aocr.lib.aocr_crop_lines(None, one, 10, 10, 10, None, None, 1, 32, 100, one) != 0 and "NULL" in aocr.last_error()
    assert aocr.lib.aocr_crop_lines(None, one, 10, 10, 10, None, None, 0, 32, 100, None) == 0          # n_boxes == 0: a no-op


def test_bucket_width_rule():
    from aocr.page import bucket_width
    assert bucket_width(100, 32, 256) == 128                 # ceil(3.125 * 32) = 100 -> next multiple of 32
    assert bucket_width(10, 40, 256) == 32                   # aspect clamps at 0.5 -> 16 -> 32
    assert bucket_width(2000, 20, 256) == 256                # capped at max_img_w
    assert bucket_width(2000, 20, 100) == 100                # ... also where max_img_w is no multiple of the step
    assert bucket_width(64, 32, 256, width_step=4) == 64
