"""CPU: the numpy restatement of aocr_segment_page_spaced (tests/spacing_ref.py) against hand answers that do not use it
(tests/spacing_cases.py), against segment_ref.segment_page where every band chooses the same gap, and on glyph-atlas pages at three sizes,
where the defaults of aocr.SpacingParams must give exactly the placed words; the two-line page that no fixed word_gap cuts right; the
argument checks of the C entry point, which return before anything is enqueued and so need no device."""
import ctypes as C

import numpy as np
import pytest

import segment_ref as R
import spacing_ref as SR
from segment_cases import SEEDED, SEEDED_SHAPES, seeded_page
from spacing_atlas import SCALES, atlas_page, stacked_page
from spacing_cases import CASES, HAND, TWO_LINES, TWO_LINES_WORDS


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_hand_answers(case):
    boxes, counts, rows = SR.segment_page_spaced(case["page"], max_boxes=16, spacing=case["spacing"], **case["params"])
    np.testing.assert_array_equal(rows, case["rows"])
    np.testing.assert_array_equal(counts, case["counts"])
    np.testing.assert_array_equal(boxes, case["boxes"])


def test_hand_cases_cover_every_flag():
    flags = {int(f) for c in CASES for f in c["rows"][:, 1]}
    assert {0, 1, 2, 3, 4} <= flags, flags
    assert any(int(r[4]) == 255 for c in CASES for r in c["rows"])                     # a gap clipped at the last bin
    assert any(int(r[3]) + 1 == int(r[4]) and int(r[1]) == 0 for c in CASES for r in c["rows"])


def test_no_fixed_word_gap_cuts_the_two_lines():
    """today's segmentation cannot pass the two-line case: whatever word_gap, the count is not the six words painted."""
    p = CASES[0]["params"]
    seen = set()
    for g in range(1, 65):
        _, counts = R.segment_page(TWO_LINES, **dict(p, word_gap=g))
        assert counts[1] == 2 and counts[0] != TWO_LINES_WORDS, (g, counts)
        seen.add(int(counts[0]))
    assert seen == {18, 12, 10, 4, 2}, seen                                            # G = 1, 2..4, 5, 6..14, 15..
    _, counts, rows = SR.segment_page_spaced(TWO_LINES, spacing=HAND, **p)
    assert counts[0] == TWO_LINES_WORDS and rows[:, 0].tolist() == [3, 10]


def _one_gap_pages():
    """(page, params, spacing): pages and parameters under which every band may end with the same gap"""
    for c in CASES:
        yield c["page"], c["params"], c["spacing"]
    for H, W, _, _, seed in SEEDED_SHAPES:
        page = seeded_page(H, W, seed)
        for sp in (dict(HAND, min_gaps=10 ** 6, lo_percent=1, default_percent=1),      # every band takes the default, max(1, h / 100) = 1
                   dict(HAND, min_gaps=10 ** 6, lo_percent=1, default_percent=20, hi_percent=20), HAND, SR.SPACING):
            yield page, dict(SEEDED, threshold=128, light_text=0), sp
            yield page[:14], dict(SEEDED, threshold=128, light_text=0), sp             # a page of one or two lines


def test_equal_gaps_give_the_fixed_gap_segmentation():
    """on any page where all bands choose the same G, boxes and counts are those of segment_ref.segment_page(word_gap=G)."""
    hit, gaps = 0, set()
    for page, params, sp in _one_gap_pages():
        boxes, counts, rows = SR.segment_page_spaced(page, max_boxes=4096, spacing=sp, **params)
        if len(rows) == 0 or len(set(rows[:, 0].tolist())) != 1:
            continue
        G = int(rows[0, 0])
        fb, fc = R.segment_page(page, max_boxes=4096, **dict(params, word_gap=G))
        np.testing.assert_array_equal(boxes, fb)
        np.testing.assert_array_equal(counts, fc)
        hit += 1
        gaps.add(G)
    assert hit >= 12 and len(gaps) >= 4, (hit, gaps)
    assert any(len(SR.segment_page_spaced(seeded_page(H, W, s), spacing={}, **dict(SEEDED, threshold=128))[2]) >= 10 for H, W, _, _, s in SEEDED_SHAPES)


def _words_of(page, **kw):
    """per line the (x0, x1) of the boxes"""
    boxes, counts, rows = SR.segment_page_spaced(page, max_boxes=4096, threshold=128, pad_x=0, pad_y=0, min_word_w=2, **kw)
    return [[(int(b[0]), int(b[2])) for b in boxes if b[4] == ln] for ln in range(int(counts[1]))], rows


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("face", [0, 1, 2])
def test_defaults_give_the_placed_words_on_atlas_pages(face, scale):
    """all three faces at 1x, 2x and 3x, a one-word line and a two-word line among them: the defaults cut exactly the placed words."""
    page, placed = atlas_page(face, scale)
    got, rows = _words_of(page)
    assert got == placed, (face, scale, rows.tolist())
    assert [len(ws) for ws in placed] == [4, 1, 2, 4, 1]
    assert (rows[:, 1] & 3 == 0).any(), rows                                           # some line was estimated, not only defaulted


def test_stacked_page_needs_a_gap_per_line():
    """body text above its own 3x enlargement: the defaults cut both; the fixed default word_gap of 12 splits the large lines into letters."""
    page, placed = stacked_page()
    got, rows = _words_of(page)
    assert got == placed and len(placed) == 6
    assert rows[:3, 5].max() * 2 < rows[3:, 5].min() and rows[:3, 0].max() < rows[3:, 0].min(), rows
    _, fixed = R.segment_page(page, threshold=128, word_gap=12, min_word_w=2)
    assert fixed[0] > sum(len(r) for r in placed)


def test_argument_checks_need_no_device():
    import aocr
    one = C.c_void_p(4096)
    lib = aocr.lib
    assert lib.aocr_segment_spaced_scratch_bytes(40, 100, 16) == lib.aocr_segment_scratch_bytes(40, 100, 16) > 0
    for H, W, mb in ((0, 10, 4), (10, 16385, 4), (10, 10, 0), (10, 10, 4097)):
        assert lib.aocr_segment_spaced_scratch_bytes(H, W, mb) == 0 and "bad sizes" in aocr.last_error()

    def call(seg=None, sp=None, page=one, pitch=10, scratch=one, mb=4, boxes=one, counts=one, max_lines=4, rows=one, H=10, W=10):
        seg = seg if seg is not None else aocr.SegmentParams(threshold=128)
        sp = sp if sp is not None else aocr.SpacingParams()
        return lib.aocr_segment_page_spaced(None, page, pitch, H, W, C.byref(seg) if seg else None, C.byref(sp) if sp else None, scratch, mb, boxes,
                                            counts, max_lines, rows)

    for kw, word in ((dict(page=None), "NULL"), (dict(scratch=None), "NULL"), (dict(boxes=None), "NULL"), (dict(counts=None), "NULL"),
                     (dict(seg=False), "NULL"), (dict(sp=False), "NULL"), (dict(pitch=9), "pitch"), (dict(mb=5000), "max_boxes"),
                     (dict(H=0), "page size"), (dict(W=16385, pitch=16385), "page size"), (dict(max_lines=-1), "max_lines"),
                     (dict(rows=C.c_void_p(4098)), "aligned"), (dict(scratch=C.c_void_p(4104)), "aligned"),
                     (dict(seg=aocr.SegmentParams(threshold=128, word_gap=0)), "word_gap"),
                     (dict(seg=aocr.SegmentParams(threshold=300)), "threshold"),
                     (dict(sp=aocr.SpacingParams(min_gaps=0)), "min_gaps"),
                     (dict(sp=aocr.SpacingParams(lo_percent=0)), "lo_percent"),
                     (dict(sp=aocr.SpacingParams(lo_percent=50, default_percent=40)), "lo_percent"),
                     (dict(sp=aocr.SpacingParams(default_percent=90, hi_percent=80)), "hi_percent"),
                     (dict(sp=aocr.SpacingParams(hi_percent=401)), "hi_percent"),
                     (dict(sp=aocr.SpacingParams(ratio_percent=99)), "ratio_percent"),
                     (dict(sp=aocr.SpacingParams(ratio_percent=100001)), "ratio_percent")):
        assert call(**kw) != 0 and word in aocr.last_error(), (kw, aocr.last_error())
    bad = aocr.SpacingParams()
    bad.reserved[1] = 1
    assert call(sp=bad) != 0 and "reserved" in aocr.last_error()
    assert call(rows=C.c_void_p(4096 + 64), scratch=C.c_void_p(4096 + 64)) != 0 and "overlaps" in aocr.last_error()
    d = aocr.SpacingParams()
    assert (d.min_gaps, d.lo_percent, d.hi_percent, d.default_percent, d.ratio_percent) == tuple(SR.SPACING[k] for k in
            ("min_gaps", "lo_percent", "hi_percent", "default_percent", "ratio_percent")) and C.sizeof(d) == 32
