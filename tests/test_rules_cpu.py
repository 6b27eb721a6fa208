"""CPU: the two restatements of aocr_remove_rules (tests/rules_ref.py) against each other and against hand answers, the form page of the
motive through the restatement chain, the condition on the seeded pages that the GPU test relies on, and the host surface that needs no
device (RuleParams, the rules= option)."""
import functools
import inspect

import numpy as np
import pytest

import components_ref as CR
import rules_ref as RR
import segment_ref as R
from rules_cases import CASES, MOTIVE_RULES, MOTIVE_SEG, MOTIVE_WORDS, SEEDED, SEEDED_SHAPES, motive_page, ruled_page
from segment_cases import seeded_page


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_cases(case):
    for fn in (RR.remove_rules, RR.remove_rules_by_runs):
        out, counts = fn(case["page"], **case["params"])
        np.testing.assert_array_equal(out, case["out"], err_msg=case["name"])
        np.testing.assert_array_equal(counts, case["counts"], err_msg=case["name"])
    if case["name"] in ("nothing", "one_gray", "filled_block"):
        np.testing.assert_array_equal(case["out"], case["page"])


def test_hand_cases_cover_what_they_claim():
    by = {c["name"]: c for c in CASES}
    assert by["light_text"]["page"][0, 0] == 0 and by["light_text"]["out"][3, 1] == 0        # erased pixels become 0
    assert by["o_on_rule_edge_1"]["counts"][2] - by["o_on_rule_edge_0"]["counts"][2] == 2     # one row of the o's bottom, between its stems
    assert by["stem_through_underline"]["out"][2, 3] == 0                                     # the stem keeps its pixel inside the rule's row
    frame = by["page_edges"]["page"] == 0
    assert frame[0].all() and frame[-1].all() and frame[:, 0].all() and frame[:, -1].all()


@functools.lru_cache(maxsize=None)
def _seeded(shape, thr, light, axes):
    H, W, _, _, seed = shape
    page = ruled_page(H, W, seed, bool(light))
    page.setflags(write=False)
    return page, RR.remove_rules(page, threshold=thr, light_text=light, axes=axes, **SEEDED)


@pytest.mark.parametrize("shape", SEEDED_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SEEDED_SHAPES])
def test_formulations_agree_and_every_class_occurs_on_seeded_pages(shape):
    for thr, light in ((128, 0), (-1, 0), (128, 1), (-1, 1)):
        page, (out, counts) = _seeded(shape, thr, light, 3)
        assert counts[0] == thr if thr >= 0 else 0 <= counts[0] <= 254
        assert min(counts[3:7]) > 0, (shape, thr, light, counts)                  # cross, byH, byV and kept candidates: the condition
        assert counts[2] == counts[3] + counts[4] + counts[5] and counts[2] < counts[1]
        assert ((out != page) == (out == (0 if light else 255)) & (out != page)).all()
    for axes in (1, 2, 3):
        page, (out, counts) = _seeded(shape, 128, 0, axes)
        out2, counts2 = RR.remove_rules_by_runs(page, threshold=128, light_text=0, axes=axes, **SEEDED)
        np.testing.assert_array_equal(out, out2)
        np.testing.assert_array_equal(counts, counts2)
        if axes == 1:
            assert counts[3] == counts[5] == 0
        if axes == 2:
            assert counts[3] == counts[4] == 0


def test_formulations_agree_at_other_params():
    page = seeded_page(40, 100, 3)
    for L, T, e in ((2, 1, 0), (3, 2, 4), (9, 4, 2), (17, 16, 4), (30, 3, 1), (101, 2, 1)):
        a = RR.remove_rules(page, threshold=128, min_len=L, max_thick=T, edge=e)
        b = RR.remove_rules_by_runs(page, threshold=128, min_len=L, max_thick=T, edge=e)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    same, counts = RR.remove_rules(page, threshold=128, min_len=101, max_thick=2, edge=1)     # no run of 101 on a page 100 wide
    np.testing.assert_array_equal(same, page)
    assert counts[2] == 0 and counts[6] == 0


def _boxes(page):
    return R.segment_page(page, **MOTIVE_SEG)


def test_motive_form_page():
    plain, form = motive_page(False), motive_page(True)
    want_boxes, want_counts = _boxes(plain)
    assert int(want_counts[0]) == len(MOTIVE_WORDS) == 8 and int(want_counts[1]) == 4
    # today: the rules stay (clean's defaults find nothing 200 rows high) and fuse words and lines ...
    cleaned, ccounts = CR.clean_page(form, **dict(CR.DEFAULTS, threshold=128))
    assert ccounts[2] == 0
    fused, fcounts = _boxes(cleaned)
    assert int(fcounts[0]) < 8 and int(fcounts[1]) < 4
    assert fused[0, 2] - fused[0, 0] > 200 and fused[-1, 3] - fused[-1, 1] > 90          # one box per underline, one for the whole grid
    # ... or go as whole components and take along the letters that touch them: the two p of "pump", both words of the form line,
    # the h of the grid's "hill"
    cleaned, ccounts = CR.clean_page(form, **dict(CR.DEFAULTS, threshold=128, max_w=150))
    assert ccounts[2] == 3
    lost, lcounts = _boxes(cleaned)
    assert int(lcounts[0]) == 6 and int(lcounts[1]) == 3                                # the form line's words are gone with their line
    assert lost[0, 5] < want_boxes[0, 5] and lost[0, 0] > want_boxes[0, 0] and lost[0, 2] < want_boxes[0, 2]      # "um"
    assert lost[3, 5] < want_boxes[5, 5] and lost[3, 0] > want_boxes[5, 0] and lost[3, 2] == want_boxes[5, 2]     # "ill"
    # with the rules taken out per pixel: the ink of the page that was drawn without them, pixel for pixel, and so its boxes (the gray
    # values differ where a rule was drawn over the soft edge of a stem: darker inside the stem, paper next to it)
    out, counts = RR.remove_rules(form, **MOTIVE_RULES)
    np.testing.assert_array_equal(out <= 128, plain <= 128)
    got_boxes, got_counts = _boxes(out)
    np.testing.assert_array_equal(got_boxes, want_boxes)
    np.testing.assert_array_equal(got_counts, want_counts)
    assert counts[3] > 0 and counts[4] > 0 and counts[5] > 0 and counts[6] > 0     # the stems inside the rules are the candidates kept
    assert counts[1] - counts[2] == int((plain <= 128).sum())
    np.testing.assert_array_equal(RR.remove_rules_by_runs(form, **MOTIVE_RULES)[0], out)


def test_rule_params_validation():
    import aocr
    p = aocr.RuleParams()
    assert (p.threshold, p.light_text, p.axes, p.min_len, p.max_thick, p.edge, list(p.reserved)) == (-1, 0, 3, 100, 6, 1, [0, 0])
    assert {k: getattr(p, k) for k in ("axes", "min_len", "max_thick", "edge")} == {k: RR.DEFAULTS[k] for k in ("axes", "min_len", "max_thick", "edge")}
    for kw, word in ((dict(axes=0), "axes"), (dict(axes=4), "axes"), (dict(max_thick=0), "max_thick"), (dict(max_thick=17), "max_thick"),
                     (dict(min_len=6), "min_len"), (dict(min_len=16385), "min_len"), (dict(edge=-1), "edge"), (dict(edge=5), "edge"),
                     (dict(threshold=255), "threshold"), (dict(threshold=-2), "threshold")):
        with pytest.raises(ValueError, match=word):
            aocr.RuleParams(**kw)
    aocr.RuleParams(min_len=16384, max_thick=16, edge=4, axes=1, threshold=254)


def test_rules_option_is_validated_before_any_device_work():
    import aocr
    from aocr.page_pipeline import rule_params
    seg = aocr.SegmentParams(threshold=77, light_text=1)
    p = rule_params(seg, True)
    assert (p.threshold, p.light_text, p.axes, p.min_len, p.max_thick, p.edge) == (77, 1, 3, 100, 6, 1)
    mine = aocr.RuleParams(min_len=50)
    assert rule_params(seg, mine) is mine
    for bad in (3, "yes", 1.5, aocr.CleanParams()):
        with pytest.raises(ValueError, match="RuleParams"):
            rule_params(seg, bad)
    sig = inspect.signature(aocr.Model.recognize_page)
    assert sig.parameters["rules"].default is None and list(sig.parameters)[-1] == "rules"
