"""Model.recognize_page with all of its stages on at once -- colour, rectify, flatten, binarize, scale, panels, clean, orient, deskew, dewarp,
rules, layout, deslant, spacing -- against tests/page_chain_ref.py, the same chain in numpy that never touches the device, on the planted
photograph of tests/page_chain_cases.py (test_page_chain_cpu.py shows that every stage has work to do on it).

a. every estimate given by value, as one column, at one crop width and with bucketed widths;
b. the same with layout=True and a small max_boxes;
c. the estimating forms rectify=True, scale=True, orient=True on the photograph lying on its side, with the which-way-up decision forced both ways by shifting the scores that
   the probe's second recognize_device call returns (the tensor returned to the host side of recognize_page; the device work is untouched);
d. the inverted page with light_text=1;
e. on a mismatch of the final page or of the boxes, the public stage functions are replayed one by one on the reference's pages and the
   assertion names the first stage that differs.
Every integer of the namespace is compared with assert_array_equal; the only floats are the scores, bit-equal to the same recogniser on
crops of the reference's final page, and the corner fields, equal as float64 to tests/backmap_ref.py.  The readbacks are counted and their
sizes spelled out as the sums of their parts, in the order the pipeline joins them."""
import math
import time

import numpy as np
import pytest
import torch

import page_chain_cases as C
import page_chain_ref as R
from model_harness import make

pytestmark = pytest.mark.gpu

SMALL = dict(enc_hidden=32, enc_layers=1, dec_layers=2, input_feed=True)
PAGE_B, MAX_IMG_W, LT = 32, 100, 12
BASE = {"boxes", "line", "ink", "text", "labels", "scores", "widths", "threshold", "n_found", "n_lines", "truncated"}
FIELDS = {
    "colour": {"colour_paper", "colour_balanced", "colour_hues", "colour_dropped"},
    "rectify": {"rectified", "rectify_quad", "rectify_size", "rectify_area", "photo_corners"},
    "flatten": {"flatten_radius"},
    "binarize": {"binarize_radius", "binarize_ink", "binarize_threshold_range"},
    "scale": {"scaled", "scale_size", "scale_quartiles", "scale_glyphs", "scale_shape", "unscaled_corners"},
    "panels": {"panels", "panel_counts"},
    "clean": {"clean_components", "clean_specks", "clean_rules", "clean_ink_removed"},
    "orient": {"orientation", "orient_runs", "orient_scores", "source_boxes"},
    "deskew": {"skew_steps", "skew_slope_q16", "skew_deg", "source_corners"},
    "dewarp": {"curl_shifts", "curl_group", "curl_max", "curl_pairs", "uncurled_corners"},
    "rules": {"rules_counts", "rules_erased", "rules_kept"},
    "layout": {"block", "blocks", "block_depth", "n_blocks", "layout_overflow"},
    "deslant": {"slant_q16", "slant_deg", "slant_flags", "slant_extent"},
    "spacing": {"word_gaps", "spacing_flags", "spacing_gaps"},
}


@pytest.fixture(scope="module")
def model(cuda):
    m, O, ocfg, P0, st, _ = make(SMALL, B=PAGE_B, W=MAX_IMG_W, maxlen=8, compute="f32", max_decoder_l=LT, max_beam=5)
    m.set_parameters(O.sharpen_params(P0), st)
    yield m
    m.check_health()
    m.shutdown()


_refs = {}


def reference(name, page, seg, options):
    """the numpy chain, once per case of this module; nothing changes it afterwards."""
    if name not in _refs:
        t0 = time.perf_counter()
        _refs[name] = R.read_page_ref(page, seg, options)
        print(f"[page chain] reference {name}: {time.perf_counter() - t0:.2f} s on the host")
    return _refs[name]


def device_options(options):
    """the options of the reference as recognize_page takes them: a dict of parameters becomes the stage's params object."""
    import aocr
    out = {k: v for k, v in options.items() if k not in ("half_turn",)}
    if isinstance(out.get("colour"), dict):
        out["colour"] = aocr.ColourParams(**out["colour"])
    return out


def read_page(m, page, params, options, shift=None, **kw):
    """(the namespace, the events of the call in order: the elements of every Tensor.cpu() and "rec" for every recognize_device, the st of
    the last _page_boxes).  shift: added to the scores that the SECOND recognize_device call returns -- the flipped crops of the
    which-way-up probe."""
    events, last, calls = [], [], [0]
    real_cpu, real_rec, real_boxes = torch.Tensor.cpu, m.recognize_device, m._page_boxes

    def rec(*a, **k):
        events.append("rec")
        calls[0] += 1
        lab, sc, clp, att = real_rec(*a, **k)
        if shift is not None and calls[0] == 2:
            sc = sc + shift
        return lab, sc, clp, att

    def boxes(*a, **k):
        last.append(real_boxes(*a, **k))
        return last[-1]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (events.append(t.numel()), real_cpu(t, *a, **k))[1])
        mp.setattr(m, "recognize_device", rec)
        mp.setattr(m, "_page_boxes", boxes)
        res = m.recognize_page(page, params, **device_options(options), **kw)
    return res, events, last


# ---- e. the first stage that differs -------------------------------------------------------------------------------------------------------------
def first_difference(ref, given, cuda):
    """replays the public device stage functions one by one, each on the reference's page before it, and returns the name of the first whose
    page is not the reference's page after it (None: every stage alone reproduces the reference)."""
    import aocr
    thr, light, paper = int(ref.seg["threshold"]), int(ref.seg["light_text"]), ref.paper
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    prev = given
    for name, want in ref.pages.items():
        if name == "final":
            break
        src = up(prev)
        if name == "colour":
            got = aocr.gray_page_device(src, aocr.ColourParams(**{k: ref.params["colour"][k] for k in ("drop", "fill", "balance")}), counts=True)[0]
        elif name == "rectify":
            got = aocr.warp_page_device(src, ref.warp, ref.size, paper) if ref.rectified else src
        elif name == "flatten":
            got = aocr.flatten_page_device(src, aocr.FlattenParams(light_text=light))
        elif name == "binarize":
            got = aocr.binarize_page_device(src, aocr.BinarizeParams(light_text=light), counts=True)[0]
        elif name == "scale":
            got = aocr.resize_page_device(src, ref.shape) if ref.shape is not None else src
        elif name == "panels":
            got = aocr.invert_panels_device(src, aocr.PanelParams(threshold=thr, light_text=light), R.MAX_PANELS)[0]
        elif name == "clean":
            got = aocr.clean_page_device(src, aocr.CleanParams(threshold=thr, light_text=light))[0]
        elif name == "orient":
            got = aocr.rotate_page_device(src, ref.quarter)
        elif name == "deskew":
            got = aocr.deskew_page_device(src, aocr.estimate_skew_device(src, aocr.SkewParams(threshold=thr, light_text=light)), paper)
        elif name == "dewarp":
            cp = aocr.CurlParams(threshold=thr, light_text=light)
            got = aocr.dewarp_page_device(src, aocr.estimate_curl_device(src, cp)[1], cp.group, paper)
        elif name == "rules":
            got = aocr.remove_rules_device(src, aocr.RuleParams(threshold=thr, light_text=light))[0]
        else:
            raise AssertionError(name)
        got = got.cpu().numpy()
        if got.shape != want.shape or not np.array_equal(got, want):
            return name
        prev = want
    return None


def check_page_and_boxes(res, st, ref, given, cuda):
    """the page that was segmented and the boxes on it; a mismatch names the first stage that differs."""
    final = st.page.cpu().numpy()
    same = final.shape == ref.pages["final"].shape and np.array_equal(final, ref.pages["final"]) and \
        res.boxes.shape == ref.rows[:, :4].shape and np.array_equal(res.boxes, ref.rows[:, :4])
    if not same:
        stage = first_difference(ref, given, cuda)
        where = f"the first stage that differs from the reference on its own is {stage}" if stage is not None else \
            "every stage alone reproduces the reference: what is handed from one stage to the next, or the segmentation, differs"
        raise AssertionError(f"final page {final.shape} against {ref.pages['final'].shape}, {len(res.boxes)} boxes against {len(ref.rows)}: {where}")


# ---- the namespace against the reference ---------------------------------------------------------------------------------------------------------
def same(got, want, dtype=None):
    want = np.asarray(want)
    got = np.asarray(got)
    if dtype is not None:
        assert got.dtype == dtype, (got.dtype, dtype)
    np.testing.assert_array_equal(got, want)


def check_fields(m, res, ref, options, cuda, width, width_step=32, orient_scores=False):
    """every field of the namespace but the layout's, which check_layout holds."""
    o = options
    n = len(ref.rows)
    assert n > 0
    same(res.boxes, ref.rows[:, :4], np.int32)
    same(res.line, ref.rows[:, 4], np.int32)
    same(res.ink, ref.rows[:, 5], np.int32)
    assert (res.n_found, res.n_lines, res.threshold) == ref.counts and res.truncated is False
    w = ref.words
    if R.asked(o.get("colour")):
        assert res.colour_paper == tuple(int(v) for v in w["colour"][:3]) and res.colour_balanced is bool(ref.params["colour"]["balance"])
        same(res.colour_hues, w["colour"][4:10], np.int64)
        assert res.colour_dropped == int(w["colour"][10])
    assert res.flatten_radius == 16
    assert (res.binarize_radius, res.binarize_ink, res.binarize_threshold_range) == (20, int(w["binarize"][0]), (int(w["binarize"][1]), int(w["binarize"][2])))
    same(res.panel_counts, w["panels"], np.int64)
    same(res.panels, w["panel_rows"], np.int32)                                  # in the coordinates of the page before the quarter turn
    assert (res.clean_components, res.clean_specks, res.clean_rules, res.clean_ink_removed) == tuple(int(w["clean"][i]) for i in (0, 1, 2, 5))
    assert res.orientation == ref.quarter
    if o["orient"] is True:
        assert res.orient_runs == (int(w["orient"][1]), int(w["orient"][2])) and isinstance(res.orient_scores, tuple) and len(res.orient_scores) == 2
    else:
        assert (res.orient_runs, res.orient_scores) == (None, None)
    assert (res.skew_steps, res.skew_slope_q16) == (int(w["deskew"][0]), int(w["deskew"][1]))
    assert res.skew_deg == math.degrees(math.atan(int(w["deskew"][1]) / 65536.0))
    same(res.curl_shifts, w["curl_shifts"], np.int32)
    assert (res.curl_group, res.curl_max, res.curl_pairs) == (ref.curl_group, int(w["dewarp"][1]), int(w["dewarp"][3]))
    same(res.rules_counts, w["rules"], np.int64)
    assert (res.rules_erased, res.rules_kept) == (int(w["rules"][2]), int(w["rules"][6]))
    same(res.slant_q16, ref.slant[:, 1], np.int32)
    same(res.slant_flags, ref.slant[:, 2], np.int32)
    same(res.slant_extent, ref.extent, np.int32)
    same(res.slant_deg, np.degrees(np.arctan(ref.slant[:, 1].astype(np.int32) / 65536.0)), np.float64)
    same(res.word_gaps, ref.spacing[:, 0], np.int32)
    same(res.spacing_flags, ref.spacing[:, 1], np.int32)
    same(res.spacing_gaps, ref.spacing[:, 2], np.int32)
    assert len(res.word_gaps) == res.n_lines
    if o["scale"] is True:
        g = w["scale"]
        assert (res.scaled, res.scale_size, res.scale_quartiles, res.scale_glyphs, res.scale_shape) == \
            (ref.shape is not None, int(g[0]), (int(g[1]), int(g[2])), int(g[3]), ref.shape)
    else:
        assert (res.scaled, res.scale_size, res.scale_quartiles, res.scale_glyphs, res.scale_shape) == (True, None, None, None, ref.shape)
    assert (res.rectified, res.rectify_size, res.rectify_area) == (True, ref.size, ref.area)
    same(res.rectify_quad, ref.quad, np.int64)
    want = ref.corners()
    assert sorted(want) == ["photo_corners", "source_boxes", "source_corners", "uncurled_corners", "unscaled_corners"]
    for k, v in want.items():
        got = getattr(res, k)
        assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v), k
    # the crop widths: one bucket, or DataGen's rule on the box widened by the slant's extent on either side
    import aocr
    from aocr.page import bucket_width
    if width is not None:
        widths = np.full(n, width, np.int64)
    else:
        widths = np.array([bucket_width(int(r[2] - r[0]) + 2 * int(d), int(r[3] - r[1]), MAX_IMG_W, width_step) for r, d in zip(ref.rows, ref.extent)], np.int64)
        plain = np.array([bucket_width(int(r[2] - r[0]), int(r[3] - r[1]), MAX_IMG_W, width_step) for r in ref.rows], np.int64)
        assert np.any(plain != widths), "no box whose bucket the slant's extent changes"
    same(res.widths, widths, np.int64)
    # the recogniser on crops of the REFERENCE's final page at the reference's boxes and slants
    final = torch.from_numpy(ref.pages["final"]).to(cuda)
    boxes_dev = torch.from_numpy(np.ascontiguousarray(ref.rows)).to(cuda)
    slant_dev = torch.from_numpy(np.ascontiguousarray(ref.slant)).to(cuda)
    for wd in sorted(set(widths.tolist())):
        members = np.nonzero(widths == wd)[0]
        for c0 in range(0, len(members), PAGE_B):
            idx = members[c0:c0 + PAGE_B]
            idx_dev = torch.from_numpy(idx).to(cuda)
            got = m.recognize(aocr.crop_lines_slanted_device(final, boxes_dev[idx_dev], None, slant_dev[idx_dev], int(wd), 32, ref.paper))
            np.testing.assert_array_equal(res.labels[idx], got.labels)
            np.testing.assert_array_equal(res.scores[idx].view(np.int32), got.scores.view(np.int32))
            assert [res.text[i] for i in idx] == got.text
    assert res.labels.dtype == np.int32 and res.scores.dtype == np.float32 and res.labels.shape == (n, LT)
    names = set(BASE)
    for k, v in o.items():
        if k in FIELDS and R.asked(v):
            names |= FIELDS[k]
    assert set(vars(res)) == names, set(vars(res)) ^ names


def riders(ref, colour=True):
    """the elements that ride with the first readback, in the order page_boxes joins them: skew, cleaned, curl, colour, rules, panels,
    binarize."""
    ng = len(ref.words["curl_shifts"])
    return 4 + 8 + (4 + ng) + (16 if colour else 0) + 8 + (8 + 8 * R.MAX_PANELS) + 4


def reads_single(ref, colour=True):
    n, lines = len(ref.rows), ref.counts[1]
    return [4 + riders(ref, colour), 6 * n + 4 * n + 8 * lines]                 # the counts with the riders; boxes, slant words, spacing rows


def reads_layout(ref, max_boxes):
    nb = len(ref.blocks)
    gap_rows = sum((int(b[3] - b[1]) + 1) // 2 for b in ref.blocks)              # what every block's spacing buffer holds: (height + 1) // 2 rows
    return [4 + 4 + riders(ref) + 6 * R.MAX_BLOCKS, 4 * nb + 6 * nb * max_boxes + 4 * nb * max_boxes + 8 * gap_rows]


def loop_reads(events, n_chunks):
    """what follows the boxes: for every chunk one recognize_device, then its labels and its scores."""
    assert [e == "rec" for e in events] == [True, False, False] * n_chunks, events


def chunks(widths):
    return sum(-(-int((widths == w).sum()) // PAGE_B) for w in set(widths.tolist()))


# ---- a. values given, one column ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,width_step", [(100, 32), (None, 8)])
def test_every_stage_values_given(cuda, model, width, width_step):
    import aocr
    photo, _ = C.planted_photo()
    options = C.options_given()
    ref = reference("given", photo, C.SEGMENT, options)
    params = aocr.SegmentParams(**C.SEGMENT)
    assert params.threshold == -1
    t0 = time.perf_counter()
    res, events, sts = read_page(model, photo, params, options, width=width, width_step=width_step)
    dt = time.perf_counter() - t0
    assert params.threshold == -1 and res.threshold == 127                       # the caller's object is not modified
    assert len(sts) == 1
    check_page_and_boxes(res, sts[0], ref, photo, cuda)
    check_fields(model, res, ref, options, cuda, width, width_step)
    at = events.index("rec")
    assert events[:at] == reads_single(ref), (events[:at], reads_single(ref))
    loop_reads(events[at:], chunks(res.widths))
    print(f"[page chain] values given, width {width}: {len(ref.rows)} boxes in {ref.counts[1]} lines, widths {sorted(set(res.widths.tolist()))}, "
          f"reads {events[:at]}; recognize_page took {dt:.2f} s")


# ---- b. the same with layout ---------------------------------------------------------------------------------------------------------------------------
def test_every_stage_layout(cuda, model):
    import aocr
    photo, _ = C.planted_photo()
    mb = C.LAYOUT_MAX_BOXES
    options = dict(C.options_given(), layout=True, max_boxes=mb)
    ref = reference("layout", photo, C.SEGMENT, options)
    params = aocr.SegmentParams(**C.SEGMENT)
    res, events, sts = read_page(model, photo, params, options, width=100)
    check_page_and_boxes(res, sts[0], ref, photo, cuda)
    nb = len(ref.blocks)
    assert nb >= 2 and res.n_blocks == nb and res.layout_overflow is False and max(ref.block_found) <= mb
    same(res.blocks, ref.blocks[:, :4], np.int32)
    same(res.block_depth, ref.blocks[:, 4], np.int32)
    same(res.block, ref.block_id, np.int32)
    # the line numbers run on across the blocks, and the spacing rows with them
    firsts = np.cumsum([0] + ref.n_block_lines[:-1])
    for b in range(nb):
        lines = res.line[res.block == b]
        assert lines.min() >= firsts[b] and lines.max() < firsts[b] + ref.n_block_lines[b], (b, lines, firsts)
    assert len(res.word_gaps) == sum(ref.n_block_lines) == res.n_lines
    check_fields(model, res, ref, options, cuda, 100)
    at = events.index("rec")
    assert events[:at] == reads_layout(ref, mb), (events[:at], reads_layout(ref, mb))
    loop_reads(events[at:], chunks(res.widths))
    print(f"[page chain] layout: {len(ref.rows)} boxes in {ref.counts[1]} lines of {nb} blocks (lines per block {ref.n_block_lines}), slants "
          f"{res.slant_q16[res.slant_q16 != 0].tolist()}, reads {events[:at]}")


# ---- c. the estimating forms, the restart forced both ways ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
def test_estimating_forms(cuda, model, flip):
    import aocr
    upright, _ = C.planted_photo()
    photo = np.ascontiguousarray(np.rot90(upright))                               # lying on its side: the estimate has a quarter turn to find
    options = dict(C.options_estimated(), half_turn=flip)
    ref = reference(f"estimated_{int(flip)}", photo, C.SEGMENT, options)
    first = reference("estimated_0", photo, C.SEGMENT, dict(options, half_turn=False))
    params = aocr.SegmentParams(**C.SEGMENT)
    res, events, sts = read_page(model, photo, params, options, shift=1000.0 if flip else -1000.0, width=100)
    assert len(sts) == (2 if flip else 1)
    check_page_and_boxes(res, sts[-1], ref, photo, cuda)
    assert res.orientation == ((int(first.words["orient"][0]) + (2 if flip else 0)) & 3)
    assert (res.orient_scores[1] > res.orient_scores[0]) is flip and abs(res.orient_scores[1] - res.orient_scores[0]) > 500.0
    assert int(first.words["orient"][0]) == 1 and first.rectified                # so the restart's turn of the page before the first turn shows
    assert ref.shape is not None and ref.shape != first.pages["binarize"].shape[::-1]      # the glyph estimate asked for a resize
    check_fields(model, res, ref, options, cuda, 100)
    # three more reads than with the values given, in the order of the stages: the quad's 16 words, the glyph size's 8, the orientation's 8;
    # then the two of the boxes, the probe (two recognize_device calls, one read of the two mean scores) and, after a flip, the two again
    want = [16, 8, 8] + reads_single(first) + ["rec", "rec", 2] + (reads_single(ref) if flip else [])
    assert events[:len(want)] == want, (events[:len(want)], want)
    loop_reads(events[len(want):], chunks(res.widths))
    print(f"[page chain] estimating forms, flip {flip}: quad area {res.rectify_area}, glyphs {res.scale_size} {res.scale_quartiles} x{res.scale_glyphs} -> "
          f"{res.scale_shape}, runs {res.orient_runs}, orientation {res.orientation}, scores {res.orient_scores}, {len(ref.rows)} boxes")


# ---- d. polarity ---------------------------------------------------------------------------------------------------------------------------------------
def test_polarity(cuda, model):
    import aocr
    gray, _ = C.gray_photo()
    options = dict(C.options_given(), colour=None)
    dark = reference("dark", gray, C.SEGMENT, options)
    light_seg = dict(C.SEGMENT, light_text=1)
    light = reference("light", np.ascontiguousarray(255 - gray), light_seg, options)
    assert light.paper == 0 and dark.paper == 255
    runs = {}
    for name, page, seg, ref in (("dark", gray, C.SEGMENT, dark), ("light", np.ascontiguousarray(255 - gray), light_seg, light)):
        res, events, sts = read_page(model, page, aocr.SegmentParams(**seg), options, width=100)
        check_page_and_boxes(res, sts[0], ref, page, cuda)
        check_fields(model, res, ref, options, cuda, 100)
        at = events.index("rec")
        assert events[:at] == reads_single(ref, colour=False), events[:at]
        runs[name] = res
    d, l = runs["dark"], runs["light"]
    for k in ("boxes", "line", "slant_q16", "slant_flags", "slant_extent", "word_gaps", "spacing_flags", "spacing_gaps"):
        np.testing.assert_array_equal(getattr(d, k), getattr(l, k), err_msg=k)
    print(f"[page chain] polarity: {len(d.boxes)} boxes, the same dark on light and light on dark; fills 255 and 0")
