"""The numpy chain of tests/page_chain_ref.py on the planted photograph of tests/page_chain_cases.py, without a device: every stage has
something to do on it, none of the limits that would make recognize_page drop something is met, and turning panels, rules, binarize or
spacing off changes the number of boxes -- so that test_page_chain_gpu.py, which holds recognize_page to this chain, tests every stage."""
import time

import numpy as np
import pytest

import orient_ref as OR
import page_chain_cases as C
import page_chain_ref as R

LABEL_LIMIT = 4096                    # the component table of aocr_label_components at its default


@pytest.fixture(scope="module")
def chain():
    photo, _ = C.planted_photo()
    t0 = time.perf_counter()
    ref = R.read_page_ref(photo, C.SEGMENT, C.options_given())
    dt = time.perf_counter() - t0
    print(f"[page chain] photo {photo.shape} -> final page {ref.pages['final'].shape}: the numpy chain took {dt:.2f} s")
    assert photo.shape[0] * photo.shape[1] <= 1260 * 1680 and photo.dtype == np.uint8
    assert dt < 5.0, dt                                                         # a few seconds at the most: shrink the page otherwise
    return ref


@pytest.fixture(scope="module")
def blocks():
    photo, _ = C.planted_photo()
    return R.read_page_ref(photo, C.SEGMENT, dict(C.options_given(), layout=True, max_boxes=C.LAYOUT_MAX_BOXES))


def test_every_stage_ran_in_order(chain):
    assert tuple(chain.pages) == R.STAGES + ("final",)
    assert chain.pages["final"] is chain.pages["rules"]
    for a, b in zip(list(chain.pages)[:-2], list(chain.pages)[1:-1]):
        assert chain.pages[a].shape != chain.pages[b].shape or not np.array_equal(chain.pages[a], chain.pages[b]), f"{b} left the page as it was"


def test_every_stage_had_work(chain):
    w = chain.words
    print("[page chain] " + "; ".join(f"{k} {v.tolist()}" for k, v in w.items() if v.size <= 16))
    assert w["deskew"][1] != 0
    assert w["dewarp"][1] > 0 and np.any(w["curl_shifts"] != 0)
    assert w["rules"][2] > 0
    assert w["clean"][1] > 0
    assert w["binarize"][1] < w["binarize"][2]
    assert w["colour"][10] > 0 and w["colour"][4] > 0                            # red pixels counted, and dropped
    assert tuple(w["colour"][:3]) != (255, 255, 255) and w["colour"][3] == 1     # tinted paper, estimated
    assert np.any(chain.slant[:, 1] != 0) and np.all(chain.slant[:, 2] == 0)
    assert len(set(chain.spacing[:, 0].tolist())) >= 2
    assert chain.counts[2] == 127 and chain.seg["threshold"] == 127              # Otsu was asked for; binarize put 127 in its place
    assert chain.rectified and chain.resize == chain.pages["flatten"].shape + chain.pages["scale"].shape


def test_panel_inverted_and_its_words_found(chain):
    counts, rows = chain.words["panels"], chain.words["panel_rows"]
    assert counts[3] >= 1 and len(rows) == counts[2]
    x0, y0, x1, y1 = next(r[:4] for r in rows.tolist() if r[7])
    src = OR.unrotate_boxes(chain.rows[:, :4], *chain.turn)                      # the boxes on the page before the quarter turn: the panels' frame
    inside = [b for b in src.tolist() if x0 - 8 <= b[0] and b[2] <= x1 + 8 and y0 - 8 <= b[1] and b[3] <= y1 + 8]
    print(f"[page chain] panel {x0, y0, x1, y1}: {len(inside)} boxes inside it")
    assert len(inside) >= len(C.SLAB_WORDS)                                      # the line's own gap may cut a word once more


def test_glyph_estimate_calls_for_a_resize():
    photo, _ = C.planted_photo()
    ref = R.read_page_ref(photo, C.SEGMENT, dict(C.options_given(), scale=True, panels=None, clean=None, orient=None, deskew=None, dewarp=None,
                                                 rules=None, deslant=None, spacing=None))
    H, W = ref.pages["binarize"].shape
    print(f"[page chain] glyph words {ref.words['scale'].tolist()}: {(W, H)} -> {ref.shape}")
    assert ref.shape is not None and ref.shape[0] < W and ref.shape[1] < H
    assert ref.words["scale"][4] <= LABEL_LIMIT


def test_no_limit_is_met(chain, blocks):
    assert not chain.truncated and chain.counts[0] == len(chain.rows) <= 1024
    assert not blocks.truncated and max(blocks.block_found) <= C.LAYOUT_MAX_BOXES
    assert blocks.lcounts[3] == 0 and len(blocks.blocks) == blocks.lcounts[0] >= 2
    assert chain.words["panels"][1] <= R.MAX_PANELS
    assert chain.words["panels"][0] <= LABEL_LIMIT and chain.words["clean"][0] <= LABEL_LIMIT
    print(f"[page chain] {len(chain.rows)} boxes in {chain.counts[1]} lines as one column; {len(blocks.rows)} in {blocks.counts[1]} lines of "
          f"{len(blocks.blocks)} blocks, at most {max(blocks.block_found)} in one")
    assert len(blocks.rows) == blocks.counts[0] and len(blocks.spacing) == blocks.counts[1] == sum(blocks.n_block_lines)
    assert len(set(blocks.block_id.tolist())) == len(blocks.blocks) and np.all(np.diff(blocks.rows[:, 4]) >= 0)


@pytest.mark.parametrize("stage", ["panels", "rules", "binarize", "spacing"])
def test_turning_a_stage_off_changes_the_boxes(chain, stage):
    photo, _ = C.planted_photo()
    off = R.read_page_ref(photo, C.SEGMENT, dict(C.options_given(), **{stage: None}))
    print(f"[page chain] {len(chain.rows)} boxes, {len(off.rows)} without {stage}")
    assert len(off.rows) != len(chain.rows)
