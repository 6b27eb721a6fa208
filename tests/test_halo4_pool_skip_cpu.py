"""CPU: csrc/halo4_skip.h's row-split order of a (2,1)-pooled tile of gemm_halo4_bf16_kernel -- which map row and x range a (wave-row, mi)
holds, where its pool partner sits, which of the tile's 128 pooled rows a pair leaves, and the dead counts -- against an enumeration of the
pixels.  The header is compiled alone by the host compiler into tests/halo4_pool_main.cc's program (no HIP, no device)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch-attention-ocr_amd", "csrc")
# (W, H, y0): conv6's map (the tile is the image), conv4's two tiles, and the 128-wide maps of one and of two tiles
CASES = [(64, 4, 0), (64, 8, 0), (64, 8, 4), (128, 2, 0), (128, 4, 0), (128, 4, 2)]


def _host_cxx():
    for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = _host_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("halo4pool") / "halo4_pool_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "halo4_pool_main.cc"), "-o", exe], check=True, capture_output=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
        return [ln.split() for ln in out.splitlines()]
    return run


def _pixels(blk, W, y0):
    """(map row, x) of the block's 32 pixels: the tile is 256 / W whole map rows from y0 on, in plain order"""
    return [(y0 + (blk * 32 + j) // W, (blk * 32 + j) % W) for j in range(32)]


@pytest.mark.parametrize("W,H,y0", CASES, ids=[f"{w}x{h}@{y}" for w, h, y in CASES])
def test_row_split_order_matches_the_pixel_enumeration(probe, W, H, y0):
    lines = probe("map", W, H, y0)
    assert lines[0] == ["E", "1"]
    blocks = {(int(a[1]), int(a[2])): tuple(int(v) for v in a[3:]) for a in lines if a[0] == "B"}
    counts = {(int(a[1]), int(a[2])): int(a[3]) for a in lines if a[0] == "N"}
    assert sorted(b[0] for b in blocks.values()) == list(range(8)), "every block of the tile exactly once"
    pooled = []
    for (wm, mi), (blk, row, top, pmi, prow) in blocks.items():
        px = _pixels(blk, W, y0)
        assert {y for y, _ in px} == {row}, "a block lies in one map row"
        assert top == int((row - y0) % 2 == 0), "upper rows of the windows: even rows of the tile (y0 is even)"
        if not top:
            assert (pmi, prow) == (-1, -1)
            continue
        assert pmi == mi + W // 64 and pmi < 4
        pblk, prow_map, ptop = blocks[(wm, pmi)][:3]                       # the partner: the SAME wave-row
        assert ptop == 0 and prow_map == row + 1
        assert [x for _, x in _pixels(pblk, W, y0)] == [x for _, x in px], "the partner has the same x range, lane for lane"
        # pooled row inside the tile: (tile row pair) * W + x, 32 consecutive ones per pair of blocks
        assert prow == ((row - y0) // 2) * W + px[0][1]
        pooled += [((y - y0) // 2) * W + x for y, x in px]
        assert pooled[-32:] == list(range(prow, prow + 32))
    assert sorted(pooled) == list(range(128)), "the pairs cover the tile's 128 pooled rows exactly once"
    for wm in (0, 1):
        for dyi in (0, 1, 2):
            dead = [all(not (0 <= y + dyi - 1 < H) for y, _ in _pixels(blocks[(wm, mi)][0], W, y0)) for mi in range(4)]
            n = counts[(wm, dyi)]
            assert n == sum(dead)
            assert dead == ([True] * n + [False] * (4 - n) if dyi == 0 else [False] * (4 - n) + [True] * n), "the first n / the last n of the four"
    got = (counts[(0, 0)], counts[(0, 2)])
    assert got == (counts[(1, 0)], counts[(1, 2)]), "both wave-rows lose the same blocks"
    # each is one of the seven loop bodies the kernel has: (0,0) (1,1) (1,0) (0,1) (2,2) (2,0) (0,2)
    assert got == {(64, 4, 0): (1, 1), (64, 8, 0): (1, 0), (64, 8, 4): (0, 1), (128, 2, 0): (2, 2), (128, 4, 0): (2, 0), (128, 4, 2): (0, 2)}[(W, H, y0)]


def test_width_32_is_ineligible(probe):
    """at W = 32 a block is a whole map row and its pool partner, block 2 mi + wm + 1, belongs to the other wave-row"""
    assert probe("map", 32, 8, 0) == [["E", "0"]]
    assert probe("map", 256, 2, 0) == [["E", "0"]]
