"""CPU: csrc/halo4_skip.h -- the block a (wave-row, mi) of gemm_halo4_bf16_kernel holds, the blocks whose products with one kernel row
are all padding, and the placement of a shortened half-step's reads and LDS-DMA pieces -- against an enumeration of the pixels.
The header is compiled alone by the host compiler into tests/halo4_skip_main.cc's program (no HIP, no device)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch-attention-ocr_amd", "csrc")
# (H, W) of the maps: tests/test_halo4_skip_gpu.py's shapes, the C3 workload's conv3 / conv4 (8 x 64) and conv5 / conv6 (4 x 64) maps, and
# the other widths the halo kernel takes (32, 128) at heights of one and of several tiles
MAPS = [(4, 64), (8, 64), (2, 128), (4, 128), (16, 64), (8, 32), (16, 32), (32, 128)]


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
    exe = str(tmp_path_factory.mktemp("halo4") / "halo4_skip_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "halo4_skip_main.cc"), "-o", exe], check=True, capture_output=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
        return [ln.split() for ln in out.splitlines()]
    return run


def _brute_dead(blk, dyi, W, H, y0):
    """every pixel of the block reads a row outside the map at halo row offset dyi (dy = dyi - 1)"""
    rows = [y0 + (blk * 32 + j) // W for j in range(32)]
    return all(not (0 <= y + dyi - 1 < H) for y in rows)


@pytest.mark.parametrize("H,W", MAPS, ids=[f"{h}x{w}" for h, w in MAPS])
def test_blocks_and_dead_blocks_match_the_pixel_enumeration(probe, H, W):
    R = 256 // W
    assert H % R == 0
    for y0 in range(0, H, R):
        lines = probe("map", W, H, y0)
        blocks = {(int(a[1]), int(a[2]), int(a[3])): tuple(int(v) for v in a[4:]) for a in lines if a[0] == "B"}
        counts = {(int(a[1]), int(a[2])): int(a[3]) for a in lines if a[0] == "N"}
        for il in (0, 1):
            owned = sorted(blocks[(il, wm, mi)][0] for wm in (0, 1) for mi in range(4))
            assert owned == list(range(8)), f"ownership {il}: every block of the tile exactly once"
        for (il, wm, mi), (blk, row, d0, d2) in blocks.items():
            assert blk == (2 * mi + wm if il else 4 * wm + mi)
            assert {y0 + (blk * 32 + j) // W for j in range(32)} == {row}, "a block lies in one map row"
            assert (d0, d2) == (int(_brute_dead(blk, 0, W, H, y0)), int(_brute_dead(blk, 2, W, H, y0))), (il, wm, mi)
            assert not _brute_dead(blk, 1, W, H, y0)
        for wm in (0, 1):
            dead0 = [blocks[(1, wm, mi)][2] for mi in range(4)]
            dead2 = [blocks[(1, wm, mi)][3] for mi in range(4)]
            n0, n2 = counts[(wm, 0)], counts[(wm, 2)]
            assert (n0, counts[(wm, 1)], n2) == (sum(dead0), 0, sum(dead2))
            assert dead0 == [1] * n0 + [0] * (4 - n0), "dead blocks of dy = -1 are the first mi"
            assert dead2 == [0] * (4 - n2) + [1] * n2, "dead blocks of dy = +1 are the last mi"
            assert n0 <= 2 and n2 <= 2
        if W >= 64:                                              # both wave-rows hold part of every map row: the skipped work is shared evenly
            assert counts[(0, 0)] == counts[(1, 0)] and counts[(0, 2)] == counts[(1, 2)]


def test_c3_maps_lose_the_expected_share(probe):
    """conv5 / conv6 (4 x 64, the tile is the image): one block of four is dead in six of the nine taps; conv3 / conv4 (8 x 64): in three of nine per tile."""
    for H, dead_taps in ((4, [6]), (8, [3, 3])):
        got = []
        for y0 in range(0, H, 4):
            c = {(int(a[1]), int(a[2])): int(a[3]) for a in probe("map", 64, H, y0) if a[0] == "N"}
            assert c[(0, 0)] == c[(1, 0)] and c[(0, 2)] == c[(1, 2)]
            got.append(3 * c[(0, 0)] + 3 * c[(0, 2)])
        assert got == dead_taps


def test_tap_rows(probe):
    t = {(int(a[1]), int(a[2])): int(a[3]) for a in probe("taps")}
    assert [t[(1, k)] for k in range(9)] == [0, 0, 0, 1, 1, 1, 2, 2, 2]          # forward: source row y + kh - 1
    assert [t[(-1, k)] for k in range(9)] == [2, 2, 2, 1, 1, 1, 0, 0, 0]         # data gradient: d y row y - kh + 1


# the half-steps the kernel instantiates: live mi = lo..hi-1 with 1 or 2 dead at either end; A reads of the live blocks only, or of all four
# (the reads of the next kernel row's first step), with and without a halo piece
PLANS = [(lo, hi, rlo, rhi, halo) for lo, hi in ((1, 4), (2, 4), (0, 3), (0, 2)) for rlo, rhi in ((lo, hi), (0, 4)) for halo in (0, 1)]


@pytest.mark.parametrize("lo,hi,rlo,rhi,halo", PLANS)
def test_shortened_half_step_plan(probe, lo, hi, rlo, rhi, halo):
    lines = probe("plan", lo, hi, rlo, rhi, halo)
    nm, no = (int(v) for v in lines[0][1:])
    ops = [(int(a[2]), int(a[3])) for a in lines[1:]]
    assert nm == 4 * (hi - lo) and no == len(ops)
    codes = [c for c, _ in ops]
    want = sorted([mi for mi in range(rlo, rhi)] + [4, 5, 6, 7] + [8, 9] + ([12] if halo else []))
    assert sorted(codes) == want, "every B read and DMA piece once, A reads of exactly the blocks asked for"
    dma = [c for c in codes if c >= 8]
    assert dma == sorted(dma), "the DMA pieces keep their order: weight piece, weight piece, halo piece"
    # the order of the full half-step, restricted to the ops that remain
    full = [c for mi in range(4) for c in ([mi] if rlo <= mi < rhi else []) + [4 + mi] + ([8 + mi] if mi < 2 else []) + ([12] if mi == 2 and halo else [])]
    assert codes == full
    at = [a for _, a in ops]
    assert at == sorted(at) and at[0] == 0 and at[-1] <= nm - 1
    per_gap = max(at.count(j) for j in set(at))
    if nm > no:                                                  # one dead block (the C3 maps): one op per gap, none behind the last MFMA
        assert per_gap == 1 and at[-1] <= nm - 2
    else:                                                        # two dead blocks (W = 128): eight MFMAs for eight to eleven ops
        assert per_gap <= (1 if nm == no else 2)
