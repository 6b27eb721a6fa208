"""GPU: the (2,1)-pooled launches of gemm_halo4_bf16_kernel (conv4 / conv6 forward) in the skipping form with the row-split pixel order
(csrc/halo4_skip.h: the tile's pixels in plain order, a pool window taken from acc[mi] and acc[mi + W / 64] of one lane; the default at map
widths 64 and 128 where every tile leaves as the staged pooled bf16 + arg-max tile) against the kernel's first form
(AOCR_NO_HALO4_POOL_SKIP=1), bit for bit, and against the float64 (2,1)-maximum of the convolution on the bf16-rounded operands with
tests/test_halo4_skip_gpu.py's bound: one bf16 rounding + BOUND_C * sqrt(K) * 2^-24 * (|A| |B|) per element.

Through tests/libkprobe.so's kp_conv_forward, bf16 shadows, 3 x 3, pad 1, Cin = Cout = 256, pool 2, two 256-pixel tiles per shape:
  (B, H, W) = (2, 4, 64)   conv6's map: a tile is a whole image, first AND last map row in it
              (1, 8, 64)   conv4's map: the upper tile has the first map row, the lower one the last
              (2, 2, 128)  two rows: every block's row is first or last, two dead blocks per wave and kernel row
each with the ReLU off and on.  With it on about half the windows tie at 0, the arg-max rule's only hard case: a tie picks the upper row.
Every output buffer starts as sentinels.  Which form ran is read from the AOCR_TRACE line: this form's ends in " pskip".  A width of 32
(the partner row belongs to the other wave-row), an fp32 destination and AOCR_HALO4_STAGED without its pooled bit (the quad epilogue, which
assumes the window-pair order) must keep the first form and stay correct."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module
from kernel_harness import SENT, Buf, bits, bound, call, nhwc, rnd, trace_of

pytestmark = pytest.mark.gpu

CH = 256
SHAPES = [(2, 4, 64), (1, 8, 64), (2, 2, 128)]
IDS = [f"{b}x{h}x{w}" for b, h, w in SHAPES]
KNOB = "AOCR_NO_HALO4_POOL_SKIP"
KERNEL = "gemm_halo4_bf16_kernel[fwd]"
_cache = {}


def operands(B, H, W):
    """x / w / bias and the float64 reference of the un-pooled convolution with its magnitudes, computed once per shape and left unchanged.
    Outputs are symmetric about 0 and a window's two rows uncorrelated, so about a quarter of the windows have both candidates negative; the seeds
    are chosen so that at the three shapes 26.3 / 26.4 / 26.8 % are negative by more than the bound (computed on the CPU; check_pooled asserts >= 25 %)."""
    key = (B, H, W)
    if key not in _cache:
        x, w, b = rnd(B, CH, H, W, seed=446).float(), (rnd(CH, CH, 3, 3, seed=447) / 48.0).float(), (rnd(CH, seed=448) * 0.1).float()
        assert (x[:, :, 0].abs() > 0).float().mean() > 0.99 and (x[:, :, -1].abs() > 0).float().mean() > 0.99
        xq, wq = x.to(torch.bfloat16).double(), w.to(torch.bfloat16).double()
        ref = F.conv2d(xq, wq, b.double(), padding=1)
        mag = F.conv2d(xq.abs(), wq.abs(), None, padding=1) + b.double().abs().view(1, -1, 1, 1)
        _cache[key] = (x, w, b, ref, mag)
    return _cache[key]


def windows(t, B, H, W):
    """(B, C, H, W) -> the two candidates of every (2,1) window, each (B, H / 2, W, C)"""
    p = t.reshape(B, CH, H // 2, 2, W)
    return nhwc(p[:, :, :, 0]), nhwc(p[:, :, :, 1])


def forward(x, w, b, relu, dst="yb"):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    oshape = (B, H // 2, W, Cout)
    xd, wd, bd, xb = Buf(nhwc(x)), Buf(w.permute(0, 2, 3, 1)), Buf(b), Buf(nhwc(x), torch.bfloat16)
    wb, wtb = Buf((Cout, 3, 3, Cin), torch.bfloat16, fill=0), Buf((Cin, 9, Cout), torch.bfloat16, fill=0)
    call("kp_conv_weight_shadows", wd.ptr(), wb.ptr(), wtb.ptr(), Cout, 9, Cin)
    y = Buf(oshape, fill=SENT) if "y32" in dst else None
    yb = Buf(oshape, torch.bfloat16, fill=-3.0) if "yb" in dst else None
    idx = Buf(oshape, torch.uint8, fill=0x77)
    call("kp_conv_forward", 1, xd.ptr(), wd.ptr(), bd.ptr(), y.ptr() if y else None, idx.ptr(), B, H, W, Cin, Cout, 3, 1,
         relu, 2, xb.ptr(), wb.ptr(), yb.ptr() if yb else None, None, None, None, None, None)
    torch.cuda.synchronize()
    for t, nm in ((y, "y"), (yb, "yb"), (idx, "idx")):
        if t is not None:
            t.check_tail(nm)
    return dict(y=y, yb=yb, idx=idx)


def last_line(capfd, pskip):
    lines = trace_of(capfd, "conv_forward")
    assert lines, "conv_forward: no dispatch trace line (AOCR_TRACE)"
    assert f": {KERNEL}" in lines[-1], lines
    assert not lines[-1].endswith(" skip"), f"a pooled launch never carries the plain-order word: {lines}"
    assert lines[-1].endswith(" pskip") == pskip, f"expected the {'row-split skipping' if pskip else 'first'} form: {lines}"


def both(monkeypatch, capfd, run, pskip=True):
    """run() with the switch unset (the row-split skipping form, where it applies) and set (the first form)"""
    monkeypatch.delenv(KNOB, raising=False)
    monkeypatch.delenv("AOCR_NO_HALO4_SKIP", raising=False)
    capfd.readouterr()
    new = run()
    last_line(capfd, pskip)
    monkeypatch.setenv(KNOB, "1")
    capfd.readouterr()
    old = run()
    last_line(capfd, False)
    return new, old


def check_pooled(val, idx, B, H, W, relu, what):
    """val (float64, (B, H / 2, W, C)) and idx against the float64 reference; returns the share of windows whose arg-max is forced to 0"""
    x, w, b, ref, mag = operands(B, H, W)
    top, bot = windows(ref, B, H, W)
    mtop, mbot = windows(mag, B, H, W)
    if relu:
        top, bot = top.clamp(min=0), bot.clamp(min=0)
    pr, pm = torch.maximum(top, bot), torch.maximum(mtop, mbot)
    err = ((val - pr).abs() - 2.0 ** -8 * pr.abs()).clamp(min=0)          # + one bf16 rounding
    r = (err / (bound(pm, 9 * CH) + 2.0 ** -24 * pr.abs())).max().item()
    print(f"[halo4-pool-skip] {what} {B}x{H}x{W} relu={relu}: largest error / bound = {r:.3f}")
    assert r <= 1.0
    assert (idx <= 1).all()
    if not relu:
        return 0.0
    rtop, rbot = windows(ref, B, H, W)
    tie = (rtop < -bound(mtop, 9 * CH)) & (rbot < -bound(mbot, 9 * CH))    # both candidates are 0 after the ReLU whatever the rounding did
    share = tie.float().mean().item()
    assert share >= 0.25, f"only {share:.3f} of the windows tie at 0: choose another seed"
    assert (idx[tie] == 0).all(), "a tie at 0 picks the upper row"
    assert (val[tie] == 0).all()
    return share


@pytest.mark.parametrize("B,H,W", SHAPES, ids=IDS)
@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
def test_forward_pooled_row_split(B, H, W, relu, monkeypatch, capfd):
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    x, w, b, ref, mag = operands(B, H, W)
    new, old = both(monkeypatch, capfd, lambda: forward(x, w, b, relu))
    assert torch.equal(bits(new["yb"]), bits(old["yb"])), "yb differs between the two forms"
    assert torch.equal(new["idx"].cpu(), old["idx"].cpu()), "idx differs between the two forms"
    check_pooled(new["yb"].cpu().double(), new["idx"].cpu(), B, H, W, relu, "row-split")


def test_no_halo4_skip_switches_it_off_too(monkeypatch, capfd):
    """AOCR_NO_HALO4_SKIP=1 stays "the first form everywhere" """
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    monkeypatch.setenv("AOCR_NO_HALO4_SKIP", "1")
    monkeypatch.delenv(KNOB, raising=False)
    B, H, W = SHAPES[0]
    x, w, b, ref, mag = operands(B, H, W)
    capfd.readouterr()
    res = forward(x, w, b, 1)
    last_line(capfd, False)
    check_pooled(res["yb"].cpu().double(), res["idx"].cpu(), B, H, W, 1, "AOCR_NO_HALO4_SKIP")


def test_width_32_keeps_the_first_form(monkeypatch, capfd):
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    B, H, W = 1, 8, 32
    x, w, b, ref, mag = operands(B, H, W)
    new, old = both(monkeypatch, capfd, lambda: forward(x, w, b, 0), pskip=False)
    assert torch.equal(bits(new["yb"]), bits(old["yb"])) and torch.equal(new["idx"].cpu(), old["idx"].cpu())
    check_pooled(new["yb"].cpu().double(), new["idx"].cpu(), B, H, W, 0, "W = 32")


@pytest.mark.parametrize("case", ["fp32-destination", "staged-without-bit-4"])
def test_other_epilogues_keep_the_first_form(case, monkeypatch, capfd):
    """the quad epilogue these launches fall back to assumes the window-pair order"""
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    B, H, W = SHAPES[0]
    x, w, b, ref, mag = operands(B, H, W)
    if case == "staged-without-bit-4":
        monkeypatch.setenv("AOCR_HALO4_STAGED", "3")
    dst = "y32+yb" if case == "fp32-destination" else "yb"
    new, old = both(monkeypatch, capfd, lambda: forward(x, w, b, 1, dst), pskip=False)
    assert torch.equal(bits(new["yb"]), bits(old["yb"])) and torch.equal(new["idx"].cpu(), old["idx"].cpu())
    check_pooled(new["yb"].cpu().double(), new["idx"].cpu(), B, H, W, 1, case)
    if new["y"] is not None:
        y = new["y"].cpu()
        assert torch.equal(y.view(torch.int32), old["y"].cpu().view(torch.int32))
        assert torch.equal(y.to(torch.bfloat16).view(torch.int16), bits(new["yb"])), "the bf16 shadow is the rounded fp32 output"
