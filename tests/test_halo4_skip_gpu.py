"""GPU: gemm_halo4_bf16_kernel's interleaved block ownership with the padding rows' dead blocks skipped (the default where it applies) against
the same kernel's contiguous ownership without a skip (AOCR_NO_HALO4_SKIP=1), bit for bit, and against float64 on the bf16-rounded operands
with tests/test_kernels_bf16_gpu.py's bound: BOUND_C * sqrt(K) * 2^-24 * (|A| |B|) per element.

Through tests/libkprobe.so's kp_conv_forward / kp_conv_backward_data, bf16 shadows, 3 x 3, pad 1, Cin = Cout = 256, two 256-pixel tiles each:
  (B, H, W) = (2, 4, 64)   a tile is a whole image: first AND last map row in it
              (1, 8, 64)   the upper tile has the first map row, the lower one the last
              (2, 2, 128)  two rows: every block's row is first or last, two dead blocks per wave and kernel row
Operands are uniform in (-1, 1) everywhere, the first and last map rows included, and every output buffer starts as sentinels, so a block
stored to another block's rows, or a live block skipped, cannot pass.  Which form ran is read from the AOCR_TRACE line: the skipping form's
ends in " skip".  The (2,1)-pooled epilogue orders its rows in window pairs (no block lies in one map row), a width of 96 is not a halo
shape at all: both must take the form they took before."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from kernel_harness import _switches  # noqa: F401  this import IS how the autouse fixture reaches the module
from kernel_harness import SENT, Buf, bf, bits, bound, call, kp, nhwc, rnd, trace_of

pytestmark = pytest.mark.gpu

CH = 256
SHAPES = [(2, 4, 64), (1, 8, 64), (2, 2, 128)]
IDS = [f"{b}x{h}x{w}" for b, h, w in SHAPES]
KNOB = "AOCR_NO_HALO4_SKIP"
_cache = {}


def operands(B, H, W):
    """x / w / bias of the forward cases and their float64 reference, computed once per shape"""
    key = ("fwd", B, H, W)
    if key not in _cache:
        x, w, b = rnd(B, CH, H, W, seed=301).float(), (rnd(CH, CH, 3, 3, seed=302) / 48.0).float(), (rnd(CH, seed=303) * 0.1).float()
        assert (x[:, :, 0].abs() > 0).float().mean() > 0.99 and (x[:, :, -1].abs() > 0).float().mean() > 0.99
        xq, wq = x.to(torch.bfloat16).double(), w.to(torch.bfloat16).double()
        ref = F.conv2d(xq, wq, b.double(), padding=1)
        mag = F.conv2d(xq.abs(), wq.abs(), None, padding=1) + b.double().abs().view(1, -1, 1, 1)
        _cache[key] = (x, w, b, ref, mag)
    return _cache[key]


def forward(x, w, b, pool, dst, bn_part=None):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    oshape = (B, H, W, Cout) if pool == 0 else (B, H // 2, W, Cout)
    xd, wd, bd, xb = Buf(nhwc(x)), Buf(w.permute(0, 2, 3, 1)), Buf(b), Buf(nhwc(x), torch.bfloat16)
    wb, wtb = Buf((Cout, 3, 3, Cin), torch.bfloat16, fill=0), Buf((Cin, 9, Cout), torch.bfloat16, fill=0)
    call("kp_conv_weight_shadows", wd.ptr(), wb.ptr(), wtb.ptr(), Cout, 9, Cin)
    y = Buf(oshape, fill=SENT) if "y" in dst else None
    yb = Buf(oshape, torch.bfloat16, fill=-3.0) if "yb" in dst else None
    idx = Buf(oshape, torch.uint8, fill=0x77) if pool else None
    chunks = C.c_int(-1)
    call("kp_conv_forward", 1, xd.ptr(), wd.ptr(), bd.ptr(), y.ptr() if y else None, idx.ptr() if idx else None, B, H, W, Cin, Cout, 3, 1,
         0, pool, xb.ptr(), wb.ptr(), yb.ptr() if yb else None, None, None, None,
         C.c_void_p(bn_part.data_ptr()) if bn_part is not None else None, C.byref(chunks) if bn_part is not None else None)
    torch.cuda.synchronize()
    for t, nm in ((y, "y"), (yb, "yb"), (idx, "idx")):
        if t is not None:
            t.check_tail(nm)
    return dict(y=y, yb=yb, idx=idx, chunks=chunks.value)


def last_line(capfd, fn, kernel, skip):
    lines = trace_of(capfd, fn)
    assert lines, f"{fn}: no dispatch trace line (AOCR_TRACE)"
    assert f": {kernel}" in lines[-1], (kernel, lines)
    assert lines[-1].endswith(" skip") == skip, f"expected the {'skipping' if skip else 'first'} form: {lines}"


def both(monkeypatch, capfd, fn, kernel, run, skips=True):
    """run() with the switch unset (the skipping form, where it applies) and set (the first form)"""
    monkeypatch.delenv(KNOB, raising=False)
    capfd.readouterr()
    new = run()
    last_line(capfd, fn, kernel, skips)
    monkeypatch.setenv(KNOB, "1")
    capfd.readouterr()
    old = run()
    last_line(capfd, fn, kernel, False)
    return new, old


@pytest.mark.parametrize("B,H,W", SHAPES, ids=IDS)
@pytest.mark.parametrize("dst", ["y", "y+yb"])
def test_forward_plain(B, H, W, dst, monkeypatch, capfd):
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    x, w, b, ref, mag = operands(B, H, W)
    new, old = both(monkeypatch, capfd, "conv_forward", "gemm_halo4_bf16_kernel[fwd]", lambda: forward(x, w, b, 0, dst))
    y = new["y"].cpu()
    assert torch.equal(y.view(torch.int32), old["y"].cpu().view(torch.int32)), "y differs between the two forms"
    if new["yb"] is not None:
        assert torch.equal(bits(new["yb"]), bits(old["yb"])) and torch.equal(bits(new["yb"]), bf(y))
    r = ((y.double() - nhwc(ref)).abs() / (bound(nhwc(mag), 9 * CH) + 2.0 ** -24 * nhwc(ref).abs())).max().item()
    print(f"[halo4-skip] forward {B}x{H}x{W} {dst}: largest error / bound = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("B,H,W", SHAPES, ids=IDS)
def test_forward_batchnorm_sums(B, H, W, monkeypatch, capfd):
    """conv3 / conv5's epilogue: the fp32 tile and the (sum y, sum y^2) partials of every row tile and column"""
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    x, w, b, ref, mag = operands(B, H, W)
    n = kp().kp_bn_scratch_bytes(CH) // 8 + 8
    parts = []

    def run():
        scratch = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        res = forward(x, w, b, 0, "y", bn_part=scratch)
        parts.append(scratch.cpu())
        return res
    new, old = both(monkeypatch, capfd, "conv_forward", "gemm_halo4_bf16_kernel[fwd]", run)
    tiles = B * H * W // 256
    assert new["chunks"] == tiles and old["chunks"] == tiles, "fused statistics not taken"
    y = new["y"].cpu()
    assert torch.equal(y.view(torch.int32), old["y"].cpu().view(torch.int32)), "y differs between the two forms"
    assert torch.equal(parts[0].view(torch.int64), parts[1].view(torch.int64)), "BatchNorm partial sums differ between the two forms"
    r = ((y.double() - nhwc(ref)).abs() / (bound(nhwc(mag), 9 * CH) + 2.0 ** -24 * nhwc(ref).abs())).max().item()
    assert r <= 1.0
    # the partials are sums of exactly the stored values: a thread adds 64 rows in fp32 (error <= 64 * 2^-24 * sum |term|), fp64 from there on
    got = parts[0][:tiles * CH * 2].view(tiles, CH, 2)
    yt = y.double().reshape(tiles, 256, CH)
    assert ((got[:, :, 0] - yt.sum(1)).abs() <= 64 * 2.0 ** -24 * yt.abs().sum(1)).all(), "sum y"
    assert ((got[:, :, 1] - (yt * yt).sum(1)).abs() <= 64 * 2.0 ** -24 * (yt * yt).sum(1)).all(), "sum y^2"
    assert (parts[0][tiles * CH * 2:] == -7.0).all(), "written past the tiles' partials"


@pytest.mark.parametrize("B,H,W", SHAPES, ids=IDS)
def test_forward_pooled_keeps_the_first_form(B, H, W, monkeypatch, capfd):
    """the (2,1)-pooled epilogue (conv4 / conv6): rows in window pairs, so a block spans two map rows and none is dead"""
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    x, w, b, ref, mag = operands(B, H, W)
    new, old = both(monkeypatch, capfd, "conv_forward", "gemm_halo4_bf16_kernel[fwd]", lambda: forward(x, w, b, 2, "yb"), skips=False)
    assert torch.equal(bits(new["yb"]), bits(old["yb"])) and torch.equal(new["idx"].cpu(), old["idx"].cpu())
    pr = ref.reshape(B, CH, H // 2, 2, W).max(dim=3).values
    pm = mag.reshape(B, CH, H // 2, 2, W).max(dim=3).values
    err = ((new["yb"].cpu().double() - nhwc(pr)).abs() - 2.0 ** -8 * nhwc(pr).abs()).clamp(min=0)          # + one bf16 rounding
    r = (err / (bound(nhwc(pm), 9 * CH) + 2.0 ** -24 * nhwc(pr).abs())).max().item()
    assert r <= 1.0
    assert (new["idx"].cpu() <= 1).all()


@pytest.mark.parametrize("B,H,W", SHAPES, ids=IDS)
def test_backward_data(B, H, W, monkeypatch, capfd):
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    key = ("dgrad", B, H, W)
    if key not in _cache:
        w, dy = (rnd(CH, CH, 3, 3, seed=311) / 48.0).float(), rnd(B, CH, H, W, seed=312).float()
        wq, dyq = w.to(torch.bfloat16).double(), dy.to(torch.bfloat16).double()
        _cache[key] = (w, dy, nhwc(torch.nn.grad.conv2d_input((B, CH, H, W), wq, dyq, padding=1)),
                       nhwc(torch.nn.grad.conv2d_input((B, CH, H, W), wq.abs(), dyq.abs(), padding=1)))
    w, dy, ref, mag = _cache[key]

    def run():
        dyd, dyb, wd = Buf(nhwc(dy)), Buf(nhwc(dy), torch.bfloat16), Buf(w.permute(0, 2, 3, 1))
        wb, wtb = Buf((CH, 9, CH), torch.bfloat16, fill=0), Buf((CH, 9, CH), torch.bfloat16, fill=0)
        call("kp_conv_weight_shadows", wd.ptr(), wb.ptr(), wtb.ptr(), CH, 9, CH)
        dx = Buf((B, H, W, CH), fill=SENT)
        call("kp_conv_backward_data", 1, dyd.ptr(), wd.ptr(), dx.ptr(), B, H, W, CH, CH, 3, 1, dyb.ptr(), wtb.ptr(), None)
        torch.cuda.synchronize()
        dx.check_tail("dx")
        return dx
    new, old = both(monkeypatch, capfd, "conv_backward_data", "gemm_halo4_bf16_kernel[dgrad]", run)
    dx = new.cpu()
    assert torch.equal(dx.view(torch.int32), old.cpu().view(torch.int32)), "dx differs between the two forms"
    r = ((dx.double() - ref).abs() / (bound(mag, 9 * CH) + 1e-30)).max().item()
    print(f"[halo4-skip] data gradient {B}x{H}x{W}: largest error / bound = {r:.3f}")
    assert r <= 1.0


def test_other_shapes_keep_their_kernel(monkeypatch, capfd):
    """W = 96 is no halo shape: the im2col LDS-DMA kernel, whatever the switch says"""
    monkeypatch.setenv("AOCR_FORCE_DMA", "1")
    B, H, W = 1, 8, 96
    x, w, b = rnd(B, CH, H, W, seed=321).float(), (rnd(CH, CH, 3, 3, seed=322) / 48.0).float(), (rnd(CH, seed=323) * 0.1).float()
    new, old = both(monkeypatch, capfd, "conv_forward", "gemm_dma_bf16_kernel[]", lambda: forward(x, w, b, 0, "y"), skips=False)
    assert torch.equal(new["y"].cpu().view(torch.int32), old["y"].cpu().view(torch.int32))
    xq, wq = x.to(torch.bfloat16).double(), w.to(torch.bfloat16).double()
    ref = nhwc(F.conv2d(xq, wq, b.double(), padding=1))
    mag = nhwc(F.conv2d(xq.abs(), wq.abs(), None, padding=1) + b.double().abs().view(1, -1, 1, 1))
    assert ((new["y"].cpu().double() - ref).abs() / (bound(mag, 9 * CH) + 2.0 ** -24 * ref.abs())).max().item() <= 1.0
