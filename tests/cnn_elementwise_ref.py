"""Plain float64 restatements of conv1, un-pool + ReLU backward and BatchNorm (+ ReLU) forward / backward for
tests/test_cnn_elementwise_kernels_gpu.py.  Written from cnn.lua's semantics and the comments of csrc/ops.h: tensor expressions
over whole maps, none of the kernels' strip / quad / chunk indexing."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                      # one fp32 rounding, relative


# ---- conv1: y (B,Hp,Wp,64) = maxpool2x2(relu(conv3x3((x - 128) / 128, pad 1) + b)), x (B,H,W) raw pixels, w (64,3,3)
def conv1_windows(x, w, b):
    """v (B,Hp,Wp,64,4): the four conv values of every pooling window in the order (0,0),(0,1),(1,0),(1,1); a (B,64,H,W): sum |w p| + |b|."""
    B, H, W = x.shape
    xn = (x.double() - 128.0) / 128.0
    z = F.conv2d(xn[:, None], w.double().view(64, 1, 3, 3), b.double(), padding=1)
    a = F.conv2d(xn[:, None].abs(), w.double().abs().view(64, 1, 3, 3), b.double().abs(), padding=1)
    Hp, Wp = H // 2, W // 2

    def win(t):
        return t[:, :, :2 * Hp, :2 * Wp].reshape(B, 64, Hp, 2, Wp, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, Hp, Wp, 64, 4)
    return win(z), win(a), xn


def conv1_route(v):
    """-1: nothing above the ReLU floor (a value of exactly 0 routes nothing); else the FIRST strict maximum of the window."""
    m = v.max(dim=-1).values
    first = (v == m.unsqueeze(-1)).to(torch.int8).argmax(dim=-1)
    return torch.where(m > 0, first, torch.full_like(first, -1)), m.clamp(min=0)


def conv1_grads(xn, route, g):
    """dw (64,9), db (64), and sum |term| per channel, for d(pooled) g (B,Hp,Wp,64) sent to position `route` of its window."""
    B, H, W = xn.shape
    Hp, Wp = route.shape[1], route.shape[2]
    dz = torch.zeros(B, 64, H, W, dtype=torch.float64)
    gc, rc = g.double().permute(0, 3, 1, 2), route.permute(0, 3, 1, 2)
    for q in range(4):
        dz[:, :, q >> 1:2 * Hp:2, q & 1:2 * Wp:2] = torch.where(rc == q, gc, torch.zeros_like(gc))
    patches = F.unfold(xn[:, None], 3, padding=1)                                  # (B, 9, H W): the nine taps of every pixel
    dw = torch.einsum("bcp,bkp->ck", dz.reshape(B, 64, H * W), patches)
    mag = torch.einsum("bcp,bkp->ck", dz.reshape(B, 64, H * W).abs(), patches.abs())
    return dw, dz.sum(dim=(0, 2, 3)), mag, dz.abs().sum(dim=(0, 2, 3))


# ---- un-pool + ReLU backward: dy (B,Ho,Wo,C) from d(pooled) g, the arg-max position idx and the pooled value (> 0 <=> ReLU passed)
def unpool(g, pooled, idx, Ho, Wo, pool):
    B, Hp, Wp, C = g.shape
    gv = torch.where(pooled > 0, g, torch.zeros_like(g))
    dy = torch.zeros(B, Ho, Wo, C, dtype=g.dtype)
    for pos in range(4 if pool == 1 else 2):
        o = torch.where(idx == pos, gv, torch.zeros_like(gv))
        if pool == 1:
            dy[:, pos >> 1:2 * Hp:2, pos & 1:2 * Wp:2] = o
        else:
            dy[:, pos:2 * Hp:2, :] = o
    return dy, gv.sum(dim=(0, 1, 2))


# ---- BatchNorm (+ ReLU): momentum 0.1, unbiased running variance, var < 0 clamped, eps 1e-5
def bn_stats(x, rm0, rv0):
    n = x.shape[0]
    xd = x.double()
    mean = xd.sum(0) / n
    var = ((xd * xd).sum(0) / n - mean * mean).clamp(min=0)
    unb = var * n / (n - 1.0) if n > 1 else var
    return mean, 1.0 / torch.sqrt(var + 1e-5), 0.1 * mean + 0.9 * rm0.double(), 0.1 * unb + 0.9 * rv0.double()


def to_tb(t, T, Bt):
    """rows (b, t) -> rows (t, b): the last layer's output order."""
    return t.reshape(Bt, T, -1).transpose(0, 1).reshape(T * Bt, -1)


def bn_fwd(x, save, w, b):
    """y and the magnitude its error bound is taken against, in float64 on the given {mean, invstd}."""
    C = x.shape[1]
    m, iv = save[:C].double(), save[C:].double()
    s = iv * w.double()
    return ((x.double() - m) * s + b.double()).clamp(min=0), (x.double().abs() + m.abs()) * s.abs() + b.double().abs()


def bn_bwd(x, mask, dA, save, w, sums=None):
    """x (rows,C) and mask / dA already in x's row order.  Returns a dict of float64 results and bound magnitudes.
    sums = (sum d, sum d xhat, sum |d xhat|) handed over by a producer instead of taken from this d A (the launchers' sums_chunks)."""
    n, C = x.shape
    m, iv = save[:C].double(), save[C:].double()
    d = torch.where(mask > 0, dA.double(), torch.zeros(1, dtype=torch.float64))
    xhat = (x.double() - m) * iv
    axhat = (x.double().abs() + m.abs()) * iv.abs()
    s, ss, ass = sums if sums is not None else (d.sum(0), (d * xhat).sum(0), (d.abs() * axhat).sum(0))
    dx = (d - s / n - xhat * (ss / n)) * iv * w.double()
    dxmag = (d.abs() + (s / n).abs() + axhat * (ass / n)) * (iv * w.double()).abs()
    return dict(db=s, dw=ss, dwmag=ass, dx=dx, dxmag=dxmag, d=d, xhat=xhat)


def ulps(gpu, ref):
    """|gpu - ref| in units of the fp32 spacing at ref (gpu: fp32 tensor, ref: float64 tensor); the largest."""
    r = ref.numpy()
    sp = np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(gpu.double().numpy() - r) / sp)) if r.size else 0.0
