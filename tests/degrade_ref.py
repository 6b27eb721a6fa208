"""Test helper: numpy-float32 restatement of aocr_degrade_lines (include/aocr.h), one rounded single-precision operation at a time in the
header's order, so the kernel can be compared with it bit for bit.  Whole images, no tiles: whatever the kernel's tiling does at a border or
a tile seam shows as a difference.  np.fmax / np.fmin drop a NaN operand like fmaxf / fminf.  The only import from the package is the
splitmix64 of aocr/synth.py; nothing here touches the library or aocr/degrade.py."""
import numpy as np

from aocr.synth import _splitmix64 as splitmix64

F = np.float32
DEGRADE_DTYPE = np.dtype([("amp_x", "<f4"), ("amp_y", "<f4"), ("pitch", "<i4"), ("inv_pitch", "<f4"), ("thick", "<f4"), ("taps", "<f4", (5,)),
                          ("fill", "<f4")])                                      # aocr_degrade, in the header's order
_K = np.uint64(0xD1342543DE82EF95)
STREAM = np.uint64(0x4445475241444531)                                           # AOCR_DEGRADE_STREAM


def record(amp=(0.0, 0.0), pitch=8, thick=0.0, taps=(1, 0, 0, 0, 0), fill=255.0):
    return (F(amp[0]), F(amp[1]), int(pitch), F(1.0 / pitch), F(thick), tuple(F(t) for t in taps), F(fill))


def records(rows):
    """structured array of aocr_degrade records from an iterable of record(...) tuples."""
    out = np.zeros(len(rows), DEGRADE_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def gauss_taps(sigma):
    """w0..w4 of a normalised 9-tap Gaussian, float64 then fp32 (the host's job; written again here so the tests do not lean on aocr/degrade.py)."""
    w = np.exp(-np.arange(5, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return tuple((w / (w[0] + 2.0 * w[1:].sum())).astype(F))


def node_field(i, H, W, pitch, amp_x, amp_y, seed, counter):
    """(GY, GX) float32 dx and dy of image i's displacement nodes."""
    GX, GY = (W - 1) // pitch + 2, (H - 1) // pitch + 2
    with np.errstate(over="ignore"):
        base = splitmix64(np.array([seed], np.uint64) ^ (np.array([counter], np.uint64) * _K) ^ STREAM)
        r = splitmix64(base + (np.uint64(i * GY * GX) + np.arange(GY * GX, dtype=np.uint64)))
    k24 = F(1.0 / 16777216.0)
    u1 = (r >> np.uint64(40)).astype(F) * k24                                    # 24 bits: exact
    u2 = ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(F) * k24
    dx = F(amp_x) * ((u1 + u1) - F(1))
    dy = F(amp_y) * ((u2 + u2) - F(1))
    return dx.reshape(GY, GX), dy.reshape(GY, GX)


def _cell(n, pitch, inv_pitch):
    p = np.arange(n)
    g = p // pitch
    f = (p - g * pitch).astype(F) * F(inv_pitch)
    return g, (f * f) * (F(3) - (f + f))


def elastic(img, rec, i, seed, counter):
    H, W = img.shape
    pitch = int(rec["pitch"])
    dx, dy = node_field(i, H, W, pitch, rec["amp_x"], rec["amp_y"], seed, counter)
    gx, ax = _cell(W, pitch, rec["inv_pitch"])
    gy, ay = _cell(H, pitch, rec["inv_pitch"])
    gx, ax, gy, ay = gx[None, :], ax[None, :], gy[:, None], ay[:, None]
    bx, by = F(1) - ax, F(1) - ay

    def field(d):
        top = bx * d[gy, gx] + ax * d[gy, gx + 1]
        bot = bx * d[gy + 1, gx] + ax * d[gy + 1, gx + 1]
        return by * top + ay * bot

    Y, X = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    sx, sy = X + field(dx), Y + field(dy)
    sx = np.fmin(np.fmax(sx, F(-1)), F(W))
    sy = np.fmin(np.fmax(sy, F(-1)), F(H))
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)

    def tap(r, c):
        inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        return np.where(inside, img[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)], F(rec["fill"])).astype(F)

    a, b, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    gxw, gyw = F(1) - fx, F(1) - fy
    top = gxw * a + fx * b
    bot = gxw * c + fx * d
    E = gyw * top + fy * bot
    assert E.dtype == np.float32 and sx.dtype == np.float32
    return E


def _shift(a, dy, dx):
    """a sampled at (y + dy, x + dx), coordinates clamped to the image."""
    H, W = a.shape
    return a[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]


def stroke(E, thick):
    lo, hi = E, E
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            s = _shift(E, dy, dx)
            lo, hi = np.fmin(lo, s), np.fmax(hi, s)
    thick = F(thick)
    t, ext = (thick, lo) if thick >= 0 else (-thick, hi)
    M = (F(1) - t) * E + t * ext
    assert M.dtype == np.float32
    return M


def blur(M, taps):
    w = [F(t) for t in taps]
    for axis in (1, 0):                                                         # along x first, then along y
        acc = w[0] * M
        for k in range(1, 5):
            lo, hi = (_shift(M, 0, -k), _shift(M, 0, k)) if axis == 1 else (_shift(M, -k, 0), _shift(M, k, 0))
            acc = acc + w[k] * (lo + hi)
        assert acc.dtype == np.float32
        M = acc
    return M


def degrade(inp, rec, seed=0, counter=0):
    """inp (n,1,H,W) or (n,H,W) float32 in 0..255, rec: n aocr_degrade records -> the same shape, float32."""
    inp = np.asarray(inp)
    assert inp.dtype == np.float32
    img = inp.reshape(inp.shape[0], inp.shape[-2], inp.shape[-1])
    out = np.empty_like(img)
    with np.errstate(invalid="ignore"):
        for i in range(img.shape[0]):
            B = blur(stroke(elastic(img[i], rec[i], i, seed, counter), rec[i]["thick"]), rec[i]["taps"])
            out[i] = np.fmin(np.fmax(B, F(0)), F(255))
    return out.reshape(inp.shape)
