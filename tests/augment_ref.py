"""Test helper: numpy-float32 restatement of aocr_augment_lines (include/aocr.h), one rounded single-precision operation at a
time in the kernel's order, so the kernel can be compared with it bit for bit.  np.fmax / np.fmin drop a NaN operand like
fmaxf / fminf.  Nothing here imports the library."""
import numpy as np

F = np.float32
FIELDS = ("m00", "m01", "m02", "m10", "m11", "m12", "gain", "offset", "fill", "noise")          # aocr_warp, in the header's order
WARP_DTYPE = np.dtype([(n, "<f4") for n in FIELDS])
_K = np.uint64(0xD1342543DE82EF95)


def warp_records(rows):
    """structured array of aocr_warp records from an iterable of 10-tuples in the header's field order."""
    out = np.zeros(len(rows), WARP_DTYPE)
    for i, r in enumerate(rows):
        out[i] = tuple(F(v) for v in r)
    return out


def identity(fill=255.0):
    return (1, 0, 0, 0, 1, 0, 1, 0, fill, 0)


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def noise_field(n, H, W, seed, counter):
    """(n,H,W) float32: (u1 + u2) - 1 of every pixel, triangular on (-1, 1)."""
    with np.errstate(over="ignore"):
        base = splitmix64(np.array([seed], np.uint64) ^ (np.array([counter], np.uint64) * _K))
        r = splitmix64(base + np.arange(n * H * W, dtype=np.uint64))
    k24 = F(1.0 / 16777216.0)
    u1 = (r >> np.uint64(40)).astype(F) * k24                                  # 24 bits: exact
    u2 = ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(F) * k24
    return ((u1 + u2) - F(1)).reshape(n, H, W)


def augment(inp, warp, seed=0, counter=0):
    """inp (n,1,H,W) or (n,H,W) float32 in 0..255, warp: n aocr_warp records -> the same shape, float32."""
    inp = np.asarray(inp)
    assert inp.dtype == np.float32
    shape = inp.shape
    img = inp.reshape(shape[0], shape[-2], shape[-1])
    n, H, W = img.shape
    Y, X = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    tri = noise_field(n, H, W, seed, counter)
    out = np.empty_like(img)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            w = {k: F(warp[i][k]) for k in FIELDS}
            sx = (w["m00"] * X + w["m01"] * Y) + w["m02"]
            sy = (w["m10"] * X + w["m11"] * Y) + w["m12"]
            sx = np.fmin(np.fmax(sx, F(-1)), F(W))
            sy = np.fmin(np.fmax(sy, F(-1)), F(H))
            x0f, y0f = np.floor(sx), np.floor(sy)
            fx, fy = sx - x0f, sy - y0f
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)

            def tap(r, c):
                inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
                return np.where(inside, img[i][np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)], w["fill"]).astype(F)

            a, b, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
            gx, gy = F(1) - fx, F(1) - fy
            top = gx * a + fx * b
            bot = gx * c + fx * d
            s = gy * top + fy * bot
            v = w["gain"] * s + w["offset"]
            v = v + w["noise"] * tri[i]
            out[i] = np.fmin(np.fmax(v, F(0)), F(255))
            assert out[i].dtype == np.float32 and sx.dtype == np.float32 and s.dtype == np.float32
    return out.reshape(shape)
