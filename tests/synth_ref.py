"""Test helper: numpy-float32 restatement of aocr_synth_lines (include/aocr.h), one rounded single-precision operation at a time in
the kernel's order, so the kernel can be compared with it bit for bit.  np.fmax / np.fmin drop a NaN operand like fmaxf / fminf.
Nothing here imports the library."""
import numpy as np

F = np.float32
PAD, GO, EOS = 1, 2, 3
FIELDS = ("word", "face", "spacing", "sx", "sy", "x0", "y0", "fg", "bg")                       # aocr_synth_style, in the header's order
STYLE_DTYPE = np.dtype([(n, "<i4") for n in FIELDS[:2]] + [(n, "<f4") for n in FIELDS[2:]])
MAX_COORD = F(16384)


def style_records(rows):
    """structured array of aocr_synth_style records from an iterable of 9-tuples in the header's field order."""
    out = np.zeros(len(rows), STYLE_DTYPE)
    for i, r in enumerate(rows):
        out[i] = tuple(r[:2]) + tuple(F(v) for v in r[2:])
    return out


def identity(word, face=0):
    return (word, face, 0.0, 1.0, 1.0, 0.0, 0.0, 255.0, 0.0)


def counter_atlas(n_faces, n_glyphs, gh, gw, seed=1, binary=False):
    """(pixels, advance) from a multiplicative counter sequence (no generator state): every fourth advance is 0."""
    idx = np.arange(n_faces * n_glyphs * gh * gw, dtype=np.uint64)
    with np.errstate(over="ignore"):
        v = ((idx + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(56)
    pixels = v.astype(np.uint8).reshape(n_faces, n_glyphs, gh, gw)
    if binary:
        pixels = np.where(pixels >= 128, 255, 0).astype(np.uint8)
    g = np.arange(n_faces * n_glyphs).reshape(n_faces, n_glyphs)
    advance = np.where(g % 4 == 3, 0, 1 + (g * 7 + seed) % gw).astype(np.uint8)
    return pixels, advance


def pack(words, stride=16):
    """(n_words, stride) uint8 lexicon rows from lists of ids."""
    a = np.zeros((len(words), stride), np.uint8)
    for i, w in enumerate(words):
        a[i, :len(w)] = w
    return a


BLIT_GH, BLIT_GW = 8, 6


def blit_atlas():
    """for the hand answers: one face, five 8 x 6 glyphs of 0 / 255 ink inside their [0, adv) columns only; glyph 1 has no advance."""
    pixels, _ = counter_atlas(1, 5, BLIT_GH, BLIT_GW, seed=3, binary=True)
    advance = np.array([[3, 0, 5, 6, 2]], np.uint8)
    for g in range(5):
        pixels[0, g, :, advance[0, g]:] = 0
    assert pixels.any(axis=(2, 3))[0, [0, 2, 3, 4]].all()
    return pixels, advance


def side_by_side(pixels, advance, ids, W, H=BLIT_GH):
    """the hand answer of the identity style: the [0, adv) columns of the glyphs of `ids` next to each other, 0 elsewhere."""
    gh = pixels.shape[2]
    cols = [pixels[0, v - 4, :, :advance[0, v - 4]] for v in ids]
    strip = np.concatenate(cols + [np.zeros((gh, W), np.uint8)], axis=1)[:, :W]
    return np.concatenate([strip, np.zeros((max(H - gh, 0), W), np.uint8)], axis=0).astype(F)


def word_of(words, stride, st, n_faces):
    """the ids style record `st` draws: lexicon row `word` up to its first 0 (at most stride-1), empty for a bad word or face."""
    w, f = int(st["word"]), int(st["face"])
    if not (0 <= w < words.shape[0] and 0 <= f < n_faces):
        return np.zeros(0, np.int64)
    row = words[w, :stride - 1].astype(np.int64)
    z = np.flatnonzero(row == 0)
    return row[:z[0]] if z.size else row


def pens_of(ids, advance_face, spacing):
    """p_0 .. p_{n-1}, summed sequentially in float32: p_{k+1} = (p_k + adv_k) + sp."""
    sp = np.fmax(F(spacing), F(0))
    pens = np.zeros(len(ids), F)
    p = F(0)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, v in enumerate(ids):
            pens[k] = p
            g = int(v) - 4
            adv = F(advance_face[g]) if 0 <= g < len(advance_face) else F(0)
            p = F(F(p + adv) + sp)
    return pens


def synth(words, pixels, advance, style, H, W):
    """words (n_words, stride) uint8, pixels (faces, glyphs, gh, gw) uint8, advance (faces, glyphs) uint8, style: STYLE_DTYPE records
    -> (n, 1, H, W) float32."""
    n_faces, n_glyphs, gh, gw = pixels.shape
    stride = words.shape[1]
    Y, X = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    out = np.empty((len(style), 1, H, W), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, st in enumerate(style):
            ids = word_of(words, stride, st, n_faces)
            n = len(ids)
            u = (X - st["x0"]) * st["sx"]
            v = (Y - st["y0"]) * st["sy"]
            u = np.fmin(np.fmax(u, F(-1)), MAX_COORD)
            v = np.fmin(np.fmax(v, F(-1)), MAX_COORD)
            s = np.zeros((H, W), F)
            if n:
                face = int(st["face"])
                pens = pens_of(ids, advance[face], st["spacing"])
                k = np.searchsorted(pens, u, side="right") - 1                # the largest k with p_k <= u; -1: none (u < 0)
                kc = np.clip(k, 0, n - 1)
                g = ids[kc] - 4
                drawn = (k >= 0) & (g >= 0) & (g < n_glyphs)
                gc = np.clip(g, 0, n_glyphs - 1)
                lu = np.where(drawn, u - pens[kc], F(0)).astype(F)
                xif, yif = np.floor(lu), np.floor(v)
                fx, fy = lu - xif, v - yif
                xi, yi = xif.astype(np.int64), yif.astype(np.int64)

                def tap(r, c):
                    inside = drawn & (r >= 0) & (r < gh) & (c >= 0) & (c < gw)
                    return np.where(inside, pixels[face, gc, np.clip(r, 0, gh - 1), np.clip(c, 0, gw - 1)], 0).astype(F)

                a, b, c, d = tap(yi, xi), tap(yi, xi + 1), tap(yi + 1, xi), tap(yi + 1, xi + 1)
                gx, gy = F(1) - fx, F(1) - fy
                top = gx * a + fx * b
                bot = gx * c + fx * d
                s = np.where(drawn, gy * top + fy * bot, F(0)).astype(F)
                assert lu.dtype == np.float32 and top.dtype == np.float32
            o = st["bg"] + (st["fg"] - st["bg"]) * (s / F(255))
            out[i, 0] = np.fmin(np.fmax(o, F(0)), F(255))
            assert u.dtype == np.float32 and s.dtype == np.float32 and o.dtype == np.float32
    return out


def targets(words, style, n_faces, L):
    """(targets, targets_eval), (n, L) int32: GO ids.. PAD.. and ids.. EOS PAD.., a word longer than L-1 cut."""
    stride = words.shape[1]
    tg = np.full((len(style), L), PAD, np.int32)
    te = np.full((len(style), L), PAD, np.int32)
    for i, st in enumerate(style):
        ids = word_of(words, stride, st, n_faces)
        n = len(ids)
        for j in range(L):
            tg[i, j] = GO if j == 0 else (ids[j - 1] if j - 1 < n else PAD)
            te[i, j] = ids[j] if j < n else (EOS if j == n else PAD)
    return tg, te
