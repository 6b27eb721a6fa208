"""On-device synthetic word lines: lexicon words rendered from a glyph atlas into a batch of line crops and its targets, through
``aocr_synth_lines`` (include/aocr.h).  The reference trains on such data (src/train.lua:21: rendered dictionary words, each stretched to
32 x 100 by data_gen.lua:78); ``SynthGen`` produces it where the train step reads it, with no image files and no host image path.  The host
only draws one small style record per image; everything is counter-based, so ``(seed, counter)`` fixes a batch and a resumed run that
restores the counter sees the same pixels.  There is no CPU fallback for the rendering.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from . import synth
from ._lib import GlyphAtlasDesc, SynthStyle, check, lib, ptr
from .data import IMG_H

STYLE_STREAM = 0x53594E00          # stream of the per-image uniforms: counter_uniform(seed, STYLE_STREAM + counter, 9 n)
DRAWS = 9
FIRST_GLYPH_ID = 4                 # glyph g draws vocab id g + 4 (ids 1..3 are PAD, GO, EOS)
DEFAULT_CHARS = "0123456789abcdefghijklmnopqrstuvwxyz"          # ids 4..39 in the order of utils.lua:104-118
DEFAULT_ATLAS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "glyph_atlas.txt")
ATLAS_MAGIC = "aocr-glyph-atlas 1"
ATLAS_LEVELS = ".123456789abcdef"  # the text form's 16 ink levels: character l is coverage 17 l, so '.' is paper and 'f' is 255
STYLE_DTYPE = np.dtype([("word", "<i4"), ("face", "<i4")] + [(n, "<f4") for n in ("spacing", "sx", "sy", "x0", "y0", "fg", "bg")])
assert STYLE_DTYPE.itemsize == C.sizeof(SynthStyle)


def render_atlas(paths, gh=32, chars=DEFAULT_CHARS):
    """(pixels, advance, names) of the fonts at `paths`, one face each, through Pillow: every face is set at the largest size at which
    the ink of `chars` (highest ascender to lowest descender) fits `gh` rows, on one baseline; glyph g is chars[g] drawn with its pen at
    column 0, its advance rounded to whole atlas pixels in 1..gw; gw is the widest advance or ink extent of any face, at most 64."""
    try:
        from PIL import Image, ImageDraw, ImageFont
    except ImportError as e:
        raise ImportError("GlyphAtlas.from_font needs Pillow (GlyphAtlas.default() and the rendering itself do not)") from e
    faces, names = [], []
    for path in paths:
        size, font, box = 4, None, None
        while True:                                                     # the largest size whose ink fits gh rows
            f = ImageFont.truetype(path, size)
            b = f.getbbox(chars, anchor="ls")
            if b[3] - b[1] > gh:
                break
            font, box, size = f, b, size + 1
        if font is None:
            raise ValueError(f"{path}: no size of this font fits {gh} rows")
        base = -box[1]                                                  # row of the baseline
        glyphs = []
        for ch in chars:
            right = max(int(math.ceil(font.getbbox(ch, anchor="ls")[2])), 1)
            im = Image.new("L", (max(right, 1), gh), 0)
            ImageDraw.Draw(im).text((0, base), ch, font=font, fill=255, anchor="ls")
            glyphs.append((np.asarray(im, dtype=np.uint8), int(round(font.getlength(ch)))))
        faces.append(glyphs)
        names.append("%s %s %dpx" % (font.getname() + (size - 1,)))
    gw = min(64, max(max(g.shape[1], a) for glyphs in faces for g, a in glyphs))
    pixels = np.zeros((len(faces), len(chars), gh, gw), np.uint8)
    advance = np.zeros((len(faces), len(chars)), np.uint8)
    for i, glyphs in enumerate(faces):
        for j, (g, a) in enumerate(glyphs):
            w = min(g.shape[1], gw)
            pixels[i, j, :, :w] = g[:, :w]
            advance[i, j] = min(max(a, 1), gw)
    return pixels, advance, names


class GlyphAtlas:
    """The bitmaps `aocr_synth_lines` draws from: ``pixels`` (faces, glyphs, gh, gw) uint8 ink coverage (0 paper, 255 ink) and
    ``advance`` (faces, glyphs) uint8 pen advance in atlas pixels.  Glyph g draws vocab id g + 4; gh, gw in 1..64, at most 252 glyphs.
    ``names`` lists what the faces were made from.  ``.to(device)`` uploads once; ``.desc()`` is the `aocr_glyph_atlas` over the upload."""

    def __init__(self, pixels, advance, names=None):
        pixels, advance = np.asarray(pixels), np.asarray(advance)
        if pixels.dtype != np.uint8 or advance.dtype != np.uint8 or pixels.ndim != 4 or advance.shape != pixels.shape[:2]:
            raise ValueError("GlyphAtlas takes pixels (faces, glyphs, gh, gw) and advance (faces, glyphs), both uint8")
        f, g, gh, gw = pixels.shape
        if not (f >= 1 and 1 <= g <= 252 and 1 <= gh <= 64 and 1 <= gw <= 64):
            raise ValueError(f"GlyphAtlas: faces={f} (>= 1) glyphs={g} (1..252) gh={gh} gw={gw} (1..64)")
        self.pixels, self.advance = np.ascontiguousarray(pixels), np.ascontiguousarray(advance)
        self.names = list(names) if names is not None else []
        self._dev = None

    n_faces = property(lambda self: int(self.pixels.shape[0]))
    n_glyphs = property(lambda self: int(self.pixels.shape[1]))
    gh = property(lambda self: int(self.pixels.shape[2]))
    gw = property(lambda self: int(self.pixels.shape[3]))

    @classmethod
    def default(cls) -> "GlyphAtlas":
        """the shipped atlas: 0-9 a-z at gh = 32 (tools/make_glyph_atlas.py wrote it; `names` says from which fonts)."""
        return cls.load(DEFAULT_ATLAS)

    @classmethod
    def load(cls, path) -> "GlyphAtlas":
        """reads the text form `save` writes."""
        with open(path, encoding="ascii") as f:
            lines = [ln.rstrip("\n") for ln in f if not ln.startswith("#")]
        head = lines[0].split() if lines else []
        if not lines or not lines[0].startswith(ATLAS_MAGIC + " ") or head[2:9:2] != ["faces", "glyphs", "gh", "gw"]:
            raise ValueError(f"{path}: not a glyph atlas ('{ATLAS_MAGIC} faces F glyphs G gh H gw W' expected on the first line)")
        nf, ng, gh, gw = (int(v) for v in head[3:10:2])
        pixels, advance, names = np.zeros((nf, ng, gh, gw), np.uint8), np.zeros((nf, ng), np.uint8), []
        level = {c: 17 * l for l, c in enumerate(ATLAS_LEVELS)}
        at = 1
        for i in range(nf):
            tag, idx, name = lines[at].split(" ", 2)
            if tag != "face" or int(idx) != i:
                raise ValueError(f"{path}: 'face {i} NAME' expected, found {lines[at]!r}")
            names.append(name)
            at += 1
            for j in range(ng):
                w = lines[at].split()
                if w[0::2] != ["glyph", "advance"] or int(w[1]) != j:
                    raise ValueError(f"{path}: 'glyph {j} advance A' expected, found {lines[at]!r}")
                advance[i, j] = int(w[3])
                rows = lines[at + 1:at + 1 + gh]
                if len(rows) != gh:
                    raise ValueError(f"{path}: face {i} glyph {j}: {gh} rows expected")
                for y, row in enumerate(rows):
                    if row[:1] != "|" or len(row) > gw + 1:
                        raise ValueError(f"{path}: face {i} glyph {j} row {y}: '|' and at most {gw} level characters expected")
                    pixels[i, j, y, :len(row) - 1] = [level[c] for c in row[1:]]
                at += 1 + gh
        return cls(pixels, advance, names)

    @classmethod
    def from_font(cls, paths, gh=32, chars=DEFAULT_CHARS) -> "GlyphAtlas":
        """one face per font file (TrueType / OpenType), rendered now through Pillow; `chars[g]` becomes glyph g."""
        return cls(*render_atlas([paths] if isinstance(paths, (str, os.PathLike)) else list(paths), gh, chars))

    def save(self, path):
        """writes the atlas as text that reads as pictures: a line 'aocr-glyph-atlas 1 faces F glyphs G gh H gw W', then per face
        'face i NAME', and per glyph 'glyph g advance A' and gh rows, each '|' and one character of ATLAS_LEVELS per pixel, trailing
        paper left off.  The coverage is rounded to the 16 levels (to 17 l; 0 and 255 stay exact), so `load` returns the rounded atlas."""
        q = (self.pixels.astype(np.int32) * 15 + 127) // 255
        names = self.names + [""] * (self.n_faces - len(self.names))
        with open(path, "w", encoding="ascii") as f:
            f.write("%s faces %d glyphs %d gh %d gw %d\n" % (ATLAS_MAGIC, self.n_faces, self.n_glyphs, self.gh, self.gw))
            for i in range(self.n_faces):
                f.write("face %d %s\n" % (i, names[i] or "unnamed"))
                for j in range(self.n_glyphs):
                    f.write("glyph %d advance %d\n" % (j, self.advance[i, j]))
                    for row in q[i, j]:
                        f.write("|" + "".join(ATLAS_LEVELS[v] for v in row).rstrip(ATLAS_LEVELS[0]) + "\n")

    def to(self, device) -> "GlyphAtlas":
        device = torch.device(device)
        self._dev = (torch.from_numpy(self.pixels).to(device), torch.from_numpy(self.advance).to(device))
        return self

    def desc(self) -> GlyphAtlasDesc:
        """`aocr_glyph_atlas` over the uploaded arrays (keep this GlyphAtlas alive while the descriptor is in use)."""
        if self._dev is None:
            raise RuntimeError("GlyphAtlas.to(device) has not been called")
        return GlyphAtlasDesc(ptr(self._dev[0]), ptr(self._dev[1]), self.n_faces, self.n_glyphs, self.gh, self.gw)


def word_ids(row):
    """the ids of a lexicon row: up to its first 0, at most stride-1."""
    row = np.asarray(row)[:-1]
    z = np.flatnonzero(row == 0)
    return row[:z[0]] if z.size else row


def host_targets(rows):
    """(targets, targets_eval, num_nonzeros) of lexicon rows as DataGen._emit builds them: L = longest word + 1."""
    ids = [word_ids(r) for r in rows]
    L = max((len(i) for i in ids), default=0) + 1
    targets = np.full((len(ids), L), synth.PAD, np.int32)
    targets_eval = np.full((len(ids), L), synth.PAD, np.int32)
    nnz = 0
    for b, i in enumerate(ids):
        n = len(i)
        targets[b, 0] = synth.GO
        targets[b, 1:n + 1] = i
        targets_eval[b, :n] = i
        targets_eval[b, n] = synth.EOS
        nnz += n + 1
    return targets, targets_eval, nnz


def synth_lines(lexicon, atlas, style, H, W, L=None, stream=None):
    """`aocr_synth_lines` on an uploaded Lexicon and GlyphAtlas and a STYLE_DTYPE array: the (n,1,H,W) fp32 device images, and with
    `L` also the (n,L) int32 device targets and targets_eval.  Enqueues only."""
    dev = lexicon._dev.device
    n = len(style)
    out = torch.empty((n, 1, H, W), dtype=torch.float32, device=dev)
    tg = torch.empty((n, L), dtype=torch.int32, device=dev) if L else None
    te = torch.empty((n, L), dtype=torch.int32, device=dev) if L else None
    if n:
        sd = torch.from_numpy(np.ascontiguousarray(style, dtype=STYLE_DTYPE).view(np.uint8).copy()).to(dev)
        ld, ad = lexicon.desc(), atlas.desc()
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(lib.aocr_synth_lines(st, C.byref(ld), C.byref(ad), ptr(sd), n, H, W, L or 1, ptr(out), ptr(tg), ptr(te)), "aocr_synth_lines")
    return (out, tg, te) if L else out


class SynthGen:
    """``SynthGen(lexicon, atlas, width=100, ...)``: DataGen's surface (``shuffle()``, ``size()``, ``nextBatch(batch_size)``) over rendered
    words of an ``aocr.Lexicon``.  ``nextBatch`` returns ``[images_dev, targets, targets_eval, num_nonzeros, words]``: the images a
    (n,1,32,width) fp32 device tensor, the targets host arrays built from ``Lexicon.array`` by DataGen's rule, so ``Model.step`` takes the
    batch as it is; ``None`` ends an epoch of ``size()`` = ``epoch_size`` (default: the lexicon's length) images.  ``next_device`` returns
    ``[images_dev, targets_dev, targets_eval_dev]`` with the kernel-made device targets, for a loop on ``Model.train_step_device`` that
    never waits for the device.  Batch k is drawn under ``synth_counter = k`` (+1 per batch; a plain attribute: a resumed run sets it);
    ``augment=Augmenter(...)`` is applied to every batch under ``augment_counter``, exactly as DataGen applies it.  Words are drawn
    independently per image, so ``shuffle()`` has nothing to reorder; it is kept for the surface.

    ``params(n, counter)`` -- the `aocr_synth_style` records of the n images of batch ``counter`` (STYLE_DTYPE).  Image i draws nine
    uniforms ``u0..u8 = synth.counter_uniform(seed, 0x53594E00 + counter, 9 n)[9 i : 9 i + 9]`` and, in float64, with (lo, hi) the
    constructor's ranges and r(u, (lo, hi)) = lo + u (hi - lo):

        word    = min(floor(u0 * n_words), n_words - 1)         face = min(floor(u1 * n_faces), n_faces - 1)
        spacing = r(u2, spacing)                                th   = 32 * r(u3, height)     (text height in output pixels, <= 32)
        total   = sum of the word's advances in `face` (0 for an id the atlas lacks) + (n_ids - 1) * spacing
        tw      = width                                         if fill_width (data_gen.lua:78: every word fills the crop)
                = min(total / (sy * stretch ** (2 u4 - 1)), width)   otherwise (the glyphs' aspect up to `stretch`, shrunk to fit)
        sy      = gh / th                                       sx   = total / tw        (sx = sy for a word without width)
        x0      = u5 * (width - tw)                             y0   = u6 * (32 - th)
        fg      = r(u7, fg)                                     bg   = r(u8, bg)

    so the text box [x0, x0 + tw) x [y0, y0 + th) lies inside the image in both modes.  The values are cast once to fp32.
    """

    def __init__(self, lexicon, atlas, width=100, seed=910820, augment=None, spacing=(0.0, 2.0), height=(0.6, 1.0), stretch=1.25,
                 fg=(0.0, 80.0), bg=(170.0, 255.0), fill_width=True, epoch_size=None, device=None):
        if lexicon.n_words < 1:
            raise ValueError("SynthGen needs a lexicon with at least one word")
        if not (0 < height[0] <= height[1] <= 1) or spacing[0] < 0 or spacing[1] < spacing[0] or stretch < 1 or width < 1:
            raise ValueError("height: fractions of 32 with 0 < lo <= hi <= 1; spacing: 0 <= lo <= hi; stretch >= 1; width >= 1")
        self.lexicon, self.atlas = lexicon, atlas
        self.imgH, self.width, self.seed = IMG_H, int(width), int(seed)
        self.augment = augment                   # an aocr.Augmenter or None
        self.augment_counter = 0                 # +1 per emitted batch, as DataGen's
        self.synth_counter = 0                   # batch counter of the style draw: +1 per emitted batch; a resumed run sets it
        self.spacing, self.height, self.stretch = tuple(map(float, spacing)), tuple(map(float, height)), float(stretch)
        self.fg, self.bg, self.fill_width = tuple(map(float, fg)), tuple(map(float, bg)), bool(fill_width)
        self.epoch_size = int(epoch_size) if epoch_size is not None else lexicon.n_words
        self.device = device
        self.cursor = 0
        ids = lexicon.array.astype(np.int64)
        live = np.cumprod(ids[:, :-1] != 0, axis=1).astype(bool)                                  # up to the first 0, at most stride-1 ids
        g = ids[:, :-1] - FIRST_GLYPH_ID
        known = live & (g >= 0) & (g < atlas.n_glyphs)
        adv = atlas.advance.astype(np.float64)[:, np.clip(g, 0, atlas.n_glyphs - 1)]              # (faces, words, stride-1)
        self._adv_sum = (adv * known[None]).sum(axis=2)                                           # (faces, words)
        self._n_ids = live.sum(axis=1)

    def shuffle(self, seed=None):
        pass

    def size(self):
        return self.epoch_size

    def params(self, n, counter):
        """numpy structured array (STYLE_DTYPE, one `aocr_synth_style` per image) of batch ``counter``; host only."""
        u = synth.counter_uniform(self.seed, STYLE_STREAM + int(counter), DRAWS * n).reshape(n, DRAWS)
        r = lambda col, rng: rng[0] + u[:, col] * (rng[1] - rng[0])
        W, H = float(self.width), float(self.imgH)
        word = np.minimum(np.floor(u[:, 0] * self.lexicon.n_words), self.lexicon.n_words - 1).astype(np.int64)
        face = np.minimum(np.floor(u[:, 1] * self.atlas.n_faces), self.atlas.n_faces - 1).astype(np.int64)
        sp = r(2, self.spacing)
        th = H * r(3, self.height)
        sy = self.atlas.gh / th
        total = self._adv_sum[face, word] + np.maximum(self._n_ids[word] - 1, 0) * sp
        if self.fill_width:
            tw = np.full(n, W)
        else:
            tw = np.minimum(total / (sy * np.exp((2.0 * u[:, 4] - 1.0) * math.log(self.stretch))), W)
        wide = total > 0
        sx = np.where(wide, total / np.where(wide, tw, 1.0), sy)
        out = np.zeros(n, STYLE_DTYPE)
        out["word"], out["face"] = word, face
        cols = dict(spacing=sp, sx=sx, sy=sy, x0=u[:, 5] * (W - np.where(wide, tw, 0.0)), y0=u[:, 6] * (H - th), fg=r(7, self.fg), bg=r(8, self.bg))
        for name, v in cols.items():
            out[name] = v.astype(np.float32)
        return out

    def _device(self):
        dev = self.device or torch.device("cuda", torch.cuda.current_device())
        if self.lexicon._dev is None or self.lexicon._dev.device != torch.device(dev):
            self.lexicon.to(dev)
        if self.atlas._dev is None or self.atlas._dev[0].device != torch.device(dev):
            self.atlas.to(dev)

    def _next(self, batch_size, device_targets):
        if self.cursor >= self.epoch_size:
            self.cursor = 0
            return None
        n = min(int(batch_size), self.epoch_size - self.cursor)
        self.cursor += n
        self._device()
        style = self.params(n, self.synth_counter)
        self.synth_counter += 1
        rows = self.lexicon.array[style["word"]]
        if device_targets:
            L = int(self._n_ids[style["word"]].max()) + 1
            images, tg, te = synth_lines(self.lexicon, self.atlas, style, self.imgH, self.width, L)
        else:
            images = synth_lines(self.lexicon, self.atlas, style, self.imgH, self.width)
        if self.augment is not None:
            images = self.augment.apply(images, self.augment_counter)
            self.augment_counter += 1
        if device_targets:
            return [images, tg, te]
        tg, te, nnz = host_targets(rows)
        return [images, tg, te, nnz, [self.lexicon.words[w] for w in style["word"]]]

    def nextBatch(self, batch_size):
        return self._next(batch_size, False)

    def next_device(self, batch_size):
        return self._next(batch_size, True)
