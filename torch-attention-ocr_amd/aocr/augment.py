"""On-device training augmentation: a random affine warp, contrast / brightness jitter and additive noise of a preprocessed
``(n,1,H,W)`` batch, through ``aocr_augment_lines`` (include/aocr.h).  The image never leaves HBM; the host only draws the
per-image records.  Everything is counter-based: ``(seed, counter)`` fixes the records and the noise field, so a resumed run
that restores the counter sees the same pixels.  There is no CPU fallback for ``apply``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import synth
from ._lib import check, lib, ptr
from .degrade import Degrader

PARAM_STREAM = 0x41554700          # stream of the per-image uniforms: counter_uniform(seed, PARAM_STREAM + counter, 8 n)


class Warp(C.Structure):
    """mirror of `aocr_warp` (include/aocr.h)."""
    _fields_ = [(n, C.c_float) for n in ("m00", "m01", "m02", "m10", "m11", "m12", "gain", "offset", "fill", "noise")]


WARP_DTYPE = np.dtype([(n, "<f4") for n, _ in Warp._fields_])


class Augmenter:
    """``Augmenter(rotate_deg, shear, scale, translate, contrast, brightness, noise, fill, seed)``: every range is symmetric
    about "no change" and the defaults are no change, so a default ``Augmenter`` is the identity.

    ``params(n, H, W, counter)`` -- the records of the ``n`` images of batch ``counter``.  Image ``i`` draws eight uniforms
    ``u0..u7 = synth.counter_uniform(seed, 0x41554700 + counter, 8 n)[8 i : 8 i + 8]`` and, with ``j(u) = 2 u - 1``, in float64:

        theta = radians(j(u0) * rotate_deg)             k  = j(u1) * shear
        sx    = exp(j(u2) * ln scale)                   sy = exp(j(u3) * ln scale)
        tx    = j(u4) * translate[0]                    ty = j(u5) * translate[1]
        g     = exp(j(u6) * ln contrast)                b  = j(u7) * brightness

        A = R(theta) . S(k) . diag(1/sx, 1/sy)
          = [[cos, -sin], [sin, cos]] . [[1, k], [0, 1]] . [[1/sx, 0], [0, 1/sy]]
          = [[cos / sx, (k cos - sin) / sy],
             [sin / sx, (k sin + cos) / sy]]

    ``A`` maps an output pixel to its source about the image centre ``c = ((W-1)/2, (H-1)/2)``, then the translation is added:
    ``source = A (p - c) + c + t``, that is

        m00 = A00   m01 = A01   m02 = cx + tx - (A00 cx + A01 cy)
        m10 = A10   m11 = A11   m12 = cy + ty - (A10 cx + A11 cy)
        gain = g    offset = 128 (1 - g) + b            fill, noise: the constructor's

    (det A = 1 / (sx sy)).  The ten values are composed in float64 and cast once to fp32; negative zeros are normalised to +0.

    ``degrade``: a ``Degrader`` (aocr/degrade.py) whose elastic displacement, stroke weight and blur ``apply`` runs first, under the same
    counter and on the same stream: ink, paper and optics come before the camera's map and the sensor's noise (a blur after the noise would
    remove it).  None: this stage alone.
    """

    def __init__(self, rotate_deg=0.0, shear=0.0, scale=1.0, translate=(0.0, 0.0), contrast=1.0, brightness=0.0, noise=0.0,
                 fill=255.0, seed=910820, degrade=None):
        if degrade is not None and not isinstance(degrade, Degrader):
            raise TypeError("degrade is an aocr.Degrader or None")
        self.degrade = degrade
        if scale <= 0 or contrast <= 0:
            raise ValueError("scale and contrast are ratios > 0 (1 = no change)")
        self.rotate_deg, self.shear, self.scale = float(rotate_deg), float(shear), float(scale)
        self.translate = (float(translate[0]), float(translate[1]))
        self.contrast, self.brightness, self.noise, self.fill = float(contrast), float(brightness), float(noise), float(fill)
        self.seed = int(seed)

    def params(self, n, H, W, counter):
        """numpy structured array (WARP_DTYPE, one `aocr_warp` per image) of batch ``counter``; host only."""
        u = synth.counter_uniform(self.seed, PARAM_STREAM + int(counter), 8 * n).reshape(n, 8)
        j = 2.0 * u - 1.0
        theta = np.radians(j[:, 0] * self.rotate_deg)
        k = j[:, 1] * self.shear
        sx, sy = np.exp(j[:, 2] * math.log(self.scale)), np.exp(j[:, 3] * math.log(self.scale))
        tx, ty = j[:, 4] * self.translate[0], j[:, 5] * self.translate[1]
        g = np.exp(j[:, 6] * math.log(self.contrast))
        b = j[:, 7] * self.brightness
        cos, sin = np.cos(theta), np.sin(theta)
        a00, a01 = cos / sx, (k * cos - sin) / sy
        a10, a11 = sin / sx, (k * sin + cos) / sy
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        cols = dict(m00=a00, m01=a01, m02=cx + tx - (a00 * cx + a01 * cy),
                    m10=a10, m11=a11, m12=cy + ty - (a10 * cx + a11 * cy),
                    gain=g, offset=128.0 * (1.0 - g) + b,
                    fill=np.full(n, self.fill), noise=np.full(n, self.noise))
        out = np.zeros(n, WARP_DTYPE)
        for name, v in cols.items():
            out[name] = (v + 0.0).astype(np.float32)           # + 0.0: -0 -> +0
        return out

    def apply(self, images_dev, counter, stream=None):
        """a new ``(n,1,H,W)`` fp32 device tensor: ``images_dev`` under the records and the noise field of batch ``counter``."""
        if not (images_dev.is_cuda and images_dev.dtype == torch.float32 and images_dev.dim() == 4 and images_dev.shape[1] == 1):
            raise ValueError("apply() takes a (n,1,H,W) fp32 device tensor (there is no CPU fallback)")
        if self.degrade is not None:
            images_dev = self.degrade.apply(images_dev, counter, stream)
        images_dev = images_dev.contiguous()
        n, _, H, W = images_dev.shape
        if n == 0:
            return torch.empty_like(images_dev)
        warp = torch.from_numpy(self.params(n, H, W, counter).view(np.uint8).copy()).to(images_dev.device)
        out = torch.empty_like(images_dev)
        st = stream if stream is not None else torch.cuda.current_stream(images_dev.device).cuda_stream
        check(lib.aocr_augment_lines(st, ptr(images_dev), ptr(warp), n, H, W, self.seed, int(counter), ptr(out)), "aocr_augment_lines")
        return out
