"""On-device scan degradation of a ``(n,1,H,W)`` batch, through ``aocr_degrade_lines`` (include/aocr.h): a local (elastic) displacement,
stroke thickening or thinning, and optical blur -- what a rendered glyph lacks and a global affine map cannot give it.  It runs before
``aocr_augment_lines`` (``Augmenter(degrade=Degrader(...))``): ink, paper and optics come before the camera's map and the sensor's noise.
The host draws the per-image records, blur taps included (the device computes no exp); the displacement field is counter-based on the device.
``(seed, counter)`` fixes both, so a resumed run that restores the counter sees the same pixels.  There is no CPU fallback for ``apply``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import synth
from ._lib import check, lib, ptr

PARAM_STREAM = 0x4445475200000000   # stream of the per-image uniforms: counter_uniform(seed, PARAM_STREAM + counter, 4 n); not augment.PARAM_STREAM
MAX_BLUR_SIGMA = 1.5                # the blur has taps at -4..4: a wider Gaussian would be cut off visibly (at 1.5 the first dropped tap is 0.4 % of the centre)


class Degrade(C.Structure):
    """mirror of `aocr_degrade` (include/aocr.h)."""
    _fields_ = [("amp_x", C.c_float), ("amp_y", C.c_float), ("pitch", C.c_int32), ("inv_pitch", C.c_float), ("thick", C.c_float),
                ("taps", C.c_float * 5), ("fill", C.c_float)]


DEGRADE_DTYPE = np.dtype([("amp_x", "<f4"), ("amp_y", "<f4"), ("pitch", "<i4"), ("inv_pitch", "<f4"), ("thick", "<f4"), ("taps", "<f4", (5,)),
                          ("fill", "<f4")])
assert DEGRADE_DTYPE.itemsize == C.sizeof(Degrade)


def blur_taps(sigma):
    """(n, 5) float64: w0..w4 of the 9-tap Gaussian of every sigma, w0 + 2 (w1 + .. + w4) = 1; sigma 0 gives (1, 0, 0, 0, 0)."""
    sigma = np.asarray(sigma, np.float64).reshape(-1)
    k = np.arange(5, dtype=np.float64)
    w = np.zeros((sigma.size, 5))
    w[:, 0] = 1.0
    on = sigma > 0
    with np.errstate(divide="ignore"):                      # a denormal sigma squares to 0: exp(-inf) = 0, the identity taps
        w[on, 1:] = np.exp(-(k[1:] ** 2) / (2.0 * sigma[on, None] ** 2))
    return w / (w[:, :1] + 2.0 * w[:, 1:].sum(axis=1, keepdims=True))


def degrade_lines(images_dev, records, seed, counter, stream=None):
    """``aocr_degrade_lines`` on a ``(n,1,H,W)`` fp32 device tensor under ``records`` (host, DEGRADE_DTYPE, one per image): a new tensor.
    The C call cannot see the records (they are device memory by then), so what it cannot check is checked here, before anything is uploaded
    or enqueued."""
    if not (images_dev.is_cuda and images_dev.dtype == torch.float32 and images_dev.dim() == 4 and images_dev.shape[1] == 1):
        raise ValueError("degrade takes a (n,1,H,W) fp32 device tensor (there is no CPU fallback)")
    images_dev = images_dev.contiguous()
    n, _, H, W = images_dev.shape
    records = np.ascontiguousarray(records)
    if records.dtype != DEGRADE_DTYPE or records.shape != (n,):
        raise ValueError(f"records: {n} aocr_degrade records (DEGRADE_DTYPE), one per image")
    if n and int(records["pitch"].min()) < 2:
        raise ValueError("aocr_degrade.pitch must be >= 2")
    if n == 0:
        return torch.empty_like(images_dev)
    rec = torch.from_numpy(records.view(np.uint8).copy()).to(images_dev.device)
    out = torch.empty_like(images_dev)
    st = stream if stream is not None else torch.cuda.current_stream(images_dev.device).cuda_stream
    check(lib.aocr_degrade_lines(st, ptr(images_dev), ptr(rec), n, H, W, int(seed), int(counter), ptr(out)), "aocr_degrade_lines")
    return out


class Degrader:
    """``Degrader(blur_sigma, thickness, elastic, pitch, fill, seed)``: every argument is the largest amount of its effect and the defaults are
    none, so a default ``Degrader`` is the identity.

    ``params(n, H, W, counter)`` -- the records of the ``n`` images of batch ``counter``.  Image ``i`` draws four uniforms
    ``u0..u3 = synth.counter_uniform(seed, 0x4445475200000000 + counter, 4 n)[4 i : 4 i + 4]`` and, in float64:

        sigma = u0 * blur_sigma                         thick = (2 u1 - 1) * thickness
        amp_x = u2 * elastic[0]                         amp_y = u3 * elastic[1]
        taps[k] = exp(-k^2 / (2 sigma^2)) / (the sum over k = -4..4), k = 0..4;  sigma = 0: (1, 0, 0, 0, 0)
        pitch, inv_pitch = 1 / pitch, fill: the constructor's

    each value cast once to fp32; negative zeros are normalised to +0.  thick > 0 darkens (thickens) strokes, < 0 thins them.
    """

    def __init__(self, blur_sigma=0.0, thickness=0.0, elastic=(0.0, 0.0), pitch=8, fill=255.0, seed=910820):
        if not 0 <= blur_sigma <= MAX_BLUR_SIGMA:
            raise ValueError(f"blur_sigma must be in 0..{MAX_BLUR_SIGMA}: the blur has four taps a side, which would cut a wider Gaussian off visibly")
        if not abs(thickness) <= 1:
            raise ValueError("thickness must be in -1..1 (the share of the 3x3 minimum or maximum in a pixel)")
        if int(pitch) != pitch or pitch < 2:
            raise ValueError("pitch must be an integer >= 2 (pixels between displacement nodes)")
        if not (elastic[0] >= 0 and elastic[1] >= 0):
            raise ValueError("elastic amplitudes (x, y) are >= 0 pixels")
        self.blur_sigma, self.thickness = float(blur_sigma), float(thickness)
        self.elastic = (float(elastic[0]), float(elastic[1]))
        self.pitch, self.fill, self.seed = int(pitch), float(fill), int(seed)

    def params(self, n, H, W, counter):
        """numpy structured array (DEGRADE_DTYPE, one `aocr_degrade` per image) of batch ``counter``; host only.  H and W play no part (the
        amplitudes are in pixels); they are taken for symmetry with ``Augmenter.params``."""
        u = synth.counter_uniform(self.seed, PARAM_STREAM + int(counter), 4 * n).reshape(n, 4)
        out = np.zeros(n, DEGRADE_DTYPE)
        cols = dict(amp_x=u[:, 2] * self.elastic[0], amp_y=u[:, 3] * self.elastic[1], inv_pitch=np.full(n, 1.0 / self.pitch),
                    thick=(2.0 * u[:, 1] - 1.0) * self.thickness, taps=blur_taps(u[:, 0] * self.blur_sigma), fill=np.full(n, self.fill))
        for name, v in cols.items():
            out[name] = (v + 0.0).astype(np.float32)           # + 0.0: -0 -> +0
        out["pitch"] = self.pitch
        return out

    def apply(self, images_dev, counter, stream=None):
        """a new ``(n,1,H,W)`` fp32 device tensor: ``images_dev`` under the records and the displacement field of batch ``counter``."""
        n, H, W = images_dev.shape[0], images_dev.shape[-2], images_dev.shape[-1]
        return degrade_lines(images_dev, self.params(n, H, W, counter), self.seed, counter, stream)
