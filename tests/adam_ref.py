"""numpy restatement of aocr_adam_update (include/aocr.h; csrc/optim.hip): the element arithmetic in float32, every operation rounded on its
own and in the header's order, the running products of the bias correction in float64.  The clip scales are an INPUT (the kernel's norms are
sums in another order; tests compare those against float64 norms and hand the reported scales to this file).  A plain module imported by bare
name, like the other *_ref.py files."""
import numpy as np

F = np.float32


class State:
    """{m | v} and the tail {p1, p2, steps}: all zero = a fresh optimizer."""

    def __init__(self, n):
        self.m, self.v = np.zeros(n, F), np.zeros(n, F)
        self.p1, self.p2, self.steps = 0.0, 0.0, 0

    def to_bytes(self):
        """the device image: 2n floats, then double p1, double p2, int64 steps, int64 reserved"""
        return self.m.tobytes() + self.v.tobytes() + np.array([self.p1, self.p2], np.float64).tobytes() + np.array([self.steps, 0], np.int64).tobytes()

    def copy(self):
        s = State(0)
        s.m, s.v, s.p1, s.p2, s.steps = self.m.copy(), self.v.copy(), self.p1, self.p2, self.steps
        return s


def per_element(scale, off):
    """scale[k] of the element's group, as a float32 vector of off[5] elements"""
    out = np.ones(off[5], F)
    for k in range(5):
        out[off[k]:off[k + 1]] = F(scale[k])
    return out


def step(w, g, st, off, scale, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0):
    """one applied step: returns the new w (float32) and advances st in place.  w, g: float32 vectors of off[5] elements; scale: 5 floats."""
    lr, beta1, beta2, eps, wd = F(lr), F(beta1), F(beta2), F(eps), F(wd)
    p1, p2 = (1.0, 1.0) if st.steps == 0 else (st.p1, st.p2)
    p1 *= float(beta1); p2 *= float(beta2)                     # Python floats: IEEE double products
    c1, c2 = F(1.0 - p1), F(1.0 - p2)
    w, g = np.asarray(w, F), np.asarray(g, F)
    one = F(1.0)
    gs = g * per_element(scale, off)
    m = beta1 * st.m + (one - beta1) * gs
    v = beta2 * st.v + (one - beta2) * (gs * gs)
    u = (m / c1) / (np.sqrt(v / c2) + eps)
    w2 = w - lr * (u + wd * w)
    assert w2.dtype == F and m.dtype == F and v.dtype == F
    st.m, st.v, st.p1, st.p2, st.steps = m, v, p1, p2, st.steps + 1
    return w2


def norms64(w, g, off):
    """(pn[5], gn[5]) in float64"""
    w, g = np.asarray(w, np.float64), np.asarray(g, np.float64)
    return (np.array([np.sqrt((w[off[k]:off[k + 1]] ** 2).sum()) for k in range(5)]),
            np.array([np.sqrt((g[off[k]:off[k + 1]] ** 2).sum()) for k in range(5)]))


def adamw64(w, grads, lr, beta1, beta2, eps, wd):
    """torch.optim.AdamW's update written out in float64 (no amsgrad, no maximize), over the gradient vectors of `grads` in turn:
    w *= 1 - lr wd; m, v moments; w -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps).  Returns w after every step."""
    w = np.asarray(w, np.float64).copy()
    m, v, out = np.zeros_like(w), np.zeros_like(w), []
    for t, g in enumerate(grads, 1):
        g = np.asarray(g, np.float64)
        w *= 1.0 - lr * wd
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        w -= (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
        out.append(w.copy())
    return out
