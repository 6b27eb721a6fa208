"""Float64 restatement of ONE direction of ONE layer of the BiLSTM encoder recurrence as the whole-sequence kernels run it
(csrc/rnn_seq.hip, csrc/rnn_cluster.hip; model.lua:291-316 forward, :662-690 BPTT; the cell of LSTM.lua:79-105), in plain loops over t.
Used by tests/test_enc_seq_ref_cpu.py (checked there against oracle_torch and torch autograd) and tests/test_encoder_seq_kernels_gpu.py.

Conventions (csrc/ops.h: EncSeqDir / EncSeqBwdDir):
  zx      [T][B][4He]   the input part of the pre-activation incl. both biases, gate order [in, forget, out, g]
  W       [4He][He]     the recurrent weight W_h2h:  z(t) = zx(t) + h_b(t') . W^T,  h_b = the bf16 image of h
  slots   [T+2][B][He]  state slot t+1 holds step t; slots 0 and T+1 are the zero initial states
  reverse               the direction that walks t = T-1 .. 0 (its previous step t' = t+1 sits in slot t+2)
  ctx     [B][T][Hd]    element (b, t, j) of direction dir at ctx[(b*T + t)*Hd + dir*He + j]
  gates   "seq": [T][B][4He] (rnn_seq.hip)   "cl": [T][B][He][4] (the cluster kernels)

Two modes:
  free-running  h is rounded to bf16 (RNE of its fp32 image) where the kernels round it (the operand of the next step's product), and
                so is d z in the backward pass; round=False switches the rounding off (the exact recurrence).
  device-fed    step t is computed from the DEVICE's saved hsb(t') and cs(t') (fed=dict(hsb=, cs=), slot layout), in the backward pass
                from the device's dzb of the step processed before (fed_dzb, [T][B][4He]): nothing compounds, every step is an
                independent one-step problem whose only noise is the fp32 product and the cell's transcendental functions."""
import torch

F64 = torch.float64


def rne(x):
    """bf16 image (round to nearest even) of the fp32 image of x, as float64"""
    return x.float().to(torch.bfloat16).to(F64)


def prev_slot(t, reverse):
    """state slot of the step processed before step t"""
    return t + 2 if reverse else t


def steps(T, reverse, it0=0, it1=None):
    """the time steps of iterations [it0, it1) in processing order"""
    it1 = T if it1 is None else it1
    return [T - 1 - it if reverse else it for it in range(it0, it1)]


def gates_layout(g, layout):
    """g [..., 4, He] -> the saved-gates layout of the kernels, flattened to [..., 4He]"""
    if layout == "cl":
        g = g.transpose(-1, -2)
    return g.reshape(*g.shape[:-2], -1)


def gates_unlayout(flat, He, layout):
    """inverse of gates_layout: [..., 4He] -> [..., 4, He]"""
    if layout == "cl":
        return flat.reshape(*flat.shape[:-1], He, 4).transpose(-1, -2)
    return flat.reshape(*flat.shape[:-1], 4, He)


def cell(z, c_prev):
    """LSTM.lua:79-105 on the pre-activation z [B][4][He] -> c, h, gates [B][4][He] = {in, forget, out, g}"""
    i, f, o, g = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.sigmoid(z[:, 2]), torch.tanh(z[:, 3])
    c = f * c_prev + i * g
    return c, o * torch.tanh(c), torch.stack([i, f, o, g], 1)


def forward(zx, W, reverse, round=True, fed=None, it0=0, it1=None):
    """-> dict(cs, hs: [T+2][B][He] slots; gates, z, mag: [T][B][4][He]), float64.  Only the steps of iterations [it0, it1) are filled
    in (the rest stays zero).  mag = |h_b(t')| . |W|^T, the magnitude the fp32 product's error bound scales with.
    fed: the device's slots dict(hsb=, cs=): every step but the sequence's first takes its previous state from them (device-fed)."""
    T, B, He = zx.shape[0], zx.shape[1], W.shape[1]
    zx, W = zx.to(F64), W.to(F64)
    cs, hs = torch.zeros(T + 2, B, He, dtype=F64), torch.zeros(T + 2, B, He, dtype=F64)
    gates, zs, mag = (torch.zeros(T, B, 4, He, dtype=F64) for _ in range(3))
    for n, t in enumerate(steps(T, reverse, it0, it1)):
        ps = prev_slot(t, reverse)
        first = it0 + n == 0
        if first:                                                     # the zero initial state, whatever the slot holds
            h_prev, c_prev = torch.zeros(B, He, dtype=F64), torch.zeros(B, He, dtype=F64)
        elif fed is not None:
            h_prev, c_prev = fed["hsb"][ps].to(F64), fed["cs"][ps].to(F64)
        else:
            h_prev, c_prev = (rne(hs[ps]) if round else hs[ps]), cs[ps]
        z = (zx[t] + h_prev @ W.t()).view(B, 4, He)
        c, h, g = cell(z, c_prev)
        cs[t + 1], hs[t + 1], gates[t], zs[t] = c, h, g, z
        mag[t] = (h_prev.abs() @ W.abs().t()).view(B, 4, He)
    return dict(cs=cs, hs=hs, gates=gates, z=zs, mag=mag)


def context(hs_fw, hs_bw):
    """the two directions' state slots -> ctx [B][T][2He]"""
    return torch.cat([hs_fw[1:-1].transpose(0, 1), hs_bw[1:-1].transpose(0, 1)], 2)


def cell_backward(dh, dc_in, gates, c, c_prev):
    """EpGatesBwd::quad's formulas.  gates [B][4][He] -> d z [B][4][He], d c leaving the step"""
    i, f, o, g = gates[:, 0], gates[:, 1], gates[:, 2], gates[:, 3]
    tc = torch.tanh(c)
    dc = dh * o * (1 - tc * tc) + dc_in
    d_o, di, dg, df = dh * tc, dc * g, dc * i, dc * c_prev
    return torch.stack([di * i * (1 - i), df * f * (1 - f), d_o * o * (1 - o), dg * (1 - g * g)], 1), dc * f


def backward(W, gates, cs, dh1, dh2, dc0, forward_dir, round=True, fed_dzb=None, it0=0, it1=None):
    """BPTT of the direction whose forward pass walked t = 0..T-1 (forward_dir; its BPTT walks T-1..0 and c_prev = slot t) or T-1..0.
    gates [T][B][4][He], cs [T+2][B][He] slots, dh1 [T][B][He] (d h from above), dh2 [B][He] or None (joins the FIRST processed step
    only), dc0 [B][He] (d c entering iteration it0).  -> dict(dz [T][B][4][He], dc (leaving iteration it1-1), db [4][He] = the sum of
    d z over rows and the steps of [it0, it1) -- what the kernels ADD to both bias gradients --, dh, mag [T][B][He])."""
    T, B, He = gates.shape[0], gates.shape[1], gates.shape[3]
    W, gates, cs, dh1 = W.to(F64), gates.to(F64), cs.to(F64), dh1.to(F64)
    dz, dhs, mag = torch.zeros(T, B, 4, He, dtype=F64), torch.zeros(T, B, He, dtype=F64), torch.zeros(T, B, He, dtype=F64)
    dc = dc0.to(F64).clone()
    bptt_reverse = bool(forward_dir)                                  # the BPTT of the forward direction walks t = T-1 .. 0
    for n, t in enumerate(steps(T, bptt_reverse, it0, it1)):
        tb = t + 1 if bptt_reverse else t - 1                         # the step processed before
        if it0 + n == 0:
            zp = torch.zeros(B, 4 * He, dtype=F64)
        elif fed_dzb is not None:
            zp = fed_dzb[tb].to(F64).reshape(B, 4 * He)
        else:
            zp = (rne(dz[tb]) if round else dz[tb]).reshape(B, 4 * He)
        dh = dh1[t] + zp @ W
        if it0 + n == 0 and dh2 is not None:
            dh = dh + dh2.to(F64)
        c_prev = cs[t if forward_dir else t + 2]
        dz[t], dc = cell_backward(dh, dc, gates[t], cs[t + 1], c_prev)
        dhs[t], mag[t] = dh, zp.abs() @ W.abs()
    ts = steps(T, bptt_reverse, it0, it1)
    return dict(dz=dz, dc=dc, db=dz[ts].sum(dim=(0, 1)), dh=dhs, mag=mag)


# ------------------------------------------------------------------------------------------------------------------------------
# operand generators of the GPU test (here, so that the CPU test can assert their condition on every shape the GPU test uses)
# ------------------------------------------------------------------------------------------------------------------------------
Q = 2.0 ** -4                       # weight quantum: W entries are integers in [-W_INT, W_INT] times Q, exact in bf16
W_INT = 2
ZX_SCALE = 2.0                      # zx uniform in [-ZX_SCALE, ZX_SCALE]: with |h| < 1 the product part at He = 512 has a standard
                                    # deviation of ~sqrt(512 * 2) * 0.3 / 16 = 0.6, so well over 90 % of |z| stays inside 4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def weights(He, seed):
    """W_h2h [4He][He], float32 (exact in bf16)"""
    return torch.randint(-W_INT, W_INT + 1, (4 * He, He), generator=_gen(seed)).float() * Q


def inputs(T, B, He, seed):
    """zx [T][B][4He] float32: independent values per row, step and (through the seed) direction"""
    return ((torch.rand(T, B, 4 * He, generator=_gen(seed), dtype=F64) * 2 - 1) * ZX_SCALE).float()


def uniform(shape, scale, seed):
    return ((torch.rand(*shape, generator=_gen(seed), dtype=F64) * 2 - 1) * scale).float()


def z_share(z):
    """share of the pre-activations inside |z| <= 4"""
    return (z.abs() <= 4).double().mean().item()


# (B, T, He) of every forward / backward problem of tests/test_encoder_seq_kernels_gpu.py
SEQ_SHAPES = [(16, 1, 64), (32, 2, 128), (16, 5, 256), (32, 5, 64), (16, 2, 256), (32, 1, 128)]
CL_SHAPES = [(5, 1, 64), (5, 3, 128), (16, 2, 256), (21, 7, 256), (21, 7, 64), (40, 3, 128), (40, 2, 256), (21, 3, 512), (70, 2, 512),
             (16, 7, 128), (5, 7, 512)]
