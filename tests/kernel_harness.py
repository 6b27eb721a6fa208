"""What the kernel-level GPU tests (tests/test_*_kernels*_gpu.py) share: the handle of tests/libkprobe.so with ONE ctypes signature table for
every extern "C" wrapper of tests/kprobe.hip, the launch helpers, the autouse fixture that clears the dispatch switches, sentinel-tailed
device buffers (Buf) and strided windows of them (Mat), exact-operand generators, the bf16 bit images, the AOCR_TRACE assertions and
the shared tolerances.  A plain module imported by bare name, like page_harness.py and the *_ref.py files; the helper bodies are those of
tests/test_kernels_bf16_gpu.py and tests/test_step_kernels_bf16_gpu.py, where the method is described.

pytest rewrites the asserts of test modules only, so every assert here carries its own message.
tests/test_kernel_harness_cpu.py holds SIGS to the source text of tests/kprobe.hip (names, parameter counts, return types) without a device."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_C = 4.0                       # per-element bound of the random cases: BOUND_C * sqrt(K) * 2^-24 * (|A| |B|)
SLACK = 4096                        # sentinel elements behind every device buffer
SENT = -12345.0
SWITCHES = ("AOCR_FORCE_DMA", "AOCR_HALO8", "AOCR_HALO4_STAGED", "AOCR_NO_HALO", "AOCR_NO_DMA128", "AOCR_DMA128_W4", "AOCR_NO_NARROW_STAGED",
            "AOCR_NO_WGRAD_HALO", "AOCR_WGRAD_HALO_RAGGED", "AOCR_NO_WGRAD_ISSUE_MID", "AOCR_WGRAD_ATOMIC", "AOCR_WGRAD_HALO_MINSTEPS",
            "AOCR_HH_NARROW_FULL_ONLY", "AOCR_NO_HH_CAT", "AOCR_NO_WGRAD_DMA_GROUPED", "AOCR_WGRAD_DMA_MINK", "AOCR_DX16", "AOCR_NO_DMA",
            "AOCR_NO_HH_NARROW", "AOCR_NO_NARROW_WIDE", "AOCR_WGRAD_HALO_MINN", "AOCR_BN_Y16", "AOCR_NO_BN_STATS_FUSE", "AOCR_BNB_FUSE",
            "AOCR_WGRAD_DMA_WGS", "AOCR_BN_PARTIAL_OLD", "AOCR_UNPOOL4", "AOCR_CONV1_SCALAR",
            # the exact-fp32 conv / GEMM / step launchers
            "AOCR_NO_LDS_F32", "AOCR_NO_F32T", "AOCR_F32T_TILE", "AOCR_NO_F32W", "AOCR_F32W_MINK", "AOCR_NO_STEP_F32", "AOCR_STEP_F32_W16",
            "AOCR_NO_QUARTER_TILES",
            # the recurrent-step launchers
            "AOCR_NO_HALF_TILES", "AOCR_HALF_TILES_MAXGRID", "AOCR_NO_STEP_MT2", "AOCR_STEP_MT2_MINK", "AOCR_NO_STEPL", "AOCR_STEPL_MIN_WGS",
            "AOCR_STEP_WAVES4", "AOCR_STEP_WAVES16", "AOCR_BIG_STEP", "AOCR_BIG_STEP_MIN_ROWS",
            # the attention launchers
            "AOCR_NO_ATTN_BF16", "AOCR_ATTN_NW16", "AOCR_NO_ATTN_BEAM_GROUP", "AOCR_ATTN_BWD_TWO_PASS", "AOCR_NO_CHAIN_CTXA",
            # the whole-sequence decoder launchers
            "AOCR_NO_DEC_CHAINS", "AOCR_NO_DEC_CHAINS_BWD", "AOCR_NO_DEC_CHAINS_GREEDY", "AOCR_NO_DEC_CHAINS_BEAM", "AOCR_CH_NO_RES", "AOCR_NO_DEC_EARLY", "AOCR_CL_REMOTE",
            "AOCR_DC_STAMPS")
EP_RELU, EP_TANH, EP_ACCUM = 1, 2, 4
TOL_CELL = 2e-5                     # test_ops_gpu.py::test_lstm_cell, exact-fp32 cell
TOL_BWD = 5e-5                      # its backward part (times max(1, max |dh|))
TOL_A, TOL_C = 2e-5, 5e-5           # test_ops_gpu.py::test_attention (c: times max |ctx|)
TOL_DS, TOL_DQ = 5e-5, 1e-4         # times max(1, max |d a|) (d q: and max |ctx|)
JUNK = 3.0                          # what surrounds every operand window (exact in bf16: a wrong stride changes sums)

_KP = None
vp, i32, i64, sz, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float

# ---- tests/kprobe.hip's wrappers: the ctypes argument types of each, in the order of the file.  A stream comes first wherever the wrapper launches.
_STEP = [vp, i32, vp, i32, i32]                                       # stream, nz, the problems (a struct array of the test file), M, cols
_INT = {                                                              # return int: hipGetLastError(), a yes / no, or a constant
    "kp_conv_forward": [vp, i32, vp, vp, vp, vp, vp] + [i32] * 9 + [vp] * 8,
    "kp_conv_backward_data": [vp, i32, vp, vp, vp] + [i32] * 7 + [vp, vp, vp],
    "kp_conv_weight_transpose_f32": [vp, vp, vp, i32, i32, i32],
    "kp_conv_backward_data_f32": [vp, vp, vp, vp, vp] + [i32] * 7,
    "kp_conv_backward_filter": [vp, i32, vp, vp, vp, vp] + [i32] * 7 + [vp, vp, vp, sz],
    "kp_conv_weight_shadows": [vp, vp, vp, vp, i32, i32, i32],
    "kp_splitk_reduce": [vp, vp, i32, sz, vp],
    "kp_gemm_hh": [vp, vp, i64, vp, i64, vp, i64, i32, i32, i32, vp, vp, i32],
    "kp_gemm_hh_shadow": [vp, vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32],
    "kp_gemm_hh_cat": [vp, vp, vp, i64, vp, vp, i64, vp, i64, i32, i32, i32, i32, vp],
    "kp_grouped_wgrad": [vp, i32, i32] + [vp] * 11 + [vp, sz],
    "kp_bn_relu_forward": [vp] * 9 + [i64, i32, i32, i32, i32],
    "kp_bn_eval_prepare": [vp, vp, vp, vp, i32],
    # BatchNorm, un-pool, conv1, column sums (tests/test_cnn_elementwise_kernels_gpu.py)
    "kp_bn_relu_forward2": [vp] * 9 + [i64, i32, i32, i32, i32, vp, i32, i32, vp],
    "kp_bn_relu_backward": [vp] * 10 + [i64, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, i32],
    "kp_unpool_relu_backward": [vp] * 5 + [i32] * 5 + [vp, vp, vp, vp, i32, vp],
    "kp_conv1_forward": [vp] * 5 + [i32] * 3 + [vp, vp],
    "kp_conv1_backward": [vp] * 7 + [i32] * 3 + [vp, i32, vp],
    "kp_colsum_accum": [vp, vp, i64, i64, i32, vp, vp],
    "kp_colsum_jobs": [vp, i32] + [vp] * 7,
    # attention (tests/test_attention_kernels_gpu.py)
    "kp_attention_forward": [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, i64, vp],
    "kp_attention_backward": [vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, vp, vp, vp, i64],
    "kp_attention_forward_dual": [vp, vp, i64, vp, vp, i64, i32, i32, i32, vp, i64, vp, vp],
    "kp_attention_backward_dual": [vp, vp, vp, i64, vp, vp, vp, vp, i32, i32, vp, vp],
    "kp_attention_dual_ok": [i32, i32, vp, vp],
    "kp_attention_dctx": [vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, i32],
    # the fused recurrent-step launchers (tests/test_step_kernels_bf16_gpu.py)
    "kp_small_gates_fwd_hh": _STEP, "kp_small_gates_fwd_h": _STEP, "kp_small_hh": _STEP, "kp_small_h": _STEP,
    "kp_small_gates_bwd_hh": _STEP, "kp_small_gates_bwd_h": _STEP,
    # their exact-fp32 forms (tests/test_kernels_f32_gpu.py, tests/test_step_kernels_f32_gpu.py)
    "kp_big_kk_f32": [vp, vp, i32, i32, i32],
    "kp_small_f32_gates_fwd": _STEP, "kp_small_f32_kk": _STEP, "kp_small_f32_kmn": _STEP, "kp_small_f32_gates_bwd_kk": _STEP,
    "kp_small_f32_gates_bwd": _STEP,
    "kp_gates_elem_bwd": [vp, vp, i32, i32],
    "kp_big_step_store": [vp, vp, i32, i32, vp],
    "kp_big_step_gates_fwd": [vp, vp, i32, i32, vp, sz, vp],
    # loss, sums by token, optimizer, weight shadows, beam search, small elementwise kernels (tests/test_tail_kernels_gpu.py)
    "kp_logsoftmax_nll": [vp, vp, i64, vp, i64, i64, i32, vp, vp, vp, i64, i32, f32],
    "kp_project_loss_ok": [i32, i32, i32],
    "kp_project_loss": [vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, i64, i64, i32, i32, i32, i32, f32],
    "kp_gemm": [vp, i32, vp, i64, i32, vp, i64, i32, vp, i64, i32, i32, i32, vp, vp, i32, vp],
    "kp_sum_to_scalar": [vp, vp, i64, vp],
    "kp_gold_scores": [vp, vp, vp, i32, i32],
    "kp_segsum_supported": [i32, i32, i32],
    "kp_segsum_by_token": [vp, vp, i64, vp, i64, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp, i32, vp, vp],
    "kp_embedding_gather": [vp, vp, vp, i64, i64, vp, i32, i32, i32],
    "kp_embedding_scatter_accum": [vp, vp, vp, i64, i64, vp, i32, i32, i32, i32],
    "kp_cl_err_latch": [], "kp_cl_err_sticky": [],
    "kp_sgd_clip_update": [vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp, i32],
    "kp_adadelta_update": [vp, vp, vp, vp, vp, i64, f32, f32, f32, vp, vp, vp, i32],
    "kp_step_snapshot": [vp, vp, vp, i32, vp],
    "kp_shadow_jobs": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp],
    "kp_beam_select": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i64, vp, vp],
    "kp_project_select": [vp, vp, i64, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp],
    "kp_gather_beam_rows_many": [vp, i32, vp, vp, i64, vp, i32, i32, i32, i32, vp],
    "kp_gather_beam_rows": [vp, vp, i64, vp, i64, vp, i32, i32, i32, i32],
    "kp_token_rows": [vp, vp, vp, i64, vp, i32, i32],
    "kp_beam_backtrace": [vp, vp, vp, vp, vp, vp, i32, i32, i32],
    "kp_recognize_gather": [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32],
    "kp_dec_init": [vp, vp],
    "kp_dpre_tanh": [vp, vp, vp, vp, vp, i64, vp, vp],
    "kp_dropout_apply": [vp, vp, vp, vp, i64, vp],
    "kp_dropout_apply_b": [vp, vp, vp, vp, i64, vp],
    "kp_zero_many": [vp, i32, vp, vp],
    "kp_copy2d_bf16": [vp, vp, i64, vp, i64, i32, i32],
    "kp_edit_distance": [vp, vp, vp, i32, i32, vp, vp],              # wrapped by the shim, called by no test (in no table before this one)
    # the whole-sequence encoder kernels (tests/test_encoder_seq_kernels_gpu.py)
    "kp_enc_seq_supported": [i32, i32],
    "kp_enc_seq_forward": [vp, vp], "kp_enc_seq_backward": [vp, vp], "kp_enc_cluster_forward": [vp, vp], "kp_enc_cluster_backward": [vp, vp],
    "kp_enc_cluster_plan": [i32, i32, i32, i32, vp, vp, vp],
    # the whole-sequence decoder kernels (tests/test_decoder_seq_kernels_gpu.py)
    "kp_dec_cluster_supported": [i32] * 5, "kp_dec_cluster_bwd_supported": [i32] * 5,
    "kp_dec_cluster_forward": [vp, vp], "kp_dec_cluster_backward": [vp, vp],
    # beam search on the chain kernel (the beam tests of tests/test_decoder_seq_kernels_gpu.py)
    "kp_dec_chain_beam_supported": [i32] * 4, "kp_dec_chain_beam_passes": [i32] * 3, "kp_dec_chain_beam_group_cap": [],
    "kp_dec_chain_beam_forward": [vp, vp],
}
_SIZE = {                                                             # return size_t
    "kp_bn_scratch_bytes": [i32],
    "kp_conv1_route_elems": [i32, i32, i32],
    "kp_segsum_index_ints": [i32, i32], "kp_sgd_scratch_bytes": [], "kp_shadow_job_bytes": [],
    "kp_enc_cluster_xbuf_bytes": [i32, i32], "kp_enc_cluster_pbuf_bytes": [i32, i32],
    "kp_dec_cluster_xbuf_bytes": [i32], "kp_dec_cluster_bwd_xbuf_bytes": [i32], "kp_dec_cluster_pbuf_bytes": [i32], "kp_dec_cluster_xtab_bytes": [i32],
}
SIGS = {**{n: (i32, a) for n, a in _INT.items()}, **{n: (sz, a) for n, a in _SIZE.items()}}       # name -> (restype, argtypes)


def kp():
    global _KP
    if _KP is None:
        import aocr  # noqa: F401  (libaocr.so first; the shim resolves against it)
        lib = C.CDLL(os.path.join(ROOT, "tests", "libkprobe.so"))
        for n, (r, a) in SIGS.items():
            getattr(lib, n).argtypes = a
            getattr(lib, n).restype = r
        _KP = lib
    return _KP


def call(name, *args):
    rc = getattr(kp(), name)(C.c_void_p(torch.cuda.current_stream().cuda_stream), *args)
    assert rc == 0, f"{name}: hipGetLastError() = {rc}"


def call_sync(name, *args):
    """call, then wait for the device: what tests/test_tail_kernels_gpu.py's own `call` did.  Kept apart from `call`, which the other files
    follow with a synchronisation of their own where they need one."""
    call(name, *args)
    torch.cuda.synchronize()


def launch(name, args):
    """the wrapper's return value, NOT asserted: tests/test_encoder_seq_kernels_gpu.py's call form (one struct by reference), whose
    wrappers answer with KP_ENC_* refusals that the tests compare."""
    return getattr(kp(), name)(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(args))


@pytest.fixture(autouse=True)
def _switches(monkeypatch, cuda):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("AOCR_TRACE", "1")


def ints(*shape, seed, lo=-4, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


class Buf:
    """A device buffer (from a CPU tensor, or of `shape` filled with `fill`) with SLACK sentinel elements behind it."""

    def __init__(self, t, dtype=torch.float32, fill=None):
        if fill is not None:
            shape = tuple(t)
            n = 1
            for s in shape:
                n *= s
            self.full = torch.full((n + SLACK,), fill, dtype=dtype, device="cuda")
        else:
            shape = tuple(t.shape)
            n = t.numel()
            self.full = torch.empty(n + SLACK, dtype=dtype, device="cuda")
            self.full[:n] = t.reshape(-1).to(dtype).cuda()
        self.tail_val = SENT if dtype.is_floating_point else 0x5A
        self.full[n:] = self.tail_val
        self.n, self.shape, self.dtype = n, shape, dtype
        self.t = self.full[:n].view(shape)

    def ptr(self):
        return C.c_void_p(self.full.data_ptr())

    def cpu(self):
        return self.t.cpu()

    def check_tail(self, what):
        tail = self.full[self.n:].cpu()
        assert torch.equal(tail, torch.full_like(tail, self.tail_val)), f"{what}: write past the end of the buffer"


def bf(t):
    """torch's RNE bf16 image of t, as a bit-comparable int16 tensor."""
    return t.float().to(torch.bfloat16).view(torch.int16)


def bits(buf):
    return buf.cpu().view(torch.int16)


def trace_of(capfd, fn):
    err = capfd.readouterr().err
    return [ln for ln in err.splitlines() if ln.startswith(f"[aocr] {fn}: ")]


def expect(capfd, fn, kernel):
    lines = trace_of(capfd, fn)
    assert lines, f"{fn}: no dispatch trace line (AOCR_TRACE)"
    assert all(f": {kernel}" in ln for ln in lines), (kernel, lines)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def bound(mag, K):
    return BOUND_C * (K ** 0.5) * 2.0 ** -24 * mag


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class Drop(C.Structure):
    _fields_ = [("base", C.c_ulonglong), ("thr", C.c_ulonglong), ("scale", C.c_float), ("off", C.c_longlong)]


class Mat:
    """A [rows][cols] window at column `off` of a device buffer with row stride ld = off + cols + pad (Buf: sentinel tail behind it).
    data: the window's content, the rest is JUNK (an operand); no data: everything is `fill` (an output)."""

    def __init__(self, rows, cols, dtype=torch.float32, data=None, pad=8, off=0, fill=SENT):
        self.rows, self.cols, self.off, self.ld = rows, cols, off, off + cols + pad
        host = torch.full((rows, self.ld), JUNK if data is not None else fill, dtype=torch.float64)
        if data is not None:
            host[:, off:off + cols] = data.double()
        self.buf = Buf(host, dtype)
        self.init = self.buf.cpu().clone()
        self.addr = self.buf.full.data_ptr() + off * self.buf.full.element_size()

    def win(self):
        return self.buf.cpu()[:, self.off:self.off + self.cols]

    def check(self, what):
        """nothing outside the window was written: the padding columns and the tail"""
        self.buf.check_tail(what)
        now = self.buf.cpu().clone()
        now[:, self.off:self.off + self.cols] = self.init[:, self.off:self.off + self.cols]
        assert torch.equal(now.view(torch.int16 if now.dtype == torch.bfloat16 else torch.int32),
                           self.init.view(torch.int16 if now.dtype == torch.bfloat16 else torch.int32)), f"{what}: write outside its columns"


# ---- the flat problem structs of tests/kprobe.hip's recurrent-step wrappers (KpOperand, KpStore, KpGatesFwd, KpGatesBwd), field by field
class Operand(C.Structure):
    _fields_ = [("p0", vp), ("ld0", i64), ("K0", i32), ("p1", vp), ("ld1", i64), ("K1", i32), ("rows", i32)]


class Store(C.Structure):
    _fields_ = [("a", Operand), ("b", Operand), ("C", vp), ("ldc", i64), ("bias", vp), ("bias2", vp), ("flags", i32),
                ("C1", vp), ("ldc1", i64), ("N0", i32), ("Cb", vp), ("ldcb", i64), ("dg", vp), ("dout", vp), ("ldd", i64)]


class GatesFwd(C.Structure):
    _fields_ = [("a", Operand), ("b", Operand), ("zx", vp), ("ldzx", i64), ("b1", vp), ("b2", vp), ("c_prev", vp), ("ldcp", i64),
                ("c_out", vp), ("ldc", i64), ("h_out", vp), ("ldh", i64), ("h_out2", vp), ("ldh2", i64), ("gates", vp), ("ldg", i64),
                ("hb", vp), ("ldhb", i64), ("hb2", vp), ("ldhb2", i64), ("zx_tok", vp), ("zx_tok_stride", i64), ("drop", Drop)]


class GatesBwd(C.Structure):
    _fields_ = [("a", Operand), ("b", Operand), ("dh1", vp), ("ld1", i64), ("dh2", vp), ("ld2", i64), ("dh3", vp), ("ld3", i64),
                ("dc_in", vp), ("lddc", i64), ("gates", vp), ("ldg", i64), ("c_prev", vp), ("ldcp", i64), ("c", vp), ("ldcc", i64),
                ("dz", vp), ("lddz", i64), ("dc_out", vp), ("lddco", i64), ("dzb", vp), ("lddzb", i64), ("drop", Drop), ("gil", i32)]


def operand(t, segs, dtype, vary=0):
    """t [rows][K] as one or two K segments with different row strides -> (Operand, the Mats that own the memory)."""
    o, K0 = Operand(), segs[0]
    m0 = Mat(t.shape[0], K0, dtype, t[:, :K0], pad=8 + 8 * vary, off=8 * vary)
    o.p0, o.ld0, o.K0, o.rows, o.p1, o.ld1, o.K1 = m0.addr, m0.ld, K0, t.shape[0], None, 0, 0
    mats = [m0]
    if len(segs) == 2:
        m1 = Mat(t.shape[0], segs[1], dtype, t[:, K0:], pad=24, off=16)
        o.p1, o.ld1, o.K1 = m1.addr, m1.ld, segs[1]
        mats.append(m1)
    return o, mats


def no_drop():
    return Drop(0, 0, 1.0, 0)


# ---- max-pooling reference of the conv epilogue (EpConv), shared by the bf16 and the exact-fp32 conv files
def pool_ref(z, pool):
    """max-pool of an NCHW map and the kernels' arg-max rule: the FIRST maximum in window order (i = 2 dy + dx; (2,1): i = dy)."""
    B, Cc, H, W = z.shape
    if pool == 1:
        Hp, Wp = H // 2, W // 2
        v = z[:, :, :2 * Hp, :2 * Wp].reshape(B, Cc, Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, Cc, Hp, Wp, 4)
    else:
        Hp = H // 2
        v = z[:, :, :2 * Hp, :].reshape(B, Cc, Hp, 2, W).permute(0, 1, 2, 4, 3)
    m = v.max(dim=-1).values
    first = (v == m.unsqueeze(-1)).float().argmax(dim=-1)          # first index holding the maximum
    return m, first.to(torch.uint8)


def check_exact(res, z, pool, what):
    """z: the exact pre-pool map (NCHW).  y / yb equal the (pooled) map; idx is the first maximum of every window."""
    m, first = (z, None) if pool == 0 else pool_ref(z, pool)
    m = nhwc(m)
    if res["y"] is not None:
        assert torch.equal(res["y"].cpu(), m), f"{what}: y (max diff {(res['y'].cpu() - m).abs().max().item()})"
    if res["yb"] is not None:
        assert torch.equal(bits(res["yb"]), bf(m)), f"{what}: yb"
    if pool:
        bad = res["idx"].cpu() != nhwc(first)
        assert not bad.any(), f"{what}: arg-max not the first maximum of its window at {bad.sum().item()} of {bad.numel()} outputs"


# ---- wide-integer operands of the exact-fp32 files: a bf16 demotion of an operand changes them, small integers (|v| <= 4) would not notice it
WIDE = 300


def wide_ints(*shape, seed):
    """integers in [-300, 300]; every second element (at least) an ODD magnitude in 257..299, which bf16 (8 significand bits) cannot hold"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(-WIDE, WIDE + 1, shape, generator=g)
    odd = (2 * torch.randint(128, 150, shape, generator=g) + 1) * (2 * torch.randint(0, 2, shape, generator=g) - 1)      # +-(257, 259 .. 299)
    n = base.numel()
    pick = (torch.randperm(n, generator=g) < (n + 1) // 2).view(base.shape)          # exactly half of the positions (rounded up)
    t = torch.where(pick, odd, base).float()
    assert 2 * (t != rb(t)).sum().item() >= n, "wide_ints: fewer than half of the values change under a bf16 rounding"
    return t


def assert_exact_range(K, amax, bmax, extra=0.0):
    """every partial sum of K products (plus what the epilogue adds) is an integer below 2^24: fp32 accumulation is exact in ANY order"""
    assert K * amax * bmax + extra < 2 ** 24, f"K {K} x {amax} x {bmax} + {extra} reaches 2^24: fp32 sums are no longer exact"


def out(rows, cols, dtype=torch.float32, pad=8, off=0):
    return Mat(rows, cols, dtype, None, pad, off, SENT if dtype == torch.float32 else -3.0)


def rb(t):
    """round to bf16, as float32"""
    return t.float().to(torch.bfloat16).float()


def ratio(got, ref, tol):
    """largest |got - ref| / tol (tol a number or a tensor)"""
    return ((got.double() - ref).abs() / tol).max().item()


# ---- exact-fp32 EpStore problems, shared by tests/test_kernels_f32_gpu.py (launch_big_kk) and tests/test_step_kernels_f32_gpu.py (launch_small_kk / _kmn)
def eq_bits(got, ref64, what):
    """got (fp32) equals the float64 reference cast to fp32, bit for bit"""
    ref = ref64.float()
    same = torch.equal(got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32))
    assert same, f"{what}: {(got != ref).sum().item()} of {got.numel()} elements differ (max diff {(got.double() - ref64).abs().max().item()})"


def pair(M, N, K, seed, wide_a):
    """A [M][K], B [N][K]: one side wide integers, the other in [-4, 4]"""
    return (wide_ints(M, K, seed=seed), ints(N, K, seed=seed + 1)) if wide_a else (ints(M, K, seed=seed), wide_ints(N, K, seed=seed + 1))


ST_VARIANTS = ("bias", "bias2", "relu", "accum", "tanh", "split")          # (any other name: a plain store)
TQ = 2.0 ** -12                     # the tanh variant's B-side quantum: |x| stays near 1, every product still exact


def store_problem(M, N, segs, variant, seed, wide_a, random=False, b_mn=False):
    """One exact-fp32 EpStore problem as tests/kprobe.hip's KpStore (A [M][K] in one or two K segments; B [N][K] likewise, or with b_mn ONE segment stored
    [K][N]), its output windows and the float64 reference."""
    K = sum(segs)
    if random:
        A, Bm = rnd(M, K, seed=seed).float(), rnd(N, K, seed=seed + 1).float()
    else:
        A, Bm = pair(M, N, K, seed, wide_a)
        assert_exact_range(K, WIDE, 4, 1000)
        if variant == "tanh":
            Bm = Bm * TQ
    p, keep, o = Store(), [], {}
    p.a, ka = operand(A, segs, torch.float32, vary=seed % 2)
    if b_mn:
        mb = Mat(K, N, data=Bm.t(), pad=8, off=4)
        p.b.p0, p.b.ld0, p.b.K0, p.b.rows, kb = mb.addr, mb.ld, K, N, [mb]
    else:
        p.b, kb = operand(Bm, segs, torch.float32, vary=(seed + 1) % 2)
    x, mag = A.double() @ Bm.double().t(), A.double().abs() @ Bm.double().abs().t()
    if variant in ("bias", "bias2", "relu", "accum", "split"):
        b1, b2 = ints(N, seed=seed + 2, lo=-500, hi=500), ints(N, seed=seed + 3, lo=-500, hi=500)
        m1, m2 = Buf(b1), Buf(b2)
        keep += [m1, m2]
        p.bias = m1.full.data_ptr()
        x = x + b1.double()
        if variant in ("bias2", "relu", "split"):
            p.bias2 = m2.full.data_ptr()
            x = x + b2.double()
    if variant == "relu":
        p.flags = EP_RELU
        x = x.clamp(min=0)
    if variant == "tanh":
        p.flags = EP_TANH
        x = torch.tanh(x)
    N0 = N
    if variant == "accum":
        c0 = ints(M, N, seed=seed + 6, lo=-1000, hi=1000)
        o["C"] = Mat(M, N, data=c0, pad=8)
        p.flags = EP_ACCUM
        x = c0.double() + x
    else:
        o["C"] = out(M, N, pad=8)
    if variant == "split":
        N0 = N - 24                                                       # the second destination takes the last 24 columns
        o["C1"] = out(M, N - N0, pad=4, off=4)
        p.C1, p.ldc1, p.N0 = o["C1"].addr, o["C1"].ld, N0
    p.C, p.ldc = o["C"].addr, o["C"].ld
    return p, o, dict(x=x, mag=mag, N0=N0, variant=variant), keep + ka + kb


def store_check(o, ref, K, what, random=False, tanh_tol=1e-5):
    for k, m in o.items():
        m.check(f"{what} {k}")
    x, N0, N = ref["x"], ref["N0"], ref["x"].shape[1]
    got = o["C"].win()
    if random:
        r = ratio(got, x, bound(ref["mag"], K) + 1e-30)
        assert r <= 1.0, f"{what}: error / bound = {r:.3f}"
        return r
    if ref["variant"] == "tanh":                                          # the kernel's own tanh: not exact (tests/test_kernels_bf16_gpu.py: 1e-5)
        e = (got.double() - x).abs().max().item()
        assert e <= tanh_tol, f"{what}: tanh error {e:.2e}"
        return e
    eq_bits(got[:, :N0], x[:, :N0], f"{what}: C")
    if N0 < N:
        assert torch.equal(got[:, N0:], torch.full((got.shape[0], N - N0), SENT)), f"{what}: C written past N0"
        eq_bits(o["C1"].win(), x[:, N0:], f"{what}: C1")
    return 0.0
