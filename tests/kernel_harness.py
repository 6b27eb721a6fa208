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
            # the recurrent-step launchers
            "AOCR_NO_HALF_TILES", "AOCR_HALF_TILES_MAXGRID", "AOCR_NO_STEP_MT2", "AOCR_STEP_MT2_MINK", "AOCR_NO_STEPL", "AOCR_STEPL_MIN_WGS",
            "AOCR_STEP_WAVES4", "AOCR_STEP_WAVES16", "AOCR_BIG_STEP", "AOCR_BIG_STEP_MIN_ROWS",
            # the attention launchers
            "AOCR_NO_ATTN_BF16", "AOCR_ATTN_NW16", "AOCR_NO_ATTN_BEAM_GROUP", "AOCR_ATTN_BWD_TWO_PASS", "AOCR_NO_CHAIN_CTXA",
            # the whole-sequence decoder launchers
            "AOCR_NO_DEC_CHAINS", "AOCR_NO_DEC_CHAINS_BWD", "AOCR_NO_DEC_CHAINS_GREEDY", "AOCR_CH_NO_RES", "AOCR_NO_DEC_EARLY", "AOCR_CL_REMOTE",
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


def out(rows, cols, dtype=torch.float32, pad=8, off=0):
    return Mat(rows, cols, dtype, None, pad, off, SENT if dtype == torch.float32 else -3.0)


def rb(t):
    """round to bf16, as float32"""
    return t.float().to(torch.bfloat16).float()


def ratio(got, ref, tol):
    """largest |got - ref| / tol (tol a number or a tensor)"""
    return ((got.double() - ref).abs() / tol).max().item()
