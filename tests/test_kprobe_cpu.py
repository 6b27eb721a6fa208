"""CPU: the kernel-test shim (tests/kprobe.hip) still matches csrc/ops.h.  The shim is compiled here and every aocr:: symbol it
leaves undefined must be defined by libaocr.so -- a launcher whose signature changed in ops.h without the library being rebuilt,
or a wrapper calling a signature that no longer exists, fails here instead of as a load error on the GPU box."""
import os
import shutil
import subprocess

import pytest

from kernel_harness import SIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch-attention-ocr_amd", "csrc")
LIB = os.path.join(ROOT, "torch-attention-ocr_amd", "aocr", "libaocr.so")


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def _symbols(path, *flags):
    out = subprocess.run(["nm", "-D", *flags, path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_kprobe_symbols_resolve_in_libaocr(tmp_path):
    hipcc = _hipcc()
    if hipcc is None or shutil.which("nm") is None:
        pytest.skip("no hipcc / nm on this machine")
    assert os.path.exists(LIB), "libaocr.so not built (run __graft_entry__.build())"
    so = str(tmp_path / "libkprobe.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "kprobe.hip"), "-o", so,
                    "-L" + os.path.dirname(LIB), "-laocr"], check=True, capture_output=True)
    undef = _symbols(so, "--undefined-only")
    wanted = {s for s in undef if s.startswith("_ZN4aocr")}
    # every launcher the shim wraps is reached through a mangled aocr:: reference
    for name in ("conv_forward", "conv_backward_data", "conv_backward_filter", "conv_weight_shadows", "splitk_reduce", "gemm_hh",
                 "gemm_hh_shadow", "gemm_hh_cat", "grouped_wgrad", "bn_relu_forward",
                 "launch_small_gates_fwd_hh", "launch_small_gates_fwd_h", "launch_small_hh", "launch_small_h", "launch_small_gates_bwd_hh",
                 "launch_small_gates_bwd_h", "gates_elem_bwd", "big_step_store", "big_step_gates_fwd",
                 "conv_weight_transpose_f32", "launch_big_kk", "launch_small_gates_fwd", "launch_small_kk", "launch_small_kmn",
                 "launch_small_gates_bwd_kk", "launch_small_gates_bwd", "gemm",
                 "attention_forward", "attention_backward", "attention_forward_dual", "attention_backward_dual", "attention_dual_ok",
                 "attention_dctx", "bn_relu_backward", "unpool_relu_backward", "conv1_forward", "conv1_route_elems", "conv1_backward",
                 "colsum_accum", "colsum_defer", "colsum_flush",
                 "logsoftmax_nll", "project_loss", "project_loss_ok", "segsum_by_token", "segsum_supported", "segsum_index_ints", "embedding_gather",
                 "embedding_scatter_accum", "sgd_clip_update", "sgd_scratch_bytes", "adadelta_update", "step_snapshot", "shadow_jobs", "beam_select",
                 "project_select", "gather_beam_rows_many", "gather_beam_rows", "token_rows", "beam_backtrace", "recognize_gather", "dec_init",
                 "dpre_tanh", "dropout_apply", "dropout_apply_b", "zero_many", "copy2d_bf16", "sum_to_scalar", "gold_scores", "edit_distance",
                 "enc_seq_supported", "enc_seq_forward", "enc_seq_backward", "enc_cluster_plan", "enc_cluster_xbuf_bytes", "enc_cluster_pbuf_bytes",
                 "enc_cluster_forward", "enc_cluster_backward",
                 "dec_cluster_supported", "dec_cluster_bwd_supported", "dec_cluster_xbuf_bytes", "dec_cluster_bwd_xbuf_bytes", "dec_cluster_pbuf_bytes",
                 "dec_cluster_xtab_bytes", "dec_cluster_forward", "dec_cluster_backward",
                 "dec_chain_beam_supported", "dec_chain_beam_passes", "dec_chain_beam_group_cap", "dec_chain_beam_forward"):
        assert any(f"{len(name)}{name}E" in s for s in wanted), f"the shim does not call aocr::{name}"
    defined = _symbols(LIB, "--defined-only")
    missing = sorted(wanted - defined)
    assert not missing, f"aocr:: symbols the shim needs but libaocr.so does not define (ops.h signature drift?): {missing}"
    exported = _symbols(so, "--defined-only")
    for name in ("kp_conv_forward", "kp_conv_backward_data", "kp_conv_backward_filter", "kp_grouped_wgrad", "kp_gemm_hh_cat",
                 "kp_small_gates_fwd_hh", "kp_small_gates_fwd_h", "kp_small_hh", "kp_small_h", "kp_small_gates_bwd_hh", "kp_small_gates_bwd_h",
                 "kp_gates_elem_bwd", "kp_big_step_store", "kp_big_step_gates_fwd",
                 "kp_conv_weight_transpose_f32", "kp_conv_backward_data_f32", "kp_big_kk_f32", "kp_small_f32_gates_fwd", "kp_small_f32_kk",
                 "kp_small_f32_kmn", "kp_small_f32_gates_bwd_kk", "kp_small_f32_gates_bwd",
                 "kp_attention_forward", "kp_attention_backward", "kp_attention_forward_dual", "kp_attention_backward_dual",
                 "kp_attention_dual_ok", "kp_attention_dctx", "kp_bn_relu_forward2", "kp_bn_relu_backward", "kp_unpool_relu_backward",
                 "kp_conv1_forward", "kp_conv1_route_elems", "kp_conv1_backward", "kp_colsum_accum", "kp_colsum_jobs",
                 "kp_logsoftmax_nll", "kp_project_loss", "kp_project_loss_ok", "kp_gemm", "kp_segsum_by_token", "kp_segsum_supported",
                 "kp_segsum_index_ints", "kp_embedding_gather", "kp_embedding_scatter_accum", "kp_sgd_clip_update", "kp_sgd_scratch_bytes",
                 "kp_adadelta_update", "kp_step_snapshot", "kp_shadow_jobs", "kp_beam_select", "kp_project_select", "kp_gather_beam_rows_many",
                 "kp_gather_beam_rows", "kp_token_rows", "kp_beam_backtrace", "kp_recognize_gather", "kp_dec_init", "kp_dpre_tanh",
                 "kp_dropout_apply", "kp_dropout_apply_b", "kp_zero_many", "kp_copy2d_bf16", "kp_sum_to_scalar", "kp_gold_scores",
                 "kp_enc_seq_supported", "kp_enc_seq_forward", "kp_enc_seq_backward", "kp_enc_cluster_plan", "kp_enc_cluster_xbuf_bytes",
                 "kp_enc_cluster_pbuf_bytes", "kp_enc_cluster_forward", "kp_enc_cluster_backward",
                 "kp_dec_cluster_supported", "kp_dec_cluster_bwd_supported", "kp_dec_cluster_xbuf_bytes", "kp_dec_cluster_bwd_xbuf_bytes",
                 "kp_dec_cluster_pbuf_bytes", "kp_dec_cluster_xtab_bytes", "kp_dec_cluster_forward", "kp_dec_cluster_backward",
                 "kp_dec_chain_beam_supported", "kp_dec_chain_beam_passes", "kp_dec_chain_beam_group_cap", "kp_dec_chain_beam_forward"):
        assert name in exported
    unexported = sorted(set(SIGS) - exported)
    assert not unexported, f"in kernel_harness.SIGS, not exported by the compiled shim: {unexported}"
