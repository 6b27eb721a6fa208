"""CPU: BOUND_C of tests/kernel_harness.py against fp32 operands.  The random cases of tests/test_kernels_f32_gpu.py and
tests/test_step_kernels_f32_gpu.py hold a kernel's error against float64 to bound = BOUND_C sqrt(K) 2^-24 sum |a_k b_k|.  The constant was
argued for bf16 operands (exact products); with fp32 operands every product is rounded too.  Here: a numpy float32 restatement of ONE
sequential fused-multiply-add chain (acc <- fl32(a_k b_k + acc): the product of two floats is exact in float64, the sum is rounded once to
float64 and once to float32 -- a double rounding that differs from a true FMA in far fewer cases than the bound's slack), at the K of the
GPU cases, on the operand distributions of those cases.  A kernel's order (MFMA chains of K / 2 .. K / 16 terms, then a few adds) has
shorter chains than this one, so the sequential chain is the pessimistic order.  The worst ratio error / (sqrt(K) 2^-24 sum |a b|) must stay
below BOUND_C / 2 = 2; measured 0.50 at K = 40, 0.45 at K = 32 and less at every other K below (printed): an eighth of the bound, so
BOUND_C = 4 stands and is not stretched."""
import numpy as np
import pytest

from kernel_harness import BOUND_C

KS = (32, 40, 64, 72, 128, 144, 200, 288, 512, 777, 2048)      # every K of the random cases, and the largest of the exact ones


def fma_chain_f32(a, b):
    """rows of a, b (float32, [n][K]) -> the sequential fp32 chain of every row"""
    acc = np.zeros(a.shape[0], dtype=np.float32)
    for k in range(a.shape[1]):
        acc = (a[:, k].astype(np.float64) * b[:, k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


@pytest.mark.parametrize("K", KS)
def test_bound_c_covers_a_sequential_fp32_chain(K):
    rng = np.random.default_rng(1234 + K)
    n = 4096
    worst = 0.0
    for scale_b in (1.0, 1.0 / np.sqrt(K)):                     # uniform operands, and weights scaled as the conv / gate cases scale them
        a = rng.uniform(-1, 1, (n, K)).astype(np.float32)
        b = (rng.uniform(-1, 1, (n, K)) * scale_b).astype(np.float32)
        exact = (a.astype(np.float64) * b.astype(np.float64)).sum(axis=1)
        mag = np.abs(a.astype(np.float64) * b.astype(np.float64)).sum(axis=1)
        ratio = np.abs(fma_chain_f32(a, b).astype(np.float64) - exact) / (np.sqrt(K) * 2.0 ** -24 * mag)
        worst = max(worst, float(ratio.max()))
    print(f"[f32-bound] K = {K}: worst error / (sqrt(K) 2^-24 sum |a b|) = {worst:.3f} (BOUND_C = {BOUND_C})")
    assert worst <= 0.5 * BOUND_C
