"""The exact reference and the per-element error bars for the dense GEMV / GEMM family (zhilight_amd/csrc/dense_gemv.hip,
dense_gemm.hip): numpy and float64 only, no GPU.  tests/test_dense_ref_host.py shows that the bars admit an honest kernel and reject
a subtly wrong one; tests/test_gpu_dense.py holds the kernels to them.

Reference: oracle.gemm_nt_exact_blas on inputs that are already values of T (fp16 / bf16 bit patterns), so every product
x[r, i] * w[c, i] is exact in float64 and the float64 sum is off by ~k * 2^-53 of S -- nothing next to the bars below.

Bars, all per element, |got - exact| <= bar, with
    u_T      = 2^-11 (fp16), 2^-8 (bf16): half an ulp of T relative to the value
    S[r, c]  = sum_i |x[r, i] * w[c, i]| in float64
    exact    = alpha * (x . w^T) + bias

  outputs rounded to T:   1.01 * u_T * |exact| + c * 2^-24 * |alpha| * S + tiny
      The first term is the one rounding to T (1 % on top because the kernel rounds its own fp32 value, not the exact one); the second
      is the fp32 accumulation: a sum in which no term passes through more than c fp32 roundings is off by at most
      ((1 + 2^-24)^c - 1) * S ~ c * 2^-24 * S; tiny is half the spacing of T's subnormals, where the error of the rounding is
      absolute.
  fp32 outputs:           c * 2^-24 * |alpha| * S                                       (nothing is rounded to T)
  fused final norm:       the exact product on oracle.rmsnorm(x) (the bit-level normalisation) and u_T * |alpha| * S more: the
                          kernel's block-wide sum of squares associates differently from the oracle's, which may flip the last bit
                          of a normalised element.

c is DERIVED from the kernels' summation order, not measured:
  GEMV (k_dense_gemv): one lane's chain is 8 fused multiply-adds per 512-k wave-load, ceil(k / 512) loads, then the 6 adds of the
      64-lane butterfly, then alpha and bias: 8 * ceil(k / 512) + 6 + 2.  Doubled, because the rounding inside fp16 v_dot2_f32_f16
      (two products and the accumulator in one instruction) is not documented.
  fp32 router GEMM (k_gemm_nt_f32): the same chain, NOT doubled: the kernel has the GEMV's order but only fmaf for both types, one
      IEEE rounding per step, so there is nothing undocumented to allow for (its own chain is 8 * ceil(k / 512) + 6 + 1: no bias).
  matrix-core GEMM (k_dense_gemm): 2 * k -- k roundings is the worst case of ANY summation order of k products, doubled for the MFMA's
      undocumented internal rounding.
"""
import numpy as np

import glue_ref as G
import zl_oracle

U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY = {"f16": 2.0 ** -25, "bf16": 2.0 ** -134}            # half the smallest subnormal of T
DT = {"f16": 0, "bf16": 1}                                   # the oracle's dtype argument
F32_EPS = 2.0 ** -24
DEFAULT_CUS = 256                                            # MI355X: what the host test assumes for the launch geometry


def to_bits(x64, t):
    """float64 -> bit patterns of T (one rounding): the inputs of every test are values of T"""
    return G.round_to(np.asarray(x64, np.float64), t)


def values(bits, t):
    return G.bits_to_f64(bits, t)


def inputs(seed, m, n, k, t, w_scale=0.05, bias=True):
    """x ~ N(0, 1), w ~ w_scale * N(0, 1), bias ~ N(0, 1) from numpy.random.default_rng(seed), in this order, rounded to T"""
    rng = np.random.default_rng(seed)
    x = to_bits(rng.standard_normal((m, k)), t)
    w = to_bits(w_scale * rng.standard_normal((n, k)), t)
    b = to_bits(rng.standard_normal(n), t) if bias else None
    return x, w, b


def exact(x, w, t, bias=None, alpha=1.0):
    """alpha * (x . w^T) + bias in float64; x, w, bias are bit patterns of T"""
    with np.errstate(invalid="ignore", over="ignore"):
        y = float(alpha) * zl_oracle.gemm_nt_exact_blas(x, w, None, DT[t])
        if bias is not None:
            y = y + values(bias, t)[None, :]
    return y


def abs_sum(x, w, t):
    """S[r, c] = sum_i |x[r, i] * w[c, i]|"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(values(x, t)) @ np.abs(values(w, t)).T


def gemv_chain(k):
    """longest fp32 chain of the wave-per-row kernels, doubled (see the module docstring)"""
    return 2 * (8 * ((k + 511) // 512) + 6 + 2)


def f32_chain(k):
    """k_gemm_nt_f32: the GEMV's chain without the doubling (fmaf only)"""
    return 8 * ((k + 511) // 512) + 6 + 2


def mfma_chain(k):
    return 2 * k


def bar_rounded(exact_v, s, alpha, c, t):
    with np.errstate(invalid="ignore"):
        return 1.01 * U[t] * np.abs(exact_v) + c * F32_EPS * abs(float(alpha)) * s + TINY[t]


def bar_f32(s, alpha, c):
    return c * F32_EPS * abs(float(alpha)) * s


def bar_norm(exact_v, s, alpha, c, t):
    """s: S on the normalised activations"""
    return bar_rounded(exact_v, s, alpha, c, t) + U[t] * abs(float(alpha)) * s


def worst_ratio(got, exact_v, bar, what):
    """max |got - exact| / bar over the finite reference values; where the reference is a NaN or an infinity the
    output has to be that (any NaN for a NaN).  Raises AssertionError naming the worst element when a value is out of its bar."""
    got, exact_v, bar = (np.asarray(a, np.float64) for a in (got, exact_v, bar))
    assert got.shape == exact_v.shape == bar.shape, (what, got.shape, exact_v.shape, bar.shape)
    fin = np.isfinite(exact_v)
    with np.errstate(invalid="ignore"):
        bad = np.where(np.isnan(exact_v), ~np.isnan(got), got != exact_v) & ~fin
    assert not bad.any(), f"{what}: {int(bad.sum())} non-finite reference values not reproduced, first at {tuple(np.argwhere(bad)[0])}"
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(fin, np.abs(got - exact_v), 0.0)
        ratio = np.where(fin & (err != 0.0), err / bar, 0.0)  # an exact output is inside any bar, a bar of 0 (S = 0) included
    ratio = np.where(np.isnan(ratio), np.inf, ratio)          # a NaN / inf output where the reference is finite
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio[i] <= 1.0, (f"{what}: {int((ratio > 1).sum())} of {ratio.size} elements out of their bar; worst at {tuple(int(v) for v in i)}: "
                             f"got {got[i]!r} exact {exact_v[i]!r} |err| {err[i]:.3e} bar {bar[i]:.3e} ratio {ratio[i]:.3f}")
    return float(ratio[i])


# ---- the launcher's decisions, restated (dense_gemv.hip: dense_waves, gemm_nt_small_m_impl, launch) -------------------------------------
def gemv_geometry(m, n, k, cus=DEFAULT_CUS):
    waves = 8 * cus
    rows_per_wave = (n + waves - 1) // waves
    loads_per_row = (k + 511) // 512
    kp = loads_per_row * 512
    mt = min(m, 4)
    while mt > 1 and mt * kp * 2 + 64 > 64 * 1024:
        mt -= 1
    if mt == 3:
        mt = 2
    return dict(rows_per_wave=rows_per_wave, loads_per_row=loads_per_row, loads_per_wave=rows_per_wave * loads_per_row, mt=mt,
                row_blocks=(m + mt - 1) // mt, lds_bytes=mt * kp * 2 + 64,
                total_waves=((n + rows_per_wave - 1) // rows_per_wave + 3) // 4 * 4)


# ---- the shapes of tests/test_gpu_dense.py, (m, n, k) per family; test_dense_ref_host.py runs its emulations and mutations on the same --
def gemv_shapes(cus=DEFAULT_CUS):
    w = 8 * cus
    return {
        "rows_per_wave": [(m, 2 * w + 3, 1536) for m in (1, 2, 4)],     # several rows per wave, the ring refills across a row boundary
        "ring_in_row": [(3, 300, 5000), (5, 300, 5000)],                # 10 loads per row, the last one partial; mt = 2 with a dead row
        "lds": [(4, 96, 8192), (4, 96, 16384), (2, 96, 53248)],         # mt 4 -> 2, mt -> 1, more than 64 KiB of dynamic LDS
        "tiny": [(m, n, k) for k in (8, 72) for n in (1, 3) for m in (1, 4)],
        "strided": [(3, 131, 1096)],                                    # ldx = k + 64, bias, alpha = 0.5, out=; plain and with the norm
        "norm_edge": [(4, 131, 1096)],                                  # an all-zero row, rows of very different scale in one block
    }


GEMM_M = (15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
GEMM_N = (1, 15, 127, 128, 129)
GEMM_K = (384, 640, 1152)                                               # 3, 5 and 9 chunks of 128: every one an odd count
F32_SHAPES = ((1, 128, 2048), (64, 128, 2048), (64, 256, 7168), (64, 128, 72), (64, 60, 4096), (3, 1, 8))
# (shape, seed, top-k) of the routing check and the tokens the reference alone gives up on (a near-tie among its own top k + 1)
ROUTING = (((64, 128, 2048), 1, 8), ((64, 256, 7168), 2, 8), ((64, 128, 72), 3, 8), ((64, 60, 4096), 4, 4))
ROUTING_MAX_SKIPPED = 10
ROUTING_SKIPPED_F16 = (2, 5, 0, 0)                                      # near-ties of the exact fp16 logits: pins how the inputs are drawn


def routing_inputs(shape, seed, t):
    m, n, k = shape
    rng = np.random.default_rng(seed)
    x = to_bits(rng.standard_normal((m, k)), t)
    w = to_bits(0.05 * rng.standard_normal((n, k)), t)
    return x, w


def routing_skipped(exact_logits, top_k, max_bar):
    """tokens whose ranked top-k the bar cannot decide: among the top k + 1 exact logits some adjacent gap is at most 2 * max_bar"""
    top = -np.sort(-np.asarray(exact_logits, np.float64), axis=1)[:, :top_k + 1]
    return ((top[:, :-1] - top[:, 1:]) <= 2.0 * max_bar).any(axis=1)


def ranked_top_k(logits, top_k):
    """ids of the top_k largest logits per row, largest first, the lower index first among equals"""
    return np.argsort(-np.asarray(logits, np.float64), axis=1, kind="stable")[:, :top_k]


def first_argmax(logits64):
    """zl_argmax_advance's rule per row: the first index of the largest value, a NaN counting as the largest"""
    logits64 = np.asarray(logits64, np.float64)
    nan = np.isnan(logits64)
    return np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, logits64).argmax(axis=1))
