"""The exact reference and the per-element error bars for the MXFP4 linears (zhilight_amd/csrc/mxfp4.hip): numpy and float64 only,
no GPU.  tests/test_mxfp4_host.py shows that the bars admit an honest kernel and reject subtly wrong ones; tests/test_gpu_mxfp4.py
holds the kernels to them.

Format (include/zhilight_amd.h "MXFP4"): codes uint8 (N, K/2), element 2j in bits 0-3 of byte j, 2j + 1 in bits 4-7;
value(c) = (-1)^(c >> 3) * {0, .5, 1, 1.5, 2, 3, 4, 6}[c & 7], code 8 is 0; scales uint8 (N, K/32); W = value * 2^(scale - 127).

Reference: float64 x . W^T on the EXACTLY dequantised weight -- W has at most 2 significant bits and x is a value of T, so every
product is exact in float64 and the float64 sum is off by ~k 2^-53 of S, nothing next to the bars.

Bars (tests/dense_ref.py: bar_rounded, worst_ratio), per element:  |got - exact| <= 1.01 u_T |exact| + c 2^-24 S + tiny,
S = sum_k |x w|.  c is DERIVED from each kernel's summation order:
  GEMV (k_mxfp4_gemv): a lane sums a block's 32 products with 32 fused multiply-adds (v_fma_mix / v_fma: IEEE, one rounding each),
      scales the partial by a power of two and adds it to its accumulator in ONE fma per block, ceil(K / 32 / 64) blocks per lane;
      then the 6 adds of the 64-lane butterfly and the bias: 32 + ceil(K / 2048) + 6 + 2.
  matrix-core kernels (k_mxfp4_stream, k_mxfp4_tiled): 2 K -- K roundings is the worst case of ANY summation order of K products,
      doubled for the MFMA's undocumented internal rounding.  It is the ceiling and needs no measurement.
"""
import numpy as np

import dense_ref as D

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
VALUE = np.concatenate([E2M1, -E2M1])
VALUE[8] = 0.0                                                # code 8 ("-0") is 0
BLOCK = 32
GEMV, STREAM, TILED = 1, 2, 3


def unpack_codes(codes):
    """(N, K/2) bytes -> (N, K) codes 0..15"""
    codes = np.asarray(codes, np.uint8)
    out = np.empty((codes.shape[0], codes.shape[1] * 2), np.uint8)
    out[:, 0::2] = codes & 15
    out[:, 1::2] = codes >> 4
    return out


def pack_codes(c):
    c = np.asarray(c, np.uint8)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def decode(codes, scales):
    """the exact weight (N, K) in float64"""
    c = unpack_codes(codes)
    e = np.repeat(np.asarray(scales, np.int64), BLOCK, axis=1) - 127
    return np.ldexp(VALUE[c], e)


def quantize(w64):
    """OCP MX rule on float64 (N, K): block exponent floor(log2(amax)) - 2, all-zero block -> byte 0; nearest E2M1 value, ties to the
    even code, saturating at 6.  Written apart from ops.mxfp4_quantize (search over the table instead of thresholds)."""
    w64 = np.asarray(w64, np.float64)
    n, k = w64.shape
    blocks = w64.reshape(n, k // BLOCK, BLOCK)
    amax = np.abs(blocks).max(axis=2)
    _, ex = np.frexp(amax)                                    # amax = m 2^ex, m in [0.5, 1)
    byte = np.where(amax > 0, np.clip(ex - 1 - 2 + 127, 0, 254), 0).astype(np.int64)
    a = np.ldexp(np.abs(blocks), (127 - byte)[:, :, None])
    dist = np.abs(a[..., None] - E2M1)                        # (n, nb, 32, 8); at a midpoint both distances are exact, hence equal
    best = dist.min(axis=-1, keepdims=True)
    cand = dist == best                                       # one or two neighbours; of two, take the even code
    even = cand & (np.arange(8) % 2 == 0)
    code = np.where(cand.sum(axis=-1) > 1, even.argmax(axis=-1), cand.argmax(axis=-1))
    code = np.where((blocks < 0) & (code > 0), code + 8, code).reshape(n, k)
    return pack_codes(code), byte.astype(np.uint8)


def inputs(seed, m, n, k, t, w_scale=0.05):
    """x ~ N(0, 1) rounded to T, w = quantise(w_scale N(0, 1)), bias ~ N(0, 1) rounded to T, from default_rng(seed) in this order"""
    rng = np.random.default_rng(seed)
    x = D.to_bits(rng.standard_normal((m, k)), t)
    codes, scales = quantize(w_scale * rng.standard_normal((n, k)))
    bias = D.to_bits(rng.standard_normal(n), t)
    return x, codes, scales, bias


def small_scale_inputs(seed, m, n, k):
    """the fp16 no-weight-rounding case: every scale byte 103 (2^-24, below fp16's normal range: a weight rounded to fp16 loses
    bits or vanishes), x ~ N(0, 1) 2^10"""
    rng = np.random.default_rng(seed)
    x = D.to_bits(rng.standard_normal((m, k)) * 1024.0, "f16")
    codes = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
    scales = np.full((n, k // BLOCK), 103, np.uint8)
    return x, codes, scales


def exact(x, codes, scales, t):
    return D.values(x, t) @ decode(codes, scales).T


def abs_sum(x, codes, scales, t):
    return np.abs(D.values(x, t)) @ np.abs(decode(codes, scales)).T


def route(m):
    return GEMV if m <= 4 else STREAM if m <= 32 else TILED


def chain(m, k):
    """c of the kernel that takes m rows (see the module docstring)"""
    if route(m) == GEMV:
        return 32 + (k // BLOCK + 63) // 64 + 6 + 2
    return 2 * k


def bar(exact_v, s, m, k, t):
    return D.bar_rounded(exact_v, s, 1.0, chain(m, k), t)


# ---- what a kernel may and may not do, in numpy fp32 ----------------------------------------------------------------------------
def emulate(x, codes, scales, t, variant="honest", seed=0):
    """A kernel of the family's structure in fp32: each block's 32 products summed sequentially in a PERMUTED order, the partial
    scaled by the block's power of two, partials added block after block, one rounding to T.  Variants are the mistakes the bars must
    catch: "nibbles" (the two codes of a byte swapped), "scale_shift" (block b scaled with block b + 1's byte), "round_w" (fp16: the
    scaled weight rounded to fp16 before the product)."""
    xv = D.values(x, t).astype(np.float32)
    c = unpack_codes(codes)
    if variant == "nibbles":
        c = c.reshape(c.shape[0], -1, 2)[:, :, ::-1].reshape(c.shape[0], -1)
    sc = np.asarray(scales, np.int64)
    if variant == "scale_shift":
        sc = np.roll(sc, -1, axis=1)
    n, k = c.shape
    nb = k // BLOCK
    perm = np.random.default_rng(seed).permutation(BLOCK)
    acc = np.zeros((xv.shape[0], n), np.float32)
    if variant == "round_w":
        w = D.values(D.to_bits(np.ldexp(VALUE[c], np.repeat(sc, BLOCK, axis=1) - 127), "f16"), "f16").astype(np.float32)
        f = np.ones((n, nb), np.float32)
    else:
        w = VALUE[c].astype(np.float32)
        f = np.ldexp(np.float32(1.0), (sc - 127).astype(np.int32)).astype(np.float32)
    for b in range(nb):
        part = np.zeros_like(acc)
        for i in perm:
            part = (part + xv[:, None, b * BLOCK + i] * w[None, :, b * BLOCK + i]).astype(np.float32)   # exact product, one rounding
        acc = (acc + part * f[None, :, b]).astype(np.float32)
    return D.values(D.to_bits(acc.astype(np.float64), t), t)


# ---- epilogues: bounds against the UNROUNDED arithmetic (include/zhilight_amd.h, zl_w4a16_gemm's epilogue list with half = T) --------
def rounded(v64, t):
    return D.values(D.to_bits(v64, t), t)


def residual_bar(inner_exact, inner_bar, residual64, t):
    """y = T(residual + T(acc + bias)): the inner value is within inner_bar of inner_exact (its own rounding included), the outer sum
    is exact in fp32 up to one rounding (2^-24) and rounded once more to T"""
    total = residual64 + inner_exact
    return total, inner_bar + (1.01 * D.U[t] + 2.0 ** -23) * np.abs(total) + D.TINY[t]


def silu64(g):
    return g / (1.0 + np.exp(-g))


def gated_bar(g_exact, g_bar, u_exact, u_bar, t):
    """out = T(silu(T(g)) T(u)) in fp32: |silu'| <= 1.1, expf / divide / multiply of fp32 within 8 ulp together"""
    out = silu64(g_exact) * u_exact
    err = 1.1 * g_bar * (np.abs(u_exact) + u_bar) + np.abs(silu64(g_exact)) * u_bar
    return out, err + (1.01 * D.U[t] + 8 * 2.0 ** -23) * (np.abs(out) + err) + D.TINY[t]
