"""The OCP MXFP8 activation quantiser (zl_mxfp8_quantize, include/zhilight_amd.h) in numpy float64, written apart from the kernel: the
nearest E4M3 value is found by search over the table, not by bit arithmetic.  decode() is exact in float64, so the reference of the
A8 GEMM is decode(xq, xs) @ mxfp4_ref.decode(codes, scales).T under mxfp4_ref's matrix-core bar."""
import numpy as np

import dense_ref as D

BLOCK = 32
# the 127 non-negative E4M3 "fn" values by code: c 2^-9 below code 8, then (1 + m / 8) 2^(e - 7); 126 is 448, 127 the NaN
E4M3 = np.array([c * 2.0 ** -9 if c < 8 else (1 + (c & 7) / 8) * 2.0 ** ((c >> 3) - 7) for c in range(127)])


def quantize(x_bits, t):
    """(M, K) bit patterns of T -> (codes uint8 (M, K), scale bytes uint8 (M, K/32)): byte = clamp(floor(log2(amax)) - 8 + 127, 0, 254),
    0 for an all-zero block; x / 2^(byte - 127) to the nearest table value, ties to the even code, past 448 to 448"""
    x = D.values(x_bits, t)
    m, k = x.shape
    blocks = x.reshape(m, k // BLOCK, BLOCK)
    amax = np.abs(blocks).max(axis=2)
    _, ex = np.frexp(amax)                                    # amax = f 2^ex, f in [0.5, 1)
    byte = np.where(amax > 0, np.clip(ex - 1 - 8 + 127, 0, 254), 0).astype(np.int64)
    a = np.ldexp(np.abs(blocks), (127 - byte)[:, :, None])
    dist = np.abs(a[..., None] - E4M3)                        # at a midpoint both distances are exact, hence equal
    cand = dist == dist.min(axis=-1, keepdims=True)
    even = cand & (np.arange(127) % 2 == 0)
    code = np.where(cand.sum(axis=-1) > 1, even.argmax(axis=-1), cand.argmax(axis=-1))
    code = np.where(np.signbit(blocks), code + 128, code).reshape(m, k)
    return code.astype(np.uint8), byte.astype(np.uint8)


def decode(xq, xs):
    """the exact activations (M, K) in float64"""
    xq = np.asarray(xq, np.uint8)
    v = np.where(xq & 128, -1.0, 1.0) * E4M3[xq & 127]
    return np.ldexp(v, np.repeat(np.asarray(xs, np.int64), BLOCK, axis=1) - 127)
