"""The MXFP8-activation prompt route of MXFP4 models (csrc/mxfp4_a8.hip) on the GPU: the quantiser against tests/mxfp8_ref.py exactly,
the scaled MFMA's operand map with one-hot rows bit for bit, the GEMM against the exact float64 product of the decoded operands under
mxfp4_ref's matrix-core bar (c = 2 K), the epilogues, two wrong-argument cases.  "mxfp4_a8_errors:" lines (pytest -s): worst |err| / bar."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_ref as D
import mxfp4_ref as R
import mxfp8_ref as Q
from test_gpu_mxfp4 import TORCH, TYPES, _down, _up, _weight

pytestmark = pytest.mark.gpu


def _u8(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("t", TYPES)
def test_quantiser_exact(dev, t):
    """three random rows across the type's range and ten constructed blocks, through a row stride of 168: equal scale bytes, equal
    decoded elements (so +0 and -0 are one value)"""
    from zhilight_amd import ops
    rng = np.random.default_rng(5)
    x = np.zeros((5, 160))
    x[:3] = rng.standard_normal((3, 160)) * np.array([2.0 ** -12, 1.0, 2.0 ** (6 if t == "f16" else 12)])[:, None]
    blk = x[3:].reshape(10, 32)                                # block 0 stays all zero
    blk[1] = rng.uniform(-3.9, 3.9, 32)
    blk[1, 7] = -4.0                                            # amax an exact power of two
    blk[2, :12] = [256, 1.0625, 1.1875, -1.0625, 17, 19, -17, 2.0 ** -10, 1.5 * 2.0 ** -9, -2.5 * 2.0 ** -9, 3.5 * 2.0 ** -9, 15.5 * 2.0 ** -9]   # ties
    blk[3, :6] = [511 if t == "f16" else 510, 484, 496, -500, 508, 470]      # 510: the largest bf16 value below 512; (480, 512) -> 448
    blk[4, :8] = [60000, 0.3, 0.1, 0.125, -0.375, 1.0, 0.62, -0.05]           # subnormal codes and flushes under scale 2^7
    blk[5, :6] = np.array([1, 3, 7, 100, 1023, -512]) * 2.0 ** -24            # fp16 subnormals
    bits = D.to_bits(x, t)
    wide = np.zeros((5, 168), np.uint16)
    wide[:, :160] = bits
    xd = _up(wide, dev, t)[:, :160]
    assert xd.stride(0) == 168
    xq, xs = ops.mxfp8_quantize(xd)
    want_q, want_s = Q.quantize(bits, t)
    assert np.array_equal(xs.cpu().numpy(), want_s), (xs.cpu().numpy(), want_s)
    bad = np.argwhere(Q.decode(xq.cpu().numpy(), want_s) != Q.decode(want_q, want_s))
    assert bad.size == 0, (bad[:5], xq.cpu().numpy()[tuple(bad[0])], want_q[tuple(bad[0])])
    assert (want_q[3, 96:101] & 127 == 126).all() and want_s[3, 0] == 0 and (want_q[3, 64 + 4:64 + 8] & 127).tolist() == [88, 90, 88, 0]


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("k", (160, 4128))
def test_one_hot_rows_bit_exact(dev, t, k):
    """xq row m = the code of 1.0 at column (37 m + 5) % K: y[m, n] = 2^(xs - 127) W[n, k_m] exactly -- lane and nibble order of both
    operands, both scale paths and the op_sel byte, a full 128-step plus tail blocks.  fp16: byte ranges that keep every value normal"""
    from zhilight_amd import ops
    m, n, nb = 33, 48, k // 32
    rng = np.random.default_rng(k)
    lo, span, slo, shi = (124, 7, 120, 135) if t == "f16" else (120, 15, 110, 141)
    codes, scales = rng.integers(0, 256, (n, k // 2), dtype=np.uint8), rng.integers(slo, shi, (n, nb)).astype(np.uint8)
    hot = (37 * np.arange(m) + 5) % k
    xq = np.zeros((m, k), np.uint8)
    xq[np.arange(m), hot] = 0x38
    xs = (lo + (np.arange(m)[:, None] + np.arange(nb)[None, :]) % span).astype(np.uint8)
    want = D.to_bits(np.ldexp(R.decode(codes, scales)[:, hot].T, xs[np.arange(m), hot // 32].astype(np.int64)[:, None] - 127), t)
    got = ops.mxfp4_a8_linear(_u8(xq, dev), _u8(xs, dev), _weight(codes, scales, dev), TORCH[t])
    got = got.view(torch.int16).cpu().numpy().view(np.uint16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5])


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("mnk", ((33, 48, 128), (64, 272, 160), (100, 128, 1024), (257, 144, 512)), ids=lambda s: "x".join(map(str, s)))
def test_bars(dev, mnk, t):
    from zhilight_amd import ops
    m, n, k = mnk
    x, codes, scales, _ = R.inputs(1, m, n, k, t)
    xq, xs = Q.quantize(x, t)
    a, w = Q.decode(xq, xs), R.decode(codes, scales)
    got = _down(ops.mxfp4_a8_linear(_u8(xq, dev), _u8(xs, dev), _weight(codes, scales, dev), TORCH[t]), t)
    ratio = D.worst_ratio(got, a @ w.T, R.bar(a @ w.T, np.abs(a) @ np.abs(w).T, m, k, t), f"mxfp4_a8_linear {mnk} {t}")
    print(f"mxfp4_a8_errors: {t} {m}x{n}x{k}: worst |err| / bar {ratio:.4f}")


@pytest.mark.parametrize("t", TYPES)
def test_epilogues(dev, t):
    """bias + residual with out aliasing the residual, and silu*mul on the row-interleaved weight, against the stated arithmetic"""
    from zhilight_amd import ops
    m, n, k = 40, 64, 256
    x, codes, scales, bias = R.inputs(2, m, n, k, t)
    xq, xs = Q.quantize(x, t)
    a, w, b64 = Q.decode(xq, xs), R.decode(codes, scales), D.values(bias, t)
    inner = a @ w.T + b64[None, :]
    inner_bar = R.bar(inner, np.abs(a) @ np.abs(w).T, m, k, t)
    xqd, xsd = _u8(xq, dev), _u8(xs, dev)
    res = D.to_bits(np.random.default_rng(3).standard_normal((m, n)), t)
    hid = _up(res, dev, t)
    out = ops.mxfp4_a8_linear(xqd, xsd, _weight(codes, scales, dev), TORCH[t], bias=_up(bias, dev, t), residual=hid, out=hid)
    assert out.data_ptr() == hid.data_ptr()
    total, total_bar = R.residual_bar(inner, inner_bar, D.values(res, t), t)
    r_res = D.worst_ratio(_down(hid, t), total, total_bar, f"residual {t}")
    h = n // 2
    bi = _up(np.stack([bias[:h], bias[h:]], axis=1).reshape(-1), dev, t)
    act = ops.mxfp4_a8_linear(xqd, xsd, _weight(codes, scales, dev, row_interleave=True), TORCH[t], bias=bi, epilogue=ops.EPI_SILU_MUL)
    assert tuple(act.shape) == (m, h)
    want, want_bar = R.gated_bar(inner[:, :h], inner_bar[:, :h], inner[:, h:], inner_bar[:, h:], t)
    r_act = D.worst_ratio(_down(act, t), want, want_bar, f"silu_mul {t}")
    print(f"mxfp4_a8_errors: epilogues {t}: residual {r_res:.4f} silu_mul {r_act:.4f}")


def test_argument_checks(dev):
    from zhilight_amd import ops
    from zhilight_amd._lib import lib
    w = ops.Mxfp4Weight.from_checkpoint(torch.zeros((16, 48), dtype=torch.uint8, device=dev), torch.full((16, 3), 127, dtype=torch.uint8, device=dev))
    xq, xs = torch.zeros((40, 96), dtype=torch.uint8, device=dev), torch.full((40, 3), 127, dtype=torch.uint8, device=dev)
    y = ops.mxfp4_a8_linear(xq, xs, w, torch.float16)
    assert tuple(y.shape) == (40, 16) and not y.any()
    with pytest.raises(ops.ZLError):                          # K % 32 != 0
        ops.mxfp8_quantize(torch.zeros((40, 48), dtype=torch.float16, device=dev))
    with pytest.raises(ops.ZLError, match="xs"):
        ops.mxfp4_a8_linear(xq, xs[:, :2].contiguous(), w, torch.float16)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda xs_p, k: lib().zl_mxfp4_a8_linear(p(xq), xs_p, p(w.codes), p(w.scales), None, None, p(y), C.c_int64(40), C.c_int64(16),  # noqa: E731
                                                    C.c_int64(k), C.c_int(0), C.c_int(0), None)
    assert call(p(xs), 48) == -2 and call(None, 96) == -1    # ZL_ESHAPE, ZL_EINVAL
