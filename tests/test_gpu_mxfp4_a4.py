"""The W4A4 prompt route of MXFP4 models (csrc/mxfp4_a4.hip) on the GPU: the activation quantiser against mxfp4_ref.quantize exactly,
the FP4 x FP4 scaled MFMA's operand map with one-hot rows bit for bit, the GEMM against the exact float64 product of the decoded
operands under mxfp4_ref's matrix-core bar (c = 2 K), the epilogues, three wrong-argument cases.  "mxfp4_a4_errors:" lines
(pytest -s): worst |err| / bar."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_ref as D
import mxfp4_ref as R
from test_gpu_mxfp4 import TORCH, TYPES, _bits, _down, _up, _weight
from test_gpu_mxfp4_a8 import _u8

pytestmark = pytest.mark.gpu


def _quantized(x_bits, t):
    """(codes, scales, decoded float64) of mxfp4_ref.quantize on the values of the bits"""
    xq, xs = R.quantize(D.values(x_bits, t))
    return xq, xs, R.decode(xq, xs)


@pytest.mark.parametrize("t", TYPES)
def test_quantiser_exact(dev, t):
    """three random rows across the type's range and ten constructed blocks, row stride 168: equal scale bytes and decoded elements"""
    from zhilight_amd import ops
    rng = np.random.default_rng(5)
    x = np.zeros((5, 160))
    x[:3] = rng.standard_normal((3, 160)) * np.array([2.0 ** -12, 1.0, 2.0 ** (6 if t == "f16" else 12)])[:, None]
    blk = x[3:].reshape(10, 32)                                # block 0 stays all zero
    blk[1] = rng.uniform(-3.9, 3.9, 32)
    blk[1, 7] = -4.0                                            # amax an exact power of two
    ties = 8 * np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5])
    blk[2, :15] = [48, *ties, *-ties]                           # every tie point under scale 2^3, both signs
    blk[3, :8] = [7.75, 6.5, 7, -7.5, 6.25, 5.5, 5, -0.2]       # (6, 8) saturates at 6; 5 ties to 4; -0.2 rounds to a zero
    blk[4, :6] = np.array([1, 3, 7, 100, 1023, -512]) * 2.0 ** -24            # fp16 subnormals
    blk[5, :6] = np.array([1, 1.5, 0.75, 0.25, 0.125, -1]) * 2.0 ** -126      # bf16: byte clamps to 0, subnormal elements (fp16: zeros)
    bits = D.to_bits(x, t)
    xq, xs = ops.mxfp4_act_quantize(_up(np.pad(bits, ((0, 0), (0, 8))), dev, t)[:, :160])
    want_q, want_s, want = _quantized(bits, t)
    assert np.array_equal(xs.cpu().numpy(), want_s), (xs.cpu().numpy(), want_s)
    bad = np.argwhere(R.decode(xq.cpu().numpy(), want_s) != want)
    assert bad.size == 0, (bad[:5], want[tuple(bad[0])])
    codes = R.unpack_codes(want_q)[3:].reshape(10, 32) & 7      # the reference does what the cases are named for
    assert want_s[3, 2] == 130 and codes[2, 1:8].tolist() == [0, 2, 2, 4, 4, 6, 6] and codes[3, :8].tolist() == [7, 7, 7, 7, 7, 7, 6, 0]
    assert want_s[4, 0] == 0 and (t == "f16" or codes[5, :5].tolist() == [4, 5, 3, 1, 0])


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("k", (160, 4128))
def test_one_hot_rows_bit_exact(dev, t, k):
    """xq row m = the code of 1.0 at column (37 m + 5) % K (both nibbles occur): y[m, n] = 2^(xs - 127) W[n, k_m] exactly -- lane and
    nibble order, both scale paths, op_sel, full super-steps plus a tail; 65 x 80 crosses the row tile and a wave's 64 columns"""
    from zhilight_amd import ops
    m, n, nb = 65, 80, k // 32
    rng = np.random.default_rng(k)
    lo, span, slo, shi = (124, 7, 120, 135) if t == "f16" else (120, 15, 110, 141)
    codes, scales = rng.integers(0, 256, (n, k // 2), dtype=np.uint8), rng.integers(slo, shi, (n, nb)).astype(np.uint8)
    hot = (37 * np.arange(m) + 5) % k
    xq = np.zeros((m, k // 2), np.uint8)
    xq[np.arange(m), hot // 2] = 0x2 << (4 * (hot & 1))
    xs = (lo + (np.arange(m)[:, None] + np.arange(nb)[None, :]) % span).astype(np.uint8)
    want = D.to_bits(np.ldexp(R.decode(codes, scales)[:, hot].T, xs[np.arange(m), hot // 32].astype(np.int64)[:, None] - 127), t)
    got = _bits(ops.mxfp4_a4_linear(_u8(xq, dev), _u8(xs, dev), _weight(codes, scales, dev), TORCH[t]))
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5])


# K below one super-step; past a 64 x 256 tile with byte-gathered scales; two full super-steps; 129 rows, two super-steps + tail
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("mnk", ((33, 48, 128), (65, 272, 160), (100, 128, 1024), (129, 144, 1152)), ids=lambda s: "x".join(map(str, s)))
def test_bars(dev, mnk, t):
    from zhilight_amd import ops
    m, n, k = mnk
    x, codes, scales, _ = R.inputs(1, m, n, k, t)
    xq, xs, a = _quantized(x, t)
    w = R.decode(codes, scales)
    got = _down(ops.mxfp4_a4_linear(_u8(xq, dev), _u8(xs, dev), _weight(codes, scales, dev), TORCH[t]), t)
    ratio = D.worst_ratio(got, a @ w.T, R.bar(a @ w.T, np.abs(a) @ np.abs(w).T, m, k, t), f"mxfp4_a4_linear {mnk} {t}")
    print(f"mxfp4_a4_errors: {t} {m}x{n}x{k}: worst |err| / bar {ratio:.4f}")


@pytest.mark.parametrize("t", TYPES)
def test_epilogues(dev, t):
    """bias + residual with out aliasing the residual, and silu*mul on the row-interleaved weight"""
    from zhilight_amd import ops
    m, n, k = 40, 64, 256
    x, codes, scales, bias = R.inputs(2, m, n, k, t)
    xq, xs, a = _quantized(x, t)
    w, b64 = R.decode(codes, scales), D.values(bias, t)
    inner = a @ w.T + b64[None, :]
    inner_bar = R.bar(inner, np.abs(a) @ np.abs(w).T, m, k, t)
    xqd, xsd = _u8(xq, dev), _u8(xs, dev)
    res = D.to_bits(np.random.default_rng(3).standard_normal((m, n)), t)
    hid = _up(res, dev, t)
    ops.mxfp4_a4_linear(xqd, xsd, _weight(codes, scales, dev), TORCH[t], bias=_up(bias, dev, t), residual=hid, out=hid)
    total, total_bar = R.residual_bar(inner, inner_bar, D.values(res, t), t)
    r_res = D.worst_ratio(_down(hid, t), total, total_bar, f"residual {t}")
    h = n // 2
    bi = _up(np.stack([bias[:h], bias[h:]], axis=1).reshape(-1), dev, t)
    act = ops.mxfp4_a4_linear(xqd, xsd, _weight(codes, scales, dev, row_interleave=True), TORCH[t], bias=bi, epilogue=ops.EPI_SILU_MUL)
    want, want_bar = R.gated_bar(inner[:, :h], inner_bar[:, :h], inner[:, h:], inner_bar[:, h:], t)
    r_act = D.worst_ratio(_down(act, t), want, want_bar, f"silu_mul {t}")
    print(f"mxfp4_a4_errors: epilogues {t}: residual {r_res:.4f} silu_mul {r_act:.4f}")


def test_argument_checks(dev):
    from zhilight_amd import ops
    from zhilight_amd._lib import lib
    w = ops.Mxfp4Weight.from_checkpoint(torch.zeros((16, 48), dtype=torch.uint8, device=dev), torch.full((16, 3), 127, dtype=torch.uint8, device=dev))
    xq, xs = torch.zeros((40, 48), dtype=torch.uint8, device=dev), torch.full((40, 3), 127, dtype=torch.uint8, device=dev)
    y = ops.mxfp4_a4_linear(xq, xs, w, torch.float16)
    assert tuple(y.shape) == (40, 16) and not y.any()
    with pytest.raises(ops.ZLError):                          # K % 32 != 0
        ops.mxfp4_act_quantize(torch.zeros((40, 48), dtype=torch.float16, device=dev))
    with pytest.raises(ops.ZLError, match="xs"):
        ops.mxfp4_a4_linear(xq, xs[:, :2].contiguous(), w, torch.float16)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda xs_p, k: lib().zl_mxfp4_a4_linear(p(xq), xs_p, p(w.codes), p(w.scales), None, None, p(y), C.c_int64(40), C.c_int64(16),  # noqa: E731
                                                    C.c_int64(k), C.c_int(0), C.c_int(0), None)
    assert call(p(xs), 48) == -2 and call(None, 96) == -1    # ZL_ESHAPE, ZL_EINVAL
