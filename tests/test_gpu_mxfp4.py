"""The MXFP4 kernels (csrc/mxfp4.hip) on the GPU: the dequantiser bit for bit, the layout of every route with one-hot rows (no
tolerance), every route against the exact float64 product with the per-element bars of tests/mxfp4_ref.py (shown on the CPU to admit an
honest kernel and reject wrong ones by tests/test_mxfp4_host.py), the epilogues, strides and aliasing, and the fp16 case in which a
rounded weight would be wrong.  Lines starting "mxfp4_errors:" (pytest -s) are the measured worst |err| / bar."""
import functools

import numpy as np
import pytest
import torch

import dense_ref as D
import mxfp4_ref as R

pytestmark = pytest.mark.gpu

TYPES = ("f16", "bf16")
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16}
BAR_M = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 40, 64, 130)
BAR_NK = ((48, 96), (80, 4128), (144, 1056), (4096, 256))
ROUTE_M = {R.GEMV: 3, R.STREAM: 17, R.TILED: 40}             # one row count per route for the epilogue / layout cases


def _up(bits, dev, t):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(TORCH[t])


def _bits(y):
    return y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _down(y, t):
    return D.values(_bits(y), t)


def _weight(codes, scales, dev, row_interleave=False):
    from zhilight_amd import ops
    return ops.Mxfp4Weight.from_checkpoint(torch.from_numpy(np.array(codes)).to(dev), torch.from_numpy(np.array(scales)).to(dev), row_interleave)


@functools.lru_cache(maxsize=None)
def _case(n, k, t):
    """inputs for the largest row count and their exact product, shared by every row count (rows are independent)"""
    x, codes, scales, bias = R.inputs(0, max(BAR_M), n, k, t)
    ex, s = R.exact(x, codes, scales, t), R.abs_sum(x, codes, scales, t)
    for a in (x, codes, scales, bias, ex, s):
        a.setflags(write=False)
    return x, codes, scales, bias, ex, s


def test_row_counts_reach_every_route():
    from zhilight_amd import ops
    for n, k in BAR_NK:
        routes = {ops.mxfp4_route(m, n, k) for m in BAR_M}
        assert routes == {ops.MXFP4_GEMV, ops.MXFP4_STREAM, ops.MXFP4_TILED}
        assert all(ops.mxfp4_route(m, n, k) == R.route(m) for m in BAR_M)
    assert {ops.mxfp4_route(m, 144, 1056): m for m in ROUTE_M.values()} == {r: m for r, m in ROUTE_M.items()}


@pytest.mark.parametrize("t", TYPES)
def test_dequantize_bit_exact(dev, t):
    """every byte value (all 256 code pairs, code 8 among them) under scale bytes from 0 to 254: fp32 subnormals, fp16 subnormals
    and overflow, the exact range"""
    from zhilight_amd import ops
    bytes_ = np.array([0, 1, 2, 103, 104, 111, 112, 113, 126, 127, 128, 140, 141, 142, 143, 200, 253, 254], np.uint8)
    codes = np.tile(np.arange(256, dtype=np.uint8), (len(bytes_), 1))                  # (18, 256) -> K = 512, 16 blocks per row
    scales = np.repeat(bytes_[:, None], 16, axis=1)
    got = ops.mxfp4_dequantize(torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev), TORCH[t])
    with np.errstate(over="ignore"):
        want = D.to_bits(R.decode(codes, scales), t)
    assert np.array_equal(_bits(got), want), np.argwhere(_bits(got) != want)[:5]
    assert not (_bits(got)[:, 16] & 0x8000).any()             # byte 8 = codes (8, 0): -0 decodes to +0
    w = _weight(codes, scales, dev)
    assert torch.equal(w.dequantize(TORCH[t]), got) and w.nbytes() == codes.size + scales.size


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("m", (4, 32, 48))
def test_layout_one_hot_rows_exact(dev, t, m):
    """x = rows of the identity: y[i, n] must be T(W[n, k_i]) bit for bit, every other product being an exact zero -- nibble order, scale
    addressing and the fragment maps of every route, with no tolerance; the hot column walks over all of K (129 blocks: three trips
    of the GEMV's lane loop, an odd block count for the 4-wave K split)"""
    from zhilight_amd import ops
    n, k = 80, 4128
    _, codes, scales, _, _, _ = _case(n, k, t)
    w = _weight(codes, scales, dev)
    want = D.to_bits(R.decode(codes, scales), t).T            # (K, N)
    eye = torch.eye(k, dtype=TORCH[t], device=dev)
    got = torch.empty((k, n), dtype=TORCH[t], device=dev)
    assert ops.mxfp4_route(m, n, k) == R.route(m)
    for r0 in range(0, k, m):
        rows = min(m, k - r0)
        if ops.mxfp4_route(rows, n, k) != R.route(m):          # the last, shorter piece: keep it on the route under test
            r0, rows = k - m, m
        ops.mxfp4_linear(eye[r0:r0 + rows], w, out=got[r0:r0 + rows])
    bad = np.argwhere(_bits(got) != want)
    assert bad.size == 0, (len(bad), bad[:5])


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("nk", BAR_NK, ids=lambda nk: f"{nk[0]}x{nk[1]}")
def test_bars(dev, nk, t):
    from zhilight_amd import ops
    n, k = nk
    x, codes, scales, _, ex, s = _case(n, k, t)
    w, xd = _weight(codes, scales, dev), _up(x, dev, t)
    for m in BAR_M:
        got = _down(ops.mxfp4_linear(xd[:m], w), t)
        ratio = D.worst_ratio(got, ex[:m], R.bar(ex[:m], s[:m], m, k, t), f"mxfp4_linear {m}x{n}x{k} {t}")
        print(f"mxfp4_errors: route {R.route(m)} {t} {m}x{n}x{k}: worst |err| / bar {ratio:.4f}")


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("route", sorted(ROUTE_M))
def test_epilogues_strides_aliasing(dev, route, t):
    """bias, residual (out aliasing it) and silu*mul against the stated arithmetic, through a strided x (ldx = K + 64, the padding
    holding values a kernel must not read)"""
    from zhilight_amd import ops
    m, (n, k) = ROUTE_M[route], (144, 1056)
    assert ops.mxfp4_route(m, n, k) == route
    x, codes, scales, bias, ex, s = _case(n, k, t)
    x, ex, s = x[:m], ex[:m], s[:m]
    wide = np.full((m, k + 64), D.to_bits(np.array([777.0]), t)[0], np.uint16)
    wide[:, :k] = x
    xd = _up(wide, dev, t)[:, :k]
    assert xd.stride(0) == k + 64
    w, bd, b64 = _weight(codes, scales, dev), _up(bias, dev, t), D.values(bias, t)
    # plain through the stride: the same bits as from contiguous rows
    plain = ops.mxfp4_linear(xd, w)
    assert torch.equal(plain, ops.mxfp4_linear(_up(x, dev, t), w))
    # bias
    inner, inner_bar = ex + b64[None, :], R.bar(ex + b64[None, :], s, m, k, t)
    r_bias = D.worst_ratio(_down(ops.mxfp4_linear(xd, w, bias=bd), t), inner, inner_bar, f"bias {route} {t}")
    # residual, in place
    res = D.to_bits(np.random.default_rng(3).standard_normal((m, n)), t)
    hid = _up(res, dev, t)
    out = ops.mxfp4_linear(xd, w, bias=bd, residual=hid, out=hid)
    assert out.data_ptr() == hid.data_ptr()
    total, total_bar = R.residual_bar(inner, inner_bar, D.values(res, t), t)
    r_res = D.worst_ratio(_down(hid, t), total, total_bar, f"residual {route} {t}")
    # ... and it is the two-step arithmetic exactly: T(residual + T(acc + bias)) on the biased launch's own output
    two_step = R.rounded(D.values(res, t) + _down(ops.mxfp4_linear(xd, w, bias=bd), t), t)
    assert np.array_equal(_down(hid, t), two_step)
    # silu * mul on the row-interleaved weight: gate = rows 0 .. N/2 - 1 of the checkpoint matrix, up = the rest
    wi = _weight(codes, scales, dev, row_interleave=True)
    h = n // 2
    bi = _up(np.stack([bias[:h], bias[h:]], axis=1).reshape(-1), dev, t)
    act = ops.mxfp4_linear(xd, wi, bias=bi, epilogue=ops.EPI_SILU_MUL)
    assert tuple(act.shape) == (m, h)
    want, want_bar = R.gated_bar(inner[:, :h], inner_bar[:, :h], inner[:, h:], inner_bar[:, h:], t)
    r_act = D.worst_ratio(_down(act, t), want, want_bar, f"silu_mul {route} {t}")
    # ... and the two-launch arithmetic on the rounded halves, to the last rounding of T (expf is the only inexact step)
    yb = _down(ops.mxfp4_linear(xd, w, bias=bd), t)
    g, u = yb[:, :h].astype(np.float32), yb[:, h:].astype(np.float32)
    two = (g / (np.float32(1) + np.exp(-g, dtype=np.float32))) * u
    ulp = np.maximum(np.abs(two.astype(np.float64)) * 2 * D.U[t], 2 * D.TINY[t])
    assert (np.abs(_down(act, t) - two.astype(np.float64)) <= 1.01 * ulp).all()
    print(f"mxfp4_errors: epilogues route {route} {t}: bias {r_bias:.4f} residual {r_res:.4f} silu_mul {r_act:.4f}")
    with pytest.raises(ops.ZLError):
        ops.mxfp4_linear(xd, w, epilogue=ops.EPI_SILU_MUL)    # not a row-interleaved weight


@pytest.mark.parametrize("m", (4, 9, 40))
def test_no_weight_rounding_fp16(dev, m):
    """every scale 2^-24: a kernel that rounds the scaled weight to fp16 loses it (test_mxfp4_host: 759 x the bar); the same bars"""
    from zhilight_amd import ops
    n, k = 48, 256
    x, codes, scales = R.small_scale_inputs(0, m, n, k)
    ex, s = R.exact(x, codes, scales, "f16"), R.abs_sum(x, codes, scales, "f16")
    got = _down(ops.mxfp4_linear(_up(x, dev, "f16"), _weight(codes, scales, dev)), "f16")
    ratio = D.worst_ratio(got, ex, R.bar(ex, s, m, k, "f16"), f"small scales {m}x{n}x{k}")
    assert np.abs(got).max() > 0
    print(f"mxfp4_errors: small scales route {R.route(m)} f16 {m}x{n}x{k}: worst |err| / bar {ratio:.4f}")


def test_argument_checks(dev):
    from zhilight_amd import ops
    codes = torch.zeros((16, 48), dtype=torch.uint8, device=dev)
    scales = torch.full((16, 3), 127, dtype=torch.uint8, device=dev)
    w = ops.Mxfp4Weight.from_checkpoint(codes, scales)
    with pytest.raises(ops.ZLError, match="size K"):
        ops.mxfp4_linear(torch.zeros((2, 64), dtype=torch.float16, device=dev), w)
    with pytest.raises(ops.ZLError):
        ops.mxfp4_linear(torch.zeros((2, 96), dtype=torch.float32, device=dev), w)
    bad = scales.clone()
    bad[3, 1] = 255
    with pytest.raises(ops.ZLError, match="255"):
        ops.Mxfp4Weight.from_checkpoint(codes, bad)
    with pytest.raises(ops.ZLError):
        ops.Mxfp4Weight.from_checkpoint(codes, scales[:, :2].contiguous())
    blocks = ops.Mxfp4Weight.from_checkpoint(codes.view(16, 3, 16), scales)               # the weight_blocks shape
    assert (blocks.n, blocks.k) == (16, 96)
