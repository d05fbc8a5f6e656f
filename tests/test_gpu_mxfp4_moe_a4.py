"""The expert-grouped MXFP4 x MXFP4 GEMM (csrc/mxfp4_moe_a4.hip) on the GPU, at every tile height: each live row bit for bit against
ops.mxfp4_a4_linear on that row and that expert's matrix, and against the exact float64 product of the decoded operands under
mxfp4_ref's matrix-core bar (c = 2 K); two wrong-argument cases.  "mxfp4_moe_a4_errors:" lines (pytest -s): worst |err| / bar."""
import functools

import numpy as np
import pytest
import torch

import dense_ref as D
import mxfp4_ref as R
from test_gpu_mxfp4 import TORCH, TYPES, _bits, _down
from test_gpu_mxfp4_moe import E, SENTINEL, _routing

pytestmark = pytest.mark.gpu

# (80, 160): 5 blocks -- byte-gathered scales, K padded to 128 with the zero block, less than one super-step, N one wave and a quarter
# (the second wave partly filled, two waves only stage); (272, 640): 20 blocks -- dword scales, one full super-step plus a tail, two
# workgroup columns with a partly filled last one
SHAPES = ((80, 160), (272, 640))
GROUPED = {80: 16, 150: 32, 400: 64}              # pairs -> rows per tile (_routing: loads 0, 1, BM, BM + 1, three tiles and more, 0)
ROWS = max(GROUPED)


@functools.lru_cache(maxsize=None)
def _case(n, k, t):
    """ROWS activation rows of type t quantised to MXFP4, E quantised (n, k) matrices, every expert's exact product with every row
    and its bar"""
    rng = np.random.default_rng(4000 * n + k)
    xq, xs = R.quantize(D.values(D.to_bits(rng.standard_normal((ROWS, k)), t), t))
    ws = [R.quantize(0.05 * rng.standard_normal((n, k))) for _ in range(E)]
    a, dec = R.decode(xq, xs), [R.decode(c, s) for c, s in ws]
    ex = np.stack([a @ w.T for w in dec])
    bar = np.stack([R.bar(v, np.abs(a) @ np.abs(w).T, ROWS, k, t) for v, w in zip(ex, dec)])
    return xq, xs, ws, ex, bar


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("nk", SHAPES, ids=lambda nk: f"{nk[0]}x{nk[1]}")
@pytest.mark.parametrize("pairs", sorted(GROUPED))
def test_grouped_bits_and_float64(dev, pairs, nk, t):
    """gate|up (tokens gathered with in_div = 2, silu*mul) and down (row j scattered to row index[j], y five rows short): live rows
    equal mxfp4_a4_linear's bits and stay inside the float64 bar; rows of ids outside the stack and rows past y_rows keep the sentinel"""
    from zhilight_amd import ops
    (n, k), bm, live, h = nk, GROUPED[pairs], pairs - 2, nk[0] // 2
    assert ops.mxfp4_moe_a4_bm(pairs, E) == bm
    xq, xs, ws, ex, bar = _case(n, k, t)
    xqd, xsd = torch.from_numpy(xq).to(dev), torch.from_numpy(xs).to(dev)
    parts = [[torch.from_numpy(w[i]).to(dev) for w in ws] for i in range(2)]
    w, wi = ops.Mxfp4MoEWeight.from_checkpoint(*parts), ops.Mxfp4MoEWeight.from_checkpoint(*parts, row_interleave=True)
    ids, order, ld, od = _routing(pairs, bm, dev)
    ee, pos = ids[order[:live]], np.arange(live)

    act = torch.full((pairs, h), SENTINEL, dtype=TORCH[t], device=dev)
    ops.mxfp4_moe_a4_grouped(xqd[:pairs // 2], xsd[:pairs // 2], wi, TORCH[t], ld, od, pairs, in_div=2, out=act, epilogue=ops.EPI_SILU_MUL)
    alone = np.stack([_bits(ops.mxfp4_a4_linear(xqd[:pairs // 2], xsd[:pairs // 2], ops.Mxfp4Weight(wi.codes[e], wi.scales[e], True), TORCH[t],
                                                epilogue=ops.EPI_SILU_MUL)) for e in range(E)])
    assert np.array_equal(_bits(act[:live]), alone[ee, order[:live] // 2])
    assert bool((act[live:] == SENTINEL).all())
    rows = order[:live] // 2
    want, want_bar = R.gated_bar(ex[ee, rows, :h], bar[ee, rows, :h], ex[ee, rows, h:], bar[ee, rows, h:], t)
    r_up = D.worst_ratio(_down(act[:live], t), want, want_bar, f"gate|up {pairs} {n}x{k} {t}")

    yr = pairs - 5
    y = torch.full((pairs, n), SENTINEL, dtype=TORCH[t], device=dev)
    ops.mxfp4_moe_a4_grouped(xqd[:pairs], xsd[:pairs], w, TORCH[t], ld, od, pairs, out_scatter=True, out=y[:yr], out_rows=yr)
    alone = np.stack([_bits(ops.mxfp4_a4_linear(xqd[:pairs], xsd[:pairs], ops.Mxfp4Weight(w.codes[e], w.scales[e]), TORCH[t])) for e in range(E)])
    got, kept = _bits(y), order[:live] < yr
    assert kept.sum() >= live - 5 and np.array_equal(got[order[:live][kept]], alone[ee[kept], pos[kept]])
    dead = np.setdiff1d(np.arange(pairs), order[:live][kept])
    assert len(dead) == pairs - kept.sum() and bool((y[torch.from_numpy(dead).to(dev)] == SENTINEL).all())
    r_down = D.worst_ratio(D.values(got[order[:live][kept]], t), ex[ee[kept], pos[kept]], bar[ee[kept], pos[kept]], f"down {pairs} {n}x{k} {t}")
    print(f"mxfp4_moe_a4_errors: grouped bm {bm} {t} {pairs} pairs {n}x{k}: gate|up {r_up:.4f} down {r_down:.4f}")


def test_argument_checks(dev):
    from zhilight_amd import ops
    w = ops.Mxfp4MoEWeight.from_checkpoint(torch.zeros((2, 16, 48), dtype=torch.uint8, device=dev), torch.full((2, 16, 3), 127, dtype=torch.uint8, device=dev))
    xq, xs = torch.zeros((40, 48), dtype=torch.uint8, device=dev), torch.full((40, 3), 127, dtype=torch.uint8, device=dev)
    loads = torch.tensor([25, 15], dtype=torch.int32, device=dev)
    y = ops.mxfp4_moe_a4_grouped(xq, xs, w, torch.float16, loads, None, 40)
    assert tuple(y.shape) == (40, 16) and not y.any()
    with pytest.raises(ops.ZLError, match="K mismatch"):
        ops.mxfp4_moe_a4_grouped(torch.zeros((40, 64), dtype=torch.uint8, device=dev), xs, w, torch.float16, loads, None, 40)
    with pytest.raises(ops.ZLError, match="xs"):
        ops.mxfp4_moe_a4_grouped(xq, xs[:, :2].contiguous(), w, torch.float16, loads, None, 40)
