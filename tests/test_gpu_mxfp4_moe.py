"""The expert-grouped MXFP4 GEMMs (csrc/mxfp4_moe.hip) on the GPU: the grouped form at every tile shape and the pairs form against
the exact float64 product (bars of tests/mxfp4_ref.py with the chain constant c = 2 K, the module's ceiling for any summation order,
doubled for the MFMA), the layout of both forms with one-hot rows and no tolerance, and the bits of a row with and without company.
Lines starting "mxfp4_moe_errors:" (pytest -s) are the measured worst |err| / bar."""
import functools

import numpy as np
import pytest
import torch

import dense_ref as D
import mxfp4_ref as R
from test_gpu_mxfp4 import TORCH, TYPES, _bits, _down, _up

pytestmark = pytest.mark.gpu

E = 6
SHAPES = ((80, 1056), (48, 96))                   # K = 33 blocks (odd, no multiple of 4) and 3 blocks (less than one quad per wave); N % 64 != 0
GROUPED = {40: 16, 80: 16, 150: 32, 400: 64}      # pairs -> rows per tile.  40 pairs cannot hold a 3-tile run next to the other loads: 80 does
ROWS = max(GROUPED)
SENTINEL = 768.0                                  # a value of fp16 and of bf16
shape_id = lambda nk: f"{nk[0]}x{nk[1]}"          # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(n, k, t):
    """ROWS activation rows, E quantised (n, k) matrices, every expert's exact product with every row and its bar"""
    rng = np.random.default_rng(1000 * n + k)
    x = D.to_bits(rng.standard_normal((ROWS, k)), t)
    ws = [R.quantize(0.05 * rng.standard_normal((n, k))) for _ in range(E)]
    ex = np.stack([R.exact(x, c, s, t) for c, s in ws])
    bar = np.stack([D.bar_rounded(v, R.abs_sum(x, c, s, t), 1.0, 2 * k, t) for v, (c, s) in zip(ex, ws)])
    return x, ws, ex, bar


@functools.lru_cache(maxsize=None)
def _device(dev, n, k, t):
    """x with row stride K + 64 (the padding poisoned), the plain stack and the row-interleaved gate|up stack of the same matrices"""
    from zhilight_amd import ops
    x, ws, _, _ = _case(n, k, t)
    wide = np.full((ROWS, k + 64), D.to_bits(np.array([SENTINEL]), t)[0], np.uint16)
    wide[:, :k] = x
    parts = [[torch.from_numpy(w[i]).to(dev) for w in ws] for i in range(2)]
    return _up(wide, dev, t)[:, :k], ops.Mxfp4MoEWeight.from_checkpoint(*parts), ops.Mxfp4MoEWeight.from_checkpoint(*parts, row_interleave=True)


def _routing(pairs, bm, dev):
    """ids by hand: a zero-load expert first and last, loads 1, bm, bm + 1 and the rest (3 tiles and more, but for 40 pairs), dealt to
    the pairs in a fixed shuffle, with two ids outside the stack, sorted behind it -> (ids, loads, order, device loads, device order)"""
    loads = np.array([0, 1, bm, bm + 1, pairs - 2 * bm - 4, 0], np.int32)
    assert loads[4] > 2 * bm or pairs == 40
    ids = np.concatenate([np.repeat(np.arange(E), loads), [-1, E + 1]])[np.random.default_rng(pairs).permutation(pairs)].astype(np.int32)
    order = np.argsort(np.where((ids < 0) | (ids >= E), E, ids), kind="stable").astype(np.int32)
    return ids, order, torch.from_numpy(loads).to(dev), torch.from_numpy(order).to(dev)


def _gated(ex, bar, ee, rows, t):
    h = ex.shape[2] // 2
    return R.gated_bar(ex[ee, rows, :h], bar[ee, rows, :h], ex[ee, rows, h:], bar[ee, rows, h:], t)


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("nk", SHAPES, ids=shape_id)
@pytest.mark.parametrize("pairs", sorted(GROUPED))
def test_grouped_against_float64(dev, pairs, nk, t):
    """gate|up: tokens gathered with in_div = 2 under silu*mul; down, separately: row j of independent inputs scattered to row
    index[j].  The rows of the two ids outside the stack keep their sentinel."""
    from zhilight_amd import ops
    (n, k), bm, live = nk, GROUPED[pairs], pairs - 2
    assert ops.mxfp4_moe_bm(pairs, E) == bm
    _, _, ex, bar = _case(n, k, t)
    xd, w, wi = _device(dev, n, k, t)
    ids, order, ld, od = _routing(pairs, bm, dev)
    ee = ids[order[:live]]
    act = torch.full((pairs, n // 2), SENTINEL, dtype=TORCH[t], device=dev)
    ops.mxfp4_moe_grouped(xd[:pairs // 2], wi, ld, od, pairs, in_div=2, out=act, epilogue=ops.EPI_SILU_MUL)
    want, want_bar = _gated(ex, bar, ee, order[:live] // 2, t)
    r_up = D.worst_ratio(_down(act[:live], t), want, want_bar, f"gate|up {pairs} {n}x{k} {t}")
    assert bool((act[live:] == SENTINEL).all())
    y = torch.full((pairs, n), SENTINEL, dtype=TORCH[t], device=dev)
    ops.mxfp4_moe_grouped(xd[:pairs], w, ld, od, pairs, out_scatter=True, out=y)
    got, rows = _down(y, t), np.arange(live)
    r_down = D.worst_ratio(got[order[:live]], ex[ee, rows], bar[ee, rows], f"down {pairs} {n}x{k} {t}")
    assert (got[order[live:]] == SENTINEL).all()
    print(f"mxfp4_moe_errors: grouped bm {bm} {t} {pairs} pairs {n}x{k}: gate|up {r_up:.4f} down {r_down:.4f}")


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("nk", SHAPES, ids=shape_id)
@pytest.mark.parametrize("pairs", (1, 8, 13))
def test_pairs_against_float64(dev, pairs, nk, t):
    """repeated experts and (past one pair) an id outside the stack, whose row keeps its sentinel; row j / in_div, both epilogues"""
    from zhilight_amd import ops
    n, k = nk
    _, _, ex, bar = _case(n, k, t)
    xd, w, wi = _device(dev, n, k, t)
    ids = (np.arange(pairs) * 5 % 4).astype(np.int32)
    if pairs > 1:
        ids[pairs // 2] = E
    ok, idd = ids < E, torch.from_numpy(ids).to(dev)
    for in_div in (0, 2):
        rows = np.arange(pairs) // in_div if in_div else np.arange(pairs)
        for epi in (0, ops.EPI_SILU_MUL):
            out = torch.full((pairs, n // 2 if epi else n), SENTINEL, dtype=TORCH[t], device=dev)
            ops.mxfp4_moe_pairs(xd[:pairs], wi if epi else w, idd, in_div=in_div, out=out, epilogue=epi)
            want, want_bar = _gated(ex, bar, ids[ok], rows[ok], t) if epi else (ex[ids[ok], rows[ok]], bar[ids[ok], rows[ok]])
            got = _down(out, t)
            ratio = D.worst_ratio(got[ok], want, want_bar, f"pairs {pairs} in_div {in_div} epi {epi} {n}x{k} {t}")
            assert (got[~ok] == SENTINEL).all()
            print(f"mxfp4_moe_errors: pairs {t} {pairs} pairs in_div {in_div} epilogue {epi} {n}x{k}: {ratio:.4f}")


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("e", (6, 48, 96))
def test_layout_identity_rows_exact(dev, e, t):
    """x = the K rows of the identity, top-k 1, ids[j] = j % E: y[j] must be T(W_{ids[j]}[:, j]) bit for bit -- nibble order, scale
    addressing, the expert stride and both row maps (gather by index[j], scatter to index[j]) with no tolerance, at every tile shape"""
    from zhilight_amd import ops
    n, k = 80, 1056
    assert ops.mxfp4_moe_bm(k, e) == {6: 64, 48: 32, 96: 16}[e]
    rng = np.random.default_rng(e)
    codes, scales = rng.integers(0, 256, (e, n, k // 2), dtype=np.uint8), rng.integers(120, 131, (e, n, k // 32)).astype(np.uint8)
    ids = (np.arange(k) % e).astype(np.int32)
    want = D.to_bits(R.decode(codes.reshape(e * n, -1), scales.reshape(e * n, -1)).reshape(e, n, k)[ids, :, np.arange(k)], t)
    w = ops.Mxfp4MoEWeight.from_checkpoint(torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev))
    eye = torch.eye(k, dtype=TORCH[t], device=dev)
    order = torch.from_numpy(np.argsort(ids, kind="stable").astype(np.int32)).to(dev)
    loads = torch.from_numpy(np.bincount(ids, minlength=e).astype(np.int32)).to(dev)
    got = ops.mxfp4_moe_grouped(eye, w, loads, order, k, in_div=1, out_scatter=True)
    bad = np.argwhere(_bits(got) != want)
    assert bad.size == 0, (len(bad), bad[:5])
    assert np.array_equal(_bits(ops.mxfp4_moe_pairs(eye[:13], w, torch.from_numpy(ids[:13]).to(dev))), want[:13])


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("pairs", sorted(GROUPED))
def test_a_rows_bits_do_not_depend_on_its_company(dev, pairs, t):
    """the only row of a tile, the last row of a full tile and the last row of the last run of the launch above, each against the
    same pair run alone through the grouped form (one 16-row tile): the same bits"""
    from zhilight_amd import ops
    (n, k), bm = SHAPES[0], GROUPED[pairs]
    xd, _, wi = _device(dev, n, k, t)
    ids, order, ld, od = _routing(pairs, bm, dev)
    act = ops.mxfp4_moe_grouped(xd[:pairs // 2], wi, ld, od, pairs, in_div=2, epilogue=ops.EPI_SILU_MUL)
    for j in (0, bm, pairs - 3):
        one = torch.zeros(E, dtype=torch.int32, device=dev)
        one[ids[order[j]]] = 1
        alone = ops.mxfp4_moe_grouped(xd[:pairs // 2], wi, one, od[j:j + 1], 1, in_div=2, epilogue=ops.EPI_SILU_MUL)
        assert torch.equal(alone[0], act[j]), (j, bm)
