"""tests/dense_ref.py pinned on the CPU.  Two things have to hold for the bars test_gpu_dense.py uses, at the very shapes it uses:

1. they admit an honest kernel: numpy fp32 emulations of the GEMV's lane-strided summation (8 steps per 512-k load per lane, the
   64-lane butterfly, alpha, bias, one rounding to T) and of a matrix-core order (32 products per block summed in fp32, the blocks added
   in turn) stay inside them;
2. they reject a subtly wrong kernel: each mutation below, rounded to T like an honest result, breaks the bar on at least one element
   wherever the shape has the thing the mutation touches (a second weight row, a second activation row, a bias).
"""
import numpy as np
import pytest

import dense_ref as D

TYPES = ("f16", "bf16")
ALPHA = 0.5


def _f32(bits, t):
    return D.values(bits, t).astype(np.float32)


def _round_t(y, t):
    """fp32 / float64 results -> T -> float64, as the kernels' one final rounding"""
    return D.values(D.to_bits(np.asarray(y, np.float64), t), t)


def emulate_gemv(x, w, t, bias=None, alpha=1.0, to_t=True):
    """k_dense_gemv / k_gemm_nt_f32 in numpy fp32: lane l takes elements 512 j + 8 l + e of load j one after the other (the product of
    two T values is exact in fp32, so acc + a * b in fp32 is the fused step), the lanes meet in the xor butterfly, then alpha and bias"""
    xf, wf = _f32(x, t), _f32(w, t)
    m, k = xf.shape
    n = wf.shape[0]
    loads = (k + 511) // 512
    xp = np.zeros((m, loads * 512), np.float32)
    xp[:, :k] = xf
    xp = xp.reshape(m, loads, 64, 8)
    lanes = np.arange(64)
    out = np.empty((m, n), np.float32)
    for c0 in range(0, n, 512):
        wc = wf[c0:c0 + 512]
        wp = np.zeros((wc.shape[0], loads * 512), np.float32)
        wp[:, :k] = wc
        wp = wp.reshape(wc.shape[0], loads, 64, 8)
        acc = np.zeros((m, wc.shape[0], 64), np.float32)
        for j in range(loads):
            for e in range(8):
                acc = acc + xp[:, None, j, :, e] * wp[None, :, j, :, e]
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, :, lanes ^ off]
        out[:, c0:c0 + 512] = acc[:, :, 0]
    y = np.float32(alpha) * out
    if bias is not None:
        y = y + _f32(bias, t)[None, :]
    assert y.dtype == np.float32
    return _round_t(y, t) if to_t else y.astype(np.float64)


def emulate_mfma(x, w, t, bias=None, alpha=1.0):
    """a matrix-core order: the 32 products of one MFMA step summed in fp32, the steps accumulated one after the other"""
    xf, wf = _f32(x, t), _f32(w, t)
    m, k = xf.shape
    n = wf.shape[0]
    xb, wb = xf.reshape(m, k // 32, 32), wf.reshape(n, k // 32, 32)
    blocks = np.zeros((m, n, k // 32), np.float32)
    for e in range(32):
        blocks = blocks + xb[:, None, :, e] * wb[None, :, :, e]
    acc = np.zeros((m, n), np.float32)
    for g in range(k // 32):
        acc = acc + blocks[:, :, g]
    y = np.float32(alpha) * acc
    if bias is not None:
        y = y + _f32(bias, t)[None, :]
    return _round_t(y, t)


def mutants(x, w, bias, alpha, t, rows_per_wave=1):
    """(name, float64 (m, n) result before the rounding to T) of every mutation the shape can carry"""
    xv, wv = D.values(x, t), D.values(w, t)
    bv = 0.0 if bias is None else D.values(bias, t)[None, :]
    m, k = xv.shape
    n = wv.shape[0]
    prod = xv @ wv.T
    col = n // 2                                                           # the weight row the first two mutations hit
    lo = (((k + 511) // 512) // 2) * 512                                   # a 512-k load in the middle of the row
    y = prod.copy()
    y[:, col] -= xv[:, lo:lo + 512] @ wv[col, lo:lo + 512]
    yield "load_dropped", alpha * y + bv
    if n >= 2:
        first = (col // rows_per_wave) * rows_per_wave if rows_per_wave > 1 else col - 1
        second = first + 1                                                 # the second row of a wave (of two neighbours when a wave has one)
        y = prod.copy()
        y[:, second] = prod[:, first]
        yield "second_row_reads_first", alpha * y + bv
    tail = ((k + 127) // 128 - 1) * 128
    yield "last_chunk_skipped", alpha * (prod - xv[:, tail:] @ wv[:, tail:].T) + bv
    if bias is not None and alpha != 1.0:
        yield "alpha_after_bias", alpha * (prod + bv)
    if m >= 2:
        yield "row_reads_neighbour", alpha * np.roll(prod, -1, axis=0) + bv


MUTATIONS = ("load_dropped", "second_row_reads_first", "last_chunk_skipped", "alpha_after_bias", "row_reads_neighbour")


def _broken(got, exact, bar):
    with np.errstate(invalid="ignore"):
        return bool((np.abs(got - exact) > bar).any())


def _check_family(shapes, t, seed, emulate, chain, norm=None, f32=False, cus=D.DEFAULT_CUS):
    """the emulation inside the bar at every shape; every mutation a shape can carry outside it; returns the mutations seen"""
    seen, worst = set(), 0.0
    for i, (m, n, k) in enumerate(shapes):
        x, w, b = D.inputs(seed + i, m, n, k, t, bias=not f32)
        if norm is not None:
            x = norm(x, k, seed + i)
        c = chain(k)
        s = D.abs_sum(x, w, t)
        for alpha, bias in ((1.0, None), (ALPHA, b)):
            ex = D.exact(x, w, t, bias, alpha)
            if f32:
                bar, got = D.bar_f32(s, alpha, c), emulate(x, w, t, None, alpha, to_t=False)
            else:
                bar = (D.bar_norm if norm is not None else D.bar_rounded)(ex, s, alpha, c, t)
                got = emulate(x, w, t, bias, alpha)
            worst = max(worst, D.worst_ratio(got, ex, bar, f"emulation {t} {(m, n, k)} alpha {alpha}"))
        # mutations: with the bias and alpha = 0.5 (ex, bar are still those)
        rpw = D.gemv_geometry(m, n, k, cus)["rows_per_wave"]
        for name, y in mutants(x, w, bias, alpha, t, rpw):
            got = y if f32 else _round_t(y, t)
            assert _broken(got, ex, bar), f"mutation {name} passes the bar: {t} {(m, n, k)}"
            seen.add(name)
    return seen, worst


def _flip_some_last_bits(xn, seed):
    """what the fused norm may do to oracle.rmsnorm's bits: the last bit of 2 % of the elements moved by one"""
    rng = np.random.default_rng(seed)
    pick = rng.random(xn.shape) < 0.02
    step = np.where(rng.random(xn.shape) < 0.5, 1, -1)
    mag = (xn & 0x7FFF).astype(np.int64)
    moved = np.clip(mag + step, 0, 0x7BFF).astype(np.uint16) | (xn & 0x8000)
    return np.where(pick & (mag > 0), moved, xn).astype(np.uint16)


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("family", ["rows_per_wave", "ring_in_row", "lds", "tiny", "strided"])
def test_gemv_bar_admits_the_lane_order_and_rejects_mutations(t, family):
    shapes = D.gemv_shapes()[family]
    if family == "rows_per_wave":
        shapes = shapes[-1:]                                               # m = 4 holds the rows of m = 1 and 2
    seen, worst = _check_family(shapes, t, 100, emulate_gemv, D.gemv_chain)
    assert seen == set(MUTATIONS), (family, sorted(set(MUTATIONS) - seen))
    assert worst < 1.0


@pytest.mark.parametrize("t", TYPES)
def test_norm_bar_admits_flipped_last_bits_and_rejects_mutations(oracle, t):
    """the fused-norm bar on oracle.rmsnorm's bits, with the last bit of some normalised elements moved as the kernel's own sum of
    squares may; edge rows: all zero, and rows 1e-3, 1 and 100 times the unit scale in one block"""
    def norm(x, k, seed):
        rng = np.random.default_rng(seed + 1000)
        nw = D.to_bits(1 + 0.1 * rng.standard_normal(k), t)
        xs = D.values(x, t)
        if x.shape[0] == 4:
            xs = xs * np.array([[0.0], [1e-3], [1.0], [100.0]])
        return _flip_some_last_bits(oracle.rmsnorm(D.to_bits(xs, t), nw, 1e-5, dtype=D.DT[t]), seed)
    shapes = D.gemv_shapes()
    seen, worst = _check_family(shapes["strided"] + shapes["norm_edge"], t, 200, emulate_gemv, D.gemv_chain, norm=norm)
    assert seen == set(MUTATIONS) and worst < 1.0


@pytest.mark.parametrize("t", TYPES)
def test_mfma_bar_admits_a_blocked_order_and_rejects_mutations(t):
    """every m, n and k of the GPU test at least once (the full product runs on the GPU); k = 384, 640, 1152 are 3, 5, 9 chunks"""
    shapes = [(m, D.GEMM_N[i % 5], D.GEMM_K[i % 3]) for i, m in enumerate(D.GEMM_M)]
    assert {s[1] for s in shapes} == set(D.GEMM_N) and {s[2] for s in shapes} == set(D.GEMM_K)
    assert all((k // 128) % 2 == 1 and k // 128 >= 3 for k in D.GEMM_K)
    seen, worst = _check_family(shapes, t, 300, emulate_mfma, D.mfma_chain)
    assert seen == set(MUTATIONS) and worst < 1.0


@pytest.mark.parametrize("t", TYPES)
def test_f32_bar_admits_the_lane_order_and_rejects_mutations(t):
    """gemm_nt_f32 has no bias, so alpha cannot come after it: the other four mutations"""
    seen, worst = _check_family(list(D.F32_SHAPES), t, 400, emulate_gemv, D.f32_chain, f32=True)
    assert seen == set(MUTATIONS) - {"alpha_after_bias"} and worst < 1.0


def test_launch_geometry_of_the_gpu_shapes():
    """the shapes reach the code they are chosen for (on 256 compute units)"""
    sh = D.gemv_shapes()
    for m, n, k in sh["rows_per_wave"]:
        g = D.gemv_geometry(m, n, k)
        assert n == 4099 and g["rows_per_wave"] == 3 and g["loads_per_row"] == 3 and g["loads_per_wave"] == 9 > 8
    assert D.gemv_geometry(1, 1000, 2304)["loads_per_wave"] == 5                      # test_dense_gemm_small_m: the ring never refills
    g3, g5 = (D.gemv_geometry(m, 300, 5000) for m in (3, 5))
    assert g3["loads_per_row"] == 10 and 5000 % 512 != 0 and (g3["mt"], g3["row_blocks"]) == (2, 2) and (g5["mt"], g5["row_blocks"]) == (4, 2)
    lds = [D.gemv_geometry(*s) for s in sh["lds"]]
    assert [g["mt"] for g in lds] == [2, 1, 1] and D.gemv_geometry(4, 96, 4096)["mt"] == 4
    assert lds[0]["lds_bytes"] <= 64 * 1024 and lds[1]["lds_bytes"] <= 64 * 1024 < lds[2]["lds_bytes"] <= 160 * 1024
    assert D.gemv_geometry(3, 131, 1096)["mt"] == 2 and D.gemv_geometry(1, 4099, 8)["total_waves"] == 1368


def test_chain_lengths_and_bar_terms():
    assert D.gemv_chain(8) == D.gemv_chain(512) == 32 and D.gemv_chain(513) == 48 and D.gemv_chain(53248) == 2 * (8 * 104 + 8)
    assert D.mfma_chain(384) == 768 and D.f32_chain(2048) == 40 and 2 * D.f32_chain(7168) == D.gemv_chain(7168)
    ex, s = np.array([[0.0, 2.0, -4.0]]), np.array([[1.0, 1.0, 3.0]])
    for t in TYPES:
        bar = D.bar_rounded(ex, s, -0.5, 32, t)
        want = 1.01 * D.U[t] * np.abs(ex) + 32 * 2.0 ** -24 * 0.5 * s + D.TINY[t]
        assert np.array_equal(bar, want) and np.array_equal(D.bar_norm(ex, s, -0.5, 32, t), want + D.U[t] * 0.5 * s)
        # half an ulp of T at 1.0 and the smallest subnormal of T: what the u_T and the tiny term stand for
        one = D.values(np.array([0x3C00 if t == "f16" else 0x3F80], np.uint16), t)[0]
        nxt = D.values(np.array([0x3C01 if t == "f16" else 0x3F81], np.uint16), t)[0]
        assert one == 1.0 and (nxt - one) / 2 == D.U[t] and D.values(np.array([1], np.uint16), t)[0] == 2 * D.TINY[t]
    assert np.array_equal(D.bar_f32(s, 0.37, 32), 32 * 2.0 ** -24 * 0.37 * s)


def test_worst_ratio_reports_and_raises():
    ex = np.array([[1.0, np.nan, -np.inf, 2.0]])
    bar = np.array([[0.5, 0.5, 0.5, 0.5]])
    assert D.worst_ratio(np.array([[1.25, np.nan, -np.inf, 2.0]]), ex, bar, "ok") == 0.5
    zero = np.zeros((1, 2))                                                            # S = 0: a bar of 0 admits the exact 0 only
    assert D.worst_ratio(zero, zero, zero, "zero bar") == 0.0
    with pytest.raises(AssertionError):
        D.worst_ratio(np.array([[0.0, 1e-30]]), zero, zero, "zero bar")
    for got in ([[1.75, np.nan, -np.inf, 2.0]], [[1.0, 0.0, -np.inf, 2.0]], [[1.0, np.nan, 5.0, 2.0]], [[np.nan, np.nan, -np.inf, 2.0]],
                [[1.0, np.nan, -np.inf, np.inf]]):
        with pytest.raises(AssertionError):
            D.worst_ratio(np.array(got), ex, bar, "bad")


def test_first_argmax_and_ranked_top_k():
    nan, inf = np.nan, np.inf
    rows = np.array([[1.0, 3.0, 3.0, 2.0], [-inf, -inf, -inf, -inf], [5.0, nan, 9.0, nan], [-0.0, 0.0, -1.0, -2.0]])
    assert D.first_argmax(rows).tolist() == [1, 0, 1, 0]
    assert D.ranked_top_k(np.array([[1.0, 3.0, 3.0, 2.0]]), 3).tolist() == [[1, 2, 3]]
    assert D.routing_skipped(np.array([[10.0, 8.0, 6.0, 5.9], [10.0, 8.0, 6.0, 1.0]]), 2, 0.06).tolist() == [False, False]
    assert D.routing_skipped(np.array([[10.0, 8.0, 6.0, 5.9], [10.0, 8.0, 7.9, 1.0]]), 2, 0.06).tolist() == [False, True]
    assert D.routing_skipped(np.array([[10.0, 8.0, 6.0, 5.9]]), 3, 0.06).tolist() == [True]


@pytest.mark.parametrize("t", TYPES)
def test_routing_check_keeps_most_tokens(t):
    """the routing check of test_gpu_dense.py on the reference alone: few tokens have a near-tie among their top k + 1 logits"""
    counts = []
    for shape, seed, top_k in D.ROUTING:
        x, w = D.routing_inputs(shape, seed, t)
        ex = D.exact(x, w, t)
        bar = D.bar_f32(D.abs_sum(x, w, t), 1.0, D.f32_chain(shape[2]))
        skipped = int(D.routing_skipped(ex, top_k, bar.max()).sum())
        counts.append(skipped)
        assert skipped <= D.ROUTING_MAX_SKIPPED, (t, shape, skipped)
        # the emulated kernel routes every decidable token as the exact logits do
        got = emulate_gemv(x, w, t, to_t=False)
        keep = ~D.routing_skipped(ex, top_k, bar.max())
        assert np.array_equal(D.ranked_top_k(got.astype(np.float32), top_k)[keep], D.ranked_top_k(ex.astype(np.float32), top_k)[keep])
    if t == "f16":
        assert tuple(counts) == D.ROUTING_SKIPPED_F16
