"""The dense GEMV / GEMM family (csrc/dense_gemv.hip, csrc/dense_gemm.hip) against the exact float64 product with the per-element bars of
tests/dense_ref.py (derived there, shown on the CPU to admit an honest kernel and reject a subtly wrong one by test_dense_ref_host.py):
gemm_nt_small_m at the shapes where its weight ring refills, crosses weight rows and its launcher changes branch; the greedy pick
(argmax_ws + greedy_advance) against the first maximum of the logits the same launch returned, NaN the largest; gemm_nt / gemm_nt_packed
at odd chunk counts and the tile edges; gemm_nt_f32 with the routing it feeds.  Lines starting "dense_errors:" (pytest -s) are the
figures kept in profiles/dense_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_ref as D

pytestmark = pytest.mark.gpu

TYPES = ("f16", "bf16")
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16}


def _up(bits, dev, t):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(TORCH[t])


def _down(y, t):
    """a device tensor of T -> the exact float64 values of its elements"""
    return D.values(y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), t)


def _cus():
    from zhilight_amd import _lib
    cus = int(_lib.lib().zl_device_cu_count())
    assert cus > 0
    return cus


def _report(kernel, t, family, ratio):
    print(f"dense_errors: {kernel} {t} {family}: worst |err| / bar {ratio:.4f}")


def _strided(bits, dev, t, pad=64):
    """the rows as a column slice of an (m, k + pad) tensor: ldx > k, the padding filled with large values a kernel must not read"""
    m, k = bits.shape
    wide = np.full((m, k + pad), D.to_bits(np.array([777.0]), t)[0], np.uint16)
    wide[:, :k] = bits
    return _up(wide, dev, t)[:, :k]


def _abi(name, xd, wd, bd, alpha, t, out_dtype=None, norm_weight=None, norm_eps=0.0, out=None):
    """zl_gemm_nt_small_m / zl_gemm_nt / zl_gemm_nt_packed / zl_gemm_nt_f32 through the C ABI with the rows' own stride as ldx: the
    ops.py wrappers take contiguous tensors only, the launchers take any ldx >= k (wd: the weight tensor, or a DenseMWeight)"""
    from zhilight_amd import _lib
    assert xd.dim() == 2 and xd.stride(1) == 1 and xd.stride(0) > xd.shape[1]
    m, k = xd.shape
    n = wd.n if hasattr(wd, "n") else wd.shape[0]
    wt = wd.data if hasattr(wd, "n") else wd
    y = out if out is not None else torch.empty((m, n), dtype=out_dtype or xd.dtype, device=xd.device)
    p = lambda a: C.c_void_p(0 if a is None else a.data_ptr())
    i, f = (lambda v: C.c_int64(int(v))), (lambda v: C.c_float(float(v)))
    head = (p(xd), i(xd.stride(0)), p(wt))
    dims = (i(m), i(n), i(k), f(alpha), C.c_int(D.DT[t]))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if name == "zl_gemm_nt_f32":
        args = head + (p(y),) + dims + (stream,)
    elif name == "zl_gemm_nt_small_m":
        args = head + (p(bd), p(y)) + dims + (p(norm_weight), f(norm_eps), stream)
    else:
        args = head + (p(bd), p(y)) + dims + (stream,)
    _lib.check(getattr(_lib.lib(), name)(*args), name)
    return y


def _small_m(x, w, t, dev, bias=None, alpha=1.0, what="", norm=None, oracle=None, strided=False, out=None, **kw):
    """ops.gemm_nt_small_m on the device against the exact product; returns (worst ratio, device output).  norm = (weight bits, eps):
    the fused final norm, referred to the exact product on oracle.rmsnorm(x)"""
    from zhilight_amd import ops
    xd = _strided(x, dev, t) if strided else _up(x, dev, t)
    assert xd.stride(0) == x.shape[1] + (64 if strided else 0)
    k = x.shape[1]
    if norm is not None:
        kw.update(norm_weight=_up(norm[0], dev, t), norm_eps=norm[1])
        x = oracle.rmsnorm(x, norm[0], norm[1], dtype=D.DT[t])
    if strided:
        y = _abi("zl_gemm_nt_small_m", xd, _up(w, dev, t), None if bias is None else _up(bias, dev, t), alpha, t, out=out, **kw)
    else:
        y = ops.gemm_nt_small_m(xd, _up(w, dev, t), None if bias is None else _up(bias, dev, t), alpha, out=out, **kw)
    assert out is None or y is out
    ex = D.exact(x, w, t, bias, alpha)
    bar = (D.bar_rounded if norm is None else D.bar_norm)(ex, D.abs_sum(x, w, t), alpha, D.gemv_chain(k), t)
    return D.worst_ratio(_down(y, t), ex, bar, f"gemm_nt_small_m {t} {x.shape[0], w.shape[0], k} {what}"), y


# ---- gemm_nt_small_m: values --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_small_m_several_rows_per_wave(dev, t):
    """n = 2 * (8 * CUs) + 3, k = 1536: three weight rows per wave, nine loads through the 8-slot ring -- it refills, across a row"""
    cus = _cus()
    worst = 0.0
    for m, n, k in D.gemv_shapes(cus)["rows_per_wave"]:
        g = D.gemv_geometry(m, n, k, cus)
        assert n == 2 * 8 * cus + 3 and g["rows_per_wave"] >= 2 and g["loads_per_wave"] > 8, g
        x, w, b = D.inputs(10 + m, m, n, k, t)
        worst = max(worst, _small_m(x, w, t, dev)[0], _small_m(x, w, t, dev, b, 0.5, "bias alpha")[0])
    _report("gemm_nt_small_m", t, "rows_per_wave", worst)


@pytest.mark.parametrize("t", TYPES)
def test_small_m_ring_refills_inside_a_row(dev, t):
    """k = 5000: ten loads per row, the last one partial; m = 3 runs mt = 2 in two row blocks, the second with a dead row; m = 5"""
    worst = 0.0
    for m, n, k in D.gemv_shapes()["ring_in_row"]:
        assert D.gemv_geometry(m, n, k, _cus())["loads_per_row"] == 10
        x, w, b = D.inputs(20 + m, m, n, k, t)
        worst = max(worst, _small_m(x, w, t, dev)[0], _small_m(x, w, t, dev, b, 0.5, "bias alpha")[0])
    _report("gemm_nt_small_m", t, "ring_in_row", worst)


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("shape", D.gemv_shapes()["lds"], ids=lambda s: "x".join(map(str, s)))
def test_small_m_lds_branches(dev, t, shape):
    """(4, 8192): the LDS rule drops mt from 4 to 2; (4, 16384): to 1; (2, 53248): more than 64 KiB of dynamic LDS"""
    m, n, k = shape
    x, w, b = D.inputs(30, m, n, k, t)
    worst = max(_small_m(x, w, t, dev)[0], _small_m(x, w, t, dev, b, 0.5, "bias alpha")[0])
    _report("gemm_nt_small_m", t, f"lds k={k}", worst)


@pytest.mark.parametrize("t", TYPES)
def test_small_m_tiny_shapes(dev, t):
    worst = 0.0
    for i, (m, n, k) in enumerate(D.gemv_shapes()["tiny"]):
        x, w, b = D.inputs(40 + i, m, n, k, t, w_scale=1.0)
        worst = max(worst, _small_m(x, w, t, dev)[0], _small_m(x, w, t, dev, b, 0.5, "bias alpha")[0])
    _report("gemm_nt_small_m", t, "tiny", worst)


@pytest.mark.parametrize("t", TYPES)
def test_small_m_strided_rows_bias_alpha_out(oracle, dev, t):
    """x a column slice (ldx = k + 64), bias, alpha = 0.5 and out= together; the same with the fused norm"""
    (m, n, k), = D.gemv_shapes()["strided"]
    x, w, b = D.inputs(50, m, n, k, t)
    nw = D.to_bits(1 + 0.1 * np.random.default_rng(51).standard_normal(k), t)
    for norm in (None, (nw, 1e-5)):
        out = torch.full((m, n), 7.0, dtype=TORCH[t], device=dev)
        r, _ = _small_m(x, w, t, dev, b, 0.5, "strided", norm=norm, oracle=oracle, strided=True, out=out)
        _report("gemm_nt_small_m", t, "strided bias alpha out" + (" norm" if norm else ""), r)


@pytest.mark.parametrize("t", TYPES)
def test_small_m_fused_norm_edge_rows(oracle, dev, t):
    """an all-zero activation row gives finite output (the bias), rows of 1e-3, 1 and 100 times the unit scale share one block"""
    (m, n, k), = D.gemv_shapes()["norm_edge"]
    x, w, b = D.inputs(60, m, n, k, t)
    x = D.to_bits(D.values(x, t) * np.array([[0.0], [1e-3], [1.0], [100.0]]), t)
    nw = D.to_bits(1 + 0.1 * np.random.default_rng(61).standard_normal(k), t)
    r, y = _small_m(x, w, t, dev, b, 1.0, "norm edge rows", norm=(nw, 1e-5), oracle=oracle)
    y = _down(y, t)
    assert np.isfinite(y).all() and np.array_equal(y[0], D.values(b, t))
    _report("gemm_nt_small_m", t, "norm edge rows", r)


# ---- the greedy pick -----------------------------------------------------------------------------------------------------------------------
def _greedy(x, w, t, dev, bias=None, alpha=1.0, what=""):
    """one lm_head launch with argmax_ws + greedy_advance: the logits inside their bar, the pick the first maximum of THOSE logits (a
    NaN the largest), the counters advanced by one, next_tokens == tokens.  Returns (picks, logits as float64, device logits)"""
    from zhilight_amd import ops
    m, n = x.shape[0], w.shape[0]
    xd, wd = _up(x, dev, t), _up(w, dev, t)
    bd = None if bias is None else _up(bias, dev, t)
    ws = ops.argmax_workspace(m, n, dev)
    ws.fill_(float("nan"))
    y = ops.gemm_nt_small_m(xd, wd, bd, alpha, argmax_ws=ws)
    i32 = dict(dtype=torch.int32, device=dev)
    tokens, pos, place, valid = torch.full((m,), -7, **i32), torch.full((m,), 3, **i32), torch.full((m,), 4, **i32), torch.full((m,), 5, **i32)
    nxt = torch.full((m,), -9, dtype=torch.int64, device=dev)
    ops.greedy_advance(ws, m, n, tokens, pos, place, valid, nxt)
    logits = _down(y, t)
    ex = D.exact(x, w, t, bias, alpha)
    bar = D.bar_rounded(ex, D.abs_sum(x, w, t), alpha, D.gemv_chain(x.shape[1]), t)
    D.worst_ratio(logits, ex, bar, f"greedy logits {t} {m, n, x.shape[1]} {what}")
    want = D.first_argmax(logits)
    picks = nxt.cpu().numpy()
    assert picks.tolist() == want.tolist(), (what, t, (m, n), picks.tolist(), want.tolist())
    assert tokens.cpu().numpy().tolist() == picks.tolist()
    assert pos.tolist() == [4] * m and place.tolist() == [5] * m and valid.tolist() == [6] * m
    return picks, logits, y


@pytest.mark.parametrize("t", TYPES)
def test_greedy_pick_plain_shapes(dev, t):
    """the several-rows-per-wave shape (its logits bit-identical to a launch without argmax_ws), n = 1 and 3 (most waves empty), m = 5, 8"""
    from zhilight_amd import ops
    cus = _cus()
    m, n, k = D.gemv_shapes(cus)["rows_per_wave"][-1]
    assert D.gemv_geometry(m, n, k, cus)["rows_per_wave"] >= 2
    x, w, b = D.inputs(70, m, n, k, t)
    _, _, y = _greedy(x, w, t, dev, what="rows per wave")
    plain = ops.gemm_nt_small_m(_up(x, dev, t), _up(w, dev, t))
    assert torch.equal(y.view(torch.int16), plain.view(torch.int16))
    _, _, y = _greedy(x, w, t, dev, b, 0.5, what="rows per wave, bias alpha")
    plain = ops.gemm_nt_small_m(_up(x, dev, t), _up(w, dev, t), _up(b, dev, t), 0.5)
    assert torch.equal(y.view(torch.int16), plain.view(torch.int16))
    for i, (m, n, k) in enumerate([(2, 1, 72), (2, 3, 72), (5, 300, 520), (8, 300, 520)]):
        x, w, b = D.inputs(71 + i, m, n, k, t)
        _greedy(x, w, t, dev, what="small")


@pytest.mark.parametrize("t", TYPES)
def test_greedy_pick_bias_alpha_and_minus_inf(dev, t):
    m, n, k = 3, 300, 520
    x, w, b = D.inputs(80, m, n, k, t)
    base, _, _ = _greedy(x, w, t, dev, what="no bias")
    # a bias that moves the winner: 60 on one column that wins nowhere without it (the logits are N(0, 1.1^2))
    col = next(c for c in range(n) if c not in base.tolist())
    bias = D.values(b, t)
    bias[col] = 60.0
    moved, _, _ = _greedy(x, w, t, dev, D.to_bits(bias, t), what="bias moves the winner")
    assert moved.tolist() == [col] * m
    # alpha = -1: the winner is the smallest product
    neg, _, _ = _greedy(x, w, t, dev, None, -1.0, what="alpha -1")
    assert not np.array_equal(neg, base)
    _greedy(x, w, t, dev, b, -1.0, what="alpha -1 with bias")
    # a bias of -inf on every column: every logit is -inf, the pick is index 0
    ninf = D.to_bits(np.full(n, -np.inf), t)
    picks, logits, _ = _greedy(x, w, t, dev, ninf, what="-inf")
    assert np.isneginf(logits).all() and picks.tolist() == [0] * m


@pytest.mark.parametrize("t", TYPES)
def test_greedy_pick_ties_and_nan(dev, t):
    """on the several-rows-per-wave shape: ties inside one wave and across waves far apart keep the first index; a NaN logit wins
    wherever it sits -- the first row of a wave, a later row, two waves at once (the first NaN) -- as in zl_argmax_advance"""
    cus = _cus()
    m, n, k = D.gemv_shapes(cus)["rows_per_wave"][-1]
    rpw = D.gemv_geometry(m, n, k, cus)["rows_per_wave"]
    assert rpw >= 2 and n > rpw * 700 + 1
    x, w, _ = D.inputs(90, m, n, k, t)
    xv = D.values(x, t)
    peak = D.to_bits(0.125 * xv[0], t)                      # a weight row along x[0]: logit 0.125 |x0|^2 ~ 190 in row 0, far above N(0, 2^2)
    nan_row = w[5].copy()
    nan_row[3] = 0x7E00 if t == "f16" else 0x7FC0

    def planted(rows, pattern):
        w2 = w.copy()
        w2[list(rows)] = pattern
        return w2
    # ties: the same weight row twice
    for what, rows in (("tie inside a wave", (rpw * 5, rpw * 5 + 1)), ("tie across far waves", (rpw * 2 + 1, n - 1)),
                       ("tie, later wave first in its thread", (rpw * 300, rpw * 44)), ("three-way tie", (n - 2, rpw * 256, rpw * 700 + 1))):
        picks, logits, _ = _greedy(x, planted(rows, peak), t, dev, what=what)
        assert picks[0] == min(rows) and logits[0, min(rows)] == logits[0, max(rows)] == logits[0].max(), (what, picks)
    # NaN logits (every activation row sees them): the first NaN wins, also over a larger finite peak in another wave
    for what, rows in (("NaN on the first row of a wave", (rpw * 10,)), ("NaN on a later row of a wave", (rpw * 10 + 1,)),
                       ("NaN on the last row of a wave", (rpw * 11 - 1,)), ("NaN in two waves", (rpw * 700 + 1, rpw * 20 + rpw - 1)),
                       ("NaN in the last wave and the first", (n - 1, 1))):
        w2 = planted(rows, nan_row)
        w2[rpw * 3] = peak
        picks, logits, _ = _greedy(x, w2, t, dev, what=what)
        assert np.isnan(logits[:, list(rows)]).all() and picks.tolist() == [min(rows)] * m, (what, picks)


# ---- gemm_nt / gemm_nt_packed ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gemm_data():
    """one (129, 1152) activation and weight matrix per type; the cases are its leading (m, k) / (n, k) corners"""
    out = {}
    for t in TYPES:
        x, w, b = D.inputs(110, max(D.GEMM_M), max(D.GEMM_N), max(D.GEMM_K), t)
        out[t] = (x, w, b)
    return out


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("k", D.GEMM_K)
def test_gemm_nt_tile_edges_odd_chunk_counts(dev, gemm_data, t, k):
    """every m at the 16 / 32 / 64 tile edges from both sides x every n (1 and 15: a tile whose rows are all clamped) at an odd chunk
    count (3, 5, 9: the guarded second ring slot); every (m, n) plain, and with ldx > k, bias and alpha"""
    from zhilight_amd import ops
    assert (k // 128) % 2 == 1 and k // 128 >= 3
    xa, wa, ba = gemm_data[t]
    worst = 0.0
    for m in D.GEMM_M:
        x = np.ascontiguousarray(xa[:m, :k])
        for n in D.GEMM_N:
            w, b = np.ascontiguousarray(wa[:n, :k]), ba[:n]
            s = D.abs_sum(x, w, t)
            for xd, bias, alpha, what in ((_up(x, dev, t), None, 1.0, ""), (_strided(x, dev, t), b, 0.5, "strided bias alpha")):
                wd, bd = _up(w, dev, t), None if bias is None else _up(bias, dev, t)
                y = _abi("zl_gemm_nt", xd, wd, bd, alpha, t) if what else ops.gemm_nt(xd, wd, bd, alpha)
                ex = D.exact(x, w, t, bias, alpha)
                bar = D.bar_rounded(ex, s, alpha, D.mfma_chain(k), t)
                worst = max(worst, D.worst_ratio(_down(y, t), ex, bar, f"gemm_nt {t} {m, n, k} {what}"))
                if m <= 32:
                    wp = ops.DenseMWeight(wd)
                    yp = _abi("zl_gemm_nt_packed", xd, wp, bd, alpha, t) if what else ops.gemm_nt_packed(xd, wp, bd, alpha)
                    assert torch.equal(yp.view(torch.int16), y.view(torch.int16)), ("gemm_nt_packed", t, m, n, k, what)
    _report("gemm_nt", t, f"tile edges k={k}", worst)


@pytest.mark.parametrize("t", TYPES)
def test_gemm_nt_packed_bit_identical_at_odd_chunk_counts(dev, t):
    from zhilight_amd import ops
    for k in (384, 640):
        x, w, b = D.inputs(120 + k, 32, 272, k, t)
        wd, bd = _up(w, dev, t), _up(b, dev, t)
        for n in (1, 15, 272):
            wn = wd[:n].contiguous()
            wp = ops.DenseMWeight(wn)
            for m in (1, 17, 32):
                xd = _up(x[:m], dev, t)
                assert torch.equal(ops.gemm_nt_packed(xd, wp).view(torch.int16), ops.gemm_nt(xd, wn).view(torch.int16)), (t, m, n, k)
                assert torch.equal(ops.gemm_nt_packed(xd, wp, bd[:n], 0.5).view(torch.int16), ops.gemm_nt(xd, wn, bd[:n], 0.5).view(torch.int16)), (t, m, n, k)
            ex = D.exact(x, w[:n], t)
            bar = D.bar_rounded(ex, D.abs_sum(x, w[:n], t), 1.0, D.mfma_chain(k), t)
            D.worst_ratio(_down(ops.gemm_nt_packed(_up(x, dev, t), wp), t), ex, bar, f"gemm_nt_packed {t} {32, n, k}")


# ---- gemm_nt_f32 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_gemm_nt_f32_values(dev, t):
    from zhilight_amd import ops
    worst = 0.0
    for i, (m, n, k) in enumerate(D.F32_SHAPES):
        x, w, _ = D.inputs(130 + i, m, n, k, t, bias=False)
        s = D.abs_sum(x, w, t)
        for alpha in (1.0, 0.37):
            for xd in (_up(x, dev, t), _strided(x, dev, t)):
                wd = _up(w, dev, t)
                y = ops.gemm_nt_f32(xd, wd, alpha) if xd.is_contiguous() else _abi("zl_gemm_nt_f32", xd, wd, None, alpha, t, out_dtype=torch.float32)
                assert y.dtype == torch.float32 and tuple(y.shape) == (m, n)
                ex = D.exact(x, w, t, None, alpha)
                r = D.worst_ratio(y.cpu().numpy().astype(np.float64), ex, D.bar_f32(s, alpha, D.f32_chain(k)), f"gemm_nt_f32 {t} {m, n, k} alpha {alpha}")
                worst = max(worst, r)
    _report("gemm_nt_f32", t, "values", worst)


@pytest.mark.parametrize("t", TYPES)
def test_gemm_nt_f32_routes_tokens_like_the_exact_logits(dev, t):
    """the ranked top-k expert ids moe_top_k_softmax takes from the kernel's logits equal those it takes from the exact logits cast to
    fp32; a token is left out only if its own top k + 1 exact logits have an adjacent gap within twice the shape's largest bar"""
    from zhilight_amd import ops
    for shape, seed, top_k in D.ROUTING:
        x, w = D.routing_inputs(shape, seed, t)
        ex = D.exact(x, w, t)
        bar = D.bar_f32(D.abs_sum(x, w, t), 1.0, D.f32_chain(shape[2]))
        skip = D.routing_skipped(ex, top_k, bar.max())
        assert skip.sum() <= D.ROUTING_MAX_SKIPPED, (shape, int(skip.sum()))
        y = ops.gemm_nt_f32(_up(x, dev, t), _up(w, dev, t))
        r = D.worst_ratio(y.cpu().numpy().astype(np.float64), ex, bar, f"gemm_nt_f32 {t} {shape} routing")
        _, got = ops.moe_top_k_softmax(y, top_k)
        _, want = ops.moe_top_k_softmax(torch.from_numpy(ex.astype(np.float32)).to(dev), top_k)
        got, want = got.cpu().numpy(), want.cpu().numpy()
        assert np.array_equal(want[~skip], D.ranked_top_k(ex.astype(np.float32), top_k)[~skip]), (shape, "the router itself")
        bad = np.nonzero((got != want).any(axis=1) & ~skip)[0]
        assert bad.size == 0, (t, shape, bad.tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())
        print(f"dense_errors: gemm_nt_f32 {t} routing {shape} top-{top_k}: worst |err| / bar {r:.4f}, {int(skip.sum())} of {shape[0]} tokens undecidable, "
              f"the others routed as the exact logits")


def test_gemm_nt_f32_refusals(dev):
    from zhilight_amd import ops
    from zhilight_amd._lib import ZLError
    h = dict(dtype=torch.float16, device=dev)
    with pytest.raises(ZLError):
        ops.gemm_nt_f32(torch.zeros(2, 64, **h), torch.zeros(4, 72, **h))                                   # K mismatch
    with pytest.raises(ZLError):
        ops.gemm_nt_f32(torch.zeros(2, 64, **h), torch.zeros(4, 64, dtype=torch.bfloat16, device=dev))      # dtype mismatch
    with pytest.raises(ZLError):
        ops.gemm_nt_f32(torch.zeros(2, 68, **h), torch.zeros(4, 68, **h))                                   # k % 8 != 0
