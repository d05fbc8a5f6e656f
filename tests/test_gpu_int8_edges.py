"""The INT8 quantisers and W8A8 GEMMs on the inputs of tests/int8_cases.py (ties, zero rows, outliers, subnormals, rounding maxima,
-128 operands) and at the shapes where a launcher changes path, against the CPU oracle -- bit for bit wherever the project claims
that.  tests/test_int8_cases_host.py shows on the CPU that a quantiser with another rounding mode, or with the maximum not reduced
in T, fails on exactly these inputs and that the Gaussian rows of the older tests cannot see it.

The bars that are not bit-equality come from tests/test_gpu_ops.py::test_int8_path_bit_exact: the rmsnorm scale at rtol 3e-7, the
norm output at <= 1 ulp on fewer than 2% of the elements, quant_back_act_mul at <= 1 ulp on fewer than 0.5% of the elements.  Several
shapes here have so few elements that such a share admits none; `_Share` applies the share to every case large enough for the cap
to admit one element and to the pooled elements of each test, and <= 1 ulp to every element.
"""
import numpy as np
import pytest
import torch

import int8_cases as ic
import synth
from test_gpu_kvquant import _empty_cache, _scatter_host
from test_gpu_ops import _bits, _np, _t, _tt

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])
TDT = (torch.float16, torch.bfloat16)


def _same_f32(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class _Share:
    """<= 1 ulp everywhere; fewer than `cap` of the elements differ: per case where cap * size > 1, and over all cases added"""

    def __init__(self, cap):
        self.cap, self.diff, self.total, self.bad = cap, 0, 0, []

    def add(self, got, ref, tag):
        ulp = synth.ulp_diff_f16(got, ref)
        n = int((ulp > 0).sum())
        self.diff += n
        self.total += ulp.size
        if ulp.max() > 1:
            self.bad.append((tag, "ulp", int(ulp.max())))
        elif self.cap * ulp.size > 1 and n >= self.cap * ulp.size:
            self.bad.append((tag, "share", n, ulp.size))

    def check(self, bad=()):
        print(f"{self.diff} of {self.total} elements differ by one ulp")
        assert not self.bad and not bad and self.diff < self.cap * self.total, (self.bad, list(bad), self.diff, self.total)


# ---- a. quant_calc_scale ----------------------------------------------------------------------------------------------------------------
QUANT_K = (8, 24, 100, 2047, 2048, 2056, 14336)       # vector path: under one trip, one trip, one trip + one thread, 7 trips; 100, 2047: scalar


def _quant_rows_case(oracle, ops, dev, xb, dtype, x_dev=None):
    rq, rs = oracle.quant_calc_scale(xb, dtype)
    gq, gs = ops.quant_calc_scale(_tt(xb, dev, dtype) if x_dev is None else x_dev)
    return np.array_equal(_np(gq), rq), _same_f32(_np(gs), rs)


@DT
@pytest.mark.parametrize("name", ic.ROW_PROFILES)
def test_quant_calc_scale_profiles(oracle, dev, name, dtype):
    from zhilight_amd import ops
    bad = []
    for k in QUANT_K:
        for m in (1, 33):
            ok = _quant_rows_case(oracle, ops, dev, ic.rows(name, m, k, dtype), dtype)
            if ok != (True, True):
                bad.append((m, k) + ok)
    assert not bad, bad                                # (m, k, codes equal, scales equal)


@DT
def test_quant_calc_scale_unaligned_view_and_wide_grid(oracle, dev, dtype):
    """K % 8 == 0 but the rows start 8 bytes into an allocation: the scalar instantiation (ops.quant_calc_scale passes the view's own
    pointer, it does not copy); and 70000 rows, a grid beyond 65535 in x"""
    from zhilight_amd import ops
    m, k = 33, 2048
    for name in ("ties_shuffled", "zero_row", "tiny", "gauss"):
        xb = ic.rows(name, m, k, dtype)
        buf = torch.zeros(m * k + 8, dtype=TDT[dtype], device=dev)
        view = buf[4:4 + m * k].view(m, k)
        view.copy_(_tt(xb, dev, dtype))
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        assert _quant_rows_case(oracle, ops, dev, xb, dtype, view) == (True, True), name
    xb = np.tile(np.concatenate([ic.rows(n, 175, 64, dtype) for n in ("ties_shuffled", "zero_row", "one_outlier", "gauss")]), (100, 1))
    assert xb.shape == (70000, 64)
    assert _quant_rows_case(oracle, ops, dev, xb, dtype) == (True, True)


# ---- b. layernorm_quant -----------------------------------------------------------------------------------------------------------------
NORM_PROFILES = ("ties_sorted", "ties_shuffled", "zero_row", "neg_zero_row", "amax_rounds", "one_outlier", "gauss")


@DT
@pytest.mark.parametrize("name", NORM_PROFILES)
def test_layernorm_quant_profiles(oracle, dev, name, dtype):
    """dims: the reference's reduction width is 32, 64, 128 and 1024; 1000 leaves threads without an element; 8184 is the largest vector
    size, 8192 and 16368 take the scalar instantiation by the LDS rule.  ties and one_outlier use weight 1 (the products are the
    inputs; 3e38 times a weight above 1 is not finite)."""
    from zhilight_amd import ops
    rng = np.random.default_rng(ic.seed_of("norm_w", name, dtype))
    share, bad = _Share(0.02), []
    for dim in ic.NORM_DIMS:
        for rows_ in ic.NORM_ROWS:
            top = None
            if name == "amax_rounds":
                xb, wb, _, down = ic.norm_amax_rounds(rows_, dim, dtype, seed=ic.AMAX_SEEDS[("norm", rows_, dim, dtype)])
                top = np.abs(ic.f32(xb, dtype) * ic.f32(wb, dtype)[None, :]).argmax(axis=1)
            else:
                xb = ic.rows(name, rows_, dim, dtype)
                wb = ic.exact_bits(np.ones(dim), dtype) if name.startswith("ties") or name == "one_outlier" else \
                    ic.to_bits(1 + 0.1 * rng.standard_normal(dim), dtype)
            for scale in (1.0, 1.4):
                tag = (dim, rows_, scale)
                ro, rq, rs = oracle.rmsnorm_quant(xb, wb, 1e-5, scale, dtype)
                go, gq, gs = ops.layernorm_quant(_tt(xb, dev, dtype), _tt(wb, dev, dtype), 1e-5, scale)
                gq, gs = _np(gq), _np(gs)
                if not np.array_equal(gq, rq):
                    bad.append((tag, "codes", int((gq != rq).sum())))
                if not np.allclose(gs, rs, rtol=3e-7, atol=0):          # (test_int8_path_bit_exact)
                    bad.append((tag, "scale", gs.tolist(), rs.tolist()))
                share.add(_bits(go), ro, tag)
                if top is not None and scale == 1.0 and not (np.abs(gq[np.arange(rows_), top].astype(np.int32)) == 127).all():
                    bad.append((tag, "the largest element does not code as +-127"))
    share.check(bad)


@DT
def test_layernorm_quant_refuses_a_row_beyond_its_lds(oracle, dev, dtype):
    from zhilight_amd import ops
    x = _tt(ic.rows("gauss", 1, 16376, dtype), dev, dtype)
    with pytest.raises(ops.ZLError):
        ops.layernorm_quant(x, _tt(ic.exact_bits(np.ones(16376), dtype), dev, dtype), 1e-5)


# ---- c. the group-of-32 quantisers ------------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("groups", ic.G32_GROUPS)
def test_group_32_quantisers(oracle, dev, groups, dtype):
    """quant_group_32 / dequant_group_32 / dequant_sum_quant_g32 on the group form of ties, zero groups and sums whose maximum rounds
    in T; 7, 9 and 4097 groups leave a ragged last workgroup of 8"""
    from zhilight_amd import ops
    seed = ic.seed_of("g32", groups, dtype)
    xb = ic.ties_groups(groups, dtype, seed)
    if groups >= 7:
        xb[3], xb[5] = 0, 0x8000                       # a group of +0.0 and one of -0.0: codes 0, scale 0
    rq, rs = oracle.quant_group_32(xb, dtype)
    gq, gs = ops.quant_group_32(_tt(xb, dev, dtype))
    assert np.array_equal(_np(gq), rq) and np.array_equal(_bits(gs), rs)
    if groups >= 7:
        assert not rq[3].any() and not rq[5].any() and rs[3] == 0 and rs[5] == 0
    assert np.array_equal(_bits(ops.dequant_group_32(gq, gs)), oracle.dequant_group_32(rq, rs, dtype))
    for world in ic.G32_WORLDS:
        my, qo, so, sums = ic.g32_ties_case(groups, world, dtype, seed)
        if groups >= 7:
            my[3], my[5], qo[:, 3], qo[:, 5] = 0, 0x8000, 0, 0
        rq, rs = oracle.dequant_sum_quant_g32(my, qo, so, dtype)
        if groups < 7:
            assert np.array_equal(rq, np.rint(sums).astype(np.int8))
        gq, gs = ops.dequant_sum_quant_g32(_tt(my, dev, dtype), _t(qo, dev), _tt(so, dev, dtype))
        assert np.array_equal(_np(gq), rq) and np.array_equal(_bits(gs), rs), ("ties", world)
        my, qo, so, _, down = ic.g32_amax_rounds(groups, world, dtype, seed=ic.AMAX_SEEDS[("g32", groups, world, dtype)])
        rq, rs = oracle.dequant_sum_quant_g32(my, qo, so, dtype)
        gq, gs = ops.dequant_sum_quant_g32(_tt(my, dev, dtype), _t(qo, dev), _tt(so, dev, dtype))
        gq = _np(gq)
        assert np.array_equal(gq, rq) and np.array_equal(_bits(gs), rs), ("amax_rounds", world)
        top = np.abs(ic.g32_sums(my, qo, so, dtype)).argmax(axis=1)
        assert (np.abs(gq[np.arange(groups), top].astype(np.int32)) == 127).all() and down.any()
        assert np.array_equal(_bits(ops.dequant_group_32(_t(rq, dev), _tt(rs, dev, dtype))), oracle.dequant_group_32(rq, rs, dtype))


# ---- d. the INT8 KV cache's quantisers --------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_kv_cache_quantisers_on_ties_zero_rows_and_max_finite(oracle, dev, d, bshd, dtype):
    """quant_calc_scale_zp, quant_copy_to_rag_buffer and rope_quant_scatter_decode (position 0: cos 1, sin 0, the rotation leaves
    every value as it is) against the oracle functions of tests/test_gpu_kvquant.py; ties code as 1 .. 255"""
    from zhilight_amd import ops
    h, hkv, len_q = 2, 2, 2
    lens = [4, 8, 5]
    b = len(lens)
    lens_t = _t(np.array(lens, np.int32), dev)
    for name in ("ties_sorted", "ties_shuffled", "zero_row", "neg_zero_row", "max_finite"):
        xb = ic.rows(name, 33, d, dtype)
        rq, rs = oracle.quant_calc_scale_zp(xb, 128, dtype)
        gq, gs = ops.quant_calc_scale_zp(_tt(xb, dev, dtype))
        assert np.array_equal(_np(gq), rq) and _same_f32(_np(gs), rs), name
        if name.startswith("ties"):
            assert rq.min() >= 1 and rq.max() == 255
        # the plain scatter: (b * len_q, hkv, d) K and V rows
        ksrc = np.roll(ic.rows(name, b * len_q * hkv, d, dtype, seed=1), 1, axis=0).reshape(b * len_q, hkv, d)
        vsrc = np.roll(ic.rows(name, b * len_q * hkv, d, dtype, seed=2), 2, axis=0).reshape(b * len_q, hkv, d)
        placement = np.array([[2, 0], [7, -1], [4, 1]], np.int32)
        host, devt = _empty_cache(lens, hkv, d, bshd, dev)
        kq, ksc = oracle.quant_calc_scale_zp(ksrc.reshape(-1, d), 128, dtype)
        vq, vsc = oracle.quant_calc_scale_zp(vsrc.reshape(-1, d), 128, dtype)
        for bi in range(b):
            for qi in range(len_q):
                for hk in range(hkv):
                    r = ((bi * len_q) + qi) * hkv + hk
                    if placement[bi, qi] >= 0:
                        _scatter_host(host, bi, placement[bi, qi], hk, bshd, kq[r], ksc[r], vq[r], vsc[r])
        ops.quant_copy_to_rag_buffer(_t(placement.reshape(-1), dev), lens_t, _tt(ksrc, dev, dtype), _tt(vsrc, dev, dtype),
                                     *[ops.make_ptr_table(x) for x in devt], len_q=len_q, bshd=bshd)
        for bi in range(b):
            for h_arr, d_arr in zip(host, devt):
                assert np.array_equal(_np(d_arr[bi]).view(np.uint8), h_arr[bi].view(np.uint8)), (name, "copy", bi)
        # the fused rotation + scatter of a decode step, every task at position 0
        qkv = np.roll(ic.rows(name, b * (h + 2 * hkv), d, dtype, seed=3), 2, axis=0).reshape(b, (h + 2 * hkv) * d)
        cs, sn = oracle.rope_cos_sin(np.zeros(b, np.int32), d, 5e5, True)
        assert (cs == 1).all() and (sn == 0).all()
        rq_, rk, rv = oracle.rope_qk_cache(cs, sn, qkv, h, hkv, d, True, dtype)
        if name.startswith("ties") or name == "max_finite":
            assert np.array_equal(rk.reshape(b, -1), qkv[:, h * d:(h + hkv) * d])          # the rotation kept every value
        place1 = np.array([3, -1, 0], np.int32)
        host, devt = _empty_cache(lens, hkv, d, bshd, dev)
        kq, ksc = oracle.quant_calc_scale_zp(rk.reshape(-1, d), 128, dtype)
        vq, vsc = oracle.quant_calc_scale_zp(rv.reshape(-1, d), 128, dtype)
        for bi in range(b):
            for hk in range(hkv):
                if place1[bi] >= 0:
                    _scatter_host(host, bi, place1[bi], hk, bshd, kq[bi * hkv + hk], ksc[bi * hkv + hk], vq[bi * hkv + hk], vsc[bi * hkv + hk])
        gq_ = ops.rope_quant_scatter_decode(_t(cs, dev), _t(sn, dev), _tt(qkv, dev, dtype), _t(place1, dev), lens_t,
                                            *[ops.make_ptr_table(x) for x in devt], h, hkv, d, neox=True, bshd=bshd)
        assert np.array_equal(_bits(gq_), rq_), (name, "rope q")
        for bi in range(b):
            for h_arr, d_arr in zip(host, devt):
                assert np.array_equal(_np(d_arr[bi]).view(np.uint8), h_arr[bi].view(np.uint8)), (name, "rope", bi)


# ---- e. int8_gemm_nt --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "min"])
def test_int8_gemm_full_range_operands_and_tile_edges(oracle, dev, kind):
    """operands over -128 .. 127 (and all -128); K of 1, 2, 3 chunks under the tiled kernel's two-chunk weight prefetch, N below one
    wave's columns, M on both sides of every row-tile edge; the output starts as 0x5a5a5a5a so that an unwritten element shows"""
    from zhilight_amd import ops
    shapes = ic.gemm_shapes()
    assert {s[0] for s in shapes} == set(ic.GEMM_M) and {s[1] for s in shapes} == set(ic.GEMM_N) and {s[2] for s in shapes} == set(ic.GEMM_K)
    bad = []
    for m, n, k in shapes:
        a, b = ic.gemm_operands(m, n, k, kind)
        assert a.min() == -128 and b.min() == -128
        out = torch.full((m, n), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        got = _np(ops.int8_gemm_nt(_t(a, dev), _t(b, dev), out=out))
        ref = oracle.int8_gemm_nt(a, b)
        if not np.array_equal(got, ref):
            bad.append((m, n, k, int((got != ref).sum()), int((got == 0x5a5a5a5a).sum())))
    assert not bad, bad                                # (m, n, k, wrong elements, elements never written)


# ---- f. w8a8_gemm_phase -----------------------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("rounds", [1, 8])
def test_w8a8_phase_epilogues_both_types(oracle, dev, rounds, dtype, monkeypatch):
    """every epilogue of zl_w8a8_gemm_phase in fp16 and bf16 (sy, addend and output in that type), BACK_ADD with scale != 1, the GELU
    gate, K that is no multiple of 128, N of one column: bit-identical to the unfused launchers (as
    test_w8a8_streaming_gemm_bit_identical), and against the oracle's int8_gemm_nt + scale-back -- bit-equal for BACK and BACK_ADD
    (test_int8_path_bit_exact, test_int8_scale_back_variants_bit_exact), the act_mul bar of test_int8_path_bit_exact for the gates"""
    from zhilight_amd import ops
    monkeypatch.setenv("ZL_W8_PHASE_ROUNDS", str(rounds))
    tdt = TDT[dtype]
    shares, bad = {"silu": _Share(5e-3), "gelu": _Share(5e-3)}, []
    for m in ic.W8_M:
        for k, n in ic.W8_KN:
            tag = (m, k, n)
            rng = np.random.default_rng(ic.seed_of("w8", m, k, n, dtype))
            a, w = ic.gemm_operands(m, n, k, "uniform")
            sx = rng.uniform(0.01, 0.05, m).astype(np.float32)
            sy = ic.to_bits(rng.uniform(0.001, 0.01, n), dtype)
            add = ic.to_bits(rng.standard_normal((m, n)), dtype)
            ta, tw, tsx, tsy, tadd = _t(a, dev), _t(w, dev), _t(sx, dev), _tt(sy, dev, dtype), _tt(add, dev, dtype)
            rc = oracle.int8_gemm_nt(a, w)
            c = ops.int8_gemm_nt(ta, tw)
            if not np.array_equal(_np(c), rc):
                bad.append((tag, "int8_gemm_nt"))
            w8 = ops.W8MWeight.from_rows(tw, tsy)
            got = ops.w8a8_gemm_phase(ta, tsx, w8, ops.W8_BACK, dtype=tdt)
            if not torch.equal(got, ops.quant_scale_back(c, tsx, tsy, tdt)):
                bad.append((tag, "BACK vs unfused"))
            if not np.array_equal(_bits(got), oracle.quant_scale_back(rc, sx, sy, dtype)):
                bad.append((tag, "BACK vs oracle"))
            for scale in (1.0, 0.25, 1.4):
                got = ops.w8a8_gemm_phase(ta, tsx, w8, ops.W8_BACK_ADD, addend=tadd, scale=scale, dtype=tdt)
                if not torch.equal(got, ops.quant_back_element_add_scale(c, tsx, tsy, tadd, scale)):
                    bad.append((tag, "BACK_ADD vs unfused", scale))
                if not np.array_equal(_bits(got), oracle.quant_back_element_add_scale(rc, sx, sy, add, scale, dtype)):
                    bad.append((tag, "BACK_ADD vs oracle", scale))
            # the gates: n even, the rows interleaved (gate_n, up_n)
            n2 = n + n % 2
            h2 = n2 // 2
            a, w, sx, sy = ic.gated_case(m, k, n2, dtype)
            ta, tw, tsx, tsy = _t(a, dev), _t(w, dev), _t(sx, dev), _tt(sy, dev, dtype)
            rc = oracle.int8_gemm_nt(a, w)
            c = ops.int8_gemm_nt(ta, tw)
            if not np.array_equal(_np(c), rc):
                bad.append(((m, k, n2), "int8_gemm_nt"))
            w8g = ops.W8MWeight.from_rows(tw, tsy, row_interleave=True)
            for act, epi in (("silu", ops.W8_ACT_SILU), ("gelu", ops.W8_ACT_GELU)):
                got = ops.w8a8_gemm_phase(ta, tsx, w8g, epi, dtype=tdt)
                ref = ops.quant_back_act_mul(c[:, :h2].contiguous(), tsx, tsy[:h2].contiguous(), c[:, h2:].contiguous(), tsx,
                                             tsy[h2:].contiguous(), act, tdt)
                if not torch.equal(got, ref):
                    bad.append(((m, k, n2), act + " vs unfused"))
                shares[act].add(_bits(got), oracle.quant_back_act_mul(rc[:, :h2], sx, sy[:h2], rc[:, h2:], sx, sy[h2:], act, dtype),
                                (m, k, n2, act))
    shares["silu"].check(bad + shares["gelu"].bad)
    shares["gelu"].check()


# ---- g. w8a8_qkv_rope_scatter in bf16 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 17])
@pytest.mark.parametrize("bshd", [True, False])
def test_w8a8_fused_qkv_rotary_scatter_bf16(oracle, dev, m, bshd):
    """the bf16 branches of zl_w8a8_qkv_rope_scatter == zl_w8a8_gemm_phase(BACK, bf16) + zl_rope_scatter_decode, bit for bit (q and
    the K / V buffers), operands incl. -128, one task with placement -1 (test_w8a8_fused_qkv_rotary_scatter_bit_identical is fp16)"""
    from zhilight_amd import ops
    rng = np.random.default_rng(500 + m)
    h, hkv, d, k = 8, 2, 128, 1024 + 256
    n = (h + 2 * hkv) * d
    a, w = ic.gemm_operands(m, n, k, "uniform")
    a, w = _t(a, dev), _t(w, dev)
    sx = _t(rng.uniform(0.002, 0.01, m).astype(np.float32), dev)
    sy = _tt(ic.to_bits(rng.uniform(0.001, 0.004, n), 1), dev, 1)
    w8 = ops.W8MWeight.from_rows(w, sy)
    lens = [int(v) for v in rng.integers(2, 6, m) * 32]
    pos = np.array([int(rng.integers(0, L)) for L in lens], np.int32)
    placement = pos.copy()
    if m > 1:
        placement[1] = -1
    cs, sn = oracle.rope_cos_sin(pos, d, 5e5, True, (8.0, 1.0, 4.0, 8192.0))
    shape = (lambda L: (L, hkv, d)) if bshd else (lambda L: (hkv, L, d))
    mk = lambda: [torch.full(shape(L), 3.0, dtype=torch.bfloat16, device=dev) for L in lens]  # noqa: E731
    k1, v1, k2, v2 = mk(), mk(), mk(), mk()
    lens_t, place_t = _t(np.array(lens, np.int32), dev), _t(placement, dev)
    qkv = ops.w8a8_gemm_phase(a, sx, w8, ops.W8_BACK, dtype=torch.bfloat16)
    q_ref = ops.rope_scatter_decode(_t(cs, dev), _t(sn, dev), qkv, place_t, lens_t, ops.make_ptr_table(k1), ops.make_ptr_table(v1),
                                    h, hkv, d, True, bshd)
    q_got = ops.w8a8_qkv_rope_scatter(a, sx, w8, _t(cs, dev), _t(sn, dev), place_t, lens_t, ops.make_ptr_table(k2),
                                      ops.make_ptr_table(v2), h, hkv, d, bshd=bshd, dtype=torch.bfloat16)
    assert q_got.dtype == torch.bfloat16 and torch.equal(q_got, q_ref)
    for x1, x2 in zip(k1 + v1, k2 + v2):
        assert torch.equal(x1, x2)
    assert not torch.equal(k1[0], torch.full_like(k1[0], 3.0))
    if m > 1:
        assert torch.equal(k2[1], torch.full_like(k2[1], 3.0)) and torch.equal(v2[1], torch.full_like(v2[1], 3.0))


# ---- h. end to end on ties ----------------------------------------------------------------------------------------------------------------
@DT
def test_ties_through_layernorm_quant_and_the_phase_gemm(oracle, dev, dtype):
    """layernorm_quant (and quant_calc_scale) -> w8a8_gemm_phase(BACK) on ties rows == the oracle chain, bit for bit: a rounding-mode
    slip in the quantiser moves most of the 16-bit outputs
    (tests/test_int8_cases_host.py::test_half_away_reaches_the_16_bit_output_of_the_chain)"""
    from zhilight_amd import ops
    x, w1, w8, sy = ic.chain_case(dtype)
    _, rq, rs = oracle.rmsnorm_quant(x, w1, 1e-5, 1.0, dtype)
    ref = oracle.quant_scale_back(oracle.int8_gemm_nt(rq, w8), rs, sy, dtype)
    _, gq, gs = ops.layernorm_quant(_tt(x, dev, dtype), _tt(w1, dev, dtype), 1e-5)
    w8m = ops.W8MWeight.from_rows(_t(w8, dev), _tt(sy, dev, dtype))
    got = ops.w8a8_gemm_phase(gq, gs, w8m, ops.W8_BACK, dtype=TDT[dtype])
    assert np.array_equal(_np(gq), rq), int((_np(gq) != rq).sum())
    assert np.array_equal(_bits(got), ref), int((_bits(got) != ref).sum())
    # the same rows through the layer's other quantiser (no fused norm): quant_calc_scale -> GEMM + scale back
    rq, rs = oracle.quant_calc_scale(x, dtype)
    ref = oracle.quant_scale_back(oracle.int8_gemm_nt(rq, w8), rs, sy, dtype)
    gq, gs = ops.quant_calc_scale(_tt(x, dev, dtype))
    got = ops.w8a8_gemm_phase(gq, gs, w8m, ops.W8_BACK, dtype=TDT[dtype])
    assert np.array_equal(_bits(got), ref), int((_bits(got) != ref).sum())
