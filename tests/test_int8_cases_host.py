"""CPU checks behind tests/test_gpu_int8_edges.py (no GPU):

  (a) every profile of tests/int8_cases.py decodes to the values it promises, in fp16 and bf16; the ties ARE ties under the oracle's
      own arithmetic (x * bs has fraction exactly 0.5);
  (b) the numpy restatements of the five quantisers equal the CPU oracle bit for bit on every profile, so their mutants are mutants of
      the oracle's arithmetic;
  (c) each profile discriminates: round-half-away and truncation differ from the oracle on `ties` (all five quantisers), the amax taken
      without its rounding to T differs on `amax_rounds` (rmsnorm_quant, dequant_sum_quant_g32) -- and half-away does NOT differ on
      `gauss`: what the old data could not see;
  (d) the zero-row contract: codes 0 (q_zero) and scale 0 from all five oracle quantisers;
  (e) the end-to-end chain rmsnorm_quant -> int8 GEMM -> scale back on `ties` rows: the half-away mutant changes the 16-bit OUTPUT;
  (f) the gated scale-back inputs of the GPU test: where the oracle's float32 formula and its fp64 evaluation round to different T
      values is counted, so that a share-cap miss on the GPU can be told from an input the oracle itself is unsure about.
"""
import numpy as np
import pytest

import int8_cases as ic

DT = pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])


def _frac_is_half(v):
    return np.array_equal(np.abs(v - np.trunc(v)), np.full(v.shape, 0.5, v.dtype))


@DT
@pytest.mark.parametrize("k", [8, 100, 256, 2047])
def test_ties_rows_decode_and_are_ties(oracle, dtype, k):
    m = 33
    for shuffled in (False, True):
        xb = ic.ties_rows(m, k, dtype, 5, shuffled)
        x = ic.f32(xb, dtype)
        assert np.array_equal(np.abs(x).max(axis=1), np.full(m, 127, np.float32))
        assert (x.max(axis=1) == 127).all() and (x.min(axis=1) == -127).all()
        t = x[np.abs(x) != 127]
        assert t.size == m * (k - 2) and _frac_is_half(t)
        if m * (k - 2) >= 254:
            assert np.array_equal(np.unique(t), ic.TIES.astype(np.float32))      # every j = -127 .. 126
        if not shuffled:
            assert (np.diff(x, axis=1) >= 0).all()
        # under the oracle's arithmetic: bs = 127.f / amax == 1.0f, x * bs is the tie itself; the oracle rounds it to the even neighbour
        bs = np.float32(127) / np.abs(x).max(axis=1)
        assert np.array_equal(bs, np.ones(m, np.float32))
        q, s = oracle.quant_calc_scale(xb, dtype)
        assert np.array_equal(s, np.ones(m, np.float32))
        assert np.array_equal(q, np.rint(x).astype(np.int8)) and (q[np.abs(x) != 127] % 2 == 0).all()
        qz, _ = oracle.quant_calc_scale_zp(xb, 128, dtype)
        assert qz.min() >= 1 and qz.max() == 255 and np.array_equal(qz.astype(np.int32) - 128, q)


@DT
def test_ties_groups_cover_every_tie(oracle, dtype):
    xb = ic.ties_groups(9, dtype, 3)
    x = ic.f32(xb, dtype)
    assert x.shape == (9, 32) and np.array_equal(np.abs(x).max(axis=1), np.full(9, 127, np.float32))
    t = x[np.abs(x) != 127]
    assert t.size == 270 and _frac_is_half(t) and np.array_equal(np.unique(t), ic.TIES.astype(np.float32))
    # v * 127.0f / amax under the oracle's arithmetic: the product is exact (15 bits), the quotient is the tie
    assert np.array_equal((x * np.float32(127)) / np.float32(127), x)
    q, s = oracle.quant_group_32(xb, dtype)
    assert np.array_equal(q, np.rint(x).astype(np.int8)) and np.array_equal(ic.f32(s, dtype), np.ones(9, np.float32))
    for world in ic.G32_WORLDS:
        my, qo, so, sums = ic.g32_ties_case(9, world, dtype, 3)
        assert np.array_equal(sums, x)
        q2, s2 = oracle.dequant_sum_quant_g32(my, qo, so, dtype)
        assert np.array_equal(q2, q) and np.array_equal(s2, s)


@DT
def test_other_profiles_decode(dtype):
    m, k = 5, 100
    for name in ("zero_row", "neg_zero_row"):
        xb = ic.rows(name, m, k, dtype)
        assert (xb[1] == (0x8000 if name == "neg_zero_row" else 0)).all()
        assert all((ic.f32(xb[r], dtype) != 0).any() for r in (0, 2))            # between two ordinary rows
        assert (ic.rows(name, 1, k, dtype)[0] == xb[1]).all()
    x = ic.f32(ic.rows("one_outlier", m, k, dtype), dtype)
    big = np.abs(x) > 1e3
    assert (big.sum(axis=1) == 1).all() and (x[big] == np.float32(60000.0 if dtype == 0 else ic.from_bits(ic.to_bits(np.array([3e38]), 1), 1)[0])).all()
    xb = ic.rows("tiny", 6, k, dtype)
    x = ic.f32(xb, dtype)
    assert (x != 0).all() and np.abs(x).max() <= 255 * 2.0 ** -24
    if dtype == 0:
        assert ((xb & 0x7C00) == 0).all()                                         # subnormal in fp16
    assert np.abs(x[0]).max() / 127 < 3e-9 and np.float32(127) / np.abs(x[0]).max() > 7e8
    x = ic.f32(ic.rows("max_finite", m, k, dtype), dtype)
    assert np.isfinite(x).all() and (np.abs(x) == np.float32(ic.MAX_FINITE[dtype])).all() and (x > 0).any() and (x < 0).any()
    nxt = ic.to_bits(np.array([np.inf]), dtype)[0] - 1                            # the pattern below +inf
    assert ic.from_bits(np.array([nxt], np.uint16), dtype)[0] == ic.MAX_FINITE[dtype]
    for name in ic.ROW_PROFILES:                                                  # seeded: the same call gives the same bits
        assert np.array_equal(ic.rows(name, 3, 24, dtype), ic.rows(name, 3, 24, dtype))
        assert np.isfinite(ic.f32(ic.rows(name, 3, 24, dtype), dtype)).all()


@DT
def test_numpy_restatements_equal_the_oracle(oracle, dtype):
    for name in ic.ROW_PROFILES:
        for m, k in ((5, 100), (3, 256)):
            xb = ic.rows(name, m, k, dtype)
            for got, want in ((ic.np_quant_rows(xb, dtype), oracle.quant_calc_scale(xb, dtype)),
                              (ic.np_quant_rows(xb, dtype, q_zero=128), oracle.quant_calc_scale_zp(xb, 128, dtype))):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        if name in ("max_finite", "one_outlier"):
            continue                                                              # v * 127.0f overflows fp32 in bf16: not a g32 input
        xb = ic.rows(name, 8, 32, dtype)
        got, want = ic.np_quant_group_32(xb, dtype), oracle.quant_group_32(xb, dtype)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    for rows_, dim in ((5, 100), (1, 1032)):
        x, w, _, _ = ic.norm_amax_rounds(rows_, dim, dtype)
        for scale in (1.0, 1.4):
            assert np.array_equal(ic.np_rmsnorm_quant_codes(x, w, scale, dtype)[0], oracle.rmsnorm_quant(x, w, 1e-5, scale, dtype)[1])
    for world in ic.G32_WORLDS:
        my, q, sc, _, _ = ic.g32_amax_rounds(9, world, dtype)
        got, want = ic.np_dequant_sum_quant_g32(my, q, sc, dtype), oracle.dequant_sum_quant_g32(my, q, sc, dtype)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _differs(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


def _both_mutants_caught(quant, ref, ties):
    """quant(rounding) -> codes.  Every tie is moved by exactly one of the two mutants: half-away moves j + 0.5 for even j >= 0 and odd
    j < 0 (128 of the 254 ties), truncation the other 126.  Returns the two counts."""
    away, trunc = _differs(quant("away"), ref), _differs(quant("trunc"), ref)
    assert away + trunc == ties and min(away, trunc) >= 0.49 * ties, (away, trunc, ties)
    assert not ((quant("away") != ref) & (quant("trunc") != ref)).any()
    return away, trunc


@DT
def test_rounding_mutants_differ_on_ties_and_half_away_hides_on_gauss(oracle, dtype):
    """how many codes each rounding mutant moves on `ties`, per quantiser; on `gauss` half-away moves none"""
    m, k = 33, 256
    for name in ("ties_sorted", "ties_shuffled"):
        xb = ic.rows(name, m, k, dtype)
        ties = m * (k - 2)
        q = oracle.quant_calc_scale(xb, dtype)[0]
        assert _both_mutants_caught(lambda r: ic.np_quant_rows(xb, dtype, r)[0], q, ties) == (128 * m, 126 * m)     # 4224 + 4158 of 8382
        qz = oracle.quant_calc_scale_zp(xb, 128, dtype)[0]
        assert _both_mutants_caught(lambda r: ic.np_quant_rows(xb, dtype, r, 128)[0], qz, ties) == (128 * m, 126 * m)
        w1 = ic.exact_bits(np.ones(k), dtype)
        qn = oracle.rmsnorm_quant(xb, w1, 1e-5, 1.0, dtype)[1]
        assert np.array_equal(qn, q)                                              # weight 1, scale 1: the products are the inputs
        assert _both_mutants_caught(lambda r: ic.np_rmsnorm_quant_codes(xb, w1, 1.0, dtype, r)[0], qn, ties) == (128 * m, 126 * m)
    gb = ic.ties_groups(9, dtype, 3)                                              # 270 ties: all 254 and j = -127 .. -112 again
    qg = oracle.quant_group_32(gb, dtype)[0]
    assert _both_mutants_caught(lambda r: ic.np_quant_group_32(gb, dtype, r)[0], qg, 270) == (136, 134)
    my, qo, so, _ = ic.g32_ties_case(9, 4, dtype, 3)
    qs = oracle.dequant_sum_quant_g32(my, qo, so, dtype)[0]
    assert _both_mutants_caught(lambda r: ic.np_dequant_sum_quant_g32(my, qo, so, dtype, r)[0], qs, 270) == (136, 134)
    # the control: on today's data (the rows of test_int8_path_bit_exact's family, 33 x 4096) half-away moves NOTHING
    xb = ic.rows("gauss", 33, 4096, dtype)
    assert _differs(ic.np_quant_rows(xb, dtype, "away")[0], oracle.quant_calc_scale(xb, dtype)[0]) == 0
    assert _differs(ic.np_quant_rows(xb, dtype, "away", 128)[0], oracle.quant_calc_scale_zp(xb, 128, dtype)[0]) == 0
    assert _differs(ic.np_quant_rows(xb, dtype, "trunc")[0], oracle.quant_calc_scale(xb, dtype)[0]) > 33 * 4096 // 3   # truncation it does see


@DT
def test_amax_mutant_differs_on_amax_rounds(oracle, dtype):
    """the amax taken WITHOUT its rounding to T: the codes move on the rows / groups whose maximum rounds (counts printed with -s),
    and the largest element of a rounded-down row codes as +-127, never +-128"""
    moved = {}
    for rows_, dim in ((5, 4096), (5, 1000)):
        x, w, seed, down = ic.norm_amax_rounds(rows_, dim, dtype)
        q = oracle.rmsnorm_quant(x, w, 1e-5, 1.0, dtype)[1]
        mut, amax32 = ic.np_rmsnorm_quant_codes(x, w, 1.0, dtype, round_amax=False)
        p = np.abs(ic.f32(x, dtype) * ic.f32(w, dtype)[None, :])
        top = p.argmax(axis=1)
        assert (np.abs(q[np.arange(rows_), top].astype(np.int32)) == 127).all()
        assert (np.float32(127) * (amax32 / ic.round_T(amax32, dtype)))[down].min() > 127          # the largest lands above 127 ...
        assert (np.abs(q.astype(np.int32)) <= 127).all()                                            # ... and nothing reaches 128
        moved[("norm", rows_, dim)] = n = _differs(mut, q)
        assert n > 0 and (mut != q)[down].any(), (rows_, dim, seed, n)
    for world in ic.G32_WORLDS:
        my, qo, so, seed, down = ic.g32_amax_rounds(4097, world, dtype)
        q = oracle.dequant_sum_quant_g32(my, qo, so, dtype)[0]
        mut = ic.np_dequant_sum_quant_g32(my, qo, so, dtype, round_amax=False)[0]
        s = np.abs(ic.g32_sums(my, qo, so, dtype))
        assert (np.abs(q[np.arange(4097), s.argmax(axis=1)].astype(np.int32)) == 127).all() and (np.abs(q.astype(np.int32)) <= 127).all()
        moved[("g32", world)] = n = _differs(mut, q)
        assert n > 0 and (mut != q)[down].any(), (world, seed, n)
    print("codes moved by the unrounded-amax mutant:", moved)


def test_recorded_amax_seeds_are_what_the_search_finds():
    found = {}
    for dtype in (0, 1):
        for rows_ in ic.NORM_ROWS:
            for dim in ic.NORM_DIMS:
                found[("norm", rows_, dim, dtype)] = ic.norm_amax_rounds(rows_, dim, dtype)[2]
        for groups in ic.G32_GROUPS:
            for world in ic.G32_WORLDS:
                found[("g32", groups, world, dtype)] = ic.g32_amax_rounds(groups, world, dtype)[3]
    assert found == ic.AMAX_SEEDS, found


@DT
def test_zero_row_contract_of_the_five_oracle_quantisers(oracle, dtype):
    for name, pattern in (("zero_row", 0), ("neg_zero_row", 0x8000)):
        for m in (1, 5):
            xb = ic.rows(name, m, 40, dtype)
            z = min(1, m - 1)
            q, s = oracle.quant_calc_scale(xb, dtype)
            assert not q[z].any() and s[z] == 0 and np.isfinite(s).all()
            qz, sz = oracle.quant_calc_scale_zp(xb, 128, dtype)
            assert (qz[z] == 128).all() and sz[z] == 0
            w = ic.to_bits(1 + 0.1 * np.random.default_rng(0).standard_normal(40), dtype)
            for scale in (1.0, 1.4):
                o, qn, sn = oracle.rmsnorm_quant(xb, w, 1e-5, scale, dtype)
                assert not qn[z].any() and sn[z] == 0 and not (o[z] & 0x7FFF).any()
            if m > 1:                                                             # nothing moves on the rows around it
                keep = [r for r in range(m) if r != z]
                assert np.array_equal(q[keep], oracle.quant_calc_scale(xb[keep], dtype)[0])
        gb = ic.rows("gauss", 3, 32, dtype)
        gb[1] = pattern
        q, s = oracle.quant_group_32(gb, dtype)
        assert not q[1].any() and s[1] == 0 and q[0].any() and q[2].any()
        qo, so = np.zeros((3, 3, 32), np.int8), np.zeros((3, 3), np.uint16)
        q, s = oracle.dequant_sum_quant_g32(gb, qo, so, dtype)
        assert not q[1].any() and s[1] == 0 and q[0].any()


@DT
def test_half_away_reaches_the_16_bit_output_of_the_chain(oracle, dtype):
    x, w1, w8, sy = ic.chain_case(dtype)
    _, q, s = oracle.rmsnorm_quant(x, w1, 1e-5, 1.0, dtype)
    out = oracle.quant_scale_back(oracle.int8_gemm_nt(q, w8), s, sy, dtype)
    q_away = ic.np_rmsnorm_quant_codes(x, w1, 1.0, dtype, "away")[0]
    assert _differs(q_away, q) >= 0.49 * 5 * 1022
    out_away = oracle.quant_scale_back(oracle.int8_gemm_nt(q_away, w8), s, sy, dtype)
    n = _differs(out_away, out)
    assert n > out.size // 2, n                                                   # most of the 240 outputs move
    q, s = oracle.quant_calc_scale(x, dtype)                                      # the route without the fused norm
    out = oracle.quant_scale_back(oracle.int8_gemm_nt(q, w8), s, sy, dtype)
    out_away = oracle.quant_scale_back(oracle.int8_gemm_nt(ic.np_quant_rows(x, dtype, "away")[0], w8), s, sy, dtype)
    assert _differs(out_away, out) > out.size // 2


@DT
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_oracle_act_mul_against_fp64_on_the_gated_cases(oracle, dtype, act):
    """over the gated cases of the GPU test: the oracle's float32 formula is within 1 ulp of the fp64 evaluation everywhere and
    differs on fewer than 0.5% of the pooled elements (the cap of test_int8_path_bit_exact) -- the input leaves a correct fp32
    kernel room"""
    import synth
    diff = total = 0
    for m in ic.W8_M:
        for k, n in ic.W8_KN:
            n += n % 2
            a, w, sx, sy = ic.gated_case(m, k, n, dtype)
            c = oracle.int8_gemm_nt(a, w)
            h = n // 2
            ref = oracle.quant_back_act_mul(c[:, :h], sx, sy[:h], c[:, h:], sx, sy[h:], act, dtype)
            ulp = synth.ulp_diff_f16(ref, ic.act_mul_f64(c[:, :h], c[:, h:], sx, sy[:h], sy[h:], act, dtype))
            assert ulp.max() <= 1, (m, k, n)
            diff += int((ulp > 0).sum())
            total += ulp.size
    print(f"oracle vs fp64, {act}: {diff} of {total} elements differ")
    assert diff < 5e-3 * total, (diff, total)
