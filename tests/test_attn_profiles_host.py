"""CPU checks behind tests/test_gpu_attn_profiles.py (no GPU):

  (a) the CPU oracle's exact attention (oracle.mqa_rag_buffer(exact=True), oracle.mla_decode_attn(flavour="E")) agrees with the plain
      numpy fp64 softmax of tests/attn_profiles.py on every score profile -- the reference itself subtracts its maximum correctly
      at scores of +-60 and with finite data behind the mask;
  (b) the GPU tests use every kernel's EXISTING bar: on every profile, workload and dtype they run, a float32 restatement of the
      attention (attn_profiles.attend in float32, unrounded output) stays within a quarter of the bar's absolute term, so a correct
      fp32 kernel has room.  The oracle's own fp32 route (mqa_rag_buffer without exact) returns T bits: it is checked to sit within
      that noise plus one output rounding;
  (c) a float32 online-softmax restatement (chunks of 32, splits of 128) with one switch per kernel defect: every defect exceeds the
      kernel bar on at least one profile in fp16 and in bf16, the unmutated restatement passes all of them -- and the "last visible
      key dropped" defect PASSES the bf16 bar on the i.i.d. data of test_decode_attention_matrix_core_path at 1025 visible keys:
      what the flat data cannot see.
"""
import numpy as np
import pytest

import attn_profiles as ap

SMALL_LENS, SMALL_VALID = [640, 640, 640], [33, 517, 640]


def _ulp(dtype):
    return 2.0 ** (-7 if dtype else -10)


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ap.PROFILES)
def test_oracle_agrees_with_plain_numpy(oracle, name, dtype):
    rng = np.random.default_rng(ap.seed_of("host_a", name, dtype))
    d, h, hkv = 128, 8, 2
    for holes in (False, True):
        c = ap.build_decode(name, rng, SMALL_LENS, SMALL_VALID, h, hkv, d, 2, dtype, 1.0 / np.sqrt(d), holes=holes)
        for bshd in (True, False):
            k = c.k if bshd else [np.ascontiguousarray(np.moveaxis(a, 1, 0)) for a in c.k]
            v = c.v if bshd else [np.ascontiguousarray(np.moveaxis(a, 1, 0)) for a in c.v]
            exact = oracle.mqa_rag_buffer(c.q, np.array(SMALL_LENS, np.int32), k, v, c.mask, hkv, c.scale, bshd, dtype=dtype, exact=True)
            assert np.abs(exact - c.ref).max() <= 1e-6, np.abs(exact - c.ref).max()
    if name == "equal":                                        # the normaliser: the mean of the visible V rows
        for u in c.units:
            want = np.stack([u["v"][u["vis"][r]].mean(0) for r in range(u["q"].shape[0])])
            assert np.abs(c.ref[u["where"]].reshape(want.shape) - want).max() <= 1e-12
    # the INT8 cache's exact oracle on the rows quantised by the project's quantiser
    cq = ap.build_decode(name, rng, SMALL_LENS, SMALL_VALID, h, hkv, d, 1, dtype, 1.0 / np.sqrt(d), quant=lambda x: oracle.quant_calc_scale_zp(x, dtype=dtype))
    eq = oracle.mqa_rag_buffer_quant(cq.q, np.array(SMALL_LENS, np.int32), cq.k, cq.v, cq.ks, cq.vs, cq.mask, hkv, cq.scale, True, dtype=dtype)
    assert np.abs(eq - cq.ref).max() <= 1e-6 * max(1.0, np.abs(cq.ref).max()), np.abs(eq - cq.ref).max()
    # MLA, flavour E: the fp64 statement rounded once to T
    m = ap.build_mla(name, rng, 320, [1, 65, 300], 8, dtype, ap.MLA_SCALE)
    E = ap.from_bits(oracle.mla_decode_attn(m.q, [320] * 3, m.vis_lens, m.kv, scale=ap.MLA_SCALE, dtype=dtype, flavour="E"), dtype)
    assert (np.abs(E - m.ref) <= 0.5 * _ulp(dtype) * np.abs(m.ref) * (1 + 1e-6) + 1e-7).all(), np.abs(E - m.ref).max()


def _noise32(case):
    r32 = case.restate(lambda q, k, v, vis: ap.attend(q, k, v, vis, case.scale, np.float32)[0])
    return np.abs(r32 - case.ref).max()


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ap.PROFILES)
def test_fp32_noise_is_a_quarter_of_the_decode_bars(oracle, name, dtype):
    """every decode workload of the GPU tests: the fp16 / bf16 cache routes, the half-record route and the INT8 cache"""
    quant = lambda x: oracle.quant_calc_scale_zp(x, dtype=dtype)
    for geom in ap.DECODE_GEOMS:
        c = ap.decode_case(geom, name, dtype)
        n32 = _noise32(c)
        assert n32 <= 0.25 * ap.decode_bar(c.ref, dtype), (geom, n32)
        assert n32 <= 0.25 * ap.half_record_bar(c.ref)
        if geom in ("h8", "h16_q4"):                           # the oracle's own fp32 route: T bits
            d, h, hkv, len_q, _ = ap.DECODE_GEOMS[geom]
            o32 = ap.from_bits(oracle.mqa_rag_buffer(c.q, np.array(c.buf_lens, np.int32), c.k, c.v, c.mask, hkv, c.scale, True, dtype=dtype), dtype)
            assert (np.abs(o32 - c.ref) <= 0.5 * _ulp(dtype) * np.abs(c.ref) + 0.25 * ap.decode_bar(c.ref, dtype)).all()
    for geom in ("d64", "d64_holes", "h8", "h16_q4"):
        if geom != "d64" and geom != "d64_holes" and dtype:
            continue                                           # the matrix-core INT8 kernel is fp16 only
        c = ap.decode_case(geom, name, dtype, quant=quant)
        assert _noise32(c) <= 0.25 * ap.decode_bar(c.ref, dtype), geom
    if name in ("stairs", "late_spike"):
        for geom in ("h8", "h8_holes"):
            c = ap.decode_case(geom, name, dtype, long=True)
            assert _noise32(c) <= 0.25 * ap.decode_bar(c.ref, dtype), geom


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ap.PROFILES)
def test_fp32_noise_is_a_quarter_of_the_prefill_and_mla_bars(name, dtype):
    for geom in ap.PREFILL_GEOMS:
        c = ap.prefill_case(geom, name, dtype)
        assert _noise32(c) <= 0.25 * ap.prefill_bar(c.ref, dtype), geom
    for geom in ap.MLA_GEOMS:
        c = ap.mla_case(geom, name, dtype)
        assert _noise32(c) <= 0.25 * 2e-5 * np.abs(c.ref).max(), geom


def _mutant_table(dtype):
    """{mutant or None: {profile: max|restatement - fp64| / bar}} on the (8, 2, 1) decode workload"""
    table = {}
    for mutant in (None,) + ap.MUTANTS:
        row = {}
        for name in ap.PROFILES:
            c = ap.decode_case("h8", name, dtype)
            got = c.restate(lambda q, k, v, vis: ap.online_softmax(q, k, v, vis, c.scale, mutant))
            err = np.abs(got - c.ref).max() if np.isfinite(got).all() else np.inf
            row[name] = err / ap.decode_bar(c.ref, dtype)
        table[mutant] = row
    return table


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])
def test_every_defect_exceeds_the_bar_on_some_profile(dtype):
    table = _mutant_table(dtype)
    print("\n".join(f"{str(m):18s} " + " ".join(f"{n}={r:.3g}" for n, r in row.items()) for m, row in table.items()))
    assert max(table[None].values()) < 1.0, table[None]        # the restatement itself passes every profile
    for mutant in ap.MUTANTS:
        assert max(table[mutant].values()) > 1.0, (mutant, table[mutant])
    # and each defect is seen by the profile built for it
    assert table["drop_last"]["late_spike"] > 1.0 and table["no_rescale"]["rise"] > 1.0 and table["hidden_in_max"]["hidden_spike"] > 1.0
    assert table["no_max"]["offset_pos"] > 1.0 and table["no_max"]["offset_neg"] > 1.0
    assert table["merge_no_max"]["stairs"] > 1.0 and table["lane_skip"]["sparse_spikes"] > 1.0


def test_flat_data_does_not_see_a_dropped_last_key():
    """the data of test_decode_attention_matrix_core_path[bf16, bshd, (32, 8, 1)] (rng 33, i.i.d. normals), its task with 1025 visible
    keys of 1088: the online softmax that skips key 1024 is inside the bf16 bar -- a fact about the OLD data, recorded here"""
    rng = np.random.default_rng(33)
    d, h, hkv = 128, 32, 8
    lens = [64, 64, 64, 160, 160, 160, 1088, 1088, 640]
    valid = [1, 31, 33, 127, 128, 129, 1025, 517, 640]
    kb, vb = [], []
    for L in lens:
        kb.append(ap.to_bits(rng.standard_normal((L, hkv, d)), 1))
        vb.append(ap.to_bits(rng.standard_normal((L, hkv, d)), 1))
    q = ap.to_bits(rng.standard_normal((len(lens), 1, h, d)), 1)
    t, scale = valid.index(1025), 1.0 / np.sqrt(d)
    worst, top = 0.0, 1.0
    for bi, (L, n) in enumerate(zip(lens, valid)):             # the old test's bar: 5e-3 of max(1, max|exact|) over ALL nine tasks
        K, V, Q = ap.from_bits(kb[bi], 1), ap.from_bits(vb[bi], 1), ap.from_bits(q[bi, 0], 1)
        vis = np.broadcast_to(np.arange(L) < n, (h // hkv, L))
        for hk in range(hkv):
            uq = Q[hk * 4:(hk + 1) * 4]
            exact, _ = ap.attend(uq, K[:, hk], V[:, hk], vis, scale)
            top = max(top, np.abs(exact).max())
            if bi == t:
                bad = ap.online_softmax(uq, K[:, hk], V[:, hk], vis, scale, "drop_last")
                good = ap.online_softmax(uq, K[:, hk], V[:, hk], vis, scale)
                assert np.abs(good - exact).max() < 1e-5
                worst = max(worst, np.abs(bad - exact).max())
    print("last key dropped at 1025 flat keys:", worst, "bar", 5e-3 * top)
    assert 0.0 < worst < 5e-3 * top, (worst, top)
