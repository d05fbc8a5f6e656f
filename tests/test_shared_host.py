"""The host side of shared prefixes, no device: the rule of the two-segment decode attention as tests/shared_ref.py states it, the
float32 noise floor the GPU tests' bar rests on, and serving.PrefixPool."""
import numpy as np
import pytest

import shared_ref
from attn_profiles import attend, decode_bar, from_bits, to_bits

D = 128
SCALE = 1.0 / np.sqrt(D)


def _data(rng, caps, buf_lens, hkv, bshd=True, dtype=0):
    """fp16-representable values: prefix and own K / V buffers, NaN nowhere yet"""
    def buf(n):
        shape = (n, hkv, D) if bshd else (hkv, n, D)
        return from_bits(to_bits(rng.standard_normal(shape), dtype), dtype).reshape(shape)
    return [buf(c) for c in caps], [buf(c) for c in caps], [buf(n) for n in buf_lens], [buf(n) for n in buf_lens]


@pytest.mark.parametrize("bshd", [True, False])
def test_shared_ref_is_attend_over_the_concatenated_keys(bshd):
    rng = np.random.default_rng(1)
    h, hkv = 8, 2
    caps, plens, prefix_of = (96, 64), (70, 33), [0, 0, -1, 1, 0]
    valid, buf_lens = [71, 115, 50, 233, 73], [128, 128, 64, 256, 80]
    pk, pv, ok, ov = _data(rng, caps, buf_lens, hkv, bshd)
    q = rng.standard_normal((5, h, D))
    ps = shared_ref.prefix_rows(prefix_of, plens, caps, valid, buf_lens)
    assert ps == [70, 70, 0, 33, 70]
    # poison what the rule says is unread: the reference must not touch it
    rows = (lambda a, lo, hi: a[lo:hi]) if bshd else (lambda a, lo, hi: a[:, lo:hi])
    for g in range(2):
        for a in (pk[g], pv[g]):
            rows(a, plens[g], caps[g])[...] = np.nan
    clean_k, clean_v = [a.copy() for a in ok], [a.copy() for a in ov]
    for b in range(5):
        for a in (ok[b], ov[b]):
            rows(a, 0, ps[b])[...] = np.nan
            rows(a, valid[b], buf_lens[b])[...] = np.nan
    got = shared_ref.shared_attention(q, ok, ov, valid, buf_lens, prefix_of, plens, caps, pk, pv, hkv, SCALE, bshd)
    assert np.isfinite(got).all()
    n_rep = h // hkv
    for b in range(5):
        for hk in range(hkv):
            k = np.concatenate([rows(pk[prefix_of[b]], 0, ps[b])[:, hk] if bshd else pk[prefix_of[b]][hk, :ps[b]],
                                clean_k[b][ps[b]:valid[b], hk] if bshd else clean_k[b][hk, ps[b]:valid[b]]]) if ps[b] else \
                (clean_k[b][:valid[b], hk] if bshd else clean_k[b][hk, :valid[b]])
            v = np.concatenate([pv[prefix_of[b]][:ps[b], hk] if bshd else pv[prefix_of[b]][hk, :ps[b]],
                                clean_v[b][ps[b]:valid[b], hk] if bshd else clean_v[b][hk, ps[b]:valid[b]]]) if ps[b] else \
                (clean_v[b][:valid[b], hk] if bshd else clean_v[b][hk, :valid[b]])
            want = attend(q[b, hk * n_rep:(hk + 1) * n_rep], k, v, np.ones((n_rep, len(k)), bool), SCALE)[0]
            assert np.abs(got[b, hk * n_rep:(hk + 1) * n_rep] - want).max() < 1e-12
    # sharing changes nothing: the same keys in buffers that hold the prefix as a copy
    mk = shared_ref.materialise(ok, valid, buf_lens, prefix_of, plens, caps, pk, bshd)
    mv = shared_ref.materialise(ov, valid, buf_lens, prefix_of, plens, caps, pv, bshd)
    none = shared_ref.shared_attention(q, mk, mv, valid, buf_lens, [-1] * 5, plens, caps, pk, pv, hkv, SCALE, bshd)
    assert np.abs(got - none).max() < 1e-12


def test_the_clamps_of_the_rule():
    caps, plens = (64, 48, 32), (0, 60, 20)
    #          empty prefix  valid == P  g == G  g < 0  own rows  valid == P  valid 0  valid < len  valid > buf
    prefix_of = [0,           1,          3,      -7,    1,        2,          1,       1,           2]
    valid = [40,              48,         33,     20,    90,       20,         0,       30,          70]
    buf_lens = [64,           64,         64,     32,    128,      64,         64,      64,          40]
    assert shared_ref.prefix_rows(prefix_of, plens, caps, valid, buf_lens) == [0, 48, 0, 0, 48, 20, 0, 30, 20]
    assert shared_ref.prefix_rows([0], (50,), (64,), [-3], [64]) == [0] and shared_ref.prefix_rows([0], (-5,), (64,), [9], [64]) == [0]
    rng = np.random.default_rng(2)
    pk, pv, ok, ov = _data(rng, caps, buf_lens, 2)
    q = rng.standard_normal((9, 8, D))
    out = shared_ref.shared_attention(q, ok, ov, valid, buf_lens, prefix_of, plens, caps, pk, pv, 2, SCALE)
    assert not out[6].any() and np.isfinite(out).all()                       # no visible key: a zero row
    # task 1 sees the prefix only, task 8 its prefix and own rows 20 .. 39 (the buffer ends at 40)
    k, v = shared_ref.task_keys(1, 0, ok, ov, valid, buf_lens, prefix_of, plens, caps, pk, pv)
    assert np.array_equal(k, pk[1][:48, 0]) and np.array_equal(v, pv[1][:48, 0])
    k, _ = shared_ref.task_keys(8, 1, ok, ov, valid, buf_lens, prefix_of, plens, caps, pk, pv)
    assert np.array_equal(k, np.concatenate([pk[2][:20, 1], ok[8][20:40, 1]]))
    k, _ = shared_ref.task_keys(3, 1, ok, ov, valid, buf_lens, prefix_of, plens, caps, pk, pv)
    assert np.array_equal(k, ok[3][:20, 1])


@pytest.mark.parametrize("dtype", [0, 1])
def test_float32_noise_floor_is_well_below_the_bar(dtype):
    """a float32 restatement of the two-segment merge (records per split of either segment, one merge) on the GPU tests' data: below 0.4
    of decode_bar, which the kernel tests hold the kernel to -- a short, a many-member and a several-splits shape"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for caps, plens, valid, buf_lens in (((96,), (70,), [71, 115, 128], [128] * 3), ((1152,), (1100,), [1101, 1164, 1800], [2048] * 3)):
        hkv, h = 2, 8
        pk, pv, ok, ov = _data(rng, caps, buf_lens, hkv, dtype=dtype)
        q = from_bits(to_bits(rng.standard_normal((3, h, D)), dtype), dtype).reshape(3, h, D)
        exact = shared_ref.shared_attention(q, ok, ov, valid, buf_lens, [0] * 3, plens, caps, pk, pv, hkv, SCALE)
        for b in range(3):
            for hk in range(hkv):
                rows = q[b, hk * 4:(hk + 1) * 4]
                got = shared_ref.restate_f32(rows, pk[0][:plens[0], hk], pv[0][:plens[0], hk], ok[b][plens[0]:valid[b], hk],
                                             ov[b][plens[0]:valid[b], hk], SCALE)
                # through the output's rounding to T, as the kernel's rows
                got = from_bits(to_bits(got, dtype), dtype).reshape(got.shape)
                worst = max(worst, np.abs(got - exact[b, hk * 4:(hk + 1) * 4]).max() / decode_bar(exact, dtype))
    assert worst < 0.4, worst


def test_prefix_pool():
    from zhilight_amd import ops
    from zhilight_amd.serving import SHARE_MIN_ROWS, SHARE_PAIR_MAX_ROWS, PrefixPool
    big = PrefixPool(1, 2 * SHARE_PAIR_MAX_ROWS)                             # a pair goes back to copying from SHARE_PAIR_MAX_ROWS rows on
    assert big.take_group(SHARE_PAIR_MAX_ROWS, members=2) is None and big.take_group(SHARE_MIN_ROWS - 1, members=3) is None
    assert big.take_group(SHARE_PAIR_MAX_ROWS - 1, members=2) == 0 and big.release([0]) == [] and big.free() == []
    big = PrefixPool(1, 2 * SHARE_PAIR_MAX_ROWS)
    assert big.take_group(SHARE_PAIR_MAX_ROWS, members=3) == 0
    pool = PrefixPool(2, 64)
    assert pool.free() == [0, 1]
    assert pool.pin(0) is None and pool.pin(65) is None                     # rows a buffer cannot hold
    h = pool.pin(50)
    assert h == 0 and pool.lens[0] == 50 and pool.free() == [1]
    pool.attach(h, [3, 5])
    assert pool.users(h) == [3, 5] and not pool.drop(h)                      # read by slots: refused
    assert pool.release([3]) == [] and not pool.drop(h)
    assert pool.release([5]) == [] and h in pool.pinned                      # a pinned buffer outlives its readers
    assert pool.drop(h) and not pool.drop(h) and pool.free() == [0, 1] and pool.lens[0] == 0
    # a group's buffer: free again only when the LAST slot was parked or re-admitted
    assert pool.take_group(40, min_rows=41) is None and pool.take_group(65, min_rows=1) is None
    assert pool.take_group(SHARE_MIN_ROWS - 1) is None                       # the default threshold
    g = pool.take_group(40, min_rows=8)
    assert g == 0 and pool.free() == [1]
    pool.attach(g, [0, 1, 2])
    assert pool.release([1]) == [] and pool.release([7]) == [] and g in pool.group
    h = pool.pin(10)
    assert h == 1 and pool.take_group(40, min_rows=8) is None                # none free: the copying route
    assert pool.release([0, 2]) == [g] and pool.free() == [0] and pool.users(g) == []
    assert pool.take_group(40, min_rows=8) == 0
    with pytest.raises(ops.ZLError):
        PrefixPool(2, 64).attach(1, [0])                                     # neither pinned nor a group's
