"""Host-side checks of the logit bias and the top-N log-probabilities of the sampling step (no GPU): the sort-free restatement of the
kernel's count select and ordered gather against the sort, the bias add's rounding against an exact add with one rounding, and the
refusals of ops.logit_bias_pack's host half."""
import math

import numpy as np
import pytest

import penalty_ref as pr
import sample_opts_ref as so
import sample_ref


def _rows(rng, count, n, bf16):
    """random rows with few distinct values (ties everywhere) and with many"""
    out = []
    for r in range(count):
        x = rng.normal(0, 3, n) if r % 2 else rng.integers(-4, 5, n) * 0.5
        x = x.astype(np.float32)
        out.append(pr._round16(x, bf16))
    return out


def edge_rows(n, N, bf16=False):
    """the rows the gather can get wrong, as float32 values: all equal; a run of equal values across the N-th place; the N-th class
    alone in its high-byte bin; +-0.0"""
    rows = [np.full(n, 1.5, np.float32)]
    x = np.linspace(-3, -1, n).astype(np.float32)
    x[::3] = 2.0                                                       # the run: every third class, far more than N of them
    if n > 2:
        x[n // 2] = 4.0
    rows.append(x)
    x = np.linspace(-3, -2, n).astype(np.float32)
    x[:min(N, n)] = 2.0 ** (np.arange(min(N, n)) * 0.5)                # distinct values, one or two per high-byte bin
    rows.append(x)
    x = np.where(np.arange(n) % 2, 0.0, -0.0).astype(np.float32)
    if n > 3:
        x[3] = -1.0
    rows.append(x)
    return [pr._round16(r, bf16) for r in rows]


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
def test_sort_free_top_n_equals_the_sort(bf16):
    rng = np.random.default_rng(5 + bf16)
    checked = 0
    for n in (1, 2, 7, 33, 300):
        for N in (1, 5, 32):
            rows = _rows(rng, 8, n, bf16) + edge_rows(n, N, bf16)
            for bits in rows:
                ids, lps = so.top_n(bits, bf16, 0.7, N)
                got = so.top_n_sort_free(bits, N)
                ne = min(N, n)
                assert np.array_equal(ids[:ne], got), (n, N)
                assert (ids[ne:] == -1).all() and np.isnan(lps[ne:]).all() and np.isfinite(lps[:ne]).all()
                assert (np.diff(lps[:ne]) <= 0).all()
                checked += 1
    assert checked >= 150


def test_top_n_edge_rows():
    bits = pr._round16(np.full(40, 0.25, np.float32), False)
    assert so.top_n(bits, False, 1.0, 5)[0].tolist() == [0, 1, 2, 3, 4]                  # all equal: the lowest indices
    z = pr._round16(np.array([0.0, -0.0, -0.0, 0.0], np.float32), False)
    assert so.top_n(z, False, 1.0, 3)[0].tolist() == [0, 1, 2]                           # -0.0 and +0.0 are one value
    assert so.top_n(z, False, 1.0, 32)[0].tolist() == [0, 1, 2, 3] + [-1] * 28           # N > n
    for bad in (np.nan, np.inf):
        x = np.linspace(-1, 1, 9).astype(np.float32)
        x[4] = bad
        ids, lps = so.top_n(pr._round16(x, False), False, 1.0, 4)
        assert (ids == -1).all() and np.isnan(lps).all()
    ids, lps = so.top_n(pr._round16(np.full(9, -np.inf, np.float32), False), False, 1.0, 4)
    assert (ids == -1).all() and np.isnan(lps).all()
    # T <= 0: the log-probabilities are taken at T = 1
    x = pr._round16(np.linspace(-2, 2, 17).astype(np.float32), True)
    assert np.array_equal(so.top_n(x, True, 0.0, 5)[1], so.top_n(x, True, 1.0, 5)[1])
    # the pick's log-probability is its entry's
    assert so.top_n(x, True, 0.7, 5)[1][0] == sample_ref.logprob(sample_ref.values_of(x, True), 0.7, 16)


def _round_exact(v, bf16):
    """a float64 -> the nearest value of the 16-bit type, ties to even, in one rounding (normal range, no overflow)"""
    if v == 0 or not math.isfinite(v):
        return v
    m, e = math.frexp(v)                                               # v = m 2^e, 0.5 <= |m| < 1
    p = 8 if bf16 else 11
    if not bf16 and e - 1 < -14:                                       # fp16 subnormals: a fixed grid of 2^-24
        return round(v / 2.0 ** -24) * 2.0 ** -24                      # Python rounds halves to even
    return math.ldexp(round(math.ldexp(m, p)), e - p)


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
def test_bias_add_is_one_rounding_of_the_exact_sum(bf16):
    """y and T(bias) are 16-bit values, so their fp32 sum rounds once more to 16 bits; fp32's 24 bits are at least twice the type's
    plus two, which makes that double rounding the single rounding of the exact sum"""
    rng = np.random.default_rng(21 + bf16)
    y = pr._round16((rng.normal(0, 1, 4000) * 2.0 ** rng.integers(-12, 8, 4000)).astype(np.float32), bf16)
    bias = (rng.normal(0, 1, 4000) * 2.0 ** rng.integers(-12, 8, 4000)).astype(np.float32)
    bias[:500] = -pr._f32_of(y[:500], bf16) * (1 + 2.0 ** -rng.integers(1, 12, 500))      # cancellation
    got = sample_ref.values_of(so.bias_add(y, bf16, bias), bf16)
    yv = sample_ref.values_of(y, bf16)
    bv = sample_ref.values_of(pr._round16(bias, bf16), bf16)
    want = np.array([_round_exact(float(a) + float(b), bf16) for a, b in zip(yv, bv)])   # the float64 sum of two such values is exact
    assert np.array_equal(got, want)
    # -inf bans, 0 leaves the class (up to -0.0 + 0.0), and the bias is rounded to the type first
    assert np.isneginf(sample_ref.values_of(so.bias_add(y[:8], bf16, np.full(8, -np.inf, np.float32)), bf16)).all()
    assert np.array_equal(sample_ref.values_of(so.bias_add(y[:8], bf16, np.zeros(8, np.float32)), bf16), yv[:8])


def test_modified_row_order_is_penalty_then_bias():
    bits = pr._round16(np.array([2.0, -2.0, 1.0, 3.0], np.float32), False)
    row = so.modified_row(bits, False, [0, 1], 2.0, 0.0, {1: 0.5, 2: -1.0, 3: -np.inf})
    assert sample_ref.values_of(row, False).tolist() == [1.0, -3.5, 0.0, -np.inf]        # (-2 * 2) + 0.5, not (-2 + 0.5) * 2
    assert sample_ref.values_of(bits, False).tolist() == [2.0, -2.0, 1.0, 3.0]           # the input stays
    assert np.array_equal(so.modified_row(bits, False, None, 1.0, 0.0, None), bits)


def test_logit_bias_rows_layout_and_refusals():
    from zhilight_amd import ops
    ids, vals, cnt, bits = ops.logit_bias_rows([{40: 1.5, 3: -np.inf, 32: 0.0}, None, {}], 41)
    assert ids.dtype == np.int32 and vals.dtype == np.float32 and cnt.dtype == np.int32 and bits.dtype == np.uint32
    assert ids.tolist() == [[3, 32, 40], [-1, -1, -1], [-1, -1, -1]] and cnt.tolist() == [3, 0, 0]
    assert vals[0].tolist() == [-np.inf, 0.0, 1.5] and bits.shape == (3, 2)
    assert [s.tolist() for s in pr.unpack(bits, 41)] == [[3, 32, 40], [], []]
    want = so.pack_bias([{40: 1.5, 3: -np.inf, 32: 0.0}, None, {}], 41)
    for a, b in zip((ids, vals, cnt, bits), want):
        assert np.array_equal(a, b)
    assert ops.logit_bias_rows([None], 5)[0].shape == (1, 1)                            # never a zero-width list
    full = {i: 0.25 for i in range(1024)}
    assert ops.logit_bias_rows([full], 2000)[2].tolist() == [1024]
    for maps, n, what in (([{1: 0.5, "1": 0.25}], 8, "given twice"), ([{1: 0.5, 1.5: 0.1}], 8, "given twice"),
                          ([{8: 0.5}], 8, "outside"), ([{-1: 0.5}], 8, "outside"), ([{**full, 1024: 0.0}], 2000, "at most 1024"),
                          ([{1: float("nan")}], 8, "not NaN"), ([{1: float("inf")}], 8, "not NaN"),
                          ([{1: 1e39}], 8, "float32's range"), ([{1: -1e39}], 8, "float32's range"),
                          ([[1, 2]], 8, "one dict"), ([{1: "x"}], 8, "integer ids")):
        with pytest.raises(ops.ZLError, match=what):
            ops.logit_bias_rows(maps, n)
