"""The numpy reference of the penalised sampling step (tests/penalty_ref.py) against independent statements: `pen` against the
reference kernel's arithmetic IN the logits' type (src/generator/beam_util.cu:212-218: l - T(presence), l * T(value), l / T(value)),
restated in float64 with one rounding -- the exact product, quotient or difference of two 16-bit floats rounded once is the type's own
correctly rounded operation -- over all 65 536 patterns; the sets of a speculative step's rows; the bitmap's pack / unpack."""
import numpy as np
import pytest

import penalty_ref as pr
import sample_ref

PAIRS = [(1.3, 0.0), (1.0, 0.7), (1.3, 0.7), (0.5, 0.0), (1.0, 0.0), (1.3, -0.25), (60000.0, 0.0), (3.1415, 0.0)]


def _round_to_T(x64, bf16):
    with np.errstate(over="ignore"):
        if not bf16:
            return x64.astype(np.float16).view(np.uint16)
        return pr._round16(x64.astype(np.float32), True)       # 24 bits >= 2 * 8 + 2: the intermediate rounding is innocuous


def _in_T(v, bf16):
    return sample_ref.values_of(_round_to_T(np.array([v], np.float64), bf16), bf16)[0]


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("factor,presence", PAIRS)
def test_pen_is_the_reference_kernels_arithmetic(bf16, factor, presence):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    l = sample_ref.values_of(bits, bf16)
    with np.errstate(all="ignore"):
        if presence != 0.0:
            want = l - _in_T(presence, bf16)
        else:
            v = _in_T(factor, bf16)
            want = np.where(l < 0, l * v, l / v)
        want = _round_to_T(want, bf16)
    got = pr.pen(bits, bf16, factor, presence)
    inf = 0x7F80 if bf16 else 0x7C00
    nan_w, nan_g = (want & 0x7FFF) > inf, (got & 0x7FFF) > inf
    assert np.array_equal(nan_w, nan_g)                                                # NaN payloads are not compared
    assert np.array_equal(want[~nan_w], got[~nan_w])
    if (factor, presence) == (1.0, 0.0):                                                # every non-NaN pattern unchanged
        assert np.array_equal(got[~nan_g], bits[~nan_g])


def test_presence_takes_precedence():
    bits = np.array([0x3C00, 0xBC00, 0x0000, 0x4500], np.uint16)
    assert np.array_equal(pr.pen(bits, False, 7.0, 0.5), pr.pen(bits, False, 1.0, 0.5))
    assert not np.array_equal(pr.pen(bits, False, 7.0, 0.0), pr.pen(bits, False, 1.0, 0.0))


def test_row_sets():
    n = 40
    sets = pr.row_sets([[3, 9], []], np.array([[5, -1, 40, 5], [39, 0, 0, 7]]), n)
    assert sets[0] == [[3, 9], [3, 5, 9], [3, 5, 9], [3, 5, 9], [3, 5, 9]]              # -1 and 40 add nothing; a repeat adds nothing
    assert sets[1] == [[], [39], [0, 39], [0, 39], [0, 7, 39]]                          # row 0 sees the task's set alone
    # the last draft is in no row's set: no row follows it
    assert all(7 not in s for s in sets[1][:4])


def test_penalised_rows_touch_the_sets_only():
    rng = np.random.default_rng(3)
    n, b, len_q = 70, 2, 3
    bits = (rng.standard_normal((b * len_q, n)) * 3).astype(np.float16).view(np.uint16)
    seen = pr.pack([[1, 69], [33]], n, ld=4)
    seen[:, 3] = 0xFFFFFFFF                                                             # a whole word above n
    seen[0, 2] |= np.uint32(1 << 7)                                                     # bit 71 >= n
    drafts = np.array([[4, 4], [-1, 2]])
    out = pr.penalised_rows(bits, seen, drafts, False, [1.5, 2.0], [0.0, 0.25])
    want = {0: [1, 69], 1: [1, 4, 69], 2: [1, 4, 69], 3: [33], 4: [33], 5: [2, 33]}
    for r, s in want.items():
        t = r // len_q
        changed = np.flatnonzero(out[r] != bits[r])
        assert set(changed) <= set(s)
        assert np.array_equal(out[r, s], pr.pen(bits[r, s], False, [1.5, 2.0][t], [0.0, 0.25][t]))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 128256])
def test_bitmap_round_trip(n):
    rng = np.random.default_rng(n)
    ids = [np.unique(rng.integers(0, n, min(n, 50))), np.array([n - 1]), np.array([], np.int64), np.array([0, n - 1])]
    seen = pr.pack(ids, n)
    assert seen.shape == (4, pr.words(n)) and seen.dtype == np.uint32
    for got, want in zip(pr.unpack(seen, n), ids):
        assert np.array_equal(got, np.unique(want))
    for t, s in enumerate(ids):                                                         # the layout itself
        for i in s:
            assert seen[t, i >> 5] >> np.uint32(i & 31) & 1
    assert int(sum(bin(int(w)).count("1") for w in seen.reshape(-1))) == sum(np.unique(s).size for s in ids)
    # mark skips what is no class, survives duplicates; a wider row's stray bits are not unpacked
    wide = np.zeros((1, pr.words(n) + 2), np.uint32)
    pr.mark(wide, np.array([[-1, n, n + 5, 0, 0, n - 1, -7]]), n)
    assert np.array_equal(pr.unpack(wide, n)[0], np.unique([0, n - 1]))
    wide[0, -1] = 0xFFFFFFFF
    if n % 32:
        wide[0, (n - 1) >> 5] |= np.uint32(0xFFFFFFFF << (n % 32) & 0xFFFFFFFF)
    assert np.array_equal(pr.unpack(wide, n)[0], np.unique([0, n - 1]))


def test_sample_pen_changes_the_pick_and_records_it():
    """a two-class row: the larger class is in the set and its penalty puts it behind the other"""
    bits = np.array([[2.0, 1.5, -4.0]], np.float16).view(np.uint16)
    T, k, p, u = [0.0], [0], [1.0], [0.0]
    picks, after = pr.sample_pen(bits, False, pr.pack([[]], 3), [2.0], [0.0], T, k, p, u)
    assert picks.tolist() == [0] and pr.unpack(after, 3)[0].tolist() == [0]
    picks, after = pr.sample_pen(bits, False, after, [2.0], [0.0], T, k, p, u)          # 2.0 / 2 = 1.0 < 1.5
    assert picks.tolist() == [1] and pr.unpack(after, 3)[0].tolist() == [0, 1]
    picks, _ = pr.sample_pen(bits, False, after, [2.0], [0.0], T, k, p, u)              # 1.0 > 0.75 > -8
    assert picks.tolist() == [0]
