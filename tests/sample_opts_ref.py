"""numpy statement of the logit bias and the top-N log-probabilities of zl_sample_advance_opts / zl_spec_sample_accept_opts, shared by
test_sample_opts_host.py and test_gpu_sample_opts.py.
`modified_row` is the row the pick sees: the penalty on the classes of the seen set (penalty_ref.pen), then `bias_add` on the classes
of the bias set -- zl_scatter_logits' add expression, fp32 arithmetic on the widened operands and one rounding to the logits' type.
`top_n` is the rule with a sort: the first min(N, n) classes by (key descending, index ascending) and sample_ref.logprob of each.
`top_n_sort_free` restates the kernel's procedure -- the count select on the key's high and low byte, the ties at the N-th place cut
in index order, the gather, the rank of a candidate = the number of candidates in front of it -- and must equal the sort exactly."""
import numpy as np

import penalty_ref as pr
import sample_ref

MAX_BIAS = 1024
MAX_TOP = 32


def bias_add(bits, bf16, bias):
    """T(f32(y) + f32(T(bias))) per element; bias: float32 values, one per element of bits"""
    y = pr._f32_of(bits, bf16)
    tb = pr._f32_of(pr._round16(np.asarray(bias, np.float32), bf16), bf16)
    with np.errstate(all="ignore"):
        return pr._round16((y + tb).astype(np.float32), bf16)


def modified_row(bits, bf16, seen_ids, factor, presence, bias):
    """bits: one row of uint16 patterns; seen_ids: the penalty set (None / empty: no penalty); bias: {id: value} or None -> the row as
    the pick sees it: penalty first, then the bias.  The input is left alone"""
    out = np.array(bits, np.uint16, copy=True)
    s = np.asarray(sorted(set(int(i) for i in seen_ids)) if seen_ids is not None else [], np.int64)
    if s.size:
        out[s] = pr.pen(out[s], bf16, factor, presence)
    if bias:
        ids = np.asarray(sorted(bias), np.int64)
        out[ids] = bias_add(out[ids], bf16, np.asarray([bias[int(i)] for i in ids], np.float32))
    return out


def is_plain_bits(bits, bf16):
    return sample_ref.is_plain(sample_ref.values_of(bits, bf16))


def top_n(bits_modified, bf16, T, N):
    """-> (ids (N) int64, logprobs (N) float64): the first min(N, n) classes of the order (key descending, index ascending) with their
    tempered log-probabilities (T <= 0: at T = 1); -1 / NaN behind them, and everywhere on a plain row"""
    bits = np.asarray(bits_modified, np.uint16)
    n = bits.size
    ids, lps = np.full(N, -1, np.int64), np.full(N, np.nan)
    if is_plain_bits(bits, bf16):
        return ids, lps
    keys = sample_ref.keys_of(bits).astype(np.int64)
    order = np.lexsort((np.arange(n), -keys))[:min(N, n)]
    x = sample_ref.values_of(bits, bf16)
    ids[:order.size] = order
    with np.errstate(all="ignore"):
        lps[:order.size] = [sample_ref.logprob(x, T, int(i)) for i in order]
    return ids, lps


def top_n_sort_free(bits_modified, N):
    """the kernel's selection of the ids on a row that is not plain, without a sort -> ids (min(N, n)) in the order"""
    keys = sample_ref.keys_of(np.asarray(bits_modified, np.uint16)).astype(np.int64)
    n = keys.size
    ne = min(N, n)

    def select(cnt, above, want):
        for b in range(255, -1, -1):
            if above < want <= above + cnt[b]:
                return b, above
            above += cnt[b]
        raise AssertionError("no bin selected")

    b1, ca = select(np.bincount(keys >> 8, minlength=256), 0, ne)
    cnt2 = np.bincount(keys[(keys >> 8) == b1] & 255, minlength=256)
    b2, ca = select(cnt2, ca, ne)
    kn, need = (b1 << 8) | b2, ne - ca
    assert 1 <= need <= cnt2[b2] and ca < N
    last = n                                                        # every class of the key is taken ...
    if need < cnt2[b2]:
        last = int(np.flatnonzero(keys == kn)[need - 1])            # ... or its first `need` in index order
    cand = [i for i in range(n) if keys[i] > kn or (keys[i] == kn and i <= last)]
    assert len(cand) == ne
    cand = cand[::-1]                                               # the arrival order is immaterial
    out = [-1] * ne
    for i in cand:
        rank = sum(1 for j in cand if keys[j] > keys[i] or (keys[j] == keys[i] and j < i))
        out[rank] = i
    return np.asarray(out, np.int64)


# ---- the packed bias of ops.logit_bias_pack ------------------------------------------------------------------------------------------
def pack_bias(maps, n):
    """maps: per task {id: value} or None -> (ids (b, ld) int32 ascending, -1 behind cnt; vals (b, ld) float32; cnt (b) int32;
    bits (b, ceil(n / 32)) uint32), ld = the longest list, at least 1"""
    maps = [m or {} for m in maps]
    ld = max([1] + [len(m) for m in maps])
    ids, vals = np.full((len(maps), ld), -1, np.int32), np.zeros((len(maps), ld), np.float32)
    cnt = np.asarray([len(m) for m in maps], np.int32)
    for t, m in enumerate(maps):
        k = sorted(int(i) for i in m)
        ids[t, :len(k)] = k
        vals[t, :len(k)] = [m[i] for i in k]
    return ids, vals, cnt, pr.pack([sorted(m) for m in maps], n)
