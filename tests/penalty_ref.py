"""numpy statement of the penalties of zl_sample_advance_ex / zl_spec_sample_accept_ex / zl_seen_mark, shared by
test_sample_penalty_host.py and test_gpu_sample_penalty.py: the per-task bitmap (token i = bit i & 31 of word i >> 5), `pen` on 16-bit
patterns (zl_repetition_penalty's expression: fp32 arithmetic on the widened operands, one rounding to the logits' type), the sets of
the rows of a speculative step, and the penalised calls composed from sample_ref / spec_sample_ref: penalise the rows, then the
existing rule, unchanged."""
import numpy as np

import sample_ref
import spec_sample_ref


# ---- the bitmap ---------------------------------------------------------------------------------------------------------------------
def words(n):
    return (int(n) + 31) // 32


def mark(seen, tokens, n):
    """set the bits of the ids of tokens (b, n_tok) that lie in [0, n) in seen (b, ld) uint32, in place; others are skipped"""
    tokens = np.asarray(tokens, np.int64).reshape(seen.shape[0], -1)
    for t, row in enumerate(tokens):
        ids = row[(row >= 0) & (row < n)]
        np.bitwise_or.at(seen[t], ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))      # .at: duplicates inside one word
    return seen


def pack(sets, n, ld=None):
    """sets: per task an iterable of ids in [0, n) -> (b, ld) uint32, ld = ceil(n / 32) by default"""
    ld = words(n) if ld is None else ld
    assert ld >= words(n)
    seen = np.zeros((len(sets), ld), np.uint32)
    for t, s in enumerate(sets):
        s = np.asarray(sorted(s), np.int64)
        assert s.size == 0 or (s.min() >= 0 and s.max() < n)
        mark(seen[t:t + 1], s.reshape(1, -1), n)
    return seen


def unpack(seen, n):
    """(b, ld) uint32 -> per task the sorted ids below n whose bit is set; bits at or above n are not classes"""
    seen = np.asarray(seen, np.uint32)
    out = []
    for row in seen:
        bits = ((row[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).reshape(-1)[:n]
        out.append(np.flatnonzero(bits).astype(np.int64))
    return out


# ---- pen ----------------------------------------------------------------------------------------------------------------------------
def _f32_of(bits, bf16):
    bits = np.asarray(bits, np.uint16)
    if bf16:
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float16).astype(np.float32)


def _round16(x, bf16):
    """float32 -> the 16-bit pattern, round to nearest even; a NaN stays a NaN (the payload is not specified)"""
    x = np.asarray(x, np.float32)
    if not bf16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def pen(bits, bf16, factor, presence):
    """the penalised pattern of every element of bits: presence != 0 ? l - T(presence) : (l < 0 ? l * T(factor) : l / T(factor)),
    evaluated in float32 on the widened operands, rounded once to T"""
    l = _f32_of(bits, bf16)
    with np.errstate(all="ignore"):
        if np.float32(presence) != 0:
            tp = _f32_of(_round16(np.float32(presence), bf16), bf16)
            r = l - tp
        else:
            f = _f32_of(_round16(np.float32(factor), bf16), bf16)
            r = np.where(l < 0, l * f, l / f)
        return _round16(r.astype(np.float32), bf16)


# ---- the sets of a speculative step ---------------------------------------------------------------------------------------------------
def row_sets(seen_ids, drafts, n):
    """seen_ids: per task its ids; drafts (b, K) -> sets[t][i], i = 0 .. K: the task's ids and the drafts j < i that lie in [0, n) (row i
    counts only if they were emitted).  Row 0 sees the task's set alone"""
    drafts = np.asarray(drafts, np.int64)
    out = []
    for t, ids in enumerate(seen_ids):
        base = set(int(i) for i in ids)
        rows = []
        for i in range(drafts.shape[1] + 1):
            rows.append(sorted(base | {int(d) for d in drafts[t, :i] if 0 <= d < n}))
        out.append(rows)
    return out


def penalised_rows(bits, seen, drafts, bf16, factor, presence):
    """bits (b * len_q, n) uint16 task-major, seen (b, ld) uint32, drafts (b, len_q - 1) or None (len_q = 1), factor / presence per task
    -> a penalised copy"""
    bits = np.asarray(bits, np.uint16)
    n = bits.shape[1]
    b = seen.shape[0]
    len_q = bits.shape[0] // b
    ids = unpack(seen, n)
    sets = row_sets(ids, np.zeros((b, 0), np.int64) if drafts is None else drafts, n)
    out = bits.copy()
    for t in range(b):
        for i in range(len_q):
            s = np.asarray(sets[t][i], np.int64)
            if s.size:
                out[t * len_q + i, s] = pen(bits[t * len_q + i, s], bf16, factor[t], presence[t])
    return out


# ---- the penalised calls --------------------------------------------------------------------------------------------------------------
def sample_pen(bits, bf16, seen, factor, presence, T, top_k, top_p, u):
    """zl_sample_advance_ex per row: (picks, seen afterwards) -- sample_ref.sample on the penalised rows' values"""
    rows = penalised_rows(bits, seen, None, bf16, factor, presence)
    picks = np.array([sample_ref.sample(sample_ref.values_of(rows[r], bf16), T[r], int(top_k[r]), top_p[r], u[r])[0]
                      for r in range(rows.shape[0])], np.int64)
    after = mark(np.array(seen, np.uint32, copy=True), picks.reshape(-1, 1), bits.shape[1])
    return picks, after


def spec_sample_pen(bits, bf16, seen, drafts, factor, presence, T, top_k, top_p, **kw):
    """zl_spec_sample_accept_ex: spec_sample_ref.spec_sample on the penalised rows; adds "seen": the bitmap plus the emitted tokens"""
    rows = penalised_rows(bits, seen, drafts, bf16, factor, presence)
    res = spec_sample_ref.spec_sample(sample_ref.values_of(rows.reshape(-1), bf16).reshape(rows.shape), drafts, T, top_k, top_p, **kw)
    res["seen"] = mark(np.array(seen, np.uint32, copy=True), res["out_tokens"], bits.shape[1])
    return res
