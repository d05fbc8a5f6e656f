"""Logit bias and top-N log-probabilities inside the device sampling step: zl_sample_advance_opts / zl_spec_sample_accept_opts and
LLaMA.new_sampler(logit_bias=, top_logprobs=).  The bias's bar is EQUALITY with what the project already had -- ops.repetition_penalty
over the set on a copy of the logits, then ops.scatter_logits(add=True), then the existing call on the copy: both paths run the same
arithmetic on the same 16-bit patterns, so every result is compared bit for bit.  The top-N ids are integers selected on patterns and
must EQUAL the stable sort of the modified row (sample_opts_ref.top_n); their log-probabilities are held to the pick's bar."""
import ctypes as C

import numpy as np
import pytest
import torch

import penalty_ref as pr
import sample_opts_ref as so
import sample_ref
import test_gpu_sample as ts
import test_gpu_sample_penalty as tp
import test_gpu_spec_verify as sv
from test_gpu_prefill_batch import _gptq_model
from test_sample_opts_host import edge_rows
from test_score_host import bound

pytestmark = pytest.mark.gpu

NS = [1, 7, 33, 1025, 4097, 128256]
KINDS = ["push", "lift", "both", "ban", "zero", "many", "edges"]
_np, _same, _bits = sv._np, tp._same, tp._bits


def _to(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)


def _bias_dev(maps, n, dev, extra=0):
    """so.pack_bias on the device (int32 storage of the bitmap, `extra` words of junk behind a row's ceil(n / 32))"""
    ids, vals, cnt, bits = so.pack_bias(maps, n)
    if extra:
        bits = np.concatenate([bits, np.full((bits.shape[0], extra), 0xDEADBEEF, np.uint32)], axis=1)
    return (_to(ids, np.int32, dev), _to(vals, np.float32, dev), _to(cnt, np.int32, dev), tp._seen_dev(bits, dev))


def _scatter_bias(ops, buf2d, maps, dev):
    """ops.scatter_logits(add=True) of maps[r] onto row r of buf2d (rows, ld) contiguous"""
    maps = maps or []
    tok = [i for m in maps for i in sorted(m or {})]
    if not tok:
        return
    bid = [r for r, m in enumerate(maps) for _ in (m or {})]
    val = [(m or {})[i] for m in maps for i in sorted(m or {})]
    ops.scatter_logits(_to(val, np.float32, dev), _to(tok, np.int32, dev), _to(bid, np.int32, dev), buf2d, add=True)


def _maps(kind, rng, bits, bf16, n, sets):
    """per row a bias map of the kind; sets[r] = the row's penalty set (for "both")"""
    out = []
    for r in range(bits.shape[0]):
        am = sample_ref.argmax(sample_ref.values_of(bits[r], bf16))
        j = int(rng.integers(0, n))
        if kind == "push":
            m = {am: -40.0}                                            # the stored arg-max falls below the rest
        elif kind == "lift":
            m = {j: 60.0}                                              # an id becomes the arg-max
        elif kind == "both":
            m = {int(sets[r][0]): 3.5, j: -1.25} if len(sets[r]) else {j: -1.25}       # in seen AND biased
        elif kind == "ban":
            m = {am: -np.inf, j: -np.inf}
        elif kind == "zero":
            m = {am: 0.0, j: 0.0}
        elif kind == "many":
            ids = rng.choice(n, min(n, 1024), replace=False)
            m = {int(i): float(v) for i, v in zip(ids, rng.normal(0, 2, ids.size))}
        else:                                                          # the unaligned head and tail of the row
            m = {int(i): float(1.0 + i % 3) for i in {0, min(1, n - 1), max(n - 2, 0), n - 1}}
        out.append(m)
    return out


def _three_paths(ops, dev, bits, ld, bf16, sets, factor, presence, seen, maps, T, k, p, u, top_n=0, bits_extra=0):
    """the one call on the raw rows against repetition_penalty + scatter_logits(add) + the plain call on a copy; seen None: no penalty.
    -> (fused outputs, three-launch outputs, seen afterwards or None, top ids, top logprobs, the modified rows as patterns)"""
    rows, n = bits.shape
    flat_a, raw = ts._logits_dev(bits, ld, bf16, dev)
    flat_b, copy = ts._logits_dev(bits, ld, bf16, dev)
    before = flat_a.clone()
    buf = flat_b[:rows * ld].view(rows, ld)
    if seen is not None:
        tp._penalise(ops, buf, sets, factor, presence, dev)
    _scatter_bias(ops, buf, maps, dev)
    par = dict(temperature=_to(T, np.float32, dev), top_k=_to(k, np.int32, dev), top_p=_to(p, np.float32, dev), u=_to(u, np.float32, dev))
    three, one = tp._Out(rows, dev), tp._Out(rows, dev)
    ops.sample_advance(copy, **par, **three.kw)
    kw = {}
    seen_dev = None
    if seen is not None:
        seen_dev = tp._seen_dev(seen, dev)
        kw.update(rep_penalty=_to(factor, np.float32, dev), presence=_to(presence, np.float32, dev), seen=seen_dev)
    if maps is not None:
        kw["bias"] = _bias_dev(maps, n, dev, bits_extra)
    ti = tl = None
    if top_n:
        ti = torch.full((rows, top_n), -7, dtype=torch.int32, device=dev)
        tl = torch.full((rows, top_n), -77.0, dtype=torch.float32, device=dev)
        kw.update(top_n=top_n, top_ids=ti, top_logprobs=tl)
    ops.sample_advance(raw, **par, **one.kw, **kw)
    torch.cuda.synchronize()
    _same(flat_a, before, "the raw logits")
    modified = _np(copy.contiguous().view(torch.int16)).view(np.uint16)
    return one, three, (tp._seen_np(seen_dev) if seen is not None else None), ti, tl, modified


def _row_params(rows):
    r = np.arange(rows)
    return np.where(r & 1, 0.0, 0.7), np.where(r & 2, 5, 0), np.where(r & 1, 1.0, 0.9)


# ---- 1. the bias: the kernel against repetition_penalty + scatter_logits + sample_advance -------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("n", NS)
def test_kernel_equals_penalty_bias_then_sample(dev, n, bf16):
    from zhilight_amd import ops
    rng = np.random.default_rng(13 * n + bf16)
    moved = banned = 0
    for ki, kind in enumerate(KINDS):
        for rows in (1, 3):
            for ld in (n, n + 3):
                bits = ts._make_rows(rng, rows, n, bf16, shift=ki)
                T, k, p = _row_params(rows)
                if rows == 1:
                    T, k, p = np.array([0.7 if ki & 1 else 0.0]), np.array([5 if ki & 2 else 0]), np.array([0.9])
                u = rng.random(rows).astype(np.float32)
                sets = [np.unique(rng.integers(0, n, max(1, n // 100))) for _ in range(rows)]
                factor = np.array([tp.PENS[(j + ki) % 5][0] for j in range(rows)], np.float32)
                presence = np.array([tp.PENS[(j + ki) % 5][1] for j in range(rows)], np.float32)
                maps = _maps(kind, rng, bits, bf16, n, sets)
                for with_seen in (True, False):
                    seen = pr.pack(sets, n, ld=pr.words(n) + 1) if with_seen else None
                    one, three, after, _, _, modified = _three_paths(ops, dev, bits, ld, bf16, sets, factor, presence, seen, maps, T, k, p, u,
                                                                     bits_extra=ki % 2)
                    for name in tp._Out.NAMES:
                        _same(one.kw[name], three.kw[name], (kind, rows, ld, with_seen, name))
                    picks = _np(one.kw["tokens"]).astype(np.int64)
                    assert picks.min() >= 0 and picks.max() < n
                    if with_seen:                                      # the picks enter seen, the bias entries do not
                        assert np.array_equal(after, pr.mark(seen.copy(), picks.reshape(-1, 1), n)), (kind, rows, ld)
                    for r in range(rows):                              # the copy is sample_opts_ref's modified row
                        want = so.modified_row(bits[r], bf16, sets[r] if with_seen else None, factor[r], presence[r], maps[r])
                        assert np.array_equal(modified[r], want), (kind, r)
                        am = sample_ref.argmax(sample_ref.values_of(bits[r], bf16))
                        if kind in ("push", "lift") and not T[r] > 0:
                            moved += int(picks[r] != am)
                        if kind == "ban" and n > 2 and not sample_ref.is_plain(sample_ref.values_of(want, bf16)):
                            assert picks[r] not in maps[r], (kind, r)
                            banned += 1
    if n >= 33:
        assert moved > 0 and banned > 0                                # the bias did reach the arg-max, and bans were exercised


def test_inconsistent_bias_inputs(dev):
    """a bias bit without a list entry reads the class unbiased; a list entry without a bit is ignored; a count beyond bias_ld is
    clamped to the list; bits at or above n are not classes"""
    from zhilight_amd import ops
    n, rows = 70, 2
    rng = np.random.default_rng(3)
    bits = ts._make_rows(rng, rows, n, False)
    am = [sample_ref.argmax(sample_ref.values_of(bits[r], False)) for r in range(rows)]
    ids, vals, cnt, bb = so.pack_bias([{am[0]: -50.0, 5: 1.0}, {am[1]: -50.0}], n)
    bb[0, 5 >> 5] &= ~np.uint32(1 << 5)                                # row 0: entry 5 without its bit
    bb[1, 9 >> 5] |= np.uint32(1 << 9)                                 # row 1: bit 9 without an entry
    bb[:, (n - 1) >> 5] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    cnt[0] = 1000                                                      # beyond bias_ld = 2: clamped to row 0's two entries
    bias = (_to(ids, np.int32, dev), _to(vals, np.float32, dev), _to(cnt, np.int32, dev), tp._seen_dev(bb, dev))
    _, raw = ts._logits_dev(bits, n + 3, False, dev)
    tok = torch.zeros(rows, dtype=torch.int32, device=dev)
    f32 = lambda v: torch.full((rows,), v, dtype=torch.float32, device=dev)             # noqa: E731
    ops.sample_advance(raw, f32(0.0), torch.zeros(rows, dtype=torch.int32, device=dev), f32(1.0), u=f32(0.5), tokens=tok, bias=bias)
    for r in range(rows):
        want = so.modified_row(bits[r], False, None, 1.0, 0.0, {am[r]: -50.0})
        assert int(tok[r]) == sample_ref.argmax(sample_ref.values_of(want, False)) != am[r]


# ---- 2. top-N -------------------------------------------------------------------------------------------------------------------------
def _check_top(bits_mod, bf16, T, N, ti, tl, picks, lps, what):
    """ids EQUAL the sort; log-probabilities within test_gpu_sample.py:157's bar for the pick's, fin * 2 * eps_t + bound(n): the value
    is read at the type's precision, the log-sum-exp is fp32 over stored logits (test_score_host.bound); the pick's entry bit-equal"""
    eps_t = 2.0 ** -8 if bf16 else 2.0 ** -11
    ti, tl = _np(ti), _np(tl)
    for r in range(bits_mod.shape[0]):
        ids, ref = so.top_n(bits_mod[r], bf16, T[r], N)
        assert np.array_equal(ti[r], ids), what + (r, ti[r].tolist(), ids.tolist())
        live = ids >= 0
        assert np.isnan(tl[r][~live]).all(), what + (r,)
        if live.any():
            x = sample_ref.values_of(bits_mod[r], bf16)
            fin = np.abs(x[np.isfinite(x)]).max()
            with np.errstate(invalid="ignore"):
                err = np.abs(tl[r][live].astype(np.float64) - ref[live])
            err[np.isneginf(ref[live]) & np.isneginf(tl[r][live])] = 0.0
            assert (err <= fin * 2 * eps_t + bound(x.size)).all(), what + (r, float(err.max()))
            at = np.flatnonzero(ids == picks[r])
            if at.size and lps is not None:
                assert tl[r][at[0]].view(np.int32) == lps[r].view(np.int32), what + (r, "the pick's entry")


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("n", NS)
def test_top_n_equals_the_sorted_row(dev, n, bf16):
    from zhilight_amd import ops
    rng = np.random.default_rng(17 * n + bf16)
    for N in (1, 5, 32):
        for rows, ld in ((1, n), (1, n + 3), (3, n), (3, n + 3)):
            for mode in ("plain", "pen+bias", "bias"):
                bits = ts._make_rows(rng, rows, n, bf16, shift=N)
                T, k, p = _row_params(rows)
                u = rng.random(rows).astype(np.float32)
                sets = [np.unique(rng.integers(0, n, max(1, n // 50))) for _ in range(rows)]
                factor, presence = np.full(rows, 1.4, np.float32), np.array([0.0, 0.6, 0.0][:rows], np.float32)
                maps = _maps("many" if N == 5 else "lift", rng, bits, bf16, n, sets) if mode != "plain" else None
                seen = pr.pack(sets, n) if mode == "pen+bias" else None
                one, three, _, ti, tl, modified = _three_paths(ops, dev, bits, ld, bf16, sets, factor, presence, seen, maps, T, k, p, u, top_n=N)
                for name in tp._Out.NAMES:
                    _same(one.kw[name], three.kw[name], (N, rows, mode, name))
                _check_top(modified, bf16, T, N, ti, tl, _np(one.kw["tokens"]), _np(one.kw["logprobs"]), (n, N, rows, mode))


def _top_call(ops, dev, bits, bf16, T, N, k=0, logprobs=True, ld=None):
    rows, n = bits.shape
    _, raw = ts._logits_dev(bits, ld or n + 3, bf16, dev)
    f32 = lambda v: _to(np.broadcast_to(np.asarray(v, np.float32), (rows,)), np.float32, dev)   # noqa: E731
    tok = torch.zeros(rows, dtype=torch.int32, device=dev)
    lp = torch.full((rows,), -77.0, dtype=torch.float32, device=dev) if logprobs else None
    ti = torch.full((rows, N), -7, dtype=torch.int32, device=dev)
    tl = torch.full((rows, N), -77.0, dtype=torch.float32, device=dev)
    ops.sample_advance(raw, f32(T), _to(np.full(rows, k), np.int32, dev), f32(1.0), u=f32(0.37), tokens=tok, logprobs=lp, top_n=N, top_ids=ti,
                       top_logprobs=tl)
    torch.cuda.synchronize()
    return ti, tl, _np(tok), (_np(lp) if logprobs else None)


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
def test_top_n_rows_built_to_break_the_gather(dev, bf16):
    from zhilight_amd import ops
    for n in (7, 33, 4097, 20011):
        for N in (1, 5, 32):
            rows = edge_rows(n, N, bf16)
            # a run of equal values at the N-th place across the head / body / tail pieces and the wave pieces of the body
            x = np.linspace(-3, -1, n).astype(np.float32)
            x[[i for i in (0, 2, 9, n // 16 + 3, n // 16 + 4, n // 2, n - 9, n - 2, n - 1) if 0 <= i < n]] = 2.0
            x[1 % n] = 5.0
            rows.append(pr._round16(x, bf16))
            # the N-th class sharing its high-byte bin with top-k's k-th (k = N + 2: neighbours of one run of close values)
            x = np.linspace(-3, -1, n).astype(np.float32)
            x[:min(n, 40)] = 1.0 + np.arange(min(n, 40)) * 2.0 ** -7
            rows.append(pr._round16(x, bf16))
            bits = np.stack(rows)
            for T, k, lp in ((0.7, 0, True), (0.7, N + 2, True), (0.0, 0, False), (0.0, 0, True)):
                ti, tl, tok, lps = _top_call(ops, dev, bits, bf16, T, N, k=k, logprobs=lp)
                _check_top(bits, bf16, np.full(len(rows), T), N, ti, tl, tok, lps, (n, N, T, k, lp))
            assert _np(ti)[0].tolist() == list(range(min(N, n))) + [-1] * (N - min(N, n))        # the all-equal row
    # rows without a distribution: a NaN, a +inf, all -inf -> -1 / NaN in every slot
    n = 70
    x = np.tile(np.linspace(-3, 3, n).astype(np.float32), (3, 1))
    x[0, 17], x[1, 50], x[2] = np.nan, np.inf, -np.inf
    ti, tl, tok, _ = _top_call(ops, dev, pr._round16(x, bf16), bf16, 0.7, 5)
    assert (_np(ti) == -1).all() and np.isnan(_np(tl)).all() and tok.tolist() == [17, 50, 0]
    # a ban that leaves nothing but -inf is such a row too
    _, raw = ts._logits_dev(pr._round16(np.array([[1.0, -np.inf, 2.0]], np.float32), bf16), 3, bf16, dev)
    ti = torch.full((1, 2), -7, dtype=torch.int32, device=dev)
    tl = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    one = lambda v, dt=torch.float32: torch.full((1,), v, dtype=dt, device=dev)          # noqa: E731
    ops.sample_advance(raw, one(0.7), one(0, torch.int32), one(1.0), u=one(0.5), tokens=one(0, torch.int32),
                       bias=_bias_dev([{0: -np.inf, 2: -np.inf}], 3, dev), top_n=2, top_ids=ti, top_logprobs=tl)
    assert ti.tolist() == [[-1, -1]] and torch.isnan(tl).all()


# ---- 3. the speculative kernel --------------------------------------------------------------------------------------------------------
def _spec_call(ops, dev, logits, drafts, T, k, p, u, b, len_q, **kw):
    i32, f32 = torch.int32, torch.float32
    out = dict(tokens=torch.arange(b, dtype=i32, device=dev) + 3, positions=torch.arange(b, dtype=i32, device=dev) + 10,
               placement=torch.arange(b, dtype=i32, device=dev) + 20, valid_lens=torch.arange(b, dtype=i32, device=dev) + 30,
               accepted=torch.full((b,), -7, dtype=i32, device=dev), out_tokens=torch.full((b, len_q), -7, dtype=i32, device=dev),
               out_logprobs=torch.full((b, len_q), -77.0, dtype=f32, device=dev), logprobs=torch.full((b,), -77.0, dtype=f32, device=dev),
               u_out=torch.full((b, len_q), -77.0, dtype=f32, device=dev))
    ops.spec_sample_accept(logits, _to(drafts, np.int32, dev), _to(T, np.float32, dev), _to(k, np.int32, dev), _to(p, np.float32, dev),
                           u=_to(u, np.float32, dev), **out, **kw)
    return out


@pytest.mark.parametrize("n", [33, 128256])
@pytest.mark.parametrize("len_q", [2, 5, 32])
@pytest.mark.parametrize("b", [1, 3])
def test_spec_opts(dev, b, len_q, n):
    """the speculative call with penalty + bias + top-N against (a) the three-launch path: repetition_penalty with penalty_ref's row
    sets, scatter_logits(add) of the task's bias onto each of its rows, the plain speculative call; (b) the one-row calls, row by row
    under the row's penalty set, for the top-N"""
    from zhilight_amd import ops
    bf16 = bool(b & 2)
    rng = np.random.default_rng(100 * len_q + n + b)
    K, m, N, ld = len_q - 1, b * len_q, 5, n + 3
    bits = ts._make_rows(rng, m, n, bf16, shift=2)
    factor, presence = np.array([1.3, 1.0, 0.5][:b], np.float32), np.array([0.0, 0.7, 0.0][:b], np.float32)
    T, k, p = np.array([0.0, 0.7, 0.7][:b], np.float32), np.array([0, 5, 0][:b], np.int32), np.array([1.0, 0.9, 1.0][:b], np.float32)
    ids = [np.unique(rng.integers(0, n, max(1, n // 100))) for _ in range(b)]
    seen = pr.pack(ids, n)
    maps = [{int(i): float(v) for i, v in zip(rng.choice(n, min(n, 9), replace=False), rng.normal(0, 3, 9))} for _ in range(b)]
    maps[0][int(ids[0][0])] = 2.5                                       # in seen and biased
    u = rng.random((b, len_q)).astype(np.float32)
    # drafts: task 0 (greedy) follows the modified arg-max of every row up to one wrong draft; the others take large classes
    drafts = np.empty((b, K), np.int64)
    for t in range(b):
        for i in range(K):
            s = sorted(set(ids[t].tolist()) | {int(d) for d in drafts[t, :i] if 0 <= d < n})
            row = so.modified_row(bits[t * len_q + i], bf16, s, factor[t], presence[t], maps[t])
            order = np.argsort(-np.nan_to_num(sample_ref.values_of(row, bf16), nan=np.inf), kind="stable")
            drafts[t, i] = int(order[0]) if t == 0 else int(order[rng.integers(0, min(3, n))])
    wrong = K - 1 if K > 2 else K
    if wrong < K:
        drafts[0, wrong] = (drafts[0, wrong] + 1) % n
    flat_a, raw = ts._logits_dev(bits, ld, bf16, dev)
    flat_b, copy = ts._logits_dev(bits, ld, bf16, dev)
    before = flat_a.clone()
    sets = pr.row_sets(ids, drafts, n)
    buf = flat_b[:m * ld].view(m, ld)
    tp._penalise(ops, buf, [sets[t][i] for t in range(b) for i in range(len_q)], np.repeat(factor, len_q), np.repeat(presence, len_q), dev)
    _scatter_bias(ops, buf, [maps[t] for t in range(b) for _ in range(len_q)], dev)
    three = _spec_call(ops, dev, copy, drafts, T, k, p, u, b, len_q)
    seen_dev = tp._seen_dev(seen, dev)
    ti = torch.full((b, len_q, N), -7, dtype=torch.int32, device=dev)
    tl = torch.full((b, len_q, N), -77.0, dtype=torch.float32, device=dev)
    one = _spec_call(ops, dev, raw, drafts, T, k, p, u, b, len_q, rep_penalty=_to(factor, np.float32, dev),
                     presence=_to(presence, np.float32, dev), seen=seen_dev, bias=_bias_dev(maps, n, dev), top_n=N, top_ids=ti, top_logprobs=tl)
    torch.cuda.synchronize()
    for name in three:
        _same(one[name], three[name], name)
    _same(flat_a, before, "the raw logits")
    out = _np(one["out_tokens"])
    acc = _np(one["accepted"])
    assert np.array_equal(tp._seen_np(seen_dev), pr.mark(seen.copy(), out, n))          # the emitted tokens only, no bias entry
    assert acc[0] == min(wrong, K)
    # per-row equality of the top-N with the one-row call under the row's set, -1 / NaN behind the bonus token
    modified = _np(copy.contiguous().view(torch.int16)).view(np.uint16)
    rows_T = np.repeat(T, len_q)
    ti1 = torch.full((m, N), -7, dtype=torch.int32, device=dev)
    tl1 = torch.full((m, N), -77.0, dtype=torch.float32, device=dev)
    row_seen = pr.pack([sets[t][i] for t in range(b) for i in range(len_q)], n)
    rep = lambda a, dt: _to(np.repeat(a, len_q), dt, dev)              # noqa: E731
    ops.sample_advance(raw, rep(T, np.float32), rep(k, np.int32), rep(p, np.float32), u=_to(u.reshape(-1), np.float32, dev),
                       tokens=torch.zeros(m, dtype=torch.int32, device=dev), rep_penalty=rep(factor, np.float32), presence=rep(presence, np.float32),
                       seen=tp._seen_dev(row_seen, dev), bias=_bias_dev([maps[t] for t in range(b) for _ in range(len_q)], n, dev), top_n=N,
                       top_ids=ti1, top_logprobs=tl1)
    torch.cuda.synchronize()
    tin, tln = _np(ti), _np(tl)
    for t in range(b):
        a = int(acc[t])
        assert np.array_equal(tin[t, :a + 1], _np(ti1).reshape(b, len_q, N)[t, :a + 1])
        assert np.array_equal(tln[t, :a + 1].view(np.int32), _np(tl1).reshape(b, len_q, N)[t, :a + 1].view(np.int32))
        assert (tin[t, a + 1:] == -1).all() and np.isnan(tln[t, a + 1:]).all()
        for i in range(a + 1):
            want, _ = so.top_n(modified[t * len_q + i], bf16, rows_T[t * len_q + i], N)
            assert np.array_equal(tin[t, i], want), (t, i)


def test_spec_bias_decides_acceptance(dev):
    """hand-made rows, T = 1 sampling, len_q = 3.  Task 0: a -inf bias on its first draft forces the rejection at row 0 whatever u.
    Task 1: a bias that bans every class but the drafts makes each draft the only non-zero class: accepted whatever u"""
    from zhilight_amd import ops
    n, b, len_q = 33, 2, 3
    bits = pr._round16(np.random.default_rng(1).normal(0, 1, (b * len_q, n)).astype(np.float32), False)
    drafts = np.array([[int(np.argmax(sample_ref.values_of(bits[0], False))), 7], [4, 4]], np.int64)
    maps = [{int(drafts[0, 0]): -np.inf}, {i: -np.inf for i in range(n) if i != 4}]
    _, raw = ts._logits_dev(bits, n + 3, False, dev)
    for uv in (0.0, 0.5, 0.999):
        got = _spec_call(ops, dev, raw, drafts, np.ones(b), np.zeros(b), np.ones(b), np.full((b, len_q), uv), b, len_q, bias=_bias_dev(maps, n, dev))
        assert got["accepted"].tolist() == [0, 2], uv
        out = got["out_tokens"].tolist()
        assert out[0][0] != drafts[0, 0] and out[0][1:] == [-1, -1] and out[1] == [4, 4, 4]
        assert _np(got["out_logprobs"])[1].tolist() == [0.0, 0.0, 0.0]


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------
def test_deterministic_under_repetition_and_replay(dev):
    from zhilight_amd import ops
    n, rows, N = 4097, 3, 32
    rng = np.random.default_rng(9)
    bits = ts._make_rows(rng, rows, n, False, shift=4)                  # four values only among them: ties at every place
    sets = [np.unique(rng.integers(0, n, 40)) for _ in range(rows)]
    maps = _maps("many", rng, bits, False, n, sets)
    _, raw = ts._logits_dev(bits, n + 3, False, dev)
    f32 = lambda v: torch.full((rows,), v, dtype=torch.float32, device=dev)             # noqa: E731
    seen0 = tp._seen_dev(pr.pack(sets, n), dev)
    st = dict(seen=seen0.clone(), tokens=torch.zeros(rows, dtype=torch.int32, device=dev), logprobs=f32(0.0),
              top_ids=torch.zeros((rows, N), dtype=torch.int32, device=dev), top_logprobs=torch.zeros((rows, N), dtype=torch.float32, device=dev))
    par = dict(temperature=f32(0.7), top_k=torch.full((rows,), 20, dtype=torch.int32, device=dev), top_p=f32(0.9), u=f32(0.61),
               rep_penalty=f32(1.3), presence=f32(0.0), bias=_bias_dev(maps, n, dev), top_n=N)

    def run():
        st["seen"].copy_(seen0)
        ops.sample_advance(raw, **par, **st)

    def snap():
        torch.cuda.synchronize()
        return [_bits(st[name]).clone() for name in ("tokens", "logprobs", "top_ids", "top_logprobs", "seen")]
    run()
    first = snap()
    for _ in range(2):
        run()
        assert all(torch.equal(a, b) for a, b in zip(first, snap()))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        for name in ("tokens", "top_ids"):
            st[name].fill_(-5)
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(first, snap()))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_abi_refusals(dev):
    from zhilight_amd import ops
    from zhilight_amd._lib import SampleOpts, lib
    n = 40
    logits = torch.zeros((2, n), dtype=torch.float16, device=dev)
    f32 = lambda v: torch.full((2,), v, dtype=torch.float32, device=dev)                # noqa: E731
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)              # noqa: E731
    kw = dict(temperature=f32(1.0), top_k=i32(2), top_p=f32(1.0), u=f32(0.5), tokens=i32(2))
    ids, vals, cnt, bb = _bias_dev([{1: 0.5}, {}], n, dev)
    ti, tl = i32(2, 4), torch.zeros((2, 4), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)                   # noqa: E731
    i = C.c_int64

    ptr = lambda t: None if t is None else t.data_ptr()                                 # noqa: E731

    def call(b_ids, b_vals, b_cnt, b_ld, b_bits, b_bits_ld, top_n, t_ids, t_lp, null_opts=False):
        opts = None if null_opts else C.byref(SampleOpts(bias_ids=ptr(b_ids), bias_vals=ptr(b_vals), bias_cnt=ptr(b_cnt), bias_ld=b_ld,
                                                         bias_bits=ptr(b_bits), bias_bits_ld=b_bits_ld, top_n=top_n, top_ids=ptr(t_ids),
                                                         top_logprobs=ptr(t_lp)))
        return lib().zl_sample_advance_ex(p(logits), C.c_int(2), i(2), i(n), i(n), p(kw["temperature"]), p(kw["top_k"]), p(kw["top_p"]), p(None),
                                          p(None), p(kw["u"]), p(kw["tokens"]), p(None), p(None), p(None), p(None), p(None), p(None), opts,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    einval = [call(ids, None, cnt, 1, bb, 2, 0, None, None), call(None, vals, None, 1, None, 2, 0, None, None),
              call(ids, vals, cnt, 1, None, 2, 0, None, None), call(None, None, None, 0, None, 0, 4, ti, None),
              call(None, None, None, 0, None, 0, 4, None, tl)]
    eshape = [call(ids, vals, cnt, 1025, bb, 2, 0, None, None), call(ids, vals, cnt, 0, bb, 2, 0, None, None),
              call(ids, vals, cnt, 1, bb, 1, 0, None, None), call(None, None, None, 0, None, 0, -1, ti, tl),
              call(None, None, None, 0, None, 0, 33, ti, tl)]
    assert len(set(einval)) == 1 and len(set(eshape)) == 1 and einval[0] != 0 and eshape[0] != 0 and einval[0] != eshape[0]
    assert call(None, None, None, 0, None, 0, 0, None, None) == 0                       # a zeroed struct ...
    assert call(None, None, None, 0, None, 0, 0, None, None, null_opts=True) == 0       # ... and NULL opts: the plain call
    assert call(ids, vals, cnt, 1, bb, 2, 4, ti, tl) == 0                               # seen == NULL with a bias is legal
    torch.cuda.synchronize()
    # the wrappers
    with pytest.raises(ops.ZLError, match="logit_bias_pack"):
        ops.sample_advance(logits, **kw, bias=(ids, vals, cnt))
    with pytest.raises(ops.ZLError, match="bias bits"):
        ops.sample_advance(logits, **kw, bias=(ids, vals, cnt, bb[:, :1].contiguous()))
    with pytest.raises(ops.ZLError, match="top_n in 0"):
        ops.sample_advance(logits, **kw, top_n=33, top_ids=ti, top_logprobs=tl)
    with pytest.raises(ops.ZLError, match="top_ids"):
        ops.sample_advance(logits, **kw, top_n=4, top_logprobs=tl)
    with pytest.raises(ops.ZLError, match="top_logprobs"):
        ops.sample_advance(logits, **kw, top_n=4, top_ids=ti, top_logprobs=tl[:, :3].contiguous())
    packed = ops.logit_bias_pack([{3: 1.0}, None], n, dev)
    assert [t.dtype for t in packed] == [torch.int32, torch.float32, torch.int32, torch.int32] and packed[3].shape == (2, 2)
    with pytest.raises(ops.ZLError, match="outside"):
        ops.logit_bias_pack([{n: 1.0}], n, dev)


# ---- 6. the model -----------------------------------------------------------------------------------------------------------------------
K, STEPS, N_TOP = sv.K, 10, 5
KW = dict(temperature=0.8, top_k=20, top_p=0.95, seed=77)
PEN_KW = dict(repetition_penalty=[1.3, 1.0, 1.6], presence_penalty=[0.0, 0.7, 0.25])


class _Case:
    pass


@pytest.fixture(scope="module")
def case(dev):
    c = _Case()
    rng, c.cfg, c.sd, c.model = _gptq_model(dev)
    c.vocab = c.cfg.vocab_size
    c.motifs = [np.tile(rng.integers(0, c.vocab, 8), 5)[:s].astype(np.int32) for s in (16, 40, 24)]
    c.bias = [{int(i): float(v) for i, v in zip(rng.choice(c.vocab, 40, replace=False), rng.normal(0, 4, 40))} for _ in range(3)]
    c.bias[1][int(c.motifs[1][0])] = -np.inf
    c.loops = {}
    return c


def _opt_kw(c, b):
    return dict(**{name: v[:b] for name, v in PEN_KW.items()}, logit_bias=c.bias[:b], top_logprobs=N_TOP)


def _host_loop(c, b, dev):
    """the path a caller had: encode, repetition_penalty over the emitted tokens and scatter_logits(add) of the bias on a copy, the
    plain sample_advance with the generator's uniforms; the top-N of each step from the copy, by the sort -> (tokens (b, STEPS),
    logprobs as patterns, top ids (b, STEPS, N), the modified rows as patterns (b, STEPS, vocab))"""
    if b in c.loops:
        return c.loops[b]
    from zhilight_amd import ops
    ctx = sv._fresh(c.model, c.motifs[:b])
    emitted = [[int(t)] for t in ctx.tokens.tolist()]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)                    # noqa: E731
    T, k, p = f32([0.8] * b), torch.tensor([20] * b, dtype=torch.int32, device=dev), f32([0.95] * b)
    nxt, lp = torch.empty(b, dtype=torch.int64, device=dev), torch.empty(b, dtype=torch.float32, device=dev)
    toks, lps, tops, mods = [], [], [], []
    for step in range(STEPS):
        copy = c.model.encode(ctx).clone()
        tp._penalise(ops, copy, [sorted(set(e)) for e in emitted], PEN_KW["repetition_penalty"][:b], PEN_KW["presence_penalty"][:b], dev)
        _scatter_bias(ops, copy, c.bias[:b], dev)
        u = torch.from_numpy(sample_ref.uniforms(77 + np.arange(b), np.full(b, step))).to(dev)
        ops.sample_advance(copy, T, k, p, u=u, tokens=ctx.tokens, positions=ctx.positions, placement=ctx.placement, valid_lens=ctx.valid_lens,
                           next_tokens=nxt, logprobs=lp)
        ctx.steps_left -= 1
        for j, t in enumerate(nxt.tolist()):
            emitted[j].append(t)
        rows = _np(copy.view(torch.int16)).view(np.uint16)
        tops.append(np.stack([so.top_n(rows[j], False, 0.8, N_TOP)[0] for j in range(b)]))
        mods.append(rows.copy())
        toks.append(_np(nxt).copy())
        lps.append(_np(lp).view(np.int32).copy())
    c.loops[b] = (np.stack(toks, axis=1), np.stack(lps, axis=1), np.stack(tops, axis=1), np.stack(mods, axis=1))
    return c.loops[b]


@pytest.mark.parametrize("b", [1, 3])
def test_generate_sample_is_the_host_loop(case, dev, b):
    c = case
    toks, lps, tops, _ = _host_loop(c, b, dev)
    ctx = sv._fresh(c.model, c.motifs[:b])
    pending = ctx.tokens.tolist()
    state = c.model.new_sampler(ctx, **KW, **_opt_kw(c, b))
    assert state.top_n == N_TOP and state.top_ids.shape == (b, N_TOP) and state.bias_bits.shape == (b, (c.vocab + 31) // 32)
    got, got_lp, (ti, tl) = c.model.generate_sample(ctx, state, STEPS)
    assert np.array_equal(_np(got), toks)
    assert np.array_equal(_np(got_lp).view(np.int32), lps)
    assert ti.shape == (b, STEPS, N_TOP) and np.array_equal(_np(ti), tops)
    tin, tln = _np(ti), _np(tl)
    for j in range(b):
        for s in range(STEPS):                                         # a pick under top-k 20 need not be among the 5; where it is: bit-equal
            at = np.flatnonzero(tin[j, s] == toks[j, s])
            if at.size:
                assert tln[j, s, at[0]].view(np.int32) == lps[j, s]
        if j == 1:
            assert int(c.motifs[1][0]) not in toks[1].tolist()                           # the banned id is never emitted
        seen = pr.unpack(tp._seen_np(state.seen), c.vocab)[j].tolist()                  # emitted tokens only: no bias entry
        assert seen == sorted(set([pending[j]] + toks[j].tolist()))


@pytest.mark.parametrize("b", [1, 3])
def test_generate_lookup_emits_the_same_tokens_and_top_n(case, dev, b):
    """speculation changes the speed, not the sample: generate_lookup(sampler=) emits the host loop's tokens, and per emitted token
    step_sample's top-N.  The tokens are equal.  The alternatives cannot be bit-equal in general: a verify row's logits Y come from
    another GEMM route than the one-row step's X (test_gpu_sample_penalty.py:423 records the same of the log-probabilities), so they
    are held to what that difference allows and no more.  With d = max |Y' - X'| over the row AS MODIFIED (penalty and bias applied to
    both on the host; the test measures d from the two routes' logits, not from the sampler):
      ids   the s-th order statistic is 1-Lipschitz in the sup norm, so the class the lookup step reports in slot s has an X' value
            within 2 d of the class step_sample's sort has there: |X'[L[s]] - X'[H[s]]| <= 2 d for every slot; where d = 0 the ids are equal
      lp    a log-probability moves by at most d / T through its own value and d / T through the log-sum-exp: within 2 d / T of the
            float64 log-probability under X', plus the kernel's own bar against float64 (test_gpu_sample.py:157, fin 2 eps_t + bound(n))
    and EXACTLY to the sort of the verify rows' own modified logits.  generate_lookup's stats are the eager steps' rows, bit for bit"""
    c = case
    toks, _, tops, mods = _host_loop(c, b, dev)
    ctx = sv._fresh(c.model, c.motifs[:b])
    look = c.model.new_lookup(ctx, c.motifs[:b], K)
    samp = c.model.new_sampler(ctx, **KW, **_opt_kw(c, b))
    got, stats = c.model.generate_lookup(ctx, look, STEPS, sampler=samp)
    assert got == toks.tolist()
    ti, tl = np.array(stats["top_ids"]), np.array(stats["top_logprobs"], np.float32)
    assert ti.shape == tops.shape and tl.shape == tops.shape and (ti >= 0).all() and (ti < c.vocab).all()
    assert samp.row_top_ids.shape == (b, K + 1, N_TOP)
    # the same steps by hand, with the rows' logits at hand
    ctx = sv._fresh(c.model, c.motifs[:b])
    emitted = [[int(t)] for t in ctx.tokens.tolist()]
    look = c.model.new_lookup(ctx, c.motifs[:b], K)
    samp = c.model.new_sampler(ctx, **KW, **_opt_kw(c, b))
    out, ids_by_hand, lps_by_hand = [[] for _ in range(b)], [[] for _ in range(b)], [[] for _ in range(b)]
    T, eps_t, exact, worst = 0.8, 2.0 ** -11, 0, 0.0
    while min(len(o) for o in out) < STEPS:
        drafts = _np(look.drafts).copy()
        res = c.model.step_lookup(ctx, look, sampler=samp)
        rows = _np(res.logits.contiguous().view(torch.int16)).view(np.uint16).reshape(b, K + 1, c.vocab)
        acc, tok = res.accepted.tolist(), res.tokens.tolist()
        rti, rtl, rlp = _np(samp.row_top_ids), _np(samp.row_top_logprobs), _np(samp.row_logprobs)
        for j in range(b):
            for i in range(acc[j] + 1):
                pset = set(emitted[j]) | {int(d) for d in drafts[j, :i] if 0 <= d < c.vocab}
                row = so.modified_row(rows[j, i], False, pset, PEN_KW["repetition_penalty"][j], PEN_KW["presence_penalty"][j], c.bias[j])
                assert np.array_equal(rti[j, i], so.top_n(row, False, T, N_TOP)[0]), (j, i)
                at = np.flatnonzero(rti[j, i] == tok[j][i])
                if at.size:
                    assert rtl[j, i, at[0]].view(np.int32) == rlp[j, i].view(np.int32)
                step = len(out[j]) + i                                  # the one-row step that emitted this token
                if step < STEPS:
                    assert tok[j][i] == toks[j, step]
                    x, y = sample_ref.values_of(mods[j, step], False), sample_ref.values_of(row, False)
                    live = ~np.isneginf(x)                              # a ban is -inf on both routes
                    assert np.isfinite(x[live]).all() and live.any()
                    d = float(np.abs(x[live] - y[live]).max()) if np.array_equal(live, ~np.isneginf(y)) else np.inf
                    H, href = so.top_n(mods[j, step], False, T, N_TOP)
                    assert np.array_equal(H, tops[j, step])
                    L = rti[j, i].astype(np.int64)
                    with np.errstate(invalid="ignore"):
                        gap = np.abs(x[L] - x[H])
                    gap[np.isneginf(x[L]) & np.isneginf(x[H])] = 0.0
                    assert (gap <= 2 * d).all(), (j, step, L.tolist(), H.tolist(), d)
                    fin = np.abs(x[live]).max()
                    for slot, cls in enumerate(L):
                        if cls in H and np.isfinite(x[cls]):
                            err = abs(float(rtl[j, i, slot]) - href[int(np.flatnonzero(H == cls)[0])])
                            assert err <= 2 * d / T + fin * 2 * eps_t + bound(c.vocab), (j, step, slot, err, d)
                            worst = max(worst, err)
                    exact += int(np.array_equal(L, H))
            assert (rti[j, acc[j] + 1:] == -1).all() and np.isnan(rtl[j, acc[j] + 1:]).all()
            emitted[j] += tok[j][:acc[j] + 1]
            out[j] += tok[j][:acc[j] + 1]
            ids_by_hand[j] += rti[j, :acc[j] + 1].tolist()
            lps_by_hand[j] += rtl[j, :acc[j] + 1].view(np.int32).tolist()
    print("lookup steps whose top-N ids equal step_sample's:", exact, "of", b * STEPS, "; largest |logprob difference|", worst)
    for j in range(b):
        assert out[j][:STEPS] == toks[j].tolist()
        assert ti[j].tolist() == ids_by_hand[j][:STEPS]                 # generate_lookup reported these rows
        assert tl[j].view(np.int32).tolist() == lps_by_hand[j][:STEPS]


def test_captured_steps_continue_the_eager_sequence(case, dev):
    c, b = case, 3
    toks, _, tops, _ = _host_loop(c, b, dev)
    ctx = sv._fresh(c.model, c.motifs[:b])
    state = c.model.new_sampler(ctx, **KW, **_opt_kw(c, b))
    _, nxt = c.model.step_sample(ctx, state)
    assert np.array_equal(_np(nxt), toks[:, 0]) and np.array_equal(_np(state.top_ids), tops[:, 0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gnxt = c.model.step_sample(ctx, state)
    for step in range(1, 5):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(gnxt), toks[:, step]) and np.array_equal(_np(state.top_ids), tops[:, step]), step

    def start():
        x = sv._fresh(c.model, c.motifs[:b])
        return x, c.model.new_lookup(x, c.motifs[:b], K), c.model.new_sampler(x, **KW, **_opt_kw(c, b))
    ectx, elook, esamp = start()
    eager = []
    for _ in range(3):
        res = c.model.step_lookup(ectx, elook, sampler=esamp)
        eager.append((res.accepted.clone(), res.tokens.clone(), esamp.row_top_ids.clone(), _bits(esamp.row_top_logprobs).clone()))
    tctx, tlook, tsamp = start()
    c.model.step_lookup(tctx, tlook, sampler=tsamp)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = c.model.step_lookup(tctx, tlook, sampler=tsamp)
    for step in range(1, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(r.accepted, eager[step][0]) and torch.equal(r.tokens, eager[step][1]), step
        assert torch.equal(tsamp.row_top_ids, eager[step][2]) and torch.equal(_bits(tsamp.row_top_logprobs), eager[step][3]), step


def test_options_off_is_todays_state(case, dev, monkeypatch):
    from zhilight_amd import ops
    c, b = case, 3
    ctx, ctx2 = sv._fresh(c.model, c.motifs[:b]), sv._fresh(c.model, c.motifs[:b])
    plain = c.model.new_sampler(ctx, **KW)
    off = c.model.new_sampler(ctx2, **KW, logit_bias=[None, {}, None], top_logprobs=0)
    for s in (plain, off):
        assert s.opts() == {} and s.top_n == 0
        assert all(getattr(s, f) is None for f in ("bias_ids", "bias_vals", "bias_cnt", "bias_bits", "top_ids", "top_logprobs", "row_top_ids",
                                                   "row_top_logprobs", "row_top_bufs", "seen"))
    called = []
    real = ops.sample_advance
    monkeypatch.setattr(ops, "sample_advance", lambda *a, **kw: (called.append(sorted(kw)), real(*a, **kw))[1])
    a = c.model.generate_sample(ctx, plain, 3)
    o = c.model.generate_sample(ctx2, off, 3)
    assert len(a) == len(o) == 2 and torch.equal(a[0], o[0])
    assert all("bias" not in kw and "top_n" not in kw for kw in called) and len(called) == 6


def test_model_refusals(case, dev):
    from zhilight_amd import ops
    c = case
    ctx = sv._fresh(c.model, c.motifs[:3])
    for bad in (-1, 33, 2.5, True):
        with pytest.raises(ops.ZLError, match="top_logprobs is an integer"):
            c.model.new_sampler(ctx, top_logprobs=bad)
    with pytest.raises(ops.ZLError, match="2 maps of logit_bias"):
        c.model.new_sampler(ctx, logit_bias=[{1: 1.0}, None])
    for bad, what in (({c.vocab: 1.0}, "outside"), ({1: float("nan")}, "not NaN"), ({1: float("inf")}, "not NaN"),
                      ({i: 0.0 for i in range(1025)}, "at most 1024"), ({1: 0.5, "1": 1.0}, "given twice")):
        with pytest.raises(ops.ZLError, match=what):
            c.model.new_sampler(ctx, logit_bias=bad)
    state = c.model.new_sampler(ctx, logit_bias={1: -np.inf}, top_logprobs=3)
    assert state.seen is None and state.bias_cnt.tolist() == [1, 1, 1]
    two = sv._fresh(c.model, c.motifs[:2])
    with pytest.raises(ops.ZLError, match="another batch size"):
        c.model.step_sample(two, state)
    with pytest.raises(ops.ZLError, match="another batch size"):
        c.model.verify(two, torch.zeros((2, K), dtype=torch.int32, device=dev), sampler=state)
