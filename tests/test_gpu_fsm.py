"""The token automaton inside the device sampling step: zl_sample_advance_fsm / zl_spec_sample_accept_fsm / zl_slots_admit_fsm.
The bar of the masking is EQUALITY with what the project already had: fsm_ref.masked (masked_fill(-inf) of the disallowed classes) on a
copy of the logits, then the existing call with the same penalty / bias / top-N options on the copy -- both paths run the same
arithmetic on the same 16-bit patterns, so every output is compared bit for bit.  The states are integers and must equal fsm_ref's."""
import ctypes as C

import numpy as np
import pytest
import torch

import fsm_ref
import penalty_ref as pr
import sample_opts_ref as so
import test_gpu_sample as ts
import test_gpu_sample_opts as tso
import test_gpu_sample_penalty as tp
import test_gpu_slots as tslots
import test_gpu_spec_verify as sv
import test_slot_host as host
from test_gpu_prefill_batch import _gptq_model

pytestmark = pytest.mark.gpu

NS = tso.NS
_np, _same, _to = tso._np, tso._same, tso._to
NEG = fsm_ref.NEG_INF


def _tables_dev(tb, dev):
    from zhilight_amd import ops
    return ops.grammar_tables(tb.arrays(), dev)


def _bitmap(sets, n, extra_words=0, junk=False):
    """(S, ceil(n / 32) + extra_words) uint32 from id sets; junk: every bit at or above n set, the extra words 0xDEADBEEF"""
    m = pr.pack([np.asarray(sorted(s), np.int64) for s in sets], n)
    if junk and n & 31:
        m[:, -1] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF)
    if extra_words:
        m = np.concatenate([m, np.full((m.shape[0], extra_words), 0xDEADBEEF if junk else 0, np.uint32)], axis=1)
    return m


def _general_tables(rng, n):
    """five states: half of the classes; the last class alone; every class; about 1 %; the unaligned head and tail of a row.  Defaults
    walk the ring, a handful of allowed tokens per state are exceptions to anywhere, outside [0, S) included"""
    ids = np.arange(n)
    sets = [set(ids[rng.random(n) < 0.5].tolist()) | {int(rng.integers(0, n))}, {n - 1}, set(ids.tolist()),
            set(rng.integers(0, n, max(1, n // 100)).tolist()), set(ids[:8].tolist()) | set(ids[-8:].tolist())]
    S = len(sets)
    off, tok, nxt = [0], [], []
    for s in range(S):
        al = np.asarray(sorted(sets[s]))
        ex = np.unique(rng.choice(al, min(al.size, 6)))
        tok += ex.tolist()
        nxt += rng.choice(np.array([-1, 0, 1, 2, 3, 4, S + 3]), ex.size).tolist()
        off.append(len(tok))
    return fsm_ref.Tables(_bitmap(sets, n, 1, junk=True), (np.arange(S) + 1) % S, off, tok, nxt)


def _two_paths(ops, dev, bits, ld, bf16, tb, states, T, k, p, u, sets=None, factor=None, presence=None, maps=None, top_n=0):
    """zl_sample_advance_fsm on the raw rows against the existing call on fsm_ref.masked's copy, the same options on both sides
    -> (fused outputs, copy's outputs, per side (seen, top ids, top logprobs), the states afterwards, the masked rows)"""
    rows, n = bits.shape
    states = np.asarray(states, np.int32)
    mrows = np.stack([fsm_ref.masked(bits[r], tb, states[r], bf16) for r in range(rows)])
    flat_a, raw = ts._logits_dev(bits, ld, bf16, dev)
    _, copy = ts._logits_dev(mrows, ld, bf16, dev)
    before = flat_a.clone()
    par = dict(temperature=_to(T, np.float32, dev), top_k=_to(k, np.int32, dev), top_p=_to(p, np.float32, dev), u=_to(u, np.float32, dev))
    side = []
    outs = []
    for logits in (raw, copy):
        kw = {}
        if sets is not None:
            kw.update(rep_penalty=_to(factor, np.float32, dev), presence=_to(presence, np.float32, dev),
                      seen=tp._seen_dev(pr.pack(sets, n, ld=pr.words(n) + 1), dev))
        if maps is not None:
            kw["bias"] = tso._bias_dev(maps, n, dev)
        if top_n:
            kw.update(top_n=top_n, top_ids=torch.full((rows, top_n), -7, dtype=torch.int32, device=dev),
                      top_logprobs=torch.full((rows, top_n), -77.0, dtype=torch.float32, device=dev))
        out = tp._Out(rows, dev)
        if logits is raw:
            st = _to(states, np.int32, dev)
            ops.sample_advance(raw, **par, **out.kw, **kw, fsm=_tables_dev(tb, dev), fsm_state=st)
        else:
            ops.sample_advance(copy, **par, **out.kw, **kw)
        outs.append(out)
        side.append((kw.get("seen"), kw.get("top_ids"), kw.get("top_logprobs")))
    torch.cuda.synchronize()
    _same(flat_a, before, "the raw logits")
    return outs[0], outs[1], side, _np(st), mrows


def _assert_equal(one, two, side, what):
    for name in tp._Out.NAMES:
        _same(one.kw[name], two.kw[name], what + (name,))
    for x, y, name in zip(side[0], side[1], ("seen", "top_ids", "top_logprobs")):
        if x is not None:
            _same(x, y, what + (name,))


def _want_states(tb, states, picks, n):
    return [fsm_ref.delta(tb, s, t, n) for s, t in zip(states, picks)]


# ---- 1. the kernel against masked_fill + the existing call ------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("n", NS)
def test_kernel_equals_masked_fill_then_sample(dev, n, bf16):
    """rows misaligned (ld = n + 1); a mixed batch: every state of _general_tables, a row with state -1 and one with a state >= S
    (both unconstrained, their states unwritten); mask rows one word wider than needed, with junk at and above n"""
    from zhilight_amd import ops
    rng = np.random.default_rng(29 * n + bf16)
    tb = _general_tables(rng, n)
    states = [0, 1, 2, 3, 4, -1, tb.S + 2]
    rows, ld = len(states), n + 1
    moved = 0
    for shift, mode in enumerate(("none", "pen", "pen+bias+top")):
        bits = ts._make_rows(rng, rows, n, bf16, shift=shift)
        T, k, p, u = ts._params(rng, rows, n)
        sets = factor = presence = maps = None
        if mode != "none":
            sets = [np.unique(rng.integers(0, n, max(1, n // 100))) for _ in range(rows)]
            factor = np.array([tp.PENS[(j + shift) % 5][0] for j in range(rows)], np.float32)
            presence = np.array([tp.PENS[(j + shift) % 5][1] for j in range(rows)], np.float32)
        if mode == "pen+bias+top":
            maps = tso._maps("many", rng, bits, bf16, n, sets)
        one, two, side, after, mrows = _two_paths(ops, dev, bits, ld, bf16, tb, states, T, k, p, u, sets, factor, presence, maps,
                                                  top_n=5 if maps else 0)
        _assert_equal(one, two, side, (n, bf16, mode))
        picks = _np(one.kw["tokens"])
        assert after.tolist() == _want_states(tb, states, picks, n), (mode, picks.tolist())
        assert after[5] == -1 and after[6] == tb.S + 2
        for r in range(5):                                                  # a constrained row with a distribution picks an allowed class
            if not so.is_plain_bits(mrows[r], bf16) and maps is None:
                assert fsm_ref.allowed(tb, states[r], int(picks[r])), (mode, r)
        moved += int((after[:5] != np.asarray(states[:5])).sum())
    assert moved > 0


# ---- 2. rows built to break it ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("n", [70, 4097])
def test_rows_built_to_break_the_mask(dev, n, bf16):
    from zhilight_amd import ops
    nan = 0x7E00 if not bf16 else 0x7FC0
    base = pr._round16(np.linspace(-3, 3, n).astype(np.float32), bf16)
    half, odd = set(range(0, n, 2)), set(range(1, n, 2))
    rows, sets, names = [], [], []

    def add(name, row, allowed):
        names.append(name), rows.append(np.asarray(row, np.uint16)), sets.append(set(allowed))

    add("the last class alone (n & 31 != 0)", base, {n - 1})
    add("every class", base, range(n))
    add("head and tail fragments only", base, list(range(3)) + list(range(n - 3, n)))
    add("the stored maximum is disallowed", base, range(n - 1))
    x = base.copy()
    x[5] = nan
    add("a disallowed NaN", x, set(range(n)) - {5})
    x = base.copy()
    x[[2, 40, n - 2]] = NEG[bf16]
    add("an allowed -inf", x, half | {2, 40, n - 2})
    x = base.copy()
    x[list(odd)] = NEG[bf16]
    add("every allowed class -inf: a plain row", x, odd)                   # the arg-max of the all -inf row, class 0, is disallowed
    x = pr._round16(np.full(n, -1.0, np.float32), bf16)
    x[10:30] = pr._round16(np.array([1.5], np.float32), bf16)[0]
    add("top-k's boundary inside a run of equal values, half of them disallowed", x, set(range(n)) - set(range(10, 30, 2)))
    add("fewer allowed classes than top_n", base, {1, 33 % n, n - 2})
    add("in seen, biased and disallowed at once", base, set(range(n)) - {7, n - 1})
    R = len(rows)
    tb = fsm_ref.Tables(_bitmap(sets, n, 0, junk=True), np.arange(R) + 100, np.zeros(R + 1, np.int32), [], [])     # defaults leave [0, S)
    bits, states = np.stack(rows), list(range(R))
    pens = [np.array([7, n - 1, 12]) for _ in range(R)]
    maps = [{7: 4.0, n - 1: 9.0, 3: -0.5} for _ in range(R)]
    for T, k in ((0.0, 0), (0.8, 0), (0.8, 6), (1.0, 15)):
        for u in (0.0, 0.37, ts.LAST):
            one, two, side, after, mrows = _two_paths(ops, dev, bits, n + 1, bf16, tb, states, np.full(R, T), np.full(R, k), np.full(R, 0.95),
                                                      np.full(R, u), pens, np.full(R, 1.3), np.zeros(R), maps, top_n=5)
            _assert_equal(one, two, side, (n, bf16, T, k, u))
            picks = _np(one.kw["tokens"])
            assert after.tolist() == _want_states(tb, states, picks, n)
            for r in range(R):                                              # -inf stays -inf through the penalty and the bias
                if not so.is_plain_bits(so.modified_row(mrows[r], bf16, pens[r], 1.3, 0.0, maps[r]), bf16):
                    assert int(picks[r]) in sets[r], (names[r], T, k, u)
    # without penalty and bias: the plain row's pick (class 0) is disallowed and its state does not move; top-N shows exactly the
    # allowed classes in front where there are fewer than N
    one, two, side, after, mrows = _two_paths(ops, dev, bits, n + 1, bf16, tb, states, np.full(R, 0.8), np.full(R, 4), np.full(R, 1.0),
                                              np.full(R, 0.5), top_n=5)
    _assert_equal(one, two, side, (n, bf16, "bare"))
    picks, ti, tl = _np(one.kw["tokens"]), _np(side[0][1]), _np(side[0][2])
    r = names.index("every allowed class -inf: a plain row")
    assert picks[r] == 0 and after[r] == r and np.isnan(_np(one.kw["logprobs"])[r]) and (ti[r] == -1).all()
    r = names.index("fewer allowed classes than top_n")
    assert sorted(ti[r][:3].tolist()) == sorted(sets[r]) and np.isfinite(tl[r][:3]).all() and np.isneginf(tl[r][3:]).all()
    assert all(fsm_ref.allowed(tb, r, int(picks[r])) for r in range(R) if r != names.index("every allowed class -inf: a plain row"))
    r = names.index("the last class alone (n & 31 != 0)")
    assert picks[r] == n - 1 and after[r] == 100 + r
    r = names.index("top-k's boundary inside a run of equal values, half of them disallowed")
    assert picks[r] in range(11, 30, 2)


# ---- 3. transitions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 63, 64, 65, 5000])
def test_exception_lists(dev, size):
    """a state whose exception list holds `size` ids: the pick is the first, the last, one in the middle and one that is missing (the
    default); a negative target unconstrains the next step"""
    from zhilight_amd import ops
    n, bf16 = 12007, False
    rng = np.random.default_rng(size)
    exc = np.sort(rng.choice(n - 1, size, replace=False))                   # class n - 1 is never an exception
    missing = n - 1
    # state 0: a list of 3 in front; state 1: the list under test; state 2: a list of 2 behind it
    tok = np.concatenate([[1, 5, 9], exc, [0, 2]])
    nxt = np.concatenate([[7, 7, 7], 1000 + np.arange(size), [7, 7]])
    nxt[3 + size // 2] = -1                                                 # the middle entry ends the grammar
    tb = fsm_ref.Tables(_bitmap([range(n)] * 3, n), [50, 60, 70], [0, 3, 3 + size, 5 + size], tok, nxt)
    want_tok = [int(exc[0]), int(exc[-1]), int(exc[size // 2]), missing]
    bits = np.tile(pr._round16(np.linspace(-2, 0, n).astype(np.float32), bf16), (4, 1))
    for r, t in enumerate(want_tok):
        bits[r, t] = pr._round16(np.array([4.0], np.float32), bf16)[0]
    R = 4
    _, raw = ts._logits_dev(bits, n + 1, bf16, dev)
    st = _to(np.ones(R), np.int32, dev)
    tok_out = torch.zeros(R, dtype=torch.int32, device=dev)
    par = dict(temperature=_to(np.zeros(R), np.float32, dev), top_k=_to(np.zeros(R), np.int32, dev), top_p=_to(np.ones(R), np.float32, dev),
               u=_to(np.full(R, 0.5), np.float32, dev))
    fsm = _tables_dev(tb, dev)
    ops.sample_advance(raw, **par, tokens=tok_out, fsm=fsm, fsm_state=st)
    assert _np(tok_out).tolist() == want_tok
    want = _want_states(tb, [1] * R, want_tok, n)
    assert _np(st).tolist() == want and want[2] == -1 and want[3] == 60
    if size > 2:
        assert want[:2] == [1000, 1000 + size - 1]
    # the next step: every state is outside [0, S) now -- the rows are read as stored, the states stay
    tb2 = fsm_ref.Tables(_bitmap([[3]] * 3, n), tb.default, tb.exc_off, tb.exc_tok, tb.exc_next)
    ops.sample_advance(raw, **par, tokens=tok_out, fsm=_tables_dev(tb2, dev), fsm_state=st)
    assert _np(tok_out).tolist() == want_tok and _np(st).tolist() == want


# ---- 4. the speculative call ------------------------------------------------------------------------------------------------------------
def _spec_tables(rng, n):
    """a ring of three dense states, the third of which ends the grammar by default (-1); a few exceptions jump inside the ring"""
    ids = np.arange(n)
    sets = [set(ids[rng.random(n) < 0.6].tolist()) | {0, n - 1} for _ in range(4)]
    off, tok, nxt = [0], [], []
    for s in range(4):
        ex = np.unique(rng.choice(np.asarray(sorted(sets[s])), min(len(sets[s]), 8)))
        tok += ex.tolist()
        nxt += rng.integers(0, 4, ex.size).tolist()
        off.append(len(tok))
    return fsm_ref.Tables(_bitmap(sets, n, 0, junk=True), [1, 2, -1, 0], off, tok, nxt)


def _sequential(ops, dev, raw_rows, tb, fsm, state, seen_row, drafts, par_t, u_row, factor, presence, n):
    """one task, row after row through zl_sample_advance_fsm with the task's state and set carried: the emitted tokens, the states
    behind each of them"""
    one = lambda v, dt: torch.tensor([v], dtype=dt, device=dev)             # noqa: E731
    st = one(int(state), torch.int32)
    seen = seen_row.clone().view(1, -1)
    toks, states = [], []
    for i in range(raw_rows.shape[0]):
        tok = one(0, torch.int32)
        ops.sample_advance(raw_rows[i:i + 1], one(par_t[0], torch.float32), one(int(par_t[1]), torch.int32), one(par_t[2], torch.float32),
                           u=one(float(u_row[i]), torch.float32), tokens=tok, rep_penalty=one(factor, torch.float32),
                           presence=one(presence, torch.float32), seen=seen, fsm=fsm, fsm_state=st)
        toks.append(int(tok[0]))
        states.append(int(st[0]))
        if drafts is not None and (i >= len(drafts) or toks[-1] != int(drafts[i])):        # drafts None: every pick is confirmed
            break
    return toks, states, seen


@pytest.mark.parametrize("n", [33, 128256])
@pytest.mark.parametrize("len_q", [2, 5, 32])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("kind", ["accepted", "disallowed", "minus_one", "unconstrains"])
def test_spec_equals_the_sequential_loop(dev, kind, b, len_q, n):
    """out_tokens, accepted, row_states, fsm_state and seen equal the sequential zl_sample_advance_fsm loop fed the same uniforms.  The
    drafts are the loop's own picks (all accepted: the states run through the ring and out of the grammar), then one of them is
    replaced: by a token its state disallows, by -1, or -- "unconstrains" -- left alone with every task started in the state whose
    default target is -1, so that the draft chain itself leaves the grammar"""
    from zhilight_amd import ops
    bf16 = bool(b & 2)
    rng = np.random.default_rng(1000 * len_q + n + 7 * b + len(kind))
    K, m, ld = len_q - 1, b * len_q, n + 1
    tb = _spec_tables(rng, n)
    fsm = _tables_dev(tb, dev)
    bits = ts._make_rows(rng, m, n, bf16, shift=1)
    T, k, p = np.array([0.0, 0.7, 0.9][:b], np.float32), np.array([0, 5, 0][:b], np.int32), np.array([1.0, 0.9, 1.0][:b], np.float32)
    factor, presence = np.array([1.3, 1.0, 0.5][:b], np.float32), np.array([0.0, 0.7, 0.0][:b], np.float32)
    start = np.array([2, 2, 2] if kind == "unconstrains" else [0, 1, 3], np.int32)[:b]
    ids = [np.unique(rng.integers(0, n, max(1, n // 100))) for _ in range(b)]
    seen0 = tp._seen_dev(pr.pack(ids, n), dev)
    u = rng.random((b, len_q)).astype(np.float32)
    _, raw = ts._logits_dev(bits, ld, bf16, dev)
    # the drafts: the loop's own picks under "every draft accepted"
    drafts = np.empty((b, K), np.int64)
    for t in range(b):
        toks, _, _ = _sequential(ops, dev, raw[t * len_q:(t + 1) * len_q], tb, fsm, start[t], seen0[t], None, (T[t], k[t], p[t]), u[t], factor[t],
                                 presence[t], n)
        drafts[t] = toks[:K]
    mid = min(K // 2, 1)                                                    # in front of the ring's exit: the row's state constrains
    cut = np.zeros(b, bool)                                                 # the tasks whose draft `mid` cannot be accepted
    if kind == "disallowed":
        for t in range(b):
            s = fsm_ref.chain(tb, start[t], drafts[t, :mid], n)[-1]
            banned = [i for i in range(n) if 0 <= s < tb.S and not fsm_ref.allowed(tb, s, i)]
            if banned and not so.is_plain_bits(fsm_ref.masked(bits[t * len_q + mid], tb, s, bf16), bf16):
                drafts[t, mid], cut[t] = banned[0], True
        assert cut.any()
    elif kind == "minus_one":
        drafts[:, mid], cut[:] = -1, True
    want_tok, want_states, want_seen = [], [], []
    for t in range(b):
        toks, states, seen_t = _sequential(ops, dev, raw[t * len_q:(t + 1) * len_q], tb, fsm, start[t], seen0[t], drafts[t], (T[t], k[t], p[t]),
                                           u[t], factor[t], presence[t], n)
        want_tok.append(toks), want_states.append(states), want_seen.append(seen_t)
    st = _to(start, np.int32, dev)
    row_states = torch.full((b, len_q), -77, dtype=torch.int32, device=dev)
    seen = seen0.clone()
    out = tso._spec_call(ops, dev, raw, drafts, T, k, p, u, b, len_q, rep_penalty=_to(factor, np.float32, dev),
                         presence=_to(presence, np.float32, dev), seen=seen, fsm=fsm, fsm_state=st, row_states=row_states)
    torch.cuda.synchronize()
    acc, got, rs = _np(out["accepted"]), _np(out["out_tokens"]), _np(row_states)
    for t in range(b):
        a = len(want_tok[t]) - 1
        assert acc[t] == a and got[t, :a + 1].tolist() == want_tok[t] and (got[t, a + 1:] == -1).all(), (t, acc[t], got[t], want_tok[t])
        assert rs[t, :a + 1].tolist() == want_states[t], (t, rs[t], want_states[t])
        assert int(st[t]) == want_states[t][-1]
        _same(seen[t], want_seen[t].view(-1), (t, "seen"))
        chain = fsm_ref.chain(tb, start[t], drafts[t], n)
        for i in range(a + 1, len_q):                                       # behind the bonus token: some delta of the row's chained state
            s = chain[i]
            assert rs[t, i] == s or (0 <= s < tb.S and (rs[t, i] == tb.default[s] or rs[t, i] in tb.exc_next[tb.exc_off[s]:tb.exc_off[s + 1]]))
    if kind in ("accepted", "unconstrains"):
        assert (acc == K).all()
    assert (acc[cut] <= mid).all()
    if kind == "unconstrains":                                              # state 2 leaves the grammar unless the pick is an exception
        chains = [fsm_ref.chain(tb, start[t], drafts[t], n) for t in range(b)]
        assert any(not 0 <= c[1] < tb.S for c in chains) or b == 1


# ---- 5. admission -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_grammar", [True, False], ids=["grammar", "plain-blob"])
@pytest.mark.parametrize("b,which", [(5, "scattered"), (33, "all"), (1, "one")])
def test_admit_fsm_equals_the_reference(dev, b, which, with_grammar):
    """zl_slots_admit_fsm against fsm_ref.admit, bit for bit on every tensor from garbage states: admitted slots get the start state
    and the pending override wherever the rule says pending, parked slots -1, every other slot's rows stay (fsm_state included); a
    blob without grammar requests through the new entry gives zl_slots_admit's rows"""
    from zhilight_amd import ops
    vocab, groups = 1003, host.ALL
    rng = np.random.default_rng(100 * b + with_grammar)
    entries, w = host.scenario(rng, b, vocab, groups, which)
    w = dict(w, grammar=True)
    ctx, sampler, stop, lookup = host.garbage_states(rng, b, vocab, {k: v for k, v in w.items() if k != "grammar"}, groups, 1)
    parks = {s for s, rq in entries if rq is None}
    for s in parks:
        stop["finished"][s] = 2
    if with_grammar:
        for j, (s, rq) in enumerate(entries):
            if rq is not None and j % 3 != 2:
                rq["grammar"] = (int(rng.integers(0, 50)), int(rng.integers(0, vocab))) if j % 3 == 0 else int(rng.integers(0, 50))
    blob, h = ops.slots_pack(entries, vocab, w)
    assert bool(h["flags"] & 16) == (with_grammar and any(rq and "grammar" in rq for _, rq in entries))
    state = rng.integers(-5, 90, b).astype(np.int32)
    guards = []
    dctx, dsam, dstop, dlook = (tslots._upload(d, dev, guards) for d in (ctx, sampler, stop, lookup))
    dsam.fsm_state, g = ts._guarded(b, torch.int32, dev, state)
    guards.append(g)
    dnew, g = ts._guarded(b, torch.int32, dev)
    guards.append(g)
    before = [tslots._download(ns, like) for ns, like in ((dctx, ctx), (dsam, sampler), (dstop, stop), (dlook, lookup))]
    state0 = state.copy()
    new = np.full(b, 12345, np.int32)
    fsm_ref.admit(blob, ctx, sampler, stop, lookup, new, state)
    ops.slots_admit(blob, dctx.tokens, dctx.positions, dctx.placement, dctx.valid_lens, sampler=dsam, stop=dstop, lookup=dlook, draft_new=dnew,
                    parked_ok=parks)
    torch.cuda.synchronize()
    got = [tslots._download(ns, like) for ns, like in ((dctx, ctx), (dsam, sampler), (dstop, stop), (dlook, lookup))]
    for x, y, what in zip(got, (ctx, sampler, stop, lookup), ("ctx", "sampler", "stop", "lookup")):
        host.same(x, y, what)
    assert np.array_equal(_np(dnew), new) and np.array_equal(_np(dsam.fsm_state), state)
    ts._intact(guards)
    touched = {s for s, _ in entries}
    rest = [t for t in range(b) if t not in touched]
    assert np.array_equal(state[rest], state0[rest]) and all(state[s] == -1 for s in parks)
    for x, old in zip(got, before):
        if x is not None:
            for key in x:
                if key != "live":
                    assert x[key][rest].tobytes() == old[key][rest].tobytes(), key
    if not with_grammar:                                                    # ... and equals the old entry's result on the same garbage
        assert all(state[s] == -1 for s in touched)


# ---- 6. the C calls' refusals -------------------------------------------------------------------------------------------------------------
def test_abi_refusals(dev):
    from zhilight_amd import _lib
    lib = _lib.lib()
    n, rows, S = 70, 2, 3
    i32, f32 = torch.int32, torch.float32
    logits = torch.zeros((rows, n), dtype=torch.float16, device=dev)
    t = dict(T=torch.ones(rows, dtype=f32, device=dev), k=torch.zeros(rows, dtype=i32, device=dev), p=torch.ones(rows, dtype=f32, device=dev),
             u=torch.zeros(rows, dtype=f32, device=dev), tok=torch.zeros(rows, dtype=i32, device=dev),
             mask=torch.full((S, 3), -1, dtype=i32, device=dev), dflt=torch.zeros(S, dtype=i32, device=dev),
             off=torch.zeros(S + 1, dtype=i32, device=dev), etok=torch.zeros(1, dtype=i32, device=dev), enext=torch.zeros(1, dtype=i32, device=dev),
             state=torch.zeros(rows, dtype=i32, device=dev), drafts=torch.zeros((1, 1), dtype=i32, device=dev),
             acc=torch.zeros(1, dtype=i32, device=dev), out=torch.zeros((1, 2), dtype=i32, device=dev), rs=torch.zeros((1, 2), dtype=i32, device=dev))
    p = lambda name: C.c_void_p(0 if name is None else t[name].data_ptr())   # noqa: E731
    i = C.c_int64
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    six = ["mask", "dflt", "off", "etok", "enext", "state"]
    ptr = lambda name: None if name is None else t[name].data_ptr()          # noqa: E731

    def fsm_opts(names, mask_ld, s, e, rs=None):
        m, d, o, et, en, st = names
        return C.byref(_lib.SampleOpts(fsm_mask=ptr(m), fsm_mask_ld=mask_ld, fsm_default=ptr(d), fsm_exc_off=ptr(o), fsm_exc_tok=ptr(et),
                                       fsm_exc_next=ptr(en), fsm_states=s, fsm_exceptions=e, fsm_state=ptr(st), fsm_row_states=ptr(rs)))

    def plain(names=six, mask_ld=3, s=S, e=1, null_opts=False):
        opts = None if null_opts else fsm_opts(names, mask_ld, s, e)
        return lib.zl_sample_advance_ex(C.c_void_p(logits.data_ptr()), C.c_int(2), i(rows), i(n), i(n), p("T"), p("k"), p("p"), p(None),
                                        p(None), p("u"), p("tok"), *[p(None)] * 6, opts, stream)

    def spec(names=six, rs="rs", mask_ld=3, s=S, e=1, null_opts=False):
        opts = None if null_opts else fsm_opts(names, mask_ld, s, e, rs)
        return lib.zl_spec_sample_accept_ex(C.c_void_p(logits.data_ptr()), C.c_int(2), i(1), i(2), i(n), i(n), p("drafts"), p("T"), p("k"), p("p"),
                                            p(None), p(None), p("u"), *[p(None)] * 4, p("acc"), p("out"), *[p(None)] * 3, opts, stream)

    EINVAL, ESHAPE = -1, -2
    assert plain() == 0 and spec() == 0
    assert plain([None] * 6) == 0 and spec([None] * 6, rs=None) == 0        # no pointer of the group: the plain calls
    assert plain(null_opts=True) == 0 and spec(null_opts=True) == 0         # ... as NULL opts is
    for drop in range(6):                                                   # some but not all of the six
        names = list(six)
        names[drop] = None
        assert plain(names) == EINVAL and spec(names) == EINVAL, drop
    assert plain([None] * 5 + ["state"]) == EINVAL
    assert spec(rs=None) == EINVAL                                          # tables without row_states
    assert plain(s=0) == ESHAPE and plain(mask_ld=2) == ESHAPE and plain(s=1 << 31) == ESHAPE and plain(e=1 << 31) == ESHAPE
    assert spec(s=0) == ESHAPE and spec(mask_ld=2) == ESHAPE and spec(e=1 << 31) == ESHAPE
    torch.cuda.synchronize()


# ---- 7. the model: new_sampler(grammar=), load_grammar, admit, BatchServer ----------------------------------------------------------------
LEN_BUF, K = tslots.LEN_BUF, tslots.K
STEPS = 10
KW = dict(temperature=1.0, top_k=0, top_p=1.0)


class _Case:
    pass


@pytest.fixture(scope="module")
def case(dev):
    from zhilight_amd.grammar import from_choices
    c = _Case()
    rng, c.cfg, c.sd, c.model = _gptq_model(dev)
    c.vocab = c.cfg.vocab_size
    c.prompts = [rng.integers(0, c.vocab, s).astype(np.int32) for s in (5, 40, 17, 23, 9, 30)]
    ids = rng.choice(c.vocab - 1, 12, replace=False).tolist()
    c.eos = c.vocab - 1
    c.choices = [ids[0:3], ids[0:2], ids[3:4], [ids[4], ids[5], ids[4], ids[6], ids[7]], ids[8:12]]
    c.grammar = from_choices(c.vocab, c.choices, c.eos)
    c.other = from_choices(c.vocab, [ids[9:11], ids[2:3]], c.eos)
    return c


def _cut(row):
    row = list(row)
    return row[:row.index(-1)] if -1 in row else row


def _sample_run(c, seed, grammar, b=3, kw=KW):
    ctx = sv._fresh(c.model, c.prompts[:b])
    samp = c.model.new_sampler(ctx, **kw, seed=seed, grammar=grammar)
    stop = c.model.new_stopper(ctx, stop_ids=[c.eos])
    toks, _ = c.model.generate_sample(ctx, samp, STEPS, stop=stop)
    return [_cut(r) for r in toks.tolist()], stop.finished.tolist(), samp


@pytest.mark.parametrize("seed", [1, 77, 4242])
def test_generate_sample_emits_a_choice_then_eos(case, seed):
    c = case
    got, fin, samp = _sample_run(c, seed, [c.grammar, c.grammar, None])
    for j in (0, 1):
        assert got[j][-1] == c.eos and got[j][:-1] in c.choices and fin[j] == 1, (j, got[j])
    assert fin[2] != 1 or got[2][-1] == c.eos
    assert samp.fsm_state[2].item() == -1 and samp.fsm_used[0] == c.grammar.states
    # the unconstrained task draws what it draws without any grammar in the batch: its row is read as stored
    bare, _, _ = _sample_run(c, seed, None)
    assert got[2] == bare[2] and (got[0] != bare[0] or got[1] != bare[1])


def test_generate_lookup_emits_the_same_tokens(case):
    """speculation changes the speed, not the sample: under a grammar too.  The siblings' sampling parameters (test_gpu_sample_penalty.KW):
    a verify row's logits come from another GEMM route than a one-row step's, and the truncated distribution keeps the picks of the
    unconstrained task away from the low-probability classes where that difference decides"""
    c = case
    kw = dict(temperature=tp.KW["temperature"], top_k=tp.KW["top_k"], top_p=tp.KW["top_p"])
    want, fin, _ = _sample_run(c, 5, [c.grammar, None, c.other], kw=kw)
    ctx = sv._fresh(c.model, c.prompts[:3])
    look = c.model.new_lookup(ctx, c.prompts[:3], K)
    samp = c.model.new_sampler(ctx, **kw, seed=5, grammar=[c.grammar, None, c.other])
    stop = c.model.new_stopper(ctx, stop_ids=[c.eos])
    got, stats = c.model.generate_lookup(ctx, look, STEPS, sampler=samp, stop=stop)
    assert got == want and stats["finished"] == fin
    assert got[0][:-1] in c.choices and got[2][:-1] in _choices_of(c.other, c.eos)


def test_captured_steps_continue_the_eager_sequence_and_take_a_later_grammar(case):
    """one graph captured over step_sample: its replays continue the eager sequence; a grammar loaded AFTER the capture (the tables'
    pointers do not change) constrains a task from the step its state is set"""
    c = case
    want, _, _ = _sample_run(c, 9, [c.grammar, c.grammar, None])
    ctx = sv._fresh(c.model, c.prompts[:3])
    samp = c.model.new_sampler(ctx, **KW, seed=9, grammar_states=c.grammar.states + c.other.states, grammar_edges=64)
    assert c.model.load_grammar(samp, c.grammar) == 0
    samp.fsm_state.copy_(torch.tensor([0, 0, -1], dtype=torch.int32))
    stop = c.model.new_stopper(ctx, stop_ids=[c.eos])
    seq = [c.model.step_sample(ctx, samp, stop)[1].tolist()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gnxt = c.model.step_sample(ctx, samp, stop)
    for _ in range(1, 4):
        graph.replay()
        seq.append(gnxt.tolist())
    h = c.model.load_grammar(samp, c.other)                                 # no recapture
    assert h == c.grammar.states
    samp.fsm_state[2:3].fill_(h)
    for _ in range(4, STEPS):
        graph.replay()
        seq.append(gnxt.tolist())
    torch.cuda.synchronize()
    got = [_cut(r) for r in np.asarray(seq).T.tolist()]
    assert got[0] == want[0] and got[1] == want[1] and got[2][:4] == want[2][:4]
    tail = got[2][4:]
    assert tail[-1] == c.eos and tail[:-1] in _choices_of(c.other, c.eos)
    from zhilight_amd import ops
    with pytest.raises(ops.ZLError, match="full"):
        c.model.load_grammar(samp, c.grammar)
    samp.fsm_state.fill_(-1)
    c.model.clear_grammars(samp)
    assert c.model.load_grammar(samp, c.other) == 0
    samp.fsm_state[0:1].fill_(0)
    with pytest.raises(ops.ZLError, match="still inside"):
        c.model.clear_grammars(samp)


def _choices_of(automaton, eos):
    """the token sequences a from_choices automaton accepts (a walk over its trie)"""
    out, todo = [], [(automaton.start, [])]
    while todo:
        s, seq = todo.pop()
        for t, nxt in automaton.transitions[s].items():
            if t == eos:
                out.append(seq)
            else:
                todo.append((nxt, seq + [t]))
    return out


def test_without_grammar_arguments_the_state_and_the_tokens_are_todays(case):
    c = case
    ctx = sv._fresh(c.model, c.prompts[:3])
    samp = c.model.new_sampler(ctx, **KW, seed=3)
    assert samp.fsm is None and samp.fsm_state is None and "fsm" not in samp.opts() and not c.model.slot_widths(samp, None, None)["grammar"]
    a, _ = c.model.generate_sample(ctx, samp, 6)
    ctx = sv._fresh(c.model, c.prompts[:3])
    samp = c.model.new_sampler(ctx, **KW, seed=3, grammar_states=4, grammar_edges=4)      # tables, every task unconstrained
    assert samp.fsm_state.tolist() == [-1] * 3
    b_, _ = c.model.generate_sample(ctx, samp, 6)
    assert torch.equal(a, b_) and samp.fsm_state.tolist() == [-1] * 3


def _serve(c, grammar_states, constrained, prompts=None):
    from zhilight_amd.serving import BatchServer
    kw = dict(grammar_states=grammar_states, grammar_edges=64) if grammar_states else {}
    srv = BatchServer(c.model, 3, LEN_BUF, poll=4, **kw)
    h = srv.load_grammar(c.grammar) if grammar_states else None
    for i, p in enumerate(c.prompts if prompts is None else prompts):
        rq = dict(temperature=1.0, seed=100 + i, stop_ids=[c.eos], max_new_tokens=8)
        if i in constrained:
            rq["grammar"] = h
        srv.submit(p, **rq)
    return srv, srv.run()


def test_batch_server_with_half_the_requests_constrained(case):
    from zhilight_amd import ops
    c = case
    srv, res = _serve(c, c.grammar.states, (0, 2, 4))
    _, bare = _serve(c, 0, ())
    for r in (0, 2, 4):                                                     # a listed choice, the first token included, then EOS
        assert res[r]["first_token"] is None and res[r]["reason"] == 1, r
        assert res[r]["tokens"][-1] == c.eos and res[r]["tokens"][:-1] in c.choices, (r, res[r]["tokens"])
    for r in (1, 3, 5):                                                     # untouched by the grammar next to them
        assert (res[r]["first_token"], res[r]["tokens"], res[r]["reason"]) == (bare[r]["first_token"], bare[r]["tokens"], bare[r]["reason"]), r
    # bit for bit, log-probabilities included, where the prompt encode runs at the same shape on both servers: one round of three
    # requests, the constrained ones' prompts one token shorter on the server without grammars (admit encodes prompt[:-1])
    _, one = _serve(c, c.grammar.states, (0, 2), c.prompts[:3])
    _, two = _serve(c, 0, (), [c.prompts[0][:-1], c.prompts[1], c.prompts[2][:-1]])
    assert (one[1]["first_token"], one[1]["tokens"], one[1]["reason"]) == (two[1]["first_token"], two[1]["tokens"], two[1]["reason"])
    assert np.array_equal(np.asarray(one[1]["logprobs"], np.float32).view(np.int32), np.asarray(two[1]["logprobs"], np.float32).view(np.int32))
    assert one[0]["tokens"][:-1] in c.choices and one[2]["tokens"][:-1] in c.choices
    with pytest.raises(ops.ZLError):
        srv.submit(c.prompts[0][:1], grammar=0)                             # a 1-token prompt with a grammar
    with pytest.raises(ops.ZLError):
        srv.submit(c.prompts[0], grammar=srv.sampler.fsm_used[0])           # no such handle
    srv0, _ = _serve(c, 0, ())
    with pytest.raises(ops.ZLError):
        srv0.submit(c.prompts[0], grammar=0)                                # a server without tables
