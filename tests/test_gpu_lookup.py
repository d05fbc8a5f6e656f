"""The prompt-lookup drafter on the GPU: zl_lookup_draft bit for bit against tests/lookup_ref.py (drafts, match, lengths and the WHOLE
history buffer with a guard region behind every buffer), and LLaMA.new_lookup / step_lookup / generate_lookup on the small GPTQ model of
test_gpu_spec_verify.py -- composition with verify (bit-identical), rounds against one oracle pass, capture, refusals."""
import numpy as np
import pytest
import torch

import lookup_ref
import test_gpu_spec_verify as sv
from test_gpu_prefill_batch import _gptq_model
from test_gpu_score import AllRowsOracle

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
CAP = 4099                                  # odd: rows start at every alignment
GUARD, POISON = 64, -7
_np = sv._np


def _guarded(shape, dev, fill=POISON):
    """an int32 tensor of `shape` at the start of a buffer with GUARD poisoned elements behind it -> (tensor, guard view)"""
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), fill, dtype=torch.int32, device=dev)
    return flat[:n].view(*shape), flat[n:]


def _check(hist, lens, k, mx, mn, new, dev):
    """one ops.lookup_draft call on copies of hist / lens against the reference -> (history, lens, drafts, match) as numpy"""
    from zhilight_amd import ops
    b, cap = hist.shape
    h_dev, h_guard = _guarded((b, cap), dev)
    h_dev.copy_(torch.from_numpy(hist))
    l_dev, l_guard = _guarded((b,), dev)
    l_dev.copy_(torch.from_numpy(np.asarray(lens, np.int32)))
    d_dev, d_guard = _guarded((b, k), dev)
    m_dev, m_guard = _guarded((b, 2), dev)
    new_dev = None if new is None else torch.from_numpy(np.asarray(new, np.int32)).to(dev)
    d, m = ops.lookup_draft(h_dev, l_dev, k, mx, mn, new_tokens=new_dev, drafts=d_dev, match=m_dev)
    assert d.data_ptr() == d_dev.data_ptr() and m.data_ptr() == m_dev.data_ptr()
    rh, rl, rd, rm = lookup_ref.lookup(hist, lens, k, mx, mn, new)
    got = tuple(_np(t) for t in (h_dev, l_dev, d_dev, m_dev))
    for name, g, r in zip(("history", "hist_lens", "drafts", "match"), got, (rh, rl, rd, rm)):
        bad = np.argwhere(g != r)
        assert bad.size == 0, (name, bad[:4].tolist(), g[tuple(bad[0])], r[tuple(bad[0])])
    for guard in (h_guard, l_guard, d_guard, m_guard):
        assert bool((guard == POISON).all())
    if new is not None:
        assert np.array_equal(_np(new_dev), np.asarray(new, np.int32))
    return got


def _histories(rng, lengths, alphabet):
    """(len(lengths), CAP) rows of random ids over `alphabet` symbols per task (a range: drawn per task), POISON-free tail of 0"""
    hist = np.zeros((len(lengths), CAP), np.int32)
    for t, L in enumerate(lengths):
        a = alphabet if isinstance(alphabet, int) else int(rng.integers(alphabet[0], alphabet[1] + 1))
        hist[t, :L] = rng.integers(0, a, L)
    return hist


@pytest.mark.parametrize("ngram", [(1, 1), (3, 1), (3, 2), (8, 2), (16, 16)])
@pytest.mark.parametrize("k", [1, 3, 7, 31])
@pytest.mark.parametrize("b", [1, 3, 8])
def test_kernel_against_reference(dev, b, k, ngram):
    """every boundary length at every batch size, mixed within a batch; 2 - 4 symbols (matches and ties everywhere) and 2^20 symbols
    (none, bar a birthday pair)"""
    rng = np.random.default_rng(1000 * b + 10 * k + ngram[0])
    order = [int(v) for v in rng.permutation(LENGTHS)]
    order += [int(v) for v in rng.choice(LENGTHS, -len(order) % b)]
    matched = 0
    for alphabet in ((2, 4), 1 << 20):
        for i in range(0, len(order), b):
            lens = order[i:i + b]
            _, _, _, m = _check(_histories(rng, lens, alphabet), lens, k, ngram[0], ngram[1], None, dev)
            matched += int((m[:, 0] > 0).sum())
            if alphabet == 1 << 20 and ngram[1] >= 2:
                assert (m[:, 0] == 0).all()
    assert matched > 0 or ngram == (16, 16)


def test_planted_matches(dev):
    """histories of distinct ids (a permutation: no accidental match) with one planted n-gram"""
    rng = np.random.default_rng(5)
    L, k = 700, 3
    base = rng.permutation(1 << 16)[:L].astype(np.int32)
    rows, expect = [], []
    h = base.copy()                                  # the only match at s = 0 (n = 3)
    h[L - 3:] = h[:3]
    rows.append(h)
    expect.append(((3, 0), h[3:6].tolist()))
    h = base.copy()                                  # the only match ends at L - 1: x x x at the end, n = 2 at s = L - 3
    h[L - 3:] = h[L - 1]
    rows.append(h)
    expect.append(((2, L - 3), [int(h[L - 1]), -1, -1]))
    h = base.copy()                                  # a match one token short of a full continuation loses to an earlier full one
    h[100] = h[L - k] = h[L - 1]
    rows.append(h)
    expect.append(((1, 100), h[101:104].tolist()))
    h = base.copy()                                  # ... and wins as soon as it is full
    h[100] = h[L - k - 1] = h[L - 1]
    rows.append(h)
    expect.append(((1, L - k - 1), h[L - k:L].tolist()))
    hist = np.zeros((len(rows), CAP), np.int32)
    hist[:, :L] = np.stack(rows)
    _, _, d, m = _check(hist, [L] * len(rows), k, 3, 1, None, dev)
    for t, ((n, s), cont) in enumerate(expect):
        assert m[t].tolist() == [n, s] and d[t].tolist() == cont, t


@pytest.mark.parametrize("n_new", [1, 4, 32])
def test_append(dev, n_new):
    """the append path: rows without a negative id, with the first one at 0 / in the middle, with ids BEHIND it (never appended); cap
    reached exactly, exceeded by one, exceeded mid-row, exceeded long ago.  _check compares the whole buffer (the neighbouring rows)
    and the guard behind it"""
    rng = np.random.default_rng(n_new)
    cap, mid = 50, n_new // 2
    lens = [cap - n_new, cap - n_new + 1, cap - mid, 20, 20, cap + 5, cap - 1, 0]
    b = len(lens)
    hist = np.full((b, cap), 3, np.int32)
    for t, L in enumerate(lens):
        hist[t, :min(L, cap)] = rng.integers(0, 3, min(L, cap))
    new = rng.integers(0, 3, (b, n_new)).astype(np.int32)
    new[3, 0] = -1                                  # nothing appended, ids behind the -1
    new[4, mid] = -5                                # a prefix appended, ids behind the negative one
    new[6, 0] = 2                                   # one slot left
    h, l, d, m = _check(hist, lens, 3, 3, 1, new, dev)
    assert l.tolist() == [cap, cap + 1, cap - mid + n_new, 20, 20 + mid, cap + 5 + n_new, cap - 1 + n_new, n_new]
    assert (d[1] == -1).all() and m[1].tolist() == [0, -1] and (d[5] == -1).all()       # overflowed rows draft nothing
    assert m[0, 0] > 0 and np.array_equal(h[0, cap - n_new:], new[0])                    # cap reached exactly: still drafting
    assert np.array_equal(h[3], hist[3]) and np.array_equal(h[5], hist[5])
    assert np.array_equal(h[7, :n_new], new[7]) and (h[7, n_new:] == 3).all()            # an empty history takes the append


def test_two_calls_equal_one_on_the_concatenation(dev):
    rng = np.random.default_rng(9)
    lens = [1, 64, 300, 1023, 0]
    hist = _histories(rng, lens, (2, 4))
    first, second = rng.integers(0, 3, (5, 3)).astype(np.int32), rng.integers(0, 3, (5, 2)).astype(np.int32)
    first[2, 1] = -1                                # one id, then two: three in all
    h1, l1, _, _ = _check(hist, lens, 3, 3, 1, first, dev)
    two = _check(h1, l1, 3, 3, 1, second, dev)
    cat = np.concatenate([first, second], axis=1)
    cat[2] = [first[2, 0], second[2, 0], second[2, 1], -1, -1]
    one = _check(hist, lens, 3, 3, 1, cat, dev)
    for g, r in zip(two, one):
        assert np.array_equal(g, r)


def test_lookup_draft_does_not_synchronise(dev):
    from zhilight_amd import ops
    rng = np.random.default_rng(2)
    hist = torch.from_numpy(_histories(rng, [300, 1025], 3)).to(dev)
    lens = torch.tensor([300, 1025], dtype=torch.int32, device=dev)
    new = torch.tensor([[1, 2, -1, 0], [0, 0, 1, 2]], dtype=torch.int32, device=dev)
    ops.lookup_draft(hist, lens, 3, new_tokens=new)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d, m = ops.lookup_draft(hist, lens, 3, new_tokens=new)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _np(lens).tolist() == [304, 1033] and d.shape == (2, 3) and m.shape == (2, 2)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
LENS, LEN_BUF, K = sv.LENS, sv.LEN_BUF, sv.K
MOTIF_LENS = [16, 40, 24]
LOOKUP = ("history", "hist_lens", "drafts", "match")


class _Case:
    pass


@pytest.fixture(scope="module")
def case(oracle, dev):
    c = _Case()
    rng, c.cfg, c.sd, c.model = _gptq_model(dev)
    c.vocab, c.oracle = c.cfg.vocab_size, oracle
    c.prompts = [rng.integers(0, c.vocab, s).astype(np.int32) for s in LENS]
    c.motifs = [np.tile(rng.integers(0, c.vocab, 8), 5)[:s].astype(np.int32) for s in MOTIF_LENS]
    return c


def _ref_state(prompts, t0, cap, k, mx, mn):
    hist = np.zeros((len(prompts), cap), np.int32)
    for j, p in enumerate(prompts):
        hist[j, :len(p)] = p
    return lookup_ref.lookup(hist, [len(p) for p in prompts], k, mx, mn, np.asarray(t0, np.int32).reshape(-1, 1))


def _assert_state(state, ref):
    for name, r in zip(LOOKUP, ref):
        assert np.array_equal(_np(getattr(state, name)), r), name


def _admissible(c, prompts, t0, emitted):
    """test_four_rounds_with_a_repeating_drafter's check: every emitted token within 2 bar of the row maximum of ONE oracle pass"""
    om = AllRowsOracle(c.oracle, c.cfg, c.sd, 128, len(prompts), LEN_BUF)
    for j, p in enumerate(prompts):
        rows = om.prefill_all(j, list(p) + [int(t0[j])] + emitted[j][:-1])
        ref = rows[len(p):len(p) + len(emitted[j])]
        bar = sv._bar(ref)
        for i, t in enumerate(emitted[j]):
            assert ref[i, t] >= ref[i].max() - 2 * bar, (j, i)


def test_new_lookup(case):
    c = case
    ctx = sv._fresh(c.model, c.prompts)
    state = c.model.new_lookup(ctx, c.prompts, K)
    assert (state.k, state.max_ngram, state.min_ngram) == (K, 3, 1) and state.history.shape == (len(LENS), LEN_BUF + 1)
    _assert_state(state, _ref_state(c.prompts, _np(ctx.tokens), LEN_BUF + 1, K, 3, 1))
    assert _np(state.hist_lens).tolist() == [s + 1 for s in LENS]
    small = c.model.new_lookup(ctx, [torch.from_numpy(p) for p in c.prompts], 2, max_ngram=2, min_ngram=2, cap=41)    # tensors, a tight cap
    _assert_state(small, _ref_state(c.prompts, _np(ctx.tokens), 41, 2, 2, 2))


def test_step_lookup_is_verify_on_the_looked_up_drafts(case, dev):
    """histories seeded with the greedy continuation behind t0: with max_ngram = 1 the pending t0 finds itself there and the drafts are
    the greedy tokens (wherever t0 does not occur again).  Same code path as verify on those drafts: bit-identity"""
    c = case
    twin = sv._fresh(c.model, c.prompts)
    t0 = _np(twin.tokens).copy()
    g = np.stack([_np(c.model.step_greedy(twin)[1]).astype(np.int32) for _ in range(K)], axis=1)
    seeded = [np.concatenate([p, [t0[j]], g[j]]).astype(np.int32) for j, p in enumerate(c.prompts)]
    ref = _ref_state(seeded, t0, LEN_BUF + 1, K, 1, 1)
    assert any(ref[2][j].tolist() == g[j].tolist() for j in range(len(LENS)))
    ctx = sv._fresh(c.model, c.prompts)
    state = c.model.new_lookup(ctx, seeded, K, max_ngram=1)
    _assert_state(state, ref)
    res = c.model.step_lookup(ctx, state)
    other = sv._fresh(c.model, c.prompts)
    exp = c.model.verify(other, torch.from_numpy(ref[2]).to(dev))
    assert torch.equal(res.logits, exp.logits) and torch.equal(res.accepted, exp.accepted) and torch.equal(res.tokens, exp.tokens)
    for n in sv.STATE:
        assert torch.equal(getattr(ctx, n), getattr(other, n)), n
    assert ctx.steps_left == other.steps_left
    for j in range(len(LENS)):
        if ref[2][j].tolist() == g[j].tolist():
            assert int(res.accepted[j]) == K
    _assert_state(state, lookup_ref.lookup(ref[0], ref[1], K, 1, 1, _np(res.tokens)))


def test_six_rounds_on_repeating_prompts(case):
    """prompts = an 8-id motif repeated: lookup matches as soon as the model emits an id of the motif (the first pending token need
    not be one: on this model the first round has no match, later rounds accept 8 drafts).  After every round the history is prompt +
    [t0] + emitted, the drafts are the reference's over it and the positions follow; at the end every emitted token is admissible
    under one oracle pass"""
    c = case
    ctx = sv._fresh(c.model, c.motifs)
    t0 = _np(ctx.tokens).copy()
    state = c.model.new_lookup(ctx, c.motifs, K)
    print("first-round matches (n, start):", _np(state.match).tolist())       # a match as soon as the pending token is one of the motif's
    emitted, accepted = [[] for _ in MOTIF_LENS], 0
    for _ in range(6):
        res = c.model.step_lookup(ctx, state)
        acc, out = _np(res.accepted), _np(res.tokens)
        accepted += int(acc.sum())
        lens, hist = _np(state.hist_lens), _np(state.history)
        for j, p in enumerate(c.motifs):
            emitted[j] += [int(t) for t in out[j, :acc[j] + 1]]
            full = list(p) + [int(t0[j])] + emitted[j]
            assert lens[j] == len(full) and hist[j, :lens[j]].tolist() == full
            d, m = lookup_ref.draft(full, K, 3, 1)
            assert _np(state.drafts)[j].tolist() == d and _np(state.match)[j].tolist() == list(m)
        assert _np(ctx.positions).tolist() == [len(p) + len(e) for p, e in zip(c.motifs, emitted)]
    print("accepted drafts over 6 rounds x 3 tasks (synthetic weights):", accepted)
    _admissible(c, c.motifs, t0, emitted)


def _snapshot(ctx, state):
    return ([getattr(ctx, n).clone() for n in sv.STATE], [t.clone() for t in ctx.kv], [getattr(state, n).clone() for n in LOOKUP], ctx.steps_left)


def _restore(ctx, state, snap):
    for n, v in zip(sv.STATE, snap[0]):
        getattr(ctx, n).copy_(v)
    for t, v in zip(ctx.kv, snap[1]):
        t.copy_(v)
    for n, v in zip(LOOKUP, snap[2]):
        getattr(state, n).copy_(v)
    ctx.steps_left = snap[3]


def test_step_lookup_no_sync_and_graph_replay(case, dev):
    c = case
    ctx = sv._fresh(c.model, c.motifs)
    state = c.model.new_lookup(ctx, c.motifs, K)
    c.model.step_lookup(ctx, state)                                 # warm: verify's tables, code objects
    torch.cuda.synchronize()
    snap = _snapshot(ctx, state)
    torch.cuda.set_sync_debug_mode("error")
    try:
        e = c.model.step_lookup(ctx, state)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    eager = [t.clone() for t in e] + _snapshot(ctx, state)[0] + _snapshot(ctx, state)[2]
    _restore(ctx, state, snap)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = c.model.step_lookup(ctx, state)
    _restore(ctx, state, snap)
    graph.replay()
    torch.cuda.synchronize()
    replayed = list(r) + [getattr(ctx, n) for n in sv.STATE] + [getattr(state, n) for n in LOOKUP]
    assert len(replayed) == len(eager)
    for i, (g, x) in enumerate(zip(replayed, eager)):
        assert torch.equal(g, x), i


def test_generate_lookup(case):
    c = case
    ctx = sv._fresh(c.model, c.motifs)
    t0 = _np(ctx.tokens).copy()
    state = c.model.new_lookup(ctx, c.motifs, K)
    toks, stats = c.model.generate_lookup(ctx, state, 10)
    b, steps = len(MOTIF_LENS), stats["steps"]
    assert 3 <= steps <= 10 and ctx.steps_left == LEN_BUF - max(MOTIF_LENS) - steps * (K + 1)
    assert [len(t) for t in toks] == [10] * b and min(stats["emitted"]) >= 10
    assert stats["emitted"] == [steps + a for a in stats["accepted"]]
    assert stats["mean_accepted"] == sum(stats["accepted"]) / (steps * b)
    lens, hist = _np(state.hist_lens), _np(state.history)
    for j, p in enumerate(c.motifs):                                # the history holds everything emitted; the lists are its first 10
        assert lens[j] == len(p) + 1 + stats["emitted"][j]
        assert hist[j, len(p) + 1:len(p) + 11].tolist() == toks[j]
    assert _np(ctx.positions).tolist() == [len(p) + e for p, e in zip(c.motifs, stats["emitted"])]
    _admissible(c, c.motifs, t0, toks)
    # out of room: 64-slot buffers, 24 slots left behind the longest prompt = 6 steps of K + 1 rows, then a clean stop
    tight = c.model.new_context(b, 64, 0)
    c.model.prefill_batch(tight, list(range(b)), [torch.from_numpy(p) for p in c.motifs])
    st = c.model.new_lookup(tight, c.motifs, K)
    toks, stats = c.model.generate_lookup(tight, st, 1000)
    assert stats["steps"] == 6 and tight.steps_left == 0 and [len(t) for t in toks] == stats["emitted"]
    assert c.model.generate_lookup(tight, st, 1000) == ([[], [], []], {"steps": 0, "emitted": [0] * b, "accepted": [0] * b, "mean_accepted": 0.0})


def test_refusals(case, dev, monkeypatch):
    from zhilight_amd import ops
    c, model = case, case.model
    ctx = sv._fresh(model, c.prompts)
    with pytest.raises(ops.ZLError, match="INT8 KV"):
        model.new_lookup(model.new_context(3, LEN_BUF, 4, kv_cache_dtype="int8"), c.prompts, K)
    with pytest.raises(ops.ZLError, match="32 rows"):              # 3 * (10 + 1) = 33
        model.new_lookup(ctx, c.prompts, 10)
    with pytest.raises(ops.ZLError, match="32 rows"):
        model.new_lookup(ctx, c.prompts, 0)
    with pytest.raises(ops.ZLError, match="histories"):
        model.new_lookup(ctx, c.prompts[:2], K)
    with pytest.raises(ops.ZLError, match="do not fit cap"):       # 40 ids and the pending one need cap 41
        model.new_lookup(ctx, c.prompts, K, cap=40)
    with pytest.raises(ops.ZLError, match="ids outside"):
        model.new_lookup(ctx, [c.prompts[0], c.prompts[1], np.array([1, c.vocab])], K)
    with pytest.raises(ops.ZLError, match="ids outside"):
        model.new_lookup(ctx, [c.prompts[0], np.array([-1]), c.prompts[2]], K)
    with pytest.raises(ops.ZLError, match="min_ngram"):
        model.new_lookup(ctx, c.prompts, K, max_ngram=2, min_ngram=3)
    with pytest.raises(ops.ZLError, match="cap >= 2"):
        model.new_lookup(ctx, [[], [], []], K, cap=1)
    with monkeypatch.context() as mp:
        mp.setattr(model.cfg, "dim_head", 64)
        with pytest.raises(ops.ZLError, match="head size 128"):
            model.new_lookup(ctx, c.prompts, K)
    with monkeypatch.context() as mp:
        mp.setattr(model, "tp", object())
        with pytest.raises(ops.ZLError, match="tensor parallelism"):
            model.new_lookup(ctx, c.prompts, K)
    state = model.new_lookup(ctx, c.prompts, K)
    with pytest.raises(ops.ZLError, match="INT8 KV"):              # step_lookup: whatever verify refuses
        model.step_lookup(model.new_context(3, LEN_BUF, 4, kv_cache_dtype="int8"), state)
    with pytest.raises(ops.ZLError, match="another batch size"):
        model.step_lookup(model.new_context(2, LEN_BUF, 4), state)
    with pytest.raises(ops.ZLError, match="'auto', 'causal' or 'rows'"):
        model.step_lookup(ctx, state, attn="tree")
    short = model.new_context(3, LEN_BUF, LEN_BUF - K)              # three slots left, four rows wanted
    before = [_np(getattr(state, n)).copy() for n in LOOKUP]
    with pytest.raises(ops.ZLError, match="do not fit the KV buffers"):
        model.step_lookup(short, state)
    for n, v in zip(LOOKUP, before):                                # a refused step leaves the drafter's state alone
        assert np.array_equal(_np(getattr(state, n)), v), n
