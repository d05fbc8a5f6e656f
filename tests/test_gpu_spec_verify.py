"""LLaMA.verify -- one speculative step over K draft tokens per task through the decode layer loop -- on a small GPTQ model against the
CPU oracle's prompt pass over prompt + [t0] + drafts (rows p .. p + K are the step's reference logits), the numpy accept reference,
and the state / K/V / roll-back behaviour the issue's contract lists."""
import numpy as np
import pytest
import torch

import spec_ref
from test_gpu_prefill_batch import _close, _gptq_model
from test_gpu_score import AllRowsOracle

pytestmark = pytest.mark.gpu

LENS, LEN_BUF, K = [5, 40, 17], 128, 3
EXPECT = [3, 1, 0]
STATE = ("tokens", "positions", "placement", "valid_lens")


def _np(t):
    return t.detach().cpu().numpy()


def _bar(ref):
    return (1e-3 + 2.0 ** -11) * np.abs(ref).max()


def _state(ctx):
    return [_np(getattr(ctx, n)).copy() for n in STATE]


def _fresh(model, prompts):
    ctx = model.new_context(len(prompts), LEN_BUF, 0)
    model.prefill_batch(ctx, list(range(len(prompts))), [torch.from_numpy(p) for p in prompts])
    return ctx


class _Case:
    pass


@pytest.fixture(scope="module")
def case(oracle, dev):
    """the model, one verify call from the state prefill_batch leaves, two greedy steps behind it, and the oracle's rows"""
    c = _Case()
    rng, cfg, sd, model = _gptq_model(dev)
    c.cfg, c.sd, c.model, c.vocab = cfg, sd, model, cfg.vocab_size
    c.prompts = [rng.integers(0, cfg.vocab_size, s).astype(np.int32) for s in LENS]
    twin = _fresh(model, c.prompts)
    c.t0 = _np(twin.tokens).copy()
    g = np.stack([_np(model.step_greedy(twin)[1]).astype(np.int32) for _ in range(K)], axis=1)       # (B, K): g1 .. g3 per task
    c.drafts = g.copy()
    c.drafts[1, 1] = (g[1, 1] + 1) % c.vocab
    c.drafts[2, 0] = (g[2, 0] + 1) % c.vocab
    c.ctx = _fresh(model, c.prompts)
    assert np.array_equal(_np(c.ctx.tokens), c.t0)
    c.before, c.steps_before = _state(c.ctx), c.ctx.steps_left
    c.drafts_dev = torch.from_numpy(c.drafts).to(dev)
    res = model.verify(c.ctx, c.drafts_dev, attn="causal")
    c.logits = _np(res.logits.float()).astype(np.float64).reshape(len(LENS), K + 1, c.vocab)
    c.accepted, c.tokens = _np(res.accepted).copy(), _np(res.tokens).copy()
    c.after, c.steps_after = _state(c.ctx), c.ctx.steps_left
    c.kv_after = [[_np(c.ctx.kv[j][li, :, p:p + K + 1]).astype(np.float64) for li in range(cfg.num_layers)] for j, p in enumerate(LENS)]
    # two greedy steps behind the verify (the roll-back check): logits, and the tokens they were fed
    c.follow = []
    for _ in range(2):
        fed = _np(c.ctx.tokens).copy()
        lg, _ = model.step_greedy(c.ctx)
        c.follow.append((fed, _np(lg.float()).astype(np.float64)))
    om = AllRowsOracle(oracle, cfg, sd, 128, len(LENS), LEN_BUF)
    c.ref, c.ref_kv = [], []
    for j, p in enumerate(LENS):
        rows = om.prefill_all(j, list(c.prompts[j]) + [int(c.t0[j])] + [int(t) for t in c.drafts[j]])
        c.ref.append(rows[p:p + K + 1])
        c.ref_kv.append([[oracle.u2h(b[li][j][p:p + K + 1]).astype(np.float64) for b in (om.kb, om.vb)] for li in range(cfg.num_layers)])
    c.oracle = oracle
    return c


def _margins_decide(c, j):
    """True where the oracle's rows decide task j's count by more than 2 bar: rows before EXPECT[j] put their draft first by that
    margin, row EXPECT[j] (if a draft sits there) leaves its draft that far behind the maximum"""
    ref, bar, n = c.ref[j], _bar(c.ref[j]), EXPECT[j]
    for i in range(n):
        top = np.sort(ref[i])[-2:]
        if not (int(ref[i].argmax()) == c.drafts[j, i] and top[1] - top[0] > 2 * bar):
            return False
    return n == K or ref[n, c.drafts[j, n]] < ref[n].max() - 2 * bar


def test_logits_match_the_oracle_rows(case):
    for j in range(len(LENS)):
        ok, err = _close(case.logits[j], case.ref[j], 1e-3)
        print("task", j, "max |logits - ref| / max|ref| =", err)
        assert ok, (j, err)


def test_accept_and_state_are_the_reference_on_the_returned_logits(case):
    c = case
    picks = spec_ref.argmax_rows(c.logits.reshape(-1, c.vocab)).reshape(len(LENS), K + 1)
    acc, out = spec_ref.accept(picks, c.drafts)
    assert np.array_equal(c.accepted, acc) and np.array_equal(c.tokens, out)
    for name, got, ref in zip(STATE, c.after, spec_ref.advance(acc, out, *c.before)):
        assert np.array_equal(got, ref), name
    assert c.steps_after == c.steps_before - (K + 1)


def test_every_pick_is_admissible_and_counts_follow(case):
    c = case
    picks = spec_ref.argmax_rows(c.logits.reshape(-1, c.vocab)).reshape(len(LENS), K + 1)
    decided = []
    for j in range(len(LENS)):
        bar = _bar(c.ref[j])
        for i in range(K + 1):
            assert c.ref[j][i, picks[j, i]] >= c.ref[j][i].max() - 2 * bar, (j, i)
        decided.append(_margins_decide(c, j))
        if decided[-1]:
            assert c.accepted[j] == EXPECT[j], (j, c.accepted[j])
    print("accepted", c.accepted.tolist(), "decided by the oracle's margins:", decided)


def test_kv_rows_of_the_step(case):
    c = case
    for j in range(len(LENS)):
        for li in range(c.cfg.num_layers):
            for kv in (0, 1):
                g, r = c.kv_after[j][li][kv], c.ref_kv[j][li][kv]
                assert np.abs(g - r).max() <= 2.0 ** -9 * np.abs(r).max(), (j, li, kv)


def test_greedy_steps_after_the_roll_back(case):
    """two step_greedy calls behind the verify against the oracle teacher-forced over the accepted sequence; task 2's first step
    overwrites the slot of a rejected draft"""
    c = case
    om = AllRowsOracle(c.oracle, c.cfg, c.sd, 128, len(LENS), LEN_BUF)
    for j, p in enumerate(LENS):
        n = int(c.accepted[j])
        seq = list(c.prompts[j]) + [int(c.t0[j])] + [int(t) for t in c.tokens[j, :n + 1]]
        assert c.follow[0][0][j] == seq[-1]
        seq.append(int(c.follow[1][0][j]))
        rows = om.prefill_all(j, seq)
        for s in range(2):
            ref = rows[p + n + 1 + s]
            ok, err = _close(c.follow[s][1][j], ref, 1e-3)
            assert ok, (j, s, err)


def test_rows_route_agrees(case, dev):
    c = case
    ctx = _fresh(c.model, c.prompts)
    res = c.model.verify(ctx, c.drafts_dev, attn="rows")
    lg = _np(res.logits.float()).astype(np.float64).reshape(len(LENS), K + 1, c.vocab)
    for j in range(len(LENS)):
        assert np.abs(lg[j] - c.logits[j]).max() <= 2 * _bar(c.ref[j]), j
        if _margins_decide(c, j):
            assert int(res.accepted[j]) == int(c.accepted[j]) == EXPECT[j]
    picks = spec_ref.argmax_rows(lg.reshape(-1, c.vocab)).reshape(len(LENS), K + 1)
    acc, out = spec_ref.accept(picks, c.drafts)
    assert np.array_equal(_np(res.accepted), acc) and np.array_equal(_np(res.tokens), out)
    assert ctx.steps_left == c.steps_after
    # the default picks a route by row count (DESIGN: measured table): 12 rows run the rows route
    auto_ctx = _fresh(c.model, c.prompts)
    rows_logits, rows_acc = res.logits.clone(), res.accepted.clone()
    auto = c.model.verify(auto_ctx, c.drafts_dev)
    assert c.model.verify_route(len(LENS), K + 1) == "rows" and c.model.verify_route(1, 4) == "causal"
    assert torch.equal(auto.logits, rows_logits) and torch.equal(auto.accepted, rows_acc)


@pytest.mark.parametrize("attn", ["rows", "causal"])
def test_without_the_matrix_core_attention(case, dev, monkeypatch, attn):
    """ZL_ATTN_MFMA=0: encode()'s len_q = 1 route would scatter and attend in ONE launch, which orders only a row's own K/V; the
    rows of a task read each other's, so a row-expanded view must take scatter-then-attend.  Against the oracle's rows."""
    c = case
    ctx = _fresh(c.model, c.prompts)
    monkeypatch.setenv("ZL_ATTN_MFMA", "0")
    res = c.model.verify(ctx, c.drafts_dev, attn=attn)
    lg = _np(res.logits.float()).astype(np.float64).reshape(len(LENS), K + 1, c.vocab)
    for j in range(len(LENS)):
        ok, err = _close(lg[j], c.ref[j], 1e-3)
        assert ok, (j, err)
        if _margins_decide(c, j):
            assert int(res.accepted[j]) == EXPECT[j]
    picks = spec_ref.argmax_rows(lg.reshape(-1, c.vocab)).reshape(len(LENS), K + 1)
    acc, out = spec_ref.accept(picks, c.drafts)
    assert np.array_equal(_np(res.accepted), acc) and np.array_equal(_np(res.tokens), out)


@pytest.mark.parametrize("attn", ["rows", "causal"])
def test_tables_rewritten_in_place_and_out_of_range_drafts(case, dev, attn):
    """a task's buffers swapped by rewriting the context's pointer tables IN PLACE between two calls: the second call must use the
    new ones (the old ones are poisoned); and drafts outside the vocabulary (-1, vocab) are rejected, their rows harmless"""
    c = case
    ref_ctx = _fresh(c.model, c.prompts)
    bad = c.drafts.copy()
    bad[0, 1], bad[1, 0] = -1, c.vocab
    bad_dev = torch.from_numpy(bad).to(dev)
    e = c.model.verify(ref_ctx, bad_dev, attn=attn)
    e_logits, e_acc, e_tok = e.logits.clone(), e.accepted.clone(), e.tokens.clone()
    assert int(e_acc[0]) <= 1 and int(e_acc[1]) == 0 and torch.isfinite(e_logits.float()).all()
    ok, err = _close(_np(e_logits.float()).astype(np.float64)[0], c.ref[0][0], 1e-3)       # task 0's first row: as with good drafts
    assert ok, err
    ctx = _fresh(c.model, c.prompts)
    start = [getattr(ctx, n).clone() for n in STATE]
    c.model.verify(ctx, c.drafts_dev, attn=attn)                       # builds the view from the first tables
    for n, v in zip(STATE, start):
        getattr(ctx, n).copy_(v)
    fresh = _fresh(c.model, c.prompts)                                 # the same history in other buffers
    old = ctx.kv[0]
    ctx.kv[0] = fresh.kv[0]
    ctx.k_addrs[:, 0] = fresh.k_addrs[:, 0]
    ctx.v_addrs[:, 0] = fresh.v_addrs[:, 0]
    old.fill_(float("nan"))
    r = c.model.verify(ctx, bad_dev, attn=attn)
    assert torch.equal(r.logits, e_logits) and torch.equal(r.accepted, e_acc) and torch.equal(r.tokens, e_tok)


def test_four_rounds_with_a_repeating_drafter(case, dev):
    """the drafter proposes the previous round's picks again; every emitted token must be admissible under ONE oracle pass over
    prompt + [t0] + emitted per task, and the emitted count is sum(accepted + 1)"""
    c = case
    ctx = _fresh(c.model, c.prompts)
    drafts = c.drafts_dev.clone()
    emitted, total = [[] for _ in LENS], 0
    for _ in range(4):
        res = c.model.verify(ctx, drafts, attn="causal")
        acc, out = _np(res.accepted), _np(res.tokens)
        for j in range(len(LENS)):
            assert (out[j, :acc[j] + 1] >= 0).all() and (out[j, acc[j] + 1:] == -1).all()
            emitted[j] += [int(t) for t in out[j, :acc[j] + 1]]
        total += int((acc + 1).sum())
        drafts = res.tokens[:, :K].contiguous()                         # -1 padding included: such a draft is never accepted
    assert sum(len(e) for e in emitted) == total
    assert _np(ctx.positions).tolist() == [p + len(e) for p, e in zip(LENS, emitted)]
    om = AllRowsOracle(c.oracle, c.cfg, c.sd, 128, len(LENS), LEN_BUF)
    for j, p in enumerate(LENS):
        rows = om.prefill_all(j, list(c.prompts[j]) + [int(c.t0[j])] + emitted[j][:-1])
        ref = rows[p:p + len(emitted[j])]
        bar = _bar(ref)
        for i, t in enumerate(emitted[j]):
            assert ref[i, t] >= ref[i].max() - 2 * bar, (j, i)


def test_no_host_synchronisation(case, dev):
    c = case
    for attn in ("causal", "rows"):
        ctx = _fresh(c.model, c.prompts)
        c.model.verify(ctx, c.drafts_dev, attn=attn)                   # warm: tables built, code objects loaded
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            res = c.model.verify(ctx, c.drafts_dev, attn=attn)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert int(res.accepted.min()) >= 0


@pytest.mark.parametrize("attn", ["causal", "rows"])
def test_graph_capture_replays_on_new_drafts(case, dev, attn):
    c = case
    other = c.drafts.copy()
    other[0, 2] = (other[0, 2] + 1) % c.vocab                          # another draft set: task 0 now stops at 2
    other[1, 1] = c.drafts[1, 1] - 1 if c.drafts[1, 1] else c.vocab - 1   # (the greedy token again: task 1 goes on)
    eager_ctx = _fresh(c.model, c.prompts)
    e = c.model.verify(eager_ctx, torch.from_numpy(other).to(dev), attn=attn)
    e_logits, e_acc, e_tok, e_state = e.logits.clone(), e.accepted.clone(), e.tokens.clone(), _state(eager_ctx)
    ctx = _fresh(c.model, c.prompts)
    start = [getattr(ctx, n).clone() for n in STATE]
    kv0 = [t.clone() for t in ctx.kv]
    drafts = c.drafts_dev.clone()
    c.model.verify(ctx, drafts, attn=attn)                             # eager warm-up builds the expanded tables
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = c.model.verify(ctx, drafts, attn=attn)
    for n, v in zip(STATE, start):                                     # restore the context, hand over the new drafts
        getattr(ctx, n).copy_(v)
    for t, v in zip(ctx.kv, kv0):
        t.copy_(v)
    drafts.copy_(torch.from_numpy(other).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(r.logits, e_logits) and torch.equal(r.accepted, e_acc) and torch.equal(r.tokens, e_tok)
    for n, v in zip(STATE, e_state):
        assert np.array_equal(_np(getattr(ctx, n)), v), n


def test_refusals(case, dev):
    from zhilight_amd import ops
    c, model = case, case.model
    with pytest.raises(ops.ZLError):                                   # INT8 context
        q8 = model.new_context(3, LEN_BUF, 4, kv_cache_dtype="int8")
        model.verify(q8, c.drafts_dev)
    with pytest.raises(ops.ZLError):                                   # B * len_q = 33
        model.verify(model.new_context(11, LEN_BUF, 4), torch.zeros((11, 2), dtype=torch.int32, device=dev))
    ctx = model.new_context(3, LEN_BUF, 4)
    with pytest.raises(ops.ZLError):                                   # drafts dtype
        model.verify(ctx, c.drafts_dev.to(torch.int64))
    with pytest.raises(ops.ZLError):                                   # drafts shape
        model.verify(ctx, c.drafts_dev[:2].contiguous())
    with pytest.raises(ops.ZLError):                                   # drafts device
        model.verify(ctx, c.drafts_dev.cpu())
    with pytest.raises(ops.ZLError):
        model.verify(ctx, c.drafts_dev, attn="tree")
    short = model.new_context(3, LEN_BUF, LEN_BUF - K)                  # three slots left, four rows wanted
    with pytest.raises(ops.ZLError):
        model.verify(short, c.drafts_dev)
    assert short.steps_left == K
