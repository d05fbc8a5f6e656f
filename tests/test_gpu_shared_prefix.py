"""Shared prefixes in the model, on the small GPTQ model of test_gpu_slots.py (2 layers, H, Hkv = 8, 2), len_buf 128, prefix buffers of 64
rows: admit_samples(share=) against its copying twin, a running slot beside a sharing group, one captured graph across a shared
admission and a park, requests behind a loaded system prompt (admit(prefixes=)) against a plain admit of the concatenated prompts,
BatchServer, and the refusals.

A sharing slot and its twin run different attention kernels (zl_decode_attn_shared; the in-launch merge), so their logits are compared
at the tolerance the model tests hold either to against the oracle (_close(.., 1e-3)); both are fed the TWIN's sampled tokens, so the
streams cannot drift apart.  What does not pass through the attention -- the rows of context, sampler and stop state after admission --
is bit-equal."""
import numpy as np
import pytest
import torch

import stop_ref as sr
import test_gpu_fork as tfork
import test_gpu_slots as tslots
from test_gpu_model import OracleModel
from test_gpu_prefill_batch import _close

pytestmark = pytest.mark.gpu

LEN_BUF, BIAS_LD, TOP = tslots.LEN_BUF, tslots.BIAS_LD, tslots.TOP
ROWS = 64
case = tslots.case
_req, _snap, _rows_equal, _bits, _fresh, _step = tslots._req, tslots._snap, tslots._rows_equal, tslots._bits, tfork._fresh, tfork._step
I32 = torch.int32


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _sharing(c, b, count=2):
    st = _fresh(c, b, False)
    c.model.new_shared_prefixes(st[0], count, ROWS)
    return st


def _poison_own(ctx, slots):
    for s in slots:
        ctx.kv[s].fill_(float("nan"))


def _forced_steps(c, A, Bt, steps, slots, om=None, pending=None, pos=None, oracle_steps=0):
    """`steps` steps: the twin Bt samples, A is fed the twin's tokens; A's logits within 1e-3 of the twin's at every step and, for the
    first oracle_steps, of the oracle's over the whole prompt"""
    model = c.model
    tok = np.array(pending, np.int32) if pending is not None else None
    for i in range(steps):
        la = _f64(model.encode(A[0]))
        lb, nxt = model.step_sample(Bt[0], Bt[1], stop=Bt[2])
        lb = _f64(lb)
        for s in slots:
            ok, err = _close(la[s], lb[s], 1e-3)
            assert ok, ("twin", i, s, err)
        if om is not None and i < oracle_steps:
            ex, _ = om.step(tok, [p + i for p in pos], flavour="E", commit=False)
            om.step(tok, [p + i for p in pos], flavour="R")
            for j, s in enumerate(slots):
                ok, err = _close(la[s], ex[j], 1e-3)
                assert ok, ("oracle", i, s, err)
            tok = nxt.cpu().numpy().astype(np.int32)[slots]
        model.advance(A[0], nxt)


def _own_rows_close(A, Bt, slots, lo, hi):
    for s in slots:
        a, b = _f64(A[0].kv[s][:, :, lo:hi]), _f64(Bt[0].kv[s][:, :, lo:hi])
        assert np.isfinite(a).all() and np.abs(a - b).max() <= 2.0 ** -9 * np.abs(b).max(), s


def test_shared_samples_against_the_copying_twin(case, oracle):
    c, model = case, case.model
    prompt = np.concatenate([c.prompts[1], np.array([7], np.int32)])         # 41 tokens: 40 shared rows
    p, P, slots = torch.from_numpy(prompt), 40, [2, 0, 1]
    reqs = [_req(c, 3, seed=4100 + j, max_new_tokens=40) for j in range(3)]
    A, Bt = _sharing(c, 3), _fresh(c, 3, False)
    _poison_own(A[0], slots)
    out_a = model.admit_samples(A[0], [(slots, p, reqs)], A[1], A[2], share=[1])
    out_b = model.admit_samples(Bt[0], [(slots, p, reqs)], Bt[1], Bt[2])
    assert out_a.shape == out_b.shape == (1, c.vocab) and _close(_f64(out_a), _f64(out_b), 1e-3)[0]
    _rows_equal(_snap(*A), _snap(*Bt), slots, "after admission")
    sh = A[0].shared
    assert sh.prefix_of.tolist() == [1, 1, 1] and sh.prefix_lens.tolist() == [0, P] and sh.of_host == [1, 1, 1] and sh.lens_host == [0, P]
    assert A[0].tokens.tolist() == [7] * 3 and A[0].positions.tolist() == [P] * 3 and A[0].valid_lens.tolist() == [P + 1] * 3
    for s in slots:                                                         # nothing was copied: the own buffers are as they were
        assert torch.isnan(A[0].kv[s]).all()
    pre, src = _f64(sh.kv[1][:, :, :P]), _f64(Bt[0].kv[2][:, :, :P])
    assert np.abs(pre - src).max() <= 2.0 ** -9 * np.abs(src).max()
    om = OracleModel(oracle, c.cfg, c.sd, 128, 3, LEN_BUF)
    for j in range(3):
        om.prefill(j, prompt[:-1])
    _forced_steps(c, A, Bt, 12, slots, om, [7] * 3, [P] * 3, oracle_steps=3)
    assert len({tuple(r) for r in Bt[2].tail.tolist()}) > 1                  # the samples went apart
    _own_rows_close(A, Bt, slots, P, P + 12)
    for s in slots:
        assert torch.isnan(A[0].kv[s][:, :, :P]).all()                      # and the steps wrote nothing below P


def test_a_running_slot_keeps_its_stream_beside_a_sharing_group(case):
    c, model = case, case.model
    runs = []
    for shared in (True, False):
        st = _sharing(c, 4)
        model.admit_samples(st[0], [([0], torch.from_numpy(c.prompts[2]), [_req(c, 2, max_new_tokens=20)])], st[1], st[2])
        rec = [_step(model, *st) for _ in range(3)]
        if shared:
            before = _snap(*st)
            model.admit_samples(st[0], [([3, 1, 2], torch.from_numpy(c.prompts[3]), [_req(c, 3, seed=j, max_new_tokens=9) for j in range(3)])],
                                st[1], st[2], share=[0])
            after = _snap(*st)
            _rows_equal(after, before, [0], "the running slot")
            assert torch.equal(after["kv.0"], before["kv.0"])
        rec += [_step(model, *st) for _ in range(5)]
        runs.append([(t[0].clone(), l[0].clone(), p[0].clone()) for t, l, p in rec])
    assert len(runs[0]) == 8
    for i, ((t, l, p), (tt, ll, pp)) in enumerate(zip(*runs)):
        assert torch.equal(t, tt) and torch.equal(l, ll) and torch.equal(p.view(I32), pp.view(I32)), i


def _scripted(c, captured):
    """a plain admission, steps, a sharing group of two short requests, steps, the group parked, steps; captured: every step behind the
    first replays ONE graph"""
    model = c.model
    ctx, samp, stop, _ = _sharing(c, 3)
    model.admit_samples(ctx, [([1], torch.from_numpy(c.prompts[2]), [_req(c, 2, max_new_tokens=30)])], samp, stop)
    rec, graph, out = [], None, None

    def steps(n):
        nonlocal graph, out
        for _ in range(n):
            if graph is not None:
                graph.replay()
            else:
                out = model.step_sample(ctx, samp, stop=stop)
                if captured:
                    torch.cuda.synchronize()
                    rec.append([out[1].clone(), samp.logprobs.clone(), stop.finished.clone(), ctx.positions.clone()])
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        out = model.step_sample(ctx, samp, stop=stop)
                    continue
            rec.append([out[1].clone(), samp.logprobs.clone(), stop.finished.clone(), ctx.positions.clone()])

    steps(3)
    model.admit_samples(ctx, [([2, 0], torch.from_numpy(c.prompts[3]), [_req(c, 3, seed=j, max_new_tokens=2) for j in range(2)])], samp, stop,
                        share=[1])
    steps(3)
    assert stop.finished.tolist() == [3, 0, 3] and ctx.shared.of_host == [1, -1, 1]
    model.park(ctx, [0, 2], samp, stop, finished=stop.finished.tolist())
    assert ctx.shared.of_host == [-1] * 3 and ctx.shared.prefix_of.tolist() == [-1] * 3
    steps(3)
    assert stop.gen_lens.tolist()[1] == 9
    return rec


def test_one_captured_graph_survives_a_shared_admission_and_a_park(case):
    eager, replayed = _scripted(case, False), _scripted(case, True)
    assert len(eager) == len(replayed) == 9
    for s, (a, b) in enumerate(zip(eager, replayed)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(_bits(x), _bits(y)), (s, i)


def test_requests_behind_a_loaded_system_prompt(case):
    c, model = case, case.model
    system = c.rng.integers(0, c.vocab, 50).astype(np.int32)
    own = [c.prompts[0], c.prompts[2], c.rng.integers(0, c.vocab, 30).astype(np.int32)]                      # 5, 17, 30 tokens
    slots, P = [1, 2, 0], 50
    reqs = [_req(c, i, max_new_tokens=20) for i in range(3)]
    A, Bt = _sharing(c, 3), _fresh(c, 3, False)
    _poison_own(A[0], slots)
    model.load_prefix(A[0], 1, torch.from_numpy(system))
    assert A[0].shared.prefix_lens.tolist() == [0, P]
    la = model.admit(A[0], slots, [torch.from_numpy(p) for p in own], reqs, A[1], A[2], prefixes=[1, 1, 1])
    lb = model.admit(Bt[0], slots, [torch.from_numpy(np.concatenate([system, p])) for p in own], reqs, Bt[1], Bt[2])
    for j in range(3):
        ok, err = _close(_f64(la)[j], _f64(lb)[j], 1e-3)
        assert ok, (j, err)
    assert A[0].positions.tolist() == Bt[0].positions.tolist() == [P + 30, P + 5, P + 17]
    assert A[0].valid_lens.tolist() == Bt[0].valid_lens.tolist() and A[0].shared.of_host == [1, 1, 1]
    a, b = _snap(*A), _snap(*Bt)
    a["ctx.tokens"], b["ctx.tokens"] = a["ctx.tokens"] * 0, b["ctx.tokens"] * 0      # the greedy picks may differ where two logits are close
    _rows_equal(a, b, slots, "after admission")
    assert (A[0].steps_left, A[0].slot_guard) == (Bt[0].steps_left, Bt[0].slot_guard)
    for s, p in zip(slots, own):
        _own_rows_close(A, Bt, [s], P, P + len(p))
        assert torch.isnan(A[0].kv[s][:, :, :P]).all()
    A[0].tokens.copy_(Bt[0].tokens)                                          # both continue from the twin's first tokens
    _forced_steps(c, A, Bt, 8, slots)
    # a slot admitted without a prefix lets go of the one it read
    model.admit(A[0], [2], [torch.from_numpy(c.prompts[4])], [_req(c, 4)], A[1], A[2], prefixes=[None])
    assert A[0].shared.of_host == [1, 1, -1] and A[0].shared.prefix_of.tolist() == [1, 1, -1]


def _drive(c, ctx, samp, stop):
    """step until every slot has finished -> per slot (ids, log-probabilities, reason)"""
    b = ctx.tokens.numel()
    ids, lps = [[] for _ in range(b)], [[] for _ in range(b)]
    for _ in range(LEN_BUF):
        if stop.live.item() == 0:
            break
        tok, _, lp = _step(c.model, ctx, samp, stop, None)
        for s, (row, lrow) in enumerate(zip(tok.tolist(), lp.tolist())):
            m = len(sr.emitted(row))
            ids[s] += row[:m]
            lps[s] += lrow[:m]
    return ids, lps, stop.finished.tolist()


def test_batch_server_shares_samples_and_serves_a_system_prompt(case):
    from zhilight_amd import ops
    from zhilight_amd.serving import BatchServer
    c, model = case, case.model
    system = torch.from_numpy(c.rng.integers(0, c.vocab, 50).astype(np.int32))
    p_n, p_own = torch.from_numpy(c.prompts[3]), torch.from_numpy(c.prompts[0])
    r_n, r_own = _req(c, 1, max_new_tokens=6), _req(c, 0, max_new_tokens=3)
    srv = BatchServer(model, 4, LEN_BUF, bias_ld=BIAS_LD, top_logprobs=TOP, poll=4, shared_prefixes=2, shared_rows=ROWS, share_min_rows=8)
    with pytest.raises(ops.ZLError, match="handle"):
        srv.submit(p_own, prefix=0)                                          # nothing loaded yet
    h = srv.load_prefix(system)
    assert h == 0
    assert [srv.submit(p_n, n=3, **r_n), srv.submit(p_own, prefix=h, **r_own)] == [0, 1]
    with pytest.raises(ops.ZLError):
        srv.drop_prefix(h)                                                   # a queued request names it
    with pytest.raises(ops.ZLError, match="does not fit"):
        srv.submit(torch.zeros(LEN_BUF - 50, dtype=I32), prefix=h)           # P + prompt + 1 > len_buf
    with pytest.raises(ops.ZLError, match="one token at least"):
        srv.submit(torch.zeros(0, dtype=I32), prefix=h)                      # nothing behind the prefix
    res = srv.run()
    assert srv.log == [(1, [(0, 0), (1, 0), (2, 0), (3, 1)])]
    assert srv.stats["shared_groups"] == 1 and srv.stats["forks"] == 0
    # run() parks what it leaves finished: no slot reads a buffer any more, the group's buffer is free and the pinned one can go
    assert srv.pool.users(h) == [] and srv.pool.free() == [1] and srv.ctx.shared.of_host == [-1] * 4
    # the hand-driven twin: the same primitives in the same order on a fresh batch
    ctx, samp, stop, _ = _sharing(c, 4)
    model.load_prefix(ctx, 0, system)
    model.admit(ctx, [3], [p_own], [r_own], samp, stop, prefixes=[0])
    model.admit_samples(ctx, [([0, 1, 2], p_n, [dict(r_n, seed=r_n["seed"] + j) for j in range(3)])], samp, stop, share=[1])
    first = ctx.tokens.tolist()
    ids, lps, fin = _drive(c, ctx, samp, stop)
    lp_bits = lambda x: np.asarray(x, np.float32).view(np.int32)                                             # noqa: E731
    for j, sm in enumerate(res[0]["samples"]):
        assert (sm["first_token"], sm["tokens"], sm["reason"], sm["seed"]) == (None, ids[j], fin[j], r_n["seed"] + j) and len(ids[j]) == 6
        assert np.array_equal(lp_bits(sm["logprobs"]), lp_bits(lps[j]))
    assert (res[1]["first_token"], res[1]["tokens"], res[1]["reason"]) == (first[3], ids[3], fin[3]) and len(ids[3]) == 3
    assert np.array_equal(lp_bits(res[1]["logprobs"]), lp_bits(lps[3])) and res[1]["clamped"] == 3
    srv.drop_prefix(h)
    assert srv.pool.free() == [0, 1]
    with pytest.raises(ops.ZLError, match="handle"):
        srv.submit(p_own, prefix=h)


def test_batch_server_falls_back_to_copies(case):
    """no free buffer (one group holds the only one, then a pinned prompt does) and a prompt longer than a buffer: the copying route"""
    from zhilight_amd.serving import BatchServer
    c, model = case, case.model
    p = torch.from_numpy(c.prompts[3])
    # three groups of two in one round, one buffer: the first shares, the others copy; the buffer stays the group's until its last
    # slot is parked or re-admitted
    srv = BatchServer(model, 6, LEN_BUF, bias_ld=BIAS_LD, top_logprobs=TOP, poll=4, shared_prefixes=1, shared_rows=ROWS, share_min_rows=8)
    for i, limit in enumerate((3, 14, 14)):
        srv.submit(p, n=2, **_req(c, i, max_new_tokens=limit))
    res = srv.run()
    assert srv.stats["shared_groups"] == 1 and srv.stats["forks"] == 2 and srv.stats["parks"] >= 1
    assert [len(sm["tokens"]) for r in range(3) for sm in res[r]["samples"]] == [3, 3, 14, 14, 14, 14]
    assert srv.pool.free() == [0] and srv.ctx.shared.of_host[:2] == [-1, -1]    # slots 0, 1 were parked while the others ran
    # pinned: none free
    srv = BatchServer(model, 2, LEN_BUF, bias_ld=BIAS_LD, top_logprobs=TOP, poll=4, shared_prefixes=1, shared_rows=ROWS, share_min_rows=8)
    srv.load_prefix(p)
    srv.submit(p, n=2, **_req(c, 0, max_new_tokens=3))
    srv.run()
    assert srv.stats["shared_groups"] == 0 and srv.stats["forks"] == 1
    # P > L, and below the threshold
    for rows, low in ((16, 8), (ROWS, 23)):
        srv = BatchServer(model, 2, LEN_BUF, bias_ld=BIAS_LD, top_logprobs=TOP, poll=4, shared_prefixes=1, shared_rows=rows, share_min_rows=low)
        srv.submit(p, n=2, **_req(c, 0, max_new_tokens=3))                   # 22 shared rows
        srv.run()
        assert srv.stats["shared_groups"] == 0 and srv.stats["forks"] == 1


def test_a_groups_buffer_is_not_reused_before_its_last_slot_is_parked(case):
    """round 1: two plain requests (slots 0, 1) and a sharing pair (slots 2, 3), all short, and a long copying pair (4, 5: no buffer
    left).  When the short ones have finished, the queued pair goes into slots 0 and 1 while slots 2 and 3 are finished but not parked
    yet: they still read the only buffer, so the pair copies.  The park that follows frees the buffer, and the pair queued behind it
    shares again."""
    from zhilight_amd.serving import BatchServer
    c = case
    p, q = torch.from_numpy(c.prompts[3]), torch.from_numpy(c.prompts[0])
    srv = BatchServer(c.model, 6, LEN_BUF, bias_ld=BIAS_LD, top_logprobs=TOP, poll=4, shared_prefixes=1, shared_rows=ROWS, share_min_rows=8)
    srv.submit(q, **_req(c, 0, max_new_tokens=3))
    srv.submit(q, **_req(c, 1, max_new_tokens=3))
    srv.submit(p, n=2, **_req(c, 2, max_new_tokens=3))                       # shares
    srv.submit(p, n=2, **_req(c, 3, max_new_tokens=40))                      # none free: copies
    srv.submit(p, n=2, **_req(c, 4, max_new_tokens=7))                       # round 2, slots 0, 1: slots 2, 3 still read the buffer
    rounds = {}                                                             # round -> the pool right after its admission
    admit = srv._admit

    def spy():
        admit()
        rounds.setdefault(srv.round, [srv.stats["shared_groups"], srv.stats["forks"], srv.pool.free(), srv.pool.users(0)])
    srv._admit = spy
    srv.run()
    assert srv.log[:2] == [(1, [(0, 0), (1, 1), (2, 2), (3, 2), (4, 3), (5, 3)]), (2, [(0, 4), (1, 4)])]
    assert rounds[1] == [1, 1, [], [2, 3]]
    assert rounds[2] == [1, 2, [], [2, 3]]                                   # the pair copied; the finished slots were still readers
    assert srv.pool.free() == [0] and srv.stats["parks"] >= 1
    srv.submit(p, n=2, **_req(c, 5, max_new_tokens=3))                       # the buffer is free now: this pair shares
    srv.run()
    assert srv.stats["shared_groups"] == 2 and srv.stats["forks"] == 2


def test_nine_sharing_slots_take_the_statistics_route(case, dev):
    """9 slots at Llama-3-8B's layer geometry (2 layers, synthetic weights: the model of test_gpu_decode_routes' "wide" cases), where the
    decode step hands the rows' statistics from projection to projection (norm = "row_ss") around the shared attention; against the
    copying twin's steps as in the three-slot test"""
    import types
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    cfg.num_layers, cfg.vocab_size = 2, 512
    model = LLaMA(cfg, QuantConfig(5, 128), dev).init_synthetic(seed=5)
    c = types.SimpleNamespace(model=model, vocab=512, prompts=case.prompts)
    prompt = c.prompts[3]                                                    # 23 tokens: 22 shared rows
    p, P, slots = torch.from_numpy(prompt), 22, list(range(9))
    reqs = [_req(c, 3, seed=4200 + j, max_new_tokens=40) for j in range(9)]
    A, Bt = _sharing(c, 9), _fresh(c, 9, False)
    _poison_own(A[0], slots)
    out_a = model.admit_samples(A[0], [(slots, p, reqs)], A[1], A[2], share=[0])
    out_b = model.admit_samples(Bt[0], [(slots, p, reqs)], Bt[1], Bt[2])
    route, twin = model._decode_route(A[0], 9, False, False, None), model._decode_route(Bt[0], 9, False, False, None)
    assert (route.attn, route.norm, route.out) == ("shared", "row_ss", "linear") and route.stats is not None
    assert (twin.attn, twin.norm) == ("la", "row_ss")
    assert _close(_f64(out_a), _f64(out_b), 1e-3)[0]
    _rows_equal(_snap(*A), _snap(*Bt), slots, "after admission")
    _forced_steps(c, A, Bt, 8, slots)
    _own_rows_close(A, Bt, slots, P, P + 8)
    for s in slots:
        assert torch.isnan(A[0].kv[s][:, :, :P]).all()


def test_refusals_come_before_any_launch(case):
    from zhilight_amd import ops
    from zhilight_amd.serving import BatchServer
    c, model = case, case.model
    with pytest.raises(ops.ZLError, match="INT8"):
        model.new_shared_prefixes(model.new_context(2, LEN_BUF, 0, kv_cache_dtype="int8"), 1, ROWS)
    tp, model.tp = model.tp, object()
    try:
        with pytest.raises(ops.ZLError, match="tensor parallelism"):
            model.new_shared_prefixes(model.new_context(2, LEN_BUF, 0), 1, ROWS)
    finally:
        model.tp = tp
    with pytest.raises(ops.ZLError, match="drafter"):
        BatchServer(model, 2, LEN_BUF, lookup_k=2, shared_prefixes=1, shared_rows=ROWS)
    ctx, samp, stop, _ = _sharing(c, 3)
    with pytest.raises(ops.ZLError, match="one table per context"):
        model.new_shared_prefixes(ctx, 1, ROWS)
    model.load_prefix(ctx, 0, torch.from_numpy(c.prompts[1]))                # 40 rows
    model.admit(ctx, [0], [torch.from_numpy(c.prompts[0])], [_req(c, 0)], samp, stop, prefixes=[0])
    cache = model.new_prefix_cache(model.new_context(1, LEN_BUF, 0), 4, block_size=16)
    look = model.new_lookup(ctx, [[] for _ in range(3)], 2)
    before = _snap(ctx, samp, stop, None)
    pre = [t.clone() for t in ctx.shared.kv] + [ctx.shared.prefix_of.clone(), ctx.shared.prefix_lens.clone()]
    host = (ctx.steps_left, dict(ctx.slot_guard), dict(ctx.slot_room), list(ctx.shared.of_host), list(ctx.shared.lens_host))
    p = torch.from_numpy(c.prompts[3])
    drafts = torch.zeros((3, 2), dtype=I32, device=ctx.tokens.device)
    cases = [
        ("shared prefixes", lambda: model.verify(ctx, drafts)),
        ("shared prefixes", lambda: model.step_lookup(ctx, look, sampler=samp, stop=stop)),
        ("not with cache=", lambda: model.admit_samples(ctx, [([1, 2], p, [{}, {}])], samp, stop, cache=cache, share=[1])),
        ("not with cache=", lambda: model.admit(ctx, [1], [p], [{}], samp, stop, cache=cache, prefixes=[0])),
        ("loaded prefixes", lambda: model.admit(ctx, [1], [p], [{}], samp, stop, prefixes=[1])),                  # nothing loaded into 1
        ("loaded prefixes", lambda: model.admit(ctx, [1], [p], [{}], samp, stop, prefixes=[2])),
        ("does not fit", lambda: model.admit(ctx, [1], [torch.zeros(LEN_BUF - 40, dtype=I32)], [{}], samp, stop, prefixes=[0])),
        ("does not fit a prefix buffer", lambda: model.admit_samples(ctx, [([1, 2], torch.zeros(ROWS + 2, dtype=I32), [{}, {}])], samp, stop, share=[1])),
        ("the buffer holds", lambda: model.load_prefix(ctx, 1, torch.zeros(ROWS + 1, dtype=I32))),
        ("is read by slots", lambda: model.load_prefix(ctx, 0, p)),
        ("outside this call", lambda: model.admit_samples(ctx, [([1, 2], p, [{}, {}])], samp, stop, share=[0])),
        ("one prefix per group", lambda: model.admit_samples(ctx, [([1, 2], p, [{}, {}])], samp, stop, share=[0, 1])),
        ("distinct prefix indices", lambda: model.admit_samples(ctx, [([1], p, [{}]), ([2], p, [{}])], samp, stop, share=[1, 1])),
        ("no shared prefixes", lambda: model.load_prefix(model.new_context(1, LEN_BUF, 0), 0, p)),
        # slot 0 reads prefix 0 (45 rows behind it): a continued piece would attend over own rows below the prefix's length
        ("reads a shared prefix", lambda: model.prefill_batch(ctx, [0], [p], pos0=[45])),
    ]
    for match, call in cases:
        with pytest.raises(ops.ZLError, match=match):
            call()
    after = _snap(ctx, samp, stop, None)
    for k in before:                                                        # nothing ran: every tensor as before
        assert torch.equal(_bits(before[k]), _bits(after[k])), k
    for x, y in zip(pre, [t for t in ctx.shared.kv] + [ctx.shared.prefix_of, ctx.shared.prefix_lens]):
        assert torch.equal(x, y)
    assert host == (ctx.steps_left, ctx.slot_guard, ctx.slot_room, ctx.shared.of_host, ctx.shared.lens_host)
    model.admit_samples(ctx, [([1, 2], p, [_req(c, 3), _req(c, 4)])], samp, stop, share=[1])       # and the accepted call
