"""The stop conditions of a decode step on the GPU: zl_stop_advance against tests/stop_ref.py with exact equality of every array after
every one of 20 chained steps (all optional arrays, none of them, and the one-token form whose row IS ctx.tokens), the partition
invariance on the device, and the stop= keyword of LLaMA.step_sample / step_greedy / verify / step_lookup and of the generate loops on
the small GPTQ model of test_gpu_spec_verify.py: the stopped runs emit a twin's streams cut where stop_ref cuts them, a finished task's
context stands still, ids accepted behind a stop are undone and never reach the drafter's history, and a captured step carries the stop
state forward.  Every buffer of the kernel tests has a poisoned guard region behind it."""
import numpy as np
import pytest
import torch

import stop_ref as sr
import test_gpu_sample as gs
import test_gpu_spec_verify as sv
import test_stop_host as host
from test_gpu_prefill_batch import _gptq_model

pytestmark = pytest.mark.gpu

_np, _guarded = gs._np, gs._guarded
I32, I64 = torch.int32, torch.int64
STEPS, ALPHABET = 20, host.ALPHABET
CTX_NAMES = sv.STATE                                                    # tokens, positions, placement, valid_lens
STOP_NAMES = ("gen_lens", "tail", "last_token", "finished", "emit_lens", "live")


# ---- the kernel against the reference ---------------------------------------------------------------------------------------------------
def _plan(b, n_new, variant, seed, kinds):
    """The whole chained run on the host.  kinds[t]: 0 .. 3 = a task built from its own id stream to end by a stop id, by a stop
    sequence, by the length limit, or never; anything else = one of test_stop_host's random mixtures.  A row holds a random number of
    ids (none at all in one of ten), -1 behind them and now and then a stray id behind the first -1.
    -> (parameter arrays, the initial state, [per step: dict(before=..., after=...)], the reasons seen, a frozen task was stepped twice)"""
    rng = np.random.default_rng(seed)
    rows = np.full((STEPS, b, n_new), -1, np.int32)
    for s in range(STEPS):
        for t in range(b):
            m = 0 if rng.random() < 0.1 else int(rng.integers(1, n_new + 1))
            rows[s, t, :m] = rng.integers(0, ALPHABET, m)
            if m + 1 < n_new and rng.random() < 0.2:
                rows[s, t, int(rng.integers(m + 1, n_new))] = rng.integers(0, ALPHABET)
    stops, max_new = [], np.zeros(b, np.int32)
    for t in range(b):
        st = [i for s in range(STEPS) for i in sr.emitted(rows[s, t].tolist())]
        assert len(st) >= 6
        one, lim = host.random_stops(rng, 1)
        if kinds[t] > 3:
            stops.append(one[0])
            max_new[t] = lim[0]
        else:
            stops.append((([st[3]], []), ([], [st[4:6]]), ([], []), ([], []))[kinds[t]])
            max_new[t] = 3 if kinds[t] == 2 else 0
    params = sr.pack(stops) + (max_new,)
    state = sr.new_state(b, rng.integers(0, ALPHABET, b))
    state0 = {n: v.copy() for n, v in state.items()}
    ctx = {n: (rng.integers(0, ALPHABET, b) if n == "tokens" else 100 * (i + 1) + np.arange(b)).astype(np.int32) for i, n in enumerate(CTX_NAMES)}
    acc, nxt = np.zeros(b, np.int32), np.zeros(b, np.int64)
    steps, frozen_steps, reasons = [], np.zeros(b, np.int64), set()
    for s in range(STEPS):
        row = rows[s].copy()
        for t in range(b):                                              # what the step's advance / accept launch leaves
            e = sr.emitted(row[t].tolist())
            acc[t], nxt[t] = len(e) - 1, (e[-1] if e else -1)
            for n in CTX_NAMES[1:]:
                ctx[n][t] += len(e)
            if variant == "alias":
                ctx["tokens"][t] = row[t, 0]
            elif e:
                ctx["tokens"][t] = e[-1]
            frozen_steps[t] += bool(e) and state["finished"][t] != 0
        before = dict(new_tokens=row.copy(), accepted=acc.copy(), next_tokens=nxt.copy(), **{n: v.copy() for n, v in ctx.items()})
        if variant == "alias":
            row = ctx["tokens"].reshape(b, 1)
        opt = {} if variant == "null" else ctx
        emit, live = sr.stop_advance(*params, state, row, acc, None if variant == "null" else nxt, **opt)
        after = dict(new_tokens=row.copy(), accepted=acc.copy(), next_tokens=nxt.copy(), emit_lens=emit, live=np.array([live], np.int32),
                     **{n: v.copy() for n, v in ctx.items()}, **{n: v.copy() for n, v in state.items()})
        steps.append(dict(before=before, after=after))
    reasons.update(int(r) for r in state["finished"])
    return params, state0, steps, reasons, bool((frozen_steps >= 2).any())


def _episodes(b):
    """(seed offset, kinds) per run of a parametrisation: B = 1 takes five runs to see every kind of task"""
    return [(ep, [ep]) for ep in range(5)] if b == 1 else [(0, list(range(b)))]


VARIANTS = [(n_new, v) for n_new in (1, 2, 8, 32) for v in ("ctx", "null")] + [(1, "alias")]


def _seed(b, n_new, variant, ep):
    return 1000 * b + 10 * n_new + ep + (500 if variant == "alias" else 0)


@pytest.mark.parametrize("n_new,variant", VARIANTS, ids=[f"{n}-{v}" for n, v in VARIANTS])
@pytest.mark.parametrize("b", [1, 5, 33])
def test_kernel_equals_the_reference_after_every_step(dev, b, n_new, variant):
    """ctx: all four context arrays, accepted and next_tokens; null: none of the four and no next_tokens; alias: the row IS tokens.
    The device carries the state from step to step; each step's inputs are uploaded, every array is compared after it"""
    from zhilight_amd import ops
    seen, frozen_twice = set(), False
    for ep, kinds in _episodes(b):
        (ids, seqs, lens, max_new), state0, steps, reasons, twice = _plan(b, n_new, variant, _seed(b, n_new, variant, ep), kinds)
        seen |= reasons
        frozen_twice |= twice
        params = dict(stop_ids=ids, stop_seqs=seqs, seq_lens=lens, max_new=max_new)
        bufs = {n: _guarded(v.size, I32, dev, v.reshape(-1)) for n, v in dict(**params, **state0).items()}
        for n in ("new_tokens", "accepted", "emit_lens", "live") + CTX_NAMES:
            bufs[n] = _guarded(steps[0]["after"][n].size, I32, dev)
        bufs["next_tokens"] = _guarded(b, I64, dev)
        dv = {n: t for n, (t, _) in bufs.items()}
        for s, step in enumerate(steps):
            for n, v in step["before"].items():
                dv[n].copy_(torch.from_numpy(np.ascontiguousarray(v).reshape(-1)))
            new = dv["tokens"].view(b, 1) if variant == "alias" else dv["new_tokens"].view(b, n_new)
            opt = {} if variant == "null" else dict(next_tokens=dv["next_tokens"], **{n: dv[n] for n in CTX_NAMES})
            emit, live = ops.stop_advance(dv["stop_ids"].view(ids.shape), dv["stop_seqs"].view(seqs.shape), dv["seq_lens"].view(lens.shape),
                                          dv["max_new"], dv["gen_lens"], dv["tail"].view(b, sr.TAIL), dv["last_token"], dv["finished"], new,
                                          accepted=dv["accepted"], emit_lens=dv["emit_lens"], live=dv["live"], **opt)
            assert emit.data_ptr() == dv["emit_lens"].data_ptr() and live.data_ptr() == dv["live"].data_ptr()
            for n, want in step["after"].items():
                if not (variant == "alias" and n == "new_tokens"):
                    assert np.array_equal(_np(dv[n]).reshape(want.shape), want), (ep, s, n)
            gs._intact([g for _, g in bufs.values()])
        for n, v in params.items():                                     # the parameters are read only
            assert np.array_equal(_np(dv[n]).reshape(v.shape), v), n
    assert {0, 1, 2, 3} <= seen and frozen_twice, (seen, frozen_twice)


def test_partition_invariance_on_the_device(dev):
    """the same 64-id streams of 16 tasks fed one id per call and eight per call end in equal state and equal concatenated output"""
    from zhilight_amd import ops
    rng = np.random.default_rng(8)
    b, n = 16, 64
    stops, max_new = host.random_stops(rng, b, max_hi=80)
    stops[0], max_new[0] = ([], []), 0                                  # one task runs to the end
    stops[1], max_new[1] = ([], []), 20                                 # and one to its length limit
    streams = rng.integers(0, ALPHABET, (b, n)).astype(np.int32)
    params = [torch.from_numpy(a).to(dev) for a in sr.pack(stops) + (max_new,)]
    ends = []
    for width in (1, 8):
        st = {k: torch.from_numpy(v).to(dev) for k, v in sr.new_state(b, streams[:, 0]).items()}
        out = [[] for _ in range(b)]
        for at in range(1, n - 7, width):
            row = torch.from_numpy(np.ascontiguousarray(streams[:, at:at + width])).to(dev)
            emit, _ = ops.stop_advance(*params, st["gen_lens"], st["tail"], st["last_token"], st["finished"], row)
            for t, (r, e) in enumerate(zip(row.tolist(), emit.tolist())):
                out[t] += r[:e]
                assert r[e:] == [-1] * (width - e)
        ends.append((out, {k: _np(v).copy() for k, v in st.items()}))
    (out1, st1), (out8, st8) = ends
    assert out1 == out8
    for k in st1:
        assert np.array_equal(st1[k], st8[k]), k
    assert st1["gen_lens"].tolist() == [len(o) for o in out1] and st1["finished"][0] == 0 and st1["gen_lens"][0] == 56
    assert {1, 2, 3} <= set(st1["finished"].tolist())
    for t in range(b):
        assert out1[t] == streams[t, 1:1 + len(out1[t])].tolist()


# ---- the model ----------------------------------------------------------------------------------------------------------------------
LEN_BUF, K = sv.LEN_BUF, sv.K
LENS5 = sv.LENS + [23, 9]
KW = dict(temperature=0.8, top_k=20, top_p=0.95, seed=77)


class _Case:
    pass


@pytest.fixture(scope="module")
def case(dev):
    c = _Case()
    rng, c.cfg, c.sd, c.model = _gptq_model(dev)
    c.vocab = c.cfg.vocab_size
    c.prompts = [rng.integers(0, c.vocab, s).astype(np.int32) for s in LENS5]
    return c


def _ctx_state(ctx):
    return np.stack(sv._state(ctx), axis=1)                             # (B, 4): a task's tokens, positions, placement, valid_lens


def _cut(stream, ids=(), seqs=(), max_new=0, pending=None):
    """stop_ref on one task's stream, one id at a time -> (ids kept, reason)"""
    out, st, _ = host.run_stream([(list(ids), [list(s) for s in seqs])], np.array([max_new], np.int32), np.asarray(stream, np.int32),
                                 [1] * len(stream), pending, n_new=1)
    return len(out), int(st["finished"][0])


def _stops_from(streams, b):
    """task 0: the id of step 3; task 1: the two ids of steps 4 - 5; task 2: two ids at most; further tasks: nothing"""
    ids = [[int(streams[0][3])]] + [None] * (b - 1)
    seqs = [None, [[int(v) for v in streams[1][4:6]]]] + [None] * (b - 2)
    lims = [0, 0, 2] + [0] * (b - 3)
    cuts = [_cut(streams[0], ids=ids[0]), _cut(streams[1], seqs=seqs[1]), _cut(streams[2], max_new=2)] + [(len(streams[0]), 0)] * (b - 3)
    assert [r for _, r in cuts[:3]] == [1, 2, 3] and cuts[0][0] <= 4 and cuts[1][0] <= 6 and cuts[2][0] == 2
    return dict(stop_ids=ids, stop_sequences=seqs, max_new_tokens=lims), cuts


def _one_token_steps(c, b, step, steps=10):
    """`steps` one-token steps of a twin without stop= and of a run with the stops _stops_from takes from the twin's streams; step(model,
    ctx, state, stop) -> (logits, next_tokens)"""
    model = c.model
    twin = sv._fresh(model, c.prompts[:b])
    tstate = model.new_sampler(twin, **KW)
    t_tok, t_log, t_ctx = [], [], []
    for _ in range(steps):
        logits, nxt = step(model, twin, tstate, None)
        t_tok.append(_np(nxt).copy())
        t_log.append(logits.clone())
        t_ctx.append(_ctx_state(twin))
    streams = np.stack(t_tok, axis=1)
    kw, cuts = _stops_from(streams, b)
    ctx = sv._fresh(model, c.prompts[:b])
    state = model.new_sampler(ctx, **KW)
    stop = model.new_stopper(ctx, **kw)
    assert stop.live.tolist() == [b] and stop.tail[:, -1].tolist() == ctx.tokens.tolist()
    left = ctx.steps_left
    for s in range(steps):
        logits, nxt = step(model, ctx, state, stop)
        nxt, now = _np(nxt), _ctx_state(ctx)
        for t, (cut, _) in enumerate(cuts):
            if s < cut:                                                 # live at this step: the twin's row, bit for bit
                assert nxt[t] == streams[t, s] and torch.equal(logits[t], t_log[s][t]), (s, t)
                assert np.array_equal(now[t], t_ctx[s][t]), (s, t)
            else:                                                       # finished: -1, the context of its last step for good
                assert nxt[t] == -1 and np.array_equal(now[t], t_ctx[cut - 1][t]), (s, t)
        assert stop.emit_lens.tolist() == [int(s < cut) for cut, _ in cuts]
        assert stop.live.tolist() == [sum(s + 1 < cut or r == 0 for cut, r in cuts)]
    assert ctx.steps_left == left - steps                               # the host-side bound counts every step
    assert stop.finished.tolist() == [r for _, r in cuts] and stop.gen_lens.tolist() == [min(cut, steps) for cut, _ in cuts]
    assert max(cut for cut, r in cuts if r) + 4 <= steps                # every finished task was stepped four more times at least
    assert stop.last_token.tolist() == [int(streams[t, min(cut, steps) - 1]) for t, (cut, _) in enumerate(cuts)]


def test_step_sample_stops(case):
    _one_token_steps(case, 3, lambda model, ctx, state, stop: model.step_sample(ctx, state, stop=stop))


@pytest.mark.parametrize("b", [3, 5], ids=["in-launch-pick", "argmax-advance"])
def test_step_greedy_stops(case, b):
    _one_token_steps(case, b, lambda model, ctx, state, stop: model.step_greedy(ctx, stop=stop))


# ---- speculative steps: accepted drafts behind the stop ---------------------------------------------------------------------------------
def _spec_run(c, b, sampled, steps, source=None, stop_kw=None, lookup=False):
    """`steps` verify (or step_lookup) calls from the prompts' end.  source: per task the id stream the drafts are read from, at the
    task's own position (None: no drafts, -1).  -> [per step: dict(drafts, tokens, accepted, ctx (B, 4))], streams, stop state, lookup state"""
    model, dev = c.model, c.model.device
    ctx = sv._fresh(model, c.prompts[:b])
    samp = model.new_sampler(ctx, **KW) if sampled else None
    stop = model.new_stopper(ctx, **stop_kw) if stop_kw else None
    look = model.new_lookup(ctx, c.prompts[:b], K) if lookup else None
    out, rec = [[] for _ in range(b)], []
    for _ in range(steps):
        drafts = np.full((b, K), -1, np.int32)
        if source is not None:
            for t in range(b):
                d = source[t][len(out[t]):len(out[t]) + K]
                drafts[t, :len(d)] = d
        dd = torch.from_numpy(drafts).to(dev)
        if lookup:
            look.drafts.copy_(dd)                                       # the drafter's proposal replaced: the step is verify + the history's append
            res = model.step_lookup(ctx, look, sampler=samp, stop=stop)
        else:
            res = model.verify(ctx, dd, sampler=samp, stop=stop)
        tok, acc = _np(res.tokens).copy(), _np(res.accepted).copy()
        for t in range(b):
            out[t] += sr.emitted(tok[t].tolist())
        rec.append(dict(drafts=drafts, tokens=tok, accepted=acc, ctx=_ctx_state(ctx)))
    return rec, out, stop, look


def _pick_stop(rec, streams, b):
    """a (task, step, offset) of the record with accepted ids BEHIND the offset, and a stop that first hits exactly there: a stop id
    if the id is new to the stream at that point, else a stop sequence of the 2 .. 4 ids that end there"""
    at = [0] * b
    for s, r in enumerate(rec):
        for t in range(b):
            for j in range(int(r["accepted"][t])):                      # j < accepted: ids j + 1 .. accepted are accepted ids behind it
                g = at[t] + j
                for n in (1, 2, 3, 4):
                    if g + 1 >= n:
                        seq = streams[t][g + 1 - n:g + 1]
                        kw = dict(ids=seq) if n == 1 else dict(seqs=[seq])
                        if _cut(streams[t], **kw) == (g + 1, 1 if n == 1 else 2):
                            return t, s, j, g + 1, kw
        for t in range(b):
            at[t] += int(r["accepted"][t]) + 1
    return None


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampler"])
def test_verify_undoes_what_it_accepted_behind_a_stop(case, sampled):
    c, b, steps = case, 3, 5
    _, first, _, _ = _spec_run(c, b, sampled, steps * (K + 1))          # the same route without drafts: the ids to draft from
    rec, streams, _, _ = _spec_run(c, b, sampled, steps, source=first)
    print("accepted per step of the record:", [r["accepted"].tolist() for r in rec])
    found = _pick_stop(rec, streams, b)
    assert found is not None, "no accepted run in the record to stop inside"
    task, s_stop, j, kept, kw = found
    m = int(rec[s_stop]["accepted"][task]) + 1
    assert m - (j + 1) >= 1                                             # the cut removes at least one accepted id
    ids, seqs = [None] * b, [None] * b
    ids[task], seqs[task] = kw.get("ids"), kw.get("seqs")
    stop_kw = dict(stop_ids=ids, stop_sequences=seqs)
    for lookup in (False, True):
        got, out, stop, look = _spec_run(c, b, sampled, steps, source=first, stop_kw=stop_kw, lookup=lookup)
        for s, (g, r) in enumerate(zip(got, rec)):
            for t in range(b):
                if t != task or s < s_stop:                             # untouched by the stop: the record
                    assert np.array_equal(g["tokens"][t], r["tokens"][t]) and g["accepted"][t] == r["accepted"][t], (s, t)
                    assert np.array_equal(g["ctx"][t], r["ctx"][t]), (s, t)
            if s == s_stop:                                             # the record's row cut behind j, the counters as if j + 1 ids were emitted
                want = r["tokens"][task].copy()
                want[j + 1:] = -1
                assert np.array_equal(g["tokens"][task], want) and g["accepted"][task] == j
                after = r["ctx"][task] - [0, m - j - 1, m - j - 1, m - j - 1]
                after[0] = want[j]
                assert np.array_equal(g["ctx"][task], after)
            if s > s_stop:                                              # frozen
                assert (g["tokens"][task] == -1).all() and g["accepted"][task] == -1
                assert np.array_equal(g["ctx"][task], got[s_stop]["ctx"][task])
        assert out[task] == streams[task][:kept] and [out[t] for t in range(b) if t != task] == [streams[t] for t in range(b) if t != task]
        assert stop.gen_lens.tolist() == [len(o) for o in out] and stop.finished[task].item() == (1 if "ids" in kw else 2)
        assert stop.live.item() == b - 1
        if lookup:                                                      # nothing behind the stop entered the history
            lens, pending = _np(look.hist_lens), _np(sv._fresh(c.model, c.prompts[:b]).tokens).tolist()
            for t in range(b):
                want = c.prompts[t].tolist() + [pending[t]] + out[t]
                assert lens[t] == len(want) and _np(look.history[t, :lens[t]]).tolist() == want, t


# ---- capture ------------------------------------------------------------------------------------------------------------------------
def _motif_start(c, b, lims):
    rng = np.random.default_rng(4)
    motifs = [np.tile(rng.integers(0, c.vocab, 8), 5)[:s].astype(np.int32) for s in (16, 40, 24)][:b]
    ctx = sv._fresh(c.model, motifs)
    return ctx, c.model.new_lookup(ctx, motifs, K), c.model.new_sampler(ctx, **KW), c.model.new_stopper(ctx, max_new_tokens=lims)


@pytest.mark.parametrize("b", [1, 3])
def test_capture_replay_and_no_host_synchronisation(case, b):
    """captured after one eager call, five replays continue a twin's eager sequence: tokens, accepted, the stop state, the context and the
    drafter's state agree; the length limit of task 0 (six ids: more than one step emits, no more than six do) fires during the replays;
    an eager step synchronises nowhere"""
    c, lims = case, [6, 0, 9][:b]
    ctx, look, samp, stop = _motif_start(c, b, lims)
    eager = []
    for _ in range(6):
        res = c.model.step_lookup(ctx, look, sampler=samp, stop=stop)
        eager.append([res.accepted.clone(), res.tokens.clone()] + [getattr(stop, n).clone() for n in STOP_NAMES]
                     + [getattr(ctx, n).clone() for n in CTX_NAMES])
    assert eager[0][5].tolist() == [0] * b and stop.finished[0].item() == 3 and stop.gen_lens[0].item() == 6
    tctx, tlook, tsamp, tstop = _motif_start(c, b, lims)
    res = c.model.step_lookup(tctx, tlook, sampler=tsamp, stop=tstop)
    assert torch.equal(res.tokens, eager[0][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = c.model.step_lookup(tctx, tlook, sampler=tsamp, stop=tstop)
    for step in range(1, 6):
        graph.replay()
        torch.cuda.synchronize()
        got = [r.accepted, r.tokens] + [getattr(tstop, n) for n in STOP_NAMES] + [getattr(tctx, n) for n in CTX_NAMES]
        for i, (x, y) in enumerate(zip(got, eager[step])):
            assert torch.equal(x, y), (step, i)
    for name in ("history", "hist_lens", "drafts", "match"):
        assert torch.equal(getattr(tlook, name), getattr(look, name)), name
    assert torch.equal(tsamp.draws, samp.draws)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = c.model.step_lookup(ctx, look, sampler=samp, stop=stop)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert res.accepted[0].item() == -1 and stop.emit_lens[0].item() == 0


# ---- the generate loops ---------------------------------------------------------------------------------------------------------------
def _gen_start(c, b=3):
    ctx = sv._fresh(c.model, c.prompts[:b])
    return ctx, c.model.new_sampler(ctx, **KW)


def test_generate_sample_stops_early(case):
    c, b, n = case, 3, 16
    ctx, samp = _gen_start(c)
    toks, lps = c.model.generate_sample(ctx, samp, n)
    streams = _np(toks)
    assert streams.shape == (b, n)
    kw, cuts = _stops_from(streams, b)
    ctx, samp = _gen_start(c)
    stop = c.model.new_stopper(ctx, **kw)
    got, glp = c.model.generate_sample(ctx, samp, n, stop=stop, poll=2)
    got, last = _np(got), max(cut for cut, _ in cuts)
    print("finished after", [cut for cut, _ in cuts], "steps; the loop ran", got.shape[1], "of", n)
    assert last <= got.shape[1] <= last + 1 and got.shape[1] < n and glp.shape == got.shape
    for t, (cut, _) in enumerate(cuts):
        assert got[t, :cut].tolist() == streams[t, :cut].tolist() and (got[t, cut:] == -1).all(), t
        assert torch.equal(glp[t, :cut].view(I32), lps[t, :cut].view(I32))
    assert stop.gen_lens.tolist() == [cut for cut, _ in cuts] and stop.finished.tolist() == [r for _, r in cuts] and stop.live.item() == 0
    from zhilight_amd import ops
    with pytest.raises(ops.ZLError, match="poll"):
        c.model.generate_sample(ctx, samp, n, stop=stop, poll=0)


def test_generate_lookup_stops(case):
    """the loop's own twin without stop= gives the streams (a lookup step's logits come from another GEMM route than step_sample's, so
    its samples may differ from generate_sample's in a near-tie; the comparison is printed); the stops are taken from them"""
    c, b, n = case, 3, 16
    ctx, samp = _gen_start(c)
    plain, _ = c.model.generate_lookup(ctx, c.model.new_lookup(ctx, c.prompts[:b], K), n, sampler=samp)
    ctx, samp = _gen_start(c)
    print("generate_lookup's streams are generate_sample's:", plain == _np(c.model.generate_sample(ctx, samp, n)[0]).tolist())
    kw, cuts = _stops_from(plain, b)
    ctx, samp = _gen_start(c)
    stop = c.model.new_stopper(ctx, **kw)
    got, stats = c.model.generate_lookup(ctx, c.model.new_lookup(ctx, c.prompts[:b], K), n, sampler=samp, stop=stop)
    assert got == [plain[t][:cut] for t, (cut, _) in enumerate(cuts)]
    assert stats["finished"] == [r for _, r in cuts] == [1, 2, 3] and stats["emitted"] == [cut for cut, _ in cuts]
    assert [len(l) for l in stats["logprobs"]] == stats["emitted"] and stats["steps"] <= max(cut for cut, _ in cuts)
    assert stop.gen_lens.tolist() == stats["emitted"] and stop.live.item() == 0


def test_generate_loops_without_stop_are_the_hand_loops(case):
    c, b, n = case, 3, 6
    ctx, samp = _gen_start(c)
    toks, lps = c.model.generate_sample(ctx, samp, n)
    tctx, tsamp = _gen_start(c)
    hand = [(c.model.step_sample(tctx, tsamp)[1].clone(), tsamp.logprobs.clone()) for _ in range(n)]
    assert torch.equal(toks, torch.stack([h[0] for h in hand], dim=1)) and torch.equal(lps.view(I32), torch.stack([h[1] for h in hand], dim=1).view(I32))
    assert int(toks.min()) >= 0 and ctx.steps_left == tctx.steps_left
    ctx, samp = _gen_start(c)
    look = c.model.new_lookup(ctx, c.prompts[:b], K)
    toks, stats = c.model.generate_lookup(ctx, look, n, sampler=samp)
    tctx, tsamp = _gen_start(c)
    tlook = c.model.new_lookup(tctx, c.prompts[:b], K)
    out, acc, rounds = [[] for _ in range(b)], [0] * b, 0
    while min(len(o) for o in out) < n:
        res = c.model.step_lookup(tctx, tlook, sampler=tsamp)
        a, t = res.accepted.tolist(), res.tokens.tolist()
        for j in range(b):
            out[j] += t[j][:a[j] + 1]
            acc[j] += a[j]
        rounds += 1
    assert toks == [o[:n] for o in out] and stats["steps"] == rounds and stats["accepted"] == acc and stats["emitted"] == [len(o) for o in out]
    assert sorted(stats) == ["accepted", "emitted", "logprobs", "mean_accepted", "steps"]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(case, dev):
    from zhilight_amd import ops
    c, model = case, case.model
    ctx, samp = _gen_start(c)
    stop = model.new_stopper(ctx, stop_ids=1)
    other = sv._fresh(model, c.prompts[:2])
    osamp = model.new_sampler(other, **KW)
    for call in (lambda: model.step_sample(other, osamp, stop=stop), lambda: model.step_greedy(other, stop=stop),
                 lambda: model.verify(other, torch.zeros((2, K), dtype=I32, device=dev), stop=stop),
                 lambda: model.step_lookup(other, model.new_lookup(other, c.prompts[:2], K), stop=stop)):
        with pytest.raises(ops.ZLError, match="stop state belongs to another batch size"):
            call()
    assert stop.gen_lens.tolist() == [0, 0, 0] and stop.live.tolist() == [3]
    for match, kw in (("3 tasks, 2 lists of stop_ids", dict(stop_ids=[[1], [2]])), ("lists of stop_sequences", dict(stop_sequences=[[[1]], None])),
                      ("values of max_new_tokens", dict(max_new_tokens=[1, 2])), ("integer >= 0", dict(max_new_tokens=-1)),
                      ("outside", dict(stop_ids=c.vocab)), ("17 stop ids", dict(stop_ids=list(range(17))))):
        with pytest.raises(ops.ZLError, match=match):
            model.new_stopper(ctx, **kw)
    b = 3
    z = lambda *shape: torch.zeros(shape, dtype=I32, device=dev)                                  # noqa: E731
    good = dict(stop_ids=z(b, 2), stop_seqs=z(b, 2, 4), seq_lens=z(b, 2), max_new=z(b), gen_lens=z(b), tail=z(b, 15), last_token=z(b),
                finished=z(b), new_tokens=z(b, 4))
    ops.stop_advance(**good)                                            # the baseline is accepted
    ops.stop_advance(**{**good, "stop_ids": None, "stop_seqs": None, "seq_lens": None, "max_new": None})
    for match, change in (("at most 32", dict(new_tokens=z(b, 33))), ("gen_lens", dict(gen_lens=None)), ("tail", dict(tail=None)),
                          ("last_token", dict(last_token=None)), ("finished", dict(finished=None)), ("another batch size", dict(finished=z(b + 1))),
                          ("tail", dict(tail=z(b, 16))), ("new_tokens", dict(new_tokens=z(b, 4).long())), ("stop_ids", dict(stop_ids=z(b, 17))),
                          ("stop_seqs", dict(stop_seqs=z(b, 9, 4))), ("stop_seqs", dict(stop_seqs=z(b, 2, 17))), ("come together", dict(seq_lens=None)),
                          ("seq_lens", dict(seq_lens=z(b, 3))), ("next_tokens", dict(next_tokens=z(b))), ("live", dict(live=z(2))),
                          ("n_new = 1 only", dict(tokens=good["new_tokens"].view(-1)[:b])), ("device", dict(max_new=torch.zeros(b, dtype=I32)))):
        with pytest.raises(ops.ZLError, match=match):
            ops.stop_advance(**{**good, **change})
    torch.cuda.synchronize()
