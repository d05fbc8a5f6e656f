"""Slot admission on the GPU.  The kernel: zl_slots_admit against tests/slot_ref.py, bit for bit on every tensor, from states full of
random garbage (a row left partly stale shows), with a poisoned guard region behind every buffer.  The model, on the small GPTQ model of
test_gpu_stop.py: after LLaMA.admit a slot's rows are those of a fresh context set up through prefill_batch + new_sampler + new_stopper +
new_lookup, the slot's stream is its twin's from admission to finish, the tasks running across an admission are not disturbed, one
captured graph survives admissions and a park, and BatchServer serves a queue through three slots with every request equal to its twin."""
import types

import numpy as np
import pytest
import torch

import slot_ref as sl
import stop_ref as sr
import test_gpu_sample as gs
import test_gpu_stop as gstop
import test_slot_host as host

pytestmark = pytest.mark.gpu

_np, _guarded = gs._np, gs._guarded
I32, I64, F32 = torch.int32, torch.int64, torch.float32
TDT = {np.dtype(np.int32): I32, np.dtype(np.int64): I64, np.dtype(np.float32): F32}


# ---- the kernel against the reference -------------------------------------------------------------------------------------------------
def _upload(d, dev, guards):
    """a dict of numpy arrays -> a namespace of guarded device tensors of the same bits (None stays None)"""
    if d is None:
        return None
    ns = types.SimpleNamespace(seen=None, repetition_penalty=None, presence_penalty=None, bias_ids=None, bias_vals=None, bias_cnt=None,
                               bias_bits=None, top_n=0, top_ids=None, top_logprobs=None)
    for k, v in d.items():
        v = np.ascontiguousarray(v)
        t, g = _guarded(v.size, I32 if v.dtype.itemsize == 4 else I64, dev, v.reshape(-1).view(np.int32 if v.dtype.itemsize == 4 else np.int64))
        guards.append(g)
        setattr(ns, k, t.view(TDT[v.dtype]).view(v.shape))
    if getattr(ns, "top_ids", None) is not None:
        ns.top_n = ns.top_ids.shape[1]
    return ns


def _download(ns, like):
    return None if like is None else {k: _np(getattr(ns, k)).copy() for k in like}


@pytest.mark.parametrize("groups", [host.ALL] + [tuple(g for g in host.ALL if g != off) for off in host.ALL],
                         ids=["all"] + ["no-" + g for g in host.ALL])
@pytest.mark.parametrize("vocab,ld_extra", [(1003, 0), (1003, 1), (128256, 0)], ids=["1003", "1003-odd-rows", "128256"])
@pytest.mark.parametrize("which", ["one", "all", "scattered"])
@pytest.mark.parametrize("b", [1, 5, 33])
def test_kernel_equals_the_reference(dev, b, which, vocab, ld_extra, groups):
    """ld_extra = 1: bitmap rows of an odd number of words, so every other row is not 16-byte aligned (the dword store path) and the
    row's last word lies behind the vocabulary.  Every penalty list of the blob carries ids the kernel must skip (test_slot_host's
    poison_penalty_ids: -1 padding, vocab, 1023 at 1003 ids, the last bit of the row, INT32_MAX / MIN): slots_pack never packs them,
    the C call promises to skip them, and without the skip they would set bits of the last word and of the extra word"""
    from zhilight_amd import ops
    rng = np.random.default_rng(1000 * b + vocab + 17 * len(groups) + sum(map(ord, which + "".join(groups))) + ld_extra)
    entries, w = host.scenario(rng, b, vocab, groups, which)
    ctx, sampler, stop, lookup = host.garbage_states(rng, b, vocab, w, groups, ld_extra)
    parks = {s for s, rq in entries if rq is None}
    if "stop" not in groups:                                                # without a stop state nothing is known to be finished
        entries = [(s, rq if rq is not None else host.request(rng, vocab, w, 3)) for s, rq in entries]
        parks = set()
    for s in parks:
        stop["finished"][s] = 2
    blob, _ = ops.slots_pack(entries, vocab, w)
    _, touched = host.poison_penalty_ids(blob, entries, vocab, ops.seen_words(vocab) + ld_extra)
    assert touched or "pen" not in groups or (b == 1 and which != "one")                    # a lone slot of the empty shape
    guards = []
    dctx, dsam, dstop, dlook = (_upload(d, dev, guards) for d in (ctx, sampler, stop, lookup))
    dnew, g = _guarded(b, I32, dev)
    guards.append(g)
    before = [_download(ns, like) for ns, like in ((dctx, ctx), (dsam, sampler), (dstop, stop), (dlook, lookup))]
    for x, y in zip(before, (ctx, sampler, stop, lookup)):                  # the upload kept every bit (NaN payloads included)
        host.same(x, y, "upload")
    new = np.full(b, 12345, np.int32)
    sl.admit(blob, ctx, sampler, stop, lookup, new)
    ops.slots_admit(blob, dctx.tokens, dctx.positions, dctx.placement, dctx.valid_lens, sampler=dsam, stop=dstop, lookup=dlook,
                    draft_new=dnew, parked_ok=parks)
    torch.cuda.synchronize()
    got = [_download(ns, like) for ns, like in ((dctx, ctx), (dsam, sampler), (dstop, stop), (dlook, lookup))]
    for x, y, what in zip(got, (ctx, sampler, stop, lookup), ("ctx", "sampler", "stop", "lookup")):
        host.same(x, y, what)
    assert np.array_equal(_np(dnew), new)
    gs._intact(guards)
    rest = [t for t in range(b) if t not in {s for s, _ in entries}]
    for x, old in zip(got, before):                                         # rows of the other slots: bit-equal to before
        if x is not None:
            for k in x:
                if k != "live":
                    assert x[k][rest].tobytes() == old[k][rest].tobytes(), k


def test_kernel_drops_a_slot_outside_the_batch_and_ops_refuses_it(dev):
    from zhilight_amd import ops
    rng = np.random.default_rng(5)
    b, vocab, groups = 5, 1003, host.ALL
    w = host.widths_of(groups)
    ctx, sampler, stop, lookup = host.garbage_states(rng, b, vocab, w, groups)
    entries = [(1, host.request(rng, vocab, w, 1)), (b, host.request(rng, vocab, w, 2)), (3, host.request(rng, vocab, w, 3))]
    blob, h = ops.slots_pack(entries, vocab, w)
    guards = []
    dctx, dsam, dstop, dlook = (_upload(d, dev, guards) for d in (ctx, sampler, stop, lookup))
    args = (dctx.tokens, dctx.positions, dctx.placement, dctx.valid_lens)
    with pytest.raises(ops.ZLError, match="distinct indices of the batch of 5"):
        ops.slots_admit(blob, *args, sampler=dsam, stop=dstop, lookup=dlook)
    twice = blob.copy()
    ops.slots_records(twice)[1, 0] = 1
    with pytest.raises(ops.ZLError, match="distinct indices"):
        ops.slots_admit(twice, *args, sampler=dsam, stop=dstop, lookup=dlook)
    park, _ = ops.slots_pack([(2, None)], vocab, w)
    with pytest.raises(ops.ZLError, match="known to be finished"):
        ops.slots_admit(park, *args, sampler=dsam, stop=dstop, lookup=dlook)
    good, _ = ops.slots_pack([entries[0], entries[2]], vocab, w)
    for kw, match in ((dict(sampler=dsam, stop=None, lookup=dlook), "stop state differ"), (dict(sampler=dsam, stop=dstop, lookup=None), "history's cap"),
                      (dict(sampler=None, stop=dstop, lookup=dlook), "penalty bitmap")):
        with pytest.raises(ops.ZLError, match=match):
            ops.slots_admit(good, *args, **kw)
    for x, y in zip((dctx, dsam, dstop, dlook), (ctx, sampler, stop, lookup)):      # refused before any launch
        host.same(_download(x, y), y, "refused")
    # the C call itself drops the record: the launch runs, slots 1 and 3 are admitted, nothing else moves
    from zhilight_amd import _lib
    import ctypes as C
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                                                # noqa: E731
    dev_blob = torch.from_numpy(blob).to(dev)
    st = _lib.lib().zl_slots_admit(
        p(dev_blob), h["n"], h["rec"], b, vocab, p(dctx.tokens), p(dctx.positions), p(dctx.placement), p(dctx.valid_lens), p(dsam.temperature),
        p(dsam.top_k), p(dsam.top_p), p(dsam.seeds), p(dsam.draws), p(dsam.logprobs), p(dsam.u), p(dsam.repetition_penalty), p(dsam.presence_penalty),
        p(dsam.seen), dsam.seen.shape[1], p(dsam.bias_ids), p(dsam.bias_vals), p(dsam.bias_cnt), p(dsam.bias_bits), w["bias_ld"],
        dsam.bias_bits.shape[1], p(dsam.top_ids), p(dsam.top_logprobs), dsam.top_n, p(dstop.stop_ids), p(dstop.stop_seqs), p(dstop.seq_lens),
        w["n_ids"], w["n_seqs"], w["seq_ld"], p(dstop.max_new), p(dstop.gen_lens), p(dstop.tail), p(dstop.last_token), p(dstop.finished),
        p(dstop.emit_lens), p(dstop.live), p(dlook.history), w["hist_cap"], p(dlook.hist_lens), None,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    sl.admit(blob, ctx, sampler, stop, lookup)
    for x, y, what in zip((dctx, dsam, dstop, dlook), (ctx, sampler, stop, lookup), ("ctx", "sampler", "stop", "lookup")):
        host.same(_download(x, y), y, what)
    gs._intact(guards)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
LEN_BUF, K = gstop.LEN_BUF, gstop.K
BIAS_LD, TOP = 4, 3
WIDE = (16, 8, 16)
SAMPLER = sl.SAMPLER + sl.PENALTY + sl.BIAS + sl.TOP
STOP = sl.STOP
LOOK = ("history", "hist_lens", "drafts", "match")
DEFAULTS = dict(temperature=1.0, top_k=0, top_p=1.0, seed=0, repetition_penalty=1.0, presence_penalty=0.0, penalty_tokens=None,
                logit_bias=None, stop_ids=None, stop_sequences=None, max_new_tokens=0)


@pytest.fixture(scope="module")
def case(dev):
    c = gstop._Case()
    rng, c.cfg, c.sd, c.model = gstop._gptq_model(dev)
    c.vocab = c.cfg.vocab_size
    c.prompts = [rng.integers(0, c.vocab, s).astype(np.int32) for s in (5, 40, 17, 23, 9, 100, 64)]
    c.rng = rng
    return c


def _req(c, i, **kw):
    """request i of the tests: sampling with penalties and a bias, each with another seed"""
    rq = dict(temperature=0.7 + 0.1 * (i % 3), top_k=20, top_p=0.95, seed=1000 + 7 * i, repetition_penalty=1.0 + 0.1 * (i % 2),
              presence_penalty=0.25 * (i % 3 == 2), penalty_tokens=c.prompts[i % len(c.prompts)][:6].tolist(),
              logit_bias={(11 * i + 3) % c.vocab: -float("inf"), (5 * i + 1) % c.vocab: 1.5})
    rq.update(kw)
    return rq


def _setup(c, b, placed, lookup, len_buf=LEN_BUF, cache=None, matched=None):
    """A fresh context of b slots set up WITHOUT admit: ONE prefill_batch over placed = [(slot, prompt, request)] in that order, then
    new_sampler / new_stopper / new_lookup at the full widths with the requests' values in their slots and the defaults elsewhere; a
    request's length limit is the clamped one, the other slots get the limit 1 so that they finish at once.  cache: the prompts go
    through prefill_cached and this prefix cache instead, and the list `matched` takes what it supplied per prompt.
    -> (ctx, sampler, stop, lookup state or None, the prefill's logits)"""
    from zhilight_amd import ops
    model = c.model
    ctx = model.new_context(b, len_buf, 0)
    if cache is None:
        logits = model.prefill_batch(ctx, [s for s, _, _ in placed], [torch.from_numpy(p) for _, p, _ in placed])
    else:
        logits, got = model.prefill_cached(ctx, cache, [s for s, _, _ in placed], [torch.from_numpy(p) for _, p, _ in placed])
        matched += got
    per = {k: [v] * b for k, v in DEFAULTS.items()}
    per["max_new_tokens"] = [1] * b
    hist = [[] for _ in range(b)]
    for s, p, rq in placed:
        for k in DEFAULTS:
            if k in rq:
                per[k][s] = rq[k]
        per["max_new_tokens"][s] = ops.slot_max_new(len(p), rq.get("max_new_tokens", 0), len_buf, K if lookup else 0)
        hist[s] = p
    samp = model.new_sampler(ctx, **{k: per[k] for k in ("temperature", "top_k", "top_p", "seed", "repetition_penalty", "presence_penalty",
                                                         "logit_bias")},
                             penalty_tokens=[v if v is not None else [] for v in per["penalty_tokens"]], top_logprobs=TOP, penalties=True,
                             bias_ld=BIAS_LD)
    stop = model.new_stopper(ctx, stop_ids=per["stop_ids"], stop_sequences=per["stop_sequences"], max_new_tokens=per["max_new_tokens"],
                             widths=WIDE)
    look = model.new_lookup(ctx, hist, K) if lookup else None
    ctx.steps_left = 1 << 60            # the test bounds its steps itself: every request ends by its clamped limit, inside its buffer
    return ctx, samp, stop, look, logits


def _snap(ctx, samp, stop, look):
    d = {"ctx." + n: getattr(ctx, n).clone() for n in sl.CTX}
    d.update({"sampler." + n: getattr(samp, n).clone() for n in SAMPLER})
    d.update({"stop." + n: getattr(stop, n).clone() for n in STOP})
    if look is not None:
        d.update({"lookup." + n: getattr(look, n).clone() for n in LOOK})
    d.update({f"kv.{t}": kv.clone() for t, kv in enumerate(ctx.kv)})
    return d


def _bits(t):
    return t.view(I32) if t.dtype == F32 else t


def _rows_equal(a, b, slots, what, hist_lens=None):
    """the rows `slots` of two snapshots are bit-equal (a history row: its first hist_lens ids -- the rest is never read)"""
    for k in a:
        if k.startswith("kv.") or k == "stop.live":
            continue
        for s in slots:
            x, y = _bits(a[k][s]), _bits(b[k][s])
            if k == "lookup.history":
                n = int(a["lookup.hist_lens"][s])
                x, y = x[:n], y[:n]
            assert torch.equal(x, y), (what, k, s)


def _step(model, ctx, samp, stop, look):
    """one step by the state's method -> (ids emitted per slot (B, width) int32 with -1 behind them, logits, log-probabilities)"""
    b = ctx.tokens.numel()
    if look is not None:
        res = model.step_lookup(ctx, look, sampler=samp, stop=stop)
        return res.tokens.clone(), res.logits.view(b, K + 1, -1).clone(), samp.row_logprobs.clone()
    logits, nxt = model.step_sample(ctx, samp, stop=stop)
    return nxt.to(I32).view(b, 1), logits.view(b, 1, -1).clone(), samp.logprobs.view(b, 1).clone()


def _start_running(c, lookup):
    """three tasks set up the old way that have run six steps: task 2 has finished (limit 4), tasks 0 and 1 run"""
    placed = [(t, c.prompts[t], _req(c, t, max_new_tokens=(0, 0, 4)[t])) for t in range(3)]
    ctx, samp, stop, look, _ = _setup(c, 3, placed, lookup)
    for _ in range(6):
        _step(c.model, ctx, samp, stop, look)
    assert stop.finished.tolist() == [0, 0, 3]
    return ctx, samp, stop, look


@pytest.mark.parametrize("lookup", [False, True], ids=["sample", "lookup"])
def test_admitted_rows_are_a_fresh_contexts_rows(case, lookup):
    c, model = case, case.model
    ctx, samp, stop, look = _start_running(c, lookup)
    pa, pb = c.prompts[3], c.prompts[4]
    ra = _req(c, 3, stop_ids=[3, 4], stop_sequences=[[1, 2], [5] * 16], max_new_tokens=9)
    rb = _req(c, 4)                                                         # no limit of its own: the clamp's
    before = _snap(ctx, samp, stop, look)
    ptrs = {k: v.data_ptr() for k, v in vars(samp).items() if torch.is_tensor(v)}
    logits = model.admit(ctx, [2, 0], [torch.from_numpy(pa), torch.from_numpy(pb)], [ra, rb], samp, stop, look).clone()
    after = _snap(ctx, samp, stop, look)
    fctx, fsamp, fstop, flook, flogits = _setup(c, 3, [(2, pa, ra), (0, pb, rb)], lookup)
    fresh = _snap(fctx, fsamp, fstop, flook)
    assert torch.equal(logits, flogits)
    _rows_equal(after, fresh, [2, 0], "admitted")
    for s, p in ((2, pa), (0, pb)):                                         # the prompt's K/V rows
        assert torch.equal(after[f"kv.{s}"][:, :, :len(p)], fresh[f"kv.{s}"][:, :, :len(p)]), s
    _rows_equal(after, before, [1], "the running task")
    assert torch.equal(after["kv.1"], before["kv.1"])
    assert stop.live.item() == 3 and stop.max_new.tolist()[0] == LEN_BUF - len(pb) - (K if lookup else 0) - 1 and stop.max_new.tolist()[2] == 9
    assert ptrs == {k: v.data_ptr() for k, v in vars(samp).items() if torch.is_tensor(v)}
    assert ctx.slot_guard == {2: len(pa) + 9 + (K if lookup else 0) + 1, 0: LEN_BUF}


def _stream(model, ctx, samp, stop, look, slot, steps):
    """step until `slot` has finished (at most `steps` steps) -> [(ids, logits rows, log-probabilities)] of the slot per step"""
    out = []
    for _ in range(steps):
        tok, logits, lp = _step(model, ctx, samp, stop, look)
        out.append((tok[slot].tolist(), logits[slot], lp[slot]))
        if stop.finished[slot].item():
            break
    return out


def _same_stream(got, want, what):
    assert len(got) == len(want), what
    for i, ((t, l, p), (tt, ll, pp)) in enumerate(zip(got, want)):
        m = len(sr.emitted(t))
        assert t == tt and m >= 1, (what, i)
        assert torch.equal(l[:m], ll[:m]) and torch.equal(p[:m].view(I32), pp[:m].view(I32)), (what, i)


@pytest.mark.parametrize("lookup", [False, True], ids=["step_sample", "step_lookup"])
def test_an_admitted_slots_stream_is_its_twins(case, lookup):
    """the request alone in the same slot of a fresh context, set up without admit, is the twin; the stop sequence is taken from a scout
    run of that twin, so it ends the request (reason 2) in the middle of its stream"""
    c, model = case, case.model
    prompt = np.tile(c.prompts[3][:8], 3) if lookup else c.prompts[3]       # a repeating prompt: the drafter finds matches
    scout = _setup(c, 3, [(2, prompt, _req(c, 3, max_new_tokens=12))], lookup)
    ids = [i for t, _, _ in _stream(model, *scout[:4], 2, 12) for i in sr.emitted(t)]
    rq = _req(c, 3, max_new_tokens=12, stop_sequences=[ids[4:6]])
    twin = _setup(c, 3, [(2, prompt, rq)], lookup)
    want = _stream(model, *twin[:4], 2, 12)
    assert twin[2].finished[2].item() == 2 and 2 <= twin[2].gen_lens[2].item() <= 6
    # the running batch, and its own twin that is never interrupted
    ctx, samp, stop, look = _start_running(c, lookup)
    plain = _start_running(c, lookup)
    model.admit(ctx, [2], [torch.from_numpy(prompt)], [rq], samp, stop, look)
    got, others, others_plain = [], [], []
    for _ in range(len(want)):
        tok, logits, lp = _step(model, ctx, samp, stop, look)
        got.append((tok[2].tolist(), logits[2], lp[2]))
        others.append((tok[:2].clone(), logits[:2], lp[:2]))
        tok, logits, lp = _step(model, *plain)
        others_plain.append((tok[:2].clone(), logits[:2], lp[:2]))
    _same_stream(got, want, "admitted")
    assert stop.finished[2].item() == 2 and stop.gen_lens[2].item() == twin[2].gen_lens[2].item()
    for i, ((t, l, p), (tt, ll, pp)) in enumerate(zip(others, others_plain)):       # tasks 0 and 1 ran across the admission undisturbed
        assert torch.equal(t, tt) and torch.equal(l, ll) and torch.equal(p.view(I32), pp.view(I32)), i
    assert stop.finished.tolist()[:2] == [0, 0]


def _scripted_run(c, captured):
    """steps of step_sample around two admissions and a park; with captured=True every step after the first is a replay of ONE graph"""
    model = c.model
    placed = [(t, c.prompts[t], _req(c, t, max_new_tokens=(4, 0, 6)[t])) for t in range(3)]
    ctx, samp, stop, _, _ = _setup(c, 3, placed, False)
    ptrs = {k: v.data_ptr() for o in (ctx, samp, stop) for k, v in vars(o).items() if torch.is_tensor(v)}
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
                    eager = [t.clone() for t in out]
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        out = model.step_sample(ctx, samp, stop=stop)
                    rec.append(eager + [samp.logprobs.clone()] + [getattr(stop, n).clone() for n in STOP] + [getattr(ctx, n).clone() for n in sl.CTX])
                    continue
            rec.append([out[0].clone(), out[1].clone(), samp.logprobs.clone()] + [getattr(stop, n).clone() for n in STOP]
                       + [getattr(ctx, n).clone() for n in sl.CTX])

    steps(6)
    assert stop.finished.tolist() == [3, 0, 3]
    model.admit(ctx, [0], [torch.from_numpy(c.prompts[3])], [_req(c, 3, max_new_tokens=2)], samp, stop)
    steps(3)
    assert stop.finished.tolist() == [3, 0, 3]
    model.admit(ctx, [2], [torch.from_numpy(c.prompts[4])], [_req(c, 4, max_new_tokens=20)], samp, stop)
    steps(4)
    model.park(ctx, [0], samp, stop, finished=stop.finished.tolist())
    steps(3)
    assert ctx.tokens[0].item() == 0 and ctx.positions[0].item() == 0 and ctx.valid_lens[0].item() == 1 and stop.finished.tolist() == [3, 0, 0]
    assert ptrs == {k: v.data_ptr() for o in (ctx, samp, stop) for k, v in vars(o).items() if torch.is_tensor(v)}
    return rec


def test_one_captured_graph_across_admissions_and_a_park(case):
    eager = _scripted_run(case, False)
    replayed = _scripted_run(case, True)
    assert len(eager) == len(replayed) == 16
    for s, (a, b) in enumerate(zip(eager, replayed)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(_bits(x), _bits(y)), (s, i)
    assert eager[-1][1][0].item() == -1                                 # the parked slot emits nothing


# ---- BatchServer ----------------------------------------------------------------------------------------------------------------------
LIMITS = (6, 12, 30, 9, 3, 0, 200)                                          # requests 5 and 6 (100 and 64 tokens) run into the clamp


def _serve(c, capture, lookup_k=0, **kw):
    from zhilight_amd.serving import BatchServer
    srv = BatchServer(c.model, 3, LEN_BUF, bias_ld=BIAS_LD, top_logprobs=TOP, lookup_k=lookup_k, capture=capture, poll=4, **kw)
    for i, p in enumerate(c.prompts):
        srv.submit(p, **_req(c, i, max_new_tokens=LIMITS[i]))
    return srv, srv.run()


def _twins(c, srv, lookup, prompts=None, reqs=None, **setup):
    """every request's (first token, ids, log-probabilities, reason) from a context rebuilt from the server's admission log; prompts /
    reqs: the requests' (default: the seven of _serve); setup: _setup's len_buf / cache / matched"""
    out = {}
    prompts = c.prompts if prompts is None else prompts
    reqs = [_req(c, r, max_new_tokens=LIMITS[r]) for r in range(len(LIMITS))] if reqs is None else reqs
    for _, group in srv.log:
        placed = [(s, prompts[r], reqs[r]) for s, r in group]
        ctx, samp, stop, look, _ = _setup(c, srv.b, placed, lookup, **setup)
        first = ctx.tokens.tolist()
        ids, lps = {r: [] for _, r in group}, {r: [] for _, r in group}
        for _ in range(srv.len_buf):
            if stop.live.item() == 0:
                break
            tok, _, lp = _step(c.model, ctx, samp, stop, look)
            tok, lp = tok.tolist(), lp.tolist()
            for s, r in group:
                m = len(sr.emitted(tok[s]))
                ids[r] += tok[s][:m]
                lps[r] += lp[s][:m]
        fin = stop.finished.tolist()
        for s, r in group:
            out[r] = (first[s], ids[r], lps[r], fin[s])
    return out


@pytest.mark.parametrize("lookup", [False, True], ids=["step_sample", "step_lookup"])
def test_batch_server_serves_seven_requests_through_three_slots(case, lookup):
    from zhilight_amd import ops
    c = case
    srv, res = _serve(c, False, K if lookup else 0)
    assert sorted(res) == list(range(7)) and not srv.queue and not srv.active
    assert [g for _, g in srv.log][0] == [(0, 0), (1, 1), (2, 2)] and len(srv.log) >= 3 and srv.stats["admissions"] == len(srv.log)
    twins = _twins(c, srv, lookup)
    for r in range(7):
        first, ids, lps, fin = twins[r]
        got = res[r]
        assert (got["first_token"], got["tokens"], got["reason"]) == (first, ids, fin), r
        assert np.array_equal(np.asarray(got["logprobs"], np.float32).view(np.int32), np.asarray(lps, np.float32).view(np.int32)), r
        assert len(got["top_ids"]) == len(ids) and all(len(t) == TOP for t in got["top_ids"]), r
        assert min(got["tokens"]) >= 0 and got["reason"] in (1, 2, 3), r   # nothing of a finished or parked slot reached a request
    k = K if lookup else 0
    for r in (5, 6):                                                        # the clamped ones end by length exactly at the clamp
        clamp = LEN_BUF - len(c.prompts[r]) - k - 1
        assert res[r]["clamped"] == clamp == ops.slot_max_new(len(c.prompts[r]), LIMITS[r], LEN_BUF, k)
        assert res[r]["reason"] == 3 and len(res[r]["tokens"]) == clamp, r
    for r in (0, 1, 2, 3, 4):
        assert res[r]["reason"] == 3 and len(res[r]["tokens"]) == LIMITS[r], r
    st = srv.stats
    assert st["live_slot_steps"] + st["finished_slot_steps"] + st["parked_slot_steps"] == 3 * st["steps"] and st["parks"] >= 1
    srv2, res2 = _serve(c, True, K if lookup else 0)                        # the steps as replays of one captured graph
    assert srv2.graph is not None and srv2.log == srv.log
    for r in range(7):
        assert res2[r] == res[r] or all(_same(res2[r][k2], res[r][k2]) for k2 in res[r]), r


def _same(x, y):
    """equal with NaN == NaN (the top-N rows hold NaN behind the vocabulary's end)"""
    return np.array_equal(np.asarray(x, np.float64), np.asarray(y, np.float64), equal_nan=True)


def test_batch_server_through_a_prefix_cache(case):
    """two requests that share a 128-token prefix, one slot: the second finds the first one's block in the cache.  The cached run
    encodes the second prompt in another call shape than the run without the cache (9 rows behind 128 loaded ones, whose K/V the first
    prompt's 133-row call computed, against 137 rows at once), so its logits agree with that run's only to the GEMM routes' fp16 rounding
    (test_gpu_prefix_cache.py holds the bit-exact bar against the same call shape).  The requests are therefore greedy: a greedy pick
    depends on the margin between the two largest logits alone, where a sampled one moves with every boundary of the running sum."""
    from zhilight_amd.serving import BatchServer
    c = case
    rng = np.random.default_rng(9)
    prefix = rng.integers(0, c.vocab, 128).astype(np.int32)
    prompts = [np.concatenate([prefix, rng.integers(0, c.vocab, n).astype(np.int32)]) for n in (5, 9)]
    runs = []
    for cached in (False, True):
        srv = BatchServer(c.model, 1, 256, bias_ld=BIAS_LD, poll=4, prefix_blocks=8 if cached else 0)
        for i, p in enumerate(prompts):
            srv.submit(p, **_req(c, i, max_new_tokens=10, temperature=0.0))
        runs.append((srv, srv.run()))
    (plain_srv, plain), (srv, res) = runs
    assert srv.matched == {0: 0, 1: 128} and plain_srv.matched == {}
    for r in (0, 1):
        assert res[r]["tokens"] == plain[r]["tokens"] and len(res[r]["tokens"]) == 10 and res[r]["first_token"] == plain[r]["first_token"], r


def test_batch_server_admits_groups_through_a_prefix_cache(case):
    """two slots, four SAMPLED requests with a common 128-token prefix and equal limits, so that the slots free up together: round 1
    admits two prompts in one admit(cache=) call (nothing matched, the common block saved once), round 2 the other two, both served from
    the cache.  The twin replays the admission log through prefill_cached and a cache of its own -- the same call shapes on the same
    cache contents -- so the bar is the bit-exact one of the other server tests, sampling included."""
    from zhilight_amd.serving import BatchServer
    c = case
    rng = np.random.default_rng(11)
    prefix = rng.integers(0, c.vocab, 128).astype(np.int32)
    prompts = [np.concatenate([prefix, rng.integers(0, c.vocab, n).astype(np.int32)]) for n in (5, 9, 3, 12)]
    reqs = [_req(c, i, max_new_tokens=8) for i in range(4)]
    srv = BatchServer(c.model, 2, 256, bias_ld=BIAS_LD, top_logprobs=TOP, poll=4, prefix_blocks=8)
    for p, rq in zip(prompts, reqs):
        srv.submit(p, **rq)
    res = srv.run()
    assert [g for _, g in srv.log] == [[(0, 0), (1, 1)], [(0, 2), (1, 3)]] and srv.matched == {0: 0, 1: 0, 2: 128, 3: 128}
    matched = []
    twins = _twins(c, srv, False, prompts, reqs, len_buf=256, cache=c.model.new_prefix_cache(srv.ctx, 8), matched=matched)
    assert matched == [0, 0, 128, 128]
    for r in range(4):
        first, ids, lps, fin = twins[r]
        assert (res[r]["first_token"], res[r]["tokens"], res[r]["reason"]) == (first, ids, fin) and len(ids) == 8 and fin == 3, r
        assert np.array_equal(np.asarray(res[r]["logprobs"], np.float32).view(np.int32), np.asarray(lps, np.float32).view(np.int32)), r
    with pytest.raises(Exception, match="give one of them"):
        BatchServer(c.model, 1, 256, prefix_blocks=2, prefix_cache=srv.cache)


def test_steps_left_rises_when_a_guarded_slot_replaces_the_one_that_bounded_it(case):
    """prompts of 5, 100 and 17 tokens in buffers of 128 rows: the long one bounds steps_left at 28; three steps later it makes room
    for an admitted (guarded) request, and the bound becomes that of the 17-token task, 111 - 3; parking-or-admitting the rest frees it"""
    c, model = case, case.model
    lens = (5, 100, 17)
    ctx = model.new_context(3, LEN_BUF, 0)
    model.prefill_batch(ctx, [0, 1, 2], [torch.from_numpy(c.prompts[i]) for i in (0, 5, 2)])
    assert [len(c.prompts[i]) for i in (0, 5, 2)] == list(lens) and ctx.steps_left == LEN_BUF - 100
    samp = model.new_sampler(ctx, temperature=0.8, seed=3, penalties=True, bias_ld=BIAS_LD)
    stop = model.new_stopper(ctx, widths=WIDE)
    for _ in range(3):
        model.step_sample(ctx, samp, stop=stop)
    assert ctx.steps_left == LEN_BUF - 100 - 3
    model.admit(ctx, [1], [torch.from_numpy(c.prompts[4])], [_req(c, 4, max_new_tokens=5)], samp, stop)
    assert ctx.steps_left == LEN_BUF - 17 - 3 and ctx.slot_guard == {1: len(c.prompts[4]) + 5 + 1}
    model.step_sample(ctx, samp, stop=stop)
    model.admit(ctx, [2], [torch.from_numpy(c.prompts[3])], [_req(c, 3)], samp, stop)
    assert ctx.steps_left == LEN_BUF - 5 - 4
    model.admit(ctx, [0], [torch.from_numpy(c.prompts[2])], [{}], samp, stop)
    assert ctx.steps_left == 1 << 60 and not ctx.slot_room
    model.prefill_batch(ctx, [0], [torch.from_numpy(c.prompts[1])])           # a plain prefill takes the slot out of the guard
    assert ctx.steps_left == LEN_BUF - 40 and 0 not in ctx.slot_guard
    torch.cuda.synchronize()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(case, dev):
    from zhilight_amd import ops
    c, model = case, case.model
    ctx, samp, stop, look = _start_running(c, True)
    narrow = model.new_sampler(ctx, temperature=0.5)                        # no bitmap, no bias rows
    small = model.new_stopper(ctx, stop_ids=[1])                            # widths (1, 1, 1)
    q8 = model.new_context(3, LEN_BUF, 0, kv_cache_dtype="int8")
    before = _snap(ctx, samp, stop, look)
    left, guard = ctx.steps_left, dict(ctx.slot_guard)
    p = [torch.from_numpy(c.prompts[3])]
    long = [torch.from_numpy(np.resize(c.prompts[5], LEN_BUF - 1 - K))]     # fits the buffer, leaves no room behind K draft rows
    cases = [
        ("distinct indices", lambda: model.admit(ctx, [1, 1], p * 2, [{}, {}], samp, stop, look)),
        ("distinct indices", lambda: model.admit(ctx, [3], p, [{}], samp, stop, look)),
        ("one prompt", lambda: model.admit(ctx, [1], p * 2, [{}], samp, stop, look)),
        ("one request per slot", lambda: model.admit(ctx, [1], p, [{}, {}], samp, stop, look)),
        ("does not fit", lambda: model.admit(ctx, [1], [torch.zeros(LEN_BUF, dtype=I32)], [{}], samp, stop, look)),
        ("leaves no room for one generated token", lambda: model.admit(ctx, [1], long, [{}], samp, stop, look)),
        ("no bitmap", lambda: model.admit(ctx, [1], p, [dict(repetition_penalty=1.2)], narrow, stop, look)),
        ("no bias rows", lambda: model.admit(ctx, [1], p, [dict(logit_bias={1: 1.0})], narrow, stop, look)),
        ("beyond the stop state's widths", lambda: model.admit(ctx, [1], p, [dict(stop_ids=[1, 2])], samp, small, look)),
        ("5 bias ids", lambda: model.admit(ctx, [1], p, [dict(logit_bias={i: 1.0 for i in range(5)})], samp, stop, look)),
        ("temperature >= 0", lambda: model.admit(ctx, [1], p, [dict(temperature=-1)], samp, stop, look)),
        ("max_new_tokens is an integer >= 0", lambda: model.admit(ctx, [1], p, [dict(max_new_tokens=-1)], samp, stop, look)),
        ("max_new_tokens is an integer >= 0", lambda: model.admit(ctx, [1], p, [dict(max_new_tokens=1.5)], samp, stop, look)),
        ("max_new_tokens is an integer >= 0", lambda: model.admit(ctx, [1], p, [dict(max_new_tokens=True)], samp, stop, look)),
        ("outside", lambda: model.admit(ctx, [1], p, [dict(stop_ids=[c.vocab])], samp, stop, look)),
        ("no stop state", lambda: model.admit(ctx, [1], p, [dict(max_new_tokens=3)], samp, None, look)),
        ("not on the INT8 KV cache", lambda: model.admit(q8, [1], p, [{}], samp, stop, look)),
        ("kv_history", lambda: model.admit(ctx, [1], p, [{}], samp, stop, look, kv_history="x")),
        ("another batch size", lambda: model.admit(model.new_context(2, LEN_BUF, 0), [1], p, [{}], samp, stop, look)),
        ("known to be finished", lambda: model.park(ctx, [2], samp, stop, look)),
        ("known to be finished", lambda: model.park(ctx, [0], samp, stop, look, finished=stop.finished.tolist())),
        ("distinct indices", lambda: model.park(ctx, [2, 2], samp, stop, look, finished=[3, 3, 3])),
        ("needs the stop state", lambda: model.park(ctx, [2], samp, None, look, finished=[3, 3, 3])),
    ]
    for match, call in cases:
        with pytest.raises(ops.ZLError, match=match):
            call()
    tp, model.tp = model.tp, object()
    try:
        with pytest.raises(ops.ZLError, match="tensor parallelism"):
            model.admit(ctx, [1], p, [{}], samp, stop, look)
    finally:
        model.tp = tp
    after = _snap(ctx, samp, stop, look)
    for k in before:                                                        # nothing ran: every tensor as before
        assert torch.equal(_bits(before[k]), _bits(after[k])), k
    assert ctx.steps_left == left and ctx.slot_guard == guard
    model.park(ctx, [2], samp, stop, look, finished=stop.finished.tolist())                                   # and the accepted calls
    model.admit(ctx, [2], p, [_req(c, 3)], samp, stop, look)
    torch.cuda.synchronize()
