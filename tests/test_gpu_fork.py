"""Forked samples on the GPU.  The kernel: zl_kv_fork (ops.kv_fork) against tests/fork_ref.py over the WHOLE ragged buffers of six tasks,
pre-filled with random bytes and with a poisoned guard region behind every buffer and every bookkeeping vector: the copied rows, the
destination rows above them, the sources and the bystanders, bit for bit; both layouts, 16-bit rows, the fp32 scale plane and 36-byte
rows that only the dword path can move; the default piece and one of 48 bytes.  The model, on the small GPTQ model of test_gpu_slots.py:
LLaMA.admit_samples of one group of three slots against its twin, the same three requests admitted by three single-slot calls (every
prompt encode of the same shape) -- K/V rows, every state row and 12 steps of every slot bit for bit --, on an INT8 cache, through a
prefix cache, next to a running slot, under one captured graph, and BatchServer's n / best_of / sample_first."""
import ctypes as C

import numpy as np
import pytest
import torch

import fork_ref as fr
import sample_ref as sref
import stop_ref as sr
import test_gpu_sample as gs
import test_gpu_slots as tslots

pytestmark = pytest.mark.gpu

_guarded = gs._guarded
I32 = torch.int32
LAYERS, LENS, B = 3, (40, 64, 33, 128, 7, 64), 6
# source 0 -> 1, 2, 4 with 33, 0 and 7 rows (7 = the whole of task 4's buffer), source 3 -> 5 with one row, both self-descriptors
DESCS = {
    "override": [(0, 1, 33, 77), (0, 2, 0, 77), (0, 4, 7, 77), (0, 0, 0, 77), (3, 5, 1, -1), (3, 3, 0, -1)],
    "no-override": [(0, 1, 33, -1), (0, 2, 0, 9), (0, 4, 7, -1), (0, 0, 0, -1), (3, 5, 1, 12), (3, 3, 0, -1)],
}


# ---- the launch ---------------------------------------------------------------------------------------------------------------------------
def _setup(dev, rng, hkv, row_bytes, bshd):
    """-> (numpy buffers, device views of guarded copies, (k, v) pointer tables, buf_lens, numpy ctx, device ctx, guards)"""
    bufs, d_bufs, guards = [], [], []
    for n in LENS:
        a = rng.integers(0, 256, (LAYERS, 2, n, hkv, row_bytes) if bshd else (LAYERS, 2, hkv, n, row_bytes), dtype=np.uint8)
        t, g = _guarded(a.size // 4, I32, dev, a.reshape(-1).view(np.int32))
        bufs.append(a)
        d_bufs.append(t.view(torch.uint8).view(a.shape))
        guards.append(g)
    tables = [torch.tensor([[t[l, kv].data_ptr() for t in d_bufs] for l in range(LAYERS)], dtype=torch.int64, device=dev) for kv in (0, 1)]
    ctx = {f: rng.integers(0, 1 << 20, B).astype(np.int32) for f in fr.CTX}
    d_ctx = {}
    for f in fr.CTX:
        d_ctx[f], g = _guarded(B, I32, dev, ctx[f])
        guards.append(g)
    return bufs, d_bufs, tables, torch.tensor(LENS, dtype=I32, device=dev), ctx, d_ctx, guards


def _check(bufs, d_bufs, ctx, d_ctx, guards, what):
    torch.cuda.synchronize()
    for t in range(B):
        assert np.array_equal(d_bufs[t].cpu().numpy(), bufs[t]), (what, "buffer", t)
    for f in fr.CTX:
        assert np.array_equal(d_ctx[f].cpu().numpy(), ctx[f]), (what, f)
    gs._intact(guards)


@pytest.mark.parametrize("which", sorted(DESCS))
@pytest.mark.parametrize("bshd", [True, False], ids=["bshd", "bhsd"])
@pytest.mark.parametrize("row_bytes", [4, 36, 256])
@pytest.mark.parametrize("hkv", [1, 2])
def test_kv_fork_is_exact_over_whole_buffers_and_bookkeeping(dev, hkv, row_bytes, bshd, which):
    from zhilight_amd import ops
    desc = DESCS[which]
    for piece in (0, 48):                                                   # the default piece; 48 bytes: many pieces, ragged tails
        rng = np.random.default_rng(1000 * hkv + row_bytes + 7 * bshd + piece)
        bufs, d_bufs, (k_tab, v_tab), buf_lens, ctx, d_ctx, guards = _setup(dev, rng, hkv, row_bytes, bshd)
        before = [b.copy() for b in bufs]
        out = ops.kv_fork(desc, k_tab, v_tab, buf_lens, hkv, row_bytes, bshd=bshd, buf_lens_host=LENS if piece else None,
                          ctx_rows=tuple(d_ctx[f] for f in fr.CTX), piece_bytes=piece)
        assert out.shape == (len(desc), 4)
        assert fr.fork(desc, bufs, LENS, bshd, 33, ctx) == desc
        assert any((a != b).any() for a, b in zip(bufs, before))             # the model moved something
        _check(bufs, d_bufs, ctx, d_ctx, guards, ("with bookkeeping", piece))
        # the scale plane's call: NULL bookkeeping pointers, the vectors stay as they are
        bufs, d_bufs, (k_tab, v_tab), buf_lens, ctx, d_ctx, guards = _setup(dev, rng, hkv, row_bytes, bshd)
        ops.kv_fork(desc, k_tab, v_tab, buf_lens, hkv, row_bytes, bshd=bshd, piece_bytes=piece)
        fr.fork(desc, bufs, LENS, bshd, 33, None)
        _check(bufs, d_bufs, ctx, d_ctx, guards, ("without bookkeeping", piece))


def test_kv_fork_drops_bad_descriptors_and_launches_nothing_for_none(dev):
    from zhilight_amd import _lib, ops
    hkv, rb, max_rows = 2, 256, 8
    rng = np.random.default_rng(3)
    bufs, d_bufs, (k_tab, v_tab), buf_lens, ctx, d_ctx, guards = _setup(dev, rng, hkv, rb, True)
    args = (k_tab, v_tab, buf_lens, hkv, rb)
    rows4 = tuple(d_ctx[f] for f in fr.CTX)
    assert ops.kv_fork([], *args, ctx_rows=rows4) is None                   # n == 0
    for bad in ([(0, 6, 1, 0)], [(0, 1, 41, 0)], [(3, 4, 8, 0)], [(0, 1, 3, 0), (2, 1, 3, 0)], [(0, 1, 3, 0), (1, 2, 3, 0)],
                [(0, 1, 3, 5), (0, 0, 0, 6)], [(0, 1, 3)]):
        with pytest.raises(ops.ZLError):
            ops.kv_fork(bad, *args, ctx_rows=rows4)
    with pytest.raises(ops.ZLError):
        ops.kv_fork([(0, 1, 3, 0)], k_tab, v_tab, buf_lens, hkv, 126)        # row_bytes % 4
    with pytest.raises(ops.ZLError):
        ops.kv_fork([(0, 1, 3, 0)], *args, ctx_rows=rows4[:3])
    _check(bufs, d_bufs, ctx, d_ctx, guards, "refused before any launch")
    # the C entry itself: dst = b, rows = buf_lens[dst] + 1 and rows = max_rows + 1 change nothing, the good one beside them is carried out
    desc = [(0, 6, 1, 5), (3, 4, LENS[4] + 1, 5), (0, 1, 5, 3), (3, 5, max_rows + 1, 5)]
    assert max_rows >= LENS[4] + 1 and max_rows + 1 <= min(LENS[3], LENS[5])
    d_desc = torch.tensor(desc, dtype=I32, device=dev)
    p, i64 = (lambda t: C.c_void_p(t.data_ptr())), C.c_int64
    st = _lib.lib().zl_kv_fork(p(d_desc), i64(len(desc)), p(k_tab), p(v_tab), p(buf_lens), i64(LAYERS), i64(B), i64(max_rows), i64(hkv), i64(rb),
                               C.c_int(1), *(p(t) for t in rows4), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    assert fr.fork(desc, bufs, LENS, True, max_rows, ctx) == [(0, 1, 5, 3)]
    _check(bufs, d_bufs, ctx, d_ctx, guards, "dropped descriptors")


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
LEN_BUF, BIAS_LD, TOP, WIDE = tslots.LEN_BUF, tslots.BIAS_LD, tslots.TOP, tslots.WIDE
K = 2                                                                       # the drafter's drafts per step in these tests
case = tslots.case
_req, _snap, _rows_equal, _bits = tslots._req, tslots._snap, tslots._rows_equal, tslots._bits
SEED = 4100


def _step(model, ctx, samp, stop, look):
    """one step by the state's method -> (ids emitted per slot (B, width) int32 with -1 behind them, logits, log-probabilities)"""
    b = ctx.tokens.numel()
    if look is not None:
        res = model.step_lookup(ctx, look, sampler=samp, stop=stop)
        return res.tokens.clone(), res.logits.view(b, K + 1, -1).clone(), samp.row_logprobs.clone()
    logits, nxt = model.step_sample(ctx, samp, stop=stop)
    return nxt.to(I32).view(b, 1), logits.view(b, 1, -1).clone(), samp.logprobs.view(b, 1).clone()


def _fresh(c, b, lookup, grammars=(), **ctx_kw):
    """an empty batch as BatchServer builds it: every slot finished, full-width states -> (ctx, sampler, stop, lookup state or None)"""
    model = c.model
    ctx = model.new_context(b, LEN_BUF, 0, **ctx_kw)
    kw = dict(grammar_states=sum(g.states for g in grammars), grammar_edges=64) if grammars else {}
    samp = model.new_sampler(ctx, penalties=True, bias_ld=BIAS_LD, top_logprobs=TOP, **kw)
    for g in grammars:
        model.load_grammar(samp, g)
    stop = model.new_stopper(ctx, widths=WIDE)
    look = model.new_lookup(ctx, [[] for _ in range(b)], K) if lookup else None
    stop.finished.fill_(3)
    stop.live.zero_()
    return ctx, samp, stop, look


def _three(c, **kw):
    return [_req(c, 3, seed=SEED + j, max_new_tokens=40, **kw) for j in range(3)]     # 12 steps of up to K + 1 ids stay below it


def _same_kv(a, b, slots, rows, what):
    for s in slots:
        assert torch.equal(a.kv[s][:, :, :rows], b.kv[s][:, :, :rows]), (what, "K/V", s)
        if a.kv_quant:
            assert torch.equal(a.kv_scales[s][:, :, :rows].view(I32), b.kv_scales[s][:, :, :rows].view(I32)), (what, "scales", s)


def _twin_pair(c, lookup, prompt, admit_kw_a=None, admit_kw_b=None, **ctx_kw):
    """A: one group of three slots; B: the same requests by three single-slot calls -> (A, B), both checked after admission"""
    model, slots, reqs = c.model, [2, 0, 1], _three(c)
    p = torch.from_numpy(prompt)
    A, Bt = _fresh(c, 3, lookup, **ctx_kw), _fresh(c, 3, lookup, **ctx_kw)
    ptrs = {k: v.data_ptr() for o in A[:3] for k, v in vars(o).items() if torch.is_tensor(v)}
    out_a = model.admit_samples(A[0], [(slots, p, reqs)], A[1], A[2], A[3], **(admit_kw_a or {}))
    outs_b = [model.admit_samples(Bt[0], [([s], p, [rq])], Bt[1], Bt[2], Bt[3], **(admit_kw_b or {})) for s, rq in zip(slots, reqs)]
    la, lb = (out_a[0], outs_b[0][0]) if admit_kw_a and "cache" in admit_kw_a else (out_a, outs_b[0])
    assert la.shape == (1, c.vocab) and torch.equal(la, lb)
    assert ptrs == {k: v.data_ptr() for o in A[:3] for k, v in vars(o).items() if torch.is_tensor(v)}
    n = len(prompt) - 1
    _same_kv(A[0], Bt[0], slots, n, "twin")
    for s in slots[1:]:                                                     # A's other slots hold copies of its source's rows
        assert torch.equal(A[0].kv[s][:, :, :n], A[0].kv[slots[0]][:, :, :n]), s
    _rows_equal(_snap(*A), _snap(*Bt), slots, "twin")
    assert A[0].tokens.tolist() == [int(prompt[-1])] * 3 and A[0].positions.tolist() == [n] * 3 and A[0].valid_lens.tolist() == [n + 1] * 3
    assert A[1].seeds.tolist() == [SEED + 1, SEED + 2, SEED] and A[2].live.item() == Bt[2].live.item() == 3
    return A, Bt, (out_a, outs_b)


def _same_steps(c, A, Bt, steps, what):
    """tokens and log-probabilities of every slot, bit for bit (a row's log-probabilities: those of the ids it emitted)"""
    for i in range(steps):
        ta, _, pa = _step(c.model, *A)
        tb, _, pb = _step(c.model, *Bt)
        assert torch.equal(ta, tb), (what, i)
        for s, row in enumerate(ta.tolist()):
            m = len(sr.emitted(row))
            assert torch.equal(pa[s, :m].view(I32), pb[s, :m].view(I32)), (what, i, s)


def test_a_group_of_three_is_three_single_admissions_step_sample(case):
    c = case
    A, Bt, _ = _twin_pair(c, False, c.prompts[3])
    ta, _, _ = _step(c.model, *A)
    tb, _, _ = _step(c.model, *Bt)
    assert torch.equal(ta, tb)
    # the first step drew under each slot's own seed at counter 0: the first tokens are samples, not the prompt's greedy pick
    want = sref.uniforms([SEED + 1, SEED + 2, SEED], [0, 0, 0])
    assert np.array_equal(A[1].u.cpu().numpy().view(np.int32), want.view(np.int32)) and A[1].draws.tolist() == [1, 1, 1]
    assert A[2].gen_lens.tolist() == [1, 1, 1]
    _same_steps(c, A, Bt, 11, "step_sample")
    assert A[2].gen_lens.tolist() == [12] * 3 and len({tuple(r) for r in A[2].tail.tolist()}) > 1       # the samples went apart


def test_a_group_of_three_is_three_single_admissions_step_lookup(case):
    c = case
    prompt = np.tile(c.prompts[3][:8], 3)                                   # a repeating prompt: the drafter finds matches
    A, Bt, _ = _twin_pair(c, True, prompt)
    assert A[3].hist_lens.tolist() == [len(prompt)] * 3                     # prompt[:-1] and the re-fed token
    _same_steps(c, A, Bt, 12, "step_lookup")
    assert A[2].finished.tolist() == [0, 0, 0] and min(A[2].gen_lens.tolist()) >= 12


def test_the_twin_on_an_int8_cache_copies_codes_and_scales(case):
    c = case
    A, Bt, _ = _twin_pair(c, False, c.prompts[3], kv_cache_dtype="int8")
    assert A[0].kv_quant and float(A[0].kv_scales[0][:, :, :22].abs().sum()) > 0
    _same_steps(c, A, Bt, 12, "int8")


def test_the_twin_through_a_prefix_cache_with_the_second_admission_a_hit(case):
    c, model = case, case.model
    prompt = c.prompts[3]
    p = torch.from_numpy(prompt)
    scratch = _fresh(c, 3, False)
    cache = model.new_prefix_cache(scratch[0], 8, block_size=16)
    _, matched = model.admit_samples(scratch[0], [([1, 2], p, _three(c)[:2])], scratch[1], scratch[2], cache=cache)
    assert matched == [0] and len(cache.index) == 1                          # 22 rows encoded: one full block saved
    A, Bt, (out_a, outs_b) = _twin_pair(c, False, prompt, dict(cache=cache), dict(cache=cache))
    assert out_a[1] == [16] and [o[1] for o in outs_b] == [[16]] * 3         # every encode is the same hit: 6 rows behind 16 loaded ones
    _same_kv(A[0], scratch[0], [2], 16, "the loaded block")
    _same_steps(c, A, Bt, 12, "prefix cache")


def test_a_running_slot_keeps_its_stream_across_a_forked_admission(case):
    c, model = case, case.model
    runs = []
    for forked in (True, False):
        st = _fresh(c, 4, False)
        model.admit_samples(st[0], [([0], torch.from_numpy(c.prompts[2]), [_req(c, 2, max_new_tokens=20)])], st[1], st[2])
        rec = [_step(model, *st) for _ in range(3)]
        if forked:
            before = _snap(*st)
            model.admit_samples(st[0], [([3, 1, 2], torch.from_numpy(c.prompts[3]), _three(c))], st[1], st[2])
            after = _snap(*st)
            _rows_equal(after, before, [0], "the running slot")
            assert torch.equal(after["kv.0"], before["kv.0"])
        rec += [_step(model, *st) for _ in range(6)]
        runs.append([(t[0].clone(), l[0].clone(), p[0].clone()) for t, l, p in rec])
    for i, ((t, l, p), (tt, ll, pp)) in enumerate(zip(*runs)):
        assert torch.equal(t, tt) and torch.equal(l, ll) and torch.equal(p.view(I32), pp.view(I32)), i


def _scripted(c, captured):
    """a single-slot admission, steps, a forked admission of two more slots, steps; captured: every step behind the first replays ONE graph"""
    model = c.model
    ctx, samp, stop, _ = _fresh(c, 3, False)
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
    model.admit_samples(ctx, [([2, 0], torch.from_numpy(c.prompts[3]), _three(c)[:2])], samp, stop)
    steps(6)
    assert stop.finished.tolist() == [0, 0, 0] and stop.gen_lens.tolist() == [6, 9, 6]
    return rec


def test_one_captured_graph_replays_across_a_forked_admission(case):
    eager, replayed = _scripted(case, False), _scripted(case, True)
    assert len(eager) == len(replayed) == 9
    for s, (a, b) in enumerate(zip(eager, replayed)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(_bits(x), _bits(y)), (s, i)


# ---- BatchServer ----------------------------------------------------------------------------------------------------------------------------
def _twin_run(c, calls, grammars=()):
    """the admission calls `calls` -- ("admit", slots, prompts, requests) or ("samples", groups) -- into a fresh batch of four, stepped
    until every slot has finished -> {slot: (pending token after admission, ids, log-probabilities, reason)}"""
    model = c.model
    ctx, samp, stop, _ = _fresh(c, 4, False, grammars)
    for kind, *args in calls:
        if kind == "admit":
            model.admit(ctx, *args, samp, stop)
        else:
            model.admit_samples(ctx, *args, samp, stop)
    first = ctx.tokens.tolist()
    ids, lps = [[] for _ in range(4)], [[] for _ in range(4)]
    for _ in range(LEN_BUF):
        if stop.live.item() == 0:
            break
        tok, _, lp = _step(model, ctx, samp, stop, None)
        tok, lp = tok.tolist(), lp.tolist()
        for s in range(4):
            m = len(sr.emitted(tok[s]))
            ids[s] += tok[s][:m]
            lps[s] += lp[s][:m]
    fin = stop.finished.tolist()
    return {s: (first[s], ids[s], lps[s], fin[s]) for s in range(4)}


def _lp_bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def test_batch_server_n_best_of_and_sample_first(case):
    """Every sample against its sequential-admission twin: the sample admitted on its own, with no fork, by a call whose prompt encode
    has the shape of the server's (round 1: one prompt; round 2: the prompts of requests 2 and 3 in one call)"""
    from zhilight_amd.grammar import from_choices
    from zhilight_amd.serving import BatchServer
    c = case
    eos = c.vocab - 1
    choices = [[5, 6, 7], [8, 9]]
    grammar = from_choices(c.vocab, choices, eos)
    srv = BatchServer(c.model, 4, LEN_BUF, bias_ld=BIAS_LD, top_logprobs=TOP, poll=4, grammar_states=grammar.states, grammar_edges=64)
    h = srv.load_grammar(grammar)
    p = [torch.from_numpy(c.prompts[i]) for i in (0, 1, 2, 4)]
    r0, r1 = _req(c, 0, max_new_tokens=3), _req(c, 1, max_new_tokens=6)
    r2 = dict(temperature=1.0, seed=900, stop_ids=[eos], max_new_tokens=8, grammar=h)
    r3 = _req(c, 4, max_new_tokens=5)
    assert [srv.submit(p[0], **r0), srv.submit(p[1], n=3, **r1), srv.submit(p[2], n=2, best_of=3, **r2),
            srv.submit(p[3], sample_first=True, **r3)] == [0, 1, 2, 3]
    res = srv.run()
    # FIFO, all-or-nothing: slot 0 is free after the first four steps, but request 2 waits for three slots and request 3 does not overtake
    # it; after eight steps the three samples of request 1 have finished and both are admitted
    assert srv.log == [(1, [(0, 0), (1, 1), (2, 1), (3, 1)]), (2, [(0, 2), (1, 2), (2, 2), (3, 3)])]
    assert srv.stats["forks"] == 2 + 2 and srv.stats["admissions"] == 2 and not srv.queue and not srv.active
    assert res[0]["round"] == 1 and len(res[0]["tokens"]) == 3 and srv.stats["steps"] >= 12
    seeded = lambda rq, j: dict(rq, seed=rq["seed"] + j)                                                     # noqa: E731
    # the plain request is what it always was
    first, ids, lps, fin = _twin_run(c, [("admit", [0], [p[0]], [r0])])[0]
    assert (res[0]["first_token"], res[0]["tokens"], res[0]["reason"]) == (first, ids, fin) and "samples" not in res[0]
    assert np.array_equal(_lp_bits(res[0]["logprobs"]), _lp_bits(lps))
    # n = 3: the samples in sample order, each the stream of its own single admission
    twin = _twin_run(c, [("samples", [([s], p[1], [seeded(r1, j)])]) for j, s in enumerate((1, 2, 3))])
    assert res[1]["round"] == 1 and len(res[1]["samples"]) == 3
    for j, sm in enumerate(res[1]["samples"]):
        _, ids, lps, fin = twin[1 + j]
        assert (sm["first_token"], sm["tokens"], sm["reason"], sm["seed"]) == (None, ids, fin, r1["seed"] + j) and len(ids) == 6, j
        assert np.array_equal(_lp_bits(sm["logprobs"]), _lp_bits(lps)) and sm["cum_logprob"] == float(sum(lps)), j
        assert len(sm["top_ids"]) == 6 and sm["clamped"] == 6, j
    assert len({tuple(sm["tokens"]) for sm in res[1]["samples"]}) > 1
    # best_of = 3, n = 2 under a grammar of two choices, admitted together with the sample_first request
    twins = [_twin_run(c, [("samples", [([j], p[2], [seeded(r2, j)]), ([3], p[3], [r3])])], grammars=(grammar,)) for j in range(3)]
    streams = [twins[j][j] for j in range(3)]
    for _, ids, _, fin in streams:                                          # a listed choice, the first token included, then EOS
        assert ids[-1] == eos and ids[:-1] in choices and fin == 1
    order = sorted(range(3), key=lambda j: (-float(sum(streams[j][2])), j))[:2]
    assert res[2]["round"] == 2 and [sm["seed"] for sm in res[2]["samples"]] == [900 + j for j in order]
    for sm, j in zip(res[2]["samples"], order):
        assert (sm["first_token"], sm["tokens"], sm["reason"]) == (None, streams[j][1], 1), j
        assert np.array_equal(_lp_bits(sm["logprobs"]), _lp_bits(streams[j][2])) and sm["cum_logprob"] == float(sum(streams[j][2])), j
    assert res[2]["samples"][0]["cum_logprob"] >= res[2]["samples"][1]["cum_logprob"]
    # sample_first: the plain shape with no first token
    _, ids, lps, fin = twins[0][3]
    assert (res[3]["first_token"], res[3]["tokens"], res[3]["reason"], res[3]["round"]) == (None, ids, fin, 2) and len(ids) == 5
    assert np.array_equal(_lp_bits(res[3]["logprobs"]), _lp_bits(lps)) and "samples" not in res[3]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_admit_samples_refusals_come_before_any_launch(case):
    from zhilight_amd import ops
    c, model = case, case.model
    ctx, samp, stop, look = _fresh(c, 3, True)
    model.admit_samples(ctx, [([0], torch.from_numpy(c.prompts[2]), [_req(c, 2)])], samp, stop, look)
    narrow = model.new_sampler(ctx, temperature=0.5)                        # no bitmap, no bias rows
    q8 = model.new_context(3, LEN_BUF, 0, kv_cache_dtype="int8")
    before = _snap(ctx, samp, stop, look)
    left, guard, room = ctx.steps_left, dict(ctx.slot_guard), dict(ctx.slot_room)
    p = torch.from_numpy(c.prompts[3])
    long = torch.from_numpy(np.resize(c.prompts[5], LEN_BUF - K))           # len - 1 rows fit the buffer, no room behind K draft rows
    go = lambda groups, s=samp, st=stop, lk=look, cx=ctx, **kw: model.admit_samples(cx, groups, s, st, lk, **kw)      # noqa: E731
    cases = [
        ("distinct indices", lambda: go([([1, 2], p, [{}, {}]), ([2], p, [{}])])),
        ("distinct indices", lambda: go([([1, 1], p, [{}, {}])])),
        ("distinct indices", lambda: go([([1, 3], p, [{}, {}])])),
        ("one request per slot", lambda: go([([1, 2], p, [{}])])),
        ("one request per slot", lambda: go([([], p, [])])),
        ("a group is", lambda: go([([1], p)])),
        ("one group at least", lambda: go([])),
        ("2 tokens at least", lambda: go([([1], p[:1], [{}])])),
        ("does not fit", lambda: go([([1], torch.zeros(LEN_BUF + 1, dtype=I32), [{}])])),
        ("leaves no room for one generated token", lambda: go([([1], long, [{}])])),
        ("no bitmap", lambda: go([([1, 2], p, [{}, dict(repetition_penalty=1.2)])], s=narrow)),
        ("5 bias ids", lambda: go([([1], p, [dict(logit_bias={i: 1.0 for i in range(5)})])])),
        ("temperature >= 0", lambda: go([([1, 2], p, [{}, dict(temperature=-1)])])),
        ("max_new_tokens is an integer >= 0", lambda: go([([1], p, [dict(max_new_tokens=-1)])])),
        ("no stop state", lambda: go([([1], p, [dict(max_new_tokens=3)])], st=None)),
        ("grammar names no loaded automaton", lambda: go([([1], p, [dict(grammar=0)])])),
        ("not on the INT8 KV cache", lambda: go([([1], p, [{}])], cx=q8)),
        ("kv_history", lambda: go([([1], p, [{}])], kv_history="x")),
        ("another batch size", lambda: go([([1], p, [{}])], cx=model.new_context(2, LEN_BUF, 0))),
    ]
    for match, call in cases:
        with pytest.raises(ops.ZLError, match=match):
            call()
    tp, model.tp = model.tp, object()
    try:
        with pytest.raises(ops.ZLError, match="tensor parallelism"):
            go([([1], p, [{}])])
    finally:
        model.tp = tp
    after = _snap(ctx, samp, stop, look)
    for k in before:                                                        # nothing ran: every tensor as before
        assert torch.equal(_bits(before[k]), _bits(after[k])), k
    assert (ctx.steps_left, ctx.slot_guard, ctx.slot_room) == (left, guard, room)
    go([([2, 1], p, [_req(c, 3), _req(c, 4)])])                              # and the accepted call
    torch.cuda.synchronize()
