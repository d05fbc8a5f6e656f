"""The speculative sampling step on the GPU: zl_spec_sample_accept's picks, log-probabilities and uniforms against ops.sample_advance on
the same rows bit for bit, its acceptance and bookkeeping against tests/spec_ref.py, the generator's counter discipline, the sequence
property (a speculative run emits the plain sampling run's tokens whatever the drafter proposes) on the toy model of
test_spec_sample_host.py, the distribution of 4 096 tasks in one launch, determinism under repetition and graph replay, and
LLaMA.verify / step_lookup / generate_lookup with sampler= on the small GPTQ model of test_gpu_spec_verify.py.
Every buffer has a poisoned guard region behind it; a padded logit row is padded with NaNs."""
import ctypes as C

import numpy as np
import pytest
import torch

import sample_ref
import spec_ref
import spec_sample_ref as ssr
import test_gpu_sample as gs
import test_gpu_spec_verify as sv
import test_spec_sample_host as host
from test_gpu_prefill_batch import _gptq_model
from test_score_host import bound

pytestmark = pytest.mark.gpu

NS = [1, 2, 65, 257, 4097, 128256]
BS, LEN_QS = [1, 3, 8], [2, 4, 8, 32]
_np, _guarded, POISON = gs._np, gs._guarded, gs.POISON
I32, I64, F32 = torch.int32, torch.int64, torch.float32
STATE0 = (3, 10, 20, 30)


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _SpecCall:
    """one ops.spec_sample_accept call on guarded buffers; per-task parameters and state, per-row u / u_out / out_tokens / out_logprobs"""

    def __init__(self, logits, drafts, T, k, p, dev, u=None, seeds=None, draws=None, want=("tokens", "positions", "placement", "valid_lens",
                 "accepted", "out_tokens", "out_logprobs", "logprobs", "u_out")):
        b, len_q = drafts.shape[0], drafts.shape[1] + 1
        self.b, self.len_q, self.logits = b, len_q, logits
        self.bufs = dict(drafts=_guarded(b * (len_q - 1), I32, dev, np.asarray(drafts).reshape(-1)),
                         temperature=_guarded(b, F32, dev, T), top_k=_guarded(b, I32, dev, k), top_p=_guarded(b, F32, dev, p))
        if u is not None:
            self.bufs["u"] = _guarded(b * len_q, F32, dev, np.asarray(u).reshape(-1))
        if seeds is not None:
            self.bufs["seeds"], self.bufs["draws"] = _guarded(b, I64, dev, seeds), _guarded(b, I64, dev, draws)
        for name, v in zip(("tokens", "positions", "placement", "valid_lens"), STATE0):
            if name in want:
                self.bufs[name] = _guarded(b, I32, dev, np.full(b, v) + np.arange(b))
        for name, dt, count in (("accepted", I32, b), ("out_tokens", I32, b * len_q), ("out_logprobs", F32, b * len_q), ("logprobs", F32, b),
                                ("u_out", F32, b * len_q)):
            if name in want:
                self.bufs[name] = _guarded(count, dt, dev)
        self.kw = {name: t for name, (t, _) in self.bufs.items() if name != "drafts"}

    def set_drafts(self, drafts):
        self.bufs["drafts"][0].copy_(torch.from_numpy(np.asarray(drafts, np.int32).reshape(-1)))

    def reset_state(self):
        for name, v in zip(("tokens", "positions", "placement", "valid_lens"), STATE0):
            if name in self.bufs:
                self.bufs[name][0].copy_(torch.as_tensor(np.full(self.b, v) + np.arange(self.b), dtype=I32))

    def state0(self):
        return tuple(np.full(self.b, v, np.int32) + np.arange(self.b, dtype=np.int32) for v in STATE0)

    def run(self):
        from zhilight_amd import ops
        return ops.spec_sample_accept(self.logits, self.bufs["drafts"][0].view(self.b, self.len_q - 1), **self.kw)

    def out(self, name):
        a = _np(self.bufs[name][0]).copy()
        return a.reshape(self.b, self.len_q) if name in ("out_tokens", "out_logprobs", "u_out") else a

    def intact(self):
        gs._intact([gd for _, gd in self.bufs.values()])


def _wrong(rng, pick, n):
    """a draft that is not `pick`: the drafter's -1, an id past the vocabulary, or another class"""
    return (-1, n, (int(pick) + 1) % n if n > 1 else n + 3)[int(rng.integers(0, 3))]


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("n", NS)
def test_picks_are_sample_advance_s(dev, n, bf16):
    """given u.  ops.sample_advance on the same rows, the tasks' parameters expanded per row, is the yardstick: the picks, their
    log-probabilities and the uniforms EQUAL its results bit for bit; accepted, the padded tokens and the state equal spec_ref on those
    picks.  Drafts are cut from the picks so that every acceptance length 0 .. K occurs at every (b, len_q), the wrong draft at the cut
    being a -1, an id >= n or another class, and the drafts BEHIND the cut right again (a match there must not count)"""
    rng = np.random.default_rng(11 * n + bf16)
    nan = 0x7FC0 if bf16 else 0x7E00
    seen = set()
    for b in BS:
        for len_q in LEN_QS:
            rows = b * len_q
            if n == 128256 and rows > 32:
                continue
            bits = gs._make_rows(rng, rows, n, bf16, shift=b + len_q)
            if n >= 65:
                bits[rows - 1, n // 2] = nan                                                # a row without a distribution: the arg-max, a NaN log-probability
            for ld in (n, n + 3):
                flat, logits = gs._logits_dev(bits, ld, bf16, dev)
                before = flat.clone()
                T, k, p, _ = gs._params(rng, b, n)
                u = gs._params(rng, rows, n)[3]
                yard = gs._Call(logits, np.repeat(T, len_q), np.repeat(k, len_q), np.repeat(p, len_q), dev, u=u, want=("tokens", "logprobs", "u_out"))
                yard.run()
                picks, lp = yard.out("tokens").reshape(b, len_q), yard.out("logprobs").reshape(b, len_q)
                assert np.array_equal(yard.out("u_out"), u) and ((picks >= 0) & (picks < n)).all()
                # every draft right: nothing is padded, the rows are the yardstick's
                call = _SpecCall(logits, picks[:, :-1], T, k, p, dev, u=u)
                acc, out = call.run()
                assert acc.data_ptr() == call.bufs["accepted"][0].data_ptr() and out.shape == (b, len_q)
                assert np.array_equal(call.out("out_tokens"), picks) and (call.out("accepted") == len_q - 1).all()
                assert np.array_equal(_bits32(call.out("out_logprobs")), _bits32(lp))
                assert np.array_equal(_bits32(call.out("u_out")), _bits32(u.reshape(b, len_q)))
                assert np.array_equal(_bits32(call.out("logprobs")), _bits32(lp[:, -1]))
                # every acceptance length
                for c in range(-(-len_q // b)):
                    cuts = (c * b + np.arange(b)) % len_q
                    drafts = picks[:, :-1].copy()
                    for t in range(b):
                        if cuts[t] < len_q - 1:
                            drafts[t, cuts[t]] = _wrong(rng, picks[t, cuts[t]], n)
                    call.set_drafts(drafts)
                    call.reset_state()
                    for name in ("accepted", "out_tokens", "out_logprobs", "logprobs", "u_out"):
                        call.bufs[name][0].fill_(POISON[call.bufs[name][0].dtype])
                    call.run()
                    e_acc, e_out = spec_ref.accept(picks, drafts)
                    assert np.array_equal(e_acc, cuts)
                    seen.update((b, len_q, int(a)) for a in e_acc)
                    assert np.array_equal(call.out("accepted"), e_acc) and np.array_equal(call.out("out_tokens"), e_out)
                    for name, ref in zip(("tokens", "positions", "placement", "valid_lens"), spec_ref.advance(e_acc, e_out, *call.state0())):
                        assert np.array_equal(call.out(name), ref), name
                    emitted = np.arange(len_q)[None, :] <= e_acc[:, None]
                    got_lp = call.out("out_logprobs")
                    assert np.array_equal(_bits32(got_lp)[emitted], _bits32(lp)[emitted]) and np.isnan(got_lp[~emitted]).all()
                    assert np.array_equal(_bits32(call.out("logprobs")), _bits32(lp[np.arange(b), e_acc]))
                    assert np.array_equal(_bits32(call.out("u_out")), _bits32(u.reshape(b, len_q)))       # the rows behind the rejection too
                call.intact()
                yard.intact()
                assert torch.equal(flat.view(torch.int16), before.view(torch.int16))               # the logits are unmodified
    assert all((b, len_q, a) in seen for b in BS for len_q in LEN_QS for a in range(len_q) if n < 128256 or b * len_q <= 32)


def test_generator(dev):
    """row (t, i) draws at counter draws[t] + i under the task's key -- across the counter's 32-bit carry too; the step consumes
    accepted + 1 draws; given u the generator is untouched; at temperature 0 the call IS ops.spec_accept and still counts its draws"""
    from zhilight_amd import ops
    rng = np.random.default_rng(22)
    b, len_q, n = 8, 4, 257
    bits = gs._make_rows(rng, b * len_q, n, True)
    _, logits = gs._logits_dev(bits, n + 3, True, dev)
    T, k, p = np.full(b, 1.0, np.float32), np.zeros(b, np.int32), np.ones(b, np.float32)
    seeds = np.array([0, 1, -1, 2 ** 40 + 3, -2 ** 63, 2 ** 63 - 1, 12345, 7], np.int64)
    start = np.array([0, 0, 2 ** 32 - 2, 2 ** 32 - 1, 9, 2 ** 40, 0, 1], np.int64)
    x = np.stack([sample_ref.values_of(r, True) for r in bits])
    draws = start.copy()
    call = _SpecCall(logits, np.zeros((b, len_q - 1), np.int32), T, k, p, dev, seeds=seeds, draws=start)
    for step in range(4):
        u = ssr.row_uniforms(seeds, draws, len_q)
        picks = np.array([[sample_ref.sample(x[t * len_q + i], 1.0, 0, 1.0, u[t, i])[0] for i in range(len_q)] for t in range(b)])
        drafts = picks[:, :-1].copy()
        for t in range(b):
            cut = (t + step) % len_q
            if cut < len_q - 1:
                drafts[t, cut] = _wrong(rng, picks[t, cut], n)
        call.set_drafts(drafts)
        call.run()
        ref = ssr.spec_sample(x, drafts, T, k, p, seeds=seeds, draws=draws)
        assert np.array_equal(_bits32(call.out("u_out")), _bits32(u)), step
        assert np.array_equal(call.out("accepted"), ref["accepted"]) and np.array_equal(call.out("out_tokens"), ref["out_tokens"])
        assert sorted(set(ref["accepted"].tolist())) == list(range(len_q))
        draws = draws + ref["accepted"] + 1
        assert np.array_equal(call.out("draws"), draws) and np.array_equal(draws, ref["draws"])
    assert np.array_equal(call.out("seeds"), seeds)
    call.intact()
    # a caller's uniforms: used as given, seeds and draws present and untouched
    u = rng.random((b, len_q)).astype(np.float32)
    given = _SpecCall(logits, np.zeros((b, len_q - 1), np.int32), T, k, p, dev, u=u, seeds=seeds, draws=start)
    given.run()
    assert np.array_equal(given.out("draws"), start) and np.array_equal(_bits32(given.out("u_out")), _bits32(u))
    given.intact()
    # temperature 0: ops.spec_accept on the same logits, exactly; the draws still advance
    am = spec_ref.argmax_rows(x).reshape(b, len_q)
    drafts = am[:, :-1].copy()
    for t in range(b):
        if t % len_q < len_q - 1:
            drafts[t, t % len_q] = _wrong(rng, am[t, t % len_q], n)
    zero = _SpecCall(logits, drafts, np.zeros(b, np.float32), np.full(b, 5, np.int32), np.full(b, 0.5, np.float32), dev, seeds=seeds, draws=start)
    zero.run()
    greedy = {m: _guarded(c, I32, dev, v) for m, c, v in (("tokens", b, STATE0[0] + np.arange(b)), ("positions", b, STATE0[1] + np.arange(b)),
              ("placement", b, STATE0[2] + np.arange(b)), ("valid_lens", b, STATE0[3] + np.arange(b)), ("accepted", b, None), ("out_tokens", b * len_q, None))}
    ops.spec_accept(logits, zero.bufs["drafts"][0].view(b, len_q - 1), **{m: t for m, (t, _) in greedy.items()})
    for m, (t, _) in greedy.items():
        assert np.array_equal(zero.out(m).reshape(-1), _np(t)), m
    assert np.array_equal(zero.out("draws"), start + zero.out("accepted") + 1) and len(set(zero.out("accepted").tolist())) == len_q
    zero.intact()


def test_sequence_property_on_the_device(dev):
    """test_spec_sample_host's toy model with ops.sample_advance as the plain loop and ops.spec_sample_accept as the speculative one:
    the emitted ids are identical under a drafter that is always wrong, always right, or random; the right one accepts K every step"""
    from zhilight_amd import ops
    table = torch.from_numpy(host.toy_table()).to(dev)
    tasks, K, tokens = host.TOY_TASKS, host.TOY_K, host.TOY_TOKENS
    dv = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)                           # noqa: E731
    T, k, p, seeds = dv(host.TOY_T, F32), dv(host.TOY_TOPK, I32), dv(host.TOY_TOPP, F32), dv(host.TOY_SEEDS, I64)
    draws, prev = torch.zeros(tasks, dtype=I64, device=dev), dv(host.TOY_FIRST, I32)
    plain = []
    for _ in range(tokens + K + 1):
        ops.sample_advance(table[prev.long()].contiguous(), T, k, p, seeds=seeds, draws=draws, tokens=prev)
        plain.append(_np(prev).copy())
    plain = np.stack(plain, axis=1).tolist()
    assert draws.tolist() == [tokens + K + 1] * tasks
    for name, drafter in host.toy_drafters(plain).items():
        draws.zero_()
        prev.copy_(dv(host.TOY_FIRST, I32))
        emitted, steps, full = [[] for _ in range(tasks)], 0, True
        while min(len(e) for e in emitted) < tokens:
            drafts = np.stack([drafter(t, min(len(emitted[t]), tokens)) for t in range(tasks)]).astype(np.int32)
            fed = torch.cat([prev.view(tasks, 1), dv(np.clip(drafts, 0, host.TOY_N - 1), I32)], dim=1)
            acc, out = ops.spec_sample_accept(table[fed.view(-1).long()].contiguous(), dv(drafts, I32), T, k, p, seeds=seeds, draws=draws, tokens=prev)
            acc, out = acc.tolist(), out.tolist()
            for t in range(tasks):
                full &= acc[t] == K or len(emitted[t]) >= tokens
                emitted[t] += out[t][:acc[t] + 1]
            assert draws.tolist() == [len(e) for e in emitted] and prev.tolist() == [e[-1] for e in emitted]
            steps += 1
        for t in range(tasks):
            assert emitted[t][:tokens] == plain[t][:tokens], (name, t)
        if name == "right":
            assert full and steps == tokens // (K + 1)
        if name == "wrong":
            assert steps == tokens


def test_distribution(dev):
    """4 096 tasks of len_q = 2 in ONE launch share one n = 257 row pair; T = 1, top_k = 8, top_p = 0.9, one seed per task; the draft is
    the second most probable class.  The picks equal the reference in its exact fixed-point form; the acceptance frequency is within
    5 sqrt(p (1 - p) / 4096) of p(draft) and every class of the first row within the same bound of its probability -- binomial bounds,
    which test_spec_sample_host.py shows the reference's own picks for these seeds to meet"""
    bits, draft, seeds, prob0 = ssr.distribution_case()
    b = ssr.DIST_B
    _, logits = gs._logits_dev(np.tile(bits, (b, 1)), ssr.DIST_N, False, dev)
    call = _SpecCall(logits, np.full((b, 1), draft, np.int32), np.full(b, ssr.DIST_T, np.float32), np.full(b, ssr.DIST_K, np.int32),
                     np.full(b, ssr.DIST_P, np.float32), dev, seeds=seeds, draws=np.zeros(b, np.int64))
    call.run()
    picks, accepted, u = ssr.distribution_reference(bits, draft, seeds)
    e_acc, e_out = spec_ref.accept(picks, np.full((b, 1), draft))
    assert np.array_equal(_bits32(call.out("u_out")), _bits32(u))
    got, acc = call.out("out_tokens"), call.out("accepted")
    print("tasks whose tokens differ from the fixed-point reference:", int((got != e_out).any(axis=1).sum()), "of", b)
    assert np.array_equal(got, e_out) and np.array_equal(acc, e_acc) and np.array_equal(call.out("draws"), e_acc.astype(np.int64) + 1)
    bnd = 5 * np.sqrt(prob0 * (1 - prob0) / b)
    freq = np.bincount(got[:, 0], minlength=ssr.DIST_N) / b
    print("p(draft)", float(prob0[draft]), "accepted", float(acc.mean()), "bound", float(bnd[draft]),
          "largest class deviation / its bound", float((np.abs(freq - prob0)[prob0 > 0] / bnd[prob0 > 0]).max()))
    assert abs(acc.mean() - prob0[draft]) <= bnd[draft]
    assert (np.abs(freq - prob0) <= bnd).all()
    call.intact()


def test_deterministic_under_repetition_and_replay(dev):
    """the same call three times, then captured and replayed twice, each from the restored draws and state: every output bit-identical"""
    rng = np.random.default_rng(13)
    for n, b, len_q in ((4097, 8, 4), (257, 3, 32)):
        bits = gs._make_rows(rng, b * len_q, n, False)
        _, logits = gs._logits_dev(bits, n, False, dev)
        T, k, p, _ = gs._params(rng, b, n)
        T[:] = np.where(T > 0, T, 1.0)
        seeds = rng.integers(-2 ** 62, 2 ** 62, b)
        probe = _SpecCall(logits, np.zeros((b, len_q - 1), np.int32), T, k, p, dev, seeds=seeds, draws=np.full(b, 5))
        probe.run()
        drafts = probe.out("out_tokens")[:, :-1].copy()                 # the first draft right, -1 behind it (or more picks: then more is accepted)
        call = _SpecCall(logits, drafts, T, k, p, dev, seeds=seeds, draws=np.full(b, 5))
        names = ("accepted", "out_tokens", "out_logprobs", "logprobs", "u_out", "draws", "tokens", "positions", "placement", "valid_lens")
        restore = {m: call.bufs[m][0].clone() for m in ("draws", "tokens", "positions", "placement", "valid_lens")}

        def again():
            for m, v in restore.items():
                call.bufs[m][0].copy_(v)
            call.run()

        runs = []
        for _ in range(3):
            again()
            runs.append([call.bufs[m][0].clone() for m in names])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            again()
        for _ in range(2):
            for m in names[:5]:
                call.bufs[m][0].fill_(POISON[call.bufs[m][0].dtype])
            graph.replay()
            torch.cuda.synchronize()
            runs.append([call.bufs[m][0].clone() for m in names])
        as_bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t               # noqa: E731
        for run in runs[1:]:
            for m, x, y in zip(names, runs[0], run):
                assert torch.equal(as_bits(x), as_bits(y)), m
        assert int(runs[0][0].min()) >= 1 and np.array_equal(_np(runs[0][5]), 5 + _np(runs[0][0]).astype(np.int64) + 1)
        assert np.array_equal(_bits32(_np(runs[0][4]).reshape(b, len_q)), _bits32(ssr.row_uniforms(seeds, np.full(b, 5), len_q)))
        call.intact()


# ---- the model ----------------------------------------------------------------------------------------------------------------------
LEN_BUF, K = sv.LEN_BUF, sv.K
MOTIF_LENS = [16, 40, 24]
KW = dict(temperature=0.8, top_k=20, top_p=0.95, seed=77)
LOOKUP = ("history", "hist_lens", "drafts", "match")


class _Case:
    pass


@pytest.fixture(scope="module")
def case(dev):
    c = _Case()
    rng, c.cfg, c.sd, c.model = _gptq_model(dev)
    c.vocab = c.cfg.vocab_size
    c.prompts = [rng.integers(0, c.vocab, s).astype(np.int32) for s in sv.LENS]
    c.motifs = [np.tile(rng.integers(0, c.vocab, 8), 5)[:s].astype(np.int32) for s in MOTIF_LENS]
    return c


def _start(c, b, prompts=None, **kw):
    prompts = (c.motifs if prompts is None else prompts)[:b]
    ctx = sv._fresh(c.model, prompts)
    return ctx, c.model.new_lookup(ctx, prompts, K), c.model.new_sampler(ctx, **(kw or KW))


def _check_step(c, res, samp, ctx, drafts, before, draws0, b):
    """one speculative sampling step against spec_sample_ref on the step's own returned logits -> the reference's results"""
    rows = _np(res.logits.float()).astype(np.float64)
    ref = ssr.spec_sample(rows, drafts, np.full(b, 0.8, np.float32), np.full(b, 20), np.full(b, 0.95, np.float32), seeds=77 + np.arange(b),
                          draws=draws0, state=before)
    assert np.array_equal(_np(res.accepted), ref["accepted"]) and np.array_equal(_np(res.tokens), ref["out_tokens"])
    assert np.array_equal(_np(samp.draws), ref["draws"])
    for name, want in zip(sv.STATE, ref["state"]):
        assert np.array_equal(_np(getattr(ctx, name)), want), name
    assert samp.row_u.shape == samp.row_logprobs.shape == (b, K + 1)
    assert np.array_equal(_bits32(_np(samp.row_u)), _bits32(ref["u"]))
    lp = _np(samp.row_logprobs)
    for t in range(b):
        a = int(ref["accepted"][t])
        assert np.isnan(lp[t, a + 1:]).all()
        for i in range(a + 1):
            bar = np.abs(rows[t * (K + 1) + i]).max() * 2.0 ** -10 + bound(c.vocab)                # test_gpu_sample.py's bar
            assert abs(float(lp[t, i]) - ref["out_logprobs"][t, i]) <= bar, (t, i)
    assert np.array_equal(_bits32(_np(samp.logprobs)), _bits32(lp[np.arange(b), ref["accepted"]]))
    return ref


@pytest.mark.parametrize("b", [1, 3])
def test_steps_follow_the_reference(case, dev, b):
    """four rounds of step_lookup(sampler=) on a repeating motif, then one verify(sampler=) whose drafts are all wrong: tokens, accepted,
    the row log-probabilities, state.logprobs, the draws and the context equal spec_sample_ref on the step's own returned logits"""
    c = case
    ctx, look, samp = _start(c, b)
    assert samp.row_logprobs is None and samp.row_u is None
    emitted = 0
    for _ in range(4):
        before, draws0, drafts, left = sv._state(ctx), _np(samp.draws).copy(), _np(look.drafts).copy(), ctx.steps_left
        res = c.model.step_lookup(ctx, look, sampler=samp)
        ref = _check_step(c, res, samp, ctx, drafts, before, draws0, b)
        emitted += int(ref["accepted"].sum()) + b
        assert ctx.steps_left == left - (K + 1)
    assert int(samp.draws.sum()) == emitted and np.array_equal(_np(look.hist_lens), np.array(MOTIF_LENS[:b]) + 1 + _np(samp.draws))
    # adversarial drafts: a twin of the whole state shows the first pick, the draft is anything else
    twin_ctx = sv._fresh(c.model, c.motifs[:b])
    for name in sv.STATE:
        getattr(twin_ctx, name).copy_(getattr(ctx, name))
    for dst, src in zip(twin_ctx.kv, ctx.kv):
        dst.copy_(src)
    twin = c.model.new_sampler(twin_ctx, **KW)
    twin.draws.copy_(samp.draws)
    first = _np(c.model.verify(twin_ctx, look.drafts, sampler=twin).tokens)[:, 0]
    drafts = np.stack([(first + 1 + i) % c.vocab for i in range(K)], axis=1).astype(np.int32)
    before, draws0 = sv._state(ctx), _np(samp.draws).copy()
    res = c.model.verify(ctx, torch.from_numpy(drafts).to(dev), sampler=samp)
    ref = _check_step(c, res, samp, ctx, drafts, before, draws0, b)
    assert ref["accepted"].tolist() == [0] * b and np.array_equal(_np(res.tokens)[:, 0], first) and np.array_equal(_np(samp.draws), draws0 + 1)


@pytest.mark.parametrize("b", [1, 3])
def test_temperature_zero_is_greedy_verify(case, dev, b):
    c = case
    ctx, twin = sv._fresh(c.model, c.prompts[:b]), sv._fresh(c.model, c.prompts[:b])
    samp = c.model.new_sampler(ctx, temperature=0.0, top_k=20, top_p=0.95, seed=1)
    g = np.stack([_np(c.model.step_greedy(sv._fresh(c.model, c.prompts[:b]))[1]).astype(np.int32)] * K, axis=1)
    drafts = torch.from_numpy(g).to(dev)                                # the first draft right, the rest whatever they turn out to be
    for step in range(2):
        got = c.model.verify(ctx, drafts, sampler=samp)
        got = [t.clone() for t in got]
        ref = c.model.verify(twin, drafts)
        for x, y in zip(got, ref):
            assert torch.equal(x, y), step
        for name in sv.STATE:
            assert torch.equal(getattr(ctx, name), getattr(twin, name)), (step, name)
        assert ctx.steps_left == twin.steps_left
        assert int(got[1].min()) >= 1 - step
        drafts = got[2][:, :K].contiguous()
    assert torch.equal(samp.draws, (ctx.positions - torch.tensor(sv.LENS[:b], device=dev)).long())      # one draw per emitted token, used or not


@pytest.mark.parametrize("b", [1, 3])
def test_capture_replay_and_no_host_synchronisation(case, dev, b):
    """captured after one eager call, four replays continue a twin's eager sequence; draws, context and drafter state agree; an eager
    step synchronises nowhere"""
    c = case
    ctx, look, samp = _start(c, b)
    eager = []
    for _ in range(5):
        res = c.model.step_lookup(ctx, look, sampler=samp)
        eager.append((res.accepted.clone(), res.tokens.clone(), samp.row_logprobs.clone(), samp.logprobs.clone()))
    tctx, tlook, tsamp = _start(c, b)
    res = c.model.step_lookup(tctx, tlook, sampler=tsamp)
    assert torch.equal(res.tokens, eager[0][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = c.model.step_lookup(tctx, tlook, sampler=tsamp)
    as_bits = lambda t: t.view(torch.int32)                                                       # noqa: E731
    for step in range(1, 5):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(r.accepted, eager[step][0]) and torch.equal(r.tokens, eager[step][1]), step
        assert torch.equal(as_bits(tsamp.row_logprobs), as_bits(eager[step][2])) and torch.equal(as_bits(tsamp.logprobs), as_bits(eager[step][3]))
    for name in sv.STATE:
        assert torch.equal(getattr(tctx, name), getattr(ctx, name)), name
    for name in LOOKUP:
        assert torch.equal(getattr(tlook, name), getattr(look, name)), name
    assert torch.equal(tsamp.draws, samp.draws)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = c.model.step_lookup(ctx, look, sampler=samp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(res.accepted.min()) >= 0


@pytest.mark.parametrize("b", [1, 3])
def test_generate_lookup_is_the_loop(case, b):
    c = case
    ctx, look, samp = _start(c, b)
    toks, stats = c.model.generate_lookup(ctx, look, 10, sampler=samp)
    tctx, tlook, tsamp = _start(c, b)
    out, lps, acc, steps = [[] for _ in range(b)], [[] for _ in range(b)], [0] * b, 0
    while min(len(o) for o in out) < 10:
        res = c.model.step_lookup(tctx, tlook, sampler=tsamp)
        a, t, lp = res.accepted.tolist(), res.tokens.tolist(), tsamp.row_logprobs.tolist()
        for j in range(b):
            out[j] += t[j][:a[j] + 1]
            lps[j] += lp[j][:a[j] + 1]
            acc[j] += a[j]
        steps += 1
    assert toks == [o[:10] for o in out] and stats["steps"] == steps and stats["accepted"] == acc and stats["emitted"] == [len(o) for o in out]
    assert stats["mean_accepted"] == sum(acc) / (steps * b)
    assert [len(l) for l in stats["logprobs"]] == [len(t) for t in toks] == [10] * b
    assert stats["logprobs"] == [l[:10] for l in lps] and all(np.isfinite(l).all() and (np.array(l) <= 0).all() for l in stats["logprobs"])
    assert torch.equal(samp.draws, tsamp.draws) and samp.draws.tolist() == stats["emitted"]
    for name in sv.STATE:
        assert torch.equal(getattr(ctx, name), getattr(tctx, name)), name
    # without a sampler the stats are what they were
    gctx = sv._fresh(c.model, c.motifs[:b])
    _, gstats = c.model.generate_lookup(gctx, c.model.new_lookup(gctx, c.motifs[:b], K), 6)
    assert sorted(gstats) == ["accepted", "emitted", "mean_accepted", "steps"]


def test_model_refusals(case, dev):
    from zhilight_amd import ops
    c, model = case, case.model
    ctx, look, samp = _start(c, 3)
    other = sv._fresh(model, c.motifs[:2])
    with pytest.raises(ops.ZLError, match="another batch size"):       # the sampler's own refusal
        model.verify(other, look.drafts[:2].contiguous(), sampler=samp)
    with pytest.raises(ops.ZLError, match="INT8 KV"):                  # verify's own, unchanged
        model.verify(model.new_context(3, LEN_BUF, 4, kv_cache_dtype="int8"), look.drafts, sampler=samp)
    with pytest.raises(ops.ZLError, match="INT8 KV"):
        model.step_lookup(model.new_context(3, LEN_BUF, 4, kv_cache_dtype="int8"), look, sampler=samp)
    short = model.new_context(3, LEN_BUF, LEN_BUF - K)                  # three slots left, four rows wanted
    before = [_np(getattr(look, n)).copy() for n in LOOKUP]
    with pytest.raises(ops.ZLError, match="do not fit the KV buffers"):
        model.step_lookup(short, look, sampler=samp)
    assert short.steps_left == K
    toks, stats = model.generate_lookup(short, look, 5, sampler=samp)   # the loop stops before a step that would be refused
    assert toks == [[], [], []] and stats["logprobs"] == [[], [], []] and stats["steps"] == 0
    # a refused call draws nothing and leaves the drafter alone
    assert samp.draws.tolist() == [0, 0, 0] and samp.row_logprobs is None
    for n, v in zip(LOOKUP, before):
        assert np.array_equal(_np(getattr(look, n)), v), n


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_errors(dev):
    """every ZL_EINVAL / ZL_ESHAPE / ZL_EDTYPE case of the header: ops refuses each in its own words before the call, and the C entry
    point returns the status it documents (every check precedes the first launch: nothing runs)"""
    from zhilight_amd import _lib, ops
    b, len_q, n = 2, 3, 65
    t = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=dev)                                # noqa: E731
    good = dict(logits=t(torch.float16, b * len_q, n), drafts=t(I32, b, len_q - 1), temperature=t(F32, b), top_k=t(I32, b), top_p=t(F32, b),
                seeds=t(I64, b), draws=t(I64, b))
    ops.spec_sample_accept(**good)                                      # the baseline is accepted
    bad = [
        ("tensors", dict(drafts=None)), ("tensors", dict(temperature=None)), ("tensors", dict(top_k=None)), ("tensors", dict(top_p=None)),
        ("tensors", dict(logits=None)),
        ("seeds and draws, or u", dict(seeds=None)), ("seeds and draws, or u", dict(draws=None)),
        ("fp16 or bf16", dict(logits=t(F32, b * len_q, n))),
        ("unit column stride", dict(logits=t(torch.float16, n, b * len_q).t())), ("unit column stride", dict(logits=t(torch.float16, b * len_q, 0))),
        ("K >= 1", dict(drafts=t(I32, b, 0))), ("K >= 1", dict(drafts=t(I64, b, len_q - 1))), ("K >= 1", dict(drafts=t(I32, b, 2 * (len_q - 1))[:, ::2])),
        ("32 rows per task", dict(drafts=t(I32, b, 32), logits=t(torch.float16, b * 33, n))),
        ("B \\* \\(K \\+ 1\\) rows", dict(logits=t(torch.float16, b * len_q + 1, n))),
        ("temperature", dict(temperature=t(F32, b * len_q))), ("top_k", dict(top_k=t(I64, b))), ("top_p", dict(top_p=t(F32, b + 1))),
        ("seeds", dict(seeds=t(I32, b))), ("draws", dict(draws=t(I64, b * len_q))),
        ("u: ", dict(u=t(F32, b))), ("u_out", dict(u_out=t(F32, b))), ("out_logprobs", dict(out_logprobs=t(F32, b))),
        ("out_tokens", dict(out_tokens=t(I32, b))), ("out_tokens", dict(out_tokens=t(I64, b, len_q))),
        ("accepted", dict(accepted=t(I32, b * len_q))), ("tokens", dict(tokens=t(I32, b * len_q))), ("positions", dict(positions=t(I64, b))),
        ("placement", dict(placement=t(I32, b + 1))), ("valid_lens", dict(valid_lens=t(F32, b))),
        ("logprobs", dict(logprobs=t(F32, b * len_q), out_logprobs=t(F32, b, len_q))),
        ("give both", dict(logprobs=t(F32, b))),
        ("device", dict(drafts=torch.zeros((b, len_q - 1), dtype=I32))), ("device", dict(logits=torch.zeros((b * len_q, n), dtype=torch.float16))),
    ]
    for match, change in bad:
        with pytest.raises(ops.ZLError, match=match):
            ops.spec_sample_accept(**{**good, **change})
    # the C entry point
    lib = _lib.lib()
    order = ("drafts", "temperature", "top_k", "top_p", "seeds", "draws", "u", "tokens", "positions", "placement", "valid_lens", "accepted",
             "out_tokens", "out_logprobs", "logprobs", "u_out")
    full = dict(good, u=None, tokens=t(I32, b), positions=t(I32, b), placement=t(I32, b), valid_lens=t(I32, b), accepted=t(I32, b),
                out_tokens=t(I32, b, len_q), out_logprobs=t(F32, b, len_q), logprobs=t(F32, b), u_out=t(F32, b, len_q))

    def status(dtype=2, bb=b, lq=len_q, nn=n, ld=n, **null):
        args = {**full, **null}
        ptr = lambda x: C.c_void_p(0 if x is None else x.data_ptr())                              # noqa: E731
        return lib.zl_spec_sample_accept(ptr(args["logits"]), C.c_int(dtype), *(C.c_int64(v) for v in (bb, lq, nn, ld)),
                                         *(ptr(args[m]) for m in order), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    EINVAL, ESHAPE, EDTYPE = -1, -2, -3
    assert status() == 0 and status(tokens=None, positions=None, placement=None, valid_lens=None, out_logprobs=None, logprobs=None, u_out=None) == 0
    for m in ("logits", "temperature", "top_k", "top_p", "drafts", "accepted", "out_tokens", "seeds", "draws"):
        assert status(**{m: None}) == EINVAL, m
    assert status(seeds=None, draws=None, u=t(F32, b, len_q)) == 0      # u in the generator's place
    assert status(out_logprobs=None) == EINVAL                          # logprobs is read from out_logprobs
    for kw in (dict(bb=0), dict(lq=1), dict(lq=33), dict(nn=0), dict(ld=n - 1), dict(nn=1 << 31, ld=1 << 31), dict(bb=1 << 30), dict(bb=1 << 31),
               dict(bb=1 << 62)):
        assert status(**kw) == ESHAPE, kw
    assert status(dtype=1) == EDTYPE and status(dtype=0) == EDTYPE and status(dtype=6) == 0
    assert status(dtype=1, drafts=None) == EINVAL and status(dtype=1, bb=0) == ESHAPE            # the order of the checks
    torch.cuda.synchronize()
