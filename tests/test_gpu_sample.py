"""The device sampler on the GPU: zl_sample_advance against the float64 rule of tests/sample_ref.py (mass tolerance and pick equality),
its determinism under repetition and graph replay, the Philox generator bit for bit, the bookkeeping against ops.argmax_advance, the
distribution of 8 192 draws, and LLaMA.new_sampler / step_sample / generate_sample on the small GPTQ model of test_gpu_prefill_batch.py.
Every buffer has a poisoned guard region behind it; a padded logit row is padded with NaNs."""
import numpy as np
import pytest
import torch

import sample_ref
import test_gpu_spec_verify as sv
from test_gpu_prefill_batch import _gptq_model
from test_score_host import bound

pytestmark = pytest.mark.gpu

NS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 65537, 128256]
ROWS = [1, 3, 8, 32]
GUARD = 64
LAST = float(np.float32(1 - 2.0 ** -24))
POISON = {torch.int32: -7, torch.int64: -7, torch.float32: -77.0}
TOL = 2.0 ** -15
_np = sv._np


def _guarded(n, dtype, dev, values=None):
    """a tensor of n elements at the start of a buffer with GUARD poisoned elements behind it -> (tensor, guard view)"""
    flat = torch.full((n + GUARD,), POISON[dtype], dtype=dtype, device=dev)
    if values is not None:
        flat[:n].copy_(torch.as_tensor(np.asarray(values), dtype=dtype))
    return flat[:n], flat[n:]


def _intact(guards):
    for g in guards:
        assert bool((g == POISON[g.dtype]).all())


def _logits_dev(bits, ld, bf16, dev):
    """(rows, n) uint16 patterns -> a (rows, n) view with row stride ld into a buffer whose padding and guard are NaNs"""
    rows, n = bits.shape
    buf = np.full(rows * ld + GUARD, 0x7E00 if not bf16 else 0x7FC0, np.uint16)
    buf[:rows * ld].reshape(rows, ld)[:, :n] = bits
    flat = torch.from_numpy(buf.view(np.int16)).to(dev).view(torch.bfloat16 if bf16 else torch.float16)
    return flat, flat[:rows * ld].view(rows, ld)[:, :n]


def _make_rows(rng, rows, n, bf16, shift=0):
    """rows of every kind, mixed within the batch: logit scales 0.05 / 0.5 / 2 / 8 (near-uniform to one-hot), four values only, and
    -inf over 90 % of the classes"""
    out = np.empty((rows, n), np.uint16)
    for r in range(rows):
        kind = (r + shift) % 6
        if kind == 4:
            x = rng.choice(np.array([-1.5, 0.0, 0.25, 2.0]), n)
        else:
            x = rng.standard_normal(n) * (0.05, 0.5, 2.0, 8.0, 0.0, 2.0)[kind]
        if kind == 5:
            x[rng.random(n) < 0.9] = -np.inf
            x[rng.integers(0, n)] = 0.5
        x = x.astype(np.float32)
        if bf16:
            u32 = x.view(np.uint32).astype(np.uint64)
            out[r] = ((u32 + 0x7FFF + ((u32 >> 16) & 1)) >> 16).astype(np.uint16)
        else:
            out[r] = x.astype(np.float16).view(np.uint16)
        zeros = (out[r] & 0x7FFF) == 0
        out[r, zeros] = rng.choice(np.array([0, 0x8000], np.uint16), int(zeros.sum()))      # both zeros, one value
    return out


def _params(rng, rows, n):
    T = rng.choice(np.array([0.3, 0.7, 1.0, 1.5], np.float32), rows)
    T[rng.random(rows) < 0.125] = rng.choice(np.array([0.0, -1.0], np.float32))
    k = rng.choice(np.array([0, 1, 2, 5, 40, n - 1, n + 7], np.int32), rows)
    p = rng.choice(np.array([0.0, 0.1, 0.5, 0.9, 1.0], np.float32), rows)
    u = rng.random(rows).astype(np.float32)
    pick = rng.integers(0, 3, rows)
    u[pick == 0], u[pick == 1] = 0.0, LAST
    return T, k, p, u


class _Call:
    """one ops.sample_advance call on guarded buffers; every result as numpy"""

    def __init__(self, logits, T, k, p, dev, u=None, seeds=None, draws=None, state=(3, 10, 20, 30), want=("tokens", "positions", "placement",
                 "valid_lens", "next_tokens", "logprobs", "u_out")):
        from zhilight_amd import ops
        rows = logits.shape[0]
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        g = lambda dt, v=None: _guarded(rows, dt, dev, v)
        self.bufs = dict(temperature=g(f32, T), top_k=g(i32, k), top_p=g(f32, p))
        if u is not None:
            self.bufs["u"] = g(f32, u)
        if seeds is not None:
            self.bufs["seeds"], self.bufs["draws"] = g(i64, seeds), g(i64, draws)
        for name, dt, v in (("tokens", i32, state[0]), ("positions", i32, state[1]), ("placement", i32, state[2]), ("valid_lens", i32, state[3]),
                            ("next_tokens", i64, None), ("logprobs", f32, None), ("u_out", f32, None)):
            if name in want:
                self.bufs[name] = g(dt, None if v is None else np.full(rows, v) + np.arange(rows))
        self.kw = {name: t for name, (t, _) in self.bufs.items()}
        self.logits = logits
        self.run = lambda: ops.sample_advance(self.logits, **self.kw)

    def out(self, name):
        return _np(self.bufs[name][0]).copy()

    def intact(self):
        _intact([gd for _, gd in self.bufs.values()])


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("n", NS)
def test_kernel_against_the_rule(dev, n, bf16):
    """given u.  (a) every pick lies where the float64 rule allows within a mass tolerance of 2^-15 Z: the fp32 exponent argument
    reaches ~88, 88 x 2^-24 relative per term, and the kernel's sums are exact integers (no reduction error at all) -- a bound, not a
    measurement; (b) the pick EQUALS the float64 pick in at least 98 % of the rows.  Rows that the rule sends to the arg-max (T <= 0,
    top_k = 1, top_p = 0, u = 0) equal torch.argmax exactly; the log-probabilities are within test_gpu_score.py's bar for an fp32
    log-sum-exp over stored logits.  (On an MI355X all 4 224 rows of the 26 cases equal the float64 pick; the smallest tolerance that
    would have passed (a), printed per case, is 0.)"""
    rng = np.random.default_rng(7 * n + bf16)
    eps_t = 2.0 ** -8 if bf16 else 2.0 ** -11
    cases = equal = 0
    worst = 0.0
    for rnd in range(2 if n <= 4097 else 1):
        for rows in ROWS:
            for ld in (n, n + 3):
                bits = _make_rows(rng, rows, n, bf16, shift=rnd + rows)
                flat, logits = _logits_dev(bits, ld, bf16, dev)
                before = flat.clone()
                T, k, p, u = _params(rng, rows, n)
                call = _Call(logits, T, k, p, dev, u=u)
                call.run()
                tok, nxt, lp = call.out("tokens"), call.out("next_tokens"), call.out("logprobs")
                call.intact()
                assert torch.equal(flat.view(torch.int16), before.view(torch.int16))               # the logits are unmodified
                assert np.array_equal(tok, nxt) and ((tok >= 0) & (tok < n)).all()
                assert np.array_equal(call.out("u_out"), u)
                am = torch.argmax(logits.float().cpu(), dim=1).numpy()
                for r in range(rows):
                    x = sample_ref.values_of(bits[r], bf16)
                    pick, pos, c, v, order = sample_ref.sample(x, T[r], int(k[r]), p[r], u[r])
                    info = (n, bf16, rows, ld, r, float(T[r]), int(k[r]), float(p[r]), float(u[r]), int(tok[r]), pick)
                    if not T[r] > 0 or k[r] == 1 or p[r] == 0 or u[r] == 0:
                        assert tok[r] == am[r] == pick, info
                    else:
                        assert x[tok[r]] > -np.inf, info
                        inv = np.empty(n, np.int64)
                        inv[order] = np.arange(n)
                        gpos = int(inv[tok[r]])
                        lo = c[gpos - 1] if gpos else 0.0
                        need = max(lo - v, v - c[gpos], 0.0) / c[-1]
                        worst = max(worst, need)
                        assert need <= TOL, info + (need,)
                    cases += 1
                    equal += int(tok[r]) == pick
                    fin = np.abs(x[np.isfinite(x)]).max()
                    assert abs(float(lp[r]) - sample_ref.logprob(x, T[r], int(tok[r]))) <= fin * 2 * eps_t + bound(n), info
    print(f"n = {n} {'bf16' if bf16 else 'f16'}: pick == float64 pick in {equal} of {cases} rows; smallest passing mass tolerance {worst:.3e}")
    assert equal >= 0.98 * cases


def test_nan_and_inf_rows_take_the_argmax(dev):
    """a row holding a NaN or +inf, and a row of -inf only: zl_argmax_advance's pick (the first NaN wins), in range, no endless loop"""
    from zhilight_amd import ops
    rng = np.random.default_rng(4)
    n = 1025
    for bf16 in (False, True):
        bits = _make_rows(rng, 6, n, bf16)
        nan, inf = (0x7E00, 0x7C00) if not bf16 else (0x7FC0, 0x7F80)
        bits[0, [700, 33]] = nan
        bits[1, [1000, 8]] = inf
        bits[2, :] = inf | 0x8000
        bits[3, 5], bits[3, 900] = inf, nan
        bits[4, 77] = nan | 0x8000                                                                 # a negative NaN is a NaN
        flat, logits = _logits_dev(bits, n + 3, bf16, dev)
        call = _Call(logits, np.full(6, 0.7, np.float32), np.full(6, 5, np.int32), np.full(6, 0.9, np.float32), dev, u=np.full(6, 0.6, np.float32))
        call.run()
        ref = torch.empty(6, dtype=torch.int32, device=dev)
        ops.argmax_advance(logits, tokens=ref)
        tok = call.out("tokens")
        assert tok[:5].tolist() == [33, 8, 0, 900, 77] and np.array_equal(tok[:5], _np(ref)[:5]) and 0 <= tok[5] < n
        assert np.isnan(call.out("logprobs")[:5]).all() and np.isfinite(call.out("logprobs")[5])
        call.intact()


def test_deterministic_under_repetition_and_replay(dev):
    """the same call three times, then captured and replayed twice: tokens, logprobs and u_out bit-identical"""
    rng = np.random.default_rng(12)
    for n, rows in ((128256, 8), (4097, 32)):
        bits = _make_rows(rng, rows, n, False)
        _, logits = _logits_dev(bits, n, False, dev)
        T, k, p, _ = _params(rng, rows, n)
        T[:] = np.where(T > 0, T, 1.0)
        seeds = rng.integers(-2 ** 62, 2 ** 62, rows)
        call = _Call(logits, T, k, p, dev, seeds=seeds, draws=np.full(rows, 5))
        draws, draws0 = call.bufs["draws"][0], call.bufs["draws"][0].clone()
        names = ("tokens", "next_tokens", "logprobs", "u_out")
        runs = []
        for _ in range(3):
            draws.copy_(draws0)
            call.run()
            runs.append([call.bufs[m][0].clone() for m in names])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            draws.copy_(draws0)
            call.run()
        for _ in range(2):
            for m in names:
                call.bufs[m][0].fill_(POISON[call.bufs[m][0].dtype])
            graph.replay()
            torch.cuda.synchronize()
            runs.append([call.bufs[m][0].clone() for m in names])
        for run in runs[1:]:
            for a, b in zip(runs[0], run):
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
        assert np.array_equal(_np(runs[0][3]), sample_ref.uniforms(seeds, np.full(rows, 5)))
        call.intact()


def test_generator(dev):
    rng = np.random.default_rng(21)
    rows, n = 8, 257
    bits = _make_rows(rng, rows, n, True)
    _, logits = _logits_dev(bits, n + 3, True, dev)
    T, k, p = np.full(rows, 1.0, np.float32), np.zeros(rows, np.int32), np.ones(rows, np.float32)
    seeds = np.array([0, 1, -1, 2 ** 40 + 3, -2 ** 63, 2 ** 63 - 1, 12345, 7], np.int64)
    start = np.array([0, 0, 2 ** 32 - 2, 2 ** 32 - 1, 9, 2 ** 40, 0, 1], np.int64)           # the counter's low word rolls into the high one
    call = _Call(logits, T, k, p, dev, seeds=seeds, draws=start)
    perm = np.array([1, 0, 2, 3, 4, 5, 7, 6])
    swapped = _Call(logits[torch.from_numpy(perm).to(dev)].contiguous(), T, k, p, dev, seeds=seeds[perm], draws=start[perm])
    for step in range(5):
        call.run()
        swapped.run()
        expect = sample_ref.uniforms(seeds, start + step)
        assert np.array_equal(call.out("u_out").view(np.uint32), expect.view(np.uint32)), step
        assert np.array_equal(call.out("draws"), start + step + 1)
        for r in range(rows):                                                                      # the picks follow these uniforms
            assert call.out("tokens")[r] == sample_ref.sample(sample_ref.values_of(bits[r], True), 1.0, 0, 1.0, expect[r])[0]
        # a task's stream follows its seed and draw count into another slot
        assert np.array_equal(swapped.out("u_out"), expect[perm]) and np.array_equal(swapped.out("tokens"), call.out("tokens")[perm])
    # a caller's uniforms: used as given, the generator untouched
    u = rng.random(rows).astype(np.float32)
    given = _Call(logits, T, k, p, dev, u=u, seeds=seeds, draws=start)
    given.run()
    assert np.array_equal(given.out("draws"), start) and np.array_equal(given.out("u_out"), u)
    for c in (call, swapped, given):
        c.intact()
    assert np.array_equal(call.out("seeds"), seeds)


def test_bookkeeping(dev):
    """tokens / positions / placement / valid_lens / next_tokens move exactly as ops.argmax_advance moves them; each optional pointer
    may be absent"""
    from zhilight_amd import ops
    rng = np.random.default_rng(8)
    rows, n = 8, 1023
    bits = _make_rows(rng, rows, n, False)
    flat, logits = _logits_dev(bits, n + 3, False, dev)
    before = flat.clone()
    zeros, ones, u = np.zeros(rows, np.float32), np.ones(rows, np.float32), rng.random(rows).astype(np.float32)
    greedy = _Call(logits, zeros, np.zeros(rows, np.int32), ones, dev, u=u)
    greedy.run()
    ref = {m: _guarded(rows, torch.int64 if m == "next_tokens" else torch.int32, dev, greedy_init)
           for m, greedy_init in (("tokens", 3 + np.arange(rows)), ("positions", 10 + np.arange(rows)), ("placement", 20 + np.arange(rows)),
                                  ("valid_lens", 30 + np.arange(rows)), ("next_tokens", None))}
    ops.argmax_advance(logits, **{m: t for m, (t, _) in ref.items()})
    for m, (t, _) in ref.items():
        assert np.array_equal(greedy.out(m), _np(t)), m
    greedy.intact()
    T, k, p = np.full(rows, 0.9, np.float32), np.full(rows, 40, np.int32), np.full(rows, 0.95, np.float32)
    full = _Call(logits, T, k, p, dev, u=u)
    full.run()
    assert np.array_equal(full.out("positions"), 11 + np.arange(rows)) and np.array_equal(full.out("placement"), 21 + np.arange(rows))
    assert np.array_equal(full.out("valid_lens"), 31 + np.arange(rows)) and np.array_equal(full.out("tokens"), full.out("next_tokens"))
    for want in (("tokens",), ("next_tokens",), ("tokens", "placement"), ("next_tokens", "positions", "u_out"), ("tokens", "valid_lens", "logprobs")):
        part = _Call(logits, T, k, p, dev, u=u, want=want)
        part.run()
        for m in want:
            assert np.array_equal(part.out(m), full.out(m)), (want, m)
        part.intact()
    full.intact()
    assert torch.equal(flat.view(torch.int16), before.view(torch.int16))


def test_distribution(dev):
    """a pick that is plausible but biased: one row of 64 logits over 32 rows, 256 calls with distinct seeds = 8 192 draws at T = 1,
    top_k = 8, top_p = 0.9.  Nothing outside the rule's support, every class within 5 standard deviations of its exact probability"""
    rng = np.random.default_rng(30)
    rows, n, calls = 32, 64, 256
    bits = np.repeat(_make_rows(rng, 3, n, False)[2:3], rows, axis=0)                             # the scale-2 row
    _, logits = _logits_dev(bits, n, False, dev)
    prob = sample_ref.probabilities(sample_ref.values_of(bits[0], False), 1.0, 8, 0.9)
    assert 2 <= (prob > 0).sum() <= 8
    call = _Call(logits, np.ones(rows, np.float32), np.full(rows, 8, np.int32), np.full(rows, 0.9, np.float32), dev,
                 seeds=np.zeros(rows), draws=np.zeros(rows), want=("tokens",))
    seeds, draws, toks = call.bufs["seeds"][0], call.bufs["draws"][0], []
    base = torch.arange(rows, dtype=torch.int64, device=dev)
    for i in range(calls):
        seeds.copy_(base + 1000 + rows * i)
        draws.zero_()
        call.run()
        toks.append(call.bufs["tokens"][0].clone())
    counts = np.bincount(_np(torch.cat(toks)), minlength=n)
    total = rows * calls
    assert counts[prob == 0].sum() == 0
    sd = np.sqrt(total * prob * (1 - prob))
    z = np.abs(counts - total * prob)[prob > 0] / sd[prob > 0]
    print("support", int((prob > 0).sum()), "largest deviation in standard deviations", float(z.max()))
    assert (z <= 5).all()
    call.intact()


def test_plain_entry_null_opts_and_zeroed_struct_are_one_call(dev):
    """zl_sample_advance, zl_sample_advance_ex with opts = NULL and with a zeroed zl_sample_opts_t give bit-equal tokens, logprobs
    and u_out on one greedy and two sampled rows under given uniforms; the speculative pair likewise in accepted, out_tokens and
    out_logprobs at B = 2, K = 2"""
    import ctypes as C
    from zhilight_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(41)
    n = 70
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                                        # noqa: E731
    dev_of = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                          # noqa: E731
    i32, f32 = torch.int32, torch.float32
    ways = (lambda f, f_ex, a: f(*a, stream), lambda f, f_ex, a: f_ex(*a, None, stream), lambda f, f_ex, a: f_ex(*a, C.byref(_lib.SampleOpts()), stream))

    rows = 3
    _, logits = _logits_dev(_make_rows(rng, rows, n, False), n, False, dev)
    T, k, pp = dev_of(np.array([0.0, 0.8, 1.3], np.float32)), dev_of(np.array([0, 5, 0], np.int32)), dev_of(np.array([1.0, 0.9, 0.7], np.float32))
    u = dev_of(np.array([0.3, 0.55, 0.9], np.float32))
    got = []
    for way in ways:
        tok, lp, u_out = torch.full((rows,), -7, dtype=i32, device=dev), torch.full((rows,), -77.0, device=dev), torch.full((rows,), -77.0, device=dev)
        args = [p(logits), 2, rows, n, n, p(T), p(k), p(pp), None, None, p(u), p(tok), None, None, None, None, p(lp), p(u_out)]
        assert way(lib.zl_sample_advance, lib.zl_sample_advance_ex, args) == 0
        torch.cuda.synchronize()
        got.append([_np(tok), _np(lp).view(np.uint32), _np(u_out).view(np.uint32)])
    assert ((0 <= got[0][0]) & (got[0][0] < n)).all() and np.isfinite(got[0][1].view(np.float32)).all()
    assert np.array_equal(got[0][2], _np(u).view(np.uint32))
    for other in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got[0], other))

    b, len_q = 2, 3
    _, logits = _logits_dev(_make_rows(rng, b * len_q, n, False), n, False, dev)
    T, k, pp = dev_of(np.array([0.0, 0.9], np.float32)), dev_of(np.array([0, 8], np.int32)), dev_of(np.array([1.0, 0.95], np.float32))
    u = dev_of(rng.random((b, len_q)).astype(np.float32))
    first = torch.full((b, len_q), -7, dtype=i32, device=dev)           # the picks under these uniforms, for drafts that are partly accepted
    acc0 = torch.zeros(b, dtype=i32, device=dev)
    none = dev_of(np.full((b, len_q - 1), -1, np.int32))
    assert lib.zl_spec_sample_accept(p(logits), 2, b, len_q, n, n, p(none), p(T), p(k), p(pp), None, None, p(u), None, None, None, None, p(acc0),
                                     p(first), None, None, None, stream) == 0
    torch.cuda.synchronize()
    drafts = _np(none).copy()
    drafts[0, 0] = _np(first)[0, 0]                                     # task 0: its first draft is what the greedy row picks
    drafts = dev_of(drafts)
    got = []
    for way in ways:
        acc, out = torch.full((b,), -7, dtype=i32, device=dev), torch.full((b, len_q), -7, dtype=i32, device=dev)
        out_lp = torch.full((b, len_q), -77.0, dtype=f32, device=dev)
        args = [p(logits), 2, b, len_q, n, n, p(drafts), p(T), p(k), p(pp), None, None, p(u), None, None, None, None, p(acc), p(out), p(out_lp),
                None, None]
        assert way(lib.zl_spec_sample_accept, lib.zl_spec_sample_accept_ex, args) == 0
        torch.cuda.synchronize()
        got.append([_np(acc), _np(out), _np(out_lp).view(np.uint32)])
    assert got[0][0][0] >= 1 and got[0][0][1] == 0 and (got[0][1][:, 0] >= 0).all()
    for other in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got[0], other))


# ---- the model ----------------------------------------------------------------------------------------------------------------------
LEN_BUF = sv.LEN_BUF
PROMPT_LENS = [5, 40, 17, 9, 33, 1, 26, 12]


class _Case:
    pass


@pytest.fixture(scope="module")
def case(dev):
    c = _Case()
    rng, c.cfg, c.sd, c.model = _gptq_model(dev)
    c.vocab = c.cfg.vocab_size
    c.prompts = [rng.integers(0, c.vocab, s).astype(np.int32) for s in PROMPT_LENS]
    return c


@pytest.mark.parametrize("b", [1, 3, 8])
def test_temperature_zero_is_step_greedy(case, b):
    c = case
    ctx, twin = sv._fresh(c.model, c.prompts[:b]), sv._fresh(c.model, c.prompts[:b])
    state = c.model.new_sampler(ctx, temperature=0.0, top_k=20, top_p=0.95, seed=1)
    for step in range(6):
        _, got = c.model.step_sample(ctx, state)
        got = got.clone()
        _, ref = c.model.step_greedy(twin)
        assert torch.equal(got, ref), step
        for m in sv.STATE:
            assert torch.equal(getattr(ctx, m), getattr(twin, m)), (step, m)
        assert ctx.steps_left == twin.steps_left
    assert state.draws.tolist() == [6] * b


@pytest.mark.parametrize("b", [1, 3, 8])
def test_step_sample_follows_the_rule_and_replays(case, b):
    """every step's token is sample_ref.sample on that step's returned logits under sample_ref.uniforms; a captured step replayed 5
    times continues the eager sequence of a twin context; generate_sample is the loop"""
    c = case
    kw = dict(temperature=0.8, top_k=20, top_p=0.95, seed=77)
    ctx = sv._fresh(c.model, c.prompts[:b])
    state = c.model.new_sampler(ctx, **kw)
    seeds = np.arange(b) + 77
    assert state.seeds.tolist() == seeds.tolist()
    eager = []
    for step in range(6):
        pos = _np(ctx.positions).copy()
        logits, nxt = c.model.step_sample(ctx, state)
        u = sample_ref.uniforms(seeds, np.full(b, step))
        assert np.array_equal(_np(state.u), u) and state.draws.tolist() == [step + 1] * b
        rows = _np(logits.float()).astype(np.float64)
        for j in range(b):
            assert int(nxt[j]) == sample_ref.sample(rows[j], 0.8, 20, 0.95, u[j])[0], (step, j)
            assert abs(float(state.logprobs[j]) - sample_ref.logprob(rows[j], 0.8, int(nxt[j]))) <= np.abs(rows[j]).max() * 2.0 ** -10 + bound(c.vocab)
        assert np.array_equal(_np(ctx.tokens), _np(nxt).astype(np.int32)) and np.array_equal(_np(ctx.positions), pos + 1)
        eager.append(_np(nxt).copy())
    assert ctx.steps_left == LEN_BUF - max(PROMPT_LENS[:b]) - 6
    # capture after one eager step; five replays continue the twin's sequence
    twin = sv._fresh(c.model, c.prompts[:b])
    tstate = c.model.new_sampler(twin, **kw)
    _, nxt = c.model.step_sample(twin, tstate)
    assert np.array_equal(_np(nxt), eager[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gnxt = c.model.step_sample(twin, tstate)
    for step in range(1, 6):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(gnxt), eager[step]), step
    for m in sv.STATE:
        assert torch.equal(getattr(twin, m), getattr(ctx, m)), m
    assert torch.equal(tstate.draws, state.draws) and torch.equal(tstate.logprobs, state.logprobs)
    # generate_sample is the loop
    third = sv._fresh(c.model, c.prompts[:b])
    toks, lps = c.model.generate_sample(third, c.model.new_sampler(third, **kw), 6)
    assert toks.shape == (b, 6) and lps.shape == (b, 6) and toks.dtype == torch.int64 and lps.dtype == torch.float32
    assert np.array_equal(_np(toks), np.stack(eager, axis=1)) and torch.equal(lps[:, 5], state.logprobs)
    assert third.steps_left == ctx.steps_left


def test_model_refusals(case):
    from zhilight_amd import ops
    c = case
    ctx = sv._fresh(c.model, c.prompts[:3])
    state = c.model.new_sampler(ctx, temperature=[0.0, 0.8, 1.2], top_k=[0, 20, 511], top_p=[1.0, 0.95, 0.5], seed=[9, 9, 10])
    assert state.seeds.tolist() == [9, 9, 10]
    with pytest.raises(ops.ZLError, match="another batch size"):
        c.model.step_sample(sv._fresh(c.model, c.prompts[:2]), state)
    ctx.steps_left = 0                                                                             # out of room, as for step_greedy
    tokens = ctx.tokens.clone()
    with pytest.raises(ops.ZLError, match="past the end of the KV buffers"):
        c.model.step_sample(ctx, state)
    with pytest.raises(ops.ZLError, match="past the end of the KV buffers"):
        c.model.step_greedy(ctx)
    assert state.draws.tolist() == [0, 0, 0] and torch.equal(ctx.tokens, tokens)                  # a refused step draws nothing
    toks, lps = c.model.generate_sample(ctx, state, 4)
    assert toks.shape == (3, 0) and lps.shape == (3, 0)
    ctx.steps_left = 2                                                                             # generate_sample stops where the buffers end
    toks, _ = c.model.generate_sample(ctx, state, 4)
    assert toks.shape == (3, 2) and ctx.steps_left == 0
