"""Repetition and presence penalties inside the device sampling step: zl_sample_advance_ex / zl_spec_sample_accept_ex / zl_seen_mark
and LLaMA.new_sampler(repetition_penalty=, presence_penalty=, penalty_tokens=).  The bar is EQUALITY with what the project already had:
ops.repetition_penalty over the set's (token, batch_id) list on a copy of the logits, then the existing ops.sample_advance /
ops.spec_sample_accept on the copy -- both paths run the same arithmetic on the same 16-bit patterns, so every result is compared bit
for bit, NaNs included.  The raw logits stay as they were and the bitmap gains exactly the emitted tokens."""
import numpy as np
import pytest
import torch

import penalty_ref as pr
import sample_ref
import test_gpu_sample as ts
import test_gpu_spec_verify as sv
from test_gpu_prefill_batch import _gptq_model

pytestmark = pytest.mark.gpu

NS = [1, 31, 32, 33, 63, 65, 257, 1025, 4097, 128256]
ROWS = 8
PENS = [(1.3, 0.0), (1.0, 0.7), (1.3, 0.7), (0.5, 0.0), (1.0, 0.0)]
SETS = ["empty", "single", "argmax", "percent", "all", "last_word", "stray"]
_np = sv._np


def _bits(t):
    """any tensor as integers of its width: equality of floats is equality of patterns"""
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), what


def _seen_dev(seen, dev):
    return torch.from_numpy(np.ascontiguousarray(seen).view(np.int32)).to(dev)


def _seen_np(t):
    return _np(t).view(np.uint32)


def _penalise(ops, buf2d, sets, factor, presence, dev):
    """ops.repetition_penalty on the rows of buf2d (rows, ld) contiguous: sets[r] = the ids of row r, factor / presence per row"""
    tok = np.concatenate([np.asarray(s, np.int32) for s in sets]) if sets else np.zeros(0, np.int32)
    if tok.size == 0:
        return
    bid = np.concatenate([np.full(len(s), r, np.int32) for r, s in enumerate(sets)])
    f = np.asarray(factor, np.float32)[bid]
    p = np.asarray(presence, np.float32)[bid]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                    # noqa: E731
    ops.repetition_penalty(to(f), to(tok), to(bid), buf2d, presence=to(p))


def _row_sets(kind, rng, bits, bf16, n):
    rows = bits.shape[0]
    if kind == "empty":
        return [np.zeros(0, np.int64)] * rows
    if kind == "single":
        return [rng.integers(0, n, 1) for _ in range(rows)]
    if kind == "argmax":
        return [np.array([sample_ref.argmax(sample_ref.values_of(bits[r], bf16))]) for r in range(rows)]
    if kind in ("percent", "stray"):
        return [np.unique(rng.integers(0, n, max(1, n // 100))) for _ in range(rows)]
    if kind == "all":
        return [np.arange(n)] * rows
    lo = 32 * ((n - 1) // 32)
    return [np.unique(rng.integers(lo, n, 1 + r % 3)) for r in range(rows)]             # last_word


class _Out:
    NAMES = ("tokens", "positions", "placement", "valid_lens", "next_tokens", "logprobs", "u_out")

    def __init__(self, rows, dev):
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        self.kw = dict(tokens=torch.arange(rows, dtype=i32, device=dev) + 3, positions=torch.arange(rows, dtype=i32, device=dev) + 10,
                       placement=torch.arange(rows, dtype=i32, device=dev) + 20, valid_lens=torch.arange(rows, dtype=i32, device=dev) + 30,
                       next_tokens=torch.full((rows,), -7, dtype=i64, device=dev), logprobs=torch.full((rows,), -77.0, dtype=f32, device=dev),
                       u_out=torch.full((rows,), -77.0, dtype=f32, device=dev))


def _two_paths(ops, dev, bits, ld, bf16, sets, factor, presence, seen, T, k, p, u):
    """-> (fused outputs, two-step outputs, seen afterwards); asserts the raw logits unchanged"""
    rows, n = bits.shape
    flat_a, raw = ts._logits_dev(bits, ld, bf16, dev)
    flat_b, copy = ts._logits_dev(bits, ld, bf16, dev)
    before = flat_a.clone()
    _penalise(ops, flat_b[:rows * ld].view(rows, ld), sets, factor, presence, dev)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)  # noqa: E731
    par = dict(temperature=to(T, np.float32), top_k=to(k, np.int32), top_p=to(p, np.float32), u=to(u, np.float32))
    two, one = _Out(rows, dev), _Out(rows, dev)
    ops.sample_advance(copy, **par, **two.kw)
    seen_dev = _seen_dev(seen, dev)
    ops.sample_advance(raw, **par, **one.kw, rep_penalty=to(factor, np.float32), presence=to(presence, np.float32), seen=seen_dev)
    torch.cuda.synchronize()
    _same(flat_a, before, "the raw logits")
    return one, two, _seen_np(seen_dev)


# ---- 1. the kernel against repetition_penalty + sample_advance ----------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("n", NS)
def test_kernel_equals_penalty_then_sample(dev, n, bf16):
    """8 rows at ld = n + 3 (every row starts at another 16-byte offset); row r: T = 0 / 0.7, top-k = 0 / 5, top-p = 1 / 0.9 by the bits
    of r, the five penalty pairs in rotation; seven kinds of set, each with seen_ld = ceil(n / 32) and three words more"""
    from zhilight_amd import ops
    rng = np.random.default_rng(11 * n + bf16)
    ld = n + 3
    r = np.arange(ROWS)
    T, k, p = np.where(r & 1, 0.7, 0.0), np.where(r & 2, 5, 0), np.where(r & 4, 0.9, 1.0)
    moved = 0
    for si, kind in enumerate(SETS):
        bits = ts._make_rows(rng, ROWS, n, bf16, shift=si)
        u = rng.random(ROWS).astype(np.float32)
        sets = _row_sets(kind, rng, bits, bf16, n)
        factor = np.array([PENS[(j + si) % 5][0] for j in range(ROWS)], np.float32)
        presence = np.array([PENS[(j + si) % 5][1] for j in range(ROWS)], np.float32)
        if kind == "argmax":                                                            # large enough to move the arg-max
            factor, presence = np.where(r & 1, 64.0, 1.0).astype(np.float32), np.where(r & 1, 0.0, 50.0).astype(np.float32)
        for extra in (0, 3):
            seen = pr.pack(sets, n, ld=pr.words(n) + extra)
            if kind == "stray":                                                         # bits at or above n: never classes
                if n % 32:
                    seen[:, (n - 1) >> 5] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
                seen[:, pr.words(n):] = 0xDEADBEEF
            one, two, after = _two_paths(ops, dev, bits, ld, bf16, sets, factor, presence, seen, T, k, p, u)
            for name in _Out.NAMES:
                _same(one.kw[name], two.kw[name], (kind, extra, name))
            picks = _np(one.kw["tokens"]).astype(np.int64)
            assert picks.min() >= 0 and picks.max() < n
            assert np.array_equal(after, pr.mark(seen.copy(), picks.reshape(-1, 1), n)), (kind, extra)
            if kind == "argmax":
                moved += int((picks[T == 0] != np.concatenate(sets)[T == 0]).sum())
    if n >= 31:
        assert moved > 0                                                                # the penalty did reach the arg-max


# ---- 2. edge rows ---------------------------------------------------------------------------------------------------------------------
def test_edge_rows(dev):
    """a factor that takes an fp16 logit to -inf; a row whose only finite classes are all in the set (they stay the only finite ones,
    or all become -inf); a NaN row -- each against the two-step path"""
    from zhilight_amd import ops
    n, ld = 70, 73
    x = np.full((ROWS, n), -np.inf, np.float32)
    x[0] = np.linspace(-60000, 100, n)                                                  # -60000 * 4 -> -inf
    x[1] = np.linspace(-60000, 100, n)
    x[2, [3, 40, 69]] = [1.0, 2.0, -1.0]                                                # finite classes = the set
    x[3, [3, 40, 69]] = [-40000.0, -50000.0, -60000.0]                                  # ... and the penalty takes all three to -inf
    x[4] = np.linspace(-3, 3, n)
    x[4, 17] = np.nan
    x[5] = np.linspace(-3, 3, n)
    x[5, 50] = np.inf
    x[6] = np.linspace(3, -3, n)
    x[7, 0] = 0.0
    bits = x.astype(np.float16).view(np.uint16)
    sets = [np.arange(0, n, 2), np.arange(n), np.array([3, 40, 69]), np.array([3, 40, 69]), np.array([17, 18]), np.array([50]),
            np.array([0]), np.array([0])]
    factor = np.array([4.0, 4.0, 2.0, 4.0, 2.0, 2.0, 1e30, 3.0], np.float32)           # 1e30 -> T(factor) = +inf
    presence = np.zeros(ROWS, np.float32)
    for T in (np.zeros(ROWS), np.full(ROWS, 0.7)):
        for k, p in ((0, 1.0), (5, 0.9)):
            u = np.linspace(0.05, 0.95, ROWS).astype(np.float32)
            seen = pr.pack(sets, n)
            one, two, after = _two_paths(ops, dev, bits, ld, False, sets, factor, presence, seen, T, np.full(ROWS, k), np.full(ROWS, p), u)
            for name in _Out.NAMES:
                _same(one.kw[name], two.kw[name], (name, k, p))
            picks = _np(one.kw["tokens"]).astype(np.int64)
            assert np.array_equal(after, pr.mark(seen.copy(), picks.reshape(-1, 1), n))
            lp = _np(one.kw["logprobs"])
            assert np.isnan(lp[[3, 4, 5]]).all() and picks[4] == 17 and picks[5] == 50 and picks[2] in (3, 40, 69) and np.isfinite(lp[[0, 1, 2, 6, 7]]).all()


def test_abi_refusals(dev):
    from zhilight_amd import ops
    n = 40
    logits = torch.zeros((2, n), dtype=torch.float16, device=dev)
    f32 = lambda v: torch.full((2,), v, dtype=torch.float32, device=dev)                # noqa: E731
    kw = dict(temperature=f32(1.0), top_k=torch.zeros(2, dtype=torch.int32, device=dev), top_p=f32(1.0), u=f32(0.5),
              tokens=torch.zeros(2, dtype=torch.int32, device=dev))
    seen = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    with pytest.raises(ops.ZLError, match="rep_penalty"):
        ops.sample_advance(logits, **kw, seen=seen, presence=f32(0.0))
    with pytest.raises(ops.ZLError, match="give the bitmap"):
        ops.sample_advance(logits, **kw, rep_penalty=f32(1.0), presence=f32(0.0))
    with pytest.raises(ops.ZLError, match="seen"):
        ops.sample_advance(logits, **kw, rep_penalty=f32(1.0), presence=f32(0.0), seen=seen[:, :1].contiguous())
    # the C ABI's own codes
    from zhilight_amd._lib import SampleOpts, lib
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)                   # noqa: E731
    i = C.c_int64
    ptr = lambda t: None if t is None else t.data_ptr()                                 # noqa: E731

    def call(rep, pres, sn, seen_ld, null_opts=False):
        opts = None if null_opts else C.byref(SampleOpts(rep_penalty=ptr(rep), presence=ptr(pres), seen=ptr(sn), seen_ld=seen_ld))
        return lib().zl_sample_advance_ex(p(logits), C.c_int(2), i(2), i(n), i(n), p(kw["temperature"]), p(kw["top_k"]), p(kw["top_p"]), p(None),
                                          p(None), p(kw["u"]), p(kw["tokens"]), p(None), p(None), p(None), p(None), p(None), p(None), opts,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    einval, eshape = call(None, kw["u"], seen, 2), call(kw["u"], kw["u"], seen, 1)
    assert einval != 0 and eshape != 0 and einval != eshape
    assert call(None, None, None, 0) == 0 and call(None, None, None, 0, null_opts=True) == 0       # a zeroed struct / NULL opts: the plain call
    assert call(f32(1.0), f32(0.0), seen, 2) == 0
    torch.cuda.synchronize()
    assert ops.seen_words(1) == 1 and ops.seen_words(32) == 1 and ops.seen_words(33) == 2 and ops.seen_words(128256) == 4008


# ---- 3. the speculative kernel ----------------------------------------------------------------------------------------------------------
SPEC_STATE = ("tokens", "positions", "placement", "valid_lens")


def _spec_two_paths(ops, dev, bits, bf16, drafts, seen, factor, presence, T, k, p, u=None, seeds=None, draws=None):
    """ops.spec_sample_accept(seen=) on the raw rows against ops.repetition_penalty with penalty_ref's row sets + the plain call; asserts
    every output equal -> (fused outputs as numpy, seen afterwards)"""
    m, n = bits.shape
    b, len_q = drafts.shape[0], drafts.shape[1] + 1
    ld = n + 3
    flat_a, raw = ts._logits_dev(bits, ld, bf16, dev)
    flat_b, copy = ts._logits_dev(bits, ld, bf16, dev)
    before = flat_a.clone()
    sets = pr.row_sets(pr.unpack(seen, n), drafts, n)
    _penalise(ops, flat_b[:m * ld].view(m, ld), [sets[t][i] for t in range(b) for i in range(len_q)], np.repeat(factor, len_q),
              np.repeat(presence, len_q), dev)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)  # noqa: E731
    outs = []
    seen_dev = _seen_dev(seen, dev)
    for which, logits in (("two", copy), ("one", raw)):
        i32, f32 = torch.int32, torch.float32
        kw = dict(temperature=to(T, np.float32), top_k=to(k, np.int32), top_p=to(p, np.float32),
                  tokens=torch.arange(b, dtype=i32, device=dev) + 3, positions=torch.arange(b, dtype=i32, device=dev) + 10,
                  placement=torch.arange(b, dtype=i32, device=dev) + 20, valid_lens=torch.arange(b, dtype=i32, device=dev) + 30,
                  accepted=torch.full((b,), -7, dtype=i32, device=dev), out_tokens=torch.full((b, len_q), -7, dtype=i32, device=dev),
                  out_logprobs=torch.full((b, len_q), -77.0, dtype=f32, device=dev), logprobs=torch.full((b,), -77.0, dtype=f32, device=dev),
                  u_out=torch.full((b, len_q), -77.0, dtype=f32, device=dev))
        if u is not None:
            kw["u"] = to(u, np.float32)
        else:
            kw["seeds"], kw["draws"] = to(seeds, np.int64), to(draws, np.int64)
        if which == "one":
            kw.update(rep_penalty=to(factor, np.float32), presence=to(presence, np.float32), seen=seen_dev)
        ops.spec_sample_accept(logits, to(drafts, np.int32), **kw)
        outs.append(kw)
    torch.cuda.synchronize()
    two, one = outs
    for name in ("accepted", "out_tokens", "out_logprobs", "logprobs", "u_out", "draws") + SPEC_STATE:
        if name in two:
            _same(one[name], two[name], name)
    _same(flat_a, before, "the raw logits")
    after = _seen_np(seen_dev)
    assert np.array_equal(after, pr.mark(seen.copy(), _np(one["out_tokens"]), n))       # the emitted tokens; -1 is skipped
    return {name: _np(t) for name, t in one.items()}, after


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("n", [33, 1025, 128256])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("len_q", [2, 5, 32])
def test_spec_kernel_equals_penalty_then_accept(dev, len_q, b, n, bf16):
    """task 0 is greedy and its drafts follow the penalised arg-max (computed in numpy) up to one wrong draft, so rows deep into the
    step are emitted and their sets are the drafts in front of them; the other tasks sample, with drafts from the row's largest
    classes, a repeated draft, a -1 and an out-of-range id.  Given uniforms for b = 1, the generator for b = 3"""
    from zhilight_amd import ops
    rng = np.random.default_rng(1000 * len_q + 10 * n + 2 * b + bf16)
    K = len_q - 1
    bits = ts._make_rows(rng, b * len_q, n, bf16, shift=1)
    factor = np.array([1.3, 1.0, 0.5][:b], np.float32)
    presence = np.array([0.0, 0.7, 0.0][:b], np.float32)
    T, k, p = np.array([0.0, 0.7, 0.7][:b], np.float32), np.array([0, 5, 0][:b], np.int32), np.array([1.0, 0.9, 1.0][:b], np.float32)
    ids = [np.unique(rng.integers(0, n, max(1, n // 100))) for _ in range(b)]
    seen = pr.pack(ids, n, ld=pr.words(n) + (b - 1))
    drafts = np.empty((b, K), np.int64)
    for t in range(b):
        for i in range(K):
            vals = sample_ref.values_of(bits[t * len_q + i], bf16)
            drafts[t, i] = int(np.argsort(-np.nan_to_num(vals, nan=np.inf), kind="stable")[rng.integers(0, min(3, n))])
    # task 0: the penalised arg-max of every row, given the drafts in front of it
    wrong = K - 1 if K > 2 else K                                                        # one wrong draft near the end (none for len_q <= 3)
    for i in range(K):
        s = np.asarray(sorted(set(ids[0].tolist()) | {int(d) for d in drafts[0, :i]}), np.int64)
        row = bits[i].copy()
        row[s] = pr.pen(row[s], bf16, factor[0], presence[0])
        drafts[0, i] = sample_ref.argmax(sample_ref.values_of(row, bf16))
        if i == wrong:
            drafts[0, i] = (drafts[0, i] + 1) % n
    if b > 1 and K >= 2:
        drafts[1, 1] = drafts[1, 0]                                                     # a repeated draft
    if b > 1 and K >= 4:
        drafts[1, 2], drafts[2, 1] = -1, n + 5
    if b == 1:
        got, _ = _spec_two_paths(ops, dev, bits, bf16, drafts, seen, factor, presence, T, k, p, u=rng.random((b, len_q)).astype(np.float32))
    else:
        got, _ = _spec_two_paths(ops, dev, bits, bf16, drafts, seen, factor, presence, T, k, p, seeds=np.arange(b) + 5, draws=np.arange(b) * 3)
    want0 = min(wrong, K) if n > 1 else K
    assert got["accepted"][0] == want0, (got["accepted"], want0)                         # the greedy task took the constructed path


def test_spec_penalty_decides_acceptance(dev):
    """hand-made rows, greedy, len_q = 3, empty sets.  Task 0: draft 1 is accepted ONLY BECAUSE draft 0's penalty is applied to row 1
    (class 5 leads row 1 unpenalised; halved it falls behind the draft, class 7).  Task 1: draft 1 repeats draft 0 and is rejected
    ONLY BECAUSE of it.  Without the bitmap the outcomes are the opposite"""
    from zhilight_amd import ops
    n, b, len_q = 33, 2, 3
    x = np.full((b * len_q, n), -2.0, np.float32)
    for t in range(b):
        x[t * len_q + 0, 5] = 4.0
        x[t * len_q + 1, [5, 7]] = [4.0, 3.0]
        x[t * len_q + 2, 32] = 1.0
    bits = x.astype(np.float16).view(np.uint16)
    drafts = np.array([[5, 7], [5, 5]], np.int64)
    factor, presence = np.array([2.0, 2.0], np.float32), np.zeros(2, np.float32)
    T, k, p = np.zeros(2, np.float32), np.zeros(2, np.int32), np.ones(2, np.float32)
    u = np.full((b, len_q), 0.5, np.float32)
    got, after = _spec_two_paths(ops, dev, bits, False, drafts, pr.pack([[], []], n), factor, presence, T, k, p, u=u)
    assert got["accepted"].tolist() == [2, 1]
    assert got["out_tokens"].tolist() == [[5, 7, 32], [5, 7, -1]]
    assert [s.tolist() for s in pr.unpack(after, n)] == [[5, 7, 32], [5, 7]]            # task 1's rejected draft added nothing new
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)  # noqa: E731
    _, raw = ts._logits_dev(bits, n + 3, False, dev)
    acc, out = ops.spec_sample_accept(raw, to(drafts, np.int32), to(T, np.float32), to(k, np.int32), to(p, np.float32), u=to(u, np.float32))
    assert acc.tolist() == [1, 2] and out.tolist() == [[5, 5, -1], [5, 5, 32]]


# ---- 4. seen_mark -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tok", [1, 33])
@pytest.mark.parametrize("b", [1, 4])
def test_seen_mark(dev, b, n_tok):
    from zhilight_amd import ops
    rng = np.random.default_rng(b * 100 + n_tok)
    for n in (33, 4097):
        tok = rng.integers(0, n, (b, n_tok)).astype(np.int32)
        tok[:, ::5] = rng.integers(64, 96, tok[:, ::5].shape) % n                       # duplicates and neighbours inside one word
        if n_tok > 1:
            tok[:, 1] = -1
            tok[:, 3:6] = [n, n + 40, -2147483648]
            tok[:, 7] = tok[:, 8]
        for extra, tok_ld in ((0, n_tok), (2, n_tok + 5)):
            seen = pr.pack([rng.integers(0, n, 3) for _ in range(b)], n, ld=pr.words(n) + extra)
            seen[:, -1] |= np.uint32(0x80000000)                                        # what is there stays
            buf = torch.full((b, tok_ld), n - 1, dtype=torch.int32, device=dev)         # the padding of a row is not read
            buf[:, :n_tok] = torch.from_numpy(tok)
            dev_seen = _seen_dev(seen, dev)
            ops.seen_mark(dev_seen, buf[:, :n_tok], n)
            torch.cuda.synchronize()
            assert np.array_equal(_seen_np(dev_seen), pr.mark(seen.copy(), tok, n)), (n, extra)


# ---- 5. the model -------------------------------------------------------------------------------------------------------------------------
K = sv.K
STEPS = 12
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
    c.loops = {}
    return c


def _pen_kw(b):
    return {name: v[:b] for name, v in PEN_KW.items()}


def _host_loop(c, b, dev):
    """the path a caller had: encode, ops.repetition_penalty over the tokens emitted so far on a copy, ops.sample_advance with the
    generator's uniforms -> (tokens (b, STEPS), logprobs (b, STEPS) as patterns); computed once per b"""
    if b in c.loops:
        return c.loops[b]
    from zhilight_amd import ops
    ctx = sv._fresh(c.model, c.motifs[:b])
    emitted = [[int(t)] for t in ctx.tokens.tolist()]                                   # the pending token is an emitted one
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)                    # noqa: E731
    T, k, p = f32([0.8] * b), torch.tensor([20] * b, dtype=torch.int32, device=dev), f32([0.95] * b)
    pen = _pen_kw(b)
    nxt, lp = torch.empty(b, dtype=torch.int64, device=dev), torch.empty(b, dtype=torch.float32, device=dev)
    toks, lps = [], []
    for step in range(STEPS):
        copy = c.model.encode(ctx).clone()
        _penalise(ops, copy, [sorted(set(e)) for e in emitted], pen["repetition_penalty"], pen["presence_penalty"], dev)
        u = torch.from_numpy(sample_ref.uniforms(77 + np.arange(b), np.full(b, step))).to(dev)
        ops.sample_advance(copy, T, k, p, u=u, tokens=ctx.tokens, positions=ctx.positions, placement=ctx.placement, valid_lens=ctx.valid_lens,
                           next_tokens=nxt, logprobs=lp)
        ctx.steps_left -= 1
        for j, t in enumerate(nxt.tolist()):
            emitted[j].append(t)
        toks.append(_np(nxt).copy())
        lps.append(_np(lp).view(np.int32).copy())
    c.loops[b] = (np.stack(toks, axis=1), np.stack(lps, axis=1))
    return c.loops[b]


@pytest.mark.parametrize("b", [1, 3])
def test_generate_sample_is_the_host_loop(case, dev, b):
    c = case
    toks, lps = _host_loop(c, b, dev)
    ctx = sv._fresh(c.model, c.motifs[:b])
    pending = ctx.tokens.tolist()
    state = c.model.new_sampler(ctx, **KW, **_pen_kw(b))
    assert state.seen.shape == (b, (c.vocab + 31) // 32) and state.seen.dtype == torch.int32
    assert [s.tolist() for s in pr.unpack(_seen_np(state.seen), c.vocab)] == [[t] for t in pending]
    got, got_lp = c.model.generate_sample(ctx, state, STEPS)
    assert np.array_equal(_np(got), toks)
    assert np.array_equal(_np(got_lp).view(np.int32), lps)
    for j in range(b):                                                                  # the bitmap = everything emitted
        assert pr.unpack(_seen_np(state.seen), c.vocab)[j].tolist() == sorted(set([pending[j]] + toks[j].tolist()))


@pytest.mark.parametrize("b", [1, 3])
def test_generate_lookup_emits_the_same_tokens(case, dev, b):
    """speculation changes the speed, not the sample: the penalised lookup steps emit the host loop's tokens"""
    c = case
    toks, lps = _host_loop(c, b, dev)
    ctx = sv._fresh(c.model, c.motifs[:b])
    pending = ctx.tokens.tolist()
    look = c.model.new_lookup(ctx, c.motifs[:b], K)
    samp = c.model.new_sampler(ctx, **KW, **_pen_kw(b))
    got, stats = c.model.generate_lookup(ctx, look, STEPS, sampler=samp)
    assert got == toks.tolist()
    # the tokens are the claim.  The log-probabilities are those of the verify rows' logits, which another GEMM route computed: close to
    # the one-row steps', not their patterns
    lp = np.array(stats["logprobs"], np.float32)
    assert lp.shape == lps.shape and np.isfinite(lp).all() and (lp <= 0).all()
    print("max |logprob - the host loop's|", float(np.abs(lp - lps.view(np.float32)).max()))
    print("accepted drafts per task", stats["accepted"], "in", stats["steps"], "steps")
    seen = pr.unpack(_seen_np(samp.seen), c.vocab)
    for j in range(b):                                                                  # emitted, the cut-off tail of the last round included
        assert set(toks[j].tolist()) | {pending[j]} <= set(seen[j].tolist()) and len(seen[j]) <= 1 + stats["emitted"][j]


@pytest.mark.parametrize("b", [1, 3])
def test_captured_steps_continue_the_eager_sequence(case, dev, b):
    c = case
    toks, _ = _host_loop(c, b, dev)
    # step_sample
    ctx = sv._fresh(c.model, c.motifs[:b])
    state = c.model.new_sampler(ctx, **KW, **_pen_kw(b))
    _, nxt = c.model.step_sample(ctx, state)
    assert np.array_equal(_np(nxt), toks[:, 0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gnxt = c.model.step_sample(ctx, state)
    for step in range(1, 6):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(gnxt), toks[:, step]), step
    # step_lookup(sampler=): replays against an eager twin
    def start():
        x = sv._fresh(c.model, c.motifs[:b])
        return x, c.model.new_lookup(x, c.motifs[:b], K), c.model.new_sampler(x, **KW, **_pen_kw(b))
    ectx, elook, esamp = start()
    eager = []
    for _ in range(4):
        res = c.model.step_lookup(ectx, elook, sampler=esamp)
        eager.append((res.accepted.clone(), res.tokens.clone(), esamp.seen.clone()))
    tctx, tlook, tsamp = start()
    res = c.model.step_lookup(tctx, tlook, sampler=tsamp)
    assert torch.equal(res.tokens, eager[0][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = c.model.step_lookup(tctx, tlook, sampler=tsamp)
    for step in range(1, 4):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(r.accepted, eager[step][0]) and torch.equal(r.tokens, eager[step][1]) and torch.equal(tsamp.seen, eager[step][2]), step
    out = [[] for _ in range(b)]                                                        # and the eager rounds are the host loop's tokens
    for acc, tok, _ in eager:
        for j in range(b):
            out[j] += tok[j, :int(acc[j]) + 1].tolist()
    for j in range(b):
        m = min(len(out[j]), STEPS)
        assert out[j][:m] == toks[j, :m].tolist()


def test_penalty_tokens_change_the_first_pick(case, dev):
    """greedy, presence 100: the first pick g of a task is its row's arg-max outside the pending token; with penalty_tokens = [g] the
    first pick must be the arg-max outside {pending, g}"""
    c = case
    b = 3
    ctx = sv._fresh(c.model, c.motifs[:b])
    pending = ctx.tokens.tolist()
    state = c.model.new_sampler(ctx, temperature=0.0, presence_penalty=100.0)
    logits, nxt = c.model.step_sample(ctx, state)
    rows, g = _np(logits.float()).astype(np.float64), nxt.tolist()
    assert np.abs(rows).max() < 50                                                      # 100 puts a class behind every other
    ctx2 = sv._fresh(c.model, c.motifs[:b])
    state2 = c.model.new_sampler(ctx2, temperature=0.0, presence_penalty=100.0, penalty_tokens=[[t] for t in g])
    assert [s.tolist() for s in pr.unpack(_seen_np(state2.seen), c.vocab)] == [sorted({pending[j], g[j]}) for j in range(b)]
    _, nxt2 = c.model.step_sample(ctx2, state2)
    for j in range(b):
        masked = rows[j].copy()
        masked[pending[j]] = -np.inf
        assert g[j] == int(masked.argmax())
        masked[g[j]] = -np.inf
        assert int(nxt2[j]) == int(masked.argmax()) != g[j]
    # the prompt as penalty_tokens (tensors and arrays both), every id marked
    ctx3 = sv._fresh(c.model, c.motifs[:b])
    state3 = c.model.new_sampler(ctx3, repetition_penalty=1.2, penalty_tokens=[torch.from_numpy(c.motifs[0]), c.motifs[1], list(c.motifs[2])])
    for j in range(b):
        assert pr.unpack(_seen_np(state3.seen), c.vocab)[j].tolist() == sorted(set(c.motifs[j].tolist()) | {pending[j]})


@pytest.mark.parametrize("b", [1, 3])
def test_penalties_off_is_todays_state(case, dev, b):
    """(1, 0) everywhere and no penalty_tokens: no bitmap, the steps are the plain ones; a NEUTRAL bitmap (penalty_tokens = nothing,
    factor 1, presence 0) picks the same tokens through the penalised kernel and records them"""
    c = case
    ctx, ctx2, ctx3 = (sv._fresh(c.model, c.motifs[:b]) for _ in range(3))
    plain = c.model.new_sampler(ctx, **KW)
    off = c.model.new_sampler(ctx2, **KW, repetition_penalty=[1.0] * b, presence_penalty=0.0)
    for s in (plain, off):
        assert s.seen is None and s.repetition_penalty is None and s.presence_penalty is None
    neutral = c.model.new_sampler(ctx3, **KW, penalty_tokens=[[]] * b)
    assert neutral.seen is not None and neutral.repetition_penalty.tolist() == [1.0] * b and neutral.presence_penalty.tolist() == [0.0] * b
    a, a_lp = c.model.generate_sample(ctx, plain, 5)
    o, o_lp = c.model.generate_sample(ctx2, off, 5)
    x, x_lp = c.model.generate_sample(ctx3, neutral, 5)
    assert torch.equal(a, o) and torch.equal(a, x)
    _same(a_lp, o_lp, "logprobs, penalties off")
    _same(a_lp, x_lp, "logprobs, neutral bitmap")
    for j in range(b):
        assert set(a[j].tolist()) <= set(pr.unpack(_seen_np(neutral.seen), c.vocab)[j].tolist())


def test_model_refusals(case, dev):
    from zhilight_amd import ops
    c = case
    ctx = sv._fresh(c.model, c.motifs[:3])
    for bad in (0.0, -1.0, float("inf"), float("nan"), [1.0, 0.0, 1.0]):
        with pytest.raises(ops.ZLError, match="repetition_penalty > 0"):
            c.model.new_sampler(ctx, repetition_penalty=bad)
    with pytest.raises(ops.ZLError, match="presence_penalty is finite"):
        c.model.new_sampler(ctx, presence_penalty=float("nan"))
    with pytest.raises(ops.ZLError, match="2 values of repetition_penalty"):
        c.model.new_sampler(ctx, repetition_penalty=[1.1, 1.2])
    with pytest.raises(ops.ZLError, match="4 values of presence_penalty"):
        c.model.new_sampler(ctx, presence_penalty=[0.1] * 4)
    with pytest.raises(ops.ZLError, match="2 sequences of penalty_tokens"):
        c.model.new_sampler(ctx, penalty_tokens=[[1], [2]])
    with pytest.raises(ops.ZLError, match="penalty_tokens outside"):
        c.model.new_sampler(ctx, penalty_tokens=[[1], [c.vocab], [2]])
    state = c.model.new_sampler(ctx, repetition_penalty=1.3)
    two = sv._fresh(c.model, c.motifs[:2])
    with pytest.raises(ops.ZLError, match="another batch size"):
        c.model.step_sample(two, state)
    with pytest.raises(ops.ZLError, match="another batch size"):
        c.model.verify(two, torch.zeros((2, K), dtype=torch.int32, device=dev), sampler=state)
    assert state.draws.tolist() == [0, 0, 0]
