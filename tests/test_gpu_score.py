"""Scoring: the fused lm_head log-probability kernel (zl_lm_head_score, ops.lm_head_score) against ops.gemm_nt's stored logits (label
logit, arg-max: bit for bit; log-sum-exp: within the derived bound B(N) of test_score_host.py), the unfused chain, graph capture,
and LLaMA.score against the oracle composition over every prompt row and against prefill_batch for the state it leaves."""
import numpy as np
import pytest
import torch

from test_gpu_model import OracleModel
from test_gpu_prefill_batch import _gptq_model
from test_score_host import bound

pytestmark = pytest.mark.gpu

IGN = -100
SHAPES = [(1, 512, 1024), (5, 1000, 128), (70, 4099, 1024), (300, 128256, 4096)]


def _inputs(dev, m, n, k, dtype, seed, ldx=None, tie=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = (torch.randn(n, k, generator=g) * (2.0 / k ** 0.5)).to(dtype)
    for c in _tie_cols(n) if tie else ():
        w[c] = w[5]                                     # identical weight rows: identical logits in every row of y
    xs = torch.randn(m, ldx or k, generator=g).to(dtype).to(dev)
    x = xs[:, :k] if ldx else xs
    lab = torch.randint(0, n, (m,), generator=g, dtype=torch.int32)
    lab[torch.rand(m, generator=g) < 0.1] = IGN
    return x, w.to(dev), lab


def _tie_cols(n):
    """columns made identical to column 5: in its wave, in another wave of block 0, in another 128-column block (the merge across
    blocks) and in block 64 (the merge lane that strides blocks 0, 64, ... meets its own earlier candidate)"""
    return [c for c in (11, 37, 300, 64 * 128 + 5) if c < n]


def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _check_rows(r, ref, lab, n, what):
    """r: ScoreRows; ref: the (M, N) logits gemm_nt stored; lab: host int labels or None"""
    ref32 = ref.float()
    m = ref.shape[0]
    # 1. exact functions of the stored logits
    am = torch.argmax(ref32, dim=1)
    mx = ref32.max(dim=1).values
    first = (ref32 == mx[:, None]).int().argmax(dim=1)           # the lowest index that attains the maximum
    assert torch.equal(am, first), what
    assert torch.equal(r.greedy.long(), first), what
    assert torch.equal(r.greedy_logit, mx), what
    if lab is None:
        keep = torch.zeros(m, dtype=torch.bool, device=ref.device)
        ll = torch.zeros(m, device=ref.device)
    else:
        labd = lab.to(ref.device).long()
        keep = labd != IGN
        ll = torch.where(keep, ref32.gather(1, labd.clamp(min=0).view(-1, 1)).view(-1), torch.zeros(m, device=ref.device))
    assert torch.equal(r.label_logit, ll), what
    # 2. lse within B(N) + 2 ulp of the float64 log-sum-exp of the stored logits; logprob one fp32 subtraction
    ref64 = torch.logsumexp(ref.double(), dim=1).cpu().numpy()
    err = np.abs(r.lse.double().cpu().numpy() - ref64)
    lim = bound(n) + 2 * _ulp32(ref64)
    print(what, "lse err max", err.max(), "bound", bound(n))
    assert (err <= lim).all(), (what, err.max())
    assert torch.equal(r.logprob, torch.where(keep, r.label_logit - r.lse, torch.zeros_like(r.lse))), what
    assert (r.logprob[~keep] == 0).all() and (r.label_logit[~keep] == 0).all(), what


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_score_matches_stored_logits(dev, shape, dtype):
    from zhilight_amd import ops
    m, n, k = shape
    ldx = k + 64 if m == 70 else None                            # one case with a row stride above K
    x, w, lab = _inputs(dev, m, n, k, dtype, seed=m + n, ldx=ldx, tie=(m >= 70))
    ref = ops.gemm_nt(x.contiguous(), w)
    r = ops.lm_head_score(x, w, lab)                             # host labels: checked and uploaded by the wrapper
    _check_rows(r, ref, lab, n, (shape, dtype))
    if m >= 70:                                                  # the forced tie: these columns hold the same value in every row
        cols = [5] + _tie_cols(n)
        assert all(torch.equal(ref[:, 5], ref[:, c]) for c in cols)
        w2 = w.clone()
        w2[cols] *= 40.0                                         # ... and now they are the row's largest wherever they are positive
        ref2 = ops.gemm_nt(x.contiguous(), w2)
        r2 = ops.lm_head_score(x, w2, lab)
        _check_rows(r2, ref2, lab, n, (shape, dtype, "tie"))
        assert int((r2.greedy == 5).sum()) > 0 and all(int((r2.greedy == c).sum()) == 0 for c in cols[1:])
        for order in (0, 1):                                     # either launch order forced: the same bits
            for u, v in zip(ops.lm_head_score(x, w2, lab, order=order), r2):
                assert torch.equal(u, v)
    # 3. run to run: identical bits in all five outputs
    ws = ops.lm_head_score_workspace(m, n, dev)
    labd = lab.to(dev)
    a = ops.lm_head_score(x, w, labd, workspace=ws)
    b = ops.lm_head_score(x, w, labd, workspace=ws)
    for u, v, o in zip(a, b, r):
        assert torch.equal(u, v) and torch.equal(u, o)
    # labels=None: every row ignored, lse and greedy still produced
    z = ops.lm_head_score(x, w)
    _check_rows(z, ref, None, n, (shape, dtype, "no labels"))
    assert torch.equal(z.lse, r.lse) and torch.equal(z.greedy, r.greedy)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_unfused_chain_agrees(dev, dtype):
    from zhilight_amd import ops
    for (m, n, k) in [(5, 1000, 128), (70, 4099, 1024), (300, 128256, 4096)]:
        x, w, lab = _inputs(dev, m, n, k, dtype, seed=7 + m)
        ref = ops.gemm_nt(x, w)
        u = ops.lm_head_score_unfused(x, w, lab, rows_per_block=64)
        _check_rows(u, ref, lab, n, ("unfused", m, n, k, dtype))
        f = ops.lm_head_score(x, w, lab)
        assert torch.equal(u.greedy, f.greedy) and torch.equal(u.greedy_logit, f.greedy_logit) and torch.equal(u.label_logit, f.label_logit)
    # K % 128 != 0: the fused op refuses, the unfused one is checked against float64 directly.  Its logits come from the GEMV: fp32
    # sums (error far below an ulp_T, but enough to cross a rounding boundary) rounded once to T: within ONE ulp_T = 2 eps_T |y|
    m, n, k = 6, 777, 200
    x, w, lab = _inputs(dev, m, n, k, dtype, seed=99)
    with pytest.raises(ops.ZLError):
        ops.lm_head_score(x, w, lab)
    u = ops.lm_head_score_unfused(x, w, lab)
    y64 = x.double() @ w.double().t()
    eps_t = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    tol = float(y64.abs().max()) * 2 * eps_t
    lse64 = torch.logsumexp(y64, dim=1)
    assert float((u.lse.double() - lse64).abs().max()) <= tol + bound(n)
    assert float((u.greedy_logit.double() - y64.max(dim=1).values).abs().max()) <= tol
    keep = (lab != IGN).to(dev)
    ll64 = y64.gather(1, lab.to(dev).long().clamp(min=0).view(-1, 1)).view(-1)
    assert float(((u.label_logit.double() - ll64)[keep]).abs().max()) <= tol
    assert (u.label_logit[~keep] == 0).all() and (u.logprob[~keep] == 0).all()


def test_host_checks(dev):
    from zhilight_amd import ops
    x, w, lab = _inputs(dev, 8, 512, 256, torch.float16, seed=1)
    with pytest.raises(ops.ZLError):
        ops.lm_head_score(x, w.bfloat16(), lab)                  # dtype mismatch
    with pytest.raises(ops.ZLError):
        ops.lm_head_score(x[:, :128], w, lab)                    # K mismatch
    with pytest.raises(ops.ZLError):
        ops.lm_head_score(x, w, lab[:7])                         # labels: one per row
    with pytest.raises(ops.ZLError):
        ops.lm_head_score(x, w, lab.to(dev).long())              # device labels must be int32
    bad = lab.clone()
    bad[0] = 512
    with pytest.raises(ops.ZLError):
        ops.lm_head_score(x, w, bad)                             # a host label outside the vocabulary
    with pytest.raises(ops.ZLError):
        ops.lm_head_score(x.cpu(), w, lab)
    with pytest.raises(ops.ZLError):
        ops.lm_head_score(x, w, lab, workspace=torch.empty(8, device=dev))


def test_graph_capture_replays_on_new_inputs(dev):
    from zhilight_amd import ops
    m, n, k = 70, 4099, 1024
    x, w, lab = _inputs(dev, m, n, k, torch.float16, seed=5)
    x2, _, lab2 = _inputs(dev, m, n, k, torch.float16, seed=6)
    xb, lb = x.clone(), lab.to(dev)
    ws = ops.lm_head_score_workspace(m, n, dev)
    ops.lm_head_score(xb, w, lb, workspace=ws)                   # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = ops.lm_head_score(xb, w, lb, workspace=ws)
    xb.copy_(x2)
    lb.copy_(lab2.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    e = ops.lm_head_score(x2, w, lab2)
    for u, v in zip(r, e):
        assert torch.equal(u, v)


# --------------------------------------------------------------------------------------------------
# model level
# --------------------------------------------------------------------------------------------------
class AllRowsOracle(OracleModel):
    """OracleModel whose prompt pass returns the logits of EVERY row: OracleModel.prefill's composition, its last two lines over
    all rows"""

    def prefill_all(self, task, tokens):
        o, c = self.o, self.cfg
        self.w16 = getattr(self, "w16", {})
        s = len(tokens)
        h = o.embedding(np.asarray(tokens, np.int32), o.h2u(self.sd["model.embed_tokens.weight"]))
        pos = np.arange(s, dtype=np.int32)
        cs, sn = self._tables(pos)
        lens = np.full(1, self.len_buf, np.int32)
        mask = np.tril(np.ones((s, self.len_buf), np.int8))
        for i in range(c.num_layers):
            p = f"model.layers.{i}."
            xn = o.rmsnorm(h, o.h2u(self.sd[p + "input_layernorm.weight"]), c.eps)
            qkv = np.concatenate([self._lin40(xn, p + "self_attn." + n + "_proj") for n in "qkv"], axis=1)
            qkv = self._qk_norm(i, qkv)
            q, k, v = o.rope_qk_cache(cs, sn, qkv, c.num_heads, c.num_kv_heads, c.dim_head, True)
            o.copy_to_rag_buffer2(pos.reshape(1, s), lens, k.reshape(1, s, c.num_kv_heads, c.dim_head),
                                  v.reshape(1, s, c.num_kv_heads, c.dim_head), [self.kb[i][task]], [self.vb[i][task]], True)
            if self.kv_quant:
                self._quant_store(i, [task], [list(range(s))], k, v)
            att = o.mqa_rag_buffer(q.reshape(1, s, c.num_heads, c.dim_head), lens, [self.kb[i][task]], [self.vb[i][task]], mask,
                                   c.num_kv_heads, 1.0 / np.sqrt(c.dim_head), True).reshape(s, -1)
            h = o.element_add_scale(h, self._lin40(att, p + "self_attn.o_proj"), 1.0, True)
            xn = o.rmsnorm(h, o.h2u(self.sd[p + "post_attention_layernorm.weight"]), c.eps)
            act = o.silu_mul(self._lin40(xn, p + "mlp.gate_proj"), self._lin40(xn, p + "mlp.up_proj"))
            h = o.element_add_scale(h, self._lin40(act, p + "mlp.down_proj"), 1.0, True)
        xn = o.rmsnorm(h, o.h2u(self.sd["model.norm.weight"]), c.eps)
        return np.asarray(o.gemm_nt(xn, o.h2u(self.sd["lm_head.weight"]), exact=True), np.float64)


def _np(t):
    return t.detach().cpu().numpy()


def _check_against_oracle(res, row0, ref_logits, labels, n_vocab, what):
    """rows row0 .. of the result against the oracle's logits of the same rows (s, vocab) float64 -> number of rows left out of the
    arg-max comparison"""
    s = ref_logits.shape[0]
    bar = (1e-3 + 2.0 ** -11) * np.abs(ref_logits).max()
    mx = ref_logits.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(ref_logits - mx).sum(axis=1))
    lp, gr = _np(res.logprobs)[row0:row0 + s].astype(np.float64), _np(res.greedy)[row0:row0 + s]
    assert np.abs(_np(res.lse)[row0:row0 + s] - lse).max() <= bar + bound(n_vocab), what
    left = 0
    for r in range(s):
        if labels[r] != IGN:
            err = abs(lp[r] - (ref_logits[r, labels[r]] - lse[r]))
            assert err <= 2 * bar + bound(n_vocab), (what, r, err, bar)
        else:
            assert lp[r] == 0, (what, r)
        top = np.sort(ref_logits[r])[-2:]
        if top[1] - top[0] > 2 * bar:
            assert gr[r] == int(ref_logits[r].argmax()), (what, r)
        else:
            left += 1
    return left


def _same_state(model, ctx_a, ctx_b, logits_a, logits_b, tasks, decode=True):
    for name in ("tokens", "positions", "placement", "valid_lens"):
        assert torch.equal(getattr(ctx_a, name), getattr(ctx_b, name)), name
    assert ctx_a.steps_left == ctx_b.steps_left
    assert torch.equal(logits_a, logits_b)
    for t in tasks:
        assert torch.equal(ctx_a.kv[t].view(torch.uint8), ctx_b.kv[t].view(torch.uint8)), t
        if ctx_a.kv_quant:
            assert torch.equal(ctx_a.kv_scales[t], ctx_b.kv_scales[t]), t
    if decode:
        for _ in range(2):
            la, _ = model.step_greedy(ctx_a)
            lb, _ = model.step_greedy(ctx_b)
            assert torch.equal(la, lb)


def test_score_matches_oracle_and_prefill_batch(oracle, dev):
    rng, cfg, sd, model = _gptq_model(dev)
    lens, len_buf = [5, 40, 70, 17], 128
    prompts = [rng.integers(0, cfg.vocab_size, s).astype(np.int32) for s in lens]
    tp = [torch.from_numpy(p) for p in prompts]
    ctx, twin = model.new_context(4, len_buf, 0), model.new_context(4, len_buf, 0)
    res = model.score(ctx, [0, 1, 2, 3], tp)
    logits = model.prefill_batch(twin, [0, 1, 2, 3], tp)
    total = sum(lens)
    assert res.cu == [0, 5, 45, 115, 132] and res.logprobs.shape == (total,) and res.greedy.dtype == torch.int32
    assert res.logits.shape == (4, cfg.vocab_size) and res.sums.shape == (4,) and res.matches.dtype == torch.bool
    om = AllRowsOracle(oracle, cfg, sd, 128, 4, len_buf)
    left = 0
    for j, p in enumerate(prompts):
        ref = om.prefill_all(j, p)
        labels = list(p[1:]) + [IGN]
        left += _check_against_oracle(res, res.cu[j], ref, labels, cfg.vocab_size, j)
        lp = _np(res.logprobs)[res.cu[j]:res.cu[j + 1]]
        assert abs(float(res.sums[j]) - float(lp.sum(dtype=np.float32))) <= lens[j] * 2.0 ** -24 * float(np.abs(lp).sum()) + 1e-30
        gr = _np(res.greedy)[res.cu[j]:res.cu[j + 1]]
        assert bool(res.matches[j]) == bool(all(g == l for g, l in zip(gr, labels) if l != IGN))
    print("rows left out of the arg-max comparison:", left, "of", total)
    assert left <= 0.10 * total
    # 7. the state prefill_batch leaves, bit for bit, and two greedy decode steps from both
    _same_state(model, ctx, twin, res.logits, logits, range(4))


def test_scoring_tail_issues_no_host_synchronisation(dev):
    """everything score() adds behind the layer loop -- the norm, the fused launches, the per-task sums / matches -- under torch's
    synchronisation detector: a device-to-host read (an .item(), a checked segment reduction ...) raises"""
    _, cfg, _, model = _gptq_model(dev)
    lens = [5, 40, 70, 17]
    total = sum(lens)
    g = torch.Generator().manual_seed(3)
    hidden = torch.randn(total, cfg.dim_model, generator=g).half().to(dev)
    lab = torch.randint(0, cfg.vocab_size, (total,), generator=g, dtype=torch.int32)
    lab[::7] = IGN
    labels_dev = lab.to(dev)
    last_rows = torch.tensor([4, 44, 114, 131], dtype=torch.int64).to(dev)
    model._score_rows(hidden, labels_dev, lens, last_rows)               # warm: code objects loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        many = model._score_rows(hidden, labels_dev, lens, last_rows)
        one = model._score_rows(hidden, labels_dev, [total])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    lp, gr, labn = _np(many.logprobs), _np(many.greedy), lab.numpy()
    for j in range(4):
        a, b = many.cu[j], many.cu[j + 1]
        host = lp[a:b].sum(dtype=np.float32)
        assert abs(float(many.sums[j]) - float(host)) <= (b - a) * 2.0 ** -24 * float(np.abs(lp[a:b]).sum())
        kept = labn[a:b] != IGN
        assert bool(many.matches[j]) == bool((gr[a:b][kept] == labn[a:b][kept]).all())
    assert abs(float(one.sums[0]) - float(lp.sum(dtype=np.float32))) <= total * 2.0 ** -24 * float(np.abs(lp).sum())
    assert not bool(one.matches[0])
    # labels equal to the arg-max on every scored row: every task matches
    hit = many.greedy.clone()
    hit[::7] = IGN
    assert bool(model._score_rows(hidden, hit, lens, last_rows).matches.all())


def test_score_continued_one_task_and_explicit_labels(oracle, dev):
    rng, cfg, sd, model = _gptq_model(dev, seed=5)
    len_buf = 128
    p0, p1 = (rng.integers(0, cfg.vocab_size, s).astype(np.int32) for s in (70, 33))
    ctx, twin = model.new_context(2, len_buf, 0), model.new_context(2, len_buf, 0)
    for c in (ctx, twin):
        model.prefill_batch(c, [0], [torch.from_numpy(p0[:27])])
    # explicit labels: the next tokens with every third row of the continued task ignored; the fresh task's last row labelled too
    lab0 = [int(t) for t in p0[28:]] + [IGN]
    lab0 = [IGN if r % 3 == 0 else l for r, l in enumerate(lab0)]
    lab1 = [int(t) for t in p1[1:]] + [int(p1[0])]
    args = ([0, 1], [torch.from_numpy(p0[27:]), torch.from_numpy(p1)])
    res = model.score(ctx, *args, pos0=[27, 0], labels=[torch.tensor(lab0), lab1])
    logits = model.prefill_batch(twin, *args, pos0=[27, 0])
    om = AllRowsOracle(oracle, cfg, sd, 128, 2, len_buf)
    ref0, ref1 = om.prefill_all(0, p0), om.prefill_all(1, p1)
    left = _check_against_oracle(res, 0, ref0[27:], lab0, cfg.vocab_size, "continued")
    left += _check_against_oracle(res, 43, ref1, lab1, cfg.vocab_size, "fresh")
    assert left <= 0.10 * 76
    lp, gr = _np(res.logprobs), _np(res.greedy)
    for j, (a, b, lab) in enumerate(((0, 43, lab0), (43, 76, lab1))):
        kept = np.array([l != IGN for l in lab])
        assert (lp[a:b][~kept] == 0).all()
        host = lp[a:b][kept].sum(dtype=np.float32)
        assert abs(float(res.sums[j]) - float(host)) <= (b - a) * 2.0 ** -24 * float(np.abs(lp[a:b]).sum())
        assert bool(res.matches[j]) == bool((gr[a:b][kept] == np.array(lab)[kept]).all())
    _same_state(model, ctx, twin, res.logits, logits, range(2))
    # labels equal to the arg-max of every kept row: matches is True
    ctx2 = model.new_context(1, len_buf, 0)
    first = model.score(ctx2, [0], [torch.from_numpy(p1)])
    gl = [int(g) for g in _np(first.greedy)]
    gl[3] = IGN
    ctx3, twin3 = model.new_context(1, len_buf, 0), model.new_context(1, len_buf, 0)
    one = model.score(ctx3, [0], [torch.from_numpy(p1)], labels=[gl])           # a one-task call
    l1 = model.prefill_batch(twin3, [0], [torch.from_numpy(p1)])
    assert bool(one.matches[0])
    assert torch.equal(one.lse, first.lse) and torch.equal(one.greedy, first.greedy)
    # (every row is checked; the share of near-tie rows is a property of the oracle's logits and was bounded over the 76 rows above)
    _check_against_oracle(one, 0, ref1, gl, cfg.vocab_size, "one task")
    _same_state(model, ctx3, twin3, one.logits, l1, range(1))
    gl[7] = (gl[7] + 1) % cfg.vocab_size                                        # one scored row whose label is not its arg-max
    assert not bool(model.score(model.new_context(1, len_buf, 0), [0], [torch.from_numpy(p1)], labels=[gl]).matches[0])


def _ulp_t(v, dtype):
    e = np.floor(np.log2(max(abs(v), 2.0 ** -14)))
    return 2.0 ** (e - (7 if dtype == torch.bfloat16 else 10))


def test_score_int8_cache(oracle, dev):
    rng, cfg, sd, model = _gptq_model(dev, seed=21)
    lens, len_buf = [45, 17, 64], 128
    prompts = [rng.integers(0, cfg.vocab_size, s).astype(np.int32) for s in lens]
    tp = [torch.from_numpy(p) for p in prompts]
    ctx = model.new_context(3, len_buf, 0, kv_cache_dtype="int8")
    twin = model.new_context(3, len_buf, 0, kv_cache_dtype="int8")
    res = model.score(ctx, [0, 1, 2], tp)
    logits = model.prefill_batch(twin, [0, 1, 2], tp)
    om = AllRowsOracle(oracle, cfg, sd, 128, 3, len_buf, kv_quant=True)
    left = 0
    for j, p in enumerate(prompts):
        left += _check_against_oracle(res, res.cu[j], om.prefill_all(j, p), list(p[1:]) + [IGN], cfg.vocab_size, ("int8", j))
    assert left <= 0.10 * sum(lens)
    _same_state(model, ctx, twin, res.logits, logits, range(3))
    # continued prompts read from the cache (kv_history="cache"): no all-row oracle; state equivalence and last-row consistency
    more = [torch.from_numpy(rng.integers(0, cfg.vocab_size, s).astype(np.int32)) for s in (20, 9)]
    pos0 = [int(ctx.positions[0]), int(ctx.positions[2])]
    res2 = model.score(ctx, [0, 2], more, pos0=pos0, kv_history="cache")
    logits2 = model.prefill_batch(twin, [0, 2], more, pos0=pos0, kv_history="cache")
    for j, task in enumerate([0, 2]):
        last = res2.cu[j + 1] - 1
        lg = res2.logits[j].double().cpu().numpy()
        lse64 = lg.max() + np.log(np.exp(lg - lg.max()).sum())
        u = _ulp_t(np.abs(lg).max(), res2.logits.dtype)
        assert abs(float(res2.lse[last]) - lse64) <= bound(cfg.vocab_size) + 2 * u, j
        top = np.sort(lg)[-2:]
        if top[1] - top[0] > 2 * u:
            assert int(res2.greedy[last]) == int(ctx.tokens[task]), j
    _same_state(model, ctx, twin, res2.logits, logits2, range(3))
    from zhilight_amd import ops
    with pytest.raises(ops.ZLError):
        model.score(ctx, [1], [more[1]], pos0=[17])              # a continued prompt on the INT8 cache without kv_history="cache"


def test_score_refusals(dev):
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, QuantConfig
    from test_gpu_model import _ThreadTP
    rng, cfg, sd, model = _gptq_model(dev)
    ctx = model.new_context(3, 64, 0)
    p = torch.arange(10, dtype=torch.int32)
    for tasks, prompts, pos0, labels in (([0, 0], [p, p], None, None),                          # duplicate tasks
                                         ([0, 1], [p, p[:0]], None, None),                      # empty prompt
                                         ([0, 3], [p, p], None, None),                          # task out of range
                                         ([0, 1], [p, torch.zeros(64, dtype=torch.int32)], None, None),   # does not fit
                                         ([0, 1], [p, p], [0, 60], None),                       # continued past the buffer
                                         ([0, 1], [p, p], None, [list(range(10))]),             # one label sequence per task
                                         ([0, 1], [p, p], None, [list(range(10)), list(range(9))]),      # label length mismatch
                                         ([0, 1], [p, p], None, [list(range(10)), [cfg.vocab_size] * 10]),   # outside the vocabulary
                                         ([0, 1], [p, p], None, [list(range(10)), [-5] * 10])):
        with pytest.raises(ops.ZLError):
            model.score(ctx, tasks, prompts, pos0, labels=labels)
    with pytest.raises(ops.ZLError):
        model.score(ctx, [0], [p], kv_history="nope")
    assert ctx.positions.tolist() == [0, 0, 0] and ctx.tokens.tolist() == [0, 0, 0] and ctx.steps_left == model.new_context(3, 64, 0).steps_left
    tp_model = LLaMA(cfg, QuantConfig(5, 128), dev, tp=_ThreadTP(2).view(0)).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    with pytest.raises(ops.ZLError, match="tensor parallelism is not supported"):
        tp_model.score(tp_model.new_context(1, 64, 0), [0], [p])


def test_score_never_materialises_the_logits(dev):
    """2048 rows x 128 256 columns: a logits matrix would be 525 MB; the call may grow the peak by less than a quarter of it"""
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig(num_layers=2, dim_model=1024, num_heads=8, dim_head=128, dim_ff=2048, vocab_size=128256, num_kv_heads=2,
                      eps=1e-5, rope_theta=5e5)
    model = LLaMA(cfg, QuantConfig(0, 0), dev).init_random(seed=2)
    model.token_embedding.mul_(0.1)
    lens = [1024, 512, 500, 12]
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab_size, (s,), generator=g, dtype=torch.int32) for s in lens]
    ctx = model.new_context(4, 1088, 0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = model.score(ctx, [0, 1, 2, 3], prompts)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    rows = sum(lens)
    print("peak growth MB", growth / 1e6, "logits would take", rows * cfg.vocab_size * 2 / 1e6)
    assert rows == 2048 and growth < rows * cfg.vocab_size * 2 // 4
    assert torch.isfinite(res.lse).all() and torch.isfinite(res.logprobs).all() and res.logprobs.shape == (rows,)
    assert ctx.positions.tolist() == lens
