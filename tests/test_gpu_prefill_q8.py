"""Prompts that continue rows of the INT8 K/V cache: zl_prefill_attn_varlen_q8 / ops.prefill_attention_varlen_q8 (history dequantised
where the kernel stages its K / V tiles) against the reference's two-step form built from the kernels that were there before
(dequant_group into a buffer + the fp16-cache varlen attention: bit for bit) and against the fp64 oracle, and the kv_history="cache"
keyword of LLaMA.prefill_batch / LLaMA.prefill against an fp16 context that is handed the dequantised history (bit for bit)."""
import numpy as np
import pytest
import torch

from test_gpu_prefill_batch import _bits_of, _dev, _gptq_model, _host_bits

pytestmark = pytest.mark.gpu

LENS = [1, 17, 64, 130, 200]          # a one-row "decode-like" task, a fresh one, a history that ends on a tile boundary,
POS0 = [300, 0, 64, 45, 1000]         # one that ends inside a tile, a long one
D = 128


def _tdt(dtype):
    return torch.bfloat16 if dtype else torch.float16


def _deq_numpy(oracle, codes, scales, dtype):
    """rn_T((code - 128) * scale) with the product rounded to fp32 first: the statement of int8_op::dequant_group, in numpy; bits"""
    prod = (codes.astype(np.float32) - np.float32(128.0)) * scales.astype(np.float32)[..., None]
    assert prod.dtype == np.float32
    return oracle.f32_to_bf16(prod) if dtype else oracle.h2u(prod.astype(np.float16))


class _Case:
    """five tasks' INT8 caches (filled by quant_copy_to_rag_buffer up to pos0, arbitrary behind it), their new rows and the two-step
    expectation's fp16 / bf16 buffers"""

    def __init__(self, oracle, dev, h, hkv, dtype):
        from zhilight_amd import ops
        self.h, self.hkv, self.dtype, self.scale = h, hkv, dtype, 1.0 / np.sqrt(D)
        rng = np.random.default_rng(100 * h + dtype)
        total = sum(LENS)
        self.len_bufs = [(p0 + s + 63) // 64 * 64 + 32 * i for i, (s, p0) in enumerate(zip(LENS, POS0))]     # ragged
        self.q = _bits_of(oracle, rng.standard_normal((total, h, D)) * 1.5, dtype)
        self.k_new = _bits_of(oracle, rng.standard_normal((total, hkv, D)), dtype)
        self.v_new = _bits_of(oracle, rng.standard_normal((total, hkv, D)), dtype)
        self.qd, self.knd, self.vnd = (_dev(a, dev, dtype) for a in (self.q, self.k_new, self.v_new))
        self.kc, self.vc, self.ks, self.vs = [], [], [], []
        for lb, p0 in zip(self.len_bufs, POS0):
            kc = torch.from_numpy(rng.integers(0, 256, (lb, hkv, D)).astype(np.uint8)).to(dev)
            vc = torch.from_numpy(rng.integers(0, 256, (lb, hkv, D)).astype(np.uint8)).to(dev)
            ks = torch.from_numpy((rng.random((lb, hkv)) * 0.03 + 0.005).astype(np.float32)).to(dev)
            vs = torch.from_numpy((rng.random((lb, hkv)) * 0.03 + 0.005).astype(np.float32)).to(dev)
            if p0:
                # Gaussian rows of differing size, so that the scales differ from row to row
                amp = np.exp(rng.standard_normal((p0, hkv, 1)))
                kh = _dev(_bits_of(oracle, rng.standard_normal((p0, hkv, D)) * amp, dtype), dev, dtype)
                vh = _dev(_bits_of(oracle, rng.standard_normal((p0, hkv, D)) * amp, dtype), dev, dtype)
                ops.quant_copy_to_rag_buffer(torch.arange(p0, dtype=torch.int32, device=dev),
                                             torch.tensor([lb], dtype=torch.int32, device=dev), kh, vh, ops.make_ptr_table([kc]),
                                             ops.make_ptr_table([vc]), ops.make_ptr_table([ks]), ops.make_ptr_table([vs]), len_q=p0)
            self.kc.append(kc); self.vc.append(vc); self.ks.append(ks); self.vs.append(vs)
        torch.cuda.synchronize()
        self.tabs = [ops.make_ptr_table(x) for x in (self.kc, self.vc, self.ks, self.vs)]
        self.plan = ops.prefill_varlen_plan(LENS, POS0, self.len_bufs, dev)

    def two_step_buffers(self, oracle, dev):
        """the reference's fall-back: dequant_group of the history into a fresh buffer (the kernel that was there before, first
        pinned to the numpy statement), the call's own rows behind it.  Returns device buffers and their host bits."""
        from zhilight_amd import ops
        cu, dtype = self.plan.cu, self.dtype
        kd, vd, kb, vb = [], [], [], []
        for i, (s, p0, lb) in enumerate(zip(LENS, POS0, self.len_bufs)):
            bufs = []
            for codes, scales, new in ((self.kc[i], self.ks[i], self.knd), (self.vc[i], self.vs[i], self.vnd)):
                buf = torch.zeros((lb, self.hkv, D), dtype=_tdt(dtype), device=dev)
                if p0:
                    hist = ops.dequant_group(codes[:p0], scales[:p0], 128, _tdt(dtype))
                    want = _deq_numpy(oracle, codes[:p0].cpu().numpy(), scales[:p0].cpu().numpy(), dtype)
                    assert np.array_equal(_host_bits(hist), want), i
                    buf[:p0] = hist
                buf[p0:p0 + s] = new[cu[i]:cu[i + 1]]
                bufs.append(buf)
            kd.append(bufs[0]); vd.append(bufs[1]); kb.append(_host_bits(bufs[0])); vb.append(_host_bits(bufs[1]))
        return kd, vd, kb, vb

    def run(self, groups, tables=True):
        from zhilight_amd import ops
        cache = self.tabs if tables else (self.kc, self.vc, self.ks, self.vs)
        return ops.prefill_attention_varlen_q8(self.qd, LENS, POS0, self.knd, self.vnd, *cache, self.len_bufs, self.hkv, self.scale,
                                               groups=groups, plan=self.plan)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("h,hkv", [(32, 8), (4, 4)])
def test_q8_history_bit_identical_to_dequant_plus_varlen_and_oracle(oracle, dev, h, hkv, dtype):
    """1. bit identity with dequant_group + prefill_attention_varlen; 2. the fp64 oracle on numpy-dequantised buffers at the bars of
    the fp16-cache kernel (2e-3 fp16, 1.5e-2 bf16 of max|ref|); 3. nothing at or beyond pos0 is read from the cache."""
    from zhilight_amd import ops
    case = _Case(oracle, dev, h, hkv, dtype)
    kd, vd, kb, vb = case.two_step_buffers(oracle, dev)
    k_tab, v_tab = ops.make_ptr_table(kd), ops.make_ptr_table(vd)
    cu = case.plan.cu
    # the oracle's buffers are formed without the repository's kernels: history in numpy, own rows as given
    refs = []
    for i, (s, p0, lb) in enumerate(zip(LENS, POS0, case.len_bufs)):
        nk, nv = np.zeros((lb, hkv, D), np.uint16), np.zeros((lb, hkv, D), np.uint16)
        if p0:
            nk[:p0] = _deq_numpy(oracle, case.kc[i][:p0].cpu().numpy(), case.ks[i][:p0].cpu().numpy(), dtype)
            nv[:p0] = _deq_numpy(oracle, case.vc[i][:p0].cpu().numpy(), case.vs[i][:p0].cpu().numpy(), dtype)
        nk[p0:p0 + s], nv[p0:p0 + s] = case.k_new[cu[i]:cu[i + 1]], case.v_new[cu[i]:cu[i + 1]]
        mask = (np.arange(lb)[None, :] <= (p0 + np.arange(s))[:, None]).astype(np.int8)
        refs.append(oracle.mqa_rag_buffer(case.q[cu[i]:cu[i + 1]][None], np.array([lb], np.int32), [nk], [nv], mask, hkv, case.scale,
                                          True, dtype=dtype, exact=True)[0])
    bar = 1.5e-2 if dtype else 2e-3
    first = {}
    for g in (1, 2, 4):
        want = _host_bits(ops.prefill_attention_varlen(case.qd, LENS, POS0, k_tab, v_tab, case.len_bufs, hkv, case.scale, True, groups=g,
                                                       plan=case.plan))
        got = _host_bits(case.run(g))
        first[g] = got
        for i in range(len(LENS)):
            a, b = cu[i], cu[i + 1]
            differ = int((got[a:b] != want[a:b]).sum())
            gf = oracle.to_f32(got[a:b], dtype).astype(np.float64)
            err = np.abs(gf - refs[i]).max() / np.abs(refs[i]).max()
            print(f"q8 h={h} hkv={hkv} dtype={dtype} groups={g} task={i}: {differ} differing values, oracle error {err:.3e} (bar {bar})")
            assert differ == 0, (g, i, differ)
            assert np.isfinite(gf).all(), (g, i)
            assert err <= bar, (g, i, err)
    # per-task tensors instead of pointer tables: the same launch
    assert np.array_equal(_host_bits(case.run(1, tables=False)), first[1])
    # 3. everything at or beyond pos0 -- the slots of the call's own rows and never-written memory -- made poisonous
    for i, p0 in enumerate(POS0):
        case.kc[i][p0:] = 255
        case.vc[i][p0:] = 255
        case.ks[i][p0:] = float("nan")
        case.vs[i][p0:] = float("nan")
    torch.cuda.synchronize()
    for g in (1, 2, 4):
        again = _host_bits(case.run(g))
        assert np.isfinite(oracle.to_f32(again, dtype)).all(), g
        assert np.array_equal(again, first[g]), g


def test_q8_host_checks(oracle, dev):
    from zhilight_amd import ops
    case = _Case(oracle, dev, 4, 4, 0)
    args = lambda **kw: dict(dict(q=case.qd, lens=LENS, pos0=POS0, k_new=case.knd, v_new=case.vnd, k_addrs=case.tabs[0],
                                  v_addrs=case.tabs[1], ks_addrs=case.tabs[2], vs_addrs=case.tabs[3], buf_lens=case.len_bufs,
                                  num_kv_heads=4, scale=case.scale), **kw)
    ops.prefill_attention_varlen_q8(**args())
    with pytest.raises(ops.ZLError):                          # wrong row count
        ops.prefill_attention_varlen_q8(**args(q=case.qd[1:]))
    with pytest.raises(ops.ZLError):
        ops.prefill_attention_varlen_q8(**args(k_new=case.knd[1:]))
    with pytest.raises(ops.ZLError):                          # a chunk that does not fit its buffer
        ops.prefill_attention_varlen_q8(**args(buf_lens=[64] * 5))
    with pytest.raises(ops.ZLError):                          # d != 128
        ops.prefill_attention_varlen_q8(**args(q=case.qd.view(-1, 8, 64), k_new=case.knd.view(-1, 8, 64), v_new=case.vnd.view(-1, 8, 64),
                                               num_kv_heads=8))
    with pytest.raises(ops.ZLError):                          # a code tensor that is not INT8
        ops.prefill_attention_varlen_q8(**args(k_addrs=[c.to(torch.float16) for c in case.kc], v_addrs=case.vc, ks_addrs=case.ks,
                                               vs_addrs=case.vs))
    with pytest.raises(ops.ZLError):                          # scales of another type
        ops.prefill_attention_varlen_q8(**args(k_addrs=case.kc, v_addrs=case.vc, ks_addrs=[s.double() for s in case.ks],
                                               vs_addrs=case.vs))
    with pytest.raises(ops.ZLError):                          # a table of another type
        ops.prefill_attention_varlen_q8(**args(k_addrs=case.tabs[0].to(torch.int32)))
    with pytest.raises(ops.ZLError):
        ops.prefill_attention_varlen_q8(**args(q=case.qd.float()))
    with pytest.raises(ops.ZLError):
        ops.dequant_group(case.kc[0].to(torch.int32), case.ks[0])
    with pytest.raises(ops.ZLError):
        ops.dequant_group(case.kc[0], case.ks[0][1:])


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: an INT8 context with kv_history="cache" against an fp16 context that is handed the dequantised history
# ---------------------------------------------------------------------------------------------------------------------------------
def _load_dequantised_history(ctx_a, ctx_b, pos0s, layers):
    """rows < pos0 of every task's fp16 buffers in ctx_b <- numpy rn_fp16((code - 128) * scale) of ctx_a's INT8 cache"""
    for j, p0 in enumerate(pos0s):
        if not p0:
            continue
        for li in range(layers):
            for kv in (0, 1):
                codes = ctx_a.kv[j][li, kv, :p0].cpu().numpy()
                scales = ctx_a.kv_scales[j][li, kv, :p0].cpu().numpy()
                prod = (codes.astype(np.float32) - np.float32(128.0)) * scales[..., None]
                ctx_b.kv[j][li, kv, :p0] = torch.from_numpy(prod.astype(np.float16)).to(ctx_b.kv[j].device)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def test_prefill_batch_second_turn_on_int8_cache_matches_fp16_context_with_dequantised_history(dev):
    from zhilight_amd import ops
    rng, cfg, sd, model = _gptq_model(dev, seed=21)
    len_buf = 128
    first = [torch.from_numpy(rng.integers(0, cfg.vocab_size, s).astype(np.int32)) for s in (45, 17, 64)]
    second = [torch.from_numpy(rng.integers(0, cfg.vocab_size, s).astype(np.int32)) for s in (20, 33, 1)]
    pos0 = [45, 0, 64]                                        # task 1 starts over: fresh and continued tasks in one call
    ctx_a = model.new_context(3, len_buf, 0, kv_cache_dtype="int8")
    model.prefill_batch(ctx_a, [0, 1, 2], first)
    ctx_b = model.new_context(3, len_buf, 0)
    _load_dequantised_history(ctx_a, ctx_b, pos0, cfg.num_layers)
    la = model.prefill_batch(ctx_a, [0, 1, 2], second, pos0=pos0, kv_history="cache")
    lb = model.prefill_batch(ctx_b, [0, 1, 2], second, pos0=pos0)
    assert not ctx_a.unquant_kv
    assert torch.isfinite(la.float()).all()
    assert _bits_equal(la, lb), (la.float() - lb.float()).abs().max().item()
    assert ctx_a.tokens.tolist() == ctx_b.tokens.tolist() == la.argmax(dim=1).tolist()
    ends = [p + int(s.numel()) for p, s in zip(pos0, second)]
    assert ctx_a.positions.tolist() == ends and ctx_a.placement.tolist() == ends
    assert ctx_a.valid_lens.tolist() == [e + 1 for e in ends]
    assert ctx_a.steps_left == len_buf - max(ends)
    # the call's rows went to the cache as codes of exactly the rows the fp16 context holds
    for j, (p0, e) in enumerate(zip(pos0, ends)):
        for li in range(cfg.num_layers):
            for kv in (0, 1):
                rows = ctx_b.kv[j][li, kv, p0:e].contiguous()
                codes, scales = ops.quant_calc_scale_zp(rows.view(-1, cfg.dim_head), q_zero=128)
                assert torch.equal(ctx_a.kv[j][li, kv, p0:e].reshape(-1, cfg.dim_head), codes), (j, li, kv)
                assert torch.equal(ctx_a.kv_scales[j][li, kv, p0:e].reshape(-1), scales), (j, li, kv)
    for step in range(3):
        model.step_greedy(ctx_a)
        assert ctx_a.positions.tolist() == [e + step + 1 for e in ends]
        assert ctx_a.valid_lens.tolist() == [e + step + 2 for e in ends]


def test_chunked_prompt_on_int8_cache_without_temporaries(dev, monkeypatch):
    rng, cfg, sd, model = _gptq_model(dev, seed=23)
    len_buf, chunk = 128, 16
    prompt = torch.from_numpy(rng.integers(0, cfg.vocab_size, 45).astype(np.int32))
    ctx_a = model.new_context(1, len_buf, 0, kv_cache_dtype="int8")
    ctx_b = model.new_context(1, len_buf, 0)
    for p0 in range(0, 45, chunk):
        piece = prompt[p0:p0 + chunk]
        _load_dequantised_history(ctx_a, ctx_b, [p0], cfg.num_layers)
        la = model.prefill_batch(ctx_a, [0], [piece], pos0=[p0], kv_history="cache")
        lb = model.prefill_batch(ctx_b, [0], [piece], pos0=[p0])
        assert _bits_equal(la, lb), (p0, (la.float() - lb.float()).abs().max().item())
        assert ctx_a.tokens.tolist() == ctx_b.tokens.tolist()
    assert ctx_a.positions.tolist() == [45] and ctx_a.valid_lens.tolist() == [46]

    # prefill(chunk=..., kv_history="cache"): the same pieces, and the prompt's temporaries never exist
    inner = model._prefill_rows
    seen = []

    def watch(ctx, *a, **kw):
        seen.append(dict(ctx.unquant_kv))
        return inner(ctx, *a, **kw)

    monkeypatch.setattr(model, "_prefill_rows", watch)
    ctx_c = model.new_context(1, len_buf, 0, kv_cache_dtype="int8")
    lc = model.prefill(ctx_c, 0, prompt, chunk=chunk, kv_history="cache")
    assert len(seen) == 3 and all(not u for u in seen) and not ctx_c.unquant_kv
    assert _bits_equal(lc, la)
    assert ctx_c.tokens.tolist() == ctx_a.tokens.tolist() and ctx_c.positions.tolist() == [45]
    assert torch.equal(ctx_c.kv[0][:, :, :45], ctx_a.kv[0][:, :, :45])
    assert torch.equal(ctx_c.kv_scales[0][:, :, :45], ctx_a.kv_scales[0][:, :, :45])
    # the default route is what it was: temporaries for the duration of the call, released after it
    del seen[:]
    ctx_d = model.new_context(1, len_buf, 0, kv_cache_dtype="int8")
    ld = model.prefill(ctx_d, 0, prompt, chunk=chunk)
    assert len(seen) == 3 and all(0 in u for u in seen) and not ctx_d.unquant_kv
    assert torch.isfinite(ld.float()).all()


def test_kv_history_defaults_unchanged(dev):
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    rng, cfg, sd, model = _gptq_model(dev, seed=25)
    p = torch.from_numpy(rng.integers(0, cfg.vocab_size, 24).astype(np.int32))
    ctx = model.new_context(2, 64, 0, kv_cache_dtype="int8")
    model.prefill_batch(ctx, [0, 1], [p[:10], p[:7]])
    state = (ctx.positions.tolist(), ctx.tokens.tolist())
    with pytest.raises(ops.ZLError):                          # without the keyword the refusals stand
        model.prefill_batch(ctx, [0, 1], [p[10:14], p[:4]], pos0=[10, 0])
    with pytest.raises(ops.ZLError):
        model._encode_prompt(ctx, 0, p[10:14], 10)
    with pytest.raises(ops.ZLError):                          # any other value of the keyword
        model.prefill_batch(ctx, [0, 1], [p[10:14], p[:4]], pos0=[10, 0], kv_history="dequant")
    with pytest.raises(ops.ZLError):
        model.prefill(ctx, 0, p, chunk=8, kv_history=True)
    assert (ctx.positions.tolist(), ctx.tokens.tolist()) == state
    # an fp16 context has one route: the keyword changes nothing
    c1, c2 = model.new_context(2, 64, 0), model.new_context(2, 64, 0)
    for c, kw in ((c1, {}), (c2, {"kv_history": "cache"})):
        model.prefill_batch(c, [0, 1], [p[:10], p[:7]], **kw)
    l1 = model.prefill_batch(c1, [0, 1], [p[10:24], p[7:9]], pos0=[10, 7])
    l2 = model.prefill_batch(c2, [0, 1], [p[10:24], p[7:9]], pos0=[10, 7], kv_history="cache")
    assert _bits_equal(l1, l2) and c1.tokens.tolist() == c2.tokens.tolist()
    assert _bits_equal(model.prefill(model.new_context(1, 64, 0), 0, p, chunk=8),
                       model.prefill(model.new_context(1, 64, 0), 0, p, chunk=8, kv_history="cache"))
    # head size 64: the mask-form attention would read a chunk's own rows as codes -- refused before anything is touched
    cfg64 = ModelConfig.minicpm_2b()
    cfg64.num_layers = 2
    m64 = LLaMA(cfg64, QuantConfig(0, 0), dev).init_random(seed=3)
    ctx64 = m64.new_context(2, 64, 0, kv_cache_dtype="int8")
    p64 = torch.randint(0, cfg64.vocab_size, (12,), dtype=torch.int32)
    for call in (lambda: m64.prefill_batch(ctx64, [0, 1], [p64, p64[:5]], kv_history="cache"),
                 lambda: m64.prefill_batch(ctx64, [0], [p64], pos0=[3], kv_history="cache"),
                 lambda: m64.prefill(ctx64, 0, p64, chunk=4, kv_history="cache")):
        with pytest.raises(ops.ZLError):
            call()
    assert ctx64.positions.tolist() == [0, 0] and ctx64.tokens.tolist() == [0, 0]
