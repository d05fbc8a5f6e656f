"""Several prompts in one pass: the varlen prompt attention (zl_prefill_attn_varlen, ops.prefill_attention_varlen) against the
one-task launch (bit-identical) and the oracle's causal attention, and LLaMA.prefill_batch against the oracle composition per task
(fresh and continued prompts, INT8 KV cache, head size 64, TP = 2, refusals)."""
import numpy as np
import pytest
import torch

from test_gpu_model import OracleModel, _ThreadTP, _hf_state, _run_ranks

pytestmark = pytest.mark.gpu

LENS = [1, 63, 64, 65, 200]
POS0 = [0, 0, 37, 0, 100]


def _bits_of(oracle, x, dtype):
    return oracle.f32_to_bf16(x.astype(np.float32)) if dtype else oracle.h2u(x.astype(np.float16))


def _dev(bits, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16 if dtype else torch.float16)


def _host_bits(t):
    return t.detach().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("h,hkv", [(8, 2), (32, 8)])
def test_prefill_attention_varlen_matches_one_task_launch_and_oracle(oracle, dev, h, hkv, dtype, bshd):
    from zhilight_amd import ops
    rng = np.random.default_rng(h + 2 * dtype + int(bshd))
    d, scale = 128, 1.0 / np.sqrt(128)
    nan = np.uint16(0x7FC0 if dtype else 0x7E00)
    total = sum(LENS)
    q = _bits_of(oracle, rng.standard_normal((total, h, d)) * 1.5, dtype)
    kbs, vbs, kds, vds, len_bufs = [], [], [], [], []
    for s, p0 in zip(LENS, POS0):
        lb = (p0 + s + 63) // 64 * 64 + 64
        kb = _bits_of(oracle, rng.standard_normal((lb, hkv, d)), dtype)
        vb = _bits_of(oracle, rng.standard_normal((lb, hkv, d)), dtype)
        kd, vd = kb.copy(), vb.copy()
        kd[p0 + s:], vd[p0 + s:] = nan, nan                   # behind the task's visible keys: must not leak
        if not bshd:
            kb, vb, kd, vd = (np.ascontiguousarray(a.transpose(1, 0, 2)) for a in (kb, vb, kd, vd))
        kbs.append(kb); vbs.append(vb); kds.append(_dev(kd, dev, dtype)); vds.append(_dev(vd, dev, dtype)); len_bufs.append(lb)
    qd = _dev(q, dev, dtype)
    k_tab, v_tab = ops.make_ptr_table(kds), ops.make_ptr_table(vds)
    plan = ops.prefill_varlen_plan(LENS, POS0, len_bufs, dev)
    cu = plan.cu
    refs = []
    for i, (s, p0) in enumerate(zip(LENS, POS0)):
        mask = (np.arange(len_bufs[i])[None, :] <= (p0 + np.arange(s))[:, None]).astype(np.int8)
        refs.append(oracle.mqa_rag_buffer(q[cu[i]:cu[i + 1]][None], np.array([len_bufs[i]], np.int32), [kbs[i]], [vbs[i]], mask,
                                          hkv, scale, bshd, dtype=dtype, exact=True)[0])
    bar = 1.5e-2 if dtype else 2e-3
    for g in (1, 2, 4):
        out = ops.prefill_attention_varlen(qd, LENS, POS0, k_tab, v_tab, len_bufs, hkv, scale, bshd, groups=g, plan=plan)
        got = _host_bits(out)
        for i, (s, p0) in enumerate(zip(LENS, POS0)):
            alone = ops.prefill_attention(qd[cu[i]:cu[i + 1]].contiguous(), kds[i], vds[i], p0, hkv, scale, bshd, groups=g)
            assert np.array_equal(got[cu[i]:cu[i + 1]], _host_bits(alone)), (g, i)
            gf = oracle.to_f32(got[cu[i]:cu[i + 1]], dtype).astype(np.float64)
            assert np.isfinite(gf).all(), (g, i)
            err = np.abs(gf - refs[i]).max() / np.abs(refs[i]).max()
            assert err <= bar, (g, i, err)
    # the wrapper's host checks: q rows against the lengths, a chunk that does not fit its buffer
    with pytest.raises(ops.ZLError):
        ops.prefill_attention_varlen(qd[1:], LENS, POS0, k_tab, v_tab, len_bufs, hkv, scale, bshd)
    with pytest.raises(ops.ZLError):
        ops.prefill_attention_varlen(qd, LENS, POS0, k_tab, v_tab, [64] * 5, hkv, scale, bshd)


def _gptq_model(dev, seed=3, rope=True):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    rng = np.random.default_rng(seed)
    kw = dict(rope_scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                            "original_max_position_embeddings": 8192}) if rope else {}
    cfg = ModelConfig(num_layers=2, dim_model=1024, num_heads=8, dim_head=128, dim_ff=2048, vocab_size=512, num_kv_heads=2,
                      eps=1e-5, rope_theta=5e5, **kw)
    sd = _hf_state(rng, cfg, 128)
    model = LLaMA(cfg, QuantConfig(5, 128), dev).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return rng, cfg, sd, model


def _close(got, ref, rel):
    scale = np.abs(ref).max()
    return np.abs(got - ref).max() <= rel * scale + 2.0 ** -11 * scale, np.abs(got - ref).max() / scale


def test_prefill_batch_matches_oracle_and_decodes(oracle, dev):
    rng, cfg, sd, model = _gptq_model(dev)
    lens, len_buf = [5, 40, 70, 17], 128
    prompts = [rng.integers(0, cfg.vocab_size, s).astype(np.int32) for s in lens]
    ctx = model.new_context(4, len_buf, 0)
    om = OracleModel(oracle, cfg, sd, 128, 4, len_buf)
    logits = model.prefill_batch(ctx, [0, 1, 2, 3], [torch.from_numpy(p) for p in prompts])
    assert logits.shape == (4, cfg.vocab_size)
    got = logits.float().cpu().numpy().astype(np.float64)
    refs = [om.prefill(j, p)[0] for j, p in enumerate(prompts)]
    for j, s in enumerate(lens):
        ok, err = _close(got[j], refs[j], 1e-3)
        assert ok, (j, err)
        for li in range(cfg.num_layers):
            for kv, ob in ((0, om.kb), (1, om.vb)):
                g = ctx.kv[j][li, kv].cpu().numpy()[:s].astype(np.float64)
                r = oracle.u2h(ob[li][j][:s]).astype(np.float64)
                assert np.abs(g - r).max() <= 2.0 ** -9 * np.abs(r).max(), (j, li, kv)
    assert ctx.positions.tolist() == lens and ctx.placement.tolist() == lens
    assert ctx.valid_lens.tolist() == [s + 1 for s in lens]
    assert ctx.steps_left == len_buf - max(lens)
    assert ctx.tokens.tolist() == logits.argmax(dim=1).tolist()
    # two greedy decode steps over all four tasks continue from the batched prompt state
    tok = np.array([int(r.argmax()) for r in refs], np.int32)
    ctx.tokens.copy_(torch.from_numpy(tok))
    for step in range(2):
        lg = model.encode(ctx).float().cpu().numpy().astype(np.float64)
        pos = [s + step for s in lens]
        ex, _ = om.step(tok, pos, flavour="E", commit=False)
        rf, _ = om.step(tok, pos, flavour="R")
        sc = np.abs(rf).max()
        assert np.abs(lg - ex).max() <= 1e-3 * sc + 2.0 ** -11 * sc, (step, np.abs(lg - ex).max() / sc)
        assert np.abs(lg - rf).max() <= 3e-3 * sc, (step, np.abs(lg - rf).max() / sc)
        tok = rf.argmax(axis=1).astype(np.int32)
        model.advance(ctx, torch.from_numpy(tok).to(dev))


def test_prefill_batch_continued_prompt_with_fresh_ones(oracle, dev):
    rng, cfg, sd, model = _gptq_model(dev, seed=5)
    len_buf = 128
    p0, p1, p2 = (rng.integers(0, cfg.vocab_size, s).astype(np.int32) for s in (70, 33, 9))
    om = OracleModel(oracle, cfg, sd, 128, 3, len_buf)
    refs = {0: om.prefill(0, p0)[0], 1: om.prefill(1, p1)[0], 2: om.prefill(2, p2)[0]}
    ctx = model.new_context(3, len_buf, 0)
    model.prefill(ctx, 0, torch.from_numpy(p0[:27]))
    # arbitrary task order: the picks and counters are scattered to the right tasks
    logits = model.prefill_batch(ctx, [2, 0, 1], [torch.from_numpy(p2), torch.from_numpy(p0[27:]), torch.from_numpy(p1)],
                                 pos0=[0, 27, 0])
    got = logits.float().cpu().numpy().astype(np.float64)
    for row, task in enumerate([2, 0, 1]):
        ok, err = _close(got[row], refs[task], 1e-3)
        assert ok, (task, err)
    assert ctx.positions.tolist() == [70, 33, 9] and ctx.valid_lens.tolist() == [71, 34, 10]
    assert ctx.tokens.tolist() == [int(logits[1].argmax()), int(logits[2].argmax()), int(logits[0].argmax())]


def test_prefill_batch_int8_kv_cache(oracle, dev):
    from zhilight_amd import ops
    rng, cfg, sd, model = _gptq_model(dev, seed=21)
    lens, len_buf = [45, 17, 64], 128
    prompts = [rng.integers(0, cfg.vocab_size, s).astype(np.int32) for s in lens]
    ctx = model.new_context(3, len_buf, 0, kv_cache_dtype="int8")
    om = OracleModel(oracle, cfg, sd, 128, 3, len_buf, kv_quant=True)
    logits = model.prefill_batch(ctx, [0, 1, 2], [torch.from_numpy(p) for p in prompts]).float().cpu().numpy().astype(np.float64)
    for j, (s, p) in enumerate(zip(lens, prompts)):
        ref = om.prefill(j, p)
        assert np.abs(logits[j] - ref[0]).max() < 2e-3 * np.abs(ref).max(), j
        codes = ctx.kv[j][0, 0, :s].cpu().numpy().astype(np.int32)
        dcode = np.abs(codes - om.kc[0][j][:s].astype(np.int32))
        assert dcode.max() <= 1 and (dcode != 0).mean() < 0.02, j
        gs, rs = ctx.kv_scales[j][0, 0, :s].cpu().numpy(), om.ks[0][j][:s]
        assert np.abs(gs - rs).max() <= 2.0 ** -9 * rs.max(), j
    assert ctx.positions.tolist() == lens
    with pytest.raises(ops.ZLError):                  # a continued prompt on the INT8 cache
        model.prefill_batch(ctx, [0, 1], [torch.from_numpy(prompts[0][:4]), torch.from_numpy(prompts[1][:4])], pos0=[45, 0])


def test_prefill_batch_head_size_64(dev):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.minicpm_2b()
    cfg.num_layers = 2
    model = LLaMA(cfg, QuantConfig(0, 0), dev).init_random(seed=3)
    model.token_embedding.mul_(0.1)
    lens = [9, 20, 5]
    prompts = [torch.randint(0, cfg.vocab_size, (s,), dtype=torch.int32, device=dev) for s in lens]
    ctx_b = model.new_context(3, 64, 0)
    lb = model.prefill_batch(ctx_b, [0, 1, 2], prompts).float()
    for j, p in enumerate(prompts):
        ctx_1 = model.new_context(1, 64, 0)
        l1 = model.prefill(ctx_1, 0, p).float()[0]
        assert torch.isfinite(lb[j]).all()
        assert (lb[j] - l1).abs().max().item() <= 2e-2 * l1.abs().max().item(), j
        assert int(ctx_b.tokens[j]) == int(lb[j].argmax())
    assert ctx_b.positions.tolist() == lens


# measured on these inputs before the prompt path was restructured (profiles/prompt_path_refactor.txt): 0 on all three calls -- at
# these lengths the mask-form kernel splits both buffer lengths alike.  The bar is four times the measurement (another split
# partition under later kernel changes), never below one bf16 step of the largest logit, never above the 2e-2 of
# test_prefill_batch_head_size_64
HS64_INT8_BAR = min(2e-2, max(2.0 ** -7, 4 * 0.0))


def test_head_size_64_int8_cache_routes_against_fp16_cache(dev):
    """the mask-form (head size 64) prompt routes of an INT8 KV cache -- a fresh prompt on its own rows, a chunked prompt on its
    temporaries, several fresh prompts in one pass -- against the same calls on an fp16 cache: on every INT8 route the attention
    reads UNquantised rows, so the logits differ only by how the mask-form kernel partitions another buffer length"""
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.minicpm_2b()
    cfg.num_layers = 2
    model = LLaMA(cfg, QuantConfig(0, 0), dev).init_random(seed=3)
    model.token_embedding.mul_(0.1)
    g = torch.Generator().manual_seed(64)
    p9, p20, p5 = (torch.randint(0, cfg.vocab_size, (s,), generator=g, dtype=torch.int32) for s in (9, 20, 5))
    calls = {"one task": lambda ctx: model.prefill(ctx, 0, p20),
             "chunked": lambda ctx: model.prefill(ctx, 0, p20, chunk=8),          # pieces of 8, 8 and 4 rows; temporaries exist
             "three tasks": lambda ctx: model.prefill_batch(ctx, [0, 1, 2], [p9, p20, p5])}
    for name, call in calls.items():
        ctx_q, ctx_f = model.new_context(3, 64, 0, kv_cache_dtype="int8"), model.new_context(3, 64, 0)
        lq, lf = call(ctx_q).float(), call(ctx_f).float()
        n = lq.shape[0]
        for ctx, logits in ((ctx_q, lq), (ctx_f, lf)):
            assert torch.isfinite(logits).all(), name
            assert ctx.tokens[:n].tolist() == logits.argmax(dim=1).tolist(), name
        assert ctx_q.positions.tolist() == ctx_f.positions.tolist(), name
        assert ctx_q.valid_lens.tolist() == ctx_f.valid_lens.tolist(), name
        assert not ctx_q.unquant_kv, name
        err = (lq - lf).abs().max().item() / lf.abs().max().item()
        print(f"head size 64, INT8 against fp16 cache, {name}: max |dlogit| / max |logit| = {err:.3e}")
        assert err < HS64_INT8_BAR, (name, err)


def test_prefill_batch_tensor_parallel(dev):
    from zhilight_amd.llama import LLaMA, QuantConfig
    rng, cfg, sd, ref_model = _gptq_model(dev, seed=41, rope=False)
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    fake = _ThreadTP(2)
    models = [LLaMA(cfg, QuantConfig(5, 128), dev, tp=fake.view(r)).load_state_dict(sdt) for r in range(2)]
    lens, len_buf = [5, 40, 70, 17], 128
    prompts = [torch.from_numpy(rng.integers(0, cfg.vocab_size, s).astype(np.int32)) for s in lens]
    ref = ref_model.prefill_batch(ref_model.new_context(4, len_buf, 0), [0, 1, 2, 3], prompts).float()
    ctxs = [m.new_context(4, len_buf, 0) for m in models]
    outs = _run_ranks(fake, lambda r: models[r].prefill_batch(ctxs[r], [0, 1, 2, 3], prompts).float())
    assert torch.equal(outs[0], outs[1])
    assert (outs[0] - ref).abs().max().item() <= 2e-3 * ref.abs().max().item()
    assert ctxs[0].positions.tolist() == lens and torch.equal(ctxs[0].tokens, ctxs[1].tokens)


def test_prefill_batch_refusals(dev):
    from zhilight_amd import ops
    _, cfg, _, model = _gptq_model(dev)
    ctx = model.new_context(3, 64, 0)
    p = torch.arange(10, dtype=torch.int32)
    for tasks, prompts, pos0 in (([0, 0], [p, p], None),                          # duplicate tasks
                                 ([0, 1], [p, p[:0]], None),                      # empty prompt
                                 ([0, 3], [p, p], None),                          # task out of range
                                 ([0, 1], [p, torch.zeros(64, dtype=torch.int32)], None),   # does not fit max_len_buf
                                 ([0, 1], [p, p], [0, 60])):                      # continued past the buffer
        with pytest.raises(ops.ZLError):
            model.prefill_batch(ctx, tasks, prompts, pos0)
    assert ctx.positions.tolist() == [0, 0, 0] and ctx.tokens.tolist() == [0, 0, 0]
