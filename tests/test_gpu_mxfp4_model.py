"""An MXFP4 checkpoint through LLaMA (quant type 11) against THE SAME weights, dequantised, through the unquantised layer stack
(quant type 0): an MXFP4 weight is an exact value of fp16 / bf16 at these scales, so the dense stack on the dequantised tensors is the
reference and the two models differ only in where fp32 sums are rounded.  Teacher-forced -- both models are fed the dense model's
greedy tokens -- so a near-tie cannot fork the runs.  Bars: the project's own for these stacks (tests/test_gpu_model.py: decode against
the oracle), fp16 (1e-3 + 2^-11) max|ref|, bf16 2e-2 max|ref|."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import mxfp4_ref as R

pytestmark = pytest.mark.gpu

TOL = {"half": 1e-3 + 2.0 ** -11, "bfloat16": 2e-2}
LEN_BUF = 64
LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _cfg(dtype):
    from zhilight_amd.llama import ModelConfig
    return ModelConfig(num_layers=2, dim_model=512, num_heads=4, dim_head=128, dim_ff=1184, vocab_size=1024, num_kv_heads=2,
                       eps=1e-5, rope_theta=1e4, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _models(dtype):
    """(MXFP4 model, dense model on the dequantised weights), built once per dtype"""
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, QuantConfig
    dev = torch.device("cuda:0")
    cfg, tdt = _cfg(dtype), _cfg(dtype).torch_dtype
    rng = np.random.default_rng(41)
    hd, kvd = cfg.num_heads * cfg.dim_head, cfg.num_kv_heads * cfg.dim_head
    dims = {"self_attn.q_proj": (hd, cfg.dim_model), "self_attn.k_proj": (kvd, cfg.dim_model), "self_attn.v_proj": (kvd, cfg.dim_model),
            "self_attn.o_proj": (cfg.dim_model, hd), "mlp.gate_proj": (cfg.dim_ff, cfg.dim_model), "mlp.up_proj": (cfg.dim_ff, cfg.dim_model),
            "mlp.down_proj": (cfg.dim_model, cfg.dim_ff)}
    common = {"model.embed_tokens.weight": torch.from_numpy(rng.standard_normal((cfg.vocab_size, cfg.dim_model)) * 0.5).to(tdt),
              "model.norm.weight": torch.from_numpy(1 + 0.1 * rng.standard_normal(cfg.dim_model)).to(tdt),
              "lm_head.weight": torch.from_numpy(rng.standard_normal((cfg.vocab_size, cfg.dim_model)) * 0.05).to(tdt)}
    mx, dense = dict(common), dict(common)
    for i in range(cfg.num_layers):
        p = f"model.layers.{i}."
        for nm in ("input_layernorm.weight", "post_attention_layernorm.weight"):
            mx[p + nm] = dense[p + nm] = torch.from_numpy(1 + 0.1 * rng.standard_normal(cfg.dim_model)).to(tdt)
        for j, nm in enumerate(LINEARS):
            n, k = dims[nm]
            w = torch.from_numpy(rng.standard_normal((n, k)) * (0.7 / np.sqrt(k)))
            codes, scales = ops.mxfp4_quantize(w)
            w64 = R.decode(codes.numpy(), scales.numpy())
            wt = torch.from_numpy(w64).to(tdt)
            assert torch.equal(wt.to(torch.float64), torch.from_numpy(w64)), "the dequantised weight is not exact in T"
            assert float((wt.double() - w).abs().max()) <= float(w.abs().max()) / 4          # and it is the weight, quantised
            dense[p + nm + ".weight"] = wt
            if i == 1 and j % 2:                                                             # both spellings of the tensors
                mx[p + nm + ".weight_blocks"], mx[p + nm + ".weight_scales"] = codes.view(n, k // 32, 16), scales
            else:
                mx[p + nm + ".weight"], mx[p + nm + ".weight_scale"] = codes, scales
    m_mx = LLaMA(cfg, QuantConfig.from_hf(dict(quant_method="mxfp4")), dev).load_state_dict(mx)
    m_dense = LLaMA(cfg, QuantConfig(0, 0), dev).load_state_dict(dense)
    # what was loaded is what was quantised: the fused matrices dequantise to the dense model's rows
    l_mx, l_d = m_mx.layers[1], m_dense.layers[1]
    assert torch.equal(l_mx.qkv.weight.dequantize(tdt), l_d.qkv.weight)
    gu = l_mx.w_in_gated.weight.dequantize(tdt)
    assert torch.equal(gu[0::2], l_d.w_in.weight) and torch.equal(gu[1::2], l_d.w_gated.weight)
    assert m_mx.weight_bytes() < m_dense.weight_bytes()
    return m_mx, m_dense


def _close(got, ref, dtype, what):
    got, ref = got.float().cpu().numpy().astype(np.float64), ref.float().cpu().numpy().astype(np.float64)
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f"mxfp4_model: {what} {dtype}: max|got - ref| / max|ref| = {err / scale:.3e} (bar {TOL[dtype]:.3e})")
    assert np.isfinite(got).all() and err <= TOL[dtype] * scale, (what, err / scale)


def _prompts(b, lens, vocab, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, vocab, lens[j % len(lens)]).astype(np.int32)).cuda() for j in range(b)]


def _teacher_forced_decode(m_mx, m_dense, c_mx, c_d, dtype, steps, what):
    for step in range(steps):
        c_mx.tokens.copy_(c_d.tokens)                          # the dense model's greedy tokens feed both
        got, ref = m_mx.encode(c_mx), m_dense.encode(c_d)
        _close(got, ref, dtype, f"{what} decode step {step}")
        nxt = ref.float().argmax(dim=-1)
        m_mx.advance(c_mx, nxt)
        m_dense.advance(c_d, nxt)


@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
@pytest.mark.parametrize("batch", [1, 5, 9])
def test_prefill_then_decode_matches_dense_on_dequantised_weights(dtype, batch, dev):
    from zhilight_amd import ops
    m_mx, m_dense = _models(dtype)
    assert {ops.mxfp4_route(r, 512, 512) for r in (batch, 37)} >= {ops.MXFP4_TILED}
    prompts = _prompts(batch, (37,), 1024, 100 + batch)
    c_mx, c_d = m_mx.new_context(batch, LEN_BUF, 0), m_dense.new_context(batch, LEN_BUF, 0)
    for j, pr in enumerate(prompts):
        _close(m_mx.prefill(c_mx, j, pr), m_dense.prefill(c_d, j, pr), dtype, f"batch {batch} prefill task {j}")
    _teacher_forced_decode(m_mx, m_dense, c_mx, c_d, dtype, 6, f"batch {batch}")


@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
def test_prefill_batch_two_prompts(dtype, dev):
    m_mx, m_dense = _models(dtype)
    prompts = _prompts(2, (5, 41), 1024, 7)
    c_mx, c_d = m_mx.new_context(2, LEN_BUF, 0), m_dense.new_context(2, LEN_BUF, 0)
    _close(m_mx.prefill_batch(c_mx, [0, 1], prompts), m_dense.prefill_batch(c_d, [0, 1], prompts), dtype, "prefill_batch")
    _teacher_forced_decode(m_mx, m_dense, c_mx, c_d, dtype, 2, "prefill_batch")


def test_int8_kv_cache_context(dev):
    dtype = "half"
    m_mx, m_dense = _models(dtype)
    prompts = _prompts(5, (37,), 1024, 9)
    c_mx, c_d = (m.new_context(5, LEN_BUF, 0, kv_cache_dtype="int8") for m in (m_mx, m_dense))
    assert c_mx.kv_quant and c_d.kv_quant
    for j, pr in enumerate(prompts):
        _close(m_mx.prefill(c_mx, j, pr), m_dense.prefill(c_d, j, pr), dtype, f"int8 kv prefill task {j}")
    _teacher_forced_decode(m_mx, m_dense, c_mx, c_d, dtype, 3, "int8 kv")


def test_step_sample_under_a_captured_graph(dev):
    """three replays of a captured sampling step emit the tokens and log-probabilities of three eager steps, bit-equal: the serving
    layers ride on the new layer class unchanged"""
    m_mx, _ = _models("half")
    prompts = _prompts(3, (11, 7, 19), 1024, 13)
    kw = dict(temperature=0.8, top_k=20, top_p=0.95, seed=5)

    def fresh():
        ctx = m_mx.new_context(3, LEN_BUF, 0)
        m_mx.prefill_batch(ctx, [0, 1, 2], prompts)
        return ctx, m_mx.new_sampler(ctx, **kw)
    ctx, state = fresh()
    eager = []
    for _ in range(4):
        _, nxt = m_mx.step_sample(ctx, state)
        eager.append((nxt.clone(), state.logprobs.clone()))
    twin, tstate = fresh()
    _, nxt = m_mx.step_sample(twin, tstate)
    assert torch.equal(nxt, eager[0][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gnxt = m_mx.step_sample(twin, tstate)
    for step in range(1, 4):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gnxt, eager[step][0]), step
        assert torch.equal(tstate.logprobs.view(torch.int32), eager[step][1].view(torch.int32)), step
    assert torch.equal(twin.positions, ctx.positions) and torch.equal(twin.tokens, ctx.tokens)


def test_random_init_runs_both_dtypes(dev):
    from zhilight_amd.llama import LLaMA, QuantConfig
    for dtype in ("half", "bfloat16"):
        m = LLaMA(dataclasses.replace(_cfg(dtype), num_layers=1), QuantConfig(11, 32), dev).init_random(seed=1)
        ctx = m.new_context(2, 32, 0)
        logits = m.encode(ctx)
        assert logits.dtype == m.cfg.torch_dtype and torch.isfinite(logits.float()).all() and float(logits.float().abs().max()) > 0
