"""QuantConfig.act_quant = "mxfp4" (W4A4) through LLaMA (quant type 11): one synthetic checkpoint loaded twice, weight-only and with
MXFP4 activations.  The layer's wiring against the hand composition of the ops bit for bit, decode-sized calls unchanged bit for bit,
and the prompt's logits against the weight-only model's under a bar of twice the measured distance."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_mxfp4_a8_model import EPS

# max|a4 - w16| / max|w16| over the last prompt row's logits: a quality figure nobody can derive (E2M1 carries ONE mantissa bit).
# Measured on an MI355X at seed 0: half 1.301e-1, bfloat16 9.813e-2 (MXFP8: 2.946e-2, 2.687e-2); the bar is twice that, the MXFP8
# model test's margin.  The second seed (half 1.292e-1, bfloat16 1.571e-1) is inside it.
E2E_BAR = {"half": 2 * 1.3011e-1, "bfloat16": 2 * 9.8131e-2}


@functools.lru_cache(maxsize=None)
def _models(dtype):
    """(weight-only model, act_quant="mxfp4" model) from the same checkpoint tensors: the MXFP8 model test's network"""
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig(num_layers=2, dim_model=256, num_heads=2, dim_head=128, dim_ff=512, vocab_size=64, num_kv_heads=2, eps=EPS,
                      rope_theta=1e4, dtype=dtype)
    rng, tdt = np.random.default_rng(17), cfg.torch_dtype
    sd = {"model.embed_tokens.weight": torch.from_numpy(rng.standard_normal((64, 256)) * 0.5).to(tdt),
          "model.norm.weight": torch.ones(256, dtype=tdt), "lm_head.weight": torch.from_numpy(rng.standard_normal((64, 256)) * 0.05).to(tdt)}
    dims = {**{f"self_attn.{c}_proj": (256, 256) for c in "qkvo"}, "mlp.gate_proj": (512, 256), "mlp.up_proj": (512, 256), "mlp.down_proj": (256, 512)}
    for i in range(2):
        p = f"model.layers.{i}."
        for nm in ("input_layernorm.weight", "post_attention_layernorm.weight"):
            sd[p + nm] = torch.from_numpy(1 + 0.1 * rng.standard_normal(256)).to(tdt)
        for nm, (n, k) in dims.items():
            sd[p + nm + ".weight"], sd[p + nm + ".weight_scale"] = ops.mxfp4_quantize(torch.from_numpy(rng.standard_normal((n, k)) * (0.7 / np.sqrt(k))))
    return tuple(LLaMA(cfg, QuantConfig(11, 32, True, act_quant=a), torch.device("cuda:0")).load_state_dict(sd) for a in ("", "mxfp4"))


def _hidden(rows, dtype, seed=3):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, 256))).to(_models(dtype)[0].cfg.torch_dtype).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
def test_wiring_is_the_composition_of_the_ops(dtype, dev):
    from zhilight_amd import ops
    layer, hidden = _models(dtype)[1].layers[1], _hidden(40, dtype)
    tdt = hidden.dtype
    got, ref = hidden.clone(), hidden.clone()
    layer.ff_add(got, EPS)
    xq, xs = ops.mxfp4_act_quantize(ops.rmsnorm(ref, layer.ln_ff, EPS))
    aq, asc = ops.mxfp4_act_quantize(ops.mxfp4_a4_linear(xq, xs, layer.w_in_gated.weight, tdt, epilogue=ops.EPI_SILU_MUL))
    ops.mxfp4_a4_linear(aq, asc, layer.w_out.weight, tdt, residual=ref, out=ref)
    assert torch.equal(got, ref) and not torch.equal(got, hidden)
    xq, xs = ops.mxfp4_act_quantize(ops.rmsnorm(hidden, layer.ln_attn, EPS))
    assert torch.equal(layer.project_qkv(hidden, EPS), ops.mxfp4_a4_linear(xq, xs, layer.qkv.weight, tdt))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
def test_decode_rows_stay_weight_only(dtype, dev):
    """9 rows through every entry of the layer, a 9-token prompt and six decode steps: the bits of the weight-only model"""
    from zhilight_amd.llama import MXFP4_A4_ABOVE_ROWS
    models, hidden = _models(dtype), _hidden(9, dtype)
    assert MXFP4_A4_ABOVE_ROWS >= 32
    for l16, l4 in zip(*(m.layers for m in models)):
        assert torch.equal(l16.project_qkv(hidden, EPS), l4.project_qkv(hidden, EPS))
        outs = [hidden.clone(), hidden.clone()]
        for l, h in zip((l16, l4), outs):
            l.attn_out_add(hidden.clone(), h)
            l.ff_add(h, EPS)
        assert torch.equal(*outs)
    prompt = torch.from_numpy(np.random.default_rng(9).integers(0, 64, 9).astype(np.int32)).cuda()
    ctxs = [m.new_context(1, 64, 0) for m in models]
    logits = [m.prefill(c, 0, prompt) for m, c in zip(models, ctxs)]
    for _ in range(6):
        assert torch.equal(*logits) and torch.isfinite(logits[0].float()).all()
        for m, c in zip(models, ctxs):
            m.advance(c, logits[0].float().reshape(-1, 64)[-1:].argmax(dim=-1))
        logits = [m.encode(c) for m, c in zip(models, ctxs)]
    assert torch.equal(*logits)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
def test_prompt_logits_against_weight_only(dtype, seed, dev):
    w16, a4 = _models(dtype)
    prompt = torch.from_numpy(np.random.default_rng(seed).integers(0, 64, 48).astype(np.int32)).cuda()
    ref, got = (m.prefill(m.new_context(1, 64, 0), 0, prompt).float().reshape(-1, 64)[-1] for m in (w16, a4))
    dist = float((got - ref).abs().max() / ref.abs().max())
    print(f"mxfp4_a4_model: {dtype} seed {seed}: max|a4 - w16| / max|w16| = {dist:.4e} (bar {E2E_BAR[dtype]:.4e})")
    assert torch.isfinite(got).all() and 0 < dist <= E2E_BAR[dtype]


def test_act_quant_is_refused_off_mxfp4_and_for_other_formats():
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    for quant in (QuantConfig(5, 128, act_quant="mxfp4"), QuantConfig(11, 32, act_quant="int8")):
        with pytest.raises(ops.ZLError, match="act_quant"):
            LLaMA(ModelConfig(), quant, "cpu")
