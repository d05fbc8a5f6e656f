"""QuantConfig.act_quant = "mxfp8" through LLaMA (quant type 11): one synthetic checkpoint loaded twice, weight-only and with MXFP8
activations.  The layer's wiring against the hand composition of the ops bit for bit, decode-sized calls unchanged bit for bit, and
the prompt's logits against the weight-only model's under a bar of twice the measured distance."""
import functools

import numpy as np
import pytest
import torch

# max|a8 - w16| / max|w16| over the last prompt row's logits.  Expected from the arithmetic: E4M3 rounds each activation by at most
# 2^-4 relative, a few per cent rms per linear output.  Measured on an MI355X at seed 0: half 2.946e-2, bfloat16 2.687e-2; the bar is
# twice that.  The second seed (half 3.287e-2, bfloat16 4.213e-2) is inside it.
E2E_BAR = {"half": 2 * 2.9463e-2, "bfloat16": 2 * 2.6869e-2}
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _models(dtype):
    """(weight-only model, act_quant="mxfp8" model) from the same checkpoint tensors"""
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig(num_layers=2, dim_model=256, num_heads=2, dim_head=128, dim_ff=512, vocab_size=64, num_kv_heads=2, eps=EPS,
                      rope_theta=1e4, dtype=dtype)
    rng, tdt = np.random.default_rng(17), cfg.torch_dtype
    sd = {"model.embed_tokens.weight": torch.from_numpy(rng.standard_normal((64, 256)) * 0.5).to(tdt),
          "model.norm.weight": torch.ones(256, dtype=tdt), "lm_head.weight": torch.from_numpy(rng.standard_normal((64, 256)) * 0.05).to(tdt)}
    dims = {"self_attn.q_proj": (256, 256), "self_attn.k_proj": (256, 256), "self_attn.v_proj": (256, 256), "self_attn.o_proj": (256, 256),
            "mlp.gate_proj": (512, 256), "mlp.up_proj": (512, 256), "mlp.down_proj": (256, 512)}
    for i in range(2):
        p = f"model.layers.{i}."
        for nm in ("input_layernorm.weight", "post_attention_layernorm.weight"):
            sd[p + nm] = torch.from_numpy(1 + 0.1 * rng.standard_normal(256)).to(tdt)
        for nm, (n, k) in dims.items():
            sd[p + nm + ".weight"], sd[p + nm + ".weight_scale"] = ops.mxfp4_quantize(torch.from_numpy(rng.standard_normal((n, k)) * (0.7 / np.sqrt(k))))
    dev = torch.device("cuda:0")
    return tuple(LLaMA(cfg, QuantConfig(11, 32, True, act_quant=a), dev).load_state_dict(sd) for a in ("", "mxfp8"))


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
    xq, xs = ops.mxfp8_quantize(ops.rmsnorm(ref, layer.ln_ff, EPS))
    aq, asc = ops.mxfp8_quantize(ops.mxfp4_a8_linear(xq, xs, layer.w_in_gated.weight, tdt, epilogue=ops.EPI_SILU_MUL))
    ops.mxfp4_a8_linear(aq, asc, layer.w_out.weight, tdt, residual=ref, out=ref)
    assert torch.equal(got, ref) and not torch.equal(got, hidden)
    xq, xs = ops.mxfp8_quantize(ops.rmsnorm(hidden, layer.ln_attn, EPS))
    assert torch.equal(layer.project_qkv(hidden, EPS), ops.mxfp4_a8_linear(xq, xs, layer.qkv.weight, tdt))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
def test_decode_rows_stay_weight_only(dtype, dev):
    """9 rows through every entry of the layer, and the linear of a 1-row decode step: the bits of the weight-only model"""
    from zhilight_amd import ops
    from zhilight_amd.llama import MXFP4_A8_ABOVE_ROWS
    (w16, a8), hidden = _models(dtype), _hidden(9, dtype)
    assert ops.mxfp4_route(MXFP4_A8_ABOVE_ROWS, 768, 256) == ops.MXFP4_STREAM and ops.mxfp4_route(MXFP4_A8_ABOVE_ROWS + 1, 768, 256) == ops.MXFP4_TILED
    for l16, l8 in zip(w16.layers, a8.layers):
        assert torch.equal(l16.project_qkv(hidden, EPS), l8.project_qkv(hidden, EPS))
        outs = []
        for l in (l16, l8):
            h = hidden.clone()
            l.attn_out_add(hidden.clone(), h)
            l.ff_add(h, EPS)
            outs.append(h)
        assert torch.equal(outs[0], outs[1])
    # six decode steps after a 48-token prompt: one row per step, which mxfp4_route sends to the GEMV whatever act_quant says
    ctx = a8.new_context(1, 64, 0)
    logits = a8.prefill(ctx, 0, torch.from_numpy(np.random.default_rng(9).integers(0, 64, 48).astype(np.int32)).cuda())
    assert ops.mxfp4_route(ctx.tokens.shape[0], 768, 256) == ops.MXFP4_GEMV
    for _ in range(6):
        a8.advance(ctx, logits.float().reshape(-1, 64)[-1:].argmax(dim=-1))
        logits = a8.encode(ctx)
        assert torch.isfinite(logits.float()).all()
    one = _hidden(1, dtype)
    assert torch.equal(w16.layers[0].qkv.forward(one), a8.layers[0].qkv.forward(one))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
def test_prompt_logits_against_weight_only(dtype, seed, dev):
    w16, a8 = _models(dtype)
    prompt = torch.from_numpy(np.random.default_rng(seed).integers(0, 64, 48).astype(np.int32)).cuda()
    ref, got = (m.prefill(m.new_context(1, 64, 0), 0, prompt).float().reshape(-1, 64)[-1] for m in (w16, a8))
    dist = float((got - ref).abs().max() / ref.abs().max())
    print(f"mxfp4_a8_model: {dtype} seed {seed}: max|a8 - w16| / max|w16| = {dist:.4e} (bar {E2E_BAR[dtype]:.4e})")
    assert torch.isfinite(got).all() and 0 < dist <= E2E_BAR[dtype]


def test_act_quant_is_refused_off_mxfp4_and_for_other_formats():
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    for quant in (QuantConfig(5, 128, act_quant="mxfp8"), QuantConfig(11, 32, act_quant="int8")):
        with pytest.raises(ops.ZLError, match="act_quant"):
            LLaMA(ModelConfig(), quant, "cpu")
