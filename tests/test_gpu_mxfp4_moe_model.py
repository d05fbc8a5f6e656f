"""An MXFP4 Qwen3-MoE checkpoint through LLaMA (quant type 11, Mxfp4MoEEncoderLayer): one dense and one routed layer.  With the same
three matrices in every expert and renormalised routing weights the routed feed-forward IS the dense one on those matrices, so the
unquantised stack on the dequantised weights is the reference for the whole model (load path, names, layer mix, every row regime),
with the bars of tests/test_gpu_mxfp4_model.py; with distinct experts the routed layer alone is held to float64 on the route it took."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import mxfp4_ref as R
import test_gpu_mxfp4_model as M

pytestmark = pytest.mark.gpu

EXPERTS, FF = 8, 288                               # 288 = 9 blocks: no multiple of 128


def _cfg(dtype, experts=EXPERTS):
    from zhilight_amd.llama import ModelConfig
    return ModelConfig(num_layers=2, dim_model=512, num_heads=4, dim_head=128, dim_ff=FF, vocab_size=1024, num_kv_heads=2, eps=1e-5,
                       rope_theta=1e4, dtype=dtype, model_type="qwen3_moe", qk_norm="head", moe_num_experts=experts, moe_top_k=2,
                       moe_intermediate_size=FF, norm_topk_prob=True, mlp_only_layers=[0])


@functools.lru_cache(maxsize=None)
def _models(dtype, distinct=False):
    """(MXFP4 MoE model, dense model on the dequantised weights of expert 0, the routed layer's exact expert matrices [(gate, up, down)])
    -- checkpoints written as tests/test_gpu_mxfp4_model.py::_models writes them, both tensor spellings"""
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, QuantConfig
    dev = torch.device("cuda:0")
    cfg, tdt = _cfg(dtype), _cfg(dtype).torch_dtype
    rng = np.random.default_rng(43)
    hd, kvd = cfg.num_heads * cfg.dim_head, cfg.num_kv_heads * cfg.dim_head
    dims = {"self_attn.q_proj": (hd, 512), "self_attn.k_proj": (kvd, 512), "self_attn.v_proj": (kvd, 512), "self_attn.o_proj": (512, hd),
            "mlp.gate_proj": (FF, 512), "mlp.up_proj": (FF, 512), "mlp.down_proj": (512, FF)}
    t64 = lambda a: torch.from_numpy(a).to(tdt)    # noqa: E731
    mx = {"model.embed_tokens.weight": t64(rng.standard_normal((1024, 512)) * 0.5), "model.norm.weight": t64(1 + 0.1 * rng.standard_normal(512)),
          "lm_head.weight": t64(rng.standard_normal((1024, 512)) * 0.05)}
    dense, exact, spell = dict(mx), [], 0

    def linear(name, n, k, dense_name=None):
        nonlocal spell
        codes, scales = ops.mxfp4_quantize(torch.from_numpy(rng.standard_normal((n, k)) * (0.7 / np.sqrt(k))))
        w64 = R.decode(codes.numpy(), scales.numpy())
        if dense_name:
            dense[dense_name + ".weight"] = t64(w64)
            assert torch.equal(dense[dense_name + ".weight"].double(), torch.from_numpy(w64)), "the dequantised weight is not exact in T"
        spell += 1
        if spell % 2:
            mx[name + ".weight_blocks"], mx[name + ".weight_scales"] = codes.view(n, k // 32, 16), scales
        else:
            mx[name + ".weight"], mx[name + ".weight_scale"] = codes, scales
        return codes, scales, w64
    for i in range(2):
        p = f"model.layers.{i}."
        for nm in ("input_layernorm.weight", "post_attention_layernorm.weight", "self_attn.q_norm.weight", "self_attn.k_norm.weight"):
            mx[p + nm] = dense[p + nm] = t64(1 + 0.1 * rng.standard_normal(128 if "_norm" in nm else 512))
        for nm in M.LINEARS[:4] if i else M.LINEARS:
            linear(p + nm, *dims[nm], dense_name=p + nm)
    p, ff = "model.layers.1.mlp.", M.LINEARS[4:]
    mx[p + "gate.weight"] = t64(rng.standard_normal((EXPERTS, 512)) / np.sqrt(512))
    for e in range(EXPERTS):
        if e == 0 or distinct:
            parts = [linear(f"{p}experts.{e}.{nm[4:]}", *dims[nm], dense_name=None if e else "model.layers.1." + nm) for nm in ff]
        else:                                      # expert 0's tensors again
            for nm, (codes, scales, _) in zip(ff, parts):
                mx[f"{p}experts.{e}.{nm[4:]}.weight"], mx[f"{p}experts.{e}.{nm[4:]}.weight_scale"] = codes, scales
        exact.append(tuple(w for _, _, w in parts))
    m_mx = LLaMA(cfg, QuantConfig.from_hf(dict(quant_method="mxfp4")), dev).load_state_dict(mx)
    m_dense = LLaMA(_cfg(dtype, 0), QuantConfig(0, 0), dev).load_state_dict(dense)
    from zhilight_amd.llama import Mxfp4EncoderLayer, Mxfp4MoEEncoderLayer
    assert type(m_mx.layers[0]) is Mxfp4EncoderLayer and type(m_mx.layers[1]) is Mxfp4MoEEncoderLayer
    gu = m_mx.layers[1].w_up.dequantize(EXPERTS - 1, tdt).double().cpu().numpy()
    assert np.array_equal(gu[0::2], exact[-1][0]) and np.array_equal(gu[1::2], exact[-1][1])      # what was loaded is what was quantised
    assert m_mx.weight_bytes() > 0
    return m_mx, m_dense, exact


@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
@pytest.mark.parametrize("batch", [1, 5, 9])
def test_prefill_then_decode_matches_dense_on_dequantised_weights(dtype, batch, dev):
    m_mx, m_dense, _ = _models(dtype)
    prompts = M._prompts(batch, (37,), 1024, 100 + batch)
    c_mx, c_d = m_mx.new_context(batch, M.LEN_BUF, 0), m_dense.new_context(batch, M.LEN_BUF, 0)
    for j, pr in enumerate(prompts):
        M._close(m_mx.prefill(c_mx, j, pr), m_dense.prefill(c_d, j, pr), dtype, f"moe batch {batch} prefill task {j}")
    M._teacher_forced_decode(m_mx, m_dense, c_mx, c_d, dtype, 6, f"moe batch {batch}")


@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
def test_prefill_batch_two_prompts(dtype, dev):
    m_mx, m_dense, _ = _models(dtype)
    prompts = M._prompts(2, (5, 41), 1024, 7)
    c_mx, c_d = m_mx.new_context(2, M.LEN_BUF, 0), m_dense.new_context(2, M.LEN_BUF, 0)
    M._close(m_mx.prefill_batch(c_mx, [0, 1], prompts), m_dense.prefill_batch(c_d, [0, 1], prompts), dtype, "moe prefill_batch")


@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 3, 9, 40, 150])
def test_routed_layer_distinct_experts_against_float64(dtype, rows, dev):
    """out = layer.moe(xn) against sum_k w_k down_e(silu(gate_e x) up_e x) in float64 with the stated roundings to T (gate, up, silu *
    mul, each expert's down output, the combine), on the route the layer took: a wrong expert, row or weight is an O(1) error"""
    m_mx, _, exact = _models(dtype, True)
    layer, t = m_mx.layers[1], {"half": "f16", "bfloat16": "bf16"}[dtype]
    assert {r <= layer.m_thres for r in (1, 3, 9, 40, 150)} == {True, False}                      # both forms are reached
    xn = torch.from_numpy(np.random.default_rng(rows).standard_normal((rows, 512))).to(m_mx.cfg.torch_dtype).to(dev)
    out = layer.moe(xn)
    ids, weights = (a.cpu().numpy() for a in layer.last_route)
    assert len({int(e) for e in ids.reshape(-1)}) > 1 or rows == 1
    x64, ref = xn.double().cpu().numpy(), np.zeros((rows, 512))
    for e, (wg, wu, wd) in enumerate(exact):
        act = R.rounded(R.silu64(R.rounded(x64 @ wg.T, t)) * R.rounded(x64 @ wu.T, t), t)
        ref += np.where(ids == e, weights.astype(np.float64), 0.0).sum(axis=1)[:, None] * R.rounded(act @ wd.T, t)
    M._close(out, torch.from_numpy(R.rounded(ref, t)), dtype, f"routed layer {rows} rows")


def test_step_sample_under_a_captured_graph(dev, monkeypatch):
    """the dense MXFP4 model's graph test on the MoE model: three replays of a captured step_sample at batch 3 equal three eager steps
    bit for bit -- the router, the pairs launches and the combine replay like every other launch of the step"""
    monkeypatch.setattr(M, "_models", lambda dtype: _models(dtype)[:2])
    M.test_step_sample_under_a_captured_graph(dev)


def test_other_moe_architectures_are_refused():
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, QuantConfig
    with pytest.raises(ops.ZLError, match="MoE layers of model_type 'qwen3_moe' only \\(got 'gpt_oss'\\)"):
        LLaMA(dataclasses.replace(_cfg("half"), model_type="gpt_oss"), QuantConfig(11, 32), device="cpu")
