"""Qwen3-MoE in the LLaMA driver, host side: config.json fields, checkpoint names, the refusals, and the host half of the grouped
GEMM's work table (grid sizes; the table itself is built on the device)."""
import numpy as np
import pytest
import torch

QWEN3_30B_A3B = dict(model_type="qwen3_moe", hidden_size=2048, num_attention_heads=32, num_key_value_heads=4, head_dim=128,
                     intermediate_size=6144, num_hidden_layers=48, vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1000000.0,
                     num_experts=128, num_experts_per_tok=8, moe_intermediate_size=768, norm_topk_prob=True,
                     decoder_sparse_step=1, mlp_only_layers=[], torch_dtype="bfloat16")


def _mods():
    """imported per test, not at collection: other test modules reload the library bindings, and the driver must see the
    ZLError class the test expects"""
    from zhilight_amd import ops
    from zhilight_amd import llama
    return ops, llama


def _small(**kw):
    ModelConfig = _mods()[1].ModelConfig
    base = dict(num_layers=2, dim_model=1024, num_heads=8, dim_head=128, dim_ff=1024, vocab_size=512, num_kv_heads=2,
                qk_norm="head", model_type="qwen3_moe", moe_num_experts=16, moe_top_k=4, moe_intermediate_size=256, norm_topk_prob=True)
    base.update(kw)
    return ModelConfig(**base)


def test_from_hf_qwen3_moe():
    ops, _l = _mods()
    LLaMA, ModelConfig, MoEEncoderLayer, QuantConfig, hf_name_to_internal = (_l.LLaMA, _l.ModelConfig, _l.MoEEncoderLayer, _l.QuantConfig,
                                                                            _l.hf_name_to_internal)
    c = ModelConfig.from_hf(QWEN3_30B_A3B)
    assert (c.moe_num_experts, c.moe_top_k, c.moe_intermediate_size, c.norm_topk_prob) == (128, 8, 768, True)
    assert (c.decoder_sparse_step, c.mlp_only_layers, c.qk_norm) == (1, [], "head")
    assert all(c.is_moe_layer(i) for i in range(c.num_layers))
    c2 = ModelConfig.from_hf(dict(QWEN3_30B_A3B, mlp_only_layers=[0, 5], decoder_sparse_step=2, norm_topk_prob=False))
    assert [i for i in range(8) if c2.is_moe_layer(i)] == [1, 3, 7]
    assert not c2.norm_topk_prob


def test_dense_config_keeps_defaults():
    ops, _l = _mods()
    LLaMA, ModelConfig, MoEEncoderLayer, QuantConfig, hf_name_to_internal = (_l.LLaMA, _l.ModelConfig, _l.MoEEncoderLayer, _l.QuantConfig,
                                                                            _l.hf_name_to_internal)
    c = ModelConfig.from_hf(dict(hidden_size=4096, num_attention_heads=32, num_key_value_heads=8, intermediate_size=14336,
                                 num_hidden_layers=32, vocab_size=128256, rope_theta=500000.0))
    d = ModelConfig()
    assert (c.moe_num_experts, c.moe_top_k, c.moe_intermediate_size, c.norm_topk_prob, c.decoder_sparse_step, c.mlp_only_layers) == \
        (d.moe_num_experts, d.moe_top_k, d.moe_intermediate_size, d.norm_topk_prob, d.decoder_sparse_step, d.mlp_only_layers) == \
        (0, 0, 0, False, 1, [])
    assert not any(c.is_moe_layer(i) for i in range(c.num_layers))


def test_expert_and_router_names():
    ops, _l = _mods()
    LLaMA, ModelConfig, MoEEncoderLayer, QuantConfig, hf_name_to_internal = (_l.LLaMA, _l.ModelConfig, _l.MoEEncoderLayer, _l.QuantConfig,
                                                                            _l.hf_name_to_internal)
    m = hf_name_to_internal
    assert m("model.layers.3.mlp.experts.17.gate_proj.qweight") == "llama.layers.3.ff.experts.17.w_in.qweight"
    assert m("model.layers.3.mlp.experts.17.up_proj.scales") == "llama.layers.3.ff.experts.17.w_gated.scales"
    assert m("model.layers.0.mlp.experts.127.down_proj.qzeros") == "llama.layers.0.ff.experts.127.w_out.qzeros"
    assert m("model.layers.12.mlp.gate.weight") == "llama.layers.12.ff.router.weight"
    # the dense names are unchanged, and a shared expert keeps a name the MoE layer can refuse
    assert m("model.layers.2.mlp.gate_proj.qweight") == "llama.layers.2.ff.w_in.qweight"
    assert m("model.layers.2.mlp.down_proj.qweight") == "llama.layers.2.ff.w_out.qweight"
    assert m("model.layers.1.mlp.shared_expert.gate_proj.qweight").startswith("llama.layers.1.ff.shared_expert.")
    assert m("model.layers.1.mlp.shared_expert_gate.weight") == "llama.layers.1.ff.shared_expert_gate.weight"


def test_layers_follow_mlp_only_layers():
    ops, _l = _mods()
    LLaMA, ModelConfig, MoEEncoderLayer, QuantConfig, hf_name_to_internal = (_l.LLaMA, _l.ModelConfig, _l.MoEEncoderLayer, _l.QuantConfig,
                                                                            _l.hf_name_to_internal)
    model = LLaMA(_small(num_layers=3, mlp_only_layers=[1]), QuantConfig(5, 128), "cpu")
    assert [type(l).__name__ for l in model.layers] == ["MoEEncoderLayer", "EncoderLayer", "MoEEncoderLayer"]
    assert model.moe
    assert not LLaMA(_small(moe_num_experts=0), QuantConfig(5, 128), "cpu").moe


def test_refuses_shared_experts():
    ops, _l = _mods()
    LLaMA, ModelConfig, MoEEncoderLayer, QuantConfig, hf_name_to_internal = (_l.LLaMA, _l.ModelConfig, _l.MoEEncoderLayer, _l.QuantConfig,
                                                                            _l.hf_name_to_internal)
    layer = MoEEncoderLayer(_small(), QuantConfig(5, 128), 0)
    sd = {"llama.layers.0.ff.shared_expert.gate_proj.qweight": torch.zeros(1, dtype=torch.int32)}
    with pytest.raises(ops.ZLError, match="shared experts"):
        layer.load_state_dict(sd, "llama.layers.0", "cpu")


def test_refuses_tp_ep_act_order_and_other_routes():
    ops, _l = _mods()
    LLaMA, ModelConfig, MoEEncoderLayer, QuantConfig, hf_name_to_internal = (_l.LLaMA, _l.ModelConfig, _l.MoEEncoderLayer, _l.QuantConfig,
                                                                            _l.hf_name_to_internal)
    class TP:
        size, rank = 2, 0
    with pytest.raises(ops.ZLError, match="tensor parallelism"):
        LLaMA(_small(), QuantConfig(5, 128), "cpu", tp=TP())
    with pytest.raises(ops.ZLError, match="act-order"):
        LLaMA(_small(), QuantConfig(5, 128, act_order=True), "cpu")
    with pytest.raises(ops.ZLError):
        LLaMA(_small(), QuantConfig(2, 128), "cpu")                  # the int8 layer stack
    with pytest.raises(ops.ZLError):
        LLaMA(_small(), QuantConfig(5, 64), "cpu")                   # group size the grouped kernel cannot take


def test_refuses_expert_parallel(monkeypatch):
    ops, _l = _mods()
    LLaMA, ModelConfig, MoEEncoderLayer, QuantConfig, hf_name_to_internal = (_l.LLaMA, _l.ModelConfig, _l.MoEEncoderLayer, _l.QuantConfig,
                                                                            _l.hf_name_to_internal)
    monkeypatch.setenv("MOE_EXP_PARALLEL", "1")
    with pytest.raises(ops.ZLError, match="expert parallelism"):
        LLaMA(_small(), QuantConfig(5, 128), "cpu")


def test_route_switch(monkeypatch):
    ops, _l = _mods()
    LLaMA, ModelConfig, MoEEncoderLayer, QuantConfig, hf_name_to_internal = (_l.LLaMA, _l.ModelConfig, _l.MoEEncoderLayer, _l.QuantConfig,
                                                                            _l.hf_name_to_internal)
    monkeypatch.setenv("ZL_MOE_ROUTE", "fused")
    assert MoEEncoderLayer(_small(), QuantConfig(5, 128), 0).route == "fused"
    monkeypatch.setenv("ZL_MOE_ROUTE", "bogus")
    with pytest.raises(ops.ZLError):
        MoEEncoderLayer(_small(), QuantConfig(5, 128), 0)


@pytest.mark.parametrize("pairs,experts", [(1, 128), (8, 128), (256, 128), (4096, 128), (16384, 128), (7, 3), (100, 1), (2048, 16)])
def test_work_table_bound(pairs, experts):
    """the grid never has fewer slots than the tiles of ANY split of `pairs` rows over the experts (uniform, skewed, all on
    one expert, every expert one row), and agrees with the library's own sizing"""
    ops, _l = _mods()
    LLaMA, ModelConfig, MoEEncoderLayer, QuantConfig, hf_name_to_internal = (_l.LLaMA, _l.ModelConfig, _l.MoEEncoderLayer, _l.QuantConfig,
                                                                            _l.hf_name_to_internal)
    from zhilight_amd import _lib
    bm, slots = ops.moe_grouped_slots(pairs, experts)
    assert bm in (16, 32, 64, 128)
    rng = np.random.default_rng(pairs * 131 + experts)
    splits = [np.bincount(rng.integers(0, experts, pairs), minlength=experts),
              np.bincount(np.minimum(rng.geometric(0.05, pairs) - 1, experts - 1), minlength=experts),
              np.array([pairs] + [0] * (experts - 1))]
    if pairs >= experts:
        splits.append(np.array([pairs - experts + 1] + [1] * (experts - 1)))
    for loads in splits:
        assert loads.sum() == pairs
        assert int(np.sum((loads + bm - 1) // bm)) <= slots
    lib = _lib.lib()
    assert lib.zl_moe_grouped_bm(ops._i(pairs), ops._i(experts)) == bm
    assert lib.zl_moe_grouped_tiles(ops._i(pairs), ops._i(experts), ops._i(bm)) == slots
