"""QuantConfig.act_quant = "mxfp4" in the routed layer of the toy MXFP4 Qwen3-MoE model (tests/test_gpu_mxfp4_moe_model.py, distinct
experts): a chunk above the layer's threshold is the stated composition of ops bit for bit, a chunk at or below it and a decode step
are the weight-only layer's bits."""
import copy
import dataclasses

import pytest
import torch

import test_gpu_mxfp4_moe_model as MM
from test_gpu_mxfp4_moe_a8_model import _xn

pytestmark = pytest.mark.gpu


def _layers(dtype):
    """(the routed layer as loaded: weight-only, a copy on the same weights with act_quant = "mxfp4" and the threshold at 32)"""
    layer = MM._models(dtype, True)[0].layers[1]
    a4 = copy.copy(layer)
    a4.quant, a4.a4_above_rows = dataclasses.replace(layer.quant, act_quant="mxfp4"), 32
    return layer, a4


@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
@pytest.mark.parametrize("rows", [33, 150])
def test_chunk_above_threshold_is_the_composition(dtype, rows, dev):
    from zhilight_amd import ops
    layer, a4 = _layers(dtype)
    xn = _xn(rows, dtype, dev)
    out = a4.moe(xn)
    ids, weights = a4.last_route
    e, k, p = MM.EXPERTS, 2, rows * 2
    pair = ops.arange_i32(p, dev)
    loads = torch.bincount(ids.reshape(-1).long(), minlength=e).int()
    _, order = ops.sort_pairs_i32(ids.reshape(-1), pair, max_key=e)
    act = ops.mxfp4_moe_a4_grouped(*ops.mxfp4_act_quantize(xn), a4.w_up, xn.dtype, loads, order, p, in_div=k, epilogue=ops.EPI_SILU_MUL)
    down = ops.mxfp4_moe_a4_grouped(*ops.mxfp4_act_quantize(act), a4.w_down, xn.dtype, loads, order, p, out_scatter=True)
    assert torch.equal(out, ops.moe_sum_experts(down, pair, weights))
    assert not torch.equal(out, layer.moe(xn))                  # the activations carry an E2M1 rounding


@pytest.mark.parametrize("dtype", ["half", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 9, 32])
def test_short_chunks_and_decode_steps_keep_their_bits(dtype, rows, dev):
    layer, a4 = _layers(dtype)
    xn = _xn(rows, dtype, dev)
    assert torch.equal(a4.moe(xn), layer.moe(xn))
