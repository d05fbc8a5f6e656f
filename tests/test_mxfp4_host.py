"""MXFP4 without a GPU: the format's reference decode and quantiser (tests/mxfp4_ref.py) against the table, against ops.mxfp4_quantize
and against transformers' LUT; QuantConfig.from_hf and the LLaMA refusals; and that the error bars of tests/test_gpu_mxfp4.py admit an
honest fp32 kernel and reject wrong ones."""
import ctypes

import numpy as np
import pytest
import torch

import dense_ref as D
import mxfp4_ref as R

SHAPES = ((4, 48, 96), (9, 80, 4128), (33, 144, 1056))


def test_all_codes_decode_to_the_table():
    table = [0, .5, 1, 1.5, 2, 3, 4, 6, 0, -.5, -1, -1.5, -2, -3, -4, -6]
    codes = R.pack_codes(np.tile(np.arange(16, dtype=np.uint8), 2)[None, :])          # one row, one block: every code twice
    for byte in (0, 1, 103, 126, 127, 128, 140, 254):
        w = R.decode(codes, np.array([[byte]], np.uint8))
        assert np.array_equal(w[0], np.ldexp(np.array(table * 2, np.float64), byte - 127)), byte
        assert not np.signbit(w[0, 8])                                                # code 8 is 0, not -0
    # byte j: element 2j in the low nibble
    assert np.array_equal(R.unpack_codes(np.array([[0x21, 0xF0]], np.uint8)), [[1, 2, 0, 15]])


def test_quantise_of_dequantise_is_the_identity():
    from zhilight_amd import llama, ops  # noqa: F401
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 256, (6, 64), dtype=np.uint8)
    c = R.unpack_codes(codes)
    c[c == 8] = 0                                             # -0 requantises to code 0
    c[:, 0] = 7                                               # every block holds a 6 or 4: its exponent is recoverable
    c[:, 32], c[:, 64], c[:, 96] = 15, 6, 14
    codes = R.pack_codes(c)
    scales = rng.integers(1, 254, (6, 4)).astype(np.uint8)
    w = R.decode(codes, scales)
    c2, s2 = R.quantize(w)
    assert np.array_equal(c2, codes) and np.array_equal(s2, scales)
    c3, s3 = ops.mxfp4_quantize(torch.from_numpy(w))
    assert np.array_equal(c3.numpy(), codes) and np.array_equal(s3.numpy(), scales)


def test_torch_quantiser_matches_the_reference_on_ties_zero_blocks_and_saturation():
    from zhilight_amd import llama, ops  # noqa: F401
    rng = np.random.default_rng(6)
    w = 0.05 * rng.standard_normal((5, 96))
    w[0, :32] = 0.0                                           # an all-zero block: byte 0
    w[1, :32] = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 4.0] * 4) * 2.0 ** -7 * np.where(np.arange(32) % 3 == 0, -1, 1)
    w[2, 32:64] = np.linspace(-7.9, 7.9, 32) * 2.0 ** -5       # amax in [4, 8) 2^-5: above 6 saturates
    cr, sr = R.quantize(w)
    ct, st = ops.mxfp4_quantize(torch.from_numpy(w))
    assert np.array_equal(ct.numpy(), cr) and np.array_equal(st.numpy(), sr)
    assert sr[0, 0] == 0 and not R.unpack_codes(cr)[0, :32].any()
    tie = R.unpack_codes(cr)[1, :8] & 7
    assert list(tie) == [0, 2, 2, 4, 4, 6, 6, 6], tie         # .25 -> 0, .75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4: even codes
    assert (np.abs(R.decode(cr, sr)[2, 32:64]).max() == 6 * 2.0 ** -5)
    # the quantiser is the nearest point of the grid: no element is further than half the local spacing (saturation aside)
    err = np.abs(R.decode(cr, sr) - w)
    step = np.ldexp(1.0, np.repeat(sr.astype(np.int64), 32, axis=1) - 127)
    assert (err <= np.maximum(step, np.abs(w) - 6 * step) + 1e-300).all()


def test_reference_decode_equals_transformers_lut():
    m = pytest.importorskip("transformers.integrations.mxfp4")
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 256, (4, 5, 16), dtype=np.uint8)  # (rows, blocks, 16 bytes): the weight_blocks shape
    scales = rng.integers(90, 160, (4, 5)).astype(np.uint8)
    lut = torch.tensor(m.FP4_VALUES, dtype=torch.float64)
    blk = torch.from_numpy(codes).reshape(20, 16)
    out = torch.empty(20, 32, dtype=torch.float64)
    out[:, 0::2] = lut[(blk & 0x0F).to(torch.int)]
    out[:, 1::2] = lut[(blk >> 4).to(torch.int)]
    out = torch.ldexp(out, torch.from_numpy(scales.astype(np.int32) - 127).reshape(20, 1))
    assert np.array_equal(out.reshape(4, 160).numpy(), R.decode(codes.reshape(4, 80), scales))


def test_quant_config_from_hf():
    from zhilight_amd import llama, ops  # noqa: F401
    q = llama.QuantConfig.from_hf(dict(quant_method="mxfp4"))
    assert (q.quant_type, q.group_size) == (11, 32) and llama.MXFP4 == 11
    spec = dict(dtype="fp4", qscheme="per_group", group_size=32, ch_axis=-1, scale_format="e8m0")
    quark = dict(quant_method="quark", global_quant_config=dict(weight=spec, input_tensors=dict(dtype="fp4", qscheme="per_group")))
    q = llama.QuantConfig.from_hf(quark)                      # the activation spec is ignored: weight-only execution
    assert (q.quant_type, q.group_size) == (11, 32)
    for change in (dict(dtype="int4"), dict(dtype="fp8_e4m3"), dict(qscheme="per_channel"), dict(group_size=128), dict(scale_format="float32")):
        bad = dict(quant_method="quark", global_quant_config=dict(weight=dict(spec, **change)))
        with pytest.raises(ops.ZLError, match="Unsupported Quark"):
            llama.QuantConfig.from_hf(bad)
    with pytest.raises(ops.ZLError, match="Unsupported Quark"):
        llama.QuantConfig.from_hf(dict(quant_method="quark"))
    with pytest.raises(ops.ZLError, match="Unsupported quant_method"):
        llama.QuantConfig.from_hf(dict(quant_method="bitsandbytes"))
    assert llama.QuantConfig.from_hf(dict(quant_method="gptq", bits=4)).quant_type == 5


def test_llama_refuses_tp_and_moe_before_loading():
    from zhilight_amd import llama, ops  # noqa: F401
    import dataclasses
    cfg = llama.ModelConfig(num_layers=1, dim_model=256, num_heads=2, dim_head=128, dim_ff=256, vocab_size=64, num_kv_heads=2)
    q = llama.QuantConfig(11, 32)

    class TP:
        rank, size = 0, 2
    with pytest.raises(ops.ZLError, match="MXFP4 models: tensor parallelism"):
        llama.LLaMA(cfg, q, device="cpu", tp=TP())
    moe = dataclasses.replace(cfg, moe_num_experts=4, moe_top_k=2, moe_intermediate_size=128)
    with pytest.raises(ops.ZLError, match="MXFP4 models: MoE"):
        llama.LLaMA(moe, q, device="cpu")
    with pytest.raises(ops.ZLError, match="block size is 32"):
        llama.LLaMA(cfg, llama.QuantConfig(11, 128), device="cpu")
    # fp16 and bf16 both construct
    for dt in ("half", "bfloat16"):
        m = llama.LLaMA(dataclasses.replace(cfg, dtype=dt), q, device="cpu")
        assert all(isinstance(l, llama.Mxfp4EncoderLayer) for l in m.layers)


def test_checkpoint_names_and_nan_scale():
    from zhilight_amd import llama, ops  # noqa: F401
    codes = torch.zeros(4, 3, 16, dtype=torch.uint8)
    scales = torch.full((4, 3), 127, dtype=torch.uint8)
    c, s, b = llama.mxfp4_tensors({"p.weight_blocks": codes, "p.weight_scales": scales}, "p")
    assert tuple(c.shape) == (4, 48) and tuple(s.shape) == (4, 3) and b is None
    c, s, b = llama.mxfp4_tensors({"p.weight": codes.reshape(4, 48), "p.weight_scale": scales, "p.bias": torch.zeros(4)}, "p")
    assert tuple(c.shape) == (4, 48) and b is not None
    with pytest.raises(ops.ZLError, match="not found"):
        llama.mxfp4_tensors({"p.weight": codes.reshape(4, 48)}, "p")
    with pytest.raises(ops.ZLError, match="uint8"):
        llama.mxfp4_tensors({"p.weight": torch.zeros(4, 48), "p.weight_scale": scales}, "p")


def test_route_query_is_host_only():
    from zhilight_amd import llama, ops  # noqa: F401
    from zhilight_amd._lib import lib
    r = lambda m, n, k: lib().zl_mxfp4_route(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int64(k))  # noqa: E731
    assert [r(m, 48, 96) for m in (1, 4, 5, 32, 33, 4096)] == [1, 1, 2, 2, 3, 3]
    assert [R.route(m) for m in (1, 4, 5, 32, 33, 4096)] == [1, 1, 2, 2, 3, 3]
    assert r(1, 48, 100) == -2 and r(0, 48, 96) == -1
    assert (ops.MXFP4_GEMV, ops.MXFP4_STREAM, ops.MXFP4_TILED) == (R.GEMV, R.STREAM, R.TILED)


@pytest.mark.parametrize("t", ["f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_bars_admit_an_honest_kernel_and_reject_wrong_ones(shape, t):
    m, n, k = shape
    x, codes, scales, _ = R.inputs(0, m, n, k, t)
    ex, s = R.exact(x, codes, scales, t), R.abs_sum(x, codes, scales, t)
    bar = R.bar(ex, s, m, k, t)
    assert D.worst_ratio(R.emulate(x, codes, scales, t), ex, bar, f"honest {shape} {t}") <= 1.0
    for variant in ("nibbles", "scale_shift"):
        got = R.emulate(x, codes, scales, t, variant)
        out = np.abs(got - ex) > bar
        assert out.sum() > out.size // 2, (variant, shape, t, int(out.sum()), out.size)
        with pytest.raises(AssertionError, match="out of their bar"):
            D.worst_ratio(got, ex, bar, variant)


def test_bars_reject_a_weight_rounded_to_fp16():
    m, n, k = 4, 48, 256
    x, codes, scales = R.small_scale_inputs(0, m, n, k)
    ex, s = R.exact(x, codes, scales, "f16"), R.abs_sum(x, codes, scales, "f16")
    bar = R.bar(ex, s, m, k, "f16")
    assert D.worst_ratio(R.emulate(x, codes, scales, "f16"), ex, bar, "honest small scale") <= 1.0
    got = R.emulate(x, codes, scales, "f16", "round_w")
    assert (np.abs(got - ex) > bar).sum() > (m * n) // 2
    # and at checkpoint-like scales rounding the weight is no error at all: the weights are fp16 values
    x, codes, scales, _ = R.inputs(0, *SHAPES[0], "f16")
    assert np.array_equal(R.emulate(x, codes, scales, "f16", "round_w"), R.emulate(x, codes, scales, "f16"))
