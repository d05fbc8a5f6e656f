"""tests/glue_ref.py pinned on the CPU: the references test_gpu_glue_ops.py holds the kernels to must be right themselves."""
import numpy as np
import torch

import glue_ref as G


def _bf16_bits_torch(x32):
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _f32_inputs():
    rng = np.random.default_rng(20240611)
    with np.errstate(over="ignore"):
        wide = (rng.standard_normal(200_000) * 10.0 ** rng.integers(-40, 39, 200_000)).astype(np.float32).view(np.uint32)
    parts = [rng.integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32),                 # any pattern: all exponents, NaNs, subnormals
             wide]
    hi = np.arange(0, 65536, dtype=np.uint32) << np.uint32(16)                                        # every bf16 value, and around each:
    for low in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):                                      # exact, just above, tie -+ 1 and the tie
        parts.append(hi | np.uint32(low))
    return np.concatenate(parts).view(np.float32)


def test_bf16_rounding_equals_torch_on_fp32_inputs():
    """on fp32-representable inputs one rounding and torch's fp32 -> bf16 coincide: bit-identical, NaN as NaN"""
    x32 = _f32_inputs()
    assert x32.size >= 1_000_000
    with np.errstate(invalid="ignore"):
        got = G.rne_f64_to_bf16(x32.astype(np.float64))
    want = _bf16_bits_torch(x32)
    nan = np.isnan(x32)
    assert np.array_equal(G.is_nan_bits(got, "bf16"), nan) and np.array_equal(G.is_nan_bits(want, "bf16"), nan)
    bad = np.nonzero((got != want) & ~nan)[0]
    assert bad.size == 0, (bad.size, [(float(x32[i]), hex(got[i]), hex(want[i])) for i in bad[:5]])


def test_generic_rounding_equals_numpy_for_f16_and_f32():
    """the same bit routine with half's and fp32's parameters against numpy's own double -> half / float conversions"""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(300_000) * 10.0 ** rng.integers(-12, 8, 300_000),
                        rng.standard_normal(100_000) * 10.0 ** rng.integers(-50, 42, 100_000),
                        G.special_values("f16"), G.special_values("f32"), G.halfway_cases("f16", rng), G.halfway_cases("f32", rng)])
    for t, (eb, mb, dt) in (("f16", G.FORMATS["f16"]), ("f32", G.FORMATS["f32"])):
        got, want = G._rne_f64_bits(x, eb, mb).astype(dt), G.round_to(x, t)
        nan = np.isnan(x)
        assert np.array_equal(G.is_nan_bits(got, t), nan) and np.array_equal(G.is_nan_bits(want, t), nan)
        bad = np.nonzero((got != want) & ~nan)[0]
        assert bad.size == 0, (t, bad.size, [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:5]])


def test_hand_vectors():
    """double-rounding cases, largest finite values, smallest subnormals, overflow, zeros, NaN: written out by hand"""
    bf = [(1 + 2.0 ** -8 + 2.0 ** -30, 0x3F81),      # through fp32 this is the tie 1 + 2^-8 and falls to 1.0 (0x3F80)
          (1 + 2.0 ** -8, 0x3F80), (1 + 3 * 2.0 ** -8, 0x3F82), (1 + 2.0 ** -8 - 2.0 ** -40, 0x3F80),
          (-(1 + 2.0 ** -8 + 2.0 ** -30), 0xBF81),
          (0.0, 0x0000), (-0.0, 0x8000), (np.inf, 0x7F80), (-np.inf, 0xFF80),
          ((2 - 2.0 ** -7) * 2.0 ** 127, 0x7F7F),    # largest finite
          ((2 - 2.0 ** -8) * 2.0 ** 127, 0x7F80),    # the tie above it goes to inf
          (np.nextafter((2 - 2.0 ** -8) * 2.0 ** 127, 0.0), 0x7F7F), (1e39, 0x7F80), (-1e300, 0xFF80),
          (2.0 ** -133, 0x0001), (2.0 ** -134, 0x0000), (np.nextafter(2.0 ** -134, 1.0), 0x0001), (3 * 2.0 ** -134, 0x0002),
          (2.0 ** -126, 0x0080), (np.nextafter(2.0 ** -126, 0.0), 0x0080), (2.0 ** -126 - 2.0 ** -133, 0x007F), (1e-310, 0x0000),
          (-2.0 ** -140, 0x8000)]
    for x, want in bf:
        got = int(G.rne_f64_to_bf16(np.array([x]))[0])
        assert got == want, ("bf16", x, hex(got), hex(want))
    f16 = [(1 + 2.0 ** -11 + 2.0 ** -30, 0x3C01),    # through fp32: the tie 1 + 2^-11 and falls to 1.0 (0x3C00)
           (1 + 2.0 ** -11, 0x3C00), (1 + 3 * 2.0 ** -11, 0x3C02), (-(1 + 2.0 ** -11 + 2.0 ** -30), 0xBC01),
           (0.0, 0x0000), (-0.0, 0x8000), (np.inf, 0x7C00), (-np.inf, 0xFC00),
           (65504.0, 0x7BFF), (65520.0, 0x7C00), (np.nextafter(65520.0, 0.0), 0x7BFF), (1e6, 0x7C00),
           (2.0 ** -24, 0x0001), (2.0 ** -25, 0x0000), (np.nextafter(2.0 ** -25, 1.0), 0x0001), (3 * 2.0 ** -25, 0x0002),
           (2.0 ** -14, 0x0400), (2.0 ** -14 - 2.0 ** -24, 0x03FF), (-2.0 ** -30, 0x8000)]
    for x, want in f16:
        got = int(G.rne_f64_to_f16(np.array([x]))[0])
        assert got == want, ("f16", x, hex(got), hex(want))
        assert int(G._rne_f64_bits(np.array([x]), 5, 10)[0]) == want
    for t in ("f16", "bf16", "f32"):
        assert bool(G.is_nan_bits(G.round_to(np.array([np.nan]), t), t)[0])
    # the torch route the bf16 reference must NOT take really rounds twice
    assert float(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64).to(torch.bfloat16)[0]) == 1.0


def test_round_trip_and_ulp_distance():
    for t, (_, _, dt) in G.FORMATS.items():
        bits = np.arange(0, 65536, dtype=np.uint32).astype(dt) if t != "f32" else \
            np.random.default_rng(1).integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)
        nan = G.is_nan_bits(bits, t)
        back = G.round_to(G.bits_to_f64(bits, t), t)
        assert np.array_equal(back[~nan], bits[~nan]) and G.is_nan_bits(back[nan], t).all()
    assert G.ulp_diff(np.uint16(0x0000), np.uint16(0x8000), "f16") == 0          # the two zeros coincide
    assert G.ulp_diff(np.uint16(0x0001), np.uint16(0x8001), "bf16") == 2         # across zero
    assert G.ulp_diff(np.uint16(0x3C00), np.uint16(0x3BFF), "f16") == 1          # across a binade
    assert G.ulp_diff(np.uint32(0x7F7FFFFF), np.uint32(0x7F800000), "f32") == 1  # largest finite to inf
    assert np.array_equal(G.ulp_diff(np.array([3, 0x8005], np.uint16), np.array([7, 0x8001], np.uint16), "f16"), [4, 4])


def test_nibble_gather_and_permutations():
    rng = np.random.default_rng(9)
    for k, n in ((8, 1), (128, 8), (4096, 33)):
        q = rng.integers(0, 2 ** 32, (k // 8, n), dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(G.pack_nibbles(G.unpack_nibbles(q)), q)
        assert np.array_equal(G.gptq_permute_rows(q, np.arange(k)), q)                 # identity permutation: the input
        perm = rng.permutation(k)
        inv = G.perm_reverse(perm, k).astype(np.int64)
        assert np.array_equal(perm[inv], np.arange(k)) and np.array_equal(inv[perm], np.arange(k))
        assert np.array_equal(G.gptq_permute_rows(G.gptq_permute_rows(q, perm), inv), q)   # a permutation, then its reverse
        assert np.array_equal(G.perm_reverse(inv, k), perm.astype(np.uint16))
    one = np.zeros((1, 1), np.uint32)
    one[0, 0] = 0x76543210
    assert np.array_equal(G.unpack_nibbles(one)[:, 0], np.arange(8))
    assert G.gptq_permute_rows(one, [7, 6, 5, 4, 3, 2, 1, 0])[0, 0] == 0x01234567
    dropped = G.perm_reverse([2, -1, 4, 0], 4, fill=0xABCD)                            # -1 and k are dropped, their slots keep the fill
    assert dropped.tolist() == [3, 0xABCD, 0, 0xABCD]


def test_small_restatements():
    nan = np.nan
    assert np.array_equal(G.max_gt(np.array([1.0, nan, 2.0, -0.0]), np.array([2.0, 5.0, nan, 0.0])), [2.0, 5.0, nan, 0.0], equal_nan=True)
    assert np.signbit(G.max_gt(np.array([0.0]), np.array([-0.0])))[0]                  # 0 > -0 is false: b
    x = np.array([[1.0, -3.0, nan], [nan, nan, nan], [-np.inf, 2.0, 0.0], [-0.5, -0.25, 0.0]])
    assert np.array_equal(G.abs_max_rows(x), [3.0, -1e4, np.inf, 0.5])
    assert G.silu(np.array([0.0]))[0] == 0.0 and abs(G.silu(np.array([1.0]))[0] - 0.7310585786300049) < 1e-15
    s = G.silu(np.array([-np.inf, np.inf, -1e4, nan]))
    assert s[0] == 0 and np.signbit(s[0]) and s[1] == np.inf and s[2] == 0 and np.signbit(s[2]) and np.isnan(s[3])
    g = G.gelu_tanh(np.array([1.0, -1.0, np.inf, -np.inf, 0.0]))
    xs = np.linspace(-5.0, 20.0, 1001)                                                 # where the textbook form still has its digits
    assert np.allclose(G.gelu_tanh(xs), 0.5 * xs * (1 + np.tanh(np.sqrt(2 / np.pi) * xs * (1 + 0.044715 * xs * xs))), rtol=1e-8, atol=0)
    deep = G.gelu_tanh(np.array([-8.0, -10.0, -10.5, -1e4]))                             # below it: x exp(2u), no early zero
    assert abs(deep[0] / (-8.0 * np.exp(2 * np.sqrt(2 / np.pi) * -8.0 * (1 + 0.044715 * 64.0))) - 1) < 1e-12 and deep[1] < 0 and deep[2] < 0
    assert deep[3] == 0 and np.signbit(deep[3])
    assert abs(g[0] - 0.8411919906082768) < 1e-15 and abs(g[1] + 0.15880800939172324) < 1e-15 and g[2] == np.inf and np.isnan(g[3]) and g[4] == 0
    mask = np.array([0, 0, 1, 0,   1, 0, 0, 0,     0, 0, 0,   0, 0, 0,     2, -1], np.int8)       # tasks of 4, 3 and 1 keys, len_q 2
    assert G.mask_valid_lens(mask, [4, 3, 1], 2).tolist() == [1, 0, 1]
    assert G.mask_valid_lens(np.array([0, 5, 0, 1, 0, 0], np.int8), [6], 1).tolist() == [4]
    x = np.array([[[1.0, 2.0, 3.0, 4.0]]])
    c, s = np.array([[0.0, 0.0, 0.0, 0.0]]), np.array([[1.0, 1.0, 1.0, 1.0]])                      # a quarter turn
    assert np.array_equal(G.rope_rotate(x, c, s, True)[0, 0], [-3.0, -4.0, 1.0, 2.0])
    assert np.array_equal(G.rope_rotate(x, c, s, False)[0, 0], [-2.0, 1.0, -4.0, 3.0])
