"""Seeded inputs for the INT8 quantisers and W8A8 GEMMs (plain numpy, no GPU), and numpy restatements of the five quantisers.

Every other INT8 test draws Gaussian rows: a tie x * 127 / amax == j + 0.5 has probability ~0 on them, no row is zero, no amax
rounds when it is reduced in T.  The profiles here put the quantisers on exactly those inputs.  Every generator returns raw
16-bit patterns of fp16 (dtype 0) or bf16 (dtype 1) of the asked shape (m rows of k elements; the group form: groups of 32), is
seeded, and asserts that its values are exactly representable in T:

  ties_sorted / ties_shuffled  every row holds +127 and -127 (amax == 127, so 127 / amax == 1.0f exactly) and the ties j + 0.5,
                      j = -127 .. 126, dealt cyclically over the rows: x * bs has fraction exactly 0.5.  Round-half-even gives
                      the even neighbour; half-away differs on every second tie, truncation on the others.
  zero_row / neg_zero_row      Gaussian rows with one row of +0.0 / -0.0 (row 1; the only row when m == 1): codes 0 (q_zero), scale 0
  one_outlier         one element at 60000 (fp16) / 3e38 (bf16), the rest N(0, 1): every other code is 0, the scale is at the top
  tiny                magnitudes n * 2^-24, n <= 3, 31, 255 (row % 3): subnormal in fp16, scale down to ~3e-9, 127 / amax ~ 7e8.
                      bf16 gets the SAME values (normal there): a bf16-subnormal amax is < 1.2e-38 and 127 / amax overflows fp32,
                      which is the non-finite territory the reference defines nothing for.
  max_finite          every element +-65504 / +-3.39e38
  gauss               N(0, 1) rows times a row factor in 0.1 .. 10: the data of tests/test_gpu_ops.py::test_int8_path_bit_exact
  amax_rounds         (rmsnorm_quant: x, w; dequant_sum_quant_g32: my, q_others, scale_others)  the fp32 maximum max|x * w| / max|sum|
                      is not a T value and rounding it to T moves it DOWN on at least one row / group: the largest element lands
                      at 127 * (1 + eps) and must still code as +-127.  The seed is searched on the CPU (AMAX_SEEDS records what
                      the search finds for the shapes the GPU tests use; tests/test_int8_cases_host.py re-runs it).
"""
import zlib

import numpy as np

from attn_profiles import from_bits, to_bits

ROW_PROFILES = ("ties_sorted", "ties_shuffled", "zero_row", "neg_zero_row", "one_outlier", "tiny", "max_finite", "gauss")
TIES = np.arange(-127, 127) + 0.5                 # the 254 ties j + 0.5, j = -127 .. 126
MAX_FINITE = (65504.0, float(np.float32(2.0 ** 127 * (2.0 - 2.0 ** -7))))
OUTLIER = (60000.0, 3e38)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def f32(bits, dtype):
    """the float32 VALUES of T bits (exact)"""
    return from_bits(bits, dtype).astype(np.float32)


def exact_bits(x, dtype):
    """T bits of values that must already BE T values"""
    x = np.asarray(x, np.float64)
    bits = to_bits(x, dtype)
    assert np.array_equal(from_bits(bits, dtype), x), "value is not representable in T"
    return bits


def round_T(x32, dtype):
    """a float32 array rounded to T (nearest even) and back"""
    return f32(to_bits(np.asarray(x32, np.float32), dtype), dtype)


def _gauss_bits(rng, m, k, dtype):
    return to_bits(rng.standard_normal((m, k)) * rng.uniform(0.1, 10, (m, 1)), dtype)


def ties_rows(m, k, dtype, seed, shuffled):
    """(m, k >= 3): row r = -127, the k - 2 ties TIES[(r (k - 2) + i) % 254] ascending, +127; shuffled: a seeded permutation per row"""
    assert k >= 3
    rng = np.random.default_rng(seed)
    out = np.empty((m, k))
    for r in range(m):
        t = np.sort(TIES[(r * (k - 2) + np.arange(k - 2)) % len(TIES)])
        row = np.concatenate([[-127.0], t, [127.0]])
        out[r] = rng.permutation(row) if shuffled else row
    return exact_bits(out, dtype)


def ties_groups(groups, dtype, seed, shuffled=True):
    """(groups, 32): each group +-127 and 30 ties, TIES[(30 g + i) % 254]: nine groups cover every j"""
    return ties_rows(groups, 32, dtype, seed, shuffled)


def rows(name, m, k, dtype, seed=None):
    """the row profile `name` as (m, k) T bits"""
    seed = seed_of(name, m, k, dtype) if seed is None else seed
    rng = np.random.default_rng(seed)
    if name in ("ties_sorted", "ties_shuffled"):
        return ties_rows(m, k, dtype, seed, name == "ties_shuffled")
    if name in ("zero_row", "neg_zero_row"):
        x = _gauss_bits(rng, m, k, dtype)
        x[min(1, m - 1)] = 0x8000 if name == "neg_zero_row" else 0
        return x
    if name == "one_outlier":
        x = to_bits(rng.standard_normal((m, k)), dtype)
        x[np.arange(m), rng.integers(0, k, m)] = to_bits(np.array([OUTLIER[dtype]]), dtype)[0]      # 60000 is an fp16 value; bf16(3e38)
        return x
    if name == "tiny":
        top = np.array([3, 31, 255])[np.arange(m) % 3][:, None]
        n = rng.integers(1, 256, (m, k)) % top + 1
        x = exact_bits(n * rng.choice([-1.0, 1.0], (m, k)) * 2.0 ** -24, dtype)
        if dtype == 0:
            assert ((x & 0x7C00) == 0).all()                   # subnormal in fp16
        return x
    if name == "max_finite":
        return exact_bits(rng.choice([-1.0, 1.0], (m, k)) * MAX_FINITE[dtype], dtype)
    if name == "gauss":
        return _gauss_bits(rng, m, k, dtype)
    raise ValueError(name)


# ---- numpy restatements of the quantisers in the oracle's own float32 arithmetic; `rounding` is the kernel defect switch -------------
def _round(v, rounding):
    v = np.asarray(v, np.float32)
    if rounding == "even":
        return np.rint(v)
    if rounding == "away":
        return np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))
    if rounding == "trunc":
        return np.trunc(v)
    raise ValueError(rounding)


def _inv(num, amax):
    """num / amax in float32, 0 where amax == 0 (the zero-row contract)"""
    with np.errstate(divide="ignore"):
        return np.where(amax > 0, np.float32(num) / amax, np.float32(0)).astype(np.float32)


def np_quant_rows(xb, dtype, rounding="even", q_zero=0):
    """quant_calc_scale (q_zero 0: int8 codes) / quant_calc_scale_zp (q_zero 128: uint8 codes) -> (codes, fp32 scales)"""
    x = f32(xb, dtype)
    amax = np.abs(x).max(axis=1)
    codes = _round(x * _inv(127, amax)[:, None], rounding) + q_zero
    return codes.astype(np.uint8 if q_zero else np.int8), (amax / np.float32(127)).astype(np.float32)


def np_rmsnorm_quant_codes(xb, wb, scale, dtype, rounding="even", round_amax=True):
    """the int8 codes of rmsnorm_quant: p = x * w, amax = max|p| reduced in T, bs = float(127.0 / double(amax)), rint(p / scale * bs)"""
    p = f32(xb, dtype) * f32(wb, dtype)[None, :]
    amax = np.abs(p).max(axis=1)
    if round_amax:
        amax = round_T(amax, dtype)
    with np.errstate(divide="ignore"):
        bs = np.where(amax > 0, 127.0 / amax.astype(np.float64), 0.0).astype(np.float32)
    return _round((p / np.float32(scale)) * bs[:, None], rounding).astype(np.int8), amax


def np_quant_group_32(xb, dtype, rounding="even"):
    """quant_group_32: q = rint(v * 127.0f / amax) [product rounded first], scale = T(amax / 127)"""
    x = f32(xb, dtype).reshape(-1, 32)
    amax = np.abs(x).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(amax[:, None] > 0, _round((x * np.float32(127)) / amax[:, None], rounding), 0)
    return q.astype(np.int8).reshape(np.shape(xb)), to_bits(amax / np.float32(127), dtype)


def g32_sums(my, q_others, scale_others, dtype):
    """the fp32 sums of dequant_sum_quant_g32: fmaf chain over the peers (code * scale is exact in fp64, the sum rounds once to fp32)"""
    s = f32(my, dtype).reshape(-1, 32)
    for r in range(q_others.shape[0]):
        prod = q_others[r].reshape(-1, 32).astype(np.float64) * f32(scale_others[r], dtype).astype(np.float64)[:, None]
        s = (prod + s.astype(np.float64)).astype(np.float32)
    return s


def np_dequant_sum_quant_g32(my, q_others, scale_others, dtype, rounding="even", round_amax=True):
    s = g32_sums(my, q_others, scale_others, dtype)
    mag = round_T(np.abs(s), dtype) if round_amax else np.abs(s)
    amax = mag.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(amax[:, None] > 0, _round((s * np.float32(127)) / amax[:, None], rounding), 0)
    return q.astype(np.int8).reshape(np.shape(my)), to_bits(amax / np.float32(127), dtype)


# ---- amax_rounds -----------------------------------------------------------------------------------------------------------------------
def _norm_amax_draw(rows_, dim, dtype, seed):
    rng = np.random.default_rng(seed)
    x = to_bits(rng.standard_normal((rows_, dim)) * rng.uniform(0.1, 10, (rows_, 1)), dtype)
    w = to_bits(1 + 0.1 * rng.standard_normal(dim), dtype)
    p = np.abs(f32(x, dtype) * f32(w, dtype)[None, :])
    return x, w, p


def norm_amax_rounds(rows_, dim, dtype, seed=None):
    """rmsnorm_quant inputs (x (rows, dim), w (dim)) whose fp32 max|x * w| rounds DOWN in T on >= 1 row.
    Returns (x, w, seed, down): `down` marks the rows it happens on; seed None: search upwards from 0."""
    for s in ([seed] if seed is not None else range(1000)):
        x, w, p = _norm_amax_draw(rows_, dim, dtype, seed_of("norm_amax", rows_, dim, dtype, s))
        amax = p.max(axis=1)
        down = round_T(amax, dtype) < amax
        if down.any():
            return x, w, s, down
    raise AssertionError("no seed rounds the maximum down")


def _g32_amax_draw(groups, world, dtype, seed):
    rng = np.random.default_rng(seed)
    my = to_bits(rng.standard_normal((groups, 32)) * rng.uniform(0.1, 10, (groups, 1)), dtype)
    q = rng.integers(-127, 128, (world - 1, groups, 32)).astype(np.int8)
    sc = to_bits(rng.uniform(0.001, 0.08, (world - 1, groups)), dtype)
    return my, q, sc


def g32_amax_rounds(groups, world, dtype, seed=None):
    """dequant_sum_quant_g32 inputs whose largest |sum| of a group is no T value and rounds DOWN on >= 1 group -> (my, q, sc, seed, down)"""
    for s in ([seed] if seed is not None else range(1000)):
        my, q, sc = _g32_amax_draw(groups, world, dtype, seed_of("g32_amax", groups, world, dtype, s))
        mag = np.abs(g32_sums(my, q, sc, dtype))
        top = mag.max(axis=1)
        down = round_T(top, dtype) < top
        # (the group's maximum of the ROUNDED magnitudes is the rounded maximum: rounding is monotonic)
        if down.any():
            return my, q, sc, s, down
    raise AssertionError("no seed rounds the maximum down")


# the seeds the searches above return for the shapes of tests/test_gpu_int8_edges.py (key: rows, dim, dtype / groups, world, dtype);
# tests/test_int8_cases_host.py asserts that the search still finds exactly these
NORM_DIMS = (8, 40, 100, 1000, 1024, 1032, 4096, 8184, 8192, 16368)
NORM_ROWS = (1, 5)
G32_GROUPS = (1, 7, 8, 9, 4097)
G32_WORLDS = (2, 4, 8)
AMAX_SEEDS = {
    ('norm', 1, 8, 0): 0, ('norm', 1, 40, 0): 3, ('norm', 1, 100, 0): 1, ('norm', 1, 1000, 0): 0, ('norm', 1, 1024, 0): 2, ('norm', 1, 1032, 0): 0,
    ('norm', 1, 4096, 0): 0, ('norm', 1, 8184, 0): 0, ('norm', 1, 8192, 0): 0, ('norm', 1, 16368, 0): 1, ('norm', 5, 8, 0): 0, ('norm', 5, 40, 0): 0,
    ('norm', 5, 100, 0): 1, ('norm', 5, 1000, 0): 0, ('norm', 5, 1024, 0): 0, ('norm', 5, 1032, 0): 0, ('norm', 5, 4096, 0): 0, ('norm', 5, 8184, 0): 0,
    ('norm', 5, 8192, 0): 0, ('norm', 5, 16368, 0): 0, ('g32', 1, 2, 0): 3, ('g32', 1, 4, 0): 0, ('g32', 1, 8, 0): 0, ('g32', 7, 2, 0): 0,
    ('g32', 7, 4, 0): 0, ('g32', 7, 8, 0): 0, ('g32', 8, 2, 0): 0, ('g32', 8, 4, 0): 0, ('g32', 8, 8, 0): 0, ('g32', 9, 2, 0): 0,
    ('g32', 9, 4, 0): 0, ('g32', 9, 8, 0): 0, ('g32', 4097, 2, 0): 0, ('g32', 4097, 4, 0): 0, ('g32', 4097, 8, 0): 0, ('norm', 1, 8, 1): 0,
    ('norm', 1, 40, 1): 0, ('norm', 1, 100, 1): 1, ('norm', 1, 1000, 1): 0, ('norm', 1, 1024, 1): 0, ('norm', 1, 1032, 1): 0, ('norm', 1, 4096, 1): 1,
    ('norm', 1, 8184, 1): 6, ('norm', 1, 8192, 1): 1, ('norm', 1, 16368, 1): 0, ('norm', 5, 8, 1): 0, ('norm', 5, 40, 1): 0, ('norm', 5, 100, 1): 0,
    ('norm', 5, 1000, 1): 0, ('norm', 5, 1024, 1): 0, ('norm', 5, 1032, 1): 0, ('norm', 5, 4096, 1): 0, ('norm', 5, 8184, 1): 0, ('norm', 5, 8192, 1): 0,
    ('norm', 5, 16368, 1): 0, ('g32', 1, 2, 1): 0, ('g32', 1, 4, 1): 3, ('g32', 1, 8, 1): 2, ('g32', 7, 2, 1): 0, ('g32', 7, 4, 1): 0,
    ('g32', 7, 8, 1): 0, ('g32', 8, 2, 1): 0, ('g32', 8, 4, 1): 0, ('g32', 8, 8, 1): 0, ('g32', 9, 2, 1): 0, ('g32', 9, 4, 1): 0,
    ('g32', 9, 8, 1): 0, ('g32', 4097, 2, 1): 0, ('g32', 4097, 4, 1): 0, ('g32', 4097, 8, 1): 0,
}


def g32_ties_case(groups, world, dtype, seed):
    """dequant_sum_quant_g32 on ties: the sums are the group form of `ties` exactly.  Peer 0 carries code 2 d, scale 0.5 (d = sign of
    the tie on every second tie, 0 elsewhere and on +-127), `my` holds tie - d; the other peers come in +c / -c pairs with scale 0.25,
    so that every fmaf of the chain is exact.  Returns (my, q_others, scale_others, sums (groups, 32) float32)."""
    t = from_bits(ties_groups(groups, dtype, seed), dtype)
    rng = np.random.default_rng(seed + 1)
    d = np.where((np.abs(t) < 127) & (np.arange(32)[None, :] % 2 == 1), np.sign(t), 0.0)
    q = np.zeros((world - 1, groups, 32), np.int8)
    sc = np.zeros((world - 1, groups))
    q[0], sc[0] = 2 * d, 0.5
    for r in range(1, world - 1, 2):
        c = rng.integers(-127, 128, (groups, 32))
        q[r], q[r + 1] = c, -c
        sc[r] = sc[r + 1] = 0.25
    my, scb = exact_bits(t - d, dtype), exact_bits(sc, dtype)
    assert np.array_equal(g32_sums(my, q, scb, dtype), t.astype(np.float32))
    return my, q, scb, t.astype(np.float32)


# ---- int8 GEMM operands ----------------------------------------------------------------------------------------------------------------
GEMM_K = (16, 48, 256, 512, 768, 1024, 2048)
GEMM_M = (1, 16, 17, 32, 33, 64, 65)
GEMM_N = (1, 15, 17, 127, 129)


def gemm_shapes():
    """a reduced cross: every K with (65, 129); every M and every N at least once, on K of both kernels (48: the simple one, 768: the
    tiled one with three chunks)"""
    s = [(65, 129, k) for k in GEMM_K]
    s += [(m, 17, k) for m in GEMM_M for k in (48, 768) if (m, 17, k) not in s]
    s += [(33, n, k) for n in GEMM_N for k in (48, 768) if (33, n, k) not in s]
    s += [(1, 1, 256), (1, 1, 16), (64, 1, 512), (16, 127, 1024), (17, 15, 2048)]
    return s


def gemm_operands(m, n, k, kind, seed=None):
    """kind "uniform": both operands uniform over -128 .. 127 with -128 planted in row 0 of each; "min": both all -128"""
    if kind == "min":
        return np.full((m, k), -128, np.int8), np.full((n, k), -128, np.int8)
    rng = np.random.default_rng(seed_of("gemm", m, n, k) if seed is None else seed)
    a = rng.integers(-128, 128, (m, k), dtype=np.int8)
    b = rng.integers(-128, 128, (n, k), dtype=np.int8)
    a[0, 0] = b[0, 0] = a[-1, -1] = b[-1, -1] = -128
    return a, b


# ---- the chained and the gated cases (shared by the host and the GPU tests) -------------------------------------------------------------
def chain_case(dtype):
    """section h of the GPU test: ties rows through rmsnorm_quant (weight 1) -> int8 GEMM -> scale back, m = 5, k = 1024, n = 48"""
    m, k, n = 5, 1024, 48
    rng = np.random.default_rng(seed_of("chain", dtype))
    x = rows("ties_shuffled", m, k, dtype)
    w1 = exact_bits(np.ones(k), dtype)
    w8 = rng.integers(-128, 128, (n, k), dtype=np.int8)
    sy = to_bits(rng.uniform(0.001, 0.01, n), dtype)
    return x, w1, w8, sy


def gated_case(m, k, n, dtype):
    """the operands of one gated w8a8 case of the GPU test (n even): a (m, k), w (n, k) int8 incl. -128, sx (m) fp32, sy (n) T bits.
    The scales put the gate pre-activations at a few units, where silu and gelu are neither linear nor saturated."""
    rng = np.random.default_rng(seed_of("gated", m, k, n, dtype))
    a, w = gemm_operands(m, n, k, "uniform", seed_of("gated_ops", m, k, n))
    sx = rng.uniform(0.01, 0.05, m).astype(np.float32)
    sy = to_bits(rng.uniform(0.15, 0.5, n) / (74.0 * 74.0 * np.sqrt(k) * 0.03), dtype)      # |a|, |w| ~ 74: c ~ 74^2 sqrt(k)
    return a, w, sx, sy


def act_mul_f64(ca, cb, sx, sya, syb, act, dtype):
    """quant_back_act_mul with the float32 scale-backs (they are exact products rounded as the kernel rounds them) and the
    activation and final product in fp64, rounded once to T"""
    ab = ((ca.astype(np.float32) * sx[:, None]) * f32(sya, dtype)[None, :]).astype(np.float64)
    bb = ((cb.astype(np.float32) * sx[:, None]) * f32(syb, dtype)[None, :]).astype(np.float64)
    if act == "silu":
        gate = ab / (1.0 + np.exp(-ab))
    else:
        gate = 0.5 * ab * (1.0 + np.tanh(0.7978845608028654 * ab * (1.0 + 0.044715 * ab * ab)))
    return to_bits(bb * gate, dtype)


W8_M = (1, 16, 17, 32)
W8_KN = ((16, 1), (144, 8), (2064, 17), (1152, 40))
