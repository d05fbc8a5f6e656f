"""Plain references for the load-time glue kernels (zhilight_amd/csrc/tensor_ops.hip, two neighbours in misc_ops.hip): numpy and
float64 only, no GPU, written from the behaviour include/zhilight_amd.h states.  tests/test_glue_ref_host.py pins these functions
themselves; tests/test_gpu_glue_ops.py compares the kernels with them.

Element types are named "f16", "bf16", "f32"; a rounded value travels as its BIT PATTERN (uint16 / uint32), so that NaN, the
infinities and the two zeros are compared as what they are.
"""
import numpy as np

# (exponent bits, stored fraction bits, bits dtype)
FORMATS = {"f16": (5, 10, np.uint16), "bf16": (8, 7, np.uint16), "f32": (8, 23, np.uint32)}


def _rne_f64_bits(x, ebits, mbits):
    """ONE round-to-nearest-even of float64 values to a binary format with `ebits` exponent and `mbits` fraction bits, on the 52-bit
    mantissa: subnormals of the target, overflow to inf, NaN (stays NaN, quiet) and signed zeros.  Returns uint64 patterns."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    sign = (u >> np.uint64(63)) << np.uint64(ebits + mbits)
    e = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    m = u & np.uint64((1 << 52) - 1)
    bias = (1 << (ebits - 1)) - 1
    emax_field = (1 << ebits) - 1
    inf_bits = np.uint64(emax_field << mbits)
    nan_bits = np.uint64((emax_field << mbits) | (1 << (mbits - 1)))
    E = e - 1023                                              # unbiased exponent of a normal float64
    sig = m | np.uint64(1 << 52)                              # 53-bit significand, value = sig * 2^(E - 52)
    emin = 1 - bias                                           # exponent of the target's smallest normal
    # bits to drop: 52 - mbits for a normal result, more below emin (the result is a subnormal: fixed spacing 2^(emin - mbits))
    shift = np.clip((52 - mbits) + np.maximum(emin - E, 0), 0, 63).astype(np.uint64)
    q = sig >> shift
    rem = sig & ((np.uint64(1) << shift) - np.uint64(1))
    half = np.uint64(1) << (shift - np.uint64(1))
    q = q + ((rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))).astype(np.uint64)
    # normal: the hidden bit of q adds 1 to the exponent field, so the field starts one lower; a carry out of the fraction lands in
    # the exponent by itself (and reaches the inf pattern from the largest finite value).  Subnormal: field 0, q is the pattern
    field = np.where(E >= emin, E + bias - 1, 0)
    bits = (np.clip(field, 0, emax_field).astype(np.uint64) << np.uint64(mbits)) + q
    bits = np.where(E + bias >= emax_field, inf_bits, bits)   # beyond the largest exponent: inf (also float64 inf itself)
    bits = np.where(e == 0, np.uint64(0), bits)               # float64 zero / subnormal: far below every target's subnormals
    bits = np.where((e == 0x7FF) & (m != 0), nan_bits, bits)
    return bits | sign


def rne_f64_to_f16(x):
    """float64 -> float16 bit patterns: numpy converts double -> half with one rounding"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.ascontiguousarray(x, dtype=np.float64).astype(np.float16).view(np.uint16)


def rne_f64_to_bf16(x):
    """float64 -> bfloat16 bit patterns with ONE rounding (torch's float64 -> bfloat16 goes through fp32 and rounds twice)"""
    return _rne_f64_bits(x, 8, 7).astype(np.uint16)


def rne_f64_to_f32(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.ascontiguousarray(x, dtype=np.float64).astype(np.float32).view(np.uint32)


def round_to(x64, t):
    """float64 values -> bit patterns of type t, one round-to-nearest-even"""
    return {"f16": rne_f64_to_f16, "bf16": rne_f64_to_bf16, "f32": rne_f64_to_f32}[t](x64)


def bits_to_f64(bits, t):
    """bit patterns of type t -> their exact float64 values"""
    with np.errstate(invalid="ignore"):                       # a signalling NaN pattern is quieted on the way, on purpose
        if t == "f16":
            return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)
        if t == "bf16":
            return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
        return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).astype(np.float64)


def is_nan_bits(bits, t):
    ebits, mbits, _ = FORMATS[t]
    mag = np.asarray(bits).astype(np.int64) & ((1 << (ebits + mbits)) - 1)
    return mag > (((1 << ebits) - 1) << mbits)


def ulp_diff(a_bits, b_bits, t):
    """distance in units of the last place: on the monotone integer image of the patterns (sign-magnitude -> signed, the two zeros
    coincide).  Meaningful for non-NaN patterns."""
    ebits, mbits, _ = FORMATS[t]
    mask = (1 << (ebits + mbits)) - 1

    def key(b):
        b = np.asarray(b).astype(np.int64)
        return np.where(b >> (ebits + mbits) != 0, -(b & mask), b & mask)
    return np.abs(key(a_bits) - key(b_bits))


def special_values(t):
    """float64 values around the edges of type t: zeros, smallest subnormal and half of it, largest finite, first value that rounds
    to inf, and their neighbours; both signs"""
    ebits, mbits, _ = FORMATS[t]
    bias = (1 << (ebits - 1)) - 1
    tiny = 2.0 ** (1 - bias - mbits)
    big = (2.0 - 2.0 ** -mbits) * 2.0 ** bias
    to_inf = (2.0 - 2.0 ** -(mbits + 1)) * 2.0 ** bias           # halfway between the largest finite value and 2^(bias+1): ties to inf
    v = [0.0, tiny, tiny / 2, np.nextafter(tiny / 2, 1.0), np.nextafter(tiny / 2, 0.0), 1.5 * tiny, 2.5 * tiny, 2.0 ** (1 - bias),
         np.nextafter(2.0 ** (1 - bias), 0.0), big, to_inf, np.nextafter(to_inf, 0.0), np.nextafter(to_inf, np.inf), 2 * big, np.inf, 1.0]
    v = np.array(v, np.float64)
    return np.concatenate([v, -v, [np.nan]])


def halfway_cases(t, rng, count=2000):
    """exact ties of type t (float64 values in the middle of two neighbours of t), over the normal and the subnormal range"""
    ebits, mbits, dt = FORMATS[t]
    n_finite = ((1 << ebits) - 1) << mbits                         # patterns 0 .. n_finite - 1 are the non-negative finite values
    lo = rng.integers(0, n_finite - 1, count).astype(np.int64)
    a, b = bits_to_f64(lo.astype(dt), t), bits_to_f64((lo + 1).astype(dt), t)
    mid = (a + b) / 2                                              # exact: both have at most 24 significant bits
    return np.concatenate([mid, -mid])


# ---- restatements of the kernels' operations -----------------------------------------------------------------------------------------
def max_gt(a, b):
    """the reference's max: a > b ? a : b (a NaN in a gives b, a NaN in b gives NaN)"""
    return np.where(a > b, a, b)


def abs_max_rows(x64):
    """per row max |x| from the reference's start value -1e4, NaN ignored (fmax)"""
    x64 = np.asarray(x64, np.float64)
    start = np.full((x64.shape[0], 1), -1e4)
    return np.fmax.reduce(np.concatenate([start, np.abs(x64)], axis=1), axis=1)


def silu(x):
    """x / (1 + exp(-x)) in float64; -inf gives the limit -0.0 (the quotient itself is inf / inf there)"""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        y = x / (1.0 + np.exp(-x))
    return np.where(x == -np.inf, -0.0, y)


def gelu_tanh(x):
    """gelu(tanh): 0.5 x (1 + tanh(u)), u = sqrt(2 / pi) x (1 + 0.044715 x^2), in float64 -- evaluated as x / (1 + exp(-2u)), the same
    function without the cancellation: 1 + tanh(u) loses every digit from u = -19 on even in float64 (x = -7.3), while the value
    (1e-15 and smaller) is still an ordinary bf16 / fp32 number down to x = -10.7"""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        u2 = 2.0 * np.sqrt(2.0 / np.pi) * x * (1.0 + 0.044715 * x * x)
        return np.where(u2 < -700.0, x * np.exp(u2), x / (1.0 + np.exp(-u2)))


def unpack_nibbles(q):
    """(K/8, N) uint32 -> (K, N) uint8: nibble j of word r is row 8 r + j"""
    q = np.asarray(q, np.uint32)
    k8, n = q.shape
    out = np.empty((k8, 8, n), np.uint8)
    for j in range(8):
        out[:, j, :] = (q >> np.uint32(4 * j)) & np.uint32(0xF)
    return out.reshape(k8 * 8, n)


def pack_nibbles(rows):
    rows = np.asarray(rows, np.uint32)
    k, n = rows.shape
    r = rows.reshape(k // 8, 8, n)
    out = np.zeros((k // 8, n), np.uint32)
    for j in range(8):
        out |= r[:, j, :] << np.uint32(4 * j)
    return out


def gptq_permute_rows(q, perm):
    """row i of the regrouped nibble matrix is row perm[i] of the input"""
    return pack_nibbles(unpack_nibbles(q)[np.asarray(perm, np.int64)])


def perm_reverse(perm, k, fill=0):
    """out[perm[i]] = i as uint16; an entry outside [0, k) is dropped and its slot keeps `fill`"""
    perm = np.asarray(perm, np.int64)
    out = np.full(k, fill, np.uint16)
    ok = (perm >= 0) & (perm < k)
    out[perm[ok]] = np.arange(perm.size, dtype=np.int64)[ok].astype(np.uint16)
    return out


def mask_valid_lens(mask, buf_lens, len_q):
    """1 + the last nonzero entry of every task's LAST query row (0 if none); the tasks' (len_q, buf_lens[b]) masks lie back to back"""
    mask = np.asarray(mask)
    out, off = [], 0
    for lb in buf_lens:
        row = mask[off + (len_q - 1) * lb: off + len_q * lb]
        nz = np.nonzero(row)[0]
        out.append(int(nz[-1]) + 1 if nz.size else 0)
        off += len_q * lb
    return np.array(out, np.int32)


def rope_rotate(x64, cos, sin, neox):
    """float64 rotation of (n, heads, d) by the rows' cos / sin (n, d): neox pairs (i, i + d/2), else (2i, 2i + 1);
    the first of a pair gets a c - b s, the second a c + b s (c, s taken at the element's own column)"""
    x64 = np.asarray(x64, np.float64)
    d = x64.shape[-1]
    c, s = np.asarray(cos, np.float64)[:, None, :], np.asarray(sin, np.float64)[:, None, :]
    cols = np.arange(d)
    if neox:
        partner, first = np.where(cols < d // 2, cols + d // 2, cols - d // 2), cols < d // 2
    else:
        partner, first = cols ^ 1, (cols & 1) == 0
    b = x64[..., partner]
    return np.where(first, x64 * c - b * s, x64 * c + b * s)
