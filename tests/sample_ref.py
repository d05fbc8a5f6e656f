"""Pure-Python / numpy statement of zl_sample_advance (temperature, top-k and top-p sampling under the reference's rule,
src/generator/random_util.cu:83-199, in float64; the Philox4x32-10 uniforms), shared by test_sample_host.py and the GPU tests.
`sample` is the rule itself, with the sort.  `sample_sort_free` restates the kernel's procedure -- 16-bit keys, two levels of
256-bin count / mass histograms in integer fixed point, the j-th class of a value's run -- and `sample_sorted_fixed` is the sorting
rule over the same integer masses, which the restatement must equal exactly."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words -> 4 words (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)"""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [c0, c1, c2, c3]


def uniforms(seeds, draws):
    """the kernel's uniform of every row: key = the seed's two halves, counter = (the draw count's two halves, 0, 0),
    u = (word 0 >> 8) * 2^-24 -> float32 in [0, 1)"""
    out = np.empty(len(seeds), np.float32)
    for r, (s, d) in enumerate(zip(seeds, draws)):
        s, d = int(s) & 0xFFFFFFFFFFFFFFFF, int(d) & 0xFFFFFFFFFFFFFFFF
        w = philox4x32_10([d & MASK, d >> 32, 0, 0], [s & MASK, s >> 32])[0]
        out[r] = np.float32((w >> 8) * 2.0 ** -24)
    return out


def argmax(x):
    """zl_argmax_advance's pick: the first index of the largest value, a NaN counting as largest"""
    x = np.asarray(x, np.float64)
    nan = np.flatnonzero(np.isnan(x))
    return int(nan[0]) if nan.size else int(np.argmax(x))


def is_plain(x):
    """rows that take the arg-max whatever the parameters: a NaN, +inf, or nothing but -inf"""
    x = np.asarray(x, np.float64)
    return bool(np.isnan(x).any() or np.isposinf(x).any() or np.isneginf(x).all())


def sample(x, T, top_k, top_p, u):
    """the rule on one row of logits (any float array; evaluated in float64) -> (pick, pos, c, v, order): the picked class, its
    position in the sorted order, the inclusive running sums in that order, the threshold and the order itself.  T <= 0 or a
    plain row: (arg-max, 0, None, 0.0, None)"""
    x = np.asarray(x, np.float64)
    n = x.size
    if not T > 0 or is_plain(x):
        return argmax(x), 0, None, 0.0, None
    p = np.exp((x - x.max()) / float(T))
    order = np.argsort(-p, kind="stable")
    c = np.cumsum(p[order])
    Z = c[-1]
    cap = float(top_p)
    if 0 < top_k < n:
        cap = min(cap, c[top_k - 1] / Z)
    v = float(u) * cap * Z
    pos = int(np.searchsorted(c, v, side="left"))
    if pos >= n or p[order[pos]] == 0:
        pos = int(np.flatnonzero(p[order] > 0)[-1])
    return int(order[pos]), pos, c, v, order


def probabilities(x, T, top_k, top_p):
    """the exact probability of every class under the rule for a uniform u: (min(c[i], cap Z) - min(c[i-1], cap Z)) / (cap Z)"""
    _, _, c, _, order = sample(x, T, top_k, top_p, 0.5)
    n = c.size
    cap = float(top_p)
    if 0 < top_k < n:
        cap = min(cap, c[top_k - 1] / c[-1])
    lim = cap * c[-1]
    hi = np.minimum(c, lim)
    lo = np.concatenate([[0.0], hi[:-1]])
    out = np.zeros(n)
    out[order] = (hi - lo) / lim
    return out


def logprob(x, T, pick):
    """the tempered, untruncated log-probability of the pick; T <= 0: at T = 1"""
    x = np.asarray(x, np.float64)
    T = float(T) if T > 0 else 1.0
    a = (x - x.max()) / T
    return float(a[pick] - np.log(np.exp(a).sum()))


# ---- the kernel's procedure, restated ---------------------------------------------------------------------------------------------
def bits_of(x16):
    """a float16 array, or uint16 patterns as they are"""
    x16 = np.asarray(x16)
    return x16.view(np.uint16) if x16.dtype == np.float16 else x16.astype(np.uint16)


def values_of(bits, bf16):
    bits = np.asarray(bits, np.uint16)
    if bf16:
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.view(np.float16).astype(np.float64)


def keys_of(bits):
    """the monotone 16-bit key: larger value <=> larger key, -0.0 on +0.0's key"""
    v = np.asarray(bits, np.uint16).astype(np.uint32)
    v = np.where((v & 0x7FFF) == 0, 0, v)
    return v ^ np.where(v & 0x8000, 0xFFFF, 0x8000)


def fixed_masses(bits, bf16, T):
    """integer masses q = trunc(exp((x - max) / T) * 2^sh), sh = 62 - ceil(log2 n): a row sums below 2^62"""
    x = values_of(bits, bf16)
    n = x.size
    sh = 62 - (0 if n <= 1 else (n - 1).bit_length())
    p = np.minimum(np.exp((x - x.max()) / float(T)), 1.0)
    return np.array([int(math.floor(math.ldexp(float(v), sh))) for v in p], dtype=object), sh


def _threshold(u, top_p, Z, ck):
    lim = float(top_p) * float(Z)
    if ck is not None:
        lim = min(lim, float(ck))
    v = min(int(math.ceil(float(u) * lim)), Z)
    return v if ck is None else min(v, ck)


def sample_sorted_fixed(bits, bf16, T, top_k, top_p, u):
    """the sorting rule over the integer masses: order by (key descending, index ascending)"""
    bits = bits_of(bits)
    n = bits.size
    q, _ = fixed_masses(bits, bf16, T)
    keys = keys_of(bits)
    order = np.lexsort((np.arange(n), -keys.astype(np.int64)))
    c = np.cumsum(q[order])
    v = _threshold(u, top_p, int(c[-1]), int(c[top_k - 1]) if 0 < top_k < n else None)
    return int(order[next(i for i in range(n) if c[i] >= v)])


def sample_sort_free(bits, bf16, T, top_k, top_p, u):
    """no sort: histograms over the key's high byte, then over the low byte inside one bin, by count (top-k) and by mass (the
    nucleus); the pick is the j-th class, in index order, of the selected key"""
    bits = bits_of(bits)
    n = bits.size
    q, _ = fixed_masses(bits, bf16, T)
    keys = keys_of(bits).astype(np.int64)

    def hist(sel, byte):
        cnt, mass = [0] * 256, [0] * 256
        for b, m in zip(byte[sel], q[sel]):
            cnt[b] += 1
            mass[b] += int(m)
        return cnt, mass

    def select(cnt, mass, c_above, m_above, by_count, want):
        for b in range(255, -1, -1):
            have = cnt[b] if by_count else mass[b]
            above = c_above if by_count else m_above
            if have > 0 and above < want <= above + have:
                return b, c_above, m_above
            c_above, m_above = c_above + cnt[b], m_above + mass[b]
        raise AssertionError("no bin selected")

    everything = np.ones(n, bool)
    cnt1, mass1 = hist(everything, keys >> 8)
    Z, ck = sum(mass1), None
    if 0 < top_k < n:
        b1, ca, ma = select(cnt1, mass1, 0, 0, True, top_k)
        cnt2, mass2 = hist((keys >> 8) == b1, keys & 255)
        b2, ca, ma = select(cnt2, mass2, ca, ma, True, top_k)
        ck = ma + (top_k - ca) * (mass2[b2] // cnt2[b2])
    v = _threshold(u, top_p, Z, ck)
    if v == 0:
        return int(np.flatnonzero(keys == keys.max())[0])
    b1, ca, ma = select(cnt1, mass1, 0, 0, False, v)
    cnt2, mass2 = hist((keys >> 8) == b1, keys & 255)
    b2, ca, ma = select(cnt2, mass2, ca, ma, False, v)
    qk = mass2[b2] // cnt2[b2]
    j = min(max(-(-(v - ma) // qk), 1), cnt2[b2])
    return int(np.flatnonzero(keys == (b1 << 8 | b2))[j - 1])
