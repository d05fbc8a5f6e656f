// sample_rows.hip -- the stochastic pick of a decode step, kept on the device.
//   zl_sample_advance   per logit row: temperature, top-k and top-p (nucleus) sampling under the reference's rule
//                       (src/generator/random_util.cu:83-199: sort the probabilities descending, stable; cap = min(top_p, c[k-1] / Z);
//                       the first sorted class whose running sum reaches u * cap * Z), a Philox4x32-10 uniform per row and call, the
//                       pick's log-probability, and zl_argmax_advance's bookkeeping -- one launch.
//   zl_spec_sample_accept   the acceptance of a speculative step under sampling.  The drafter is deterministic, so its proposal is a
//                       point mass on the draft d, and the optimal speculative-sampling rule (Leviathan et al., ICML'23; Chen et al.,
//                       2023) reduces to: accept d with probability p(d), on rejection draw from p with d removed and renormalised
//                       -- which is: draw x ~ p with the task's next uniform, accept iff x == d, otherwise emit x.  So every row
//                       (t, i) of the step takes zl_sample_advance's pick under task t's parameters with the uniform of counter
//                       draws[t] + i, and the step consumes accepted + 1 draws: the emitted tokens are the same function of
//                       (logits, seed, tokens emitted so far) as without speculation.  TWO launches, as zl_spec_accept and for its
//                       reason: the sampling kernel in its per-row form (SPEC: no state, no draws written), then one thread per task
//                       for the prefix match, the padding, the state and the draws.
// The reference sorts on the host.  Nothing is sorted here: the logits are 16-bit, so a row holds at most 65 536 distinct values, a
// class's probability depends on its value alone, and the sorted order is "larger value, then lower index".  Both selections are
// radix selects on the monotone 16-bit key of the value, high byte then low byte: top-k selects by count, the nucleus by mass, and the
// pick among the classes that share the selected value is the j-th of them in index order.
// Determinism: mass is INTEGER fixed point, q = trunc(p * 2^sh) with p = exp((x - max) / T) <= 1 and sh = 62 - ceil(log2 n), so that a
// whole row sums below 2^62.  Histograms are filled with integer LDS atomics, whose sum does not depend on arrival order; the level-2
// bins of a level-1 bin sum to that bin exactly; the position inside a value's run is an integer division.  No float is ever
// accumulated, so the same inputs give the same pick on every run, replay and rank.
// One 1024-thread workgroup per row streams the row (L2-resident behind the lm_head) four to six times:
//   1  arg-max (zl_argmax_advance's key: NaN largest, first index wins) -> the max, and the whole pick of a T <= 0 / NaN / inf row
//   2  256-bin mass (top-k on: and count) histogram of the key's high byte -> Z; scanned from the top
//   3  top-k on: the low-byte COUNT histogram inside the bin of the k-th class, a bin's mass = count x mass of its key -> c[k-1]
//      exactly -> v = ceil(u * min(top_p Z, c[k-1]))
//   4  the same inside the bin where the running mass reaches v (skipped when it is pass 3's bin) -> the value, j
//   5  per-wave counts of the classes equal to that value, then one wave walks its 1/16 of the row to the j-th
#include <hip/hip_runtime.h>

#include "zl_common.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / ZL_WAVE;
constexpr int kBins = 256;
constexpr int kCopies = 16;        // histogram copies, one per lane & 15: logits crowd into a few high-byte bins, and lanes that
                                   // hit one LDS word are served one after the other
constexpr int kLoads = 4;          // 16-byte loads in flight per thread (zl_argmax_advance's streaming loop)

template <bool BF> struct H16;
template <> struct H16<false> {
    static constexpr uint32_t kInf = 0x7c00u;
    static __device__ __forceinline__ float f32(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
};
template <> struct H16<true> {
    static constexpr uint32_t kInf = 0x7f80u;
    static __device__ __forceinline__ float f32(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }
};

// the monotone key of a 16-bit float pattern: larger value <=> larger key; -0.0 takes +0.0's key (one value, ties by index)
__device__ __forceinline__ uint32_t key16(uint16_t h) {
    const uint32_t v = (h & 0x7fffu) == 0 ? 0u : (uint32_t)h;
    return v ^ ((v & 0x8000u) ? 0xffffu : 0x8000u);
}
__device__ __forceinline__ uint16_t unkey16(uint32_t k) { return (uint16_t)(k ^ ((k & 0x8000u) ? 0x8000u : 0xffffu)); }

// the fixed-point mass of every class whose value has this key: a pure function of (key, max, T, scale), evaluated by the same
// instructions wherever it is needed
template <bool BF>
__device__ __forceinline__ u64 mass_of(uint32_t key, float vmax, float t, float scale) {
    const float p = fminf(expf((H16<BF>::f32(unkey16(key)) - vmax) / t), 1.0f);
    return (u64)(p * scale);
}

// f(pattern, index) for every element of the row, in no particular order: up to 7 elements in front of the first 16-byte boundary,
// 16-byte lanes with kLoads loads in flight, up to 7 elements behind the last whole lane
template <class F>
__device__ __forceinline__ void for_each(const uint16_t* __restrict__ row, int n, F&& f) {
    const int tid = threadIdx.x;
    int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 1);
    head = head < n ? head : n;
    if (tid < head) f(row[tid], tid);
    const uint4* body = reinterpret_cast<const uint4*>(row + head);
    const int nv = (n - head) >> 3;
    for (int c0 = tid; c0 < nv; c0 += kLoads * kThreads) {
        uint4 v4[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int c = c0 + u * kThreads;
            v4[u] = body[c < nv ? c : c0];
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int c = c0 + u * kThreads;
            if (c < nv) {
                const uint32_t w[4] = {v4[u].x, v4[u].y, v4[u].z, v4[u].w};
#pragma unroll
                for (int e = 0; e < 8; ++e) f((uint16_t)(w[e >> 1] >> (16 * (e & 1))), head + c * 8 + e);
            }
        }
    }
    for (int i = head + nv * 8 + tid; i < n; i += kThreads) f(row[i], i);
}

struct Hist {                       // 48 KB: kCopies interleaved copies of a 256-bin (count, mass) histogram
    u64 mass[kBins * kCopies];
    uint32_t cnt[kBins * kCopies];
};

__device__ __forceinline__ void hist_zero(Hist& h) {
    for (int i = threadIdx.x; i < kBins * kCopies; i += kThreads) {
        h.mass[i] = 0;
        h.cnt[i] = 0;
    }
    __syncthreads();
}
__device__ __forceinline__ void hist_count(Hist& h, uint32_t bin) {
    atomicAdd(&h.cnt[(int)bin * kCopies + (threadIdx.x & (kCopies - 1))], 1u);
}
__device__ __forceinline__ void hist_mass(Hist& h, uint32_t bin, u64 q) {
    if (q) atomicAdd(&h.mass[(int)bin * kCopies + (threadIdx.x & (kCopies - 1))], q);
}
// thread t < 256 takes bin 255 - t: the scan over threads runs from the largest key down
__device__ __forceinline__ void hist_take(const Hist& h, uint32_t& c, u64& m) {
    __syncthreads();
    c = 0;
    m = 0;
    if (threadIdx.x < kBins) {
        const int at = (kBins - 1 - (int)threadIdx.x) * kCopies;
#pragma unroll
        for (int i = 0; i < kCopies; ++i) {
            c += h.cnt[at + i];
            m += h.mass[at + i];
        }
    }
}
// threads 0 .. 255 hold (c, m) of bin 255 - tid -> the sums over the bins ABOVE theirs (integers: the order is immaterial)
__device__ __forceinline__ void scan_from_top(uint32_t c, u64 m, uint32_t& c_above, u64& m_above, uint32_t* wc, u64* wm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t ci = c;
    u64 mi = m;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t oc = __shfl_up(ci, off, 64);
        const u64 om = __shfl_up(mi, off, 64);
        if (lane >= off) {
            ci += oc;
            mi += om;
        }
    }
    __syncthreads();                // the last reader of wc / wm, and of the histogram hist_take read, is done
    if (lane == 63 && wave < kBins / 64) {
        wc[wave] = ci;
        wm[wave] = mi;
    }
    __syncthreads();
    for (int w = 0; w < wave && w < kBins / 64; ++w) {
        ci += wc[w];
        mi += wm[w];
    }
    c_above = ci - c;
    m_above = mi - m;
}

struct Sel {                        // a selected bin / key and the count and mass of everything above it
    int bin;
    uint32_t c_above;
    u64 m_above;
};

// Philox4x32-10 (Salmon et al., SC'11), counter (c0, c1, 0, 0), key (k0, k1) -> word 0
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1) {
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ int count8(const uint4& d, uint32_t key) {
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
    int c = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) c += key16((uint16_t)(w[e >> 1] >> (16 * (e & 1)))) == key;
    return c;
}

// the j-th (1-based) class of the row, in index order, whose key is `key` -> *pick (left alone if there are fewer: never the case for a
// j taken from the histograms).  Order = for_each's three pieces; the 16-byte lanes are cut into one contiguous piece per wave
__device__ __forceinline__ void find_jth(const uint16_t* __restrict__ row, int n, uint32_t key, int j, int* wcnt, int* pick) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 1);
    head = head < n ? head : n;
    const uint4* body = reinterpret_cast<const uint4*>(row + head);
    const int nv = (n - head) >> 3, tail = head + nv * 8;
    const int vpw = (nv + kWaves - 1) / kWaves;
    const int v0 = wave * vpw < nv ? wave * vpw : nv, v1 = v0 + vpw < nv ? v0 + vpw : nv;
    int c = 0;
    for (int v = v0 + lane; v < v1; v += 64) c += count8(body[v], key);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    int hc = 0;
    for (int i = 0; i < head; ++i) hc += key16(row[i]) == key;
    if (j <= hc) {
        if (tid == 0)
            for (int i = 0; i < head; ++i)
                if (key16(row[i]) == key && --j == 0) *pick = i;
        return;
    }
    j -= hc;
    int w = 0;
    for (; w < kWaves; ++w) {
        if (j <= wcnt[w]) break;
        j -= wcnt[w];
    }
    if (w == kWaves) {
        if (tid == 0)
            for (int i = tail; i < n; ++i)
                if (key16(row[i]) == key && --j == 0) *pick = i;
        return;
    }
    if (wave != w) return;
    for (int base = v0; base < v1; base += 64) {       // wave-uniform trip count and exit
        const int v = base + lane;
        uint4 d = make_uint4(0, 0, 0, 0);
        int own = 0;
        if (v < v1) {
            d = body[v];
            own = count8(d, key);
        }
        int incl = own;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        const int total = __shfl(incl, 63, 64);
        if (j <= total) {
            if (incl - own < j && j <= incl) {
                int left = j - (incl - own);
                const uint32_t wd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (key16((uint16_t)(wd[e >> 1] >> (16 * (e & 1)))) == key && --left == 0) *pick = head + v * 8 + e;
            }
            return;
        }
        j -= total;
    }
}

// SPEC (zl_spec_sample_accept's first launch): row r belongs to task r / len_q -- its parameters, seed and draw count are the task's,
// its counter is draws[task] + r % len_q -- and the epilogue writes the row's pick, log-probability and uniform only: draws and the
// batch state are the second launch's.  u_in / u_out / tokens / logprobs stay per row.  !SPEC: len_q is not read
template <bool BF, bool SPEC>
__global__ __launch_bounds__(kThreads) void k_sample_advance(const uint16_t* __restrict__ x, int64_t ld, int n, int len_q, const float* __restrict__ temperature,
                                                             const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                             const int64_t* __restrict__ seeds, int64_t* __restrict__ draws,
                                                             const float* __restrict__ u_in, int32_t* __restrict__ tokens,
                                                             int32_t* __restrict__ positions, int32_t* __restrict__ placement,
                                                             int32_t* __restrict__ valid_lens, int64_t* __restrict__ next_tokens,
                                                             float* __restrict__ logprobs, float* __restrict__ u_out) {
    __shared__ Hist hist;
    __shared__ u64 red[kWaves];
    __shared__ u64 wm[kBins / 64];
    __shared__ uint32_t wc[kBins / 64];
    __shared__ int wcnt[kWaves];
    __shared__ Sel sel_k, sel_v, sel_key;
    __shared__ u64 s_z, s_ck, s_v;
    __shared__ int s_j, s_pick;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pr = SPEC ? r / len_q : r;                                // the row of the parameters and of the generator
    const uint16_t* row = x + (size_t)r * ld;

    // ---- the uniform of this row and call ---------------------------------------------------------------------------------------
    float u = 0.f;
    if (tid == 0) {
        if (u_in) {
            u = u_in[r];
        } else {
            const u64 seed = (u64)seeds[pr], ctr = (u64)draws[pr] + (SPEC ? (u64)(r - pr * len_q) : 0);
            u = (float)(philox_word0((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed, (uint32_t)(seed >> 32)) >> 8) * 0x1p-24f;
            if (!SPEC) draws[r] = (int64_t)(ctr + 1);
        }
        if (u_out) u_out[r] = u;
        u = u >= 0.f ? (u < 1.f ? u : 1.f - 0x1p-24f) : 0.f;            // a caller's u outside [0, 1) (or a NaN) is clamped, never trusted
    }

    // ---- pass 1: zl_argmax_advance's pick -----------------------------------------------------------------------------------------
    u64 best = 0;
    for_each(row, n, [&](uint16_t h, int i) {
        const uint32_t k = (h & 0x7fffu) > H16<BF>::kInf ? 0xffffffffu : key16(h);       // a NaN is the largest value, the first one wins
        const u64 key = ((u64)k << 32) | (uint32_t)~(uint32_t)i;
        best = key > best ? key : best;
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if (lane == 0) red[wave] = best;
    if (tid == 0) s_pick = -1;
    __syncthreads();
    best = red[0];
    for (int w = 1; w < kWaves; ++w) best = red[w] > best ? red[w] : best;
    const uint32_t kmax = (uint32_t)(best >> 32);
    const int amax = (int)~(uint32_t)best;

    const float t_in = temperature[pr];
    const bool greedy = !(t_in > 0.f);
    const float t = greedy ? 1.0f : t_in;
    // a row whose largest value is a NaN, +inf or -inf has no distribution: the arg-max pick, a NaN log-probability
    const bool plain = kmax == 0xffffffffu || kmax == key16((uint16_t)H16<BF>::kInf) || kmax == key16((uint16_t)(H16<BF>::kInf | 0x8000u));
    const float vmax = H16<BF>::f32(unkey16(kmax));
    const int sh = 62 - (n > 1 ? 32 - __clz(n - 1) : 0);
    const float scale = __builtin_bit_cast(float, (uint32_t)(127 + sh) << 23);
    float lse = __builtin_nanf("");

    if (!plain && !(greedy && logprobs == nullptr)) {                   // uniform over the workgroup, as every branch below
        // ---- pass 2: the high byte's histogram, Z ---------------------------------------------------------------------------------
        const int k = greedy ? 0 : top_k[pr];
        const bool k_on = k > 0 && k < n;
        hist_zero(hist);
        for_each(row, n, [&](uint16_t h, int) {
            const uint32_t kk = key16(h);
            if (k_on) hist_count(hist, kk >> 8);                        // the count select is top-k's alone
            hist_mass(hist, kk >> 8, mass_of<BF>(kk, vmax, t, scale));
        });
        uint32_t c1, c1_above;
        u64 m1, m1_above;
        hist_take(hist, c1, m1);
        scan_from_top(c1, m1, c1_above, m1_above, wc, wm);
        if (tid == kBins - 1) s_z = m1_above + m1;
        __syncthreads();
        const u64 z = s_z;                                              // >= 2^sh: the largest value's own mass
        lse = logf((float)((double)z * (double)__builtin_bit_cast(float, (uint32_t)(127 - sh) << 23)));

        if (!greedy) {
            uint32_t c2 = 0, c2_above = 0;
            u64 m2 = 0, m2_above = 0, q2 = 0;
            // the low byte inside one high-byte bin: COUNTS only -- every class of a key has the key's mass, so a bin's mass is
            // count x mass_of(key), one exponential per bin instead of one per class, and sums to the level-1 bin exactly
            auto low_byte = [&](int bin) {
                hist_zero(hist);
                for_each(row, n, [&](uint16_t h, int) {
                    const uint32_t kk = key16(h);
                    if ((int)(kk >> 8) == bin) hist_count(hist, kk & 0xffu);
                });
                hist_take(hist, c2, m2);
                q2 = mass_of<BF>((uint32_t)(bin << 8) | (uint32_t)((kBins - 1 - tid) & 0xff), vmax, t, scale);
                m2 = (u64)c2 * q2;
                scan_from_top(c2, m2, c2_above, m2_above, wc, wm);
            };
            if (k_on) {
                // ---- pass 3: c[k-1], the running mass at the k-th class ---------------------------------------------------------------
                if (tid < kBins && c1_above < (uint32_t)k && (uint32_t)k <= c1_above + c1) sel_k = Sel{kBins - 1 - tid, c1_above, m1_above};
                __syncthreads();
                low_byte(sel_k.bin);
                const uint32_t ca = sel_k.c_above + c2_above;
                if (tid < kBins && ca < (uint32_t)k && (uint32_t)k <= ca + c2) s_ck = sel_k.m_above + m2_above + (u64)((uint32_t)k - ca) * q2;
                __syncthreads();
            }
            if (tid == 0) {                                             // v = ceil(u * cap * Z) in fixed point: c >= v  <=>  c >= ceil(v)
                float tp = top_p[pr];
                tp = tp >= 0.f ? (tp < 1.f ? tp : 1.f) : 0.f;
                double lim = (double)tp * (double)z;
                if (k_on) lim = fmin(lim, (double)s_ck);
                const double vd = ceil((double)u * lim);
                u64 v = vd < 9.0e18 ? (u64)vd : z;
                v = v < z ? v : z;
                if (k_on) v = v < s_ck ? v : s_ck;
                s_v = v;
            }
            __syncthreads();
            const u64 v = s_v;
            if (v > 0) {                                                // v == 0: the first class of the order, the arg-max
                if (tid < kBins && m1_above < v && v <= m1_above + m1) sel_v = Sel{kBins - 1 - tid, c1_above, m1_above};
                __syncthreads();
                const int bin = sel_v.bin;
                if (!(k_on && bin == sel_k.bin)) {
                    // ---- pass 4: the low byte's histogram inside the bin where the running mass reaches v -----------------------------
                    low_byte(bin);
                }
                const u64 ma = sel_v.m_above + m2_above;
                if (tid < kBins && m2 > 0 && ma < v && v <= ma + m2) {
                    const u64 j = (v - ma + q2 - 1) / q2;
                    sel_key.bin = (bin << 8) | (kBins - 1 - tid);
                    s_j = (int)(j < 1 ? 1 : (j > c2 ? c2 : j));
                }
                __syncthreads();
                // ---- pass 5: the j-th class with that value, in index order ------------------------------------------------------------
                find_jth(row, n, (uint32_t)sel_key.bin, s_j, wcnt, &s_pick);
                __syncthreads();
            }
        }
    }

    if (tid == 0) {
        int pick = s_pick;
        pick = pick >= 0 && pick < n ? pick : amax;
        if (tokens) tokens[r] = pick;
        if (!SPEC) {
            if (next_tokens) next_tokens[r] = pick;
            if (positions) positions[r] += 1;
            if (placement) placement[r] += 1;
            if (valid_lens) valid_lens[r] += 1;
        }
        if (logprobs) logprobs[r] = plain ? __builtin_nanf("") : (H16<BF>::f32(row[pick]) - vmax) / t - lse;
    }
}

// zl_spec_sample_accept's second launch: out_tokens / out_logprobs hold the picks of the (b, len_q) rows and their log-probabilities
// (k_sample_advance<.., SPEC> left them); one thread per task finds the longest prefix of its drafts that the picks confirm (a draft
// outside [0, n) equals no pick), pads the rows behind the bonus token with -1 / NaN, advances the task's state by accepted + 1 and
// -- where the generator gave the uniforms -- its draw count by as much: the rows behind the rejection drew nothing that counts
__global__ void k_spec_sample_accept(const int32_t* __restrict__ drafts, int32_t* __restrict__ out_tokens, float* __restrict__ out_logprobs,
                                     int32_t* __restrict__ accepted, int32_t* __restrict__ tokens, int32_t* __restrict__ positions,
                                     int32_t* __restrict__ placement, int32_t* __restrict__ valid_lens, float* __restrict__ logprobs,
                                     int64_t* __restrict__ draws, int b, int len_q) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    int32_t* pk = out_tokens + (int64_t)t * len_q;
    float* lp = out_logprobs ? out_logprobs + (int64_t)t * len_q : nullptr;
    const int32_t* dr = drafts + (int64_t)t * (len_q - 1);
    int a = 0;
    while (a < len_q - 1 && dr[a] == pk[a]) ++a;
    const int32_t last = pk[a];
    for (int j = a + 1; j < len_q; ++j) {
        pk[j] = -1;
        if (lp) lp[j] = __builtin_nanf("");
    }
    accepted[t] = a;
    if (tokens) tokens[t] = last;
    if (positions) positions[t] += a + 1;
    if (placement) placement[t] += a + 1;
    if (valid_lens) valid_lens[t] += a + 1;
    if (logprobs) logprobs[t] = lp[a];
    if (draws) draws[t] += a + 1;
}

}  // namespace

extern "C" {

int zl_sample_advance(const void* logits, int type, int64_t rows, int64_t n, int64_t ld, const float* temperature, const int32_t* top_k,
                      const float* top_p, const int64_t* seeds, int64_t* draws, const float* u_in, int32_t* tokens, int32_t* positions,
                      int32_t* placement, int32_t* valid_lens, int64_t* next_tokens, float* logprobs, float* u_out, zl_stream_t s) {
    ZL_CHECK_ARG(logits && temperature && top_k && top_p, ZL_EINVAL);
    ZL_CHECK_ARG((seeds && draws) || u_in, ZL_EINVAL);
    ZL_CHECK_ARG(tokens || next_tokens, ZL_EINVAL);
    ZL_CHECK_ARG(rows >= 1 && n >= 1 && ld >= n && n < ((int64_t)1 << 31) && rows < ((int64_t)1 << 31), ZL_ESHAPE);
    ZL_CHECK_ARG(type == ZL_T_F16 || type == ZL_T_BF16, ZL_EDTYPE);
    const dim3 g((unsigned)rows), b(kThreads);
    hipStream_t hs = (hipStream_t)s;
    if (type == ZL_T_F16)
        hipLaunchKernelGGL((k_sample_advance<false, false>), g, b, 0, hs, (const uint16_t*)logits, ld, (int)n, 1, temperature, top_k, top_p, seeds, draws,
                           u_in, tokens, positions, placement, valid_lens, next_tokens, logprobs, u_out);
    else
        hipLaunchKernelGGL((k_sample_advance<true, false>), g, b, 0, hs, (const uint16_t*)logits, ld, (int)n, 1, temperature, top_k, top_p, seeds, draws,
                           u_in, tokens, positions, placement, valid_lens, next_tokens, logprobs, u_out);
    return zl_launch_status();
}

int zl_spec_sample_accept(const void* logits, int type, int64_t b, int64_t len_q, int64_t n, int64_t ld, const int32_t* drafts,
                          const float* temperature, const int32_t* top_k, const float* top_p, const int64_t* seeds, int64_t* draws,
                          const float* u_in, int32_t* tokens, int32_t* positions, int32_t* placement, int32_t* valid_lens,
                          int32_t* accepted, int32_t* out_tokens, float* out_logprobs, float* logprobs, float* u_out, zl_stream_t s) {
    ZL_CHECK_ARG(logits && temperature && top_k && top_p && drafts && accepted && out_tokens, ZL_EINVAL);
    ZL_CHECK_ARG((seeds && draws) || u_in, ZL_EINVAL);
    ZL_CHECK_ARG(out_logprobs || !logprobs, ZL_EINVAL);                 // the task's log-probability is read from its rows'
    ZL_CHECK_ARG(b >= 1 && len_q >= 2 && len_q <= 32 && n >= 1 && ld >= n && n < ((int64_t)1 << 31) && b < ((int64_t)1 << 31) &&
                     b * len_q < ((int64_t)1 << 31),
                 ZL_ESHAPE);
    ZL_CHECK_ARG(type == ZL_T_F16 || type == ZL_T_BF16, ZL_EDTYPE);
    // the picks: one 1024-thread workgroup per logit row, zl_sample_advance's kernel under the task's parameters, into out_tokens
    const dim3 g((unsigned)(b * len_q)), blk(kThreads);
    hipStream_t hs = (hipStream_t)s;
    if (type == ZL_T_F16)
        hipLaunchKernelGGL((k_sample_advance<false, true>), g, blk, 0, hs, (const uint16_t*)logits, ld, (int)n, (int)len_q, temperature, top_k,
                           top_p, seeds, draws, u_in, out_tokens, nullptr, nullptr, nullptr, nullptr, out_logprobs, u_out);
    else
        hipLaunchKernelGGL((k_sample_advance<true, true>), g, blk, 0, hs, (const uint16_t*)logits, ld, (int)n, (int)len_q, temperature, top_k,
                           top_p, seeds, draws, u_in, out_tokens, nullptr, nullptr, nullptr, nullptr, out_logprobs, u_out);
    const int e = zl_launch_status();
    if (e) return e;
    hipLaunchKernelGGL(k_spec_sample_accept, dim3((unsigned)((b + 63) / 64)), dim3(64), 0, hs, drafts, out_tokens, out_logprobs, accepted, tokens,
                       positions, placement, valid_lens, logprobs, u_in ? nullptr : draws, (int)b, (int)len_q);
    return zl_launch_status();
}

}  // extern "C"
