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
//   zl_sample_advance_ex / zl_spec_sample_accept_ex / zl_seen_mark   the same picks with the reference generator's repetition and
//                       presence penalties (src/generator/batch_generator.cpp:1670-1692) applied INSIDE the walk: a task's emitted tokens
//                       are a bitmap in global memory (bit i & 31 of word i >> 5), a class whose bit is set is read as
//                       zl_repetition_penalty's value of it -- again a 16-bit pattern -- and everything above selects on that pattern.
//                       The logits in memory are left alone.  Pass 1 and the last walk of pass 5 stream the row with the set's classes
//                       masked (a 16-byte lane of eight classes fetches the one or two bitmap words that cover it; a row of a
//                       speculative step adds the drafts in front of it through a 256-bit LDS filter keyed by i & 255, and compares
//                       ids only where the filter hits) and take the set's classes from a walk over the bitmap itself.  The histogram
//                       passes stream the STORED row exactly as without a penalty and then move each class of the set from the bin of
//                       its stored pattern to the bin of its penalised one -- the histograms are integers, so this is exact -- which
//                       costs them a walk over the bitmap (n / 32 words) and nothing per class.  PEN = false compiles none of it.
//   zl_sample_advance_opts / zl_spec_sample_accept_opts   the same picks with the reference generator's logit bias
//                       (src/generator/batch_generator.cpp:1709-1729) added behind the penalty, and the top-N classes of every row with
//                       their log-probabilities (:923-948).  The bias set is a second bitmap beside seen plus an ascending id list:
//                       the "set" of everything above becomes the union of the two bitmaps, and a class of it is read as "penalised
//                       if in seen, then T(f32(y) + f32(T(bias))) if its bias bit is set and the list holds it" (a binary search, only
//                       where a bit hits) -- again a 16-bit pattern.  Top-N is one more COUNT select on the same histograms (the key
//                       of the N-th class), find_jth only where the N-th place cuts a run of equal values, one gather stream into an
//                       LDS list of min(N, n) candidates, and a rank by counting.  sample_row<.., MODE 2> below; MODE 0 / 1 are the
//                       kernels above, unchanged.
//   zl_sample_advance_fsm / zl_spec_sample_accept_fsm   the same picks under a TOKEN AUTOMATON: a DFA over token ids, resident on the
//                       device and shared by every row -- per state a dense allow-bitmap over the vocabulary (seen's layout), a
//                       default next state and an ascending exception list (CSR).  A row owns one int32, its state; a class whose
//                       bit is clear in the state's bitmap is read as -inf WHEREVER a stored pattern is loaded (Mask below: a 16-byte
//                       lane fetches the one or two bitmap words that cover it and selects branchlessly -- the disallowed set is
//                       dense, so nothing loops per bit), in front of the penalty and the bias; after the pick one wave advances the
//                       state (fsm_delta: a 64-ary search of the exception list, a few dependent loads).  A row of a speculative
//                       step first walks its task's state over the drafts in front of it.  sample_row<.., MODE 3>; a state outside
//                       [0, S) leaves the row unconstrained.  MODE 0 / 1 / 2 never see a Mask.
#include <hip/hip_runtime.h>

#include <type_traits>

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

// float -> the 16-bit pattern, one rounding to nearest even: the instructions of sampling_ops.hip's ET<>::cvt, so that a penalised
// class has the pattern zl_repetition_penalty would have stored
template <bool BF>
__device__ __forceinline__ uint16_t cvt16(float f) {
    if (BF) {
        uint32_t u = __builtin_bit_cast(uint32_t, f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    }
    asm volatile("" : "+v"(f));
    return __builtin_bit_cast(uint16_t, (_Float16)f);
}

constexpr int kFilt = 256;         // bits of the draft filter of a speculative row
constexpr int kMaxDrafts = 31;     // zl_spec_sample_accept's row limit - 1

struct NoPen {                      // PEN = false: a class is read as it is stored, and nothing below is compiled
    static constexpr bool on = false;
};
// what the _opts entry points add to a launch (one kernel argument; the instantiations without OPT never read it)
struct Opts {
    const int32_t* bias_ids;        // (rows or b, bias_ld): a row's first bias_cnt ids, ascending
    const float* bias_vals;
    const int32_t* bias_cnt;
    int64_t bias_ld;
    const uint32_t* bias_bits;      // (rows or b, bias_bits_ld): seen's layout
    int64_t bias_bits_ld;
    int top_n;
    int32_t* top_ids;               // (rows, top_n)
    float* top_lp;
};
constexpr int kMaxTop = 32;        // top_n's limit: one candidate per lane of half a wave
// what the _fsm entry points add to a launch (one kernel argument of the MODE 3 kernels alone)
struct Fsm {
    const uint32_t* mask;           // (S, mask_ld): bit i of state s set <=> token i is allowed in s
    int64_t mask_ld;
    const int32_t* dflt;            // (S): the next state of an allowed token without an exception entry
    const int32_t* exc_off;         // (S + 1): state s owns the entries exc_off[s] .. exc_off[s + 1] - 1
    const int32_t* exc_tok;         // (E): ascending and distinct inside a state
    const int32_t* exc_next;        // (E)
    int S, E;
    int32_t* state;                 // (rows or b), in place
    int32_t* row_states;            // SPEC: (b, len_q), the state behind every row's pick
};

struct NoMask {                     // MODE 0 / 1 / 2: a stored pattern is what the row holds
    static constexpr bool on = false;
};
// MODE 3: the row's view of its stored patterns under its state's allow-bitmap; bits == NULL: an unconstrained row (uniform over the
// workgroup), read as stored
template <bool BF>
struct Mask {
    static constexpr bool on = true;
    static constexpr uint32_t kNeg = H16<BF>::kInf | 0x8000u;
    const uint32_t* bits;
    __device__ __forceinline__ uint16_t at(uint16_t h, int i) const {
        if (!bits) return h;
        return (bits[i >> 5] >> (i & 31) & 1u) ? h : (uint16_t)kNeg;
    }
    // the eight classes i0 .. i0 + 7 of one 16-byte lane; the caller has i0 + 7 < n, so both words lie inside ceil(n / 32)
    __device__ __forceinline__ uint4 lane(uint4 d, int i0) const {
        if (!bits) return d;
        const uint32_t lo = bits[i0 >> 5], hi = bits[(i0 + 7) >> 5];
        const uint32_t m = (uint32_t)((((u64)hi << 32) | lo) >> (i0 & 31));
        auto sel = [](uint32_t w, uint32_t b2) {
            const uint32_t keep = ((0u - (b2 & 1u)) & 0xffffu) | ((0u - ((b2 >> 1) & 1u)) & 0xffff0000u);
            return (w & keep) | ((kNeg | (kNeg << 16)) & ~keep);
        };
        return make_uint4(sel(d.x, m), sel(d.y, m >> 2), sel(d.z, m >> 4), sel(d.w, m >> 6));
    }
};
// every read of a stored pattern goes through these two
template <class M>
__device__ __forceinline__ uint16_t ld1(const uint16_t* __restrict__ row, int i, const M& mk) {
    if constexpr (M::on) return mk.at(row[i], i);
    else return row[i];
}
template <class M>
__device__ __forceinline__ uint4 ld8(const uint4* __restrict__ body, int v, int i0, const M& mk) {
    if constexpr (M::on) return mk.lane(body[v], i0);
    else return body[v];
}

// delta(s, tok) by ONE WHOLE WAVE (every lane calls it with the same arguments and gets the same result): s outside [0, S), tok outside
// [0, n) or not allowed in s -> s; else the exception's target where the list of s holds tok, else the default.  The list is searched
// 64 ways at a time: 5000 entries take three dependent loads where a binary search takes thirteen
__device__ __forceinline__ int fsm_delta(const Fsm& a, int s, int tok, int n) {
    if (s < 0 || s >= a.S || tok < 0 || tok >= n) return s;
    if (!(a.mask[(size_t)s * a.mask_ld + (tok >> 5)] >> (tok & 31) & 1u)) return s;
    const int lane = threadIdx.x & 63;
    int lo = a.exc_off[s], hi = a.exc_off[s + 1];
    lo = lo < 0 ? 0 : (lo > a.E ? a.E : lo);                            // never outside the lists, whatever the offsets hold
    hi = hi < lo ? lo : (hi > a.E ? a.E : hi);
    while (hi - lo > 64) {
        const int step = (hi - lo + 63) >> 6;
        const int idx = lo + lane * step;
        bool le = false;
        if (idx < hi) le = a.exc_tok[idx] <= tok;
        const int c = __popcll(__ballot(le));                           // ascending: a prefix of the lanes
        if (c == 0) return a.dflt[s];
        lo += (c - 1) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    bool eq = false;
    if (lo + lane < hi) eq = a.exc_tok[lo + lane] == tok;
    const u64 hit = __ballot(eq);
    return hit ? a.exc_next[lo + __ffsll((unsigned long long)hit) - 1] : a.dflt[s];
}

// the row's view of its penalty: the set = the task's bitmap, and for row i of a speculative step the in-range drafts 0 .. i - 1
// OPT (the _opts entry points): the set is the union of that and of the task's BIAS bitmap; a class of the set is read as "the
// penalty if it is in seen or a draft, then + bias if its bias bit is set and the task's id list holds it" (a binary search, paid only
// where the bit hits).  Either bitmap may be missing (NULL): a bias needs no penalty, top-N needs neither
template <bool BF, bool SPEC, bool OPT>
struct Pen {
    static constexpr bool on = true;
    const uint32_t* seen;           // the task's bitmap row (global); OPT: or NULL
    const uint32_t* bbits;          // OPT: the task's bias bitmap row (global) or NULL
    const int32_t* bids;            // OPT: the task's bias ids, bcnt of them ascending
    const float* bvals;
    int bcnt;
    const uint32_t* filt;           // SPEC: kFilt bits, bit (id & 255) of every draft in front of the row (LDS)
    const int32_t* ids;             // SPEC: those drafts, -1 where out of range (LDS)
    int nd;                         // SPEC: how many
    float f, tp;                    // T(factor), T(presence) widened
    bool sub;                       // presence != 0: it takes precedence

    // k_repetition_penalty's expression
    __device__ __forceinline__ uint16_t apply(uint16_t h) const {
        const float l = H16<BF>::f32(h);
        const float r = sub ? l - tp : (l < 0.f ? l * f : l / f);
        return cvt16<BF>(r);
    }
    // word w of the set's bitmap
    __device__ __forceinline__ uint32_t sw(int w) const {
        if constexpr (OPT) return seen ? seen[w] : 0u;
        else return seen[w];
    }
    __device__ __forceinline__ uint32_t bw(int w) const { return bbits ? bbits[w] : 0u; }
    __device__ __forceinline__ uint32_t uw(int w) const {
        if constexpr (OPT) return sw(w) | bw(w);
        else return seen[w];
    }
    // OPT: the class as the pick sees it -- k_repetition_penalty's expression where the penalty's set holds it, then k_scatter_logits'
    // add, T(f32(y) + f32(T(bias))), where the bias set does.  A bias bit without a list entry leaves the class unbiased
    __device__ __forceinline__ uint16_t modified(uint16_t h, int i) const {
        bool in = sw(i >> 5) >> (i & 31) & 1u;
        if constexpr (SPEC)
            if (!in && (filt[(i & (kFilt - 1)) >> 5] >> (i & 31) & 1u)) in = draft(i);
        uint16_t y = in ? apply(h) : h;
        if (bw(i >> 5) >> (i & 31) & 1u) {
            int lo = 0, hi = bcnt;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (bids[mid] < i) lo = mid + 1;
                else hi = mid;
            }
            if (lo < bcnt && bids[lo] == i) y = cvt16<BF>(H16<BF>::f32(y) + H16<BF>::f32(cvt16<BF>(bvals[lo])));
        }
        return y;
    }
    __device__ __forceinline__ bool draft(int i) const {
        bool hit = false;
        for (int j = 0; j < nd; ++j) hit |= ids[j] == i;
        return hit;
    }
    // bit e <=> class i0 + e is in the set, e < 8; the caller has i0 + 7 < n, so both words lie inside the row's ceil(n / 32)
    __device__ __forceinline__ uint32_t mask8(int i0) const {
        const uint32_t lo = uw(i0 >> 5), hi = uw((i0 + 7) >> 5);        // the same word twice where the lane does not straddle
        uint32_t m = (uint32_t)((((u64)hi << 32) | lo) >> (i0 & 31)) & 0xffu;
        if constexpr (SPEC) {
            const int p = i0 & (kFilt - 1);
            const uint32_t flo = filt[p >> 5], fhi = filt[((p + 7) >> 5) & (kFilt / 32 - 1)];
            uint32_t fm = (uint32_t)((((u64)fhi << 32) | flo) >> (p & 31)) & 0xffu & ~m;
            while (fm) {
                const int e = __ffs((int)fm) - 1;
                fm &= fm - 1;
                if (draft(i0 + e)) m |= 1u << e;
            }
        }
        return m;
    }
    // the set classes of one 16-byte lane, one at a time: sets are sparse (a task's emitted tokens), so a wave takes the loop once or
    // twice where eight predicated copies of the arithmetic would cost every lane of every pass
    __device__ __forceinline__ void apply8(uint4& d, uint32_t m, int i0) const {
        while (m) {
            const int e = __ffs((int)m) - 1;
            m &= m - 1;
            const int wi = e >> 1, sft = 16 * (e & 1);
            const uint32_t w = wi == 0 ? d.x : (wi == 1 ? d.y : (wi == 2 ? d.z : d.w));
            uint16_t y;
            if constexpr (OPT) y = modified((uint16_t)(w >> sft), i0 + e);
            else y = apply((uint16_t)(w >> sft));
            const uint32_t nw = (w & ~(0xffffu << sft)) | ((uint32_t)y << sft);
            d.x = wi == 0 ? nw : d.x;
            d.y = wi == 1 ? nw : d.y;
            d.z = wi == 2 ? nw : d.z;
            d.w = wi == 3 ? nw : d.w;
        }
    }
    // one class, i < n
    __device__ __forceinline__ bool has(int i) const {
        bool in = uw(i >> 5) >> (i & 31) & 1u;
        if constexpr (SPEC)
            if (!in && (filt[(i & (kFilt - 1)) >> 5] >> (i & 31) & 1u)) in = draft(i);
        return in;
    }
    __device__ __forceinline__ uint16_t one(uint16_t h, int i) const {
        if constexpr (OPT) return modified(h, i);
        else return has(i) ? apply(h) : h;
    }
    // g(stored pattern, penalised pattern, index) for every class of the set, each once, in no particular order: the bitmap's words
    // below n over the threads -- 4 loads per thread at 128 256 classes, and as many trips as a task has emitted tokens there --
    // then (SPEC) the drafts in front of the row that the bitmap does not hold, one thread each
    template <class M, class G>
    __device__ __forceinline__ void for_set(const uint16_t* __restrict__ row, int n, const M& mk, G&& g) const {
        const int nw = (n + 31) >> 5;
        for (int w = threadIdx.x; w < nw; w += kThreads) {
            uint32_t bits = uw(w);
            if (w == nw - 1 && (n & 31)) bits &= (1u << (n & 31)) - 1u;
            while (bits) {
                const int i = w * 32 + __ffs((int)bits) - 1;
                bits &= bits - 1;
                const uint16_t h = ld1(row, i, mk);
                if constexpr (OPT) g(h, modified(h, i), i);
                else g(h, apply(h), i);
            }
        }
        if constexpr (SPEC) {
            const int t = threadIdx.x;
            if (t < nd) {
                const int id = ids[t];
                bool fresh = id >= 0;
                if (fresh) fresh = !(uw(id >> 5) >> (id & 31) & 1u);    // OPT: a draft with a bias bit came with the bitmaps' walk
                for (int j = 0; j < t; ++j) fresh &= ids[j] != id;
                if (fresh) {
                    const uint16_t h = ld1(row, id, mk);
                    g(h, apply(h), id);
                }
            }
        }
    }
};

// f(pattern, index) for every element of the row, in no particular order: up to 7 elements in front of the first 16-byte boundary,
// 16-byte lanes with kLoads loads in flight, up to 7 elements behind the last whole lane.  pen.on: the pattern is the penalised one --
// the streaming loop leaves the set's classes out (the mask of a lane is one or two bitmap words) and pen.for_set brings them in
// mk.on (MODE 3): every pattern is loaded through the row's allow-bitmap first
template <class P, class M, class F>
__device__ __forceinline__ void for_each(const uint16_t* __restrict__ row, int n, const P& pen, const M& mk, F&& f) {
    const int tid = threadIdx.x;
    int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 1);
    head = head < n ? head : n;
    auto one = [&](int i) {
        if constexpr (P::on) {
            if (!pen.has(i)) f(ld1(row, i, mk), i);
        } else {
            f(ld1(row, i, mk), i);
        }
    };
    if (tid < head) one(tid);
    const uint4* body = reinterpret_cast<const uint4*>(row + head);
    const int nv = (n - head) >> 3;
    for (int c0 = tid; c0 < nv; c0 += kLoads * kThreads) {
        uint4 v4[kLoads];
        uint32_t m8[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int c = c0 + u * kThreads;
            v4[u] = ld8(body, c < nv ? c : c0, head + (c < nv ? c : c0) * 8, mk);
            if constexpr (P::on) m8[u] = pen.mask8(head + (c < nv ? c : c0) * 8);
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int c = c0 + u * kThreads;
            if (c < nv) {
                const uint32_t w[4] = {v4[u].x, v4[u].y, v4[u].z, v4[u].w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if constexpr (P::on) {
                        if (!(m8[u] >> e & 1u)) f((uint16_t)(w[e >> 1] >> (16 * (e & 1))), head + c * 8 + e);
                    } else {
                        f((uint16_t)(w[e >> 1] >> (16 * (e & 1))), head + c * 8 + e);
                    }
                }
            }
        }
    }
    for (int i = head + nv * 8 + tid; i < n; i += kThreads) one(i);
    if constexpr (P::on) pen.for_set(row, n, mk, [&](uint16_t, uint16_t ph, int i) { f(ph, i); });
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
// a class moves from the bin of its stored pattern to the bin of its penalised one: integers modulo 2^32 / 2^64, so a copy may wrap
// below zero while the sum over the copies that hist_take forms is exact
__device__ __forceinline__ void hist_uncount(Hist& h, uint32_t bin) {
    atomicAdd(&h.cnt[(int)bin * kCopies + (threadIdx.x & (kCopies - 1))], 0xffffffffu);
}
__device__ __forceinline__ void hist_unmass(Hist& h, uint32_t bin, u64 q) {
    if (q) atomicAdd(&h.mass[(int)bin * kCopies + (threadIdx.x & (kCopies - 1))], (u64)0 - q);
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
// j taken from the histograms).  Order = for_each's three pieces; the 16-byte lanes are cut into one contiguous piece per wave.
// pen.on: the keys are the penalised patterns', as in for_each
template <class P, class M>
__device__ __forceinline__ void find_jth(const uint16_t* __restrict__ row, int n, const P& pen, const M& mk, uint32_t key, int j, int* wcnt,
                                         int* pick) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 1);
    head = head < n ? head : n;
    const uint4* body = reinterpret_cast<const uint4*>(row + head);
    const int nv = (n - head) >> 3, tail = head + nv * 8;
    const int vpw = (nv + kWaves - 1) / kWaves;
    const int v0 = wave * vpw < nv ? wave * vpw : nv, v1 = v0 + vpw < nv ? v0 + vpw : nv;
    auto at = [&](int i) -> uint16_t {
        if constexpr (P::on) return pen.one(ld1(row, i, mk), i);
        else return ld1(row, i, mk);
    };
    auto lane8 = [&](int v) -> uint4 {
        uint4 d = ld8(body, v, head + v * 8, mk);
        if constexpr (P::on) pen.apply8(d, pen.mask8(head + v * 8), head + v * 8);
        return d;
    };
    int c = 0;
    for (int v = v0 + lane; v < v1; v += 64) c += count8(ld8(body, v, head + v * 8, mk), key);        // the stored patterns; pen.on: corrected below
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    if constexpr (P::on) {
        pen.for_set(row, n, mk, [&](uint16_t raw, uint16_t ph, int i) {
            const int d = (int)(key16(ph) == key) - (int)(key16(raw) == key);
            if (d != 0 && i >= head && i < tail) atomicAdd(&wcnt[((i - head) >> 3) / vpw], d);
        });
        __syncthreads();
    }
    int hc = 0;
    for (int i = 0; i < head; ++i) hc += key16(at(i)) == key;
    if (j <= hc) {
        if (tid == 0)
            for (int i = 0; i < head; ++i)
                if (key16(at(i)) == key && --j == 0) *pick = i;
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
                if (key16(at(i)) == key && --j == 0) *pick = i;
        return;
    }
    if (wave != w) return;
    for (int base = v0; base < v1; base += 64) {       // wave-uniform trip count and exit
        const int v = base + lane;
        uint4 d = make_uint4(0, 0, 0, 0);
        int own = 0;
        if (v < v1) {
            d = lane8(v);
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
// PEN (the _ex entry points): the row's classes are read through Pen -- rep_penalty / presence / seen row pr, and under SPEC the
// drafts in front of the row -- and !SPEC sets the pick's bit in the row's bitmap: one workgroup owns the row, every read of it lies
// in front of a barrier that thread 0 has passed.  !PEN: the four arguments and drafts are not read
// MODE 2 (the _opts entry points with a bias or top_n > 0): MODE 1's reading through Pen<.., OPT> -- seen may be NULL then: no penalty,
// no drafts, no bit set -- and, top_n > 0, the row's first min(top_n, n) classes of the order with their log-probabilities into
// o.top_ids / o.top_lp (row r's top_n slots; -1 / NaN behind min(top_n, n) and on a plain row):
//   2   counts the high byte whenever top-N is on, and runs for a greedy row without logprobs too
//   3n  the low-byte count pass inside the bin of the N-th class (shared with pass 3 where that is top-k's bin) -> the key k_N of the
//       N-th class, the count above it (< N) and how many classes of k_N belong to the N
//   5n  only where fewer than all classes of k_N belong: find_jth, the index of the last one that does
//   6n  one stream: the classes above k_N and those of k_N up to that index into an LDS list of exactly min(top_n, n) entries (the
//       arrival order does not matter); a candidate's slot is the number of candidates in front of it by (key descending, index
//       ascending), its log-probability the pick's expression on its pattern
// MODE 3 (the _fsm entry points with an automaton): MODE 2's reading of a row whose stored patterns pass through Mask first.  Wave 0
// reads the row's state -- SPEC: the task's state walked over the drafts in front of the row -- before pass 1, and advances it over
// the pick behind the epilogue: !SPEC into fa.state[r], SPEC into fa.row_states[r] (the second launch picks the accepted row's)
// The body of the kernels below: k_sample_advance keeps the argument list it always had, k_sample_advance_opts adds o, _fsm adds fa
template <bool BF, bool SPEC, int MODE>
__device__ __forceinline__ void sample_row(const uint16_t* __restrict__ x, int64_t ld, int n, int len_q, const float* __restrict__ temperature,
                                           const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                           const int64_t* __restrict__ seeds, int64_t* __restrict__ draws, const float* __restrict__ u_in,
                                           int32_t* __restrict__ tokens, int32_t* __restrict__ positions, int32_t* __restrict__ placement,
                                           int32_t* __restrict__ valid_lens, int64_t* __restrict__ next_tokens, float* __restrict__ logprobs,
                                           float* __restrict__ u_out, const float* __restrict__ rep_penalty,
                                           const float* __restrict__ presence, uint32_t* seen, int64_t seen_ld,
                                           const int32_t* __restrict__ drafts, const Opts& o, const Fsm& fa) {
    constexpr bool PEN = MODE >= 1, OPT = MODE >= 2, FSM = MODE == 3;
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

    typedef typename std::conditional<PEN, Pen<BF, SPEC, OPT>, NoPen>::type P;
    typedef typename std::conditional<FSM, Mask<BF>, NoMask>::type M;
    P pen;
    M mk;
    int st = -1;                                                        // FSM: the row's state
    bool con = false;                                                   // ... and whether it constrains the row
    if constexpr (FSM) {
        __shared__ int s_state;
        if (wave == 0) {
            int s = fa.state[pr];
            if constexpr (SPEC)
                for (int j = 0; j < r - pr * len_q; ++j) s = fsm_delta(fa, s, drafts[(size_t)pr * (len_q - 1) + j], n);
            if (lane == 0) s_state = s;
        }
        __syncthreads();
        st = s_state;
        con = st >= 0 && st < fa.S;
        mk.bits = con ? fa.mask + (size_t)st * fa.mask_ld : nullptr;
    }
    const bool sn = !OPT || seen != nullptr;                            // a penalty set: always under MODE 1
    if constexpr (PEN) {
        __shared__ uint32_t s_filt[kFilt / 32];
        __shared__ int32_t s_ids[kMaxDrafts];
        const float pp = sn ? presence[pr] : 0.f;
        pen.seen = sn ? seen + (size_t)pr * seen_ld : nullptr;
        pen.filt = s_filt;
        pen.ids = s_ids;
        pen.nd = 0;
        pen.sub = pp != 0.f;
        pen.tp = H16<BF>::f32(cvt16<BF>(pp));
        pen.f = H16<BF>::f32(cvt16<BF>(sn ? rep_penalty[pr] : 1.f));
        if constexpr (OPT) {
            const bool bs = o.bias_ids != nullptr;                      // the launcher: all four bias pointers or none
            int bc = bs ? o.bias_cnt[pr] : 0;
            bc = bc < 0 ? 0 : (bc > (int)o.bias_ld ? (int)o.bias_ld : bc);      // never past the task's list
            pen.bbits = bs ? o.bias_bits + (size_t)pr * o.bias_bits_ld : nullptr;
            pen.bids = bs ? o.bias_ids + (size_t)pr * o.bias_ld : nullptr;
            pen.bvals = bs ? o.bias_vals + (size_t)pr * o.bias_ld : nullptr;
            pen.bcnt = bc;
        } else {
            pen.bbits = nullptr;
            pen.bids = nullptr;
            pen.bvals = nullptr;
            pen.bcnt = 0;
        }
        if constexpr (SPEC) {
            const int i = sn ? r - pr * len_q : 0;                      // <= kMaxDrafts: the launcher's len_q <= 32; no set, no drafts
            pen.nd = i;
            if (tid < kFilt / 32) s_filt[tid] = 0;
            __syncthreads();
            if (tid < i) {
                const int32_t d = drafts[(size_t)pr * (len_q - 1) + tid];
                const bool in = d >= 0 && d < n;
                s_ids[tid] = in ? d : -1;
                if (in) atomicOr(&s_filt[(d & (kFilt - 1)) >> 5], 1u << (d & 31));
            }
            __syncthreads();
        }
    }

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
    for_each(row, n, pen, mk, [&](uint16_t h, int i) {
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

    (void)sn;
    bool topn_on = false;
    if constexpr (OPT) topn_on = o.top_n > 0;
    if (!plain && !(greedy && logprobs == nullptr && !topn_on)) {       // uniform over the workgroup, as every branch below
        // ---- pass 2: the high byte's histogram, Z ---------------------------------------------------------------------------------
        const int k = greedy ? 0 : top_k[pr];
        const bool k_on = k > 0 && k < n;
        const bool c_on = k_on || topn_on;                              // the count selects: top-k's and top-N's
        hist_zero(hist);
        // PEN, here and in the low byte's pass: the stored row as it is, then the set's classes move to their penalised bins
        for_each(row, n, NoPen(), mk, [&](uint16_t h, int) {
            const uint32_t kk = key16(h);
            if (c_on) hist_count(hist, kk >> 8);
            hist_mass(hist, kk >> 8, mass_of<BF>(kk, vmax, t, scale));
        });
        if constexpr (PEN)
            pen.for_set(row, n, mk, [&](uint16_t raw, uint16_t ph, int) {
                const uint32_t kr = key16(raw), kp = key16(ph);
                if (kr == kp) return;
                if (c_on) {
                    hist_uncount(hist, kr >> 8);
                    hist_count(hist, kp >> 8);
                }
                hist_unmass(hist, kr >> 8, mass_of<BF>(kr, vmax, t, scale));
                hist_mass(hist, kp >> 8, mass_of<BF>(kp, vmax, t, scale));
            });
        uint32_t c1, c1_above;
        u64 m1, m1_above;
        hist_take(hist, c1, m1);
        scan_from_top(c1, m1, c1_above, m1_above, wc, wm);
        if (tid == kBins - 1) s_z = m1_above + m1;
        __syncthreads();
        const u64 z = s_z;                                              // >= 2^sh: the largest value's own mass
        lse = logf((float)((double)z * (double)__builtin_bit_cast(float, (uint32_t)(127 - sh) << 23)));

        uint32_t c2 = 0, c2_above = 0;
        u64 m2 = 0, m2_above = 0, q2 = 0;
        // the low byte inside one high-byte bin: COUNTS only -- every class of a key has the key's mass, so a bin's mass is
        // count x mass_of(key), one exponential per bin instead of one per class, and sums to the level-1 bin exactly
        auto low_byte = [&](int bin) {
            hist_zero(hist);
            for_each(row, n, NoPen(), mk, [&](uint16_t h, int) {
                const uint32_t kk = key16(h);
                if ((int)(kk >> 8) == bin) hist_count(hist, kk & 0xffu);
            });
            if constexpr (PEN)
                pen.for_set(row, n, mk, [&](uint16_t raw, uint16_t ph, int) {
                    const uint32_t kr = key16(raw), kp = key16(ph);
                    if (kr == kp) return;
                    if ((int)(kr >> 8) == bin) hist_uncount(hist, kr & 0xffu);
                    if ((int)(kp >> 8) == bin) hist_count(hist, kp & 0xffu);
                });
            hist_take(hist, c2, m2);
            q2 = mass_of<BF>((uint32_t)(bin << 8) | (uint32_t)((kBins - 1 - tid) & 0xff), vmax, t, scale);
            m2 = (u64)c2 * q2;
            scan_from_top(c2, m2, c2_above, m2_above, wc, wm);
        };
        int cur = -1;                                                   // OPT: the bin that c2 / m2 / q2 describe now
        // OPT, top_n > 0: passes 3n, 5n and 6n; behind pass 3 on a sampling row, on its own on a greedy one
        auto top_rows = [&]() __attribute__((always_inline)) {
            if constexpr (OPT) {
                __shared__ Sel sel_n;
                __shared__ uint32_t s_kn, c_key[kMaxTop];
                __shared__ int s_need, s_all, s_last, s_nc, c_idx[kMaxTop];
                __shared__ uint16_t c_pat[kMaxTop];
                const int top = o.top_n;                                // 1 .. kMaxTop: the launcher
                const uint32_t ne = (uint32_t)(top < n ? top : n);
                // ---- pass 3n: the key of the N-th class of the order, by count -------------------------------------------------------
                if (tid < kBins && c1_above < ne && ne <= c1_above + c1) sel_n = Sel{kBins - 1 - tid, c1_above, 0};
                if (tid == 0) {
                    s_nc = 0;
                    s_last = n;                                         // every class of k_N belongs, unless pass 5n says otherwise
                }
                __syncthreads();
                if (sel_n.bin != cur) {
                    low_byte(sel_n.bin);
                    cur = sel_n.bin;
                }
                const uint32_t ca = sel_n.c_above + c2_above;
                if (tid < kBins && ca < ne && ne <= ca + c2) {
                    s_kn = (uint32_t)(sel_n.bin << 8) | (uint32_t)(kBins - 1 - tid);
                    s_need = (int)(ne - ca);
                    s_all = ne - ca == c2;
                }
                __syncthreads();
                const uint32_t kn = s_kn;
                if (!s_all) {
                    // ---- pass 5n: the run of k_N is cut: the index of its last class that belongs ---------------------------------------
                    find_jth(row, n, pen, mk, kn, s_need, wcnt, &s_last);
                    __syncthreads();
                }
                const int last = s_last;
                // ---- pass 6n: the candidates, exactly ne of them ----------------------------------------------------------------------
                for_each(row, n, pen, mk, [&](uint16_t h, int i) {
                    const uint32_t kk = key16(h);
                    if (kk > kn || (kk == kn && i <= last)) {
                        const int at = atomicAdd(&s_nc, 1);
                        if (at < kMaxTop) {
                            c_key[at] = kk;
                            c_idx[at] = i;
                            c_pat[at] = h;
                        }
                    }
                });
                __syncthreads();
                if (tid < top) {
                    const int nc = s_nc < top ? s_nc : top;             // == ne; the clamp keeps every slot below inside the row's top
                    int32_t* ti = o.top_ids + (size_t)r * top;
                    float* tl = o.top_lp + (size_t)r * top;
                    if (tid < nc) {
                        const uint32_t mk = c_key[tid];
                        const int mi = c_idx[tid];
                        int rank = 0;
                        for (int j = 0; j < nc; ++j) rank += c_key[j] > mk || (c_key[j] == mk && c_idx[j] < mi);
                        ti[rank] = mi;
                        tl[rank] = (H16<BF>::f32(c_pat[tid]) - vmax) / t - lse;        // the pick's expression
                    } else {
                        ti[tid] = -1;
                        tl[tid] = __builtin_nanf("");
                    }
                }
            }
        };
        if (!greedy) {
            if (k_on) {
                // ---- pass 3: c[k-1], the running mass at the k-th class -----------------------------------------------------------------
                if (tid < kBins && c1_above < (uint32_t)k && (uint32_t)k <= c1_above + c1) sel_k = Sel{kBins - 1 - tid, c1_above, m1_above};
                __syncthreads();
                low_byte(sel_k.bin);
                const uint32_t ca = sel_k.c_above + c2_above;
                if (tid < kBins && ca < (uint32_t)k && (uint32_t)k <= ca + c2) s_ck = sel_k.m_above + m2_above + (u64)((uint32_t)k - ca) * q2;
                __syncthreads();
            }
            if constexpr (OPT) {
                if (k_on) cur = sel_k.bin;
                if (topn_on) top_rows();
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
                bool have = k_on && bin == sel_k.bin;                   // pass 3 counted this bin
                if constexpr (OPT) have = bin == cur;                   // ... or pass 3n did, after it
                if (!have) {
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
                find_jth(row, n, pen, mk, (uint32_t)sel_key.bin, s_j, wcnt, &s_pick);
                __syncthreads();
            }
        } else if constexpr (OPT) {
            if (topn_on) top_rows();
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
        uint16_t hp = ld1(row, pick, mk);
        if constexpr (PEN) hp = pen.one(hp, pick);
        if (logprobs) logprobs[r] = plain ? __builtin_nanf("") : (H16<BF>::f32(hp) - vmax) / t - lse;
        if constexpr (PEN && !SPEC)
            if (sn) seen[(size_t)r * seen_ld + (pick >> 5)] |= 1u << (pick & 31);       // a bias entry does not enter the set
    }
    if constexpr (OPT)
        if (topn_on && plain && tid < o.top_n) {                        // no distribution, no alternatives
            o.top_ids[(size_t)r * o.top_n + tid] = -1;
            o.top_lp[(size_t)r * o.top_n + tid] = __builtin_nanf("");
        }
    if constexpr (FSM)
        if (wave == 0 && (SPEC || con)) {                               // s_pick: final behind the barriers every path above ends with
            int pick = s_pick;
            pick = pick >= 0 && pick < n ? pick : amax;
            const int ns = fsm_delta(fa, st, pick, n);                  // an unconstrained state stays what it is
            if (lane == 0) (SPEC ? fa.row_states : fa.state)[r] = ns;
        }
}

template <bool BF, bool SPEC, bool PEN>
__global__ __launch_bounds__(kThreads) void k_sample_advance(const uint16_t* __restrict__ x, int64_t ld, int n, int len_q, const float* __restrict__ temperature,
                                                             const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                             const int64_t* __restrict__ seeds, int64_t* __restrict__ draws,
                                                             const float* __restrict__ u_in, int32_t* __restrict__ tokens,
                                                             int32_t* __restrict__ positions, int32_t* __restrict__ placement,
                                                             int32_t* __restrict__ valid_lens, int64_t* __restrict__ next_tokens,
                                                             float* __restrict__ logprobs, float* __restrict__ u_out,
                                                             const float* __restrict__ rep_penalty, const float* __restrict__ presence,
                                                             uint32_t* seen, int64_t seen_ld, const int32_t* __restrict__ drafts) {
    sample_row<BF, SPEC, PEN ? 1 : 0>(x, ld, n, len_q, temperature, top_k, top_p, seeds, draws, u_in, tokens, positions, placement, valid_lens,
                                      next_tokens, logprobs, u_out, rep_penalty, presence, seen, seen_ld, drafts, Opts{}, Fsm{});
}

template <bool BF, bool SPEC>
__global__ __launch_bounds__(kThreads) void k_sample_advance_opts(const uint16_t* __restrict__ x, int64_t ld, int n, int len_q, const float* __restrict__ temperature,
                                                                  const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                                  const int64_t* __restrict__ seeds, int64_t* __restrict__ draws,
                                                                  const float* __restrict__ u_in, int32_t* __restrict__ tokens,
                                                                  int32_t* __restrict__ positions, int32_t* __restrict__ placement,
                                                                  int32_t* __restrict__ valid_lens, int64_t* __restrict__ next_tokens,
                                                                  float* __restrict__ logprobs, float* __restrict__ u_out,
                                                                  const float* __restrict__ rep_penalty, const float* __restrict__ presence,
                                                                  uint32_t* seen, int64_t seen_ld, const int32_t* __restrict__ drafts, const Opts o) {
    sample_row<BF, SPEC, 2>(x, ld, n, len_q, temperature, top_k, top_p, seeds, draws, u_in, tokens, positions, placement, valid_lens, next_tokens,
                            logprobs, u_out, rep_penalty, presence, seen, seen_ld, drafts, o, Fsm{});
}

template <bool BF, bool SPEC>
__global__ __launch_bounds__(kThreads) void k_sample_advance_fsm(const uint16_t* __restrict__ x, int64_t ld, int n, int len_q, const float* __restrict__ temperature,
                                                                 const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                                 const int64_t* __restrict__ seeds, int64_t* __restrict__ draws,
                                                                 const float* __restrict__ u_in, int32_t* __restrict__ tokens,
                                                                 int32_t* __restrict__ positions, int32_t* __restrict__ placement,
                                                                 int32_t* __restrict__ valid_lens, int64_t* __restrict__ next_tokens,
                                                                 float* __restrict__ logprobs, float* __restrict__ u_out,
                                                                 const float* __restrict__ rep_penalty, const float* __restrict__ presence,
                                                                 uint32_t* seen, int64_t seen_ld, const int32_t* __restrict__ drafts, const Opts o,
                                                                 const Fsm fa) {
    sample_row<BF, SPEC, 3>(x, ld, n, len_q, temperature, top_k, top_p, seeds, draws, u_in, tokens, positions, placement, valid_lens, next_tokens,
                            logprobs, u_out, rep_penalty, presence, seen, seen_ld, drafts, o, fa);
}

// zl_spec_sample_accept's second launch: out_tokens / out_logprobs hold the picks of the (b, len_q) rows and their log-probabilities
// (k_sample_advance<.., SPEC> left them); one thread per task finds the longest prefix of its drafts that the picks confirm (a draft
// outside [0, n) equals no pick), pads the rows behind the bonus token with -1 / NaN, advances the task's state by accepted + 1 and
// -- where the generator gave the uniforms -- its draw count by as much: the rows behind the rejection drew nothing that counts.
// seen (zl_spec_sample_accept_ex): the emitted tokens' bits are set in the task's bitmap; the rejected drafts' are not
// TOP (zl_spec_sample_accept_opts with top_n > 0): one 64-thread workgroup per task instead of one thread -- thread 0 does the above,
// then all 64 pad the top-N slots of the rows behind the bonus token, up to 31 x 32 ids and log-probabilities, with -1 / NaN
// FSM (zl_spec_sample_accept_fsm with an automaton): the task's state <- the state behind its last emitted row (the first launch left
// one per row in row_states)
template <bool TOP, bool FSM>
__global__ void k_spec_sample_accept(const int32_t* __restrict__ drafts, int32_t* __restrict__ out_tokens, float* __restrict__ out_logprobs,
                                     int32_t* __restrict__ accepted, int32_t* __restrict__ tokens, int32_t* __restrict__ positions,
                                     int32_t* __restrict__ placement, int32_t* __restrict__ valid_lens, float* __restrict__ logprobs,
                                     int64_t* __restrict__ draws, int b, int len_q, uint32_t* __restrict__ seen, int64_t seen_ld, int top_n,
                                     int32_t* __restrict__ top_ids, float* __restrict__ top_lp, int32_t* __restrict__ fsm_state,
                                     const int32_t* __restrict__ row_states) {
    const int t = TOP ? blockIdx.x : blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;                                                 // TOP: uniform over the workgroup
    int32_t* pk = out_tokens + (int64_t)t * len_q;
    if constexpr (TOP) {
        __shared__ int s_a;
        if (threadIdx.x == 0) {
            const int32_t* dr = drafts + (int64_t)t * (len_q - 1);
            int a = 0;
            while (a < len_q - 1 && dr[a] == pk[a]) ++a;
            s_a = a;
        }
        __syncthreads();                                                // thread 0 rewrites pk behind the bonus token only below
        const int first = (s_a + 1) * top_n, end = len_q * top_n;       // the task's (len_q, top_n) slots behind row s_a
        for (int i = first + (int)threadIdx.x; i < end; i += (int)blockDim.x) {
            top_ids[(int64_t)t * end + i] = -1;
            top_lp[(int64_t)t * end + i] = __builtin_nanf("");
        }
        if (threadIdx.x != 0) return;
    }
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
    if constexpr (FSM) fsm_state[t] = row_states[(int64_t)t * len_q + a];
    if (seen)
        for (int j = 0; j <= a; ++j) seen[(int64_t)t * seen_ld + (pk[j] >> 5)] |= 1u << (pk[j] & 31);     // picks lie in [0, n)
}

// zl_seen_mark: one thread per (task, position); ids outside [0, n) are skipped
__global__ void k_seen_mark(uint32_t* __restrict__ seen, int64_t seen_ld, int64_t b, int n, const int32_t* __restrict__ tokens, int64_t n_tok,
                            int64_t tok_ld) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b * n_tok) return;
    const int64_t t = i / n_tok;
    const int32_t id = tokens[t * tok_ld + (i - t * n_tok)];
    if (id >= 0 && id < n) atomicOr(&seen[t * seen_ld + (id >> 5)], 1u << (id & 31));
}

constexpr zl_sample_opts_t kNoOpts{};                                   // opts == NULL

// every refusal the two operations share (0 = fine), in the order of their codes: the pointers (own_ptrs: the operation's own),
// the shape (own_shape: the operation's own), the dtype, then the bias / top-N group's checks and the automaton's
int sample_check(const void* logits, int type, int64_t n, int64_t ld, const float* temperature, const int32_t* top_k, const float* top_p,
                 const int64_t* seeds, const int64_t* draws, const float* u_in, bool own_ptrs, bool own_shape, const zl_sample_opts_t& so,
                 bool spec) {
    ZL_CHECK_ARG(logits && temperature && top_k && top_p && own_ptrs, ZL_EINVAL);
    ZL_CHECK_ARG((seeds && draws) || u_in, ZL_EINVAL);
    ZL_CHECK_ARG(!so.seen || (so.rep_penalty && so.presence), ZL_EINVAL);
    ZL_CHECK_ARG(own_shape && n >= 1 && ld >= n && n < ((int64_t)1 << 31), ZL_ESHAPE);
    ZL_CHECK_ARG(!so.seen || so.seen_ld >= (n + 31) / 32, ZL_ESHAPE);
    ZL_CHECK_ARG(type == ZL_T_F16 || type == ZL_T_BF16, ZL_EDTYPE);
    const int bias = (so.bias_ids != nullptr) + (so.bias_vals != nullptr) + (so.bias_cnt != nullptr) + (so.bias_bits != nullptr);
    ZL_CHECK_ARG(bias == 0 || bias == 4, ZL_EINVAL);
    ZL_CHECK_ARG(so.top_n <= 0 || (so.top_ids && so.top_logprobs), ZL_EINVAL);
    ZL_CHECK_ARG(bias == 0 || (so.bias_ld >= 1 && so.bias_ld <= 1024 && so.bias_bits_ld >= (n + 31) / 32), ZL_ESHAPE);
    ZL_CHECK_ARG(so.top_n >= 0 && so.top_n <= kMaxTop, ZL_ESHAPE);
    const int fsm = (so.fsm_mask != nullptr) + (so.fsm_default != nullptr) + (so.fsm_exc_off != nullptr) + (so.fsm_exc_tok != nullptr) +
                    (so.fsm_exc_next != nullptr) + (so.fsm_state != nullptr);
    ZL_CHECK_ARG(fsm == 0 || fsm == 6, ZL_EINVAL);
    if (fsm == 0) return 0;
    ZL_CHECK_ARG(!spec || so.fsm_row_states, ZL_EINVAL);
    ZL_CHECK_ARG(so.fsm_states >= 1 && so.fsm_states < ((int64_t)1 << 31) && so.fsm_exceptions >= 0 && so.fsm_exceptions < ((int64_t)1 << 31) &&
                     so.fsm_mask_ld >= (n + 31) / 32,
                 ZL_ESHAPE);
    return 0;
}

// the one selection and launch of k_sample_advance*, one 1024-thread workgroup per logit row; a... = the 22 arguments every
// instantiation takes.  MODE: 3 with an automaton, else 2 where a bias or top-N is asked for, else 1 <=> seen != NULL, else 0 -- so
// a call without options launches the instantiation it always has, and a bias without seen stays MODE 2
template <bool BF, bool SPEC, class... A>
void launch_rows_as(const zl_sample_opts_t& so, unsigned grid, hipStream_t hs, A... a) {
    const Opts o{so.bias_ids, so.bias_vals, so.bias_cnt, so.bias_ld, so.bias_bits, so.bias_bits_ld, (int)so.top_n, so.top_ids, so.top_logprobs};
    const Fsm fa{so.fsm_mask,     so.fsm_mask_ld,     so.fsm_default,         so.fsm_exc_off, so.fsm_exc_tok,
                 so.fsm_exc_next, (int)so.fsm_states, (int)so.fsm_exceptions, so.fsm_state,   SPEC ? so.fsm_row_states : nullptr};
    const dim3 g(grid), b(kThreads);
    if (so.fsm_mask) hipLaunchKernelGGL((k_sample_advance_fsm<BF, SPEC>), g, b, 0, hs, a..., o, fa);
    else if (so.bias_ids || so.top_n > 0) hipLaunchKernelGGL((k_sample_advance_opts<BF, SPEC>), g, b, 0, hs, a..., o);
    else if (so.seen) hipLaunchKernelGGL((k_sample_advance<BF, SPEC, true>), g, b, 0, hs, a...);
    else hipLaunchKernelGGL((k_sample_advance<BF, SPEC, false>), g, b, 0, hs, a...);
}

template <bool SPEC, class... A>
void launch_rows(int type, const zl_sample_opts_t& so, unsigned grid, hipStream_t hs, A... a) {
    if (type == ZL_T_F16) launch_rows_as<false, SPEC>(so, grid, hs, a...);
    else launch_rows_as<true, SPEC>(so, grid, hs, a...);
}

}  // namespace

extern "C" {

int zl_sample_advance_ex(const void* logits, int type, int64_t rows, int64_t n, int64_t ld, const float* temperature, const int32_t* top_k,
                         const float* top_p, const int64_t* seeds, int64_t* draws, const float* u_in, int32_t* tokens, int32_t* positions,
                         int32_t* placement, int32_t* valid_lens, int64_t* next_tokens, float* logprobs, float* u_out,
                         const zl_sample_opts_t* opts, zl_stream_t s) {
    const zl_sample_opts_t& so = opts ? *opts : kNoOpts;
    if (const int e = sample_check(logits, type, n, ld, temperature, top_k, top_p, seeds, draws, u_in, tokens || next_tokens,
                                   rows >= 1 && rows < ((int64_t)1 << 31), so, false))
        return e;
    launch_rows<false>(type, so, (unsigned)rows, (hipStream_t)s, (const uint16_t*)logits, ld, (int)n, 1, temperature, top_k, top_p, seeds, draws,
                       u_in, tokens, positions, placement, valid_lens, next_tokens, logprobs, u_out, so.rep_penalty, so.presence, so.seen,
                       so.seen_ld, (const int32_t*)nullptr);
    return zl_launch_status();
}

int zl_sample_advance(const void* logits, int type, int64_t rows, int64_t n, int64_t ld, const float* temperature, const int32_t* top_k,
                      const float* top_p, const int64_t* seeds, int64_t* draws, const float* u_in, int32_t* tokens, int32_t* positions,
                      int32_t* placement, int32_t* valid_lens, int64_t* next_tokens, float* logprobs, float* u_out, zl_stream_t s) {
    return zl_sample_advance_ex(logits, type, rows, n, ld, temperature, top_k, top_p, seeds, draws, u_in, tokens, positions, placement,
                                valid_lens, next_tokens, logprobs, u_out, nullptr, s);
}

int zl_spec_sample_accept_ex(const void* logits, int type, int64_t b, int64_t len_q, int64_t n, int64_t ld, const int32_t* drafts,
                             const float* temperature, const int32_t* top_k, const float* top_p, const int64_t* seeds, int64_t* draws,
                             const float* u_in, int32_t* tokens, int32_t* positions, int32_t* placement, int32_t* valid_lens,
                             int32_t* accepted, int32_t* out_tokens, float* out_logprobs, float* logprobs, float* u_out,
                             const zl_sample_opts_t* opts, zl_stream_t s) {
    const zl_sample_opts_t& so = opts ? *opts : kNoOpts;
    if (const int e = sample_check(logits, type, n, ld, temperature, top_k, top_p, seeds, draws, u_in,
                                   drafts && accepted && out_tokens && (out_logprobs || !logprobs),   // the task's log-probability is read from its rows'
                                   b >= 1 && len_q >= 2 && len_q <= kMaxDrafts + 1 && b < ((int64_t)1 << 31) && b * len_q < ((int64_t)1 << 31),
                                   so, true))
        return e;
    // the picks: zl_sample_advance's kernel under the task's parameters, into out_tokens
    hipStream_t hs = (hipStream_t)s;
    launch_rows<true>(type, so, (unsigned)(b * len_q), hs, (const uint16_t*)logits, ld, (int)n, (int)len_q, temperature, top_k, top_p, seeds, draws,
                      u_in, out_tokens, nullptr, nullptr, nullptr, nullptr, out_logprobs, u_out, so.rep_penalty, so.presence, so.seen, so.seen_ld,
                      drafts);
    if (const int e = zl_launch_status()) return e;
#define ZL_ACCEPT(TOP, FSM, grid, tn, ti, tl)                                                                                                  \
    hipLaunchKernelGGL((k_spec_sample_accept<TOP, FSM>), grid, dim3(64), 0, hs, drafts, out_tokens, out_logprobs, accepted, tokens, positions,   \
                       placement, valid_lens, logprobs, u_in ? nullptr : draws, (int)b, (int)len_q, so.seen, so.seen_ld, tn, ti, tl,            \
                       so.fsm_state, (const int32_t*)so.fsm_row_states)
    const dim3 per_task((unsigned)b), per_lane((unsigned)((b + 63) / 64));
    if (so.top_n > 0) {
        if (so.fsm_mask) ZL_ACCEPT(true, true, per_task, (int)so.top_n, so.top_ids, so.top_logprobs);
        else ZL_ACCEPT(true, false, per_task, (int)so.top_n, so.top_ids, so.top_logprobs);
    } else {
        if (so.fsm_mask) ZL_ACCEPT(false, true, per_lane, 0, (int32_t*)nullptr, (float*)nullptr);
        else ZL_ACCEPT(false, false, per_lane, 0, (int32_t*)nullptr, (float*)nullptr);
    }
#undef ZL_ACCEPT
    return zl_launch_status();
}

int zl_spec_sample_accept(const void* logits, int type, int64_t b, int64_t len_q, int64_t n, int64_t ld, const int32_t* drafts,
                          const float* temperature, const int32_t* top_k, const float* top_p, const int64_t* seeds, int64_t* draws,
                          const float* u_in, int32_t* tokens, int32_t* positions, int32_t* placement, int32_t* valid_lens,
                          int32_t* accepted, int32_t* out_tokens, float* out_logprobs, float* logprobs, float* u_out, zl_stream_t s) {
    return zl_spec_sample_accept_ex(logits, type, b, len_q, n, ld, drafts, temperature, top_k, top_p, seeds, draws, u_in, tokens, positions,
                                    placement, valid_lens, accepted, out_tokens, out_logprobs, logprobs, u_out, nullptr, s);
}


int zl_seen_mark(uint32_t* seen, int64_t seen_ld, int64_t b, int64_t n, const int32_t* tokens, int64_t n_tok, int64_t tok_ld, zl_stream_t s) {
    ZL_CHECK_ARG(seen && tokens, ZL_EINVAL);
    ZL_CHECK_ARG(b >= 1 && n >= 1 && n < ((int64_t)1 << 31) && n_tok >= 1 && tok_ld >= n_tok && seen_ld >= (n + 31) / 32 &&
                     b * n_tok < ((int64_t)1 << 39),
                 ZL_ESHAPE);
    hipLaunchKernelGGL(k_seen_mark, dim3((unsigned)((b * n_tok + 255) / 256)), dim3(256), 0, (hipStream_t)s, seen, seen_ld, b, (int)n, tokens, n_tok,
                       tok_ld);
    return zl_launch_status();
}

}  // extern "C"
