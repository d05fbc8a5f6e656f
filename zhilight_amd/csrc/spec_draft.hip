// spec_draft.hip -- the drafter of the speculative step: prompt lookup over the tasks' token histories, kept on the device.
//   zl_lookup_draft   per task: append the tokens the last step emitted to the task's history row, then find the latest n-gram of the
//                     history earlier in it and propose what followed it as the next step's K drafts (LLaMA.step_lookup feeds them to
//                     LLaMA.verify).  The reference has no counterpart: it leaves drafting to the caller of SessionGenerator.feed /
//                     rollback_speculative (zhilight/session_generator.py:25-66).
// Exact integer work, one launch, one workgroup of 1024 threads per task: a row is at most a KV buffer's length of int32 ids (tens of
// thousands, <= ~128 KB), so one workgroup walks it in a few dozen coalesced rounds and the append can precede the search behind a
// plain __syncthreads() -- no hand-off between workgroups, no workspace.
#include <hip/hip_runtime.h>

#include "zl_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / ZL_WAVE;
constexpr int kMaxNgram = 16;
constexpr int kMaxNew = 32;
constexpr int kUnroll = 4;

// The rule as ONE maximisation: over every candidate end e = s + n in [1, L - 1] with n = the length of the common suffix of h[:e] and
// h[:L] capped at min(max_ngram, e) (n >= min_ngram), take the largest (n, c = min(k, L - e), c == k ? s : -s).  The longest n decides;
// among its matches the latest with a full continuation, else the earliest (= the longest continuation).  0 = no match.
__device__ __forceinline__ uint64_t pack_key(int n, int c, int k, int64_t s) {
    const uint32_t sp = c == k ? (uint32_t)s : 0x7fffffffu - (uint32_t)s;
    return ((uint64_t)n << 40) | ((uint64_t)c << 32) | sp;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void k_lookup_draft(int32_t* __restrict__ history, int64_t cap, int32_t* __restrict__ hist_lens,
                                                           const int32_t* __restrict__ new_tokens, int n_new, int k, int max_ngram,
                                                           int min_ngram, int32_t* __restrict__ drafts, int32_t* __restrict__ match) {
    __shared__ int32_t suf[kMaxNgram];          // suf[j] = h[L - 1 - j]
    __shared__ uint64_t red[kWaves];
    const int task = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    int32_t* row = history + (int64_t)task * cap;

    // ---- append: the ids of new_tokens[task] before the first negative one --------------------------------------------------
    const int64_t len0 = hist_lens[task];       // every thread reads it BEFORE the barrier, thread 0 rewrites it behind it
    int a = 0;
    if (new_tokens) {                           // every wave counts for itself: lanes >= n_new (<= 32) hold -1, so the ballot is never 0
        const int32_t t = lane < n_new ? new_tokens[(int64_t)task * n_new + lane] : -1;
        a = __ffsll((unsigned long long)__ballot(t < 0)) - 1;
        const int64_t at = len0 + lane;
        if (tid < a && at >= 0 && at < cap) row[at] = t;     // wave 0 only; a token beyond the row is dropped, the length still counts it
    }
    int64_t len = len0 + a;
    if (len > 0x7fffffff) len = 0x7fffffff;
    __syncthreads();                            // the appended ids are visible to the whole workgroup
    if (tid == 0) hist_lens[task] = (int32_t)len;

    // ---- draft -----------------------------------------------------------------------------------------------------------------
    uint64_t best = 0;
    if (len >= 2 && len <= cap) {               // wave-uniform (workgroup-uniform): the barriers inside are reached by all or none
        const int L = (int)len;
        const int ns = max_ngram < L - 1 ? max_ngram : L - 1;
        if (tid < ns) suf[tid] = row[L - 1 - tid];
        __syncthreads();
        const int32_t last = suf[0];
        // consecutive threads take consecutive ends e: the first compare (h[e - 1] against the last id) is a coalesced read and almost
        // always the only one; kUnroll rounds of it are in flight at once
        for (int64_t e0 = 1 + tid; e0 < L; e0 += (int64_t)kUnroll * kThreads) {
            int32_t v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int64_t e = e0 + (int64_t)u * kThreads;
                v[u] = e < L ? row[e - 1] : ~last;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                if (v[u] != last) continue;
                const int64_t e = e0 + (int64_t)u * kThreads;
                const int lim = e < ns ? (int)e : ns;
                int n = 1;
                while (n < lim && row[e - 1 - n] == suf[n]) ++n;
                if (n < min_ngram) continue;
                const int64_t rest = L - e;
                const uint64_t key = pack_key(n, rest < k ? (int)rest : k, k, e - n);
                best = key > best ? key : best;
            }
        }
        best = wave_max_u64(best);
        if (lane == 0) red[tid >> 6] = best;
        __syncthreads();
        best = red[lane & (kWaves - 1)];
        best = wave_max_u64(best);
    }

    // ---- the K drafts: what followed the match, -1 behind the history's end -------------------------------------------------------
    if (tid < ZL_WAVE) {
        const int n = (int)(best >> 40), c = (int)((best >> 32) & 0xff);
        const uint32_t sp = (uint32_t)best;
        const int64_t s = best == 0 ? -1 : (c == k ? (int64_t)sp : (int64_t)(0x7fffffffu - sp));
        if (lane < k) drafts[(int64_t)task * k + lane] = lane < c ? row[s + n + lane] : -1;
        if (match && lane < 2) match[(int64_t)task * 2 + lane] = lane == 0 ? n : (int32_t)s;
    }
}
}  // namespace

extern "C" {

int zl_lookup_draft(int32_t* history, int64_t cap, int32_t* hist_lens, const int32_t* new_tokens, int64_t n_new, int64_t b, int64_t k,
                    int max_ngram, int min_ngram, int32_t* drafts, int32_t* match, zl_stream_t s) {
    ZL_CHECK_ARG(history && hist_lens && drafts, ZL_EINVAL);
    ZL_CHECK_ARG(b >= 1 && k >= 1 && cap >= 2 && n_new >= 0 && (new_tokens == nullptr || n_new > 0), ZL_EINVAL);
    ZL_CHECK_ARG(1 <= min_ngram && min_ngram <= max_ngram && max_ngram <= kMaxNgram, ZL_EINVAL);
    ZL_CHECK_ARG(k <= 31 && n_new <= kMaxNew && cap < ((int64_t)1 << 31) && b < ((int64_t)1 << 31), ZL_ESHAPE);
    hipLaunchKernelGGL(k_lookup_draft, dim3((unsigned)b), dim3(kThreads), 0, (hipStream_t)s, history, cap, hist_lens, new_tokens,
                       new_tokens ? (int)n_new : 0, (int)k, max_ngram, min_ngram, drafts, match);
    return zl_launch_status();
}

}  // extern "C"
