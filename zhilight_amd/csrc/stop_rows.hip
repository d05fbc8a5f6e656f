// stop_rows.hip -- the stop conditions of a decode step, applied on the device behind the step's advance / accept launch.
//   zl_stop_advance   per task: test the ids the step emitted against the task's stop ids, its multi-token stop sequences and its length
//                     limit, cut the step's results behind the first hit, take the batch state back to the cut, and freeze a task that
//                     has finished: from then on it re-feeds its last token at the same position into the same slot.  The reference
//                     tests these on the host between steps (src/generator/batch_generator.cpp); here a captured step carries them.
// Exact integer work on a few dozen ids per task, one launch of ONE workgroup: a wave takes a task (lane j tests emitted id j), the
// waves stride over the tasks, and the count of live tasks is a plain sum through LDS behind one barrier -- no atomics, no workspace.
#include <hip/hip_runtime.h>

#include "zl_common.h"

namespace {

constexpr int kMaxWaves = 16;
constexpr int kTail = 15;       // ids a task remembers
constexpr int kMaxNew = 32;     // ids a step emits per task
constexpr int kMaxIds = 16;
constexpr int kMaxSeqs = 8;
constexpr int kMaxSeqLen = kTail + 1;

struct StopArgs {
    const int32_t* stop_ids;    // (b, n_ids)
    const int32_t* stop_seqs;   // (b, n_seqs, seq_ld)
    const int32_t* seq_lens;    // (b, n_seqs)
    const int32_t* max_new;     // (b)
    int32_t *gen_lens, *tail, *last_token, *finished;
    int32_t* new_tokens;        // (b, n_new); may be `tokens` itself at n_new == 1
    int32_t* accepted;
    int64_t* next_tokens;
    int32_t *tokens, *positions, *placement, *valid_lens;
    int32_t *emit_lens, *live;
    int n_ids, n_seqs, seq_ld, n_new, b;
};

__global__ __launch_bounds__(kMaxWaves* ZL_WAVE) void k_stop_advance(const StopArgs a) {
    __shared__ int32_t red[kMaxWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    int alive = 0;                                           // wave-uniform: the live tasks among this wave's
    for (int t = wave; t < a.b; t += waves) {                // everything below is uniform over the wave but the lane's own id
        const int32_t fin = __builtin_amdgcn_readfirstlane(a.finished[t]);
        int32_t* row = a.new_tokens + (int64_t)t * a.n_new;
        // the window of the task in ONE register over the wave: lanes 0 .. 14 the tail, lanes 15 .. 46 the step's row (read before any
        // write of this task), -1 behind it
        int32_t w = -1;
        if (lane < kTail) w = a.tail[(int64_t)t * kTail + lane];
        else if (lane - kTail < a.n_new) w = row[lane - kTail];
        const int32_t e = __shfl(w, (lane + kTail) & 63, 64);                           // lane j < 32: emitted id j
        const int m = __ffsll((unsigned long long)__ballot(lane >= kMaxNew || e < 0)) - 1;      // ids before the first negative one
        if (m == 0) {                                        // nothing emitted: nothing changes
            if (lane == 0) a.emit_lens[t] = 0;
            alive += fin == 0;
            continue;
        }
        if (fin != 0) {                                      // frozen: undo the step, re-feed the last token
            if (lane < a.n_new) row[lane] = -1;
            if (lane == 0) {
                a.emit_lens[t] = 0;
                if (a.accepted) a.accepted[t] = -1;
                if (a.next_tokens) a.next_tokens[t] = -1;
                if (a.positions) a.positions[t] -= m;
                if (a.placement) a.placement[t] -= m;
                if (a.valid_lens) a.valid_lens[t] -= m;
                if (a.tokens) a.tokens[t] = a.last_token[t];         // behind the row's store: the row may be this very word
            }
            continue;
        }
        // ---- lane j: is emitted id j a hit, and for which reason ---------------------------------------------------------------
        int reason = 0;
        for (int i = 0; i < a.n_ids; ++i) {
            const int32_t id = a.stop_ids[(int64_t)t * a.n_ids + i];
            if (id >= 0 && id == e) reason = 1;
        }
        bool seq_hit = false;
        for (int q = 0; q < a.n_seqs; ++q) {
            const int len = __builtin_amdgcn_readfirstlane(a.seq_lens[(int64_t)t * a.n_seqs + q]);
            if (len < 1 || len > a.seq_ld) continue;        // unused (a length beyond the row is never read)
            const int32_t* sq = a.stop_seqs + ((int64_t)t * a.n_seqs + q) * a.seq_ld;
            bool ok = true;
            for (int i = 0; i < len; ++i) {                  // the last len ids of (tail ++ e[0 .. j]) end at window index 15 + j
                const int32_t v = __shfl(w, (lane + kTail - len + 1 + i) & 63, 64);
                ok = ok && v >= 0 && v == sq[i];
            }
            seq_hit = seq_hit || ok;
        }
        if (reason == 0 && seq_hit) reason = 2;
        const int32_t lim = a.max_new ? a.max_new[t] : 0;
        if (reason == 0 && lim > 0 && (int64_t)a.gen_lens[t] + lane + 1 >= lim) reason = 3;
        if (lane >= m) reason = 0;
        const unsigned long long hits = __ballot(reason != 0);
        const int first = __ffsll(hits) - 1;
        const int c = hits ? first + 1 : m;                  // 1 <= c <= m
        const int why = __shfl(reason, hits ? first : 0, 64);
        const int32_t nt = __shfl(w, (lane + c) & 63, 64);  // the new tail: the last 15 of (tail ++ e[0 .. c - 1])
        const int32_t last = __shfl(w, kTail + c - 1, 64);
        if (lane >= c && lane < a.n_new) row[lane] = -1;
        if (lane < kTail) a.tail[(int64_t)t * kTail + lane] = nt;
        if (lane == 0) {
            a.emit_lens[t] = c;
            a.gen_lens[t] += c;
            if (a.accepted) a.accepted[t] = c - 1;
            if (a.positions) a.positions[t] -= m - c;
            if (a.placement) a.placement[t] -= m - c;
            if (a.valid_lens) a.valid_lens[t] -= m - c;
            if (a.tokens) a.tokens[t] = last;
            if (a.next_tokens) a.next_tokens[t] = last;
            a.last_token[t] = last;
            a.finished[t] = why;
        }
        alive += why == 0;
    }
    if (lane == 0) red[wave] = alive;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int i = 0; i < waves; ++i) total += red[i];
        a.live[0] = total;
    }
}
}  // namespace

extern "C" {

int zl_stop_advance(const int32_t* stop_ids, int64_t n_ids, const int32_t* stop_seqs, const int32_t* seq_lens, int64_t n_seqs, int64_t seq_ld,
                    const int32_t* max_new, int32_t* gen_lens, int32_t* tail, int32_t* last_token, int32_t* finished, int32_t* new_tokens,
                    int64_t n_new, int64_t b, int32_t* accepted, int64_t* next_tokens, int32_t* tokens, int32_t* positions,
                    int32_t* placement, int32_t* valid_lens, int32_t* emit_lens, int32_t* live, zl_stream_t s) {
    ZL_CHECK_ARG(gen_lens && tail && last_token && finished && new_tokens && emit_lens && live, ZL_EINVAL);
    ZL_CHECK_ARG(n_ids >= 0 && n_seqs >= 0 && seq_ld >= 0 && (stop_ids != nullptr) == (n_ids > 0), ZL_EINVAL);
    ZL_CHECK_ARG((n_seqs > 0) == (stop_seqs != nullptr) && (n_seqs > 0) == (seq_lens != nullptr) && (n_seqs > 0) == (seq_ld > 0), ZL_EINVAL);
    ZL_CHECK_ARG(b >= 1 && n_new >= 1 && ((const void*)new_tokens != (const void*)tokens || n_new == 1), ZL_EINVAL);
    ZL_CHECK_ARG(n_ids <= kMaxIds && n_seqs <= kMaxSeqs && seq_ld <= kMaxSeqLen && n_new <= kMaxNew && b < ((int64_t)1 << 31), ZL_ESHAPE);
    StopArgs a;
    a.stop_ids = stop_ids, a.stop_seqs = stop_seqs, a.seq_lens = seq_lens, a.max_new = max_new;
    a.gen_lens = gen_lens, a.tail = tail, a.last_token = last_token, a.finished = finished;
    a.new_tokens = new_tokens, a.accepted = accepted, a.next_tokens = next_tokens;
    a.tokens = tokens, a.positions = positions, a.placement = placement, a.valid_lens = valid_lens;
    a.emit_lens = emit_lens, a.live = live;
    a.n_ids = (int)n_ids, a.n_seqs = (int)n_seqs, a.seq_ld = (int)seq_ld, a.n_new = (int)n_new, a.b = (int)b;
    const int waves = b < kMaxWaves ? (int)b : kMaxWaves;
    hipLaunchKernelGGL(k_stop_advance, dim3(1), dim3(waves * ZL_WAVE), 0, (hipStream_t)s, a);
    return zl_launch_status();
}

}  // extern "C"
