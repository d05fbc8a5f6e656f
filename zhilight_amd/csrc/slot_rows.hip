// slot_rows.hip -- slot admission: put new requests into slots of a running batch.
//   zl_slots_admit   per admitted slot: re-initialise its row of every per-task state tensor -- the sampler's parameters, generator and
//                    bitmaps, the stop state's parameters and memory, the lookup drafter's history -- from ONE packed int32 blob, in
//                    place, behind the prompt encode that left the slot's first token pending.  The reference builds a new task's
//                    state on the host when the task enters the active batch (SearcherImplV1, src/generator/batch_generator.cpp) and
//                    seeds its first token in fill_search_tokens; here the states live on the device under a captured step, so their
//                    rows are rewritten where they are.  A record without a request parks the slot (token 0, position 0, one key).
//   zl_slots_admit_fsm   the same with the sampler's token-automaton state: header flag 16 says that header word 12 points at an (n, 2)
//                    array of (start state, pending-token override) per record; an admitted slot's fsm_state row takes the start
//                    state, and an override >= 0 replaces the pending token wherever the rule above uses it.  A parked slot: -1.
// Exact integer / bit work: one 256-thread workgroup per record.  The bitmap rows (16 KB each at 128 256 ids) are built in LDS with LDS
// atomics and leave with 16-byte stores; everything else is a handful of dword stores.  No global atomics, no workspace; rows of slots
// that are not in the blob are neither read-modified nor written (workgroup 0 READS their `finished` entries to recount `live`).
#include <hip/hip_runtime.h>

#include "zl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsWords = 4096;          // 16 KB: one bitmap row of 131 072 ids, or a piece of a longer one
constexpr int kHdr = 16;                 // header words of the blob (the host's)
constexpr int kRec = 16;                 // fixed words of a record, the stop rows behind them
constexpr int kTail = 15;                // zl_stop_advance's tail
constexpr int kMaxB = kLdsWords * 32;

struct SlotArgs {
    const int32_t* blob;
    int n, rec, b, vocab;
    int32_t *tokens, *positions, *placement, *valid_lens;
    float* temperature;
    int32_t* top_k;
    float* top_p;
    int64_t *seeds, *draws;
    float *logprobs, *u, *rep, *pres;
    uint32_t* seen;
    int64_t seen_ld;
    int32_t* bias_ids;
    float* bias_vals;
    int32_t* bias_cnt;
    uint32_t* bias_bits;
    int bias_ld;
    int64_t bits_ld;
    int32_t* top_ids;
    float* top_logprobs;
    int top_n;
    int32_t *stop_ids, *stop_seqs, *seq_lens;
    int n_ids, n_seqs, seq_ld;
    int32_t *max_new, *gen_lens, *tail, *last_token, *finished, *emit_lens, *live;
    int32_t* history;
    int64_t cap;
    int32_t *hist_lens, *draft_new;
    int32_t* fsm_state;
};

// row[0 .. ld) <- the bitmap of the ids[0 .. cnt) and of `extra` that lie in [0, vocab), 0 everywhere else: built piece by piece in lds
// (kLdsWords words, 16-byte aligned).  Called by the whole workgroup; ends behind a barrier.
__device__ void bitmap_row(uint32_t* lds, uint32_t* row, int64_t ld, int vocab, const int32_t* ids, int cnt, int32_t extra) {
    const int tid = threadIdx.x;
    for (int64_t base = 0; base < ld; base += kLdsWords) {
        const int w = ld - base < kLdsWords ? (int)(ld - base) : kLdsWords;
        for (int i = tid; i < w; i += kThreads) lds[i] = 0u;
        __syncthreads();
        for (int i = tid; i <= cnt; i += kThreads) {                  // entry cnt = the extra id
            const int32_t id = i < cnt ? ids[i] : extra;
            if (id < 0 || id >= vocab) continue;
            const int64_t wi = (int64_t)(id >> 5) - base;
            if (wi >= 0 && wi < w) atomicOr(&lds[wi], 1u << (id & 31));
        }
        __syncthreads();
        uint32_t* dst = row + base;                                   // base is a multiple of 4: dst is aligned as the row is
        const int nv = ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) ? w >> 2 : 0;
        for (int i = tid; i < nv; i += kThreads) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(lds)[i];
        for (int i = nv * 4 + tid; i < w; i += kThreads) dst[i] = lds[i];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void k_slots_admit(const SlotArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
    __shared__ int32_t red[kThreads / ZL_WAVE];
    const int tid = threadIdx.x;
    const int32_t* r = a.blob + kHdr + (int64_t)blockIdx.x * a.rec;

    // ---- workgroup 0: who is in the blob, as a bitmap over the slots -> live and the drafter's new-token column ------------------
    if (blockIdx.x == 0 && (a.live || a.draft_new)) {
        const int words = (a.b + 31) >> 5;
        for (int i = tid; i < words; i += kThreads) lds[i] = 0u;
        __syncthreads();
        for (int e = tid; e < a.n; e += kThreads) {                   // bit set = the slot is admitted (a parked one is "the rest")
            const int32_t* q = a.blob + kHdr + (int64_t)e * a.rec;
            if (q[0] >= 0 && q[0] < a.b && q[1] != 0) atomicOr(&lds[q[0] >> 5], 1u << (q[0] & 31));
        }
        __syncthreads();
        int alive = 0;
        for (int t = tid; t < a.b; t += kThreads) {
            const bool in = (lds[t >> 5] >> (t & 31)) & 1u;
            if (a.live) alive += in ? 1 : (a.finished[t] == 0);       // finished[t] of a slot that is not admitted: nobody writes it
            if (a.draft_new && !in) a.draft_new[t] = -1;
        }
        if (a.live) {
            for (int off = 32; off > 0; off >>= 1) alive += __shfl_xor(alive, off, 64);
            if ((tid & 63) == 0) red[tid >> 6] = alive;
            __syncthreads();
            if (tid == 0) {
                int total = 0;
                for (int i = 0; i < kThreads / ZL_WAVE; ++i) total += red[i];
                a.live[0] = total;
            }
        }
        __syncthreads();                                              // lds is free again
    }

    const int s = r[0];
    if (s < 0 || s >= a.b) return;                                    // uniform over the workgroup
    if (r[1] == 0) {                                                  // ---- park ----------------------------------------------------
        if (tid == 0) {
            a.tokens[s] = 0;
            a.positions[s] = 0;
            a.placement[s] = 0;
            a.valid_lens[s] = 1;
            if (a.tail) {
                a.last_token[s] = 0;
                a.emit_lens[s] = 0;
            }
            if (a.fsm_state) a.fsm_state[s] = -1;
        }
        if (a.tail && tid < kTail) a.tail[(int64_t)s * kTail + tid] = -1;
        return;
    }
    // the record's ranges of the variable part: inside the blob (header word 10 = its words), else read as empty
    const int64_t total = a.blob[10];
    auto inside = [&](int32_t off, int64_t cnt) { return off >= kHdr && cnt >= 0 && off + cnt <= total; };
    // the grammar side array (flag 16, header word 12): this record's start state and pending-token override, -1 / -1 without one
    int32_t start = -1, ovr = -1;
    if (a.fsm_state && (a.blob[3] & 16) && inside(a.blob[12], 2 * (int64_t)a.n)) {
        start = a.blob[a.blob[12] + 2 * (int64_t)blockIdx.x];
        ovr = a.blob[a.blob[12] + 2 * (int64_t)blockIdx.x + 1];
    }
    const bool over = ovr >= 0 && ovr < a.vocab;
    const int32_t pending = over ? ovr : a.tokens[s];                 // tokens[s] is rewritten with the same value below
    if (tid == 0) {
        if (over) a.tokens[s] = pending;
        if (a.fsm_state) a.fsm_state[s] = start;
    }
    const int pen_cnt = inside(r[10], r[11]) ? r[11] : 0;
    const int bias_n = inside(r[12], 2 * (int64_t)r[13]) ? r[13] : 0;
    const int hist_n = inside(r[14], r[15]) ? r[15] : 0;

    // ---- sampler ----------------------------------------------------------------------------------------------------------------
    if (a.temperature && tid == 0) {
        a.temperature[s] = __builtin_bit_cast(float, r[2]);
        a.top_k[s] = r[3];
        a.top_p[s] = __builtin_bit_cast(float, r[4]);
        a.seeds[s] = (int64_t)(((uint64_t)(uint32_t)r[6] << 32) | (uint32_t)r[5]);
        a.draws[s] = 0;
        a.logprobs[s] = 0.f;
        a.u[s] = 0.f;
        if (a.seen) {
            a.rep[s] = __builtin_bit_cast(float, r[7]);
            a.pres[s] = __builtin_bit_cast(float, r[8]);
        }
    }
    if (a.top_ids) {
        for (int i = tid; i < a.top_n; i += kThreads) {
            a.top_ids[(int64_t)s * a.top_n + i] = -1;
            a.top_logprobs[(int64_t)s * a.top_n + i] = __builtin_bit_cast(float, 0x7fc00000u);
        }
    }
    if (a.seen) bitmap_row(lds, a.seen + (int64_t)s * a.seen_ld, a.seen_ld, a.vocab, a.blob + r[10], pen_cnt, pending);
    if (a.bias_ids) {
        const int cnt = bias_n < a.bias_ld ? bias_n : a.bias_ld;
        const int32_t* ids = a.blob + r[12];
        for (int i = tid; i < a.bias_ld; i += kThreads) {
            a.bias_ids[(int64_t)s * a.bias_ld + i] = i < cnt ? ids[i] : -1;
            a.bias_vals[(int64_t)s * a.bias_ld + i] = i < cnt ? __builtin_bit_cast(float, ids[bias_n + i]) : 0.f;
        }
        if (tid == 0) a.bias_cnt[s] = cnt;
        bitmap_row(lds, a.bias_bits + (int64_t)s * a.bits_ld, a.bits_ld, a.vocab, ids, cnt, -1);
    }

    // ---- stop -------------------------------------------------------------------------------------------------------------------
    if (a.tail) {
        const int32_t* p = r + kRec;
        for (int i = tid; i < a.n_ids; i += kThreads) a.stop_ids[(int64_t)s * a.n_ids + i] = p[i];
        p += a.n_ids;
        for (int i = tid; i < a.n_seqs; i += kThreads) a.seq_lens[(int64_t)s * a.n_seqs + i] = p[i];
        p += a.n_seqs;
        const int sw = a.n_seqs * a.seq_ld;
        for (int i = tid; i < sw; i += kThreads) a.stop_seqs[(int64_t)s * sw + i] = p[i];
        if (tid < kTail) a.tail[(int64_t)s * kTail + tid] = tid == kTail - 1 ? pending : -1;
        if (tid == 0) {
            a.max_new[s] = r[9];
            a.gen_lens[s] = 0;
            a.last_token[s] = pending;
            a.finished[s] = 0;
            a.emit_lens[s] = 0;
        }
    }

    // ---- lookup -----------------------------------------------------------------------------------------------------------------
    if (a.history) {
        const int64_t len = hist_n < a.cap ? hist_n : a.cap;
        const int32_t* h = a.blob + r[14];
        for (int64_t i = tid; i < len; i += kThreads) a.history[(int64_t)s * a.cap + i] = h[i];
        if (tid == 0) a.hist_lens[s] = (int32_t)len;
    }
    if (a.draft_new && tid == 0) a.draft_new[s] = pending;
}
// the checks and the launch of both entry points; fsm_state == NULL: zl_slots_admit
int slots_admit_launch(const int32_t* blob, int64_t n, int64_t rec_words, int64_t b, int64_t vocab, int32_t* tokens, int32_t* positions,
                   int32_t* placement, int32_t* valid_lens, float* temperature, int32_t* top_k, float* top_p, int64_t* seeds, int64_t* draws,
                   float* logprobs, float* u, float* rep_penalty, float* presence, int32_t* seen, int64_t seen_ld, int32_t* bias_ids,
                   float* bias_vals, int32_t* bias_cnt, int32_t* bias_bits, int64_t bias_ld, int64_t bits_ld, int32_t* top_ids,
                   float* top_logprobs, int64_t top_n, int32_t* stop_ids, int32_t* stop_seqs, int32_t* seq_lens, int64_t n_ids, int64_t n_seqs,
                   int64_t seq_ld, int32_t* max_new, int32_t* gen_lens, int32_t* tail, int32_t* last_token, int32_t* finished,
                   int32_t* emit_lens, int32_t* live, int32_t* history, int64_t cap, int32_t* hist_lens, int32_t* draft_new,
                   int32_t* fsm_state, zl_stream_t s) {
    ZL_CHECK_ARG(blob && tokens && positions && placement && valid_lens && n >= 1 && b >= 1 && vocab >= 1, ZL_EINVAL);
    const bool sampler = temperature != nullptr;
    ZL_CHECK_ARG(sampler == (top_k != nullptr) && sampler == (top_p != nullptr) && sampler == (seeds != nullptr) &&
                     sampler == (draws != nullptr) && sampler == (logprobs != nullptr) && sampler == (u != nullptr), ZL_EINVAL);
    const bool pen = seen != nullptr;
    ZL_CHECK_ARG(pen == (rep_penalty != nullptr) && pen == (presence != nullptr) && (!pen || sampler) && pen == (seen_ld > 0), ZL_EINVAL);
    const bool bias = bias_ids != nullptr;
    ZL_CHECK_ARG(bias == (bias_vals != nullptr) && bias == (bias_cnt != nullptr) && bias == (bias_bits != nullptr) && bias == (bias_ld > 0) &&
                     bias == (bits_ld > 0), ZL_EINVAL);
    ZL_CHECK_ARG((top_ids != nullptr) == (top_logprobs != nullptr) && (top_ids != nullptr) == (top_n > 0), ZL_EINVAL);
    const bool stop = tail != nullptr;
    ZL_CHECK_ARG(stop == (stop_ids != nullptr) && stop == (stop_seqs != nullptr) && stop == (seq_lens != nullptr) && stop == (max_new != nullptr) &&
                     stop == (gen_lens != nullptr) && stop == (last_token != nullptr) && stop == (finished != nullptr) &&
                     stop == (emit_lens != nullptr) && stop == (live != nullptr), ZL_EINVAL);
    ZL_CHECK_ARG(n_ids >= 0 && n_seqs >= 0 && seq_ld >= 0 && (!stop || (n_ids >= 1 && n_seqs >= 1 && seq_ld >= 1)), ZL_EINVAL);
    ZL_CHECK_ARG(n_ids <= 16 && n_seqs <= 8 && seq_ld <= 16, ZL_ESHAPE);
    ZL_CHECK_ARG(stop ? rec_words == kRec + n_ids + n_seqs + n_seqs * seq_ld : rec_words >= kRec, ZL_EINVAL);
    ZL_CHECK_ARG((history != nullptr) == (hist_lens != nullptr) && (history != nullptr) == (cap > 0), ZL_EINVAL);
    ZL_CHECK_ARG(b <= kMaxB && n <= b && vocab < ((int64_t)1 << 31) && cap < ((int64_t)1 << 31) && rec_words < (1 << 20), ZL_ESHAPE);
    ZL_CHECK_ARG(bias_ld <= 1024 && top_n <= 32, ZL_ESHAPE);
    ZL_CHECK_ARG((!pen || seen_ld >= (vocab + 31) / 32) && (!bias || bits_ld >= (vocab + 31) / 32), ZL_ESHAPE);
    SlotArgs a;
    a.blob = blob, a.n = (int)n, a.rec = (int)rec_words, a.b = (int)b, a.vocab = (int)vocab;
    a.tokens = tokens, a.positions = positions, a.placement = placement, a.valid_lens = valid_lens;
    a.temperature = temperature, a.top_k = top_k, a.top_p = top_p, a.seeds = seeds, a.draws = draws, a.logprobs = logprobs, a.u = u;
    a.rep = rep_penalty, a.pres = presence, a.seen = reinterpret_cast<uint32_t*>(seen), a.seen_ld = seen_ld;
    a.bias_ids = bias_ids, a.bias_vals = bias_vals, a.bias_cnt = bias_cnt, a.bias_bits = reinterpret_cast<uint32_t*>(bias_bits);
    a.bias_ld = (int)bias_ld, a.bits_ld = bits_ld;
    a.top_ids = top_ids, a.top_logprobs = top_logprobs, a.top_n = (int)top_n;
    a.stop_ids = stop_ids, a.stop_seqs = stop_seqs, a.seq_lens = seq_lens;
    a.n_ids = (int)n_ids, a.n_seqs = (int)n_seqs, a.seq_ld = (int)seq_ld;
    a.max_new = max_new, a.gen_lens = gen_lens, a.tail = tail, a.last_token = last_token, a.finished = finished;
    a.emit_lens = emit_lens, a.live = live;
    a.history = history, a.cap = cap, a.hist_lens = hist_lens, a.draft_new = draft_new;
    a.fsm_state = fsm_state;
    hipLaunchKernelGGL(k_slots_admit, dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)s, a);
    return zl_launch_status();
}

}  // namespace

extern "C" {

#define ZL_SLOT_ARGS                                                                                                                       \
    blob, n, rec_words, b, vocab, tokens, positions, placement, valid_lens, temperature, top_k, top_p, seeds, draws, logprobs, u, rep_penalty, \
        presence, seen, seen_ld, bias_ids, bias_vals, bias_cnt, bias_bits, bias_ld, bits_ld, top_ids, top_logprobs, top_n, stop_ids, stop_seqs,   \
        seq_lens, n_ids, n_seqs, seq_ld, max_new, gen_lens, tail, last_token, finished, emit_lens, live, history, cap, hist_lens, draft_new

int zl_slots_admit(const int32_t* blob, int64_t n, int64_t rec_words, int64_t b, int64_t vocab, int32_t* tokens, int32_t* positions,
                   int32_t* placement, int32_t* valid_lens, float* temperature, int32_t* top_k, float* top_p, int64_t* seeds, int64_t* draws,
                   float* logprobs, float* u, float* rep_penalty, float* presence, int32_t* seen, int64_t seen_ld, int32_t* bias_ids,
                   float* bias_vals, int32_t* bias_cnt, int32_t* bias_bits, int64_t bias_ld, int64_t bits_ld, int32_t* top_ids,
                   float* top_logprobs, int64_t top_n, int32_t* stop_ids, int32_t* stop_seqs, int32_t* seq_lens, int64_t n_ids, int64_t n_seqs,
                   int64_t seq_ld, int32_t* max_new, int32_t* gen_lens, int32_t* tail, int32_t* last_token, int32_t* finished,
                   int32_t* emit_lens, int32_t* live, int32_t* history, int64_t cap, int32_t* hist_lens, int32_t* draft_new, zl_stream_t s) {
    return slots_admit_launch(ZL_SLOT_ARGS, nullptr, s);
}

int zl_slots_admit_fsm(const int32_t* blob, int64_t n, int64_t rec_words, int64_t b, int64_t vocab, int32_t* tokens, int32_t* positions,
                       int32_t* placement, int32_t* valid_lens, float* temperature, int32_t* top_k, float* top_p, int64_t* seeds,
                       int64_t* draws, float* logprobs, float* u, float* rep_penalty, float* presence, int32_t* seen, int64_t seen_ld,
                       int32_t* bias_ids, float* bias_vals, int32_t* bias_cnt, int32_t* bias_bits, int64_t bias_ld, int64_t bits_ld,
                       int32_t* top_ids, float* top_logprobs, int64_t top_n, int32_t* stop_ids, int32_t* stop_seqs, int32_t* seq_lens,
                       int64_t n_ids, int64_t n_seqs, int64_t seq_ld, int32_t* max_new, int32_t* gen_lens, int32_t* tail, int32_t* last_token,
                       int32_t* finished, int32_t* emit_lens, int32_t* live, int32_t* history, int64_t cap, int32_t* hist_lens,
                       int32_t* draft_new, int32_t* fsm_state, zl_stream_t s) {
    ZL_CHECK_ARG(!fsm_state || temperature, ZL_EINVAL);                 // the state belongs to a sampler
    return slots_admit_launch(ZL_SLOT_ARGS, fsm_state, s);
}
#undef ZL_SLOT_ARGS

}  // extern "C"
