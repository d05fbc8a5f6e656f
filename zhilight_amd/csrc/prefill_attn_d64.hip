// prefill_attn_d64.hip -- causal prompt attention for head size 64 on the matrix cores (zl_prefill_attn_d64, zl_prefill_attn_d64_varlen).
//
// The arithmetic is prefill_attn.hip's by definition: out[q,h,:] = softmax_{j <= pos(q)}(scale * q.K_j) . V, fp32 softmax with the running
// maximum starting at -1e20, probabilities rounded to T for the P.V product, fp32 accumulation, one rounding to T at the end, GQA
// hk = head / (h / hkv), K / V buffers BSHD (len_buf, Hkv, 64) or BHSD (Hkv, len_buf, 64).  The design is for D = 64:
//
//   work split   one workgroup = 64 query rows of one q head (the 64-row query tiles of ops.prefill_work_items, shared with D = 128),
//                4 waves x 16 rows, walking the keys in tiles of 128.  Per 64 keys a wave issues half the MFMAs of the D = 128 kernel
//                (2 per 16-key block for S^T, 4 column blocks of O) for the same exponentials and row-max steps, so what a tile costs
//                here is the softmax and the fixed steps -- two barriers, the running-max update, the rescale strip: a tile twice as
//                long halves those per key, in the LDS a 64-key tile takes at D = 128.
//   diagonal     a 128-key tile against a wave's 16 rows is mostly above the diagonal where it crosses it: each 32-key group a wave's
//                last row cannot see is skipped whole (wave-uniform: no S^T MFMAs, no exponentials, no P.V MFMAs -- its probabilities
//                are exactly 0, so the sums do not change).
//   staging      8 lanes load one 128-byte K (V) row as 16-byte pieces -- whole rows per request, 4 K + 4 V pieces per thread and tile --
//                and store them row-major with ds_write_b128.  The next tile's pieces ride one tile ahead in registers.
//   LDS          K rows are padded to 144 bytes: the b128 reads of S^T (16 lanes = 16 rows at one 16-byte column) start 36 dwords
//                apart, 36 r mod 64 = {0, 4, .., 60}: every bank once.  V rows are padded to 160 bytes: ds_read_b64_tr_b16 reads 8 rows
//                x 32 bytes per half wave, 40 r mod 64 = {0, 8, .., 56}: every bank once.  (The 272 / 288-byte strides of D = 128 are
//                the same residues, 4 and 8 dwords, on a 256-byte row.)  128 x (144 + 160) + 4 x 64 bytes = 39 168 bytes.
//   registers    S^T = K.Q^T: a lane's 32 scores belong to ONE query (lane & 15); rounded to T they ARE the A operand of P.V, no
//                transposition.  Q is two 16-byte fragments, O four accumulators (16 registers) per lane.
//   work map     longest first, the paired form when every workgroup is resident, the caller's table for the varlen launch: as in
//                prefill_attn.hip.  There are no wave groups (they measured slower at D = 128).
//
// A row's bits depend on its own query row and on the keys it sees only: tiles are cut at absolute key positions, the skipped groups
// and the tiles a row sees nothing of add exact zeros, and keys behind a workgroup's last visible key are never loaded (their slots
// hold a clamped K row and a zero V row), so neither len_buf nor the other tasks of a launch nor the entry point reach the result.
//
// Window / sink variant (WIN, zl_prefill_attn_d64_window / _varlen_window): the row at position t sees the keys
// max(0, t - window + 1) <= j <= t, and an optional per-head sink logit joins the normaliser (no value row).
//   tiles        the walk starts at the 128-key tile of the workgroup's first row's first key, k_lo = max(0, pos0 + q0 - window + 1),
//                and so do the staged loads: a workgroup touches at most window + 63 keys (+ the tile's rounding) however long the
//                prefix.  Slots of the first tile in front of k_lo are addressed at k_lo (a clamped K row, a zero V row), the mirror
//                image of the slots behind the last visible key: nothing outside a workgroup's rows' windows is loaded.
//   skip         a 32-key group wholly in front of the window of the wave's FIRST row is skipped, wave-uniformly, as a group
//                beyond the wave's last row is.  The lower-bound select runs only in tiles that reach in front of the window of the
//                wave's LAST row, as `diag` does for the upper edge.  A row whose window has not begun keeps the maximum -1e20, its
//                probabilities are exp2(-inf) = 0 exactly.
//   sink         once, in the normalise step: m = max(m_run, sink * log2 e), the factor exp2(m_run - m) on l and -- folded into the
//                reciprocal that goes through the strip -- on O, and exp2(sink * log2 e - m) added to l.
//   work map     the same tables and orders are accepted.  With a window every item walks about (window + 64) / 128 + 1 tiles, so
//                longest-first and the paired map neither help nor hurt: any order balances.
#include <stdlib.h>
#include "zl_common.h"

namespace {

constexpr int kBQ = 64, kBK = 128, kD = 64;
constexpr int kKRow = kD + 8;       // K tile row (halfs): 144 B
constexpr int kVRow = kD + 16;      // V tile row (halfs): 160 B

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

struct Prefill64Params {
    const uint16_t* q;      // (s_q, h, 64); varlen: (total_q, h, 64), task i's rows cu_q[i] .. cu_q[i + 1] - 1
    const uint16_t* k;      // the task's buffer, BSHD (len_buf, hkv, 64) or BHSD (hkv, len_buf, 64); varlen: k_bufs[task]
    const uint16_t* v;
    uint16_t* out;
    int s_q, pos0, h, hkv, n_rep, len_buf, bshd;
    float scale;
    int nx, pair;           // query tiles; pair != 0: the paired work map
    // varlen (work != nullptr): item w = (task, query tile) at work[2 w], work[2 w + 1]; s_q / pos0 / len_buf / k / v come from the tables
    const int32_t* work;
    const int32_t* cu_q;    // (b + 1)
    const int32_t* pos0s;   // (b)
    const int32_t* buf_lens;
    const uint16_t* const* k_bufs;
    const uint16_t* const* v_bufs;
    int n_work, b, total_q;
    // WIN: keys per row (0 < window <= 2^30; "no window" is 2^30) and the (h) fp32 sink logits or null
    int window;
    const float* sinks;
};

template <int DT>
__device__ __forceinline__ f4 pf64_mfma(uint4 a, uint4 b, f4 c) {
    typedef __bf16 b8 __attribute__((ext_vector_type(8)));
    if constexpr (DT == ZL_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
}

template <int DT>
__device__ __forceinline__ uint16_t pf64_round(float x) {      // a probability in [0, 1] -> T, nearest even
    if constexpr (DT == ZL_F16) return __builtin_bit_cast(uint16_t, (_Float16)x);
    else {
        const uint32_t u = __builtin_bit_cast(uint32_t, x);
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
}

template <int DT, bool WIN = false>
__global__ __launch_bounds__(256, 2) void k_prefill_attn_d64(const Prefill64Params p) {
    __shared__ __attribute__((aligned(16))) uint16_t ks[kBK * kKRow];
    __shared__ __attribute__((aligned(16))) uint16_t vt[kBK * kVRow];
    __shared__ __attribute__((aligned(16))) float strip[4][16];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nq = lane & 15, kq = lane >> 4;
    // work item k of the launch, longest first: query tile nx - 1 - k / h of head k % h.  Workgroup i takes item i, or (pair) the
    // first half of the workgroups takes the long items in order and the second half the short ones in reverse, so that the two
    // workgroups a CU receives add up to the same number of key tiles
    const int total = (p.work ? p.n_work : p.nx) * p.h;
    int item = (int)blockIdx.x;
    if (p.pair && item >= total / 2) item = total - 1 - (item - total / 2);
    const int head = item % p.h;
    int qt;
    const uint16_t* qb = p.q;
    const uint16_t* kb = p.k;
    const uint16_t* vb = p.v;
    uint16_t* ob = p.out;
    int s_q = p.s_q, pos0 = p.pos0, len_buf = p.len_buf;
    if (p.work) {
        // a wrong table cannot make the workgroup read or write outside the operands: an item outside the tasks or past its task's
        // rows is dropped (workgroup-uniform, before any barrier), rows are clamped to total_q and keys to the buffer's length
        const int w = item / p.h;
        const int task = __builtin_amdgcn_readfirstlane(p.work[2 * w]);
        qt = __builtin_amdgcn_readfirstlane(p.work[2 * w + 1]);
        if (task < 0 || task >= p.b || qt < 0) return;
        const int qa = max(p.cu_q[task], 0), qe = min(p.cu_q[task + 1], p.total_q);
        s_q = qe - qa;
        pos0 = max(p.pos0s[task], 0);
        len_buf = p.buf_lens[task];
        kb = p.k_bufs[task];
        vb = p.v_bufs[task];
        if (qt >= (s_q + kBQ - 1) / kBQ || len_buf <= 0 || !kb || !vb) return;
        qb += (size_t)qa * p.h * kD;
        ob += (size_t)qa * p.h * kD;
    } else {
        qt = p.nx - 1 - item / p.h;
    }
    const int hk = head / p.n_rep;
    const int q0 = qt * kBQ;
    const int qrow = q0 + wave * 16 + nq;                 // the query this lane's scores belong to
    const int qpos = pos0 + qrow;                         // keys 0 .. qpos are visible to it
    const int wave_last = pos0 + q0 + wave * 16 + 15;     // the last position any row of this wave may have
    const size_t kv_stride = p.bshd ? (size_t)p.hkv * kD : (size_t)kD;
    const size_t kv_off = p.bshd ? (size_t)hk * kD : (size_t)hk * len_buf * kD;

    // Q fragments (B operand of S^T = K.Q^T): column q = nq, k-chunk d = 32 t + 8 kq .. + 7
    uint4 qf[2];
    {
        const int qr = qrow < s_q ? qrow : s_q - 1;
        const uint16_t* qp = qb + ((size_t)qr * p.h + head) * kD + 8 * kq;
        qf[0] = *reinterpret_cast<const uint4*>(qp);
        qf[1] = *reinterpret_cast<const uint4*>(qp + 32);
    }

    f4 o[4];                                              // O block: column d = 16 db + nq, rows q = 4 kq + i
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = (f4){0.f, 0.f, 0.f, 0.f};
    float m_run = -1e20f, l_run = 0.f;                    // per query nq, replicated over kq (l: the lane's partial sum)

    const int last_q = min(q0 + kBQ, s_q) - 1;
    const int n_keys = min(pos0 + last_q + 1, len_buf);   // keys any row of this workgroup may see, never past the buffer
    const int n_tiles = (n_keys + kBK - 1) / kBK;
    // WIN: the workgroup's first visible key (addresses stay inside [k_lo, n_keys)), its tile, and the first keys of the windows of
    // the wave's first and last row
    const int k_lo = WIN ? min(max(pos0 + q0 - p.window + 1, 0), n_keys - 1) : 0;
    const int tile0 = WIN ? max(pos0 + q0 - p.window + 1, 0) / kBK : 0;
    const int wave_lo = WIN ? max(pos0 + q0 + wave * 16 - p.window + 1, 0) : 0;
    const int wave_lo_last = WIN ? max(wave_last - p.window + 1, 0) : 0;
    const int qlo = WIN ? qpos - p.window + 1 : 0;         // keys qlo .. qpos are visible to this lane's query

    // staging: thread -> 16-byte piece spc of the rows srow + 32 c.  Named registers: arrays filled from two places end up on the stack
    uint4 kr0, kr1, kr2, kr3, vr0, vr1, vr2, vr3;
    const int srow = threadIdx.x >> 3, spc = (threadIdx.x & 7) * 8;
#define ZL_P64_LOAD1(c_, key0_)                                                                            \
    {                                                                                                      \
        const int kg_ = (key0_) + srow + 32 * c_;                                                          \
        const int kc_ = WIN && kg_ < k_lo ? k_lo : (kg_ < n_keys ? kg_ : n_keys - 1);                      \
        const size_t ro_ = kv_off + (size_t)kc_ * kv_stride + spc;                                         \
        kr##c_ = *reinterpret_cast<const uint4*>(kb + ro_);                                                \
        vr##c_ = *reinterpret_cast<const uint4*>(vb + ro_);                                                \
        if (kg_ != kc_) vr##c_ = make_uint4(0, 0, 0, 0);      /* finite: its probability is exactly 0 */   \
    }
#define ZL_P64_LOAD(tile_) ZL_P64_LOAD1(0, (tile_) * kBK) ZL_P64_LOAD1(1, (tile_) * kBK) ZL_P64_LOAD1(2, (tile_) * kBK) ZL_P64_LOAD1(3, (tile_) * kBK)
#define ZL_P64_ST(c_)                                                                                      \
    *reinterpret_cast<uint4*>(&ks[(srow + 32 * c_) * kKRow + spc]) = kr##c_;                               \
    *reinterpret_cast<uint4*>(&vt[(srow + 32 * c_) * kVRow + spc]) = vr##c_;
    ZL_P64_LOAD(tile0)

    const float sl2 = p.scale * 1.44269504088896340736f;  // scores live in the log2 domain: v_exp_f32 is exp2
    typedef short s4 __attribute__((ext_vector_type(4)));
    typedef short s8 __attribute__((ext_vector_type(8)));
    const uint16_t* vtr = vt + (4 * kq + (nq >> 2)) * kVRow + 4 * (nq & 3);

    for (int tile = tile0; tile < n_tiles; ++tile) {
        const int key0 = tile * kBK;
        __syncthreads();                                  // the previous tile is consumed
        ZL_P64_ST(0) ZL_P64_ST(1) ZL_P64_ST(2) ZL_P64_ST(3)
        __syncthreads();
        ZL_P64_LOAD(tile + 1)                             // clamped past the end; in flight during this tile's MFMAs

        // ---- S^T = K . Q^T per 32-key group j (two 16-key blocks x two d steps); lane: query nq, keys key0 + 16 kb + 4 kq + i.
        //      A group beyond the wave's last row is skipped; the causal select runs only where the tile reaches the wave's diagonal
        const bool diag = key0 + kBK - 1 > pos0 + q0 + wave * 16;
        const bool edge = WIN && key0 < wave_lo_last;     // some key of the tile lies in front of some row's window
        f4 st[8];
        float mloc = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (key0 + 32 * j > wave_last) continue;      // wave-uniform
            if (WIN && key0 + 32 * j + 31 < wave_lo) continue;
#pragma unroll
            for (int kb2 = 2 * j; kb2 < 2 * j + 2; ++kb2) {
                const uint16_t* kp = &ks[(kb2 * 16 + nq) * kKRow + 8 * kq];
                f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
                acc = pf64_mfma<DT>(*reinterpret_cast<const uint4*>(kp), qf[0], acc);
                acc = pf64_mfma<DT>(*reinterpret_cast<const uint4*>(kp + 32), qf[1], acc);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = key0 + kb2 * 16 + 4 * kq + i;
                    const float sv = ((!diag || key <= qpos) && (!edge || key >= qlo)) ? acc[i] * sl2 : -INFINITY;
                    acc[i] = sv;
                    mloc = fmaxf(mloc, sv);
                }
                st[kb2] = acc;
            }
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        const float m_new = fmaxf(m_run, mloc);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        // ---- rescale O: the factor of row q = 4 kq + i comes from the lane whose nq is that row, through the wave's strip -- only when
        //      some row's maximum moved (wave-uniform; a factor of 1 changes no bit)
        if (!__all(alpha == 1.0f)) {
            if (kq == 0) strip[wave][nq] = alpha;
            __builtin_amdgcn_s_waitcnt(0xc07f);           // lgkmcnt(0): the strip write has landed (wave-private)
            const f4 al = *reinterpret_cast<const f4*>(&strip[wave][4 * kq]);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                o[db][0] *= al[0]; o[db][1] *= al[1]; o[db][2] *= al[2]; o[db][3] *= al[3];
            }
        }
        // ---- P = exp2(S - m) rounded to T, O += P . V per group: A = the lane's 8 probabilities (keys 32 j + {4 kq + i, 16 + 4 kq + i}),
        //      B (column d = 16 db + nq, the same keys) = two transposed 8-byte reads of the row-major V tile
        float lsum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (key0 + 32 * j > wave_last) continue;
            if (WIN && key0 + 32 * j + 31 < wave_lo) continue;
            uint32_t w[4];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
#pragma unroll
                for (int i2 = 0; i2 < 2; ++i2) {
                    const uint16_t p0 = pf64_round<DT>(__builtin_amdgcn_exp2f(st[2 * j + half][2 * i2] - m_new));
                    const uint16_t p1 = pf64_round<DT>(__builtin_amdgcn_exp2f(st[2 * j + half][2 * i2 + 1] - m_new));
                    lsum += ZT<DT>::to_f32(p0) + ZT<DT>::to_f32(p1);   // the normaliser sums what the product uses
                    w[half * 2 + i2] = (uint32_t)p0 | ((uint32_t)p1 << 16);
                }
            }
            const uint4 pa = make_uint4(w[0], w[1], w[2], w[3]);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(vtr + (32 * j) * kVRow + 16 * db));
                const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(vtr + (32 * j + 16) * kVRow + 16 * db));
                const s8 bv = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                o[db] = pf64_mfma<DT>(pa, __builtin_bit_cast(uint4, bv), o[db]);
            }
        }
        l_run = l_run * alpha + lsum;
    }
#undef ZL_P64_ST
#undef ZL_P64_LOAD
#undef ZL_P64_LOAD1

    // ---- normalise: l of query nq = the sum over its 4 lanes; 1 / l reaches the C layout through the strip
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    float inv_l = 1.0f / (l_run + 1e-20f);
    if constexpr (WIN) {
        if (p.sinks) {
            const float sk = p.sinks[head] * 1.44269504088896340736f;
            const float m2 = fmaxf(m_run, sk);
            const float f = __builtin_amdgcn_exp2f(m_run - m2);
            inv_l = f / (l_run * f + __builtin_amdgcn_exp2f(sk - m2) + 1e-20f);
        }
    }
    if (kq == 0) strip[wave][nq] = inv_l;
    __builtin_amdgcn_s_waitcnt(0xc07f);
    const f4 inv = *reinterpret_cast<const f4*>(&strip[wave][4 * kq]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = q0 + wave * 16 + 4 * kq + i;
        if (row >= s_q) continue;
        uint16_t* op = ob + ((size_t)row * p.h + head) * kD + nq;
#pragma unroll
        for (int db = 0; db < 4; ++db) op[db * 16] = ZT<DT>::from_f32(o[db][i] * inv[i]);
    }
}

// one workgroup per (work item, head); the paired map when the launch has at most two workgroups per CU (all resident at once: three
// fit by registers), the rule of the D = 128 launch
int launch_prefill_d64(Prefill64Params& p, int64_t items, int dtype, hipStream_t hs) {
    ZL_CHECK_ARG(items * p.h < ((int64_t)1 << 31), ZL_ELIMIT);
    const int total = (int)(items * p.h);
    int cus = zl_device_cu_count();
    if (cus <= 0) cus = 256;
    p.pair = (total % 2 == 0 && total <= 2 * cus) ? 1 : 0;
    if (p.window > 0) {
        if (dtype == ZL_F16) hipLaunchKernelGGL((k_prefill_attn_d64<ZL_F16, true>), dim3((unsigned)total), dim3(256), 0, hs, p);
        else hipLaunchKernelGGL((k_prefill_attn_d64<ZL_BF16, true>), dim3((unsigned)total), dim3(256), 0, hs, p);
    } else {
        if (dtype == ZL_F16) hipLaunchKernelGGL(k_prefill_attn_d64<ZL_F16>, dim3((unsigned)total), dim3(256), 0, hs, p);
        else hipLaunchKernelGGL(k_prefill_attn_d64<ZL_BF16>, dim3((unsigned)total), dim3(256), 0, hs, p);
    }
    return zl_launch_status();
}

// the window entry points' two arguments (window >= 0 checked) -> the kernel's: every row sees at most 2^30 keys
void set_window(Prefill64Params& p, int64_t window, const float* sinks) {
    constexpr int64_t kNone = (int64_t)1 << 30;
    p.window = (int)(window == 0 || window > kNone ? kNone : window);
    p.sinks = sinks;
}

}  // namespace

// the one-task launch; win: the WIN instantiation with `window` (>= 0, 0 = none) and `sinks` (or null)
static int prefill_d64(const uint16_t* q, const uint16_t* k_buf, const uint16_t* v_buf, uint16_t* out, int64_t s_q, int64_t pos0,
                       int64_t h, int64_t hkv, float scale, int64_t len_buf, int bshd, int dtype, bool win, int64_t window,
                       const float* sinks, zl_stream_t s) {
    ZL_CHECK_ARG(q && k_buf && v_buf && out && s_q > 0 && pos0 >= 0 && h > 0 && hkv > 0 && len_buf > 0, ZL_EINVAL);
    ZL_CHECK_ARG(!win || window >= 0, ZL_EINVAL);
    ZL_CHECK_ARG(h % hkv == 0 && pos0 + s_q <= len_buf, ZL_ESHAPE);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(h <= 65535 && len_buf < ((int64_t)1 << 31), ZL_ELIMIT);
    Prefill64Params p = {};
    p.q = q; p.k = k_buf; p.v = v_buf; p.out = out;
    p.s_q = (int)s_q; p.pos0 = (int)pos0; p.h = (int)h; p.hkv = (int)hkv; p.n_rep = (int)(h / hkv);
    p.len_buf = (int)len_buf; p.bshd = bshd; p.scale = scale;
    p.nx = (int)((s_q + kBQ - 1) / kBQ);
    if (win) set_window(p, window, sinks);
    return launch_prefill_d64(p, p.nx, dtype, (hipStream_t)s);
}

static int prefill_d64_varlen(const uint16_t* q, const int32_t* cu_seqlens_q, const int32_t* pos0, const int32_t* buf_lens,
                              const uint16_t* const* k_bufs, const uint16_t* const* v_bufs, uint16_t* out, const int32_t* work,
                              int64_t n_work, int64_t b, int64_t total_q, int64_t h, int64_t hkv, float scale, int bshd, int dtype,
                              bool win, int64_t window, const float* sinks, zl_stream_t s) {
    ZL_CHECK_ARG(q && cu_seqlens_q && pos0 && buf_lens && k_bufs && v_bufs && out && work, ZL_EINVAL);
    ZL_CHECK_ARG(b > 0 && total_q > 0 && n_work > 0 && h > 0 && hkv > 0 && (!win || window >= 0), ZL_EINVAL);
    ZL_CHECK_ARG(h % hkv == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(h <= 65535 && b < ((int64_t)1 << 30) && total_q < ((int64_t)1 << 31) && n_work < ((int64_t)1 << 31), ZL_ELIMIT);
    Prefill64Params p = {};
    p.q = q; p.out = out;
    p.h = (int)h; p.hkv = (int)hkv; p.n_rep = (int)(h / hkv); p.bshd = bshd; p.scale = scale;
    p.work = work; p.cu_q = cu_seqlens_q; p.pos0s = pos0; p.buf_lens = buf_lens; p.k_bufs = k_bufs; p.v_bufs = v_bufs;
    p.n_work = (int)n_work; p.b = (int)b; p.total_q = (int)total_q;
    if (win) set_window(p, window, sinks);
    return launch_prefill_d64(p, n_work, dtype, (hipStream_t)s);
}

extern "C" {

int zl_prefill_attn_d64(const uint16_t* q, const uint16_t* k_buf, const uint16_t* v_buf, uint16_t* out, int64_t s_q, int64_t pos0,
                        int64_t h, int64_t hkv, float scale, int64_t len_buf, int bshd, int dtype, zl_stream_t s) {
    return prefill_d64(q, k_buf, v_buf, out, s_q, pos0, h, hkv, scale, len_buf, bshd, dtype, false, 0, nullptr, s);
}

int zl_prefill_attn_d64_window(const uint16_t* q, const uint16_t* k_buf, const uint16_t* v_buf, uint16_t* out, int64_t s_q, int64_t pos0,
                               int64_t h, int64_t hkv, float scale, int64_t len_buf, int bshd, int dtype, int64_t window,
                               const float* sinks, zl_stream_t s) {
    return prefill_d64(q, k_buf, v_buf, out, s_q, pos0, h, hkv, scale, len_buf, bshd, dtype, true, window, sinks, s);
}

int zl_prefill_attn_d64_varlen(const uint16_t* q, const int32_t* cu_seqlens_q, const int32_t* pos0, const int32_t* buf_lens,
                               const uint16_t* const* k_bufs, const uint16_t* const* v_bufs, uint16_t* out, const int32_t* work,
                               int64_t n_work, int64_t b, int64_t total_q, int64_t h, int64_t hkv, float scale, int bshd, int dtype,
                               zl_stream_t s) {
    return prefill_d64_varlen(q, cu_seqlens_q, pos0, buf_lens, k_bufs, v_bufs, out, work, n_work, b, total_q, h, hkv, scale, bshd,
                              dtype, false, 0, nullptr, s);
}

int zl_prefill_attn_d64_varlen_window(const uint16_t* q, const int32_t* cu_seqlens_q, const int32_t* pos0, const int32_t* buf_lens,
                                      const uint16_t* const* k_bufs, const uint16_t* const* v_bufs, uint16_t* out, const int32_t* work,
                                      int64_t n_work, int64_t b, int64_t total_q, int64_t h, int64_t hkv, float scale, int bshd,
                                      int dtype, int64_t window, const float* sinks, zl_stream_t s) {
    return prefill_d64_varlen(q, cu_seqlens_q, pos0, buf_lens, k_bufs, v_bufs, out, work, n_work, b, total_q, h, hkv, scale, bshd,
                              dtype, true, window, sinks, s);
}

}  // extern "C"
