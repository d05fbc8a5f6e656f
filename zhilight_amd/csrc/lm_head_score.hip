// lm_head_score.hip -- score every row against the lm_head without storing the logits: per row of y = x . W^T the log-sum-exp,
// the label's logit, the label's log-probability and the arg-max, formed in the epilogue of the GEMM tile that computes y.
//
// Replaces the reference's functions::Gemm + nn::log_prob_raw / greedy_match_raw (src/nn/functions/cross_entropy.cu:7-69, 358-403,
// called by LLaMA::calc_log_prob / calc_greedy_match, src/model/llama.cpp:220-244), which write the (M, N) logits, read them for
// max, sum and log-softmax and write an (M, N) probability tensor to keep one number per row.
//
// Numerics contract: y[m, n] is the value zl_gemm_nt would have stored -- fp32 MFMA accumulation over K in ascending 128-k chunks
// with v_mfma_f32_16x16x32_{f16,bf16} (k_dense_gemm's main loop, dense_gemm.hip, repeated here so that file's code generation stays
// what it is), ONE rounding to T -- and max / exp / sum / arg-max run on that rounded value in fp32.  label_logit, greedy and
// greedy_logit are therefore exact functions of zl_gemm_nt's output; lse carries a summation-order tolerance only.
//
// Launch 1 (k_score_tile): workgroup = 4 waves = BM rows x 128 columns.  Per (row, 128-column block) it leaves one 16-byte record
// {max, sum exp(y - max), max again as the arg-max value, col0 + lowest column that attains it} in the workspace (M, NB) and, in the
// block that holds the row's label, the label's logit in the workspace's tail.  Reduction order inside a block: the two columns of
// a lane, a 16-lane butterfly, the four waves in ascending order -- fixed, no atomics.
// Launch 2 (k_score_merge): one wave per row over its NB records: max of the maxima, sum of s_b exp(m_b - max) with the lanes
// striding the blocks in ascending order and a butterfly, lse = max + log(sum); the arg-max with the lowest column on ties.
//
// Launch order of the tiles (the matrix is 1.05 GB at Llama-3 geometry and the rows are thousands, unlike zl_gemm_nt's callers):
// a 1-D grid with the ROW tile fastest, so all row tiles of a column block are adjacent and a 128-column weight tile (1 MB at
// K = 4096) is fetched from HBM once and served to the other row tiles from L2.  Workgroups are dealt round-robin to the 8 XCDs,
// each with its own L2: with few row tiles the adjacent tiles of a column block land on different XCDs and each fetches the weights
// again, so up to 16 row tiles (order 1) workgroup b takes tile (b mod 8) * ceil(tiles / 8) + b / 8 -- an XCD runs a contiguous
// range of tiles.  Beyond that every XCD holds several row tiles of a column block anyway and the plain order (0) is 4 % faster
// (DESIGN.md has the table; zl_gemm_nt's column-block-fastest order was measured 37-45 % slower and is not built).
// zl_lm_head_score_ex takes the order explicitly for A/B runs; the results do not depend on it.
// Logits are assumed finite: a rounded logit of +inf (fp16 overflow) makes the row's lse NaN (inf - inf).
#include "zl_common.h"

namespace {

constexpr int kSW = 4, kST = kSW * 64, kSBN = kSW * 32, kSRow = 128 + 8, kXcd = 8;

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

struct ScoreParams {
    const uint16_t* x;
    int64_t ldx;
    const uint16_t* w;
    const int32_t* labels;
    float4* part;            // (m, nb) records
    float* label_ws;         // (m) the label's logit, written by the block that holds it
    int ignore_index, col0;
    int m, n, k, groups;
    int nb, mt, order, per_xcd;
};

template <int DT>
__device__ __forceinline__ f4 mfma16(uint4 a, uint4 b, f4 c) {
    if constexpr (DT == ZL_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
}

// (value, column) candidates: the larger value, the lower column on equal values
__device__ __forceinline__ void arg_take(float& v, int& c, float ov, int oc) {
    if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
}

template <int DT, int BM>
__global__ __launch_bounds__(kST, 2) void k_score_tile(const ScoreParams p) {
    constexpr int RB = BM / 16, XR = BM / 16;
    __shared__ __attribute__((aligned(16))) uint16_t xs[2][BM * kSRow];
    __shared__ float red_v[kSW][BM];
    __shared__ int red_c[kSW][BM];
    __shared__ float red_s[kSW][BM];

    // tile of this workgroup
    int tile = blockIdx.x;
    if (p.order == 1) {                      // XCD x of the round-robin runs the contiguous tiles [x * per_xcd, (x + 1) * per_xcd)
        tile = (blockIdx.x % kXcd) * p.per_xcd + blockIdx.x / kXcd;
        if (tile >= p.mt * p.nb) return;     // workgroup-uniform, before any barrier
    }
    const int bx = tile / p.mt;              // column block
    const int by = tile % p.mt;              // row tile: fastest, so all row tiles of a column block are adjacent

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nrow = lane & 15, kq = lane >> 4;
    const int m0 = by * BM;
    const int n_base = bx * kSBN + wave * 32;
    const int G = p.groups;

    // ---- k_dense_gemm's main loop (NS = 2, row-major weights): the per-element K order is zl_gemm_nt's ----
    int nr[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n_base + 16 * j + nrow;
        nr[j] = n < p.n ? n : p.n - 1;
    }
    uint4 wf[2][2][4];                       // [ring slot][tile][t]
    auto load_w = [&](int slot, int g) {
        const int gc = g < G ? g : G - 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint16_t* src = p.w + (size_t)nr[j] * p.k + (size_t)gc * 128 + 8 * kq;
#pragma unroll
            for (int t = 0; t < 4; ++t) wf[slot][j][t] = *reinterpret_cast<const uint4*>(src + 32 * t);   // (re-read by the other row tiles: cached)
        }
    };
    const int xrow = threadIdx.x >> 4, xcol = (threadIdx.x & 15) * 8;
    uint4 xr[XR];
    auto load_x = [&](int g) {
        const int gc = g < G ? g : G - 1;
#pragma unroll
        for (int r = 0; r < XR; ++r) {
            const int row = m0 + xrow + 16 * r;
            const int rc = row < p.m ? row : p.m - 1;
            xr[r] = *reinterpret_cast<const uint4*>(p.x + (size_t)rc * p.ldx + (size_t)gc * 128 + xcol);
            if (row >= p.m) xr[r] = make_uint4(0, 0, 0, 0);
        }
    };
    auto store_x = [&](int buf) {
#pragma unroll
        for (int r = 0; r < XR; ++r) *reinterpret_cast<uint4*>(&xs[buf][(xrow + 16 * r) * kSRow + xcol]) = xr[r];
    };

    load_x(0);
    load_w(0, 0);
    load_w(1, 1);
    store_x(0);
    load_x(1);
    __syncthreads();

    f4 acc[RB][2];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        acc[rb][0] = (f4){0.f, 0.f, 0.f, 0.f};
        acc[rb][1] = (f4){0.f, 0.f, 0.f, 0.f};
    }

#pragma unroll 1
    for (int g = 0; g < G; g += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (g + u < G) {                 // workgroup-uniform; g even: chunk parity = u
                const uint16_t* xb = &xs[u][nrow * kSRow + kq * 8];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        const uint4 a = *reinterpret_cast<const uint4*>(xb + rb * 16 * kSRow + t * 32);
                        acc[rb][0] = mfma16<DT>(a, wf[u][0][t], acc[rb][0]);
                        acc[rb][1] = mfma16<DT>(a, wf[u][1][t], acc[rb][1]);
                    }
                }
                load_w(u, g + u + 2);
                store_x(u ^ 1);
                load_x(g + u + 2);
                __syncthreads();
            }
        }
    }

    // ---- epilogue: acc[rb][j][i] is y[m0 + 16 rb + 4 kq + i][n_base + 16 j + nrow] before its rounding ----
    const int c0 = n_base + nrow, c1 = c0 + 16;
    const bool ok0 = c0 < p.n, ok1 = c1 < p.n;
    const float ninf = -__builtin_inff();
    float y[RB][2][4];
    int lab[RB][4];                                          // the lane's rows' labels relative to col0; -1: none in this launch's columns
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + rb * 16 + 4 * kq + i;
            const int l = (p.labels && row < p.m) ? p.labels[row] : p.ignore_index;
            lab[rb][i] = (l != p.ignore_index && l >= p.col0) ? l - p.col0 : -1;
        }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int tr = rb * 16 + 4 * kq + i;             // row of the tile
            const float y0 = ok0 ? ZT<DT>::to_f32(ZT<DT>::from_f32(acc[rb][0][i])) : ninf;
            const float y1 = ok1 ? ZT<DT>::to_f32(ZT<DT>::from_f32(acc[rb][1][i])) : ninf;
            y[rb][0][i] = y0;
            y[rb][1][i] = y1;
            if (ok0 && lab[rb][i] == c0) p.label_ws[m0 + tr] = y0;
            if (ok1 && lab[rb][i] == c1) p.label_ws[m0 + tr] = y1;
            float v = y0;
            int c = c0;
            if (y1 > v) { v = y1; c = c1; }                  // c1 > c0: the lower column stays on a tie
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) {          // the 16 lanes of one kq hold the row's 32 columns of this wave
                const float ov = __shfl_xor(v, off, 64);
                const int oc = __shfl_xor(c, off, 64);
                arg_take(v, c, ov, oc);
            }
            if (nrow == 0) {
                red_v[wave][tr] = v;
                red_c[wave][tr] = c;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int tr = rb * 16 + 4 * kq + i;
            // the block's first column is < N, so the maximum is finite; columns >= N are -inf and add exp(-inf) = 0
            const float mx = fmaxf(fmaxf(red_v[0][tr], red_v[1][tr]), fmaxf(red_v[2][tr], red_v[3][tr]));
            float s = __expf(y[rb][0][i] - mx) + __expf(y[rb][1][i] - mx);
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (nrow == 0) red_s[wave][tr] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < BM) {
        const int tr = threadIdx.x, row = m0 + tr;
        if (row < p.m) {
            float v = red_v[0][tr];
            int c = red_c[0][tr];
            float s = red_s[0][tr];
#pragma unroll
            for (int w = 1; w < kSW; ++w) {
                arg_take(v, c, red_v[w][tr], red_c[w][tr]);
                s += red_s[w][tr];
            }
            p.part[(size_t)row * p.nb + bx] = make_float4(v, s, v, __int_as_float(p.col0 + c));
        }
    }
}

struct MergeParams {
    const float4* part;
    const float* label_ws;
    const int32_t* labels;
    float *lse, *label_logit, *logprob, *greedy_logit;
    int32_t* greedy;
    int ignore_index, col0, m, n, nb;
};

__global__ __launch_bounds__(256) void k_score_merge(const MergeParams p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.m) return;                  // wave-uniform
    const float4* rec = p.part + (size_t)row * p.nb;
    float v = -__builtin_inff();
    int c = 0x7fffffff;
    for (int b = lane; b < p.nb; b += 64) {  // ascending blocks = ascending columns: a strict > keeps the lowest column
        const float4 r = rec[b];
        if (r.z > v) { v = r.z; c = __float_as_int(r.w); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oc = __shfl_xor(c, off, 64);
        arg_take(v, c, ov, oc);
    }
    float s = 0.f;
    for (int b = lane; b < p.nb; b += 64) {
        const float4 r = rec[b];
        s += r.y * expf(r.x - v);            // v: the row's maximum in every lane
    }
    s = zl_wave_sum(s);
    if (lane == 0) {
        const float lse = v + logf(s);
        float ll = 0.f;
        bool has = false;
        if (p.labels) {
            const int lab = p.labels[row];
            has = lab != p.ignore_index && lab >= p.col0 && lab < p.col0 + p.n;
            if (has) ll = p.label_ws[row];
        }
        if (p.lse) p.lse[row] = lse;
        if (p.label_logit) p.label_logit[row] = ll;
        if (p.logprob) p.logprob[row] = has ? ll - lse : 0.f;
        if (p.greedy) p.greedy[row] = c;
        if (p.greedy_logit) p.greedy_logit[row] = v;
    }
}

}  // namespace

// (m, ceil(n / 128)) 16-byte records + m label logits (rounded up to 16 bytes)
extern "C" int64_t zl_lm_head_score_ws_bytes(int64_t m, int64_t n) {
    if (m <= 0 || n <= 0) return ZL_EINVAL;
    if (m >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return ZL_ESHAPE;
    const int64_t nb = (n + kSBN - 1) / kSBN;
    return m * nb * 16 + (m * 4 + 15) / 16 * 16;
}

extern "C" int zl_lm_head_score(const uint16_t* x, int64_t ldx, const uint16_t* w, const int32_t* labels, int32_t ignore_index,
                                int32_t col0, float* lse, float* label_logit, float* logprob, int32_t* greedy, float* greedy_logit,
                                void* workspace, int64_t m, int64_t n, int64_t k, int dtype, zl_stream_t s) {
    return zl_lm_head_score_ex(x, ldx, w, labels, ignore_index, col0, lse, label_logit, logprob, greedy, greedy_logit, workspace, m, n, k,
                               dtype, ZL_SCORE_ORDER_AUTO, s);
}

extern "C" int zl_lm_head_score_ex(const uint16_t* x, int64_t ldx, const uint16_t* w, const int32_t* labels, int32_t ignore_index,
                                   int32_t col0, float* lse, float* label_logit, float* logprob, int32_t* greedy, float* greedy_logit,
                                   void* workspace, int64_t m, int64_t n, int64_t k, int dtype, int order, zl_stream_t s) {
    ZL_CHECK_ARG(order >= ZL_SCORE_ORDER_AUTO && order <= 1, ZL_EINVAL);
    ZL_CHECK_ARG(x && w && workspace && m > 0 && n > 0 && k > 0, ZL_EINVAL);
    ZL_CHECK_ARG(k % 128 == 0 && ldx % 8 == 0 && ldx >= k && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 &&
                 ((uintptr_t)workspace & 15) == 0 && k < ((int64_t)1 << 31), ZL_ESHAPE);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(m < ((int64_t)1 << 31) && n < ((int64_t)1 << 31) && (int64_t)col0 + n <= 0x7fffffff && col0 >= 0, ZL_ESHAPE);
    const int bm = m <= 16 ? 16 : (m <= 32 ? 32 : 64);
    const int64_t nb = (n + kSBN - 1) / kSBN, mt = (m + bm - 1) / bm;
    const int64_t per_xcd = (mt * nb + kXcd - 1) / kXcd;
    ZL_CHECK_ARG(per_xcd * kXcd <= 0x7fffffff && m * nb <= 0x7fffffff, ZL_ELIMIT);
    ScoreParams p;
    p.x = x; p.ldx = ldx; p.w = w; p.labels = labels;
    p.part = reinterpret_cast<float4*>(workspace);
    p.label_ws = reinterpret_cast<float*>(p.part + m * nb);
    p.ignore_index = ignore_index; p.col0 = col0;
    p.m = (int)m; p.n = (int)n; p.k = (int)k; p.groups = (int)(k / 128);
    p.nb = (int)nb; p.mt = (int)mt; p.order = order == ZL_SCORE_ORDER_AUTO ? (mt <= 16 ? 1 : 0) : order; p.per_xcd = (int)per_xcd;
    const dim3 grid((unsigned)(p.order == 1 ? per_xcd * kXcd : mt * nb));
    hipStream_t hs = (hipStream_t)s;
#define ZL_SC(DT)                                                                         \
    if (bm == 16) hipLaunchKernelGGL((k_score_tile<DT, 16>), grid, dim3(kST), 0, hs, p);  \
    else if (bm == 32) hipLaunchKernelGGL((k_score_tile<DT, 32>), grid, dim3(kST), 0, hs, p); \
    else hipLaunchKernelGGL((k_score_tile<DT, 64>), grid, dim3(kST), 0, hs, p);
    if (dtype == ZL_F16) { ZL_SC(ZL_F16) } else { ZL_SC(ZL_BF16) }
#undef ZL_SC
    int st = zl_launch_status();
    if (st != ZL_OK) return st;
    MergeParams q;
    q.part = p.part; q.label_ws = p.label_ws; q.labels = labels;
    q.lse = lse; q.label_logit = label_logit; q.logprob = logprob; q.greedy_logit = greedy_logit; q.greedy = greedy;
    q.ignore_index = ignore_index; q.col0 = col0; q.m = (int)m; q.n = (int)n; q.nb = (int)nb;
    hipLaunchKernelGGL(k_score_merge, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, hs, q);
    return zl_launch_status();
}
