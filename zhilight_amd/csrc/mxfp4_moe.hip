// mxfp4_moe.hip -- the routed feed-forward of MXFP4 mixture-of-experts models (include/zhilight_amd.h "MXFP4", expert stacks): ONE
// launch multiplies every active expert's MXFP4 matrix with that expert's routed rows, T = fp16 / bf16.
//
// OPERAND.  An expert stack is the checkpoint's tensors, stacked: codes uint8 (E, N, K/2), scales uint8 (E, N, K/32), expert e
// `stride` bytes after expert 0 (one stride per tensor).  No packed copy: 0.53125 B per weight.  K % 32 == 0 is the only shape rule.
//
// NUMERICS: those of mxfp4.hip, through the same device code (zl_mxfp4.h) -- no weight is rounded, the unscaled E2M1 values meet the
// activations in exact products, a block's 32-term partial sum is scaled by 2^(e - 127) in fp32 and joins the fp32 accumulator, one
// rounding to T, then the epilogue's (0 or ZL_EPI_SILU_MUL on a row-interleaved gate|up stack: gate and up rounded to T, T(silu(g) u)).
// One workgroup owns an output over all of K: no atomics, the same bits on every run.
//
// GROUPED FORM (rows sorted by expert: decode batches, prompts).  The work table is w4_moe_grouped.hip's: expert e owns the run of
// loads[e] sorted positions after those of the experts before it, runs are cut into BM-row tiles, blockIdx.y enumerates the tiles of all
// experts in expert order and every workgroup derives its (expert, tile, offset, length) from the device-side loads in a wave-wide
// scan; the host only sizes the grid from the bound pairs / BM + min(E, pairs), idle slots exit, nothing synchronises with the host.
// THE GATHER IS FREE: mx_run reads its A fragments from global memory through one row pointer per lane, so lane (nrow, kq) simply
// points at x + clamp(index[off + row] / in_div) ldx -- no LDS staging of the activations, no gathered copy.  A tile's output rows
// (j or index[j]) sit one per lane and reach the epilogue by shuffle.
//   BM 16 / 32 (a few rows per expert, many experts: decode)   k_mxfp4_moe_stream: workgroup = 16 weight rows of the expert x BM sorted
//       rows, its 4 waves split K by quads of four blocks (quad j -> wave j % 4) and fold through LDS: the structure of k_mxfp4_stream.
//       An expert's weights are read once per BM of its rows.
//   BM 64 (prompts)   k_mxfp4_moe_tiled: workgroup = 64 sorted rows x 64 weight rows, a wave 16 weight rows x 64 rows over all of K: the
//       structure of k_mxfp4_tiled, no K split between waves and no barrier.
// A ROW'S BITS DO NOT DEPEND ON ITS TILE: continuous batching moves a row between tiles, tile shapes and tile positions from step to
// step.  An MFMA output depends on its own A row only, and both kernels sum K in ONE order: four sums, quad j into sum j % 4 in walk
// order, folded as ((s0 + s1) + s2) + s3.  The stream kernel keeps one sum per wave; the tiled kernel keeps all four in one wave's
// registers (mx_run's NC = 4) -- 64 accumulators per lane buy the same bits at every BM.
//
// PAIRS FORM (the first few rows of a decode step; no sort, no table): blockIdx.y = pair j, expert ids[j] (outside the stack: row j is
// not written), activation row j / in_div, output row j; the GEMV walk of k_mxfp4_gemv (mx_gemv_run): a wave owns two weight rows, lane
// l walks blocks l, l + 64, ... -- batch 1 of Qwen3-MoE is 8 pairs over 8 different experts.
// The two forms sum in different orders (an FMA chain per lane and a butterfly against MFMA partial sums): they are NOT bit-equal to
// each other, unlike the GPTQ pair zl_w4a16_gemm_grouped / _pairs, whose pairs form is the grouped kernel at one row.  Both stay
// inside the same error bound; a row keeps its bits for as long as it stays in one form.
#include "zl_mxfp4.h"

namespace {

typedef mx_f4 f4;

// the tile's rows: lane (nrow, kq)'s A-fragment pointers (tile row 16 t + nrow) and, in lane l, the output row of tile row l (< 0: none)
template <int MT>
__device__ __forceinline__ int mx_moe_rows(const Mx4MoeParams& p, const Mx4MoeTile& w, int lane, const uint16_t* (&xrow)[MT], bool (&live)[MT]) {
    const int nrow = lane & 15;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int lr = 16 * t + nrow;
        live[t] = lr < w.nvalid;
        int src = 0;
        if (live[t]) {
            const int j = w.pos0 + lr;
            src = p.in_div > 0 ? p.index[j] / p.in_div : j;
            src = src < 0 ? 0 : (src >= p.x_rows ? p.x_rows - 1 : src);
        }
        xrow[t] = p.x + (size_t)src * p.ldx;
    }
    int dst = -1;
    if (lane < w.nvalid) {
        const int j = w.pos0 + lane;
        dst = p.out_scatter ? p.index[j] : j;
        if (dst < 0 || dst >= p.y_rows) dst = -1;
    }
    return dst;
}

template <int DT, int MT>
__global__ __launch_bounds__(256) void k_mxfp4_moe_stream(const Mx4MoeParams p) {
    __shared__ float red[3][MT * 4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nrow = lane & 15, kq = lane >> 4;
    const Mx4MoeTile w = mx_moe_tile<16 * MT>(p, blockIdx.y, lane);
    if (w.expert < 0) return;                     // the whole workgroup
    const int n = blockIdx.x * 16 + nrow;
    const int nc = n < p.n ? n : p.n - 1;
    const uint32_t* crow = reinterpret_cast<const uint32_t*>(p.codes + (size_t)w.expert * p.stride_codes + (size_t)nc * (p.k / 2));
    const uint8_t* srow = p.scales + (size_t)w.expert * p.stride_scales + (size_t)nc * p.nb;
    const uint16_t* xrow[MT];
    bool live[MT];
    f4 acc[MT];
    const int dst = mx_moe_rows<MT>(p, w, lane, xrow, live);
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = (f4){0.f, 0.f, 0.f, 0.f};
    mx_run<DT, MT, 2>(p, crow, srow, wave, 4, xrow, live, kq, acc);

    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[wave - 1][t * 4 + i][lane] = acc[t][i];
    }
    __syncthreads();
    if (wave == 0) {
        const int ld = mx_ld_out(p);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][i] = ((acc[t][i] + red[0][t * 4 + i][lane]) + red[1][t * 4 + i][lane]) + red[2][t * 4 + i][lane];
            mx_store_tile<DT>(p, 16 * t, n, kq, acc[t], [&](int r) { return __shfl(dst, r, 64); }, ld);
        }
    }
}

constexpr int kMoeTM = 4;        // 16-row tiles of the BM 64 kernel

template <int DT>
__global__ __launch_bounds__(256) void k_mxfp4_moe_tiled(const Mx4MoeParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nrow = lane & 15, kq = lane >> 4;
    const int tile = blockIdx.x * 4 + wave;
    if (tile * 16 >= p.n) return;                 // the whole wave; the kernel has no barrier
    const Mx4MoeTile w = mx_moe_tile<16 * kMoeTM>(p, blockIdx.y, lane);
    if (w.expert < 0) return;
    const int n = tile * 16 + nrow;
    const int nc = n < p.n ? n : p.n - 1;
    const uint32_t* crow = reinterpret_cast<const uint32_t*>(p.codes + (size_t)w.expert * p.stride_codes + (size_t)nc * (p.k / 2));
    const uint8_t* srow = p.scales + (size_t)w.expert * p.stride_scales + (size_t)nc * p.nb;
    const uint16_t* xrow[kMoeTM];
    bool live[kMoeTM];
    f4 acc[4 * kMoeTM];                           // set s = the sum wave s of the stream kernel keeps
    const int dst = mx_moe_rows<kMoeTM>(p, w, lane, xrow, live);
#pragma unroll
    for (int t = 0; t < 4 * kMoeTM; ++t) acc[t] = (f4){0.f, 0.f, 0.f, 0.f};
    mx_run<DT, kMoeTM, 2, 4>(p, crow, srow, 0, 1, xrow, live, kq, acc);
    const int ld = mx_ld_out(p);
#pragma unroll
    for (int t = 0; t < kMoeTM; ++t) {
        f4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ((acc[t][i] + acc[kMoeTM + t][i]) + acc[2 * kMoeTM + t][i]) + acc[3 * kMoeTM + t][i];
        mx_store_tile<DT>(p, 16 * t, n, kq, v, [&](int r) { return __shfl(dst, r, 64); }, ld);
    }
}

// ---- pairs ----------------------------------------------------------------------------------------------------------------------
constexpr int kPW = 4;           // waves per workgroup; a wave owns weight rows 2 w, 2 w + 1 of the pair's expert

template <int DT>
__global__ __launch_bounds__(kPW * 64) void k_mxfp4_moe_pairs(const Mx4MoeParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = blockIdx.y;
    const int expert = p.ids[j];
    if (expert < 0 || expert >= p.experts) return;
    const int n0 = (blockIdx.x * kPW + wave) * 2;
    if (n0 >= p.n) return;
    const bool two = n0 + 1 < p.n;
    const int n1 = two ? n0 + 1 : n0;
    const uint8_t* codes = p.codes + (size_t)expert * p.stride_codes;
    const uint8_t* scales = p.scales + (size_t)expert * p.stride_scales;
    int src = p.in_div > 0 ? j / p.in_div : j;
    src = src >= p.x_rows ? p.x_rows - 1 : src;
    float acc[2][1] = {{0.f}, {0.f}};
    mx_gemv_run<DT, 1>(p.nb, reinterpret_cast<const uint4*>(codes + (size_t)n0 * (p.k / 2)), reinterpret_cast<const uint4*>(codes + (size_t)n1 * (p.k / 2)),
                       scales + (size_t)n0 * p.nb, scales + (size_t)n1 * p.nb, p.x + (size_t)src * p.ldx, p.ldx, lane, acc);
    acc[0][0] = zl_wave_sum(acc[0][0]);
    acc[1][0] = zl_wave_sum(acc[1][0]);
    if (lane == 0) {
        if (p.epi & ZL_EPI_SILU_MUL) {
            mx_store_gated<DT>(p, j, p.n / 2, n0 / 2, acc[0][0], acc[1][0]);          // n is even: the wave holds the pair
        } else {
            mx_store_plain<DT>(p, j, p.n, n0, acc[0][0]);
            if (two) mx_store_plain<DT>(p, j, p.n, n1, acc[1][0]);
        }
    }
}

int mx_moe_args(Mx4MoeParams& p, const uint16_t* x, int64_t ldx, int64_t x_rows, const uint8_t* codes, const uint8_t* scales, int64_t num_experts,
                int64_t stride_codes, int64_t stride_scales, int64_t pairs, int in_div, uint16_t* y, int64_t n, int64_t k, int dtype, int epilogue) {
    ZL_CHECK_ARG(x && codes && scales && y && x_rows > 0 && n > 0 && k > 0 && num_experts > 0 && pairs >= 0 && in_div >= 0, ZL_EINVAL);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(epilogue == 0 || epilogue == ZL_EPI_SILU_MUL, ZL_EINVAL);
    ZL_CHECK_ARG(k % 32 == 0 && ldx >= k && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)codes & 15) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(!epilogue || n % 2 == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(n < ((int64_t)1 << 31) - 64 && k < ((int64_t)1 << 31) && x_rows < ((int64_t)1 << 31) && num_experts <= 65536, ZL_ELIMIT);
    ZL_CHECK_ARG(stride_codes >= n * (k / 2) && stride_scales >= n * (k / 32) && stride_codes % 16 == 0, ZL_ESHAPE);
    p.x = x; p.ldx = ldx; p.codes = codes; p.scales = scales; p.bias = nullptr; p.residual = nullptr; p.y = y;
    p.m = (int)pairs; p.n = (int)n; p.k = (int)k; p.nb = (int)(k / 32); p.epi = epilogue;
    p.x_rows = (int)x_rows; p.y_rows = (int)pairs;
    p.stride_codes = stride_codes; p.stride_scales = stride_scales; p.experts = (int)num_experts;
    p.loads = nullptr; p.index = nullptr; p.ids = nullptr;
    p.pairs = (int)pairs; p.in_div = in_div; p.out_scatter = 0;
    return ZL_OK;
}

}  // namespace

extern "C" int zl_mxfp4_moe_bm(int64_t pairs, int64_t num_experts) {
    if (pairs <= 0 || num_experts <= 0) return 16;
    // rows per active expert if the pairs spread evenly (at most one expert per pair)
    const int64_t active = pairs < num_experts ? pairs : num_experts;
    const int64_t avg = (pairs + active - 1) / active;
    return avg <= 16 ? 16 : (avg <= 32 ? 32 : 64);
}

extern "C" int zl_mxfp4_moe_grouped(const uint16_t* x, int64_t ldx, int64_t x_rows, const uint8_t* codes, const uint8_t* scales,
                                    int64_t num_experts, int64_t expert_stride_codes, int64_t expert_stride_scales,
                                    const int32_t* expert_loads, const int32_t* index, int64_t pairs, int in_div, int out_scatter,
                                    uint16_t* y, int64_t y_rows, int64_t n, int64_t k, int dtype, int epilogue, zl_stream_t s) {
    Mx4MoeParams p;
    int st = mx_moe_args(p, x, ldx, x_rows, codes, scales, num_experts, expert_stride_codes, expert_stride_scales, pairs, in_div, y, n, k,
                         dtype, epilogue);
    if (st) return st;
    ZL_CHECK_ARG(expert_loads && y_rows > 0, ZL_EINVAL);
    ZL_CHECK_ARG(index || (in_div == 0 && !out_scatter), ZL_EINVAL);
    ZL_CHECK_ARG(pairs < ((int64_t)1 << 24) && y_rows < ((int64_t)1 << 31), ZL_ELIMIT);    // (pairs < 2^24: the work-table scan sums 64
    // clamped loads per round in int32)
    if (pairs == 0) return ZL_OK;
    p.loads = expert_loads; p.index = index; p.out_scatter = out_scatter; p.y_rows = (int)y_rows;
    const int bm = zl_mxfp4_moe_bm(pairs, num_experts);
    const int64_t slots = zl_moe_grouped_tiles(pairs, num_experts, bm);
    ZL_CHECK_ARG(slots <= 65535, ZL_ELIMIT);
    hipStream_t hs = (hipStream_t)s;
    if (bm == 64) {
        const dim3 grid((unsigned)((n + 63) / 64), (unsigned)slots);
        if (dtype == ZL_F16) hipLaunchKernelGGL((k_mxfp4_moe_tiled<ZL_F16>), grid, dim3(256), 0, hs, p);
        else hipLaunchKernelGGL((k_mxfp4_moe_tiled<ZL_BF16>), grid, dim3(256), 0, hs, p);
    } else {
        const dim3 grid((unsigned)((n + 15) / 16), (unsigned)slots);
        if (dtype == ZL_F16) {
            if (bm == 16) hipLaunchKernelGGL((k_mxfp4_moe_stream<ZL_F16, 1>), grid, dim3(256), 0, hs, p);
            else hipLaunchKernelGGL((k_mxfp4_moe_stream<ZL_F16, 2>), grid, dim3(256), 0, hs, p);
        } else {
            if (bm == 16) hipLaunchKernelGGL((k_mxfp4_moe_stream<ZL_BF16, 1>), grid, dim3(256), 0, hs, p);
            else hipLaunchKernelGGL((k_mxfp4_moe_stream<ZL_BF16, 2>), grid, dim3(256), 0, hs, p);
        }
    }
    return zl_launch_status();
}

extern "C" int zl_mxfp4_moe_pairs(const uint16_t* x, int64_t ldx, int64_t x_rows, const uint8_t* codes, const uint8_t* scales,
                                  int64_t num_experts, int64_t expert_stride_codes, int64_t expert_stride_scales, const int32_t* expert_ids,
                                  int64_t pairs, int in_div, uint16_t* y, int64_t n, int64_t k, int dtype, int epilogue, zl_stream_t s) {
    Mx4MoeParams p;
    int st = mx_moe_args(p, x, ldx, x_rows, codes, scales, num_experts, expert_stride_codes, expert_stride_scales, pairs, in_div, y, n, k,
                         dtype, epilogue);
    if (st) return st;
    ZL_CHECK_ARG(expert_ids, ZL_EINVAL);
    ZL_CHECK_ARG(pairs <= 65535, ZL_ELIMIT);
    if (pairs == 0) return ZL_OK;
    p.ids = expert_ids;
    const dim3 grid((unsigned)((n + 2 * kPW - 1) / (2 * kPW)), (unsigned)pairs);
    if (dtype == ZL_F16) hipLaunchKernelGGL((k_mxfp4_moe_pairs<ZL_F16>), grid, dim3(kPW * 64), 0, (hipStream_t)s, p);
    else hipLaunchKernelGGL((k_mxfp4_moe_pairs<ZL_BF16>), grid, dim3(kPW * 64), 0, (hipStream_t)s, p);
    return zl_launch_status();
}
