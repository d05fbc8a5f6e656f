// mxfp4_moe_a4.hip -- the routed feed-forward of MXFP4 mixture-of-experts models on MXFP4 activations, W4A4 (include/zhilight_amd.h
// "MXFP4", EXPERT STACKS ON MXFP4 ACTIVATIONS; opt-in prompt route): ONE launch multiplies every active expert's MXFP4 matrix with
// that expert's routed rows of xq / xs (zl_mxfp4_act_quantize's codes and scale bytes) on the FP4 x FP4 form of
// v_mfma_scale_f32_16x16x128_f8f6f4.  The grouped form of k_mxfp4_a4 (mxfp4_a4.hip has the instruction's operand map: the A
// operand MIRRORS B, one MX block of 16 bytes per lane) over the device-side work table of mxfp4_moe.hip (mx_moe_tile).
//
// BIT CONTRACT.  Output row j has the bits zl_mxfp4_a4_linear gives for the same xq / xs row on the same expert's matrix: an MFMA
// output depends on its own A row and B column only, block 16 S + 4 g + j meets lane group g in MFMA step j of super-step S as in
// k_mxfp4_a4 -- the step is ONE piece of code, mx_a4_step (zl_mxfp4_a4.h) -- every super-step runs its four steps in order (blocks
// past K / 32 add exact zeros there and here), and the epilogue is mx_store_tile's.  So a row's bits do not depend on its tile, its
// place in the tile, BM or its company in the batch.
//
// SPLIT.  A workgroup is one (expert, tile of BM = 16 TM sorted rows) slot of the work table times 256 weight rows of that expert:
// four waves side by side along N, a wave owns BM x 64 outputs as TM x 4 MFMA tiles (TM = 1, 2, 4; 16 TM fp32 accumulators per
// lane).  No K split, no atomics, no host synchronisation; idle slots exit before any barrier; a wave whose 64 columns lie past N
// loads no weights, multiplies nothing and stores nothing -- it stays for the staging below and the barriers.  All three heights
// hold TWO waves per SIMD (__launch_bounds__(256, 2)) without scratch: the 4-register operands make the room at BM 64 that the
// 8-register E4M3 operand of k_mxfp4_moe_a8 does not leave (DESIGN 4 has the resource table).
//
// K is walked in SUPER-STEPS of 16 blocks, K / 32 % 4 a template argument (DW: a row's four scale bytes of a super-step are one
// aligned dword for op_sel = j; otherwise mx_scale4 gathers them byte by byte).
// B (weights): a lane's 16 code bytes of a step and the scale dword of a super-step straight from global memory into the operand
// registers through the expert's base pointer (codes + e * expert_stride_codes); k_mxfp4_a4's RING OF FOUR register slots, slot j =
// step j of a super-step, filled THREE steps ahead.  A code byte is used by exactly one wave: no LDS.
// A (gathered MXFP4 rows): THROUGH LDS, IN FRAGMENT ORDER, once per workgroup.  The BM row indices (index[j] / in_div clamped to
// [0, x_rows), and the output row j or index[j], -1 outside [0, y_rows) or past the run) are resolved once into LDS.  A super-step's
// A operand is 4 TM pieces of 1 KB: piece f = j TM + tm holds at 16 l the operand of lane l = r + 16 g in step j on row tile tm --
// the 16 bytes of block 16 S + 4 g + j of row 16 tm + r.  Piece f is staged by wave f % 4, so with TM < 4 no wave idles in the
// staging: wave w stages the TM pieces w + 4 i, all of row tile w % TM (one row pointer per lane), of steps (w + 4 i) / TM.  A lane
// loads ITS OWN 16 bytes of each piece through its gathered row pointer at the head of the super-step before, keeps them in 4 TM
// VGPRs while that super-step multiplies and writes them with ds_write_b128 after its MFMAs; a step reads its TM pieces with
// ds_read_b128 one step ahead, row tile by row tile, into the second of two A register buffers -- whole contiguous KBs either way,
// no bank conflicts.  The scale dwords of tile tm go the same way, staged by wave tm.  Two LDS buffers, ONE barrier per super-step:
// buffer (S + 1) & 1 is written after the multiplies of S and was last read in S - 1, before the barrier that ended it.
// LDS: 2 (4 TM 1024 + TM 256) + 8 BM bytes = 8.6 / 17.2 / 34.5 KB.  There is no direct-load form of A to compare against: unmeasured.
// ZERO BLOCKS AND CLAMPED ROWS: k_mxfp4_a4's rules (zl_mxfp4_a4.h) -- every global load of the K walk is unconditional, a block past
// K / 32 selects the ADDRESS of a zero block under scale byte 127 and reads exact zeros; the source-order pin follows each row
// tile's MFMAs.  Rows past the run read a clamped row and are not stored.
#include "zl_mxfp4_a4.h"

namespace {

typedef mx_f4 f4;

struct Mx4MoeA4Params : Mx4MoeParams {  // x = nullptr, ldx = 0: the activations are
    const uint8_t* xq;                    // (x_rows, k / 2) E2M1 codes
    const uint8_t* xs;                    // (x_rows, nb) E8M0 scale bytes
};

constexpr int kCols = 4 * 16 * kA4TN;     // weight rows per workgroup

template <int DT, int TM, bool DW>
__global__ __launch_bounds__(256, 2) void k_mxfp4_moe_a4(const Mx4MoeA4Params p) {
    constexpr int BM = 16 * TM, PIECES = 4 * TM;                         // a wave stages TM of the PIECES per super-step
    __shared__ uint4 lds_a[2][PIECES][64];                               // [buffer][step j * TM + row tile][lane]
    __shared__ uint32_t lds_s[2][TM][64];                                // [buffer][row tile][lane]
    __shared__ int lds_src[BM], lds_dst[BM];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const Mx4MoeTile w = mx_moe_tile<BM>(p, blockIdx.y, lane);
    if (w.expert < 0) return;                                            // the whole workgroup, before any barrier
    const int n0 = (int)blockIdx.x * kCols + wave * (16 * kA4TN);
    const bool active = n0 < p.n;                                        // wave-uniform; an idle wave still stages

    if (threadIdx.x < BM) {
        const int lr = threadIdx.x;
        int src = 0, dst = -1;
        if (lr < w.nvalid) {
            const int j = w.pos0 + lr;
            src = p.in_div > 0 ? p.index[j] / p.in_div : j;
            dst = p.out_scatter ? p.index[j] : j;
            if (dst < 0 || dst >= p.y_rows) dst = -1;
        }
        lds_src[lr] = src < 0 ? 0 : (src >= p.x_rows ? p.x_rows - 1 : src);
        lds_dst[lr] = dst;
    }
    __syncthreads();

    // staging: piece f = wave + 4 i = j TM + tm, so tm = wave % TM for every i (4 % TM == 0) and j = (wave + 4 i) / TM
    const int srow = lds_src[16 * (wave % TM) + r16];
    const uint8_t* arow = p.xq + (size_t)srow * (p.k / 2);
    const uint8_t* asrow = p.xs + (size_t)srow * p.nb;                   // wave tm < TM stages the scales of tile tm (= wave % TM)
    uint4 st[TM];
    uint32_t sts;
    auto stage_load = [&](int s0) {                                      // global -> registers: the wave's pieces of blocks s0 .. s0 + 15
#pragma unroll
        for (int i = 0; i < TM; ++i) st[i] = mx_a4_block<true>(arow, s0 + 4 * g + (wave + 4 * i) / TM, p.nb);
        sts = mx_a4_scale4<DW>(asrow, s0 + 4 * g, p.nb);                // by every wave: a load under `wave < TM` would cost the wait counts
    };
    auto stage_store = [&](int buf) {                                    // registers -> LDS
#pragma unroll
        for (int i = 0; i < TM; ++i) lds_a[buf][wave + 4 * i][lane] = st[i];
        if (wave < TM) lds_s[buf][wave][lane] = sts;
    };

    const uint8_t* brow[kA4TN];
    const uint8_t* bsrow[kA4TN];
#pragma unroll
    for (int t = 0; t < kA4TN; ++t) {
        const int col = min(n0 + 16 * t + r16, p.n - 1);                 // an idle wave's pointers are never used
        brow[t] = p.codes + (size_t)w.expert * p.stride_codes + (size_t)col * (p.k / 2);
        bsrow[t] = p.scales + (size_t)w.expert * p.stride_scales + (size_t)col * p.nb;
    }
    f4 acc[TM][kA4TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < kA4TN; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};

    // B: the ring of four register slots, slot j = step j of a super-step, filled THREE steps ahead.  A: two register buffers, step j
    // reads a[j & 1] and refills the other row tile by row tile.
    uint4 a[2][TM], b[4][kA4TN];
    uint32_t sa[TM], sb[kA4TN], sbn[kA4TN];
    auto load_b = [&](auto guard, uint4 (&f)[kA4TN], int sj) {           // the lane's B of the step on blocks sj + 4 b: block sj + 4 g
#pragma unroll
        for (int t = 0; t < kA4TN; ++t) f[t] = mx_a4_block<decltype(guard)::value>(brow[t], sj + 4 * g, p.nb);
    };
    stage_load(0);
    stage_store(0);
    if (active) {
#pragma unroll
        for (int t = 0; t < kA4TN; ++t) sb[t] = mx_a4_scale4<DW>(bsrow[t], 4 * g, p.nb);
        load_b(std::true_type(), b[0], 0);
        load_b(std::true_type(), b[1], 1);
        load_b(std::true_type(), b[2], 2);
    }
    __syncthreads();
    // one super-step, blocks s0 .. s0 + 15; FULL: all 16 exist, so only what is asked for the NEXT super-step needs the guard
    auto super_step = [&](auto full, int s0) {
        const int cur = (s0 >> 4) & 1;
        stage_load(s0 + 16);                                             // past the end: the zero block, never read back
        if (active) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
                sa[tm] = lds_s[cur][tm][lane];
                a[0][tm] = lds_a[cur][tm][lane];                         // step 0's pieces
            }
#pragma unroll
            for (int t = 0; t < kA4TN; ++t) sbn[t] = mx_a4_scale4<DW>(bsrow[t], s0 + 16 + 4 * g, p.nb);
            auto piece = [&](int j) { return [&, j](int tm) { a[j & 1][tm] = lds_a[cur][j * TM + tm][lane]; }; };
            load_b(std::integral_constant<bool, !decltype(full)::value>(), b[3], s0 + 3);
            mx_a4_step<0>(a[0], b[0], sa, sb, acc, piece(1));
            load_b(std::true_type(), b[0], s0 + 16);
            mx_a4_step<1>(a[1], b[1], sa, sb, acc, piece(2));
            load_b(std::true_type(), b[1], s0 + 17);
            mx_a4_step<2>(a[0], b[2], sa, sb, acc, piece(3));
            load_b(std::true_type(), b[2], s0 + 18);
            mx_a4_step<3>(a[1], b[3], sa, sb, acc, [](int) {});
#pragma unroll
            for (int t = 0; t < kA4TN; ++t) sb[t] = sbn[t];
            // in both arms, as in k_mxfp4_a4: behind the join the wait for st would be vmcnt(0), the B ring's loads included
            stage_store(cur ^ 1);
            asm volatile("" : : : "memory");
        } else {
            stage_store(cur ^ 1);
        }
        __syncthreads();
    };
    int s0 = 0;
#pragma unroll 1
    for (; s0 + 16 <= p.nb; s0 += 16) super_step(std::true_type(), s0);
    if (s0 < p.nb) super_step(std::false_type(), s0);
    if (!active) return;
    const int ld = mx_ld_out(p);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < kA4TN; ++tn)
            mx_store_tile<DT>(p, 16 * tm, n0 + 16 * tn + r16, g, acc[tm][tn], [&](int r) { return lds_dst[r]; }, ld);
}

template <int DT, bool DW>
void mx_moe_a4_launch(const Mx4MoeA4Params& p, int bm, const dim3& grid, hipStream_t hs) {
    if (bm == 16) hipLaunchKernelGGL((k_mxfp4_moe_a4<DT, 1, DW>), grid, dim3(256), 0, hs, p);
    else if (bm == 32) hipLaunchKernelGGL((k_mxfp4_moe_a4<DT, 2, DW>), grid, dim3(256), 0, hs, p);
    else hipLaunchKernelGGL((k_mxfp4_moe_a4<DT, 4, DW>), grid, dim3(256), 0, hs, p);
}

}  // namespace

extern "C" int zl_mxfp4_moe_a4_bm(int64_t pairs, int64_t num_experts) {
    if (pairs <= 0 || num_experts <= 0) return 16;
    // rows per active expert if the pairs spread evenly (at most one expert per pair)
    const int64_t active = pairs < num_experts ? pairs : num_experts;
    const int64_t avg = (pairs + active - 1) / active;
    return avg <= 16 ? 16 : (avg <= 32 ? 32 : 64);
}

extern "C" int zl_mxfp4_moe_a4_grouped(const uint8_t* xq, const uint8_t* xs, int64_t x_rows, const uint8_t* codes, const uint8_t* scales,
                                       int64_t num_experts, int64_t expert_stride_codes, int64_t expert_stride_scales,
                                       const int32_t* expert_loads, const int32_t* index, int64_t pairs, int in_div, int out_scatter,
                                       uint16_t* y, int64_t y_rows, int64_t n, int64_t k, int dtype, int epilogue, zl_stream_t s) {
    ZL_CHECK_ARG(xq && xs && codes && scales && y && x_rows > 0 && n > 0 && k > 0 && num_experts > 0 && pairs >= 0 && in_div >= 0, ZL_EINVAL);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(epilogue == 0 || epilogue == ZL_EPI_SILU_MUL, ZL_EINVAL);
    ZL_CHECK_ARG(k % 32 == 0 && ((uintptr_t)xq & 15) == 0 && ((uintptr_t)codes & 15) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(!epilogue || n % 2 == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(n < ((int64_t)1 << 31) - kCols && k < ((int64_t)1 << 31) && x_rows < ((int64_t)1 << 31) && num_experts <= 65536, ZL_ELIMIT);
    ZL_CHECK_ARG(expert_stride_codes >= n * (k / 2) && expert_stride_scales >= n * (k / 32) && expert_stride_codes % 16 == 0, ZL_ESHAPE);
    // the scale rows read as dwords: every row of xs and of every expert's scales starts on a dword
    ZL_CHECK_ARG((k / 32) % 4 != 0 || (((((uintptr_t)xs) | ((uintptr_t)scales)) & 3) == 0 && expert_stride_scales % 4 == 0), ZL_ESHAPE);
    ZL_CHECK_ARG(expert_loads && y_rows > 0, ZL_EINVAL);
    ZL_CHECK_ARG(index || (in_div == 0 && !out_scatter), ZL_EINVAL);
    ZL_CHECK_ARG(pairs < ((int64_t)1 << 24) && y_rows < ((int64_t)1 << 31), ZL_ELIMIT);    // (pairs < 2^24: the work-table scan sums 64
    // clamped loads per round in int32)
    if (pairs == 0) return ZL_OK;
    Mx4MoeA4Params p;
    p.x = nullptr; p.ldx = 0; p.codes = codes; p.scales = scales; p.bias = nullptr; p.residual = nullptr; p.y = y;
    p.m = (int)pairs; p.n = (int)n; p.k = (int)k; p.nb = (int)(k / 32); p.epi = epilogue;
    p.x_rows = (int)x_rows; p.y_rows = (int)y_rows;
    p.stride_codes = expert_stride_codes; p.stride_scales = expert_stride_scales; p.experts = (int)num_experts;
    p.loads = expert_loads; p.index = index; p.ids = nullptr;
    p.pairs = (int)pairs; p.in_div = in_div; p.out_scatter = out_scatter;
    p.xq = xq; p.xs = xs;
    const int bm = zl_mxfp4_moe_a4_bm(pairs, num_experts);
    const int64_t slots = zl_moe_grouped_tiles(pairs, num_experts, bm);
    ZL_CHECK_ARG(slots <= 65535, ZL_ELIMIT);
    const dim3 grid((unsigned)((n + kCols - 1) / kCols), (unsigned)slots);
    const hipStream_t hs = (hipStream_t)s;
    if (p.nb % 4 == 0) {
        if (dtype == ZL_F16) mx_moe_a4_launch<ZL_F16, true>(p, bm, grid, hs);
        else mx_moe_a4_launch<ZL_BF16, true>(p, bm, grid, hs);
    } else {
        if (dtype == ZL_F16) mx_moe_a4_launch<ZL_F16, false>(p, bm, grid, hs);
        else mx_moe_a4_launch<ZL_BF16, false>(p, bm, grid, hs);
    }
    return zl_launch_status();
}
