// mxfp4_moe_a8.hip -- the routed feed-forward of MXFP4 mixture-of-experts models on MXFP8 activations (include/zhilight_amd.h
// "MXFP4", EXPERT STACKS ON MXFP8 ACTIVATIONS; opt-in prompt route): ONE launch multiplies every active expert's MXFP4 matrix with
// that expert's routed rows of xq / xs (zl_mxfp8_quantize's codes and scale bytes) on v_mfma_scale_f32_16x16x128_f8f6f4.  The grouped
// form of k_mxfp4_a8 (mxfp4_a8.hip has the instruction's operand map) over the device-side work table of mxfp4_moe.hip.
//
// BIT CONTRACT.  Output row j has the bits zl_mxfp4_a8_linear gives for the same xq / xs row on the same expert's matrix: an MFMA
// output depends on its own A row and B column only, block 16 S + 4 g + j meets lane group g in MFMA step j of super-step S as in
// k_mxfp4_a8, the steps accumulate in the same order and the epilogue is mx_store_tile's.  So a row's bits do not depend on its tile,
// its place in the tile, BM or its company in the batch.
//
// SPLIT.  A workgroup is one (expert, tile of BM sorted rows) slot of the work table (mx_moe_tile) times 256 weight rows of that
// expert: four waves side by side along N, a wave owns BM x 64 outputs as TM x 4 MFMA tiles (TM = BM / 16 = 1, 2, 4; 16 TM fp32
// accumulators per lane).  No K split, no atomics, no host synchronisation; idle slots exit; a wave whose 64 columns lie past N loads
// no weights, multiplies nothing and stores nothing -- it stays for the staging below, which is dealt over all four waves.
//
// B (weights): a lane's 16 contiguous code bytes of one block and the aligned scale dword of a super-step, straight from global
// memory into the operand registers, step t + 1's in flight while step t multiplies (k_mxfp4_a8's walk).  A code byte is used by
// exactly one wave: no LDS.
//
// A (gathered MXFP8 rows): THROUGH LDS, IN FRAGMENT ORDER.  The BM row indices (index[j] / in_div clamped to [0, x_rows), and the
// output row j or index[j], -1 outside [0, y_rows) or past the run) are resolved once per workgroup into LDS.  A super-step's A
// operand is 8 TM fragment pieces of 1 KB: piece ((j TM + tm) 2 + h) holds, for lane l = r + 16 g, the 16 bytes that are half h of
// the lane's A registers in step j on row tile tm -- bytes 16 (g & 1) .. + 15 of block 16 S + j + 4 (g / 2) + 8 h of row 16 tm + r.
// Piece f is staged by wave f % 4: lane l loads ITS OWN 16 bytes of the piece from global memory (a row's 32-byte block by lanes g,
// g ^ 1) at the head of the super-step before, keeps them in 2 TM x 4 VGPRs while that super-step multiplies, and writes them with
// one ds_write_b128 at piece 1024 + 16 l -- a wave writes and later reads whole contiguous KBs: no bank conflicts either way.  The
// four scale bytes a lane feeds through op_sel in the super-step are one dword at [tm][l], staged by wave tm.  Two LDS buffers, ONE
// barrier per super-step: buffer (S + 1) & 1 is written after the multiplies of S, and was last read in S - 1, before the barrier
// that ended it.  Every byte of xq is pulled through the vector cache once per workgroup, not once per wave, and A needs no second
// register buffer across super-steps.  LDS: BM (512 + 16) 2 + 8 BM bytes = 17 / 34 / 68 KB.
// Blocks past K / 32 are zero codes under scale byte 127 in registers (exact zeros); rows past the run read row 0 and are not stored.
#include "zl_mxfp4.h"

namespace {

typedef int i8v __attribute__((ext_vector_type(8)));
typedef mx_f4 f4;

struct Mx4MoeA8Params : Mx4MoeParams {  // x = nullptr, ldx = 0: the activations are
    const uint8_t* xq;                    // (x_rows, k) E4M3 codes
    const uint8_t* xs;                    // (x_rows, nb) E8M0 scale bytes
};

constexpr int kTN = 4;                    // 16-column tiles per wave
constexpr int kCols = 4 * 16 * kTN;       // weight rows per workgroup

template <int TM>
struct Mx4MoeA8Frag {
    i8v a[TM];
    uint4 b[kTN];
};

// MFMA step J of a super-step: the TM x 4 tiles of the wave, scale byte J of the super-step's dwords (cbsz 0: A = E4M3, blgp 4: B = E2M1)
template <int J, int TM>
__device__ __forceinline__ void mx_moe_a8_step(const Mx4MoeA8Frag<TM>& f, const uint32_t (&sa)[TM], const uint32_t (&sb)[kTN], f4 (&acc)[TM][kTN]) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < kTN; ++tn) {
            const i8v bv = {(int)f.b[tn].x, (int)f.b[tn].y, (int)f.b[tn].z, (int)f.b[tn].w, 0, 0, 0, 0};
            acc[tm][tn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(f.a[tm], bv, acc[tm][tn], 0, 4, J, (int)sa[tm], J, (int)sb[tn]);
        }
}

// BM 16 / 32 fit 256 registers without scratch: two workgroups per CU cover each other's barriers; BM 64 takes the CU alone
template <int DT, int TM>
__global__ __launch_bounds__(256, TM == 4 ? 1 : 2) void k_mxfp4_moe_a8(const Mx4MoeA8Params p) {
    constexpr int BM = 16 * TM, PIECES = 8 * TM, MINE = PIECES / 4;      // a wave stages MINE pieces per super-step
    constexpr int NT = TM == 4 ? 2 : 1;                                  // ... of NT row tiles
    __shared__ uint4 lds_a[2][PIECES][64];
    __shared__ uint32_t lds_s[2][TM][64];
    __shared__ int lds_src[BM], lds_dst[BM];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const Mx4MoeTile w = mx_moe_tile<BM>(p, blockIdx.y, lane);
    if (w.expert < 0) return;                                            // the whole workgroup, before any barrier
    const int n0 = (int)blockIdx.x * kCols + wave * (16 * kTN);
    const bool active = n0 < p.n;                                        // wave-uniform
    const bool dwords = (p.nb & 3) == 0;

    if (threadIdx.x < BM) {
        const int lr = threadIdx.x;
        int src = 0, dst = -1;
        if (lr < w.nvalid) {
            const int j = w.pos0 + lr;
            src = p.in_div > 0 ? p.index[j] / p.in_div : j;
            src = src < 0 ? 0 : (src >= p.x_rows ? p.x_rows - 1 : src);
            dst = p.out_scatter ? p.index[j] : j;
            if (dst < 0 || dst >= p.y_rows) dst = -1;
        }
        lds_src[lr] = src;
        lds_dst[lr] = dst;
    }
    __syncthreads();

    // staging: piece f = wave + 4 i = ((j TM + tm) 2 + h), so h = wave & 1 and j TM + tm = wave / 2 + 2 i; the wave's row tiles are
    // tm_u = (wave / 2 + 2 u) % TM, u < NT, piece i being of tile u = i % NT
    const int h8 = 8 * (wave & 1), ga = 4 * (g >> 1), half = 16 * (g & 1);
    const uint8_t* arow[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) arow[u] = p.xq + (size_t)lds_src[16 * (((wave >> 1) + 2 * u) % TM) + r16] * p.k;
    const uint8_t* asrow = p.xs + (size_t)lds_src[16 * (wave % TM) + r16] * p.nb;    // wave tm < TM stages the scales of tile tm
    uint4 st[MINE];
    uint32_t sts = 0;
    auto stage_load = [&](int s0) {                                      // global -> registers: super-step of blocks s0 .. s0 + 15
#pragma unroll
        for (int i = 0; i < MINE; ++i) {
            const int blk = s0 + ((wave >> 1) + 2 * i) / TM + ga + h8;
            st[i] = make_uint4(0, 0, 0, 0);
            if (blk < p.nb) st[i] = *reinterpret_cast<const uint4*>(arow[i % NT] + (size_t)blk * 32 + half);
        }
        if (wave < TM) sts = mx_scale4(asrow, s0 + 4 * g, p.nb, dwords);
    };
    auto stage_store = [&](int buf) {                                    // registers -> LDS
#pragma unroll
        for (int i = 0; i < MINE; ++i) lds_a[buf][wave + 4 * i][lane] = st[i];
        if (wave < TM) lds_s[buf][wave][lane] = sts;
    };

    const uint8_t* brow[kTN];
    const uint8_t* bsrow[kTN];
#pragma unroll
    for (int t = 0; t < kTN; ++t) {
        const int col = min(n0 + 16 * t + r16, p.n - 1);                 // an idle wave's pointers are never used
        brow[t] = p.codes + (size_t)w.expert * p.stride_codes + (size_t)col * (p.k / 2);
        bsrow[t] = p.scales + (size_t)w.expert * p.stride_scales + (size_t)col * p.nb;
    }
    f4 acc[TM][kTN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < kTN; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};

    Mx4MoeA8Frag<TM> buf[2];
    auto load_b = [&](Mx4MoeA8Frag<TM>& f, int sj) {                     // the lane's B of the step on blocks sj + 4 b: block sj + 4 g
        const int bb = sj + 4 * g;
#pragma unroll
        for (int t = 0; t < kTN; ++t) {
            f.b[t] = make_uint4(0, 0, 0, 0);
            if (bb < p.nb) f.b[t] = *reinterpret_cast<const uint4*>(brow[t] + (size_t)bb * 16);
        }
    };
    auto load_a = [&](Mx4MoeA8Frag<TM>& f, int cur, int j) {             // the lane's A of step j: its two pieces per row tile
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const uint4 a0 = lds_a[cur][(j * TM + tm) * 2][lane], a1 = lds_a[cur][(j * TM + tm) * 2 + 1][lane];
            f.a[tm] = (i8v){(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
        }
    };
    uint32_t sa[TM], sb[kTN], sbn[kTN];
    stage_load(0);
    stage_store(0);
    if (active) {
#pragma unroll
        for (int t = 0; t < kTN; ++t) sb[t] = mx_scale4(bsrow[t], 4 * g, p.nb, dwords);
        load_b(buf[0], 0);
    }
    __syncthreads();
#pragma unroll 1
    for (int s0 = 0; s0 < p.nb; s0 += 16) {                              // one super-step: blocks s0 .. s0 + 15
        const int cur = (s0 >> 4) & 1;
        const bool more = s0 + 16 < p.nb;                                // uniform over the workgroup
        if (more) stage_load(s0 + 16);
        if (active) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) sa[tm] = lds_s[cur][tm][lane];
#pragma unroll
            for (int t = 0; t < kTN; ++t) sbn[t] = mx_scale4(bsrow[t], s0 + 16 + 4 * g, p.nb, dwords);
            load_a(buf[0], cur, 0);
            load_a(buf[1], cur, 1); load_b(buf[1], s0 + 1); mx_moe_a8_step<0, TM>(buf[0], sa, sb, acc);
            load_a(buf[0], cur, 2); load_b(buf[0], s0 + 2); mx_moe_a8_step<1, TM>(buf[1], sa, sb, acc);
            load_a(buf[1], cur, 3); load_b(buf[1], s0 + 3); mx_moe_a8_step<2, TM>(buf[0], sa, sb, acc);
            load_b(buf[0], s0 + 16); mx_moe_a8_step<3, TM>(buf[1], sa, sb, acc);
#pragma unroll
            for (int t = 0; t < kTN; ++t) sb[t] = sbn[t];
        }
        if (more) stage_store(cur ^ 1);
        __syncthreads();
    }
    if (!active) return;
    const int ld = mx_ld_out(p);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < kTN; ++tn)
            mx_store_tile<DT>(p, 16 * tm, n0 + 16 * tn + r16, g, acc[tm][tn], [&](int r) { return lds_dst[r]; }, ld);
}

template <int DT>
void mx_moe_a8_launch(const Mx4MoeA8Params& p, int bm, const dim3& grid, hipStream_t hs) {
    if (bm == 16) hipLaunchKernelGGL((k_mxfp4_moe_a8<DT, 1>), grid, dim3(256), 0, hs, p);
    else if (bm == 32) hipLaunchKernelGGL((k_mxfp4_moe_a8<DT, 2>), grid, dim3(256), 0, hs, p);
    else hipLaunchKernelGGL((k_mxfp4_moe_a8<DT, 4>), grid, dim3(256), 0, hs, p);
}

}  // namespace

extern "C" int zl_mxfp4_moe_a8_bm(int64_t pairs, int64_t num_experts) {
    if (pairs <= 0 || num_experts <= 0) return 16;
    // rows per active expert if the pairs spread evenly (at most one expert per pair)
    const int64_t active = pairs < num_experts ? pairs : num_experts;
    const int64_t avg = (pairs + active - 1) / active;
    return avg <= 16 ? 16 : (avg <= 32 ? 32 : 64);
}

extern "C" int zl_mxfp4_moe_a8_grouped(const uint8_t* xq, const uint8_t* xs, int64_t x_rows, const uint8_t* codes, const uint8_t* scales,
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
    Mx4MoeA8Params p;
    p.x = nullptr; p.ldx = 0; p.codes = codes; p.scales = scales; p.bias = nullptr; p.residual = nullptr; p.y = y;
    p.m = (int)pairs; p.n = (int)n; p.k = (int)k; p.nb = (int)(k / 32); p.epi = epilogue;
    p.x_rows = (int)x_rows; p.y_rows = (int)y_rows;
    p.stride_codes = expert_stride_codes; p.stride_scales = expert_stride_scales; p.experts = (int)num_experts;
    p.loads = expert_loads; p.index = index; p.ids = nullptr;
    p.pairs = (int)pairs; p.in_div = in_div; p.out_scatter = out_scatter;
    p.xq = xq; p.xs = xs;
    const int bm = zl_mxfp4_moe_a8_bm(pairs, num_experts);
    const int64_t slots = zl_moe_grouped_tiles(pairs, num_experts, bm);
    ZL_CHECK_ARG(slots <= 65535, ZL_ELIMIT);
    const dim3 grid((unsigned)((n + kCols - 1) / kCols), (unsigned)slots);
    if (dtype == ZL_F16) mx_moe_a8_launch<ZL_F16>(p, bm, grid, (hipStream_t)s);
    else mx_moe_a8_launch<ZL_BF16>(p, bm, grid, (hipStream_t)s);
    return zl_launch_status();
}
