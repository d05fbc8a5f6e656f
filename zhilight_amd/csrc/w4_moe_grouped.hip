// w4_moe_grouped.hip -- expert-grouped W4A16 GEMM of the MoE feed-forward for more than a few rows (prompts, decode batches).
//
// Reference: MOEImpl::forward (src/nn/feedforward/feedforward.cpp:698-790) above GPTQ_MOE_M_THRES rows: route, sort the
// (token, slot) pairs by expert, one Int4GPTQ linear per active expert over that expert's rows, then sum_experts.  Those
// linears take gptq_gemm_k_major's M > 40 branch (q_gemm_k_major.cu:1083-1100): W16 = rn16(rn16(q - z) * s), exact products,
// fp32 accumulation, one rounding to half.  Here ONE launch runs the GEMMs of every active expert: the fused decode GEMVs
// (w4_moe.hip) stream an expert's weights once per (token, expert) pair, this kernel once per 16..128-row tile of the expert's
// rows.
//
// Work table: the pairs are sorted by expert, so expert e owns the run [off_e, off_e + load_e) of sorted positions
// (off = exclusive prefix sum of load over e' < e).  Each run is cut into BM-row tiles; blockIdx.y enumerates the tiles of all
// experts in expert order.  Every workgroup derives its (expert, run, tile) from the device-side loads in a wave-wide scan at
// its start (E / 64 rounds of one load and two prefix sums), so the table lives on the device and the host only sizes the grid
// from the bound ceil(P / BM) + min(E, P) tiles; slots past the last tile exit.  No host synchronisation anywhere.
//
// Rows: sorted position j reads activation row index[j] / in_div (in_div = 0: row j) and writes output row j (out_scatter = 0)
// or index[j] (out_scatter = 1): gate|up gathers the tokens of its pairs, down writes the (token, slot) rows that sum_experts
// reads.  Indices are clamped to the activation rows, and output rows outside [0, y_rows) are not written.
//
// Tile: the inner structure of k_w4a16_gemm_tiled (w4_gemm_tiled.hip) on the same ZLW4M operands, one matrix per expert
// `stride` bytes apart: workgroup = 4 waves = BM x 128 outputs, wave = BM x 32 (two 16-row weight tiles), 128-k chunks, the
// gathered activation chunk double-buffered in LDS with padded rows (register staging: a 16-lane group loads one row's 256 B,
// no piece crosses a row), the weight items on an 8-slot ring of non-temporal buffer loads, v_mfma_f32_16x16x32_f16.  The
// k order of every output is the tiled kernel's (chunks in order, the four 32-k steps of a chunk in order, no K split), so
// the result is bit-identical to zl_w4a16_gemm_tiled run on each expert's gathered rows.
#include "zl_common.h"
#include "zl_w4m_dequant.h"
#include "zl_w4m_epilogue.h"

namespace {

constexpr int kWavesG = 4;
constexpr int kThreadsG = kWavesG * 64;
constexpr int kBNG = kWavesG * 32;
constexpr int kRingG = 8;          // items (2 per chunk)
constexpr int kRowHalfsG = 128 + 8; // padded LDS row

typedef float f4 __attribute__((ext_vector_type(4)));

struct GroupedParams {
    const uint16_t* x;
    int64_t ldx;
    int x_rows;
    const unsigned char* qw;          // expert 0's ZLW4M words; expert e at qw + e * stride_qw
    const unsigned char* meta;
    int64_t stride_qw, stride_meta;   // bytes
    uint32_t qw_bytes, meta_bytes;    // one expert's matrix
    int experts;
    const int32_t* loads;             // (experts) rows per expert
    const int32_t* index;             // (pairs) sorted position -> pair id
    const int32_t* ids;               // PAIRS: (pairs) expert of each pair
    int pairs, in_div, out_scatter;
    uint16_t* y;
    int y_rows, ld_out;
    int n, groups, tiles;             // tiles = ceil(n / 16) (padded weight rows)
    int epi;
};


// PAIRS: the small-M form (rows <= GPTQ_MOE_M_THRES in the driver) -- no sort and no work table: blockIdx.y = (token, slot) pair j,
// expert ids[j] (outside the stack: dropped), one valid row x[j / in_div] (in_div = 0: x[j]), output row j.  Each output is the same
// sum over K in the same order as in the sorted form, so both forms give the same bits.
template <int BM, bool PAIRS>
__global__ __launch_bounds__(kThreadsG, 2) void k_w4a16_gemm_grouped(const GroupedParams p) {
    constexpr int RB = BM / 16;               // 16-row blocks of the M tile
    constexpr int XR = BM / 16;               // uint4 per thread per x chunk (16 threads x 16 B per row)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_g[];
    uint16_t (*xs)[BM * kRowHalfsG] = reinterpret_cast<uint16_t (*)[BM * kRowHalfsG]>(smem_g);   // [2][BM * kRowHalfsG]
    int* dst_rows = reinterpret_cast<int*>(smem_g + (size_t)2 * BM * kRowHalfsG * 2);          // [BM] output row or -1

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nrow = lane & 15, kq = lane >> 4;

    // ---- work table: which expert / tile this slot is (every wave scans the same loads: no barrier needed)
    const int slot = blockIdx.y;
    int f_e = -1, f_t = 0, f_off = 0, f_len = 0;
    if (PAIRS) {
        const int e = p.ids[slot];
        if (e >= 0 && e < p.experts) { f_e = e; f_off = slot; f_len = 1; }
    } else {
        int tile_base = 0, row_base = 0;
        for (int c = 0; c < p.experts; c += 64) {
            const int e = c + lane;
            int l = e < p.experts ? p.loads[e] : 0;
            l = l < 0 ? 0 : (l > p.pairs ? p.pairs : l);
            const int t = (l + BM - 1) / BM;
            int ti = t, li = l;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int a = __shfl_up(ti, d, 64), b = __shfl_up(li, d, 64);
                if (lane >= d) { ti += a; li += b; }
            }
            const int t_ex = tile_base + ti - t, l_ex = row_base + li - l;
            const unsigned long long hit = __ballot(slot >= t_ex && slot < t_ex + t);
            if (hit) {
                const int src = __builtin_ctzll(hit);
                f_e = __shfl(e, src, 64);
                f_t = slot - __shfl(t_ex, src, 64);
                f_off = __shfl(l_ex, src, 64);
                f_len = __shfl(l, src, 64);
                break;
            }
            tile_base += __shfl(ti, 63, 64);
            row_base += __shfl(li, 63, 64);
            if (row_base >= p.pairs) break;      // the runs past here start beyond the last pair
        }
    }
    const int expert = __builtin_amdgcn_readfirstlane(f_e);
    if (expert < 0) return;                   // an idle slot of the bound
    const int pos0 = __builtin_amdgcn_readfirstlane(f_off + f_t * BM);
    int nvalid = __builtin_amdgcn_readfirstlane(f_len - f_t * BM);
    nvalid = nvalid > BM ? BM : nvalid;
    nvalid = nvalid > p.pairs - pos0 ? p.pairs - pos0 : nvalid;
    if (nvalid <= 0) return;

    const int tile0 = blockIdx.x * (kBNG / 16) + wave * 2;   // this wave's two 16-row weight tiles
    const int G = p.groups;

    // ---- weight ring of this expert's matrix: item (j, g) = tile (tile0 + j), chunk g
    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(p.qw + (size_t)expert * p.stride_qw), 0, p.qw_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(p.meta + (size_t)expert * p.stride_meta), 0, p.meta_bytes, 0x00020000);
    const uint32_t q_off = (uint32_t)lane * 16u, m_off = (uint32_t)nrow * 4u;
    const int t0c = tile0 < p.tiles ? tile0 : p.tiles - 1, t1c = tile0 + 1 < p.tiles ? tile0 + 1 : p.tiles - 1;
    const uint32_t base0 = (uint32_t)t0c * (uint32_t)p.groups, base1 = (uint32_t)t1c * (uint32_t)p.groups;
    uint4 wq[kRingG];
    uint32_t mt[kRingG];
    int iss_g = 0;
    auto issue_pair = [&](int slot0) {
        const uint32_t g = (uint32_t)(iss_g < G ? iss_g : G - 1);
        const uint32_t it0 = base0 + g, it1 = base1 + g;
        wq[slot0] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rq, q_off, it0 * 1024u, 2));
        mt[slot0] = __builtin_amdgcn_raw_buffer_load_b32(rm, m_off, it0 * 64u, 2);
        wq[slot0 + 1] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rq, q_off, it1 * 1024u, 2));
        mt[slot0 + 1] = __builtin_amdgcn_raw_buffer_load_b32(rm, m_off, it1 * 64u, 2);
        ++iss_g;
    };

    // ---- gathered activation rows: thread -> (tile row tid / 16 + 16 r, 16-byte column tid % 16)
    const int xrow = threadIdx.x >> 4, xcol = (threadIdx.x & 15) * 8;
    const uint16_t* xsrc[XR];
#pragma unroll
    for (int r = 0; r < XR; ++r) {
        const int lr = xrow + 16 * r;
        int src = 0;
        if (lr < nvalid) {
            const int j = pos0 + lr;
            src = p.in_div > 0 ? (PAIRS ? j : p.index[j]) / p.in_div : j;
            src = src < 0 ? 0 : (src >= p.x_rows ? p.x_rows - 1 : src);
        }
        xsrc[r] = lr < nvalid ? p.x + (size_t)src * p.ldx + xcol : nullptr;
    }
    if (threadIdx.x < BM) {
        int d = -1;
        if ((int)threadIdx.x < nvalid) {
            const int j = pos0 + threadIdx.x;
            d = (!PAIRS && p.out_scatter) ? p.index[j] : j;
            if (d < 0 || d >= p.y_rows) d = -1;
        }
        dst_rows[threadIdx.x] = d;
    }
    uint4 xr[XR];
    auto load_x = [&](int g) {
        const int gc = g < G ? g : G - 1;
#pragma unroll
        for (int r = 0; r < XR; ++r)
            xr[r] = xsrc[r] ? *reinterpret_cast<const uint4*>(xsrc[r] + (size_t)gc * 128) : make_uint4(0, 0, 0, 0);
    };
    auto store_x = [&](int buf) {
#pragma unroll
        for (int r = 0; r < XR; ++r)
            *reinterpret_cast<uint4*>(&xs[buf][(xrow + 16 * r) * kRowHalfsG + xcol]) = xr[r];
    };

    load_x(0);
#pragma unroll
    for (int s = 0; s < kRingG; s += 2) {
        issue_pair(s);
        __builtin_amdgcn_sched_barrier(0);
    }
    store_x(0);
    load_x(1);
    __syncthreads();

    const uint32_t mask_lo = __builtin_amdgcn_readfirstlane(0x000f000fu);
    const uint32_t mask_hi = __builtin_amdgcn_readfirstlane(0x00f000f0u);
    uint32_t magic = 0x64006400u;
    asm volatile("" : "+v"(magic));
    const hv2 c960 = {(_Float16)960.f, (_Float16)960.f};

    f4 acc[RB][2];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        acc[rb][0] = (f4){0.f, 0.f, 0.f, 0.f};
        acc[rb][1] = (f4){0.f, 0.f, 0.f, 0.f};
    }

    auto chunk = [&](int slot0, int buf) {
        h8 bfr[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t mw = mt[slot0 + j];
            const hv2 z1 = __builtin_bit_cast(hv2, __builtin_amdgcn_perm(mw, mw, 0x03020302u));
            const hv2 z16 = z1 + c960;
            const hv2 s2 = __builtin_bit_cast(hv2, __builtin_amdgcn_perm(mw, mw, 0x01000100u));
            const uint32_t wds[4] = {wq[slot0 + j].x, wq[slot0 + j].y, wq[slot0 + j].z, wq[slot0 + j].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) bfr[j][t] = zl_w4m_dequant8(wds[t], z1, z16, s2, mask_lo, mask_hi, magic);
        }
        issue_pair(slot0);
        const uint16_t* xb = &xs[buf][nrow * kRowHalfsG + kq * 8];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const h8 a = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(xb + rb * 16 * kRowHalfsG + t * 32));
                acc[rb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bfr[0][t], acc[rb][0], 0, 0, 0);
                acc[rb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bfr[1][t], acc[rb][1], 0, 0, 0);
            }
        }
    };

    // ---- main loop: 4 chunks per turn of the ring (static slot indices)
#pragma unroll 1
    for (int g = 0; g < G; g += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (g + u < G) {                  // workgroup-uniform
                chunk(2 * u, u & 1);
                store_x((u + 1) & 1);         // chunk g+u+1 (loaded one step ago) -> the other buffer
                load_x(g + u + 2);
                __syncthreads();
            }
        }
    }

    // ---- epilogue: C fragment = column n (lane & 15), rows 4 kq + i of each 16-row block
    const bool silu = (p.epi & (ZL_EPI_SILU_MUL | ZL_EPI_SILU_MUL_F32)) != 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = (tile0 + j) * 16 + nrow;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int lr = rb * 16 + 4 * kq + i;
                const int row = dst_rows[lr];
                const float v = acc[rb][j][i];
                if (!silu) {
                    if (row >= 0 && n < p.n) p.y[(size_t)row * p.ld_out + n] = __builtin_bit_cast(uint16_t, zl_f32_to_f16(v));
                } else {
                    // rows of the packed matrix interleave gate (even n) and up (odd n): partner = lane ^ 1
                    const float other = __shfl_xor(v, 1, 64);
                    if ((nrow & 1) == 0 && row >= 0 && n + 1 < p.n) {
                        p.y[(size_t)row * p.ld_out + n / 2] = __builtin_bit_cast(uint16_t, zl_f32_to_f16(zl_w4m_finish_gated(v, other, p.epi)));
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" int zl_moe_grouped_bm(int64_t pairs, int64_t num_experts) {
    if (pairs <= 0 || num_experts <= 0) return 16;
    // rows per active expert if the pairs spread evenly (at most one expert per pair)
    const int64_t active = pairs < num_experts ? pairs : num_experts;
    const int64_t avg = (pairs + active - 1) / active;
    return avg <= 16 ? 16 : (avg <= 32 ? 32 : (avg < 128 ? 64 : 128));
}

extern "C" int64_t zl_moe_grouped_tiles(int64_t pairs, int64_t num_experts, int64_t bm) {
    if (pairs <= 0 || num_experts <= 0 || bm <= 0) return 0;
    // sum over experts of ceil(load_e / bm) <= floor(pairs / bm) + (experts with a row): at most min(E, pairs) runs end in a
    // partial tile
    const int64_t active = pairs < num_experts ? pairs : num_experts;
    return pairs / bm + active;
}

extern "C" int zl_w4a16_gemm_grouped(const uint16_t* x, int64_t ldx, int64_t x_rows, const uint32_t* qw, const uint32_t* meta,
                                     int64_t num_experts, int64_t expert_stride_qw, int64_t expert_stride_meta,
                                     const int32_t* expert_loads, const int32_t* index, int64_t pairs, int in_div, int out_scatter,
                                     uint16_t* y, int64_t y_rows, int64_t n, int64_t k, int64_t group_size, int epilogue,
                                     zl_stream_t s) {
    ZL_CHECK_ARG(x && qw && meta && expert_loads && y && x_rows > 0 && y_rows > 0 && n > 0 && k > 0 && num_experts > 0 &&
                 pairs >= 0 && in_div >= 0, ZL_EINVAL);
    ZL_CHECK_ARG(index || (in_div == 0 && !out_scatter), ZL_EINVAL);
    ZL_CHECK_ARG(epilogue == 0 || epilogue == ZL_EPI_SILU_MUL || epilogue == ZL_EPI_SILU_MUL_F32, ZL_EINVAL);
    ZL_CHECK_ARG(ldx >= k && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && k % 128 == 0, ZL_ESHAPE);
    const bool silu = epilogue != 0;
    ZL_CHECK_ARG(!silu || n % 2 == 0, ZL_ESHAPE);
    zl_w4_layout_t L;
    int st = zl_w4m_layout(n, k, group_size, &L);
    if (st) return st;
    ZL_CHECK_ARG(expert_stride_qw >= L.qw_bytes && expert_stride_meta >= L.scales_bytes && expert_stride_qw % 16 == 0 &&
                 expert_stride_meta % 4 == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(L.qw_bytes < ((int64_t)1 << 32) && pairs < ((int64_t)1 << 24) && x_rows < ((int64_t)1 << 31) &&
                 y_rows < ((int64_t)1 << 31) && num_experts <= 65536, ZL_ELIMIT);   // (pairs < 2^24: the
    // work-table scan sums 64 clamped loads per round in int32)
    if (pairs == 0) return ZL_OK;
    const int bm = zl_moe_grouped_bm(pairs, num_experts);
    const int64_t slots = zl_moe_grouped_tiles(pairs, num_experts, bm);
    ZL_CHECK_ARG(slots <= 65535, ZL_ELIMIT);
    GroupedParams p;
    p.x = x; p.ldx = ldx; p.x_rows = (int)x_rows;
    p.qw = reinterpret_cast<const unsigned char*>(qw);
    p.meta = reinterpret_cast<const unsigned char*>(meta);
    p.stride_qw = expert_stride_qw; p.stride_meta = expert_stride_meta;
    p.qw_bytes = (uint32_t)L.qw_bytes; p.meta_bytes = (uint32_t)L.scales_bytes;
    p.experts = (int)num_experts;
    p.loads = expert_loads; p.index = index; p.ids = nullptr;
    p.pairs = (int)pairs; p.in_div = in_div; p.out_scatter = out_scatter;
    p.y = y; p.y_rows = (int)y_rows;
    p.ld_out = (int)(silu ? n / 2 : n);
    p.n = (int)n; p.groups = (int)(k / 128); p.tiles = (int)(L.np / 16);
    p.epi = epilogue;
    const dim3 grid((unsigned)((L.np + kBNG - 1) / kBNG), (unsigned)slots);
    const size_t lds = (size_t)2 * bm * kRowHalfsG * 2 + (size_t)bm * sizeof(int);
    hipStream_t hs = (hipStream_t)s;
#define ZL_GROUPED_LAUNCH(BMV)                                                                                  \
    {                                                                                                           \
        if (lds > 64 * 1024) {                                                                                  \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_w4a16_gemm_grouped<BMV, false>),       \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);           \
            if (e != hipSuccess) return ZL_ELIMIT;                                                              \
        }                                                                                                       \
        hipLaunchKernelGGL((k_w4a16_gemm_grouped<BMV, false>), grid, dim3(kThreadsG), lds, hs, p);                       \
    }
    if (bm == 16) ZL_GROUPED_LAUNCH(16)
    else if (bm == 32) ZL_GROUPED_LAUNCH(32)
    else if (bm == 64) ZL_GROUPED_LAUNCH(64)
    else ZL_GROUPED_LAUNCH(128)
#undef ZL_GROUPED_LAUNCH
    return zl_launch_status();
}

extern "C" int zl_w4a16_gemm_pairs(const uint16_t* x, int64_t ldx, int64_t x_rows, const uint32_t* qw, const uint32_t* meta,
                                   int64_t num_experts, int64_t expert_stride_qw, int64_t expert_stride_meta, const int32_t* expert_ids,
                                   int64_t pairs, int in_div, uint16_t* y, int64_t n, int64_t k, int64_t group_size, int epilogue,
                                   zl_stream_t s) {
    ZL_CHECK_ARG(x && qw && meta && expert_ids && y && x_rows > 0 && n > 0 && k > 0 && num_experts > 0 && pairs >= 0 && in_div >= 0,
                 ZL_EINVAL);
    ZL_CHECK_ARG(epilogue == 0 || epilogue == ZL_EPI_SILU_MUL || epilogue == ZL_EPI_SILU_MUL_F32, ZL_EINVAL);
    ZL_CHECK_ARG(ldx >= k && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && k % 128 == 0, ZL_ESHAPE);
    const bool silu = epilogue != 0;
    ZL_CHECK_ARG(!silu || n % 2 == 0, ZL_ESHAPE);
    zl_w4_layout_t L;
    int st = zl_w4m_layout(n, k, group_size, &L);
    if (st) return st;
    ZL_CHECK_ARG(expert_stride_qw >= L.qw_bytes && expert_stride_meta >= L.scales_bytes && expert_stride_qw % 16 == 0 &&
                 expert_stride_meta % 4 == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(L.qw_bytes < ((int64_t)1 << 32) && pairs <= 65535 && x_rows < ((int64_t)1 << 31) && num_experts <= 65536, ZL_ELIMIT);
    if (pairs == 0) return ZL_OK;
    GroupedParams p;
    p.x = x; p.ldx = ldx; p.x_rows = (int)x_rows;
    p.qw = reinterpret_cast<const unsigned char*>(qw);
    p.meta = reinterpret_cast<const unsigned char*>(meta);
    p.stride_qw = expert_stride_qw; p.stride_meta = expert_stride_meta;
    p.qw_bytes = (uint32_t)L.qw_bytes; p.meta_bytes = (uint32_t)L.scales_bytes;
    p.experts = (int)num_experts;
    p.loads = nullptr; p.index = nullptr; p.ids = expert_ids;
    p.pairs = (int)pairs; p.in_div = in_div; p.out_scatter = 0;
    p.y = y; p.y_rows = (int)pairs;
    p.ld_out = (int)(silu ? n / 2 : n);
    p.n = (int)n; p.groups = (int)(k / 128); p.tiles = (int)(L.np / 16);
    p.epi = epilogue;
    const dim3 grid((unsigned)((L.np + kBNG - 1) / kBNG), (unsigned)pairs);
    const size_t lds = (size_t)2 * 16 * kRowHalfsG * 2 + (size_t)16 * sizeof(int);
    hipLaunchKernelGGL((k_w4a16_gemm_grouped<16, true>), grid, dim3(kThreadsG), lds, (hipStream_t)s, p);
    return zl_launch_status();
}
