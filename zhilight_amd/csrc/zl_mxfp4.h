// zl_mxfp4.h -- what the MXFP4 kernels share (mxfp4.hip: fp16 / bf16 activations; mxfp4_a8.hip: MXFP8 activations; mxfp4_a4.hip:
// MXFP4 activations; mxfp4_moe.hip: expert stacks; mxfp4_moe_a8.hip: expert stacks on MXFP8 activations): the launch parameters, the work table of the grouped forms,
// the epilogues of zl_w4a16 (include/zhilight_amd.h) for either T, and the device code of the weight-only kernels -- the E2M1
// decode, the 32-wide MFMA step, the per-lane GEMV walk (mx_gemv_run) and the quad walk of the matrix-core kernels (mx_run).  One
// copy: a kernel that calls them has the numerics stated in mxfp4.hip.
#pragma once
#include "zl_common.h"
#include "zl_w4m_epilogue.h"

struct Mx4Params {
    const uint16_t* x;
    int64_t ldx;
    const uint8_t* codes;
    const uint8_t* scales;
    const uint16_t* bias;
    const uint16_t* residual;
    uint16_t* y;
    int m, n, k, nb, epi;       // nb = k / 32
};

typedef _Float16 mx_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 mx_b8 __attribute__((ext_vector_type(8)));
typedef float mx_f4 __attribute__((ext_vector_type(4)));

// ---- epilogues ---------------------------------------------------------------------------------------------------------------
// v: the fp32 sum of the output in row `row` (>= 0) of y (leading dimension ld), column n
template <int DT>
__device__ __forceinline__ void mx_store_plain(const Mx4Params& p, int row, int ld, int n, float v) {
    if ((p.epi & ZL_EPI_BIAS) && p.bias) v += ZT<DT>::to_f32(p.bias[n]);
    uint16_t o = ZT<DT>::from_f32(v);
    const size_t at = (size_t)(uint32_t)row * (uint32_t)ld + n;
    if (p.epi & ZL_EPI_RESIDUAL) o = ZT<DT>::from_f32(ZT<DT>::to_f32(p.residual[at]) + ZT<DT>::to_f32(o));
    p.y[at] = o;
}
// g, u: the sums of rows 2 j (gate) and 2 j + 1 (up) of the row-interleaved matrix; writes column j of the ld (= n / 2) columns
template <int DT>
__device__ __forceinline__ void mx_store_gated(const Mx4Params& p, int row, int ld, int j, float g, float u) {
    if ((p.epi & ZL_EPI_BIAS) && p.bias) {
        g += ZT<DT>::to_f32(p.bias[2 * j]);
        u += ZT<DT>::to_f32(p.bias[2 * j + 1]);
    }
    g = ZT<DT>::to_f32(ZT<DT>::from_f32(g));
    u = ZT<DT>::to_f32(ZT<DT>::from_f32(u));
    p.y[(size_t)(uint32_t)row * (uint32_t)ld + j] = ZT<DT>::from_f32(silu_f32(g) * u);
}
// the leading dimension of y under p.epi
__device__ __forceinline__ int mx_ld_out(const Mx4Params& p) { return (p.epi & ZL_EPI_SILU_MUL) ? p.n / 2 : p.n; }

// the outputs of one 16 x 16 MFMA tile, lane (nrow = lane % 16, kq = lane / 16): tile rows m0 + 4 kq + i, column n.  rows(r) maps a
// tile row to its row of y (leading dimension ld), < 0: not written; it is called by every lane and may shuffle.  Gated: columns
// pair up across lanes n, n ^ 1 (n even = gate); every lane of the wave must call it
template <int DT, class V, class RowMap>
__device__ __forceinline__ void mx_store_tile(const Mx4Params& p, int m0, int n, int kq, const V& v, RowMap rows, int ld) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = rows(m0 + 4 * kq + i);
        if (p.epi & ZL_EPI_SILU_MUL) {
            const float other = __shfl_xor(v[i], 1, 64);
            if (!(n & 1) && n + 1 < p.n && row >= 0) mx_store_gated<DT>(p, row, ld, n >> 1, v[i], other);
        } else if (n < p.n && row >= 0) {
            mx_store_plain<DT>(p, row, ld, n, v[i]);
        }
    }
}
// ... of a plain linear: tile row r is row r of y (M, N) -- (M, N / 2) gated
template <int DT, class V>
__device__ __forceinline__ void mx_store_tile(const Mx4Params& p, int m0, int n, int kq, const V& v) {
    mx_store_tile<DT>(p, m0, n, kq, v, [&](int r) { return r < p.m ? r : -1; }, mx_ld_out(p));
}

// ---- decode ------------------------------------------------------------------------------------------------------------------
// 2^(e - 127) as fp32; byte 0 is 2^-127, an fp32 subnormal
__device__ __forceinline__ float mx_scale_f32(uint32_t e) { return __builtin_bit_cast(float, e ? e << 23 : 0x00400000u); }

// E2M1 -> T, eight codes of one dword (element 2j in bits 0-3 of byte j, 2j + 1 in bits 4-7) to four packed pairs in
// element order.  |code| indexes an 8-entry byte table through v_perm_b32; the sign bit is moved on top of it.
// fp16: the high byte of the value is the whole value (0x00 0x38 0x3C 0x3E 0x40 0x42 0x44 0x46 = 0 .5 1 1.5 2 3 4 6)
__device__ __forceinline__ void mx_decode8_f16(uint32_t q, uint32_t out[4]) {
    const uint32_t lo = q & 0x07070707u, hi = (q >> 4) & 0x07070707u;
    const uint32_t bl = __builtin_amdgcn_perm(0x46444240u, 0x3E3C3800u, lo) | ((q << 4) & 0x80808080u);   // elements 0 2 4 6
    const uint32_t bh = __builtin_amdgcn_perm(0x46444240u, 0x3E3C3800u, hi) | (q & 0x80808080u);          // elements 1 3 5 7
    out[0] = __builtin_amdgcn_perm(bh, bl, 0x040C000Cu);
    out[1] = __builtin_amdgcn_perm(bh, bl, 0x050C010Cu);
    out[2] = __builtin_amdgcn_perm(bh, bl, 0x060C020Cu);
    out[3] = __builtin_amdgcn_perm(bh, bl, 0x070C030Cu);
}
// bf16: two bytes per value (0 3F00 3F80 3FC0 4000 4040 4080 40C0)
__device__ __forceinline__ void mx_decode8_bf16(uint32_t q, uint32_t out[4]) {
    const uint32_t lo = q & 0x07070707u, hi = (q >> 4) & 0x07070707u;
    const uint32_t hl = __builtin_amdgcn_perm(0x40404040u, 0x3F3F3F00u, lo) | ((q << 4) & 0x80808080u);
    const uint32_t hh = __builtin_amdgcn_perm(0x40404040u, 0x3F3F3F00u, hi) | (q & 0x80808080u);
    const uint32_t ll = __builtin_amdgcn_perm(0xC0804000u, 0xC0800000u, lo);
    const uint32_t lh = __builtin_amdgcn_perm(0xC0804000u, 0xC0800000u, hi);
    const uint32_t e02 = __builtin_amdgcn_perm(hl, ll, 0x05010400u), e46 = __builtin_amdgcn_perm(hl, ll, 0x07030602u);   // (e0, e2), (e4, e6)
    const uint32_t e13 = __builtin_amdgcn_perm(hh, lh, 0x05010400u), e57 = __builtin_amdgcn_perm(hh, lh, 0x07030602u);   // (e1, e3), (e5, e7)
    out[0] = __builtin_amdgcn_perm(e13, e02, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(e13, e02, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(e57, e46, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(e57, e46, 0x07060302u);
}

template <int DT>
__device__ __forceinline__ mx_f4 mx_mfma(uint4 a, uint4 b, mx_f4 c) {
    if constexpr (DT == ZL_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(mx_h8, a), __builtin_bit_cast(mx_h8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mx_b8, a), __builtin_bit_cast(mx_b8, b), c, 0, 0, 0);
}

template <int DT>
__device__ __forceinline__ float mx_x_lo(uint32_t pair) {
    if constexpr (DT == ZL_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(pair & 0xffffu));
    else return __builtin_bit_cast(float, pair << 16);
}
template <int DT>
__device__ __forceinline__ float mx_x_hi(uint32_t pair) {
    if constexpr (DT == ZL_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(pair >> 16));
    else return __builtin_bit_cast(float, pair & 0xffff0000u);
}

// ---- the GEMV walk -----------------------------------------------------------------------------------------------------------
// Two weight rows (their codes c0 / c1 and scale bytes s0 / s1) against the MT activation rows x + m ldx: lane l walks blocks l,
// l + 64, ... of nb; per block 16 B of codes and one scale byte per weight row, the activations' block (64 B per row of x) kept in
// registers for both weight rows, 32 fp32 FMAs per (weight row, activation row), the partial scaled into acc by one more.  The
// weights of the lane's next block are asked for before this one is consumed.  acc[r][m]: the lane's share; the caller sums the wave
template <int DT, int MT>
__device__ __forceinline__ void mx_gemv_run(int nb, const uint4* __restrict__ c0, const uint4* __restrict__ c1,
                                            const uint8_t* __restrict__ s0, const uint8_t* __restrict__ s1,
                                            const uint16_t* __restrict__ x, int64_t ldx, int lane, float (&acc)[2][MT]) {
    uint4 q0n = make_uint4(0, 0, 0, 0), q1n = q0n;
    uint32_t e0n = 0, e1n = 0;
    if (lane < nb) {
        q0n = zl_load_nt(c0 + lane); q1n = zl_load_nt(c1 + lane);
        e0n = s0[lane]; e1n = s1[lane];
    }
#pragma unroll 1
    for (int b = lane; b < nb; b += 64) {
        const uint4 q0 = q0n, q1 = q1n;
        const float f0 = mx_scale_f32(e0n), f1 = mx_scale_f32(e1n);
        if (b + 64 < nb) {
            q0n = zl_load_nt(c0 + b + 64); q1n = zl_load_nt(c1 + b + 64);
            e0n = s0[b + 64]; e1n = s1[b + 64];
        }
        uint4 xv[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)m * ldx + (size_t)b * 32);
#pragma unroll
            for (int t = 0; t < 4; ++t) xv[m][t] = xp[t];
        }
        float part[2][MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) part[0][m] = part[1][m] = 0.f;
        const uint32_t qq[2][4] = {{q0.x, q0.y, q0.z, q0.w}, {q1.x, q1.y, q1.z, q1.w}};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                uint32_t w[4];
                mx_decode8_f16(qq[r][t], w);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const uint32_t xs[4] = {xv[m][t].x, xv[m][t].y, xv[m][t].z, xv[m][t].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float wl = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] & 0xffffu));
                        const float wh = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] >> 16));
                        part[r][m] = __builtin_fmaf(wl, mx_x_lo<DT>(xs[i]), part[r][m]);
                        part[r][m] = __builtin_fmaf(wh, mx_x_hi<DT>(xs[i]), part[r][m]);
                    }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            acc[0][m] = __builtin_fmaf(part[0][m], f0, acc[0][m]);
            acc[1][m] = __builtin_fmaf(part[1][m], f1, acc[1][m]);
        }
    }
}

// ---- the matrix-core walk ----------------------------------------------------------------------------------------------------
// One 32-element block of 16 weight rows against MT x 16 activation rows: lane (nrow = lane % 16, kq = lane / 16) needs codes
// 8 kq .. 8 kq + 7 of row n (one dword) as its B fragment and x[row nrow of the tile][the same k] (16 B) as its A fragment; the
// product lands as D[row 4 kq + i][column nrow], i.e. one weight row and therefore one scale per lane.
// mx_run walks QUADS of four consecutive blocks, q0, q0 + step, ...: lane (nrow, kq) loads the whole block 4 quad + kq of its row
// (16 B: a wave instruction covers 64 contiguous bytes of each of 16 rows), and a 4 x 4 transposition between the four 16-lane
// groups -- v_permlane32_swap on registers (0, 2), (1, 3), then v_permlane16_swap on (0, 1), (2, 3) -- leaves in register b the
// lane's dword of block 4 quad + b: its B fragment.  The operands of the next PF quads are in flight (a ring of PF register slots,
// static indices); blocks past the last one hold zeros, which add an exact 0.  The A fragments come straight from global memory
// through the lane's row pointers xrow[t], which need not be consecutive rows of one matrix (mxfp4_moe.hip: gathered rows).
// NC accumulator sets (1, or a multiple of PF): the i-th quad of the walk adds to set i % NC, each set in walk order -- with NC = 4,
// q0 = 0, step = 1 one wave keeps the four sums that the waves of a 4-way K split (q0 = wave, step = 4, NC = 1) keep one each.
__device__ __forceinline__ void mx_transpose4(uint32_t (&r)[4]) {
    auto s02 = __builtin_amdgcn_permlane32_swap(r[0], r[2], false, false);
    auto s13 = __builtin_amdgcn_permlane32_swap(r[1], r[3], false, false);
    auto t01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
    auto t23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
    r[0] = t01[0]; r[1] = t01[1]; r[2] = t23[0]; r[3] = t23[1];
}

template <int DT, int MT, int PF, int NC = 1>
__device__ __forceinline__ void mx_run(const Mx4Params& p, const uint32_t* __restrict__ crow, const uint8_t* __restrict__ srow, int q0, int step,
                                       const uint16_t* (&xrow)[MT], bool (&live)[MT], int kq, mx_f4 (&acc)[NC * MT]) {
    static_assert(NC == 1 || NC % PF == 0, "the sets take turns on the ring's slots");
    constexpr int U = NC > PF ? NC : PF;        // quads per trip of the loop
    const int nq = (p.nb + 3) >> 2;
    uint4 q[PF];
    uint32_t e[PF][4];
    uint4 a[PF][4][MT];
    auto load = [&](int slot, int quad) {
        q[slot] = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            e[slot][g] = 0;
#pragma unroll
            for (int t = 0; t < MT; ++t) a[slot][g][t] = make_uint4(0, 0, 0, 0);
        }
        if (quad < nq) {
            if (4 * quad + kq < p.nb) q[slot] = zl_load_nt(reinterpret_cast<const uint4*>(crow) + 4 * quad + kq);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int b = 4 * quad + g;
                if (b < p.nb) {
                    e[slot][g] = srow[b];
#pragma unroll
                    for (int t = 0; t < MT; ++t)
                        if (live[t]) a[slot][g][t] = *reinterpret_cast<const uint4*>(xrow[t] + (size_t)b * 32 + kq * 8);
                }
            }
        }
    };
#pragma unroll
    for (int u = 0; u < PF; ++u) load(u, q0 + u * step);
#pragma unroll 1
    for (int quad = q0; quad < nq; quad += U * step) {
#pragma unroll
        for (int c = 0; c < U; ++c) {
            const int u = c % PF, set = (c % NC) * MT;
            uint32_t frag[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
            mx_transpose4(frag);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float f = mx_scale_f32(e[u][g]);
                uint32_t w[4];
                if constexpr (DT == ZL_F16) mx_decode8_f16(frag[g], w);
                else mx_decode8_bf16(frag[g], w);
                const uint4 bf = make_uint4(w[0], w[1], w[2], w[3]);
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    const mx_f4 part = mx_mfma<DT>(a[u][g][t], bf, (mx_f4){0.f, 0.f, 0.f, 0.f});
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[set + t][i] = __builtin_fmaf(part[i], f, acc[set + t][i]);
                }
            }
            load(u, quad + (c + PF) * step);
        }
    }
}

// ---- what the scaled-MFMA kernels share (mxfp4_a8.hip, mxfp4_a4.hip, mxfp4_moe_a8.hip, mxfp4_moe_a4.hip; FP4 x FP4 alone: zl_mxfp4_a4.h) ----
// the four scale bytes of blocks b0 .. b0 + 3 of a row (b0 % 4 == 0); blocks past nb read as 127 (their codes are zeros)
__device__ __forceinline__ uint32_t mx_scale4(const uint8_t* srow, int b0, int nb, bool dwords) {
    if (dwords) return b0 < nb ? *reinterpret_cast<const uint32_t*>(srow + b0) : 0x7f7f7f7fu;
    uint32_t v = 0x7f7f7f7fu;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (b0 + j < nb) v = (v & ~(0xffu << (8 * j))) | ((uint32_t)srow[b0 + j] << (8 * j));
    return v;
}

// ---- what the expert-stack kernels share (mxfp4_moe.hip, mxfp4_moe_a8.hip, mxfp4_moe_a4.hip) ----------------------------------------
struct Mx4MoeParams : Mx4Params {       // x, ldx, y, n, k, nb, epi; codes / scales: expert 0's; bias = residual = nullptr; m unused
    int x_rows, y_rows;
    int64_t stride_codes, stride_scales;  // bytes between experts
    int experts;
    const int32_t* loads;                 // grouped: (experts) rows per expert
    const int32_t* index;                 // grouped: (pairs) sorted position -> pair id
    const int32_t* ids;                   // pairs: (pairs) expert of each pair
    int pairs, in_div, out_scatter;
};

// ---- grouped: which expert / tile slot blockIdx.y is (every wave scans the same loads: uniform over the workgroup, no barrier) -----
struct Mx4MoeTile { int expert, pos0, nvalid; };     // expert < 0: an idle slot of the bound

template <int BM>
__device__ __forceinline__ Mx4MoeTile mx_moe_tile(const Mx4MoeParams& p, int slot, int lane) {
    int f_e = -1, f_t = 0, f_off = 0, f_len = 0;
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
        if (row_base >= p.pairs) break;          // the runs past here start beyond the last pair
    }
    Mx4MoeTile r;
    r.expert = __builtin_amdgcn_readfirstlane(f_e);
    r.pos0 = __builtin_amdgcn_readfirstlane(f_off + f_t * BM);
    int nv = __builtin_amdgcn_readfirstlane(f_len - f_t * BM);
    nv = nv > BM ? BM : nv;
    r.nvalid = nv > p.pairs - r.pos0 ? p.pairs - r.pos0 : nv;
    if (r.nvalid <= 0) r.expert = -1;
    return r;
}
