// mxfp4.hip -- linears on OCP MXFP4 weights (E2M1 codes, one E8M0 scale per 32 elements; include/zhilight_amd.h "MXFP4"):
// y = T(x . W^T [+ bias]) for T = fp16 / bf16, fp32 accumulation, the bias / residual / silu*mul epilogues of the W4A16 family.
//
// The kernels read the CHECKPOINT layout (codes (N, K/2), scales (N, K/32)): a row's 32-element block is 16 contiguous bytes,
// which is one lane's 16-byte load in the GEMV and, after a 4 x 4 register transposition between lane groups, the four lanes' dwords
// of an MFMA B fragment, so there is no packed copy.
//
// NUMERICS: a weight is never rounded.  An E2M1 value (0, 0.5 .. 6) is exact in fp16 AND bf16; every kernel multiplies the
// UNSCALED code values with the activations (exact products, fp32 sums), finishes the block's 32-term partial sum and scales that
// by 2^(e - 127) in fp32 -- a power of two, exact -- before it joins the accumulator.  So one path serves both types and every
// scale byte 0..254; there is no fp16 scale range to leave.  v_mfma_f32_16x16x32_{f16,bf16} has K = 32 = one MX block, which is
// what makes the per-block scaling free of any regrouping on the matrix cores.
//
// Routes (zl_mxfp4_route):
//   1..4 rows   k_mxfp4_gemv   a wave owns two weight rows, lane l walks blocks l, l + 64, ...: 16 B of codes + 1 scale byte per
//                              block and row, the activations' block (64 B per row of x) kept in registers for both weight rows
//   5..32 rows  k_mxfp4_stream one workgroup per 16 weight rows, its 4 waves split K by quads of four blocks (quad j -> wave j % 4)
//                              and fold through LDS: the weight is read once, in 16-byte loads that a register transposition between
//                              the lane groups turns into MFMA B fragments; 16 / 32 activation rows as A fragments
//   > 32 rows   k_mxfp4_tiled  64 x 64 outputs per workgroup (a wave: 64 rows x 16 columns), no K split; weights re-read per
//                              64-row slice of x (prompt chunks)
#include "zl_common.h"
#include "zl_w4m_epilogue.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

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

// 2^(e - 127) as fp32; byte 0 is 2^-127, an fp32 subnormal
__device__ __forceinline__ float mx_scale_f32(uint32_t e) { return __builtin_bit_cast(float, e ? e << 23 : 0x00400000u); }

// ---- E2M1 -> T, eight codes of one dword (element 2j in bits 0-3 of byte j, 2j + 1 in bits 4-7) to four packed pairs in
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
__device__ __forceinline__ f4 mx_mfma(uint4 a, uint4 b, f4 c) {
    if constexpr (DT == ZL_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
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

// ---- the epilogues of zl_w4a16 (include/zhilight_amd.h) for either T.  v: the fp32 sum of output (m, n)
template <int DT>
__device__ __forceinline__ void mx_store_plain(const Mx4Params& p, int m, int n, float v) {
    if ((p.epi & ZL_EPI_BIAS) && p.bias) v += ZT<DT>::to_f32(p.bias[n]);
    uint16_t o = ZT<DT>::from_f32(v);
    const size_t at = (size_t)m * p.n + n;
    if (p.epi & ZL_EPI_RESIDUAL) o = ZT<DT>::from_f32(ZT<DT>::to_f32(p.residual[at]) + ZT<DT>::to_f32(o));
    p.y[at] = o;
}
// g, u: the sums of rows 2 j (gate) and 2 j + 1 (up) of the row-interleaved matrix; writes column j of n / 2
template <int DT>
__device__ __forceinline__ void mx_store_gated(const Mx4Params& p, int m, int j, float g, float u) {
    if ((p.epi & ZL_EPI_BIAS) && p.bias) {
        g += ZT<DT>::to_f32(p.bias[2 * j]);
        u += ZT<DT>::to_f32(p.bias[2 * j + 1]);
    }
    g = ZT<DT>::to_f32(ZT<DT>::from_f32(g));
    u = ZT<DT>::to_f32(ZT<DT>::from_f32(u));
    p.y[(size_t)m * (p.n / 2) + j] = ZT<DT>::from_f32(silu_f32(g) * u);
}

// ---- 1..4 rows ------------------------------------------------------------------------------------------------------------
constexpr int kGW = 4;          // waves per workgroup; a wave owns weight rows 2 w, 2 w + 1

template <int DT, int MT>
__global__ __launch_bounds__(kGW * 64) void k_mxfp4_gemv(const Mx4Params p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n0 = (blockIdx.x * kGW + wave) * 2;
    if (n0 >= p.n) return;
    const bool two = n0 + 1 < p.n;
    const int n1 = two ? n0 + 1 : n0;
    const uint4* c0 = reinterpret_cast<const uint4*>(p.codes + (size_t)n0 * (p.k / 2));
    const uint4* c1 = reinterpret_cast<const uint4*>(p.codes + (size_t)n1 * (p.k / 2));
    const uint8_t* s0 = p.scales + (size_t)n0 * p.nb;
    const uint8_t* s1 = p.scales + (size_t)n1 * p.nb;

    float acc[2][MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[0][m] = acc[1][m] = 0.f;

    // the weights of the lane's next block are asked for before this one is consumed
    uint4 q0n = make_uint4(0, 0, 0, 0), q1n = q0n;
    uint32_t e0n = 0, e1n = 0;
    if (lane < p.nb) {
        q0n = zl_load_nt(c0 + lane); q1n = zl_load_nt(c1 + lane);
        e0n = s0[lane]; e1n = s1[lane];
    }
#pragma unroll 1
    for (int b = lane; b < p.nb; b += 64) {
        const uint4 q0 = q0n, q1 = q1n;
        const float f0 = mx_scale_f32(e0n), f1 = mx_scale_f32(e1n);
        if (b + 64 < p.nb) {
            q0n = zl_load_nt(c0 + b + 64); q1n = zl_load_nt(c1 + b + 64);
            e0n = s0[b + 64]; e1n = s1[b + 64];
        }
        uint4 xv[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const uint4* xp = reinterpret_cast<const uint4*>(p.x + (size_t)m * p.ldx + (size_t)b * 32);
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
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        acc[0][m] = zl_wave_sum(acc[0][m]);
        acc[1][m] = zl_wave_sum(acc[1][m]);
    }
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (p.epi & ZL_EPI_SILU_MUL) {
                mx_store_gated<DT>(p, m, n0 / 2, acc[0][m], acc[1][m]);       // n is even: the wave holds the pair
            } else {
                mx_store_plain<DT>(p, m, n0, acc[0][m]);
                if (two) mx_store_plain<DT>(p, m, n1, acc[1][m]);
            }
        }
    }
}

// ---- the matrix-core kernels ----------------------------------------------------------------------------------------------
// One 32-element block of 16 weight rows against MT x 16 activation rows: lane (nrow = lane % 16, kq = lane / 16) needs codes
// 8 kq .. 8 kq + 7 of row n (one dword) as its B fragment and x[row nrow of the tile][the same k] (16 B) as its A fragment; the
// product lands as D[row 4 kq + i][column nrow], i.e. one weight row and therefore one scale per lane.
// mx_run walks QUADS of four consecutive blocks, q0, q0 + step, ...: lane (nrow, kq) loads the whole block 4 quad + kq of its row
// (16 B: a wave instruction covers 64 contiguous bytes of each of 16 rows), and a 4 x 4 transposition between the four 16-lane
// groups -- v_permlane32_swap on registers (0, 2), (1, 3), then v_permlane16_swap on (0, 1), (2, 3) -- leaves in register b the
// lane's dword of block 4 quad + b: its B fragment.  The operands of the next PF quads are in flight (a ring of PF register slots,
// static indices); blocks past the last one hold zeros, which add an exact 0.
__device__ __forceinline__ void mx_transpose4(uint32_t (&r)[4]) {
    auto s02 = __builtin_amdgcn_permlane32_swap(r[0], r[2], false, false);
    auto s13 = __builtin_amdgcn_permlane32_swap(r[1], r[3], false, false);
    auto t01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
    auto t23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
    r[0] = t01[0]; r[1] = t01[1]; r[2] = t23[0]; r[3] = t23[1];
}

template <int DT, int MT, int PF>
__device__ __forceinline__ void mx_run(const Mx4Params& p, const uint32_t* __restrict__ crow, const uint8_t* __restrict__ srow, int q0, int step,
                                       const uint16_t* (&xrow)[MT], bool (&live)[MT], int kq, f4 (&acc)[MT]) {
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
    for (int quad = q0; quad < nq; quad += PF * step) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
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
                    const f4 part = mx_mfma<DT>(a[u][g][t], bf, (f4){0.f, 0.f, 0.f, 0.f});
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[t][i] = __builtin_fmaf(part[i], f, acc[t][i]);
                }
            }
            load(u, quad + (u + PF) * step);
        }
    }
}

// the outputs of one 16 x 16 tile: rows m0 + 4 kq + i, column n.  Gated: columns pair up across lanes n, n ^ 1 (n even = gate)
template <int DT>
__device__ __forceinline__ void mx_store_tile(const Mx4Params& p, int m0, int n, int kq, const f4& v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = m0 + 4 * kq + i;
        if (p.epi & ZL_EPI_SILU_MUL) {
            const float other = __shfl_xor(v[i], 1, 64);
            if (!(n & 1) && n + 1 < p.n && row < p.m) mx_store_gated<DT>(p, row, n >> 1, v[i], other);
        } else if (n < p.n && row < p.m) {
            mx_store_plain<DT>(p, row, n, v[i]);
        }
    }
}

template <int DT, int MT>
__global__ __launch_bounds__(256) void k_mxfp4_stream(const Mx4Params p) {
    __shared__ float red[3][MT * 4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nrow = lane & 15, kq = lane >> 4;
    const int n = blockIdx.x * 16 + nrow;
    const int nc = n < p.n ? n : p.n - 1;
    const uint32_t* crow = reinterpret_cast<const uint32_t*>(p.codes + (size_t)nc * (p.k / 2));
    const uint8_t* srow = p.scales + (size_t)nc * p.nb;
    const uint16_t* xrow[MT];
    bool live[MT];
    f4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int row = 16 * t + nrow;
        live[t] = row < p.m;
        xrow[t] = p.x + (size_t)(live[t] ? row : 0) * p.ldx;
        acc[t] = (f4){0.f, 0.f, 0.f, 0.f};
    }
    mx_run<DT, MT, 2>(p, crow, srow, wave, 4, xrow, live, kq, acc);

    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[wave - 1][t * 4 + i][lane] = acc[t][i];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][i] = ((acc[t][i] + red[0][t * 4 + i][lane]) + red[1][t * 4 + i][lane]) + red[2][t * 4 + i][lane];
            mx_store_tile<DT>(p, 16 * t, n, kq, acc[t]);
        }
    }
}

constexpr int kTM = 4;          // 16-row activation tiles per wave of the tiled kernel: 64 rows

template <int DT>
__global__ __launch_bounds__(256) void k_mxfp4_tiled(const Mx4Params p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nrow = lane & 15, kq = lane >> 4;
    const int tile = blockIdx.x * 4 + wave;
    if (tile * 16 >= p.n) return;
    const int n = tile * 16 + nrow;
    const int nc = n < p.n ? n : p.n - 1;
    const int m0 = blockIdx.y * (16 * kTM);
    const uint32_t* crow = reinterpret_cast<const uint32_t*>(p.codes + (size_t)nc * (p.k / 2));
    const uint8_t* srow = p.scales + (size_t)nc * p.nb;
    const uint16_t* xrow[kTM];
    bool live[kTM];
    f4 acc[kTM];
#pragma unroll
    for (int t = 0; t < kTM; ++t) {
        const int row = m0 + 16 * t + nrow;
        live[t] = row < p.m;
        xrow[t] = p.x + (size_t)(live[t] ? row : 0) * p.ldx;
        acc[t] = (f4){0.f, 0.f, 0.f, 0.f};
    }
    mx_run<DT, kTM, 2>(p, crow, srow, 0, 1, xrow, live, kq, acc);
#pragma unroll
    for (int t = 0; t < kTM; ++t) mx_store_tile<DT>(p, m0 + 16 * t, n, kq, acc[t]);
}

// ---- dequantise (tests, debugging): W[n, k] = T(value(code) * 2^(e - 127)), one rounding.  The fp32 value is put together from
// integers, so scale bytes that land in fp32's subnormals (0, 1) are exact whatever the float mode
__device__ __forceinline__ float mx_value_f32(uint32_t code, uint32_t e) {
    const uint32_t mag = code & 7u;
    if (mag == 0) return 0.f;                                                     // code 8 (-0) is 0
    // |value| = (1 + frac / 2) * 2^ex: 0.5 = 2^-1; codes 2.. : ex = mag / 2 - 1, frac = mag & 1
    const int ex = mag == 1 ? -1 : (int)(mag >> 1) - 1;
    const uint32_t frac = mag == 1 ? 0u : (mag & 1u);
    const int field = ex + (int)e;                                               // biased fp32 exponent: ex + (e - 127) + 127
    uint32_t bits;
    if (field >= 255) bits = 0x7f800000u;                                        // 6 * 2^127 and its like: past fp32, an infinity of T
    else if (field >= 1) bits = ((uint32_t)field << 23) | (frac << 22);
    else bits = (0x00800000u | (frac << 22)) >> (1 - field);                     // field is 0 or -1: nothing is shifted out
    return __builtin_bit_cast(float, bits | ((code & 8u) << 28));
}

template <int DT>
__global__ __launch_bounds__(256) void k_mxfp4_dequant(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                                       uint16_t* __restrict__ out, int64_t bytes, int k2) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= bytes) return;
    const int64_t row = at / k2;
    const int col = (int)(at - row * k2);
    const uint32_t c = codes[at], e = scales[row * (k2 / 16) + col / 16];
    const uint32_t lo = ZT<DT>::from_f32(mx_value_f32(c & 15u, e)), hi = ZT<DT>::from_f32(mx_value_f32(c >> 4, e));
    reinterpret_cast<uint32_t*>(out)[at] = lo | (hi << 16);
}

}  // namespace

extern "C" int zl_mxfp4_route(int64_t m, int64_t n, int64_t k) {
    ZL_CHECK_ARG(m > 0 && n > 0 && k > 0, ZL_EINVAL);
    ZL_CHECK_ARG(k % 32 == 0, ZL_ESHAPE);
    return m <= 4 ? ZL_MXFP4_GEMV : (m <= 32 ? ZL_MXFP4_STREAM : ZL_MXFP4_TILED);
}

extern "C" int zl_mxfp4_linear(const uint16_t* x, int64_t ldx, const uint8_t* codes, const uint8_t* scales, const uint16_t* bias,
                               const uint16_t* residual, uint16_t* y, int64_t m, int64_t n, int64_t k, int dtype, int epilogue,
                               zl_stream_t s) {
    ZL_CHECK_ARG(x && codes && scales && y && m > 0 && n > 0 && k > 0, ZL_EINVAL);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(k % 32 == 0 && ldx >= k && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)codes & 15) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG((epilogue & ~(ZL_EPI_BIAS | ZL_EPI_RESIDUAL | ZL_EPI_SILU_MUL)) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(!((epilogue & ZL_EPI_SILU_MUL) && ((epilogue & ZL_EPI_RESIDUAL) || n % 2 != 0)), ZL_ESHAPE);
    ZL_CHECK_ARG(!((epilogue & ZL_EPI_RESIDUAL) && !residual) && !((epilogue & ZL_EPI_BIAS) && !bias), ZL_EINVAL);
    ZL_CHECK_ARG(n < ((int64_t)1 << 31) - 64 && k < ((int64_t)1 << 31) && m < ((int64_t)1 << 31) - 64, ZL_ELIMIT);
    Mx4Params p;
    p.x = x; p.ldx = ldx; p.codes = codes; p.scales = scales; p.bias = bias; p.residual = residual; p.y = y;
    p.m = (int)m; p.n = (int)n; p.k = (int)k; p.nb = (int)(k / 32); p.epi = epilogue;
    hipStream_t hs = (hipStream_t)s;
    const int route = zl_mxfp4_route(m, n, k);
    if (route == ZL_MXFP4_GEMV) {
        const dim3 grid((unsigned)((n + 2 * kGW - 1) / (2 * kGW)));
#define ZL_MXG(DT)                                                                                        \
        switch (m) {                                                                                      \
            case 1: hipLaunchKernelGGL((k_mxfp4_gemv<DT, 1>), grid, dim3(kGW * 64), 0, hs, p); break;     \
            case 2: hipLaunchKernelGGL((k_mxfp4_gemv<DT, 2>), grid, dim3(kGW * 64), 0, hs, p); break;     \
            case 3: hipLaunchKernelGGL((k_mxfp4_gemv<DT, 3>), grid, dim3(kGW * 64), 0, hs, p); break;     \
            default: hipLaunchKernelGGL((k_mxfp4_gemv<DT, 4>), grid, dim3(kGW * 64), 0, hs, p); break;    \
        }
        if (dtype == ZL_F16) { ZL_MXG(ZL_F16) } else { ZL_MXG(ZL_BF16) }
#undef ZL_MXG
    } else if (route == ZL_MXFP4_STREAM) {
        const dim3 grid((unsigned)((n + 15) / 16));
        if (dtype == ZL_F16) {
            if (m <= 16) hipLaunchKernelGGL((k_mxfp4_stream<ZL_F16, 1>), grid, dim3(256), 0, hs, p);
            else hipLaunchKernelGGL((k_mxfp4_stream<ZL_F16, 2>), grid, dim3(256), 0, hs, p);
        } else {
            if (m <= 16) hipLaunchKernelGGL((k_mxfp4_stream<ZL_BF16, 1>), grid, dim3(256), 0, hs, p);
            else hipLaunchKernelGGL((k_mxfp4_stream<ZL_BF16, 2>), grid, dim3(256), 0, hs, p);
        }
    } else {
        const int64_t gy = (m + 16 * kTM - 1) / (16 * kTM);
        ZL_CHECK_ARG(gy <= 65535, ZL_ELIMIT);
        const dim3 grid((unsigned)((n + 63) / 64), (unsigned)gy);
        if (dtype == ZL_F16) hipLaunchKernelGGL((k_mxfp4_tiled<ZL_F16>), grid, dim3(256), 0, hs, p);
        else hipLaunchKernelGGL((k_mxfp4_tiled<ZL_BF16>), grid, dim3(256), 0, hs, p);
    }
    return zl_launch_status();
}

extern "C" int zl_mxfp4_dequant(const uint8_t* codes, const uint8_t* scales, uint16_t* out, int64_t n, int64_t k, int dtype,
                                zl_stream_t s) {
    ZL_CHECK_ARG(codes && scales && out && n > 0 && k > 0, ZL_EINVAL);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(k % 32 == 0 && ((uintptr_t)out & 3) == 0 && k < ((int64_t)1 << 31), ZL_ESHAPE);
    const int64_t bytes = n * (k / 2);
    ZL_CHECK_ARG((bytes + 255) / 256 < ((int64_t)1 << 31), ZL_ELIMIT);
    const dim3 grid((unsigned)((bytes + 255) / 256));
    if (dtype == ZL_F16) hipLaunchKernelGGL((k_mxfp4_dequant<ZL_F16>), grid, dim3(256), 0, (hipStream_t)s, codes, scales, out, bytes, (int)(k / 2));
    else hipLaunchKernelGGL((k_mxfp4_dequant<ZL_BF16>), grid, dim3(256), 0, (hipStream_t)s, codes, scales, out, bytes, (int)(k / 2));
    return zl_launch_status();
}
