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
#include "zl_mxfp4.h"

namespace {

typedef mx_f4 f4;

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
    mx_gemv_run<DT, MT>(p.nb, c0, c1, s0, s1, p.x, p.ldx, lane, acc);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        acc[0][m] = zl_wave_sum(acc[0][m]);
        acc[1][m] = zl_wave_sum(acc[1][m]);
    }
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (p.epi & ZL_EPI_SILU_MUL) {
                mx_store_gated<DT>(p, m, p.n / 2, n0 / 2, acc[0][m], acc[1][m]);       // n is even: the wave holds the pair
            } else {
                mx_store_plain<DT>(p, m, p.n, n0, acc[0][m]);
                if (two) mx_store_plain<DT>(p, m, p.n, n1, acc[1][m]);
            }
        }
    }
}

// ---- the matrix-core kernels ----------------------------------------------------------------------------------------------
// (zl_mxfp4.h: mx_run has the fragment maps, the quad walk and the operand ring)
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
