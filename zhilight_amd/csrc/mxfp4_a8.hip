// mxfp4_a8.hip -- the prompt route of MXFP4 models with MXFP8 activations (include/zhilight_amd.h "MXFP4", opt-in):
//   zl_mxfp8_quantize   x (M, K) fp16 / bf16 -> E4M3 codes (M, K) + one E8M0 scale byte per 32 elements (M, K/32), the OCP MX rule
//   zl_mxfp4_a8_linear  y = T(sum_b 2^(xs + ws - 254) sum_{i<32} E4M3(xq) E2M1(code) [+ bias]) on v_mfma_scale_f32_16x16x128_f8f6f4:
//                       the instruction decodes both operands and applies both block scales, so the kernel has no decode VALU at all
//
// THE INSTRUCTION (cbsz 0: A = E4M3, blgp 4: B = E2M1), as measured on an MI355X with one-hot operands and pinned by
// tests/test_gpu_mxfp4_a8.py's one-hot case.  Lane l = r + 16 g holds row (A) / column (B) r; of the step's 128 k elements
//   B (4 VGPRs, 16 bytes)  k = 32 g .. 32 g + 31 in order, element 2 j in bits 0-3 of byte j: one MX block per lane;
//   A (8 VGPRs, 32 bytes)  bytes 0-15 are k = 16 g .. 16 g + 15, bytes 16-31 are k = 64 + 16 g .. 64 + 16 g + 15 (the layout of the
//                          64-wide FP8 MFMA, twice) -- NOT 32 consecutive elements: a lane holds half of block g / 2 and half of
//                          block 2 + g / 2;
//   scales (one VGPR each) the byte that op_sel (0..3) picks in lane r + 16 b scales k block b (k = 32 b .. 32 b + 31) of row /
//                          column r, for A and for B alike;
// D[4 g + i][r] in register i like the other 16 x 16 MFMAs.  Which block of the matrix a step calls "block b" is the kernel's choice
// as long as A, B and the scales agree, and both layouts in memory ALREADY ARE fragments: a lane's B operand is the 16 contiguous
// bytes of a block of codes, its A operand two 16-byte halves of two blocks of xq.
//
// SPLIT.  A workgroup is 4 waves side by side along N, a wave owns 64 x 64 outputs (4 x 4 MFMA tiles, 64 fp32 accumulators per
// lane): workgroup tile 64 x 256, no K split, no atomics -- the sum order is fixed by the shape.  Workgroups are numbered M-fastest,
// so the row slices of one weight tile run together and its second and later readers hit the L2.
// K is walked in SUPER-STEPS of 16 blocks (512 elements).  In super-step S group g owns blocks 16 S + 4 g .. + 3 and MFMA step j takes
// block 16 S + 4 g + j of every group.  That choice makes
//   - a lane's four scale bytes of a row for the whole super-step ONE aligned dword (bytes 16 S + 4 g .. + 3 of the row): one VGPR
//     per row tile feeds the super-step's 16 MFMAs of that tile through op_sel = j (rows whose K / 32 is no multiple of 4 are not
//     dword aligned and gather the four bytes one by one);
//   - a lane's loads of a super-step one contiguous run of codes (64 B per row, 16 B per step) and eight 16 B halves of xq (two
//     per step, 32 B apart: the lanes of groups g and g ^ 1 together read whole 128 B lines), straight from global memory into the
//     MFMA operand registers.
// DATA PATH.  No LDS: the four waves share the 64 activation rows, and the bytes they share are already in fragment order, so an LDS
// stage would be a write and a read of the same 16-byte pieces; the sharing is left to the CU's vector cache (8 KB of xq per step).
// Every code byte is loaded once per workgroup.  Step t + 1's operands (4 x 8 + 4 x 4 VGPRs) are in flight while step t's 16 MFMAs
// run (two register buffers, static indices: the four steps of a super-step are unrolled); the next super-step's scale dwords are
// asked for at its head.  Blocks past K / 32 (K no multiple of 512) are zero codes under scale byte 127: exact zeros.
// Rows / columns past M / N are clamped for the loads and not stored.
#include "zl_mxfp4.h"

namespace {

typedef int i8v __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ---- quantiser ---------------------------------------------------------------------------------------------------------------
// |v| (fp32, finite) -> the E4M3 code of the nearest value, ties to even, saturating at 448 (0x7E).  Normal range (>= 2^-6): round
// the fp32 mantissa to 3 bits in integer arithmetic and rebias; below: the code IS the multiple of 2^-9 (code 8 = 2^-6).
__device__ __forceinline__ uint32_t mx_e4m3(float v) {
    const uint32_t sign = (__builtin_bit_cast(uint32_t, v) >> 24) & 0x80u;
    const float a = fminf(fabsf(v), 448.f);
    uint32_t code;
    if (a >= 0.015625f) {
        uint32_t u = __builtin_bit_cast(uint32_t, a);
        u += 0x7ffffu + ((u >> 20) & 1u);
        code = (u >> 20) - ((127u - 7u) << 3);
    } else {
        code = (uint32_t)__builtin_rintf(a * 512.f);                                 // exact product, v_rndne_f32: ties to even
    }
    return code | sign;
}

// Four lanes own a block: 8 elements each (one 16-byte load), amax over the quad by two butterflies, 8 codes = one 8-byte store.
// A wave covers 16 whole blocks; 256-thread workgroups walk the (M x K / 32) blocks in row-major order.
template <int DT>
__global__ __launch_bounds__(256) void k_mxfp8_quantize(const uint16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ xq,
                                                        uint8_t* __restrict__ xs, int64_t blocks, int nb) {
    const int64_t at = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
    const int part = threadIdx.x & 3;
    const bool live = at < blocks;
    const int64_t blk = live ? at : blocks - 1;
    const int64_t row = blk / nb;
    const int b = (int)(blk - row * nb);
    const uint4 raw = *reinterpret_cast<const uint4*>(x + row * ldx + (int64_t)b * 32 + part * 8);
    const uint32_t pairs[4] = {raw.x, raw.y, raw.z, raw.w};
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = ZT<DT>::to_f32((uint16_t)(pairs[i] & 0xffffu));
        v[2 * i + 1] = ZT<DT>::to_f32((uint16_t)(pairs[i] >> 16));
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    // floor(log2(amax)) + 127 is the fp32 exponent field (0 for zero and for bf16's subnormals, which clamp to byte 0 anyway)
    const int field = (int)(__builtin_bit_cast(uint32_t, amax) >> 23);
    const int byte = field > 8 ? field - 8 : 0;                                      // <= 246
    const float inv = __builtin_bit_cast(float, (uint32_t)(254 - byte) << 23);       // 2^(127 - byte): a normal fp32, the product exact
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        lo |= mx_e4m3(v[i] * inv) << (8 * i);
        hi |= mx_e4m3(v[4 + i] * inv) << (8 * i);
    }
    if (live) {
        *reinterpret_cast<uint2*>(xq + blk * 32 + part * 8) = make_uint2(lo, hi);
        if (part == 0) xs[blk] = (uint8_t)byte;
    }
}

// ---- GEMM --------------------------------------------------------------------------------------------------------------------
struct Mx4A8Params : Mx4Params {
    const uint8_t* xq;
    const uint8_t* xs;
    int mtiles;                 // ceil(m / 64)
};

constexpr int kA8T = 4;         // 16 x 16 tiles per wave along M and along N
constexpr int kA8Rows = 16 * kA8T, kA8Cols = 4 * 16 * kA8T;      // workgroup tile 64 x 256

struct Mx4A8Frag {
    i8v a[kA8T];
    uint4 b[kA8T];
};

// MFMA step J of a super-step: the 16 tiles of the wave on block 16 S + 4 g + J, scale byte J of the super-step's dwords
template <int J>
__device__ __forceinline__ void mx_a8_step(const Mx4A8Frag& f, const uint32_t (&sa)[kA8T], const uint32_t (&sb)[kA8T], f4 (&acc)[kA8T][kA8T]) {
#pragma unroll
    for (int tm = 0; tm < kA8T; ++tm)
#pragma unroll
        for (int tn = 0; tn < kA8T; ++tn) {
            const i8v bv = {(int)f.b[tn].x, (int)f.b[tn].y, (int)f.b[tn].z, (int)f.b[tn].w, 0, 0, 0, 0};
            acc[tm][tn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(f.a[tm], bv, acc[tm][tn], 0, 4, J, (int)sa[tm], J, (int)sb[tn]);
        }
}

template <int DT>
__global__ __launch_bounds__(256) void k_mxfp4_a8(const Mx4A8Params p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int m0 = (int)(blockIdx.x % (unsigned)p.mtiles) * kA8Rows;
    const int n0 = (int)(blockIdx.x / (unsigned)p.mtiles) * kA8Cols + wave * (16 * kA8T);
    if (n0 >= p.n) return;                                                           // the whole wave; the kernel has no barrier
    const bool dwords = (p.nb & 3) == 0;
    const uint8_t* arow[kA8T];
    const uint8_t* asrow[kA8T];
    const uint8_t* brow[kA8T];
    const uint8_t* bsrow[kA8T];
#pragma unroll
    for (int t = 0; t < kA8T; ++t) {
        const int row = min(m0 + 16 * t + r16, p.m - 1), col = min(n0 + 16 * t + r16, p.n - 1);
        arow[t] = p.xq + (size_t)row * p.k;
        asrow[t] = p.xs + (size_t)row * p.nb;
        brow[t] = p.codes + (size_t)col * (p.k / 2);
        bsrow[t] = p.scales + (size_t)col * p.nb;
    }
    f4 acc[kA8T][kA8T];
#pragma unroll
    for (int i = 0; i < kA8T; ++i)
#pragma unroll
        for (int j = 0; j < kA8T; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};

    // the operands of the MFMA step whose k block b is block sj + 4 b of the matrices: the lane's B is block sj + 4 g, its A the
    // halves (g & 1) of blocks sj + 4 (g / 2) and sj + 4 (2 + g / 2); a block past the last one is zeros
    const int ga = 4 * (g >> 1), half = 16 * (g & 1);
    auto load = [&](Mx4A8Frag& f, int sj) {
        const int bb = sj + 4 * g, ba0 = sj + ga, ba1 = sj + 8 + ga;
#pragma unroll
        for (int t = 0; t < kA8T; ++t) {
            uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
            f.b[t] = a0;
            if (ba0 < p.nb) a0 = *reinterpret_cast<const uint4*>(arow[t] + (size_t)ba0 * 32 + half);
            if (ba1 < p.nb) a1 = *reinterpret_cast<const uint4*>(arow[t] + (size_t)ba1 * 32 + half);
            if (bb < p.nb) f.b[t] = *reinterpret_cast<const uint4*>(brow[t] + (size_t)bb * 16);
            f.a[t] = (i8v){(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
        }
    };
    auto scales = [&](uint32_t (&sa)[kA8T], uint32_t (&sb)[kA8T], int b0) {
#pragma unroll
        for (int t = 0; t < kA8T; ++t) {
            sa[t] = mx_scale4(asrow[t], b0, p.nb, dwords);
            sb[t] = mx_scale4(bsrow[t], b0, p.nb, dwords);
        }
    };

    Mx4A8Frag buf[2];
    uint32_t sa[kA8T], sb[kA8T], san[kA8T], sbn[kA8T];
    scales(sa, sb, 4 * g);
    load(buf[0], 0);
#pragma unroll 1
    for (int s0 = 0; s0 < p.nb; s0 += 16) {                                          // one super-step: blocks s0 .. s0 + 15
        const int b0 = s0 + 4 * g;
        scales(san, sbn, b0 + 16);
        load(buf[1], s0 + 1); mx_a8_step<0>(buf[0], sa, sb, acc);
        load(buf[0], s0 + 2); mx_a8_step<1>(buf[1], sa, sb, acc);
        load(buf[1], s0 + 3); mx_a8_step<2>(buf[0], sa, sb, acc);
        load(buf[0], s0 + 16); mx_a8_step<3>(buf[1], sa, sb, acc);
#pragma unroll
        for (int t = 0; t < kA8T; ++t) { sa[t] = san[t]; sb[t] = sbn[t]; }
    }
#pragma unroll
    for (int tm = 0; tm < kA8T; ++tm)
#pragma unroll
        for (int tn = 0; tn < kA8T; ++tn) mx_store_tile<DT>(p, m0 + 16 * tm, n0 + 16 * tn + r16, g, acc[tm][tn]);
}

}  // namespace

extern "C" int zl_mxfp8_quantize(const uint16_t* x, int64_t ldx, uint8_t* xq, uint8_t* xs, int64_t m, int64_t k, int dtype, zl_stream_t s) {
    ZL_CHECK_ARG(x && xq && xs && m > 0 && k > 0, ZL_EINVAL);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(k % 32 == 0 && ldx >= k && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)xq & 15) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(k < ((int64_t)1 << 31), ZL_ELIMIT);
    const int64_t blocks = m * (k / 32);
    ZL_CHECK_ARG((blocks + 63) / 64 < ((int64_t)1 << 31), ZL_ELIMIT);
    const dim3 grid((unsigned)((blocks + 63) / 64));
    if (dtype == ZL_F16) hipLaunchKernelGGL((k_mxfp8_quantize<ZL_F16>), grid, dim3(256), 0, (hipStream_t)s, x, ldx, xq, xs, blocks, (int)(k / 32));
    else hipLaunchKernelGGL((k_mxfp8_quantize<ZL_BF16>), grid, dim3(256), 0, (hipStream_t)s, x, ldx, xq, xs, blocks, (int)(k / 32));
    return zl_launch_status();
}

extern "C" int zl_mxfp4_a8_linear(const uint8_t* xq, const uint8_t* xs, const uint8_t* codes, const uint8_t* scales, const uint16_t* bias,
                                  const uint16_t* residual, uint16_t* y, int64_t m, int64_t n, int64_t k, int dtype, int epilogue,
                                  zl_stream_t s) {
    ZL_CHECK_ARG(xq && xs && codes && scales && y && m > 0 && n > 0 && k > 0, ZL_EINVAL);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(k % 32 == 0 && ((uintptr_t)xq & 15) == 0 && ((uintptr_t)codes & 15) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG((k / 32) % 4 != 0 || ((((uintptr_t)xs) | ((uintptr_t)scales)) & 3) == 0, ZL_ESHAPE);     // the scale rows read as dwords
    ZL_CHECK_ARG((epilogue & ~(ZL_EPI_BIAS | ZL_EPI_RESIDUAL | ZL_EPI_SILU_MUL)) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(!((epilogue & ZL_EPI_SILU_MUL) && ((epilogue & ZL_EPI_RESIDUAL) || n % 2 != 0)), ZL_ESHAPE);
    ZL_CHECK_ARG(!((epilogue & ZL_EPI_RESIDUAL) && !residual) && !((epilogue & ZL_EPI_BIAS) && !bias), ZL_EINVAL);
    ZL_CHECK_ARG(n < ((int64_t)1 << 31) - kA8Cols && k < ((int64_t)1 << 31) && m < ((int64_t)1 << 31) - kA8Rows, ZL_ELIMIT);
    Mx4A8Params p;
    p.x = nullptr; p.ldx = 0; p.codes = codes; p.scales = scales; p.bias = bias; p.residual = residual; p.y = y;
    p.m = (int)m; p.n = (int)n; p.k = (int)k; p.nb = (int)(k / 32); p.epi = epilogue;
    p.xq = xq; p.xs = xs; p.mtiles = (int)((m + kA8Rows - 1) / kA8Rows);
    const int64_t groups = (int64_t)p.mtiles * ((n + kA8Cols - 1) / kA8Cols);
    ZL_CHECK_ARG(groups < ((int64_t)1 << 31), ZL_ELIMIT);
    if (dtype == ZL_F16) hipLaunchKernelGGL((k_mxfp4_a8<ZL_F16>), dim3((unsigned)groups), dim3(256), 0, (hipStream_t)s, p);
    else hipLaunchKernelGGL((k_mxfp4_a8<ZL_BF16>), dim3((unsigned)groups), dim3(256), 0, (hipStream_t)s, p);
    return zl_launch_status();
}
