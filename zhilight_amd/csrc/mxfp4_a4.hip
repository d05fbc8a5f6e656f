// mxfp4_a4.hip -- the prompt route of MXFP4 models with MXFP4 activations, W4A4 (include/zhilight_amd.h "MXFP4", opt-in):
//   zl_mxfp4_act_quantize  x (M, K) fp16 / bf16 -> E2M1 codes (M, K/2) + one E8M0 scale byte per 32 elements (M, K/32): the
//                          checkpoint's weight layout, the OCP MX rule
//   zl_mxfp4_a4_linear     y = T(sum_b 2^(xs + ws - 254) sum_{i<32} E2M1(xq) E2M1(code) [+ bias]) on the FP4 x FP4 form of
//                          v_mfma_scale_f32_16x16x128_f8f6f4: both operands decoded and both block scales applied by the instruction
//
// THE INSTRUCTION (cbsz 4: A = E2M1, blgp 4: B = E2M1), as measured on an MI355X with one-hot operands and pinned by
// tests/test_gpu_mxfp4_a4.py's one-hot case.  Lane l = r + 16 g holds row (A) / column (B) r; of the step's 128 k elements
//   A and B alike (4 VGPRs, 16 bytes)  k = 32 g .. 32 g + 31 in order, element 2 j in bits 0-3 of byte j: one MX block per lane --
//                          unlike the E4M3 A operand of mxfp4_a8.hip, the FP4 A operand MIRRORS B;
//   scales (one VGPR each) the byte that op_sel (0..3) picks in lane r + 16 b scales k block b of row / column r, for A and B alike;
// D[4 g + i][r] in register i.  xq has the weights' layout, so a lane's A operand is 16 contiguous bytes of xq as its B operand is 16
// contiguous bytes of codes: both tensors already are fragments.
//
// SPLIT.  A workgroup is 4 waves side by side along N, a wave owns 64 x 64 outputs (4 x 4 MFMA tiles, 64 fp32 accumulators per lane):
// workgroup tile 64 x 256, no K split, no atomics.  Workgroups are numbered M-fastest (the row slices of one weight tile run together
// and share it in the L2).  K is walked in SUPER-STEPS of 16 blocks: in super-step S lane group g owns blocks 16 S + 4 g .. + 3 and
// MFMA step j takes block 16 S + 4 g + j of every group, so a row's four scale bytes of a super-step are ONE aligned dword feeding
// op_sel = j (mx_scale4 gathers them byte by byte for rows with K / 32 % 4 != 0) and a lane's codes of a super-step are 64
// contiguous bytes.  The kernel is held to TWO waves per SIMD (__launch_bounds__(256, 2), two workgroups per CU: one multiplies while
// the other waits at its barrier or for its loads); the 4-register operands are what makes room for that -- 203 VGPRs, no scratch.
//
// DATA PATH.  B (weights): a lane's 16 code bytes per step and the scale dword of a super-step straight from global memory into the
// operand registers; a code byte is used by exactly one wave.  A RING OF FOUR register slots, slot j = step j of a super-step,
// filled THREE steps (48 MFMAs) ahead.
// A (activations): THROUGH LDS, IN FRAGMENT ORDER, once per workgroup.  The reason: an FP4 x FP4 step is 16 MFMAs of 4 passes --
// about 256 cycles per wave -- for 4 KB of A and 4 KB of B per wave; with every wave pulling its own A the four SIMDs of a CU ask the
// vector cache for 32 KB per 256 cycles, twice its 64 B / clk, and half of that is the same 4 KB four times over.  Staged, the
// cache delivers 20 KB per step and the shared bytes come from LDS (128 B / clk).  The direct form (k_mxfp4_a8's) was not built
// for this operand: that A/B is unmeasured.  Wave w stages row tile w: lane r + 16 g loads the 64 contiguous bytes of blocks
// 16 S + 4 g .. + 3 of row 16 w + r (four 16-byte loads) at the head of the super-step before, keeps them in 16 VGPRs while that
// super-step multiplies and writes them as pieces [j][w] -- piece [j][tm] holds at 16 l the A operand of lane l in step j on row tile
// tm -- with ds_write_b128; a step reads its four pieces with ds_read_b128 one step ahead, row tile by row tile, into the second of
// two A register buffers: whole contiguous KBs either way, no bank conflicts.  The scale dwords of tile w go the same way.  Two LDS
// buffers (2 x 17 KB), ONE barrier per super-step: buffer (S + 1) & 1 is written after the multiplies of S and was last read in
// S - 1, before the barrier that ended it.
// WHAT THE COMPILER NEEDED (each found in the assembly, see the comments at the code, zl_mxfp4_a4.h): every global load is unconditional -- a block
// past K / 32 selects the ADDRESS of a zero block (scale byte 127), so it reads exact zeros -- because a load under a branch turns
// the following waits into vmcnt(0); an empty asm statement after each row tile's MFMAs pins the source order, or all 64 MFMAs of a
// super-step sink below its loads and the kernel spills; K / 32 % 4 is a template argument.
// Rows / columns past M / N are clamped for the loads and not stored; a wave whose 64 columns lie past N multiplies nothing but
// stays for the staging and the barriers.
#include "zl_mxfp4_a4.h"

namespace {

typedef mx_f4 f4;

// ---- quantiser ---------------------------------------------------------------------------------------------------------------
// v (fp32, finite) -> the E2M1 code of the nearest value, ties to the even code, saturating at 6.  Plain integer arithmetic, no
// hardware converter.  Normal range (>= 1): round the fp32 mantissa to 1 bit and rebias (exponent bias 1); below: the code IS the
// multiple of 0.5 (code 2 = 1.0).  A negative value that rounds to zero keeps its sign bit (code 8, which decodes to 0).
__device__ __forceinline__ uint32_t mx_e2m1(float v) {
    const uint32_t sign = (__builtin_bit_cast(uint32_t, v) >> 28) & 8u;
    const float a = fminf(fabsf(v), 6.f);
    uint32_t code;
    if (a >= 1.f) {
        uint32_t u = __builtin_bit_cast(uint32_t, a);
        u += 0x1fffffu + ((u >> 22) & 1u);
        code = (u >> 22) - ((127u - 1u) << 1);
    } else {
        code = (uint32_t)__builtin_rintf(a * 2.f);                                   // exact product, v_rndne_f32: ties to even
    }
    return code | sign;
}

// Two lanes own a block: 16 elements each (two 16-byte loads, 32 contiguous bytes), amax over the pair by one butterfly, 16 codes
// = one 8-byte store; the pair writes the block's 16 bytes.  A wave covers 32 whole blocks (2 KB of x in, 512 B out); 256-thread
// workgroups walk the (M x K / 32) blocks in row-major order.
template <int DT>
__global__ __launch_bounds__(256) void k_mxfp4_act_quantize(const uint16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ xq,
                                                            uint8_t* __restrict__ xs, int64_t blocks, int nb) {
    const int64_t at = (int64_t)blockIdx.x * 128 + (threadIdx.x >> 1);
    const int part = threadIdx.x & 1;
    const bool live = at < blocks;
    const int64_t blk = live ? at : blocks - 1;
    const int64_t row = blk / nb;
    const int b = (int)(blk - row * nb);
    const uint4* src = reinterpret_cast<const uint4*>(x + row * ldx + (int64_t)b * 32 + part * 16);
    const uint4 r0 = src[0], r1 = src[1];
    const uint32_t pairs[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    float v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[2 * i] = ZT<DT>::to_f32((uint16_t)(pairs[i] & 0xffffu));
        v[2 * i + 1] = ZT<DT>::to_f32((uint16_t)(pairs[i] >> 16));
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    // floor(log2(amax)) + 127 is the fp32 exponent field (0 for zero and for bf16's subnormals, which clamp to byte 0 anyway)
    const int field = (int)(__builtin_bit_cast(uint32_t, amax) >> 23);
    const int byte = field > 2 ? field - 2 : 0;                                      // <= 252
    const float inv = __builtin_bit_cast(float, (uint32_t)(254 - byte) << 23);       // 2^(127 - byte): a normal fp32, the product exact
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        lo |= mx_e2m1(v[i] * inv) << (4 * i);
        hi |= mx_e2m1(v[8 + i] * inv) << (4 * i);
    }
    if (live) {
        *reinterpret_cast<uint2*>(xq + blk * 16 + part * 8) = make_uint2(lo, hi);
        if (part == 0) xs[blk] = (uint8_t)byte;
    }
}

// ---- GEMM --------------------------------------------------------------------------------------------------------------------
struct Mx4A4Params : Mx4Params {
    const uint8_t* xq;          // (m, k / 2) E2M1 codes
    const uint8_t* xs;          // (m, nb) E8M0 scale bytes
    int mtiles;                 // ceil(m / 64)
};

constexpr int kA4T = kA4TN;     // 16 x 16 tiles per wave along M and along N (the step, the zero block and the guarded loads: zl_mxfp4_a4.h)
constexpr int kA4Rows = 16 * kA4T, kA4Cols = 4 * 16 * kA4T;      // workgroup tile 64 x 256

template <int DT, bool DW>
__global__ __launch_bounds__(256, 2) void k_mxfp4_a4(const Mx4A4Params p) {
    __shared__ uint4 lds_a[2][4 * kA4T][64];                                         // [buffer][step j * 4 + row tile][lane]
    __shared__ uint32_t lds_s[2][kA4T][64];                                          // [buffer][row tile][lane]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int m0 = (int)(blockIdx.x % (unsigned)p.mtiles) * kA4Rows;
    const int n0 = (int)(blockIdx.x / (unsigned)p.mtiles) * kA4Cols + wave * (16 * kA4T);
    const bool active = n0 < p.n;                                                    // wave-uniform; an idle wave still stages

    // staging: wave w owns row tile w
    const int srow = min(m0 + 16 * wave + r16, p.m - 1);
    const uint8_t* arow = p.xq + (size_t)srow * (p.k / 2);
    const uint8_t* asrow = p.xs + (size_t)srow * p.nb;
    uint4 st[4];
    uint32_t sts;
    auto stage_load = [&](int s0) {                                                  // global -> registers: blocks s0 + 4 g .. + 3
#pragma unroll
        for (int j = 0; j < 4; ++j) st[j] = mx_a4_block<true>(arow, s0 + 4 * g + j, p.nb);
        sts = mx_a4_scale4<DW>(asrow, s0 + 4 * g, p.nb);
    };
    auto stage_store = [&](int buf) {                                                // registers -> LDS
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_a[buf][j * kA4T + wave][lane] = st[j];
        lds_s[buf][wave][lane] = sts;
    };

    const uint8_t* brow[kA4T];
    const uint8_t* bsrow[kA4T];
#pragma unroll
    for (int t = 0; t < kA4T; ++t) {
        const int col = min(n0 + 16 * t + r16, p.n - 1);                             // an idle wave's pointers are never used
        brow[t] = p.codes + (size_t)col * (p.k / 2);
        bsrow[t] = p.scales + (size_t)col * p.nb;
    }
    f4 acc[kA4T][kA4T];
#pragma unroll
    for (int i = 0; i < kA4T; ++i)
#pragma unroll
        for (int j = 0; j < kA4T; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};

    // B: a ring of four register slots, slot j = step j of a super-step, filled THREE steps ahead (about 48 MFMAs, 768 cycles, for
    // the L2 or HBM to answer).  A: two register buffers, step j reads a[j & 1] and refills the other row tile by row tile.
    uint4 a[2][kA4T], b[4][kA4T];
    uint32_t sa[kA4T], sb[kA4T], sbn[kA4T];
    auto load_b = [&](auto guard, uint4 (&f)[kA4T], int sj) {                        // the lane's B of the step on blocks sj + 4 b: block sj + 4 g
#pragma unroll
        for (int t = 0; t < kA4T; ++t) f[t] = mx_a4_block<decltype(guard)::value>(brow[t], sj + 4 * g, p.nb);
    };
    stage_load(0);
    stage_store(0);
    if (active) {
#pragma unroll
        for (int t = 0; t < kA4T; ++t) sb[t] = mx_a4_scale4<DW>(bsrow[t], 4 * g, p.nb);
        load_b(std::true_type(), b[0], 0);
        load_b(std::true_type(), b[1], 1);
        load_b(std::true_type(), b[2], 2);
    }
    __syncthreads();
    // one super-step, blocks s0 .. s0 + 15; FULL: all 16 exist, so only what is asked for the NEXT super-step needs the guard
    auto super_step = [&](auto full, int s0) {
        const int cur = (s0 >> 4) & 1;
        stage_load(s0 + 16);                                                         // past the end: the zero block, never read back
        if (active) {
#pragma unroll
            for (int tm = 0; tm < kA4T; ++tm) {
                sa[tm] = lds_s[cur][tm][lane];
                a[0][tm] = lds_a[cur][tm][lane];                                     // step 0's pieces
            }
#pragma unroll
            for (int t = 0; t < kA4T; ++t) sbn[t] = mx_a4_scale4<DW>(bsrow[t], s0 + 16 + 4 * g, p.nb);
            auto piece = [&](int j) { return [&, j](int tm) { a[j & 1][tm] = lds_a[cur][j * kA4T + tm][lane]; }; };
            load_b(std::integral_constant<bool, !decltype(full)::value>(), b[3], s0 + 3);
            mx_a4_step<0>(a[0], b[0], sa, sb, acc, piece(1));
            load_b(std::true_type(), b[0], s0 + 16);
            mx_a4_step<1>(a[1], b[1], sa, sb, acc, piece(2));
            load_b(std::true_type(), b[1], s0 + 17);
            mx_a4_step<2>(a[0], b[2], sa, sb, acc, piece(3));
            load_b(std::true_type(), b[2], s0 + 18);
            mx_a4_step<3>(a[1], b[3], sa, sb, acc, [](int) {});
#pragma unroll
            for (int t = 0; t < kA4T; ++t) sb[t] = sbn[t];
            // in both arms: behind the join the wait for st would be vmcnt(0), the B ring's loads included (the empty statement
            // keeps the compiler from merging the two arms' stores behind the join again)
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
#pragma unroll
    for (int tm = 0; tm < kA4T; ++tm)
#pragma unroll
        for (int tn = 0; tn < kA4T; ++tn) mx_store_tile<DT>(p, m0 + 16 * tm, n0 + 16 * tn + r16, g, acc[tm][tn]);
}

}  // namespace

extern "C" int zl_mxfp4_act_quantize(const uint16_t* x, int64_t ldx, uint8_t* xq, uint8_t* xs, int64_t m, int64_t k, int dtype, zl_stream_t s) {
    ZL_CHECK_ARG(x && xq && xs && m > 0 && k > 0, ZL_EINVAL);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(k % 32 == 0 && ldx >= k && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)xq & 15) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(k < ((int64_t)1 << 31), ZL_ELIMIT);
    const int64_t blocks = m * (k / 32);
    ZL_CHECK_ARG((blocks + 127) / 128 < ((int64_t)1 << 31), ZL_ELIMIT);
    const dim3 grid((unsigned)((blocks + 127) / 128));
    if (dtype == ZL_F16) hipLaunchKernelGGL((k_mxfp4_act_quantize<ZL_F16>), grid, dim3(256), 0, (hipStream_t)s, x, ldx, xq, xs, blocks, (int)(k / 32));
    else hipLaunchKernelGGL((k_mxfp4_act_quantize<ZL_BF16>), grid, dim3(256), 0, (hipStream_t)s, x, ldx, xq, xs, blocks, (int)(k / 32));
    return zl_launch_status();
}

extern "C" int zl_mxfp4_a4_linear(const uint8_t* xq, const uint8_t* xs, const uint8_t* codes, const uint8_t* scales, const uint16_t* bias,
                                  const uint16_t* residual, uint16_t* y, int64_t m, int64_t n, int64_t k, int dtype, int epilogue,
                                  zl_stream_t s) {
    ZL_CHECK_ARG(xq && xs && codes && scales && y && m > 0 && n > 0 && k > 0, ZL_EINVAL);
    ZL_CHECK_ARG(dtype == ZL_F16 || dtype == ZL_BF16, ZL_EDTYPE);
    ZL_CHECK_ARG(k % 32 == 0 && ((uintptr_t)xq & 15) == 0 && ((uintptr_t)codes & 15) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG((k / 32) % 4 != 0 || ((((uintptr_t)xs) | ((uintptr_t)scales)) & 3) == 0, ZL_ESHAPE);     // the scale rows read as dwords
    ZL_CHECK_ARG((epilogue & ~(ZL_EPI_BIAS | ZL_EPI_RESIDUAL | ZL_EPI_SILU_MUL)) == 0, ZL_ESHAPE);
    ZL_CHECK_ARG(!((epilogue & ZL_EPI_SILU_MUL) && ((epilogue & ZL_EPI_RESIDUAL) || n % 2 != 0)), ZL_ESHAPE);
    ZL_CHECK_ARG(!((epilogue & ZL_EPI_RESIDUAL) && !residual) && !((epilogue & ZL_EPI_BIAS) && !bias), ZL_EINVAL);
    ZL_CHECK_ARG(n < ((int64_t)1 << 31) - kA4Cols && k < ((int64_t)1 << 31) && m < ((int64_t)1 << 31) - kA4Rows, ZL_ELIMIT);
    Mx4A4Params p;
    p.x = nullptr; p.ldx = 0; p.codes = codes; p.scales = scales; p.bias = bias; p.residual = residual; p.y = y;
    p.m = (int)m; p.n = (int)n; p.k = (int)k; p.nb = (int)(k / 32); p.epi = epilogue;
    p.xq = xq; p.xs = xs; p.mtiles = (int)((m + kA4Rows - 1) / kA4Rows);
    const int64_t groups = (int64_t)p.mtiles * ((n + kA4Cols - 1) / kA4Cols);
    ZL_CHECK_ARG(groups < ((int64_t)1 << 31), ZL_ELIMIT);
    const dim3 grid((unsigned)groups);
    if (p.nb % 4 == 0) {
        if (dtype == ZL_F16) hipLaunchKernelGGL((k_mxfp4_a4<ZL_F16, true>), grid, dim3(256), 0, (hipStream_t)s, p);
        else hipLaunchKernelGGL((k_mxfp4_a4<ZL_BF16, true>), grid, dim3(256), 0, (hipStream_t)s, p);
    } else {
        if (dtype == ZL_F16) hipLaunchKernelGGL((k_mxfp4_a4<ZL_F16, false>), grid, dim3(256), 0, (hipStream_t)s, p);
        else hipLaunchKernelGGL((k_mxfp4_a4<ZL_BF16, false>), grid, dim3(256), 0, (hipStream_t)s, p);
    }
    return zl_launch_status();
}
