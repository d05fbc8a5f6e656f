// zl_w4m_dequant.h -- the ZLW4M word -> fp16 weight step, one definition per flavour:
//   dequant_word     (q - z), exact: the streaming kernels (w4_mfma.hip, w4_phase.hip, w4_slab.hip), which apply the scale to the
//                    fp32 group sums;
//   zl_w4m_dequant8  rn16((q - z) * s): the M-tiled GEMM (w4_gemm_tiled.hip) and the expert-grouped GEMM (w4_moe_grouped.hip),
//                    which must produce the same W16 to stay bit-identical.
// (zl_w4m_dequant8 is not written in terms of dequant_word: multiplying the assembled h8 instead of the four pairs changed the
// tiled kernels' assembly -- profiles/w4m_shared_epilogue.txt.)
#pragma once
#include "zl_common.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 hv2 __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ uint32_t and_or(uint32_t w, uint32_t mask_s, uint32_t magic_v) {
    uint32_t r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(w), "s"(mask_s), "v"(magic_v));
    return r;
}

// word -> 8 fp16 (q - z), exact; natural k order (w0..w7) = MFMA A-fragment element order.  z1 = -(1024 + z), z16 = z1 + 960 (the
// high nibbles arrive times 16), magic = 0x6400 | nibble = 1024 + q
static __device__ __forceinline__ h8 dequant_word(uint32_t w, hv2 z1, hv2 z16, uint32_t mask_lo, uint32_t mask_hi, uint32_t magic) {
    const hv2 one16 = {(_Float16)0.0625f, (_Float16)0.0625f};
    const hv2 d0 = __builtin_bit_cast(hv2, and_or(w, mask_lo, magic)) + z1;
    const hv2 d1 = __builtin_elementwise_fma(__builtin_bit_cast(hv2, and_or(w, mask_hi, magic)), one16, z16);
    const uint32_t wb = w >> 8;
    const hv2 d2 = __builtin_bit_cast(hv2, and_or(wb, mask_lo, magic)) + z1;
    const hv2 d3 = __builtin_elementwise_fma(__builtin_bit_cast(hv2, and_or(wb, mask_hi, magic)), one16, z16);
    h8 a;
    a[0] = d0.x; a[1] = d0.y; a[2] = d1.x; a[3] = d1.y; a[4] = d2.x; a[5] = d2.y; a[6] = d3.x; a[7] = d3.y;
    return a;
}

// word -> 8 x fp16 rn16((q - z) * s): exact (q - z), one rounding in the multiply == dequant_k_major
static __device__ __forceinline__ h8 zl_w4m_dequant8(uint32_t w, hv2 z1, hv2 z16, hv2 s2, uint32_t mask_lo, uint32_t mask_hi,
                                                     uint32_t magic) {
    const hv2 one16 = {(_Float16)0.0625f, (_Float16)0.0625f};
    const hv2 d0 = (__builtin_bit_cast(hv2, and_or(w, mask_lo, magic)) + z1) * s2;
    const hv2 d1 = __builtin_elementwise_fma(__builtin_bit_cast(hv2, and_or(w, mask_hi, magic)), one16, z16) * s2;
    const uint32_t wb = w >> 8;
    const hv2 d2 = (__builtin_bit_cast(hv2, and_or(wb, mask_lo, magic)) + z1) * s2;
    const hv2 d3 = __builtin_elementwise_fma(__builtin_bit_cast(hv2, and_or(wb, mask_hi, magic)), one16, z16) * s2;
    h8 a;
    a[0] = d0.x; a[1] = d0.y; a[2] = d1.x; a[3] = d1.y; a[4] = d2.x; a[5] = d2.y; a[6] = d3.x; a[7] = d3.y;
    return a;
}
