// zl_mxfp4_a4.h -- what the FP4 x FP4 kernels share (mxfp4_a4.hip: the dense W4A4 linear; mxfp4_moe_a4.hip: its expert-grouped
// form): the MFMA step on the instruction's FP4 x FP4 form and the unconditional guarded loads of a block's codes and of a
// super-step's scale dword.  mxfp4_a4.hip's header has the instruction's operand map and the K walk; ONE copy of the step is what
// the grouped kernel's bit contract with the dense one rests on.
#pragma once
#include <type_traits>

#include "zl_mxfp4.h"

typedef int mx_i8v __attribute__((ext_vector_type(8)));

constexpr int kA4TN = 4;        // 16-column tiles per wave along N

__device__ __forceinline__ mx_i8v mx_a4_operand(const uint4& q) { return (mx_i8v){(int)q.x, (int)q.y, (int)q.z, (int)q.w, 0, 0, 0, 0}; }

// MFMA step J of a super-step: the TM x 4 tiles of the wave on block 16 S + 4 g + J, scale byte J of the super-step's dwords.  After a
// row tile's four MFMAs `next(tm)` asks LDS for that row tile's piece of the FOLLOWING step (into the other A buffer): it is used a
// whole step later.
template <int J, int TM, class Next>
__device__ __forceinline__ void mx_a4_step(const uint4 (&a)[TM], const uint4 (&b)[kA4TN], const uint32_t (&sa)[TM],
                                           const uint32_t (&sb)[kA4TN], mx_f4 (&acc)[TM][kA4TN], Next next) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
        for (int tn = 0; tn < kA4TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mx_a4_operand(a[tm]), mx_a4_operand(b[tn]), acc[tm][tn], 4, 4, J,
                                                                           (int)sa[tm], J, (int)sb[tn]);
        // an empty statement that pins the source order of loads and MFMAs: left alone, instruction selection sinks all 64 MFMAs of a
        // super-step below its loads -- four steps of A and B live at once, past 256 VGPRs into scratch -- and no load may cross it,
        // so the prefetch distances of the callers are the ones that run
        asm volatile("" : "+v"(acc[tm][0]), "+v"(acc[tm][1]), "+v"(acc[tm][2]), "+v"(acc[tm][3]) : : "memory");
        next(tm);
    }
}

// What a block past the last one reads as: zero codes under scale byte 127.  Never written, and NOT const: a constant would be
// folded into the kernel and the selected load below would turn back into a load under a branch.
static __device__ uint4 kA4ZeroCodes = {0u, 0u, 0u, 0u};
static __device__ uint32_t kA4UnitScales = 0x7f7f7f7fu;

// The 16 bytes of block blk of a row of codes; GUARD: a block past the last one reads the zero block instead.  The ADDRESS is
// selected and the load is unconditional: after a load under a branch the compiler's wait counts can no longer tell how many
// younger loads are in flight and every wait becomes vmcnt(0) -- a step would wait for the operands it has just asked for.
template <bool GUARD>
__device__ __forceinline__ uint4 mx_a4_block(const uint8_t* row, int blk, int nb) {
    const uint4* at = reinterpret_cast<const uint4*>(row + (size_t)blk * 16);
    if (GUARD) at = blk < nb ? at : &kA4ZeroCodes;
    return *at;
}
// mx_scale4 with the dword form's load unconditional for the same reason.  DW (K / 32 % 4 == 0, every model shape) is a template
// argument: the byte-by-byte form loads under branches, and a kernel that merely CONTAINS it loses its wait counts
template <bool DW>
__device__ __forceinline__ uint32_t mx_a4_scale4(const uint8_t* srow, int b0, int nb) {
    if (!DW) return mx_scale4(srow, b0, nb, false);
    return *(b0 < nb ? reinterpret_cast<const uint32_t*>(srow + b0) : &kA4UnitScales);
}
