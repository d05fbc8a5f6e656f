// zl_w4m_epilogue.h -- the output arithmetic the W4A16 kernels share (w4_mfma / w4_phase / w4_slab / w4_i8p / w4_gemv /
// w4_gemm_tiled .hip, and w8_phase.hip for the qkv operands and destination).  Each kernel keeps its own way of gathering the
// operands; what happens to them is defined here once, so every route of a projection gives the same bits.
#pragma once
#include "zl_common.h"

static __device__ __forceinline__ float silu_f32(float x) { return x / (1.0f + expf(-x)); }

// plain finish: ((c_in +) v) + bias, rounded to fp16; then the residual added in fp32 and rounded again.  c_in / residual are
// read only under their ZL_EPI_ flag; bias is 0 where there is none
static __device__ __forceinline__ _Float16 zl_w4m_finish(float v, float bias, float c_in, float residual, int epi) {
    float ov;
    if (epi & ZL_EPI_ADD_C) ov = (c_in + v) + bias;
    else ov = v + bias;
    _Float16 y16 = zl_f32_to_f16(ov);
    if (epi & ZL_EPI_RESIDUAL) y16 = zl_f32_to_f16(residual + (float)y16);
    return y16;
}

// gated finish (bias already added): ZL_EPI_SILU_MUL = silu of the fp16-rounded gate times the fp16-rounded up, the two-launch
// result; ZL_EPI_SILU_MUL_F32 = the unrounded pair with the quotient in double (gate_fuse)
static __device__ __forceinline__ float zl_w4m_finish_gated(float g, float u, int epi) {
    if (epi & ZL_EPI_SILU_MUL) {
        g = (float)zl_f32_to_f16(g);
        u = (float)zl_f32_to_f16(u);
        return silu_f32(g) * u;
    }
    return (float)((double)g / (1.0 + (double)expf(-g))) * u;
}

// ---- the fused qkv projection of a decode step: rotate q and k (neox) on the fp16-rounded projection outputs, scatter k / v
// into the ragged KV buffers, q to its own buffer (rope_qk_cache + copy_to_rag_buffer2; roundings of the separate kernels:
// one rounding to T after the fp32 rotation).  A thread owns row m, columns n0 and n0 + d / 2 of the fused qkv row (n0 % d < d / 2).
// P: a kernel parameter block with cosv, sinv, placement, buf_lens, k_bufs, v_bufs, q_out, h, hkv, d, bshd (+ bias, epi for the
// fp16 store).
struct ZlRopeOperands {
    float c0 = 0.f, s0 = 0.f, c1 = 0.f, s1 = 0.f;    // rotation table entries of the two columns (q and k heads)
    int place = -1, blen = 0;                        // the task's slot and buffer length (k and v heads)
    uint16_t* kv = nullptr;                          // ... and its K or V buffer
};

// what the output needs from memory; kernels that can afford it ask ahead of their weight stream
template <class P>
static __device__ __forceinline__ ZlRopeOperands zl_rope_prefetch(const P& p, int m, int n0) {
    ZlRopeOperands r;
    const int head = n0 / p.d, dcol = n0 % p.d, half = p.d / 2;
    if (head < p.h + p.hkv) {
        r.c0 = p.cosv[(size_t)m * p.d + dcol]; r.s0 = p.sinv[(size_t)m * p.d + dcol];
        r.c1 = p.cosv[(size_t)m * p.d + dcol + half]; r.s1 = p.sinv[(size_t)m * p.d + dcol + half];
    }
    if (head >= p.h) {
        r.place = p.placement[m];
        r.blen = p.buf_lens[m];
        r.kv = head < p.h + p.hkv ? p.k_bufs[m] : p.v_bufs[m];
    }
    return r;
}

// where column n0 of row m goes (its partner: + d / 2): q_out, or the task's K / V row in bshd or hsd layout; null = a dropped
// row (placement outside the buffer)
template <class P>
static __device__ __forceinline__ uint16_t* zl_rope_dest(const P& p, const ZlRopeOperands& r, int m, int n0) {
    const int head = n0 / p.d, dcol = n0 % p.d;
    if (head < p.h) return p.q_out + ((size_t)m * p.h + head) * p.d + dcol;
    if (!(r.place >= 0 && r.place < r.blen)) return nullptr;
    const int hk = head - p.h - (head >= p.h + p.hkv ? p.hkv : 0);
    const size_t row = p.bshd ? (size_t)r.place * p.hkv + hk : (size_t)hk * r.blen + r.place;
    return r.kv + row * p.d + dcol;
}

// fp16 outputs: bias, round (the projection's outputs), rotate q / k heads in fp32, round, store
template <class P>
static __device__ __forceinline__ void zl_rope_store_f16(const P& p, const ZlRopeOperands& r, int m, int n0, float v0, float v1) {
    const int half = p.d / 2;
    if ((p.epi & ZL_EPI_BIAS) && p.bias) {
        v0 += (float)__builtin_bit_cast(_Float16, p.bias[n0]);
        v1 += (float)__builtin_bit_cast(_Float16, p.bias[n0 + half]);
    }
    _Float16 r0 = zl_f32_to_f16(v0), r1 = zl_f32_to_f16(v1);
    if (n0 / p.d < p.h + p.hkv) {
        const float a = (float)r0, bb = (float)r1;
        r0 = zl_f32_to_f16(__builtin_fmaf(-bb, r.s0, a * r.c0));
        r1 = zl_f32_to_f16(__builtin_fmaf(a, r.s1, bb * r.c1));
    }
    uint16_t* dst = zl_rope_dest(p, r, m, n0);
    if (dst) {
        dst[0] = __builtin_bit_cast(uint16_t, r0);
        dst[half] = __builtin_bit_cast(uint16_t, r1);
    }
}
