// w4_i8p_common.h -- what the integer-plane W4A16 kernels share (w4_i8p.hip: one launch per projection, register ring;
// w4_engine.hip: LDS-DMA loader wave + consumer waves, fused launches): the launch parameters and the wave64 DPP helpers.
#pragma once
#include "w4m_internal.h"
#include "zl_w4m_epilogue.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

struct I8Params {
    const uint16_t* x = nullptr;
    int64_t ldx = 0;
    const uint4* qw = nullptr;
    const uint32_t* meta = nullptr;
    uint32_t qw_bytes = 0, meta_bytes = 0;
    const uint16_t* bias = nullptr;
    const uint16_t* residual = nullptr;
    uint16_t* y = nullptr;
    int m = 0, n = 0, k = 0;
    int groups = 0;    // 128-k items per row tile
    int tiles = 0;     // 16-row tiles
    int epi = 0, ld_out = 0;
    const uint16_t* norm_w = nullptr;
    float norm_eps = 0.f;
    // ROPE instantiations (fused qkv projection of a decode step)
    const float* cosv = nullptr;
    const float* sinv = nullptr;
    const int32_t* placement = nullptr;
    const int32_t* buf_lens = nullptr;
    uint16_t* const* k_bufs = nullptr;
    uint16_t* const* v_bufs = nullptr;
    uint16_t* q_out = nullptr;
    int h = 0, hkv = 0, d = 0, bshd = 0;
    int pair_stride = 1;
    // MERGE instantiations (attn_out projection of a decode step): the activation rows are merged from the decode attention's
    // half-precision split partials (zl_decode_attn_splits_h: fp16 [row][head][split][128], then fp32 (max, sum) pairs)
    const uint16_t* mg_part = nullptr;
    const float* mg_stat = nullptr;
    const int32_t* mg_valid_lens = nullptr;   // with buf_lens: keys per task -> live splits
    int mg_split_len = 0, mg_max_splits = 0;
};

// the block of a problem; the qkv and the merging launches add their part
inline I8Params i8_params(const W4Problem& pb) {
    I8Params p;
    zl_w4m_fill_problem(p, pb);
    p.norm_w = pb.norm_w; p.norm_eps = pb.norm_eps;
    return p;
}
inline void i8_fill_rope(I8Params& p, const W4Rope& rp) {
    zl_w4m_fill_rope(p, rp);
    p.pair_stride = rp.d / 32;
}
inline void i8_fill_merge(I8Params& p, const W4Merge& mg) {
    p.buf_lens = mg.buf_lens;
    p.mg_part = reinterpret_cast<const uint16_t*>(mg.ws);
    p.mg_stat = reinterpret_cast<const float*>(mg.ws) + (size_t)p.m * p.groups * mg.max_splits * 64;   // behind the fp16 rows (128 halfs each)
    p.mg_valid_lens = mg.valid_lens; p.mg_split_len = mg.split_len; p.mg_max_splits = mg.max_splits;
}

// ---- DPP helpers (wave64, rows of 16 lanes) ----------------------------------------------------------------------------
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int dpp_i(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xF, false);
}
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float old, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}
// all-reduce inside each row of 16 lanes by rotations (row_ror:8,4,2,1)
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<0x128>(0.f, v);
    v += dpp_f<0x124>(0.f, v);
    v += dpp_f<0x122>(0.f, v);
    v += dpp_f<0x121>(0.f, v);
    return v;
}
__device__ __forceinline__ int row16_sum(int v) {
    v += dpp_i<0x128>(0, v);
    v += dpp_i<0x124>(0, v);
    v += dpp_i<0x122>(0, v);
    v += dpp_i<0x121>(0, v);
    return v;
}
__device__ __forceinline__ int row16_max(int v) {
    v = max(v, dpp_i<0x128>(0, v));
    v = max(v, dpp_i<0x124>(0, v));
    v = max(v, dpp_i<0x122>(0, v));
    v = max(v, dpp_i<0x121>(0, v));
    return v;
}
// sum over the 64 lanes, valid in lanes 48..63 (row_bcast15 into rows 1 / 3, row_bcast31 into rows 2 / 3)
__device__ __forceinline__ float wave_sum_hi(float v) {
    v = row16_sum(v);
    v += dpp_f<0x142, 0xA>(0.f, v);
    v += dpp_f<0x143, 0xC>(0.f, v);
    return v;
}

}  // namespace
