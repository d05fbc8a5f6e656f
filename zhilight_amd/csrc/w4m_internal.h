// w4m_internal.h -- the host side of the W4A16 matrix-core family: what the dispatcher (w4_mfma.hip) hands to the launchers that
// live in the other files (w4_phase / w4_slab / w4_i8p .hip; tools/experimental/w4_engine.hip in the experimental build).  The
// dispatcher and the file that defines a launcher both include this header, so the compiler checks that they agree.
#pragma once
#include "zl_common.h"

// one projection y (m, n) = x (m, k) . W^T in the ZLW4M layout.  The dispatcher has checked the pointers and that the packed
// weights stay below 4 GiB (32-bit buffer offsets) before a launcher sees this.
struct W4Problem {
    const uint16_t* x;
    int64_t ldx;
    const uint32_t* qw;
    const uint32_t* meta;
    uint32_t qw_bytes, meta_bytes;
    const uint16_t* bias;
    const uint16_t* residual;
    uint16_t* y;
    int m, n, k;
    int groups;        // 128-k items per row tile
    int tiles;         // 16-row tiles
    int epilogue, ld_out;
    const uint16_t* norm_w;
    float norm_eps;
};

// the fused qkv projection of a decode step: neox tables (m, d), the tasks' slots and buffers, q's own buffer (m, h * d)
struct W4Rope {
    const float* cosv;
    const float* sinv;
    const int32_t* placement;
    const int32_t* buf_lens;
    uint16_t* const* k_bufs;
    uint16_t* const* v_bufs;
    uint16_t* q_out;
    int h, hkv, d, bshd;
};

// the attention output projection of a decode step reading the decode attention's split partials instead of merged rows
struct W4Merge {
    const void* ws;
    const int32_t* buf_lens;
    const int32_t* valid_lens;
    int split_len, max_splits;
};

// the problem of a layout: ld_out = n, or n / 2 for the gated epilogues
inline W4Problem zl_w4m_problem(const zl_w4_layout_t& L, const uint16_t* x, int64_t ldx, const uint32_t* qw, const uint32_t* meta,
                                const uint16_t* bias, const uint16_t* residual, uint16_t* y, int64_t m, int epilogue,
                                const uint16_t* norm_w, float norm_eps) {
    const bool silu = epilogue & (ZL_EPI_SILU_MUL | ZL_EPI_SILU_MUL_F32);
    return {x, ldx, qw, meta, (uint32_t)L.qw_bytes, (uint32_t)L.scales_bytes, bias, residual, y, (int)m, (int)L.n, (int)L.k,
            (int)L.q, (int)(L.np / 16), epilogue, (int)(silu ? L.n / 2 : L.n), norm_w, norm_eps};
}

// the fields every kernel parameter block of the family names alike
template <class P>
void zl_w4m_fill_problem(P& p, const W4Problem& pb) {
    p.x = pb.x; p.ldx = pb.ldx; p.qw = reinterpret_cast<const uint4*>(pb.qw); p.meta = pb.meta; p.qw_bytes = pb.qw_bytes;
    p.meta_bytes = pb.meta_bytes; p.bias = pb.bias; p.residual = pb.residual; p.y = pb.y; p.m = pb.m; p.n = pb.n; p.k = pb.k;
    p.groups = pb.groups; p.tiles = pb.tiles; p.epi = pb.epilogue; p.ld_out = pb.ld_out;
}
template <class P>
void zl_w4m_fill_rope(P& p, const W4Rope& rp) {
    p.cosv = rp.cosv; p.sinv = rp.sinv; p.placement = rp.placement; p.buf_lens = rp.buf_lens; p.k_bufs = rp.k_bufs;
    p.v_bufs = rp.v_bufs; p.q_out = rp.q_out; p.h = rp.h; p.hkv = rp.hkv; p.d = rp.d; p.bshd = rp.bshd;
}
// a qkv problem: n = (h + 2 hkv) d in whole tiles, d / 32 tiles between a column and its rotation partner
inline bool zl_w4m_rope_shape_ok(const W4Problem& pb, const W4Rope& rp) {
    return rp.d % 32 == 0 && pb.n == (rp.h + 2 * rp.hkv) * rp.d && pb.tiles * 16 == pb.n;
}

inline const zl_w4_opts_t& zl_w4_opts_or_default(const zl_w4_opts_t* opts) {
    static const zl_w4_opts_t kNoOpts = {};
    return opts ? *opts : kNoOpts;
}

// ---- launchers.  ZL_ESHAPE = not this launcher's shape (the dispatcher takes its next route where it has one)
// w4_phase.hip: the phase-pipelined streaming kernel, 1..32 rows
int zl_w4a16_gemm_phase(const W4Problem& pb, const zl_w4_opts_t* opts, hipStream_t hs);
int zl_w4a16_gemm_phase_rope(const W4Problem& pb, const W4Rope& rp, hipStream_t hs);
int zl_w4a16_gemm_phase_merge(const W4Problem& pb, const W4Merge& mg, hipStream_t hs);      // fp32 partials (zl_decode_attn_splits)
// w4_slab.hip: 128-column x K-slice tiles; also ZL_ESHAPE without scratch for the K split
int zl_w4a16_gemm_slab(const W4Problem& pb, const zl_w4_opts_t* opts, hipStream_t hs);
int zl_w4a16_gemm_slab_rope(const W4Problem& pb, const W4Rope& rp, const zl_w4_opts_t* opts, hipStream_t hs);
// w4_i8p.hip: the integer-plane kernel, 1..4 rows
bool zl_w4a16_i8p_covers(int64_t m, int64_t k);
int zl_w4a16_gemm_i8p(const W4Problem& pb, int rounds_override, hipStream_t hs);
int zl_w4a16_gemm_i8p_rope(const W4Problem& pb, const W4Rope& rp, hipStream_t hs);
int zl_w4a16_gemm_i8p_merge(const W4Problem& pb, const W4Merge& mg, hipStream_t hs);        // fp16 partials (zl_decode_attn_splits_h)
#ifdef ZL_EXPERIMENTAL
// w4_engine.hip: the loader / consumer engine
bool zl_w4_engine_covers(int64_t m, int64_t k, int r);
int zl_w4a16_gemm_engine(const W4Problem& pb, int slots_cap, hipStream_t hs);
int zl_w4a16_gemm_engine_rope(const W4Problem& pb, const W4Rope& rp, hipStream_t hs);
int zl_w4a16_gemm_engine_merge(const W4Problem& pb, const W4Merge& mg, hipStream_t hs);
// attn_out (pb1 + mg; y = the hidden rows, updated in place) and gate|up (pb2; x = those rows) in one launch
int zl_w4_engine_o_gateup_launch(const W4Problem& pb1, const W4Merge& mg, const W4Problem& pb2, void* granules, const uint32_t* epoch_ptr,
                                 uint32_t epoch_add, uint32_t* err, hipStream_t hs);
int zl_engine_epoch_advance_launch(uint32_t* epoch, uint32_t by, hipStream_t hs);
// w4_phase.hip: the digit-plane instantiations (5..32 rows); pb.x is unused, the activations arrive as planes
int64_t zl_w4_planes_bytes_(int64_t m, int64_t k);
int zl_w4_planes_launch(const uint16_t* x, int64_t ldx, int m, int k, const uint16_t* norm_w, float norm_eps, void* planes, hipStream_t hs);
int zl_w4a16_gemm_phase_planes(const void* planes, const W4Problem& pb, const zl_w4_opts_t* opts, hipStream_t hs);
int zl_w4a16_gemm_phase_planes_rope(const void* planes, const W4Problem& pb, const W4Rope& rp, hipStream_t hs);
#endif
