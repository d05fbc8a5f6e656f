// zl_mxfp4.h -- what the MXFP4 kernels share (mxfp4.hip: fp16 / bf16 activations; mxfp4_a8.hip: MXFP8 activations): the launch
// parameters and the epilogues of zl_w4a16 (include/zhilight_amd.h) for either T.
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

// v: the fp32 sum of output (m, n)
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

// the outputs of one 16 x 16 MFMA tile, lane (nrow = lane % 16, kq = lane / 16): rows m0 + 4 kq + i, column n.  Gated: columns pair
// up across lanes n, n ^ 1 (n even = gate); every lane of the wave must call it
template <int DT, class V>
__device__ __forceinline__ void mx_store_tile(const Mx4Params& p, int m0, int n, int kq, const V& v) {
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
