// decode_attn_d64.h -- what attention.hip's launchers hand to the head-size-64 matrix-core decode kernel (decode_attn_d64.hip).
#pragma once
#include "zl_common.h"

// The fields of attention.hip's launch parameters that the kernel reads, with their meaning there.  rows = len_q * (h / hkv) <= 16;
// split_len and max_splits are attn_geometry's; ws receives one fp32 (acc[64], max, sum) record per (task, query, head, split),
// k_decode_attn_partial<DT, 64, ..>'s format, which k_decode_attn_combine<DT, 64> merges.
struct DecodeD64Params {
    const uint16_t* q = nullptr;              // plain form: (b, len_q, h, 64)
    const int32_t* buf_lens = nullptr;
    const int32_t* valid_lens = nullptr;
    const uint16_t* const* k_bufs = nullptr;
    const uint16_t* const* v_bufs = nullptr;
    float* ws = nullptr;
    int b = 0, len_q = 0, h = 0, hkv = 0, n_rep = 0, rows = 0, split_len = 0, max_splits = 0, bshd = 0;
    float scale = 0.f;
    // fused form (qkv != nullptr; len_q == 1): zl_decode_attn_fused's operands
    const uint16_t* qkv = nullptr;            // (b, (h + 2 hkv) * 64)
    const float* cosv = nullptr;              // (b, 64)
    const float* sinv = nullptr;
    const int32_t* placement = nullptr;       // (b)
    uint16_t* const* k_bufs_w = nullptr;      // writable views of k_bufs / v_bufs
    uint16_t* const* v_bufs_w = nullptr;
    int neox = 1;
    // window form (window > 0; plain form only, zl_decode_attn_window): the rows of task b see the keys [max(0, elen - window), elen),
    // elen = min(buf_lens[b], valid_lens[b]); split s starts s * split_len keys behind the window's first key and max_splits counts
    // the window's splits.  max_splits == 1: the workgroup writes `out` (T, (b, len_q, h, 64)) itself, with sinks (h) fp32 or null
    int window = 0;
    const float* sinks = nullptr;
    uint16_t* out = nullptr;
};

// the partial launch alone: grid (max_splits, hkv, b), 256 threads; the caller follows it with the merge -- except in the window form
// with max_splits == 1, which leaves the finished rows in `out`
int zl_decode_attn_d64_launch(const DecodeD64Params& p, int dtype, hipStream_t st);
