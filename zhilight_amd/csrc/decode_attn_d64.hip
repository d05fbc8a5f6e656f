// decode_attn_d64.hip -- prefix-visibility decode attention for head size 64 on the matrix cores (k_decode_attn_d64; reached through
// zl_decode_attn_ex, zl_decode_attn_fused and, with a sliding window and sinks, zl_decode_attn_window, attention.hip).
//
// The arithmetic is zl_decode_attn's: out[b,q,h,:] = softmax_{j < min(buf_lens[b], valid_lens[b])}(scale * q.K_j) . V, scores in fp32, the
// running maximum starting at -1e20, probabilities rounded to T for the P.V product (the normaliser sums what the product uses), fp32
// accumulation, GQA hk = head / (h / hkv), buffers BSHD (len, Hkv, 64) or BHSD (Hkv, len, 64).  The design is for D = 64:
//
//   work split   grid (split, kv head, task) with attn_geometry's split length, the VALU route's grid.  A workgroup = 4 waves, all
//                len_q * h / hkv <= 16 query rows of its kv head in one 16-row MFMA tile.  Wave w walks the 64-key chunks
//                t0 + 64 w, t0 + 64 w + 256, .. of the split (a split is a multiple of 128 keys).  A K or V row is 128 bytes, so a
//                64-key chunk is the 8 KB of K and 8 KB of V that a 32-key chunk is at D = 128: 16 x 16 B per lane in flight per
//                register set, for one softmax step, one rescale and one wait per 64 keys instead of per 32.  The price: at the
//                shortest split, 128 keys -- attn_split_len's choice whenever max_len * b * hkv < 256 Ki, every batch-1 launch
//                measured -- only waves 0 and 1 have a chunk; waves 2 and 3 issue clamped loads (cache hits), hold their 20 KB of
//                the workgroup's LDS and only join the merge.  From 256-key splits on all four waves work, from 320 on a wave
//                walks more than one chunk.
//   scores       S^T = K . Q^T on v_mfma_f32_16x16x32: two MFMAs per 16-key block (D = 64 is two k-steps).  K fragments come
//                straight from global memory into the A operand: lane (key r = lane & 15 of the block, piece kq = lane >> 4) reads
//                the 16-byte pieces at elements 8 kq + 32 t, t = 0, 1.  Q^T is the B operand (column = query row r, same pieces).
//                C: lane (r, kq) holds the scores of QUERY r against keys 16 blk + 4 kq + i of the chunk.
//   P -> P.V     a lane's 16 scores belong to one query row; rounded to T, the 8 of a 32-key group (keys 32 g + {4 kq + i,
//                16 + 4 kq + i}) ARE the B operand of O^T += V^T . P^T -- no transposition, no LDS for P.  O^T keeps the query in
//                the lane (C: d = 16 db + 4 kq + i, query r), so the running maximum, the rescale factor and the normaliser are
//                lane-local: no strip through LDS as in the prompt kernel, whose O is row-major.
//   V            through wave-private LDS: 8 lanes load one 128-byte row as 16-byte pieces (8 rows per request, 8 requests per
//                chunk), ds_write_b128 row-major, and ds_read_b64_tr_b16 delivers the A operand V^T (row d = 16 db + r, k = the
//                group's keys in the order P uses).  The next chunk's K and V loads are issued once this chunk's K fragments are
//                consumed and its V rows are in LDS; they fly during the softmax and P.V.
//   LDS          V rows are padded to 160 bytes (40 dwords).  A transposed read takes, per half wave, 8 rows x 32 bytes: rows
//                4 kq + (r >> 2), kq = 0, 1, at dword 2 (r & 3) + 8 db.  40 row mod 64 = {0, 40, 16, 56, 32, 8, 48, 24}: eight
//                disjoint runs of 8 banks, every bank once.  (The b128 writes of two neighbouring rows, 40 dwords apart, share 8 of
//                their 32 banks; there are 8 writes per 16 reads.)  64 x 160 B x 4 waves = 40 960 bytes; the wave merge reuses it
//                with rows of 68 floats (16-byte aligned float4 stores; 68 r mod 64 = 4 r).
//   fused form   zl_decode_attn_fused: q and the new k row are pieces of the fused qkv row.  With the fragment layout above a lane
//                holds elements e (t = 0) and e + 32 (t = 1) -- both halves of a neox pair -- and both elements of an interleaved
//                pair, so the rotation (rope8's fp32 expression, one rounding to T) needs no other lane.  The workgroup whose split
//                covers placement[b] stores the rotated K row and the V row (also when the split has no visible key; only for
//                placement < len); the lanes whose fragment (K) or LDS row (V) would have held slot placement[b] take the row from
//                registers, so the launch never reads its own store.
//
// Properties: keys at or behind min(buf_lens, valid_lens) are never loaded -- addresses are clamped to the split's last visible
// key, their scores are -inf by selection and their V rows are zeroed before LDS, so NaN there cannot leak (the fused form's
// clamped reads may race its own store: they are the ones zeroed).  A task without a visible key leaves no record and the merge
// writes a zero row.  MFMA columns, softmax state and records are per query row: a row's bits do not depend on the other rows of its
// tile.  Table values only clip: valid_lens <= 0 ends the workgroup, placement outside [0, len) stores nothing.
//
// Window / sink variant (WIN != 0, zl_decode_attn_window; plain form only).  With elen = min(buf_lens, valid_lens) a task's rows see
// the keys lo <= j < elen, lo = max(0, elen - window), and an optional per-head sink logit joins the normaliser (no value row):
//   work split   RELATIVE to lo: workgroup (s, kv head, task) walks [lo + s * split_len, min(elen, lo + (s + 1) * split_len)), so the
//                grid is ceil(min(window, max_len_buf) / split_len) splits whatever the buffer's length -- scalar arguments only, the
//                launch can be captured.  A chunk starts at any key (a row is 128 bytes, every piece stays 16-byte aligned); the loads
//                start at lo, clamp at the split's last visible key as above, and nothing in front of lo is ever addressed.
//   WIN == 2     the window fits ONE split (gpt-oss: 128 keys): after the four-wave merge the workgroup takes the sink into the
//                normaliser, divides, rounds to T and stores the `out` rows itself -- no records, no merge launch.  A task without a
//                visible key gets its zero rows here.  Without a sink the bits are those of the record + merge pair (one split's
//                factor is exp(0) = 1).
//   WIN == 1     longer windows: the fp32 record goes to relative split index s; k_decode_attn_combine counts its splits from
//                elen - lo and takes the sink.
// Sinks without a window run the plain form (WIN == 0) and meet the sink in the merge.  Not covered: the fused form, the INT8
// cache, the shared-prefix and causal launches, D = 128.
#include "decode_attn_d64.h"

namespace {

constexpr int kD = 64;
constexpr int kChunk = 64;          // keys per wave step
constexpr int kWaves = 4;
constexpr int kVRow = kD + 16;      // V staging row (halfs): 160 B
constexpr int kXRow = kD + 4;       // wave-merge row (floats): acc[64], max, sum, pad

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

template <int DT>
__device__ __forceinline__ f4 dd64_mfma(uint4 a, uint4 b, f4 c) {
    typedef __bf16 b8 __attribute__((ext_vector_type(8)));
    if constexpr (DT == ZL_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
}

template <int DT>
__device__ __forceinline__ uint16_t dd64_round(float x) {      // a probability in [0, 1] -> T, nearest even
    if constexpr (DT == ZL_F16) return __builtin_bit_cast(uint16_t, (_Float16)x);
    else {
        const uint32_t u = __builtin_bit_cast(uint32_t, x);
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
}

template <int DT>
__device__ __forceinline__ void dd64_unpack(const uint4& v, float (&f)[8]) {
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = ZT<DT>::to_f32((uint16_t)(u[e] & 0xffff));
        f[2 * e + 1] = ZT<DT>::to_f32((uint16_t)(u[e] >> 16));
    }
}

__device__ __forceinline__ void dd64_load8(const float* src, float (&f)[8]) {
    const float4 a = reinterpret_cast<const float4*>(src)[0], b = reinterpret_cast<const float4*>(src)[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// rotate a lane's two pieces of a head row in place: x[0] = elements e0 .. e0 + 7 (e0 < 32), x[1] = elements e0 + 32 .. e0 + 39, with
// the cos / sin of those elements.  The fp32 expression of attention.hip's rope8 (rope_one_value), one rounding to T.
template <int DT>
__device__ __forceinline__ void dd64_rope(uint4 (&x)[2], const float (&c)[2][8], const float (&s)[2][8], int neox) {
    float f[2][8];
    dd64_unpack<DT>(x[0], f[0]);
    dd64_unpack<DT>(x[1], f[1]);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            float r[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int i = e + u;
                // neox: the pair is (e, e + 32), the low half subtracts; interleaved: (2 j, 2 j + 1), the even one subtracts
                const bool minus = neox ? t == 0 : (i & 1) == 0;
                const float partner = neox ? f[t ^ 1][i] : f[t][i ^ 1];
                r[u] = minus ? __builtin_fmaf(-partner, s[t][i], f[t][i] * c[t][i]) : __builtin_fmaf(partner, s[t][i], f[t][i] * c[t][i]);
            }
            o[e / 2] = (uint32_t)ZT<DT>::from_f32(r[0]) | ((uint32_t)ZT<DT>::from_f32(r[1]) << 16);
        }
        x[t] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// (FUSE: three workgroups per CU instead of the four that LDS allows -- the new row's 12 registers and the injection took the loop
// past the plain form's 128-register budget and into scratch; its first V loads go out behind the rotation for the same reason)
template <int DT, bool FUSE, int WIN = 0>
__global__ __launch_bounds__(64 * kWaves, FUSE ? 3 : 4) void k_decode_attn_d64(const DecodeD64Params p) {
    static_assert(!(FUSE && WIN), "the window form has no fused front end");
    __shared__ __attribute__((aligned(16))) uint16_t vs[kWaves][kChunk * kVRow];     // 10 KB per wave; reused for the wave merge

    const int b = blockIdx.z, hk = blockIdx.y, split = blockIdx.x;
    // the scalar inputs first: one level of dependent loads
    const int len = p.buf_lens[b];
    const int vlen = p.valid_lens[b];
    const uint16_t* kbase = p.k_bufs[b];
    const uint16_t* vbase = p.v_bufs[b];
    const int place = FUSE ? p.placement[b] : -1;
    const int elen = min(len, vlen);
    // WIN: the split counts from the window's first key
    const int t0 = (WIN && elen > p.window ? elen - p.window : 0) + split * p.split_len;
    // FUSE: the workgroup whose split covers the new token's slot stores it even when nothing of the split is visible
    const bool owns_new = FUSE && place >= t0 && place < t0 + p.split_len && place < len;
    if (len <= 0 || (t0 >= elen && !owns_new)) {
        if constexpr (WIN == 2) {                         // no merge launch behind this one: the task's zero rows (workgroup-uniform)
            for (int idx = threadIdx.x; idx < p.rows * kD; idx += 64 * kWaves) {
                const int i = idx / kD, head = hk * p.n_rep + i % p.n_rep;
                p.out[(((size_t)b * p.len_q + i / p.n_rep) * p.h + head) * kD + idx % kD] = 0;
            }
        }
        return;
    }
    const int t1 = min(elen, t0 + p.split_len);
    const int last_key = t1 > 0 ? t1 - 1 : 0;             // 0 <= last_key < len

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;               // MFMA: key of a block / query row; 16-byte piece
    const int vrow = lane >> 3, vpc = (lane & 7) * 8;      // V staging: row of a request, element of the piece
    const size_t kv_stride = p.bshd ? (size_t)p.hkv * kD : (size_t)kD;
    const size_t kv_off = p.bshd ? (size_t)hk * kD : (size_t)hk * len * kD;

    // ---- the wave's first chunk goes out before anything else.  Clamped, branch-free: past the split's last visible key the loads
    //      re-read that key's row
    uint4 kk[4][2], vv[8];
#define ZL_DD64_LOAD_K(base)                                                                                       \
    _Pragma("unroll") for (int blk_ = 0; blk_ < 4; ++blk_) {                                                      \
        const int key_ = (base) + 16 * blk_ + r;                                                                  \
        const uint16_t* src_ = kbase + kv_off + (size_t)(key_ < last_key ? key_ : last_key) * kv_stride + 8 * kq; \
        kk[blk_][0] = *reinterpret_cast<const uint4*>(src_);                                                      \
        kk[blk_][1] = *reinterpret_cast<const uint4*>(src_ + 32);                                                 \
    }
#define ZL_DD64_LOAD_V(base)                                                                                       \
    _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) {                                                            \
        const int key_ = (base) + 8 * j_ + vrow;                                                                  \
        vv[j_] = *reinterpret_cast<const uint4*>(vbase + kv_off + (size_t)(key_ < last_key ? key_ : last_key) * kv_stride + vpc); \
    }
    const int c0 = t0 + wave * kChunk;
    ZL_DD64_LOAD_K(c0)
    if constexpr (!FUSE) ZL_DD64_LOAD_V(c0)               // FUSE: behind the rotation, which needs the registers

    // ---- Q^T fragments (B operand): column = query row r -> (qi, head), pieces 8 kq + 32 t; rows beyond the tile's are zero
    uint4 qf[2];
    uint4 k_new[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)}, v_new = make_uint4(0, 0, 0, 0);
    {
        const bool live = r < p.rows;
        const int rr = live ? r : 0;
        const int head = hk * p.n_rep + rr % p.n_rep;
        if constexpr (FUSE) {
            float c[2][8], s[2][8];
            dd64_load8(p.cosv + (size_t)b * kD + 8 * kq, c[0]);
            dd64_load8(p.cosv + (size_t)b * kD + 8 * kq + 32, c[1]);
            dd64_load8(p.sinv + (size_t)b * kD + 8 * kq, s[0]);
            dd64_load8(p.sinv + (size_t)b * kD + 8 * kq + 32, s[1]);
            const uint16_t* row = p.qkv + (size_t)b * (p.h + 2 * p.hkv) * kD;
            const uint16_t* qp = row + (size_t)head * kD + 8 * kq;
            qf[0] = *reinterpret_cast<const uint4*>(qp);
            qf[1] = *reinterpret_cast<const uint4*>(qp + 32);
            dd64_rope<DT>(qf, c, s, p.neox);
            const uint16_t* kp = row + (size_t)(p.h + hk) * kD + 8 * kq;
            k_new[0] = *reinterpret_cast<const uint4*>(kp);
            k_new[1] = *reinterpret_cast<const uint4*>(kp + 32);
            dd64_rope<DT>(k_new, c, s, p.neox);
            v_new = *reinterpret_cast<const uint4*>(row + (size_t)(p.h + p.hkv + hk) * kD + vpc);
            // copy_to_rag_buffer2: the K row from the four lanes of key 0's fragment, the V row from the eight lanes of staging row 0
            if (owns_new && wave == 0) {
                if (r == 0) {
                    uint16_t* kd = p.k_bufs_w[b] + kv_off + (size_t)place * kv_stride + 8 * kq;
                    *reinterpret_cast<uint4*>(kd) = k_new[0];
                    *reinterpret_cast<uint4*>(kd + 32) = k_new[1];
                }
                if (vrow == 0) *reinterpret_cast<uint4*>(p.v_bufs_w[b] + kv_off + (size_t)place * kv_stride + vpc) = v_new;
            }
            if (t0 >= elen) return;                       // workgroup-uniform, before any barrier: nothing visible in this split
            ZL_DD64_LOAD_V(c0)
        } else {
            const uint16_t* qp = p.q + (((size_t)b * p.len_q + rr / p.n_rep) * p.h + head) * kD + 8 * kq;
            qf[0] = *reinterpret_cast<const uint4*>(qp);
            qf[1] = *reinterpret_cast<const uint4*>(qp + 32);
        }
        if (!live) qf[0] = qf[1] = make_uint4(0, 0, 0, 0);
    }

    f4 o[4];                                              // O^T: d = 16 db + 4 kq + i, query r
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = (f4){0.f, 0.f, 0.f, 0.f};
    float m_run = -1e20f, l_run = 0.f;                    // of query r, replicated over kq (l: this lane's share of the sum)
    uint16_t* vdst = vs[wave] + vrow * kVRow + vpc;
    const uint16_t* vtr = vs[wave] + (4 * kq + (r >> 2)) * kVRow + 4 * (r & 3);      // transposed-read address of this lane
    typedef short s4 __attribute__((ext_vector_type(4)));
    typedef short s8 __attribute__((ext_vector_type(8)));

    for (int cur = c0; cur < t1; cur += kWaves * kChunk) {
        if constexpr (FUSE) {                             // the row this launch stores: from registers, never from memory
#pragma unroll
            for (int blk = 0; blk < 4; ++blk)
                if (cur + 16 * blk + r == place) {
                    kk[blk][0] = k_new[0];
                    kk[blk][1] = k_new[1];
                }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (cur + 8 * j + vrow == place) vv[j] = v_new;
        }
        if (cur + kChunk > t1) {                          // wave-uniform: the split's last, partial chunk
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (cur + 8 * j + vrow >= t1) vv[j] = make_uint4(0, 0, 0, 0);       // probability 0 times a finite row
        }
        // ---- S^T = K . Q^T
        f4 st[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            st[blk] = dd64_mfma<DT>(kk[blk][0], qf[0], (f4){0.f, 0.f, 0.f, 0.f});
            st[blk] = dd64_mfma<DT>(kk[blk][1], qf[1], st[blk]);
        }
        // ---- the V chunk to LDS, row-major; then the wave's next chunk
#pragma unroll
        for (int j = 0; j < 8; ++j) *reinterpret_cast<uint4*>(vdst + 8 * j * kVRow) = vv[j];
        ZL_DD64_LOAD_K(cur + kWaves * kChunk)
        ZL_DD64_LOAD_V(cur + kWaves * kChunk)
        // ---- online softmax of query r over this lane's 16 keys and the row's three other lanes
        float mloc = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float sv = cur + 16 * blk + 4 * kq + i < t1 ? st[blk][i] * p.scale : -INFINITY;
                st[blk][i] = sv;
                mloc = fmaxf(mloc, sv);
            }
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        const float m_new = fmaxf(m_run, mloc);
        const float alpha = __expf(m_run - m_new);
        m_run = m_new;
        uint32_t pw[8];
        float lsum = 0.f;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
#pragma unroll
            for (int i2 = 0; i2 < 2; ++i2) {
                const uint16_t p0 = dd64_round<DT>(__expf(st[blk][2 * i2] - m_new));
                const uint16_t p1 = dd64_round<DT>(__expf(st[blk][2 * i2 + 1] - m_new));
                lsum += ZT<DT>::to_f32(p0) + ZT<DT>::to_f32(p1);
                pw[2 * blk + i2] = (uint32_t)p0 | ((uint32_t)p1 << 16);
            }
        }
        l_run = l_run * alpha + lsum;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            o[db][0] *= alpha; o[db][1] *= alpha; o[db][2] *= alpha; o[db][3] *= alpha;
        }
        // ---- O^T += V^T . P^T per 32-key group g: B = the lane's probabilities of blocks 2 g and 2 g + 1, A = two transposed reads
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint4 pf = make_uint4(pw[4 * g], pw[4 * g + 1], pw[4 * g + 2], pw[4 * g + 3]);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(vtr + (32 * g) * kVRow + 16 * db));
                const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(vtr + (32 * g + 16) * kVRow + 16 * db));
                const s8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                o[db] = dd64_mfma<DT>(__builtin_bit_cast(uint4, a), pf, o[db]);
            }
        }
    }
#undef ZL_DD64_LOAD_K
#undef ZL_DD64_LOAD_V

    // ---- merge: a row's normaliser lives in 4 lanes; then the waves through LDS (over the V staging).  A wave without a chunk
    //      contributes (0, -1e20, 0), which the merge weighs with exp(-1e20 - m) = 0
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    __syncthreads();
    float* xw = reinterpret_cast<float*>(&vs[0][0]);       // [wave][16 rows][kXRow]
    if (r < p.rows) {
        float* dst = xw + ((size_t)wave * 16 + r) * kXRow;
#pragma unroll
        for (int db = 0; db < 4; ++db) *reinterpret_cast<f4*>(dst + 16 * db + 4 * kq) = o[db];
        if (kq == 0) {
            dst[kD] = m_run;
            dst[kD + 1] = l_run;
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < p.rows * kD; idx += 64 * kWaves) {
        const int i = idx / kD, d = idx % kD;
        const float* src = xw + (size_t)i * kXRow;
        constexpr int WS = 16 * kXRow;
        float mn = src[kD];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) mn = fmaxf(mn, src[w * WS + kD]);
        float a = 0.f, lt = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const float f = __expf(src[w * WS + kD] - mn);
            a = __builtin_fmaf(src[w * WS + d], f, a);
            lt = __builtin_fmaf(src[w * WS + kD + 1], f, lt);
        }
        const int qi = i / p.n_rep, head = hk * p.n_rep + i % p.n_rep;
        if constexpr (WIN == 2) {
            // the only split: m = max(max_j s_j, sink), out = sum p V / (sum p + exp(sink - m) + 1e-20); no sink: f = 1, the pair's bits
            const float sink = p.sinks ? p.sinks[head] : -INFINITY;
            const float m2 = fmaxf(mn, sink);
            const float f = __expf(mn - m2);
            p.out[(((size_t)b * p.len_q + qi) * p.h + head) * kD + d] = ZT<DT>::from_f32(a * f / (lt * f + __expf(sink - m2) + 1e-20f));
            continue;
        }
        float* dst = p.ws + ((((size_t)b * p.len_q + qi) * p.h + head) * p.max_splits + split) * (kD + 2);
        dst[d] = a;
        if (d == 0) {
            dst[kD] = mn;
            dst[kD + 1] = lt;
        }
    }
}

}  // namespace

int zl_decode_attn_d64_launch(const DecodeD64Params& p, int dtype, hipStream_t st) {
    const dim3 grid((unsigned)p.max_splits, (unsigned)p.hkv, (unsigned)p.b), block(64 * kWaves);
    if (p.window > 0) {                                   // max_splits counts the window's splits; one split: the direct form
        if (p.qkv) return ZL_EINVAL;
        if (p.max_splits == 1) {
            if (dtype == ZL_F16) hipLaunchKernelGGL((k_decode_attn_d64<ZL_F16, false, 2>), grid, block, 0, st, p);
            else hipLaunchKernelGGL((k_decode_attn_d64<ZL_BF16, false, 2>), grid, block, 0, st, p);
        } else {
            if (dtype == ZL_F16) hipLaunchKernelGGL((k_decode_attn_d64<ZL_F16, false, 1>), grid, block, 0, st, p);
            else hipLaunchKernelGGL((k_decode_attn_d64<ZL_BF16, false, 1>), grid, block, 0, st, p);
        }
    } else if (p.qkv) {
        if (dtype == ZL_F16) hipLaunchKernelGGL((k_decode_attn_d64<ZL_F16, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((k_decode_attn_d64<ZL_BF16, true>), grid, block, 0, st, p);
    } else {
        if (dtype == ZL_F16) hipLaunchKernelGGL((k_decode_attn_d64<ZL_F16, false>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((k_decode_attn_d64<ZL_BF16, false>), grid, block, 0, st, p);
    }
    return zl_launch_status();
}
