// kv_blocks.hip -- block copies between the per-task ragged K/V buffers and a prefix-cache pool (zl_kv_blocks_copy).
//
// One launch moves, for every descriptor (task, first slot, pool block), every layer and both K and V, `block` rows of the task's
// buffer into the pool block or back.  A (descriptor, layer, K/V) slice is one contiguous run of block * hkv * row_bytes bytes
// under BSHD and hkv runs of block * row_bytes under BHSD, on BOTH sides: the pool keeps the buffers' layout inside a block, so a
// run is a plain byte copy.  The runs are cut into pieces of a fixed size and the pieces go to workgroups through a flat index.
#include "zl_common.h"

#define ZL_KVB_THREADS 256
#define ZL_KVB_UNROLL 4                                                   // up to 4 16-byte loads outstanding per lane and pass
// the default piece: 8 KiB, two loads per lane all issued before the first store.  Measured at Llama-3-8B geometry
// (tools/bench_prefix_cache.py (e), profiles/prefix_cache.txt, DESIGN 4 "Prefix cache"): 8 KiB is the fastest or tied at 1 and at 7
// blocks in both directions, 4 KiB is clearly slower, 16 / 32 / 64 KiB are at most 14 % behind
#define ZL_KVB_PIECE 8192

// TO_POOL: buffers -> pool, else pool -> buffers.  The pool side is streamed (non-temporal: a block is read or written once per
// call), the buffer side uses the default policy: a loaded prefix is read by the prompt attention right behind this launch, a
// saved one was written by it right before.
template <bool TO_POOL>
__global__ void __launch_bounds__(ZL_KVB_THREADS)
k_kv_blocks_copy(const int32_t* __restrict__ desc, unsigned char* const* __restrict__ k_bufs, unsigned char* const* __restrict__ v_bufs,
                 const int32_t* __restrict__ buf_lens, unsigned char* __restrict__ pool, int layers, int b, int block, int hkv,
                 int row_bytes, int bshd, int64_t run_bytes, int piece_bytes, int pieces_per_run) {
    // flat index -> (descriptor, layer, K/V, [head under BHSD], piece); the run index inside a descriptor is the pool's own order
    const int runs_per_slice = bshd ? 1 : hkv;
    int64_t w = blockIdx.x;
    const int piece = (int)(w % pieces_per_run);
    w /= pieces_per_run;
    const int runs_per_desc = layers * 2 * runs_per_slice;
    const int run = (int)(w % runs_per_desc);
    const int di = (int)(w / runs_per_desc);
    const int head = run % runs_per_slice, kv = (run / runs_per_slice) & 1, layer = run / (2 * runs_per_slice);

    const int task = desc[di * 3 + 0], slot = desc[di * 3 + 1], pb = desc[di * 3 + 2];
    if (task < 0 || task >= b || slot < 0 || pb < 0) return;
    const int64_t len_buf = buf_lens[task];
    if ((int64_t)slot + block > len_buf) return;                          // never a stray access: the wrapper refuses these
    unsigned char* buf = (kv ? v_bufs : k_bufs)[(size_t)layer * b + task];
    buf += (bshd ? (size_t)slot * hkv : (size_t)head * len_buf + slot) * row_bytes;
    unsigned char* pl = pool + ((size_t)pb * runs_per_desc + run) * run_bytes;

    const int64_t begin = (int64_t)piece * piece_bytes;
    const int len = (int)(run_bytes - begin < piece_bytes ? run_bytes - begin : piece_bytes);
    const unsigned char* src = (TO_POOL ? buf : pl) + begin;
    unsigned char* dst = (TO_POOL ? pl : buf) + begin;

    if ((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)run_bytes) & 15) == 0) {       // piece_bytes % 16 == 0: begin and len follow
        const u32x4* s16 = reinterpret_cast<const u32x4*>(src);
        u32x4* d16 = reinterpret_cast<u32x4*>(dst);
        const int nvec = len >> 4;
        for (int i0 = threadIdx.x; i0 < nvec; i0 += ZL_KVB_THREADS * ZL_KVB_UNROLL) {
            u32x4 v[ZL_KVB_UNROLL];
#pragma unroll
            for (int u = 0; u < ZL_KVB_UNROLL; ++u) {
                const int i = i0 + u * ZL_KVB_THREADS;
                if (i < nvec) v[u] = TO_POOL ? s16[i] : __builtin_nontemporal_load(s16 + i);
            }
#pragma unroll
            for (int u = 0; u < ZL_KVB_UNROLL; ++u) {
                const int i = i0 + u * ZL_KVB_THREADS;
                if (i < nvec) {
                    if (TO_POOL) __builtin_nontemporal_store(v[u], d16 + i);
                    else d16[i] = v[u];
                }
            }
        }
    } else {                                                               // row_bytes % 4 == 0 and 4-byte aligned bases
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
        const int nw = len >> 2;
        for (int i0 = threadIdx.x; i0 < nw; i0 += ZL_KVB_THREADS * ZL_KVB_UNROLL) {
            uint32_t v[ZL_KVB_UNROLL];
#pragma unroll
            for (int u = 0; u < ZL_KVB_UNROLL; ++u) {
                const int i = i0 + u * ZL_KVB_THREADS;
                if (i < nw) v[u] = s4[i];
            }
#pragma unroll
            for (int u = 0; u < ZL_KVB_UNROLL; ++u) {
                const int i = i0 + u * ZL_KVB_THREADS;
                if (i < nw) d4[i] = v[u];
            }
        }
    }
}

int zl_kv_blocks_copy_ex(const int32_t* desc, int64_t n, void* const* k_bufs, void* const* v_bufs, const int32_t* buf_lens, void* pool,
                         int64_t layers, int64_t b, int64_t block, int64_t hkv, int64_t row_bytes, int bshd, int to_pool,
                         int64_t piece_bytes, zl_stream_t s) {
    ZL_CHECK_ARG(n >= 0 && layers > 0 && b > 0 && block > 0 && hkv > 0 && row_bytes > 0 && piece_bytes >= 0, ZL_EINVAL);
    if (n == 0) return ZL_OK;
    ZL_CHECK_ARG(desc && k_bufs && v_bufs && buf_lens && pool, ZL_EINVAL);
    if (piece_bytes == 0) piece_bytes = ZL_KVB_PIECE;
    ZL_CHECK_ARG(row_bytes % 4 == 0 && piece_bytes % 16 == 0 && ((uintptr_t)pool & 3) == 0, ZL_ESHAPE);
    const int64_t i31 = ((int64_t)1 << 31) - 1;
    ZL_CHECK_ARG(layers <= 65535 && hkv <= 65535 && b <= i31 && block <= i31 && row_bytes < ((int64_t)1 << 30) && piece_bytes <= ((int64_t)1 << 30) &&
                 n <= i31 / 3, ZL_ELIMIT);
    const int64_t runs_per_desc = layers * 2 * (bshd ? 1 : hkv);
    ZL_CHECK_ARG(block * row_bytes <= ((int64_t)1 << 40) / hkv && runs_per_desc <= i31, ZL_ELIMIT);
    const int64_t run_bytes = block * row_bytes * (bshd ? hkv : 1);
    const int64_t pieces = (run_bytes + piece_bytes - 1) / piece_bytes;
    ZL_CHECK_ARG(pieces <= i31 && n * runs_per_desc <= i31 / pieces, ZL_ELIMIT);
    const dim3 grid((unsigned)(n * runs_per_desc * pieces)), tb(ZL_KVB_THREADS);
    if (to_pool)
        hipLaunchKernelGGL(k_kv_blocks_copy<true>, grid, tb, 0, (hipStream_t)s, desc, (unsigned char* const*)k_bufs, (unsigned char* const*)v_bufs,
                           buf_lens, (unsigned char*)pool, (int)layers, (int)b, (int)block, (int)hkv, (int)row_bytes, bshd, run_bytes,
                           (int)piece_bytes, (int)pieces);
    else
        hipLaunchKernelGGL(k_kv_blocks_copy<false>, grid, tb, 0, (hipStream_t)s, desc, (unsigned char* const*)k_bufs, (unsigned char* const*)v_bufs,
                           buf_lens, (unsigned char*)pool, (int)layers, (int)b, (int)block, (int)hkv, (int)row_bytes, bshd, run_bytes,
                           (int)piece_bytes, (int)pieces);
    return zl_launch_status();
}

int zl_kv_blocks_copy(const int32_t* desc, int64_t n, void* const* k_bufs, void* const* v_bufs, const int32_t* buf_lens, void* pool,
                      int64_t layers, int64_t b, int64_t block, int64_t hkv, int64_t row_bytes, int bshd, int to_pool, zl_stream_t s) {
    return zl_kv_blocks_copy_ex(desc, n, k_bufs, v_bufs, buf_lens, pool, layers, b, block, hkv, row_bytes, bshd, to_pool, 0, s);
}
