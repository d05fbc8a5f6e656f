// kv_fork.hip -- fork a prefilled task: copy its first rows into other tasks' ragged K/V buffers and hand every task of the group its
// pending token (zl_kv_fork).
//
// One launch moves, for every descriptor (src, dst, rows, token), every layer and both K and V, rows [0, rows) of the source task's
// buffer into the destination task's.  A (descriptor, layer, K/V) slice is one contiguous run of rows * hkv * row_bytes bytes under
// BSHD and hkv runs of rows * row_bytes under BHSD, whose head stride is each side's OWN buffer length (the buffers are ragged).  The
// runs are cut into pieces of a fixed size; the flat workgroup index is sized from max_rows and a workgroup past the end of a shorter
// descriptor's run exits.  The descriptor is the FASTEST digit of the index and the index is dealt to the XCDs in contiguous chunks, so
// the workgroups that read one source piece (one per destination of that source, neighbours in the caller's descriptor order) run
// side by side behind one L2: the piece comes from HBM once and from that L2 for the other destinations.
#include "zl_common.h"

#define ZL_KVF_THREADS 256
#define ZL_KVF_UNROLL 4                                                   // up to 4 16-byte loads outstanding per lane and pass
// the default piece: 16 KiB, one pass of four loads per lane, all issued before the first store.  Measured at Llama-3-8B geometry
// (tools/bench_fork.py (b), profiles/kv_fork.txt, DESIGN 4 "Forked samples"): at 4 and 8 KiB the launch is bound by the rate at which
// workgroups are dispatched (about 1.7 ns each: the time doubles as the piece halves), from 16 KiB on by the memory; 16 KiB is the
// fastest or tied at 1 and at 7 destinations
#define ZL_KVF_PIECE 16384
#define ZL_KVF_XCDS 8                                                     // workgroups w and w + 8 share an XCD's L2 (observed, speed only)

// The source piece is loaded with the default policy (its neighbours read it again), the destination is stored non-temporally: it is
// written once per call and must not push the shared source lines out on its way.
__global__ void __launch_bounds__(ZL_KVF_THREADS)
k_kv_fork(const int32_t* __restrict__ desc, int n, unsigned char* const* __restrict__ k_bufs, unsigned char* const* __restrict__ v_bufs,
          const int32_t* __restrict__ buf_lens, int layers, int b, int max_rows, int hkv, int row_bytes, int bshd, int piece_bytes,
          int pieces_per_run, int64_t total, int32_t* __restrict__ tokens, int32_t* __restrict__ positions,
          int32_t* __restrict__ placement, int32_t* __restrict__ valid_lens) {
    // the grid is 8 chunks of `chunk` workgroups: workgroup w works on logical index (w % 8) * chunk + w / 8, so that one XCD gets a
    // contiguous stretch of the logical order; a wrong guess about the placement is slower, never wrong
    const int64_t chunk = (int64_t)gridDim.x / ZL_KVF_XCDS;
    int64_t w = (int64_t)(blockIdx.x % ZL_KVF_XCDS) * chunk + blockIdx.x / ZL_KVF_XCDS;
    if (w >= total) return;
    // logical index -> (layer, K/V, [head under BHSD], piece, descriptor), the descriptor fastest
    const int di = (int)(w % n);
    w /= n;
    const int piece = (int)(w % pieces_per_run);
    const int run = (int)(w / pieces_per_run);
    const int runs_per_slice = bshd ? 1 : hkv;
    const int head = run % runs_per_slice, kv = (run / runs_per_slice) & 1, layer = run / (2 * runs_per_slice);

    const int src = desc[di * 4 + 0], dst = desc[di * 4 + 1], rows = desc[di * 4 + 2], token = desc[di * 4 + 3];
    if (src < 0 || src >= b || dst < 0 || dst >= b || rows < 0 || rows > max_rows) return;      // dropped whole, before any table access
    const int64_t len_src = buf_lens[src], len_dst = buf_lens[dst];
    if (rows > len_src || rows > len_dst) return;

    if (tokens && run == 0 && piece == 0 && threadIdx.x == 0) {              // exactly one thread writes a descriptor's four words
        if (src != dst) {
            positions[dst] = positions[src];
            placement[dst] = placement[src];
            valid_lens[dst] = valid_lens[src];
            tokens[dst] = token >= 0 ? token : tokens[src];
        } else if (token >= 0) {
            tokens[src] = token;
        }
    }
    if (src == dst) return;

    const int64_t run_bytes = (int64_t)rows * row_bytes * (bshd ? hkv : 1);
    const int64_t begin = (int64_t)piece * piece_bytes;
    if (begin >= run_bytes) return;                                          // a shorter descriptor than max_rows
    const int len = (int)(run_bytes - begin < piece_bytes ? run_bytes - begin : piece_bytes);
    unsigned char* const* tab = (kv ? v_bufs : k_bufs) + (size_t)layer * b;
    const unsigned char* sp = tab[src] + (size_t)head * len_src * row_bytes + begin;           // head == 0 under BSHD
    unsigned char* dp = tab[dst] + (size_t)head * len_dst * row_bytes + begin;

    // the run's two base addresses and its length, as in kv_blocks.hip: piece_bytes % 16 == 0, so begin and len follow
    if ((((uintptr_t)sp | (uintptr_t)dp | (uintptr_t)run_bytes) & 15) == 0) {
        const u32x4* s16 = reinterpret_cast<const u32x4*>(sp);
        u32x4* d16 = reinterpret_cast<u32x4*>(dp);
        const int nvec = len >> 4;
        for (int i0 = threadIdx.x; i0 < nvec; i0 += ZL_KVF_THREADS * ZL_KVF_UNROLL) {
            u32x4 v[ZL_KVF_UNROLL];
#pragma unroll
            for (int u = 0; u < ZL_KVF_UNROLL; ++u) {
                const int i = i0 + u * ZL_KVF_THREADS;
                if (i < nvec) v[u] = s16[i];
            }
#pragma unroll
            for (int u = 0; u < ZL_KVF_UNROLL; ++u) {
                const int i = i0 + u * ZL_KVF_THREADS;
                if (i < nvec) __builtin_nontemporal_store(v[u], d16 + i);
            }
        }
    } else {                                                               // row_bytes % 4 == 0 and 4-byte aligned bases
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(sp);
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dp);
        const int nw = len >> 2;
        for (int i0 = threadIdx.x; i0 < nw; i0 += ZL_KVF_THREADS * ZL_KVF_UNROLL) {
            uint32_t v[ZL_KVF_UNROLL];
#pragma unroll
            for (int u = 0; u < ZL_KVF_UNROLL; ++u) {
                const int i = i0 + u * ZL_KVF_THREADS;
                if (i < nw) v[u] = s4[i];
            }
#pragma unroll
            for (int u = 0; u < ZL_KVF_UNROLL; ++u) {
                const int i = i0 + u * ZL_KVF_THREADS;
                if (i < nw) d4[i] = v[u];
            }
        }
    }
}

int zl_kv_fork_ex(const int32_t* desc, int64_t n, void* const* k_bufs, void* const* v_bufs, const int32_t* buf_lens, int64_t layers,
                  int64_t b, int64_t max_rows, int64_t hkv, int64_t row_bytes, int bshd, int32_t* tokens, int32_t* positions,
                  int32_t* placement, int32_t* valid_lens, int64_t piece_bytes, zl_stream_t s) {
    ZL_CHECK_ARG(n >= 0 && layers > 0 && b > 0 && max_rows >= 0 && hkv > 0 && row_bytes > 0 && piece_bytes >= 0, ZL_EINVAL);
    const int given = (tokens != nullptr) + (positions != nullptr) + (placement != nullptr) + (valid_lens != nullptr);
    ZL_CHECK_ARG(given == 0 || given == 4, ZL_EINVAL);
    if (n == 0) return ZL_OK;
    ZL_CHECK_ARG(desc && k_bufs && v_bufs && buf_lens, ZL_EINVAL);
    if (piece_bytes == 0) piece_bytes = ZL_KVF_PIECE;
    ZL_CHECK_ARG(row_bytes % 4 == 0 && piece_bytes % 16 == 0, ZL_ESHAPE);
    const int64_t i31 = ((int64_t)1 << 31) - 1;
    ZL_CHECK_ARG(layers <= 65535 && hkv <= 65535 && b <= i31 && max_rows <= i31 && row_bytes < ((int64_t)1 << 30) &&
                 piece_bytes <= ((int64_t)1 << 30) && n <= i31 / 4, ZL_ELIMIT);
    const int64_t runs = layers * 2 * (bshd ? 1 : hkv);
    ZL_CHECK_ARG(max_rows * row_bytes <= ((int64_t)1 << 40) / hkv && runs <= i31, ZL_ELIMIT);
    const int64_t run_bytes = max_rows * row_bytes * (bshd ? hkv : 1);
    int64_t pieces = (run_bytes + piece_bytes - 1) / piece_bytes;
    if (pieces < 1) pieces = 1;                                              // max_rows == 0: the bookkeeping still needs its workgroup
    ZL_CHECK_ARG(pieces <= i31 && n * runs <= (i31 - ZL_KVF_XCDS) / pieces, ZL_ELIMIT);
    const int64_t total = n * runs * pieces;
    const dim3 grid((unsigned)((total + ZL_KVF_XCDS - 1) / ZL_KVF_XCDS * ZL_KVF_XCDS)), tb(ZL_KVF_THREADS);
    hipLaunchKernelGGL(k_kv_fork, grid, tb, 0, (hipStream_t)s, desc, (int)n, (unsigned char* const*)k_bufs, (unsigned char* const*)v_bufs,
                       buf_lens, (int)layers, (int)b, (int)max_rows, (int)hkv, (int)row_bytes, bshd, (int)piece_bytes, (int)pieces, total,
                       tokens, positions, placement, valid_lens);
    return zl_launch_status();
}

int zl_kv_fork(const int32_t* desc, int64_t n, void* const* k_bufs, void* const* v_bufs, const int32_t* buf_lens, int64_t layers, int64_t b,
               int64_t max_rows, int64_t hkv, int64_t row_bytes, int bshd, int32_t* tokens, int32_t* positions, int32_t* placement,
               int32_t* valid_lens, zl_stream_t s) {
    return zl_kv_fork_ex(desc, n, k_bufs, v_bufs, buf_lens, layers, b, max_rows, hkv, row_bytes, bshd, tokens, positions, placement,
                         valid_lens, 0, s);
}
