"""Operator-level Python mirror of the reference's `nn::` / `gptq::` / `int8_op::` free functions
(the "bmengine op" surface of SURVEY.md 8b) on top of the C ABI.

PyTorch is used for device memory and streams only: every function takes CUDA tensors, allocates its
output like the reference op does with `ctx.tensor(...)`, and enqueues ONE C-ABI launcher on the
current torch stream.  There is no CPU / eager fallback: without the HIP library these raise.

Names, argument meaning and error behaviour follow the reference (citations on each function;
paths relative to the ZhiLight tree).
"""
import collections
import ctypes as C
import os
import math

import numpy as np
import torch

from . import _lib
from ._lib import SampleOpts, W4Layout, W4Opts, ZLError, check, lib

F16, BF16 = 0, 1
EPI_BIAS, EPI_ADD_C, EPI_RESIDUAL, EPI_SILU_MUL, EPI_SILU_MUL_F32 = 1, 2, 4, 8, 16


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _i(v):
    return C.c_int64(int(v))


def _f(v):
    return C.c_float(float(v))


def _chk_out(out, m, n, dtype, device, what):
    """a caller-supplied output: (m, n) elements of `dtype`, contiguous rows, on the input's device (the launchers write
    m * n elements at out.data_ptr(): a wrong one is a silent overrun)"""
    if out.dtype != dtype or out.device != device or not out.is_contiguous() or out.numel() != m * n:
        raise ZLError(f"{what}: Wrong output size() / dtype / layout")


def _dt(t):
    if t.dtype == torch.float16:
        return F16
    if t.dtype == torch.bfloat16:
        return BF16
    raise ZLError(f"unsupported activation dtype {t.dtype}")


def _dt_logits(t):
    """router logits: T, or fp32 (ZL_F32 = 2) -- the reference's router Linear writes fp32 logits (feedforward.cpp:285-286)"""
    return 2 if t.dtype == torch.float32 else _dt(t)


def _chk_cuda(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.is_contiguous()):
            raise ZLError("tensors must be contiguous CUDA tensors")


# --------------------------------------------------------------------------------------------------
# a4: load-time layout transforms  (src/nn/quant/gptq/gptq.h:24-49,141-148)
# --------------------------------------------------------------------------------------------------
def gptq_shuffle(qweight):
    """In place on a (K/8, N) int32 tensor -- nn::gptq::gptq_shuffle without act-order."""
    _chk_cuda(qweight)
    check(lib().zl_gptq_shuffle(_p(qweight), _i(qweight.shape[0]), _i(qweight.shape[1]), _stream()), "gptq_shuffle")
    return qweight


def increase_zero(qzeros):
    _chk_cuda(qzeros)
    check(lib().zl_gptq_increase_zero(_p(qzeros), _i(qzeros.numel()), _stream()), "increase_zero")
    return qzeros


def q4_to_q8(qzeros):
    _chk_cuda(qzeros)
    out = torch.empty(qzeros.shape[:-1] + (qzeros.shape[-1] * 8,), dtype=torch.uint8, device=qzeros.device)
    check(lib().zl_gptq_q4_to_q8(_p(qzeros), _p(out), _i(qzeros.numel()), _stream()), "q4_to_q8")
    return out


def transpose_2d(t):
    """functions::Transpose for a 2-D tensor of 1/2/4-byte elements."""
    _chk_cuda(t)
    rows, cols = t.shape
    out = torch.empty((cols, rows), dtype=t.dtype, device=t.device)
    check(lib().zl_transpose_2d(_p(t), _p(out), _i(rows), _i(cols), C.c_int(t.element_size()), _stream()), "transpose")
    return out


def awq_un_shuffle(q):
    _chk_cuda(q)
    check(lib().zl_awq_un_shuffle(_p(q), _i(q.shape[0]), _i(q.shape[1]), _stream()), "un_shuffle")
    return q


def shuffle_awq(qweight, use_exllama=True):
    _chk_cuda(qweight)
    k, n8 = qweight.shape
    out = torch.empty((k // 8, n8 * 8), dtype=qweight.dtype, device=qweight.device)
    check(lib().zl_awq_shuffle(_p(qweight), _p(out), _i(k), _i(n8 * 8), C.c_int(int(use_exllama)), _stream()),
          "shuffle_awq")
    return out


class W4Weight:
    """A W4 (GPTQ / AWQ-as-exllama) linear weight in the gfx950-native ZLW4 layout (include/zhilight_amd.h).

    Plays the role of Int4GPTQ's device-side state after load_state_dict -> preprocess_weight ->
    transpose_weight (src/nn/linear/linear.cpp:1139-1244)."""

    def __init__(self, n, k, group_size, qw, scales, zeros, sym=False, row_interleave=False):
        self.n, self.k, self.group_size = n, k, group_size
        self.qw, self.scales, self.zeros = qw, scales, zeros
        self.sym, self.row_interleave = sym, row_interleave

    @staticmethod
    def layout(n, k, group_size):
        L = W4Layout()
        check(lib().zl_w4_layout(_i(n), _i(k), _i(group_size), C.byref(L)), "w4_layout")
        return L

    @classmethod
    def from_k_major(cls, qweight_km, qzeros_km, scales_km, group_size, sym=False, row_interleave=False):
        """qweight (N,K/8) int32 shuffled words, qzeros (N,K/G) uint8, scales (N,K/G) fp16."""
        _chk_cuda(qweight_km, qzeros_km, scales_km)
        n, k = qweight_km.shape[0], qweight_km.shape[1] * 8
        L = cls.layout(n, k, group_size)
        dev = qweight_km.device
        qw = torch.empty(L.qw_bytes // 4, dtype=torch.int32, device=dev)
        sc = torch.empty(L.scales_bytes // 2, dtype=torch.float16, device=dev)
        zs = torch.empty(L.zeros_bytes // 2, dtype=torch.int16, device=dev)
        check(lib().zl_w4_pack(_p(qweight_km), _p(qzeros_km), _p(scales_km), _i(n), _i(k), _i(group_size),
                               C.c_int(int(row_interleave)), _p(qw), _p(sc), _p(zs), _stream()), "w4_pack")
        return cls(n, k, group_size, qw, sc, zs, sym, row_interleave)

    @classmethod
    def from_hf_gptq(cls, qweight, qzeros, scales, group_size, sym=False, row_interleave=False):
        """HF / AutoGPTQ tensors: qweight (K/8,N) int32, qzeros (K/G,N/8) int32, scales (K/G,N) fp16.
        Same steps as the reference's load path: shuffle, +1 zeros, nibble->byte, transpose x3."""
        qw = gptq_shuffle(qweight.clone())
        qz = q4_to_q8(increase_zero(qzeros.clone()))
        return cls.from_k_major(transpose_2d(qw), transpose_2d(qz), transpose_2d(scales.contiguous()), group_size,
                                sym, row_interleave)

    def dequant(self):
        """(N, K) fp16 = rn16(rn16(q - z) * s) -- nn::gptq::dequant_k_major(out_type=0)."""
        out = torch.empty((self.n, self.k), dtype=torch.float16, device=self.qw.device)
        check(lib().zl_w4_dequant(_p(self.qw), _p(self.scales), _p(self.zeros), _i(self.n), _i(self.k),
                                  _i(self.group_size), _p(out), _stream()), "w4_dequant")
        return out

    def nbytes(self):
        return self.qw.numel() * 4 + self.scales.numel() * 2 + self.zeros.numel() * 2

    @classmethod
    def random(cls, n, k, group_size, device, gen=None, scale_mag=0.005, sym=False, row_interleave=False):
        """Synthetic weight generated directly in the packed layout (benchmarks: no checkpoint I/O)."""
        L = cls.layout(n, k, group_size)
        qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (L.qw_bytes // 4,), dtype=torch.int32, device=device, generator=gen)
        sc = (torch.rand(L.scales_bytes // 2, device=device, generator=gen) * scale_mag + 1e-4).to(torch.float16)
        zs = torch.randint(-2 ** 15, 2 ** 15 - 1, (L.zeros_bytes // 2,), dtype=torch.int16, device=device, generator=gen)
        return cls(n, k, group_size, qw, sc, zs, sym, row_interleave)



class W4MoEWeight:
    """The experts of one MoE projection, each packed like a W4Weight, stacked `stride` elements apart (what the reference
    keeps as (E, N, K/8) / (E, N, K/G) tensors for its fused MoE kernels, src/nn/feedforward/feedforward.cpp FUSE_GPTQ_MOE).
    gate / up: pass the (2 n_ff, K) [gate; up] k-major tensors of every expert with row_interleave=True."""

    def __init__(self, experts, n, k, group_size, qw, scales, zeros, row_interleave):
        self.experts, self.n, self.k, self.group_size = experts, n, k, group_size
        self.qw, self.scales, self.zeros, self.row_interleave = qw, scales, zeros, row_interleave
        L = W4Weight.layout(n, k, group_size)
        self.stride_bytes = (L.qw_bytes, L.scales_bytes, L.zeros_bytes)

    @classmethod
    def from_k_major(cls, qweights, qzeros, scales, group_size, row_interleave=False):
        """lists (one entry per expert) of qweight (N, K/8) int32, qzeros (N, K/G) uint8, scales (N, K/G) fp16"""
        ws = [W4Weight.from_k_major(q, z, s, group_size, False, row_interleave) for q, z, s in zip(qweights, qzeros, scales)]
        w0 = ws[0]
        return cls(len(ws), w0.n, w0.k, group_size, torch.stack([w.qw for w in ws]).contiguous(),
                   torch.stack([w.scales for w in ws]).contiguous(), torch.stack([w.zeros for w in ws]).contiguous(), row_interleave)

    def nbytes(self):
        return self.qw.numel() * 4 + self.scales.numel() * 2 + self.zeros.numel() * 2


def moe_up(x, w: W4MoEWeight, expert_ids, n_shared=0, exp_parallel=False, world_size=1, rank=0, out=None):
    """nn::gptq::gemm_moe_up (q_gemm_k_major.cu:392-455): out (M, top_k + n_shared, n_ff) = silu(x . gate_e) * (x . up_e) for
    the token's experts; the shared experts are the LAST n_shared of the stack."""
    if x.dtype != torch.float16 or not w.row_interleave:
        raise ZLError("moe_up: half activations, row-interleaved [gate; up] experts")
    _chk_cuda(x, expert_ids)
    m, k = x.shape
    if k != w.k or expert_ids.dtype != torch.int32 or expert_ids.shape[0] != m:
        raise ZLError("moe_up: shape / dtype mismatch")
    top_k, n_ff = expert_ids.shape[1], w.n // 2
    if out is None:
        out = torch.empty((m, top_k + n_shared, n_ff), dtype=torch.float16, device=x.device)
    else:
        _chk_out(out, m * (top_k + n_shared), n_ff, torch.float16, x.device, "moe_up")
    sq, ss, sz = w.stride_bytes
    check(lib().zl_w4a16_moe_up(_p(x), _i(x.stride(0)), _p(w.qw), _p(w.scales), _p(w.zeros), _i(sq), _i(ss), _i(sz), _p(expert_ids),
                                _p(out), _i(m), _i(n_ff), _i(k), _i(w.group_size), C.c_int(top_k), C.c_int(n_shared),
                                C.c_int(w.experts - n_shared), C.c_int(int(exp_parallel)), C.c_int(world_size), C.c_int(rank),
                                _stream()), "w4a16_moe_up")
    return out


def moe_down(a, w: W4MoEWeight, expert_ids, expert_weights, n_shared=0, exp_parallel=False, world_size=1, rank=0, out=None,
             add_c=False):
    """nn::gptq::gemm_moe_down (q_gemm_k_major.cu:457-520): out (M, N) = sum over the token's experts of weight * (a[m, t] . W_e)
    (+ out with add_c); a (M, top_k + n_shared, K)."""
    if a.dtype != torch.float16 or w.row_interleave:
        raise ZLError("moe_down: half activations, plain experts")
    _chk_cuda(a, expert_ids, expert_weights)
    m, t, k = a.shape
    top_k = expert_ids.shape[1]
    if k != w.k or t != top_k + n_shared or expert_ids.dtype != torch.int32 or expert_weights.dtype != torch.float32 or \
            tuple(expert_weights.shape) != tuple(expert_ids.shape) or expert_ids.shape[0] != m:
        raise ZLError("moe_down: shape / dtype mismatch")
    if out is None:
        if add_c:
            raise ZLError("moe_down: add_c needs the output to add to")
        out = torch.empty((m, w.n), dtype=torch.float16, device=a.device)
    else:
        _chk_out(out, m, w.n, torch.float16, a.device, "moe_down")
    sq, ss, sz = w.stride_bytes
    check(lib().zl_w4a16_moe_down(_p(a), _i(k), _p(w.qw), _p(w.scales), _p(w.zeros), _i(sq), _i(ss), _i(sz), _p(expert_ids),
                                  _p(expert_weights), _p(out), _i(m), _i(w.n), _i(k), _i(w.group_size), C.c_int(top_k),
                                  C.c_int(n_shared), C.c_int(w.experts - n_shared), C.c_int(int(exp_parallel)), C.c_int(world_size),
                                  C.c_int(rank), C.c_int(int(add_c)), _stream()), "w4a16_moe_down")
    return out


class W4MMoEWeight:
    """The experts of one MoE projection in the ZLW4M layout (what zl_w4a16_gemm_grouped reads), stacked: expert e's words at
    qw[e], its meta at meta[e].  gate / up: the (2 n_ff, K) [gate; up] k-major tensors of every expert with row_interleave=True."""

    def __init__(self, experts, n, k, group_size, qw, meta, row_interleave):
        self.experts, self.n, self.k, self.group_size = experts, n, k, group_size
        self.qw, self.meta, self.row_interleave = qw, meta, row_interleave
        L = W4MWeight.layout(n, k, group_size)
        self.stride_bytes = (L.qw_bytes, L.scales_bytes)

    @classmethod
    def from_k_major(cls, qweights, qzeros, scales, group_size, row_interleave=False):
        """lists (one entry per expert) of qweight (N, K/8) int32, qzeros (N, K/G) uint8, scales (N, K/G) fp16; packed into
        the stack one expert at a time (no second copy of the stack)"""
        e = len(qweights)
        n, k = qweights[0].shape[0], qweights[0].shape[1] * 8
        L = W4MWeight.layout(n, k, group_size)
        dev = qweights[0].device
        qw = torch.empty((e, L.qw_bytes // 4), dtype=torch.int32, device=dev)
        meta = torch.empty((e, L.scales_bytes // 4), dtype=torch.int32, device=dev)
        for i, (q, z, s) in enumerate(zip(qweights, qzeros, scales)):
            _chk_cuda(q, z, s)
            if q.shape != (n, k // 8):
                raise ZLError("W4MMoEWeight: every expert has the same shape")
            check(lib().zl_w4m_pack(_p(q), _p(z), _p(s), _i(n), _i(k), _i(group_size), C.c_int(int(row_interleave)), _p(qw[i]),
                                    _p(meta[i]), _stream()), "w4m_pack")
        return cls(e, n, k, group_size, qw, meta, row_interleave)

    def expert(self, e):
        """expert e as a W4MWeight (a view: tests, per-expert references)"""
        return W4MWeight(self.n, self.k, self.group_size, self.qw[e], self.meta[e], self.row_interleave)

    def nbytes(self):
        return self.qw.numel() * 4 + self.meta.numel() * 4


def moe_grouped_slots(pairs, num_experts):
    """(M-tile rows, grid slots) of a zl_w4a16_gemm_grouped launch over `pairs` sorted rows: the host half of the work table,
    sizes only -- sum over experts of ceil(load / BM) <= pairs // BM + min(E, pairs)"""
    if pairs <= 0:
        return 16, 0
    a = min(pairs, num_experts)
    avg = (pairs + a - 1) // a
    bm = 16 if avg <= 16 else 32 if avg <= 32 else 64 if avg < 128 else 128
    return bm, pairs // bm + a


def moe_gemm_grouped(x, w: W4MMoEWeight, expert_loads, index, pairs, in_div=0, out_scatter=False, out=None, out_rows=None,
                     epilogue=0):
    """zl_w4a16_gemm_grouped: the W4A16 GEMM of every expert over its sorted rows in one launch.  Sorted position j (< pairs)
    reads x row index[j] // in_div (in_div = 0: row j) and writes out row j (out_scatter: row index[j]); expert e owns the
    expert_loads[e] positions after those of experts < e.  out: (out_rows or pairs, n) -- n / 2 columns with EPI_SILU_MUL."""
    if x.dtype != torch.float16 or x.dim() != 2:
        raise ZLError("moe_gemm_grouped: (rows, K) half activations")
    _chk_cuda(x, expert_loads, index)
    if x.shape[1] != w.k or x.stride(1) != 1:
        raise ZLError("moe_gemm_grouped: size K mismatch")
    if expert_loads.dtype != torch.int32 or expert_loads.numel() != w.experts:
        raise ZLError("moe_gemm_grouped: expert_loads is one int32 per expert of the stack")
    if index is not None and (index.dtype != torch.int32 or index.numel() < pairs):
        raise ZLError("moe_gemm_grouped: index holds pairs int32")
    if index is None and (in_div or out_scatter):
        raise ZLError("moe_gemm_grouped: gathering or scattering rows needs the index")
    if epilogue not in (0, EPI_SILU_MUL, EPI_SILU_MUL_F32) or (epilogue and not w.row_interleave):
        raise ZLError("moe_gemm_grouped: epilogue 0, or the silu*mul of a row-interleaved gate|up stack")
    if w.group_size % 128 or w.k % 128:
        raise ZLError("moe_gemm_grouped: K and the group size are multiples of 128")
    n_out = w.n // 2 if epilogue else w.n
    rows = out_rows if out_rows is not None else pairs
    if out is None:
        out = torch.empty((rows, n_out), dtype=torch.float16, device=x.device)
    else:
        _chk_out(out, rows, n_out, torch.float16, x.device, "moe_gemm_grouped")
    if pairs == 0:
        return out
    sq, sm = w.stride_bytes
    check(lib().zl_w4a16_gemm_grouped(_p(x), _i(x.stride(0)), _i(x.shape[0]), _p(w.qw), _p(w.meta), _i(w.experts), _i(sq), _i(sm),
                                      _p(expert_loads), _p(index), _i(pairs), C.c_int(int(in_div)), C.c_int(int(bool(out_scatter))),
                                      _p(out), _i(rows), _i(w.n), _i(w.k), _i(w.group_size), C.c_int(epilogue), _stream()),
          "w4a16_gemm_grouped")
    return out


def moe_gemm_pairs(x, w: W4MMoEWeight, expert_ids, in_div=0, out=None, epilogue=0):
    """zl_w4a16_gemm_pairs, the small-M form of moe_gemm_grouped: pair j of expert_ids (any shape, flattened) multiplies x row
    j // in_div (in_div = 0: row j) with its expert's matrix -> out row j; the same bits as the sorted form for the same row"""
    if x.dtype != torch.float16 or x.dim() != 2:
        raise ZLError("moe_gemm_pairs: (rows, K) half activations")
    _chk_cuda(x, expert_ids)
    if x.shape[1] != w.k or x.stride(1) != 1:
        raise ZLError("moe_gemm_pairs: size K mismatch")
    if expert_ids.dtype != torch.int32:
        raise ZLError("moe_gemm_pairs: int32 expert ids")
    if epilogue not in (0, EPI_SILU_MUL, EPI_SILU_MUL_F32) or (epilogue and not w.row_interleave):
        raise ZLError("moe_gemm_pairs: epilogue 0, or the silu*mul of a row-interleaved gate|up stack")
    if w.group_size % 128 or w.k % 128:
        raise ZLError("moe_gemm_pairs: K and the group size are multiples of 128")
    p = expert_ids.numel()
    if p > 65535:
        raise ZLError("moe_gemm_pairs: at most 65535 pairs")
    n_out = w.n // 2 if epilogue else w.n
    if out is None:
        out = torch.empty((p, n_out), dtype=torch.float16, device=x.device)
    else:
        _chk_out(out, p, n_out, torch.float16, x.device, "moe_gemm_pairs")
    if p == 0:
        return out
    sq, sm = w.stride_bytes
    check(lib().zl_w4a16_gemm_pairs(_p(x), _i(x.stride(0)), _i(x.shape[0]), _p(w.qw), _p(w.meta), _i(w.experts), _i(sq), _i(sm),
                                    _p(expert_ids), _i(p), C.c_int(int(in_div)), _p(out), _i(w.n), _i(w.k), _i(w.group_size),
                                    C.c_int(epilogue), _stream()), "w4a16_gemm_pairs")
    return out


def w4a16_gemm(x, w, bias=None, residual=None, out=None, norm_weight=None, norm_eps=1e-5, epilogue=0):
    """y = x . dequant(W)^T with optional fused RMSNorm prologue and bias / ADD_C / residual / silu*mul
    epilogue -- nn::gptq::gptq_gemm_k_major (M <= 40 branch) and nn::gptq::gemm_fuse_gate_in
    (src/nn/quant/gptq/q_gemm_k_major.cu:957-1116, 765-829)."""
    if x.dtype != torch.float16:
        raise ZLError("A must be half")  # q_gemm_k_major.cu:989
    _chk_cuda(x, bias, residual, norm_weight)
    x2 = x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    if k != w.k:
        raise ZLError("size K mismatch")
    silu = epilogue & (EPI_SILU_MUL | EPI_SILU_MUL_F32)
    n_out = w.n // 2 if silu else w.n
    if out is None:
        out = torch.empty((m, n_out), dtype=torch.float16, device=x.device)
    elif tuple(out.shape[-2:]) != (m, n_out) and out.numel() != m * n_out:
        raise ZLError("Wrong output size()")
    if bias is not None:
        epilogue |= EPI_BIAS
    check(lib().zl_w4a16_gemm(_p(x2), _i(x2.stride(0)), _p(w.qw), _p(w.scales), _p(w.zeros), _p(bias), _p(residual),
                              _p(out), _i(m), _i(w.n), _i(k), _i(w.group_size), C.c_int(int(w.sym)),
                              _p(norm_weight), _f(norm_eps), C.c_int(epilogue), _stream()), "w4a16_gemm")
    return out


class W4MWeight:
    """The same W4 linear weight in the MFMA-oriented ZLW4M layout (16-row x 128-k tiles + per-row meta)."""

    def __init__(self, n, k, group_size, qw, meta, row_interleave=False):
        self.n, self.k, self.group_size = n, k, group_size
        self.qw, self.meta, self.row_interleave = qw, meta, row_interleave

    @staticmethod
    def layout(n, k, group_size):
        L = W4Layout()
        check(lib().zl_w4m_layout(_i(n), _i(k), _i(group_size), C.byref(L)), "w4m_layout")
        return L

    @classmethod
    def from_k_major(cls, qweight_km, qzeros_km, scales_km, group_size, row_interleave=False):
        _chk_cuda(qweight_km, qzeros_km, scales_km)
        n, k = qweight_km.shape[0], qweight_km.shape[1] * 8
        L = cls.layout(n, k, group_size)
        dev = qweight_km.device
        qw = torch.empty(L.qw_bytes // 4, dtype=torch.int32, device=dev)
        meta = torch.empty(L.scales_bytes // 4, dtype=torch.int32, device=dev)
        check(lib().zl_w4m_pack(_p(qweight_km), _p(qzeros_km), _p(scales_km), _i(n), _i(k), _i(group_size),
                                C.c_int(int(row_interleave)), _p(qw), _p(meta), _stream()), "w4m_pack")
        return cls(n, k, group_size, qw, meta, row_interleave)

    def nbytes(self):
        return self.qw.numel() * 4 + self.meta.numel() * 4

    def to_k_major(self):
        """zl_w4m_unpack: (qweight (N,K/8) int32, qzeros (N,K/G) uint8, scales (N,K/G) fp16) -- the operands of
        gptq_gemm_k_major (q_gemm_k_major.cu:957-1116), in checkpoint row order even for a row-interleaved weight."""
        dev = self.qw.device
        ng = self.k // self.group_size
        qw = torch.empty((self.n, self.k // 8), dtype=torch.int32, device=dev)
        qz = torch.empty((self.n, ng), dtype=torch.uint8, device=dev)
        sc = torch.empty((self.n, ng), dtype=torch.float16, device=dev)
        check(lib().zl_w4m_unpack(_p(self.qw), _p(self.meta), _i(self.n), _i(self.k), _i(self.group_size),
                                  C.c_int(int(self.row_interleave)), _p(qw), _p(qz), _p(sc), _stream()), "w4m_unpack")
        return qw, qz, sc

    @classmethod
    def random(cls, n, k, group_size, device, gen=None, scale_mag=0.005, row_interleave=False):
        """Synthetic weight generated directly in the packed layout (benchmarks: no checkpoint I/O)."""
        L = cls.layout(n, k, group_size)
        qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (L.qw_bytes // 4,), dtype=torch.int32, device=device, generator=gen)
        gi = group_size // 128                          # the (scale, zero) pair is repeated on each 128-k item of its group
        cnt = L.scales_bytes // 4 // gi
        sc = (torch.rand(cnt, device=device, generator=gen) * scale_mag + 1e-4).to(torch.float16)
        sc = sc.view(torch.int16).to(torch.int32) & 0xffff
        z = torch.randint(0, 16, (cnt,), dtype=torch.int32, device=device, generator=gen)
        meta = (sc | ((0xe400 | z) << 16)).to(torch.int64)
        meta = torch.where(meta >= 2 ** 31, meta - 2 ** 32, meta).to(torch.int32)
        if gi > 1:
            meta = meta.view(-1, 1, 16).expand(-1, gi, 16).reshape(-1).contiguous()
        return cls(n, k, group_size, qw, meta, row_interleave)


def decode_attn_split_len(b, num_kv_heads, max_len_buf):
    """keys per split of the split-KV decode attention kernels for this batch geometry (zl_decode_attn_split_len)"""
    return int(lib().zl_decode_attn_split_len(_i(b), _i(num_kv_heads), _i(max_len_buf)))


def _attn_algo():
    """zl_decode_attn_ex algo: ZL_ATTN_MFMA=0 forces the VALU split-KV kernel (tests cover both)"""
    return 1 if os.environ.get("ZL_ATTN_MFMA", "1") == "0" else 0


_SCRATCH = {}
_SCRATCH_RETIRED = []   # outgrown scratch buffers, kept alive for the graphs that captured them
# tuning overrides of the W4A16 launchers: read HERE, on the host side, per call (the C ABI reads no environment); the
# tests and micro-benchmarks sweep them
_W4_ENV = (("phase_rounds", "ZL_W4_PHASE_ROUNDS"), ("phase_ksplit", "ZL_W4_PHASE_KSPLIT"), ("phase_ksplit_min_m", "ZL_W4_PHASE_KSPLIT_MINM"),
           ("phase_min_m", "ZL_W4_PHASE_MIN_M"), ("phase_max_m", "ZL_W4_PHASE_MAX_M"), ("tiled_min_m", "ZL_W4_TILED_MIN_M"),
           ("tiled_bm", "ZL_W4_TILED_BM"), ("tiled_splitk", "ZL_W4_TILED_SPLITK"), ("mfma_ks", "ZL_MFMA_KS"), ("mfma_rounds", "ZL_MFMA_ROUNDS"), ("tiled_wide", "ZL_W4_TILED_WIDE"),
           ("slab", "ZL_W4_SLAB"), ("slab_min_m", "ZL_W4_SLAB_MIN_M"), ("slab_nw", "ZL_W4_SLAB_NW"), ("slab_gpw", "ZL_W4_SLAB_GPW"), ("slab_r", "ZL_W4_SLAB_R"),
           ("defer_norm", "ZL_DEFER_NORM"))


def w4_scratch(device, m, n):
    """The caller-provided scratch of the K-split W4A16 paths (zl_w4_opts_t::scratch): one zero-initialised buffer per
    device, grown on demand OUTSIDE stream capture (run a step eagerly before capturing it, as bench.py does).  Launches
    that use it must be ordered among themselves -- one compute stream per device at a time, like the reference's engine
    (the dual-stream prompt encode only runs collectives on its second stream); a caller with concurrent GEMM streams
    passes its own buffers through zl_w4a16_gemm_mfma_ex."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    need = int(lib().zl_w4a16_scratch_bytes(_i(m), _i(n)))
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            return buf                                 # too small during capture: the launchers take their unsplit routes
        if buf is not None:
            # a buffer that has been handed out is NEVER freed: a hipGraph captured earlier has its address baked into the
            # K-split launches (arrival counters + fp32 partials) and would scribble over whatever the allocator put there next
            _SCRATCH_RETIRED.append(buf)
        buf = torch.zeros(max(need, 64 << 20), dtype=torch.uint8, device=device)
        _SCRATCH[key] = buf
    return buf


def w4_scratch_reserve(device, m_max, n_max):
    """size the device's K-split scratch once for the largest (rows, columns) any later call will ask for -- before capturing
    graphs, so that no later growth retires the buffer they hold"""
    return w4_scratch(device, m_max, n_max)


def _w4_opts(device, m, n):
    o = W4Opts()
    buf = w4_scratch(device, m, n) if m > 2 else None   # up to 2 rows no launcher splits over workgroups (3..4: the long-K slab route)
    if buf is not None:
        o.scratch, o.scratch_bytes = buf.data_ptr(), buf.numel()
    for field, env in _W4_ENV:
        v = os.environ.get(env)
        if v:
            setattr(o, field, int(v))
    if os.environ.get("ZL_W4_PHASE_SMALL") == "0":
        o.phase_small_off = 1
    if os.environ.get("ZL_W4_SMALL_ALGO"):             # 1: the fp16-dequant kernels of rounds 1-2 for 1..4 rows
        o.small_algo = int(os.environ["ZL_W4_SMALL_ALGO"])
    return o


def row_ss(x, out=None):
    """zl_row_ss: per row and 16-column tile the sum of squares of x (M, K) -> fp32 (M, K / 16): the statistics a normalising
    W4 launch takes through row_ss= instead of walking the rows again (zl_w4_opts_t::row_ss)"""
    _chk_cuda(x, out)
    if x.dtype != torch.float16 or x.dim() != 2 or x.shape[1] % 16:
        raise ZLError("row_ss: fp16 (M, K), K a multiple of 16")
    m, k = x.shape
    if out is None:
        out = torch.empty((m, k // 16), dtype=torch.float32, device=x.device)
    check(lib().zl_row_ss(_p(x), _i(x.stride(0)), _i(m), _i(k), _p(out), _stream()), "row_ss")
    return out


def w4_row_ss_routes(m, w_producers, w_consumers, device):
    """does every producing projection (plain / residual epilogue) leave the rows' statistics and every normalising one take them?
    (the route questions of zl_w4a16_gemm_mfma_ex, asked without launching; consumers: (weight, rope) pairs)"""
    dummy = C.c_void_p(16)
    for w in w_producers:
        o = _w4_opts(device, m, w.n)
        o.row_ss_out = dummy
        if not isinstance(w, W4MWeight) or not lib().zl_w4a16_emits_row_ss(_i(m), _i(w.n), _i(w.k), _i(w.group_size), C.c_int(EPI_RESIDUAL), C.byref(o)):
            return False
    for w, rope in w_consumers:
        o = _w4_opts(device, m, w.n)
        o.row_ss = dummy
        if not isinstance(w, W4MWeight) or not lib().zl_w4a16_takes_row_ss(_i(m), _i(w.n), _i(w.k), _i(w.group_size), C.c_int(int(rope)), C.byref(o)):
            return False
    return True


def w4a16_gemm_mfma(x, w, bias=None, residual=None, out=None, norm_weight=None, norm_eps=1e-5, epilogue=0, row_ss=None, row_ss_out=None):
    """MFMA flavour of w4a16_gemm (fp32 accumulation = the numerics of the reference's M > 40 branch).
    row_ss (M, K / 16) fp32 with norm_weight: the rows' statistics (ops.row_ss or a producing launch's row_ss_out);
    row_ss_out (M, N / 16): filled with the statistics of the rows this launch stores where its route does that (w4_row_ss_routes)."""
    if x.dtype != torch.float16:
        raise ZLError("A must be half")
    _chk_cuda(x, bias, residual, norm_weight)
    x2 = x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    if k != w.k:
        raise ZLError("size K mismatch")
    silu = epilogue & (EPI_SILU_MUL | EPI_SILU_MUL_F32)
    n_out = w.n // 2 if silu else w.n
    if out is None:
        out = torch.empty((m, n_out), dtype=torch.float16, device=x.device)
    else:
        _chk_out(out, m, n_out, torch.float16, x.device, "w4a16_gemm_mfma")
    if bias is not None:
        epilogue |= EPI_BIAS
    opts = _w4_opts(x.device, m, w.n)
    _chk_cuda(row_ss, row_ss_out)
    if row_ss is not None:
        opts.row_ss = row_ss.data_ptr()
    if row_ss_out is not None:
        opts.row_ss_out = row_ss_out.data_ptr()
    check(lib().zl_w4a16_gemm_mfma_ex(_p(x2), _i(x2.stride(0)), _p(w.qw), _p(w.meta), _p(bias), _p(residual),
                                      _p(out), _i(m), _i(w.n), _i(k), _i(w.group_size), _p(norm_weight), _f(norm_eps),
                                      C.c_int(epilogue), C.byref(opts), _stream()), "w4a16_gemm_mfma")
    return out


def w4a16_gemm_tiled(x, w, bias=None, residual=None, out=None, epilogue=0):
    """The M-tiled MFMA GEMM called directly (w4a16_gemm_mfma forwards to it for M > 64)."""
    if x.dtype != torch.float16:
        raise ZLError("A must be half")
    _chk_cuda(x, bias, residual)
    x2 = x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    if k != w.k:
        raise ZLError("size K mismatch")
    silu = epilogue & (EPI_SILU_MUL | EPI_SILU_MUL_F32)
    if out is None:
        out = torch.empty((m, w.n // 2 if silu else w.n), dtype=torch.float16, device=x.device)
    else:
        _chk_out(out, m, w.n // 2 if silu else w.n, torch.float16, x.device, "w4a16_gemm_tiled")
    if bias is not None:
        epilogue |= EPI_BIAS
    opts = _w4_opts(x.device, max(m, 5), w.n)
    check(lib().zl_w4a16_gemm_tiled_ex(_p(x2), _i(x2.stride(0)), _p(w.qw), _p(w.meta), _p(bias), _p(residual), _p(out),
                                       _i(m), _i(w.n), _i(k), _i(w.group_size), C.c_int(epilogue), C.byref(opts), _stream()),
          "w4a16_gemm_tiled")
    return out


def arange_i32(n, device, start=0, step=1):
    """functions::arange (bmengine init.h:10) as a kernel: int32 start, start + step, ..."""
    out = torch.empty(n, dtype=torch.int32, device=device)
    if n:
        check(lib().zl_arange_i32(_p(out), C.c_int32(start), C.c_int32(step), _i(n), _stream()), "arange_i32")
    return out


def divide_i32(a, divisor):
    """functions::divide on int32 (element.h:25): truncating integer quotient"""
    _chk_cuda(a)
    out = torch.empty_like(a)
    if a.numel():
        check(lib().zl_divide_i32(_p(a), _p(out), C.c_int32(int(divisor)), _i(a.numel()), _stream()), "divide_i32")
    return out


def sort_pairs_i32(keys, values, max_key=0):
    """functions::sort_pair_1d (sort.h:8-12): STABLE sort of (int32 key >= 0, int32 value) pairs by key -> (keys, values)"""
    _chk_cuda(keys, values)
    if keys.dtype != torch.int32 or values.dtype != torch.int32 or keys.numel() != values.numel():
        raise ZLError("sort_pairs_i32: two int32 tensors of one length")
    ko, vo = torch.empty_like(keys), torch.empty_like(values)
    n = keys.numel()
    if n:
        ws = torch.empty(2 * n, dtype=torch.int32, device=keys.device)
        check(lib().zl_sort_pairs_i32(_p(keys), _p(values), _p(ko), _p(vo), _p(ws), _i(n), C.c_int32(int(max_key)), _stream()), "sort_pairs_i32")
    return ko, vo


def scatter_update_dim0(dst, dst_index, src, src_index=None):
    """functions::scatter_update_dim0 (scatter.h:7-13): dst[dst_index[i], :] = src[src_index[i] if given else i, :] in place"""
    _chk_cuda(dst, dst_index, src, src_index)
    if dst.dim() != 2 or src.dim() != 2 or dst.shape[1] != src.shape[1] or dst.dtype != src.dtype or not (dst.is_contiguous() and src.is_contiguous()):
        raise ZLError("scatter_update_dim0: dense (X, D) <- (Y, D) of one dtype")
    if dst_index.numel():
        check(lib().zl_scatter_update_dim0(_p(dst), _p(dst_index), _p(src), _p(src_index), _i(dst_index.numel()), _i(src.shape[1] * src.element_size()),
                                           _i(dst.shape[0]), _i(src.shape[0]), _stream()), "scatter_update_dim0")
    return dst


def experimental_build():
    """True when the loaded library is a ZL_BUILD_EXPERIMENTAL=1 build (digit-plane route, engine's fused launch)"""
    lib()
    return _lib.experimental


def _need_experimental(what):
    if not experimental_build():
        raise ZLError(what + ": only in a ZL_BUILD_EXPERIMENTAL=1 build of libzhilight_amd.so (measured, not faster: DESIGN 5.R4)")


def w4_planes_ok(m, k):
    """what the digit-plane route of the W4A16 linears covers: decode batches of 5..32 rows (1..4 rows: the integer-plane GEMV
    converts inside its own prologue), K a multiple of 128 up to 16384"""
    return experimental_build() and 5 <= m <= 32 and k % 128 == 0 and k <= 16384


def w4_planes(x, norm_weight=None, norm_eps=1e-5, out=None):
    """digit planes of an activation matrix (zl_w4a16_planes): x (M <= 32, K) fp16 -> an opaque uint8 buffer for
    w4_linear_planes / w4_qkv_rope_scatter_planes; with norm_weight the RMSNorm of every row is applied first."""
    _need_experimental("w4_planes")
    if x.dtype != torch.float16:
        raise ZLError("A must be half")
    _chk_cuda(x, norm_weight, out)
    x2 = x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    nbytes = int(lib().zl_w4a16_planes_bytes(_i(m), _i(k)))
    if nbytes < 0:
        check(nbytes, "w4a16_planes_bytes")
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    elif out.numel() < nbytes or out.dtype != torch.uint8:
        raise ZLError("w4_planes: out too small")
    check(lib().zl_w4a16_planes(_p(x2), _i(x2.stride(0)), _i(m), _i(k), _p(norm_weight), _f(norm_eps), _p(out), _stream()),
          "w4a16_planes")
    return out


def w4_linear_planes(planes, m, w, bias=None, residual=None, out=None, epilogue=0):
    """w4a16_gemm_mfma on digit planes (zl_w4a16_gemm_planes): planes = w4_planes(x) of an (m, w.k) matrix."""
    _chk_cuda(planes, bias, residual)
    if not isinstance(w, W4MWeight):
        raise ZLError("w4_linear_planes: a ZLW4M weight")
    silu = epilogue & (EPI_SILU_MUL | EPI_SILU_MUL_F32)
    n_out = w.n // 2 if silu else w.n
    if out is None:
        out = torch.empty((m, n_out), dtype=torch.float16, device=planes.device)
    else:
        _chk_out(out, m, n_out, torch.float16, planes.device, "w4_linear_planes")
    if bias is not None:
        epilogue |= EPI_BIAS
    opts = _w4_opts(planes.device, m, w.n)
    check(lib().zl_w4a16_gemm_planes(_p(planes), _p(w.qw), _p(w.meta), _p(bias), _p(residual), _p(out), _i(m), _i(w.n), _i(w.k),
                                     _i(w.group_size), C.c_int(epilogue), C.byref(opts), _stream()), "w4a16_gemm_planes")
    return out


def w4_qkv_rope_scatter_planes(planes, m, w, cos, sin, placement, buf_lens, k_addrs, v_addrs, num_heads, num_kv_heads, dim_head,
                               bias=None, bshd=True, q_out=None):
    """w4_qkv_rope_scatter on digit planes (the norm went into w4_planes)"""
    _chk_cuda(planes, cos, sin, placement, buf_lens, k_addrs, v_addrs, bias)
    if not isinstance(w, W4MWeight):
        raise ZLError("w4_qkv_rope_scatter_planes: a ZLW4M weight")
    if q_out is None:
        q_out = torch.empty((m, num_heads * dim_head), dtype=torch.float16, device=planes.device)
    check(lib().zl_w4a16_qkv_rope_scatter_planes(_p(planes), _p(w.qw), _p(w.meta), _p(bias), _p(cos), _p(sin), _p(placement),
                                                 _p(buf_lens), _p(k_addrs), _p(v_addrs), _p(q_out), _i(m), _i(num_heads),
                                                 _i(num_kv_heads), _i(dim_head), _i(w.k), _i(w.group_size), C.c_int(int(bshd)),
                                                 _stream()), "w4a16_qkv_rope_scatter_planes")
    return q_out


def w4_linear(x, w, **kw):
    """W4A16 linear on whichever packed layout the weight holds (W4Weight: bit-exact warp-reduce
    arithmetic; W4MWeight: fp32-accumulating MFMA arithmetic)."""
    if isinstance(w, W4MWeight):
        return w4a16_gemm_mfma(x, w, **kw)
    return w4a16_gemm(x, w, **kw)


def gemm_nt_small_m(x, weight, bias=None, alpha=1.0, out=None, norm_weight=None, norm_eps=1e-5, argmax_ws=None):
    """y = T(alpha * x . W^T + bias) -- functions::Gemm(trans_b=True) on the decode path (lm_head).
    With argmax_ws (argmax_workspace) the launch also leaves per-wave greedy candidates for greedy_advance."""
    _chk_cuda(x, weight, bias, norm_weight, argmax_ws)
    x2 = x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    n = weight.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=x.dtype, device=x.device)
    else:
        _chk_out(out, m, n, x.dtype, x.device, "gemm_nt_small_m")
    if argmax_ws is None:
        check(lib().zl_gemm_nt_small_m(_p(x2), _i(x2.stride(0)), _p(weight), _p(bias), _p(out), _i(m), _i(n), _i(k),
                                       _f(alpha), C.c_int(_dt(x)), _p(norm_weight), _f(norm_eps), _stream()),
              "gemm_nt_small_m")
    else:
        check(lib().zl_gemm_nt_small_m_argmax(_p(x2), _i(x2.stride(0)), _p(weight), _p(bias), _p(out), _i(m), _i(n),
                                              _i(k), _f(alpha), C.c_int(_dt(x)), _p(norm_weight), _f(norm_eps),
                                              _p(argmax_ws), _stream()), "gemm_nt_small_m_argmax")
    return out


def gemm_nt(x, weight, bias=None, alpha=1.0, out=None):
    """functions::Gemm(trans_b=True) for any M on the matrix cores (K % 128 == 0); M <= 4 callers want
    gemm_nt_small_m, which streams the weights at HBM speed."""
    _chk_cuda(x, weight, bias)
    x2 = x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    n = weight.shape[0]
    if weight.shape[1] != k:
        raise ZLError("size K mismatch")
    if out is None:
        out = torch.empty((m, n), dtype=x.dtype, device=x.device)
    else:
        _chk_out(out, m, n, x.dtype, x.device, "gemm_nt")
    check(lib().zl_gemm_nt(_p(x2), _i(x2.stride(0)), _p(weight), _p(bias), _p(out), _i(m), _i(n), _i(k), _f(alpha),
                           C.c_int(_dt(x)), _stream()), "gemm_nt")
    return out


class DenseMWeight:
    """A dense (N, K) fp16 / bf16 matrix in the ZLD16M layout (zl_dense_pack_m): 16-row x 128-k tiles whose MFMA fragments are 1 KiB
    contiguous -- for matrices streamed with 5..32 rows (the lm_head of a decode batch).  A second copy of the matrix: the row-major one
    stays what the embedding, the 1..4-row GEMV and the prompt GEMM read."""

    def __init__(self, weight):
        _chk_cuda(weight)
        n, k = weight.shape
        nbytes = int(lib().zl_dense_m_bytes(_i(n), _i(k)))
        if nbytes < 0:
            check(nbytes, "dense_m_bytes")
        self.n, self.k, self.dtype = n, k, weight.dtype
        self.data = torch.empty(nbytes // 2, dtype=weight.dtype, device=weight.device)
        w = weight if weight.is_contiguous() else weight.contiguous()
        check(lib().zl_dense_pack_m(_p(w), _p(self.data), _i(n), _i(k), _stream()), "dense_pack_m")


def gemm_nt_packed(x, w, bias=None, alpha=1.0, out=None):
    """gemm_nt on a DenseMWeight for up to 32 rows: the same bits, the weights streamed in 1 KiB contiguous fragment loads"""
    _chk_cuda(x, bias)
    x2 = x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    if k != w.k or x.dtype != w.dtype:
        raise ZLError("gemm_nt_packed: size K / dtype mismatch")
    if out is None:
        out = torch.empty((m, w.n), dtype=x.dtype, device=x.device)
    else:
        _chk_out(out, m, w.n, x.dtype, x.device, "gemm_nt_packed")
    check(lib().zl_gemm_nt_packed(_p(x2), _i(x2.stride(0)), _p(w.data), _p(bias), _p(out), _i(m), _i(w.n), _i(k), _f(alpha),
                                  C.c_int(_dt(x)), _stream()), "gemm_nt_packed")
    return out


def gemm_nt_f32(x, weight, alpha=1.0):
    """functions::Gemm(trans_b=True) with set_output_type(kFloat): fp32 output, no rounding to T (the MoE router's logits)"""
    _chk_cuda(x, weight)
    x2 = x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    n = weight.shape[0]
    if weight.shape[1] != k or weight.dtype != x.dtype:
        raise ZLError("size K / dtype mismatch")
    out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    check(lib().zl_gemm_nt_f32(_p(x2), _i(x2.stride(0)), _p(weight), _p(out), _i(m), _i(n), _i(k), _f(alpha), C.c_int(_dt(x)), _stream()), "gemm_nt_f32")
    return out


def argmax_workspace(m, n, device):
    nbytes = lib().zl_argmax_workspace_bytes(_i(m), _i(n))
    if nbytes < 0:
        check(int(nbytes), "argmax_workspace_bytes")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def greedy_advance(argmax_ws, m, n, tokens=None, positions=None, placement=None, valid_lens=None, next_tokens=None):
    """Reduce the lm_head's per-wave candidates to the greedy token of each row and advance the decode
    batch's device state (tokens <- pick, the three counters += 1); returns next_tokens (int64) if given."""
    _chk_cuda(argmax_ws, tokens, positions, placement, valid_lens, next_tokens)
    check(lib().zl_greedy_advance(_p(argmax_ws), _i(m), _i(n), _p(tokens), _p(positions), _p(placement),
                                  _p(valid_lens), _p(next_tokens), _stream()), "greedy_advance")
    return next_tokens


def argmax_advance(logits, tokens=None, positions=None, placement=None, valid_lens=None, next_tokens=None):
    """Greedy pick over whole logit rows (first index of the largest value, as torch.argmax) and the batch state's advance in one
    launch: tokens <- pick (int32), next_tokens <- pick (int64), the three counters += 1."""
    _chk_cuda(tokens, positions, placement, valid_lens, next_tokens)
    if not (logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]):
        raise ZLError("argmax_advance: (rows, n) CUDA logits with unit column stride")
    rows, n = logits.shape
    code = {torch.float16: 2, torch.bfloat16: 6, torch.float32: 1}[logits.dtype]
    check(lib().zl_argmax_advance(_p(logits), C.c_int(code), _i(rows), _i(n), _i(logits.stride(0)), _p(tokens), _p(positions), _p(placement),
                                  _p(valid_lens), _p(next_tokens), _stream()), "argmax_advance")
    return next_tokens if next_tokens is not None else tokens


def spec_accept(logits, drafts, tokens=None, positions=None, placement=None, valid_lens=None, accepted=None, out_tokens=None):
    """Greedy acceptance of a speculative step (zl_spec_accept): logits (B * len_q, n) rows, task-major, unit column stride; drafts
    (B, K) int32, len_q = K + 1.  picks = per-row arg-max (argmax_advance's rule); accepted[b] = length of the longest prefix of
    drafts[b] that the picks confirm; out_tokens[b] = picks[b, :accepted + 1], -1 behind them; tokens <- picks[b, accepted],
    positions / placement / valid_lens += accepted + 1 (each optional).  Returns (accepted (B) int32, out_tokens (B, len_q) int32);
    accepted / out_tokens: buffers to write into (a captured call)."""
    if not (torch.is_tensor(logits) and torch.is_tensor(drafts)):
        raise ZLError("spec_accept: logits and drafts are tensors")
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1] or logits.shape[1] < 1:
        raise ZLError("spec_accept: (B * len_q, n) logits with unit column stride")
    if logits.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ZLError(f"spec_accept: unsupported logits dtype {logits.dtype}")
    if drafts.dim() != 2 or drafts.shape[1] < 1 or drafts.dtype != torch.int32 or not drafts.is_contiguous():
        raise ZLError("spec_accept: drafts are (B, K) contiguous int32, K >= 1")
    b, len_q = drafts.shape[0], drafts.shape[1] + 1
    if b < 1 or logits.shape[0] != b * len_q:
        raise ZLError("spec_accept: one logit row per task and draft position: B * (K + 1) rows")
    if not logits.is_cuda or drafts.device != logits.device:
        raise ZLError("spec_accept: CUDA logits, drafts on the logits' device")
    for t, what in ((tokens, "tokens"), (positions, "positions"), (placement, "placement"), (valid_lens, "valid_lens"), (accepted, "accepted")):
        if t is not None and (t.dtype != torch.int32 or t.numel() != b or not t.is_contiguous() or t.device != logits.device):
            raise ZLError(f"spec_accept: {what}: contiguous int32 of length B on the logits' device")
    if accepted is None:
        accepted = torch.empty(b, dtype=torch.int32, device=logits.device)
    if out_tokens is None:
        out_tokens = torch.empty((b, len_q), dtype=torch.int32, device=logits.device)
    elif out_tokens.dtype != torch.int32 or out_tokens.numel() != b * len_q or not out_tokens.is_contiguous() or out_tokens.device != logits.device:
        raise ZLError("spec_accept: out_tokens: contiguous int32 (B, K + 1) on the logits' device")
    code = {torch.float16: 2, torch.bfloat16: 6, torch.float32: 1}[logits.dtype]
    check(lib().zl_spec_accept(_p(logits), C.c_int(code), _i(b), _i(len_q), _i(logits.shape[1]), _i(logits.stride(0)), _p(drafts), _p(tokens),
                               _p(positions), _p(placement), _p(valid_lens), _p(accepted), _p(out_tokens), _stream()), "spec_accept")
    return accepted, out_tokens.view(b, len_q)


def lookup_draft(history, hist_lens, k, max_ngram=3, min_ngram=1, new_tokens=None, drafts=None, match=None):
    """The drafter of a speculative step by prompt lookup (zl_lookup_draft, one launch): history (B, cap) int32 rows and hist_lens (B)
    int32 are the tasks' token histories, updated in place.  Per task: append the ids of new_tokens[b] (B, n_new <= 32, int32) before its
    first negative one -- a row of spec_accept's out_tokens -- to the row (ids beyond cap are dropped, the length still counts them:
    such a task has overflowed and drafts nothing from then on), then find the longest n-gram (max_ngram down to min_ngram) at the
    history's end that also occurs earlier in it, at the latest start that has k tokens behind it (else the earliest), and propose
    those tokens.  Returns (drafts (B, k) int32, -1 where the history ends or nothing matched; match (B, 2) int32 = (n, start), (0, -1)
    without a match); drafts / match: buffers to write into (a captured call)."""
    if not (torch.is_tensor(history) and torch.is_tensor(hist_lens)):
        raise ZLError("lookup_draft: history and hist_lens are tensors")
    if history.dim() != 2 or history.dtype != torch.int32 or not history.is_contiguous() or history.shape[0] < 1 or history.shape[1] < 2:
        raise ZLError("lookup_draft: history is (B, cap) contiguous int32, cap >= 2")
    b, cap = history.shape
    if cap >= 1 << 31:
        raise ZLError("lookup_draft: a history row holds fewer than 2^31 ids")
    if hist_lens.dtype != torch.int32 or hist_lens.dim() != 1 or hist_lens.numel() != b or not hist_lens.is_contiguous():
        raise ZLError("lookup_draft: hist_lens is (B) contiguous int32")
    k, max_ngram, min_ngram = int(k), int(max_ngram), int(min_ngram)
    if not 1 <= k <= 31:
        raise ZLError("lookup_draft: 1 <= k <= 31 (a verify step has at most 32 rows per task)")
    if not 1 <= min_ngram <= max_ngram <= 16:
        raise ZLError("lookup_draft: 1 <= min_ngram <= max_ngram <= 16")
    n_new = 0
    if new_tokens is not None:
        if not (torch.is_tensor(new_tokens) and new_tokens.dim() == 2 and new_tokens.shape[0] == b and 1 <= new_tokens.shape[1] <= 32
                and new_tokens.dtype == torch.int32 and new_tokens.is_contiguous()):
            raise ZLError("lookup_draft: new_tokens is (B, n_new) contiguous int32, 1 <= n_new <= 32")
        n_new = new_tokens.shape[1]
    if drafts is not None and not (torch.is_tensor(drafts) and drafts.dtype == torch.int32 and drafts.numel() == b * k
                                   and drafts.is_contiguous()):
        raise ZLError("lookup_draft: drafts: contiguous int32 (B, k)")
    if match is not None and not (torch.is_tensor(match) and match.dtype == torch.int32 and match.numel() == b * 2 and match.is_contiguous()):
        raise ZLError("lookup_draft: match: contiguous int32 (B, 2)")
    if not history.is_cuda or any(t is not None and t.device != history.device for t in (hist_lens, new_tokens, drafts, match)):
        raise ZLError("lookup_draft: CUDA history, every other tensor on the history's device")
    if drafts is None:
        drafts = torch.empty((b, k), dtype=torch.int32, device=history.device)
    if match is None:
        match = torch.empty((b, 2), dtype=torch.int32, device=history.device)
    check(lib().zl_lookup_draft(_p(history), _i(cap), _p(hist_lens), _p(new_tokens), _i(n_new), _i(b), _i(k), C.c_int(max_ngram),
                                C.c_int(min_ngram), _p(drafts), _p(match), _stream()), "lookup_draft")
    return drafts.view(b, k), match.view(b, 2)


STOP_IDS_MAX = 16          # stop ids per task
STOP_SEQS_MAX = 8          # stop sequences per task
STOP_SEQ_LEN_MAX = 16      # ids per stop sequence
STOP_TAIL = 15             # emitted ids a task remembers: a sequence's ids but its last
STOP_NEW_MAX = 32          # ids a step emits per task


def stop_rows(stops, vocab):
    """The host half of stop_pack, numpy only: stops = B pairs (stop_ids, stop_sequences) -- a list of ids and a list of id lists, either
    None or empty for none -- over a vocabulary of `vocab` ids -> (stop_ids (B, n_ids) int32, -1 behind a task's ids; stop_seqs
    (B, n_seqs, ld) int32, -1 behind a sequence's ids; seq_lens (B, n_seqs) int32, 0 = unused), each width the longest list's, at least 1.
    Refuses (ZLError) more than 16 ids or 8 sequences per task, a sequence that is empty or longer than 16, and ids outside [0, vocab)."""
    vocab = int(vocab)
    if vocab < 1 or vocab >= 1 << 31:
        raise ZLError("stop_pack: 1 <= vocab < 2^31")
    rows = []
    try:
        for t, pair in enumerate(stops):
            ids, seqs = (None, None) if pair is None else pair
            ids = [] if ids is None else [int(i) for i in ids]
            seqs = [] if seqs is None else [[int(i) for i in s] for s in seqs]
            rows.append((ids, seqs))
    except (TypeError, ValueError):
        raise ZLError("stop_pack: one pair (stop ids, stop sequences) of integer ids per task") from None
    if not rows:
        raise ZLError("stop_pack: one pair (stop ids, stop sequences) of integer ids per task")
    for t, (ids, seqs) in enumerate(rows):
        if len(ids) > STOP_IDS_MAX:
            raise ZLError(f"stop_pack: task {t}: {len(ids)} stop ids, at most {STOP_IDS_MAX}")
        if len(seqs) > STOP_SEQS_MAX:
            raise ZLError(f"stop_pack: task {t}: {len(seqs)} stop sequences, at most {STOP_SEQS_MAX}")
        if any(not 1 <= len(s) <= STOP_SEQ_LEN_MAX for s in seqs):
            raise ZLError(f"stop_pack: task {t}: a stop sequence has 1 .. {STOP_SEQ_LEN_MAX} ids")
        if any(not 0 <= i < vocab for i in ids) or any(not 0 <= i < vocab for s in seqs for i in s):
            raise ZLError(f"stop_pack: task {t}: ids outside [0, {vocab})")
    b = len(rows)
    ids = np.full((b, max([1] + [len(i) for i, _ in rows])), -1, np.int32)
    seqs = np.full((b, max([1] + [len(s) for _, s in rows]), max([1] + [len(q) for _, s in rows for q in s])), -1, np.int32)
    lens = np.zeros(seqs.shape[:2], np.int32)
    for t, (i, s) in enumerate(rows):
        ids[t, :len(i)] = i
        for q, sq in enumerate(s):
            seqs[t, q, :len(sq)], lens[t, q] = sq, len(sq)
    return ids, seqs, lens


def stop_pack(stops, vocab, device):
    """B pairs (stop_ids, stop_sequences) (None = none for that task) -> stop_advance's padded parameter tensors (stop_ids (B, n_ids),
    stop_seqs (B, n_seqs, ld), seq_lens (B, n_seqs)), int32 on `device`; stop_rows states the layout and the refusals."""
    return tuple(torch.from_numpy(a).to(device) for a in stop_rows(stops, vocab))


def stop_advance(stop_ids, stop_seqs, seq_lens, max_new, gen_lens, tail, last_token, finished, new_tokens, accepted=None, next_tokens=None,
                 tokens=None, positions=None, placement=None, valid_lens=None, emit_lens=None, live=None):
    """The stop conditions of a decode step (zl_stop_advance, one launch), directly behind the step's advance / accept call: per task,
    test the ids the step emitted -- new_tokens (B, n_new <= 32) int32, a row's ids before its first negative one; at n_new = 1 it may be
    tokens.view(B, 1) itself -- against the task's stop ids (stop_ids (B, <= 16) int32, -1 = unused), its stop sequences (stop_seqs
    (B, <= 8, <= 16) int32 with seq_lens (B, <= 8), 0 = unused; matched against the task's last 15 emitted ids and the new ones, so across
    steps) and its length limit (max_new (B) int32, <= 0 = none); each of the three may be None.  The first hit ends the task: its row
    keeps the ids up to and including the hit and -1 behind, accepted / tokens / next_tokens and positions / placement / valid_lens
    (each optional) become what a step that emitted only those ids leaves, and finished[b] = 1 (stop id), 2 (stop sequence) or 3
    (length).  A task already finished is frozen: its row becomes -1, accepted and next_tokens -1, the three counters drop by what the
    step added and tokens[b] = last_token[b], so it re-feeds the same token at the same position for good.  State, in place: gen_lens
    (B), tail (B, 15), last_token (B), finished (B), all int32.  Returns (emit_lens (B) int32 = ids each task emitted in this step,
    live (1) int32 = tasks still live); emit_lens / live: buffers to write into (a captured call)."""
    if not (torch.is_tensor(new_tokens) and new_tokens.dim() == 2 and new_tokens.dtype == torch.int32 and new_tokens.is_contiguous()
            and new_tokens.shape[0] >= 1 and new_tokens.shape[1] >= 1):
        raise ZLError("stop_advance: new_tokens is (B, n_new) contiguous int32, n_new >= 1")
    b, n_new = new_tokens.shape
    if n_new > STOP_NEW_MAX:
        raise ZLError(f"stop_advance: at most {STOP_NEW_MAX} new ids per task and step")
    dev = new_tokens.device
    if not new_tokens.is_cuda:
        raise ZLError("stop_advance: CUDA new_tokens, every other tensor on its device")

    def i32(t, shape, what, dtype=torch.int32):
        if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev):
            raise ZLError(f"stop_advance: {what}: contiguous {str(dtype).replace('torch.', '')} {shape} on new_tokens' device"
                          + (" (the state belongs to another batch size?)" if what in ("gen_lens", "tail", "last_token", "finished") else ""))

    for t, shape, what in ((gen_lens, (b,), "gen_lens"), (tail, (b, STOP_TAIL), "tail"), (last_token, (b,), "last_token"),
                           (finished, (b,), "finished")):
        i32(t, shape, what)
    n_ids = n_seqs = ld = 0
    if stop_ids is not None:
        if not (torch.is_tensor(stop_ids) and stop_ids.dim() == 2 and 1 <= stop_ids.shape[1] <= STOP_IDS_MAX):
            raise ZLError(f"stop_advance: stop_ids is (B, 1 .. {STOP_IDS_MAX}) int32")
        n_ids = stop_ids.shape[1]
        i32(stop_ids, (b, n_ids), "stop_ids")
    if (stop_seqs is None) != (seq_lens is None):
        raise ZLError("stop_advance: stop_seqs and seq_lens come together")
    if stop_seqs is not None:
        if not (torch.is_tensor(stop_seqs) and stop_seqs.dim() == 3 and 1 <= stop_seqs.shape[1] <= STOP_SEQS_MAX
                and 1 <= stop_seqs.shape[2] <= STOP_SEQ_LEN_MAX):
            raise ZLError(f"stop_advance: stop_seqs is (B, 1 .. {STOP_SEQS_MAX}, 1 .. {STOP_SEQ_LEN_MAX}) int32")
        n_seqs, ld = stop_seqs.shape[1:]
        i32(stop_seqs, (b, n_seqs, ld), "stop_seqs")
        i32(seq_lens, (b, n_seqs), "seq_lens")
    for t, what in ((max_new, "max_new"), (accepted, "accepted"), (tokens, "tokens"), (positions, "positions"), (placement, "placement"),
                    (valid_lens, "valid_lens"), (emit_lens, "emit_lens")):
        if t is not None:
            i32(t, (b,), what)
    if next_tokens is not None:
        i32(next_tokens, (b,), "next_tokens", torch.int64)
    if live is not None:
        i32(live, (1,), "live")
    if tokens is not None and tokens.data_ptr() == new_tokens.data_ptr() and n_new != 1:
        raise ZLError("stop_advance: new_tokens may be tokens itself at n_new = 1 only")
    if emit_lens is None:
        emit_lens = torch.empty(b, dtype=torch.int32, device=dev)
    if live is None:
        live = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().zl_stop_advance(_p(stop_ids), _i(n_ids), _p(stop_seqs), _p(seq_lens), _i(n_seqs), _i(ld), _p(max_new), _p(gen_lens), _p(tail),
                                _p(last_token), _p(finished), _p(new_tokens), _i(n_new), _i(b), _p(accepted), _p(next_tokens), _p(tokens),
                                _p(positions), _p(placement), _p(valid_lens), _p(emit_lens), _p(live), _stream()), "stop_advance")
    return emit_lens, live


def seen_words(n):
    """The uint32 words of one task's row of a penalty bitmap over n token ids: ceil(n / 32)."""
    return (int(n) + 31) // 32


def seen_mark(seen, tokens, n):
    """Set the bits of the ids tokens[t, :] (int32 (B, n_tok), unit column stride) that lie in [0, n) in the penalty bitmap seen (B, seen_ld)
    uint32-sized words (int32 storage), in place (zl_seen_mark, one launch): token i of task t is bit i & 31 of seen[t, i >> 5].  Ids
    outside [0, n) -- -1 padding -- are skipped.  Seeds a task's set from its prompt or history."""
    if not (torch.is_tensor(seen) and torch.is_tensor(tokens)):
        raise ZLError("seen_mark: seen and tokens are tensors")
    if seen.dtype != torch.int32 or seen.dim() != 2 or not seen.is_contiguous() or seen.shape[1] < seen_words(n) or n < 1:
        raise ZLError("seen_mark: seen is (B, >= ceil(n / 32)) contiguous int32")
    if tokens.dtype != torch.int32 or tokens.dim() != 2 or tokens.shape[0] != seen.shape[0] or tokens.shape[1] < 1 or tokens.stride(1) != 1 \
            or tokens.stride(0) < tokens.shape[1]:
        raise ZLError("seen_mark: tokens are (B, n_tok >= 1) int32 with unit column stride")
    if not seen.is_cuda or tokens.device != seen.device:
        raise ZLError("seen_mark: CUDA tensors on one device")
    check(lib().zl_seen_mark(_p(seen), _i(seen.shape[1]), _i(seen.shape[0]), _i(n), _p(tokens), _i(tokens.shape[1]), _i(tokens.stride(0)),
                             _stream()), "seen_mark")
    return seen


LOGIT_BIAS_MAX = 1024      # bias entries per task
TOP_LOGPROBS_MAX = 32      # top-N alternatives per row


def logit_bias_rows(maps, n):
    """The host half of logit_bias_pack, numpy only: maps = B dicts {token id: bias} (or None = no bias) over n classes ->
    (ids (B, ld) int32, each row's first cnt ascending and -1 behind them; vals (B, ld) float32; cnt (B) int32; bits (B, ceil(n / 32))
    uint32, bit i & 31 of word i >> 5 per id), ld = the longest list, at least 1.  Refuses (ZLError) ids that repeat after int(),
    ids outside [0, n), more than 1024 entries, NaN and +inf values, and finite values beyond float32's range on either side (they
    would turn into +inf or into a ban); -inf is legal and bans the class."""
    n = int(n)
    if n < 1 or n >= 1 << 31:
        raise ZLError("logit_bias_pack: 1 <= n < 2^31 classes")
    maps = [({} if m is None else m) for m in maps]
    if not maps or not all(isinstance(m, dict) for m in maps):
        raise ZLError("logit_bias_pack: one dict {token id: bias} (or None) per task")
    rows = []
    for t, m in enumerate(maps):
        if len(m) > LOGIT_BIAS_MAX:
            raise ZLError(f"logit_bias_pack: task {t}: {len(m)} entries, at most {LOGIT_BIAS_MAX}")
        try:
            pairs = sorted((int(i), float(v)) for i, v in m.items())
        except (TypeError, ValueError):
            raise ZLError(f"logit_bias_pack: task {t}: integer ids and real values") from None
        ids = [i for i, _ in pairs]
        if len(set(ids)) != len(ids):
            raise ZLError(f"logit_bias_pack: task {t}: an id is given twice")
        if ids and (ids[0] < 0 or ids[-1] >= n):
            raise ZLError(f"logit_bias_pack: task {t}: ids outside [0, {n})")
        if any(v != v or v == float("inf") for _, v in pairs):
            raise ZLError(f"logit_bias_pack: task {t}: a bias is finite or -inf (a ban), not NaN or +inf")
        rows.append(pairs)
    ld = max([1] + [len(r) for r in rows])
    ids = np.full((len(rows), ld), -1, np.int32)
    vals = np.zeros((len(rows), ld), np.float32)
    bits = np.zeros((len(rows), seen_words(n)), np.uint32)
    for t, r in enumerate(rows):
        if r:
            i = np.asarray([p[0] for p in r], np.int64)
            ids[t, :i.size] = i
            v64 = np.asarray([p[1] for p in r], np.float64)
            with np.errstate(over="ignore"):
                vals[t, :i.size] = v64.astype(np.float32)
            if (np.isinf(vals[t, :i.size]) & np.isfinite(v64)).any():                   # a finite value must not turn into a ban
                raise ZLError(f"logit_bias_pack: task {t}: a finite bias lies within float32's range")
            np.bitwise_or.at(bits[t], i >> 5, np.uint32(1) << (i & 31).astype(np.uint32))
    return ids, vals, np.asarray([len(r) for r in rows], np.int32), bits


def logit_bias_pack(maps, n, device):
    """B dicts {token id: bias} (None = none for that task) -> the bias argument of sample_advance / spec_sample_accept: the tuple
    (ids (B, ld) int32, vals (B, ld) float32, cnt (B) int32, bits (B, ceil(n / 32)) int32) on `device`; logit_bias_rows states the
    layout and the refusals."""
    ids, vals, cnt, bits = logit_bias_rows(maps, n)
    return (torch.from_numpy(ids).to(device), torch.from_numpy(vals).to(device), torch.from_numpy(cnt).to(device),
            torch.from_numpy(bits.view(np.int32)).to(device))


# ---- slot admission: new requests into slots of a running batch (zl_slots_admit) ---------------------------------------------------
SLOT_MAGIC = 0x534C4F54    # "SLOT"
SLOT_HDR = 16              # header words of the blob
SLOT_REC = 16              # fixed words of a record; the slot's stop rows follow them
SLOT_REQUEST_KEYS = ("temperature", "top_k", "top_p", "seed", "repetition_penalty", "presence_penalty", "penalty_tokens", "logit_bias",
                     "stop_ids", "stop_sequences", "max_new_tokens", "history", "grammar")


def slot_widths(penalties=False, bias_ld=0, n_ids=0, n_seqs=0, seq_ld=0, hist_cap=0, grammar=False):
    """What the states of a batch carry, as slots_pack needs it: penalties = the sampler has a bitmap; bias_ld = the width of its bias
    rows, 0 = no bias; n_ids / n_seqs / seq_ld = the stop state's widths, all 0 = no stop state; hist_cap = ids a lookup history row
    holds, 0 = no drafter; grammar = the sampler carries a token-automaton state."""
    w = dict(penalties=bool(penalties), bias_ld=int(bias_ld), n_ids=int(n_ids), n_seqs=int(n_seqs), seq_ld=int(seq_ld), hist_cap=int(hist_cap),
             grammar=bool(grammar))
    stop = (w["n_ids"], w["n_seqs"], w["seq_ld"])
    if not 0 <= w["bias_ld"] <= LOGIT_BIAS_MAX:
        raise ZLError(f"slots_pack: bias_ld in 0 .. {LOGIT_BIAS_MAX}")
    if stop != (0, 0, 0) and not (1 <= stop[0] <= STOP_IDS_MAX and 1 <= stop[1] <= STOP_SEQS_MAX and 1 <= stop[2] <= STOP_SEQ_LEN_MAX):
        raise ZLError(f"slots_pack: stop widths within (1 .. {STOP_IDS_MAX}, 1 .. {STOP_SEQS_MAX}, 1 .. {STOP_SEQ_LEN_MAX}), or all 0")
    if w["hist_cap"] != 0 and not 2 <= w["hist_cap"] < 1 << 31:
        raise ZLError("slots_pack: hist_cap >= 2, or 0")
    return w


def _f32_bits(v):
    return int(np.float32(v).view(np.int32))


def slot_max_new(prompt_len, max_new, len_buf, k=0):
    """The length limit LLaMA.admit gives a slot: the request's max_new (0 = none) cut so that prompt_len + max_new + k + 1 <= len_buf,
    k = the drafter's K or 0.  A task writes the K/V row of its pending token at prompt_len, one row per emitted id behind it, re-feeds
    its last id at prompt_len + max_new once it has finished, and a speculative step writes k draft rows behind that: the device-side
    length stop (zl_stop_advance, reason 3) then keeps the task inside its buffer with no host count.  < 1: the prompt leaves no room
    for one generated token."""
    room = int(len_buf) - int(prompt_len) - int(k) - 1
    return room if int(max_new) <= 0 else min(int(max_new), room)


def slots_pack(entries, vocab, widths):
    """The host half of an admission, numpy only: entries = (slot, request | None) pairs -- a request is a dict over SLOT_REQUEST_KEYS
    (new_sampler's temperature / top_k / top_p / seed / repetition_penalty / presence_penalty / penalty_tokens / logit_bias, new_stopper's
    stop_ids / stop_sequences / max_new_tokens, new_lookup's history; each optional, with those calls' defaults), None parks the slot --
    over a vocabulary of `vocab` ids, for states of the widths `widths` (slot_widths) -> (blob, header): blob = ONE contiguous int32
    array, include/zhilight_amd.h states its layout at zl_slots_admit; header = its first 16 words as a dict (magic, n, vocab, flags,
    bias_ld, n_ids, n_seqs, seq_ld, rec, var, total, hist_cap).  The checks are new_sampler's, new_stopper's and new_lookup's, raised as
    ZLError before anything is launched; a request that uses an option the states do not carry is refused: penalties without a bitmap,
    a bias without bias rows or with more ids than bias_ld, stop conditions without a stop state or beyond its widths, a history
    without a drafter or longer than hist_cap - 1, a grammar without an automaton state.  Slots are distinct and >= 0 (slots_admit
    checks them against the batch).
    "grammar": the slot's start state in the sampler's automaton tables (LLaMA.load_grammar's handle), or a (start state, pending token)
    pair whose second entry replaces the slot's pending token at admission (LLaMA.admit gives the prompt's last id: the first
    generated token is then drawn under the grammar).  Only a blob with such a request carries header flag 16 and the (n, 2) side array
    at the word offset of header word 12; without one the blob is what it always was."""
    vocab = int(vocab)
    if vocab < 1 or vocab >= 1 << 31:
        raise ZLError("slots_pack: 1 <= vocab < 2^31")
    w = slot_widths(**widths)
    entries = list(entries)
    if not entries:
        raise ZLError("slots_pack: at least one (slot, request) entry")
    has_stop = w["n_ids"] > 0
    rec = SLOT_REC + w["n_ids"] + w["n_seqs"] + w["n_seqs"] * w["seq_ld"]
    recs, var, slots = [], [], []
    gram = np.full((len(entries), 2), -1, np.int32)                         # (start state, pending-token override) per record
    any_gram = False
    off = SLOT_HDR + len(entries) * rec

    def ints(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)

    def id_array(v, what, s):
        a = np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= vocab):
            raise ZLError(f"slots_pack: slot {s}: {what} outside [0, {vocab})")
        return a.astype(np.int32)

    for ent in entries:
        try:
            s, req = ent
        except (TypeError, ValueError):
            raise ZLError("slots_pack: an entry is (slot, request | None)") from None
        if not ints(s) or int(s) < 0 or int(s) >= 1 << 31:
            raise ZLError("slots_pack: a slot is an integer >= 0")
        s = int(s)
        if s in slots:
            raise ZLError(f"slots_pack: slot {s} is given twice")
        slots.append(s)
        r = np.zeros(rec, np.int32)
        r[0] = s
        if has_stop:
            r[SLOT_REC:SLOT_REC + w["n_ids"]] = -1
            r[SLOT_REC + w["n_ids"] + w["n_seqs"]:] = -1
        if req is None:
            recs.append(r)
            continue
        if not isinstance(req, dict) or any(k not in SLOT_REQUEST_KEYS for k in req):
            raise ZLError(f"slots_pack: slot {s}: a request is a dict over {', '.join(SLOT_REQUEST_KEYS)}")
        t, k, p, sd = req.get("temperature", 1.0), req.get("top_k", 0), req.get("top_p", 1.0), req.get("seed", 0)
        rp, pp = req.get("repetition_penalty", 1.0), req.get("presence_penalty", 0.0)
        try:
            if not (float(t) >= 0.0 and math.isfinite(float(t))):
                raise ZLError(f"slots_pack: slot {s}: temperature >= 0 (0 = greedy)")
            if int(k) != k or int(k) < 0 or int(k) >= 1 << 31:
                raise ZLError(f"slots_pack: slot {s}: top_k is an integer >= 0 (0 = off)")
            if not 0.0 <= float(p) <= 1.0:
                raise ZLError(f"slots_pack: slot {s}: top_p in [0, 1]")
            if int(sd) != sd:
                raise ZLError(f"slots_pack: slot {s}: seed is an integer")
            if not (float(rp) > 0.0 and math.isfinite(float(rp))):
                raise ZLError(f"slots_pack: slot {s}: repetition_penalty > 0 and finite (1 = off)")
            if not math.isfinite(float(pp)):
                raise ZLError(f"slots_pack: slot {s}: presence_penalty is finite (0 = off)")
        except (TypeError, ValueError):
            raise ZLError(f"slots_pack: slot {s}: temperature, top_k, top_p, seed and the penalties are numbers") from None
        sd = int(sd) % (1 << 64)                                            # the 64 bits of the key
        r[1] = 1
        r[2], r[3], r[4] = _f32_bits(t), int(k), _f32_bits(p)
        r[5:7] = np.array([sd & 0xFFFFFFFF, sd >> 32], np.uint32).view(np.int32)
        r[7], r[8] = _f32_bits(rp), _f32_bits(pp)
        pen = req.get("penalty_tokens")
        if not w["penalties"] and (pen is not None or float(rp) != 1.0 or float(pp) != 0.0):
            raise ZLError(f"slots_pack: slot {s}: penalties, but the sampler state has no bitmap")
        pen = np.zeros(0, np.int32) if pen is None else id_array(pen, "penalty_tokens", s)
        r[10], r[11] = off, pen.size
        var.append(pen)
        off += pen.size
        bias = req.get("logit_bias")
        if bias is not None and not isinstance(bias, dict):
            raise ZLError(f"slots_pack: slot {s}: logit_bias is one dict {{token id: bias}}")
        if bias:
            if not w["bias_ld"]:
                raise ZLError(f"slots_pack: slot {s}: a logit bias, but the sampler state has no bias rows")
            try:
                ids, vals, cnt, _ = logit_bias_rows([bias], vocab)
            except ZLError as e:
                raise ZLError(f"slots_pack: slot {s}: {e}") from None
            if int(cnt[0]) > w["bias_ld"]:
                raise ZLError(f"slots_pack: slot {s}: {int(cnt[0])} bias ids, the sampler state holds {w['bias_ld']}")
            r[12], r[13] = off, int(cnt[0])
            var += [ids[0, :cnt[0]], vals[0, :cnt[0]].view(np.int32)]
            off += 2 * int(cnt[0])
        else:
            r[12], r[13] = off, 0
        sid, ssq, lim = req.get("stop_ids"), req.get("stop_sequences"), req.get("max_new_tokens", 0)
        if not ints(lim) or not 0 <= int(lim) < 1 << 31:
            raise ZLError(f"slots_pack: slot {s}: max_new_tokens is an integer >= 0 (0 = no limit)")
        sid = [sid] if ints(sid) else sid
        if not has_stop and (sid or ssq or int(lim)):
            raise ZLError(f"slots_pack: slot {s}: stop conditions, but there is no stop state")
        if has_stop:
            try:
                ids, seqs, lens = stop_rows([(sid, ssq)], vocab)
            except ZLError as e:
                raise ZLError(f"slots_pack: slot {s}: {e}") from None
            if len(sid or []) > w["n_ids"] or len(ssq or []) > w["n_seqs"] or (len(ssq or []) and seqs.shape[2] > w["seq_ld"]):
                raise ZLError(f"slots_pack: slot {s}: stop conditions beyond the stop state's widths "
                              f"({w['n_ids']} ids, {w['n_seqs']} sequences of {w['seq_ld']} ids)")
            q = SLOT_REC
            r[q:q + len(sid or [])] = ids[0, :len(sid or [])]
            q += w["n_ids"]
            r[q:q + len(ssq or [])] = lens[0, :len(ssq or [])]
            q += w["n_seqs"]
            sq = r[q:].reshape(w["n_seqs"], w["seq_ld"])
            for j in range(len(ssq or [])):
                sq[j, :lens[0, j]] = seqs[0, j, :lens[0, j]]
            r[9] = int(lim)
        hist = req.get("history")
        if hist is not None and not w["hist_cap"]:
            raise ZLError(f"slots_pack: slot {s}: a history, but there is no lookup state")
        hist = np.zeros(0, np.int32) if hist is None else id_array(hist, "history ids", s)
        if w["hist_cap"] and hist.size > w["hist_cap"] - 1:
            raise ZLError(f"slots_pack: slot {s}: {hist.size} ids and the pending token do not fit cap = {w['hist_cap']}")
        r[14], r[15] = off, hist.size
        var.append(hist)
        off += hist.size
        g = req.get("grammar")
        if g is not None:
            if not w["grammar"]:
                raise ZLError(f"slots_pack: slot {s}: a grammar, but the sampler state has no automaton")
            g = (g, -1) if ints(g) else g
            if not (isinstance(g, (tuple, list)) and len(g) == 2 and ints(g[0]) and (g[1] is None or ints(g[1]))):
                raise ZLError(f"slots_pack: slot {s}: grammar is a start state or a (start state, pending token) pair")
            st, pend = int(g[0]), -1 if g[1] is None else int(g[1])
            if not 0 <= st < 1 << 31 or not -1 <= pend < vocab:
                raise ZLError(f"slots_pack: slot {s}: grammar: a start state >= 0 and a pending token in [0, {vocab}) or -1")
            gram[len(recs)] = (st, pend)
            any_gram = True
        recs.append(r)
    gram_off = 0
    if any_gram:
        gram_off = off
        var.append(gram.reshape(-1))
        off += gram.size
    if off >= 1 << 31:
        raise ZLError("slots_pack: the blob holds fewer than 2^31 words")
    flags = ((1 if w["penalties"] else 0) | (2 if w["bias_ld"] else 0) | (4 if has_stop else 0) | (8 if w["hist_cap"] else 0)
             | (16 if any_gram else 0))
    hdr = np.zeros(SLOT_HDR, np.int32)
    hdr[12] = gram_off
    hdr[:12] = [SLOT_MAGIC, len(entries), vocab, flags, w["bias_ld"], w["n_ids"], w["n_seqs"], w["seq_ld"], rec,
                SLOT_HDR + len(entries) * rec, off, w["hist_cap"]]
    blob = np.ascontiguousarray(np.concatenate([hdr] + recs + [np.asarray(v, np.int32) for v in var]))
    assert blob.size == off
    return blob, slots_header(blob)


def slots_header(blob):
    """the header of a slots_pack blob as a dict; refuses (ZLError) what is not such a blob"""
    names = ("magic", "n", "vocab", "flags", "bias_ld", "n_ids", "n_seqs", "seq_ld", "rec", "var", "total", "hist_cap")
    if not (isinstance(blob, np.ndarray) and blob.dtype == np.int32 and blob.ndim == 1 and blob.size >= SLOT_HDR and blob.flags.c_contiguous):
        raise ZLError("slots_admit: the blob is slots_pack's contiguous int32 array")
    h = dict(zip(names, (int(v) for v in blob[:12])))
    if (h["magic"] != SLOT_MAGIC or h["total"] != blob.size or h["n"] < 1 or h["rec"] < SLOT_REC
            or h["var"] != SLOT_HDR + h["n"] * h["rec"] or h["var"] > h["total"]
            or h["rec"] != SLOT_REC + h["n_ids"] + h["n_seqs"] + h["n_seqs"] * h["seq_ld"]):
        raise ZLError("slots_admit: the blob is slots_pack's contiguous int32 array")
    if h["flags"] & 16:                                                     # the (n, 2) grammar side array
        h["grammar"] = int(blob[12])
        if not h["var"] <= h["grammar"] <= h["total"] - 2 * h["n"]:
            raise ZLError("slots_admit: the blob is slots_pack's contiguous int32 array")
    return h


def slots_records(blob):
    """the records of a slots_pack blob: (n, rec) int32, a view"""
    h = slots_header(blob)
    return blob[SLOT_HDR:h["var"]].reshape(h["n"], h["rec"])


def slots_admit(blob, tokens, positions, placement, valid_lens, sampler=None, stop=None, lookup=None, draft_new=None, parked_ok=None):
    """Admit requests into slots of a running batch (zl_slots_admit: one upload of the blob, ONE launch): blob = slots_pack's array
    (a numpy array: uploaded here; or a (device int32 tensor, numpy array) pair from an earlier upload, for a captured launch);
    tokens / positions / placement / valid_lens (B) int32 = the batch state, tokens[s] holding the pending token the prompt encode
    left.  sampler / stop / lookup: objects with LLaMA's SamplerState / StopState / LookupState fields (None = that group is skipped);
    their optional tensors and widths must be those the blob was packed for (ZLError otherwise, and for slots outside [0, B)).
    draft_new (B) int32, optional: receives the drafter's new_tokens column (pending for admitted slots, -1 elsewhere).
    A sampler that carries an automaton state (fsm_state (B) int32) goes through zl_slots_admit_fsm: an admitted slot's state <- its
    request's start state (-1 without a grammar), a (start, pending) grammar also replaces the pending token, a parked slot's <- -1.
    parked_ok: the slots the caller knows to be finished; parking any other slot is refused.  The rule: include/zhilight_amd.h."""
    dev_blob = None
    if isinstance(blob, (tuple, list)):
        dev_blob, blob = blob
    h = slots_header(blob)
    recs = slots_records(blob)
    if not (torch.is_tensor(tokens) and tokens.is_cuda and tokens.dtype == torch.int32 and tokens.dim() == 1 and tokens.is_contiguous()):
        raise ZLError("slots_admit: tokens is (B) contiguous int32 on the device")
    b, dev = tokens.numel(), tokens.device

    def chk(t, shape, dtype, what):
        if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == dev):
            raise ZLError(f"slots_admit: {what}: contiguous {str(dtype).replace('torch.', '')} {tuple(shape)} on the tokens' device")

    for t, what in ((positions, "positions"), (placement, "placement"), (valid_lens, "valid_lens")):
        chk(t, (b,), torch.int32, what)
    if recs[:, 0].min() < 0 or recs[:, 0].max() >= b or len(set(recs[:, 0].tolist())) != h["n"]:
        raise ZLError(f"slots_admit: slots must be distinct indices of the batch of {b}")
    parks = recs[recs[:, 1] == 0, 0].tolist()
    if parks and (parked_ok is None or any(s not in parked_ok for s in parks)):
        raise ZLError("slots_admit: only a slot known to be finished is parked")
    words = seen_words(h["vocab"])
    i32, f32, i64 = torch.int32, torch.float32, torch.int64
    args = []
    sm = sampler
    if sm is not None:
        for name, dt in (("temperature", f32), ("top_k", i32), ("top_p", f32), ("seeds", i64), ("draws", i64), ("logprobs", f32), ("u", f32)):
            chk(getattr(sm, name), (b,), dt, name)
        args += [sm.temperature, sm.top_k, sm.top_p, sm.seeds, sm.draws, sm.logprobs, sm.u]
    else:
        args += [None] * 7
    has_pen = sm is not None and sm.seen is not None
    if has_pen != bool(h["flags"] & 1):
        raise ZLError("slots_admit: the blob and the sampler state differ in the penalty bitmap")
    if has_pen:
        chk(sm.repetition_penalty, (b,), f32, "repetition_penalty")
        chk(sm.presence_penalty, (b,), f32, "presence_penalty")
        if not (sm.seen.dim() == 2 and sm.seen.shape[1] >= words):
            raise ZLError("slots_admit: seen: contiguous int32 (B, >= ceil(vocab / 32))")
        chk(sm.seen, (b, sm.seen.shape[1]), i32, "seen")
        args += [sm.repetition_penalty, sm.presence_penalty, sm.seen, sm.seen.shape[1]]
    else:
        args += [None, None, None, 0]
    has_bias = sm is not None and sm.bias_ids is not None
    if (sm.bias_ids.shape[1] if has_bias and sm.bias_ids.dim() == 2 else 0) != h["bias_ld"]:
        raise ZLError("slots_admit: the blob and the sampler state differ in the bias width")
    if has_bias:
        chk(sm.bias_ids, (b, h["bias_ld"]), i32, "bias_ids")
        chk(sm.bias_vals, (b, h["bias_ld"]), f32, "bias_vals")
        chk(sm.bias_cnt, (b,), i32, "bias_cnt")
        if not (torch.is_tensor(sm.bias_bits) and sm.bias_bits.dim() == 2 and sm.bias_bits.shape[1] >= words):
            raise ZLError("slots_admit: bias_bits: contiguous int32 (B, >= ceil(vocab / 32))")
        chk(sm.bias_bits, (b, sm.bias_bits.shape[1]), i32, "bias_bits")
        args += [sm.bias_ids, sm.bias_vals, sm.bias_cnt, sm.bias_bits, h["bias_ld"], sm.bias_bits.shape[1]]
    else:
        args += [None, None, None, None, 0, 0]
    top_n = int(sm.top_n) if sm is not None and sm.top_n else 0
    if top_n:
        chk(sm.top_ids, (b, top_n), i32, "top_ids")
        chk(sm.top_logprobs, (b, top_n), f32, "top_logprobs")
        args += [sm.top_ids, sm.top_logprobs, top_n]
    else:
        args += [None, None, 0]
    if (stop is not None) != bool(h["flags"] & 4):
        raise ZLError("slots_admit: the blob and the stop state differ")
    if stop is not None:
        if (tuple(stop.stop_ids.shape[1:]), tuple(stop.stop_seqs.shape[1:])) != ((h["n_ids"],), (h["n_seqs"], h["seq_ld"])):
            raise ZLError("slots_admit: the blob and the stop state differ in their widths")
        chk(stop.stop_ids, (b, h["n_ids"]), i32, "stop_ids")
        chk(stop.stop_seqs, (b, h["n_seqs"], h["seq_ld"]), i32, "stop_seqs")
        chk(stop.seq_lens, (b, h["n_seqs"]), i32, "seq_lens")
        chk(stop.tail, (b, STOP_TAIL), i32, "tail")
        chk(stop.live, (1,), i32, "live")
        for name in ("max_new", "gen_lens", "last_token", "finished", "emit_lens"):
            chk(getattr(stop, name), (b,), i32, name)
        args += [stop.stop_ids, stop.stop_seqs, stop.seq_lens, h["n_ids"], h["n_seqs"], h["seq_ld"], stop.max_new, stop.gen_lens, stop.tail,
                 stop.last_token, stop.finished, stop.emit_lens, stop.live]
    else:
        args += [None, None, None, 0, 0, 0] + [None] * 7
    if (lookup.history.shape[1] if lookup is not None else 0) != h["hist_cap"]:
        raise ZLError("slots_admit: the blob and the lookup state differ in the history's cap")
    if lookup is not None:
        chk(lookup.history, (b, h["hist_cap"]), i32, "history")
        chk(lookup.hist_lens, (b,), i32, "hist_lens")
        args += [lookup.history, h["hist_cap"], lookup.hist_lens]
    else:
        args += [None, 0, None]
    if draft_new is not None:
        chk(draft_new, (b,), i32, "draft_new")
    fsm_state = getattr(sm, "fsm_state", None) if sm is not None else None
    if fsm_state is None and h["flags"] & 16:
        raise ZLError("slots_admit: the blob carries grammar requests, the sampler state has no automaton")
    if fsm_state is not None:
        chk(fsm_state, (b,), i32, "fsm_state")
    if dev_blob is None:
        dev_blob = torch.from_numpy(blob).to(dev)
    elif not (torch.is_tensor(dev_blob) and dev_blob.dtype == i32 and dev_blob.numel() == blob.size and dev_blob.is_contiguous()
              and dev_blob.device == dev):
        raise ZLError("slots_admit: the uploaded blob is the int32 tensor of the numpy blob, on the tokens' device")
    cargs = [_i(v) if isinstance(v, int) else _p(v) for v in args]
    if fsm_state is not None:
        check(lib().zl_slots_admit_fsm(_p(dev_blob), _i(h["n"]), _i(h["rec"]), _i(b), _i(h["vocab"]), _p(tokens), _p(positions), _p(placement),
                                       _p(valid_lens), *cargs, _p(draft_new), _p(fsm_state), _stream()), "slots_admit")
        return dev_blob
    check(lib().zl_slots_admit(_p(dev_blob), _i(h["n"]), _i(h["rec"]), _i(b), _i(h["vocab"]), _p(tokens), _p(positions), _p(placement),
                               _p(valid_lens), *cargs, _p(draft_new), _stream()), "slots_admit")
    return dev_blob


def grammar_tables(packed, device):
    """grammar.TokenAutomaton.pack()'s five arrays as the `fsm` tuple of sample_advance / spec_sample_accept: int32 tensors on the device
    (the bitmap's uint32 words viewed as int32, as seen)"""
    mask, default, exc_off, exc_tok, exc_next = packed
    return (torch.from_numpy(np.ascontiguousarray(mask).view(np.int32)).to(device), torch.from_numpy(np.ascontiguousarray(default)).to(device),
            torch.from_numpy(np.ascontiguousarray(exc_off)).to(device), torch.from_numpy(np.ascontiguousarray(exc_tok)).to(device),
            torch.from_numpy(np.ascontiguousarray(exc_next)).to(device))


def _sample_logits(what, rows_text, logits, **first):
    """The checks of the logits of sample_advance / spec_sample_accept; first = the required tensors the first message names with them."""
    names = list(first)
    if not all(torch.is_tensor(t) for t in (logits, *first.values())):
        raise ZLError(f"{what}: logits, {', '.join(names[:-1])} and {names[-1]} are tensors")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1 or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        raise ZLError(f"{what}: {rows_text} logits with unit column stride")
    if logits.dtype not in (torch.float16, torch.bfloat16):
        raise ZLError(f"{what}: fp16 or bf16 logits, not {logits.dtype} (the selection works on the 16-bit pattern)")
    if logits.shape[1] >= 1 << 31:
        raise ZLError(f"{what}: a row holds fewer than 2^31 classes")


def _sample_tensors(what, logits, one_dim, required, generator, optional):
    """The checks of the per-row / per-task tensors of sample_advance / spec_sample_accept, each entry (tensor, dtype, elements, name,
    the message's shape text): the required ones, the generator triple (seeds, draws, u), the optional ones (None = not given), and
    last that all of them are on the CUDA device of the logits.  one_dim: every tensor is 1-D."""
    def sized(t, dtype, count, name, text):
        if not (torch.is_tensor(t) and t.dtype == dtype and t.numel() == count and t.is_contiguous() and (t.dim() == 1 or not one_dim)):
            raise ZLError(f"{what}: {name}: contiguous {str(dtype).replace('torch.', '')} {text}")

    for entry in required:
        sized(*entry)
    seeds, draws, u = generator
    if u[0] is not None:
        sized(*u)
    elif seeds[0] is None or draws[0] is None:
        raise ZLError(f"{what}: give seeds and draws, or u")
    if u[0] is None or seeds[0] is not None:
        sized(*seeds)
    if u[0] is None or draws[0] is not None:
        sized(*draws)
    for entry in optional:
        if entry[0] is not None:
            sized(*entry)
    if not logits.is_cuda or any(e[0] is not None and e[0].device != logits.device for e in (*required, *generator, *optional)):
        raise ZLError(f"{what}: CUDA logits, every other tensor on the logits' device")


def _sample_opts(what, count, top_shape, n, device, rep_penalty, presence, seen, bias, top_n, top_ids, top_logprobs, fsm, fsm_state,
                 row_states=None):
    """The checks of the options of sample_advance / spec_sample_accept -> their zl_sample_opts_t (by reference), None when nothing is
    on.  count = the rows / tasks the options are per, top_shape = the leading shape of the top-N outputs (and of row_states, the
    speculative call's).
    The struct holds addresses only: the caller keeps the tensors referenced until the C call has returned (its arguments are)."""
    o = SampleOpts()
    if seen is None:
        if rep_penalty is not None or presence is not None:
            raise ZLError(f"{what}: rep_penalty / presence act on the classes of seen: give the bitmap")
    else:
        for t, name in ((rep_penalty, "rep_penalty"), (presence, "presence")):
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == count and t.is_contiguous()):
                raise ZLError(f"{what}: {name}: contiguous float32 of length {count}, given with seen")
        if not (torch.is_tensor(seen) and seen.dtype == torch.int32 and seen.dim() == 2 and seen.shape[0] == count and seen.is_contiguous()
                and seen.shape[1] >= seen_words(n)):
            raise ZLError(f"{what}: seen: contiguous int32 ({count}, >= ceil(n / 32))")
        if any(t.device != device for t in (rep_penalty, presence, seen)):
            raise ZLError(f"{what}: CUDA logits, every other tensor on the logits' device")
        o.rep_penalty, o.presence, o.seen, o.seen_ld = rep_penalty.data_ptr(), presence.data_ptr(), seen.data_ptr(), seen.shape[1]
    if row_states is not None:
        if not (torch.is_tensor(row_states) and row_states.dtype == torch.int32 and row_states.numel() == math.prod(top_shape)
                and row_states.is_contiguous()):
            raise ZLError(f"{what}: row_states: contiguous int32 (B, K + 1)")
        if row_states.device != device:
            raise ZLError(f"{what}: CUDA logits, every other tensor on the logits' device")
        o.fsm_row_states = row_states.data_ptr()
    if bias is not None:
        if not (isinstance(bias, (tuple, list)) and len(bias) == 4 and all(torch.is_tensor(t) for t in bias)):
            raise ZLError(f"{what}: bias is logit_bias_pack's (ids, vals, cnt, bits)")
        ids, vals, cnt, bits = bias
        if not (ids.dtype == torch.int32 and ids.dim() == 2 and ids.shape[0] == count and ids.is_contiguous()
                and 1 <= ids.shape[1] <= LOGIT_BIAS_MAX):
            raise ZLError(f"{what}: bias ids: contiguous int32 ({count}, 1 .. {LOGIT_BIAS_MAX})")
        if not (vals.dtype == torch.float32 and vals.shape == ids.shape and vals.is_contiguous()):
            raise ZLError(f"{what}: bias vals: contiguous float32 of the ids' shape")
        if not (cnt.dtype == torch.int32 and cnt.dim() == 1 and cnt.numel() == count and cnt.is_contiguous()):
            raise ZLError(f"{what}: bias cnt: contiguous int32 of length {count}")
        if not (bits.dtype == torch.int32 and bits.dim() == 2 and bits.shape[0] == count and bits.is_contiguous()
                and bits.shape[1] >= seen_words(n)):
            raise ZLError(f"{what}: bias bits: contiguous int32 ({count}, >= ceil(n / 32))")
        if any(t.device != device for t in bias):
            raise ZLError(f"{what}: CUDA logits, every other tensor on the logits' device")
        o.bias_ids, o.bias_vals, o.bias_cnt, o.bias_ld = ids.data_ptr(), vals.data_ptr(), cnt.data_ptr(), ids.shape[1]
        o.bias_bits, o.bias_bits_ld = bits.data_ptr(), bits.shape[1]
    top_n = int(top_n)
    if not 0 <= top_n <= TOP_LOGPROBS_MAX:
        raise ZLError(f"{what}: top_n in 0 .. {TOP_LOGPROBS_MAX}")
    if top_n:
        shape = tuple(top_shape) + (top_n,)
        for t, dtype, name in ((top_ids, torch.int32, "top_ids"), (top_logprobs, torch.float32, "top_logprobs")):
            if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.device == device):
                raise ZLError(f"{what}: {name}: contiguous {str(dtype).replace('torch.', '')} {shape} on the logits' device, given with top_n")
        o.top_n, o.top_ids, o.top_logprobs = top_n, top_ids.data_ptr(), top_logprobs.data_ptr()
    if fsm is not None:
        if not (isinstance(fsm, (tuple, list)) and len(fsm) == 5 and all(torch.is_tensor(t) and t.dtype == torch.int32 and t.is_contiguous()
                                                                         for t in fsm)):
            raise ZLError(f"{what}: fsm is (mask, default, exc_off, exc_tok, exc_next), contiguous int32 tensors (grammar_tables)")
        mask, default, exc_off, exc_tok, exc_next = fsm
        if not (mask.dim() == 2 and default.dim() == 1 and exc_off.dim() == 1 and exc_tok.dim() == 1 and exc_next.dim() == 1
                and mask.shape[0] >= 1 and default.numel() == mask.shape[0] and exc_off.numel() == mask.shape[0] + 1
                and exc_next.numel() == exc_tok.numel() and mask.shape[1] >= seen_words(n)):
            raise ZLError(f"{what}: fsm: mask (S, >= ceil(n / 32)), default (S), exc_off (S + 1), exc_tok / exc_next (E)")
        if not (torch.is_tensor(fsm_state) and fsm_state.dtype == torch.int32 and fsm_state.dim() == 1 and fsm_state.numel() == count
                and fsm_state.is_contiguous()):
            raise ZLError(f"{what}: fsm_state: contiguous int32 of length {count}, given with fsm")
        if any(t.device != device for t in tuple(fsm) + (fsm_state,)):
            raise ZLError(f"{what}: CUDA logits, every other tensor on the logits' device")
        if exc_tok.numel() == 0:                                            # no exception anywhere: the lists are never read
            exc_tok = exc_next = exc_off
        o.fsm_mask, o.fsm_mask_ld, o.fsm_default, o.fsm_exc_off = mask.data_ptr(), mask.shape[1], default.data_ptr(), exc_off.data_ptr()
        o.fsm_exc_tok, o.fsm_exc_next, o.fsm_states, o.fsm_exceptions = exc_tok.data_ptr(), exc_next.data_ptr(), mask.shape[0], fsm[3].numel()
        o.fsm_state = fsm_state.data_ptr()
    return C.byref(o) if seen is not None or bias is not None or top_n or fsm is not None else None


def sample_advance(logits, temperature, top_k, top_p, seeds=None, draws=None, u=None, tokens=None, positions=None, placement=None,
                   valid_lens=None, next_tokens=None, logprobs=None, u_out=None, rep_penalty=None, presence=None, seen=None,
                   bias=None, top_n=0, top_ids=None, top_logprobs=None, fsm=None, fsm_state=None):
    """The stochastic pick over whole logit rows and the batch state's advance in one launch (zl_sample_advance): logits (rows, n)
    fp16 / bf16 with unit column stride; temperature (rows) fp32, top_k (rows) int32 (<= 0 or >= n: off), top_p (rows) fp32 in [0, 1]
    -- per row.  A row with temperature <= 0 takes argmax_advance's pick; otherwise p = exp((x - max) / T), the classes ordered by p
    descending (ties to the lower index), c their running sum, Z its end, cap = min(top_p, c[k-1] / Z) (top_p without top-k), and the
    pick is the first class of the order with c >= u * cap * Z.  u (rows) fp32 in [0, 1) gives the uniforms; without it they are
    Philox4x32-10 words keyed by seeds[r] (int64) and counted by draws[r] (int64), and draws += 1.  tokens <- pick (int32),
    next_tokens <- pick (int64), positions / placement / valid_lens += 1 (each optional, tokens or next_tokens required); logprobs
    (rows) fp32 <- the pick's tempered log-probability (T <= 0: at T = 1); u_out (rows) fp32 <- the uniforms used.  Returns
    next_tokens if given, else tokens.  The options below travel as one zl_sample_opts_t to zl_sample_advance_ex.
    seen (rows, >= ceil(n / 32)) int32, a bitmap of token ids per row (seen_words, seen_mark), with rep_penalty / presence (rows) fp32:
    the penalty group -- a class whose bit is set is read as repetition_penalty's value of it (presence != 0 ? x - T(presence) :
    x < 0 ? x * T(factor) : x / T(factor)), the rule above runs on that row, logprobs is the penalised distribution's, the logits in
    memory stay as they are, and the pick's bit is set in seen: the same results as repetition_penalty over the set + this call
    without seen, in the one launch.
    bias = logit_bias_pack's tuple, per row: the bias group -- a class of the row's bias set is read as T(f32(y) + f32(T(bias))),
    y = the class after the penalty (scatter_logits(add=True)'s expression; -inf bans the class); the bias enters neither seen nor the
    logits in memory, and needs no seen.  top_n = N in 1 .. 32 with top_ids (rows, N) int32 / top_logprobs (rows, N) fp32: the first
    min(N, n) classes of the row AS THE PICK SAW IT, larger value first, then lower index, with their tempered log-probabilities
    (the pick's entry is bit-equal to logprobs); -1 / NaN behind n and on a row whose largest value is NaN or +-inf.  The same
    results as repetition_penalty + scatter_logits(add=True) + this call without them, in the one launch.
    fsm = grammar_tables' five tensors with fsm_state (rows) int32: the automaton group -- a row whose state s lies in [0, S) reads
    every class whose bit is clear in mask[s] as -inf (in front of the penalty and the bias; the logits in memory stay), everything
    above runs on that row, and fsm_state <- delta(s, pick): the exception's target where exc_tok[exc_off[s] : exc_off[s + 1]] holds the
    pick, else default[s].  A state outside [0, S) leaves the row unconstrained and is not changed.  The same results as
    masked_fill(-inf) on a copy + this call without fsm."""
    what = "sample_advance"
    if (fsm is None) != (fsm_state is None):
        raise ZLError(f"{what}: fsm and fsm_state are given together")
    _sample_logits(what, "(rows, n)", logits, temperature=temperature, top_k=top_k, top_p=top_p)
    rows, n = logits.shape
    if tokens is None and next_tokens is None:
        raise ZLError(f"{what}: give tokens or next_tokens")
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    per_row = lambda t, dtype, name: (t, dtype, rows, name, "of length rows")                      # noqa: E731
    _sample_tensors(what, logits, True, [per_row(temperature, f32, "temperature"), per_row(top_k, i32, "top_k"), per_row(top_p, f32, "top_p")],
                    [per_row(seeds, i64, "seeds"), per_row(draws, i64, "draws"), per_row(u, f32, "u")],
                    [per_row(tokens, i32, "tokens"), per_row(positions, i32, "positions"), per_row(placement, i32, "placement"),
                     per_row(valid_lens, i32, "valid_lens"), per_row(next_tokens, i64, "next_tokens"), per_row(logprobs, f32, "logprobs"),
                     per_row(u_out, f32, "u_out")])
    opts = _sample_opts(what, rows, (rows,), n, logits.device, rep_penalty, presence, seen, bias, top_n, top_ids, top_logprobs, fsm, fsm_state)
    check(lib().zl_sample_advance_ex(_p(logits), C.c_int(2 if logits.dtype == torch.float16 else 6), _i(rows), _i(n), _i(logits.stride(0)),
                                     _p(temperature), _p(top_k), _p(top_p), _p(seeds), _p(draws), _p(u), _p(tokens), _p(positions),
                                     _p(placement), _p(valid_lens), _p(next_tokens), _p(logprobs), _p(u_out), opts, _stream()), what)
    return next_tokens if next_tokens is not None else tokens


def spec_sample_accept(logits, drafts, temperature, top_k, top_p, seeds=None, draws=None, u=None, tokens=None, positions=None,
                       placement=None, valid_lens=None, accepted=None, out_tokens=None, out_logprobs=None, logprobs=None, u_out=None,
                       rep_penalty=None, presence=None, seen=None, bias=None, top_n=0, top_ids=None, top_logprobs=None, fsm=None,
                       fsm_state=None, row_states=None):
    """The acceptance of a speculative step under sampling (zl_spec_sample_accept, two launches): spec_accept with sample_advance's
    pick in the arg-max's place.  logits (B * len_q, n) fp16 / bf16 rows, task-major, unit column stride; drafts (B, K) int32,
    len_q = K + 1 <= 32.  temperature / top_k / top_p / seeds / draws are per task (B); u, u_out and out_logprobs per row (B, len_q).
    picks[b, i] = sample_advance's pick of row (b, i) under task b's parameters with the uniform u[b, i], or without u the Philox
    word of seeds[b] at counter draws[b] + i.  The drafter's proposal is a point mass, so "draw x ~ p, accept iff x == draft, else
    emit x" IS the optimal speculative-sampling rule: accepted[b] = length of the longest prefix of drafts[b] the picks confirm,
    out_tokens[b] = picks[b, :accepted + 1], -1 behind them; tokens <- picks[b, accepted], positions / placement / valid_lens +=
    accepted + 1, draws += accepted + 1 (only where the generator gave the uniforms): one draw per emitted token, so the emitted
    sequence is what sample_advance emits step by step.  out_logprobs <- the picks' tempered log-probabilities, NaN behind the
    bonus token; logprobs (B) <- that of picks[b, accepted] (needs out_logprobs); u_out <- the uniform of every row.  Returns
    (accepted (B) int32, out_tokens (B, len_q) int32); accepted / out_tokens: buffers to write into (a captured call).
    The options below travel as one zl_sample_opts_t to zl_spec_sample_accept_ex.
    seen (B, >= ceil(n / 32)) int32 with rep_penalty / presence (B) fp32, per task: the penalty group -- row (b, i) is
    sample_advance(seen=)'s pick under the set seen[b] + the in-range drafts[b, :i] (the row counts only if they were emitted), and
    the bits of the emitted tokens out_tokens[b, :accepted + 1] are set in seen[b]; the rejected drafts' are not.
    bias (logit_bias_pack's tuple, per task) / top_n with top_ids (B, K + 1, N) int32 and top_logprobs (B, K + 1, N) fp32:
    the bias and top-N groups -- every row (b, i) is sample_advance(bias=, top_n=)'s under task b's bias (the drafts in front of a row
    change its penalty set only), the rows behind the bonus token hold -1 / NaN.
    fsm (grammar_tables' tensors) with fsm_state (B) int32 and row_states (B, K + 1) int32: the automaton group -- row (b, i) is
    sample_advance(fsm=)'s under the state s_i, s_0 = fsm_state[b], s_{j+1} = delta(s_j, drafts[b, j]); row_states[b, i] <- delta(s_i,
    picks[b, i]) and fsm_state[b] <- row_states[b, accepted[b]]: the state has moved over exactly the emitted tokens."""
    what = "spec_sample_accept"
    if (fsm is None) != (fsm_state is None) or (fsm is None) != (row_states is None):
        raise ZLError(f"{what}: fsm, fsm_state and row_states are given together")
    _sample_logits(what, "(B * len_q, n)", logits, drafts=drafts, temperature=temperature, top_k=top_k, top_p=top_p)
    if drafts.dim() != 2 or drafts.shape[1] < 1 or drafts.dtype != torch.int32 or not drafts.is_contiguous():
        raise ZLError(f"{what}: drafts are (B, K) contiguous int32, K >= 1")
    b, len_q, n = drafts.shape[0], drafts.shape[1] + 1, logits.shape[1]
    if len_q > 32:
        raise ZLError(f"{what}: at most 32 rows per task (K <= 31)")
    if b < 1 or logits.shape[0] != b * len_q:
        raise ZLError(f"{what}: one logit row per task and draft position: B * (K + 1) rows")
    if logprobs is not None and out_logprobs is None:
        raise ZLError(f"{what}: logprobs is read from out_logprobs: give both")
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    per_task = lambda t, dtype, name: (t, dtype, b, name, "of length B")                           # noqa: E731
    per_row = lambda t, dtype, name: (t, dtype, b * len_q, name, "(B, K + 1)")                     # noqa: E731
    _sample_tensors(what, logits, False, [(drafts, i32, b * (len_q - 1), "drafts", "(B, K)"), per_task(temperature, f32, "temperature"),
                                          per_task(top_k, i32, "top_k"), per_task(top_p, f32, "top_p")],
                    [per_task(seeds, i64, "seeds"), per_task(draws, i64, "draws"), per_row(u, f32, "u")],
                    [per_task(tokens, i32, "tokens"), per_task(positions, i32, "positions"), per_task(placement, i32, "placement"),
                     per_task(valid_lens, i32, "valid_lens"), per_task(accepted, i32, "accepted"), per_task(logprobs, f32, "logprobs"),
                     per_row(out_tokens, i32, "out_tokens"), per_row(out_logprobs, f32, "out_logprobs"), per_row(u_out, f32, "u_out")])
    opts = _sample_opts(what, b, (b, len_q), n, logits.device, rep_penalty, presence, seen, bias, top_n, top_ids, top_logprobs, fsm, fsm_state,
                        row_states)
    if accepted is None:
        accepted = torch.empty(b, dtype=torch.int32, device=logits.device)
    if out_tokens is None:
        out_tokens = torch.empty((b, len_q), dtype=torch.int32, device=logits.device)
    check(lib().zl_spec_sample_accept_ex(_p(logits), C.c_int(2 if logits.dtype == torch.float16 else 6), _i(b), _i(len_q), _i(n),
                                         _i(logits.stride(0)), _p(drafts), _p(temperature), _p(top_k), _p(top_p), _p(seeds), _p(draws), _p(u),
                                         _p(tokens), _p(positions), _p(placement), _p(valid_lens), _p(accepted), _p(out_tokens),
                                         _p(out_logprobs), _p(logprobs), _p(u_out), opts, _stream()), what)
    return accepted, out_tokens.view(b, len_q)


# --------------------------------------------------------------------------------------------------
# scoring:functions::Gemm + nn::log_prob_raw / greedy_match_raw (src/nn/functions/cross_entropy.cu:7-69, 358-403) without the
# (M, N) logits: csrc/lm_head_score.hip
# --------------------------------------------------------------------------------------------------
ScoreRows = collections.namedtuple("ScoreRows", "lse label_logit logprob greedy greedy_logit")
SCORE_IGNORE = -100


def lm_head_score_workspace(m, n, device):
    nbytes = int(lib().zl_lm_head_score_ws_bytes(_i(m), _i(n)))
    if nbytes < 0:
        check(nbytes, "lm_head_score_ws_bytes")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def score_labels(prompts, labels=None, ignore_index=SCORE_IGNORE):
    """Host label list of a scoring call over the concatenated rows of `prompts` (1-D int sequences): labels None = next-token
    labels (row r of prompt j is labelled prompts[j][r + 1], its last row ignore_index); else labels[j] gives prompt j's labels,
    one per row (ignore_index = not scored), as calc_log_prob's `label` (src/model/llama.cpp:220-232).  Pure host code: the
    sequences are read with .tolist(), so give host tensors / lists (a device tensor costs a synchronising copy here)."""
    rows = []
    if labels is None:
        for pr in prompts:
            ids = [int(t) for t in (pr.tolist() if hasattr(pr, "tolist") else pr)]
            rows += ids[1:] + [ignore_index]
        return rows
    if len(labels) != len(prompts):
        raise ZLError("score: one label sequence per prompt")
    for pr, lb in zip(prompts, labels):
        ids = [int(t) for t in (lb.tolist() if hasattr(lb, "tolist") else lb)]
        if len(ids) != (int(pr.numel()) if hasattr(pr, "numel") else len(pr)):
            raise ZLError("score: a label sequence must have its prompt's length")
        rows += ids
    return rows


def _score_args(x, weight, labels, ignore_index, what):
    """host checks shared by lm_head_score / lm_head_score_unfused -> (x2, m, n, k, labels on the device or None)"""
    _chk_cuda(weight)
    if not (x.is_cuda and x.dim() >= 1 and x.stride(-1) == 1) or x.device != weight.device:
        raise ZLError(what + ": CUDA activations with unit column stride on the weight's device")
    x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    if weight.dim() != 2 or weight.shape[1] != k or weight.dtype != x.dtype or m < 1:
        raise ZLError(what + ": size K / dtype mismatch")
    _dt(x)
    n = weight.shape[0]
    if labels is not None:
        if not (torch.is_tensor(labels) and labels.is_cuda):        # host labels: checked here, one upload
            host = torch.as_tensor(labels)
            if host.dim() != 1 or host.numel() != m or host.dtype.is_floating_point:
                raise ZLError(what + ": labels: one integer per row")
            if bool(((host != ignore_index) & ((host < 0) | (host >= n))).any()):
                raise ZLError(what + ": a label lies outside the vocabulary")
            labels = host.to(torch.int32).to(x.device)
        elif labels.dtype != torch.int32 or labels.dim() != 1 or labels.numel() != m or not labels.is_contiguous() or labels.device != x.device:
            raise ZLError(what + ": device labels: contiguous int32 of length M on the activations' device")    # (their values are trusted)
    return x2, m, n, k, labels


def lm_head_score(x, weight, labels=None, ignore_index=SCORE_IGNORE, workspace=None, order=None):
    """Per row of y = x . weight^T (the values gemm_nt would store), without storing y: ScoreRows(lse, label_logit, logprob, greedy,
    greedy_logit) -- fp32 log-sum-exp, the label's logit, label_logit - lse, the arg-max column (int32, lowest on ties) and its
    value; rows whose label is ignore_index (or all rows with labels=None) get label_logit = logprob = 0.  labels: int32 device
    tensor of length M (values trusted), or a host tensor / list (checked against [0, N) here, uploaded once).  workspace:
    lm_head_score_workspace(M, N, device) to reuse one (graph capture); K % 128 == 0 (ZLError otherwise: lm_head_score_unfused
    covers other shapes).  order: the tile launch order of zl_lm_head_score_ex (0 / 1; results do not depend on it), default
    ZL_SCORE_ORDER from the environment, else the library's choice by row count (-1).  Logits are assumed finite."""
    x2, m, n, k, labels = _score_args(x, weight, labels, ignore_index, "lm_head_score")
    if workspace is None:
        workspace = lm_head_score_workspace(m, n, x.device)
    else:
        need = int(lib().zl_lm_head_score_ws_bytes(_i(m), _i(n)))
        if not (workspace.is_cuda and workspace.is_contiguous() and workspace.device == x.device) or workspace.numel() * workspace.element_size() < need:
            raise ZLError("lm_head_score: workspace too small / wrong device")
    f = torch.empty((4, m), dtype=torch.float32, device=x.device)
    greedy = torch.empty(m, dtype=torch.int32, device=x.device)
    if order is None:
        order = int(os.environ.get("ZL_SCORE_ORDER", "-1"))
    check(lib().zl_lm_head_score_ex(_p(x2), _i(x2.stride(0)), _p(weight), _p(labels), C.c_int(ignore_index), C.c_int(0), _p(f[0]),
                                    _p(f[1]), _p(f[2]), _p(greedy), _p(f[3]), _p(workspace), _i(m), _i(n), _i(k), C.c_int(_dt(x)),
                                    C.c_int(order), _stream()), "lm_head_score")
    return ScoreRows(f[0], f[1], f[2], greedy, f[3])


def lm_head_score_unfused(x, weight, labels=None, ignore_index=SCORE_IGNORE, rows_per_block=256):
    """lm_head_score's five results from the existing ops over blocks of rows_per_block rows, so that at most that slab of logits
    (and its fp32 copy) exists at once: gemm_nt (gemm_nt_small_m for K % 128 != 0), then fp32 torch logsumexp / gather / max on
    the rounded logits.  The form for shapes the fused kernel refuses and the baseline tools/bench_score.py times."""
    x2, m, n, k, labels = _score_args(x, weight, labels, ignore_index, "lm_head_score_unfused")
    f = torch.zeros((4, m), dtype=torch.float32, device=x.device)
    greedy = torch.empty(m, dtype=torch.int32, device=x.device)
    step = max(1, int(rows_per_block))
    for a in range(0, m, step):
        xb = x2[a:a + step]
        if k % 128 == 0:
            y = gemm_nt(xb if xb.is_contiguous() else xb.contiguous(), weight).float()
        else:
            y = gemm_nt_small_m(xb.contiguous(), weight).float()
        b = a + y.shape[0]
        f[0, a:b] = torch.logsumexp(y, dim=1)
        gi = torch.argmax(y, dim=1)
        f[3, a:b] = y.gather(1, gi.view(-1, 1)).view(-1)
        greedy[a:b] = gi
        if labels is not None:
            lb = labels[a:b].long()
            keep = lb != ignore_index
            ll = y.gather(1, lb.clamp(0, n - 1).view(-1, 1)).view(-1)
            f[1, a:b] = torch.where(keep, ll, torch.zeros_like(ll))
            f[2, a:b] = torch.where(keep, ll - f[0, a:b], torch.zeros_like(ll))
    return ScoreRows(f[0], f[1], f[2], greedy, f[3])


# --------------------------------------------------------------------------------------------------
# the batch generator's logit post-processing (src/generator/beam_util.cu, bmengine functions/{softmax,topk}.cu): csrc/sampling_ops.hip
# --------------------------------------------------------------------------------------------------
_ELEM = {torch.float16: 2, torch.bfloat16: 6, torch.float32: 1}


def _rows2d(logits, what):
    if not (logits.is_cuda and logits.dim() == 2 and logits.is_contiguous() and logits.dtype in _ELEM):
        raise ZLError(what + ": contiguous (rows, n) CUDA logits of fp16 / bf16 / fp32")
    return logits.shape


def log_softmax_bias(logits, bias=None, temperature=0.0, out=None):
    """beam_utility::log_softmax_bias: T((x - max) / temperature - log(sum) + bias[row]); temperature 0 = the form without the division"""
    rows, n = _rows2d(logits, "log_softmax_bias")
    out = torch.empty_like(logits) if out is None else out
    check(lib().zl_log_softmax_bias(_p(logits), _p(bias), _p(out), _i(rows), _i(n), _f(temperature), C.c_int(_ELEM[logits.dtype]), _stream()), "log_softmax_bias")
    return out


def softmax_rows(logits, temperature=1.0, out=None):
    """functions::softmax: T(exp(x / t - max / t) / sum)"""
    rows, n = _rows2d(logits, "softmax_rows")
    out = torch.empty_like(logits) if out is None else out
    check(lib().zl_softmax_rows(_p(logits), _p(out), _i(rows), _i(n), _f(temperature), C.c_int(_ELEM[logits.dtype]), _stream()), "softmax_rows")
    return out


def topk_rows(x, top):
    """functions::TopK::forward: (values (rows, top) descending in x's dtype, positions int32); ties go to the lower index"""
    rows, n = _rows2d(x, "topk_rows")
    v = torch.empty((rows, top), dtype=x.dtype, device=x.device)
    i = torch.empty((rows, top), dtype=torch.int32, device=x.device)
    check(lib().zl_topk_rows(_p(x), _p(v), _p(i), _i(rows), _i(n), C.c_int(top), C.c_int(_ELEM[x.dtype]), _stream()), "topk_rows")
    return v, i


def gather_logits(index, logits):
    """beam_utility::gather_logits: float32 values of the flattened logits at int32 positions"""
    _chk_cuda(index, logits)
    out = torch.empty(index.shape, dtype=torch.float32, device=logits.device)
    check(lib().zl_gather_logits(_p(index), _p(logits), _p(out), _i(index.numel()), C.c_int(_ELEM[logits.dtype]), _stream()), "gather_logits")
    return out


def scatter_logits(values, token_ids, batch_ids, logits, add=False):
    """beam_utility::scatter_update, in place: logits[batch_ids[i], token_ids[i]] = T(values[i]) (add: += in T)"""
    rows, n = _rows2d(logits, "scatter_logits")
    _chk_cuda(values, token_ids, batch_ids)
    check(lib().zl_scatter_logits(_p(values), _p(token_ids), _p(batch_ids), _p(logits), _i(token_ids.numel()), _i(n), C.c_int(int(add)),
                                  C.c_int(_ELEM[logits.dtype]), _stream()), "scatter_logits")
    return logits


def repetition_penalty(factor, tokens, batch_ids, logits, presence=None):
    """beam_utility::beam_repetition_penalty, in place: l = presence != 0 ? l - T(presence) : (l < 0 ? l * T(factor) : l / T(factor))"""
    rows, n = _rows2d(logits, "repetition_penalty")
    _chk_cuda(factor, tokens, batch_ids, presence)
    check(lib().zl_repetition_penalty(_p(factor), _p(presence), _p(tokens), _p(batch_ids), _p(logits), _i(tokens.numel()), _i(n),
                                      C.c_int(_ELEM[logits.dtype]), _stream()), "repetition_penalty")
    return logits


# --------------------------------------------------------------------------------------------------
# a17 / a13 / a14 / a18 / a22
# --------------------------------------------------------------------------------------------------
def rmsnorm(x, weight, eps, scale=1.0, x2=None, out=None, out_sum=None):
    """LayerNorm::forward (rms) / fuse_add (src/nn/layernorm/layernorm.cu:227-302)."""
    _chk_cuda(x, weight, x2)
    xr = x.reshape(-1, x.shape[-1])
    rows, dim = xr.shape
    if out is None:
        out = torch.empty_like(xr)
    if x2 is not None and out_sum is None:
        out_sum = torch.empty_like(xr)
    check(lib().zl_rmsnorm(_p(xr), _p(weight), _p(out), _i(rows), _i(dim), _f(eps), _f(scale), _p(x2), _p(out_sum),
                           C.c_int(_dt(x)), _stream()), "rmsnorm")
    return (out, out_sum) if x2 is not None else out


def rope_cos_sin(pos, dim_head, base, neox=True, llama3=None):
    """RopePreparer::compute_cos_sin (src/nn/position/rope_preparer.cu); llama3 = (factor, low, high, old_len)."""
    _chk_cuda(pos)
    s = pos.numel()
    cs = torch.empty((s, dim_head), dtype=torch.float32, device=pos.device)
    sn = torch.empty_like(cs)
    if llama3 is None:
        check(lib().zl_rope_cos_sin(_p(pos), _p(cs), _p(sn), _i(s), _i(dim_head), _f(base), C.c_int(int(neox)),
                                    _stream()), "rope_cos_sin")
    else:
        fac, low, high, old = llama3
        check(lib().zl_rope_cos_sin_llama3(_p(pos), _p(cs), _p(sn), _i(s), _i(dim_head), _f(base), _f(fac), _f(low),
                                           _f(high), _f(old), C.c_int(int(neox)), _stream()), "rope_cos_sin_llama3")
    return cs, sn


def rope_cos_sin_dynamic(pos, dim_head, base, factor, max_position_embeddings, seq_len=None, neox=True):
    """RotaryEmbedding "dynamic" (NTK) angles (src/nn/position/rotary_embedding.cu:19-61); seq_len (s,) int32 = the position
    the reference reads as the row's sequence length (None: the row's own position)."""
    _chk_cuda(pos)
    s = pos.numel()
    cs = torch.empty((s, dim_head), dtype=torch.float32, device=pos.device)
    sn = torch.empty_like(cs)
    if seq_len is not None:
        _chk_cuda(seq_len)
        if seq_len.numel() != s or seq_len.dtype != torch.int32:
            raise ZLError("rope_cos_sin_dynamic: seq_len must be int32 (s,)")
    check(lib().zl_rope_cos_sin_dynamic(_p(pos), _p(seq_len) if seq_len is not None else None, _p(cs), _p(sn), _i(s),
                                        _i(dim_head), _f(base), _f(factor), _f(max_position_embeddings), C.c_int(int(neox)),
                                        _stream()), "rope_cos_sin_dynamic")
    return cs, sn


def yarn_params(base, dim_head, original_max_position, factor, beta_fast=32, beta_slow=1, attn_factor=1.0, deepseek=False,
                mscale=0.0, mscale_all_dim=0.0):
    """YarnImpl's constructor (rotary_embedding.cu:506-553): (low, high, mscale) in double, narrowed to float."""
    def corr(rot):
        return (dim_head * math.log(original_max_position / (rot * 2 * 3.141592653589793))) / (2 * math.log(base))

    def get_mscale(scale, m=1.0):
        return 1.0 if scale <= 1.0 else 0.1 * m * math.log(scale) + 1.0
    f32 = lambda v: C.c_float(v).value  # noqa: E731  (the reference keeps factor / mscale / attn_factor as float members)
    factor, mscale, mscale_all_dim = f32(factor), f32(mscale), f32(mscale_all_dim)
    low = max(float(math.floor(corr(beta_fast))), 0.0)
    high = min(float(math.ceil(corr(beta_slow))), dim_head - 1.0)
    af = f32(attn_factor)
    m = get_mscale(factor) * af
    if deepseek:
        m = get_mscale(factor, mscale) / get_mscale(factor, mscale_all_dim) * af
    return f32(low), f32(high), f32(m)


def rope_cos_sin_yarn(pos, dim_head, base, factor, low, high, mscale, neox=True):
    """YaRN angles (KERNEL_yarn_rope_neox_style, rotary_embedding.cu:398-447): cos / sin already multiplied by mscale."""
    _chk_cuda(pos)
    s = pos.numel()
    cs = torch.empty((s, dim_head), dtype=torch.float32, device=pos.device)
    sn = torch.empty_like(cs)
    check(lib().zl_rope_cos_sin_yarn(_p(pos), _p(cs), _p(sn), _i(s), _i(dim_head), _f(base), _f(factor), _f(low), _f(high),
                                     _f(mscale), C.c_int(int(neox)), _stream()), "rope_cos_sin_yarn")
    return cs, sn


def head_norm(x, weight, num_heads, dim_head, eps, mode=0, out=None):
    """q_norm / k_norm over dim_head: mode 0 = Qwen3's RMSNorm with one (dim_head) weight (attention.cpp:110-113,871-876),
    mode 1 = KERNEL_layernorm_multi_head with a (heads, dim_head) weight (layernorm.cu:329-353).  x (rows, >= heads*dim_head)
    may be a column slice of a wider row (a q or k window of the fused qkv projection); in place with out=x."""
    _chk_cuda(weight)
    if not x.is_cuda or (out is not None and not out.is_cuda):
        raise ZLError("tensors must be CUDA tensors")
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] != num_heads * dim_head:
        raise ZLError("head_norm: x must be (rows, heads * dim_head) with unit column stride")
    if weight.numel() != (dim_head if mode == 0 else num_heads * dim_head) or weight.dtype != x.dtype:
        raise ZLError("head_norm: weight shape / dtype mismatch")
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
    elif out.shape != x.shape or out.stride(1) != 1 or out.dtype != x.dtype:
        raise ZLError("head_norm: out shape mismatch")
    check(lib().zl_head_norm(_p(x), _p(weight), _p(out), _i(x.shape[0]), _i(num_heads), _i(dim_head), _i(x.stride(0)),
                             _i(out.stride(0)), _f(eps), C.c_int(mode), _dt(x), _stream()), "head_norm")
    return out


def rotary_embedding_qk(pos, x, num_heads, num_kv_heads, dim_head, rope_theta):
    """nn::rotary_embedding_qk (src/nn/position/rotary_embedding_fuse.cu:70-123)."""
    _chk_cuda(pos, x)
    s = pos.numel()
    q = torch.empty((s, num_heads * dim_head), dtype=x.dtype, device=x.device)
    k = torch.empty((s, num_kv_heads * dim_head), dtype=x.dtype, device=x.device)
    v = torch.empty_like(k)
    check(lib().zl_rotary_embedding_qk(_p(pos), _p(x), _p(q), _p(k), _p(v), _i(s), _i(num_heads), _i(num_kv_heads),
                                       _i(dim_head), _f(rope_theta), C.c_int(_dt(x)), _stream()), "rotary_embedding_qk")
    return q, k, v


def rope_qk_cache(cos, sin, x, num_heads, num_kv_heads, dim_head, neox=True):
    """nn::rope_qk_cache (src/nn/position/rotary_embedding_fuse_cache.cu:65-125)."""
    _chk_cuda(cos, sin, x)
    s = cos.shape[0]
    q = torch.empty((s, num_heads * dim_head), dtype=x.dtype, device=x.device)
    k = torch.empty((s, num_kv_heads * dim_head), dtype=x.dtype, device=x.device)
    v = torch.empty_like(k)
    check(lib().zl_rope_qk_cache(_p(cos), _p(sin), _p(x), _p(q), _p(k), _p(v), _i(s), _i(num_heads), _i(num_kv_heads),
                                 _i(dim_head), C.c_int(int(neox)), C.c_int(_dt(x)), _stream()), "rope_qk_cache")
    return q, k, v


def make_ptr_table(tensors, device=None):
    """Device array of raw pointers, one per task -- RagBufferContext::buf_k_addr
    (src/model/rag_buffer_context.h:141-188)."""
    device = device or tensors[0].device
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=device)


def copy_to_rag_buffer2(placement, buf_lens, k_src, v_src, k_addrs, v_addrs, bshd=True):
    """nn::copy_to_rag_buffer2 (src/kvcache/ragged_buffer_kernel.cu:254-300)."""
    _chk_cuda(placement, buf_lens, k_src, v_src, k_addrs, v_addrs)
    b, len_q, hkv, d = k_src.shape
    if placement.dim() != 2:
        raise ZLError("placement is not 2d")
    check(lib().zl_copy_to_rag_buffer2(_p(placement), _p(buf_lens), _p(k_src), _p(v_src), _p(k_addrs), _p(v_addrs),
                                       _i(b), _i(len_q), _i(hkv), _i(d), C.c_int(int(bshd)), _stream()),
          "copy_to_rag_buffer2")


def kv_blocks_copy(desc, k_addrs, v_addrs, buf_lens, pool, block, hkv, row_bytes, to_pool, bshd=True, buf_lens_host=None,
                   piece_bytes=0):
    """zl_kv_blocks_copy: ONE launch that copies, for every descriptor (task, first slot, pool block) of `desc`, every layer and both
    K and V, `block` rows of the task's buffers into the pool block (to_pool) or back.  desc: a HOST sequence of int triples (it is
    checked here and uploaded); k_addrs / v_addrs (layers, B) device pointer tables (DynBatchContext.k_addrs / v_addrs, or ks_addrs /
    vs_addrs for the INT8 cache's scales); buf_lens (B) int32 on the device, buf_lens_host the same numbers where the caller holds
    them (else they are read back: a synchronisation); pool: a contiguous tensor of num_blocks = pool.shape[0] blocks of
    layers * 2 * block * hkv * row_bytes bytes each, laid out (layers, 2, block, hkv, row) under BSHD and (layers, 2, hkv, block, row)
    under BHSD; row_bytes % 4 == 0.  Raises ZLError before any launch for a descriptor whose rows do not fit its task's buffer, a pool
    block id out of range, or a destination that occurs twice in the call: a pool block when saving, overlapping rows of one task
    when loading (one pool block may be LOADED into several tasks by one call: two prompts that share a prefix).  An empty desc
    launches nothing."""
    _chk_cuda(k_addrs, v_addrs, buf_lens, pool)
    if k_addrs.dim() != 2 or k_addrs.shape != v_addrs.shape or k_addrs.dtype != torch.int64 or v_addrs.dtype != torch.int64:
        raise ZLError("kv_blocks_copy: k_addrs / v_addrs are (layers, B) int64 pointer tables")
    layers, b = k_addrs.shape
    block, hkv, row_bytes = int(block), int(hkv), int(row_bytes)
    if buf_lens.dtype != torch.int32 or buf_lens.numel() != b:
        raise ZLError("kv_blocks_copy: buf_lens is (B) int32")
    if block < 1 or hkv < 1 or row_bytes < 4 or row_bytes % 4:
        raise ZLError("kv_blocks_copy: block, hkv >= 1 and row_bytes a positive multiple of 4")
    block_bytes = layers * 2 * block * hkv * row_bytes
    num_blocks = pool.shape[0] if pool.dim() else 0
    if num_blocks < 1 or pool.numel() * pool.element_size() != num_blocks * block_bytes:
        raise ZLError(f"kv_blocks_copy: the pool does not hold {num_blocks} blocks of {block_bytes} bytes")
    desc = [tuple(int(x) for x in d) for d in (desc.tolist() if hasattr(desc, "tolist") else desc)]
    if not desc:
        check(lib().zl_kv_blocks_copy(None, _i(0), _p(k_addrs), _p(v_addrs), _p(buf_lens), _p(pool), _i(layers), _i(b), _i(block),
                                      _i(hkv), _i(row_bytes), C.c_int(int(bshd)), C.c_int(int(to_pool)), _stream()), "kv_blocks_copy")
        return None
    lens = buf_lens.tolist() if buf_lens_host is None else [int(x) for x in buf_lens_host]
    if len(lens) != b:
        raise ZLError("kv_blocks_copy: one buffer length per task")
    seen, rows = set(), {}
    for d in desc:
        if len(d) != 3:
            raise ZLError("kv_blocks_copy: a descriptor is (task, first slot, pool block)")
        task, slot, pb = d
        if not 0 <= task < b or slot < 0 or slot + block > lens[task]:
            raise ZLError(f"kv_blocks_copy: rows {slot} .. {slot + block - 1} of task {task} lie outside its buffer")
        if not 0 <= pb < num_blocks:
            raise ZLError(f"kv_blocks_copy: pool block {pb} outside the pool's {num_blocks}")
        if to_pool:
            if pb in seen:
                raise ZLError(f"kv_blocks_copy: pool block {pb} is written twice in one call")
            seen.add(pb)
        else:
            if any(abs(slot - other) < block for other in rows.get(task, ())):
                raise ZLError(f"kv_blocks_copy: rows {slot} .. {slot + block - 1} of task {task} are written twice in one call")
            rows.setdefault(task, []).append(slot)
    desc_dev = torch.tensor(desc, dtype=torch.int32).to(pool.device)
    fn, extra = (lib().zl_kv_blocks_copy_ex, (_i(piece_bytes),)) if piece_bytes else (lib().zl_kv_blocks_copy, ())
    check(fn(_p(desc_dev), _i(len(desc)), _p(k_addrs), _p(v_addrs), _p(buf_lens), _p(pool), _i(layers), _i(b), _i(block), _i(hkv),
             _i(row_bytes), C.c_int(int(bshd)), C.c_int(int(to_pool)), *extra, _stream()), "kv_blocks_copy")
    return desc_dev


def kv_fork_check(desc, buf_lens_host, b, vocab=None):
    """The host half of kv_fork, numpy only: desc = (src, dst, rows, token) int quadruples, buf_lens_host = the b tasks' buffer
    lengths -> (the descriptors as a list of int 4-tuples, the largest rows).  Raises ZLError for a descriptor that is not four
    ints, a task outside the batch, rows outside either buffer, a task that is a destination twice (a self-descriptor src == dst
    counts for its task's token), a destination that is also a source, a source whose self-descriptor overrides its token (token >=
    0) while one of its other descriptors names another token -- that destination would read a tokens[src] the same launch writes --,
    and with `vocab` a token >= vocab.  token < 0 = no override."""
    b = int(b)
    lens = [int(x) for x in (buf_lens_host.tolist() if hasattr(buf_lens_host, "tolist") else buf_lens_host)]
    if len(lens) != b:
        raise ZLError("kv_fork: one buffer length per task")
    rows_in = desc.tolist() if hasattr(desc, "tolist") else list(desc)
    out = []
    for d in rows_in:
        try:
            d = tuple(d)
        except TypeError:
            d = ()
        if len(d) != 4 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in d):
            raise ZLError("kv_fork: a descriptor is (src, dst, rows, token), four integers")
        out.append(tuple(int(x) for x in d))
    dests, selfs, sources = set(), {}, set()
    for src, dst, rows, token in out:
        if not (0 <= src < b and 0 <= dst < b):
            raise ZLError(f"kv_fork: tasks {src} -> {dst} lie outside the batch of {b}")
        if not 0 <= rows <= min(lens[src], lens[dst]):
            raise ZLError(f"kv_fork: rows 0 .. {rows - 1} of tasks {src} -> {dst} lie outside a buffer ({lens[src]}, {lens[dst]} rows)")
        if not -(1 << 31) <= token < (1 << 31) or (vocab is not None and token >= int(vocab)):
            raise ZLError(f"kv_fork: token {token} of tasks {src} -> {dst} lies outside the vocabulary")
        if dst in dests or dst in selfs:
            raise ZLError(f"kv_fork: task {dst} is a destination twice in one call")
        if src == dst:
            selfs[src] = token
        else:
            dests.add(dst)
        sources.add(src)
    for src, dst, rows, token in out:
        if src != dst and dst in sources:
            raise ZLError(f"kv_fork: task {dst} is a destination and a source in one call")
        if src != dst and selfs.get(src, -1) >= 0 and token != selfs[src]:
            raise ZLError(f"kv_fork: task {src} overrides its token with {selfs[src]}, its descriptor to task {dst} names {token}")
    return out, max((d[2] for d in out), default=0)


def kv_fork(desc, k_addrs, v_addrs, buf_lens, hkv, row_bytes, bshd=True, buf_lens_host=None, ctx_rows=None, piece_bytes=0, vocab=None):
    """zl_kv_fork: ONE launch that, for every descriptor (src, dst, rows, token) of `desc`, every layer and both K and V, copies rows
    [0, rows) of task src's buffers into task dst's and, with ctx_rows = (tokens, positions, placement, valid_lens) (B) int32, hands
    dst the source's position, placement and valid length and the pending token `token` (token < 0: the source's); a self-descriptor
    (src == dst) copies nothing and only sets the task's own pending token.  desc: a HOST sequence, checked here (kv_fork_check states
    the refusals, all raised before any launch) and uploaded once; k_addrs / v_addrs (layers, B) device pointer tables
    (DynBatchContext.k_addrs / v_addrs, or ks_addrs / vs_addrs with row_bytes = 4 and ctx_rows = None for the INT8 cache's scales);
    buf_lens (B) int32 on the device, buf_lens_host the same numbers where the caller holds them (else they are read back: a
    synchronisation); row_bytes % 4 == 0.  An empty desc launches nothing.  Returns the uploaded descriptors, or None."""
    _chk_cuda(k_addrs, v_addrs, buf_lens)
    if k_addrs.dim() != 2 or k_addrs.shape != v_addrs.shape or k_addrs.dtype != torch.int64 or v_addrs.dtype != torch.int64:
        raise ZLError("kv_fork: k_addrs / v_addrs are (layers, B) int64 pointer tables")
    layers, b = k_addrs.shape
    hkv, row_bytes, piece_bytes = int(hkv), int(row_bytes), int(piece_bytes)
    if buf_lens.dtype != torch.int32 or buf_lens.numel() != b:
        raise ZLError("kv_fork: buf_lens is (B) int32")
    if hkv < 1 or row_bytes < 4 or row_bytes % 4 or piece_bytes < 0 or piece_bytes % 16:
        raise ZLError("kv_fork: hkv >= 1, row_bytes a positive multiple of 4, piece_bytes a multiple of 16")
    if ctx_rows is not None:
        if len(ctx_rows) != 4:
            raise ZLError("kv_fork: ctx_rows is (tokens, positions, placement, valid_lens)")
        for t in ctx_rows:
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.numel() == b and t.is_contiguous()
                    and t.device == k_addrs.device):
                raise ZLError("kv_fork: ctx_rows: four contiguous (B) int32 tensors on the tables' device")
    rows4 = [_p(t) for t in ctx_rows] if ctx_rows is not None else [_p(None)] * 4
    n_desc = len(desc)
    if not n_desc:
        check(lib().zl_kv_fork(None, _i(0), _p(k_addrs), _p(v_addrs), _p(buf_lens), _i(layers), _i(b), _i(0), _i(hkv), _i(row_bytes),
                               C.c_int(int(bshd)), *rows4, _stream()), "kv_fork")
        return None
    desc, max_rows = kv_fork_check(desc, buf_lens.tolist() if buf_lens_host is None else buf_lens_host, b, vocab)
    desc_dev = torch.tensor(desc, dtype=torch.int32).to(k_addrs.device)
    fn, extra = (lib().zl_kv_fork_ex, (_i(piece_bytes),)) if piece_bytes else (lib().zl_kv_fork, ())
    check(fn(_p(desc_dev), _i(len(desc)), _p(k_addrs), _p(v_addrs), _p(buf_lens), _i(layers), _i(b), _i(max_rows), _i(hkv), _i(row_bytes),
             C.c_int(int(bshd)), *rows4, *extra, _stream()), "kv_fork")
    return desc_dev


def rope_scatter_decode(cos, sin, qkv, placement, buf_lens, k_addrs, v_addrs, num_heads, num_kv_heads, dim_head,
                        neox=True, bshd=True, q_out=None):
    """rope_qk_cache + copy_to_rag_buffer2 fused for len_q == 1 decode rows."""
    _chk_cuda(cos, sin, qkv, placement, buf_lens, k_addrs, v_addrs)
    b = qkv.shape[0]
    if q_out is None:
        q_out = torch.empty((b, num_heads * dim_head), dtype=qkv.dtype, device=qkv.device)
    check(lib().zl_rope_scatter_decode(_p(cos), _p(sin), _p(qkv), _p(q_out), _p(placement), _p(buf_lens), _p(k_addrs),
                                       _p(v_addrs), _i(b), _i(num_heads), _i(num_kv_heads), _i(dim_head),
                                       C.c_int(int(neox)), C.c_int(int(bshd)), C.c_int(_dt(qkv)), _stream()),
          "rope_scatter_decode")
    return q_out


def w4_qkv_rope_scatter_ok(m, k, dim_head, norm):
    """what zl_w4a16_qkv_rope_scatter covers (otherwise: w4_linear + rope_scatter_decode)"""
    return m <= 32 and dim_head % 32 == 0 and (not norm or k <= 4096 or m > 8) and (m <= 16 or k <= 8192)


def w4_qkv_rope_scatter(x, w, cos, sin, placement, buf_lens, k_addrs, v_addrs, num_heads, num_kv_heads, dim_head, bias=None,
                        norm_weight=None, norm_eps=1e-5, bshd=True, q_out=None, row_ss=None):
    """fused qkv projection (W4MWeight w, (H + 2 Hkv) D rows) + neox rotary + KV scatter for decode rows; returns the
    rotated q (M, H*D).  Bit-identical to w4_linear(..) followed by rope_scatter_decode(..)."""
    _chk_cuda(x, cos, sin, placement, buf_lens, k_addrs, v_addrs, bias, norm_weight)
    if not isinstance(w, W4MWeight) or x.dtype != torch.float16:
        raise ZLError("w4_qkv_rope_scatter: fp16 activations and a ZLW4M weight")
    m, k = x.shape
    if q_out is None:
        q_out = torch.empty((m, num_heads * dim_head), dtype=x.dtype, device=x.device)
    opts = _w4_opts(x.device, m, w.n)
    if row_ss is not None:
        _chk_cuda(row_ss)
        opts.row_ss = row_ss.data_ptr()
    check(lib().zl_w4a16_qkv_rope_scatter_ex(_p(x), _i(x.stride(0)), _p(w.qw), _p(w.meta), _p(bias), _p(norm_weight),
                                             _f(norm_eps), _p(cos), _p(sin), _p(placement), _p(buf_lens), _p(k_addrs),
                                             _p(v_addrs), _p(q_out), _i(m), _i(num_heads), _i(num_kv_heads), _i(dim_head),
                                             _i(k), _i(w.group_size), C.c_int(int(bshd)), C.byref(opts), _stream()),
          "w4a16_qkv_rope_scatter")
    return q_out


def decode_attn_workspace(b, len_q, h, d, max_len_buf, device):
    nbytes = lib().zl_decode_attn_workspace_bytes(_i(b), _i(len_q), _i(h), _i(d), _i(max_len_buf))
    if nbytes < 0:
        check(int(nbytes), "decode_attn_workspace_bytes")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def multi_query_attention_rag_buffer(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, mask, scale, max_len_buf,
                                     num_kv_heads, valid_lens=None, bshd=True, out=None, workspace=None):
    """nn::multi_query_attention_rag_buffer / attention_qkv_rag_buffer
    (src/nn/attention/attention_kernel.cu:1252-1457, 1150-1213).  batch_q (B, len_q, H, D)."""
    _chk_cuda(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, mask, valid_lens)
    b, len_q, h, d = batch_q.shape
    if out is None:
        out = torch.empty_like(batch_q)
    if workspace is None:
        workspace = decode_attn_workspace(b, len_q, h, d, max_len_buf, batch_q.device)
    check(lib().zl_decode_attn_ex(_p(batch_q), _p(buf_lens), _p(key_buf_addrs), _p(val_buf_addrs), _p(mask),
                               _p(valid_lens), _p(out), _p(workspace), _i(b), _i(len_q), _i(h), _i(num_kv_heads),
                               _i(d), _f(scale), _i(max_len_buf), C.c_int(int(bshd)), C.c_int(_dt(batch_q)),
                               C.c_int(_attn_algo()), _stream()), "decode_attn")
    return out


def causal_step_mask(buf_lens, valid_lens, len_q):
    """The int8 mask of a speculative step in multi_query_attention_rag_buffer's layout, built on the host: task b contributes a
    (len_q, buf_lens[b]) block with mask[qi, j] = j < min(buf_lens[b], valid_lens[b] + qi), the blocks concatenated.  What
    decode_attention_causal computes without a mask; returns a 1-D int8 host tensor."""
    lens = [int(v) for v in (buf_lens.tolist() if hasattr(buf_lens, "tolist") else buf_lens)]
    valid = [int(v) for v in (valid_lens.tolist() if hasattr(valid_lens, "tolist") else valid_lens)]
    if len(lens) != len(valid) or int(len_q) < 1 or any(n < 0 for n in lens):
        raise ZLError("causal_step_mask: one buffer length and one valid length per task, len_q >= 1")
    parts = [(torch.arange(n)[None, :] < (torch.arange(int(len_q)) + v)[:, None]).to(torch.int8).reshape(-1) for n, v in zip(lens, valid)]
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int8)


def decode_attention_causal(batch_q, buf_lens, k_addrs, v_addrs, valid_lens, scale, max_len_buf, num_kv_heads, bshd=True, out=None,
                            workspace=None):
    """Decode attention of a speculative step (zl_decode_attn_causal): batch_q (B, len_q, H, 128), row qi of task b sees the keys
    j < min(buf_lens[b], valid_lens[b] + qi) -- multi_query_attention_rag_buffer with causal_step_mask(...), on the matrix cores and
    with one pass over a task's K / V for all of its rows.  workspace: decode_attn_workspace(B, len_q, H, 128, max_len_buf, device).
    Returns out, shaped like batch_q."""
    _chk_cuda(batch_q, buf_lens, k_addrs, v_addrs, valid_lens, out, workspace)
    if batch_q.dim() != 4:
        raise ZLError("decode_attention_causal: batch_q is (B, len_q, H, D)")
    b, len_q, h, d = batch_q.shape
    dt = _dt(batch_q)
    if d != 128 or num_kv_heads < 1 or h % num_kv_heads:
        raise ZLError("decode_attention_causal: head size 128, H a multiple of the kv heads")
    if not 1 <= len_q <= 32:
        raise ZLError("decode_attention_causal: 1 <= len_q <= 32")
    for t, dty, what in ((buf_lens, torch.int32, "buf_lens"), (valid_lens, torch.int32, "valid_lens"), (k_addrs, torch.int64, "k_addrs"),
                         (v_addrs, torch.int64, "v_addrs")):
        if t.dtype != dty or t.numel() != b or t.device != batch_q.device:
            raise ZLError(f"decode_attention_causal: {what}: {b} entries of {dty} on the queries' device")
    if out is None:
        out = torch.empty_like(batch_q)
    else:
        _chk_out(out, b * len_q, h * d, batch_q.dtype, batch_q.device, "decode_attention_causal")
    need = int(lib().zl_decode_attn_workspace_bytes(_i(b), _i(len_q), _i(h), _i(d), _i(max_len_buf)))
    if need < 0:
        check(need, "decode_attn_workspace_bytes")
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=batch_q.device)
    elif workspace.device != batch_q.device or workspace.numel() * workspace.element_size() < need:
        raise ZLError("decode_attention_causal: workspace too small / wrong device")
    check(lib().zl_decode_attn_causal(_p(batch_q), _p(buf_lens), _p(k_addrs), _p(v_addrs), _p(valid_lens), _p(out), _p(workspace),
                                      _i(b), _i(len_q), _i(h), _i(num_kv_heads), _i(d), _f(scale), _i(max_len_buf), C.c_int(int(bshd)),
                                      C.c_int(dt), _stream()), "decode_attn_causal")
    return out


def decode_attn_shared_workspace_bytes(b, g, h, num_kv_heads, d, max_prefix_len, max_len_buf):
    """bytes of split records decode_attention_shared needs (zl_decode_attn_shared_workspace_bytes)"""
    nbytes = int(lib().zl_decode_attn_shared_workspace_bytes(_i(b), _i(g), _i(h), _i(num_kv_heads), _i(d), _i(max_prefix_len), _i(max_len_buf)))
    if nbytes < 0:
        check(nbytes, "decode_attn_shared_workspace_bytes")
    return nbytes


def decode_attn_shared_workspace(b, g, h, num_kv_heads, d, max_prefix_len, max_len_buf, device):
    return torch.empty(decode_attn_shared_workspace_bytes(b, g, h, num_kv_heads, d, max_prefix_len, max_len_buf) // 4, dtype=torch.float32,
                       device=device)


def decode_attention_shared(batch_q, buf_lens, k_addrs, v_addrs, valid_lens, prefix_of, prefix_lens, prefix_caps, prefix_k_addrs,
                            prefix_v_addrs, scale, max_prefix_len, max_len_buf, num_kv_heads, bshd=True, out=None, workspace=None,
                            shared_split_len=0, own_split_len=0):
    """Two-segment decode attention (zl_decode_attn_shared): batch_q (B, 1, H, 128) or (B, H, 128); task b's first
    P = min(prefix_lens[g], prefix_caps[g], valid_lens[b], buf_lens[b]) keys are rows of prefix buffer g = prefix_of[b] (P = 0 for a g
    outside [0, G)), its keys [P, valid) rows of its own buffer.  prefix_k_addrs / prefix_v_addrs: pointer tables of the G prefix buffers
    (make_ptr_table), each prefix_caps[g] rows in the own buffers' layout; prefix_caps[g] <= max_prefix_len is the caller's to keep.
    workspace: decode_attn_shared_workspace(...).  Split lengths: multiples of 32 from 128 on, 0 = the launcher's.  Returns out, shaped
    like batch_q."""
    what = "decode_attention_shared"
    _chk_cuda(batch_q, buf_lens, k_addrs, v_addrs, valid_lens, prefix_of, prefix_lens, prefix_caps, prefix_k_addrs, prefix_v_addrs, out,
              workspace)
    if batch_q.dim() not in (3, 4) or (batch_q.dim() == 4 and batch_q.shape[1] != 1) or not batch_q.is_contiguous():
        raise ZLError(f"{what}: batch_q is a contiguous (B, 1, H, D) or (B, H, D): one query row per task")
    b, h, d = batch_q.shape[0], batch_q.shape[-2], batch_q.shape[-1]
    dt = _dt(batch_q)
    if batch_q.dtype not in (torch.float16, torch.bfloat16):
        raise ZLError(f"{what}: fp16 or bf16 queries")
    if d != 128 or num_kv_heads < 1 or h % num_kv_heads or h // num_kv_heads > 16:
        raise ZLError(f"{what}: head size 128, H a multiple of the kv heads, at most 16 query heads per kv head")
    g = int(prefix_lens.numel())
    if b < 1 or g < 1 or int(max_prefix_len) < 1 or int(max_len_buf) < 1:
        raise ZLError(f"{what}: at least one task, one prefix buffer and one row on either side")
    for t, dty, n, name in ((buf_lens, torch.int32, b, "buf_lens"), (valid_lens, torch.int32, b, "valid_lens"),
                            (prefix_of, torch.int32, b, "prefix_of"), (k_addrs, torch.int64, b, "k_addrs"), (v_addrs, torch.int64, b, "v_addrs"),
                            (prefix_lens, torch.int32, g, "prefix_lens"), (prefix_caps, torch.int32, g, "prefix_caps"),
                            (prefix_k_addrs, torch.int64, g, "prefix_k_addrs"), (prefix_v_addrs, torch.int64, g, "prefix_v_addrs")):
        if t.dtype != dty or t.numel() != n or t.device != batch_q.device or not t.is_contiguous():
            raise ZLError(f"{what}: {name}: {n} contiguous entries of {dty} on the queries' device")
    for sl in (shared_split_len, own_split_len):
        if sl and (sl < 128 or sl % 32):
            raise ZLError(f"{what}: a split length is a multiple of 32, at least 128 (0: the launcher's)")
    if out is None:
        out = torch.empty_like(batch_q)
    else:
        _chk_out(out, b, h * d, batch_q.dtype, batch_q.device, what)
    need = decode_attn_shared_workspace_bytes(b, g, h, num_kv_heads, d, max_prefix_len, max_len_buf)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=batch_q.device)
    elif workspace.device != batch_q.device or workspace.numel() * workspace.element_size() < need:
        raise ZLError(f"{what}: workspace too small / wrong device")
    check(lib().zl_decode_attn_shared_ex(_p(batch_q), _p(buf_lens), _p(k_addrs), _p(v_addrs), _p(valid_lens), _p(prefix_of), _p(prefix_lens),
                                         _p(prefix_caps), _p(prefix_k_addrs), _p(prefix_v_addrs), _p(out), _p(workspace), _i(b), _i(g), _i(h),
                                         _i(num_kv_heads), _i(d), _f(scale), _i(max_prefix_len), _i(max_len_buf), C.c_int(int(bshd)),
                                         C.c_int(dt), _i(shared_split_len), _i(own_split_len), _stream()), "decode_attn_shared")
    return out


def decode_attn_la_split_len(b, num_kv_heads, max_len_buf):
    """keys per split zl_decode_attn_la picks for this batch geometry (a multiple of 32)"""
    return int(lib().zl_decode_attn_la_split_len(_i(b), _i(num_kv_heads), _i(max_len_buf)))


def decode_attn_la_workspace(b, h, num_kv_heads, max_len_buf, device, split_len=0):
    """zero-initialised workspace of decode_attention_la (arrival words + split records); split_len = 0: large enough for any
    split length.  One per stream of launches that may overlap."""
    nbytes = lib().zl_decode_attn_la_workspace_bytes(_i(b), _i(h), _i(num_kv_heads), _i(max_len_buf), _i(split_len))
    if nbytes < 0:
        check(int(nbytes), "decode_attn_la_workspace_bytes")
    return torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=device)


def decode_attention_la(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, valid_lens, scale, max_len_buf, num_kv_heads, workspace,
                        out=None, bshd=True, split_len=0, half=False):
    """multi_query_attention_rag_buffer for decode rows (len_q = 1, prefix visibility) as ONE launch: the split merge is done by
    the last-arriving workgroup of every (task, kv head) pair (zl_decode_attn_la).  batch_q (B, 1, H, 128) or (B, H, 128);
    workspace from decode_attn_la_workspace (zeroed once).  Returns out, shaped like batch_q."""
    _chk_cuda(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, valid_lens, workspace)
    b, h, d = batch_q.shape[0], batch_q.shape[-2], batch_q.shape[-1]
    if batch_q.dim() == 4 and batch_q.shape[1] != 1:
        raise ZLError("decode_attention_la: one query row per task")
    if out is None:
        out = torch.empty_like(batch_q)
    check(lib().zl_decode_attn_la(_p(batch_q), _p(buf_lens), _p(key_buf_addrs), _p(val_buf_addrs), _p(valid_lens), _p(out),
                                  _p(workspace), _i(b), _i(h), _i(num_kv_heads), _i(d), _f(scale), _i(max_len_buf),
                                  C.c_int(int(bshd)), C.c_int(_dt(batch_q)), _i(split_len),
                                  C.c_int(int(bool(half)) | (int(os.environ.get("ZL_ATTN_LA_WAVES", "0") or 0) << 8)), _stream()),
          "decode_attn_la")
    return out


def attn_merge_plan(b, num_heads, num_kv_heads, dim_head, max_len_buf, w, dtype=torch.float16):
    """(split_len, max_splits) when zl_decode_attn_splits + zl_w4a16_gemm_attn_merge cover this decode batch and
    projection weight, else None (callers use multi_query_attention_rag_buffer + w4_linear).  ZL_ATTN_MERGE_MAX_B
    (default 1) bounds the batch: every workgroup of the projection merges all rows, which stops paying early."""
    if not isinstance(w, W4MWeight) or dim_head != 128 or num_heads % num_kv_heads or num_heads // num_kv_heads > 16:
        return None
    if b > min(4, int(os.environ.get("ZL_ATTN_MERGE_MAX_B", "1"))) or w.k != num_heads * 128 or w.k > 4096:
        return None
    split_len = int(lib().zl_decode_attn_split_len(_i(b), _i(num_kv_heads), _i(max_len_buf)))
    max_splits = (max_len_buf + split_len - 1) // split_len
    cus = lib().zl_device_cu_count()
    if max_splits > 16 or (w.n + 15) // 16 > 2 * (cus if cus > 0 else 256):
        return None
    return split_len, max_splits, _merge_half_dtype(dtype)     # [2]: fp16 partial records (decided ONCE, for both launches)


def _merge_half_dtype(dtype):
    return _merge_half() and dtype == torch.float16


def _merge_half(t=None):
    """half-precision split partials + the integer-plane merging projection (zl_decode_attn_splits_h /
    zl_w4a16_gemm_attn_merge_h) unless the round-2 kernels are asked for (ZL_W4_SMALL_ALGO=1) or the rows are not fp16"""
    return os.environ.get("ZL_W4_SMALL_ALGO", "0") != "1" and os.environ.get("ZL_ATTN_MERGE_HALF", "1") != "0" and \
        (t is None or t.dtype == torch.float16)


def decode_attention_splits(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, valid_lens, scale, max_len_buf, num_kv_heads,
                            workspace, bshd=True):
    """multi_query_attention_rag_buffer without its merge launch: the split-KV partials stay in `workspace` for
    w4_attn_out_merge.  batch_q (B, 1, H, 128) or (B, H, 128)."""
    _chk_cuda(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, valid_lens, workspace)
    b, h, d = batch_q.shape[0], batch_q.shape[-2], batch_q.shape[-1]
    if _merge_half(batch_q):
        check(lib().zl_decode_attn_splits_h(_p(batch_q), _p(buf_lens), _p(key_buf_addrs), _p(val_buf_addrs), _p(valid_lens),
                                            _p(workspace), _i(b), _i(h), _i(num_kv_heads), _i(d), _f(scale), _i(max_len_buf),
                                            C.c_int(int(bshd)), _stream()), "decode_attn_splits_h")
        return workspace
    check(lib().zl_decode_attn_splits(_p(batch_q), _p(buf_lens), _p(key_buf_addrs), _p(val_buf_addrs), _p(valid_lens),
                                      _p(workspace), _i(b), _i(h), _i(num_kv_heads), _i(d), _f(scale), _i(max_len_buf),
                                      C.c_int(int(bshd)), C.c_int(_dt(batch_q)), _stream()), "decode_attn_splits")
    return workspace


def decode_attention_splits_mask(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, mask, scale, max_len_buf, num_kv_heads, workspace,
                                 bshd=True):
    """decode_attention_splits with the reference's int8 visibility mask (one row of buf_lens[b] entries per task) instead of prefix
    lengths (zl_decode_attn_splits_h_mask): half-precision records of EVERY split of the buffer; the merging projection
    (w4_attn_out_merge) and decode_attention_combine_h take them with valid_lens = buf_lens.  fp16 only."""
    _chk_cuda(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, mask, workspace)
    b, h, d = batch_q.shape[0], batch_q.shape[-2], batch_q.shape[-1]
    if batch_q.dtype != torch.float16:
        raise ZLError("decode_attention_splits_mask: fp16 rows")
    check(lib().zl_decode_attn_splits_h_mask(_p(batch_q), _p(buf_lens), _p(key_buf_addrs), _p(val_buf_addrs), _p(mask), _p(workspace),
                                             _i(b), _i(h), _i(num_kv_heads), _i(d), _f(scale), _i(max_len_buf), C.c_int(int(bshd)),
                                             _stream()), "decode_attn_splits_h_mask")


def decode_attention_combine_h(workspace, buf_lens, valid_lens, b, h, num_kv_heads, max_len_buf, out=None):
    """the merge of half-precision split records as a launch of its own (zl_decode_attn_combine_h): bit for bit the rows
    w4_attn_out_merge's prologue multiplies.  valid_lens None: every split of the buffer (the mask form's records)."""
    _chk_cuda(workspace, buf_lens, valid_lens)
    if out is None:
        out = torch.empty((b, 1, h, 128), dtype=torch.float16, device=workspace.device)
    check(lib().zl_decode_attn_combine_h(_p(workspace), _p(buf_lens), _p(valid_lens), _p(out), _i(b), _i(h), _i(num_kv_heads),
                                         _i(max_len_buf), _stream()), "decode_attn_combine_h")
    return out


def w4_attn_out_merge(workspace, buf_lens, valid_lens, plan, b, w, bias=None, residual=None, out=None, epilogue=0):
    """attn_out projection whose activation rows are merged from the decode attention's split-KV partials in the GEMV
    prologue (zl_w4a16_gemm_attn_merge): bit-identical to the merge launch + w4a16_gemm_mfma."""
    _chk_cuda(workspace, buf_lens, valid_lens, bias, residual)
    split_len, max_splits = plan[0], plan[1]
    if out is None:
        out = torch.empty((b, w.n), dtype=torch.float16, device=workspace.device)
    if bias is not None:
        epilogue |= EPI_BIAS
    # the partial layout was decided by decode_attention_splits from the query dtype; the plan carries that decision
    # (a bare _merge_half() here read fp16 records out of an fp32 workspace for non-fp16 queries)
    half = plan[2] if len(plan) > 2 else _merge_half()
    if half:
        opts = _w4_opts(workspace.device, b, w.n)
        check(lib().zl_w4a16_gemm_attn_merge_h_ex(_p(workspace), _p(buf_lens), _p(valid_lens), _i(split_len), _i(max_splits),
                                                  _p(w.qw), _p(w.meta), _p(bias), _p(residual), _p(out), _i(b), _i(w.n), _i(w.k),
                                                  _i(w.group_size), C.c_int(epilogue), C.byref(opts), _stream()),
              "w4a16_gemm_attn_merge_h")
        return out
    check(lib().zl_w4a16_gemm_attn_merge(_p(workspace), _p(buf_lens), _p(valid_lens), _i(split_len), _i(max_splits), _p(w.qw),
                                         _p(w.meta), _p(bias), _p(residual), _p(out), _i(b), _i(w.n), _i(w.k),
                                         _i(w.group_size), C.c_int(epilogue), _stream()), "w4a16_gemm_attn_merge")
    return out


_ENGINE_STATE = {}


def engine_state(device):
    """granules + epoch + error words of the fused decode launches (zl_w4a16_attn_out_gate_up): one set per device, shared by
    every layer (the epoch differs per layer and per step)."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    st = _ENGINE_STATE.get(key)
    if st is None:
        st = dict(granules=torch.zeros(4 * 4096 * 4, dtype=torch.uint8, device=device),
                  epoch=torch.ones(1, dtype=torch.int32, device=device), err=torch.zeros(1, dtype=torch.int32, device=device))
        _ENGINE_STATE[key] = st
    return st


def engine_epoch_advance(device, by=256):
    """once per decode step, ahead of the step's fused launches"""
    _need_experimental("engine_epoch_advance")
    st = engine_state(device)
    check(lib().zl_engine_epoch_advance(_p(st["epoch"]), C.c_uint32(by), _stream()), "engine_epoch_advance")


def w4_attn_out_gate_up(workspace, buf_lens, valid_lens, plan, b, w_o, hidden, w_ff, norm_weight, norm_eps, act, layer_index,
                        bias_o=None, bias_ff=None):
    """zl_w4a16_attn_out_gate_up: hidden += attn_out(merge(partials)); act = silu(w_in(ln(hidden))) * w_gated(ln(hidden)) in one
    launch.  Returns False (nothing launched) outside the launcher's range."""
    _chk_cuda(workspace, buf_lens, valid_lens, hidden, norm_weight, act, bias_o, bias_ff)
    split_len, max_splits = plan[0], plan[1]
    if (len(plan) > 2 and not plan[2]) or not experimental_build():
        return False
    st = engine_state(hidden.device)
    rc = lib().zl_w4a16_attn_out_gate_up(_p(workspace), _p(buf_lens), _p(valid_lens), _i(split_len), _i(max_splits), _p(w_o.qw),
                                         _p(w_o.meta), _p(bias_o), _p(hidden), _p(w_ff.qw), _p(w_ff.meta), _p(bias_ff),
                                         _p(norm_weight), _f(norm_eps), _p(act), _i(b), _i(w_o.n), _i(w_o.k), _i(w_ff.n),
                                         _i(w_o.group_size), _p(st["granules"]), _p(st["epoch"]), C.c_uint32(layer_index),
                                         _p(st["err"]), _stream())
    if rc in (-2, -4):                                    # ZL_ESHAPE / ZL_ELIMIT: the caller takes the two launches
        return False
    check(rc, "w4a16_attn_out_gate_up")
    return True


def decode_attention_fused(cos, sin, qkv, placement, buf_lens, valid_lens, k_addrs, v_addrs, num_heads, num_kv_heads,
                           dim_head, scale, max_len_buf, neox=True, bshd=True, out=None, workspace=None):
    """rope_qk_cache + copy_to_rag_buffer2 + multi_query_attention_rag_buffer for len_q == 1 decode rows in
    one launch pair (partial + combine); returns the attention output (B, H*D)."""
    _chk_cuda(cos, sin, qkv, placement, buf_lens, valid_lens, k_addrs, v_addrs)
    b = qkv.shape[0]
    if out is None:
        out = torch.empty((b, num_heads * dim_head), dtype=qkv.dtype, device=qkv.device)
    if workspace is None:
        workspace = decode_attn_workspace(b, 1, num_heads, dim_head, max_len_buf, qkv.device)
    check(lib().zl_decode_attn_fused(_p(cos), _p(sin), _p(qkv), _p(placement), _p(buf_lens), _p(valid_lens), _p(k_addrs),
                                     _p(v_addrs), _p(out), _p(workspace), _i(b), _i(num_heads), _i(num_kv_heads),
                                     _i(dim_head), _f(scale), _i(max_len_buf), C.c_int(int(neox)), C.c_int(int(bshd)),
                                     C.c_int(_dt(qkv)), _stream()), "decode_attn_fused")
    return out


def quant_calc_scale_zp(x, q_zero=128):
    """int8_op::quant_calc_scale(ctx, x, 127, q_zero) (src/nn/quant/int8/quant_kernel.cu:49-80): the INT8 KV cache's
    row quantiser -> (u8 codes (M, K), fp32 scale (M))."""
    _chk_cuda(x)
    xr = x.reshape(-1, x.shape[-1])
    m, k = xr.shape
    q = torch.empty((m, k), dtype=torch.uint8, device=x.device)
    s = torch.empty((m,), dtype=torch.float32, device=x.device)
    check(lib().zl_quant_calc_scale_zp(_p(xr), _p(q), _p(s), _i(m), _i(k), C.c_int(q_zero), C.c_int(_dt(x)), _stream()),
          "quant_calc_scale_zp")
    return q, s


def dequant_group(codes, scale, q_zero=128, dtype=torch.float16, out=None):
    """int8_op::dequant_group (src/nn/quant/int8/quant_reduce_kernel.cu:144-190): rows of codes back to `dtype`,
    out = rn_T((code - q_zero) * scale[row]), the fp32 product rounded once.  codes (..., G) uint8 (q_zero = 128: the INT8 KV
    cache) or int8 (q_zero = 0), scale fp32 with one entry per row; TransformerBuffer::copy(need_dequant) uses it to hand a prompt
    chunk the cached rows of a quantised buffer (src/kvcache/transformer_buffer.cu:135-151)."""
    _chk_cuda(codes, scale)
    if codes.dtype not in (torch.uint8, torch.int8) or scale.dtype != torch.float32:
        raise ZLError("dequant_group: uint8 / int8 codes and fp32 scales")
    if (codes.dtype == torch.uint8) != (q_zero != 0):
        raise ZLError("dequant_group: unsigned codes go with q_zero != 0, signed codes with q_zero = 0")
    if dtype not in (torch.float16, torch.bfloat16):
        raise ZLError("dequant_group: fp16 / bf16 only")
    if codes.dim() < 1 or codes.numel() == 0 or scale.numel() * codes.shape[-1] != codes.numel() or scale.device != codes.device:
        raise ZLError("dequant_group: one scale per row of codes")
    g = codes.shape[-1]
    m = codes.numel() // g
    if out is None:
        out = torch.empty(codes.shape, dtype=dtype, device=codes.device)
    else:
        _chk_out(out.view(m, -1), m, g, dtype, codes.device, "dequant_group")
    check(lib().zl_dequant_group(_p(codes), _p(scale), _p(out), _i(m), _i(g), C.c_int(int(q_zero)),
                                 C.c_int(F16 if dtype == torch.float16 else BF16), _stream()), "dequant_group")
    return out


def quant_copy_to_rag_buffer(placement, buf_lens, k_src, v_src, k_addrs, v_addrs, k_scale_addrs, v_scale_addrs, len_q=1,
                             bshd=True):
    """quant_calc_scale(127, 128) + copy_to_rag_buffer2 for the codes and the scales (attention.cpp:656-676).
    k_src / v_src (B*len_q, Hkv, D)."""
    _chk_cuda(placement, buf_lens, k_src, v_src, k_addrs, v_addrs, k_scale_addrs, v_scale_addrs)
    tokens, hkv, d = k_src.shape
    check(lib().zl_quant_copy_to_rag_buffer(_p(placement), _p(buf_lens), _p(k_src), _p(v_src), _p(k_addrs), _p(v_addrs),
                                            _p(k_scale_addrs), _p(v_scale_addrs), _i(tokens // len_q), _i(len_q), _i(hkv),
                                            _i(d), C.c_int(int(bshd)), C.c_int(_dt(k_src)), _stream()),
          "quant_copy_to_rag_buffer")


def rope_quant_scatter_decode(cos, sin, qkv, placement, buf_lens, k_addrs, v_addrs, k_scale_addrs, v_scale_addrs,
                              num_heads, num_kv_heads, dim_head, neox=True, bshd=True, q_out=None):
    """rope_qk_cache + quantise + scatter of the new K/V rows for len_q == 1 decode rows; returns the rotated q."""
    _chk_cuda(cos, sin, qkv, placement, buf_lens, k_addrs, v_addrs, k_scale_addrs, v_scale_addrs)
    b = qkv.shape[0]
    if q_out is None:
        q_out = torch.empty((b, num_heads * dim_head), dtype=qkv.dtype, device=qkv.device)
    check(lib().zl_rope_quant_scatter_decode(_p(cos), _p(sin), _p(qkv), _p(q_out), _p(placement), _p(buf_lens),
                                             _p(k_addrs), _p(v_addrs), _p(k_scale_addrs), _p(v_scale_addrs), _i(b),
                                             _i(num_heads), _i(num_kv_heads), _i(dim_head), C.c_int(int(neox)),
                                             C.c_int(int(bshd)), C.c_int(_dt(qkv)), _stream()),
          "rope_quant_scatter_decode")
    return q_out


def multi_query_attention_rag_buffer_quant(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, scale_k_addrs, scale_v_addrs,
                                           mask, scale, max_len_buf, num_kv_heads, valid_lens=None, bshd=True, out=None,
                                           workspace=None):
    """nn::multi_query_attention_rag_buffer with scale_key_addrs / scale_val_addrs (INT8 KV cache;
    src/nn/attention/attention_kernel.cu:1384-1416).  batch_q (B, len_q, H, D)."""
    _chk_cuda(batch_q, buf_lens, key_buf_addrs, val_buf_addrs, scale_k_addrs, scale_v_addrs, mask, valid_lens)
    b, len_q, h, d = batch_q.shape
    if out is None:
        out = torch.empty_like(batch_q)
    if workspace is None:
        workspace = decode_attn_workspace(b, len_q, h, d, max_len_buf, batch_q.device)
    check(lib().zl_decode_attn_quant_ex(_p(batch_q), _p(buf_lens), _p(key_buf_addrs), _p(val_buf_addrs), _p(scale_k_addrs),
                                     _p(scale_v_addrs), _p(mask), _p(valid_lens), _p(out), _p(workspace), _i(b),
                                     _i(len_q), _i(h), _i(num_kv_heads), _i(d), _f(scale), _i(max_len_buf),
                                     C.c_int(int(bshd)), C.c_int(_dt(batch_q)), C.c_int(_attn_algo()), _stream()), "decode_attn_quant")
    return out


def prefill_attention(q, k_buf, v_buf, pos0, num_kv_heads, scale, bshd=True, out=None, groups=None):
    """Causal attention of one task's prompt chunk (attn_encode_group -> flash attention in the reference,
    src/nn/attention/attention.cpp:442-622).  q (s_q, H, D); k_buf / v_buf the task's buffers (len_buf, Hkv, D)
    [bshd] or (Hkv, len_buf, D), already holding the chunk's rows at pos0 .. pos0 + s_q - 1."""
    _chk_cuda(q, k_buf, v_buf)
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ZLError("prefill_attention: fp16 / bf16 only")
    s_q, h, d = q.shape
    len_buf = k_buf.shape[0] if bshd else k_buf.shape[1]
    if out is None:
        out = torch.empty_like(q)
    groups = int(os.environ.get("ZL_PREFILL_GROUPS", "0") or 0) if groups is None else groups     # 0: the launcher's choice
    check(lib().zl_prefill_attn_ex(_p(q), _p(k_buf), _p(v_buf), _p(out), _i(s_q), _i(pos0), _i(h), _i(num_kv_heads), _i(d),
                                   _f(scale), _i(len_buf), C.c_int(int(bshd)), C.c_int(_dt(q)), C.c_int(groups), _stream()), "prefill_attn")
    return out


def prefill_work_items(lens, pos0):
    """The work map of zl_prefill_attn_varlen (host only): every (task, 64-row query tile) of the tasks' chunks once, longest first
    -- by the key tiles the tile's last row sees -- ties in task order, the later tile first.  For one task this is the order of
    zl_prefill_attn's own map."""
    keyed = []
    for t, (s, p0) in enumerate(zip(lens, pos0)):
        for qt in range((int(s) + 63) // 64):
            last = min((qt + 1) * 64, int(s))
            keyed.append((-((int(p0) + last + 63) // 64), t, -qt))
    keyed.sort()
    return [(t, -nqt) for _, t, nqt in keyed]


class PrefillVarlenPlan:
    """The device tables of one varlen prompt-attention call, uploaded once per forward and used by every layer: cu_seqlens_q
    (b + 1), pos0 (b), buf_lens (b) and the work table (n_work, 2), in one int32 tensor.  The host lists stay for the checks."""

    def __init__(self, lens, pos0, buf_lens, device):
        self.lens, self.pos0, self.buf_lens = [int(x) for x in lens], [int(x) for x in pos0], [int(x) for x in buf_lens]
        b = self.b = len(self.lens)
        if b < 1 or len(self.pos0) != b or len(self.buf_lens) != b:
            raise ZLError("prefill_varlen_plan: one length, pos0 and buffer length per task")
        for s, p0, lb in zip(self.lens, self.pos0, self.buf_lens):
            if s < 1 or p0 < 0 or p0 + s > lb:
                raise ZLError(f"prefill_varlen_plan: chunk of {s} rows at pos0 {p0} does not fit a buffer of {lb} rows")
        self.work_items = prefill_work_items(self.lens, self.pos0)
        self.n_work = len(self.work_items)
        cu = [0]
        for s in self.lens:
            cu.append(cu[-1] + s)
        self.total_q = cu[-1]
        self.cu = cu
        flat = [x for item in self.work_items for x in item]
        self.tables = torch.tensor(cu + self.pos0 + self.buf_lens + flat, dtype=torch.int32).to(device)
        self.cu_seqlens_q = self.tables[:b + 1]
        self.pos0_dev = self.tables[b + 1:2 * b + 1]
        self.buf_lens_dev = self.tables[2 * b + 1:3 * b + 1]
        self.work = self.tables[3 * b + 1:]


def prefill_varlen_plan(lens, pos0, buf_lens, device):
    """Plan of a varlen prompt-attention call: lens / pos0 / buf_lens are host ints per task (rows of the chunk, position of its
    first row, rows of its K/V buffers); raises ZLError for a chunk that does not fit its buffer.  Returns PrefillVarlenPlan."""
    return PrefillVarlenPlan(lens, pos0, buf_lens, device)


def _varlen_args(what, q, lens, pos0, buf_lens, plan, out, groups):
    """the checks prefill_attention_varlen and prefill_attention_varlen_q8 share, in `what`'s name: q's dtype, the plan against the
    host lists (made here when the caller has none), q's rows against the plan, the plan's device, `out`; the ZL_PREFILL_GROUPS
    default of `groups` -> (plan, out, groups)"""
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ZLError(f"{what}: fp16 / bf16 only")
    if plan is None:
        plan = prefill_varlen_plan(lens, pos0, buf_lens, q.device)
    elif plan.lens != [int(x) for x in lens] or plan.pos0 != [int(x) for x in pos0] or plan.buf_lens != [int(x) for x in buf_lens]:
        raise ZLError(f"{what}: the plan was made for other lengths")
    total_q, h, d = q.shape
    if total_q != plan.total_q:
        raise ZLError(f"{what}: q has {total_q} rows, the lengths add up to {plan.total_q}")
    if plan.tables.device != q.device:
        raise ZLError(f"{what}: the plan lives on another device")
    if out is None:
        out = torch.empty_like(q)
    else:
        _chk_out(out.view(total_q, -1), total_q, h * d, q.dtype, q.device, what)
    groups = int(os.environ.get("ZL_PREFILL_GROUPS", "0") or 0) if groups is None else groups     # 0: the launcher's choice
    return plan, out, groups


def prefill_attention_varlen(q, lens, pos0, k_addrs, v_addrs, buf_lens, num_kv_heads, scale, bshd=True, out=None, groups=None,
                             plan=None):
    """Causal attention of B tasks' prompt chunks in one launch (attn_encode_group's per-task flash-attention loop,
    src/nn/attention/attention.cpp:442-562, as one varlen call).  q (total_q, H, D): task i's rows back to back, lens[i] of them, at
    positions pos0[i] ..; k_addrs / v_addrs device int64 tables of the tasks' K/V buffers (buf_lens[i] rows each, BSHD or BHSD),
    which already hold the chunks' own rows.  lens / pos0 / buf_lens are host ints (checked here); `plan` (prefill_varlen_plan of
    the same lists) spares the upload when several layers share it.  Per task bit-identical to prefill_attention(.., groups)."""
    _chk_cuda(q, k_addrs, v_addrs)
    plan, out, groups = _varlen_args("prefill_attention_varlen", q, lens, pos0, buf_lens, plan, out, groups)
    total_q, h, d = q.shape
    for t in (k_addrs, v_addrs):
        if t.dtype != torch.int64 or t.numel() != plan.b:
            raise ZLError("prefill_attention_varlen: one int64 K / V pointer per task")
    check(lib().zl_prefill_attn_varlen(_p(q), _p(plan.cu_seqlens_q), _p(plan.pos0_dev), _p(plan.buf_lens_dev), _p(k_addrs),
                                       _p(v_addrs), _p(out), _p(plan.work), _i(plan.n_work), _i(plan.b), _i(total_q), _i(h),
                                       _i(num_kv_heads), _i(d), _f(scale), C.c_int(int(bshd)), C.c_int(_dt(q)), C.c_int(groups),
                                       _stream()), "prefill_attn_varlen")
    return out


def _q8_cache_table(x, plan, hkv, d, dtype, what, device):
    """one operand of prefill_attention_varlen_q8: the device int64 pointer table a context keeps (one pointer per task; what the
    pointers lead to cannot be checked here), or the per-task tensors themselves -- (buf_lens[i], Hkv, D) uint8 codes or
    (buf_lens[i], Hkv) fp32 scales, checked, None for a task without history -- from which the table is made"""
    if torch.is_tensor(x):
        if not (x.is_cuda and x.is_contiguous()) or x.device != device or x.dtype != torch.int64 or x.numel() != plan.b:
            raise ZLError(f"prefill_attention_varlen_q8: {what}: one int64 pointer per task, on q's device")
        return x
    if len(x) != plan.b:
        raise ZLError(f"prefill_attention_varlen_q8: {what}: one tensor per task")
    ptrs = []
    for i, t in enumerate(x):
        if t is None and plan.pos0[i] == 0:
            ptrs.append(0)
            continue
        shape = (plan.buf_lens[i], hkv, d) if d else (plan.buf_lens[i], hkv)
        if t is None or t.dtype != dtype or tuple(t.shape) != shape or t.device != device or not t.is_contiguous():
            raise ZLError(f"prefill_attention_varlen_q8: {what} of task {i}: a contiguous {dtype} tensor of shape {shape} on q's device")
        ptrs.append(t.data_ptr())
    return torch.tensor(ptrs, dtype=torch.int64).to(device)


def prefill_attention_varlen_q8(q, lens, pos0, k_new, v_new, k_addrs, v_addrs, ks_addrs, vs_addrs, buf_lens, num_kv_heads, scale,
                                out=None, groups=None, plan=None):
    """prefill_attention_varlen for chunks that continue rows of an INT8 K/V cache, the history dequantised inside the kernel (the
    reference's fall-back for a quantised buffer without prompt temporaries, attention.cpp:510-516: dequant_group into a fresh
    buffer + the chunk's rows + flash attention; bit-identical to dequant_group + prefill_attention_varlen on such buffers, with no
    buffer).  q (total_q, H, D) and k_new / v_new (total_q, Hkv, D): the tasks' rotated rows back to back, unquantised; key row j of
    task i is cache row j for j < pos0[i] -- rn_T((code - 128) * scale) -- and row j - pos0[i] of its k_new / v_new slice from
    there on: the cache is not read at or beyond pos0[i].  k_addrs / v_addrs / ks_addrs / vs_addrs: device int64 tables of the
    tasks' code (buf_lens[i], Hkv, D) u8 and scale (buf_lens[i], Hkv) fp32 buffers, BSHD, or the per-task tensors themselves (then
    checked; None for a task with pos0 = 0).  D = 128.  lens / pos0 / buf_lens / plan as for prefill_attention_varlen."""
    _chk_cuda(q, k_new, v_new)
    if q.dim() != 3 or k_new.dim() != 3:
        raise ZLError("prefill_attention_varlen_q8: q (total_q, H, D), k_new / v_new (total_q, Hkv, D)")
    total_q, h, d = q.shape
    if d != 128:
        raise ZLError(f"prefill_attention_varlen_q8: head size {d}: only 128 (the mask-form attention reads a chunk's own rows as codes)")
    plan, out, groups = _varlen_args("prefill_attention_varlen_q8", q, lens, pos0, buf_lens, plan, out, groups)
    if num_kv_heads < 1 or h % num_kv_heads:
        raise ZLError("prefill_attention_varlen_q8: H must be a multiple of Hkv")
    for t in (k_new, v_new):
        if tuple(t.shape) != (total_q, num_kv_heads, d) or t.dtype != q.dtype or t.device != q.device:
            raise ZLError("prefill_attention_varlen_q8: k_new / v_new: (total_q, Hkv, D) rows of q's dtype on q's device")
    k_tab = _q8_cache_table(k_addrs, plan, num_kv_heads, d, torch.uint8, "k codes", q.device)
    v_tab = _q8_cache_table(v_addrs, plan, num_kv_heads, d, torch.uint8, "v codes", q.device)
    ks_tab = _q8_cache_table(ks_addrs, plan, num_kv_heads, 0, torch.float32, "k scales", q.device)
    vs_tab = _q8_cache_table(vs_addrs, plan, num_kv_heads, 0, torch.float32, "v scales", q.device)
    check(lib().zl_prefill_attn_varlen_q8(_p(q), _p(plan.cu_seqlens_q), _p(plan.pos0_dev), _p(plan.buf_lens_dev), _p(k_tab),
                                          _p(v_tab), _p(ks_tab), _p(vs_tab), _p(k_new), _p(v_new), _p(out), _p(plan.work),
                                          _i(plan.n_work), _i(plan.b), _i(total_q), _i(h), _i(num_kv_heads), _i(d), _f(scale),
                                          C.c_int(_dt(q)), C.c_int(groups), _stream()), "prefill_attn_varlen_q8")
    return out


def prefill_attention_varlen_hist(q, lens, pos0, k_new, v_new, hist_k_addrs, hist_v_addrs, hist_lens, buf_lens, num_kv_heads, scale,
                                  out=None, groups=None, plan=None, hist_lens_dev=None):
    """prefill_attention_varlen for chunks that continue rows held in ANOTHER, unquantised buffer (a prompt encoded on top of a shared
    prefix): key row j of task i is row j of its history buffer for j < pos0[i] and row j - pos0[i] of its k_new / v_new slice from
    there on -- bit-identical to prefill_attention_varlen on buffers that hold both.  q (total_q, H, 128), k_new / v_new (total_q, Hkv,
    128); hist_k_addrs / hist_v_addrs: device int64 tables of the tasks' history buffers ((hist_lens[i], Hkv, 128), BSHD; 0 for a task
    with pos0 = 0); hist_lens: host ints, pos0[i] <= hist_lens[i] (checked here).  lens / pos0 / buf_lens / plan as for
    prefill_attention_varlen (buf_lens[i]: the keys a task may see at most, pos0[i] + lens[i] <= buf_lens[i]).  hist_lens_dev: the
    caller's int32 device copy of hist_lens (several layers share it), made here otherwise."""
    what = "prefill_attention_varlen_hist"
    _chk_cuda(q, k_new, v_new, hist_k_addrs, hist_v_addrs)
    if q.dim() != 3 or k_new.dim() != 3:
        raise ZLError(f"{what}: q (total_q, H, D), k_new / v_new (total_q, Hkv, D)")
    total_q, h, d = q.shape
    if d != 128:
        raise ZLError(f"{what}: head size {d}: only 128")
    plan, out, groups = _varlen_args(what, q, lens, pos0, buf_lens, plan, out, groups)
    if num_kv_heads < 1 or h % num_kv_heads:
        raise ZLError(f"{what}: H must be a multiple of Hkv")
    for t in (k_new, v_new):
        if tuple(t.shape) != (total_q, num_kv_heads, d) or t.dtype != q.dtype or t.device != q.device:
            raise ZLError(f"{what}: k_new / v_new: (total_q, Hkv, D) rows of q's dtype on q's device")
    for t in (hist_k_addrs, hist_v_addrs):
        if t.dtype != torch.int64 or t.numel() != plan.b or t.device != q.device:
            raise ZLError(f"{what}: one int64 history pointer per task, on q's device")
    hl = [int(x) for x in hist_lens]
    if len(hl) != plan.b or any(p0 > n for p0, n in zip(plan.pos0, hl)):
        raise ZLError(f"{what}: one history length per task, none below the task's pos0")
    if hist_lens_dev is None:
        hist_lens_dev = torch.tensor(hl, dtype=torch.int32).to(q.device)
    elif hist_lens_dev.dtype != torch.int32 or hist_lens_dev.numel() != plan.b or hist_lens_dev.device != q.device:
        raise ZLError(f"{what}: hist_lens_dev: one int32 per task on q's device")
    check(lib().zl_prefill_attn_varlen_hist(_p(q), _p(plan.cu_seqlens_q), _p(plan.pos0_dev), _p(plan.buf_lens_dev), _p(hist_k_addrs),
                                            _p(hist_v_addrs), _p(hist_lens_dev), _p(k_new), _p(v_new), _p(out), _p(plan.work),
                                            _i(plan.n_work), _i(plan.b), _i(total_q), _i(h), _i(num_kv_heads), _i(d), _f(scale),
                                            C.c_int(_dt(q)), C.c_int(groups), _stream()), "prefill_attn_varlen_hist")
    return out


def element_add_scale(a, b, scale=1.0, scale_residual=True, out=None):
    """nn::element_add_scale_out (src/nn/block/block_kernel.cu:19-50)."""
    _chk_cuda(a, b)
    if a.shape != b.shape:
        raise ZLError("a,b shape mismatch")
    if out is None:
        out = torch.empty_like(a)
    check(lib().zl_element_add_scale(_p(a), _p(b), _p(out), _i(a.numel()), _f(scale), C.c_int(int(scale_residual)),
                                     C.c_int(_dt(a)), _stream()), "element_add_scale")
    return out


def permute_input(x, perm, out=None):
    """nn::gptq::permute_input (src/nn/quant/gptq/gptq.h:155-159): out[..., i] = x[..., perm[i]] (perm int32, any length)."""
    _chk_cuda(x, perm)
    if perm.dtype != torch.int32:
        raise ZLError("perm dtype mismatch")
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    k = perm.numel()
    if out is None:
        out = torch.empty((x2.shape[0], k), dtype=x.dtype, device=x.device)
    check(lib().zl_permute_input(_p(x2), _i(x2.stride(0)), _p(perm), _p(out), _i(x2.shape[0]), _i(k), _stream()), "permute_input")
    return out


def gate_mul(inp, in2, gate_type="silu", out=None):
    """nn::gate_mul_inplace (src/nn/linear/activation_kernel.cu:82-106); out defaults to in place."""
    _chk_cuda(inp, in2)
    if gate_type not in ("silu", "gelu"):
        raise ZLError("Unsupported gate type: " + gate_type)
    out = inp if out is None else out
    check(lib().zl_gate_mul(_p(inp), _p(in2), _p(out), _i(inp.numel()), C.c_int(0 if gate_type == "silu" else 1),
                            C.c_int(_dt(inp)), _stream()), "gate_mul")
    return out


def embedding(ids, weight, scale=1.0, begin=0, end=None):
    """RawEmbedding::forward (src/nn/embedding/embedding.cu:260-272)."""
    _chk_cuda(ids, weight)
    if ids.dtype != torch.int32:
        raise ZLError("ids dtype mismatch")
    end = begin + weight.shape[0] if end is None else end
    out = torch.empty(tuple(ids.shape) + (weight.shape[1],), dtype=weight.dtype, device=weight.device)
    check(lib().zl_embedding(_p(ids), _p(weight), _p(out), _i(ids.numel()), _i(weight.shape[1]), C.c_int32(begin),
                             C.c_int32(end), _f(scale), C.c_int(_dt(weight)), _stream()), "embedding")
    return out


def embedding_rope(ids, weight, scale, pos, dim_head, base, neox=True, llama3=None):
    """embedding + rope_cos_sin in one launch (the first two kernels of a decode step): (hidden, cos, sin), bit-identical to the
    two calls"""
    _chk_cuda(ids, weight, pos)
    if ids.dtype != torch.int32 or pos.numel() != ids.numel():
        raise ZLError("ids dtype mismatch / one position per token")
    s = ids.numel()
    out = torch.empty(tuple(ids.shape) + (weight.shape[1],), dtype=weight.dtype, device=weight.device)
    cs = torch.empty((s, dim_head), dtype=torch.float32, device=pos.device)
    sn = torch.empty_like(cs)
    fac, low, high, old = llama3 if llama3 is not None else (1.0, 1.0, 1.0, 1.0)
    check(lib().zl_embedding_rope(_p(ids), _p(weight), _p(out), _i(s), _i(weight.shape[1]), C.c_int32(0), C.c_int32(weight.shape[0]), _f(scale),
                                  C.c_int(_dt(weight)), _p(pos), _p(cs), _p(sn), _i(dim_head), _f(base), C.c_int(int(neox)),
                                  C.c_int(int(llama3 is not None)), _f(fac), _f(low), _f(high), _f(old), _stream()), "embedding_rope")
    return out, cs, sn


# --------------------------------------------------------------------------------------------------
# a8..a11: INT8
# --------------------------------------------------------------------------------------------------
W8_BACK, W8_BACK_ADD, W8_ACT_SILU, W8_ACT_GELU = 0, 1, 2, 3


class W8MWeight:
    """int8 weight (N, K) in the ZLW8M streaming layout of zl_w8a8_gemm_phase + its per-row scale (T, interleaved with
    the rows when row_interleave)."""

    def __init__(self, n, k, qw, scale, row_interleave=False):
        self.n, self.k, self.qw, self.scale, self.row_interleave = n, k, qw, scale, row_interleave

    @classmethod
    def from_rows(cls, w_int8, scale, row_interleave=False):
        _chk_cuda(w_int8, scale)
        n, k = w_int8.shape
        nbytes = lib().zl_w8m_bytes(_i(n), _i(k))
        if nbytes < 0:
            check(int(nbytes), "w8m_bytes")
        qw = torch.empty(nbytes, dtype=torch.uint8, device=w_int8.device)
        check(lib().zl_w8m_pack(_p(w_int8.contiguous()), _i(n), _i(k), C.c_int(int(row_interleave)), _p(qw), _stream()), "w8m_pack")
        if row_interleave:
            scale = torch.stack([scale[:n // 2], scale[n // 2:]], dim=1).reshape(-1)
        return cls(n, k, qw, scale.contiguous(), row_interleave)

    def nbytes(self):
        return self.qw.numel() + self.scale.numel() * 2


def w8a8_gemm_phase(xq, sx, w: W8MWeight, epilogue=W8_BACK, addend=None, scale=1.0, out=None, dtype=torch.float16):
    """Int8Linear GEMM + scale-back in one launch for 1..32 rows (zl_w8a8_gemm_phase)."""
    _chk_cuda(xq, sx, addend, out)
    m, k = xq.shape
    if k != w.k:
        raise ZLError("w8a8_gemm_phase: K mismatch")
    gated = epilogue in (W8_ACT_SILU, W8_ACT_GELU)
    if gated != w.row_interleave:
        raise ZLError("w8a8_gemm_phase: gated epilogues need a row-interleaved weight (and only they do)")
    if out is None:
        out = torch.empty((m, w.n // 2 if gated else w.n), dtype=dtype, device=xq.device)
    rounds = int(os.environ.get("ZL_W8_PHASE_ROUNDS", "0") or 0)     # tests sweep the instantiations
    check(lib().zl_w8a8_gemm_phase_ex(_p(xq), _p(sx), _p(w.qw), _p(w.scale), _p(addend), _p(out), _i(m), _i(w.n), _i(k), _f(scale),
                                      C.c_int(epilogue), C.c_int(_dt(out)), C.c_int(rounds), _stream()), "w8a8_gemm_phase")
    return out


def w8a8_qkv_rope_scatter(xq, sx, w: W8MWeight, cos, sin, placement, buf_lens, k_addrs, v_addrs, num_heads, num_kv_heads,
                          dim_head, bshd=True, q_out=None, dtype=torch.float16):
    """INT8 fused qkv projection + scale-back + neox rotary + KV scatter for decode rows; returns the rotated q (M, H*D)."""
    _chk_cuda(xq, sx, cos, sin, placement, buf_lens, k_addrs, v_addrs)
    m, k = xq.shape
    if k != w.k or w.n != (num_heads + 2 * num_kv_heads) * dim_head or w.row_interleave:
        raise ZLError("w8a8_qkv_rope_scatter: weight shape")
    if q_out is None:
        q_out = torch.empty((m, num_heads * dim_head), dtype=dtype, device=xq.device)
    check(lib().zl_w8a8_qkv_rope_scatter(_p(xq), _p(sx), _p(w.qw), _p(w.scale), _p(cos), _p(sin), _p(placement), _p(buf_lens),
                                         _p(k_addrs), _p(v_addrs), _p(q_out), _i(m), _i(num_heads), _i(num_kv_heads),
                                         _i(dim_head), _i(k), C.c_int(int(bshd)), C.c_int(_dt(q_out)), _stream()),
          "w8a8_qkv_rope_scatter")
    return q_out


def quant_calc_scale(x):
    """int8_op::quant_calc_scale (src/nn/quant/int8/quant_kernel.cu:49-103) -> (int8 (M,K), fp32 scale (M))."""
    _chk_cuda(x)
    xr = x.reshape(-1, x.shape[-1])
    m, k = xr.shape
    q = torch.empty((m, k), dtype=torch.int8, device=x.device)
    s = torch.empty((m,), dtype=torch.float32, device=x.device)
    check(lib().zl_quant_calc_scale(_p(xr), _p(q), _p(s), _i(m), _i(k), C.c_int(_dt(x)), _stream()), "quant_calc_scale")
    return q, s


def layernorm_quant(x, weight, eps, scale=1.0):
    """int8_op::layernorm_quant (src/nn/quant/int8/quant_kernel.cu:153-227) -> (T out, int8, fp32 scale)."""
    _chk_cuda(x, weight)
    xr = x.reshape(-1, x.shape[-1])
    rows, dim = xr.shape
    out = torch.empty_like(xr)
    q = torch.empty((rows, dim), dtype=torch.int8, device=x.device)
    s = torch.empty((rows,), dtype=torch.float32, device=x.device)
    check(lib().zl_rmsnorm_quant(_p(xr), _p(weight), _p(out), _p(q), _p(s), _i(rows), _i(dim), _f(eps), _f(scale),
                                 C.c_int(_dt(x)), _stream()), "layernorm_quant")
    return out, q, s


def int8_gemm_nt(a, b, out=None):
    """int8 (M,K) x int8 (N,K)^T -> int32 (M,N): the IMMA GEMM of Int8Linear::forward."""
    _chk_cuda(a, b)
    m, k = a.shape
    n = b.shape[0]
    c = out if out is not None else torch.empty((m, n), dtype=torch.int32, device=a.device)
    check(lib().zl_int8_gemm_nt(_p(a), _p(b), _p(c), _i(m), _i(n), _i(k), _stream()), "int8_gemm_nt")
    return c


def quant_scale_back(c, scale_x, scale_y, dtype=torch.float16, out=None):
    """int8_op::quant_scale_back (src/nn/quant/int8/quant_kernel.cu:248-306)."""
    _chk_cuda(c, scale_x, scale_y)
    m, n = c.shape
    if out is None:
        out = torch.empty((m, n), dtype=dtype, device=c.device)
    check(lib().zl_quant_scale_back(_p(c), _p(scale_x), _p(scale_y), _p(out), _i(m), _i(n), C.c_int(_dt(out)),
                                    _stream()), "quant_scale_back")
    return out


def quant_back_act_mul(a, a_sx, a_sy, b, b_sx, b_sy, act="silu", dtype=torch.float16):
    """int8_op::quant_back_act_mul (src/nn/quant/int8/quant_kernel.cu:616-676)."""
    _chk_cuda(a, a_sx, a_sy, b, b_sx, b_sy)
    m, n = a.shape
    out = torch.empty((m, n), dtype=dtype, device=a.device)
    check(lib().zl_quant_back_act_mul(_p(a), _p(a_sx), _p(a_sy), _p(b), _p(b_sx), _p(b_sy), _p(out), _i(m), _i(n),
                                      C.c_int(0 if act == "silu" else 1), C.c_int(_dt(out)), _stream()),
          "quant_back_act_mul")
    return out


def quant_scale_back3(c, scale_x, scale_y, dim_q, dim_kv):
    """int8_op::quant_scale_back3 (src/nn/quant/int8/quant_kernel.cu:311-384): fused qkv int32 -> q, k, v."""
    _chk_cuda(c, scale_x, scale_y)
    m, n = c.shape
    if dim_q + 2 * dim_kv != n:
        raise ZLError("Wrong size")
    mk = lambda w: torch.empty((m, w), dtype=scale_y.dtype, device=c.device)  # noqa: E731
    q, k, v = mk(dim_q), mk(dim_kv), mk(dim_kv)
    check(lib().zl_quant_scale_back3(_p(c), _p(scale_x), _p(scale_y), _p(q), _p(k), _p(v), _i(m), _i(n), _i(dim_q),
                                     _i(dim_kv), C.c_int(_dt(q)), _stream()), "quant_scale_back3")
    return q, k, v


def quant_back_element_add_scale(a, scale_x, scale_y, b, scale=1.0, out=None):
    """int8_op::quant_back_element_add_scale (quant_kernel.cu:530-583): T((back(a) + float(b)) * scale);
    out may alias b (element-wise)."""
    _chk_cuda(a, scale_x, scale_y, b)
    m, n = a.shape
    if out is None:
        out = torch.empty((m, n), dtype=b.dtype, device=a.device)
    check(lib().zl_quant_back_element_add_scale(_p(a), _p(scale_x), _p(scale_y), _p(b), _f(scale), _p(out), _i(m), _i(n),
                                                C.c_int(_dt(out)), _stream()), "quant_back_element_add_scale")
    return out


def quant_back_transpose(h_q, scale_x, scale_y):
    """int8_op::quant_back_transpose (quant_kernel.cu:475-527): (B, len_q, H, D) int32 -> (B, H, len_q, D)."""
    _chk_cuda(h_q, scale_x, scale_y)
    if h_q.dim() != 4:
        raise ZLError("input is not 4d")
    b, t, h, d = h_q.shape
    out = torch.empty((b, h, t, d), dtype=scale_y.dtype, device=h_q.device)
    check(lib().zl_quant_back_transpose(_p(h_q), _p(scale_x), _p(scale_y), _p(out), _i(b), _i(t), _i(h), _i(d),
                                        C.c_int(_dt(out)), _stream()), "quant_back_transpose")
    return out


def quant_back_copy_to_buffer(src, scale_x, scale_y, placement, dst):
    """int8_op::quant_back_copy_to_buffer (quant_kernel.cu:389-469): src (B, len_kv, H, D) or (len_kv, H, D) int32
    scattered into dst (B, H, len_buf, D) / (H, len_buf, D) at placement (None = identity, < 0 = skipped)."""
    _chk_cuda(src, scale_x, scale_y, placement, dst)
    if not ((src.dim() == 3 and dst.dim() == 3) or (src.dim() == 4 and dst.dim() == 4)):
        raise ZLError("src and dst must be 3/4-dimensional")
    batch = 1 if src.dim() == 3 else src.shape[0]
    len_kv, h, d = src.shape[-3:]
    len_buf = dst.shape[-2]
    if dst.shape[-3] != h or dst.shape[-1] != d:
        raise ZLError("dim mismatch")
    src_stride = 0 if src.dim() == 3 else src.stride(0)
    dst_stride = 0 if dst.dim() == 3 else dst.stride(0)
    place_stride = 0 if placement is None or placement.dim() == 1 else placement.stride(0)
    check(lib().zl_quant_back_copy_to_buffer(_p(src), _p(scale_x), _p(scale_y), _p(placement), _p(dst), _i(batch),
                                             _i(len_kv), _i(h), _i(d), _i(len_buf), _i(src_stride), _i(dst_stride),
                                             _i(place_stride), C.c_int(_dt(dst)), _stream()), "quant_back_copy_to_buffer")
    return dst


# --------------------------------------------------------------------------------------------------
# a7  AWQ checkpoints in their on-disk layout (no repack) and f3  W4A8
# --------------------------------------------------------------------------------------------------
def awq_dequantize(qweight, qzeros, scales, group_size):
    """nn::awq::awq_dequantize (src/nn/quant/awq/gemm_kernels.cu:277-330): (K, N/8) int32 -> W16 (K, N) fp16."""
    _chk_cuda(qweight, qzeros, scales)
    k, n = qweight.shape[0], qweight.shape[1] * 8
    out = torch.empty((k, n), dtype=torch.float16, device=qweight.device)
    check(lib().zl_awq_dequantize(_p(qweight), _p(qzeros), _p(scales), _p(out), _i(k), _i(n), _i(group_size), _stream()),
          "awq_dequantize")
    return out


def awq_gemm(x, qweight, qzeros, scales, group_size, split_k_iters=32, out=None):
    """nn::awq::awq_gemm (gemm_kernels.cu:404-468) on the AWQ tensors as stored: split-K with fp16 partials summed in fp32."""
    if x.dtype != torch.float16:
        raise ZLError("in_feats must be half")
    _chk_cuda(x, qweight, qzeros, scales)
    x2 = x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    n = qweight.shape[1] * 8
    if qweight.shape[0] != k:
        raise ZLError("size K mismatch")
    if n % 64:
        raise ZLError("OC is not multiple of cta_N = 64")
    if group_size % 32:
        raise ZLError("Group size should be a multiple of 32")
    if out is None:
        out = torch.empty((m, n), dtype=torch.float16, device=x.device)
    ws = torch.empty(int(lib().zl_awq_gemm_workspace_bytes(_i(min(m, 8)), _i(n), _i(split_k_iters))), dtype=torch.uint8, device=x.device)
    check(lib().zl_awq_gemm(_p(x2), _i(x2.stride(0)), _p(qweight), _p(qzeros), _p(scales), _p(out), _p(ws), _i(m), _i(n), _i(k),
                            _i(group_size), _i(split_k_iters), _stream()), "awq_gemm")
    return out


def w4a8_weight_to_int8(w16):
    """Int4GPTQ::calc_w4a8_scale + dequant_k_major(out_type 1): W16 (N, K) fp16 -> (w8 int8 (N, K), scale fp32 (N))."""
    _chk_cuda(w16)
    n, k = w16.shape
    w8 = torch.empty((n, k), dtype=torch.int8, device=w16.device)
    sc = torch.empty((n,), dtype=torch.float32, device=w16.device)
    check(lib().zl_w4a8_weight_to_int8(_p(w16), _p(w8), _p(sc), _i(n), _i(k), _stream()), "w4a8_weight_to_int8")
    return w8, sc


def quant_scale_back_f32(c, sx, sy, out=None):
    """quant_scale_back with an fp32 per-row weight scale (the W4A8 forward): half(float(c) * sx[m] * sy[n])"""
    _chk_cuda(c, sx, sy)
    m, n = c.shape
    if out is None:
        out = torch.empty((m, n), dtype=torch.float16, device=c.device)
    check(lib().zl_quant_scale_back_f32(_p(c), _p(sx), _p(sy), _p(out), _i(m), _i(n), _stream()), "quant_scale_back_f32")
    return out


def w4a8_linear(x, w8, w_scale, out=None):
    """gptq_gemm_k_major's W4_INT8 branch (q_gemm_k_major.cu:1036-1073): quantise the activation rows, int8 x int8 -> int32
    on the matrix cores, scale back with the fp32 weight scale."""
    xq, sx = quant_calc_scale(x)
    return quant_scale_back_f32(int8_gemm_nt(xq, w8), sx, w_scale, out=out)


# ---- INT8-compressed tensor-parallel reduce (ModelContext::reduce_tp_int8, src/model/model_context.cpp:244-326)
def quant_group_32(x):
    """int8_op::quant_group_32: x (..., 32 * g) T -> (codes int8 same shape, scales T (groups,))"""
    _chk_cuda(x)
    if x.numel() % 32:
        raise ZLError("[quant_group_32]")
    groups = x.numel() // 32
    q = torch.empty(x.shape, dtype=torch.int8, device=x.device)
    s = torch.empty(groups, dtype=x.dtype, device=x.device)
    check(lib().zl_quant_group_32(_p(x), _p(q), _p(s), _i(groups), C.c_int(_dt(x)), _stream()), "quant_group_32")
    return q, s


def dequant_sum_quant_g32(my, q_others, scale_others):
    """int8_op::dequant_sum_quant_g32: my (M, 32) T, q_others (WS - 1, M, 32) int8, scale_others (WS - 1, M) T"""
    _chk_cuda(my, q_others, scale_others)
    groups, world = my.numel() // 32, q_others.shape[0] + 1
    q = torch.empty(my.shape, dtype=torch.int8, device=my.device)
    s = torch.empty(groups, dtype=my.dtype, device=my.device)
    check(lib().zl_dequant_sum_quant_g32(_p(my), _p(q_others), _p(scale_others), _p(q), _p(s), _i(groups), C.c_int(world),
                                         C.c_int(_dt(my)), _stream()), "dequant_sum_quant_g32")
    return q, s


def dequant_group_32(q, scale, out=None):
    _chk_cuda(q, scale)
    if out is None:
        out = torch.empty(q.shape, dtype=scale.dtype, device=q.device)
    check(lib().zl_dequant_group_32(_p(q), _p(scale), _p(out), _i(q.numel() // 32), C.c_int(_dt(scale)), _stream()), "dequant_group_32")
    return out


# ---- W4A8 with FP8 activations (gptq_gemm_k_major, W4_FP8_ALGO: q_gemm_k_major.cu:1003-1035; fp8_util.cu)
def fp8_calc_scale(x, max_e4m3=448.0):
    """nn::fp8::calc_scale: a (1,) fp32 DEVICE tensor max|x| / max_e4m3"""
    _chk_cuda(x)
    s = torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().zl_fp8_calc_scale(_p(x), _i(x.numel()), _f(max_e4m3), _p(s), C.c_int(_dt(x)), _stream()), "fp8_calc_scale")
    return s


def fp8_cvt_half(x, scale):
    """E4M3FN codes (uint8) of T(x) * T(1 / scale), round to nearest even, saturating (T_KERNEL_cvt_half_fp8)"""
    _chk_cuda(x, scale)
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib().zl_fp8_cvt_half(_p(x), _p(scale), _p(out), _i(x.numel()), C.c_int(_dt(x)), _stream()), "fp8_cvt_half")
    return out


def fp8_dynamic_scaled_quant(x, max_e4m3=448.0):
    """nn::fp8::dynamic_scaled_quant: (codes, scale)"""
    s = fp8_calc_scale(x, max_e4m3)
    return fp8_cvt_half(x, s), s


def w4a8_weight_to_fp8(w16, max_weight_e4m3=256.0):
    """Int4GPTQ::calc_w4a8_scale (W4_FP8_ALGO) + dequant_k_major(out_type 2): W16 (N, K) fp16 -> (w8 E4M3 codes, scale (1,) fp32)"""
    return fp8_dynamic_scaled_quant(w16, max_weight_e4m3)


def fp8_gemm_nt(a8, b8, scale_a, scale_b, out=None):
    _chk_cuda(a8, b8, scale_a, scale_b)
    m, k = a8.shape
    n = b8.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float16, device=a8.device)
    check(lib().zl_fp8_gemm_nt(_p(a8), _p(b8), _p(scale_a), _p(scale_b), _p(out), _i(m), _i(n), _i(k), _stream()), "fp8_gemm_nt")
    return out


def w4a8_fp8_linear(x, w8, w_scale, max_act_e4m3=448.0, out=None):
    """gptq_gemm_k_major's W4_FP8 branch: per-tensor dynamic E4M3 quantisation of the activations, fp8 x fp8 GEMM, scales folded
    into the fp32 accumulators, one rounding to fp16"""
    a8, sa = fp8_dynamic_scaled_quant(x, max_act_e4m3)
    return fp8_gemm_nt(a8, w8, sa, w_scale, out=out)


# ---- f4, first part: FP8 128x128-block linear (config 5) and the MoE router ----------------------------------------------
def fp8_per_token_cast(x, scale_col_major=True, max_e4m3=448.0):
    """nn::fp8::per_token_cast_to_fp8: (codes (m, n) uint8, scales fp32 (n/128, aligned_m) column-major -- what fp8_block_gemm
    reads -- or (aligned_m, n/128)); aligned_m = round_up(m, 4) like the reference's TMA alignment"""
    if not (x.is_cuda and x.dim() == 2 and x.stride(1) == 1):        # rows may be strided (Fp8Block::support_uncontinuous_input)
        raise ZLError("FP8 block_scale: input is not a 2D CUDA tensor with dense rows")
    if x.shape[1] % 128:
        raise ZLError("FP8 block_scale: input.size(1) can't divide 128")
    m, n = x.shape
    am = (m + 3) // 4 * 4
    out = torch.empty((m, n), dtype=torch.uint8, device=x.device)
    sc = torch.zeros((n // 128, am) if scale_col_major else (am, n // 128), dtype=torch.float32, device=x.device)
    check(lib().zl_fp8_per_token_cast(_p(x), _i(x.stride(0)), _p(out), _i(n), _p(sc), _i(am), _i(m), _i(n), C.c_int(int(scale_col_major)),
                                      _f(max_e4m3), C.c_int(_dt(x)), _stream()), "fp8_per_token_cast")
    return out, sc


def fp8_block_dequant(w8, scale, dtype=torch.bfloat16):
    """nn::fp8::dequant_fp8_block_weight: (N, K) codes x (ceil(N/128), ceil(K/128)) fp32 -> (N, K) T"""
    _chk_cuda(w8, scale)
    out = torch.empty(w8.shape, dtype=dtype, device=w8.device)
    check(lib().zl_fp8_block_dequant(_p(w8), _p(scale), _p(out), _i(w8.shape[0]), _i(w8.shape[1]), _i(scale.shape[1]),
                                     C.c_int(0 if dtype == torch.float16 else 1), _stream()), "fp8_block_dequant")
    return out


class Fp8BlockMWeight:
    """The e4m3 codes of a block-scaled weight -- (N, K) or (G, N, K) -- in the ZLF8M layout (zl_fp8_block_pack): fragment loads of
    1 KiB contiguous.  Pass it as `w8` to fp8_block_gemm / fp8_block_linear (up to 32 rows per launch, or the grouped form)."""

    def __init__(self, w8):
        _chk_cuda(w8)
        if w8.dtype != torch.uint8 or w8.dim() not in (2, 3):
            raise ZLError("Fp8BlockMWeight: (N, K) or (G, N, K) uint8 codes")
        self.groups = w8.shape[0] if w8.dim() == 3 else 1
        self.n, self.k = w8.shape[-2], w8.shape[-1]
        nbytes = int(lib().zl_fp8_block_packed_bytes(_i(self.n), _i(self.k), _i(self.groups)))
        if nbytes < 0:
            check(nbytes, "fp8_block_packed_bytes")
        self.data = torch.empty(nbytes, dtype=torch.uint8, device=w8.device)
        w = w8 if w8.is_contiguous() else w8.contiguous()
        check(lib().zl_fp8_block_pack(_p(w), _p(self.data), _i(self.n), _i(self.k), _i(self.groups), _stream()), "fp8_block_pack")


def fp8_block_gemm(a8, a_scale, w8, w_scale, m_indices=None, dtype=torch.bfloat16, out=None):
    """deep_gemm_fp8_block_h20_group: a8 (m, k) codes with column-major scales (k/128, aligned_m); w8 (n, k) or (G, n, k) codes
    with scales (ceil(n/128), k/128) or (G, ...); m_indices (m,) int32 = the expert of every row (grouped form)"""
    if isinstance(w8, Fp8BlockMWeight):
        _chk_cuda(a8, a_scale, w_scale, m_indices)
        m, k = a8.shape
        if out is None:
            out = torch.zeros((m, w8.n), dtype=dtype, device=a8.device)
        check(lib().zl_fp8_block_gemm_group_packed(_p(a8), _p(a_scale), _i(a_scale.shape[1]), _p(w8.data), _p(w_scale), _p(m_indices), _p(out), _i(m),
                                                   _i(w8.n), _i(k), C.c_int(w8.groups), C.c_int(0 if out.dtype == torch.float16 else 1), _stream()),
              "fp8_block_gemm_packed")
        return out
    _chk_cuda(a8, a_scale, w8, w_scale, m_indices)
    m, k = a8.shape
    n = w8.shape[-2]
    groups = w8.shape[0] if w8.dim() == 3 else 1
    if out is None:
        out = torch.zeros((m, n), dtype=dtype, device=a8.device)
    check(lib().zl_fp8_block_gemm_group(_p(a8), _p(a_scale), _i(a_scale.shape[1]), _p(w8), _p(w_scale), _p(m_indices), _p(out), _i(m), _i(n),
                                        _i(k), C.c_int(groups), C.c_int(0 if out.dtype == torch.float16 else 1), _stream()), "fp8_block_gemm")
    return out


def fp8_block_linear(x, w8, w_scale, out=None):
    """Fp8Block::forward (linear.cpp:1863-1905): per-token 1x128 activation quantisation + the block-scaled GEMM"""
    a8, sa = fp8_per_token_cast(x)
    return fp8_block_gemm(a8, sa, w8, w_scale, dtype=x.dtype, out=out)


_SCORING = {"": 1, "softmax": 1, "sigmoid": 2, "linear": 3}


def moe_top_k_softmax(logits, top_k, top_k_ext=None, norm_topk_prob=False, weight_scale=1.0, scoring_func="softmax", worker_load=None,
                      expert_load=None, num_worker=1):
    """nn::top_k_softmax: (weights fp32 (tokens, top_k_ext), expert ids int32 (tokens, top_k_ext))"""
    _chk_cuda(logits, worker_load, expert_load)
    t, e = logits.shape
    ext = top_k_ext or top_k
    v = torch.empty((t, ext), dtype=torch.float32, device=logits.device)
    idx = torch.zeros((t, ext), dtype=torch.int32, device=logits.device)
    check(lib().zl_moe_top_k_softmax(_p(logits), _i(t), C.c_int(e), C.c_int(top_k), C.c_int(ext), C.c_int(int(norm_topk_prob)), _f(weight_scale),
                                     C.c_int(_SCORING[scoring_func]), C.c_int(_dt_logits(logits)), _p(v), _p(idx), _p(worker_load), _p(expert_load),
                                     C.c_int(num_worker), _stream()), "moe_top_k_softmax")
    return v, idx


def moe_group_topk(logits, score_correction_bias, num_group, topk_group, top_k, top_k_ext=None, norm_topk_prob=True, weight_scale=1.0,
                   scoring_func="sigmoid", worker_load=None, expert_load=None, num_worker=1):
    """nn::group_topk_softmax (DeepSeek-V3 group-limited routing)"""
    _chk_cuda(logits, score_correction_bias, worker_load, expert_load)
    t, e = logits.shape
    ext = top_k_ext or top_k
    v = torch.empty((t, ext), dtype=torch.float32, device=logits.device)
    idx = torch.zeros((t, ext), dtype=torch.int32, device=logits.device)
    check(lib().zl_moe_group_topk(_p(logits), _p(score_correction_bias), _i(t), C.c_int(e), C.c_int(top_k), C.c_int(ext), C.c_int(int(norm_topk_prob)),
                                  _f(weight_scale), C.c_int(_SCORING[scoring_func]), C.c_int(num_group), C.c_int(topk_group), C.c_int(_dt_logits(logits)),
                                  _p(v), _p(idx), _p(worker_load), _p(expert_load), C.c_int(num_worker), _stream()), "moe_group_topk")
    return v, idx


# ---- f4: MoE dispatch / combine of the prompt path (ff_kernel.h:42-96) ----------------------------------------------------------
def moe_sum_experts(inp, index, weights):
    """nn::sum_experts, one concatenated input (seq_len * K, dim_model)"""
    _chk_cuda(inp, index, weights)
    seq, k = weights.shape
    out = torch.empty((seq, inp.shape[1]), dtype=inp.dtype, device=inp.device)
    check(lib().zl_moe_sum_experts(_p(inp), _p(index), _p(weights), _p(out), _i(seq), C.c_int(k), _i(inp.shape[1]), C.c_int(_dt(inp)), _stream()),
          "sum_experts")
    return out


def moe_sum_experts_arr(inputs, experts, index, weights, exp_parallel=False, world_size=1, local_rank=0):
    """nn::sum_experts, one (rows, dim_model) input per expert (None / empty where an expert got no token)"""
    live = [t for t in inputs if t is not None and t.numel()]
    if not live:
        raise ZLError("all inputs is empty")
    _chk_cuda(experts, index, weights, *live)
    dev, dim = live[0].device, live[0].shape[-1]
    ptrs = torch.tensor([0 if (t is None or not t.numel()) else t.data_ptr() for t in inputs], dtype=torch.int64).to(dev)
    seq, k = weights.shape
    out = torch.empty((seq, dim), dtype=live[0].dtype, device=dev)
    check(lib().zl_moe_sum_experts_arr(_p(ptrs), _p(experts), _p(index), _p(weights), _p(out), _i(seq), C.c_int(k), _i(dim), C.c_int(int(exp_parallel)),
                                       C.c_int(world_size), C.c_int(local_rank), C.c_int(_dt(live[0])), _stream()), "sum_experts")
    return out


def moe_route_shared_lb(exp_ids, exp_weights, worker_load, expert_load, top_k, num_local_experts):
    """nn::route_shared_lb: fills exp_ids[:, top_k:] in place, bumps the two load counters"""
    _chk_cuda(exp_ids, exp_weights, worker_load, expert_load)
    if exp_ids.shape != exp_weights.shape or exp_ids.dtype != torch.int32:
        raise ZLError("shape mismatch")
    seq, ext = exp_ids.shape
    ws = worker_load.numel()
    max_load = (exp_ids.numel() + ws - 1) // ws
    base = worker_load.clone()
    check(lib().zl_moe_route_shared_lb(_p(exp_ids), _p(base), _p(worker_load), _p(expert_load), C.c_int(max_load), C.c_int(ws), _i(seq), C.c_int(top_k),
                                       C.c_int(ext), C.c_int(num_local_experts), _stream()), "route_shared_lb")


def moe_plus_for_sort(exp_ids, num_experts, world_size):
    _chk_cuda(exp_ids)
    if num_experts % world_size:
        raise ZLError("num_experts can't divide world_size")
    out = torch.empty_like(exp_ids)
    check(lib().zl_moe_plus_for_sort(_p(exp_ids), _p(out), C.c_int(num_experts), C.c_int(world_size), _i(exp_ids.numel()), _stream()), "plus_for_sort")
    return out


def moe_calc_reverse_idx(exp_ids, indices, all_loads, num_experts, world_size=1, sorted_by_rank=False):
    """nn::calc_reverse_idx: all_loads = the host copy of [expert loads (num_experts) | rank loads (world_size)]"""
    _chk_cuda(exp_ids, indices)
    off = [0] * num_experts
    if sorted_by_rank:
        rank_offset = 0
        for rank in range(world_size):
            o = 0
            for i in range(rank, num_experts, world_size):
                off[i] = rank_offset + o
                o += int(all_loads[i])
            rank_offset += int(all_loads[num_experts + rank])
    else:
        o = 0
        for i in range(num_experts):
            off[i] = o
            o += int(all_loads[i])
    off_t = torch.tensor(off, dtype=torch.int32).to(exp_ids.device)
    rev = torch.empty_like(indices)
    check(lib().zl_moe_calc_reverse_idx(_p(exp_ids), _p(indices), _p(off_t), _p(rev), _i(indices.numel()), _stream()), "calc_reverse_idx")
    return rev


def moe_fill_m_indices_padded_indices(all_loads, block_m, num_experts, device, exp_parallel=False, rank=0, world_size=1):
    """nn::fill_m_indices_padded_indices: (m_indices, padded_indices, total_tokens_aligned)"""
    r, ws = (rank, world_size) if exp_parallel else (0, 1)
    nt = [int(all_loads[j]) for j in range(r, num_experts, ws)]
    offs, aoffs, o, a = [], [], 0, 0
    for n in nt:
        offs.append(o)
        aoffs.append(a)
        o += n
        a += (n + block_m - 1) // block_m * block_m
    aoffs.append(a)
    if a == 0:
        return None, None, 0
    # one device tensor for the three small tables (kept alive in a local: temporaries would be freed -- and their block handed to
    # the next one -- before the launch is even issued)
    tab = torch.tensor(nt + offs + aoffs, dtype=torch.int32).to(device)
    n = len(nt)
    pad = torch.empty(max(o, 1), dtype=torch.int32, device=device)[:o]
    mi = torch.empty(a, dtype=torch.int32, device=device)
    check(lib().zl_moe_fill_m_indices(_p(tab[:n]), _p(tab[n:2 * n]), _p(tab[2 * n:]), _p(pad) if o else _p(mi), _p(mi), C.c_int(n), C.c_int(max(nt)),
                                      C.c_int(block_m), _stream()), "fill_m_indices_padded_indices")
    return mi, pad, a


# ---- f4: MLA decode attention over the latent cache ------------------------------------------------------------------------------
def mla_decode_attention(q_adj, buf_lens, kv_buf_addrs, scale, max_len_buf, valid_lens=None, kv_lora_rank=512, rope_dim=64, workspace=None,
                         algo=0):
    """MLAImpl over the compressed cache for decode rows: q_adj (B, H, 576), kv_buf_addrs (B,) int64 device table of (len_buf, 576)
    buffers -> (B, H, 512).  algo 0: the matrix-core kernel, 1: the VALU kernel (zl_mla_decode_attn_ex)."""
    _chk_cuda(q_adj, buf_lens, kv_buf_addrs, valid_lens)
    b, h, cd = q_adj.shape
    if cd != kv_lora_rank + rope_dim:
        raise ZLError("q_adj: last dimension is kv_lora_rank + rope_dim")
    if workspace is None:
        workspace = torch.empty(int(lib().zl_mla_decode_workspace_bytes(_i(b), _i(h), _i(max_len_buf))), dtype=torch.uint8, device=q_adj.device)
    out = torch.empty((b, h, kv_lora_rank), dtype=q_adj.dtype, device=q_adj.device)
    check(lib().zl_mla_decode_attn_ex(_p(q_adj), _p(buf_lens), _p(valid_lens), _p(kv_buf_addrs), _p(out), _p(workspace), _i(b), _i(h),
                                      _i(kv_lora_rank), _i(rope_dim), _f(scale), _i(max_len_buf), C.c_int(_dt(q_adj)), C.c_int(algo), _stream()),
          "mla_decode_attention")
    return out


def mha_fwd_kvcache_mla(q, kcache, head_size_v, seqlens_k, block_table, softmax_scale, is_causal=False, out=None):
    """ds::mha_fwd_kvcache_mla (ds_flash_mla_api.h:16-30): q (B, len_q, H, 576), kcache (num_blocks, page, 1, 576), seqlens_k (B,) int32,
    block_table (B, max_blocks) int32 -> (out (B, len_q, H, 512), softmax_lse (B, 1, len_q * H) fp32).  Non-causal only (len_q == 1 or
    is_causal False), as every reference call site is."""
    _chk_cuda(q, kcache, seqlens_k, block_table)
    b, len_q, h, cd = q.shape
    if len_q > 1 and is_causal:
        raise ZLError("mha_fwd_kvcache_mla: causal multi-row queries are not on this path")
    if kcache.dim() != 4 or kcache.shape[2] != 1 or kcache.shape[3] != cd or not kcache.is_contiguous() or not q.is_contiguous():
        raise ZLError("mha_fwd_kvcache_mla: kcache is (num_blocks, page_block_size, 1, head_size), contiguous like q")
    if block_table.dim() != 2 or block_table.shape[0] != b or block_table.dtype != torch.int32 or seqlens_k.dtype != torch.int32:
        raise ZLError("mha_fwd_kvcache_mla: block_table (B, max_blocks) int32, seqlens_k (B,) int32")
    page, mb, hh = kcache.shape[1], block_table.shape[1], len_q * h
    workspace = torch.empty(int(lib().zl_mla_decode_workspace_bytes(_i(b), _i(hh), _i(page * mb))), dtype=torch.uint8, device=q.device)
    if out is None:
        out = torch.empty((b, len_q, h, head_size_v), dtype=q.dtype, device=q.device)
    lse = torch.empty((b, 1, hh), dtype=torch.float32, device=q.device)
    block_table = block_table.contiguous()
    check(lib().zl_mla_decode_attn_paged(_p(q), _p(kcache), _p(block_table), _p(seqlens_k), _p(out), _p(lse), _p(workspace), _i(b), _i(hh),
                                         _i(head_size_v), _i(cd - head_size_v), _i(page), _i(mb), _f(softmax_scale), C.c_int(_dt(q)), _stream()),
          "mha_fwd_kvcache_mla")
    return out, lse


# --------------------------------------------------------------------------------------------------
# MXFP4: OCP microscaled FP4 weights (include/zhilight_amd.h "MXFP4"; csrc/mxfp4.hip).  Quant type 11 of this project.
# --------------------------------------------------------------------------------------------------
MXFP4_GEMV, MXFP4_STREAM, MXFP4_TILED = 1, 2, 3
MXFP4_BLOCK = 32
_E2M1_MIDS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)       # between codes i and i + 1 of {0, .5, 1, 1.5, 2, 3, 4, 6}


def mxfp4_quantize(w):
    """A float (N, K) tensor (K % 32 == 0, any device) -> (codes uint8 (N, K/2), scales uint8 (N, K/32)) under the OCP MX rule:
    a block's exponent is floor(log2(amax)) - 2 (E2M1's largest exponent), an all-zero block gets scale byte 0; elements are
    rounded to the nearest E2M1 value, ties to the even code, and saturate at +-6.  Plain torch, float64: a tool for tests,
    init_random and the benchmarks, not a hot path."""
    if w.dim() != 2 or w.shape[1] % MXFP4_BLOCK != 0:
        raise ZLError("mxfp4_quantize: (N, K) with K % 32 == 0")
    n, k = w.shape
    blocks = w.detach().to(torch.float64).reshape(n, k // MXFP4_BLOCK, MXFP4_BLOCK)
    if not bool(torch.isfinite(blocks).all()):
        raise ZLError("mxfp4_quantize: non-finite weights")
    amax = blocks.abs().amax(dim=2)
    _, ex = torch.frexp(amax)                               # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    byte = torch.where(amax > 0, (ex.to(torch.int64) - 3 + 127).clamp(0, 254), torch.zeros_like(ex, dtype=torch.int64))
    a = torch.ldexp(blocks.abs(), (127 - byte).unsqueeze(2).to(torch.int32))
    code = torch.zeros_like(a, dtype=torch.int64)
    for i, mid in enumerate(_E2M1_MIDS):                    # a tie goes to the even one of codes i, i + 1
        code += (a >= mid) if i % 2 else (a > mid)
    code = torch.where((blocks < 0) & (code > 0), code + 8, code).reshape(n, k).to(torch.uint8)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous(), byte.to(torch.uint8).contiguous()


class Mxfp4Weight:
    """An MXFP4 matrix on the device as the kernels read it -- the checkpoint's own layout: codes uint8 (N, K/2), scales uint8
    (N, K/32); 0.53125 B per weight, no packed copy.  row_interleave stores source row (i % 2) * (N / 2) + i / 2 at row i, so
    that a vertically concatenated [gate; up] matrix becomes (gate_j, up_j) row pairs for the silu*mul epilogue."""

    def __init__(self, codes, scales, row_interleave=False):
        self.codes, self.scales, self.row_interleave = codes, scales, bool(row_interleave)
        self.n, self.k = codes.shape[0], codes.shape[1] * 2

    @classmethod
    def from_checkpoint(cls, codes, scales, row_interleave=False):
        """codes (N, K/2) or (N, K/32, 16) uint8, scales (N, K/32) uint8, CUDA tensors.  Refuses a scale byte 255 (the format's NaN)
        with one host-side check."""
        if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or not (codes.is_cuda and scales.is_cuda):
            raise ZLError("Mxfp4Weight: codes and scales are uint8 CUDA tensors")
        if codes.dim() == 3:
            codes = codes.reshape(codes.shape[0], -1)
        if (codes.dim() != 2 or scales.dim() != 2 or codes.shape[1] % 16 != 0 or scales.shape[0] != codes.shape[0]
                or scales.shape[1] * 16 != codes.shape[1]):
            raise ZLError(f"Mxfp4Weight: codes {tuple(codes.shape)} / scales {tuple(scales.shape)} are not (N, K/2) / (N, K/32)")
        if bool((scales == 255).any()):
            raise ZLError("Mxfp4Weight: scale byte 255 (the E8M0 NaN) in the checkpoint")
        if row_interleave:
            n = codes.shape[0]
            if n % 2:
                raise ZLError("Mxfp4Weight: row_interleave needs an even row count")
            idx = torch.arange(n, device=codes.device).view(2, n // 2).t().reshape(-1)
            codes, scales = codes[idx], scales[idx]
        return cls(codes.contiguous(), scales.contiguous(), row_interleave)

    @classmethod
    def random(cls, n, k, device, gen=None, std=0.05, row_interleave=False):
        codes, scales = mxfp4_quantize(torch.randn(n, k, device=device, generator=gen) * std)
        return cls.from_checkpoint(codes, scales, row_interleave)

    def nbytes(self):
        return self.codes.numel() + self.scales.numel()

    def dequantize(self, dtype=torch.float16):
        return mxfp4_dequantize(self.codes, self.scales, dtype)


def mxfp4_route(m, n, k):
    """which kernel mxfp4_linear launches for (m, n, k): MXFP4_GEMV (1..4 rows), MXFP4_STREAM (5..32), MXFP4_TILED (more)"""
    r = int(lib().zl_mxfp4_route(_i(m), _i(n), _i(k)))
    if r < 0:
        check(r, "mxfp4_route")
    return r


def mxfp4_dequantize(codes, scales, dtype=torch.float16, out=None):
    """W (N, K) in fp16 / bf16, rounded once (exact in bf16, in fp16 for 2^-23 .. 2^13 scales): tests and debugging"""
    _chk_cuda(codes, scales)
    n, k = codes.shape[0], codes.shape[1] * 2
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or tuple(scales.shape) != (n, k // 32) or k % 32:
        raise ZLError("mxfp4_dequantize: codes uint8 (N, K/2), scales uint8 (N, K/32)")
    if out is None:
        out = torch.empty((n, k), dtype=dtype, device=codes.device)
    else:
        _chk_out(out, n, k, dtype, codes.device, "mxfp4_dequantize")
    check(lib().zl_mxfp4_dequant(_p(codes), _p(scales), _p(out), _i(n), _i(k), C.c_int(_dt(out)), _stream()), "mxfp4_dequantize")
    return out


def mxfp4_linear(x, w: Mxfp4Weight, bias=None, residual=None, out=None, epilogue=0):
    """y = T(x . W^T [+ bias]) on an Mxfp4Weight, T = x.dtype (fp16 / bf16), fp32 accumulation, no rounding of a weight.
    bias adds EPI_BIAS, residual EPI_RESIDUAL (y = T(residual + T(acc + bias)); out may alias it); EPI_SILU_MUL on a
    row-interleaved [gate; up] weight writes N / 2 columns.  x: (.., K) with unit element stride; a 2-D x may have a row
    stride > K (% 8 == 0)."""
    _chk_cuda(bias, residual)
    if not x.is_cuda or x.stride(-1) != 1:
        raise ZLError("mxfp4_linear: x must be a CUDA tensor with contiguous rows")
    x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
    m, k = x2.shape
    if k != w.k:
        raise ZLError("size K mismatch")
    if m > 1 and x2.stride(0) < k:
        raise ZLError("mxfp4_linear: overlapping rows")
    silu = epilogue & EPI_SILU_MUL
    if silu and not w.row_interleave:
        raise ZLError("mxfp4_linear: EPI_SILU_MUL needs a row-interleaved [gate; up] weight")
    n_out = w.n // 2 if silu else w.n
    for t, what in ((bias, "bias"), (residual, "residual")):
        if t is not None and (t.dtype != x.dtype or t.device != x.device):
            raise ZLError(f"mxfp4_linear: {what} dtype / device")
    if bias is not None:
        if bias.numel() != w.n:
            raise ZLError("mxfp4_linear: bias size")
        epilogue |= EPI_BIAS
    if residual is not None:
        if residual.numel() != m * n_out:
            raise ZLError("mxfp4_linear: residual size")
        epilogue |= EPI_RESIDUAL
    if out is None:
        out = torch.empty((m, n_out), dtype=x.dtype, device=x.device)
    else:
        _chk_out(out, m, n_out, x.dtype, x.device, "mxfp4_linear")
    ldx = x2.stride(0) if m > 1 else k
    check(lib().zl_mxfp4_linear(_p(x2), _i(ldx), _p(w.codes), _p(w.scales), _p(bias), _p(residual), _p(out), _i(m), _i(w.n), _i(k),
                                C.c_int(_dt(x)), C.c_int(epilogue), _stream()), "mxfp4_linear")
    return out
