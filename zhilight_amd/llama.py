"""Host-side mirror of the reference's decode ("search") path for LLaMA-like models:
`model::LLaMA::encode` -> N x `nn::EncoderLayer::forward` -> `get_logits`
(src/model/llama.cpp:75-165, src/nn/block/block.cpp:86-143, src/nn/attention/attention.cpp:846-964,
src/nn/feedforward/feedforward.cpp:113-137), with the per-step device state of
`model::DynBatchContext` / `RagBufferContext` (src/model/dyn_batch_context.h:29-200,
src/model/rag_buffer_context.h:141-188).

Only what the decode hot path needs lives here: weight containers, the per-task ragged KV buffers
with their device pointer tables, and the kernel sequence of one step.  PyTorch supplies device
memory and the stream; every arithmetic step is one C-ABI launcher from `ops`.

Kernel sequence per layer (6 launches; the reference issues ~14 for the same math):
  1. w4a16_gemm  [RMSNorm(ln_attn) prologue]  hidden -> fused q|k|v             (project_q/k/v)
  2. decode_attn_fused: rotate q,k (cached cos/sin), k,v -> ragged KV, split-KV softmax(q.K^T).V
  3. combine of the KV splits
  4. w4a16_gemm  [residual epilogue]           attn_out + hidden -> hidden       (attn_out + add)
  5. w4a16_gemm  [RMSNorm(ln_ff) prologue, silu*mul epilogue]  -> act           (w_in, w_gated, gate_mul)
  6. w4a16_gemm  [residual epilogue]           w_out + hidden -> hidden
The roundings are the reference's single-stream path: every linear output, the norm output, the
rotated q/k, the attention output and each residual sum is rounded to fp16 exactly where the
reference materialises an fp16 tensor.
"""
import collections
import math
import os
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops
from . import parallel


@dataclass
class ModelConfig:
    """Subset of model::ModelConfig (src/model/model_config.hpp:27-130) used on this path; key names
    follow `pydict_to_model_config` (src/py_export/py_model_config.cpp:77-151)."""
    num_layers: int = 32
    dim_model: int = 4096
    num_heads: int = 32
    dim_head: int = 128
    dim_ff: int = 14336
    vocab_size: int = 128256
    num_kv_heads: int = 8
    eps: float = 1e-5
    rope_theta: float = 500000.0
    rope_scaling: Optional[dict] = None     # {"rope_type": "llama3", "factor":8, "low_freq_factor":1, ...}
    activate_fn: str = "silu"
    scale_emb: float = 1.0
    dim_model_base: int = 0                 # MiniCPM: logits scale = dim_model_base / dim_model
    scale_depth: float = -1.0               # MiniCPM residual scale scale_depth / sqrt(num_layers)
    tie_lm_head: bool = False
    qk_norm: Optional[str] = None           # "head": Qwen3 q_norm / k_norm (dim_head weight); "multi_head": use_qk_norm
    max_position_embeddings: int = 0        # dynamic-NTK rope threshold
    model_type: str = "llama"
    dtype: str = "half"                     # "half" | "bfloat16" (unquantised models; the W4 / int8 routes are fp16)
    # mixture of experts (Qwen3-MoE: zhilight/config/qwen3_adapter.py; HF keys num_experts, num_experts_per_tok, ...); 0 experts = dense
    moe_num_experts: int = 0
    moe_top_k: int = 0
    moe_intermediate_size: int = 0
    norm_topk_prob: bool = False
    decoder_sparse_step: int = 1            # layer i is sparse when (i + 1) % step == 0 and i is not in mlp_only_layers
    mlp_only_layers: List[int] = field(default_factory=list)

    def is_moe_layer(self, i: int) -> bool:
        """Qwen3MoeDecoderLayer's rule: an MoE feed-forward unless the layer is listed as dense or off the sparse step"""
        return (self.moe_num_experts > 0 and i not in self.mlp_only_layers and self.decoder_sparse_step > 0
                and (i + 1) % self.decoder_sparse_step == 0)

    @property
    def torch_dtype(self):
        return torch.bfloat16 if self.dtype in ("bfloat16", "bf16") else torch.float16

    @property
    def residual_scale(self):
        """EncoderLayer scale (src/nn/block/block.cpp:55-58): MiniCPM ("cpm_dragonfly") adds scale_depth/sqrt(L)
        times the sub-layer output to the residual; everything else a plain sum."""
        return (self.scale_depth / math.sqrt(self.num_layers)) if self.scale_depth > 0 else 1.0

    @classmethod
    def from_hf(cls, cfg: dict):
        """HF config.json -> ModelConfig (zhilight/config/adapter.py + py_model_config.cpp key names)."""
        hidden, heads = cfg["hidden_size"], cfg["num_attention_heads"]
        return cls(
            num_layers=cfg["num_hidden_layers"], dim_model=hidden, num_heads=heads,
            dim_head=cfg.get("head_dim", hidden // heads), dim_ff=cfg["intermediate_size"],
            vocab_size=cfg["vocab_size"], num_kv_heads=cfg.get("num_key_value_heads", heads),
            eps=cfg.get("rms_norm_eps", 1e-5), rope_theta=cfg.get("rope_theta", 10000.0),
            rope_scaling=cfg.get("rope_scaling"), activate_fn=cfg.get("hidden_act", "silu"),
            scale_emb=cfg.get("scale_emb", 1.0), dim_model_base=cfg.get("dim_model_base", 0),
            scale_depth=cfg.get("scale_depth", -1.0), tie_lm_head=cfg.get("tie_word_embeddings", False),
            qk_norm=("head" if cfg.get("model_type") in ("qwen3", "qwen3_moe") else
                     "multi_head" if cfg.get("use_qk_norm") else None),     # attention.cpp:110-117
            max_position_embeddings=cfg.get("max_position_embeddings", 0), model_type=cfg.get("model_type", "llama"),
            dtype={"bfloat16": "bfloat16", "float16": "half"}.get(cfg.get("torch_dtype", "float16"), "half"),
            moe_num_experts=int(cfg.get("num_experts", 0) or 0), moe_top_k=int(cfg.get("num_experts_per_tok", 0) or 0),
            moe_intermediate_size=int(cfg.get("moe_intermediate_size", 0) or 0), norm_topk_prob=bool(cfg.get("norm_topk_prob", False)),
            decoder_sparse_step=int(cfg.get("decoder_sparse_step", 1) or 1), mlp_only_layers=list(cfg.get("mlp_only_layers", []) or []))

    @classmethod
    def llama3_8b(cls):
        return cls()

    @classmethod
    def minicpm_2b(cls):
        """openbmb/MiniCPM-2B-sft-bf16 (BASELINE configs[0]): "cpm_dragonfly" scalings, tied lm_head, D = 64."""
        return cls(num_layers=40, dim_model=2304, num_heads=36, dim_head=64, dim_ff=5760, vocab_size=122753, num_kv_heads=36,
                   eps=1e-5, rope_theta=10000.0, scale_emb=12.0, dim_model_base=256, scale_depth=1.4, tie_lm_head=True,
                   dtype="bfloat16")


MXFP4 = 11      # QuantConfig.quant_type of OCP MXFP4 checkpoints (the reference's QuantType enum ends at 10)


@dataclass
class QuantConfig:
    """model::QuantConfig (src/model/model_config.hpp:132-177); quant_type 5 = GPTQ W4A16 k-major.
    `awq` marks an AWQ checkpoint taken through the reference's AWQ_USE_EXLLAMA route
    (Int4GPTQ with is_awq, src/nn/linear/linear.cpp:694-698, 1139-1143): the tensors are converted to the
    same k-major operands at load, the kernels are the GPTQ ones.
    quant_type 11 = MXFP4 (OCP microscaled FP4 weights, group_size 32; outside the reference's enum 0-10): Mxfp4EncoderLayer."""
    quant_type: int = 5
    group_size: int = 128
    sym: bool = False
    act_order: bool = False
    awq: bool = False

    @classmethod
    def from_hf(cls, qc: dict):
        """QuantConfig.adapt_hf_config (zhilight/quant.py:35-88): gptq -> type 5; awq -> type 5 with the AWQ
        load transform (what the reference does under AWQ_USE_EXLLAMA=1, its faster decode route)."""
        method = qc.get("quant_method", "gptq")
        if method == "mxfp4":
            # transformers' Mxfp4Config: E2M1 codes + E8M0 scales per 32 elements, nothing else to configure
            return cls(MXFP4, 32, True, False, False)
        if method == "quark":
            return cls._from_quark(qc)
        if method not in ("gptq", "awq"):
            raise ops.ZLError(f"Unsupported quant_method {method}")
        if qc.get("bits", 4) != 4:
            raise ops.ZLError("Only bits=4 is supported")
        if qc.get("is_marlin_format", False):
            raise ops.ZLError(f"Unsupported Marlin {method}")
        act_order = bool(qc.get("desc_act", False))
        if method == "awq":
            if not qc.get("zero_point", True):
                raise ops.ZLError("AWQ checkpoints without zero points are not supported")
            return cls(5, qc.get("group_size", 128), False, False, True)
        return cls(5, qc.get("group_size", 128), qc.get("sym", False), act_order, False)

    @classmethod
    def _from_quark(cls, qc: dict):
        """AMD Quark exports (quant_method "quark"): accepted only when the global weight spec is MXFP4 -- dtype fp4, per-group
        along the input axis, group size 32, E8M0 (power-of-two) scales.  Every other Quark scheme is refused by name.  An
        activation spec (`input_tensors`, e.g. the fp4 activations of a W4A4 export) is IGNORED: the model is executed weight-only,
        activations stay fp16 / bf16.  Per-layer overrides (`layer_quant_config`, `layer_type_quant_config`) other than empty are
        refused: one format for every linear."""
        g = qc.get("global_quant_config") or {}
        w = g.get("weight")
        if isinstance(w, (list, tuple)):
            w = w[0] if len(w) == 1 else None
        if not isinstance(w, dict):
            raise ops.ZLError("Unsupported Quark config: no single global weight spec")
        dtype, scheme = str(w.get("dtype", "")).lower(), str(w.get("qscheme", "")).lower()
        scale_fmt = str(w.get("scale_format", w.get("scale_type", ""))).lower()
        what = f"Quark dtype={dtype or '?'} qscheme={scheme or '?'} group_size={w.get('group_size')} scale_format={scale_fmt or '?'}"
        if dtype not in ("fp4", "mxfp4", "fp4_e2m1") or scheme != "per_group" or w.get("group_size") != 32 or scale_fmt != "e8m0":
            raise ops.ZLError(f"Unsupported {what}: only fp4 / per_group / group_size 32 / e8m0 (MXFP4) is supported")
        if w.get("ch_axis", -1) not in (-1, 1):
            raise ops.ZLError(f"Unsupported {what}: groups must run along the input axis")
        if qc.get("layer_quant_config") or qc.get("layer_type_quant_config"):
            raise ops.ZLError("Unsupported Quark config: per-layer overrides")
        return cls(MXFP4, 32, True, False, False)


def hf_name_to_internal(name: str) -> str:
    """LLaMALoader._replace_name (zhilight/loader.py:250-358), LLaMA/GPTQ subset."""
    s = name
    s = re.sub(r"model\.embed_tokens\.weight", "token_embedding.weight", s)
    s = re.sub(r"model\.norm\.weight", "output_layernorm.weight", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.input_layernorm\.", r"layers.\1.ln_attn.", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.post_attention_layernorm\.weight", r"layers.\1.ln_ff.weight", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.self_attn\.([qkv])_proj\.", r"layers.\1.attn.project_\2.", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.self_attn\.o_proj\.", r"layers.\1.attn.attn_out.", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.self_attn\.([qk])_norm\.", r"layers.\1.attn.\2_norm.", s)
    # MoE experts and router (loader.py:318-326); Qwen2-MoE's shared expert keeps a name of its own (refused at load)
    s = re.sub(r"model\.layers\.([0-9]+)\.mlp\.experts\.([0-9]+)\.gate_proj\.", r"layers.\1.ff.experts.\2.w_in.", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.mlp\.experts\.([0-9]+)\.up_proj\.", r"layers.\1.ff.experts.\2.w_gated.", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.mlp\.experts\.([0-9]+)\.down_proj\.", r"layers.\1.ff.experts.\2.w_out.", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.mlp\.gate\.weight", r"layers.\1.ff.router.weight", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.mlp\.shared_expert(_gate)?\.", r"layers.\1.ff.shared_expert\2.", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.mlp\.gate_proj\.", r"layers.\1.ff.w_in.", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.mlp\.up_proj\.", r"layers.\1.ff.w_gated.", s)
    s = re.sub(r"model\.layers\.([0-9]+)\.mlp\.down_proj\.", r"layers.\1.ff.w_out.", s)
    return "llama." + s


def _dev_t(a, device, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(device).contiguous()
    return t if dtype is None else t.view(dtype)


def w4_algo(quant) -> str:
    """Which W4A16 kernel a quantized linear runs -- the counterpart of the reference's GPTQ_KERNEL_ALGO
    switch (src/nn/quant/gptq/q_gemm_k_major.cu:1075-1100).  "mfma" (default): dequant -> MFMA with fp32
    accumulation, the arithmetic of the reference's dequant+GEMM branch; "exact": the warp-reduce
    kernel replayed bit for bit.  Set ZL_W4_ALGO=exact to select the latter; group sizes the MFMA tile
    cannot hold (not a multiple of 128) use it automatically."""
    algo = os.environ.get("ZL_W4_ALGO", "mfma").lower()
    if algo not in ("mfma", "exact"):
        raise ops.ZLError(f"ZL_W4_ALGO={algo!r}: expected 'mfma' or 'exact'")
    if quant.group_size % 128 != 0:
        return "exact"
    return algo


class Int4GPTQ:
    """nn::Linear with the Int4GPTQ implementation (src/nn/linear/linear.cpp:638-1244): holds the
    load-time-transformed weight; `fuse` mirrors Linear::fuse / fuse3 (row concatenation)."""

    def __init__(self, name, dim_in, dim_out, quant: QuantConfig):
        self.name, self.dim_in, self.dim_out, self.quant = name, dim_in, dim_out, quant
        self.km = None      # k-major (qweight, qzeros, scales) device tensors until packed
        self.weight: Optional[ops.W4Weight] = None
        self.bias = None
        self.perm = None    # act-order: activation column gather applied in forward()

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str, device, out_perm=None, input_prepermuted=False):
        """out_perm: reorder the OUTPUT columns (w_in / w_gated permuted by w_out's input order, the reference's
        permute_ff_up_out, linear.cpp:1168-1186).  input_prepermuted: the producer already delivers the activations in this
        linear's regrouped row order (w_out behind such w_in / w_gated): no gather in forward (linear.cpp:1188-1210)."""
        qw = _dev_t(sd[prefix + ".qweight"], device, torch.int32)
        qz = _dev_t(sd[prefix + ".qzeros"], device, torch.int32)
        sc = _dev_t(sd[prefix + ".scales"], device, torch.float16)
        if out_perm is not None:
            if self.quant.awq:
                raise ops.ZLError("output permutation is a GPTQ act-order transform")
            idx = out_perm.to(torch.int64)
            qw = qw.index_select(1, idx).contiguous()
            sc = sc.index_select(1, idx).contiguous()
            shifts = torch.arange(8, device=qz.device, dtype=torch.int32) * 4
            zn = ((qz.unsqueeze(-1) >> shifts) & 0xF).reshape(qz.shape[0], -1).index_select(1, idx).reshape(qz.shape[0], -1, 8)
            qz = torch.zeros_like(qz)
            for j in range(8):
                qz |= zn[:, :, j] << (4 * j)
        if self.quant.awq:
            # AWQ on disk: qweight (K, N/8) with the [0,4,1,5,2,6,3,7] nibble order, zeros stored as they are
            # used (no +1).  Int4GPTQ::preprocess_weight, is_awq branch: shuffle_awq -> (K/8, N) exllama
            # words, un_shuffle of the zero nibbles; from there on it is the GPTQ operand set.
            if qw.shape != (self.dim_in, self.dim_out // 8):
                raise ops.ZLError(f"{prefix}: qweight shape {tuple(qw.shape)} != {(self.dim_in, self.dim_out // 8)}")
            qw = ops.transpose_2d(ops.shuffle_awq(qw, True))
            qz = ops.transpose_2d(ops.q4_to_q8(ops.awq_un_shuffle(qz.clone())))
        else:
            if qw.shape != (self.dim_in // 8, self.dim_out):
                raise ops.ZLError(f"{prefix}: qweight shape {tuple(qw.shape)} != {(self.dim_in // 8, self.dim_out)}")
            if self.quant.act_order and prefix + ".g_idx" in sd:
                qw = self._apply_act_order(qw, _dev_t(sd[prefix + ".g_idx"], device, torch.int32), prefix)
            # Int4GPTQ::preprocess_weight + transpose_weight: shuffle, +1 zeros, nibble->byte, transposes
            qw = ops.transpose_2d(ops.gptq_shuffle(qw.clone()))
            qz = ops.transpose_2d(ops.q4_to_q8(ops.increase_zero(qz.clone())))
        self.km = (qw, qz, ops.transpose_2d(sc))
        if input_prepermuted:
            self.perm = None
        if prefix + ".bias" in sd:
            self.bias = _dev_t(sd[prefix + ".bias"], device, torch.float16)
            if out_perm is not None:
                self.bias = self.bias.index_select(0, out_perm.to(torch.int64)).contiguous()

    def _apply_act_order(self, qw, g_idx, prefix):
        """desc_act checkpoints (the reference sorts with argsort(g_idx) and lets its exllama
        kernel read x through that permutation, src/nn/linear/linear.cpp:1144-1147, q_gemm.cu:104-251).  Same
        math, done at the boundary: the weight ROWS are put in group order once at load (then every group is
        128 consecutive k again and zeros/scales are already in group order), and forward() gathers the
        activation columns with the same permutation before the ordinary kernel runs."""
        k, g = self.dim_in, self.quant.group_size
        if g_idx.numel() != k:
            raise ops.ZLError(f"{prefix}: g_idx has {g_idx.numel()} entries, expected {k}")
        perm = torch.argsort(g_idx.to(torch.int64), stable=True)
        if not torch.equal(g_idx.to(torch.int64)[perm], torch.arange(k, device=g_idx.device) // g):
            raise ops.ZLError(f"{prefix}: g_idx is not a regrouping into groups of {g}")
        if torch.equal(perm, torch.arange(k, device=perm.device)):
            return qw                                     # trivial order (static groups)
        shifts = torch.arange(8, device=qw.device, dtype=torch.int32) * 4
        nib = ((qw.unsqueeze(1) >> shifts.view(1, 8, 1)) & 0xF).reshape(k, -1)       # (K, N) nibbles, row 8r + j
        nib = nib.index_select(0, perm).reshape(k // 8, 8, -1)
        packed = torch.zeros_like(qw)
        for j in range(8):
            packed |= nib[:, j, :] << (4 * j)
        self.perm = perm.to(torch.int32)
        return packed

    @staticmethod
    def fuse(name, parts: List["Int4GPTQ"], row_interleave=False):
        if not Int4GPTQ.same_perm(parts):
            raise ops.ZLError("act-order linears with different input permutations cannot be fused")
        out = Int4GPTQ(name, parts[0].dim_in, sum(p.dim_out for p in parts), parts[0].quant)
        out.perm = parts[0].perm                        # shared: q/k/v (gate/up) see the same input, so GPTQ gives them one order
        out.km = tuple(torch.cat([p.km[i] for p in parts], dim=0).contiguous() for i in range(3))
        if any(p.bias is not None for p in parts):
            out.bias = torch.cat([p.bias if p.bias is not None else
                                  torch.zeros(p.dim_out, dtype=torch.float16, device=out.km[0].device) for p in parts])
        out.pack(row_interleave)
        return out

    @staticmethod
    def same_perm(parts):
        first = parts[0].perm
        return all((p.perm is None) == (first is None) and (first is None or torch.equal(p.perm, first)) for p in parts)

    def pack(self, row_interleave=False):
        if w4_algo(self.quant) == "mfma":
            self.weight = ops.W4MWeight.from_k_major(*self.km, self.quant.group_size, row_interleave)
        else:
            self.weight = ops.W4Weight.from_k_major(*self.km, self.quant.group_size, self.quant.sym, row_interleave)
        if row_interleave and self.bias is not None:
            half = self.dim_out // 2
            self.bias = torch.stack([self.bias[:half], self.bias[half:]], dim=1).reshape(-1).contiguous()
        self.km = None
        return self

    def forward(self, x, **kw):
        if self.perm is not None:
            if kw.get("norm_weight") is not None:
                raise ops.ZLError("act-order linears take an already normalised input")
            x = ops.permute_input(x, self.perm)
        return ops.w4_linear(x, self.weight, bias=self.bias, **kw)


class AWQLinear:
    """nn::Linear with the AWQ implementation (src/nn/linear/linear.cpp:1400-1600, what an AWQ checkpoint runs on when
    AWQ_USE_EXLLAMA is not set): the checkpoint tensors stay in their on-disk layout -- qweight (K, N/8), qzeros (K/G, N/8),
    scales (K/G, N) -- and forward is nn::awq::awq_gemm below 256 rows (split-K 32, fp16 partials) or awq_dequantize + a
    fp32-accumulating GEMM from 256 rows on (linear.cpp:1560-1565).  The format-faithful route; the default AWQ route
    (AWQ_USE_EXLLAMA=1, Int4GPTQ above) re-tiles the same tensors once for the matrix-core kernels."""

    def __init__(self, name, dim_in, dim_out, quant: QuantConfig):
        self.name, self.dim_in, self.dim_out, self.quant = name, dim_in, dim_out, quant
        self.qweight = self.qzeros = self.scales = self.bias = None
        self.perm = None

    @property
    def weight(self):
        return self

    def nbytes(self):
        return self.qweight.numel() * 4 + self.qzeros.numel() * 4 + self.scales.numel() * 2

    def load_state_dict(self, sd, prefix, device):
        self.qweight = _dev_t(sd[prefix + ".qweight"], device, torch.int32).contiguous()
        self.qzeros = _dev_t(sd[prefix + ".qzeros"], device, torch.int32).contiguous()
        self.scales = _dev_t(sd[prefix + ".scales"], device, torch.float16).contiguous()
        if self.qweight.shape != (self.dim_in, self.dim_out // 8):
            raise ops.ZLError(f"{prefix}: qweight shape {tuple(self.qweight.shape)} != {(self.dim_in, self.dim_out // 8)}")
        if prefix + ".bias" in sd:
            self.bias = _dev_t(sd[prefix + ".bias"], device, torch.float16)
        return self

    def pack(self, row_interleave=False):
        return self

    def forward(self, x, out=None, residual=None, epilogue=0, **kw):
        if kw.get("norm_weight") is not None:
            raise ops.ZLError("AWQ linears take an already normalised input")
        g = self.quant.group_size
        x2 = x.reshape(-1, x.shape[-1])
        if x2.shape[0] < 256:
            y = ops.awq_gemm(x2, self.qweight, self.qzeros, self.scales, g)
        else:
            w16 = ops.transpose_2d(ops.awq_dequantize(self.qweight, self.qzeros, self.scales, g))      # (N, K)
            y = ops.gemm_nt(x2, w16)
        if self.bias is not None:
            y = y + self.bias                                # add_bias in T arithmetic
        if epilogue & ops.EPI_RESIDUAL:
            return ops.element_add_scale(residual, y, 1.0, True, out=out if out is not None else residual)
        if out is not None:
            out.copy_(y)
            return out
        return y


class NormalLinear:
    """nn::Linear with the NormalLinear implementation (src/nn/linear/linear.cpp:140-428): y = T(x . W^T + bias),
    fp32 accumulation.  Up to 4 rows the wave-per-row GEMV (HBM speed, optional fused RMSNorm), above the MFMA
    GEMM."""

    def __init__(self, name, dim_in, dim_out):
        self.name, self.dim_in, self.dim_out = name, dim_in, dim_out
        self.weight = self.bias = None

    def load_state_dict(self, sd, prefix, device, dtype):
        self.weight = _dev_t(sd[prefix + ".weight"], device).to(dtype).contiguous()
        if tuple(self.weight.shape) != (self.dim_out, self.dim_in):
            raise ops.ZLError(f"{prefix}: weight shape {tuple(self.weight.shape)} != {(self.dim_out, self.dim_in)}")
        if prefix + ".bias" in sd:
            self.bias = _dev_t(sd[prefix + ".bias"], device).to(dtype)
        return self

    @staticmethod
    def fuse(name, parts: List["NormalLinear"]):
        out = NormalLinear(name, parts[0].dim_in, sum(p.dim_out for p in parts))
        out.weight = torch.cat([p.weight for p in parts], dim=0).contiguous()
        if any(p.bias is not None for p in parts):
            out.bias = torch.cat([p.bias if p.bias is not None else torch.zeros(p.dim_out, dtype=out.weight.dtype,
                                                                                  device=out.weight.device) for p in parts])
        return out

    @classmethod
    def random(cls, name, dim_in, dim_out, device, gen, dtype):
        l = cls(name, dim_in, dim_out)
        l.weight = (torch.randn(dim_out, dim_in, device=device, generator=gen) * (0.7 / math.sqrt(dim_in))).to(dtype)
        return l

    def nbytes(self):
        return self.weight.numel() * 2

    def forward(self, x, out=None, norm_weight=None, norm_eps=1e-5):
        x2 = x.reshape(-1, x.shape[-1])
        if x2.shape[0] <= 4 or self.dim_in % 128 != 0:
            return ops.gemm_nt_small_m(x2, self.weight, bias=self.bias, out=out, norm_weight=norm_weight, norm_eps=norm_eps)
        if norm_weight is not None:
            x2 = ops.rmsnorm(x2, norm_weight, norm_eps)
        # 5..32 rows (decode batches of the unquantised models, BASELINE configs[0]): the ZLD16M copy of the matrix -- 1 KiB contiguous
        # fragment loads, 5.95 instead of 5.0 TB/s on the Llama-3 lm_head, the same bits; packed on first use outside stream capture.
        # A second copy of the weights: ZL_DENSE_PACKED=0 keeps only the row-major one
        if x2.shape[0] <= 32 and os.environ.get("ZL_DENSE_PACKED", "1") != "0":
            if getattr(self, "weight_m", None) is None and not torch.cuda.is_current_stream_capturing():
                self.weight_m = ops.DenseMWeight(self.weight)
            if getattr(self, "weight_m", None) is not None:
                return ops.gemm_nt_packed(x2, self.weight_m, bias=self.bias, out=out)
        return ops.gemm_nt(x2, self.weight, bias=self.bias, out=out)


class DenseEncoderLayer:
    """EncoderLayer over NormalLinear (unquantised fp16 / bf16 models, BASELINE configs[0] MiniCPM): fused q|k|v
    projection, separate w_in / w_gated + gate_mul_inplace (src/nn/feedforward/feedforward.cpp:113-137), residual
    adds through element_add_scale_out with the layer scale (src/nn/block/block.cpp:123-140)."""

    def __init__(self, cfg: ModelConfig, quant: QuantConfig, idx: int):
        self.cfg, self.quant, self.idx = cfg, quant, idx
        self.unfused = None

    def load_state_dict(self, sd, prefix, device):
        c, dt = self.cfg, self.cfg.torch_dtype
        hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
        self.ln_attn = _dev_t(sd[prefix + ".ln_attn.weight"], device).to(dt)
        self.ln_ff = _dev_t(sd[prefix + ".ln_ff.weight"], device).to(dt)
        lin = lambda sub, din, dout: NormalLinear(prefix + "." + sub, din, dout).load_state_dict(sd, prefix + "." + sub, device, dt)  # noqa: E731
        self.qkv = NormalLinear.fuse(prefix + ".attn.project_qkv",
                                     [lin("attn.project_q", c.dim_model, hd), lin("attn.project_k", c.dim_model, kvd),
                                      lin("attn.project_v", c.dim_model, kvd)])
        self.attn_out = lin("attn.attn_out", hd, c.dim_model)
        self.w_in, self.w_gated = lin("ff.w_in", c.dim_model, c.dim_ff), lin("ff.w_gated", c.dim_model, c.dim_ff)
        self.w_out = lin("ff.w_out", c.dim_ff, c.dim_model)

    def init_random(self, device, gen):
        c, dt = self.cfg, self.cfg.torch_dtype
        hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
        self.ln_attn = (1.0 + 0.05 * torch.randn(c.dim_model, device=device, generator=gen)).to(dt)
        self.ln_ff = (1.0 + 0.05 * torch.randn(c.dim_model, device=device, generator=gen)).to(dt)
        self.qkv = NormalLinear.random("qkv", c.dim_model, hd + 2 * kvd, device, gen, dt)
        self.attn_out = NormalLinear.random("attn_out", hd, c.dim_model, device, gen, dt)
        self.w_in = NormalLinear.random("w_in", c.dim_model, c.dim_ff, device, gen, dt)
        self.w_gated = NormalLinear.random("w_gated", c.dim_model, c.dim_ff, device, gen, dt)
        self.w_out = NormalLinear.random("w_out", c.dim_ff, c.dim_model, device, gen, dt)

    def linears(self):
        return [self.qkv, self.attn_out, self.w_in, self.w_gated, self.w_out]

    def weight_bytes(self):
        return sum(l.nbytes() for l in self.linears())

    def project_qkv(self, hidden, eps, out=None):
        return self.qkv.forward(hidden, out=out, norm_weight=self.ln_attn, norm_eps=eps)

    def _add(self, hidden, sub):
        # residual first, T arithmetic: c = a + b * T(scale) for MiniCPM, (a + b) * T(1) otherwise
        rs = self.cfg.residual_scale
        ops.element_add_scale(hidden, sub, rs, scale_residual=(self.cfg.scale_depth <= 0), out=hidden)

    def attn_out_add(self, attn, hidden):
        self._add(hidden, self.attn_out.forward(attn))

    def ff_add(self, hidden, eps, act_buf=None):
        xn = ops.rmsnorm(hidden, self.ln_ff, eps)
        gate = self.w_in.forward(xn, out=act_buf)
        act = ops.gate_mul(gate, self.w_gated.forward(xn), "gelu" if self.cfg.activate_fn.startswith("gelu") else "silu")
        self._add(hidden, self.w_out.forward(act))


class Int8Linear:
    """nn::Linear with the Int8Linear implementation (src/nn/linear/linear.cpp:430-635, quant type 2 = AutoInt8):
    the fp16 weight is quantised per output row at load (quant_calc_scale: scale = amax / 127, stored in T),
    forward = per-row activation quantisation, int8 x int8 -> int32 GEMM, scale back."""

    def __init__(self, name, dim_in, dim_out):
        self.name, self.dim_in, self.dim_out = name, dim_in, dim_out
        self.weight = self.scale = self.bias = None     # int8 (N, K), T (N), T (N)

    def load_state_dict(self, sd, prefix, device):
        w = _dev_t(sd[prefix + ".weight"], device)
        if tuple(w.shape) != (self.dim_out, self.dim_in):
            raise ops.ZLError(f"{prefix}: weight shape {tuple(w.shape)} != {(self.dim_out, self.dim_in)}")
        self.weight, s = ops.quant_calc_scale(w)
        self.scale = s.to(w.dtype)                       # functions::typecast(w_scale, dtype)
        if prefix + ".bias" in sd:
            # the reference concatenates the biases in fuse3 and adds them after the scale-back (linear.cpp:459-461,
            # 631-632); the fused scale-back epilogues of this route carry none yet -- refuse instead of dropping it
            raise ops.ZLError(f"{prefix}: bias tensors are not supported on the int8 route (checkpoints with q/k/v biases, "
                              "e.g. Qwen2: use the GPTQ / fp16 routes)")
        return self

    @staticmethod
    def fuse(name, parts: List["Int8Linear"]):
        out = Int8Linear(name, parts[0].dim_in, sum(p.dim_out for p in parts))
        out.weight = torch.cat([p.weight for p in parts], dim=0).contiguous()
        out.scale = torch.cat([p.scale for p in parts]).contiguous()
        return out

    @classmethod
    def random(cls, name, dim_in, dim_out, device, gen):
        l = cls(name, dim_in, dim_out)
        l.weight = torch.randint(-127, 128, (dim_out, dim_in), dtype=torch.int8, device=device, generator=gen)
        l.scale = (torch.rand(dim_out, device=device, generator=gen) * (0.02 / math.sqrt(dim_in)) + 1e-5).to(torch.float16)
        return l

    def nbytes(self):
        return self.weight.numel() + self.scale.numel() * 2

    def gemm(self, xq):
        """int32 (M, N) = xq . W^T -- the caller fuses the scale-back"""
        return ops.int8_gemm_nt(xq, self.weight)

    def stream_weight(self):
        """the ZLW8M copy for the decode kernel (zl_w8a8_gemm_phase), packed on first use; the (N, K) rows stay for the
        tiled GEMM of prompt chunks and batches beyond 32 rows"""
        if getattr(self, "_w8m", None) is None:
            self._w8m = ops.W8MWeight.from_rows(self.weight, self.scale)
        return self._w8m


class Int8EncoderLayer:
    """EncoderLayer over Int8Linear (BASELINE configs[2]) with the fusions of the reference's
    int8 route: layernorm_quant feeds q/k/v (one shared int8 input, src/nn/linear/linear.cpp:568-583),
    quant_scale_back on the fused qkv product, quant_back_act_mul for the gated FF
    (src/nn/feedforward/feedforward.cpp:163-187), quant_back_element_add_scale for the residual adds."""

    def __init__(self, cfg: ModelConfig, quant: QuantConfig, idx: int):
        self.cfg, self.quant, self.idx = cfg, quant, idx
        self.unfused = None

    def load_state_dict(self, sd, prefix, device):
        c = self.cfg
        hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
        self.ln_attn = _dev_t(sd[prefix + ".ln_attn.weight"], device)
        self.ln_ff = _dev_t(sd[prefix + ".ln_ff.weight"], device)
        lin = lambda sub, din, dout: Int8Linear(prefix + "." + sub, din, dout).load_state_dict(sd, prefix + "." + sub, device)  # noqa: E731
        self.qkv = Int8Linear.fuse(prefix + ".attn.project_qkv",
                                   [lin("attn.project_q", c.dim_model, hd), lin("attn.project_k", c.dim_model, kvd),
                                    lin("attn.project_v", c.dim_model, kvd)])
        self.attn_out = lin("attn.attn_out", hd, c.dim_model)
        self.w_in, self.w_gated = lin("ff.w_in", c.dim_model, c.dim_ff), lin("ff.w_gated", c.dim_model, c.dim_ff)
        self.w_out = lin("ff.w_out", c.dim_ff, c.dim_model)

    def init_random(self, device, gen):
        c = self.cfg
        hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
        self.ln_attn = (1.0 + 0.05 * torch.randn(c.dim_model, device=device, generator=gen)).to(torch.float16)
        self.ln_ff = (1.0 + 0.05 * torch.randn(c.dim_model, device=device, generator=gen)).to(torch.float16)
        self.qkv = Int8Linear.random("qkv", c.dim_model, hd + 2 * kvd, device, gen)
        self.attn_out = Int8Linear.random("attn_out", hd, c.dim_model, device, gen)
        self.w_in = Int8Linear.random("w_in", c.dim_model, c.dim_ff, device, gen)
        self.w_gated = Int8Linear.random("w_gated", c.dim_model, c.dim_ff, device, gen)
        self.w_out = Int8Linear.random("w_out", c.dim_ff, c.dim_model, device, gen)

    def linears(self):
        return [self.qkv, self.attn_out, self.w_in, self.w_gated, self.w_out]

    def weight_bytes(self):
        return sum(l.nbytes() for l in self.linears())

    # Decode batches (<= 32 rows): the streaming int8 kernel with the scale-back fused in its epilogue
    # (zl_w8a8_gemm_phase: 4 GEMM launches per layer instead of 5 GEMMs + 4 scale-back kernels + split-K memsets;
    # bit-identical results).  More rows: the tiled int8 GEMM + the reference's separate scale-back kernels.
    @staticmethod
    def _stream(rows):
        return rows <= 32 and os.environ.get("ZL_W8_PHASE", "1") != "0"

    def _gated_stream_weight(self):
        if getattr(self, "_w8m_gated", None) is None:
            self._w8m_gated = ops.W8MWeight.from_rows(torch.cat([self.w_in.weight, self.w_gated.weight], dim=0),
                                                      torch.cat([self.w_in.scale, self.w_gated.scale]), row_interleave=True)
        return self._w8m_gated

    def project_qkv(self, hidden, eps, out=None):
        _, xq, sx = ops.layernorm_quant(hidden, self.ln_attn, eps)
        if self._stream(hidden.shape[0]):
            return ops.w8a8_gemm_phase(xq, sx, self.qkv.stream_weight(), ops.W8_BACK, out=out, dtype=hidden.dtype)
        return ops.quant_scale_back(self.qkv.gemm(xq), sx, self.qkv.scale, hidden.dtype, out=out)

    def attn_out_add(self, attn, hidden):
        aq, sa = ops.quant_calc_scale(attn)
        if self._stream(hidden.shape[0]):
            return ops.w8a8_gemm_phase(aq, sa, self.attn_out.stream_weight(), ops.W8_BACK_ADD, addend=hidden, scale=1.0, out=hidden)
        ops.quant_back_element_add_scale(self.attn_out.gemm(aq), sa, self.attn_out.scale, hidden, 1.0, out=hidden)

    def ff_add(self, hidden, eps, act_buf=None):
        _, xq, sx = ops.layernorm_quant(hidden, self.ln_ff, eps)
        if self._stream(hidden.shape[0]):
            act = ops.w8a8_gemm_phase(xq, sx, self._gated_stream_weight(), ops.W8_ACT_SILU, out=act_buf, dtype=hidden.dtype)
            aq, sa = ops.quant_calc_scale(act)
            return ops.w8a8_gemm_phase(aq, sa, self.w_out.stream_weight(), ops.W8_BACK_ADD, addend=hidden, scale=1.0, out=hidden)
        act = ops.quant_back_act_mul(self.w_in.gemm(xq), sx, self.w_in.scale, self.w_gated.gemm(xq), sx, self.w_gated.scale,
                                     "silu", hidden.dtype)
        aq, sa = ops.quant_calc_scale(act)
        ops.quant_back_element_add_scale(self.w_out.gemm(aq), sa, self.w_out.scale, hidden, 1.0, out=hidden)


def mxfp4_tensors(sd, prefix):
    """The ONE place that knows how an MXFP4 linear is spelled in a checkpoint -> (codes (N, K/2) uint8, scales (N, K/32) uint8,
    bias or None).  Accepted: `<name>.weight` uint8 (N, K/2) + `<name>.weight_scale` uint8 (N, K/32) (the spelling Quark's
    exporter is documented to write) and `<name>.weight_blocks` (N, K/32, 16) + `<name>.weight_scales` (transformers' mxfp4
    integration), plus an optional `<name>.bias`.  UNVERIFIED against a real Quark checkpoint: none was available when this was
    written; a different spelling is a change to this function only."""
    if prefix + ".weight_blocks" in sd:
        codes, scales = sd[prefix + ".weight_blocks"], sd.get(prefix + ".weight_scales")
    else:
        codes, scales = sd.get(prefix + ".weight"), sd.get(prefix + ".weight_scale")
    if codes is None or scales is None:
        raise ops.ZLError(f"{prefix}: MXFP4 tensors not found (.weight + .weight_scale, or .weight_blocks + .weight_scales)")
    codes, scales = (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t)) for t in (codes, scales))
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ops.ZLError(f"{prefix}: MXFP4 codes and scales are uint8 tensors (got {codes.dtype}, {scales.dtype})")
    if codes.dim() == 3:
        codes = codes.reshape(codes.shape[0], -1)
    return codes, scales, sd.get(prefix + ".bias")


class Mxfp4Linear:
    """A linear on MXFP4 weights (quant type 11): y = T(x . W^T + bias), T = fp16 or bf16, no weight ever rounded
    (ops.mxfp4_linear).  `fuse` concatenates rows like Linear::fuse; row_interleave for the gated pair."""

    def __init__(self, name, dim_in, dim_out):
        self.name, self.dim_in, self.dim_out = name, dim_in, dim_out
        self.weight: Optional[ops.Mxfp4Weight] = None
        self.bias = None

    def load_state_dict(self, sd, prefix, device, dtype):
        codes, scales, bias = mxfp4_tensors(sd, prefix)
        if tuple(codes.shape) != (self.dim_out, self.dim_in // 2) or tuple(scales.shape) != (self.dim_out, self.dim_in // 32):
            raise ops.ZLError(f"{prefix}: codes {tuple(codes.shape)} / scales {tuple(scales.shape)} do not fit a "
                              f"({self.dim_out}, {self.dim_in}) MXFP4 weight")
        self.weight = ops.Mxfp4Weight.from_checkpoint(_dev_t(codes, device), _dev_t(scales, device))
        if bias is not None:
            self.bias = _dev_t(bias, device).to(dtype).contiguous()
        return self

    @staticmethod
    def fuse(name, parts: List["Mxfp4Linear"], row_interleave=False):
        out = Mxfp4Linear(name, parts[0].dim_in, sum(p.dim_out for p in parts))
        out.weight = ops.Mxfp4Weight.from_checkpoint(torch.cat([p.weight.codes for p in parts], dim=0),
                                                     torch.cat([p.weight.scales for p in parts], dim=0), row_interleave)
        if any(p.bias is not None for p in parts):
            ref = next(p.bias for p in parts if p.bias is not None)
            b = torch.cat([p.bias if p.bias is not None else torch.zeros(p.dim_out, dtype=ref.dtype, device=ref.device) for p in parts])
            if row_interleave:
                b = b.view(2, -1).t().reshape(-1)
            out.bias = b.contiguous()
        return out

    @classmethod
    def random(cls, name, dim_in, dim_out, device, gen, row_interleave=False):
        l = cls(name, dim_in, dim_out)
        l.weight = ops.Mxfp4Weight.random(dim_out, dim_in, device, gen, std=0.25 / math.sqrt(dim_in), row_interleave=row_interleave)
        return l

    def nbytes(self):
        return self.weight.nbytes()

    def forward(self, x, out=None, residual=None, epilogue=0):
        return ops.mxfp4_linear(x, self.weight, bias=self.bias, residual=residual, out=out, epilogue=epilogue)


class Mxfp4EncoderLayer:
    """EncoderLayer over Mxfp4Linear (quant type 11), on the plain route of the decode step and of prompt encode: a stand-alone
    RMSNorm, q|k|v fused by row concatenation (its bias: Qwen2-style checkpoints), gate|up fused row-interleaved under the
    silu*mul epilogue, attn_out and w_out under the residual epilogue -- 4 GEMM launches + 2 norms per layer."""

    def __init__(self, cfg: ModelConfig, quant: QuantConfig, idx: int):
        if not cfg.activate_fn.startswith("silu"):
            raise ops.ZLError("MXFP4 layers: silu feed-forward only")
        self.cfg, self.quant, self.idx = cfg, quant, idx
        self.unfused = None

    def load_state_dict(self, sd, prefix, device):
        c, dt = self.cfg, self.cfg.torch_dtype
        hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
        self.ln_attn = _dev_t(sd[prefix + ".ln_attn.weight"], device).to(dt)
        self.ln_ff = _dev_t(sd[prefix + ".ln_ff.weight"], device).to(dt)
        lin = lambda sub, din, dout: Mxfp4Linear(prefix + "." + sub, din, dout).load_state_dict(sd, prefix + "." + sub, device, dt)  # noqa: E731
        self.qkv = Mxfp4Linear.fuse(prefix + ".attn.project_qkv",
                                    [lin("attn.project_q", c.dim_model, hd), lin("attn.project_k", c.dim_model, kvd),
                                     lin("attn.project_v", c.dim_model, kvd)])
        self.attn_out = lin("attn.attn_out", hd, c.dim_model)
        self.w_in_gated = Mxfp4Linear.fuse(prefix + ".ff.w_in_gated", [lin("ff.w_in", c.dim_model, c.dim_ff),
                                                                      lin("ff.w_gated", c.dim_model, c.dim_ff)], row_interleave=True)
        self.w_out = lin("ff.w_out", c.dim_ff, c.dim_model)

    def init_random(self, device, gen):
        """weights quantised (ops.mxfp4_quantize) from N(0, 1 / sqrt(K)) / 4"""
        c, dt = self.cfg, self.cfg.torch_dtype
        hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
        self.ln_attn = (1.0 + 0.05 * torch.randn(c.dim_model, device=device, generator=gen)).to(dt)
        self.ln_ff = (1.0 + 0.05 * torch.randn(c.dim_model, device=device, generator=gen)).to(dt)
        self.qkv = Mxfp4Linear.random("qkv", c.dim_model, hd + 2 * kvd, device, gen)
        self.attn_out = Mxfp4Linear.random("attn_out", hd, c.dim_model, device, gen)
        self.w_in_gated = Mxfp4Linear.random("w_in_gated", c.dim_model, 2 * c.dim_ff, device, gen, row_interleave=True)
        self.w_out = Mxfp4Linear.random("w_out", c.dim_ff, c.dim_model, device, gen)

    def linears(self):
        return [self.qkv, self.attn_out, self.w_in_gated, self.w_out]

    def weight_bytes(self):
        return sum(l.nbytes() for l in self.linears())

    def project_qkv(self, hidden, eps, out=None):
        return self.qkv.forward(ops.rmsnorm(hidden, self.ln_attn, eps), out=out)

    def attn_out_add(self, attn, hidden):
        self.attn_out.forward(attn, residual=hidden, out=hidden)

    def ff_add(self, hidden, eps, act_buf=None):
        rows = hidden.shape[0]
        if act_buf is not None and act_buf.shape[0] != rows:
            act_buf = None
        act = self.w_in_gated.forward(ops.rmsnorm(hidden, self.ln_ff, eps), out=act_buf, epilogue=ops.EPI_SILU_MUL)
        self.w_out.forward(act, residual=hidden, out=hidden)


# decode attention with the split merge inside its launch (zl_decode_attn_la): default of the ZL_ATTN_LA switch
_ATTN_LA_DEFAULT = "auto"


# 9..32 decode rows: RMSNorm deferred into the phase kernel (w4_phase.hip DN) instead of a stand-alone launch: the ZL_DEFER_NORM switch.
# OFF by default -- measured (round 5, profiles/r05_defer_norm.txt): +5 % tokens/s at batch 32, +10 % at batch 16, but every output of the
# qkv and gate|up projections then carries an fp16 rounding the reference does not make (T(x w) rs instead of T(x rs w)), and on the
# synthetic network that is 1e-2 of the largest logit after 4 layers (tests/test_gpu_fullgeom.py [32-4]: 1.35e-2 from R against a
# 6e-3 bar; test_gpu_model batch 20: 1.8e-3 from E against 1e-3).  Parity is the first gate: opt-in only.
_DEFER_NORM_DEFAULT = "0"


def _fused_norm_rows(weight):
    """rows up to which the W4A16 kernel of this weight fuses the RMSNorm: 8 for the phase-pipelined MFMA kernel
    (register-resident activations, K <= 4096; bit-identical to the stand-alone launch), 32 with the deferred norm on
    (ZL_DEFER_NORM=1: rs applied to the fp32 totals, not bit-identical), 4 otherwise"""
    if not (isinstance(weight, ops.W4MWeight) and weight.k <= 4096 and weight.group_size % 128 == 0):
        return 4
    return 32 if os.environ.get("ZL_DEFER_NORM", _DEFER_NORM_DEFAULT) != "0" else 8


class EncoderLayer:
    """nn::EncoderLayer (src/nn/block/block.h:15-63): ln_attn, attn{project_q,k,v,attn_out}, ln_ff,
    ff{w_in,w_gated,w_out}; q/k/v and w_in/w_gated are fused at load (CPM_FUSE_QKV / CPM_FUSE_FF_IN)."""

    def __init__(self, cfg: ModelConfig, quant: QuantConfig, idx: int, tp=None):
        self.cfg, self.quant, self.idx = cfg, quant, idx
        self.ln_attn = self.ln_ff = None
        self.qkv = self.attn_out = self.w_in_gated = self.w_out = None
        self.unfused = None     # act-order checkpoints: [q, k, v, w_in, w_gated] as separate linears
        # tensor parallelism: cfg holds the LOCAL head / ff counts; q/k/v and gate/up are column-parallel,
        # attn_out / w_out row-parallel: their partial outputs are summed over the ranks before the residual add
        self.tp = tp if tp is not None and tp.size > 1 else None

    def load_state_dict(self, sd, prefix, device, ff=True):
        """ff=False: the attention half and both norms only (MoEEncoderLayer loads its own feed-forward)"""
        c, q = self.cfg, self.quant
        hd = c.num_heads * c.dim_head
        kvd = c.num_kv_heads * c.dim_head
        self.ln_attn = _dev_t(sd[prefix + ".ln_attn.weight"], device, torch.float16)
        self.ln_ff = _dev_t(sd[prefix + ".ln_ff.weight"], device, torch.float16)

        tp = self.tp

        # act-order feed-forward: w_in / w_gated OUTPUT columns are stored in w_out's regrouped input order, so the
        # activation reaches w_out already permuted (no gather, and a TP rank's column slice of w_in / w_gated matches its
        # row slice of w_out) -- the reference's permute_ff_up_out (linear.cpp:1168-1210)
        ff_out_perm = None
        g_out = sd.get(prefix + ".ff.w_out.g_idx") if q.act_order else None
        if g_out is not None:
            g64 = _dev_t(g_out, device, torch.int32).to(torch.int64)
            op = torch.argsort(g64, stable=True)
            if not torch.equal(op, torch.arange(op.numel(), device=op.device)):
                ff_out_perm = op.to(torch.int32)

        def lin(sub, din, dout, mode=None, part=None, out_perm=None, prepermuted=False):
            # the checkpoint holds the FULL matrix; a TP rank keeps its column (output rows) or row (input columns) slice
            # (part = (index, count) overrides (rank, size): replicated kv heads)
            idx, cnt = part if part else ((tp.rank, tp.size) if tp else (0, 1))
            full_in, full_out = (din * cnt if mode == "row" else din), (dout * cnt if mode == "column" else dout)
            l = Int4GPTQ(prefix + "." + sub, full_in, full_out, q)
            l.load_state_dict(sd, prefix + "." + sub, device, out_perm=out_perm, input_prepermuted=prepermuted)
            if tp and mode:
                if l.perm is not None and mode == "row":
                    # row-parallel with an input gather left (attn_out): the rank keeps rows [idx K/cnt, ...) of the REGROUPED
                    # order, which are scattered over all heads -- forward all-gathers the attention output first
                    l.tp_gather_perm = l.perm[idx * din:(idx + 1) * din].contiguous()
                    l.perm = None
                l.km = parallel.shard_k_major(*l.km, q.group_size, mode, idx, cnt)
                l.dim_in, l.dim_out = din, dout
                if l.bias is not None and mode == "column":
                    l.bias = l.bias[idx * dout:(idx + 1) * dout].contiguous()
                if l.bias is not None and mode == "row" and tp.rank != 0:
                    l.bias = None                     # added once, by rank 0's partial sum
            return l
        if q.awq and os.environ.get("AWQ_USE_EXLLAMA", "1") == "0":
            # the reference's native AWQ route: every linear on its own, tensors as stored (no q/k/v or gate/up fusion)
            if tp:
                raise ops.ZLError("the native AWQ route is not wired into tensor parallelism (use AWQ_USE_EXLLAMA=1)")

            def alin(sub, din, dout):
                return AWQLinear(prefix + "." + sub, din, dout, q).load_state_dict(sd, prefix + "." + sub, device)
            self.unfused = [alin("attn.project_q", c.dim_model, hd), alin("attn.project_k", c.dim_model, kvd),
                            alin("attn.project_v", c.dim_model, kvd), alin("ff.w_in", c.dim_model, c.dim_ff),
                            alin("ff.w_gated", c.dim_model, c.dim_ff)]
            self.attn_out = alin("attn.attn_out", hd, c.dim_model)
            self.w_out = alin("ff.w_out", c.dim_ff, c.dim_model)
            return
        kv_part = getattr(self, "kv_part", None)
        pq, pk, pv = (lin("attn.project_q", c.dim_model, hd, "column"), lin("attn.project_k", c.dim_model, kvd, "column", kv_part),
                      lin("attn.project_v", c.dim_model, kvd, "column", kv_part))
        if ff:
            w_in = lin("ff.w_in", c.dim_model, c.dim_ff, "column", out_perm=ff_out_perm)
            w_gated = lin("ff.w_gated", c.dim_model, c.dim_ff, "column", out_perm=ff_out_perm)
        self.attn_out = lin("attn.attn_out", hd, c.dim_model, "row").pack()
        if ff:
            self.w_out = lin("ff.w_out", c.dim_ff, c.dim_model, "row", prepermuted=ff_out_perm is not None).pack()
        if not (Int4GPTQ.same_perm([pq, pk, pv]) and (not ff or Int4GPTQ.same_perm([w_in, w_gated]))):
            # act-order with DIFFERENT input orders inside a group (not what GPTQ produces for linears sharing their input,
            # but a legal checkpoint): every linear gathers x itself, q/k/v and gate/up stay separate
            self.unfused = [l.pack() for l in ((pq, pk, pv, w_in, w_gated) if ff else (pq, pk, pv))]
        else:
            self.qkv = Int4GPTQ.fuse(prefix + ".attn.project_qkv", [pq, pk, pv])
            if ff:
                self.w_in_gated = Int4GPTQ.fuse(prefix + ".ff.w_in_gated", [w_in, w_gated], row_interleave=True)

    def init_random(self, device, gen):
        """Synthetic weights of the right shapes, generated directly in the packed layout."""
        c, q = self.cfg, self.quant
        hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
        self.ln_attn = (1.0 + 0.05 * torch.randn(c.dim_model, device=device, generator=gen)).to(torch.float16)
        self.ln_ff = (1.0 + 0.05 * torch.randn(c.dim_model, device=device, generator=gen)).to(torch.float16)

        def rnd(name, din, dout, interleave=False):
            l = Int4GPTQ(name, din, dout, q)
            mag = 1.0 / math.sqrt(din) / 4.0
            if w4_algo(q) == "mfma":
                l.weight = ops.W4MWeight.random(dout, din, q.group_size, device, gen, mag, interleave)
            else:
                l.weight = ops.W4Weight.random(dout, din, q.group_size, device, gen, mag, q.sym, interleave)
            return l
        self.qkv = rnd("qkv", c.dim_model, hd + 2 * kvd)
        self.attn_out = rnd("attn_out", hd, c.dim_model)
        self.w_in_gated = rnd("w_in_gated", c.dim_model, 2 * c.dim_ff, True)
        self.w_out = rnd("w_out", c.dim_ff, c.dim_model)

    def linears(self):
        return list(self.unfused) + [self.attn_out, self.w_out] if self.unfused else [self.qkv, self.attn_out, self.w_in_gated, self.w_out]

    def weight_bytes(self):
        return sum(l.weight.nbytes() for l in self.linears())

    # the two fused projections, or their act-order stand-ins (separate RMSNorm, per-linear gather, concat / gate_mul)
    def project_qkv(self, hidden, eps, out=None, normed=None):
        """normed: ln_attn(hidden) already computed by the caller (the dual-stream path's fused add + norm)"""
        if self.unfused is None:
            if self.qkv.perm is not None:                 # act-order: RMSNorm, ONE gather for the fused q|k|v, then the GEMV
                xn = normed if normed is not None else ops.rmsnorm(hidden, self.ln_attn, eps)
                return ops.w4_linear(ops.permute_input(xn, self.qkv.perm), self.qkv.weight, bias=self.qkv.bias, out=out)
            if normed is not None:
                return ops.w4_linear(normed, self.qkv.weight, bias=self.qkv.bias, out=out)
            if hidden.shape[0] > _fused_norm_rows(self.qkv.weight):   # the fused norm prologue normalises every row in every
                xn = ops.rmsnorm(hidden, self.ln_attn, eps)           # workgroup: beyond a few rows a separate launch is cheaper
                return ops.w4_linear(xn, self.qkv.weight, bias=self.qkv.bias, out=out)
            return ops.w4_linear(hidden, self.qkv.weight, bias=self.qkv.bias, out=out, norm_weight=self.ln_attn, norm_eps=eps)
        xn = normed if normed is not None else ops.rmsnorm(hidden, self.ln_attn, eps)
        parts = [l.forward(xn) for l in self.unfused[:3]]
        return torch.cat(parts, dim=1, out=out) if out is not None else torch.cat(parts, dim=1)

    def row_partial(self, lin, x):
        """this rank's partial output of a row-parallel linear.  act-order attn_out: the rank's regrouped rows span all
        heads, so the attention output is all-gathered and read through the rank's slice of the permutation first"""
        gp = getattr(lin, "tp_gather_perm", None)
        if gp is not None:
            x = ops.permute_input(self.tp.all_gather_columns(x), gp)
        return lin.forward(x)

    def _row_parallel_add(self, lin, x, hidden):
        """hidden += sum over TP ranks of lin(x): ModelContext::reduce_sum on the fp16 partial outputs, then the
        residual add in T arithmetic (src/nn/block/block.cpp:123-140, src/model/model_context.cpp:203-242)"""
        part = self.row_partial(lin, x)
        # REDUCE_TP_INT8_THRES (the reference's switch, model_context.cpp:221-227): above that many rows the partial sums travel
        # as group-32 int8 codes (ModelContext::reduce_tp_int8)
        thres = int(os.environ.get("REDUCE_TP_INT8_THRES", "0") or 0)
        compressed = getattr(self.tp, "reduce_tp_int8", None)
        if thres > 0 and compressed is not None and part.shape[0] > thres and part.numel() % (32 * self.tp.size) == 0:
            # the one-shot INT8 exchange takes whole 64-element groups per rank, a contiguous 8-byte-aligned message that fits its
            # buffer; everything else needs the RCCL composition -- and without either transport the fp16 all-reduce below runs
            # (the branch used to be entered with only `oneshot` present and then raised for shapes it does not take)
            one = getattr(self.tp, "oneshot", None)
            fits = (one is not None and part.is_contiguous() and part.data_ptr() % 8 == 0 and part.numel() % (64 * self.tp.size) == 0
                    and part.numel() * 2 <= getattr(self.tp, "oneshot_bytes", 0))
            if fits or getattr(self.tp, "comm", None) is not None:
                ops.element_add_scale(hidden, compressed(part), 1.0, True, out=hidden)
                return
        fused = getattr(self.tp, "all_reduce_add", None)
        if fused is not None and fused(part, hidden) is not None:      # one-shot all-reduce with the residual add in its launch
            return
        self.tp.all_reduce_sum(part)
        ops.element_add_scale(hidden, part, 1.0, True, out=hidden)

    def attn_out_add(self, attn, hidden):
        """hidden += attn_out(attn) in place (linear + element_add_scale fused in the epilogue)"""
        if self.tp:
            return self._row_parallel_add(self.attn_out, attn, hidden)
        self.attn_out.forward(attn, residual=hidden, out=hidden, epilogue=ops.EPI_RESIDUAL)

    def ff_add(self, hidden, eps, act_buf=None):
        """hidden += w_out(silu(w_in(ln(hidden))) * w_gated(ln(hidden))) in place"""
        act = self.ff_in(hidden, eps, out=act_buf)
        if self.tp:
            return self._row_parallel_add(self.w_out, act, hidden)
        self.w_out.forward(act, residual=hidden, out=hidden, epilogue=ops.EPI_RESIDUAL)

    def ff_in(self, hidden, eps, out=None, normed=None):
        if self.unfused is None:
            if self.w_in_gated.perm is not None:
                xn = normed if normed is not None else ops.rmsnorm(hidden, self.ln_ff, eps)
                return ops.w4_linear(ops.permute_input(xn, self.w_in_gated.perm), self.w_in_gated.weight, bias=self.w_in_gated.bias,
                                     out=out, epilogue=ops.EPI_SILU_MUL)
            if normed is not None:
                return ops.w4_linear(normed, self.w_in_gated.weight, bias=self.w_in_gated.bias, out=out, epilogue=ops.EPI_SILU_MUL)
            if hidden.shape[0] > _fused_norm_rows(self.w_in_gated.weight):
                xn = ops.rmsnorm(hidden, self.ln_ff, eps)
                return ops.w4_linear(xn, self.w_in_gated.weight, bias=self.w_in_gated.bias, out=out, epilogue=ops.EPI_SILU_MUL)
            return ops.w4_linear(hidden, self.w_in_gated.weight, bias=self.w_in_gated.bias, out=out, norm_weight=self.ln_ff,
                                 norm_eps=eps, epilogue=ops.EPI_SILU_MUL)
        xn = normed if normed is not None else ops.rmsnorm(hidden, self.ln_ff, eps)
        gate = self.unfused[3].forward(xn, out=out)
        return ops.gate_mul(gate, self.unfused[4].forward(xn), "silu")


def moe_route():
    """Which expert layout a layer holds (ZL_MOE_ROUTE, read at load).  A layer holds ONE copy of its expert weights:
      "grouped" (default)  ZLW4M stacks.  Rows up to GPTQ_MOE_M_THRES (the reference's switch, feedforward.cpp:1248-1290) take the
                           small-M form zl_w4a16_gemm_pairs (one tile per (token, expert) pair, no sort); above it the sorted
                           zl_w4a16_gemm_grouped (one tile per BM rows of an expert).  Both: MOEImpl::forward's arithmetic (the
                           M > 40 linears), the same bits for the same rows, sum_experts as the combine
      "fused"              ZLW4 stacks; every row count through the fused GEMVs zl_w4a16_moe_up / _down -- the reference's
                           FUSE_GPTQ_MOE kernels bit for bit, which stream an expert's weights once per (token, expert) pair"""
    r = os.environ.get("ZL_MOE_ROUTE", "grouped").lower()
    if r not in ("grouped", "fused"):
        raise ops.ZLError(f"ZL_MOE_ROUTE={r!r}: expected 'grouped' or 'fused'")
    return r


_MOE_M_THRES_DEFAULT = "8"             # rows; the pair form measured faster up to 8 rows, the sorted form from 32


class MoEEncoderLayer(EncoderLayer):
    """EncoderLayer with a routed mixture-of-experts feed-forward (GPTQ experts, Qwen3-MoE; reference FeedForward with
    FUSE_GPTQ_MOE, feedforward.cpp:1248-1290): the attention half is EncoderLayer's, ln_ff + router + experts replace w_in_gated /
    w_out.  Not with tensor or expert parallelism, act-order or AWQ checkpoints, or shared experts (ZLError)."""

    def __init__(self, cfg: ModelConfig, quant: QuantConfig, idx: int, tp=None):
        if tp is not None and tp.size > 1:
            raise ops.ZLError("MoE layers: tensor parallelism is not supported")
        if os.environ.get("MOE_EXP_PARALLEL", "0") not in ("", "0"):
            raise ops.ZLError("MoE layers: expert parallelism is not supported")
        if quant.quant_type != 5 or quant.act_order or quant.awq:
            raise ops.ZLError("MoE layers: GPTQ W4A16 experts without act-order only")
        if quant.group_size % 128 or cfg.dim_model % 128 or cfg.moe_intermediate_size % 128:
            raise ops.ZLError("MoE layers: group size, dim_model and moe_intermediate_size are multiples of 128")
        if not (0 < cfg.moe_top_k <= min(32, cfg.moe_num_experts)):
            raise ops.ZLError("MoE layers: 1 <= num_experts_per_tok <= min(32, num_experts)")
        super().__init__(cfg, quant, idx, None)
        self.route = moe_route()
        # rows up to this take the pair form (GPTQ_MOE_M_THRES, read at load; default: the measured crossover)
        self.m_thres = int(os.environ.get("GPTQ_MOE_M_THRES", _MOE_M_THRES_DEFAULT) or 0)
        self.router = self.w_up = self.w_down = None

    def load_state_dict(self, sd, prefix, device):
        c, q = self.cfg, self.quant
        if any(k.startswith(prefix + ".ff.shared_expert") for k in sd):
            raise ops.ZLError(f"{prefix}: shared experts are not supported")
        super().load_state_dict(sd, prefix, device, ff=False)      # ln_attn, ln_ff, fused q|k|v, attn_out

        def lin(sub, din, dout):
            l = Int4GPTQ(prefix + "." + sub, din, dout, q)
            l.load_state_dict(sd, prefix + "." + sub, device)
            return l
        router = sd[prefix + ".ff.router.weight"]
        if tuple(router.shape) != (c.moe_num_experts, c.dim_model):
            raise ops.ZLError(f"{prefix}: router weight shape {tuple(router.shape)} != {(c.moe_num_experts, c.dim_model)}")
        self.router = _dev_t(router, device).to(torch.float16).contiguous()
        # every expert through Int4GPTQ's load transforms (shuffle, zero + 1, transposes), packed straight into ONE stack per
        # projection: gate and up row-interleaved as (gate_n, up_n) pairs for the silu*mul epilogue
        e, ff = c.moe_num_experts, c.moe_intermediate_size
        stack = ops.W4MMoEWeight if self.route == "grouped" else ops.W4MoEWeight
        up_parts, down_parts = ([], [], []), ([], [], [])
        for i in range(e):
            g, u = lin(f"ff.experts.{i}.w_in", c.dim_model, ff), lin(f"ff.experts.{i}.w_gated", c.dim_model, ff)
            for j in range(3):
                up_parts[j].append(torch.cat([g.km[j], u.km[j]]).contiguous())
            d = lin(f"ff.experts.{i}.w_out", ff, c.dim_model)
            for j in range(3):
                down_parts[j].append(d.km[j])
        self.w_up = stack.from_k_major(*up_parts, q.group_size, row_interleave=True)
        self.w_down = stack.from_k_major(*down_parts, q.group_size)

    def init_random(self, device, gen):
        raise ops.ZLError("MoE layers: use LLaMA.init_synthetic (the real load path)")

    def linears(self):
        return [self.qkv, self.attn_out]

    def weight_bytes(self):
        return sum(l.weight.nbytes() for l in self.linears()) + self.w_up.nbytes() + self.w_down.nbytes() + self.router.numel() * 2

    def moe(self, xn):
        """the routed feed-forward of normalised rows xn (T, dim_model) fp16 -> (T, dim_model) fp16"""
        c = self.cfg
        t, e, k = xn.shape[0], c.moe_num_experts, c.moe_top_k
        # MOEImpl::route (feedforward.cpp:419-482): fp32 router logits, softmax top-k (renormalised with norm_topk_prob)
        logits = ops.gemm_nt_f32(xn, self.router)
        loads = torch.zeros(e + 1, dtype=torch.int32, device=xn.device)       # tokens per expert | per worker (one)
        weights, ids = ops.moe_top_k_softmax(logits, k, norm_topk_prob=c.norm_topk_prob, worker_load=loads[e:], expert_load=loads[:e])
        self.last_route = (ids, weights)                                        # (tests: the routing the step took)
        if self.route == "fused":
            return ops.moe_down(ops.moe_up(xn, self.w_up, ids), self.w_down, ids, weights)
        # grouped: the (token, slot) pairs sorted by expert on the device (stable), gate|up over the gathered tokens in sorted order,
        # down scattered back to pair order, then the weighted combine -- deterministic: every output row sums its k slots in order
        p = t * k
        pair = ops.arange_i32(p, xn.device)
        if t <= self.m_thres:
            # a few rows: one tile per (token, slot) pair straight from the routing ids, pair order throughout
            act = ops.moe_gemm_pairs(xn, self.w_up, ids, in_div=k, epilogue=ops.EPI_SILU_MUL)
            return ops.moe_sum_experts(ops.moe_gemm_pairs(act, self.w_down, ids), pair, weights)
        _, order = ops.sort_pairs_i32(ids.reshape(-1), pair, max_key=e)
        act = ops.moe_gemm_grouped(xn, self.w_up, loads[:e], order, p, in_div=k, epilogue=ops.EPI_SILU_MUL)
        down = ops.moe_gemm_grouped(act, self.w_down, loads[:e], order, p, out_scatter=True)
        return ops.moe_sum_experts(down, pair, weights)

    def ff_add(self, hidden, eps, act_buf=None):
        """hidden += moe(ln_ff(hidden)) in place (the residual add in T arithmetic, block.cpp:123-140)"""
        ops.element_add_scale(hidden, self.moe(ops.rmsnorm(hidden, self.ln_ff, eps)), 1.0, True, out=hidden)

    def ff_in(self, hidden, eps, out=None, normed=None):
        raise ops.ZLError("MoE layers have no gate|up projection of their own (ff_add runs the experts)")


ScoreResult = collections.namedtuple("ScoreResult", "logprobs lse greedy greedy_logit cu sums matches logits")


@dataclass
class DynBatchContext:
    """Per-step device state of a decode batch (model::DynBatchContext s_token / s_position /
    s_placement / s_len_buf, src/model/dyn_batch_context.h:29-200) + the RagBufferContext tables."""
    tokens: torch.Tensor        # (B) int32
    positions: torch.Tensor     # (B) int32
    placement: torch.Tensor     # (B) int32   slot of the new token in the task's KV buffer
    buf_lens: torch.Tensor      # (B) int32   allocated length of each task's buffer
    valid_lens: torch.Tensor    # (B) int32   visible keys = position + 1 (greedy / sampling decode)
    k_addrs: torch.Tensor       # (num_layers, B) int64 raw pointers
    v_addrs: torch.Tensor
    max_len_buf: int
    kv: List[torch.Tensor] = field(default_factory=list)  # owners: per task (layers, 2, len_buf, Hkv, D)
    # INT8 KV cache (KV_CACHE_DTYPE=int8, src/model/model_context.cpp:61-79): kv holds u8 codes, one fp32
    # scale per (slot, kv head) in kv_scales: per task (layers, 2, len_buf, Hkv)
    kv_quant: bool = False
    ks_addrs: Optional[torch.Tensor] = None
    vs_addrs: Optional[torch.Tensor] = None
    kv_scales: List[torch.Tensor] = field(default_factory=list)
    # host-side bound on the device-side bookkeeping (advance / zl_greedy_advance bump placement with no host round trip):
    # decode steps that still fit the tasks' buffers.  Eager steps raise when it is used up; a caller replaying a captured
    # step bounds its replays itself (the scatter kernels drop a row whose slot lies outside its buffer -- never a stray write)
    steps_left: int = 1 << 60
    unquant_kv: Dict[int, torch.Tensor] = field(default_factory=dict)   # INT8 cache: a chunked prompt's temporary fp16 K/V
    # LLaMA.verify: per len_q the row-expanded view of this context and the call's result buffers (built on first use, the view's
    # tables refilled from this context by every call)
    spec: Dict[int, tuple] = field(default_factory=dict)
    # a row-expanded view (LLaMA.verify): several "tasks" are rows of ONE task and share its buffers, so a row's attention reads K/V
    # that other rows of the same call write -- encode() must scatter every row before any row attends (never the launch that
    # scatters and attends at once)
    row_expanded: bool = False
    # LLaMA.admit / park: slot -> the KV rows the slot can ever use (prompt + clamped length limit + draft rows + 1 <= len_buf; 0 = parked).
    # Such a slot is kept inside its buffer by the device-side length stop, so it does not bound steps_left; a plain prefill of the
    # slot takes it out again
    slot_guard: Dict[int, int] = field(default_factory=dict)
    # slot -> (room, at): the host's bound of a slot that is NOT guarded -- a prompt encode left it `room` decode steps while steps_left
    # stood at `at`, so it has room - (at - steps_left) left now; admit / park take the minimum of these when a guarded slot replaces
    # the one that bounded steps_left.  A slot in neither table is bounded by steps_left as it stands
    slot_room: Dict[int, tuple] = field(default_factory=dict)
    # LLaMA.new_shared_prefixes: prefix buffers that slots read their first keys from instead of holding a copy (SharedPrefixes); a
    # context that has them decodes through zl_decode_attn_shared
    shared: Optional["SharedPrefixes"] = None


@dataclass
class SharedPrefixes:
    """The prefix table of a context (LLaMA.new_shared_prefixes; include/zhilight_amd.h, zl_decode_attn_shared, has the rule): G buffers
    of `rows` K/V rows for every layer, and per slot the prefix it reads its first keys from.  The host mirrors are what the admission
    calls check against; nothing but LLaMA.load_prefix / admit / admit_samples / park writes either side."""
    kv: List[torch.Tensor]      # owners: per prefix (layers, 2, rows, Hkv, D)
    k_addrs: torch.Tensor       # (layers, G) int64
    v_addrs: torch.Tensor
    prefix_of: torch.Tensor     # (B) int32, -1 = none
    prefix_lens: torch.Tensor   # (G) int32 valid rows
    prefix_caps: torch.Tensor   # (G) int32, all `rows`
    rows: int
    of_host: List[int] = field(default_factory=list)
    lens_host: List[int] = field(default_factory=list)

    def users(self, g):
        """the slots that read prefix g"""
        return [s for s, v in enumerate(self.of_host) if v == g]


# LLaMA.verify's result: the (B * len_q, vocab) logits of the step's rows, accepted (B) int32 drafts per task, tokens (B, len_q) int32 =
# the accepted drafts and the model's own next token, -1 behind them (fed back as drafts, a -1 is simply a draft that is never accepted)
SpecResult = collections.namedtuple("SpecResult", "logits accepted tokens")


@dataclass
class LookupState:
    """The device-resident state of the prompt-lookup drafter (LLaMA.new_lookup / step_lookup; ops.lookup_draft states the rule):
    every task's token history -- what it has consumed plus its pending ctx.tokens entry -- and the drafts of the next step."""
    history: torch.Tensor       # (B, cap) int32; row b holds its first min(hist_lens[b], cap) ids
    hist_lens: torch.Tensor     # (B) int32   tokens fed so far; beyond cap the task has overflowed and drafts nothing (-1) from then on
    drafts: torch.Tensor        # (B, K) int32   the next verify step's drafts, -1 = none
    match: torch.Tensor         # (B, 2) int32   (n, start) of the n-gram the drafts follow, (0, -1) = no match
    k: int
    max_ngram: int
    min_ngram: int


@dataclass
class SamplerState:
    """The device-resident state of LLaMA.step_sample and of verify / step_lookup(sampler=...) (LLaMA.new_sampler builds it;
    ops.sample_advance and ops.spec_sample_accept state the rules): per-task sampling parameters, each task's generator -- its seed
    and the number of uniforms it has drawn = tokens it has emitted -- and the last step's results."""
    temperature: torch.Tensor   # (B) fp32    <= 0: greedy
    top_k: torch.Tensor         # (B) int32   <= 0 or >= vocab: off
    top_p: torch.Tensor         # (B) fp32    in [0, 1]
    seeds: torch.Tensor         # (B) int64   the Philox key of the task
    draws: torch.Tensor         # (B) int64   uniforms drawn so far = the Philox counter; bumped by the kernel
    logprobs: torch.Tensor      # (B) fp32    the last step's picks' tempered log-probabilities: of the token now pending in ctx.tokens
    u: torch.Tensor             # (B) fp32    the last step_sample's uniforms
    # verify(sampler=...): the last speculative step's rows, (B, len_q) fp32 each -- the log-probabilities of the emitted tokens (NaN
    # behind the bonus token) and the uniform of every row.  Allocated by the first eager call per len_q (row_bufs keeps them)
    row_logprobs: Optional[torch.Tensor] = None
    row_u: Optional[torch.Tensor] = None
    row_bufs: Optional[Dict[int, tuple]] = None
    # penalties inside the sampling launch (new_sampler's repetition_penalty / presence_penalty): all three set, or all None = off.
    # seen: the bitmap of the ids each task has emitted (and the caller's penalty_tokens); the sampling kernels read and extend it
    repetition_penalty: Optional[torch.Tensor] = None   # (B) fp32
    presence_penalty: Optional[torch.Tensor] = None     # (B) fp32    != 0: takes precedence over the factor
    seen: Optional[torch.Tensor] = None                 # (B, ceil(vocab / 32)) int32: token i = bit i & 31 of word i >> 5
    # logit bias inside the sampling launch (new_sampler's logit_bias): ops.logit_bias_pack's four tensors, or all None = off
    bias_ids: Optional[torch.Tensor] = None             # (B, ld) int32     a task's first bias_cnt ids, ascending
    bias_vals: Optional[torch.Tensor] = None            # (B, ld) fp32
    bias_cnt: Optional[torch.Tensor] = None             # (B) int32
    bias_bits: Optional[torch.Tensor] = None            # (B, ceil(vocab / 32)) int32: the ids as a bitmap, seen's layout
    # top-N alternatives of every pick (new_sampler's top_logprobs = N): top_n = 0 and the tensors None = off.  top_ids / top_logprobs:
    # step_sample's, the alternatives of the step that produced the token now pending in ctx.tokens.  row_top_ids / row_top_logprobs
    # (B, len_q, N): verify(sampler=...)'s, beside row_logprobs and allocated the same way (row_top_bufs keeps them); the pending
    # token's alternatives after a speculative step are row (b, accepted[b])
    top_n: int = 0
    top_ids: Optional[torch.Tensor] = None              # (B, N) int32      -1 behind the vocabulary's end / on a row without a distribution
    top_logprobs: Optional[torch.Tensor] = None         # (B, N) fp32       NaN there
    row_top_ids: Optional[torch.Tensor] = None
    row_top_logprobs: Optional[torch.Tensor] = None
    row_top_bufs: Optional[Dict[int, tuple]] = None
    # the token automaton inside the sampling launch (new_sampler's grammar_states / grammar_edges / grammar): fsm = the five tables of
    # ops.sample_advance's fsm=, allocated ONCE at that capacity and shared by the tasks -- LLaMA.load_grammar copies automata into their
    # free tail, the pointers never change -- and fsm_state, a task's state in them (outside [0, capacity): unconstrained).  None = off
    fsm: Optional[tuple] = None                         # mask (S, ceil(vocab / 32)), default (S), exc_off (S + 1), exc_tok (E), exc_next (E) int32
    fsm_state: Optional[torch.Tensor] = None            # (B) int32
    fsm_used: Optional[list] = None                     # [states, exception entries] that load_grammar has given out
    row_states: Optional[torch.Tensor] = None           # verify(sampler=...): (B, len_q) int32, the state behind every row's pick
    row_state_bufs: Optional[Dict[int, torch.Tensor]] = None

    def opts(self):
        """the bias / top-N / automaton keyword arguments of ops.sample_advance: none at all with the options off"""
        kw = {}
        if self.bias_ids is not None:
            kw["bias"] = (self.bias_ids, self.bias_vals, self.bias_cnt, self.bias_bits)
        if self.top_n:
            kw.update(top_n=self.top_n, top_ids=self.top_ids, top_logprobs=self.top_logprobs)
        if self.fsm is not None:
            kw.update(fsm=self.fsm, fsm_state=self.fsm_state)
        return kw


@dataclass
class StopState:
    """The device-resident stop conditions of a batch (LLaMA.new_stopper builds it; ops.stop_advance states the rule) for the stop= keyword
    of step_greedy / step_sample / verify / step_lookup: per-task parameters, what each task has emitted since the state was made, and
    the last step's outcome."""
    stop_ids: torch.Tensor      # (B, n_ids <= 16) int32        ids that end the task, -1 = unused
    stop_seqs: torch.Tensor     # (B, n_seqs <= 8, ld <= 16) int32   multi-token stop sequences
    seq_lens: torch.Tensor      # (B, n_seqs) int32             0 = unused
    max_new: torch.Tensor       # (B) int32                     the task's length limit, <= 0 = none
    gen_lens: torch.Tensor      # (B) int32                     ids emitted since the state was made
    tail: torch.Tensor          # (B, 15) int32                 the last 15 of them (seeded with the pending token), -1 = none yet
    last_token: torch.Tensor    # (B) int32                     the last emitted id: what a finished task re-feeds
    finished: torch.Tensor      # (B) int32                     0 = live, 1 = stop id, 2 = stop sequence, 3 = length
    emit_lens: torch.Tensor     # (B) int32                     ids each task emitted in the last step (0: finished before it)
    live: torch.Tensor          # (1) int32                     tasks still live after the last step

    def advance(self, new_tokens, ctx, accepted=None, next_tokens=None):
        """the one launch behind a step's advance / accept launch"""
        ops.stop_advance(self.stop_ids, self.stop_seqs, self.seq_lens, self.max_new, self.gen_lens, self.tail, self.last_token, self.finished,
                         new_tokens, accepted=accepted, next_tokens=next_tokens, tokens=ctx.tokens, positions=ctx.positions,
                         placement=ctx.placement, valid_lens=ctx.valid_lens, emit_lens=self.emit_lens, live=self.live)


class _PromptRows:
    """The rows of one prompt-encode call -- one task's piece, or the pieces of several tasks back to back -- as the layer loop, the
    K/V scatter, the attention and the tail see them.  Built once per call, and the only place that knows whether the call has one
    task or several: one task uploads no table (positions from torch.arange, scatter tables that are slices of the context's, the
    pick straight into ctx.tokens); several tasks gather theirs in one int32 and one int64 upload.
      tasks, lens, cu, ends      host lists: task indices, rows per task, row offsets (n + 1), pos0 + rows per task
      tokens, pos, labels_dev    int32 per row on the device (labels_dev: LLaMA.score only)
      placement, buf_lens, len_q, k_rows / v_rows / ks_rows / vs_rows    the scatter: one "task" of len_q = s rows, or one per row with
                                 len_q = 1; (layers, scatter tasks) pointer tables, ks_rows / vs_rows None on an fp16 cache
      route, att_pos0s, len_bufs, len_bufs_dev, plan    what the attention reads (LLaMA._prompt_scatter_attend lists the routes): per
                                 task the first key row's position and the buffer rows (host; device for the mask form), and the
                                 varlen plan (head size 128: several tasks, or the "q8" route)
      k_tab / v_tab / ks_tab / vs_tab, kv, kv_off    its buffers: (layers, n) pointer tables ("cache", "temp", "q8"); the one task's
                                 (layers, 2, rows, Hkv, D) tensor for the one-task launch ("cache", "temp"); "own": the byte offset
                                 of each task's first row in the call's k / v
      last_rows, tasks_dev, ends_dev    the tail: int64 row of each task's last token, its index, int32 end -- None for one task
      hist_lens, hist_lens_dev   "hist" (prompts behind a shared prefix, `prefixes` = a prefix index or None per task): the rows each task
                                 reads from its prefix buffer (= its pos0, 0 for None); k_tab / v_tab point to the prefix buffers"""
    labels_dev = ks_rows = vs_rows = len_bufs_dev = plan = k_tab = v_tab = ks_tab = vs_tab = kv = kv_off = None
    last_rows = tasks_dev = ends_dev = hist_lens = hist_lens_dev = None

    @classmethod
    def of(cls, model, ctx, tasks, prompts, pos0s, q8_history=False, labels=None, prefixes=None):
        if len(tasks) == 1 and prefixes is None:
            return cls.one(model, ctx, tasks[0], prompts[0], pos0s[0], q8_history, labels)
        return cls.many(model, ctx, tasks, prompts, pos0s, q8_history, labels, prefixes)

    @classmethod
    def one(cls, model, ctx, task, prompt, pos0, q8_history=False, labels=None, pos=None):
        """one task's piece at pos0; pos: its positions where the caller holds them already (a part of a dual-stream piece).  The
        labels are the one upload of this form"""
        r, c, dev = cls(), model.cfg, model.device
        s = int(prompt.numel())
        r.tasks, r.lens, r.cu, r.ends = [task], [s], [0, s], [pos0 + s]
        r.tokens = prompt.to(device=dev, dtype=torch.int32).contiguous()
        r.pos = torch.arange(pos0, pos0 + s, dtype=torch.int32, device=dev) if pos is None else pos
        if labels is not None:
            r.labels_dev = torch.tensor(labels, dtype=torch.int32).to(dev)
        col = slice(task, task + 1)
        r.placement, r.buf_lens, r.len_q = r.pos.view(1, s), ctx.buf_lens[col], s
        r.k_rows, r.v_rows = ctx.k_addrs[:, col], ctx.v_addrs[:, col]
        if ctx.kv_quant:
            r.ks_rows, r.vs_rows = ctx.ks_addrs[:, col], ctx.vs_addrs[:, col]
        unq = ctx.unquant_kv.get(task) if ctx.kv_quant and not q8_history else None
        if q8_history:
            r.route, r.att_pos0s, r.len_bufs = "q8", [pos0], [ctx.max_len_buf]
            r.k_tab, r.v_tab, r.ks_tab, r.vs_tab = r.k_rows, r.v_rows, r.ks_rows, r.vs_rows
            r.plan = ops.prefill_varlen_plan(r.lens, r.att_pos0s, r.len_bufs, dev)
        elif unq is not None:
            r.route, r.att_pos0s, r.len_bufs, r.kv = "temp", [pos0], [unq.shape[2]], unq
            r.len_bufs_dev = torch.tensor(r.len_bufs, dtype=torch.int32, device=dev)
            tab = ops.make_ptr_table([unq[li, j] for li in range(unq.shape[0]) for j in (0, 1)]).view(-1, 2)
            r.k_tab, r.v_tab = tab[:, 0:1], tab[:, 1:2]
        elif ctx.kv_quant:
            r.route, r.att_pos0s, r.len_bufs = "own", [0], [s]
            if c.dim_head != 128:                         # the mask form's tables; the one-task launch takes k3 / v3 themselves
                r.len_bufs_dev = torch.tensor(r.len_bufs, dtype=torch.int32, device=dev)
                r.kv_off = torch.zeros(1, dtype=torch.int64, device=dev)
        else:
            r.route, r.att_pos0s, r.len_bufs, r.kv = "cache", [pos0], [ctx.max_len_buf], ctx.kv[task]
            r.len_bufs_dev, r.k_tab, r.v_tab = r.buf_lens, r.k_rows, r.v_rows
        return r

    @classmethod
    def many(cls, model, ctx, tasks, prompts, pos0s, q8_history=False, labels=None, prefixes=None):
        """the pieces of n tasks back to back: the K/V scatter takes one "task" per row, the attention one table entry per task"""
        r, c, dev = cls(), model.cfg, model.device
        n = len(tasks)
        lens = [int(pr.numel()) for pr in prompts]
        total = sum(lens)
        cu = [0]
        for s in lens:
            cu.append(cu[-1] + s)
        r.tasks, r.lens, r.cu, r.ends = tasks, lens, cu, [p0 + s for p0, s in zip(pos0s, lens)]
        r.tokens = torch.cat([pr.to(device=dev, dtype=torch.int32).reshape(-1) for pr in prompts])
        # one upload of the call's int32 and one of its int64 tables
        ints = torch.tensor([p0 + i for p0, s in zip(pos0s, lens) for i in range(s)] + r.ends + lens + (labels or []),
                            dtype=torch.int32).to(dev)
        r.pos, r.ends_dev, lens_dev = ints[:total], ints[total:total + n], ints[total + n:total + 2 * n]
        if labels is not None:
            r.labels_dev = ints[total + 2 * n:]
        row_bytes = c.num_kv_heads * c.dim_head * c.torch_dtype.itemsize
        idx = torch.tensor(tasks + [t for t, s in zip(tasks, lens) for _ in range(s)] + [e - 1 for e in cu[1:]] +
                           [a * row_bytes for a in cu[:-1]], dtype=torch.int64).to(dev)
        r.tasks_dev, rows_dev, r.last_rows = idx[:n], idx[n:n + total], idx[n + total:2 * n + total]
        r.placement, r.len_q = r.pos.view(total, 1), 1
        r.buf_lens = ctx.buf_lens.index_select(0, rows_dev)
        r.k_rows, r.v_rows = ctx.k_addrs.index_select(1, rows_dev), ctx.v_addrs.index_select(1, rows_dev)
        if ctx.kv_quant:
            r.ks_rows, r.vs_rows = ctx.ks_addrs.index_select(1, rows_dev), ctx.vs_addrs.index_select(1, rows_dev)
        if prefixes is not None:                          # history from the tasks' prefix buffers, own rows from the concatenated k / v
            sh, g_n = ctx.shared, ctx.shared.prefix_lens.numel()
            r.route, r.att_pos0s, r.len_bufs = "hist", pos0s, [ctx.max_len_buf] * n
            r.hist_lens = [0 if g is None else p0 for g, p0 in zip(prefixes, pos0s)]
            r.hist_lens_dev = torch.tensor(r.hist_lens, dtype=torch.int32).to(dev)
            pick = torch.tensor([g_n if g is None else g for g in prefixes], dtype=torch.int64).to(dev)     # column G: a null pointer
            null = torch.zeros((sh.k_addrs.shape[0], 1), dtype=torch.int64, device=dev)
            r.k_tab, r.v_tab = (torch.cat([t, null], dim=1).index_select(1, pick) for t in (sh.k_addrs, sh.v_addrs))
        elif q8_history:                                  # history from the cache, own rows from the concatenated k / v
            r.route, r.att_pos0s, r.len_bufs = "q8", pos0s, [ctx.max_len_buf] * n
            r.k_tab, r.v_tab = ctx.k_addrs.index_select(1, r.tasks_dev), ctx.v_addrs.index_select(1, r.tasks_dev)
            r.ks_tab, r.vs_tab = ctx.ks_addrs.index_select(1, r.tasks_dev), ctx.vs_addrs.index_select(1, r.tasks_dev)
        elif ctx.kv_quant:                                # attention over the call's own rows (fresh prompts only)
            r.route, r.att_pos0s, r.len_bufs, r.len_bufs_dev = "own", [0] * n, lens, lens_dev
            r.kv_off = idx[2 * n + total:]
        else:
            r.route, r.att_pos0s, r.len_bufs = "cache", pos0s, [ctx.max_len_buf] * n
            r.k_tab, r.v_tab = ctx.k_addrs.index_select(1, r.tasks_dev), ctx.v_addrs.index_select(1, r.tasks_dev)
            r.len_bufs_dev = ctx.buf_lens.index_select(0, r.tasks_dev)
        if c.dim_head == 128:
            r.plan = ops.prefill_varlen_plan(lens, r.att_pos0s, r.len_bufs, dev)
        return r

    def att_tables(self, li, k3, v3):
        """layer li's K / V pointer tables, one entry per task; "own": they point into the concatenated k3 / v3"""
        if self.route == "own":
            return self.kv_off + k3.data_ptr(), self.kv_off + v3.data_ptr()
        return self.k_tab[li], self.v_tab[li]


@dataclass(frozen=True)
class _DecodeRoute:
    """What every layer of one decode step launches: decided once per call by LLaMA._decode_route, switched on by the three stages of
    encode's layer body (DESIGN 4 "One route, one layer body" has the condition and the ZL_* switch of every value)."""
    qkv: str                    # "w4" zl_w4a16_qkv_rope_scatter | "w8" layernorm_quant + w8a8_qkv_rope_scatter | "plain" project_qkv + rope / scatter
    norm: Optional[str]         # "w4" only, its RMSNorm: "fused" in registers | "launch" of its own | "row_ss" from statistics the projections hand on
    attn: str                   # "hook" | "shared" (zl_decode_attn_shared: a context with a prefix table) | "la" | "splits" (records left for attn_out) | "mqa" | "valu_fused" (rope / scatter included) | "quant"
    out: str                    # "merge" w4_attn_out_merge | "merge_gate_up" w4_attn_out_gate_up, "merge" where it declines | "linear" attn_out_add
    skip_attn: bool             # bench.py's legs, resolved against the route: stage 2 is left out ...
    skip_proj: bool             # ... stages 1 and 3 are
    workspace: torch.Tensor     # the split attention's partials
    scale: float
    merge_plan: Optional[tuple]
    la: Optional[tuple]         # (workspace, split, half)
    stats: Optional[torch.Tensor]   # (2, B, dim_model / 16) fp32
    hook: object                # LLaMA.verify's attend_rows, carried to the attention stage; never switched on


class LLaMA:
    """model::LLaMA (src/model/llama.cpp:11-165) restricted to the dynamic-batch decode step."""
    moe = False                 # any MoEEncoderLayer (set by __init__)

    def __init__(self, cfg: ModelConfig, quant: QuantConfig, device="cuda:0", tp=None):
        """tp: parallel.TPGroup (rank, size, process group) for tensor parallelism over the GPUs of a node -- W4 route
        only; heads, kv heads, dim_ff and the vocabulary must divide by the TP degree."""
        if cfg.scale_depth > 0 and quant.quant_type != 0:
            raise ops.ZLError("scale_depth (MiniCPM residual scaling) is only wired into the unquantised layer stack")
        if quant.quant_type not in (0, MXFP4) and cfg.torch_dtype != torch.float16:
            raise ops.ZLError("the W4A16 / int8 routes are fp16 (q_gemm_k_major.cu:989 asserts half)")
        self.cfg, self.quant, self.device = cfg, quant, torch.device(device)
        # QuantType (zhilight/quant.py:8-19): 0 NoQuant, 2 AutoInt8, 5 GPTQ (AWQ-as-exllama rides on 5); 11 MXFP4 is this project's
        layer_cls = {0: DenseEncoderLayer, 2: Int8EncoderLayer, MXFP4: Mxfp4EncoderLayer}.get(quant.quant_type, EncoderLayer)
        self.tp = tp if tp is not None and tp.size > 1 else None
        self.full_cfg = cfg
        self.moe = any(cfg.is_moe_layer(i) for i in range(cfg.num_layers))
        if quant.quant_type == MXFP4:
            if quant.group_size != 32:
                raise ops.ZLError("MXFP4: the block size is 32")
            if self.tp:
                raise ops.ZLError("MXFP4 models: tensor parallelism is not supported")
            if self.moe:
                raise ops.ZLError("MXFP4 models: MoE layers are not supported")
        if self.moe:
            # MoE models: the W4 route without tensor / expert parallelism (MoEEncoderLayer refuses the rest); the dense layers a
            # model lists in mlp_only_layers stay EncoderLayer
            if self.tp:
                raise ops.ZLError("MoE models: tensor parallelism is not supported")
            if layer_cls is not EncoderLayer:
                raise ops.ZLError("MoE models: GPTQ W4A16 checkpoints only")
            self.layers = [MoEEncoderLayer(cfg, quant, i) if cfg.is_moe_layer(i) else EncoderLayer(cfg, quant, i)
                           for i in range(cfg.num_layers)]
        elif self.tp:
            if layer_cls is not EncoderLayer:
                raise ops.ZLError("tensor parallelism is wired into the W4A16 layer stack only")
            t = self.tp.size
            # fewer kv heads than ranks: with ATTN_KV_REP_TP=1 the reference gives rank r kv head r / (TP / Hkv), i.e.
            # groups of TP / Hkv ranks hold (and cache) the same kv head (src/nn/attention/attention.cpp:126-134)
            kv_part = None
            if (cfg.num_kv_heads < t and t % cfg.num_kv_heads == 0 and int(os.environ.get("ATTN_KV_REP_TP", "0")) > 0):
                kv_part = (self.tp.rank // (t // cfg.num_kv_heads), cfg.num_kv_heads)
            if cfg.num_heads % t or (kv_part is None and cfg.num_kv_heads % t) or cfg.dim_ff % t or cfg.vocab_size % t:
                raise ops.ZLError("heads, kv heads, dim_ff and vocab_size must be divisible by the TP degree "
                                  "(fewer kv heads than ranks: ATTN_KV_REP_TP=1)")
            import dataclasses
            cfg = dataclasses.replace(cfg, num_heads=cfg.num_heads // t, num_kv_heads=1 if kv_part else cfg.num_kv_heads // t,
                                      dim_ff=cfg.dim_ff // t)
            self.cfg = cfg                            # the LOCAL geometry drives buffers, KV and kernels
            self.layers = [EncoderLayer(cfg, quant, i, self.tp) for i in range(cfg.num_layers)]
            for l in self.layers:
                l.kv_part = kv_part
        else:
            self.layers = [layer_cls(cfg, quant, i) for i in range(cfg.num_layers)]
        self.token_embedding = self.output_layernorm = self.lm_head = None
        self._bufs = {}

    # ---- weights -------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], hf_names=True):
        sd = {hf_name_to_internal(k) if hf_names else k: v for k, v in state_dict.items()}
        dev = self.device
        dt = self.cfg.torch_dtype
        self.token_embedding = _dev_t(sd["llama.token_embedding.weight"], dev).to(dt).contiguous()
        self.output_layernorm = _dev_t(sd["llama.output_layernorm.weight"], dev).to(dt).contiguous()
        self.lm_head = self.token_embedding if self.cfg.tie_lm_head else _dev_t(sd["llama.lm_head.weight"], dev).to(dt).contiguous()
        if self.tp:                                   # vocab-parallel projection (embedding.cu:353-385)
            v = self.cfg.vocab_size // self.tp.size
            self.lm_head = self.lm_head[self.tp.rank * v:(self.tp.rank + 1) * v].contiguous()
        for i, layer in enumerate(self.layers):
            layer.load_state_dict(sd, f"llama.layers.{i}", dev)
            layer.q_norm = layer.k_norm = None
            if self.cfg.qk_norm:
                layer.q_norm, layer.k_norm = (self._qk_norm_weight(sd[f"llama.layers.{i}.attn.{n}_norm.weight"], n)
                                              for n in ("q", "k"))
        return self

    def _qk_norm_weight(self, w, which):
        """q_norm / k_norm weights (attention.cpp:110-117): (dim_head) for "head"; (heads * dim_head) for "multi_head", of
        which a TP rank keeps its heads' rows (replicated kv heads: the one head it holds)."""
        c, fc = self.cfg, self.full_cfg
        t = _dev_t(w, self.device).to(c.torch_dtype).reshape(-1)
        if c.qk_norm == "head":
            if t.numel() != c.dim_head:
                raise ops.ZLError("q_norm / k_norm weight must have dim_head elements")
            return t.contiguous()
        full = fc.num_heads if which == "q" else fc.num_kv_heads
        loc = c.num_heads if which == "q" else c.num_kv_heads
        if t.numel() != full * c.dim_head:
            raise ops.ZLError("q_norm / k_norm weight must have heads * dim_head elements")
        if self.tp:
            kv_part = getattr(self.layers[0], "kv_part", None)
            first = kv_part[0] if (which == "k" and kv_part) else self.tp.rank * loc
            t = t.view(full, c.dim_head)[first:first + loc]
        return t.contiguous()

    def apply_qk_norm(self, layer, qkv):
        """q_norm / k_norm in place on the q and k windows of the fused projection, before the rotation
        (attention.cpp:864-876 fused, :904-915 separate projections)."""
        c = self.cfg
        if not c.qk_norm:
            return
        hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
        mode = 0 if c.qk_norm == "head" else 1
        ops.head_norm(qkv[:, :hd], layer.q_norm, c.num_heads, c.dim_head, c.eps, mode, out=qkv[:, :hd])
        ops.head_norm(qkv[:, hd:hd + kvd], layer.k_norm, c.num_kv_heads, c.dim_head, c.eps, mode, out=qkv[:, hd:hd + kvd])

    def init_random(self, seed=0):
        gen = torch.Generator(device=self.device).manual_seed(seed)
        c, dev = self.cfg, self.device
        dt = c.torch_dtype
        self.token_embedding = (torch.randn(c.vocab_size, c.dim_model, device=dev, generator=gen) * 0.5).to(dt)
        self.output_layernorm = torch.ones(c.dim_model, dtype=dt, device=dev)
        vloc = c.vocab_size // self.tp.size if self.tp else c.vocab_size
        self.lm_head = self.token_embedding if (c.tie_lm_head and not self.tp) else (torch.randn(vloc, c.dim_model, device=dev, generator=gen) * 0.02).to(dt)
        for layer in self.layers:
            layer.init_random(dev, gen)
            layer.q_norm = layer.k_norm = None
            if c.qk_norm:
                nq, nk = (c.dim_head, c.dim_head) if c.qk_norm == "head" else (c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head)
                layer.q_norm = (1.0 + 0.1 * torch.randn(nq, device=dev, generator=gen)).to(dt)
                layer.k_norm = (1.0 + 0.1 * torch.randn(nk, device=dev, generator=gen)).to(dt)
        return self

    def init_synthetic(self, seed=0, sink=None):
        """Synthetic GPTQ checkpoint of this geometry with SURVEY 8(d)'s recipe -- the one tests/synth.py::gptq_hf and
        tests/test_gpu_model.py::_hf_state draw on the host -- generated on the device and taken through the REAL load path
        (EncoderLayer.load_state_dict: shuffle, zero + 1, transposes, fusion, ZLW4M packing), one layer at a time:
          qweight (K/8, N) int32 from uniform nibbles 0..15; qzeros (K/G, N/8) int32 from nibbles 0..14 stored as zero - 1;
          scales (K/G, N) fp16 = |N(0,1)| * (0.5 / sqrt(K)) / 4 + 1e-4 (activations stay O(1): _hf_state's magnitude, = 8(d)'s
          0.02 / 8 at K = 4096 within 25 %); norm weights 1 + 0.1 N(0,1); embedding uniform integers / 128, lm_head uniform
          integers * 0.05 / 64 (tests/test_gpu_fullgeom.py::_state).
        W4 route, no tensor parallelism (bench.py's TP leg keeps init_random: every rank would have to draw the full matrices).
        sink(name -> device tensor): called with every checkpoint tensor under the reference's parameter names ("llama.layers.3.attn.
        project_q.qweight", "llama.token_embedding.weight", ...) before it is consumed -- tools/bench_boundary.py hands the same
        checkpoint to the reference's own model::LLaMA."""
        c, dev, q = self.cfg, self.device, self.quant
        if self.tp or not all(isinstance(l, EncoderLayer) for l in self.layers) or q.act_order or q.awq:
            raise ops.ZLError("init_synthetic: the plain GPTQ layer stack")
        gen = torch.Generator(device=dev).manual_seed(seed)
        g = q.group_size
        i64 = dict(dtype=torch.int64, device=dev, generator=gen)

        def pack8(nib, dim):                            # 8 nibbles along `dim` (stride 8) -> one int32 word, nibble j at bits 4 j
            word = torch.zeros_like(nib.select(dim, 0).unsqueeze(dim).expand(*[s // 8 if i == dim else s for i, s in enumerate(nib.shape)])).contiguous()
            for j in range(8):
                word |= (nib[j::8] if dim == 0 else nib[:, j::8]) << (4 * j)
            return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)

        def lin(sd, name, din, dout):
            sd[name + ".qweight"] = pack8(torch.randint(0, 16, (din, dout), **i64), 0)
            sd[name + ".qzeros"] = pack8(torch.randint(0, 15, (din // g, dout), **i64), 1)
            sd[name + ".scales"] = (torch.randn(din // g, dout, device=dev, generator=gen).abs() * ((0.5 / math.sqrt(din)) / 4) + 1e-4).to(torch.float16)
        hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
        dt = c.torch_dtype
        for i, layer in enumerate(self.layers):
            pfx = f"llama.layers.{i}"
            sd = {pfx + ".ln_attn.weight": (1 + 0.1 * torch.randn(c.dim_model, device=dev, generator=gen)).to(torch.float16),
                  pfx + ".ln_ff.weight": (1 + 0.1 * torch.randn(c.dim_model, device=dev, generator=gen)).to(torch.float16)}
            lin(sd, pfx + ".attn.project_q", c.dim_model, hd)
            lin(sd, pfx + ".attn.project_k", c.dim_model, kvd)
            lin(sd, pfx + ".attn.project_v", c.dim_model, kvd)
            lin(sd, pfx + ".attn.attn_out", hd, c.dim_model)
            if isinstance(layer, MoEEncoderLayer):
                # the experts with the same recipe at their own shapes; router rows N(0,1) / sqrt(dim_model): logits O(1), so
                # the top-k picks spread over the experts
                for e in range(c.moe_num_experts):
                    lin(sd, f"{pfx}.ff.experts.{e}.w_in", c.dim_model, c.moe_intermediate_size)
                    lin(sd, f"{pfx}.ff.experts.{e}.w_gated", c.dim_model, c.moe_intermediate_size)
                    lin(sd, f"{pfx}.ff.experts.{e}.w_out", c.moe_intermediate_size, c.dim_model)
                sd[pfx + ".ff.router.weight"] = (torch.randn(c.moe_num_experts, c.dim_model, device=dev, generator=gen)
                                                 / math.sqrt(c.dim_model)).to(torch.float16)
            else:
                lin(sd, pfx + ".ff.w_in", c.dim_model, c.dim_ff)
                lin(sd, pfx + ".ff.w_gated", c.dim_model, c.dim_ff)
                lin(sd, pfx + ".ff.w_out", c.dim_ff, c.dim_model)
            if c.qk_norm == "head":
                for n in ("q", "k"):
                    sd[f"{pfx}.attn.{n}_norm.weight"] = (1 + 0.1 * torch.randn(c.dim_head, device=dev, generator=gen)).to(torch.float16)
            if sink is not None:
                sink(sd)
            layer.load_state_dict(sd, pfx, dev)
            layer.q_norm = layer.k_norm = None
            if c.qk_norm == "head":
                layer.q_norm, layer.k_norm = (self._qk_norm_weight(sd[f"{pfx}.attn.{n}_norm.weight"], n) for n in ("q", "k"))
            del sd
        u8 = lambda: torch.randint(-127, 128, (c.vocab_size, c.dim_model), dtype=torch.int8, device=dev, generator=gen)
        self.token_embedding = (u8().to(dt) * (1.0 / 128)).contiguous()
        self.output_layernorm = (1 + 0.1 * torch.randn(c.dim_model, device=dev, generator=gen)).to(dt)
        self.lm_head = self.token_embedding if c.tie_lm_head else (u8().to(dt) * (0.05 / 64)).contiguous()
        if sink is not None:
            sink({"llama.token_embedding.weight": self.token_embedding, "llama.output_layernorm.weight": self.output_layernorm,
                  "llama.lm_head.weight": self.lm_head})
        return self

    # ---- KV state ------------------------------------------------------------------------------
    def new_context(self, batch: int, len_buf: int, start_pos: int, fill_random=False, kv_cache_dtype=None) -> DynBatchContext:
        """`batch` tasks whose first `start_pos` tokens are already in the KV buffers (zero- or
        random-filled here: the reference zero-fills, src/kvcache/transformer_buffer.cu:290-330).
        kv_cache_dtype: None (the model dtype) or "int8"; default from the reference's switch, the environment
        variable KV_CACHE_DTYPE (src/model/model_context.cpp:61-79)."""
        c, dev = self.cfg, self.device
        if kv_cache_dtype is None:
            kv_cache_dtype = os.environ.get("KV_CACHE_DTYPE") or None
        if kv_cache_dtype not in (None, "int8"):
            raise ops.ZLError(f"Unsupported dtype: {kv_cache_dtype}")
        kv, kv_scales = [], []
        for _ in range(batch):
            shape = (c.num_layers, 2, len_buf, c.num_kv_heads, c.dim_head)
            if kv_cache_dtype == "int8":
                t = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev) if fill_random else \
                    torch.full(shape, 128, dtype=torch.uint8, device=dev)
                sc = torch.rand(shape[:-1], dtype=torch.float32, device=dev) * 0.03 + 0.005 if fill_random else \
                    torch.zeros(shape[:-1], dtype=torch.float32, device=dev)
                kv_scales.append(sc)
            else:
                t = torch.randn(shape, dtype=c.torch_dtype, device=dev) if fill_random else torch.zeros(shape, dtype=c.torch_dtype, device=dev)
            kv.append(t)
        quant_kw = {}
        if kv_cache_dtype == "int8":
            quant_kw = dict(
                kv_quant=True, kv_scales=kv_scales,
                ks_addrs=torch.tensor([[t[l, 0].data_ptr() for t in kv_scales] for l in range(c.num_layers)], dtype=torch.int64, device=dev),
                vs_addrs=torch.tensor([[t[l, 1].data_ptr() for t in kv_scales] for l in range(c.num_layers)], dtype=torch.int64, device=dev))
        k_addrs = torch.tensor([[t[l, 0].data_ptr() for t in kv] for l in range(c.num_layers)], dtype=torch.int64, device=dev)
        v_addrs = torch.tensor([[t[l, 1].data_ptr() for t in kv] for l in range(c.num_layers)], dtype=torch.int64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        return DynBatchContext(
            steps_left=len_buf - start_pos,
            tokens=torch.zeros(batch, **i32), positions=torch.full((batch,), start_pos, **i32),
            placement=torch.full((batch,), start_pos, **i32), buf_lens=torch.full((batch,), len_buf, **i32),
            valid_lens=torch.full((batch,), start_pos + 1, **i32), k_addrs=k_addrs, v_addrs=v_addrs,
            max_len_buf=len_buf, kv=kv, **quant_kw)

    def new_shared_prefixes(self, ctx: DynBatchContext, count: int, rows: int) -> SharedPrefixes:
        """Give ctx `count` prefix buffers of `rows` K/V rows (every layer, the context's BSHD layout and element type) and the table
        that lets a slot say "my first P keys live over there" (SharedPrefixes; zl_decode_attn_shared has the rule).  From here on the
        context's decode steps run the two-segment attention; a slot whose prefix_of is -1 -- all of them now -- attends over its own
        buffer as before.  Refused: an INT8 cache, tensor parallelism, a head size other than 128 or more than 16 query heads per kv
        head, a row-expanded view, a context that has a table already."""
        c, dev = self.cfg, self.device
        count, rows = int(count), int(rows)
        if ctx.kv_quant or self.tp or c.dim_head != 128 or c.num_heads // c.num_kv_heads > 16 or ctx.row_expanded:
            raise ops.ZLError("new_shared_prefixes: not on an INT8 KV cache, under tensor parallelism, for a row-expanded view, nor for head "
                              "sizes other than 128 / more than 16 query heads per kv head")
        if ctx.shared is not None or count < 1 or rows < 1:
            raise ops.ZLError("new_shared_prefixes: one table per context, of one buffer and one row at least")
        b = ctx.tokens.numel()
        kv = [torch.zeros((c.num_layers, 2, rows, c.num_kv_heads, c.dim_head), dtype=c.torch_dtype, device=dev) for _ in range(count)]
        i32 = dict(dtype=torch.int32, device=dev)
        ctx.shared = SharedPrefixes(
            kv=kv, rows=rows,
            k_addrs=torch.tensor([[t[l, 0].data_ptr() for t in kv] for l in range(c.num_layers)], dtype=torch.int64, device=dev),
            v_addrs=torch.tensor([[t[l, 1].data_ptr() for t in kv] for l in range(c.num_layers)], dtype=torch.int64, device=dev),
            prefix_of=torch.full((b,), -1, **i32), prefix_lens=torch.zeros(count, **i32), prefix_caps=torch.full((count,), rows, **i32),
            of_host=[-1] * b, lens_host=[0] * count)
        return ctx.shared

    def _load_prefixes(self, what, ctx: DynBatchContext, gs, token_lists):
        """encode token_lists[j] into prefix buffer gs[j], all in one pass through the existing prompt path: an auxiliary context whose
        task j's buffer IS prefix gs[j] -> the logits of every list's last row.  Checked before any launch: a table, distinct indices
        in range that no slot reads, 1 <= tokens <= rows."""
        sh = ctx.shared
        if sh is None:
            raise ops.ZLError(f"{what}: the context has no shared prefixes (LLaMA.new_shared_prefixes)")
        gs = [int(g) for g in gs]
        toks = [torch.as_tensor(t).reshape(-1) for t in token_lists]
        if not gs or len(set(gs)) != len(gs) or any(not 0 <= g < len(sh.kv) for g in gs):
            raise ops.ZLError(f"{what}: distinct prefix indices below {len(sh.kv)}")
        for g, t in zip(gs, toks):
            if not 1 <= t.numel() <= sh.rows:
                raise ops.ZLError(f"{what}: prefix {g}: {t.numel()} tokens, the buffer holds 1 .. {sh.rows}")
            if sh.users(g):
                raise ops.ZLError(f"{what}: prefix {g} is read by slots {sh.users(g)}")
        n, dev = len(gs), self.device
        i32 = dict(dtype=torch.int32, device=dev)
        cols = torch.tensor(gs, dtype=torch.int64, device=dev)
        aux = DynBatchContext(tokens=torch.zeros(n, **i32), positions=torch.zeros(n, **i32), placement=torch.zeros(n, **i32),
                              buf_lens=torch.full((n,), sh.rows, **i32), valid_lens=torch.ones(n, **i32),
                              k_addrs=sh.k_addrs.index_select(1, cols), v_addrs=sh.v_addrs.index_select(1, cols), max_len_buf=sh.rows,
                              kv=[sh.kv[g] for g in gs])
        r, hidden = self._prefill_rows(aux, list(range(n)), toks, [0] * n)
        last = hidden[-1:] if r.last_rows is None else hidden.index_select(0, r.last_rows)
        logits = self._prompt_logits_and_pick(last, aux.tokens)
        lens = [int(t.numel()) for t in toks]
        sh.prefix_lens.index_copy_(0, cols, torch.tensor(lens, dtype=torch.int32).to(dev))
        for g, s in zip(gs, lens):
            sh.lens_host[g] = s
        return logits

    def load_prefix(self, ctx: DynBatchContext, g: int, tokens):
        """Encode `tokens` into prefix buffer g of the context's table and set its length -> the logits of the last row (1, vocab).
        Refused while a slot reads the prefix."""
        return self._load_prefixes("load_prefix", ctx, [g], [tokens])

    def _set_prefix_of(self, ctx: DynBatchContext, slots, values):
        """prefix_of[slots[j]] = values[j] on the device (in place: a captured step reads the table) and in the host mirror"""
        sh = ctx.shared
        both = torch.tensor(list(slots) + list(values), dtype=torch.int64).to(self.device)
        sh.prefix_of.index_copy_(0, both[:len(slots)], both[len(slots):].to(torch.int32))
        for s, v in zip(slots, values):
            sh.of_host[s] = v

    def release_prefix(self, ctx: DynBatchContext, slots):
        """the slots read no prefix any more (prefix_of = -1): for slots that are about to be admitted anew"""
        if ctx.shared is not None:
            stale = [int(s) for s in slots if ctx.shared.of_host[int(s)] != -1]
            if stale:
                self._set_prefix_of(ctx, stale, [-1] * len(stale))

    def _buffers(self, b):
        if b not in self._bufs:
            c, dev = self.cfg, self.device
            f16 = dict(dtype=c.torch_dtype, device=dev)
            hd, kvd = c.num_heads * c.dim_head, c.num_kv_heads * c.dim_head
            self._bufs[b] = dict(
                hidden=torch.empty(b, c.dim_model, **f16), qkv=torch.empty(b, hd + 2 * kvd, **f16),
                q=torch.empty(b, hd, **f16), attn=torch.empty(b, hd, **f16), act=torch.empty(b, c.dim_ff, **f16),
                logits=torch.empty(b, c.vocab_size, **f16))
        return self._bufs[b]

    # ---- one decode step -----------------------------------------------------------------------
    def _decode_route(self, ctx: DynBatchContext, b, gemv_only, skip_gemv, attend_rows, workspace=None) -> _DecodeRoute:
        """The route of one decode step and its per-batch workspaces; refuses what encode cannot run before anything is launched.  Decided
        anew by every call: the ZL_* switches and the context (max_len_buf, kv_quant, row_expanded) change under a live model."""
        c = self.cfg
        if (attend_rows is not None or self.moe) and (gemv_only or skip_gemv):
            # the two legs split a step into "the four W4 projections" and the rest; an MoE layer's feed-forward is a router, a sort
            # and two grouped launches, which belong to neither side
            raise ops.ZLError("gemv_only / skip_gemv: " + ("not with an attention hook" if attend_rows is not None else "dense models only"))
        if ctx.steps_left <= 0 and not torch.cuda.is_current_stream_capturing():
            raise ops.ZLError("decode step past the end of the KV buffers (placement >= len_buf): grow the buffers first "
                              "(the reference asserts pos_buf < len_buf, ragged_buffer_kernel.cu:194-222)")
        sh = ctx.shared
        if sh is not None:
            # a context with a prefix table: the two-segment attention between the qkv stage and a plain attn_out projection -- no
            # merging prologue, no in-launch merge (their records know one segment).  Every other context is routed as before
            if attend_rows is not None:
                raise ops.ZLError("speculative rows (verify / step_lookup) over shared prefixes are not supported")
            if gemv_only or skip_gemv:
                raise ops.ZLError("gemv_only / skip_gemv: not on a context with shared prefixes")
            key = ("shared_ws", b, len(sh.kv), sh.rows, ctx.max_len_buf)
            if key not in self._bufs:
                self._bufs[key] = ops.decode_attn_shared_workspace(b, len(sh.kv), c.num_heads, c.num_kv_heads, c.dim_head, sh.rows,
                                                                   ctx.max_len_buf, self.device)
            workspace = self._bufs[key]
        if workspace is None:
            workspace = self._bufs.setdefault(("ws", b, ctx.max_len_buf),
                                              ops.decode_attn_workspace(b, 1, c.num_heads, c.dim_head, ctx.max_len_buf, self.device))
        env, first = os.environ.get, self.layers[0]
        mfma_attn = c.dim_head == 128 and c.num_heads // c.num_kv_heads <= 16 and env("ZL_ATTN_MFMA", "1") != "0"
        # qkv: the projection with rotary + KV scatter in its epilogue where it applies (zl_w4a16_qkv_rope_scatter; W8A8: the
        # streaming kernel with the scale-back fused as well), else project_qkv and a rope / scatter launch
        fuse_rope = mfma_attn and not ctx.kv_quant and not c.qk_norm and env("ZL_FUSE_QKV_ROPE", "1") != "0"
        qkv, norm = "plain", None
        if (fuse_rope and all(isinstance(l, EncoderLayer) and l.unfused is None and l.qkv.perm is None
                              and isinstance(l.qkv.weight, ops.W4MWeight) for l in self.layers)
                and ops.w4_qkv_rope_scatter_ok(b, c.dim_model, c.dim_head, norm=b <= max(8, _fused_norm_rows(first.qkv.weight)))):
            qkv = "w4"
        elif fuse_rope and b <= 32 and c.dim_head % 32 == 0 and all(isinstance(l, Int8EncoderLayer) and l._stream(b) for l in self.layers):
            qkv = "w8"
        # a few rows: the split merge of the decode attention rides in the attn_out projection's prologue (one launch less)
        merge_plan = None
        if qkv == "w4" and not self.tp and attend_rows is None and sh is None and env("ZL_ATTN_MERGE", "1") != "0" and all(l.attn_out.perm is None for l in self.layers):
            merge_plan = ops.attn_merge_plan(b, c.num_heads, c.num_kv_heads, c.dim_head, ctx.max_len_buf, first.attn_out.weight, c.torch_dtype)
        # the split merge INSIDE the attention launch (last-arriving workgroup of a (task, kv head) pair, zl_decode_attn_la) wherever
        # the step would otherwise run the two-launch path (split kernel + merge kernel): same records, same merge arithmetic, one
        # launch less per layer.  Batch 1 keeps the merge in attn_out's prologue: there the in-launch merge was measured 1.4 us per
        # layer SLOWER at the same split length and worse with finer splits (profiles/r05_attn_la_ab.txt).
        # ZL_ATTN_LA: auto (default) / 0 off / 1 everywhere; ZL_ATTN_LA_SPLIT = keys per split (multiple of 32, 0 = the two-launch
        # path's), ZL_ATTN_LA_HALF = 1 half-precision split records
        la, la_mode = None, env("ZL_ATTN_LA", _ATTN_LA_DEFAULT)
        if mfma_attn and not ctx.kv_quant and attend_rows is None and sh is None and (la_mode == "1" or (la_mode == "auto" and merge_plan is None)):
            la_split = int(env("ZL_ATTN_LA_SPLIT", "0") or 0)
            eff = la_split or ops.decode_attn_la_split_len(b, c.num_kv_heads, ctx.max_len_buf)
            if (ctx.max_len_buf + eff - 1) // eff <= 64:
                # one block per (batch, power-of-two bucket of the buffer length): records are addressed by the launch's own split
                # count, so a block sized for a longer buffer serves every shorter one; a captured graph keeps its block's address,
                # hence buckets instead of regrowing in place -- at most log2 blocks per batch, < 2 x the largest
                key = ("la_ws", b, 1 << max(10, (ctx.max_len_buf - 1).bit_length()))
                if key not in self._bufs:
                    self._bufs[key] = ops.decode_attn_la_workspace(b, c.num_heads, c.num_kv_heads, key[2], self.device)
                la = (self._bufs[key], la_split, env("ZL_ATTN_LA_HALF", "0") == "1" and c.torch_dtype == torch.float16)
                merge_plan = None
        # the rows' statistics travel with the residual stream (zl_w4_opts_t::row_ss / row_ss_out): attn_out and w_out leave per row
        # and 16-column tile the sum of squares of what they store, the normalising projections (qkv, gate|up) read those 256 numbers
        # per row instead of running -- or waiting for -- an RMSNorm pass over the rows: no stand-alone norm launch from 9 rows on, no
        # register-resident norm prologue below.  ZL_ROW_SS=0 off; ZL_ROW_SS_MIN_M: rows it starts at
        # (not with MoE layers: their feed-forward has no w_out to produce the statistics nor a gate|up projection to consume them)
        stats = None
        if (qkv == "w4" and (la is not None or attend_rows is not None or sh is not None) and not self.tp and not self.moe
                and env("ZL_ROW_SS", "1") != "0" and int(env("ZL_ROW_SS_MIN_M", "8")) <= b <= 32 and c.dim_model % 1024 == 0
                and all(l.attn_out.perm is None and l.w_out.perm is None and l.w_in_gated.perm is None for l in self.layers)
                and ops.w4_row_ss_routes(b, [first.attn_out.weight, first.w_out.weight],
                                         [(first.qkv.weight, True), (first.w_in_gated.weight, False)], self.device)):
            stats = self._bufs.get(("row_ss", b))
            if stats is None:
                stats = self._bufs[("row_ss", b)] = torch.empty((2, b, c.dim_model // 16), dtype=torch.float32, device=self.device)
        # attention split merge + attn_out + residual and ln_ff + gate|up + silu.mul in ONE launch (w4_engine.hip)
        # (off for MoE models: the fused launch ends in the dense gate|up projection)
        fuse_o_ff = (merge_plan is not None and merge_plan[2] and not self.moe and env("ZL_FUSE_O_GATEUP", "0") == "1" and ops.experimental_build()
                     and all(l.w_in_gated.perm is None and isinstance(l.w_in_gated.weight, ops.W4MWeight) for l in self.layers))
        # the two bench legs split the W4 route's step; the W8 route runs the whole step under either, the plain route under skip_gemv
        if gemv_only and qkv == "plain":
            raise ops.ZLError("gemv_only: the fused W4 decode route only")
        if skip_gemv and qkv == "w4" and la is None and merge_plan is None:
            raise ops.ZLError("skip_gemv: the fused W4 decode route with the merging attn_out projection only")
        if qkv == "w4":                                   # 9..32 rows without the statistics: a launch of its own, or the deferred norm (ZL_DEFER_NORM)
            norm = "row_ss" if stats is not None else "fused" if b <= max(8, _fused_norm_rows(first.qkv.weight)) else "launch"
        if sh is not None:
            attn = "shared"
        elif ctx.kv_quant or attend_rows is not None:
            attn = "quant" if ctx.kv_quant else "hook"
        elif la is not None or merge_plan is not None:
            attn = "la" if la is not None else "splits"
        else:                                             # never "valu_fused" for a row-expanded view: that launch orders a row's own K/V only
            attn = "mqa" if qkv != "plain" or mfma_attn or ctx.row_expanded else "valu_fused"
        return _DecodeRoute(qkv, norm, attn, "merge_gate_up" if fuse_o_ff else "merge" if merge_plan is not None else "linear", skip_attn=gemv_only and qkv == "w4" and not skip_gemv, skip_proj=skip_gemv and qkv == "w4",
                            workspace=workspace, scale=1.0 / math.sqrt(c.dim_head), merge_plan=merge_plan, la=la, stats=stats, hook=attend_rows)

    def encode(self, ctx: DynBatchContext, workspace=None, argmax_ws=None, gemv_only=False, skip_gemv=False, attend_rows=None):
        """LLaMA::encode for a pure decode ("search") batch: returns logits (B, vocab) fp16.  The route is decided once (_decode_route), then
        every layer runs three stages: qkv, attention, output + feed-forward.  gemv_only / skip_gemv (bench.py's legs, W4 route; DESIGN 4 has
        the others): ONLY the four quantised projections of every layer, on whatever the buffers hold, returns None / all BUT those.
        attend_rows (LLaMA.verify): ctx is a row-expanded view -- several rows of one task posed as tasks of the scatter -- and
        attend_rows(li, q, out, workspace) is layer li's attention over them, q / out (rows, H * D)."""
        c = self.cfg
        b = ctx.tokens.numel()
        r = self._decode_route(ctx, b, gemv_only, skip_gemv, attend_rows, workspace)
        bufs = self._buffers(b)
        rs = c.rope_scaling
        kind = rs.get("rope_type", rs.get("type")) if rs else None
        if gemv_only:
            hidden = bufs["hidden"]
            cos, sin = self._rope_tables(ctx.positions)
        elif kind in (None, "default", "llama3") and c.dim_head <= 256 and self.token_embedding.shape[0] == c.vocab_size:
            # token_embedding + RopePreparer in one launch (two independent ~4 us kernels, half of each a kernel boundary)
            l3 = None if kind != "llama3" else (rs["factor"], rs["low_freq_factor"], rs["high_freq_factor"], rs["original_max_position_embeddings"])
            hidden, cos, sin = ops.embedding_rope(ctx.tokens, self.token_embedding, c.scale_emb, ctx.positions, c.dim_head, c.rope_theta, True, l3)
        else:
            hidden = ops.embedding(ctx.tokens, self.token_embedding, c.scale_emb)  # token_embedding
            cos, sin = self._rope_tables(ctx.positions)                            # RopePreparer
        if r.out == "merge_gate_up":
            ops.engine_epoch_advance(self.device)
        trace = getattr(self, "trace_hidden", None)          # parity tests: the hidden rows entering every layer (eager runs only)
        for li, layer in enumerate(self.layers):
            if trace is not None and not torch.cuda.is_current_stream_capturing():
                trace.append(hidden.clone())
            if not r.skip_proj:
                self._decode_qkv(r, ctx, bufs, li, layer, hidden, cos, sin)
            if not r.skip_attn:
                self._decode_attend(r, ctx, bufs, li, cos, sin)
            if not r.skip_proj:
                self._decode_out_ff(r, ctx, bufs, li, layer, hidden)
        if gemv_only:
            return None
        self.last_hidden = hidden                      # (B, dim_model) before the output norm: the parity tests read it
        return self._logits(hidden, bufs["logits"], argmax_ws)

    def _decode_qkv(self, r, ctx, bufs, li, layer, hidden, cos, sin):
        """stage 1: hidden -> rotated q in bufs["q"], the rows' K / V in the cache ("valu_fused": unrotated bufs["qkv"])"""
        c = self.cfg
        slots, heads = (ctx.placement, ctx.buf_lens, ctx.k_addrs[li], ctx.v_addrs[li]), (c.num_heads, c.num_kv_heads, c.dim_head)
        if r.qkv == "w4":
            if r.norm == "row_ss" and li == 0:
                ops.row_ss(hidden, out=r.stats[0])          # (the embedding's rows: the only statistics no projection produced)
            own = r.norm != "launch"                        # the launch normalises: in registers, or from the statistics
            ops.w4_qkv_rope_scatter(hidden if own else ops.rmsnorm(hidden, layer.ln_attn, c.eps), layer.qkv.weight, cos, sin, *slots,
                                    *heads, bias=layer.qkv.bias, norm_weight=layer.ln_attn if own else None, norm_eps=c.eps,
                                    q_out=bufs["q"], row_ss=r.stats[0] if r.norm == "row_ss" else None)
        elif r.qkv == "w8":
            # layernorm_quant, then the streaming W8A8 kernel with scale-back + rotary + KV scatter fused
            _, xq, sx = ops.layernorm_quant(hidden, layer.ln_attn, c.eps)
            ops.w8a8_qkv_rope_scatter(xq, sx, layer.qkv.stream_weight(), cos, sin, *slots, *heads, q_out=bufs["q"])
        else:
            layer.project_qkv(hidden, c.eps, out=bufs["qkv"])
            self.apply_qk_norm(layer, bufs["qkv"])
            if r.attn == "quant":
                # attention.cpp:652-676 + :725-745: rotate, quantise the new K/V rows into the u8 cache (the attention reads codes)
                ops.rope_quant_scatter_decode(cos, sin, bufs["qkv"], *slots, ctx.ks_addrs[li], ctx.vs_addrs[li], *heads, q_out=bufs["q"])
            elif r.attn != "valu_fused":
                ops.rope_scatter_decode(cos, sin, bufs["qkv"], *slots, *heads, q_out=bufs["q"])

    def _decode_attend(self, r, ctx, bufs, li, cos, sin):
        """stage 2, the decode attention of layer li over the tasks' buffers: bufs["q"] -> bufs["attn"] (B, H * D); "splits": records in
        the workspace, which the attn_out projection merges; "valu_fused": from bufs["qkv"], with the rope / scatter"""
        c = self.cfg
        k, v, shape = ctx.k_addrs[li], ctx.v_addrs[li], (bufs["q"].shape[0], 1, c.num_heads, c.dim_head)
        if r.attn == "hook":
            r.hook(li, bufs["q"], bufs["attn"], r.workspace)
        elif r.attn == "shared":
            sh = ctx.shared
            ops.decode_attention_shared(bufs["q"].view(shape), ctx.buf_lens, k, v, ctx.valid_lens, sh.prefix_of, sh.prefix_lens, sh.prefix_caps,
                                        sh.k_addrs[li], sh.v_addrs[li], r.scale, sh.rows, ctx.max_len_buf, c.num_kv_heads,
                                        out=bufs["attn"].view(shape), workspace=r.workspace)
        elif r.attn == "la":
            ops.decode_attention_la(bufs["q"].view(shape), ctx.buf_lens, k, v, ctx.valid_lens, r.scale, ctx.max_len_buf, c.num_kv_heads,
                                    r.la[0], out=bufs["attn"].view(shape), split_len=r.la[1], half=r.la[2])
        elif r.attn == "splits":
            ops.decode_attention_splits(bufs["q"].view(shape[0], c.num_heads, c.dim_head), ctx.buf_lens, k, v, ctx.valid_lens, r.scale,
                                        ctx.max_len_buf, c.num_kv_heads, r.workspace)
        elif r.attn == "mqa":
            # the matrix-core decode attention (attention.hip: k_decode_attn_mfma; 11.0 / 18.7 / 39.8 us vs 11.9 / 24.0 / 49.7 us for
            # the fused VALU kernel at batch 1 / 8 / 32)
            ops.multi_query_attention_rag_buffer(bufs["q"].view(shape), ctx.buf_lens, k, v, None, r.scale, ctx.max_len_buf, c.num_kv_heads,
                                                 valid_lens=ctx.valid_lens, out=bufs["attn"].view(shape), workspace=r.workspace)
        elif r.attn == "quant":
            ops.multi_query_attention_rag_buffer_quant(bufs["q"].view(shape), ctx.buf_lens, k, v, ctx.ks_addrs[li], ctx.vs_addrs[li], None,
                                                       r.scale, ctx.max_len_buf, c.num_kv_heads, valid_lens=ctx.valid_lens,
                                                       out=bufs["attn"].view(shape), workspace=r.workspace)
        else:
            ops.decode_attention_fused(cos, sin, bufs["qkv"], ctx.placement, ctx.buf_lens, ctx.valid_lens, k, v, c.num_heads, c.num_kv_heads,
                                       c.dim_head, r.scale, ctx.max_len_buf, out=bufs["attn"], workspace=r.workspace)

    def _decode_out_ff(self, r, ctx, bufs, li, layer, hidden):
        """stage 3: hidden += attn_out(attention), hidden += feed-forward(hidden)"""
        if r.norm == "row_ss":                              # the three projections hand the rows' statistics on
            layer.attn_out.forward(bufs["attn"], residual=hidden, out=hidden, epilogue=ops.EPI_RESIDUAL, row_ss_out=r.stats[1])
            ops.w4_linear(hidden, layer.w_in_gated.weight, bias=layer.w_in_gated.bias, out=bufs["act"], norm_weight=layer.ln_ff,
                          norm_eps=self.cfg.eps, epilogue=ops.EPI_SILU_MUL, row_ss=r.stats[1])
            layer.w_out.forward(bufs["act"], residual=hidden, out=hidden, epilogue=ops.EPI_RESIDUAL, row_ss_out=r.stats[0])
            return
        if r.out == "linear":
            layer.attn_out_add(bufs["attn"], hidden)
        elif r.out == "merge_gate_up" and ops.w4_attn_out_gate_up(r.workspace, ctx.buf_lens, ctx.valid_lens, r.merge_plan, bufs["q"].shape[0],
                                                                   layer.attn_out.weight, hidden, layer.w_in_gated.weight, layer.ln_ff, self.cfg.eps,
                                                                   bufs["act"], li, bias_o=layer.attn_out.bias, bias_ff=layer.w_in_gated.bias):
            layer.w_out.forward(bufs["act"], residual=hidden, out=hidden, epilogue=ops.EPI_RESIDUAL)
            return
        else:
            ops.w4_attn_out_merge(r.workspace, ctx.buf_lens, ctx.valid_lens, r.merge_plan, bufs["q"].shape[0], layer.attn_out.weight,
                                  bias=layer.attn_out.bias, residual=hidden, out=hidden, epilogue=ops.EPI_RESIDUAL)
        layer.ff_add(hidden, self.cfg.eps, bufs["act"])

    def _logits(self, hidden, out=None, argmax_ws=None):
        """output_layernorm + lm_head (get_logits, src/model/llama.cpp:150-165).  MiniCPM divides the normalised
        row by dim_model / dim_model_base inside the norm (ln_after_enc's scale, llama.cpp:13-21)."""
        c = self.cfg
        rows = hidden.shape[0]
        if self.tp:                                   # local vocabulary slice, then all-gather of the logits
            part = ops.gemm_nt_small_m(hidden, self.lm_head, norm_weight=self.output_layernorm, norm_eps=c.eps) if rows <= 4 else \
                ops.gemm_nt(ops.rmsnorm(hidden, self.output_layernorm, c.eps), self.lm_head)
            full = self.tp.all_gather_columns(part)
            if out is not None:
                out.copy_(full)
                return out
            return full
        ln_scale = (c.dim_model / c.dim_model_base) if c.dim_model_base > 0 else 1.0
        if (rows > 4 and argmax_ws is None and c.dim_model % 128 == 0) or ln_scale != 1.0:
            xn = ops.rmsnorm(hidden, self.output_layernorm, c.eps, ln_scale)
            if rows > 4 and argmax_ws is None and c.dim_model % 128 == 0:
                # more rows than the streaming GEMV takes per pass: the MFMA GEMM; up to 32 rows (decode batches) on the ZLD16M copy of
                # the matrix -- packed on first use, OUTSIDE stream capture (run a step eagerly before capturing it, as bench.py does)
                if rows <= 32 and os.environ.get("ZL_LM_HEAD_PACKED", "1") != "0":
                    if getattr(self, "_lm_head_m", None) is None and not torch.cuda.is_current_stream_capturing():
                        self._lm_head_m = ops.DenseMWeight(self.lm_head)
                    if getattr(self, "_lm_head_m", None) is not None:
                        return ops.gemm_nt_packed(xn, self._lm_head_m, out=out)
                return ops.gemm_nt(xn, self.lm_head, out=out)
            return ops.gemm_nt_small_m(xn, self.lm_head, out=out, argmax_ws=argmax_ws)
        return ops.gemm_nt_small_m(hidden, self.lm_head, out=out, norm_weight=self.output_layernorm, norm_eps=c.eps,
                                   argmax_ws=argmax_ws)

    def _rope_tables(self, pos):
        """cos / sin (rows, dim_head) fp32 of one forward's positions: RopePreparer (rope_preparer.cu:49-160) for plain and
        llama3 frequencies, the RotaryEmbedding variants "dynamic" (NTK) and "yarn" (rotary_embedding.cu:19-61, 398-553)
        as tables for the same fused rotation kernels."""
        c = self.cfg
        rs = c.rope_scaling
        kind = rs.get("rope_type", rs.get("type")) if rs else None
        if kind in (None, "default"):
            return ops.rope_cos_sin(pos, c.dim_head, c.rope_theta, True, None)
        if kind == "llama3":
            return ops.rope_cos_sin(pos, c.dim_head, c.rope_theta, True,
                                    (rs["factor"], rs["low_freq_factor"], rs["high_freq_factor"], rs["original_max_position_embeddings"]))
        if kind == "dynamic":
            if c.max_position_embeddings <= 0:
                raise ops.ZLError("dynamic rope scaling needs max_position_embeddings")
            # the reference reads ONE sequence length per forward: the position of the call's last row (rotary_embedding.cu:36,
            # gridDim.x - 1 of the flat (tokens, dim) view) -- for a decode batch that is the last task's position
            seq_len = pos[-1:].expand(pos.numel()).contiguous()
            return ops.rope_cos_sin_dynamic(pos, c.dim_head, c.rope_theta, rs["factor"], c.max_position_embeddings, seq_len)
        if kind == "yarn":
            deepseek = c.model_type in ("deepseek_v2", "deepseek_v3")
            low, high, msc = ops.yarn_params(c.rope_theta, c.dim_head, rs["original_max_position_embeddings"], rs["factor"],
                                             int(rs.get("beta_fast", 32)), int(rs.get("beta_slow", 1)),
                                             rs.get("attn_factor", 1.0), deepseek, rs.get("mscale", 0.0),
                                             rs.get("mscale_all_dim", 0.0))
            return ops.rope_cos_sin_yarn(pos, c.dim_head, c.rope_theta, rs["factor"], low, high, msc)
        raise ops.ZLError(f"rope_scaling type {kind!r} is not supported (supported: llama3, dynamic, yarn)")

    def _prefill_mask(self, s, len_buf, pos0=0):
        """causal mask + workspace for head sizes the MFMA prefill kernel does not cover"""
        key = ("prefill", s, len_buf, pos0)
        if key not in self._bufs:
            c, dev = self.cfg, self.device
            mask = torch.tril(torch.ones(s, len_buf, dtype=torch.int8, device=dev), diagonal=pos0).contiguous()
            ws = ops.decode_attn_workspace(1, s, c.num_heads, c.dim_head, len_buf, dev)
            self._bufs[key] = (mask, ws)
        return self._bufs[key]

    def prefill(self, ctx: DynBatchContext, task: int, prompt: torch.Tensor, chunk: int = 0, kv_history=None):
        """Prompt encode, optionally in chunks of `chunk` tokens (the reference's chunked prefill,
        src/generator/batch_generator.cpp:1048-1084: a long prompt enters the batch piece by piece, each piece
        attending to the KV of the pieces before it).
        kv_history (INT8 KV cache only; an fp16 cache has one route and ignores it) chooses what a later piece reads for the
        pieces before it:
          None      the reference's preferred branch (attention.cpp:497-509): the prompt's UNquantised K/V rows, kept for every
                    layer in a temporary (layers, 2, S, Hkv, D) buffer for the duration of the call;
          "cache"   the reference's fall-back (attention.cpp:510-516, "de-quantize prompt kv cache"): the cache itself, dequantised
                    inside the attention kernel (ops.prefill_attention_varlen_q8) -- no temporary of any kind.  Earlier pieces
                    are seen through their codes, so the logits differ from the default route's by the cache's quantisation
                    noise; the cache contents differ accordingly from the second piece on."""
        q8_history = self._check_kv_history(ctx, kv_history)
        s = int(prompt.numel())
        if chunk <= 0 or chunk >= s:
            return self._encode_prompt(ctx, task, prompt, 0)
        self._check_prompt_piece("prefill", ctx, task, s, 0, True)
        if ctx.kv_quant and not q8_history:
            # INT8 KV cache: the prompt keeps attending to its UNquantised K/V rows across the chunks, held in temporary
            # buffers for the duration of the prompt (dyn_batch->unquant_key_buf, attention.cpp:497-510) while the codes go
            # to the cache; the decode steps that follow read the cache
            c = self.cfg
            ctx.unquant_kv[task] = torch.zeros((c.num_layers, 2, (s + 63) // 64 * 64, c.num_kv_heads, c.dim_head),
                                               dtype=c.torch_dtype, device=self.device)
        try:
            for p0 in range(0, s, chunk):
                logits = self._encode_prompt(ctx, task, prompt[p0:p0 + chunk], p0, q8_history)
        finally:
            ctx.unquant_kv.pop(task, None)
        return logits

    def _check_kv_history(self, ctx: DynBatchContext, kv_history):
        """the kv_history keyword of prefill / prefill_batch: None or "cache"; "cache" on an INT8 context needs head size 128 (the
        mask-form attention of other head sizes reads a chunk's own rows as codes: another result).  Raises before any launch;
        returns whether the call reads its history from the INT8 cache."""
        if kv_history not in (None, "cache"):
            raise ops.ZLError(f"kv_history: None or 'cache', not {kv_history!r}")
        if kv_history == "cache" and ctx.kv_quant and self.cfg.dim_head != 128:
            raise ops.ZLError("kv_history='cache' on an INT8 KV cache needs head size 128")
        return bool(ctx.kv_quant and kv_history == "cache")

    def _check_prompt_piece(self, what, ctx: DynBatchContext, task, s, pos0, history_readable, behind_prefix=False):
        """the checks of one task's piece (s rows at pos0), before any launch: it fits the task's buffers, a continued piece
        into an INT8 cache has something to read its history from -- the prompt's temporaries or kv_history="cache" --, and a
        continued piece does not go to a slot that reads a shared prefix (its own buffer holds nothing below the prefix's length;
        behind_prefix: admit(prefixes=), whose attention reads the prefix buffer)."""
        if s < 1 or pos0 < 0 or pos0 + s + 1 > ctx.max_len_buf:
            raise ops.ZLError(f"{what}: prompt of task {task} ({s} tokens at {pos0}) does not fit the task's KV buffer")
        if pos0 > 0 and not behind_prefix and ctx.shared is not None and 0 <= task < len(ctx.shared.of_host) and ctx.shared.of_host[task] != -1:
            raise ops.ZLError(f"{what}: task {task} reads a shared prefix: a continued prompt piece would attend over own rows that were "
                              "never written (admit(prefixes=) encodes a prompt behind a prefix)")
        if ctx.kv_quant and pos0 != 0 and not history_readable:
            # a later piece without the prompt's temporary unquantised buffers (prefill(chunk=...) keeps them): the reference
            # falls back to de-quantising the cache there ("WARNING: de-quantize prompt kv cache!", attention.cpp:511-516)
            raise ops.ZLError(f"{what}: a continued prompt into the INT8 KV cache goes through LLaMA.prefill(chunk=...) "
                              "or kv_history='cache'")

    def _encode_prompt(self, ctx: DynBatchContext, task: int, prompt: torch.Tensor, pos0: int, q8_history=False):
        """The "encode part" of a task (LLaMA::encode with len_q = prompt length for one task:
        src/model/llama.cpp:75-165, Attention::impl::NormalImpl::dynamic_batch_forward encode branch,
        src/nn/attention/attention.cpp:846-964 / attn_encode_group :442-622): runs the piece through the layers, fills the
        task's KV buffers at slots pos0 .. pos0 + S - 1, leaves the task ready for decode steps (tokens <- greedy first token,
        positions = placement = pos0 + S, valid_lens = pos0 + S + 1) and returns the logits of the last row (1, vocab).
        LLaMA::encode's switch (src/model/llama.cpp:102-110): with DUAL_STREAM=1, more than one TP rank and more
        than DUAL_STREAM_THRESHOLD (1024) tokens in the piece, the layers run as dual_stream_encode."""
        self._check_prompt_piece("prefill", ctx, task, int(prompt.numel()), pos0,
                                 q8_history or ctx.unquant_kv.get(task) is not None)
        if (self.tp and int(os.environ.get("DUAL_STREAM", "0")) > 0 and not ctx.kv_quant
                and int(prompt.numel()) > int(os.environ.get("DUAL_STREAM_THRESHOLD", "1024"))):
            return self._prefill_dual_stream(ctx, task, prompt, pos0)
        return self._prompt_tail(ctx, *self._prefill_rows(ctx, [task], [prompt], [pos0], q8_history))

    def _prefill_dual_stream(self, ctx: DynBatchContext, task: int, prompt: torch.Tensor, pos0: int):
        """EncoderLayer::impl::dual_stream_encode (src/nn/block/block.cpp:205-441) on two HIP streams: the piece is
        cut in DUAL_STREAM_NUM_SPLIT (2) parts of round_up(ceil(S / 2), 16) rows; every row-parallel partial output
        (attn_out, w_out) is all-reduced on a second, higher-priority stream while the main stream computes the other
        part, so the xGMI transfer of one half hides behind the GEMMs / attention of the other.  Part k of a layer
        starts with add_fuse_ln (layernorm.cu:227-302: c = T(hidden + reduced), norm of the fp32 sum) once its own
        reduce has landed; the later part attends to the earlier part's K/V through the cache, like a prefill chunk:
        each part is a one-task fp16-cache piece (_PromptRows.one) at pos0 + a.
        Ordering is stream events only (main -> reduce before the collective, reduce -> main before the add); the
        partial stays referenced until the main stream has consumed it, so no allocator hand-over is needed."""
        c, dev = self.cfg, self.device
        s = int(prompt.numel())
        num_split = max(1, int(os.environ.get("DUAL_STREAM_NUM_SPLIT", "2")))
        round_up = max(1, int(os.environ.get("DUAL_STREAM_SPLIT_ROUND_UP", "16")))
        part = -(-(-(-s // num_split)) // round_up) * round_up
        bounds = [(a, min(a + part, s)) for a in range(0, s, part)]
        tokens = prompt.to(device=dev, dtype=torch.int32).contiguous()
        pos = torch.arange(pos0, pos0 + s, dtype=torch.int32, device=dev)
        parts = [_PromptRows.one(self, ctx, task, tokens[a:b], pos0 + a, pos=pos[a:b]) for a, b in bounds]
        hidden_all = ops.embedding(tokens, self.token_embedding, c.scale_emb)
        cos, sin = self._rope_tables(pos)
        main = torch.cuda.current_stream(dev)
        if "reduce_stream" not in self._bufs:
            self._bufs["reduce_stream"] = torch.cuda.Stream(device=dev, priority=int(os.environ.get("DUAL_STREAM_PRIORITY", "-1")))
        red = self._bufs["reduce_stream"]
        main_ev = [torch.cuda.Event() for _ in bounds]
        done_ev = [torch.cuda.Event() for _ in bounds]
        hidden = [hidden_all[a:b] for a, b in bounds]
        pending = [None] * len(bounds)

        def reduce_async(k, partial):
            main_ev[k].record(main)
            red.wait_event(main_ev[k])
            with torch.cuda.stream(red):
                self.tp.all_reduce_sum(partial)
                done_ev[k].record(red)
            pending[k] = partial

        def reduced(k):
            partial, pending[k] = pending[k], None
            main.wait_event(done_ev[k])
            return partial

        for li, layer in enumerate(self.layers):
            for k, (a, b) in enumerate(bounds):
                n = b - a
                if li == 0:
                    xn = ops.rmsnorm(hidden[k], layer.ln_attn, c.eps)
                else:
                    xn, hidden[k] = ops.rmsnorm(hidden[k], layer.ln_attn, c.eps, x2=reduced(k))
                qkv = layer.project_qkv(None, c.eps, normed=xn)
                self.apply_qk_norm(layer, qkv)
                q, kr, v = ops.rope_qk_cache(cos[a:b], sin[a:b], qkv, c.num_heads, c.num_kv_heads, c.dim_head, True)
                att = self._prompt_scatter_attend(parts[k], li, q.view(n, c.num_heads, c.dim_head),
                                                  kr.view(n, c.num_kv_heads, c.dim_head), v.view(n, c.num_kv_heads, c.dim_head))
                reduce_async(k, layer.row_partial(layer.attn_out, att.view(n, -1)))
            for k in range(len(bounds)):
                xn, hidden[k] = ops.rmsnorm(hidden[k], layer.ln_ff, c.eps, x2=reduced(k))
                reduce_async(k, layer.row_partial(layer.w_out, layer.ff_in(None, c.eps, normed=xn)))
        for k in range(len(bounds)):
            hidden[k] = ops.element_add_scale(hidden[k], reduced(k), 1.0, True)
        self.dual_stream_runs = getattr(self, "dual_stream_runs", 0) + 1
        return self._prompt_tail(ctx, parts[-1], hidden[-1])        # the last part ends where the piece ends

    def prefill_batch(self, ctx: DynBatchContext, tasks, prompts, pos0=None, kv_history=None):
        """Prompt encode of several tasks in ONE pass through the layers (LLaMA::encode with the prompt rows of every task of the
        step in each linear, src/model/llama.cpp:75-165; attention as one varlen launch where attn_encode_group loops over the
        tasks, src/nn/attention/attention.cpp:442-562).  prompts[j] (1-D int tensor, lengths may differ) goes to the distinct
        task tasks[j]; pos0[j] (default 0) > 0 continues a prompt whose rows 0 .. pos0[j] - 1 are already in the task's buffers.
        Returns the logits of each task's last prompt row (len(tasks), vocab) and leaves every task as prefill() does: the greedy
        first token in ctx.tokens, positions = placement = pos0 + s, valid_lens = pos0 + s + 1, steps_left bounded.
        INT8 KV cache: fresh prompts only by default (a continued prompt raises ZLError: chunked prompts go through
        prefill(chunk=...)).  kv_history="cache" accepts pos0[j] > 0 there -- a second turn, a cached prefix, batched chunks; fresh
        and continued tasks may be mixed: the call's rows are quantised into the cache as always, and the attention is one
        ops.prefill_attention_varlen_q8 launch per layer, which reads rows below pos0[j] from the cache (dequantised in the kernel:
        the reference's fall-back arithmetic, attention.cpp:510-516) and the call's own rows unquantised, with no temporary.  Head
        size 128 only; on an fp16 cache the keyword changes nothing; any other value raises ZLError.
        Head sizes other than 128: batched linears, attention per task through the mask form.  Tensor parallelism: single
        stream, the all-reduces run over the summed rows; DUAL_STREAM does not apply to a batched call.  dynamic (NTK) rope
        takes the call's last row as its sequence length, as the reference does for any forward.  Duplicate or out-of-range
        tasks, empty prompts and prompts that do not fit the buffers raise ZLError before any launch."""
        tasks, pos0, q8_history = self._check_prompt_batch("prefill_batch", ctx, tasks, prompts, pos0, kv_history)
        return self._prompt_tail(ctx, *self._prefill_rows(ctx, tasks, prompts, pos0, q8_history))

    def _check_prompt_batch(self, what, ctx: DynBatchContext, tasks, prompts, pos0, kv_history, behind_prefix=False):
        """the argument checks of prefill_batch / score, before any launch -> (tasks, pos0 as int lists, q8_history)"""
        q8_history = self._check_kv_history(ctx, kv_history)
        tasks = [int(t) for t in tasks]
        n = len(tasks)
        pos0 = [0] * n if pos0 is None else [int(p) for p in pos0]
        if n < 1 or len(prompts) != n or len(pos0) != n:
            raise ops.ZLError(f"{what}: one prompt and one pos0 per task")
        if len(set(tasks)) != n or any(t < 0 or t >= ctx.tokens.numel() for t in tasks):
            raise ops.ZLError(f"{what}: tasks must be distinct indices of the batch")
        for t, pr, p0 in zip(tasks, prompts, pos0):
            self._check_prompt_piece(what, ctx, t, int(pr.numel()), p0, q8_history, behind_prefix)
        return tasks, pos0, q8_history

    def new_prefix_cache(self, ctx: DynBatchContext, num_blocks, block_size=128, max_prefix=4096):
        """A prompt prefix cache (prefix_cache.PrefixCache) for contexts like ctx: a pool of num_blocks blocks of block_size
        tokens, every layer's K and V, in the context's element type -- model-dtype rows, or for kv_cache_dtype="int8" a u8 code
        plane and an fp32 scale plane -- and the index over it; at most max_prefix tokens of a prompt are cached.  The defaults
        are the reference's CACHE_BLOCK_SIZE and CACHE_MAX_PREFIX (src/generator/prefix_cache.hpp).  The cache serves contexts of
        this kind on this device, on the stream current now (PrefixCache has the rule)."""
        from .prefix_cache import PrefixCache
        c = self.cfg
        if int(num_blocks) < 1 or int(block_size) < 1 or int(max_prefix) < 0:
            raise ops.ZLError("new_prefix_cache: num_blocks >= 1, block_size >= 1, max_prefix >= 0")
        return PrefixCache(self.device, c.num_layers, c.num_kv_heads, c.dim_head, c.torch_dtype, ctx.kv_quant, num_blocks, block_size,
                           max_prefix)

    def prefill_cached(self, ctx: DynBatchContext, cache, tasks, prompts, kv_history=None):
        """prefill_batch through a prefix cache (the reference's scheduler with enable_prompt_caching, batch_generator.cpp:626-648,
        1033-1045) -> (logits, matched): matched[j] tokens of prompts[j] -- a multiple of cache.block_size, or 0 -- came from the
        cache and only the rest was encoded.  In order: every prompt is matched against the index; ONE ops.kv_blocks_copy launch
        loads all tasks' matched blocks into their buffers (two on an INT8 cache: codes, scales); prefill_batch(ctx, tasks,
        remainders, pos0=matched, kv_history=kv_history) encodes what is left -- at least one token per task, so logits (n, vocab)
        and the context are exactly prefill_batch's; ONE save launch (two for INT8) copies every full block of the prompts that
        the cache does not hold yet into the pool, after which they enter the index.  A block common to two tasks of the call is
        saved once, from the first of them; when the pool is full the least recently used blocks go, never one this call matched
        or reserved, and a prompt's blocks are saved only as far as the pool has room.
        A cached block is identified by ALL the tokens up to its end (prefix_cache.py), so the loaded rows are the rows this
        prompt would have computed: bit for bit where the prompt kernels are reproducible at the shape.
        Arguments are prefill_batch's (without pos0: the prompts are whole) and so are its checks; the cache must fit ctx
        (PrefixCache.fits).  An INT8 context needs kv_history="cache" and head size 128 -- a continued prompt has no other route
        there -- whether or not anything matches.  Tensor parallelism is not supported.  All of this raises ZLError before any
        launch and before the index changes.  Prompts are read on the host to be matched: give host tensors (device prompts cost a
        synchronising copy, as in score)."""
        if self.tp:
            raise ops.ZLError("prefill_cached: tensor parallelism is not supported")
        tasks, _, _ = self._check_prompt_batch("prefill_cached", ctx, tasks, prompts, None, kv_history)
        if ctx.kv_quant and (kv_history != "cache" or self.cfg.dim_head != 128):
            raise ops.ZLError("prefill_cached: an INT8 KV cache needs kv_history='cache' and head size 128")
        c = self.cfg
        why = cache.fits(ctx)
        if why is None and (cache.layers, cache.hkv, cache.dim_head, cache.dtype) != (c.num_layers, c.num_kv_heads, c.dim_head, c.torch_dtype):
            why = "the cache was built for another geometry (layers, KV heads, head size or element type)"
        if why is not None:
            raise ops.ZLError(f"prefill_cached: {why}")
        index, bs = cache.index, cache.block_size
        toks = [pr.reshape(-1).tolist() for pr in prompts]
        chains = [index.match(t) for t in toks]
        matched = [len(ch) * bs for ch in chains]
        cache.load(ctx, [(t, i * bs, pb) for t, ch in zip(tasks, chains) for i, pb in enumerate(ch)])
        logits = self.prefill_batch(ctx, tasks, [pr.reshape(-1)[m:] for pr, m in zip(prompts, matched)], pos0=matched, kv_history=kv_history)
        keep, new, desc = {pb for ch in chains for pb in ch}, [], []
        try:
            for t, tk in zip(tasks, toks):
                pairs = index.reserve(tk, keep)
                keep.update(pb for _, pb in pairs)
                new += [pb for _, pb in pairs]
                desc += [(t, i * bs, pb) for i, pb in pairs]
            cache.save(ctx, desc)
        except Exception:
            index.abort(new)
            raise
        index.commit(new)
        return logits, matched

    def score(self, ctx: DynBatchContext, tasks, prompts, pos0=None, labels=None, kv_history=None):
        """prefill_batch that also scores EVERY prompt row against the lm_head (LLaMA::calc_log_prob / calc_greedy_match,
        src/model/llama.cpp:194-244, over nn::log_prob_raw / greedy_match_raw, src/nn/functions/cross_entropy.cu:7-69, 358-403):
        same arguments, checks, refusals and effects as prefill_batch -- the same layer loop, then output_layernorm over all rows,
        ONE ops.lm_head_score launch pair that never stores the (rows, vocab) logits, then prefill_batch's own lm_head and pick
        on the last rows, so the context ends exactly as after prefill_batch.
        labels None: next-token labels (row r of task j is labelled prompts[j][r + 1], the last row is not scored); else one
        int sequence per task of its prompt's length, -100 = not scored (calc_log_prob's `label`).  Labels outside the vocabulary
        raise ZLError before any launch.  Prompts and labels are read on the host to build the labels: give host tensors (device
        prompts work as in prefill_batch but cost a synchronising copy here).
        Returns ScoreResult: logprobs / lse / greedy / greedy_logit (device tensors over the summed rows, task after task; the
        logits are the values the prompt GEMM would store, rounded once to the model dtype), cu (host row offsets per task),
        sums (n,) fp32 = per-task sum of logprobs over the scored rows (the negative of log_prob_raw's first value), matches (n,)
        bool = every scored row's greedy equals its label, logits (n, vocab) of the last rows as prefill_batch returns them.
        sums and matches are formed on the device, without a host synchronisation.  Unlike the reference's calc_greedy_match,
        no label value is exempt (it skips rows whose target is token 7) and ties go to the LOWEST index (it takes the highest).
        Tensor parallelism is not supported."""
        if self.tp:
            raise ops.ZLError("score: tensor parallelism is not supported")
        tasks, pos0, q8_history = self._check_prompt_batch("score", ctx, tasks, prompts, pos0, kv_history)
        labels = ops.score_labels(prompts, labels)
        if any(l != ops.SCORE_IGNORE and not 0 <= l < self.cfg.vocab_size for l in labels):
            raise ops.ZLError("score: a label lies outside the vocabulary")
        r, hidden = self._prefill_rows(ctx, tasks, prompts, pos0, q8_history, labels)
        scored = self._score_rows(hidden, r.labels_dev, r.lens, r.last_rows)
        return scored._replace(logits=self._prompt_tail(ctx, r, hidden))

    def _score_rows(self, hidden, labels_dev, lens, last_rows=None):
        """output_layernorm over all rows + the fused lm_head scoring; per-task sums / matches on the device"""
        c = self.cfg
        ln_scale = (c.dim_model / c.dim_model_base) if c.dim_model_base > 0 else 1.0
        xn = ops.rmsnorm(hidden, self.output_layernorm, c.eps, ln_scale)
        if c.dim_model % 128 == 0:
            r = ops.lm_head_score(xn, self.lm_head, labels_dev)
        else:
            r = ops.lm_head_score_unfused(xn, self.lm_head, labels_dev)
        miss = ((r.greedy != labels_dev) & (labels_dev != ops.SCORE_IGNORE)).float()
        cu = [0]
        for s in lens:
            cu.append(cu[-1] + s)
        if last_rows is None:
            sums, matches = r.logprob.sum().view(1), (miss.sum() == 0).view(1)
        else:
            # per-task sums as differences of ONE float64 running sum at the tasks' last rows (ignored rows hold 0; the running sum
            # of at most 2^31 fp32 terms is exact to 2^-53 relative, far inside the fp32 result): no host read, no atomics
            run = torch.stack([r.logprob.double(), miss.double()]).cumsum(1).index_select(1, last_rows)
            d = torch.diff(run, dim=1, prepend=run.new_zeros(2, 1))
            sums, matches = d[0].float(), d[1] == 0
        return ScoreResult(r.logprob, r.lse, r.greedy, r.greedy_logit, cu, sums, matches, None)

    def _prefill_rows(self, ctx: DynBatchContext, tasks, prompts, pos0s, q8_history=False, labels=None, prefixes=None):
        """The layer loop of prompt encode over the rows of the call's tasks (checked by the callers) -> (_PromptRows, hidden rows
        before the output norm).  Sequence: separate RMSNorm, W4A16 GEMM (M = rows: the M-tiled MFMA kernel, the arithmetic of
        the reference's M > 40 dequant + GEMM branch) -- every linear over the summed rows --, rope_qk_cache, then the K/V scatter
        and the attention of the call's route (_prompt_scatter_attend).  _prompt_tail finishes the call.
        q8_history (INT8 cache, head size 128): rows below a task's pos0 are read from the cache by the attention kernel
        (ops.prefill_attention_varlen_q8), for one task or several; no unquantised copy of earlier rows is used.
        labels (LLaMA.score: one host label per row) are uploaded with the call's tables for _score_rows."""
        c = self.cfg
        r = _PromptRows.of(self, ctx, tasks, prompts, pos0s, q8_history, labels, prefixes)
        total = r.cu[-1]
        hidden = ops.embedding(r.tokens, self.token_embedding, c.scale_emb)
        cos, sin = self._rope_tables(r.pos)
        for li, layer in enumerate(self.layers):
            qkv = layer.project_qkv(hidden, c.eps)
            self.apply_qk_norm(layer, qkv)
            q, k, v = ops.rope_qk_cache(cos, sin, qkv, c.num_heads, c.num_kv_heads, c.dim_head, True)
            att = self._prompt_scatter_attend(r, li, q.view(total, c.num_heads, c.dim_head),
                                              k.view(total, c.num_kv_heads, c.dim_head), v.view(total, c.num_kv_heads, c.dim_head))
            layer.attn_out_add(att.view(total, -1), hidden)
            layer.ff_add(hidden, c.eps)
        return r, hidden

    def _prompt_scatter_attend(self, r, li, q3, k3, v3):
        """One layer's K/V scatter and causal attention for the rows r (_PromptRows): q3 (rows, H, D), k3 / v3 (rows, Hkv, D), rotated.
        Scatter: copy_to_rag_buffer2 into an fp16 cache; into an INT8 cache the codes and scales, and with the prompt's temporaries
        the unquantised rows into those as well.  Attention, by r.route, over
          "cache"  the fp16 cache (rows below pos0 and the call's own);
          "own"    the call's own unquantised k3 / v3: attn_encode_group with a quantised buffer (attention.cpp:494-510), the
                   prompts attend to their UNquantised rows while the codes go to the cache;
          "temp"   the chunked prompt's temporaries, which this piece's rows have just joined (attention.cpp:497-510);
          "q8"     the INT8 cache below pos0, dequantised where the kernel stages it, and k3 / v3 from there on: a quantised buffer
                   and no prompt temporaries (attention.cpp:510-516).
          "hist"   the task's shared prefix buffer below pos0 and k3 / v3 from there on (admit(prefixes=): the own buffer holds nothing
                   below pos0).
        Head size 128: the MFMA kernels -- the one-task launch on the task's tensors, or one varlen launch over the tables of
        several tasks; other head sizes: per task the mask form of multi_query_attention_rag_buffer."""
        c = self.cfg
        h, hkv, d = c.num_heads, c.num_kv_heads, c.dim_head
        scale = 1.0 / math.sqrt(d)
        k4, v4 = k3.view(*r.placement.shape, hkv, d), v3.view(*r.placement.shape, hkv, d)
        if r.ks_rows is None:
            ops.copy_to_rag_buffer2(r.placement, r.buf_lens, k4, v4, r.k_rows[li], r.v_rows[li])
        else:
            ops.quant_copy_to_rag_buffer(r.pos, r.buf_lens, k3, v3, r.k_rows[li], r.v_rows[li], r.ks_rows[li], r.vs_rows[li],
                                         len_q=r.len_q)
            if r.route == "temp":
                ops.copy_to_rag_buffer2(r.placement, r.len_bufs_dev, k4, v4, r.k_tab[li], r.v_tab[li])
        if d == 128:
            if r.route == "hist":
                return ops.prefill_attention_varlen_hist(q3, r.lens, r.att_pos0s, k3, v3, r.k_tab[li], r.v_tab[li], r.hist_lens, r.len_bufs,
                                                         hkv, scale, plan=r.plan, hist_lens_dev=r.hist_lens_dev)
            if r.route == "q8":
                return ops.prefill_attention_varlen_q8(q3, r.lens, r.att_pos0s, k3, v3, r.k_tab[li], r.v_tab[li], r.ks_tab[li],
                                                       r.vs_tab[li], r.len_bufs, hkv, scale, plan=r.plan)
            if r.plan is None:                            # one task: the launch takes the tensors themselves
                k_buf, v_buf = (k3, v3) if r.route == "own" else (r.kv[li, 0], r.kv[li, 1])
                return ops.prefill_attention(q3, k_buf, v_buf, r.att_pos0s[0], hkv, scale)
            return ops.prefill_attention_varlen(q3, r.lens, r.att_pos0s, *r.att_tables(li, k3, v3), r.plan.buf_lens, hkv, scale,
                                                plan=r.plan)
        k_tab, v_tab = r.att_tables(li, k3, v3)
        att = torch.empty_like(q3)
        for i, (s, p0) in enumerate(zip(r.lens, r.att_pos0s)):
            a = r.cu[i]
            mask, ws = self._prefill_mask(s, r.len_bufs[i], p0)
            ops.multi_query_attention_rag_buffer(q3[a:a + s].view(1, s, h, d), r.len_bufs_dev[i:i + 1], k_tab[i:i + 1],
                                                 v_tab[i:i + 1], mask, scale, r.len_bufs[i], hkv,
                                                 out=att[a:a + s].view(1, s, h, d), workspace=ws)
        return att

    def _prompt_tail(self, ctx, r, hidden):
        """The end of a prompt-encode call over the rows r (_PromptRows): lm_head on the tasks' last rows, the greedy first tokens
        into ctx.tokens, positions = placement = end, valid_lens = end + 1, steps_left bounded -> logits (tasks, vocab).  One task
        writes in place (r.tasks_dev is None); several go through index_copy_, since greedy_advance / argmax_advance write
        consecutive rows."""
        if r.tasks_dev is None:
            task, end = r.tasks[0], r.ends[0]
            logits = self._prompt_logits_and_pick(hidden[-1:], ctx.tokens[task:task + 1])
            ctx.positions[task] = end
            ctx.placement[task] = end
            ctx.valid_lens[task] = end + 1
        else:
            picks = torch.empty(len(r.tasks), dtype=torch.int32, device=self.device)
            logits = self._prompt_logits_and_pick(hidden.index_select(0, r.last_rows), picks)
            ctx.tokens.index_copy_(0, r.tasks_dev, picks)
            ctx.positions.index_copy_(0, r.tasks_dev, r.ends_dev)
            ctx.placement.index_copy_(0, r.tasks_dev, r.ends_dev)
            ctx.valid_lens.index_copy_(0, r.tasks_dev, r.ends_dev + 1)
        ctx.steps_left = min(ctx.steps_left, ctx.max_len_buf - max(r.ends))
        for t, end in zip(r.tasks, r.ends):
            ctx.slot_guard.pop(t, None)
            ctx.slot_room[t] = (ctx.max_len_buf - end, ctx.steps_left)
        if ctx.shared is not None:                        # a task whose own rows start at 0 reads no prefix (a piece behind one: admit(prefixes=))
            stale = [t for t, end, s in zip(r.tasks, r.ends, r.lens) if end == s and ctx.shared.of_host[t] != -1]
            if stale:
                self._set_prefix_of(ctx, stale, [-1] * len(stale))
        return logits

    def _prompt_logits_and_pick(self, last_hidden, picks):
        """logits of the prompts' last rows and the first generated tokens into picks (n int32): the pick rides the lm_head launch
        (zl_gemm_nt_small_m_argmax leaves one candidate per wavefront, zl_greedy_advance reduces them -- first index on ties,
        as torch.argmax) instead of three torch launches over the 128 k logits; TP picks on the gathered rows (zl_argmax_advance)"""
        n = last_hidden.shape[0]
        if self.tp:
            logits = self._logits(last_hidden)
            ops.argmax_advance(logits, tokens=picks)
            return logits
        key = ("argmax", n)
        if key not in self._bufs:
            self._bufs[key] = (ops.argmax_workspace(n, self.cfg.vocab_size, self.device),
                               torch.empty(n, dtype=torch.int64, device=self.device))
        ws = self._bufs[key][0]
        logits = self._logits(last_hidden, argmax_ws=ws)
        ops.greedy_advance(ws, n, self.cfg.vocab_size, tokens=picks)
        return logits

    def step_greedy(self, ctx: DynBatchContext, skip_gemv=False, stop: Optional[StopState] = None):
        """One greedy decode step entirely on the device (graph-capturable): encode, pick the arg-max token
        inside the lm_head launch + one small reduction, and advance the batch state.  Returns
        (logits, next_tokens int64).  stop: a StopState (new_stopper) adds one launch behind the advance that tests the picks against
        the tasks' stop conditions (ops.stop_advance): a task that finished in an earlier step is frozen -- its next_tokens entry is -1
        and its context stays where it ended; stop.finished / gen_lens / live tell.  None: the launches of before."""
        b = ctx.tokens.numel()
        if stop is not None and stop.finished.numel() != b:
            raise ops.ZLError("step_greedy: the stop state belongs to another batch size")
        if b > 4 or self.tp:   # the in-launch pick rides the small-M GEMV; bigger batches / TP: one pick + advance launch over the logits
            logits = self.encode(ctx)
            key = ("next", b)
            if key not in self._bufs:
                self._bufs[key] = torch.empty(b, dtype=torch.int64, device=self.device)
            nxt = self._bufs[key]
            ops.argmax_advance(logits, tokens=ctx.tokens, positions=ctx.positions, placement=ctx.placement, valid_lens=ctx.valid_lens,
                               next_tokens=nxt)
            if stop is not None:
                stop.advance(ctx.tokens.view(b, 1), ctx, next_tokens=nxt)
            ctx.steps_left -= 1
            return logits, nxt
        key = ("argmax", b)
        if key not in self._bufs:
            self._bufs[key] = (ops.argmax_workspace(b, self.cfg.vocab_size, self.device),
                               torch.empty(b, dtype=torch.int64, device=self.device))
        ws, nxt = self._bufs[key]
        logits = self.encode(ctx, argmax_ws=ws, skip_gemv=skip_gemv)
        ops.greedy_advance(ws, b, self.cfg.vocab_size, ctx.tokens, ctx.positions, ctx.placement, ctx.valid_lens, nxt)
        if stop is not None:
            stop.advance(ctx.tokens.view(b, 1), ctx, next_tokens=nxt)
        ctx.steps_left -= 1
        return logits, nxt

    @staticmethod
    def verify_route(b, len_q):
        """the attention route verify(attn="auto") takes for b tasks of len_q rows, from the measured table ("Speculative
        verify step"; profiles/spec_verify.txt).  The rule: causal stays where the p10 .. p90 intervals of the two routes' step
        times overlap.  They do at every measured shape of up to 4 rows (ratios 0.987 - 1.010); from 8 rows on they are disjoint
        everywhere: the rows route is ahead by 0.7 - 1.2 % of the step at B <= 2 and by 4 - 9 % at B >= 4"""
        return "causal" if b * len_q <= 4 else "rows"

    def verify(self, ctx: DynBatchContext, drafts: torch.Tensor, attn="auto", sampler: Optional[SamplerState] = None,
               stop: Optional[StopState] = None):
        """One speculative step on the device (graph-capturable, no host round trip): check the K = drafts.shape[1] draft tokens of
        every task in ONE pass of the decode layer loop over len_q = K + 1 rows per task, keep the longest prefix the model's own
        picks confirm plus one token of its own, and roll the batch state back to there -- SessionGenerator.feed +
        rollback_speculative (zhilight/session_generator.py:25-66), which the reference runs through its prompt path.
        State as step_greedy leaves it (ctx.tokens not yet in the cache).  Row (b, i) carries ctx.tokens[b] (i = 0) or
        drafts[b, i - 1] at position positions[b] + i, writes its K / V to slot placement[b] + i and sees the keys
        j < min(buf_lens[b], valid_lens[b] + i).  Afterwards tokens[b] = the pick behind the accepted drafts, positions / placement /
        valid_lens += accepted + 1; the K / V rows of rejected drafts stay beyond valid_lens until later steps overwrite them (the
        reference's drop_token).  ctx.steps_left -= len_q: the host-side bound counts the worst case.
        attn: "causal" = zl_decode_attn_causal, a task's K / V read once for all of its rows; "rows" = every row a task of its own
        for the len_q = 1 kernels of step_greedy (valid = valid_lens[b] + i), the A/B baseline; "auto" (default) = whichever of
        the two measured faster for this many rows (verify_route).
        drafts: (B, K) int32 on the device.  A draft id outside [0, vocab) -- the -1 padding of a previous call's tokens, say -- is
        never accepted: its row runs on the id clamped into the vocabulary (no out-of-range embedding read) and the comparison
        with the pick uses the id as given.  The row-expanded view and the result buffers are allocated on the first eager call
        per K (run one before capturing); its pointer tables and buffer lengths are re-read from ctx by every call, replays
        included, so a caller may swap a task's buffers in place between calls.
        sampler: None = the picks are greedy (ops.spec_accept).  A SamplerState = the picks are step_sample's (ops.spec_sample_accept):
        row (b, i) samples under task b's temperature / top-k / top-p with the uniform of counter draws[b] + i, a draft is accepted
        iff the pick equals it -- for a deterministic drafter exactly the speculative-sampling rule -- and draws += accepted + 1,
        so the tokens a task emits are the same function of (logits, seed, tokens emitted so far) as step_sample's: speculation
        changes the speed, not the sample -- with the sampler's penalties too: row i is penalised by the task's emitted tokens and
        the drafts in front of it, and only the emitted tokens enter sampler.seen.  Everything up to the logits is the same.  sampler.row_logprobs / row_u (B, len_q) hold
        the emitted tokens' tempered log-probabilities (NaN behind the bonus token) and every row's uniform; sampler.logprobs[b]
        keeps step_sample's meaning, the log-probability of the token now pending in ctx.tokens[b].  The two row buffers follow
        the view's rule: the first eager call per K allocates them.  A sampler with a logit bias applies task b's bias to every row
        (b, i); one with top_logprobs = N leaves the rows' alternatives in sampler.row_top_ids / row_top_logprobs (B, len_q, N), -1 / NaN
        behind the bonus token -- per emitted token the same function of the row's logits that step_sample leaves in sampler.top_ids /
        top_logprobs.  The SAME VALUES only as far as the logits are: a verify row's logits come from another GEMM route than a
        one-row step's, so with d = the largest difference between the two (modified) rows, the class in a slot has a value within
        2 d of step_sample's class there and a log-probability within 2 d / T; equal logits give equal ids.  sampler.top_ids /
        top_logprobs (B, N) are NOT written by this call (the C call has no per-task output for them) and keep the last
        step_sample's values: after a speculative step the pending token's alternatives are sampler.row_top_ids[b, accepted[b]].
        stop: a StopState (new_stopper) adds one launch behind the accept launch (ops.stop_advance): the emitted ids are cut behind the
        first stop id / stop sequence / length limit -- tokens holds -1 there, accepted = ids kept - 1, and tokens / positions / placement /
        valid_lens of the context are what a step that emitted only those leaves, so the ids accepted behind a stop are undone.  A
        task finished earlier is frozen: accepted = -1, its row -1, its context unmoved.  The sampler's draws, seen and row buffers
        are NOT cut: they are valid for a task's first stop.emit_lens entries.  None: the launches of before.
        Returns SpecResult(logits (B * len_q, vocab), accepted (B) int32, tokens (B, len_q) int32); the three are reused by the next
        call with the same K."""
        c, dev = self.cfg, self.device
        if ctx.kv_quant:
            raise ops.ZLError("verify: not on the INT8 KV cache")
        if self.tp:
            raise ops.ZLError("verify: not under tensor parallelism")
        if ctx.shared is not None:
            raise ops.ZLError("verify: speculative rows over shared prefixes are not supported")
        if c.dim_head != 128:
            raise ops.ZLError("verify: head size 128 only (the matrix-core decode attention)")
        if attn not in ("auto", "causal", "rows"):
            raise ops.ZLError("verify: attn is 'auto', 'causal' or 'rows'")
        b = ctx.tokens.numel()
        if not (torch.is_tensor(drafts) and drafts.dim() == 2 and drafts.shape[0] == b and drafts.shape[1] >= 1
                and drafts.dtype == torch.int32 and drafts.device == ctx.tokens.device and drafts.is_contiguous()):
            raise ops.ZLError("verify: drafts are (B, K) contiguous int32 on the context's device, K >= 1")
        if sampler is not None and sampler.temperature.numel() != b:
            raise ops.ZLError("verify: the sampler state belongs to another batch size")
        if stop is not None and stop.finished.numel() != b:
            raise ops.ZLError("verify: the stop state belongs to another batch size")
        len_q = drafts.shape[1] + 1
        m = b * len_q
        if attn == "auto":
            attn = self.verify_route(b, len_q)
        if len_q > 32 or m > 32:
            raise ops.ZLError("verify: at most 32 rows per step (B * (K + 1) <= 32)")
        capturing = torch.cuda.is_current_stream_capturing()
        if ctx.steps_left < len_q and not capturing:
            raise ops.ZLError("verify: the draft rows do not fit the KV buffers (steps_left < K + 1)")
        if len_q not in ctx.spec:
            if capturing:
                raise ops.ZLError("verify: run one eager call before capturing (it allocates the row-expanded view)")
            i32 = dict(dtype=torch.int32, device=dev)
            rows = DynBatchContext(
                tokens=torch.empty(m, **i32), positions=torch.empty(m, **i32), placement=torch.empty(m, **i32),
                valid_lens=torch.empty(m, **i32), buf_lens=torch.empty(m, **i32),
                k_addrs=torch.empty((c.num_layers, m), dtype=torch.int64, device=dev),
                v_addrs=torch.empty((c.num_layers, m), dtype=torch.int64, device=dev),
                max_len_buf=ctx.max_len_buf, kv=ctx.kv, row_expanded=True)
            ctx.spec[len_q] = (rows, torch.arange(len_q, **i32).view(1, len_q), torch.empty(b, **i32), torch.empty((b, len_q), **i32),
                               torch.arange(b, device=dev).view(b, 1).expand(b, len_q).reshape(m))
        rows, ar, accepted, out_tokens, task_of_row = ctx.spec[len_q]
        if sampler is not None:
            if sampler.row_bufs is None:
                sampler.row_bufs = {}
            if len_q not in sampler.row_bufs:
                if capturing:
                    raise ops.ZLError("verify: run one eager call with this sampler before capturing (it allocates the row results)")
                sampler.row_bufs[len_q] = tuple(torch.full((b, len_q), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
            sampler.row_logprobs, sampler.row_u = sampler.row_bufs[len_q]
            if sampler.fsm is not None:
                if sampler.row_state_bufs is None:
                    sampler.row_state_bufs = {}
                if len_q not in sampler.row_state_bufs:
                    if capturing:
                        raise ops.ZLError("verify: run one eager call with this sampler before capturing (it allocates the row results)")
                    sampler.row_state_bufs[len_q] = torch.full((b, len_q), -1, dtype=torch.int32, device=dev)
                sampler.row_states = sampler.row_state_bufs[len_q]
            if sampler.top_n:
                if sampler.row_top_bufs is None:
                    sampler.row_top_bufs = {}
                if len_q not in sampler.row_top_bufs:
                    if capturing:
                        raise ops.ZLError("verify: run one eager call with this sampler before capturing (it allocates the row results)")
                    sampler.row_top_bufs[len_q] = (torch.full((b, len_q, sampler.top_n), -1, dtype=torch.int32, device=dev),
                                                   torch.full((b, len_q, sampler.top_n), float("nan"), dtype=torch.float32, device=dev))
                sampler.row_top_ids, sampler.row_top_logprobs = sampler.row_top_bufs[len_q]
        # the view's tables from the context as it is NOW (a swapped buffer, a regrown table), then the rows of this call: tokens
        # (draft ids clamped into the vocabulary), and the three counters of task b + 0 .. K
        torch.index_select(ctx.buf_lens, 0, task_of_row, out=rows.buf_lens)
        torch.index_select(ctx.k_addrs, 1, task_of_row, out=rows.k_addrs)
        torch.index_select(ctx.v_addrs, 1, task_of_row, out=rows.v_addrs)
        rows.max_len_buf, rows.kv = ctx.max_len_buf, ctx.kv
        tok = rows.tokens.view(b, len_q)
        tok[:, 0].copy_(ctx.tokens)
        tok[:, 1:].copy_(drafts.clamp(0, c.vocab_size - 1))
        torch.add(ctx.positions.view(b, 1), ar, out=rows.positions.view(b, len_q))
        torch.add(ctx.placement.view(b, 1), ar, out=rows.placement.view(b, len_q))
        torch.add(ctx.valid_lens.view(b, 1), ar, out=rows.valid_lens.view(b, len_q))
        rows.steps_left = ctx.steps_left
        hook = None
        if attn == "causal":
            scale = 1.0 / math.sqrt(c.dim_head)

            def hook(li, q, out, workspace):
                shape = (b, len_q, c.num_heads, c.dim_head)
                return ops.decode_attention_causal(q.view(shape), ctx.buf_lens, ctx.k_addrs[li], ctx.v_addrs[li], ctx.valid_lens, scale,
                                                   ctx.max_len_buf, c.num_kv_heads, out=out.view(shape), workspace=workspace)
        logits = self.encode(rows, attend_rows=hook)
        if sampler is None:
            ops.spec_accept(logits, drafts, ctx.tokens, ctx.positions, ctx.placement, ctx.valid_lens, accepted=accepted, out_tokens=out_tokens)
        else:
            opts = sampler.opts()                                           # the task's bias; the rows' top-N into the row buffers
            if sampler.top_n:
                opts.update(top_ids=sampler.row_top_ids, top_logprobs=sampler.row_top_logprobs)
            if sampler.fsm is not None:                                     # the task's state walks over the drafts in front of a row
                opts.update(row_states=sampler.row_states)
            ops.spec_sample_accept(logits, drafts, sampler.temperature, sampler.top_k, sampler.top_p, seeds=sampler.seeds, draws=sampler.draws,
                                   tokens=ctx.tokens, positions=ctx.positions, placement=ctx.placement, valid_lens=ctx.valid_lens,
                                   accepted=accepted, out_tokens=out_tokens, out_logprobs=sampler.row_logprobs, logprobs=sampler.logprobs,
                                   u_out=sampler.row_u, rep_penalty=sampler.repetition_penalty, presence=sampler.presence_penalty,
                                   seen=sampler.seen, **opts)
        if stop is not None:
            stop.advance(out_tokens, ctx, accepted=accepted)
        ctx.steps_left -= len_q
        return SpecResult(logits, accepted, out_tokens)

    # ---- speculative steps with the prompt-lookup drafter ----------------------------------------
    def new_lookup(self, ctx: DynBatchContext, histories, k, max_ngram=3, min_ngram=1, cap=None) -> LookupState:
        """The drafter state for step_lookup: histories[j] = the ids task j has consumed so far (normally its prompt), WITHOUT the
        pending ctx.tokens[j]; that one enters through the kernel's append path right here, so state.drafts is ready on return.
        Drafts are found by prompt lookup (ops.lookup_draft): the longest n-gram, max_ngram down to min_ngram ids, at the history's
        end that occurs earlier in it, and the k ids that followed it.  cap: ids a history row holds, default ctx.max_len_buf + 1 -- a
        task never holds more tokens than that, so the default never overflows; a task fed past a smaller cap drafts nothing
        (-1) from then on and runs as plain greedy steps."""
        k, b = int(k), ctx.tokens.numel()
        if ctx.kv_quant:                                  # what verify refuses at call time, before any drafter state exists
            raise ops.ZLError("new_lookup: not on the INT8 KV cache")
        if self.tp:
            raise ops.ZLError("new_lookup: not under tensor parallelism")
        if self.cfg.dim_head != 128:
            raise ops.ZLError("new_lookup: head size 128 only (the matrix-core decode attention)")
        if k < 1 or b * (k + 1) > 32:
            raise ops.ZLError("new_lookup: k >= 1 and at most 32 rows per step (B * (k + 1) <= 32)")
        if not 1 <= int(min_ngram) <= int(max_ngram) <= 16:
            raise ops.ZLError("new_lookup: 1 <= min_ngram <= max_ngram <= 16")
        cap = ctx.max_len_buf + 1 if cap is None else int(cap)
        if cap < 2:
            raise ops.ZLError("new_lookup: cap >= 2")
        if len(histories) != b:
            raise ops.ZLError(f"new_lookup: {b} tasks, {len(histories)} histories")
        rows = np.zeros((b, cap), np.int32)
        lens = np.zeros(b, np.int32)
        for j, h in enumerate(histories):
            h = np.asarray(h.cpu() if torch.is_tensor(h) else h, dtype=np.int64).reshape(-1)
            if h.size > cap - 1:
                raise ops.ZLError(f"new_lookup: task {j}: {h.size} ids and the pending token do not fit cap = {cap}")
            if h.size and (h.min() < 0 or h.max() >= self.cfg.vocab_size):
                raise ops.ZLError(f"new_lookup: task {j}: ids outside [0, {self.cfg.vocab_size})")
            rows[j, :h.size], lens[j] = h, h.size
        dev = ctx.tokens.device
        state = LookupState(history=torch.from_numpy(rows).to(dev), hist_lens=torch.from_numpy(lens).to(dev),
                            drafts=torch.empty((b, k), dtype=torch.int32, device=dev), match=torch.empty((b, 2), dtype=torch.int32, device=dev),
                            k=k, max_ngram=int(max_ngram), min_ngram=int(min_ngram))
        ops.lookup_draft(state.history, state.hist_lens, k, state.max_ngram, state.min_ngram, new_tokens=ctx.tokens.view(b, 1),
                         drafts=state.drafts, match=state.match)
        return state

    def step_lookup(self, ctx: DynBatchContext, state: LookupState, attn="auto", sampler: Optional[SamplerState] = None,
                    stop: Optional[StopState] = None):
        """One speculative step with the drafter inside, all on the device: verify(ctx, state.drafts, attn, sampler), then ONE launch
        (ops.lookup_draft) appends the tokens the step emitted to the tasks' histories and drafts the next step's tokens into
        state.drafts.  No host round trip; capturable after one eager call (verify's rule), and a replay carries ctx, state and the
        sampler forward together.  Returns verify's SpecResult.
        sampler: a SamplerState makes the step a SAMPLING step (verify's sampler=): the tokens are step_sample's for the same seed,
        however many drafts are accepted; None = greedy.  Sampling and lookup need no interleaving by hand.
        A caller that does interleave step_greedy or step_sample keeps the state in step by feeding the token that step left pending:
        ops.lookup_draft(state.history, state.hist_lens, state.k, state.max_ngram, state.min_ngram,
        new_tokens=ctx.tokens.view(B, 1), drafts=state.drafts, match=state.match).
        stop: verify's stop=.  Its launch runs BEFORE the drafter's, so ids behind a stop never enter the history, and a finished task's
        history stands still (its row is -1)."""
        b = ctx.tokens.numel()
        if state.drafts.shape != (b, state.k) or state.history.shape[0] != b:
            raise ops.ZLError("step_lookup: the state belongs to another batch size")
        res = self.verify(ctx, state.drafts, attn, sampler, stop)
        ops.lookup_draft(state.history, state.hist_lens, state.k, state.max_ngram, state.min_ngram, new_tokens=res.tokens,
                         drafts=state.drafts, match=state.match)
        return res

    def generate_lookup(self, ctx: DynBatchContext, state: LookupState, max_new_tokens, sampler: Optional[SamplerState] = None,
                        stop: Optional[StopState] = None):
        """The eager convenience loop around step_lookup -- the NON-captured path: it reads accepted / tokens back to the host once per
        round.  Runs rounds until every task has emitted max_new_tokens tokens or the KV buffers have no room for another step
        (ctx.steps_left < k + 1); the batch moves in lock step, so tasks that are done keep running until the last one is.
        Returns (tokens, stats): tokens[j] = the ids task j emitted behind its pending ctx.tokens[j] of the time of the call, cut to
        max_new_tokens; stats = {"steps", "emitted": ids per task before the cut (= steps + accepted), "accepted": accepted drafts per
        task, "mean_accepted": accepted drafts per task and step}.  With a sampler (step_lookup's sampler=) the steps sample, and
        stats gains "logprobs": per task the emitted ids' tempered log-probabilities, cut as the ids are; a sampler with top_logprobs
        = N adds "top_ids" / "top_logprobs": per task and emitted id the N alternatives (lists of N), cut the same way.
        stop: a StopState (new_stopper; step_lookup's stop=).  A task then ends at its stop as well: the rounds' results are sliced by
        stop.emit_lens, the loop runs until every task has emitted max_new_tokens ids OR has finished, and stats gains "finished": per
        task 0 (not finished), 1 (stop id), 2 (stop sequence) or 3 (the state's own length limit).  ctx.steps_left keeps its
        conservative host-side count (k + 1 slots per round and task), finished tasks included."""
        b = ctx.tokens.numel()
        out = [[] for _ in range(b)]
        lps = [[] for _ in range(b)]
        tis, tls = [[] for _ in range(b)], [[] for _ in range(b)]
        top = sampler is not None and sampler.top_n > 0
        accepted = [0] * b
        steps = 0
        done = [0] * b
        while min(max_new_tokens if d else len(o) for o, d in zip(out, done)) < max_new_tokens and ctx.steps_left >= state.k + 1:
            res = self.step_lookup(ctx, state, sampler=sampler, stop=stop)
            acc, tok = res.accepted.tolist(), res.tokens.tolist()
            if stop is not None:
                acc, done = [n - 1 for n in stop.emit_lens.tolist()], stop.finished.tolist()      # a frozen task: -1, an empty slice
            lp = sampler.row_logprobs.tolist() if sampler is not None else None
            ti, tl = (sampler.row_top_ids.tolist(), sampler.row_top_logprobs.tolist()) if top else (None, None)
            for j in range(b):
                out[j] += tok[j][:acc[j] + 1]
                accepted[j] += max(acc[j], 0)
                if lp is not None:
                    lps[j] += lp[j][:acc[j] + 1]
                if top:
                    tis[j] += ti[j][:acc[j] + 1]
                    tls[j] += tl[j][:acc[j] + 1]
            steps += 1
        stats = {"steps": steps, "emitted": [len(o) for o in out], "accepted": accepted,
                 "mean_accepted": sum(accepted) / (steps * b) if steps else 0.0}
        if stop is not None:
            stats["finished"] = done
        if sampler is not None:
            stats["logprobs"] = [l[:max_new_tokens] for l in lps]
        if top:
            stats["top_ids"] = [l[:max_new_tokens] for l in tis]
            stats["top_logprobs"] = [l[:max_new_tokens] for l in tls]
        return [o[:max_new_tokens] for o in out], stats

    # ---- sampling steps -----------------------------------------------------------------------------
    def new_sampler(self, ctx: DynBatchContext, temperature=1.0, top_k=0, top_p=1.0, seed=0, repetition_penalty=1.0, presence_penalty=0.0,
                    penalty_tokens=None, logit_bias=None, top_logprobs=0, penalties=False, bias_ld=0, grammar_states=0, grammar_edges=0,
                    grammar=None) -> SamplerState:
        """The state for step_sample.  temperature / top_k / top_p / seed: a scalar for every task or a sequence of B values.
        temperature 0 = greedy; top_k 0 = off; top_p 1 = off; a scalar seed s gives task j the seed s + j, so the tasks draw different
        streams and a task's stream does not depend on the rest of the batch.
        repetition_penalty (> 0, 1 = off) / presence_penalty (0 = off; it takes precedence): the reference generator's knobs, a scalar
        or B values, applied inside the sampling launch to the ids a task has emitted: the pending ctx.tokens entry and every pick
        from here on (the reference penalises generated tokens only).  penalty_tokens: B sequences of further ids to penalise from
        the start, such as the prompts.  With every task at (1, 0) and no penalty_tokens the state carries no bitmap and the steps
        are the unpenalised ones.
        logit_bias: the reference's per-task {token id: bias} map -- one dict for every task, or a sequence of B dicts / Nones; at most
        1024 ids per task, values finite or -inf (a ban).  Added inside the sampling launch behind the penalty (ops.sample_advance's
        bias=).  top_logprobs: N in 0 .. 32, one value for the state: every step also returns the N most likely tokens of the
        penalised and biased distribution with their log-probabilities (state.top_ids / top_logprobs).  With both off the state and
        the calls are the ones without them.
        penalties=True / bias_ld=N (1 .. 1024): carry the bitmap / bias rows of width N whatever the tasks ask for now, so that later
        requests may use them (LLaMA.admit rewrites a slot's rows in place and cannot widen a state).  bias_ld below the longest map
        raises.  The defaults (False, 0) build exactly the states of before.
        grammar_states = S / grammar_edges = E: carry the tables of a token automaton (zhilight_amd.grammar) of S states and E exception
        entries in all, shared by the tasks, with every task unconstrained (state -1); load_grammar copies automata into them and
        returns the start state a request names (LLaMA.admit's "grammar").  Every sampling step then masks a constrained task's row by
        its state's allow-bitmap and advances the state over the pick, inside the sampling launch.  grammar = [automaton | None per
        task]: the convenience without a server -- the tables are sized for the distinct automata (or at the given capacities) and
        task j starts in its automaton's start state.  NOTE the pending ctx.tokens entry is not constrained: it is the prompt
        encode's pick (LLaMA.admit with a "grammar" request re-feeds the prompt's last token instead, so that the first generated
        token is drawn under the grammar).  Without the three arguments the state carries no tables."""
        b, dev = ctx.tokens.numel(), ctx.tokens.device
        if grammar is not None:
            grammar = list(grammar)
            if len(grammar) != b:
                raise ops.ZLError(f"new_sampler: {b} tasks, {len(grammar)} entries of grammar")
            distinct = list({id(g): g for g in grammar if g is not None}.values())
            packs = {id(g): g.pack() for g in distinct}
            grammar_states = int(grammar_states) or max(1, sum(g.states for g in distinct))
            grammar_edges = int(grammar_edges) or sum(int(pk.exc_tok.size) for pk in packs.values())
        grammar_states, grammar_edges = int(grammar_states), int(grammar_edges)
        if not (0 <= grammar_states < 1 << 31 and 0 <= grammar_edges < 1 << 31) or (grammar_edges and not grammar_states):
            raise ops.ZLError("new_sampler: 0 <= grammar_states, grammar_edges < 2^31, and edges only with states")
        bias_ld = int(bias_ld)
        if not 0 <= bias_ld <= ops.LOGIT_BIAS_MAX:
            raise ops.ZLError(f"new_sampler: bias_ld in 0 .. {ops.LOGIT_BIAS_MAX}")

        def per_task(v, what):
            if torch.is_tensor(v):
                v = v.tolist()
            if isinstance(v, (list, tuple, np.ndarray)):
                v = [x.item() if hasattr(x, "item") else x for x in v]
                if len(v) != b:
                    raise ops.ZLError(f"new_sampler: {b} tasks, {len(v)} values of {what}")
                return v, False
            return [v] * b, True

        t, _ = per_task(temperature, "temperature")
        k, _ = per_task(top_k, "top_k")
        p, _ = per_task(top_p, "top_p")
        sd, scalar_seed = per_task(seed, "seed")
        if any(not (float(v) >= 0.0 and math.isfinite(float(v))) for v in t):
            raise ops.ZLError("new_sampler: temperature >= 0 (0 = greedy)")
        if any(int(v) != v or int(v) < 0 or int(v) >= 1 << 31 for v in k):
            raise ops.ZLError("new_sampler: top_k is an integer >= 0 (0 = off)")
        if any(not 0.0 <= float(v) <= 1.0 for v in p):
            raise ops.ZLError("new_sampler: top_p in [0, 1]")
        if any(int(v) != v for v in sd):
            raise ops.ZLError("new_sampler: seed is an integer")
        sd = [int(v) + (j if scalar_seed else 0) for j, v in enumerate(sd)]
        sd = [((v + (1 << 63)) % (1 << 64)) - (1 << 63) for v in sd]        # the 64 bits of the key, as int64
        rp, _ = per_task(repetition_penalty, "repetition_penalty")
        pp, _ = per_task(presence_penalty, "presence_penalty")
        if any(not (float(v) > 0.0 and math.isfinite(float(v))) for v in rp):
            raise ops.ZLError("new_sampler: repetition_penalty > 0 and finite (1 = off)")
        if any(not math.isfinite(float(v)) for v in pp):
            raise ops.ZLError("new_sampler: presence_penalty is finite (0 = off)")
        if penalty_tokens is not None and len(penalty_tokens) != b:
            raise ops.ZLError(f"new_sampler: {b} tasks, {len(penalty_tokens)} sequences of penalty_tokens")
        pen = {}
        if penalties or penalty_tokens is not None or any(float(v) != 1.0 for v in rp) or any(float(v) != 0.0 for v in pp):
            vocab = self.cfg.vocab_size
            seen = torch.zeros((b, ops.seen_words(vocab)), dtype=torch.int32, device=dev)
            ops.seen_mark(seen, ctx.tokens.view(b, 1), vocab)               # the pending token is an emitted one
            if penalty_tokens is not None:
                rows = [np.asarray(h.cpu() if torch.is_tensor(h) else h, dtype=np.int64).reshape(-1) for h in penalty_tokens]
                for j, h in enumerate(rows):
                    if h.size and (h.min() < 0 or h.max() >= vocab):
                        raise ops.ZLError(f"new_sampler: task {j}: penalty_tokens outside [0, {vocab})")
                width = max(h.size for h in rows)
                if width:
                    ids = np.full((b, width), -1, np.int32)                 # -1: skipped by the kernel
                    for j, h in enumerate(rows):
                        ids[j, :h.size] = h
                    ops.seen_mark(seen, torch.from_numpy(ids).to(dev), vocab)
            pen = dict(repetition_penalty=torch.tensor([float(v) for v in rp], dtype=torch.float32, device=dev),
                       presence_penalty=torch.tensor([float(v) for v in pp], dtype=torch.float32, device=dev), seen=seen)
        if isinstance(top_logprobs, bool) or not isinstance(top_logprobs, (int, np.integer)) or not 0 <= int(top_logprobs) <= ops.TOP_LOGPROBS_MAX:
            raise ops.ZLError(f"new_sampler: top_logprobs is an integer in 0 .. {ops.TOP_LOGPROBS_MAX}")
        if logit_bias is not None or bias_ld:
            maps = [logit_bias] * b if logit_bias is None or isinstance(logit_bias, dict) else list(logit_bias)
            if len(maps) != b:
                raise ops.ZLError(f"new_sampler: {b} tasks, {len(maps)} maps of logit_bias")
            if any(maps) or bias_ld:                                        # nothing but empty maps and no forced width: off
                ids, vals, cnt, bits = ops.logit_bias_rows(maps, self.cfg.vocab_size)
                if bias_ld:
                    if int(cnt.max()) > bias_ld:
                        raise ops.ZLError(f"new_sampler: a logit_bias map has {int(cnt.max())} ids, bias_ld = {bias_ld}")
                    wide_ids, wide_vals = np.full((b, bias_ld), -1, np.int32), np.zeros((b, bias_ld), np.float32)
                    keep = min(bias_ld, ids.shape[1])                       # columns behind the longest list hold -1 / 0 already
                    wide_ids[:, :keep], wide_vals[:, :keep] = ids[:, :keep], vals[:, :keep]
                    ids, vals = wide_ids, wide_vals
                pen.update(bias_ids=torch.from_numpy(ids).to(dev), bias_vals=torch.from_numpy(vals).to(dev),
                           bias_cnt=torch.from_numpy(cnt).to(dev), bias_bits=torch.from_numpy(bits.view(np.int32)).to(dev))
        if int(top_logprobs):
            pen.update(top_n=int(top_logprobs), top_ids=torch.full((b, int(top_logprobs)), -1, dtype=torch.int32, device=dev),
                       top_logprobs=torch.full((b, int(top_logprobs)), float("nan"), dtype=torch.float32, device=dev))
        if grammar_states:
            i32 = dict(dtype=torch.int32, device=dev)
            # an unused state allows nothing and leads nowhere; the exception arrays hold one entry at least (never read while empty)
            pen.update(fsm=(torch.zeros((grammar_states, ops.seen_words(self.cfg.vocab_size)), **i32), torch.full((grammar_states,), -1, **i32),
                            torch.zeros(grammar_states + 1, **i32), torch.zeros(max(1, grammar_edges), **i32),
                            torch.full((max(1, grammar_edges),), -1, **i32)),
                       fsm_state=torch.full((b,), -1, **i32), fsm_used=[0, 0])
        state = SamplerState(**pen, temperature=torch.tensor([float(v) for v in t], dtype=torch.float32, device=dev),
                             top_k=torch.tensor([int(v) for v in k], dtype=torch.int32, device=dev),
                             top_p=torch.tensor([float(v) for v in p], dtype=torch.float32, device=dev),
                             seeds=torch.tensor(sd, dtype=torch.int64, device=dev), draws=torch.zeros(b, dtype=torch.int64, device=dev),
                             logprobs=torch.zeros(b, dtype=torch.float32, device=dev), u=torch.zeros(b, dtype=torch.float32, device=dev))
        if grammar is not None and distinct:
            starts = {id(g): self.load_grammar(state, g, packed=packs[id(g)]) for g in distinct}
            state.fsm_state.copy_(torch.tensor([-1 if g is None else starts[id(g)] for g in grammar], dtype=torch.int32))
        return state

    def load_grammar(self, sampler: SamplerState, automaton, packed=None) -> int:
        """Copy a grammar.TokenAutomaton into the free tail of the sampler's automaton tables (new_sampler's grammar_states /
        grammar_edges), its state numbers rebased, and return its start state there: the handle a request's "grammar" names
        (LLaMA.admit) and the value fsm_state takes.  Plain copies into tensors whose pointers and shapes never change: a graph
        captured over the steps goes on reading them, so a grammar may be loaded between replays.  ZLError: a sampler without tables,
        an automaton over more ids than the model's vocabulary, tables that are full (clear_grammars empties them)."""
        if not isinstance(sampler, SamplerState) or sampler.fsm is None:
            raise ops.ZLError("load_grammar: the sampler carries no automaton tables (new_sampler's grammar_states)")
        vocab = self.cfg.vocab_size
        if getattr(automaton, "vocab", vocab + 1) > vocab:
            raise ops.ZLError(f"load_grammar: a grammar.TokenAutomaton over at most the model's {vocab} ids")
        mask, default, exc_off, exc_tok, exc_next = packed if packed is not None else automaton.pack()
        d_mask, d_default, d_off, d_tok, d_next = sampler.fsm
        base, ebase = sampler.fsm_used
        ns, ne = int(default.size), int(exc_tok.size)
        if base + ns > d_default.numel() or ebase + ne > (d_tok.numel() if ebase + ne else 0):
            raise ops.ZLError(f"load_grammar: the tables are full ({base} + {ns} of {d_default.numel()} states, {ebase} + {ne} exception "
                              "entries): size them with new_sampler's grammar_states / grammar_edges, or clear_grammars")
        rows = np.zeros((ns, d_mask.shape[1]), np.uint32)
        rows[:, :mask.shape[1]] = mask
        shift = lambda a: np.where(a >= 0, a.astype(np.int64) + base, a).astype(np.int32)                 # noqa: E731
        dev = d_mask.device
        d_mask[base:base + ns].copy_(torch.from_numpy(rows.view(np.int32)).to(dev))
        d_default[base:base + ns].copy_(torch.from_numpy(shift(default)).to(dev))
        d_off[base:base + ns + 1].copy_(torch.from_numpy((exc_off.astype(np.int64) + ebase).astype(np.int32)).to(dev))
        d_off[base + ns:].fill_(ebase + ne)                                 # the states behind it own empty lists
        if ne:
            d_tok[ebase:ebase + ne].copy_(torch.from_numpy(np.ascontiguousarray(exc_tok)).to(dev))
            d_next[ebase:ebase + ne].copy_(torch.from_numpy(shift(exc_next)).to(dev))
        sampler.fsm_used = [base + ns, ebase + ne]
        return base + int(automaton.start)

    def clear_grammars(self, sampler: SamplerState):
        """Forget every loaded grammar: the next load_grammar starts at state 0.  Refused while any task is constrained (one read-back
        of fsm_state): its state would name another grammar's rows."""
        if not isinstance(sampler, SamplerState) or sampler.fsm is None:
            raise ops.ZLError("clear_grammars: the sampler carries no automaton tables")
        if bool((sampler.fsm_state >= 0).any()):
            raise ops.ZLError("clear_grammars: a task is still inside a grammar (fsm_state >= 0)")
        sampler.fsm_used = [0, 0]

    def new_stopper(self, ctx: DynBatchContext, stop_ids=None, stop_sequences=None, max_new_tokens=0, widths=None) -> StopState:
        """The state for the stop= keyword of step_greedy / step_sample / verify / step_lookup and the generate loops.  stop_ids: ids that
        end a task (EOS ids, stop token ids), at most 16 -- one int or one list of ints for every task, or a sequence of B lists / Nones.
        stop_sequences: multi-token stops, at most 8 per task of 1 .. 16 ids each -- one list of id lists for every task, or a sequence
        of B such lists / Nones.  max_new_tokens: a task's length limit, 0 = none -- one int or B ints.  (new_sampler's convention; a
        flat list of ints as stop_ids is the one list for every task, and B lists are per task.)
        The state counts and tests the ids emitted AFTER its creation, as the generate_* results do.  The token pending in ctx.tokens
        seeds the memory of the last ids, so a stop sequence may begin with it; it is not itself tested or counted: a pending EOS does
        not finish the task.  With nothing set for any task the state is still valid and no task ever finishes.
        widths = (n_ids, n_seqs, ld): the widths of the three parameter tensors, at least the longest lists' -- (16, 8, 16) holds any
        later request (LLaMA.admit rewrites a slot's rows in place).  None: the longest lists', as before."""
        b, dev = ctx.tokens.numel(), ctx.tokens.device

        def ints(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)

        if stop_ids is None or ints(stop_ids):
            ids = [[] if stop_ids is None else [stop_ids]] * b
        else:
            ids = list(stop_ids)
            if all(ints(v) for v in ids):                                   # one flat list: every task's
                ids = [ids] * b
            elif len(ids) != b:
                raise ops.ZLError(f"new_stopper: {b} tasks, {len(ids)} lists of stop_ids")
        if stop_sequences is None:
            seqs = [[]] * b
        else:
            seqs = list(stop_sequences)
            if seqs and all(v is not None and len(v) and all(ints(i) for i in v) for v in seqs):       # id lists: every task's sequences
                seqs = [seqs] * b
            elif len(seqs) != b:
                raise ops.ZLError(f"new_stopper: {b} tasks, {len(seqs)} lists of stop_sequences")
        lim = max_new_tokens
        if torch.is_tensor(lim):
            lim = lim.tolist()
        lim = list(lim) if isinstance(lim, (list, tuple, np.ndarray)) else [lim] * b
        if len(lim) != b:
            raise ops.ZLError(f"new_stopper: {b} tasks, {len(lim)} values of max_new_tokens")
        if any(not ints(v) or not 0 <= int(v) < 1 << 31 for v in lim):
            raise ops.ZLError("new_stopper: max_new_tokens is an integer >= 0 (0 = no limit)")
        sid, ssq, sln = ops.stop_rows(list(zip(ids, seqs)), self.cfg.vocab_size)
        if widths is not None:
            try:
                n_ids, n_seqs, ld = (int(v) for v in widths)
            except (TypeError, ValueError):
                raise ops.ZLError("new_stopper: widths = (n_ids, n_seqs, ld)") from None
            if not (sid.shape[1] <= n_ids <= ops.STOP_IDS_MAX and ssq.shape[1] <= n_seqs <= ops.STOP_SEQS_MAX
                    and ssq.shape[2] <= ld <= ops.STOP_SEQ_LEN_MAX):
                raise ops.ZLError(f"new_stopper: widths hold the longest lists and are at most ({ops.STOP_IDS_MAX}, {ops.STOP_SEQS_MAX}, "
                                  f"{ops.STOP_SEQ_LEN_MAX})")
            wid, wsq, wln = np.full((b, n_ids), -1, np.int32), np.full((b, n_seqs, ld), -1, np.int32), np.zeros((b, n_seqs), np.int32)
            wid[:, :sid.shape[1]], wsq[:, :ssq.shape[1], :ssq.shape[2]], wln[:, :sln.shape[1]] = sid, ssq, sln
            sid, ssq, sln = wid, wsq, wln
        sid, ssq, sln = (torch.from_numpy(a).to(dev) for a in (sid, ssq, sln))
        i32 = dict(dtype=torch.int32, device=dev)
        tail = torch.full((b, ops.STOP_TAIL), -1, **i32)
        tail[:, ops.STOP_TAIL - 1].copy_(ctx.tokens)
        return StopState(stop_ids=sid, stop_seqs=ssq, seq_lens=sln, max_new=torch.tensor([int(v) for v in lim], **i32),
                         gen_lens=torch.zeros(b, **i32), tail=tail, last_token=ctx.tokens.clone(), finished=torch.zeros(b, **i32),
                         emit_lens=torch.zeros(b, **i32), live=torch.full((1,), b, **i32))

    def step_sample(self, ctx: DynBatchContext, state: SamplerState, stop: Optional[StopState] = None):
        """One sampling decode step entirely on the device (graph-capturable after one eager call, no host round trip): encode, then
        ONE launch (ops.sample_advance) picks every task's token under its temperature / top-k / top-p from its own Philox stream
        and advances the batch state, as step_greedy's pick + advance launch does above four rows -- here at every batch size and
        under TP, where every rank samples the same gathered rows with the same generator state.  (Speculative steps under the
        same sampler: verify / step_lookup(sampler=state); they emit this method's tokens.)  state.logprobs / state.u hold the
        picks' tempered log-probabilities and the uniforms used; state.draws has advanced by one.  Returns (logits, next_tokens
        int64).  Penalties: a state built with new_sampler's repetition_penalty / presence_penalty applies them inside that launch --
        the kernel reads the classes of state.seen as ops.repetition_penalty would have left them and records its pick there; the
        returned logits are the raw ones.  The launch count and the host work per step are the same.  A logit bias and the top-N
        alternatives (new_sampler's logit_bias / top_logprobs) ride in the same launch: state.top_ids / top_logprobs (B, N).
        stop: step_greedy's stop= -- one launch behind the sampling launch; a finished task's next_tokens entry is -1, its context
        stands still, and the sampler's draws / seen / logprobs of such a task go on changing and mean nothing."""
        b = ctx.tokens.numel()
        if state.temperature.numel() != b:
            raise ops.ZLError("step_sample: the state belongs to another batch size")
        if stop is not None and stop.finished.numel() != b:
            raise ops.ZLError("step_sample: the stop state belongs to another batch size")
        logits = self.encode(ctx)
        key = ("next", b)
        if key not in self._bufs:
            self._bufs[key] = torch.empty(b, dtype=torch.int64, device=self.device)
        nxt = self._bufs[key]
        ops.sample_advance(logits, state.temperature, state.top_k, state.top_p, seeds=state.seeds, draws=state.draws, tokens=ctx.tokens,
                           positions=ctx.positions, placement=ctx.placement, valid_lens=ctx.valid_lens, next_tokens=nxt,
                           logprobs=state.logprobs, u_out=state.u, rep_penalty=state.repetition_penalty, presence=state.presence_penalty,
                           seen=state.seen, **state.opts())
        if stop is not None:
            stop.advance(ctx.tokens.view(b, 1), ctx, next_tokens=nxt)
        ctx.steps_left -= 1
        return logits, nxt

    def generate_sample(self, ctx: DynBatchContext, state: SamplerState, max_new_tokens, stop: Optional[StopState] = None, poll=8):
        """The eager convenience loop around step_sample: up to max_new_tokens steps, fewer where the KV buffers run out
        (ctx.steps_left).  Returns (tokens (B, steps) int64, logprobs (B, steps) fp32): what every task emitted behind its pending
        ctx.tokens entry of the time of the call, and each token's tempered log-probability.  One read-back at the end.  A state with
        top_logprobs = N > 0 returns a third element, (top_ids (B, steps, N) int32, top_logprobs (B, steps, N) fp32).
        stop: a StopState (new_stopper) ends tasks on the device (step_sample's stop=).  The loop then reads stop.live back every `poll`
        steps and ends once no task is live, at most poll - 1 steps behind the last finish; the token matrix holds -1 behind a task's
        end (the other results are not cut there), and stop.gen_lens / stop.finished give the lengths and the reasons.  ctx.steps_left
        keeps its conservative host-side count of one slot per step and task: a finished task uses no more of its buffer, but the
        host does not know that without a read-back.  None: the loop of before, no read-back but the last."""
        b, dev = ctx.tokens.numel(), ctx.tokens.device
        poll = int(poll)
        if stop is not None and poll < 1:
            raise ops.ZLError("generate_sample: poll >= 1")
        toks, lps, tis, tls = [], [], [], []
        for step in range(max(0, min(int(max_new_tokens), ctx.steps_left))):
            if stop is not None and step and step % poll == 0 and int(stop.live) == 0:
                break
            _, nxt = self.step_sample(ctx, state, stop)
            toks.append(nxt.clone())
            lps.append(state.logprobs.clone())
            if state.top_n:
                tis.append(state.top_ids.clone())
                tls.append(state.top_logprobs.clone())
        if not toks:
            out = (torch.empty((b, 0), dtype=torch.int64, device=dev), torch.empty((b, 0), dtype=torch.float32, device=dev))
            if state.top_n:
                out += ((torch.empty((b, 0, state.top_n), dtype=torch.int32, device=dev),
                         torch.empty((b, 0, state.top_n), dtype=torch.float32, device=dev)),)
            return out
        if state.top_n:
            return torch.stack(toks, dim=1), torch.stack(lps, dim=1), (torch.stack(tis, dim=1), torch.stack(tls, dim=1))
        return torch.stack(toks, dim=1), torch.stack(lps, dim=1)

    # ---- slot admission: keep a running batch full ---------------------------------------------------------------------------------
    @staticmethod
    def slot_widths(sampler: Optional[SamplerState], stop: Optional[StopState], lookup: Optional[LookupState]):
        """what the states carry, as ops.slots_pack takes it"""
        return ops.slot_widths(penalties=sampler is not None and sampler.seen is not None,
                               bias_ld=sampler.bias_ids.shape[1] if sampler is not None and sampler.bias_ids is not None else 0,
                               n_ids=stop.stop_ids.shape[1] if stop is not None else 0, n_seqs=stop.stop_seqs.shape[1] if stop is not None else 0,
                               seq_ld=stop.stop_seqs.shape[2] if stop is not None else 0,
                               hist_cap=lookup.history.shape[1] if lookup is not None else 0,
                               grammar=sampler is not None and sampler.fsm is not None)

    def _slot_states(self, what, ctx, sampler, stop, lookup):
        b = ctx.tokens.numel()
        if self.tp:
            raise ops.ZLError(f"{what}: tensor parallelism is not supported")
        if lookup is not None and ctx.kv_quant:
            raise ops.ZLError(f"{what}: lookup: not on the INT8 KV cache")
        if not isinstance(sampler, SamplerState) or sampler.temperature.numel() != b:
            raise ops.ZLError(f"{what}: the sampler state belongs to another batch size")
        if stop is not None and stop.finished.numel() != b:
            raise ops.ZLError(f"{what}: the stop state belongs to another batch size")
        if lookup is not None and (lookup.history.shape[0] != b or lookup.drafts.shape != (b, lookup.k)):
            raise ops.ZLError(f"{what}: the lookup state belongs to another batch size")
        return b

    def _slots_launch(self, ctx, blob, sampler, stop, lookup, parked_ok=None):
        b = ctx.tokens.numel()
        new = None
        if lookup is not None:
            key = ("draft_new", b)
            if key not in self._bufs:
                self._bufs[key] = torch.empty(b, dtype=torch.int32, device=self.device)
            new = self._bufs[key]
        ops.slots_admit(blob, ctx.tokens, ctx.positions, ctx.placement, ctx.valid_lens, sampler=sampler, stop=stop, lookup=lookup,
                        draft_new=new, parked_ok=parked_ok)
        if lookup is not None:
            ops.lookup_draft(lookup.history, lookup.hist_lens, lookup.k, lookup.max_ngram, lookup.min_ngram, new_tokens=new.view(b, 1),
                             drafts=lookup.drafts, match=lookup.match)

    def _steps_left_after_admission(self, ctx, before):
        """steps_left from the slots' host-known bounds, `before` = its value before the call's prompt encode: a guarded slot
        (ctx.slot_guard) never leaves its buffer and bounds nothing; every other slot has what its last prompt encode left it minus
        the steps counted since (ctx.slot_room), or `before` where the host has no record of the slot.  steps_left = the minimum --
        it RISES when the slot that bounded it has been replaced by a guarded one -- and 1 << 60 with every slot guarded."""
        left = {}
        for t in range(ctx.tokens.numel()):
            if t in ctx.slot_guard:
                ctx.slot_room.pop(t, None)
                continue
            room, at = ctx.slot_room.get(t, (before, before))
            left[t] = max(before, room - (at - before)) if at >= before else before        # a counter set by hand: no record to trust
        ctx.steps_left = min(left.values()) if left else 1 << 60
        ctx.slot_room.update({t: (v, ctx.steps_left) for t, v in left.items()})

    def admit(self, ctx: DynBatchContext, slots, prompts, requests, sampler: SamplerState, stop: Optional[StopState] = None,
              lookup: Optional[LookupState] = None, cache=None, kv_history=None, prefixes=None):
        """Put new requests into slots of a running batch, in place (the reference's scheduler moving a task into max_batch_active,
        src/generator/batch_generator.cpp, where SearcherImplV1 builds the task's state on the host).  In order: prefill_batch(ctx,
        slots, prompts) -- prefill_cached when a prefix cache is given --; ONE upload and ONE launch (ops.slots_pack / slots_admit)
        that re-initialise the slots' rows of sampler, stop and lookup for requests[j] (a dict over ops.SLOT_REQUEST_KEYS, None = the
        defaults; history defaults to the prompt); the drafter's launch when lookup is given.  Returns the prompts' last-row logits
        (with a cache: (logits, matched)).  The first token is the greedy pick prefill leaves pending in ctx.tokens, as for new_sampler
        behind a prefill: a request admitted into a slot is the same function of (prompt, parameters, seed) as one set up through
        prefill_batch + new_sampler + new_stopper + new_lookup.  Every other slot's rows are untouched bit for bit and no tensor is
        reallocated, so a graph captured over step_sample / step_lookup stays valid.
        The states must carry what the requests use (new_sampler's penalties= / bias_ld=, new_stopper's widths=).  With a stop state
        the slot's length limit is clamped (ops.slot_max_new) so that the device-side length stop keeps the task inside its buffer,
        and ctx.steps_left is set from the slots' host-known bounds: such a slot no longer bounds it, the other slots count with
        what their own prompt encode left them (ctx.slot_room).  The guard rests on the limit: it holds while every later step of the
        context passes this stop state and, with a drafter, drafts of this K; a step without stop= or with more drafts is the
        caller's to bound.
        Refused before any launch, with nothing changed: what prefill_batch / prefill_cached refuse, tensor parallelism, lookup on an
        INT8 cache, states of another batch size, what ops.slots_pack refuses, and (with a stop state) a prompt that leaves no room
        for one generated token.
        A request with "grammar" (load_grammar's handle; the sampler carries the tables): the slot's first generated token must obey
        the grammar too, so the prompt is encoded WITHOUT its last token, which becomes the slot's pending token in the prompt pick's
        place; the first step then draws the first token under sampler and grammar.  Such a slot's prompt counts as len - 1 for the
        length limit and the guard, the returned logits row is that of prompt[:-1], the default history is prompt[:-1] (the pending
        token enters it through the drafter's append, which makes it the full prompt), and a 1-token prompt is refused.
        prefixes (a context with shared prefixes, LLaMA.new_shared_prefixes): per slot a loaded prefix index g, or None.  prompts[j] is
        then the part BEHIND prefix g: its rows sit at positions P + i (P = the prefix's length), go into the slot's own buffer at
        those rows and attend to the prefix buffer and to themselves (ops.prefill_attention_varlen_hist); the slot's prefix_of
        becomes g, and the guard and the length limit count P + len.  No K/V row of the prefix is copied.  Not with cache= nor with
        a drafter.  Every slot this call admits WITHOUT a prefix has its prefix_of reset to -1."""
        b = self._slot_states("admit", ctx, sampler, stop, lookup)
        prompts = list(prompts)
        offsets = None
        if prefixes is not None:
            sh, prefixes = ctx.shared, [None if g is None else int(g) for g in prefixes]
            if sh is None or cache is not None or lookup is not None or len(prefixes) != len(prompts):
                raise ops.ZLError("admit: prefixes= needs a context with shared prefixes and one entry per slot; not with cache= nor a drafter")
            if any(g is not None and (not 0 <= g < len(sh.kv) or sh.lens_host[g] < 1) for g in prefixes):
                raise ops.ZLError("admit: prefixes= names loaded prefixes of the context (LLaMA.load_prefix)")
            offsets = [0 if g is None else sh.lens_host[g] for g in prefixes]
        requests = [dict(rq or {}) for rq in requests]
        for j, rq in enumerate(requests if len(requests) == len(prompts) else []):      # a count that is off is refused below
            if rq.get("grammar") is not None:
                pr = torch.as_tensor(prompts[j]).reshape(-1)
                g = self._grammar_start("admit", sampler, rq["grammar"])
                if pr.numel() < 2:
                    raise ops.ZLError("admit: a request with a grammar needs a prompt of 2 tokens at least (the last one is re-fed)")
                prompts[j], rq["grammar"] = pr[:-1], (g, int(pr[-1]))
        slots, _, _ = self._check_prompt_batch("admit", ctx, slots, prompts, offsets, kv_history, behind_prefix=offsets is not None)
        if len(requests) != len(slots):
            raise ops.ZLError("admit: one request per slot")
        entries, guards = self._slot_entries("admit", ctx, slots, prompts, requests, stop, lookup, offsets)
        blob, _ = ops.slots_pack(entries, self.cfg.vocab_size, self.slot_widths(sampler, stop, lookup))
        before = ctx.steps_left
        if offsets is not None:
            out = self._prompt_tail(ctx, *self._prefill_rows(ctx, slots, prompts, offsets, prefixes=prefixes))
            named = [(s, g) for s, g in zip(slots, prefixes) if g is not None]
            if named:
                self._set_prefix_of(ctx, [s for s, _ in named], [g for _, g in named])
        elif cache is None:
            out = self.prefill_batch(ctx, slots, prompts, kv_history=kv_history)
        else:
            out = self.prefill_cached(ctx, cache, slots, prompts, kv_history=kv_history)
        self._slots_launch(ctx, blob, sampler, stop, lookup)
        if guards:
            ctx.slot_guard.update(guards)
            self._steps_left_after_admission(ctx, before)
        return out

    @staticmethod
    def _grammar_start(what, sampler, g):
        """a request's grammar= as admit / admit_samples take it: load_grammar's handle of this sampler -> int"""
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
            raise ops.ZLError(f"{what}: grammar is load_grammar's start state")
        if sampler.fsm is None or not 0 <= int(g) < sampler.fsm_used[0]:
            raise ops.ZLError(f"{what}: grammar names no loaded automaton of this sampler")
        return int(g)

    def _slot_entries(self, what, ctx, slots, prompts, requests, stop, lookup, offsets=None):
        """the per-slot half of an admission, host only: prompts[j] = the tokens the prompt encode sees for slots[j] (behind offsets[j]
        rows of a shared prefix, which count for the limit and the guard); with a stop state the request's length limit is clamped and
        the slot's guard computed, with a drafter the history defaults to those tokens -> (slots_pack's entries, {slot: guard})"""
        k = lookup.k if lookup is not None else 0
        entries, guards = [], {}
        for j, (s, pr, rq) in enumerate(zip(slots, prompts, requests)):
            n = int(pr.numel()) + (offsets[j] if offsets is not None else 0)
            if stop is not None:
                raw = rq.get("max_new_tokens", 0)
                if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)) or not 0 <= int(raw) < 1 << 31:
                    raise ops.ZLError(f"{what}: slot {s}: max_new_tokens is an integer >= 0 (0 = no limit)")
                lim = ops.slot_max_new(n, int(raw), ctx.max_len_buf, k)
                if lim < 1:
                    raise ops.ZLError(f"{what}: prompt of slot {s} ({n} tokens) leaves no room for one generated token")
                rq["max_new_tokens"] = lim
                guards[s] = n + lim + k + 1
            if lookup is not None and rq.get("history") is None:
                rq["history"] = pr.reshape(-1)
            entries.append((s, rq))
        return entries, guards

    @staticmethod
    def fork_descriptors(groups):
        """ops.kv_fork's descriptors of an admit_samples call, host only: groups = [(slots, prompt)] -> for every group (src, dst,
        len(prompt) - 1, prompt[-1]) for each slot behind slots[0] = src, then the self-descriptor (src, src, 0, prompt[-1]); the
        destinations of one source stay neighbours"""
        desc = []
        for slots, prompt in groups:
            toks = torch.as_tensor(prompt).reshape(-1)
            n, last, src = int(toks.numel()), int(toks[-1]), int(slots[0])
            desc += [(src, int(d), n - 1, last) for d in slots[1:]]
            desc.append((src, src, 0, last))
        return desc

    def admit_samples(self, ctx: DynBatchContext, groups, sampler: SamplerState, stop: Optional[StopState] = None,
                      lookup: Optional[LookupState] = None, cache=None, kv_history=None, share=None):
        """Admit several samples of one prompt for ONE prompt encode (the reference's num_results: batch_generator.cpp gives a task's
        first step num_results rows and copies its buffers per result on the host): groups = [(slots, prompt, requests)], slots[0] the
        group's source, requests[j] the request of slots[j] (dicts over ops.SLOT_REQUEST_KEYS, None = the defaults).  In order:
        prefill_batch -- prefill_cached with a prefix cache -- of every group's prompt[:-1] into its source slot, all groups in one
        call; ONE ops.kv_fork launch (a second one for the INT8 cache's scale plane) that copies the source's rows [0, len - 1) into
        the group's other slots, hands them its position, placement and valid length and gives EVERY slot of the group prompt[-1] as
        its pending token (LLaMA.fork_descriptors); the upload and launch of admit (ops.slots_pack / slots_admit) over all slots of
        all groups, which read that pending token; the drafter's launch when lookup is given.  The first step then re-feeds
        prompt[-1] in every slot and draws each slot's first token under its own sampler row: n samples with n seeds start with n
        draws of the true distribution, where admit leaves the prompt's greedy pick pending.  A group of one slot copies nothing: it
        is the admission with a sampled first token.
        The conventions are those of a request with a grammar in admit: a prompt has 2 tokens at least and counts as len - 1 for the
        length limit and the guard (every slot of a group gets the guard its source would get), the default history is prompt[:-1],
        a request's grammar handle travels as (start, prompt[-1]), and the result is the prompt encode's: the logits row of
        prompt[:-1] per GROUP (with a cache: (logits, matched)).  Every other slot's rows are untouched and no tensor is reallocated.
        Refused before any launch, with nothing changed: everything admit refuses, and a slot that occurs twice across the groups.
        share (a context with shared prefixes): one prefix index per group.  prompt[:-1] is then encoded into THAT prefix buffer
        instead of a source slot and no K/V row is copied: the group's slots get prefix_of = g, position = placement = P = len - 1,
        valid length P + 1 and prompt[-1] pending, and read the prefix in place from the first step on.  The buffer must hold P rows
        and be read by no slot outside the call's own; not with cache= nor a drafter."""
        self._slot_states("admit_samples", ctx, sampler, stop, lookup)
        what = "admit_samples"
        gs = []
        for g in groups:
            try:
                slots, prompt, requests = g
                slots, requests = [int(s) for s in slots], [dict(rq or {}) for rq in requests]
            except (TypeError, ValueError):
                raise ops.ZLError(f"{what}: a group is (slots, prompt, requests)") from None
            prompt = torch.as_tensor(prompt).reshape(-1)
            if not slots or len(requests) != len(slots):
                raise ops.ZLError(f"{what}: one request per slot, one slot at least per group")
            if prompt.numel() < 2:
                raise ops.ZLError(f"{what}: a prompt of 2 tokens at least (the last one is re-fed)")
            for rq in requests:
                if rq.get("grammar") is not None:
                    rq["grammar"] = (self._grammar_start(what, sampler, rq["grammar"]), int(prompt[-1]))
            gs.append((slots, prompt, requests))
        if not gs:
            raise ops.ZLError(f"{what}: one group at least")
        flat = [s for slots, _, _ in gs for s in slots]
        heads = [pr[:-1] for slots, pr, _ in gs for _ in slots]
        self._check_prompt_batch(what, ctx, flat, heads, None, kv_history)         # every slot: distinct, inside the batch, the rows fit
        entries, guards = self._slot_entries(what, ctx, flat, heads, [rq for _, _, rqs in gs for rq in rqs], stop, lookup)
        blob, _ = ops.slots_pack(entries, self.cfg.vocab_size, self.slot_widths(sampler, stop, lookup))
        b = ctx.tokens.numel()
        if share is not None:
            return self._admit_shared_samples(ctx, gs, share, cache, blob, guards, sampler, stop, lookup)
        lens = [ctx.max_len_buf] * b
        desc, _ = ops.kv_fork_check(self.fork_descriptors([(slots, pr) for slots, pr, _ in gs]), lens, b, self.cfg.vocab_size)
        before = ctx.steps_left
        sources, prompts = [slots[0] for slots, _, _ in gs], [pr[:-1] for _, pr, _ in gs]
        if cache is None:
            out = self.prefill_batch(ctx, sources, prompts, kv_history=kv_history)
        else:
            out = self.prefill_cached(ctx, cache, sources, prompts, kv_history=kv_history)
        ops.kv_fork(desc, ctx.k_addrs, ctx.v_addrs, ctx.buf_lens, self.cfg.num_kv_heads, self.cfg.dim_head * ctx.kv[0].element_size(),
                    buf_lens_host=lens, ctx_rows=(ctx.tokens, ctx.positions, ctx.placement, ctx.valid_lens))
        if ctx.kv_quant:
            ops.kv_fork(desc, ctx.ks_addrs, ctx.vs_addrs, ctx.buf_lens, self.cfg.num_kv_heads, 4, buf_lens_host=lens)
        for slots, _, _ in gs:                                                # the copies stand where their source stands
            for d in slots[1:]:
                ctx.slot_guard.pop(d, None)
                ctx.slot_room[d] = ctx.slot_room[slots[0]]
        if ctx.shared is not None:                                            # a copy reads no prefix (the sources: _prompt_tail)
            stale = [d for slots, _, _ in gs for d in slots[1:] if ctx.shared.of_host[d] != -1]
            if stale:
                self._set_prefix_of(ctx, stale, [-1] * len(stale))
        self._slots_launch(ctx, blob, sampler, stop, lookup)
        if guards:
            ctx.slot_guard.update(guards)
            self._steps_left_after_admission(ctx, before)
        return out

    def _admit_shared_samples(self, ctx, gs, share, cache, blob, guards, sampler, stop, lookup):
        """admit_samples(share=) behind its checks of the groups: the prefixes' own checks, the prompt encode into the prefix buffers,
        the slots' rows of the context, the admission launch"""
        what, sh = "admit_samples", ctx.shared
        try:
            share = [int(g) for g in share]
        except (TypeError, ValueError):
            raise ops.ZLError(f"{what}: share is one prefix index per group") from None
        if sh is None or cache is not None or lookup is not None or len(share) != len(gs):
            raise ops.ZLError(f"{what}: share= needs a context with shared prefixes and one prefix per group; not with cache= nor a drafter")
        mine = {s for slots, _, _ in gs for s in slots}
        if len(set(share)) != len(share) or any(not 0 <= g < len(sh.kv) for g in share):
            raise ops.ZLError(f"{what}: share: distinct prefix indices below {len(sh.kv)}")
        for g, (_, pr, _) in zip(share, gs):
            if pr.numel() - 1 > sh.rows:
                raise ops.ZLError(f"{what}: a prompt of {pr.numel()} tokens does not fit a prefix buffer of {sh.rows} rows")
            if any(s not in mine for s in sh.users(g)):
                raise ops.ZLError(f"{what}: prefix {g} is read by slots outside this call")
        before = ctx.steps_left
        old = [s for s in mine if sh.of_host[s] != -1]
        if old:                                                               # the call's own slots let go of what they read
            self._set_prefix_of(ctx, old, [-1] * len(old))
        out = self._load_prefixes(what, ctx, share, [pr[:-1] for _, pr, _ in gs])
        slots = [s for ss, _, _ in gs for s in ss]
        ps = [int(pr.numel()) - 1 for ss, pr, _ in gs for _ in ss]
        rows = torch.tensor(slots + ps + [p + 1 for p in ps] + [int(pr[-1]) for ss, pr, _ in gs for _ in ss], dtype=torch.int64).to(self.device)
        n = len(slots)
        idx, pos, valid, tok = rows[:n], rows[n:2 * n].to(torch.int32), rows[2 * n:3 * n].to(torch.int32), rows[3 * n:].to(torch.int32)
        ctx.tokens.index_copy_(0, idx, tok)
        ctx.positions.index_copy_(0, idx, pos)
        ctx.placement.index_copy_(0, idx, pos)
        ctx.valid_lens.index_copy_(0, idx, valid)
        self._set_prefix_of(ctx, slots, [g for g, (ss, _, _) in zip(share, gs) for _ in ss])
        ctx.steps_left = min(ctx.steps_left, ctx.max_len_buf - max(ps))
        for s, p in zip(slots, ps):
            ctx.slot_guard.pop(s, None)
            ctx.slot_room[s] = (ctx.max_len_buf - p, ctx.steps_left)
        self._slots_launch(ctx, blob, sampler, stop, lookup)
        if guards:
            ctx.slot_guard.update(guards)
            self._steps_left_after_admission(ctx, before)
        return out

    def park(self, ctx: DynBatchContext, slots, sampler: SamplerState, stop: StopState, lookup: Optional[LookupState] = None, finished=None):
        """Park finished slots while nothing waits for them (one upload, one launch, the drafter's with lookup): a parked slot re-feeds
        token 0 at position 0 and attends over one key instead of its whole history; stop.finished keeps its value, so the slot stays
        frozen.  finished: the caller's host copy of stop.finished -- a slot that it does not show as finished is refused, as is
        anything admit refuses of the states."""
        b = self._slot_states("park", ctx, sampler, stop, lookup)
        slots = [int(s) for s in slots]
        if stop is None:
            raise ops.ZLError("park: needs the stop state (only a finished slot is parked)")
        if not slots or len(set(slots)) != len(slots) or any(s < 0 or s >= b for s in slots):
            raise ops.ZLError("park: slots must be distinct indices of the batch")
        done = [] if finished is None else [int(v) for v in (finished.tolist() if hasattr(finished, "tolist") else finished)]
        if len(done) != b or any(done[s] == 0 for s in slots):
            raise ops.ZLError("park: only a slot known to be finished is parked (finished = the host copy of stop.finished)")
        blob, _ = ops.slots_pack([(s, None) for s in slots], self.cfg.vocab_size, self.slot_widths(sampler, stop, lookup))
        self._slots_launch(ctx, blob, sampler, stop, lookup, parked_ok=set(slots))
        if ctx.shared is not None:                            # a parked slot attends over row 0 of its OWN buffer
            stale = [s for s in slots if ctx.shared.of_host[s] != -1]
            if stale:
                self._set_prefix_of(ctx, stale, [-1] * len(stale))
        before = ctx.steps_left
        ctx.slot_guard.update({s: 0 for s in slots})
        self._steps_left_after_admission(ctx, before)

    def advance(self, ctx: DynBatchContext, next_tokens: torch.Tensor):
        """Device-side bookkeeping between steps (what fill_search_tokens does on the host in the
        reference, src/generator/batch_generator.cpp:1226-1335): no host sync, graph-capturable."""
        ctx.tokens.copy_(next_tokens.to(torch.int32))
        ctx.positions.add_(1)
        ctx.placement.add_(1)
        ctx.valid_lens.add_(1)
        ctx.steps_left -= 1

    def weight_bytes(self):
        return sum(l.weight_bytes() for l in self.layers)
