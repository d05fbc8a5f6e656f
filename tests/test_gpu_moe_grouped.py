"""Expert-grouped W4A16 GEMM (zl_w4a16_gemm_grouped, csrc/w4_moe_grouped.hip) and the Qwen3-MoE layer of the LLaMA driver.

Kernel: each expert's rows against the oracle's exact product with the dequantised weight (gemm_nt(x_e, W16_e, exact=True), the
M-tiled kernel's bar of tests/test_gpu_w4.py) and bit for bit against zl_w4a16_gemm_tiled on the same gathered rows (the grouped
kernel keeps its k order).  Model: the MoE feed-forward against an oracle chain composed from the oracle's functions, the two
routes against each other, and decode / prefill / prefill_batch / a captured step_greedy through the driver."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu


def _t(a, dev, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dt is None else t.view(dt)


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _f64(u):
    return u.view(np.float16).astype(np.float64)


def _stack(oracle, ops, dev, rng, e, n, k, g, interleave):
    """e experts of an (n, k) matrix ([gate; up] of n / 2 rows each with interleave): k-major numpy tensors + the ZLW4M stack"""
    kms = []
    for _ in range(e):
        qw, qz, sc = synth.gptq_hf(rng, k, n, g)
        sc = (np.abs(rng.standard_normal(sc.shape)) * (0.5 / np.sqrt(k)) / 4 + 1e-4).astype(np.float16).view(np.uint16)
        kms.append(oracle.gptq_prepare_k_major(qw, qz, sc, g))
    w = ops.W4MMoEWeight.from_k_major([_t(km[0].view(np.int32), dev) for km in kms], [_t(km[1], dev) for km in kms],
                                      [_t(km[2], dev, torch.float16) for km in kms], g, row_interleave=interleave)
    return kms, w


def _tiled(ops, x, w, epi):
    """zl_w4a16_gemm_tiled without scratch: no K split, every output one sum over K in chunk order"""
    import ctypes as C
    from zhilight_amd._lib import lib
    m = x.shape[0]
    y = torch.empty((m, w.n // 2 if epi else w.n), dtype=torch.float16, device=x.device)
    assert lib().zl_w4a16_gemm_tiled(ops._p(x), ops._i(x.stride(0)), ops._p(w.qw), ops._p(w.meta), None, None, ops._p(y), ops._i(m),
                                     ops._i(w.n), ops._i(w.k), ops._i(w.group_size), C.c_int(epi), ops._stream()) == 0
    return _u16(y)


def _ids(rng, m, top_k, e, kind):
    if kind == "uniform":
        return np.stack([rng.choice(e, top_k, replace=False) for _ in range(m)]).astype(np.int32)
    if kind == "ragged":      # a few hot experts, some one-row experts, the rest empty
        hot = rng.choice(e, min(e, 3), replace=False)
        ids = np.empty((m, top_k), np.int32)
        for t in range(m):
            pool = list(hot) + list(rng.choice(e, top_k, replace=False))
            ids[t] = np.array(list(dict.fromkeys(pool)))[:top_k] if t % 5 else rng.choice(e, top_k, replace=False)
        return ids
    # "one": one expert receives every token (slot 0), the other slots spread over the rest
    ids = np.empty((m, top_k), np.int32)
    for t in range(m):
        ids[t, 0] = 2
        ids[t, 1:] = rng.choice([x for x in range(e) if x != 2], top_k - 1, replace=False)
    return ids


@pytest.mark.parametrize("m,top_k,e,n,k,kind,silu", [
    (2, 2, 8, 256, 768, "uniform", False), (3, 4, 16, 512, 2048, "ragged", True), (8, 8, 32, 768, 2048, "uniform", True),
    (32, 8, 64, 256, 768, "ragged", False), (64, 4, 16, 384, 2048, "one", True), (512, 8, 32, 512, 768, "uniform", False),
    (2048, 2, 8, 256, 2048, "one", False), (2048, 8, 16, 256, 768, "ragged", True),
    (96, 4, 16, 256, 768, "uniform", False), (400, 4, 16, 256, 2048, "uniform", True)])     # BM = 32 (24 rows per expert), 64 (100)
def test_grouped_gemm(oracle, dev, m, top_k, e, n, k, kind, silu):
    from zhilight_amd import ops
    rng = np.random.default_rng(m * 7 + top_k + e)
    g = 128
    kms, w = _stack(oracle, ops, dev, rng, e, n, k, g, silu)
    ids = _ids(rng, m, top_k, e, kind)
    x = synth.act(rng, m, k)
    p = m * top_k
    flat = ids.reshape(-1)
    order = np.argsort(flat, kind="stable").astype(np.int32)
    loads = np.bincount(flat, minlength=e).astype(np.int32)
    epi = ops.EPI_SILU_MUL if silu else 0
    xt = _t(x, dev)
    got = ops.moe_gemm_grouped(xt, w, _t(loads, dev), _t(order, dev), p, in_div=top_k, epilogue=epi)
    got2 = ops.moe_gemm_grouped(xt, w, _t(loads, dev), _t(order, dev), p, in_div=top_k, epilogue=epi)
    gu = _u16(got)
    assert np.array_equal(gu, _u16(got2))                     # repeated runs are bit-identical
    off = np.concatenate([[0], np.cumsum(loads)])
    checked = 0
    for ex in range(e):
        if loads[ex] == 0:
            continue
        rows = order[off[ex]:off[ex + 1]] // top_k
        xe = np.ascontiguousarray(x[rows])
        assert np.array_equal(gu[off[ex]:off[ex + 1]], _tiled(ops, _t(xe, dev), w.expert(ex), epi)), ex   # the tiled kernel's k order
        if silu or checked >= 6:
            continue
        checked += 1
        ref = oracle.gemm_nt(oracle.h2u(xe), oracle.gptq_dequant_k_major(*kms[ex]), exact=True)
        rms = np.sqrt((ref ** 2).mean())
        d = np.abs(_f64(gu[off[ex]:off[ex + 1]]) - ref)
        assert (d <= 2.0 ** -10 * np.abs(ref) + 2e-5 * rms).all(), float((d / rms).max())


def test_grouped_gemm_scatter_and_dropped_ids(oracle, dev):
    """out_scatter writes pair rows; pairs whose id lies outside the stack (sorted behind it, no load) are dropped, never
    written; an index table pointing outside the output is not written either"""
    from zhilight_amd import ops
    rng = np.random.default_rng(5)
    e, m, top_k, n, k = 8, 24, 4, 256, 768
    kms, w = _stack(oracle, ops, dev, rng, e, n, k, 128, False)
    ids = _ids(rng, m, top_k, e, "uniform")
    ids[::5, 1] = e + 3                                       # out of range
    flat = ids.reshape(-1)
    p = flat.size
    order = np.argsort(flat, kind="stable").astype(np.int32)
    loads = np.bincount(flat[flat < e], minlength=e).astype(np.int32)
    x = synth.act(rng, p, k)                                  # rows in sorted order (the down projection's input)
    out = torch.full((p, n), 0x3C00, dtype=torch.int16, device=dev).view(torch.float16)   # 1.0 sentinel
    ops.moe_gemm_grouped(_t(x, dev), w, _t(loads, dev), _t(order, dev), p, out_scatter=True, out=out)
    go = _u16(out)
    valid = int(loads.sum())
    plain = _u16(ops.moe_gemm_grouped(_t(x, dev), w, _t(loads, dev), None, p))
    assert np.array_equal(go[order[:valid]], plain[:valid])
    assert (go[order[valid:]] == 0x3C00).all()
    # a corrupt table: pair ids past the output rows are dropped; x rows are clamped (never a stray read)
    bad = order.copy()
    bad[:4] = p + 1000
    out2 = torch.full((p, n), 0x3C00, dtype=torch.int16, device=dev).view(torch.float16)
    ops.moe_gemm_grouped(_t(x, dev), w, _t(loads, dev), _t(bad, dev), p, out_scatter=True, out=out2)
    torch.cuda.synchronize()
    g2 = _u16(out2)
    assert np.array_equal(g2[bad[4:valid]], plain[4:valid])
    ops.moe_gemm_grouped(_t(x[:3], dev), w, _t(loads, dev), _t(bad, dev), p, in_div=1)       # indices far past x's 3 rows
    torch.cuda.synchronize()


def test_grouped_gemm_argument_checks(dev):
    from zhilight_amd import ops
    from zhilight_amd._lib import lib
    import ctypes as C
    rng = np.random.default_rng(1)
    e, n, k = 4, 256, 768
    km = [synth.gptq_hf(rng, k, n, 128) for _ in range(e)]
    import zl_oracle
    kms = [zl_oracle.gptq_prepare_k_major(*a, 128) for a in km]
    w = ops.W4MMoEWeight.from_k_major([_t(a[0].view(np.int32), dev) for a in kms], [_t(a[1], dev) for a in kms],
                                      [_t(a[2], dev, torch.float16) for a in kms], 128)
    loads = _t(np.array([2, 0, 1, 1], np.int32), dev)
    idx = _t(np.arange(4, dtype=np.int32), dev)
    x = torch.zeros((4, k), dtype=torch.float16, device=dev)
    with pytest.raises(ops.ZLError):
        ops.moe_gemm_grouped(torch.zeros((4, 640), dtype=torch.float16, device=dev), w, loads, idx, 4)   # K mismatch
    with pytest.raises(ops.ZLError):
        ops.moe_gemm_grouped(x, w, loads[:3], idx, 4)                                                      # one load per expert
    with pytest.raises(ops.ZLError):
        ops.moe_gemm_grouped(x, w, loads, idx, 4, epilogue=ops.EPI_SILU_MUL)                               # not interleaved
    with pytest.raises(ops.ZLError):
        ops.moe_gemm_grouped(x.float(), w, loads, idx, 4)
    with pytest.raises(ops.ZLError):
        ops.moe_gemm_grouped(x, w, loads, None, 4, in_div=2)
    y = torch.empty((4, n), dtype=torch.float16, device=dev)
    p = ops._p
    s = ops._stream()
    sq, sm = w.stride_bytes
    call = lambda **kw: lib().zl_w4a16_gemm_grouped(
        p(kw.get("x", x)), ops._i(k), ops._i(4), p(w.qw), p(w.meta), ops._i(kw.get("e", e)), ops._i(kw.get("sq", sq)), ops._i(sm),
        p(loads), p(idx), ops._i(4), C.c_int(0), C.c_int(0), p(y), ops._i(4), ops._i(n), ops._i(kw.get("k", k)), ops._i(128),
        C.c_int(kw.get("epi", 0)), s)
    assert call() == 0
    assert call(x=None) == -1                                    # ZL_EINVAL
    assert call(epi=ops.EPI_BIAS) == -1
    assert call(k=700) == -2                                     # ZL_ESHAPE: K % 128
    assert call(sq=sq - 16) == -2                                # expert stride shorter than a matrix
    assert call(e=1 << 20) == -4                                 # ZL_ELIMIT
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# the silu*mul epilogues against the oracle
@pytest.mark.parametrize("epi_name", ["EPI_SILU_MUL", "EPI_SILU_MUL_F32"])
def test_grouped_gemm_silu_epilogues(oracle, dev, epi_name):
    """gate|up with silu*mul against the oracle: exact gate / up products, rounded to T for EPI_SILU_MUL (silu_mul of the rounded
    values), kept in fp32 for EPI_SILU_MUL_F32; both forms (sorted and pairs) give the same bits"""
    from zhilight_amd import ops
    epi = getattr(ops, epi_name)
    rng = np.random.default_rng(17)
    e, m, top_k, ff, k = 8, 40, 2, 128, 1024
    kms, w = _stack(oracle, ops, dev, rng, e, 2 * ff, k, 128, True)
    ids = _ids(rng, m, top_k, e, "uniform")
    x = synth.act(rng, m, k)
    flat = ids.reshape(-1)
    order = np.argsort(flat, kind="stable").astype(np.int32)
    loads = np.bincount(flat, minlength=e).astype(np.int32)
    got = _u16(ops.moe_gemm_grouped(_t(x, dev), w, _t(loads, dev), _t(order, dev), flat.size, in_div=top_k, epilogue=epi))
    pairs = _u16(ops.moe_gemm_pairs(_t(x, dev), w, _t(ids, dev), in_div=top_k, epilogue=epi))
    assert np.array_equal(got, pairs[order])
    for j in range(flat.size):
        tok, ex = order[j] // top_k, flat[order[j]]
        w16 = oracle.gptq_dequant_k_major(*kms[ex])           # rows [gate; up] of this expert
        full = oracle.gemm_nt(oracle.h2u(x[tok:tok + 1]), w16, exact=True)[0]
        gt, up = full[:ff], full[ff:]
        if epi == ops.EPI_SILU_MUL:
            g16, u16 = gt.astype(np.float16), up.astype(np.float16)
            ref = _f64(oracle.silu_mul(oracle.h2u(g16), oracle.h2u(u16)))
            bar = 2.0 ** -10 * np.abs(ref) + 2e-3 * np.sqrt((ref ** 2).mean())      # a 1-ulp flip of gate / up at a rounding tie
        else:
            ref = gt / (1.0 + np.exp(-gt)) * up
            bar = 2.0 ** -10 * np.abs(ref) + 2e-5 * np.sqrt((ref ** 2).mean())
        d = np.abs(_f64(got[j]) - ref)
        assert (d <= bar).all(), (j, float(d.max()))


# ---------------------------------------------------------------------------------------------------------------------------
# the model, against an oracle chain: test_gpu_model.py's OracleModel with the MoE feed-forward composed from the oracle
def _cfg(**kw):
    from zhilight_amd.llama import ModelConfig
    base = dict(num_layers=3, dim_model=1024, num_heads=8, dim_head=128, dim_ff=1024, vocab_size=512, num_kv_heads=2, eps=1e-6,
                rope_theta=1e6, rope_scaling=None, qk_norm="head", model_type="qwen3_moe", moe_num_experts=16, moe_top_k=4,
                moe_intermediate_size=256, norm_topk_prob=True, mlp_only_layers=[1])
    base.update(kw)
    return ModelConfig(**base)


def _moe_hf_state(cfg, seed=3):
    """a Qwen3-MoE GPTQ checkpoint under HF names: test_gpu_model's _hf_state (dense feed-forward of every layer; the MoE layers
    ignore theirs) + q / k norms + experts (the same recipe) and a router per MoE layer"""
    from test_gpu_model import _hf_state
    rng = np.random.default_rng(seed)
    sd = _hf_state(rng, cfg, 128)
    ff, g = cfg.moe_intermediate_size, 128
    for i in range(cfg.num_layers):
        p = f"model.layers.{i}."
        for n in ("q", "k"):
            sd[p + f"self_attn.{n}_norm.weight"] = (1 + 0.1 * rng.standard_normal(cfg.dim_head)).astype(np.float16)
        if not cfg.is_moe_layer(i):
            continue
        for e in range(cfg.moe_num_experts):
            for name, din, dout in (("gate_proj", cfg.dim_model, ff), ("up_proj", cfg.dim_model, ff), ("down_proj", ff, cfg.dim_model)):
                qw, qz, sc = synth.gptq_hf(rng, din, dout, g)
                sc = (np.abs(rng.standard_normal(sc.shape)) * (0.5 / np.sqrt(din)) / 4 + 1e-4).astype(np.float16)
                q = p + f"mlp.experts.{e}.{name}."
                sd[q + "qweight"], sd[q + "qzeros"], sd[q + "scales"] = qw.view(np.int32), qz.view(np.int32), sc
        sd[p + "mlp.gate.weight"] = (rng.standard_normal((cfg.moe_num_experts, cfg.dim_model)) / np.sqrt(cfg.dim_model)).astype(np.float16)
    return sd


def _model(dev, sd, cfg, monkeypatch, route="grouped", thres=None):
    from zhilight_amd.llama import LLaMA, QuantConfig
    monkeypatch.setenv("ZL_MOE_ROUTE", route)
    if thres is None:
        monkeypatch.delenv("GPTQ_MOE_M_THRES", raising=False)
    else:
        monkeypatch.setenv("GPTQ_MOE_M_THRES", str(thres))
    return LLaMA(cfg, QuantConfig(5, 128), dev).load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})


def _oracle_class():
    from test_gpu_model import OracleModel

    class MoEOracle(OracleModel):
        """OracleModel's decode step (flavour E, fp16 KV) with the MoE feed-forward in the sparse layers: exact router logits, the
        top-k softmax renormalised, per (token, slot) the expert's exact gate / up rounded to T, silu_mul, the exact down rounded to
        T, sum_experts, the residual add.  gpu_routes(layer) -> the GPU's ids of that layer in the step: where a k-th / (k+1)-th
        margin of the exact logits lies below 1e-4 of the row's largest logit (fp32 router noise) the GPU's pick is replayed"""
        replays = 0

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            if not self.cfg.rope_scaling:
                self.rope_kind = "plain"                    # (OracleModel's default is llama3 scaling)

        def _moe(self, i, h, gpu_ids):
            o, c = self.o, self.cfg
            p = f"model.layers.{i}."
            xn = o.rmsnorm(h, o.h2u(self.sd[p + "post_attention_layernorm.weight"]), c.eps)
            logits = o.gemm_nt(xn, o.h2u(self.sd[p + "mlp.gate.weight"]), exact=True)
            k = c.moe_top_k
            ids = np.empty((h.shape[0], k), np.int32)
            for t in range(h.shape[0]):
                mine = np.argsort(-logits[t], kind="stable")[:k]
                theirs = gpu_ids[t] if gpu_ids is not None else mine
                if set(theirs) != set(mine):
                    srt = np.sort(logits[t])[::-1]
                    assert srt[k - 1] - srt[k] < 1e-4 * np.abs(srt).max(), (i, t, "routing differs beyond the logits' noise")
                    self.replays += 1
                    ids[t] = theirs
                else:
                    ids[t] = theirs                         # (the GPU's slot order: sum_experts adds the slots in order)
            pr = np.exp(logits - logits.max(axis=1, keepdims=True))
            sel = np.take_along_axis(pr, ids.astype(np.int64), 1)
            wts = (sel / sel.sum(axis=1, keepdims=True) if c.norm_topk_prob else sel / pr.sum(axis=1, keepdims=True)).astype(np.float32)
            if not hasattr(self, "w16"):
                self.w16 = {}
            rows = np.empty((h.shape[0] * k, c.dim_model), np.uint16)
            for t in range(h.shape[0]):
                for s_ in range(k):
                    e = int(ids[t, s_])
                    key = (i, e)
                    if key not in self.w16:
                        self.w16[key] = [o.gptq_dequant_k_major(*self.km[p + f"mlp.experts.{e}.{n}"]) for n in ("gate_proj", "up_proj", "down_proj")]
                    wg, wu, wd = self.w16[key]
                    x1 = xn[t:t + 1]
                    gt = o.h2u(o.gemm_nt(x1, wg, exact=True).astype(np.float16))
                    up = o.h2u(o.gemm_nt(x1, wu, exact=True).astype(np.float16))
                    rows[t * k + s_] = o.h2u(o.gemm_nt(o.silu_mul(gt, up), wd, exact=True).astype(np.float16))[0]
            y = o.moe_sum_experts(rows, np.arange(h.shape[0] * k, dtype=np.int32), wts)
            return o.element_add_scale(h, y, 1.0, True)

        def step_moe(self, tokens, pos, gpu_routes):
            """OracleModel.step's sequence (flavour E), the feed-forward of MoE layers replaced"""
            o, c = self.o, self.cfg
            b = len(tokens)
            h = o.embedding(np.asarray(tokens, np.int32), o.h2u(self.sd["model.embed_tokens.weight"]))
            cs, sn = self._tables(pos)
            lens = np.full(b, self.len_buf, np.int32)
            mask = np.concatenate([(np.arange(self.len_buf) <= p_).astype(np.int8) for p_ in pos])
            for i in range(c.num_layers):
                p = f"model.layers.{i}."
                xn = o.rmsnorm(h, o.h2u(self.sd[p + "input_layernorm.weight"]), c.eps)
                qkv = np.concatenate([self._gemv(xn, p + "self_attn." + n + "_proj", "E") for n in "qkv"], axis=1)
                qkv = self._qk_norm(i, qkv)
                q, kk, v = o.rope_qk_cache(cs, sn, qkv, c.num_heads, c.num_kv_heads, c.dim_head, True)
                o.copy_to_rag_buffer2(np.asarray(pos, np.int32).reshape(b, 1), lens, kk.reshape(b, 1, c.num_kv_heads, c.dim_head),
                                      v.reshape(b, 1, c.num_kv_heads, c.dim_head), self.kb[i], self.vb[i], True)
                att = o.mqa_rag_buffer(q.reshape(b, 1, c.num_heads, c.dim_head), lens, self.kb[i], self.vb[i], mask,
                                       c.num_kv_heads, 1.0 / np.sqrt(c.dim_head), True).reshape(b, -1)
                h = o.element_add_scale(h, self._gemv(att, p + "self_attn.o_proj", "E"), 1.0, True)
                if c.is_moe_layer(i):
                    h = self._moe(i, h, gpu_routes(i) if gpu_routes else None)
                else:
                    xn = o.rmsnorm(h, o.h2u(self.sd[p + "post_attention_layernorm.weight"]), c.eps)
                    act = o.silu_mul(self._gemv(xn, p + "mlp.gate_proj", "E"), self._gemv(xn, p + "mlp.up_proj", "E"))
                    h = o.element_add_scale(h, self._gemv(act, p + "mlp.down_proj", "E"), 1.0, True)
            xn = o.rmsnorm(h, o.h2u(self.sd["model.norm.weight"]), c.eps)
            return o.gemm_nt(xn, o.h2u(self.sd["lm_head.weight"]), exact=True)
    return MoEOracle


BAR = 2e-3          # of the largest |logit|: test_gpu_model.py's bar for the fp32-accumulating W4 route against flavour E


def _routes(model, rows=None):
    def get(i):
        ids = model.layers[i].last_route[0].cpu().numpy()
        return ids if rows is None else ids[rows]
    return get


def _close(got, ref, what):
    err = np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max()
    assert err < BAR, (what, err)


@pytest.mark.parametrize("b", [1, 3, 8, 32])
def test_decode_against_oracle(oracle, dev, monkeypatch, b):
    """decode steps at 1 / 3 / 8 rows (the pair form: rows <= GPTQ_MOE_M_THRES, default 8) and 32 rows (the sorted grouped form)
    against the oracle chain; near-tie routing replays counted and bounded"""
    cfg = _cfg()
    sd = _moe_hf_state(cfg)
    model = _model(dev, sd, cfg, monkeypatch)
    om = _oracle_class()(oracle, cfg, sd, 128, b, 64)
    ctx = model.new_context(b, 64, 0)
    tokens = (np.arange(b) * 7 + 1).astype(np.int32)
    ctx.tokens.copy_(torch.from_numpy(tokens).to(dev))
    for step in range(2):
        got = model.encode(ctx).float().cpu().numpy()
        ref = om.step_moe(tokens, [step] * b, _routes(model))
        _close(got, ref, ("decode", b, step))
        nxt = ref.argmax(axis=1).astype(np.int32)
        model.advance(ctx, torch.from_numpy(nxt).to(dev))
        tokens = nxt
    assert om.replays <= max(1, b // 8), om.replays


def test_routes_and_threshold(oracle, dev, monkeypatch):
    """GPTQ_MOE_M_THRES moves rows between the pair form and the sorted form: the same bits either way; the fused GEMV route
    (ZL_MOE_ROUTE=fused, the reference's FUSE_GPTQ_MOE arithmetic) against the oracle at the bar of the reference's warp-reduce
    arithmetic (smoke(): 3e-3)"""
    cfg = _cfg()
    sd = _moe_hf_state(cfg)
    sorted_all, pairs_all = _model(dev, sd, cfg, monkeypatch, thres=0), _model(dev, sd, cfg, monkeypatch, thres=64)
    fused = _model(dev, sd, cfg, monkeypatch, route="fused")
    for b in (1, 3, 8):
        outs = []
        for m in (sorted_all, pairs_all, fused):
            ctx = m.new_context(b, 64, 0)
            ctx.tokens.copy_(torch.arange(b, dtype=torch.int32, device=dev) * 5 + 3)
            outs.append(m.encode(ctx).float().cpu().numpy())
        assert np.array_equal(outs[0], outs[1]), b
        om = _oracle_class()(oracle, cfg, sd, 128, b, 64)
        ref = om.step_moe((np.arange(b) * 5 + 3).astype(np.int32), [0] * b, _routes(fused))
        err = np.abs(outs[2] - ref).max() / np.abs(ref).max()
        assert err < 3e-3, (b, err)


def test_prefill_and_prefill_batch_against_oracle(oracle, dev, monkeypatch):
    """prefill of one prompt and prefill_batch of two against the oracle chain run over the prompts token by token (the same
    causal attention; the GPU's per-layer routing of the prompt rows replayed at near-ties)"""
    cfg = _cfg()
    sd = _moe_hf_state(cfg)
    model = _model(dev, sd, cfg, monkeypatch)
    prompts = [np.array([5, 9, 33, 2, 17, 101, 64, 3, 250, 7, 11], np.int32), np.array([400, 12, 77, 6, 90], np.int32)]
    MoEOracle = _oracle_class()

    def oracle_prompt(pr, routes):
        om = MoEOracle(oracle, cfg, sd, 128, 1, 64)
        for i, tok in enumerate(pr):
            ref = om.step_moe(np.array([tok], np.int32), [i], (lambda li, i=i: routes(li)[i:i + 1]) if routes else None)
        return ref[0]
    ctx = model.new_context(1, 64, 0)
    got = model.prefill(ctx, 0, torch.from_numpy(prompts[0]).to(dev)).float().reshape(-1).cpu().numpy()
    _close(got, oracle_prompt(prompts[0], _routes(model)), "prefill")
    ctxb = model.new_context(2, 64, 0)
    lb = model.prefill_batch(ctxb, [0, 1], [torch.from_numpy(p).to(dev) for p in prompts]).float().cpu().numpy()
    assert lb.shape == (2, cfg.vocab_size)
    offs = np.cumsum([0] + [len(p) for p in prompts])
    for j, pr in enumerate(prompts):          # the batched call routes all prompt rows at once: row offs[j] + i is prompt j's token i
        _close(lb[j], oracle_prompt(pr, lambda li, j=j: _routes(model)(li)[offs[j]:offs[j + 1]]), ("prefill_batch", j))


def test_captured_step_greedy_against_oracle(oracle, dev, monkeypatch):
    """step_greedy captured in a torch.cuda.graph and replayed: its logits against the oracle chain, its tokens = the eager step's
    (bit-identical: no float atomics anywhere in the MoE feed-forward)"""
    cfg = _cfg()
    sd = _moe_hf_state(cfg)
    model = _model(dev, sd, cfg, monkeypatch)
    b = 8
    tokens = (np.arange(b) * 11 + 2).astype(np.int32)
    ctxs = [model.new_context(b, 64, 0) for _ in range(3)]
    for c in ctxs:
        c.tokens.copy_(torch.from_numpy(tokens).to(dev))
    eager_logits, eager_next = (t.clone() for t in model.step_greedy(ctxs[0]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.step_greedy(ctxs[2])                               # warm the buffers outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits, nxt = model.step_greedy(ctxs[1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(logits, eager_logits) and torch.equal(nxt, eager_next)
    assert torch.equal(ctxs[1].tokens, ctxs[0].tokens)
    om = _oracle_class()(oracle, cfg, sd, 128, b, 64)
    ref = om.step_moe(tokens, [0] * b, _routes(model))
    _close(logits.float().cpu().numpy(), ref, "captured step_greedy")
