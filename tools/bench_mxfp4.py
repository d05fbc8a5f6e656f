"""MXFP4 linears and the MXFP4 decode step on the Llama-3-8B geometry (DESIGN 4 "MXFP4 weights", profiles/mxfp4.txt).

    python tools/bench_mxfp4.py [--iters 100] [--no-linears] [--no-steps] [--layers 32]
    python tools/bench_mxfp4.py --act mxfp8 [--iters 100] [--layers 32]      (DESIGN 4 "MXFP8 activations", profiles/mxfp4_a8.txt)
    python tools/bench_mxfp4.py --act mxfp4 [--iters 100] [--layers 32]      (DESIGN 4 "MXFP4 activations", profiles/mxfp4_a4.txt)
    python tools/bench_mxfp4.py --moe [--iters 100]                          (DESIGN 4 "MXFP4 experts", profiles/mxfp4_moe.txt)
    python tools/bench_mxfp4.py --moe --act mxfp8 [--iters 100]              (DESIGN 4 "MXFP8 activations for the experts", profiles/mxfp4_moe_a8.txt)
    python tools/bench_mxfp4.py --moe --act mxfp4 [--iters 100]              (DESIGN 4 "MXFP4 activations for the experts", profiles/mxfp4_moe_a4.txt)

Method: hipEvent pairs around every iteration after 10 warm-ups, >= 100 iterations; the linears rotate through >= 4
weight buffers totalling more than 256 MB, so every read of a weight comes from HBM -- an iteration is one hipGraph replay of one
launch per buffer, reported per launch (eager launches measure the host: ~14 us each); figures are the median with p10 .. p90.
  linears   the four projections (qkv 6144 x 4096, attn_out 4096 x 4096, gate|up 28672 x 4096 with silu*mul, w_out 4096 x 14336 with
            the residual) at M = 1, 4, 8, 32, 512: us and the fraction of 8 TB/s on K N 0.53125 + (M K + M N) 2 bytes
  steps     the whole decode step (hipGraph replay of step_greedy) at batch 1 / 8 / 32, sequence 1024, in tokens/s, for quant type 11
            (MXFP4), type 0 (fp16), type 5 (GPTQ) on its default route and type 5 on the plain route (ZL_FUSE_QKV_ROPE=0): the
            like-for-like comparison, MXFP4 having no fused qkv + rotary launch
  --act mxfp8  the prompt route with MXFP8 activations against the weight-only tiled route, in the same run, alternating the two:
            the four projections at M = 128, 512, 2048 -- the weight-only launch, the quantiser, the A8 GEMM and quantiser + GEMM as one
            replay, "speedup" = weight-only / (quantiser + GEMM) -- and the time to the first token of a 1024-token prompt (LLaMA.prefill,
            eager launches between two events: both ways pay the same launches but for the quantisers) on ONE model whose linears are
            switched between the routes, so both ways read the same weights
  --act mxfp4  the same run with a third route, W4A4: weight-only tiled, MXFP8 (quantiser + GEMM) and MXFP4 (ops.mxfp4_act_quantize +
            ops.mxfp4_a4_linear) alternate on the same weights; "a4_speedup" = weight-only / (quantiser + GEMM), "a4_over_a8" = MXFP8
            route / MXFP4 route, "a4_p90_below_weight_only_p10" is the condition on the route's threshold; the time to the first token
            for the three routes
  --moe     the routed feed-forward on MXFP4 expert stacks (DESIGN 4 "MXFP4 experts", profiles/mxfp4_moe.txt) at the Qwen3-30B-A3B
            geometry (128 experts, top-k 8, dim_model 2048, moe_intermediate_size 768) at 1, 4, 8, 32, 512 rows.  An iteration is one
            hipGraph replay of Mxfp4MoEEncoderLayer.moe (router, top-k, [sort,] gate|up, down, combine) on each of 16 layers (5 GB of
            experts: the few experts a small batch touches do not stay in the caches), per layer, with the pairs form (up to 32 rows)
            and the grouped form forced in turn -- their crossover is the layer's m_thres.  Against, in the same run: "loop", what the
            code before these kernels could do with the same weights -- ops.mxfp4_linear per active expert over gathered rows, which
            needs the loads on the host, so it is timed eagerly between two events, and so is layer.moe next to it ("eager") -- and
            "gptq", MoEEncoderLayer.moe (GPTQ W4A16 experts, grouped route) at the same geometry, as replays.
  --moe --act mxfp8  the same layers and replays at 64, 128, 512, 2048 rows with the grouped form forced: the weight-only experts
            (ops.mxfp4_moe_grouped) against the MXFP8 route (two ops.mxfp8_quantize + two ops.mxfp4_moe_a8_grouped), alternating in one
            process on the same weights in four rounds; "ratio" = weight-only / MXFP8 over the replays paired in order; "quantise" = a
            replay of the route's two quantiser launches alone and their share of the MXFP8 route's median.
  --moe --act mxfp4  the same run with a third route, W4A4 (two ops.mxfp4_act_quantize + two ops.mxfp4_moe_a4_grouped): the three routes
            alternate on the same weights; "a4_ratio" = weight-only / MXFP4 and "a8_over_a4" = MXFP8 / MXFP4 over the replays paired in
            order, "a4_p90_below_weight_only_p10" is the condition on MXFP4_MOE_A4_ABOVE_ROWS, "a4_quantise" the two MXFP4 quantisers.
One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zhilight_amd import ops  # noqa: E402
from zhilight_amd.llama import LLaMA, ModelConfig, MoEEncoderLayer, Mxfp4MoEEncoderLayer, QuantConfig  # noqa: E402

HBM = 8.0e12
LINEARS = (("qkv", 6144, 4096, 0), ("attn_out", 4096, 4096, ops.EPI_RESIDUAL), ("gate_up", 28672, 4096, ops.EPI_SILU_MUL),
           ("w_out", 4096, 14336, ops.EPI_RESIDUAL))
ROWS = (1, 4, 8, 32, 512)


def quantiles(ts):
    ts = sorted(ts)
    pick = lambda q: ts[min(len(ts) - 1, int(q * len(ts)))]  # noqa: E731
    return pick(0.5), pick(0.1), pick(0.9)


def timed(fn, iters, warmup=10):
    for i in range(warmup):
        fn(i)
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(pairs):
        a.record()
        fn(warmup + i)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e-3 for a, b in pairs]


def random_weight(n, k, dev, gen, row_interleave):
    """random codes under checkpoint-like scale bytes (2^-7 .. 2^-5): the kernels' time does not depend on the values"""
    codes = torch.randint(0, 256, (n, k // 2), dtype=torch.uint8, device=dev, generator=gen)
    scales = torch.randint(120, 123, (n, k // 32), dtype=torch.uint8, device=dev, generator=gen)
    return ops.Mxfp4Weight(codes, scales, row_interleave)


def bench_linears(dev, iters):
    gen = torch.Generator(device=dev).manual_seed(1)
    for name, n, k, epi in LINEARS:
        wbytes = n * k * 0.53125
        nbuf = max(4, int(256e6 // wbytes) + 2)
        ws = [random_weight(n, k, dev, gen, bool(epi & ops.EPI_SILU_MUL)) for _ in range(nbuf)]
        for dtype in (torch.float16, torch.bfloat16):
            for m in ROWS:
                x = torch.randn(m, k, device=dev, generator=gen).to(dtype)
                n_out = n // 2 if epi & ops.EPI_SILU_MUL else n
                out = torch.zeros(m, n_out, dtype=dtype, device=dev)
                res = out if epi & ops.EPI_RESIDUAL else None
                run = lambda w: ops.mxfp4_linear(x, w, residual=res, out=out, epilogue=epi & ops.EPI_SILU_MUL)  # noqa: E731
                run(ws[0])
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()               # one launch per buffer: a replay is a full rotation, without the
                with torch.cuda.graph(graph):                # host's launch cost between the kernels
                    for w in ws:
                        run(w)
                p50, p10, p90 = (t / nbuf for t in quantiles(timed(lambda i: graph.replay(), iters)))
                del graph
                nbytes = wbytes + (m * k + m * n) * 2
                print(json.dumps({"what": "linear", "name": name, "n": n, "k": k, "m": m, "dtype": str(dtype).split(".")[1],
                                  "route": ops.mxfp4_route(m, n, k), "buffers": nbuf, "us": round(p50 * 1e6, 2),
                                  "us_p10": round(p10 * 1e6, 2), "us_p90": round(p90 * 1e6, 2),
                                  "hbm_fraction": round(nbytes / p50 / HBM, 4)}), flush=True)
        del ws
        torch.cuda.empty_cache()


def bench_act(dev, iters, layers, rows=(128, 512, 2048), prompt_len=1024, a4=False):
    gen = torch.Generator(device=dev).manual_seed(1)
    us = lambda q: [round(t * 1e6, 2) for t in q]  # noqa: E731
    for name, n, k, epi in LINEARS:
        nbuf = max(4, int(256e6 // (n * k * 0.53125)) + 2)
        ws = [random_weight(n, k, dev, gen, bool(epi & ops.EPI_SILU_MUL)) for _ in range(nbuf)]
        for dtype in (torch.float16, torch.bfloat16):
            for m in rows:
                x = torch.randn(m, k, device=dev, generator=gen).to(dtype)
                out = torch.zeros(m, n // 2 if epi & ops.EPI_SILU_MUL else n, dtype=dtype, device=dev)
                kw = dict(residual=out if epi & ops.EPI_RESIDUAL else None, out=out, epilogue=epi & ops.EPI_SILU_MUL)
                q = ops.mxfp8_quantize(x)
                legs = {"weight_only": lambda w: ops.mxfp4_linear(x, w, **kw), "quantise": lambda w: ops.mxfp8_quantize(x, out=q),
                        "a8_gemm": lambda w: ops.mxfp4_a8_linear(q[0], q[1], w, dtype, **kw),
                        "a8": lambda w: ops.mxfp4_a8_linear(*ops.mxfp8_quantize(x, out=q), w, dtype, **kw)}
                if a4:
                    q4 = ops.mxfp4_act_quantize(x)
                    legs.update({"a4_quantise": lambda w: ops.mxfp4_act_quantize(x, out=q4),
                                 "a4_gemm": lambda w: ops.mxfp4_a4_linear(q4[0], q4[1], w, dtype, **kw),
                                 "a4": lambda w: ops.mxfp4_a4_linear(*ops.mxfp4_act_quantize(x, out=q4), w, dtype, **kw)})
                graphs = {}
                for leg, run in legs.items():
                    run(ws[0])
                    torch.cuda.synchronize()
                    graphs[leg] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs[leg]):
                        for w in ws:
                            run(w)
                times = {leg: [] for leg in legs}
                for _ in range(4):                                 # alternate the legs: four rounds of iters / 4 replays each
                    for leg, g in graphs.items():
                        times[leg] += timed(lambda i: g.replay(), max(1, iters // 4), warmup=3)
                res = {leg: [t / nbuf for t in quantiles(ts)] for leg, ts in times.items()}
                del graphs
                w16, a8 = res["weight_only"], res["a8"]
                rec = {"what": "act_linear", "name": name, "n": n, "k": k, "m": m, "dtype": str(dtype).split(".")[1], "buffers": nbuf,
                       **{leg + "_us_p50_p10_p90": us(r) for leg, r in res.items()},
                       "speedup_p50": round(w16[0] / a8[0], 3), "speedup_p10_p90": [round(w16[1] / a8[2], 3), round(w16[2] / a8[1], 3)],
                       "a8_tflops": round(2.0 * m * n * k / a8[0] * 1e-12, 1)}
                if a4:
                    r4 = res["a4"]
                    rec.update({"a4_speedup_p50": round(w16[0] / r4[0], 3), "a4_over_a8_p50": round(a8[0] / r4[0], 3),
                                "a4_p90_below_weight_only_p10": r4[2] < w16[1], "a4_gemm_tflops": round(2.0 * m * n * k / res["a4_gemm"][0] * 1e-12, 1)})
                print(json.dumps(rec), flush=True)
        del ws
        torch.cuda.empty_cache()
    cfg = ModelConfig.llama3_8b()
    cfg.num_layers = layers
    model = LLaMA(cfg, QuantConfig(11, 32), dev).init_random(seed=1234)
    prompt = torch.randint(0, cfg.vocab_size, (prompt_len,), device=dev, dtype=torch.int32, generator=gen)
    ctx = model.new_context(1, prompt_len + 64, 0)

    def prefill(act):
        for layer in model.layers:
            for lin in layer.linears():
                lin.act_quant = act
        ctx.positions.zero_(), ctx.placement.zero_(), ctx.valid_lens.zero_()
        model.prefill(ctx, 0, prompt)
    times = {"": [], "mxfp8": [], **({"mxfp4": []} if a4 else {})}
    for _ in range(4):
        for act in times:
            times[act] += timed(lambda i: prefill(act), max(1, iters // 10), warmup=1)
    w16, a8 = quantiles(times[""]), quantiles(times["mxfp8"])
    rec = {"what": "ttft", "layers": layers, "prompt": prompt_len, "weight_only_ms_p50_p10_p90": [round(t * 1e3, 3) for t in w16],
           "a8_ms_p50_p10_p90": [round(t * 1e3, 3) for t in a8], "speedup_p50": round(w16[0] / a8[0], 3)}
    if a4:
        r4 = quantiles(times["mxfp4"])
        rec.update({"a4_ms_p50_p10_p90": [round(t * 1e3, 3) for t in r4], "a4_speedup_p50": round(w16[0] / r4[0], 3)})
    print(json.dumps(rec), flush=True)


def moe_loop(layer, xn):
    """the routed feed-forward without the expert-grouped kernels: one mxfp4_linear pair per active expert over its gathered rows"""
    c = layer.cfg
    k = c.moe_top_k
    weights, ids = ops.moe_top_k_softmax(ops.gemm_nt_f32(xn, layer.router), k, norm_topk_prob=c.norm_topk_prob)
    flat = ids.reshape(-1).long()
    order = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=c.moe_num_experts).tolist()           # the host has to know the loads
    down = torch.empty((flat.numel(), c.dim_model), dtype=xn.dtype, device=xn.device)
    pos = 0
    for e, cnt in enumerate(counts):
        if cnt:
            sel = order[pos:pos + cnt]
            act = ops.mxfp4_linear(xn[sel // k], ops.Mxfp4Weight(layer.w_up.codes[e], layer.w_up.scales[e], True), epilogue=ops.EPI_SILU_MUL)
            down[sel] = ops.mxfp4_linear(act, ops.Mxfp4Weight(layer.w_down.codes[e], layer.w_down.scales[e]))
            pos += cnt
    return ops.moe_sum_experts(down, ops.arange_i32(flat.numel(), xn.device), weights)


def bench_moe(dev, iters, nbuf=16, rows=ROWS):
    gen = torch.Generator(device=dev).manual_seed(1)
    geo = dict(num_layers=1, dim_model=2048, num_heads=32, dim_head=128, num_kv_heads=4, dim_ff=768, model_type="qwen3_moe", qk_norm="head",
               moe_num_experts=128, moe_top_k=8, moe_intermediate_size=768, norm_topk_prob=True)
    e, d, ff = 128, 2048, 768
    u8 = lambda lo, hi, *shape: torch.randint(lo, hi, shape, dtype=torch.uint8, device=dev, generator=gen)  # noqa: E731
    router = lambda dt: (torch.randn(e, d, device=dev, generator=gen) / d ** 0.5).to(dt)  # noqa: E731

    def mx_layer(dt):
        layer = Mxfp4MoEEncoderLayer(ModelConfig(dtype=dt, **geo), QuantConfig(11, 32), 0)
        layer.router = router(layer.cfg.torch_dtype)
        layer.w_up = ops.Mxfp4MoEWeight(u8(0, 256, e, 2 * ff, d // 2), u8(120, 123, e, 2 * ff, d // 32), True)
        layer.w_down = ops.Mxfp4MoEWeight(u8(0, 256, e, d, ff // 2), u8(120, 123, e, d, ff // 32))
        return layer

    def gptq_layer():
        layer = MoEEncoderLayer(ModelConfig(**geo), QuantConfig(5, 128), 0)
        layer.router = router(torch.float16)
        km = lambda n, k: ([torch.randint(-2 ** 31, 2 ** 31 - 1, (n, k // 8), dtype=torch.int32, device=dev, generator=gen) for _ in range(e)],  # noqa: E731
                           [u8(1, 16, n, k // 128) for _ in range(e)],
                           [(torch.rand(n, k // 128, device=dev, generator=gen) * 0.01 + 1e-3).half() for _ in range(e)])
        layer.w_up = ops.W4MMoEWeight.from_k_major(*km(2 * ff, d), 128, row_interleave=True)
        layer.w_down = ops.W4MMoEWeight.from_k_major(*km(d, ff), 128)
        return layer

    def replay_us(layers, x):
        for layer in layers[:2]:
            layer.moe(x)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for layer in layers:
                layer.moe(x)
        return [round(t / len(layers) * 1e6, 2) for t in quantiles(timed(lambda i: graph.replay(), iters))]
    for dt in ("half", "bfloat16"):
        layers = [mx_layer(dt) for _ in range(nbuf)]
        for m in rows:
            x = torch.randn(m, d, device=dev, generator=gen).to(layers[0].cfg.torch_dtype)
            rec = {"what": "moe", "dtype": dt, "rows": m, "pairs": m * 8, "bm": ops.mxfp4_moe_bm(m * 8, e), "buffers": nbuf}
            for form, thres in (("pairs", 1 << 30), ("grouped", 0)):
                if form == "grouped" or m <= 32:
                    for layer in layers:
                        layer.m_thres = thres
                    rec[form + "_us_p50_p10_p90"] = replay_us(layers, x)
            if dt == "half":
                eager = lambda fn: [round(t * 1e6, 1) for t in quantiles(timed(lambda i: fn(layers[i % nbuf], x), iters))]  # noqa: E731
                rec["grouped_eager_us_p50_p10_p90"] = eager(lambda layer, x: layer.moe(x))
                rec["loop_eager_us_p50_p10_p90"] = eager(moe_loop)
            print(json.dumps(rec), flush=True)
        del layers
        torch.cuda.empty_cache()
    layers = [gptq_layer() for _ in range(nbuf)]
    for m in rows:
        x = torch.randn(m, d, device=dev, generator=gen).half()
        print(json.dumps({"what": "moe_gptq", "rows": m, "route": "pairs" if m <= layers[0].m_thres else "grouped", "buffers": nbuf,
                          "us_p50_p10_p90": replay_us(layers, x)}), flush=True)


def bench_moe_act(dev, iters, nbuf=16, rows=(64, 128, 512, 2048), a4=False):
    gen = torch.Generator(device=dev).manual_seed(1)
    e, d, ff, k = 128, 2048, 768, 8
    geo = dict(num_layers=1, dim_model=d, num_heads=32, dim_head=128, num_kv_heads=4, dim_ff=ff, model_type="qwen3_moe", qk_norm="head",
               moe_num_experts=e, moe_top_k=k, moe_intermediate_size=ff, norm_topk_prob=True)
    u8 = lambda lo, hi, *shape: torch.randint(lo, hi, shape, dtype=torch.uint8, device=dev, generator=gen)  # noqa: E731
    us = lambda ts, n: [round(t / n * 1e6, 2) for t in quantiles(ts)]  # noqa: E731
    for dt in ("half", "bfloat16"):
        layers = []
        for _ in range(nbuf):
            layer = Mxfp4MoEEncoderLayer(ModelConfig(dtype=dt, **geo), QuantConfig(11, 32), 0)
            layer.m_thres = 0                                      # the grouped form at every row count
            layer.router = (torch.randn(e, d, device=dev, generator=gen) / d ** 0.5).to(layer.cfg.torch_dtype)
            layer.w_up = ops.Mxfp4MoEWeight(u8(0, 256, e, 2 * ff, d // 2), u8(120, 123, e, 2 * ff, d // 32), True)
            layer.w_down = ops.Mxfp4MoEWeight(u8(0, 256, e, d, ff // 2), u8(120, 123, e, d, ff // 32))
            layers.append(layer)
        for m in rows:
            x = torch.randn(m, d, device=dev, generator=gen).to(layers[0].cfg.torch_dtype)
            act = torch.randn(m * k, ff, device=dev, generator=gen).to(x.dtype)

            def quantise(layer):
                ops.mxfp8_quantize(x)
                ops.mxfp8_quantize(act)

            def quantise4(layer):
                ops.mxfp4_act_quantize(x)
                ops.mxfp4_act_quantize(act)
            moe = lambda layer: layer.moe(x)  # noqa: E731
            legs = {"weight_only": ("", moe), "a8": ("mxfp8", moe), "quantise": ("", quantise)}
            if a4:
                legs.update({"a4": ("mxfp4", moe), "a4_quantise": ("", quantise4)})
            graphs = {}
            for leg, (act_quant, run) in legs.items():
                for layer in layers:                               # the route of the leg, above 32 rows
                    layer.quant, layer.a8_above_rows, layer.a4_above_rows = QuantConfig(11, 32, act_quant=act_quant), 32, 32
                run(layers[0])
                torch.cuda.synchronize()
                graphs[leg] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[leg]):
                    for layer in layers:
                        run(layer)
            times = {leg: [] for leg in legs}
            for _ in range(4):                                     # alternate the legs: four rounds of iters / 4 replays each
                for leg, g in graphs.items():
                    times[leg] += timed(lambda i: g.replay(), max(1, iters // 4), warmup=3)
            del graphs
            ratio = quantiles([a / b for a, b in zip(times["weight_only"], times["a8"])])
            w16, a8, qt = (us(times[leg], nbuf) for leg in ("weight_only", "a8", "quantise"))
            rec = {"what": "moe_act", "dtype": dt, "rows": m, "pairs": m * k, "bm_weight_only": ops.mxfp4_moe_bm(m * k, e),
                   "bm_a8": ops.mxfp4_moe_a8_bm(m * k, e), "buffers": nbuf, "weight_only_us_p50_p10_p90": w16,
                   "a8_us_p50_p10_p90": a8, "ratio_p50_p10_p90": [round(r, 3) for r in ratio],
                   "a8_p90_below_weight_only_p10": a8[2] < w16[1], "quantise_us_p50_p10_p90": qt,
                   "quantise_share": round(qt[0] / a8[0], 3)}
            if a4:
                r4, q4 = us(times["a4"], nbuf), us(times["a4_quantise"], nbuf)
                paired = lambda num: [round(r, 3) for r in quantiles([a / b for a, b in zip(times[num], times["a4"])])]  # noqa: E731
                rec.update({"bm_a4": ops.mxfp4_moe_a4_bm(m * k, e), "a4_us_p50_p10_p90": r4, "a4_ratio_p50_p10_p90": paired("weight_only"),
                            "a8_over_a4_p50_p10_p90": paired("a8"), "a4_p90_below_weight_only_p10": r4[2] < w16[1],
                            "a4_quantise_us_p50_p10_p90": q4, "a4_quantise_share": round(q4[0] / r4[0], 3)})
            print(json.dumps(rec), flush=True)
        del layers
        torch.cuda.empty_cache()


def bench_steps(dev, iters, layers, seq=1024):
    cfg = ModelConfig.llama3_8b()
    cfg.num_layers = layers
    for label, quant, env in (("mxfp4 (type 11)", QuantConfig(11, 32), {}), ("fp16 (type 0)", QuantConfig(0, 0), {}),
                              ("gptq (type 5) default route", QuantConfig(5, 128), {}),
                              ("gptq (type 5) plain route", QuantConfig(5, 128), {"ZL_FUSE_QKV_ROPE": "0"})):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            model = LLaMA(cfg, quant, dev)
            model.init_synthetic(seed=1234) if quant.quant_type == 5 else model.init_random(seed=1234)
            for batch in (1, 8, 32):
                len_buf = (seq + iters + 16 + 63) // 64 * 64
                torch.manual_seed(1234)
                ctx = model.new_context(batch, len_buf, seq, fill_random=True)
                ctx.tokens.copy_(torch.randint(0, cfg.vocab_size, (batch,), device=dev, dtype=torch.int32))
                model.step_greedy(ctx)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    model.step_greedy(ctx)
                p50, p10, p90 = quantiles(timed(lambda i: graph.replay(), iters, warmup=4))
                print(json.dumps({"what": "decode_step", "model": label, "layers": layers, "batch": batch, "seq": seq,
                                  "weight_bytes": model.weight_bytes(), "tokens_per_s": round(batch / p50, 1),
                                  "tokens_per_s_p10": round(batch / p90, 1), "tokens_per_s_p90": round(batch / p10, 1),
                                  "ms_per_step": round(p50 * 1e3, 4)}), flush=True)
                del graph, ctx
            del model
            torch.cuda.empty_cache()
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--no-linears", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--act", choices=("", "mxfp8", "mxfp4"), default="",
                    help="mxfp8: the A/B of the MXFP8-activation prompt route, nothing else; mxfp4: the same with the W4A4 route as a third leg")
    ap.add_argument("--moe", action="store_true", help="the routed feed-forward on MXFP4 expert stacks, nothing else")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.moe:
        return bench_moe_act(dev, args.iters, a4=args.act == "mxfp4") if args.act else bench_moe(dev, args.iters)
    if args.act:
        return bench_act(dev, args.iters, args.layers, a4=args.act == "mxfp4")
    if not args.no_linears:
        bench_linears(dev, args.iters)
    if not args.no_steps:
        bench_steps(dev, args.iters, args.layers)


if __name__ == "__main__":
    main()
