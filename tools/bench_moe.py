"""Fused MoE GEMVs (zl_w4a16_moe_up / _down) at a decode step's shapes: per-launch time and algorithmic HBM rate.
usage: python tools/bench_moe.py [--m 1] [--hidden 2048] [--ff 768] [--experts 128] [--topk 8] [--shared 0] [--layers 24]
       python tools/bench_moe.py --grouped [--ms 1,8,32,512,2048]: the whole routed feed-forward after the router (fused GEMV pair
       against the pair form and sort + grouped gate|up + grouped down + sum_experts) per token count, bytes / HBM share for the decode sizes and
       FLOPs / MFMA share for prompts (from shapes: distinct experts' int4 weights, 2 x pairs x (3 ff x hidden) FLOPs), crossover"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=1)
ap.add_argument("--hidden", type=int, default=2048)
ap.add_argument("--ff", type=int, default=768)
ap.add_argument("--experts", type=int, default=128)
ap.add_argument("--topk", type=int, default=8)
ap.add_argument("--shared", type=int, default=0)
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--grouped", action="store_true")
ap.add_argument("--ms", default="1,8,32,512,2048")
a = ap.parse_args()
dev = torch.device("cuda:0")
g = 128
HBM, MFMA = 8.0e12, 2.5e15          # MI355X peaks: HBM3E bytes/s, dense fp16 MFMA FLOP/s


def _graph_us(fn, layers, iters):
    fn(0)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            for i in range(layers):
                fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (iters * layers)


def grouped_leg():
    """per layer: fused = moe_up + moe_down on ZLW4 stacks; grouped = sort + gate|up + down + combine on ZLW4M stacks; random codes"""
    def w4(n, k, il):
        L = ops.W4Weight.layout(n, k, g)
        return ops.W4MoEWeight(a.experts, n, k, g, torch.randint(-2 ** 31, 2 ** 31 - 1, (a.experts, L.qw_bytes // 4), dtype=torch.int32, device=dev),
                               (torch.rand(a.experts, L.scales_bytes // 2, device=dev) * 0.005 + 1e-4).half(),
                               torch.randint(-2 ** 15, 2 ** 15 - 1, (a.experts, L.zeros_bytes // 2), dtype=torch.int16, device=dev), il)

    def w4m(n, k, il):
        L = ops.W4MWeight.layout(n, k, g)
        ws = [ops.W4MWeight.random(n, k, g, dev) for _ in range(1)]
        qw = ws[0].qw.repeat(a.experts).view(a.experts, -1).contiguous()
        meta = ws[0].meta.repeat(a.experts).view(a.experts, -1).contiguous()
        assert qw.shape[1] * 4 == L.qw_bytes
        return ops.W4MMoEWeight(a.experts, n, k, g, qw, meta, il)
    layers = max(1, min(a.layers, 4))
    fu = [(w4(2 * a.ff, a.hidden, True), w4(a.hidden, a.ff, False)) for _ in range(layers)]
    gr = [(w4m(2 * a.ff, a.hidden, True), w4m(a.hidden, a.ff, False)) for _ in range(layers)]
    rows, cross = [], None
    for m in [int(v) for v in a.ms.split(",")]:
        ids = torch.stack([torch.randperm(a.experts, device=dev)[:a.topk] for _ in range(m)]).to(torch.int32)
        wts = torch.rand(m, a.topk, device=dev)
        x = torch.randn(m, a.hidden, device=dev).half()
        loads = torch.bincount(ids.reshape(-1).long(), minlength=a.experts).to(torch.int32)
        p = m * a.topk

        def fused(i):
            ops.moe_down(ops.moe_up(x, fu[i][0], ids), fu[i][1], ids, wts)

        def grouped(i):
            pair = ops.arange_i32(p, dev)
            _, order = ops.sort_pairs_i32(ids.reshape(-1), pair, max_key=a.experts)
            act = ops.moe_gemm_grouped(x, gr[i][0], loads, order, p, in_div=a.topk, epilogue=ops.EPI_SILU_MUL)
            ops.moe_sum_experts(ops.moe_gemm_grouped(act, gr[i][1], loads, order, p, out_scatter=True), pair, wts)
        def pairs(i):
            pair = ops.arange_i32(p, dev)
            act = ops.moe_gemm_pairs(x, gr[i][0], ids, in_div=a.topk, epilogue=ops.EPI_SILU_MUL)
            ops.moe_sum_experts(ops.moe_gemm_pairs(act, gr[i][1], ids), pair, wts)
        tf, tg, tp = _graph_us(fused, layers, a.iters), _graph_us(grouped, layers, a.iters), _graph_us(pairs, layers, a.iters)
        active = int((loads > 0).sum())
        per_expert = 3 * a.ff * a.hidden * (0.5 + 4.0 / g)             # int4 codes + per-group scale / zero
        byt_f, byt_g = p * per_expert, active * per_expert
        flops = 2.0 * p * 3 * a.ff * a.hidden
        if m <= 32:
            share = f"bytes fused {byt_f / 1e6:7.1f} MB ({byt_f / (tf * 1e-6) / HBM:5.1%} HBM)  grouped {byt_g / 1e6:7.1f} MB ({byt_g / (tg * 1e-6) / HBM:5.1%} HBM)"
        else:
            share = f"{flops / 1e9:8.1f} GFLOP  fused {flops / (tf * 1e-6) / MFMA:5.1%} MFMA  grouped {flops / (tg * 1e-6) / MFMA:5.1%} MFMA"
        print(f"M={m:5d} pairs={p:6d} active experts={active:4d}: fused {tf:9.2f} us  pair form {tp:9.2f} us  sorted grouped {tg:9.2f} us  "
              f"{share}", flush=True)
        rows.append((m, tf, tg, tp))
    cross = next((m for m, tf, tg, tp in rows if tg < tp), None)
    print(f"GPTQ_MOE_M_THRES crossover: the sorted grouped form is faster than the pair form from M = {cross} (of {a.ms})")
    cross_f = next((m for m, tf, tg, tp in rows if min(tg, tp) < tf), None)
    print(f"against the fused GEMVs: the ZLW4M route is faster from M = {cross_f}")


if a.grouped:
    grouped_leg()
    sys.exit(0)


def stack(n, k, interleave):
    L = ops.W4Weight.layout(n, k, g)
    e = a.experts + a.shared
    qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (e, L.qw_bytes // 4), dtype=torch.int32, device=dev)
    sc = (torch.rand(e, L.scales_bytes // 2, device=dev) * 0.005 + 1e-4).half()
    zs = torch.randint(-2 ** 15, 2 ** 15 - 1, (e, L.zeros_bytes // 2), dtype=torch.int16, device=dev)
    return ops.W4MoEWeight(e, n, k, g, qw, sc, zs, interleave)


ups = [stack(2 * a.ff, a.hidden, True) for _ in range(a.layers)]
downs = [stack(a.hidden, a.ff, False) for _ in range(a.layers)]
t = a.topk + a.shared
ids = torch.stack([torch.randperm(a.experts, device=dev)[:a.topk] for _ in range(a.m)]).to(torch.int32)
wts = torch.rand(a.m, a.topk, device=dev)
x = torch.randn(a.m, a.hidden, device=dev).half()
mid = torch.empty(a.m, t, a.ff, dtype=torch.float16, device=dev)
out = torch.empty(a.m, a.hidden, dtype=torch.float16, device=dev)
for name, fn, byt in (("moe_up", lambda i: ops.moe_up(x, ups[i], ids, a.shared, out=mid), a.m * t * 2 * a.ff * a.hidden * (0.5 + 2.5 / g)),
                      ("moe_down", lambda i: ops.moe_down(mid, downs[i], ids, wts, a.shared, out=out), a.m * t * a.hidden * a.ff * (0.5 + 2.5 / g))):
    fn(0)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            for i in range(a.layers):
                fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (a.iters * a.layers)
    print(f"{name:9s} M={a.m} experts/token={t} ({a.hidden} x {a.ff}): {us:8.2f} us/launch  {byt / us / 1e3:8.1f} GB/s ({byt / us / 1e3 / 80:.1f}% of 8 TB/s)  {byt / 1e6:.1f} MB")
