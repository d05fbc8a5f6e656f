"""Fused decode attention (rope + KV scatter + split-KV softmax + split merge) per-launch time, hipGraph-captured:
`layers` launches over distinct KV buffers per replay, like one decode step.
usage: python tools/bench_attn.py [--batch 1] [--seq 1024] [--layers 32]
(an in-launch split merge by the last-arriving workgroup was tried against the separate combine kernel:
13.1 vs ~13.9 us stand-alone, but +0.7 us per layer inside the decode step -- not kept)"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402


def head64(a):
    """--d 64: the attention launch pair at head size 64, the matrix-core kernel (algo 0) against the VALU kernel (algo 1) and
    zl_decode_attn_fused against rope_scatter_decode + algo 1.  One process, one hipGraph of `layers` launches per route, the
    routes' replays alternated, HIP events around every replay: median [p10, p90] us per launch (pair)."""
    dev, d = torch.device("cuda:0"), 64
    dt = torch.bfloat16 if a.bf16 else torch.float16
    i32 = dict(dtype=torch.int32, device=dev)
    print(f"# head size 64, {'bf16' if a.bf16 else 'fp16'}, {'BHSD' if a.bhsd else 'BSHD'}, {a.layers} launches per replay, {a.iters} samples per route")
    print("# H Hkv keys batch | algo0 (matrix cores) | algo1 (VALU) | fused | rope_scatter + algo1 | max |algo0 - algo1|, max |fused - unfused| of the outputs"
          "      us per launch pair: median [p10, p90]")
    for h, hkv in [tuple(int(v) for v in s.split(",")) for s in a.shapes.split(";")]:
        for seq in [int(v) for v in a.seqs.split(",")]:
            for batch in [int(v) for v in a.batches.split(",")]:
                len_buf = (seq + 64 + 63) // 64 * 64
                shape = (a.layers, 2, hkv, len_buf, d) if a.bhsd else (a.layers, 2, len_buf, hkv, d)
                kv = [torch.randn(shape, dtype=dt, device=dev) for _ in range(batch)]
                k_addrs = torch.tensor([[t[l, 0].data_ptr() for t in kv] for l in range(a.layers)], dtype=torch.int64, device=dev)
                v_addrs = torch.tensor([[t[l, 1].data_ptr() for t in kv] for l in range(a.layers)], dtype=torch.int64, device=dev)
                pos, buf_lens, valid = torch.full((batch,), seq, **i32), torch.full((batch,), len_buf, **i32), torch.full((batch,), seq + 1, **i32)
                cos, sin = ops.rope_cos_sin(pos, d, 1e4, True, None)
                qkv = torch.randn(batch, (h + 2 * hkv) * d, dtype=dt, device=dev)
                q, out = torch.empty(batch, h * d, dtype=dt, device=dev), torch.empty(batch, h * d, dtype=dt, device=dev)
                ws = ops.decode_attn_workspace(batch, 1, h, d, len_buf, dev)

                def attn(l):
                    ops.multi_query_attention_rag_buffer(q.view(batch, 1, h, d), buf_lens, k_addrs[l], v_addrs[l], None, 1.0 / math.sqrt(d),
                                                         len_buf, hkv, valid_lens=valid, bshd=not a.bhsd, out=out.view(batch, 1, h, d), workspace=ws)

                def scatter(l):
                    ops.rope_scatter_decode(cos, sin, qkv, pos, buf_lens, k_addrs[l], v_addrs[l], h, hkv, d, bshd=not a.bhsd, q_out=q)

                def fused(l):
                    ops.decode_attention_fused(cos, sin, qkv, pos, buf_lens, valid, k_addrs[l], v_addrs[l], h, hkv, d, 1.0 / math.sqrt(d),
                                               len_buf, bshd=not a.bhsd, out=out, workspace=ws)

                scatter(0)
                routes = (("0", (attn,)), ("1", (attn,)), ("0", (fused,)), ("1", (scatter, attn)))
                graphs, outs, caller_algo = [], [], os.environ.get("ZL_ATTN_MFMA")
                for algo, steps in routes:                     # the wrappers read ZL_ATTN_MFMA per call: the graph keeps the kernel
                    os.environ["ZL_ATTN_MFMA"] = "1" if algo == "0" else "0"
                    def run():
                        for l in range(a.layers):
                            for f in steps:
                                f(l)
                    run()                                      # once eagerly (code objects), then into the graph
                    torch.cuda.synchronize()
                    outs.append(out.float().clone())           # the last buffer set's rows, compared across the routes below
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        run()
                    graphs.append(g)
                if caller_algo is None:                        # the caller's setting again
                    os.environ.pop("ZL_ATTN_MFMA")
                else:
                    os.environ["ZL_ATTN_MFMA"] = caller_algo
                for g in graphs:
                    g.replay()
                torch.cuda.synchronize()
                samples = [[] for _ in graphs]
                for _ in range(a.iters):
                    for g, s in zip(graphs, samples):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        g.replay()
                        e1.record()
                        e1.synchronize()
                        s.append(e0.elapsed_time(e1) * 1e3 / a.layers)
                cells = []
                for s in samples:
                    s.sort()
                    cells.append(f"{s[len(s) // 2]:7.2f} [{s[len(s) // 10]:7.2f}, {s[len(s) * 9 // 10]:7.2f}]")
                diff = f"{(outs[0] - outs[1]).abs().max().item():.2e} {(outs[2] - outs[3]).abs().max().item():.2e}"
                print(f"{h:3d} {hkv:3d} {seq:5d} {batch:3d} | " + " | ".join(cells) + " | " + diff, flush=True)
                del kv, graphs


def _alternate(fns, iters, reps):
    """fns: callables that enqueue `reps` launches (graph replays, or eager loops); replays alternated, HIP events around each:
    per route the median [p10, p90] us per launch"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    samples = [[] for _ in fns]
    for _ in range(iters):
        for f, s in zip(fns, samples):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            s.append(e0.elapsed_time(e1) * 1e3 / reps)
    cells = []
    for s in samples:
        s.sort()
        cells.append(f"{s[len(s) // 2]:8.2f} [{s[len(s) // 10]:8.2f}, {s[len(s) * 9 // 10]:8.2f}]")
    return cells


def window64(a):
    """--d 64 --window N [--sinks]: the sliding-window kernels.  Decode: zl_decode_attn_window over `seq` valid keys against the
    only way the plain call bounds its work -- zl_decode_attn_ex with valid_lens = N on the same buffers, which computes something
    else (the FIRST N keys) and is a cost reference only -- and against the plain call over all `seq` keys; one hipGraph of `layers`
    launches over distinct buffers per route.  Prompt (--prompt-rows R): zl_prefill_attn_d64_window against zl_prefill_attn_d64 on the
    same R rows, eager launches.  Median [p10, p90] us per launch (pair)."""
    dev, d = torch.device("cuda:0"), 64
    dt = torch.bfloat16 if a.bf16 else torch.float16
    i32 = dict(dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(d)
    print(f"# head size 64, window {a.window}, sinks {a.sinks}, {'bf16' if a.bf16 else 'fp16'}, {'BHSD' if a.bhsd else 'BSHD'}, "
          f"{a.layers} launches per replay, {a.iters} samples per route")
    print("# decode: H Hkv keys batch | window | plain, valid_lens = window (cost reference) | plain, all keys      us per launch (pair): median [p10, p90]")
    for h, hkv in [tuple(int(v) for v in s.split(",")) for s in a.shapes.split(";")]:
        sinks = torch.randn(h, dtype=torch.float32, device=dev) if a.sinks else None
        for seq in [int(v) for v in a.seqs.split(",")]:
            for batch in [int(v) for v in a.batches.split(",")]:
                len_buf = (seq + 64 + 63) // 64 * 64
                shape = (a.layers, 2, hkv, len_buf, d) if a.bhsd else (a.layers, 2, len_buf, hkv, d)
                kv = [torch.randn(shape, dtype=dt, device=dev) for _ in range(batch)]
                k_addrs = torch.tensor([[t[l, 0].data_ptr() for t in kv] for l in range(a.layers)], dtype=torch.int64, device=dev)
                v_addrs = torch.tensor([[t[l, 1].data_ptr() for t in kv] for l in range(a.layers)], dtype=torch.int64, device=dev)
                buf_lens, valid, first = torch.full((batch,), len_buf, **i32), torch.full((batch,), seq, **i32), torch.full((batch,), a.window, **i32)
                q, out = torch.randn(batch, 1, h, d, dtype=dt, device=dev), torch.empty(batch, 1, h, d, dtype=dt, device=dev)
                ws = ops.decode_attn_workspace(batch, 1, h, d, len_buf, dev)
                graphs = []
                for kw in (dict(valid_lens=valid, window=a.window, sinks=sinks), dict(valid_lens=first), dict(valid_lens=valid)):
                    def run():
                        for l in range(a.layers):
                            ops.multi_query_attention_rag_buffer(q, buf_lens, k_addrs[l], v_addrs[l], None, scale, len_buf, hkv,
                                                                 bshd=not a.bhsd, out=out, workspace=ws, **kw)
                    run()
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        run()
                    graphs.append(g)
                cells = _alternate([g.replay for g in graphs], a.iters, a.layers)
                print(f"{h:3d} {hkv:3d} {seq:5d} {batch:3d} | " + " | ".join(cells), flush=True)
                del kv, graphs
    if a.prompt_rows:
        print("# prompt: H Hkv rows | window | plain      us per launch: median [p10, p90]")
        for h, hkv in [tuple(int(v) for v in s.split(",")) for s in a.shapes.split(";")]:
            sinks = torch.randn(h, dtype=torch.float32, device=dev) if a.sinks else None
            for rows in [int(v) for v in a.prompt_rows.split(",")]:
                q = torch.randn(rows, h, d, dtype=dt, device=dev)
                k, v = (torch.randn((hkv, rows, d) if a.bhsd else (rows, hkv, d), dtype=dt, device=dev) for _ in range(2))
                out = torch.empty_like(q)
                reps = 4
                def win():
                    for _ in range(reps):
                        ops.prefill_attention(q, k, v, 0, hkv, scale, not a.bhsd, out=out, window=a.window, sinks=sinks)
                def plain():
                    for _ in range(reps):
                        ops.prefill_attention(q, k, v, 0, hkv, scale, not a.bhsd, out=out)
                print(f"{h:3d} {hkv:3d} {rows:5d} | " + " | ".join(_alternate([win, plain], a.iters, reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=0, help="--d 64: the sliding-window leg (window64) with this window")
    ap.add_argument("--sinks", action="store_true", help="--d 64 --window N: with attention sinks")
    ap.add_argument("--prompt-rows", default="", help="--d 64 --window N: also time windowed prompt attention over these row counts")
    ap.add_argument("--d", type=int, default=128, choices=(64, 128), help="64: the head-size-64 leg (head64), algo 0 against algo 1 in one process")
    ap.add_argument("--shapes", default="36,36;32,8;14,2;64,8", help="--d 64: H,Hkv pairs")
    ap.add_argument("--seqs", default="1024,4096", help="--d 64: visible keys")
    ap.add_argument("--batches", default="1,8,32", help="--d 64")
    ap.add_argument("--bf16", action="store_true", help="--d 64: bf16 instead of fp16")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bhsd", action="store_true", help="KV buffers (Hkv, len_buf, D) instead of (len_buf, Hkv, D)")
    ap.add_argument("--alias", action="store_true", help="experiment: every task and layer reads the SAME KV buffer (cache-resident): the kernel's compute/latency floor")
    ap.add_argument("--unfused", action="store_true", help="rope+scatter launch, then zl_decode_attn (the matrix-core kernel when it applies)")
    ap.add_argument("--q8", action="store_true", help="INT8 KV cache: rope+quantise+scatter launch, then attention over codes")
    a = ap.parse_args()
    if a.d == 64:
        return window64(a) if a.window or a.sinks else head64(a)
    dev = torch.device("cuda:0")
    h, hkv, d = 32, 8, 128
    len_buf = (a.seq + 64 + 63) // 64 * 64
    shape = (a.layers, 2, hkv, len_buf, d) if a.bhsd else (a.layers, 2, len_buf, hkv, d)
    kv = [torch.randn(shape, dtype=torch.float16, device=dev) for _ in range(1 if a.alias else a.batch)]
    if a.alias:
        kv = [kv[0]] * a.batch
    k_addrs = torch.tensor([[t[l, 0].data_ptr() for t in kv] for l in range(a.layers)], dtype=torch.int64, device=dev)
    v_addrs = torch.tensor([[t[l, 1].data_ptr() for t in kv] for l in range(a.layers)], dtype=torch.int64, device=dev)
    if a.alias:
        k_addrs[:] = k_addrs[0, 0]
        v_addrs[:] = v_addrs[0, 0]
    i32 = dict(dtype=torch.int32, device=dev)
    pos = torch.full((a.batch,), a.seq, **i32)
    buf_lens = torch.full((a.batch,), len_buf, **i32)
    valid = torch.full((a.batch,), a.seq + 1, **i32)
    cos, sin = ops.rope_cos_sin(pos, d, 5e5, True, None)
    qkv = torch.randn(a.batch, (h + 2 * hkv) * d, dtype=torch.float16, device=dev)
    out = torch.empty(a.batch, h * d, dtype=torch.float16, device=dev)
    ws = ops.decode_attn_workspace(a.batch, 1, h, d, len_buf, dev)

    if a.q8:
        kv = [torch.randint(0, 256, shape, dtype=torch.uint8, device=dev) for _ in range(a.batch)]
        sc = [torch.rand(shape[:-1], dtype=torch.float32, device=dev) * 0.03 + 0.005 for _ in range(a.batch)]
        k_addrs = torch.tensor([[t[l, 0].data_ptr() for t in kv] for l in range(a.layers)], dtype=torch.int64, device=dev)
        v_addrs = torch.tensor([[t[l, 1].data_ptr() for t in kv] for l in range(a.layers)], dtype=torch.int64, device=dev)
        ks_addrs = torch.tensor([[t[l, 0].data_ptr() for t in sc] for l in range(a.layers)], dtype=torch.int64, device=dev)
        vs_addrs = torch.tensor([[t[l, 1].data_ptr() for t in sc] for l in range(a.layers)], dtype=torch.int64, device=dev)
        qb = torch.empty(a.batch, h * d, dtype=torch.float16, device=dev)

    qb2 = torch.empty(a.batch, h * d, dtype=torch.float16, device=dev)

    def run():
        if a.unfused:
            for l in range(a.layers):
                ops.rope_scatter_decode(cos, sin, qkv, pos, buf_lens, k_addrs[l], v_addrs[l], h, hkv, d, bshd=not a.bhsd, q_out=qb2)
                ops.multi_query_attention_rag_buffer(qb2.view(a.batch, 1, h, d), buf_lens, k_addrs[l], v_addrs[l], None,
                                                     1.0 / math.sqrt(d), len_buf, hkv, valid_lens=valid, bshd=not a.bhsd,
                                                     out=out.view(a.batch, 1, h, d), workspace=ws)
            return
        if a.q8:
            for l in range(a.layers):
                ops.rope_quant_scatter_decode(cos, sin, qkv, pos, buf_lens, k_addrs[l], v_addrs[l], ks_addrs[l], vs_addrs[l],
                                              h, hkv, d, bshd=not a.bhsd, q_out=qb)
                ops.multi_query_attention_rag_buffer_quant(qb.view(a.batch, 1, h, d), buf_lens, k_addrs[l], v_addrs[l],
                                                           ks_addrs[l], vs_addrs[l], None, 1.0 / math.sqrt(d), len_buf, hkv,
                                                           valid_lens=valid, bshd=not a.bhsd,
                                                           out=out.view(a.batch, 1, h, d), workspace=ws)
            return
        for l in range(a.layers):
            ops.decode_attention_fused(cos, sin, qkv, pos, buf_lens, valid, k_addrs[l], v_addrs[l], h, hkv, d,
                                       1.0 / math.sqrt(d), len_buf, bshd=not a.bhsd, out=out, workspace=ws)
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (a.iters * a.layers)
    kvb = a.batch * 2 * hkv * (a.seq + 1) * (d + 4 if a.q8 else d * 2)
    print(f"batch={a.batch} seq={a.seq}: {us:7.2f} us/launch   KV {kvb / 1e6:.2f} MB -> {kvb / us / 1e3:7.1f} GB/s"
          "")


if __name__ == "__main__":
    main()
