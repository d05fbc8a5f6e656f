"""MXFP4 linears and the MXFP4 decode step on the Llama-3-8B geometry (DESIGN 4 "MXFP4 weights", profiles/mxfp4.txt).

    python tools/bench_mxfp4.py [--iters 100] [--no-linears] [--no-steps] [--layers 32]

Method: hipEvent pairs around every iteration after 10 warm-ups, >= 100 iterations; the linears rotate through >= 4
weight buffers totalling more than 256 MB, so every read of a weight comes from HBM -- an iteration is one hipGraph replay of one
launch per buffer, reported per launch (eager launches measure the host: ~14 us each); figures are the median with p10 .. p90.
  linears   the four projections (qkv 6144 x 4096, attn_out 4096 x 4096, gate|up 28672 x 4096 with silu*mul, w_out 4096 x 14336 with
            the residual) at M = 1, 4, 8, 32, 512: us and the fraction of 8 TB/s on K N 0.53125 + (M K + M N) 2 bytes
  steps     the whole decode step (hipGraph replay of step_greedy) at batch 1 / 8 / 32, sequence 1024, in tokens/s, for quant type 11
            (MXFP4), type 0 (fp16), type 5 (GPTQ) on its default route and type 5 on the plain route (ZL_FUSE_QKV_ROPE=0): the
            like-for-like comparison, MXFP4 having no fused qkv + rotary launch
One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zhilight_amd import ops  # noqa: E402
from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig  # noqa: E402

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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if not args.no_linears:
        bench_linears(dev, args.iters)
    if not args.no_steps:
        bench_steps(dev, args.iters, args.layers)


if __name__ == "__main__":
    main()
