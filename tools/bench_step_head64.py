"""Decode step of head-size-64 geometries (MiniCPM-2B: 36 heads on 36; Llama-3.2-1B: 32 heads on 8), --layers layers, bf16,
unquantised: hipGraph replay of LLaMA.step_greedy, HIP events around every replay, median [p10, p90] ms per step
(the decode-step table of profiles/decode_attn_d64.txt).
usage: python tools/bench_step_head64.py [--tag new] [--layers 8] [--keys 1024] [--samples 40] [--batches 1,8,32]
Against another build of the library (A/B with the parent commit): build that commit elsewhere and run, in alternating processes,
    ZHILIGHT_AMD_SO=/path/to/its/libzhilight_amd.so python tools/bench_step_head64.py --tag parent
    python tools/bench_step_head64.py --tag new
A library that predates an entry point of this tree's list is loaded without it (the decode step calls none of those)."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="new")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--keys", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--batches", default="1,8,32")
    a = ap.parse_args()
    if os.environ.get("ZHILIGHT_AMD_SO"):
        older = ctypes.CDLL(_lib.SO_PATH)
        _lib.SYMBOLS[:] = [n for n in _lib.SYMBOLS if hasattr(older, n)]
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    dev, warm = torch.device("cuda:0"), 5
    geos = {"minicpm-2b": ModelConfig.minicpm_2b(),
            "llama-3.2-1b": ModelConfig(num_layers=16, dim_model=2048, num_heads=32, dim_head=64, dim_ff=8192, vocab_size=128256,
                                        num_kv_heads=8, rope_theta=500000.0, tie_lm_head=True, dtype="bfloat16")}
    for name, cfg in geos.items():
        cfg.num_layers = a.layers
        model = LLaMA(cfg, QuantConfig(0, 0), dev).init_random(seed=1)
        for batch in [int(v) for v in a.batches.split(",")]:
            len_buf = (a.keys + warm + a.samples + 8 + 63) // 64 * 64
            ctx = model.new_context(batch, len_buf, a.keys, fill_random=True)
            ctx.tokens.copy_(torch.randint(0, cfg.vocab_size, (batch,), device=dev, dtype=torch.int32))
            model.step_greedy(ctx)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                model.step_greedy(ctx)
            for _ in range(warm):
                g.replay()
            torch.cuda.synchronize()
            s = []
            for _ in range(a.samples):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                s.append(e0.elapsed_time(e1))
            s.sort()
            print(f"{a.tag:6s} {name:13s} {a.layers} layers batch {batch:2d} keys {a.keys}: {s[len(s) // 2]:.4f} "
                  f"[{s[len(s) // 10]:.4f}, {s[len(s) * 9 // 10]:.4f}] ms per step", flush=True)
            del g, ctx
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
