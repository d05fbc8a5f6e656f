"""Prompt encode (TTFT) of the Llama-3-8B GPTQ-Int4 model: python tools/bench_prefill.py [--seq 1024] [--layers 32]
(run under rocprofv3 --kernel-trace --stats for the per-kernel split).
--prompts N: N seeded prompts of --seq tokens, encoded batched (LLaMA.prefill_batch, one pass) and sequentially (N LLaMA.prefill
calls), the two forms alternated in one process and timed with HIP events: ms per call and prompt tokens/s of each.
--model minicpm_2b: the unquantised bf16 MiniCPM-2B geometry (head size 64) instead; with --d64-ab its prompt encode and the attention
launch alone on the head-size-64 prompt kernel against ZL_PREFILL_D64=0, alternated: median, p10, p90 (profiles/prefill_attn_d64.txt)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seq", type=int, default=1024)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--prompts", type=int, default=0)
ap.add_argument("--model", choices=("llama3_8b", "minicpm_2b"), default="llama3_8b")
ap.add_argument("--d64-ab", action="store_true",
                help="head size 64: the prompt kernel against ZL_PREFILL_D64=0 (the mask form), alternated in one process -- the "
                     "whole prompt encode of --model, then the attention launch alone at (H, Hkv) = (36, 36) and (32, 8)")
a = ap.parse_args()
dev = torch.device("cuda:0")
cfg = ModelConfig.llama3_8b() if a.model == "llama3_8b" else ModelConfig.minicpm_2b()
cfg.num_layers = a.layers
model = LLaMA(cfg, QuantConfig(5, 128) if a.model == "llama3_8b" else QuantConfig(0, 0), dev).init_random(seed=1)
len_buf = (a.seq + 64 + 63) // 64 * 64


def _timed(fn, inner=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def _alternate(what, forms, reps, inner=1):
    """forms: name -> callable; one warm-up of each, then `reps` rounds that time every form in turn (`inner` calls per sample)"""
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            times[name].append(_timed(fn, inner))
    for name, ts in times.items():
        ts.sort()
        n = len(ts)
        print(f"{what} {name}: median {ts[n // 2]:.3f} ms  p10 {ts[n // 10]:.3f}  p90 {ts[min(n - 1, n * 9 // 10)]:.3f}  ({n} samples)",
              flush=True)


if a.d64_ab:
    from zhilight_amd import ops
    if cfg.dim_head != 64:
        sys.exit("--d64-ab: a head-size-64 model (--model minicpm_2b)")
    ctx = model.new_context(1, len_buf, 0)
    prompt = torch.randint(0, cfg.vocab_size, (a.seq,), device=dev, dtype=torch.int32)

    def encode(route):
        def fn():
            os.environ["ZL_PREFILL_D64"] = route
            model.prefill(ctx, 0, prompt)
        return fn
    _alternate(f"prefill {a.model} seq={a.seq} layers={a.layers}", {"kernel": encode("1"), "mask form": encode("0")}, a.reps)
    os.environ.pop("ZL_PREFILL_D64")
    for h, hkv in ((36, 36), (32, 8)):
        q = torch.randn(a.seq, h, 64, device=dev).to(cfg.torch_dtype)
        k, v = (torch.randn(len_buf, hkv, 64, device=dev).to(cfg.torch_dtype) for _ in range(2))
        mask = torch.tril(torch.ones(a.seq, len_buf, dtype=torch.int8, device=dev)).contiguous()
        ws = ops.decode_attn_workspace(1, a.seq, h, 64, len_buf, dev)
        lens_dev = torch.tensor([len_buf], dtype=torch.int32, device=dev)
        k_tab, v_tab = ops.make_ptr_table([k]), ops.make_ptr_table([v])
        out = torch.empty_like(q)
        _alternate(f"attention alone seq={a.seq} h={h} hkv={hkv}", {
            "kernel": lambda: ops.prefill_attention(q, k, v, 0, hkv, 0.125, out=out),
            "mask form": lambda: ops.multi_query_attention_rag_buffer(q.view(1, a.seq, h, 64), lens_dev, k_tab, v_tab, mask, 0.125, len_buf,
                                                                      hkv, out=out.view(1, a.seq, h, 64), workspace=ws)}, a.reps, inner=20)
    sys.exit(0)
if a.prompts > 0:
    n = a.prompts
    g = torch.Generator().manual_seed(1234)
    prompts = [torch.randint(0, cfg.vocab_size, (a.seq,), generator=g, dtype=torch.int32).to(dev) for _ in range(n)]
    ctx = model.new_context(n, len_buf, 0)
    tasks = list(range(n))

    def batched():
        model.prefill_batch(ctx, tasks, prompts)

    def sequential():
        for t in tasks:
            model.prefill(ctx, t, prompts[t])
    batched()
    sequential()
    torch.cuda.synchronize()
    times = {"batched": [], "sequential": []}
    for _ in range(a.reps):
        for name, fn in (("batched", batched), ("sequential", sequential)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    for name, ts in times.items():
        ms = sorted(ts)[len(ts) // 2]
        print(f"prefill {name} prompts={n} seq={a.seq} layers={a.layers}: {ms:.2f} ms per call (median of {len(ts)}: "
              f"{', '.join(f'{t:.2f}' for t in ts)})  {n * a.seq / ms * 1e3:.0f} prompt tokens/s")
    sys.exit(0)
ctx = model.new_context(1, len_buf, 0)
prompt = torch.randint(0, cfg.vocab_size, (a.seq,), device=dev, dtype=torch.int32)
model.prefill(ctx, 0, prompt)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(a.reps):
    model.prefill(ctx, 0, prompt)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / a.reps
if a.model != "llama3_8b":                              # unquantised linears: the time alone
    sys.exit(print(f"prefill {a.model} seq={a.seq} layers={a.layers}: {ms:.2f} ms"))
flops =2.0 * a.seq * sum(l.weight.n * l.weight.k for lay in model.layers for l in (lay.qkv, lay.attn_out, lay.w_in_gated, lay.w_out))
print(f"prefill seq={a.seq} layers={a.layers}: {ms:.2f} ms  ({flops / ms / 1e9:.1f} TFLOP/s on the linears alone)")
