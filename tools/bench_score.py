"""Scoring rows against the lm_head at Llama-3 geometry (K = 4096, N = 128 256, fp16), rows 256 / 1024 / 4096:

    fused     ops.lm_head_score: the soft-max statistics in the GEMM tile's epilogue, no logits stored -- with the launch order the
              library picks by row count, and with each of the two orders forced (`order` of zl_lm_head_score_ex: 0 = all row tiles
              of a column block adjacent, 1 = the same with each XCD taking a contiguous range of tiles)
    unfused   ops.lm_head_score_unfused: gemm_nt + fp32 torch logsumexp / gather / argmax over slabs of rows (kernels that exist
              without the fused one: the cost of the feature without it)
    gemm      ops.gemm_nt alone, all rows: the floor of the unfused form (it stores the logits and computes nothing on them)

    python tools/bench_score.py [--reps 20] [--rows 256,1024,4096] [--out FILE]

The variants are alternated inside ONE process, each call between two HIP events after a warm-up; median, minimum and the spread
(max - min) / median of the repetitions are reported, the peak of torch.cuda.max_memory_allocated over one call of each, FLOPs and
algorithmic bytes from the shapes.  The fused results are checked against the unfused ones before anything is timed.  Fails
without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402

K, N = 4096, 128256
PEAK_F16_TFLOPS = 2500.0       # MI355X dense fp16 MFMA peak (spec, ~2.5 PFLOP/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="256,1024,4096")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_score needs a GPU")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(4321)
    w = (torch.randn(N, K, generator=gen, device=dev) * (2.0 / K ** 0.5)).half()
    lines, result = [], {}
    for m in [int(r) for r in a.rows.split(",")]:
        x = torch.randn(m, K, generator=gen, device=dev).half()
        labels = torch.randint(0, N, (m,), generator=gen, device=dev, dtype=torch.int32)
        ws = ops.lm_head_score_workspace(m, N, dev)

        def fused(order):
            return lambda: ops.lm_head_score(x, w, labels, workspace=ws, order=order)

        forms = {"fused": fused(-1), "fused_plain": fused(0), "fused_xcd": fused(1),
                 "unfused": lambda: ops.lm_head_score_unfused(x, w, labels),
                 "gemm": lambda: ops.gemm_nt(x, w)}
        want = forms["unfused"]()
        for name in ("fused", "fused_plain", "fused_xcd"):
            got = forms[name]()
            torch.cuda.synchronize()
            if not (torch.equal(got.greedy, want.greedy) and torch.equal(got.label_logit, want.label_logit)
                    and float((got.lse - want.lse).abs().max()) < 1e-3):
                raise SystemExit(name + " differs from the unfused chain: not timing a wrong kernel")
        del want, got
        peak = {}
        for name, f in forms.items():
            for _ in range(2):
                f()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            f()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
        times = {name: [] for name in forms}
        for _ in range(a.reps):
            for name, f in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)            # us
        flops = 2.0 * m * N * K
        by_fused = N * K * 2 + m * K * 2 + m * 24
        by_unfused = by_fused + m * N * (2 + 2 + 4 + 3 * 4)              # logits written, read, their fp32 copy written and read thrice
        lines.append(f"rows {m}: K {K} N {N} fp16; {flops / 1e12:.2f} TFLOP; algorithmic bytes fused {by_fused / 1e6:.0f} MB, "
                     f"unfused {by_unfused / 1e6:.0f} MB, gemm {(by_fused + m * N * 2) / 1e6:.0f} MB")
        res = {}
        for name, t in times.items():
            med, mn, mx = statistics.median(t), min(t), max(t)
            tf = flops / med / 1e6
            res[name] = {"median_us": med, "min_us": mn, "spread": (mx - mn) / med, "tflops": tf, "peak_mem_bytes": peak[name]}
            lines.append(f"  {name:13s} median {med:10.1f} us  min {mn:10.1f} us  spread {(mx - mn) / med:6.3f}  {tf:7.1f} TFLOP/s "
                         f"({100 * tf / PEAK_F16_TFLOPS:4.1f} % of fp16 MFMA peak)  peak memory {peak[name] / 1e6:8.1f} MB  ({a.reps} reps)")
        lines.append(f"  fused / unfused (medians) {res['fused']['median_us'] / res['unfused']['median_us']:.3f}   "
                     f"fused / gemm {res['fused']['median_us'] / res['gemm']['median_us']:.3f}")
        result[str(m)] = res
        del x, labels, ws, forms
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"bench": "score", "k": K, "n": N, "reps": a.reps, "results": result}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
