"""Prompt chunks on top of an INT8 K/V cache, one layer's attention at Llama-3-8B head geometry (H 32, Hkv 8, D 128, fp16):

    A  zl_dequant_group of K and of V per task into fp16 buffers (2 b launches) + zl_prefill_attn_varlen on them: the reference's
       fall-back (attention.cpp:510-516) with the kernels that existed before the in-kernel dequant
    B  zl_prefill_attn_varlen_q8: the history dequantised where the kernel stages its tiles, no buffer
    C  zl_prefill_attn_varlen alone on an fp16 cache holding the same values (B - C: the price of the conversion)

    python tools/bench_prefill_q8.py [--rounds 12] [--inner 16] [--out FILE]

Shapes: (i) 8 tasks x 128 new rows on 1 024 cached rows each (second turns of a serving batch); (ii) one task x 512 new rows on
3 584 cached rows (a long chunked prompt).  The three forms are alternated in ONE process; a round of a form is `inner` calls
between two HIP events, each call on the next of a ring of cache sets whose bytes exceed the 256 MB last-level cache (A's fp16
temporaries are one set, reused: they are written and read back at once, as in the fall-back).  Each form is timed eagerly (launches
issued from Python, what the model does) and replayed from a captured graph (no host time between the launches); medians and
minima of the rounds are reported per shape and mode.  B's output is checked bit for bit against A's before anything is timed."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402

H, HKV, D = 32, 8, 128
LLC_BYTES = 256 << 20


def build(b, s_new, hist, dev, gen):
    """ring of cache sets + the call's rows for b tasks of s_new rows on `hist` cached rows"""
    lb = hist + s_new
    set_bytes = 2 * b * lb * HKV * D                       # K + V codes of one set
    n_sets = -(-(LLC_BYTES + (LLC_BYTES >> 2)) // set_bytes)
    total = b * s_new
    rnd = lambda *shape: torch.randn(*shape, generator=gen, device=dev, dtype=torch.float32)
    q = (rnd(total, H, D) * 1.5).half()
    k_new, v_new = rnd(total, HKV, D).half(), rnd(total, HKV, D).half()
    lens, pos0, len_bufs = [s_new] * b, [hist] * b, [lb] * b
    plan = ops.prefill_varlen_plan(lens, pos0, len_bufs, dev)
    sets = []
    for _ in range(n_sets):
        st = {"kc": [], "vc": [], "ks": [], "vs": [], "kf": [], "vf": []}
        for i in range(b):
            for c, sc, f, new in (("kc", "ks", "kf", k_new), ("vc", "vs", "vf", v_new)):
                codes = torch.randint(0, 256, (lb, HKV, D), generator=gen, device=dev, dtype=torch.uint8)
                scales = torch.rand(lb, HKV, generator=gen, device=dev) * 0.01 + 0.009   # (code - 128) * scale: about unit variance
                full = torch.empty((lb, HKV, D), dtype=torch.float16, device=dev)
                ops.dequant_group(codes[:hist], scales[:hist], 128, torch.float16, out=full[:hist])
                full[hist:] = new[i * s_new:(i + 1) * s_new]
                st[c].append(codes); st[sc].append(scales); st[f].append(full)
        st["tabs_q8"] = [ops.make_ptr_table(st[n]) for n in ("kc", "vc", "ks", "vs")]
        st["tabs_f16"] = [ops.make_ptr_table(st[n]) for n in ("kf", "vf")]
        sets.append(st)
    # A's temporaries: one set, the call's own rows already behind the history (the fall-back appends them with a copy of its own)
    tk = [sets[0]["kf"][i].clone() for i in range(b)]
    tv = [sets[0]["vf"][i].clone() for i in range(b)]
    tmp_tabs = [ops.make_ptr_table(tk), ops.make_ptr_table(tv)]
    out = torch.empty_like(q)
    scale = D ** -0.5

    def form_a(st):
        for i in range(b):
            ops.dequant_group(st["kc"][i][:hist], st["ks"][i][:hist], 128, torch.float16, out=tk[i][:hist])
            ops.dequant_group(st["vc"][i][:hist], st["vs"][i][:hist], 128, torch.float16, out=tv[i][:hist])
        ops.prefill_attention_varlen(q, lens, pos0, tmp_tabs[0], tmp_tabs[1], len_bufs, HKV, scale, True, out=out, groups=0, plan=plan)

    def form_b(st):
        ops.prefill_attention_varlen_q8(q, lens, pos0, k_new, v_new, *st["tabs_q8"], len_bufs, HKV, scale, out=out, groups=0, plan=plan)

    def form_c(st):
        ops.prefill_attention_varlen(q, lens, pos0, *st["tabs_f16"], len_bufs, HKV, scale, True, out=out, groups=0, plan=plan)

    form_a(sets[1 % n_sets])
    want = out.clone()
    form_b(sets[1 % n_sets])
    torch.cuda.synchronize()
    if not torch.equal(out.view(torch.int16), want.view(torch.int16)):
        raise SystemExit("B differs from A: not timing a wrong kernel")
    return sets, {"A": form_a, "B": form_b, "C": form_c}, n_sets, set_bytes


def measure(sets, forms, rounds, inner, graph):
    n_sets = len(sets)
    cursor = {name: 0 for name in forms}

    def batch(name):
        for _ in range(inner):
            forms[name](sets[cursor[name] % n_sets])
            cursor[name] += 1

    runners = {}
    if graph:
        side = torch.cuda.Stream()
        for name in forms:
            with torch.cuda.stream(side):
                batch(name)                                 # warm: code objects loaded before capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                batch(name)
            runners[name] = g.replay
    else:
        runners = {name: (lambda name=name: batch(name)) for name in forms}
    for name in forms:
        runners[name]()
    torch.cuda.synchronize()
    times = {name: [] for name in forms}
    for _ in range(rounds):
        for name in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runners[name]()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / inner)          # us per call
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--inner", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.rounds < 10:
        raise SystemExit("--rounds: at least 10")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1234)
    lines, result = [], {}
    for label, b, s_new, hist in (("i", 8, 128, 1024), ("ii", 1, 512, 3584)):
        sets, forms, n_sets, set_bytes = build(b, s_new, hist, dev, gen)
        head = (f"shape ({label}): {b} task(s) x {s_new} new rows on {hist} cached rows, H {H} Hkv {HKV} D {D} fp16; ring of {n_sets} "
                f"cache sets, {n_sets * set_bytes >> 20} MB of codes ({n_sets * set_bytes >> 19} MB as fp16 for C); "
                f"A's temporaries {2 * hist * HKV * D * 2 * b >> 10} KB, B's none")
        lines.append(head)
        for graph in (False, True):
            mode = "graph" if graph else "eager"
            times = measure(sets, forms, a.rounds, a.inner, graph)
            med = {n: statistics.median(t) for n, t in times.items()}
            mn = {n: min(t) for n, t in times.items()}
            for n in ("A", "B", "C"):
                lines.append(f"  {mode:5s} {n}: median {med[n]:8.2f} us  min {mn[n]:8.2f} us  ({a.rounds} rounds x {a.inner} calls)")
            lines.append(f"  {mode:5s} B / A (medians) {med['B'] / med['A']:.3f}   B - C (medians) {med['B'] - med['C']:+.2f} us")
            result[f"{label}_{mode}"] = {"median_us": med, "min_us": mn, "b_over_a": med["B"] / med["A"]}
        del sets, forms
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"bench": "prefill_q8", "rounds": a.rounds, "inner": a.inner, "results": result}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
