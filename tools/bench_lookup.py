"""The prompt-lookup drafter's cost (profiles/lookup_draft.txt is this tool's output).

  1. the launch alone (zl_lookup_draft), B x L x K: every shape is a captured graph of `--launches`
     calls on the same histories -- WARM: a row is at most 128 KB and stays in L2 between the calls of one replay -- the shapes'
     replays alternated, device events around each.  Two contents: ids uniform over a 128 k vocabulary (the first compare of a
     candidate end almost never hits) and over 4 symbols (a quarter of the ends extend backwards, every n-gram length ties).
     The histories must not grow from launch to launch here, so new_tokens holds its K + 1 ids behind a leading -1: the append path
     runs (the row is read and counted) and appends nothing.
  2. the whole step on the synthetic 32-layer model, 1 024 tokens of history, at the (B, K) rows of DESIGN 4's whole-step table:
     step_lookup (verify + the drafter launch; in a step the histories are COLD -- 4.8 GB of weights stream between two drafter
     launches) against verify on fixed drafts and against step_greedy, captured graphs, replays alternated.  Break-even accepted
     drafts per step = t / t_step_greedy - 1.  The histories repeat a 64-id motif, so the drafter matches (and extends to max_ngram)
     at every step; what the synthetic weights then accept is printed for what it is -- it says nothing about real text.

usage: python tools/bench_lookup.py [--launch-only | --step-only] [--reps 30] [--launches 200]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402

STEP_ROWS = [(1, 1), (2, 1), (1, 3), (4, 1), (2, 3), (1, 7), (8, 1), (4, 3), (2, 7), (16, 1), (8, 3), (4, 7)]


def _graph(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def _alternate(graphs, reps, warm=3):
    """replays of the named graphs in turn, one pair of device events around each -> {name: [ms per replay]}"""
    times = {n: [] for n in graphs}
    for r in range(warm + reps):
        for n, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            if r >= warm:
                times[n].append(e0.elapsed_time(e1))
    return times


def _stats(ms, per):
    us = sorted(t * 1e3 / per for t in ms)
    return statistics.median(us), us[len(us) // 10], us[-1 - len(us) // 10]


def launch_leg(dev, reps, launches):
    print("# the launch alone, warm histories: us per launch, median [p10 .. p90] over %d alternated replays of %d launches; max_ngram 3, "
          "min_ngram 1" % (reps, launches))
    print("#  B      L   K | 128 k symbols            matched | 4 symbols                matched")
    i32 = dict(dtype=torch.int32, device=dev)
    graphs, cells = {}, {}
    for b in (1, 8):
        for L in (1024, 8192, 32768):
            for k in (3, 7):
                for name, alphabet in (("vocab", 128 * 1024), ("four", 4)):
                    gen = torch.Generator(device="cpu").manual_seed(b * 100000 + L + k)
                    hist = torch.randint(0, alphabet, (b, L + 64), generator=gen, dtype=torch.int32).to(dev)
                    lens = torch.full((b,), L, **i32)
                    new = torch.randint(0, alphabet, (b, k + 1), generator=gen, dtype=torch.int32).to(dev)
                    new[:, 0] = -1
                    drafts, match = torch.empty((b, k), **i32), torch.empty((b, 2), **i32)

                    def run(hist=hist, lens=lens, new=new, drafts=drafts, match=match, k=k):
                        for _ in range(launches):
                            ops.lookup_draft(hist, lens, k, 3, 1, new_tokens=new, drafts=drafts, match=match)
                    graphs[(b, L, k, name)] = _graph(run)
                    cells[(b, L, k, name)] = (match, lens, hist, new, drafts)      # the graph does not keep its buffers alive
    t = _alternate(graphs, reps)
    for b in (1, 8):
        for L in (1024, 8192, 32768):
            for k in (3, 7):
                out = []
                for name in ("vocab", "four"):
                    match, lens = cells[(b, L, k, name)][:2]
                    assert int(lens.min()) == L == int(lens.max())
                    out.append("%7.2f [%6.2f .. %6.2f]   %d / %d" % (_stats(t[(b, L, k, name)], launches) + (int((match[:, 0] > 0).sum()), b)))
                print("  %2d  %5d  %2d | %s | %s" % (b, L, k, out[0], out[1]), flush=True)


def step_leg(dev, reps, rows):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    seq = 1024
    print("# whole step, synthetic Llama-3-8B GPTQ, 32 layers, %d tokens of history (a 64-id motif repeated); verify(attn=\"auto\"); ms per "
          "step, median [p10 .. p90] over %d alternated replays" % (seq, reps))
    print("#  B  K rows | step_greedy             | verify, fixed drafts    | step_lookup             | drafter in the step, us | break-even "
          "accepted drafts: verify  step_lookup | accepted per step by the synthetic weights")
    worst = 0.0
    for b, k in rows:
        len_q = k + 1
        len_buf = (seq + (reps + 8) * len_q + 63) // 64 * 64
        torch.manual_seed(7)
        ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in ("step", "verify", "lookup")}
        tok = torch.randint(0, cfg.vocab_size, (b,), device=dev, dtype=torch.int32)
        motif = torch.randint(0, cfg.vocab_size, (b, 64), dtype=torch.int32)
        tok.copy_(motif[:, 0])                                                       # the pending token continues the motif
        for c in ctxs.values():
            c.tokens.copy_(tok)
        for n in ("verify", "lookup"):
            for t, src in zip(ctxs[n].kv, ctxs["step"].kv):
                t.copy_(src)
        state = model.new_lookup(ctxs["lookup"], [motif[j].repeat(seq // 64) for j in range(b)], k)
        fixed = state.drafts.clone()
        len0 = state.hist_lens.clone()
        model.verify(ctxs["verify"], fixed)                                          # eager: the row-expanded tables
        model.step_lookup(ctxs["lookup"], state)
        graphs = {"step": _graph(lambda: model.step_greedy(ctxs["step"])),
                  "verify": _graph(lambda: model.verify(ctxs["verify"], fixed)),
                  "lookup": _graph(lambda: model.step_lookup(ctxs["lookup"], state))}
        t = _alternate(graphs, reps)
        calls = 1 + 2 + 3 + reps                                                     # eager, _graph's two, the warm and timed replays
        acc = float((state.hist_lens - len0).sum()) / (calls * b) - 1
        st = {n: tuple(v / 1e3 for v in _stats(t[n], 1)) for n in graphs}
        cell = lambda s: "%7.3f [%6.3f .. %6.3f]" % s                                # noqa: E731
        be = {n: st[n][0] / st["step"][0] - 1 for n in ("verify", "lookup")}
        worst = max(worst, be["lookup"])
        print("  %2d %2d  %3d | %s | %s | %s |        %7.1f          |                            %5.2f    %5.2f      | %.2f" % (
            b, k, b * len_q, cell(st["step"]), cell(st["verify"]), cell(st["lookup"]), (st["lookup"][0] - st["verify"][0]) * 1e3,
            be["verify"], be["lookup"], acc), flush=True)
        del graphs, ctxs, state
        torch.cuda.empty_cache()
    print("# break-even accepted drafts per step with the drafter inside: at most %.2f (the condition: below 1.0 at every shape: %s)"
          % (worst, "met" if worst < 1.0 else "MISSED"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lookup: needs a GPU")
    dev = torch.device("cuda:0")
    if not a.step_only:
        launch_leg(dev, a.reps, a.launches)
    if not a.launch_only:
        step_leg(dev, a.reps, STEP_ROWS)


if __name__ == "__main__":
    main()
