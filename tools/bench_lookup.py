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
  --sampler: the speculative SAMPLING step instead (profiles/spec_sample.txt is this leg's output), at the same (B, K) rows:
  3. the accept alone: ops.spec_sample_accept (T 0.8, top-k 40, top-p 0.95, log-probabilities and uniforms written) against
     ops.spec_accept and against ops.sample_advance on the same B x (K + 1) warm rows of 128 256 fp16 logits, captured graphs of
     `--launches` calls, replays alternated.
  4. the whole step: step_lookup(sampler=) against step_sample -- what a sampling user runs today -- and against the greedy
     step_lookup and step_greedy, all four in ONE alternated run.  Break-even accepted drafts per step under sampling =
     t(step_lookup(sampler)) / t(step_sample) - 1, beside the greedy t(step_lookup) / t(step_greedy) - 1.  Under T > 0 a lookup
     draft is accepted with probability p(draft) per position, so the synthetic weights accept next to nothing here; that figure
     says nothing about real text either way.

  --stop: the stop conditions inside the speculative step (profiles/stop_step.txt, with tools/bench_sample.py --stop):
  5. the whole captured step_lookup with and without a stop state whose stops never hit (two stop ids, two four-id stop sequences and a
     length limit per task), replays alternated, at (B, K) = (1, 3), (8, 3) and (16, 1) -- a speculative step holds at most 32 rows, so
     16 tasks are the most it takes.  The step without stop= issues exactly the launches of the commit before the stop conditions.

  --grammar: the token automaton inside the speculative sampling step (profiles/sample_grammar.txt, with tools/bench_sample.py --grammar):
  6. the whole captured step_lookup(sampler=) without automaton tables, with tables and every task unconstrained, and with every task
     in a state that allows every other class, replays alternated, at --stop's (B, K) rows.  The zl_* calls of an eager step are
     counted and must be as many with the grammar as without.

usage: python tools/bench_lookup.py [--launch-only | --step-only] [--sampler | --stop | --grammar] [--reps 30] [--launches 200]"""
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


VOCAB = 128256
SAMPLER = dict(temperature=0.8, top_k=40, top_p=0.95)


def accept_leg(dev, reps, launches, rows):
    print("# the accept alone, warm rows of %d fp16 logits (normal, sigma 2): us per call, median [p10 .. p90] over %d alternated replays of %d "
          "calls; spec_sample_accept and sample_advance at T %.1f, top-k %d, top-p %.2f with log-probabilities"
          % (VOCAB, reps, launches, SAMPLER["temperature"], SAMPLER["top_k"], SAMPLER["top_p"]))
    print("#  B  K rows | spec_accept (2 launches)   | sample_advance (1 launch)  | spec_sample_accept (2)     | over spec_accept, us | over "
          "sample_advance, us")
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    graphs, keep = {}, []
    for b, k in rows:
        len_q = k + 1
        m = b * len_q
        gen = torch.Generator(device="cpu").manual_seed(100 * b + k)
        logits = (torch.randn((m, VOCAB), generator=gen) * 2).to(torch.float16).to(dev)
        drafts = logits.view(b, len_q, VOCAB)[:, :k].float().argmax(dim=2).to(torch.int32).contiguous()     # the greedy path accepts every draft
        acc, out, tok = torch.empty(b, **i32), torch.empty((b, len_q), **i32), torch.zeros(b, **i32)
        per = lambda count: dict(temperature=torch.full((count,), SAMPLER["temperature"], **f32),           # noqa: E731
                                 top_k=torch.full((count,), SAMPLER["top_k"], **i32), top_p=torch.full((count,), SAMPLER["top_p"], **f32),
                                 seeds=torch.arange(count, dtype=torch.int64, device=dev), draws=torch.zeros(count, dtype=torch.int64, device=dev))
        task, row = per(b), per(m)
        row.update(tokens=torch.zeros(m, **i32), logprobs=torch.empty(m, **f32), u_out=torch.empty(m, **f32))
        task.update(tokens=tok, accepted=acc, out_tokens=out, out_logprobs=torch.empty((b, len_q), **f32), logprobs=torch.empty(b, **f32),
                    u_out=torch.empty((b, len_q), **f32))

        def greedy(logits=logits, drafts=drafts, tok=tok, acc=acc, out=out):
            for _ in range(launches):
                ops.spec_accept(logits, drafts, tokens=tok, accepted=acc, out_tokens=out)

        def plain(logits=logits, row=row):
            for _ in range(launches):
                ops.sample_advance(logits, **row)

        def sampled(logits=logits, drafts=drafts, task=task):
            for _ in range(launches):
                ops.spec_sample_accept(logits, drafts, **task)
        graphs[(b, k, "greedy")], graphs[(b, k, "plain")], graphs[(b, k, "sampled")] = _graph(greedy), _graph(plain), _graph(sampled)
        keep.append((logits, drafts, task, row))
    t = _alternate(graphs, reps)
    for b, k in rows:
        st = {n: _stats(t[(b, k, n)], launches) for n in ("greedy", "plain", "sampled")}
        cell = lambda s: "%7.2f [%7.2f .. %7.2f]" % s                                # noqa: E731
        print("  %2d %2d  %3d | %s | %s | %s |       %7.2f        |      %7.2f" % (
            b, k, b * (k + 1), cell(st["greedy"]), cell(st["plain"]), cell(st["sampled"]), st["sampled"][0] - st["greedy"][0],
            st["sampled"][0] - st["plain"][0]), flush=True)


def sampler_step_leg(dev, reps, rows):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    seq = 1024
    print("# whole step, synthetic Llama-3-8B GPTQ, 32 layers, %d tokens of history (a 64-id motif repeated); verify(attn=\"auto\"); sampler: "
          "T %.1f, top-k %d, top-p %.2f; ms per step, median [p10 .. p90] over %d alternated replays of the four steps"
          % (seq, SAMPLER["temperature"], SAMPLER["top_k"], SAMPLER["top_p"], reps))
    print("#  B  K rows | step_greedy             | step_sample             | step_lookup             | step_lookup(sampler)    | sampler over "
          "greedy lookup, us | break-even accepted drafts: greedy  sampling | accepted per step by the synthetic weights: greedy  sampling")
    worst = {"greedy": (0.0, None), "sampling": (0.0, None)}
    missed = []
    for b, k in rows:
        len_q = k + 1
        len_buf = (seq + (reps + 8) * len_q + 63) // 64 * 64
        torch.manual_seed(7)
        names = ("step", "sample", "lookup", "lookup_s")
        ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in names}
        motif = torch.randint(0, cfg.vocab_size, (b, 64), dtype=torch.int32)
        for c in ctxs.values():
            c.tokens.copy_(motif[:, 0])                                              # the pending token continues the motif
        for n in names[1:]:
            for t, src in zip(ctxs[n].kv, ctxs["step"].kv):
                t.copy_(src)
        hist = [motif[j].repeat(seq // 64) for j in range(b)]
        look = {n: model.new_lookup(ctxs[n], hist, k) for n in ("lookup", "lookup_s")}
        len0 = look["lookup"].hist_lens.clone()
        samp = {n: model.new_sampler(ctxs[n], seed=5, **SAMPLER) for n in ("sample", "lookup_s")}
        model.step_lookup(ctxs["lookup"], look["lookup"])                            # eager: the row-expanded tables, the sampler's row buffers
        model.step_lookup(ctxs["lookup_s"], look["lookup_s"], sampler=samp["lookup_s"])
        graphs = {"step": _graph(lambda: model.step_greedy(ctxs["step"])),
                  "sample": _graph(lambda: model.step_sample(ctxs["sample"], samp["sample"])),
                  "lookup": _graph(lambda: model.step_lookup(ctxs["lookup"], look["lookup"])),
                  "lookup_s": _graph(lambda: model.step_lookup(ctxs["lookup_s"], look["lookup_s"], sampler=samp["lookup_s"]))}
        t = _alternate(graphs, reps)
        calls = 1 + 2 + 3 + reps                                                     # eager, _graph's two, the warm and timed replays
        acc = {n: float((look[n].hist_lens - len0).sum()) / (calls * b) - 1 for n in look}
        assert int(samp["lookup_s"].draws.sum()) == int((look["lookup_s"].hist_lens - len0).sum())      # one draw per emitted token
        st = {n: tuple(v / 1e3 for v in _stats(t[n], 1)) for n in graphs}
        cell = lambda s: "%7.3f [%6.3f .. %6.3f]" % s                                # noqa: E731
        be = {"greedy": st["lookup"][0] / st["step"][0] - 1, "sampling": st["lookup_s"][0] / st["sample"][0] - 1}
        for n in be:
            if be[n] > worst[n][0]:
                worst[n] = (be[n], (b, k))
        if be["sampling"] >= 1.0:
            missed.append((b, k))
        print("  %2d %2d  %3d | %s | %s | %s | %s |            %7.1f          |                            %5.2f   %5.2f     |"
              "                                              %.2f    %.2f" % (
                  b, k, b * len_q, cell(st["step"]), cell(st["sample"]), cell(st["lookup"]), cell(st["lookup_s"]),
                  (st["lookup_s"][0] - st["lookup"][0]) * 1e3, be["greedy"], be["sampling"], acc["lookup"], acc["lookup_s"]), flush=True)
        del graphs, ctxs, look, samp
        torch.cuda.empty_cache()
    print("# break-even accepted drafts per step under sampling, t(step_lookup(sampler)) / t(step_sample) - 1: at most %.2f at (B, K) = %s; "
          "greedy, t(step_lookup) / t(step_greedy) - 1: at most %.2f at %s" % (worst["sampling"] + worst["greedy"]))
    print("# the yardstick, below 1.0 at every shape: %s" % ("met" if not missed else "MISSED at (B, K) = %s: speculative sampling should not be "
                                                             "used there" % missed))


STOPS = dict(stop_ids=[128001, 128009], stop_sequences=[[198, 198, 198, 198], [13, 13, 271, 271]], max_new_tokens=1 << 20)
STOP_ROWS = [(1, 3), (8, 3), (16, 1)]


def stop_step_leg(dev, reps, rows):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    seq = 1024
    print("# whole greedy step_lookup, synthetic Llama-3-8B GPTQ, 32 layers, %d tokens of history (a 64-id motif repeated): without stop= against a "
          "stop state whose stops never hit; ms per step, median [p10 .. p90] over %d alternated replays" % (seq, reps))
    for b, k in rows:
        len_q = k + 1
        len_buf = (seq + (reps + 8) * len_q + 63) // 64 * 64
        torch.manual_seed(7)
        ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in ("plain", "stop")}
        motif = torch.randint(0, cfg.vocab_size, (b, 64), dtype=torch.int32)
        for c in ctxs.values():
            c.tokens.copy_(motif[:, 0])                                              # the pending token continues the motif
        for t, src in zip(ctxs["stop"].kv, ctxs["plain"].kv):
            t.copy_(src)
        hist = [motif[j].repeat(seq // 64) for j in range(b)]
        look = {n: model.new_lookup(ctxs[n], hist, k) for n in ctxs}
        stop = model.new_stopper(ctxs["stop"], **STOPS)
        model.step_lookup(ctxs["plain"], look["plain"])                              # eager: the row-expanded tables
        model.step_lookup(ctxs["stop"], look["stop"], stop=stop)
        graphs = {"plain": _graph(lambda: model.step_lookup(ctxs["plain"], look["plain"])),
                  "stop": _graph(lambda: model.step_lookup(ctxs["stop"], look["stop"], stop=stop))}
        t = _alternate(graphs, reps)
        same = all(torch.equal(getattr(ctxs["plain"], n), getattr(ctxs["stop"], n)) for n in ("tokens", "positions")) and \
            torch.equal(look["plain"].hist_lens, look["stop"].hist_lens)
        st = {n: tuple(v / 1e3 for v in _stats(t[n], 1)) for n in graphs}
        spread = (st["plain"][2] - st["plain"][1]) * 1e3
        print("  %2d %2d | without %7.3f [%6.3f .. %6.3f] | with stop %7.3f [%6.3f .. %6.3f] | difference %6.1f us | the plain step's p10 .. p90 spread "
              "%6.1f us | live %d of %d, emitted %d .. %d ids per task, both runs in the same state: %s"
              % ((b, k) + st["plain"] + st["stop"] + ((st["stop"][0] - st["plain"][0]) * 1e3, spread, int(stop.live), b, int(stop.gen_lens.min()),
                                                     int(stop.gen_lens.max()), same)), flush=True)
        del graphs, ctxs, look, stop
        torch.cuda.empty_cache()


class _Count:
    """stands where ops.lib() returns the C library: counts the zl_* calls"""

    def __init__(self, real):
        self._real, self.n = real, 0

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("zl_"):
            return f

        def call(*args):
            self.n += 1
            return f(*args)
        return call


def grammar_step_leg(dev, reps, rows):
    from zhilight_amd import _lib
    from zhilight_amd.grammar import TokenAutomaton
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    seq = 1024
    auto = TokenAutomaton(cfg.vocab_size, [{i: 0 for i in range(0, cfg.vocab_size, 2)}])
    print("# whole step_lookup(sampler=) (T 0.8, top-k 40, top-p 0.95), synthetic Llama-3-8B GPTQ, %d tokens of history (a 64-id motif repeated): no "
          "tables / tables, every task unconstrained / every task in a state that allows every other class; ms per step, median [p10 .. p90] over "
          "%d alternated replays" % (seq, reps))
    names = ("plain", "tables", "grammar")
    for b, k in rows:
        len_q = k + 1
        len_buf = (seq + (reps + 8) * len_q + 63) // 64 * 64
        torch.manual_seed(7)
        ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in names}
        motif = torch.randint(0, cfg.vocab_size, (b, 64), dtype=torch.int32)
        for c in ctxs.values():
            c.tokens.copy_(motif[:, 0])
        hist = [motif[j].repeat(seq // 64) for j in range(b)]
        look = {n: model.new_lookup(ctxs[n], hist, k) for n in names}
        kw = dict(seed=5, **SAMPLER)
        samp = {"plain": model.new_sampler(ctxs["plain"], **kw), "tables": model.new_sampler(ctxs["tables"], **kw, grammar_states=8, grammar_edges=8),
                "grammar": model.new_sampler(ctxs["grammar"], **kw, grammar=[auto] * b)}
        calls = {}
        for n in names:                                                          # eager: the row-expanded tables; then the count
            model.step_lookup(ctxs[n], look[n], sampler=samp[n])
            real = ops.lib
            counter = _Count(_lib.lib())
            ops.lib = lambda counter=counter: counter
            try:
                model.step_lookup(ctxs[n], look[n], sampler=samp[n])
            finally:
                ops.lib = real
            calls[n] = counter.n
        assert calls["plain"] == calls["tables"] == calls["grammar"], calls
        graphs = {n: _graph(lambda n=n: model.step_lookup(ctxs[n], look[n], sampler=samp[n])) for n in names}
        t = _alternate(graphs, reps)
        st = {n: tuple(v / 1e3 for v in _stats(t[n], 1)) for n in graphs}
        print("  %2d %2d | plain %7.3f [%6.3f .. %6.3f] | tables, unconstrained %7.3f [%6.3f .. %6.3f] | constrained %7.3f [%6.3f .. %6.3f] | "
              "difference %6.1f / %6.1f us | %d zl_* calls per step in all three"
              % ((b, k) + st["plain"] + st["tables"] + st["grammar"] + ((st["tables"][0] - st["plain"][0]) * 1e3,
                                                                        (st["grammar"][0] - st["plain"][0]) * 1e3, calls["plain"])), flush=True)
        del graphs, ctxs, look, samp
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--sampler", action="store_true", help="the speculative sampling legs (3 and 4) instead of the greedy ones")
    ap.add_argument("--stop", action="store_true", help="step_lookup with and without the stop conditions (leg 5) instead")
    ap.add_argument("--grammar", action="store_true", help="step_lookup(sampler=) with and without the token automaton (leg 6) instead")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lookup: needs a GPU")
    dev = torch.device("cuda:0")
    if a.stop:
        stop_step_leg(dev, a.reps, STOP_ROWS)
        return
    if a.grammar:
        grammar_step_leg(dev, a.reps, STOP_ROWS)
        return
    if a.sampler:
        if not a.step_only:
            accept_leg(dev, a.reps, a.launches, STEP_ROWS)
        if not a.launch_only:
            sampler_step_leg(dev, a.reps, STEP_ROWS)
        return
    if not a.step_only:
        launch_leg(dev, a.reps, a.launches)
    if not a.launch_only:
        step_leg(dev, a.reps, STEP_ROWS)


if __name__ == "__main__":
    main()
