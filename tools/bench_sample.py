"""The device sampler's cost (profiles/sample_rows.txt is this tool's output).

  1. the launch alone (zl_sample_advance) at 1, 8 and 32 rows of 128 256 fp16 logits, next to zl_argmax_advance on the same rows:
     every cell is a captured graph of `--launches` calls on the same logits -- WARM: a row is 250 KB and stays in L2 between the
     calls of one replay, as it is behind the lm_head in a step -- the cells' replays alternated, device events around each.
     Parameter sets: top-k 40 + top-p 0.95 at T = 0.8 (every pass runs), top-p alone (no count select), T = 0 with log-probabilities
     (the arg-max and the Z pass), T = 0 without (the arg-max pass alone).  With --launch-only --parent-so PATH
     (profiles/sample_opts_struct.txt): zl_sample_advance itself from this library and from the parent's, replays alternated, and
     whether each cell's median lies inside the parent's own p10 .. p90 band.
  2. the whole step on the synthetic 32-layer model, 1 024 tokens of history, at batch 1, 8 and 32: a captured step_sample against a
     captured step_greedy, replays alternated.  Neither step_greedy nor anything it runs is changed by the sampler, so the
     step_greedy measured here is the one of the commit before it.

  3. --penalties (profiles/sample_penalties.txt): the launch alone at the same rows and parameter sets, three ways on the same logits --
     zl_sample_advance; zl_sample_advance_ex with a bitmap of about 1 % of the vocabulary per row (the options of every leg travel
     as one zl_sample_opts_t; a --parent-so that still has the tiered entry points is measured on zl_sample_advance alone); and what a caller had before the
     penalty moved into the kernel, zl_repetition_penalty over that token list followed by zl_sample_advance, two launches.  The
     factor is 1.0 (presence 0): the arithmetic per penalised class is the same division, and the two-launch form, which rewrites the
     logits on every call, then leaves them as they are, so that all cells see the same rows throughout.  --parent-so PATH: a library
     built from the commit before this one; its zl_sample_advance and its two-launch form are measured in the same process,
     replays alternated with this commit's.

  4. --bias / --top-n (profiles/sample_opts.txt): the launch alone with a logit bias (1 and 300 entries per row, all 0.0, so that the
     host forms leave the rows as they are), with top-N (5 and 20), and with both on top of the 1 % penalty bitmap -- each next to the
     same call without the option, and next to the host forms: zl_scatter_logits(add) + zl_sample_advance, and zl_repetition_penalty +
     zl_scatter_logits(add) + zl_sample_advance.  The OFF path -- zl_sample_advance and zl_sample_advance_ex as they are called today --
     is measured from this library and from --parent-so in the same process.  With --step: the whole step_sample with both options
     against the plain one at batch 1, 8 and 32.

  5. --stop (profiles/stop_step.txt, with tools/bench_lookup.py --stop): the stop conditions' launch (zl_stop_advance) alone at 1, 8 and 32
     tasks behind a one-token and a four-token step, and the whole captured step_sample with and without a stop state whose stops never
     hit (two stop ids, two four-id stop sequences and a length limit per task) at batch 1, 8 and 32, replays alternated.  The step
     without stop= issues exactly the launches of the commit before the stop conditions: it is the yardstick.

  6. --grammar (profiles/sample_grammar.txt, with tools/bench_lookup.py --grammar): the token automaton.  (a) the OFF path --
     zl_sample_advance and zl_sample_advance_ex with the penalty group alone, as they are called today -- from this library and from
     --parent-so in the same process, replays alternated.  (b) the launch alone at 1, 8 and 32 rows, masked (the automaton group, every
     row in a state that allows every other class and owns a 5000-entry exception list) against the same call unmasked;
     the speculative call (both launches) at K = 4 and K = 31 with every draft walking a 5000-entry exception list, against the call
     without tables.  With --step: the whole captured step_sample without tables, with tables and every task unconstrained, and with
     every task constrained; the zl_* calls of an eager step are counted and must be as many with the grammar as without.

usage: python tools/bench_sample.py [--launch-only | --step-only | --penalties | --bias | --top-n [--step] | --stop | --grammar [--step]]
       [--parent-so PATH] [--reps 30] [--launches 100]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402

VOCAB = 128256
SETS = [("T 0.8, top-k 40, top-p 0.95", 0.8, 40, 0.95, True), ("T 0.8, top-p 0.95", 0.8, 0, 0.95, True),
        ("T 0, log-probabilities", 0.0, 0, 1.0, True), ("T 0, none", 0.0, 0, 1.0, False)]


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


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _opts(**fields):
    """a zl_sample_opts_t by reference: tensors give their addresses, integers go in as they are"""
    from zhilight_amd._lib import SampleOpts
    return C.byref(SampleOpts(**{name: v.data_ptr() if torch.is_tensor(v) else v for name, v in fields.items()}))


def _libs(parent_so):
    """this library and, with --parent-so, the parent's -> ({"this": .., "parent": ..}, whether the parent's _ex entry points can be
    called).  A parent that still exports zl_sample_advance_opts has the tiered ABI from before zl_sample_opts_t: its zl_sample_advance,
    whose signature did not change, is measured and its other sampling entry points are skipped."""
    from zhilight_amd._lib import lib
    libs, parent_ex = {"this": lib()}, False
    if parent_so:
        parent = libs["parent"] = C.CDLL(parent_so)
        parent.zl_sample_advance.argtypes = libs["this"].zl_sample_advance.argtypes
        parent_ex = not hasattr(parent, "zl_sample_advance_opts")
        if parent_ex:
            parent.zl_sample_advance_ex.argtypes = libs["this"].zl_sample_advance_ex.argtypes
        else:
            print("# --parent-so has the tiered sampling ABI (it exports zl_sample_advance_opts): only its zl_sample_advance is measured, "
                  "its _ex / _opts / _fsm entry points are skipped")
    return libs, parent_ex


def launch_leg(dev, reps, launches, parent_so=None):
    print("# the launch alone, warm rows of %d fp16 logits (normal, sigma 2): us per launch, median [p10 .. p90] over %d alternated "
          "replays of %d launches" % (VOCAB, reps, launches))
    if parent_so:
        return plain_entry_leg(dev, reps, launches, parent_so)
    graphs, keep = {}, []
    for rows in (1, 8, 32):
        gen = torch.Generator(device="cpu").manual_seed(rows)
        logits = (torch.randn((rows, VOCAB), generator=gen) * 2).to(torch.float16).to(dev)
        tok = torch.zeros(rows, dtype=torch.int32, device=dev)

        def greedy(logits=logits, tok=tok):
            for _ in range(launches):
                ops.argmax_advance(logits, tokens=tok)
        graphs[(rows, "argmax_advance")] = _graph(greedy)
        for name, t, k, p, lp in SETS:
            f32 = dict(dtype=torch.float32, device=dev)
            args = dict(temperature=torch.full((rows,), t, **f32), top_k=torch.full((rows,), k, dtype=torch.int32, device=dev),
                        top_p=torch.full((rows,), p, **f32), seeds=torch.arange(rows, dtype=torch.int64, device=dev),
                        draws=torch.zeros(rows, dtype=torch.int64, device=dev), tokens=tok,
                        logprobs=torch.empty(rows, **f32) if lp else None)

            def sample(logits=logits, args=args):
                for _ in range(launches):
                    ops.sample_advance(logits, **args)
            graphs[(rows, name)] = _graph(sample)
            keep.append(args)
        keep.append((logits, tok))
    t = _alternate(graphs, reps)
    print("# rows | %-30s | us per launch" % "launch")
    for (rows, name), ms in t.items():
        print("  %4d | %-30s | %7.2f [%7.2f .. %7.2f]" % ((rows, name) + _stats(ms, launches)), flush=True)


def plain_entry_leg(dev, reps, launches, parent_so):
    """--launch-only --parent-so: zl_sample_advance itself from this library and from the parent's, the same rows and parameter sets,
    replays alternated; says per cell whether this library's median lies inside the parent's own p10 .. p90 band"""
    libs, _ = _libs(parent_so)
    i64 = C.c_int64
    graphs, keep = {}, []
    for rows in (1, 8, 32):
        gen = torch.Generator(device="cpu").manual_seed(rows)
        logits = (torch.randn((rows, VOCAB), generator=gen) * 2).to(torch.float16).to(dev)
        tok = torch.zeros(rows, dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        for name, t, k, tp, lp in SETS:
            a = dict(T=torch.full((rows,), t, **f32), k=torch.full((rows,), k, dtype=torch.int32, device=dev), p=torch.full((rows,), tp, **f32),
                     seeds=torch.arange(rows, dtype=torch.int64, device=dev), draws=torch.zeros(rows, dtype=torch.int64, device=dev),
                     lp=torch.empty(rows, **f32) if lp else None)

            def plain(l, a=a, logits=logits, tok=tok, rows=rows):
                for _ in range(launches):
                    assert l.zl_sample_advance(_p(logits), C.c_int(2), i64(rows), i64(VOCAB), i64(VOCAB), _p(a["T"]), _p(a["k"]), _p(a["p"]),
                                               _p(a["seeds"]), _p(a["draws"]), _p(None), _p(tok), _p(None), _p(None), _p(None), _p(None),
                                               _p(a["lp"]), _p(None), _stream()) == 0
            for which, l in libs.items():
                graphs[(rows, name, which)] = _graph(lambda l=l, plain=plain: plain(l))
            keep.append(a)
        keep.append((logits, tok))
    t = _alternate(graphs, reps)
    print("# rows | %-30s | this: zl_sample_advance     | parent: zl_sample_advance   | this median inside the parent's band" % "parameters")
    inside = True
    for rows in (1, 8, 32):
        for name, *_ in SETS:
            this, parent = _stats(t[(rows, name, "this")], launches), _stats(t[(rows, name, "parent")], launches)
            ok = parent[1] <= this[0] <= parent[2]
            inside = inside and ok
            print("  %4d | %-30s | %7.2f [%7.2f .. %7.2f] | %7.2f [%7.2f .. %7.2f] | %s"
                  % ((rows, name) + this + parent + ("yes" if ok else "NO",)), flush=True)
    print("# every cell inside: %s" % ("yes" if inside else "NO"))


def step_leg(dev, reps):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    seq = 1024
    print("# whole step, synthetic Llama-3-8B GPTQ, 32 layers, %d tokens of history; step_sample at T 0.8, top-k 40, top-p 0.95; ms per step, "
          "median [p10 .. p90] over %d alternated replays" % (seq, reps))
    print("#  B | step_greedy             | step_sample             | ratio of the medians | difference, us")
    for b in (1, 8, 32):
        len_buf = (seq + reps + 16 + 63) // 64 * 64
        torch.manual_seed(7)
        ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in ("greedy", "sample")}
        tok = torch.randint(0, cfg.vocab_size, (b,), device=dev, dtype=torch.int32)
        for c in ctxs.values():
            c.tokens.copy_(tok)
        for t, src in zip(ctxs["sample"].kv, ctxs["greedy"].kv):
            t.copy_(src)
        state = model.new_sampler(ctxs["sample"], temperature=0.8, top_k=40, top_p=0.95, seed=5)
        graphs = {"greedy": _graph(lambda: model.step_greedy(ctxs["greedy"])),
                  "sample": _graph(lambda: model.step_sample(ctxs["sample"], state))}
        t = _alternate(graphs, reps)
        assert int(state.draws.min()) == 2 + 3 + reps                             # _graph's eager call and replay, the warm and timed replays
        st = {n: tuple(v / 1e3 for v in _stats(t[n], 1)) for n in graphs}
        cell = lambda s: "%7.3f [%6.3f .. %6.3f]" % s                            # noqa: E731
        print("  %2d | %s | %s |        %6.4f        | %7.1f" % (b, cell(st["greedy"]), cell(st["sample"]), st["sample"][0] / st["greedy"][0],
                                                                  (st["sample"][0] - st["greedy"][0]) * 1e3), flush=True)
        del graphs, ctxs, state
        torch.cuda.empty_cache()


def penalty_leg(dev, reps, launches, parent_so):
    libs, _ = _libs(parent_so)
    p, i64 = _p, C.c_int64
    words = ops.seen_words(VOCAB)
    print("# the launch alone with and without penalties, warm rows of %d fp16 logits (normal, sigma 2), %d ids (about 1 %%) per row in the set, "
          "factor 1.0: us per call, median [p10 .. p90] over %d alternated replays of %d calls" % (VOCAB, VOCAB // 100, reps, launches))
    graphs, keep = {}, []
    for rows in (1, 8, 32):
        gen = torch.Generator(device="cpu").manual_seed(rows)
        logits = (torch.randn((rows, VOCAB), generator=gen) * 2).to(torch.float16).to(dev)
        ids = torch.stack([torch.randperm(VOCAB, generator=gen)[:VOCAB // 100] for _ in range(rows)]).to(torch.int32).to(dev)
        bid = torch.arange(rows, dtype=torch.int32, device=dev).view(rows, 1).expand(rows, ids.shape[1]).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        one, zero = torch.ones(ids.numel(), **f32), torch.zeros(ids.numel(), **f32)
        tok = torch.zeros(rows, dtype=torch.int32, device=dev)
        for name, t, k, tp, lp in SETS:
            a = dict(T=torch.full((rows,), t, **f32), k=torch.full((rows,), k, dtype=torch.int32, device=dev), p=torch.full((rows,), tp, **f32),
                     seeds=torch.arange(rows, dtype=torch.int64, device=dev), draws=torch.zeros(rows, dtype=torch.int64, device=dev),
                     lp=torch.empty(rows, **f32) if lp else None, seen=torch.zeros((rows, words), dtype=torch.int32, device=dev))
            ops.seen_mark(a["seen"], ids, VOCAB)
            head = lambda a=a: (p(logits), C.c_int(2), i64(rows), i64(VOCAB), i64(VOCAB), p(a["T"]), p(a["k"]), p(a["p"]), p(a["seeds"]),   # noqa: E731
                                p(a["draws"]), p(None), p(tok), p(None), p(None), p(None), p(None), p(a["lp"]), p(None))
            stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                                                             # noqa: E731

            def plain(l, head=head):
                for _ in range(launches):
                    assert l.zl_sample_advance(*head(), stream()) == 0

            def two(l, head=head):
                for _ in range(launches):
                    assert l.zl_repetition_penalty(p(one), p(zero), p(ids), p(bid), p(logits), i64(ids.numel()), i64(VOCAB), C.c_int(2), stream()) == 0
                    assert l.zl_sample_advance(*head(), stream()) == 0

            def fused(a=a, head=head):
                for _ in range(launches):
                    assert libs["this"].zl_sample_advance_ex(*head(), _opts(rep_penalty=one, presence=zero, seen=a["seen"], seen_ld=words),
                                                             stream()) == 0
            for which, l in libs.items():
                graphs[(rows, name, which + ": sample_advance")] = _graph(lambda l=l, plain=plain: plain(l))
                graphs[(rows, name, which + ": repetition_penalty + sample_advance")] = _graph(lambda l=l, two=two: two(l))
            graphs[(rows, name, "this: sample_advance_ex")] = _graph(fused)
            keep.append(a)
        keep.append((logits, ids, bid, one, zero, tok))
    t = _alternate(graphs, reps)
    print("# rows | %-30s | %-44s | us per call" % ("parameters", "call"))
    for (rows, name, which), ms in t.items():
        print("  %4d | %-30s | %-44s | %7.2f [%7.2f .. %7.2f]" % ((rows, name, which) + _stats(ms, launches)), flush=True)


def opts_leg(dev, reps, launches, parent_so, with_bias, with_top, rows_list=(1, 8)):
    libs, parent_ex = _libs(parent_so)
    p, i64 = _p, C.c_int64
    words = ops.seen_words(VOCAB)
    print("# the launch alone with a logit bias / top-N, warm rows of %d fp16 logits (normal, sigma 2); the penalty set holds %d ids per row "
          "(factor 1.0), the biases are 0.0: us per call, median [p10 .. p90] over %d alternated replays of %d calls"
          % (VOCAB, VOCAB // 100, reps, launches))
    graphs, keep = {}, []
    for rows in rows_list:
        gen = torch.Generator(device="cpu").manual_seed(rows)
        logits = (torch.randn((rows, VOCAB), generator=gen) * 2).to(torch.float16).to(dev)
        ids = torch.stack([torch.randperm(VOCAB, generator=gen)[:VOCAB // 100] for _ in range(rows)]).to(torch.int32).to(dev)
        bid = torch.arange(rows, dtype=torch.int32, device=dev).view(rows, 1).expand(rows, ids.shape[1]).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        one, zero = torch.ones(ids.numel(), **f32), torch.zeros(ids.numel(), **f32)
        tok = torch.zeros(rows, dtype=torch.int32, device=dev)
        bias = {}
        for cnt in (1, 300):
            maps = [{int(i): 0.0 for i in torch.randperm(VOCAB, generator=gen)[:cnt]} for _ in range(rows)]
            b_ids, b_vals, b_cnt, b_bits = ops.logit_bias_pack(maps, VOCAB, dev)
            flat_ids = b_ids.reshape(-1).contiguous()
            b_bid = torch.arange(rows, dtype=torch.int32, device=dev).view(rows, 1).expand(rows, cnt).reshape(-1).contiguous()
            bias[cnt] = (b_ids, b_vals, b_cnt, b_bits, flat_ids, b_bid, torch.zeros(rows * cnt, **f32))
        top = {n: (torch.empty((rows, n), dtype=torch.int32, device=dev), torch.empty((rows, n), **f32)) for n in (5, 20)}
        for name, t, k, tp, lp in (SETS[0], SETS[3]):
            a = dict(T=torch.full((rows,), t, **f32), k=torch.full((rows,), k, dtype=torch.int32, device=dev), p=torch.full((rows,), tp, **f32),
                     seeds=torch.arange(rows, dtype=torch.int64, device=dev), draws=torch.zeros(rows, dtype=torch.int64, device=dev),
                     lp=torch.empty(rows, **f32) if lp else None, seen=torch.zeros((rows, words), dtype=torch.int32, device=dev))
            ops.seen_mark(a["seen"], ids, VOCAB)
            head = lambda a=a: (p(logits), C.c_int(2), i64(rows), i64(VOCAB), i64(VOCAB), p(a["T"]), p(a["k"]), p(a["p"]), p(a["seeds"]),   # noqa: E731
                                p(a["draws"]), p(None), p(tok), p(None), p(None), p(None), p(None), p(a["lp"]), p(None))
            stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                                                             # noqa: E731
            pen = lambda a=a: dict(rep_penalty=one, presence=zero, seen=a["seen"], seen_ld=words)                                            # noqa: E731

            def fields(seen, cnt, n):
                """the struct's fields: the penalty group (seen), a bias of cnt entries per row (0: none), top-N n (0: off)"""
                f = pen() if seen else {}
                if cnt:
                    b = bias[cnt]
                    f.update(bias_ids=b[0], bias_vals=b[1], bias_cnt=b[2], bias_ld=cnt, bias_bits=b[3], bias_bits_ld=words)
                if n:
                    f.update(top_n=n, top_ids=top[n][0], top_logprobs=top[n][1])
                return f

            def cell(fn):
                def run():
                    for _ in range(launches):
                        r = fn()
                        assert (r[-1] if isinstance(r, tuple) else r) == 0
                return _graph(run)

            def scatter(l, cnt):
                b = bias[cnt]
                assert l.zl_scatter_logits(p(b[6]), p(b[4]), p(b[5]), p(logits), i64(b[4].numel()), i64(VOCAB), C.c_int(1), C.c_int(2), stream()) == 0

            def penalise(l):
                assert l.zl_repetition_penalty(p(one), p(zero), p(ids), p(bid), p(logits), i64(ids.numel()), i64(VOCAB), C.c_int(2), stream()) == 0
            this = libs["this"]
            opts = lambda l, seen, cnt, n, head=head, fields=fields: l.zl_sample_advance_ex(*head(), _opts(**fields(seen, cnt, n)), stream())   # noqa: E731
            for which, l in libs.items():                                                # the off path, both libraries
                graphs[(rows, name, which + ": sample_advance")] = cell(lambda l=l, head=head: l.zl_sample_advance(*head(), stream()))
                if l is this or parent_ex:
                    graphs[(rows, name, which + ": sample_advance_ex (seen)")] = cell(lambda l=l, opts=opts: opts(l, True, 0, 0))
            if with_bias:
                for cnt in (1, 300):
                    graphs[(rows, name, "opts: bias %d" % cnt)] = cell(lambda cnt=cnt, opts=opts: opts(this, False, cnt, 0))
                    graphs[(rows, name, "host: scatter_logits %d + sample_advance" % cnt)] = cell(
                        lambda cnt=cnt, head=head: (scatter(this, cnt), this.zl_sample_advance(*head(), stream())))
            if with_top:
                for n in (5, 20):
                    graphs[(rows, name, "opts: top-N %d" % n)] = cell(lambda n=n, opts=opts: opts(this, False, 0, n))
            if with_bias and with_top:
                graphs[(rows, name, "opts: seen + bias 300 + top-N 5")] = cell(lambda opts=opts: opts(this, True, 300, 5))
                graphs[(rows, name, "host: repetition_penalty + scatter_logits 300 + sample_advance")] = cell(
                    lambda head=head: (penalise(this), scatter(this, 300), this.zl_sample_advance(*head(), stream())))
            keep.append(a)
        keep.append((logits, ids, bid, one, zero, tok, bias, top))
    t = _alternate(graphs, reps)
    print("# rows | %-30s | %-62s | us per call" % ("parameters", "call"))
    for (rows, name, which), ms in t.items():
        print("  %4d | %-30s | %-62s | %7.2f [%7.2f .. %7.2f]" % ((rows, name, which) + _stats(ms, launches)), flush=True)


def opts_step_leg(dev, reps):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    seq = 1024
    print("# whole step_sample (T 0.8, top-k 40, top-p 0.95), synthetic Llama-3-8B GPTQ, %d tokens of history: plain against logit_bias of 300 "
          "ids + top_logprobs 5; ms per step, median [p10 .. p90] over %d alternated replays" % (seq, reps))
    for b in (1, 8, 32):
        len_buf = (seq + reps + 16 + 63) // 64 * 64
        torch.manual_seed(7)
        ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in ("plain", "opts")}
        kw = dict(temperature=0.8, top_k=40, top_p=0.95, seed=5)
        states = {"plain": model.new_sampler(ctxs["plain"], **kw),
                  "opts": model.new_sampler(ctxs["opts"], **kw, logit_bias={i * 7: 0.5 for i in range(300)}, top_logprobs=5)}
        graphs = {n: _graph(lambda n=n: model.step_sample(ctxs[n], states[n])) for n in ctxs}
        t = _alternate(graphs, reps)
        st = {n: tuple(v / 1e3 for v in _stats(t[n], 1)) for n in graphs}
        print("  %2d | plain %7.3f [%6.3f .. %6.3f] | bias + top-N %7.3f [%6.3f .. %6.3f] | difference %7.1f us"
              % ((b,) + st["plain"] + st["opts"] + ((st["opts"][0] - st["plain"][0]) * 1e3,)), flush=True)
        del graphs, ctxs, states
        torch.cuda.empty_cache()


STOPS = dict(stop_ids=[128001, 128009], stop_sequences=[[198, 198, 198, 198], [13, 13, 271, 271]], max_new_tokens=1 << 20)


def stop_launch_leg(dev, reps, launches):
    print("# zl_stop_advance alone, stops that never hit (2 stop ids, 2 stop sequences of 4 ids, a length limit; every task emits n_new ids per "
          "call): us per launch, median [p10 .. p90] over %d alternated replays of %d launches" % (reps, launches))
    i32 = dict(dtype=torch.int32, device=dev)
    graphs, keep = {}, []
    for b in (1, 8, 32):
        for n_new in (1, 4):
            ids, seqs, lens = ops.stop_pack([(STOPS["stop_ids"], STOPS["stop_sequences"])] * b, VOCAB, dev)
            st = dict(max_new=torch.full((b,), 1 << 30, **i32), gen_lens=torch.zeros(b, **i32), tail=torch.full((b, ops.STOP_TAIL), -1, **i32),
                      last_token=torch.zeros(b, **i32), finished=torch.zeros(b, **i32))
            new = torch.randint(1000, 2000, (b, n_new), **i32)
            out = dict(accepted=torch.zeros(b, **i32), tokens=torch.zeros(b, **i32), positions=torch.zeros(b, **i32),
                       placement=torch.zeros(b, **i32), valid_lens=torch.zeros(b, **i32), emit_lens=torch.zeros(b, **i32), live=torch.zeros(1, **i32))

            def run(ids=ids, seqs=seqs, lens=lens, st=st, new=new, out=out):
                for _ in range(launches):
                    ops.stop_advance(ids, seqs, lens, new_tokens=new, **st, **out)
            graphs[(b, n_new)] = _graph(run)
            keep.append((ids, seqs, lens, st, new, out))
    t = _alternate(graphs, reps)
    print("#  B  n_new | us per launch            | live at the end")
    for ((b, n_new), ms), k in zip(t.items(), keep):
        print("  %2d  %5d | %7.2f [%7.2f .. %7.2f] | %d of %d" % ((b, n_new) + _stats(ms, launches) + (int(k[5]["live"]), b)), flush=True)


def stop_step_leg(dev, reps):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    seq = 1024
    print("# whole step_sample (T 0.8, top-k 40, top-p 0.95), synthetic Llama-3-8B GPTQ, %d tokens of history: without stop= against a stop state "
          "whose stops never hit; ms per step, median [p10 .. p90] over %d alternated replays" % (seq, reps))
    for b in (1, 8, 32):
        len_buf = (seq + reps + 16 + 63) // 64 * 64
        torch.manual_seed(7)
        ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in ("plain", "stop")}
        for t, src in zip(ctxs["stop"].kv, ctxs["plain"].kv):
            t.copy_(src)
        ctxs["stop"].tokens.copy_(ctxs["plain"].tokens)
        kw = dict(temperature=0.8, top_k=40, top_p=0.95, seed=5)
        states = {n: model.new_sampler(ctxs[n], **kw) for n in ctxs}
        stop = model.new_stopper(ctxs["stop"], **STOPS)
        graphs = {"plain": _graph(lambda: model.step_sample(ctxs["plain"], states["plain"])),
                  "stop": _graph(lambda: model.step_sample(ctxs["stop"], states["stop"], stop=stop))}
        t = _alternate(graphs, reps)
        same = torch.equal(ctxs["plain"].tokens, ctxs["stop"].tokens) and torch.equal(ctxs["plain"].positions, ctxs["stop"].positions)
        st = {n: tuple(v / 1e3 for v in _stats(t[n], 1)) for n in graphs}
        spread = (st["plain"][2] - st["plain"][1]) * 1e3
        print("  %2d | without %7.3f [%6.3f .. %6.3f] | with stop %7.3f [%6.3f .. %6.3f] | difference %6.1f us | the plain step's p10 .. p90 spread "
              "%6.1f us | live %d of %d, emitted %d ids per task, both runs in the same state: %s"
              % ((b,) + st["plain"] + st["stop"] + ((st["stop"][0] - st["plain"][0]) * 1e3, spread, int(stop.live), b, int(stop.gen_lens.min()), same)),
              flush=True)
        del graphs, ctxs, states, stop
        torch.cuda.empty_cache()


def _bench_automaton(n, dev):
    """two states that allow every other class each (even / odd ids); 5000 of a state's ids, evenly spread, are exceptions that lead to
    the other state, the rest default to the state itself -> ops.grammar_tables' tuple"""
    import numpy as np
    from zhilight_amd.grammar import TokenAutomaton
    trans = []
    for s in (0, 1):
        ids = np.arange(s, n, 2)
        nxt = np.full(ids.size, s)
        nxt[np.linspace(0, ids.size - 1, 5000).astype(np.int64)] = 1 - s
        trans.append(dict(zip(ids.tolist(), nxt.tolist())))
    return ops.grammar_tables(TokenAutomaton(n, trans).pack(), dev)


def grammar_leg(dev, reps, launches, parent_so):
    libs, parent_ex = _libs(parent_so)
    p, i64 = _p, C.c_int64
    words = ops.seen_words(VOCAB)
    fsm = _bench_automaton(VOCAB, dev)
    print("# the token automaton: warm rows of %d fp16 logits (normal, sigma 2), T 0.8, top-k 40, top-p 0.95; a state allows every other class, "
          "%d exception entries per state: us per call, median [p10 .. p90] over %d alternated replays of %d calls"
          % (VOCAB, int(fsm[3].numel()) // 2, reps, launches))
    graphs, keep = {}, []
    f32 = dict(dtype=torch.float32, device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)        # noqa: E731
    for rows in (1, 8, 32):
        gen = torch.Generator(device="cpu").manual_seed(rows)
        logits = (torch.randn((rows, VOCAB), generator=gen) * 2).to(torch.float16).to(dev)
        ids = torch.stack([torch.randperm(VOCAB, generator=gen)[:VOCAB // 100] for _ in range(rows)]).to(torch.int32).to(dev)
        tok = torch.zeros(rows, dtype=torch.int32, device=dev)
        one, zero = torch.ones(rows, **f32), torch.zeros(rows, **f32)
        a = dict(T=torch.full((rows,), 0.8, **f32), k=torch.full((rows,), 40, dtype=torch.int32, device=dev), p=torch.full((rows,), 0.95, **f32),
                 seeds=torch.arange(rows, dtype=torch.int64, device=dev), draws=torch.zeros(rows, dtype=torch.int64, device=dev),
                 lp=torch.empty(rows, **f32), seen=torch.zeros((rows, words), dtype=torch.int32, device=dev))
        ops.seen_mark(a["seen"], ids, VOCAB)
        head = lambda a=a, logits=logits, tok=tok, rows=rows: (p(logits), C.c_int(2), i64(rows), i64(VOCAB), i64(VOCAB), p(a["T"]), p(a["k"]),   # noqa: E731
                                                                p(a["p"]), p(a["seeds"]), p(a["draws"]), p(None), p(tok), p(None), p(None), p(None),
                                                                p(None), p(a["lp"]), p(None))
        pen = lambda a=a, one=one, zero=zero: dict(rep_penalty=one, presence=zero, seen=a["seen"], seen_ld=words)                                # noqa: E731

        def cell(fn):
            def run():
                for _ in range(launches):
                    assert fn() == 0
            return _graph(run)
        this = libs["this"]
        for which, l in libs.items():                                        # (a) the off path, both libraries
            graphs[(rows, which + ": sample_advance")] = cell(lambda l=l, head=head: l.zl_sample_advance(*head(), stream()))
            if l is this or parent_ex:
                graphs[(rows, which + ": sample_advance_ex (seen)")] = cell(lambda l=l, head=head, pen=pen: l.zl_sample_advance_ex(*head(), _opts(**pen()),
                                                                                                                             stream()))
        st = torch.zeros(rows, dtype=torch.int32, device=dev)                # (b) masked: the rows start in state 0 and move between the two
        tables = lambda st=st: dict(fsm_mask=fsm[0], fsm_mask_ld=fsm[0].shape[1], fsm_default=fsm[1], fsm_exc_off=fsm[2], fsm_exc_tok=fsm[3],    # noqa: E731
                                    fsm_exc_next=fsm[4], fsm_states=fsm[0].shape[0], fsm_exceptions=fsm[3].numel(), fsm_state=st)
        graphs[(rows, "fsm: masked")] = cell(lambda head=head, tables=tables: this.zl_sample_advance_ex(*head(), _opts(**tables()), stream()))
        graphs[(rows, "fsm: masked + seen")] = cell(lambda head=head, pen=pen, tables=tables: this.zl_sample_advance_ex(*head(), _opts(**pen(), **tables()),
                                                                                                                       stream()))
        free = torch.full((rows,), -1, dtype=torch.int32, device=dev)
        graphs[(rows, "fsm: tables, every row unconstrained")] = cell(
            lambda head=head, tables=tables, free=free: this.zl_sample_advance_ex(*head(), _opts(**tables(free)), stream()))
        keep.append((logits, ids, tok, one, zero, a, st, free))
    t = _alternate(graphs, reps)
    print("# rows | %-50s | us per call" % "call")
    for (rows, which), ms in t.items():
        print("  %4d | %-50s | %7.2f [%7.2f .. %7.2f]" % ((rows, which) + _stats(ms, launches)), flush=True)
    # the speculative call: the chain's worst case, every draft allowed and an exception of its state
    chain = fsm
    print("# zl_spec_sample_accept(_ex with the automaton), B = 1, both launches: every draft hits a 5000-entry exception list (the states alternate); us per call")
    graphs, keep = {}, []
    for K in (4, 31):
        len_q = K + 1
        gen = torch.Generator(device="cpu").manual_seed(K)
        logits = (torch.randn((len_q, VOCAB), generator=gen) * 2).to(torch.float16).to(dev)
        exc, off = chain[3].tolist(), chain[2].tolist()
        drafts = torch.tensor([[exc[off[j % 2] + 17 * j + 4000] for j in range(K)]], dtype=torch.int32, device=dev)   # deep in the lists
        kw = dict(temperature=torch.full((1,), 0.8, **f32), top_k=torch.full((1,), 40, dtype=torch.int32, device=dev), top_p=torch.full((1,), 0.95, **f32),
                  seeds=torch.zeros(1, dtype=torch.int64, device=dev), draws=torch.zeros(1, dtype=torch.int64, device=dev),
                  accepted=torch.zeros(1, dtype=torch.int32, device=dev), out_tokens=torch.zeros((1, len_q), dtype=torch.int32, device=dev))
        st, rs = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((1, len_q), dtype=torch.int32, device=dev)

        def masked(logits=logits, drafts=drafts, kw=kw, st=st, rs=rs):
            for _ in range(launches):
                st.zero_()
                ops.spec_sample_accept(logits, drafts, **kw, fsm=chain, fsm_state=st, row_states=rs)

        def plain_zero(logits=logits, drafts=drafts, kw=kw, st=st):
            for _ in range(launches):
                st.zero_()
                ops.spec_sample_accept(logits, drafts, **kw)
        graphs[(K, "without tables (+ the state's reset)")] = _graph(plain_zero)
        graphs[(K, "fsm: every draft an exception")] = _graph(masked)
        keep.append((logits, drafts, kw, st, rs))
    t = _alternate(graphs, reps)
    for (K, which), ms in t.items():
        print("  K = %2d | %-40s | %7.2f [%7.2f .. %7.2f]" % ((K, which) + _stats(ms, launches)), flush=True)


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


def grammar_step_leg(dev, reps):
    from zhilight_amd import _lib
    from zhilight_amd.grammar import TokenAutomaton
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    seq = 1024
    auto = TokenAutomaton(cfg.vocab_size, [{i: 0 for i in range(0, cfg.vocab_size, 2)}])
    print("# whole step_sample (T 0.8, top-k 40, top-p 0.95), synthetic Llama-3-8B GPTQ, %d tokens of history: no tables / tables, every task "
          "unconstrained / every task in a state that allows every other class; ms per step, median [p10 .. p90] over %d alternated replays" % (seq, reps))
    for b in (1, 8, 32):
        len_buf = (seq + reps + 16 + 63) // 64 * 64
        torch.manual_seed(7)
        names = ("plain", "tables", "grammar")
        ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in names}
        kw = dict(temperature=0.8, top_k=40, top_p=0.95, seed=5)
        states = {"plain": model.new_sampler(ctxs["plain"], **kw), "tables": model.new_sampler(ctxs["tables"], **kw, grammar_states=8, grammar_edges=8),
                  "grammar": model.new_sampler(ctxs["grammar"], **kw, grammar=[auto] * b)}
        calls = {}
        for n in names:                                                      # the launch count: the zl_* calls of the second eager step
            model.step_sample(ctxs[n], states[n])
            real = ops.lib
            counter = _Count(_lib.lib())
            ops.lib = lambda counter=counter: counter
            try:
                model.step_sample(ctxs[n], states[n])
            finally:
                ops.lib = real
            calls[n] = counter.n
        assert calls["plain"] == calls["tables"] == calls["grammar"], calls
        graphs = {n: _graph(lambda n=n: model.step_sample(ctxs[n], states[n])) for n in names}
        t = _alternate(graphs, reps)
        st = {n: tuple(v / 1e3 for v in _stats(t[n], 1)) for n in graphs}
        ok = bool((ctxs["grammar"].tokens % 2 == 0).all())
        print("  %2d | plain %7.3f [%6.3f .. %6.3f] | tables, unconstrained %7.3f [%6.3f .. %6.3f] | constrained %7.3f [%6.3f .. %6.3f] | "
              "difference %6.1f / %6.1f us | %d zl_* calls per step in all three | every constrained pick allowed: %s"
              % ((b,) + st["plain"] + st["tables"] + st["grammar"] + ((st["tables"][0] - st["plain"][0]) * 1e3, (st["grammar"][0] - st["plain"][0]) * 1e3,
                                                                        calls["plain"], ok)), flush=True)
        del graphs, ctxs, states
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--penalties", action="store_true")
    ap.add_argument("--bias", action="store_true")
    ap.add_argument("--top-n", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--stop", action="store_true", help="the stop conditions' launch alone and inside step_sample (leg 5)")
    ap.add_argument("--grammar", action="store_true", help="the token automaton: the off path against --parent-so, masked against unmasked (leg 6)")
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--launches", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample: needs a GPU")
    dev = torch.device("cuda:0")
    if a.penalties:
        penalty_leg(dev, a.reps, a.launches, a.parent_so)
        return
    if a.grammar:
        if not a.step_only:
            grammar_leg(dev, a.reps, a.launches, a.parent_so)
        if a.step or a.step_only:
            grammar_step_leg(dev, a.reps)
        return
    if a.stop:
        if not a.step_only:
            stop_launch_leg(dev, a.reps, a.launches)
        if not a.launch_only:
            stop_step_leg(dev, a.reps)
        return
    if a.bias or a.top_n:
        opts_leg(dev, a.reps, a.launches, a.parent_so, a.bias, a.top_n)
        if a.step:
            opts_step_leg(dev, a.reps)
        return
    if not a.step_only:
        launch_leg(dev, a.reps, a.launches, a.parent_so)
    if not a.launch_only:
        step_leg(dev, a.reps)


if __name__ == "__main__":
    main()
