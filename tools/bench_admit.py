"""The cost of slot admission (profiles/slot_admit.txt is this tool's output).

  a. the launch alone (zl_slots_admit) in a captured graph at 1, 4 and 16 admitted slots of a batch of 32, vocabulary 128 256, every
     option on: a penalty set of 512 ids, 16 bias entries in rows of 64, top-N 5, stop rows at the widths (16, 8, 16), a history of
     512 ids.  The blob is uploaded once; every cell is a graph of `--launches` launches, replays alternated, device events around each.
  b. ops.slots_pack + ops.slots_admit eager, wall clock from the request dicts to the launch's end: pack, upload and launch.
  c. the baseline: the same re-initialisation written here as torch row operations (index_copy_ / index_fill_ per state tensor) plus
     the existing zl_seen_mark launches and the host packing (ops.logit_bias_rows, ops.stop_rows) with one upload per tensor --
     eager with the uploads (wall clock), and the device part alone in a captured graph.  Its result is checked against the launch's.
  d. end to end on the synthetic Llama-3-8B: a queue of requests with mixed prompt lengths and length limits through BatchServer
     with captured steps and with eager steps -- the second separates what admission gains from what replaying a graph gains --
     against the only way of the commit before: lock-step waves of B requests through prefill_batch + new_sampler + new_stopper +
     generate_sample(stop=), whose steps are eager.  Tokens per second of wall clock, and the slot-steps spent on finished slots, in both.
  e. the captured step_sample at batch 8, 1 024 tokens of history: on states built as the commit before builds them, on the full-width
     states before an admission and after one, replays alternated.  The step's code is the same in all three.

usage: python tools/bench_admit.py [--only a,b,c,d,e] [--reps 30] [--launches 50]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402
from zhilight_amd.llama import LookupState, SamplerState, StopState  # noqa: E402

VOCAB, B = 128256, 32
BIAS_LD, TOP_N, CAP = 64, 5, 2048
WIDTHS = dict(penalties=True, bias_ld=BIAS_LD, n_ids=16, n_seqs=8, seq_ld=16, hist_cap=CAP)


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


def _stats(ms, per=1):
    us = sorted(t * 1e3 / per for t in ms)
    return statistics.median(us), us[len(us) // 10], us[-1 - len(us) // 10]


def _states(dev, b=B):
    """full-width states of b slots, every row in use (so that a stale row would show in the check)"""
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    words = ops.seen_words(VOCAB)
    z = lambda *s: torch.zeros(s, **i32)                                                                      # noqa: E731
    samp = SamplerState(temperature=torch.ones(b, **f32), top_k=z(b), top_p=torch.ones(b, **f32), seeds=torch.zeros(b, dtype=torch.int64, device=dev),
                        draws=torch.ones(b, dtype=torch.int64, device=dev), logprobs=torch.ones(b, **f32), u=torch.ones(b, **f32),
                        repetition_penalty=torch.ones(b, **f32), presence_penalty=torch.zeros(b, **f32), seen=torch.full((b, words), -1, **i32),
                        bias_ids=z(b, BIAS_LD), bias_vals=torch.ones((b, BIAS_LD), **f32), bias_cnt=z(b), bias_bits=torch.full((b, words), -1, **i32),
                        top_n=TOP_N, top_ids=z(b, TOP_N), top_logprobs=torch.zeros((b, TOP_N), **f32))
    stop = StopState(stop_ids=z(b, 16), stop_seqs=z(b, 8, 16), seq_lens=z(b, 8), max_new=z(b), gen_lens=torch.ones(b, **i32), tail=z(b, 15),
                     last_token=z(b), finished=torch.ones(b, **i32), emit_lens=torch.ones(b, **i32), live=z(1))
    look = LookupState(history=z(b, CAP), hist_lens=z(b), drafts=z(b, 3), match=z(b, 2), k=3, max_ngram=3, min_ngram=1)
    ctx = dict(tokens=torch.arange(b, **i32) + 100, positions=z(b), placement=z(b), valid_lens=torch.ones(b, **i32))
    return ctx, samp, stop, look


def _requests(n, rng):
    return [dict(temperature=0.8, top_k=40, top_p=0.95, seed=int(rng.integers(0, 1 << 40)), repetition_penalty=1.1, presence_penalty=0.0,
                 penalty_tokens=rng.integers(0, VOCAB, 512).tolist(), logit_bias={int(i): 0.5 for i in rng.choice(VOCAB, 16, replace=False)},
                 stop_ids=[128001, 128009], stop_sequences=[[198, 198, 198, 198], [13, 13, 271, 271]], max_new_tokens=256,
                 history=rng.integers(0, VOCAB, 512).tolist()) for _ in range(n)]


def _baseline_host(slots, reqs):
    """the host half of the baseline: the rows as numpy arrays, through the existing packing code"""
    n = len(slots)
    ids, vals, cnt, bits = ops.logit_bias_rows([r["logit_bias"] for r in reqs], VOCAB)
    wid, wva = np.full((n, BIAS_LD), -1, np.int32), np.zeros((n, BIAS_LD), np.float32)
    wid[:, :ids.shape[1]], wva[:, :ids.shape[1]] = ids, vals
    sid, ssq, sln = ops.stop_rows([(r["stop_ids"], r["stop_sequences"]) for r in reqs], VOCAB)
    fid, fsq, fln = np.full((n, 16), -1, np.int32), np.full((n, 8, 16), -1, np.int32), np.zeros((n, 8), np.int32)
    fid[:, :sid.shape[1]], fsq[:, :ssq.shape[1], :ssq.shape[2]], fln[:, :sln.shape[1]] = sid, ssq, sln
    pen = np.full((B, max(len(r["penalty_tokens"]) for r in reqs)), -1, np.int32)          # zl_seen_mark takes one row per task of the batch
    for s, r in zip(slots, reqs):
        pen[s, :len(r["penalty_tokens"])] = r["penalty_tokens"]
    hist = np.zeros((n, max(len(r["history"]) for r in reqs)), np.int32)
    for j, r in enumerate(reqs):
        hist[j, :len(r["history"])] = r["history"]
    mask = np.zeros(B, np.int32)
    mask[slots] = 1
    return dict(idx=np.asarray(slots, np.int64), temperature=np.asarray([r["temperature"] for r in reqs], np.float32),
                top_k=np.asarray([r["top_k"] for r in reqs], np.int32), top_p=np.asarray([r["top_p"] for r in reqs], np.float32),
                seeds=np.asarray([r["seed"] for r in reqs], np.int64), rep=np.asarray([r["repetition_penalty"] for r in reqs], np.float32),
                pres=np.asarray([r["presence_penalty"] for r in reqs], np.float32), pen=pen, bias_ids=wid, bias_vals=wva, bias_cnt=cnt,
                bias_bits=bits.view(np.int32), stop_ids=fid, stop_seqs=fsq, seq_lens=fln,
                max_new=np.asarray([r["max_new_tokens"] for r in reqs], np.int32), hist=hist,
                hist_lens=np.asarray([len(r["history"]) for r in reqs], np.int32), mask=mask)


def _baseline_device(d, ctx, samp, stop, look):
    """the device half: torch row operations and the existing seen_mark launches"""
    idx = d["idx"]
    for name, src in (("temperature", "temperature"), ("top_k", "top_k"), ("top_p", "top_p"), ("seeds", "seeds"), ("repetition_penalty", "rep"),
                      ("presence_penalty", "pres"), ("bias_ids", "bias_ids"), ("bias_vals", "bias_vals"), ("bias_cnt", "bias_cnt"),
                      ("bias_bits", "bias_bits")):
        getattr(samp, name).index_copy_(0, idx, d[src])
    for t in (samp.draws, samp.logprobs, samp.u, samp.seen):
        t.index_fill_(0, idx, 0)
    samp.top_ids.index_fill_(0, idx, -1)
    samp.top_logprobs.index_fill_(0, idx, float("nan"))
    pending = torch.where(d["mask"] != 0, ctx["tokens"], -1)
    ops.seen_mark(samp.seen, pending.view(B, 1), VOCAB)
    ops.seen_mark(samp.seen, d["pen"], VOCAB)
    for name in ("stop_ids", "stop_seqs", "seq_lens", "max_new"):
        getattr(stop, name).index_copy_(0, idx, d[name])
    for t in (stop.gen_lens, stop.finished, stop.emit_lens):
        t.index_fill_(0, idx, 0)
    stop.tail.index_fill_(0, idx, -1)
    first = ctx["tokens"].index_select(0, idx)
    stop.tail[:, 14].index_copy_(0, idx, first)
    stop.last_token.index_copy_(0, idx, first)
    stop.live.copy_((stop.finished == 0).sum().view(1))
    look.history[:, :d["hist"].shape[1]].index_copy_(0, idx, d["hist"])
    look.hist_lens.index_copy_(0, idx, d["hist_lens"])
    return pending


def _same_states(x, y):
    for a, b in zip(x[1:], y[1:]):
        for k, v in vars(a).items():
            if torch.is_tensor(v) and k not in ("drafts", "match"):
                w = getattr(b, k)
                if not torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v, w.view(torch.int32) if w.dtype == torch.float32 else w):
                    return k
    return None


def launch_legs(dev, reps, launches, only):
    rng = np.random.default_rng(0)
    print("# slot admission alone: batch %d, vocabulary %d, every option on (512 penalty ids, 16 bias entries in rows of %d, top-N %d, stop rows "
          "(16, 8, 16), 512 history ids per request)" % (B, VOCAB, BIAS_LD, TOP_N))
    graphs, keep, eager = {}, [], {}
    for n in (1, 4, 16):
        slots = sorted(rng.choice(B, n, replace=False).tolist())
        reqs = _requests(n, rng)
        st, bt = _states(dev), _states(dev)
        blob, _ = ops.slots_pack(list(zip(slots, reqs)), VOCAB, WIDTHS)
        args = (st[0]["tokens"], st[0]["positions"], st[0]["placement"], st[0]["valid_lens"])
        dev_blob = ops.slots_admit(blob, *args, sampler=st[1], stop=st[2], lookup=st[3])
        host = _baseline_host(slots, reqs)
        up = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
        _baseline_device(up, *bt)
        torch.cuda.synchronize()
        diff = _same_states(st, bt)
        print("# n = %2d: blob %d words (%.1f KB); the baseline's states equal the launch's: %s" % (n, blob.size, blob.size * 4 / 1024,
                                                                                                    "yes" if diff is None else "NO, " + diff))

        def one(st=st, blob=blob, dev_blob=dev_blob, args=args):
            for _ in range(launches):
                ops.slots_admit((dev_blob, blob), *args, sampler=st[1], stop=st[2], lookup=st[3])

        def base(up=up, bt=bt):
            for _ in range(launches):
                _baseline_device(up, *bt)
        if "a" in only:
            graphs[(n, "zl_slots_admit")] = _graph(one)
        if "c" in only:
            graphs[(n, "baseline, device part")] = _graph(base)
        keep.append((st, bt, up, dev_blob))
        # eager wall clock, everything from the request dicts on
        for name, fn in (("b. slots_pack + slots_admit", lambda: ops.slots_admit(ops.slots_pack(list(zip(slots, reqs)), VOCAB, WIDTHS)[0], *args,
                                                                                  sampler=st[1], stop=st[2], lookup=st[3])),
                         ("c. baseline: host packing, uploads, row operations",
                          lambda: _baseline_device({k: torch.from_numpy(v).to(dev) for k, v in _baseline_host(slots, reqs).items()}, *bt))):
            if name[0] not in only:
                continue
            ts = []
            for r in range(reps + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= 3:
                    ts.append((time.perf_counter() - t0) * 1e3)
            eager[(n, name)] = ts
    if graphs:
        t = _alternate(graphs, reps)
        print("# a / c, captured: us per admission, median [p10 .. p90] over %d alternated replays of %d" % (reps, launches))
        for (n, name), ms in t.items():
            print("  n = %2d | %-24s | %8.2f [%8.2f .. %8.2f]" % ((n, name) + _stats(ms, launches)), flush=True)
    if eager:
        print("# b / c, eager wall clock from the request dicts to the end of the device work: us per admission, median [p10 .. p90] over %d calls" % reps)
        for (n, name), ms in eager.items():
            print("  n = %2d | %-52s | %8.1f [%8.1f .. %8.1f]" % ((n, name) + _stats(ms)), flush=True)


def _model(dev):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    model = LLaMA(ModelConfig.llama3_8b(), QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    return model


def serve_leg(dev, model, b=8, n_req=32, len_buf=1024):
    from zhilight_amd.serving import BatchServer
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, VOCAB, int(n)).astype(np.int32) for n in rng.integers(32, 384, n_req)]
    limits = [int(v) for v in rng.choice([16, 32, 64, 128, 256], n_req)]
    kw = dict(temperature=0.8, top_k=40, top_p=0.95)
    print("# d. end to end, synthetic Llama-3-8B GPTQ: %d requests, prompts of %d .. %d tokens, length limits %s, batch %d, poll 8"
          % (n_req, min(map(len, prompts)), max(map(len, prompts)), sorted(set(limits)), b))
    for run in range(2):                                                    # the first run warms allocations and kernels
        for capture in (True, False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            srv = BatchServer(model, b, len_buf, capture=capture, poll=8)
            for i, (p, lim) in enumerate(zip(prompts, limits)):
                srv.submit(p, seed=i, max_new_tokens=lim, **kw)
            res = srv.run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            toks = sum(len(r["tokens"]) for r in res.values())
            if run:
                print("  BatchServer (%s steps) | %5d tokens in %7.3f s = %7.1f tokens/s | %4d steps, slot-steps: %d live, %d on finished slots, "
                      "%d parked | %d admission rounds" % ("captured" if capture else "eager   ", toks, dt, toks / dt, srv.stats["steps"],
                                                           srv.stats["live_slot_steps"], srv.stats["finished_slot_steps"],
                                                           srv.stats["parked_slot_steps"], srv.stats["admissions"]), flush=True)
            del srv
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = steps = idle = 0
        for w in range(0, n_req, b):
            ctx = model.new_context(b, len_buf, 0)
            model.prefill_batch(ctx, list(range(b)), [torch.from_numpy(p) for p in prompts[w:w + b]])
            samp = model.new_sampler(ctx, seed=list(range(w, w + b)), **kw)
            stop = model.new_stopper(ctx, max_new_tokens=limits[w:w + b])
            out, _ = model.generate_sample(ctx, samp, max(limits[w:w + b]), stop=stop, poll=8)
            out = out.cpu()
            toks += int((out >= 0).sum())
            steps += out.shape[1]
            idle += int((out < 0).sum())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if run:
            print("  lock-step waves (eager steps) | %5d tokens in %7.3f s = %7.1f tokens/s | %4d steps, slot-steps: %d live, %d on finished slots"
                  % (toks, dt, toks / dt, steps, toks, idle), flush=True)


def step_leg(dev, model, reps, b=8, seq=1024):
    print("# e. captured step_sample, batch %d, %d tokens of history, T 0.8 / top-k 40 / top-p 0.95, with a stop state: ms per step, median "
          "[p10 .. p90] over %d alternated replays" % (b, seq, reps))
    len_buf = (seq + 4 * reps + 64 + 63) // 64 * 64
    kw = dict(temperature=0.8, top_k=40, top_p=0.95, seed=5)
    torch.manual_seed(7)
    ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in ("as before", "full width")}
    samp = {"as before": model.new_sampler(ctxs["as before"], **kw),
            "full width": model.new_sampler(ctxs["full width"], **kw, penalties=True, bias_ld=BIAS_LD, top_logprobs=TOP_N)}
    stop = {"as before": model.new_stopper(ctxs["as before"], max_new_tokens=1 << 20),
            "full width": model.new_stopper(ctxs["full width"], max_new_tokens=1 << 20, widths=(16, 8, 16))}
    graphs = {n: _graph(lambda n=n: model.step_sample(ctxs[n], samp[n], stop=stop[n])) for n in ctxs}
    for phase in ("before an admission", "after an admission"):
        if phase.startswith("after"):
            rng = np.random.default_rng(1)
            model.admit(ctxs["full width"], [1, 5], [torch.from_numpy(rng.integers(0, VOCAB, seq).astype(np.int32)) for _ in range(2)],
                        [dict(kw, seed=9, max_new_tokens=1 << 20), dict(kw, seed=10, max_new_tokens=1 << 20)], samp["full width"], stop["full width"])
        t = _alternate(graphs, reps)
        for n in graphs:
            print("  %-20s | %-50s | %7.3f [%6.3f .. %6.3f]" % ((phase, {"as before": "states as the commit before builds them",
                                                                        "full width": "full-width states (bitmap, bias rows, top-N)"}[n])
                                                               + tuple(v / 1e3 for v in _stats(t[n]))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b,c,d,e")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_admit: needs a GPU")
    dev, only = torch.device("cuda:0"), set(a.only.split(","))
    if only & {"a", "b", "c"}:
        launch_legs(dev, a.reps, a.launches, only)
    if only & {"d", "e"}:
        model = _model(dev)
        if "e" in only:
            step_leg(dev, model, a.reps)
        if "d" in only:
            serve_leg(dev, model)


if __name__ == "__main__":
    main()
