"""The speculative verify step against its baselines (profiles/spec_verify.txt is this tool's output).

  1. attention alone, Llama-3-8B geometry (H 32, Hkv 8, D 128), 1025 visible keys in 1088-key buffers, B x len_q rows:
     zl_decode_attn_causal (one pass over a task's K / V for its len_q rows) against the len_q = 1 kernels with every row posed as
     a task of its own -- the two-launch route (zl_decode_attn) and the in-launch merge (zl_decode_attn_la), what
     LLaMA.verify(attn="rows") runs from 5 rows on.  Every variant is a captured graph of `layers` launches over distinct buffers,
     enough of them that one replay streams more than the 256 MB cache; the variants' replays alternate, device events around each.
  2. the whole step on the synthetic 32-layer model: verify (K drafts, both attention routes) against step_greedy at the same B,
     captured graphs, replays alternated; break-even accepted drafts per step = t_verify / t_step - 1.

usage: python tools/bench_spec.py [--attn-only | --step-only] [--reps 30] [--layers 0] [--k 3]"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402

H, HKV, D, LEN_BUF, VISIBLE = 32, 8, 128, 1088, 1025


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


def attention_leg(dev, reps, layers_arg):
    scale = 1.0 / math.sqrt(D)
    print("# attention alone: us per layer, median [p10 .. p90] over %d alternated replays; H %d Hkv %d D %d, %d visible keys in %d-key "
          "buffers" % (reps, H, HKV, D, VISIBLE, LEN_BUF))
    print("#  B len_q rows layers |  causal                 | rows, two launches      | rows, in-launch merge   | causal/rows2  causal/rowsLA |"
          " max|causal - rows2|  max|causal - rowsLA|")
    i32 = dict(dtype=torch.int32, device=dev)
    for b in (1, 4, 8):
        for len_q in (2, 4, 8):
            m = b * len_q
            if m > 32:
                continue
            task_bytes = 2 * LEN_BUF * HKV * D * 2
            layers = layers_arg or max(8, -(-(640 << 20) // (b * task_bytes)))          # > 2 x the 256 MB cache per replay
            kv = torch.randn((layers, b, 2, LEN_BUF, HKV, D), dtype=torch.float16, device=dev)
            k_tab = torch.tensor([[kv[l, t, 0].data_ptr() for t in range(b)] for l in range(layers)], dtype=torch.int64, device=dev)
            v_tab = torch.tensor([[kv[l, t, 1].data_ptr() for t in range(b)] for l in range(layers)], dtype=torch.int64, device=dev)
            row_task = torch.arange(b, device=dev).view(b, 1).expand(b, len_q).reshape(m)
            k_rows, v_rows = k_tab.index_select(1, row_task), v_tab.index_select(1, row_task)
            lens = torch.full((b,), LEN_BUF, **i32)
            lens_rows = torch.full((m,), LEN_BUF, **i32)
            valid = torch.full((b,), VISIBLE - (len_q - 1), **i32)                      # the last row sees VISIBLE keys
            valid_rows = (valid.view(b, 1) + torch.arange(len_q, **i32).view(1, len_q)).reshape(m).contiguous()
            q = torch.randn((b, len_q, H, D), dtype=torch.float16, device=dev)
            outs = {n: torch.empty_like(q) for n in ("causal", "rows2", "rowsLA")}
            ws = ops.decode_attn_workspace(b, len_q, H, D, LEN_BUF, dev)
            ws_la = ops.decode_attn_la_workspace(m, H, HKV, LEN_BUF, dev)

            def causal():
                for l in range(layers):
                    ops.decode_attention_causal(q, lens, k_tab[l], v_tab[l], valid, scale, LEN_BUF, HKV, out=outs["causal"], workspace=ws)

            def rows2():
                for l in range(layers):
                    ops.multi_query_attention_rag_buffer(q.view(m, 1, H, D), lens_rows, k_rows[l], v_rows[l], None, scale, LEN_BUF, HKV,
                                                         valid_lens=valid_rows, out=outs["rows2"].view(m, 1, H, D), workspace=ws)

            def rows_la():
                for l in range(layers):
                    ops.decode_attention_la(q.view(m, 1, H, D), lens_rows, k_rows[l], v_rows[l], valid_rows, scale, LEN_BUF, HKV, ws_la,
                                            out=outs["rowsLA"].view(m, 1, H, D))
            graphs = {"causal": _graph(causal), "rows2": _graph(rows2), "rowsLA": _graph(rows_la)}
            t = _alternate(graphs, reps)
            st = {n: _stats(t[n], layers) for n in graphs}
            d2 = float((outs["causal"].float() - outs["rows2"].float()).abs().max())
            dla = float((outs["causal"].float() - outs["rowsLA"].float()).abs().max())
            cell = lambda s: "%7.2f [%6.2f .. %6.2f]" % s                                # noqa: E731
            print("  %2d  %2d   %3d   %4d  | %s | %s | %s |    %5.3f         %5.3f     |      %.3e           %.3e" % (
                b, len_q, m, layers, cell(st["causal"]), cell(st["rows2"]), cell(st["rowsLA"]), st["causal"][0] / st["rows2"][0],
                st["causal"][0] / st["rowsLA"][0], d2, dla), flush=True)
            del graphs, kv
            torch.cuda.empty_cache()


def step_leg(dev, reps, k, batches):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    seq, len_q = 1024, k + 1
    len_buf = (seq + (reps + 8) * len_q + 63) // 64 * 64
    print("# whole step, synthetic Llama-3-8B GPTQ, 32 layers, %d tokens of history, K = %d drafts (random: about one token kept per step); "
          "ms per step, median [p10 .. p90] over %d alternated replays" % (seq, k, reps))
    print("#  B rows | step_greedy             | verify causal           | verify rows             | causal/rows | break-even accepted drafts "
          "(causal) (rows) | same accepted / max |logits diff| causal vs rows")
    for b in batches:
        if b * len_q > 32:
            continue
        torch.manual_seed(7)
        ctxs = {n: model.new_context(b, len_buf, seq, fill_random=True) for n in ("step", "causal", "rows")}
        tok = torch.randint(0, cfg.vocab_size, (b,), device=dev, dtype=torch.int32)
        for c in ctxs.values():
            c.tokens.copy_(tok)
        for n in ("causal", "rows"):                                                     # the same history under both routes
            for t, src in zip(ctxs[n].kv, ctxs["step"].kv):
                t.copy_(src)
        drafts = torch.randint(0, cfg.vocab_size, (b, k), device=dev, dtype=torch.int32)
        res = {}
        graphs = {"step": _graph(lambda: model.step_greedy(ctxs["step"]))}
        for n in ("causal", "rows"):
            res[n] = model.verify(ctxs[n], drafts, attn=n)                               # eager: tables; first results for the A/B
            res[n] = (res[n].logits.float().clone(), res[n].accepted.clone())
        same = bool(torch.equal(res["causal"][1], res["rows"][1]))
        diff = float((res["causal"][0] - res["rows"][0]).abs().max())
        for n in ("causal", "rows"):
            graphs[n] = _graph(lambda n=n: model.verify(ctxs[n], drafts, attn=n))
        t = _alternate(graphs, reps)
        st = {n: tuple(v / 1e3 for v in _stats(t[n], 1)) for n in graphs}
        cell = lambda s: "%7.3f [%6.3f .. %6.3f]" % s                                    # noqa: E731
        print("  %2d  %3d | %s | %s | %s |    %5.3f    |        %5.2f    %5.2f                 | %s / %.3e" % (
            b, b * len_q, cell(st["step"]), cell(st["causal"]), cell(st["rows"]), st["causal"][0] / st["rows"][0],
            st["causal"][0] / st["step"][0] - 1, st["rows"][0] / st["step"][0] - 1, same, diff), flush=True)
        del graphs, ctxs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--layers", type=int, default=0, help="attention leg: launches per replay (0: enough to stream 640 MB)")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4, 8])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spec: needs a GPU")
    dev = torch.device("cuda:0")
    if not a.step_only:
        attention_leg(dev, a.reps, a.layers)
    if not a.attn_only:
        step_leg(dev, a.reps, a.k, a.batches)


if __name__ == "__main__":
    main()
