"""What sharing a prompt's K/V between slots costs and saves (profiles/shared_prefix.txt is this tool's output).  Llama-3-8B geometry
(32 layers, 32 query heads, 8 KV heads of 128, fp16, BSHD), one process.  `members` slots of a batch read ONE prefix of P rows
(zl_decode_attn_shared) and 64 rows of their own, next to the same slots holding the prefix as copies.

  (a) the attention of one layer.  Captured graphs of `--launches` launches, each over another layer's buffers (the copies of 32 slots
      at 4096 rows are 550 MB per layer: far more than the Infinity Cache; the shared prefixes of 8 layers are not: 134 MB at 4096 rows,
      so (a) flatters the shared route where (b) does not), replays alternated, median [p10 .. p90] us per launch:
        copies, la        zl_decode_attn_la over the copies: what the parent route's step launches at these batch sizes
        copies, two       zl_decode_attn (split kernel + merge) over the copies
        table unused      zl_decode_attn_shared over the copies with prefix_of = -1 everywhere: the price of enabling the feature
        shared            zl_decode_attn_shared, every slot on the one prefix
      (the "shared, spread" rows of profiles/shared_prefix.txt: the same tool against a library built with -DZL_ATTN_SHARED_SPREAD,
      which deals the 16-row tiles of one (prefix, kv head, split) to neighbouring workgroups, one per XCD, instead of behind one L2)
  (b) the whole captured step_sample, synthetic GPTQ weights: the parent route (a context without a table, the prefix as copies), the
      same context with a table nobody uses, and the sharing context; all slots members, and 2 members of 8 slots (the case
      serving.SHARE_MIN_ROWS is set from).

usage: python tools/bench_shared.py [--reps 12] [--launches 8] [--skip-model] [--skip-attn]"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402

H, HKV, D, OWN = 32, 8, 128, 64
SCALE = 1.0 / math.sqrt(D)


def _graph(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def _alternate(graphs, reps, warm=2):
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


def attention_leg(dev, reps, launches):
    f16, i32 = dict(dtype=torch.float16, device=dev), dict(dtype=torch.int32, device=dev)
    print("# (a) one layer's decode attention, us per launch, median [p10 .. p90] over %d alternated replays of %d launches (each over "
          "another layer's buffers); b slots, all on one prefix of P rows + %d own rows; MiB = K/V bytes the route reads per launch"
          % (reps, launches, OWN))
    print("#  b |    P | %-15s | %-32s | MiB read" % ("route", "captured us"))
    for b in (8, 32):
        for P in (1024, 2048, 4096):
            len_buf, valid = P + 2 * OWN, P + OWN
            copies = [[torch.randn((2, len_buf, HKV, D), **f16) for _ in range(b)] for _ in range(launches)]
            prefix = [torch.randn((2, P, HKV, D), **f16) for _ in range(launches)]
            tabs = [(ops.make_ptr_table([t[0] for t in layer]), ops.make_ptr_table([t[1] for t in layer])) for layer in copies]
            ptabs = [(ops.make_ptr_table([t[0]]), ops.make_ptr_table([t[1]])) for t in prefix]
            q, out = torch.randn((b, 1, H, D), **f16), torch.empty((b, 1, H, D), **f16)
            buf_lens, valid_lens = torch.full((b,), len_buf, **i32), torch.full((b,), valid, **i32)
            none, all0 = torch.full((b,), -1, **i32), torch.zeros(b, **i32)
            plens, caps = torch.full((1,), P, **i32), torch.full((1,), P, **i32)
            ws = ops.decode_attn_workspace(b, 1, H, D, len_buf, dev)
            ws_la = ops.decode_attn_la_workspace(b, H, HKV, len_buf, dev)
            ws_sh = ops.decode_attn_shared_workspace(b, 1, H, HKV, D, P, len_buf, dev)
            la_ok = (len_buf + ops.decode_attn_la_split_len(b, HKV, len_buf) - 1) // ops.decode_attn_la_split_len(b, HKV, len_buf) <= 64

            def shared(i, of):
                ops.decode_attention_shared(q, buf_lens, *tabs[i], valid_lens, of, plens, caps, *ptabs[i], SCALE, P, len_buf, HKV, out=out,
                                            workspace=ws_sh)
            routes = {
                "copies, two": lambda i: ops.multi_query_attention_rag_buffer(q, buf_lens, *tabs[i], None, SCALE, len_buf, HKV,
                                                                              valid_lens=valid_lens, out=out, workspace=ws),
                "table unused": lambda i: shared(i, none),
                "shared": lambda i: shared(i, all0),
            }
            if la_ok:
                routes = {"copies, la": lambda i: ops.decode_attention_la(q, buf_lens, *tabs[i], valid_lens, SCALE, len_buf, HKV, ws_la,
                                                                          out=out), **routes}
            graphs = {n: _graph(lambda fn=fn: [fn(i) for i in range(launches)]) for n, fn in routes.items()}
            t = _alternate(graphs, reps)
            row = 2 * HKV * D * 2 / 2 ** 20                                                 # MiB of one K + V row
            for n, ms in t.items():
                med, lo, hi = _stats(ms, launches)
                mib = row * (b * valid if n.startswith(("copies", "table")) else P + b * OWN)
                print(" %3d | %4d | %-15s | %9.1f [%9.1f .. %9.1f] | %8.1f" % (b, P, n, med, lo, hi, mib), flush=True)
            del graphs, copies, prefix
            torch.cuda.empty_cache()


def model_leg(dev, reps):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    print("# (b) synthetic Llama-3-8B GPTQ, one captured step_sample, ms per step, median [p10 .. p90] over %d alternated replays; b slots "
          "at position P + %d, `members` of them on one prefix of P rows (the others, and every slot of the two copy routes, hold P + %d "
          "rows of their own)" % (reps, OWN, OWN))
    print("#  b | members |    P | %-28s | %-29s | tokens/s" % ("route", "captured ms"))
    shapes = [(b, b, P) for b in (8, 32) for P in (1024, 2048, 4096)] + [(8, 2, P) for P in (256, 512, 1024, 2048, 4096)]
    for b, members, P in shapes:
        len_buf = P + OWN + 4 * (reps + 8)                                                  # every replay of every graph advances a slot by one row
        graphs = {}
        plain = model.new_context(b, len_buf, P + OWN, fill_random=True)
        samp_p = model.new_sampler(plain, temperature=0.8, top_p=0.95, seed=7)
        graphs["parent route, copies"] = _graph(lambda: model.step_sample(plain, samp_p))
        model.new_shared_prefixes(plain, 1, P)
        graphs["table unused, copies"] = _graph(lambda: model.step_sample(plain, samp_p))
        sharing = model.new_context(b, len_buf, P + OWN, fill_random=True)
        samp_s = model.new_sampler(sharing, temperature=0.8, top_p=0.95, seed=7)
        sh = model.new_shared_prefixes(sharing, 1, P)
        sh.kv[0].normal_()
        sh.prefix_lens.fill_(P)
        sh.prefix_of[:members] = 0
        graphs["shared"] = _graph(lambda: model.step_sample(sharing, samp_s))
        t = _alternate(graphs, reps)
        for n, ms in t.items():
            med, lo, hi = (v / 1e3 for v in _stats(ms))
            print(" %3d | %7d | %4d | %-28s | %8.3f [%8.3f .. %8.3f] | %8.0f" % (b, members, P, n, med, lo, hi, b / (med * 1e-3)), flush=True)
        del graphs, plain, sharing, sh
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-attn", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shared: needs a GPU")
    dev = torch.device("cuda:0")
    if not a.skip_attn:
        attention_leg(dev, a.reps, a.launches)
        torch.cuda.empty_cache()
    if not a.skip_model:
        model_leg(dev, a.reps)


if __name__ == "__main__":
    main()
