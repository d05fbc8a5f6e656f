"""The prompt prefix cache's cost and gain (profiles/prefix_cache.txt is this tool's output).  Llama-3-8B geometry (32 layers, 8 KV
heads of 128, fp16: one block of 128 tokens = 16 MiB), synthetic GPTQ weights, one process.

  (a) TTFT of a 1024-token prompt cold: LLaMA.prefill_batch, one task;
  (b) the same prompt through LLaMA.prefill_cached with 896 tokens (7 blocks) in the cache: match, one load launch, 128 rows encoded;
      both as device time (events around the call) and as wall time (synchronised before and after), calls alternated;
  (c) the load and the save launch alone (zl_kv_blocks_copy) at 1, 2, 4 and 7 blocks: captured graphs of `--launches` launches, each
      on another task's buffers and other pool blocks (8 tasks of 128 MiB and a pool of 1 GiB: far more than the 256 MB Infinity
      Cache, so the bytes come from and go to HBM), replays alternated; us per launch and GB/s counting bytes read plus bytes written;
      next to it the same call through ops.kv_blocks_copy, eager, wall time per call: the host checks and the descriptor upload included;
  (d) the same bytes by the per-layer copy loop of TransformerBuffer::dump_slice / load_slice (one copy per layer, K/V and block),
      written with torch slice copies: eager (wall time per loop: the loop is bound by its launches) and as a captured graph;
  (e) the piece size (bytes of a run per workgroup, zl_kv_blocks_copy_ex) at 1 and 7 blocks, load and save, as in (c).

usage: python tools/bench_prefix_cache.py [--reps 20] [--launches 16] [--skip-model]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd import ops  # noqa: E402
from zhilight_amd._lib import lib  # noqa: E402

LAYERS, HKV, D, BLOCK, SEQ, TASKS, POOL_BLOCKS = 32, 8, 128, 128, 1024, 8, 64
BLOCK_BYTES = LAYERS * 2 * BLOCK * HKV * D * 2


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


def _wall(fn, reps, warm=2):
    out = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def _descs(i, nb):
    """launch i of a graph: task i % TASKS, its blocks 0 .. nb - 1, pool blocks that rotate through the pool"""
    return [(i % TASKS, j * BLOCK, (i * 7 + j) % POOL_BLOCKS) for j in range(nb)]


def copy_legs(dev, reps, launches):
    f16 = dict(dtype=torch.float16, device=dev)
    kv = [torch.randn((LAYERS, 2, SEQ, HKV, D), **f16) for _ in range(TASKS)]
    pool = torch.randn((POOL_BLOCKS, LAYERS, 2, BLOCK, HKV, D), **f16)
    k_tab = torch.tensor([[t[l, 0].data_ptr() for t in kv] for l in range(LAYERS)], dtype=torch.int64, device=dev)
    v_tab = torch.tensor([[t[l, 1].data_ptr() for t in kv] for l in range(LAYERS)], dtype=torch.int64, device=dev)
    buf_lens = torch.full((TASKS,), SEQ, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    i64 = C.c_int64

    def launch(desc_dev, n, to_pool, piece=0):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib().zl_kv_blocks_copy_ex(p(desc_dev), i64(n), p(k_tab), p(v_tab), p(buf_lens), p(pool), i64(LAYERS), i64(TASKS), i64(BLOCK),
                                          i64(HKV), i64(D * 2), C.c_int(1), C.c_int(to_pool), i64(piece), st) == 0

    def loop(descs, to_pool):
        for task, slot, pb in descs:
            for l in range(LAYERS):
                for j in (0, 1):
                    if to_pool:
                        pool[pb, l, j].copy_(kv[task][l, j, slot:slot + BLOCK])
                    else:
                        kv[task][l, j, slot:slot + BLOCK].copy_(pool[pb, l, j])

    graphs, keep, eager = {}, [], {}
    for nb in (1, 2, 4, 7):
        sets = [_descs(i, nb) for i in range(launches)]
        devs = [torch.tensor(s, dtype=torch.int32, device=dev) for s in sets]
        keep.append(devs)
        for to_pool, name in ((0, "load"), (1, "save")):
            graphs[(nb, name, "one launch")] = _graph(lambda devs=devs, nb=nb, to_pool=to_pool: [launch(d, nb, to_pool) for d in devs])
            graphs[(nb, name, "copy loop")] = _graph(lambda sets=sets, to_pool=to_pool: [loop(s, to_pool) for s in sets])
            it = iter(range(1 << 30))
            eager[(nb, name, "one launch")] = _wall(lambda sets=sets, to_pool=to_pool, it=it: ops.kv_blocks_copy(
                sets[next(it) % launches], k_tab, v_tab, buf_lens, pool, BLOCK, HKV, D * 2, to_pool, buf_lens_host=[SEQ] * TASKS), reps)
            it2 = iter(range(1 << 30))
            eager[(nb, name, "copy loop")] = _wall(lambda sets=sets, to_pool=to_pool, it2=it2: loop(sets[next(it2) % launches], to_pool), reps)
    t = _alternate(graphs, reps)
    print("# (c), (d) blocks of %.1f MiB between 8 tasks' buffers and a pool of %d blocks; captured: us per launch / per loop, median [p10 .. p90] "
          "over %d alternated replays of %d; eager: wall us per call, median; GB/s = (read + written) / captured median"
          % (BLOCK_BYTES / 2 ** 20, POOL_BLOCKS, reps, launches))
    print("# blocks | dir  | %-10s | %-32s | %-9s | eager wall us" % ("how", "captured us", "GB/s"))
    for (nb, name, how), ms in t.items():
        med, lo, hi = _stats(ms, launches)
        print("  %6d | %-4s | %-10s | %9.1f [%9.1f .. %9.1f] | %9.0f | %10.1f" % (
            nb, name, how, med, lo, hi, 2 * nb * BLOCK_BYTES / (med * 1e-6) / 1e9, statistics.median(eager[(nb, name, how)]) * 1e3), flush=True)
    print("# ratio of the captured medians, copy loop / one launch, and of the eager wall medians")
    for nb in (1, 2, 4, 7):
        for name in ("load", "save"):
            a, b = _stats(t[(nb, name, "one launch")], launches)[0], _stats(t[(nb, name, "copy loop")], launches)[0]
            ea, eb = (statistics.median(eager[(nb, name, h)]) for h in ("one launch", "copy loop"))
            print("  %6d | %-4s | captured %6.2f x | eager %6.2f x" % (nb, name, b / a, eb / ea), flush=True)
    del graphs

    pieces = (4096, 8192, 16384, 32768, 65536)
    graphs = {}
    for nb in (1, 7):
        devs = [torch.tensor(_descs(i, nb), dtype=torch.int32, device=dev) for i in range(launches)]
        keep.append(devs)
        for to_pool, name in ((0, "load"), (1, "save")):
            for piece in pieces:
                graphs[(nb, name, piece)] = _graph(lambda devs=devs, nb=nb, to_pool=to_pool, piece=piece: [launch(d, nb, to_pool, piece) for d in devs])
    t = _alternate(graphs, reps)
    print("# (e) piece size: us per launch, median [p10 .. p90], GB/s")
    print("# blocks | dir  | piece bytes | workgroups | captured us                      | GB/s")
    for (nb, name, piece), ms in t.items():
        med, lo, hi = _stats(ms, launches)
        print("  %6d | %-4s | %11d | %10d | %9.1f [%9.1f .. %9.1f] | %9.0f" % (
            nb, name, piece, nb * LAYERS * 2 * (BLOCK * HKV * D * 2 // piece), med, lo, hi, 2 * nb * BLOCK_BYTES / (med * 1e-6) / 1e9), flush=True)


def model_leg(dev, reps):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    len_buf = SEQ + 64
    prompt = torch.randint(0, cfg.vocab_size, (SEQ,), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    ctx = model.new_context(2, len_buf, 0)
    cache = model.new_prefix_cache(ctx, 16)
    _, m = model.prefill_cached(ctx, cache, [0], [prompt])
    assert m == [0] and len(cache.index) == 8
    ref = model.prefill_batch(ctx, [0], [prompt])
    got, m = model.prefill_cached(ctx, cache, [1], [prompt])
    assert m == [SEQ - BLOCK]
    print("# (a), (b) synthetic Llama-3-8B GPTQ, %d-token prompt, one task; cached: %d tokens from the cache, %d encoded; the two calls' last-row "
          "logits: max |difference| %.3e (max |logit| %.3e)" % (SEQ, m[0], SEQ - m[0], (got.float() - ref.float()).abs().max().item(),
                                                              ref.float().abs().max().item()))
    calls = {"prefill_batch, cold": lambda: model.prefill_batch(ctx, [0], [prompt]),
             "prefill_cached, 896 cached": lambda: model.prefill_cached(ctx, cache, [1], [prompt])}
    dev_ms, wall_ms = {n: [] for n in calls}, {n: [] for n in calls}
    for r in range(2 + reps):
        for n, fn in calls.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                wall_ms[n].append((time.perf_counter() - t0) * 1e3)
                dev_ms[n].append(e0.elapsed_time(e1))
    print("# call                        | device ms, median [p10 .. p90]   | wall ms, median [p10 .. p90]")
    for n in calls:
        d, w = (tuple(v / 1e3 for v in _stats(x)) for x in (dev_ms[n], wall_ms[n]))
        print("  %-27s | %8.3f [%8.3f .. %8.3f] | %8.3f [%8.3f .. %8.3f]" % ((n,) + d + w), flush=True)
    a, b = (statistics.median(wall_ms[n]) for n in calls)
    print("# wall ratio cached / cold: %.3f; index counters: %s" % (b / a, cache.index.counters()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=16)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix_cache: needs a GPU")
    dev = torch.device("cuda:0")
    copy_legs(dev, a.reps, a.launches)
    torch.cuda.empty_cache()
    if not a.skip_model:
        model_leg(dev, a.reps)


if __name__ == "__main__":
    main()
