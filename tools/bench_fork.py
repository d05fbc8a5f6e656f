"""What n samples of one prompt cost (profiles/kv_fork.txt is this tool's output).  Llama-3-8B geometry (32 layers, 8 KV heads of 128,
fp16, BSHD: 1024 rows of one task = 128 MiB), one process.

  (a) the fork launch alone (zl_kv_fork): 1024 rows of one task to 1 / 3 / 7 destinations.  Captured graphs of `--launches` launches,
      each with another source and other destinations out of 16 tasks of 128 MiB (2 GiB: far more than the 256 MB Infinity Cache),
      replays alternated; us per launch and GB/s counting bytes read once per destination plus bytes written.  Next to it, in the same
      run, the route the prefix cache's launch offers for the same rows: zl_kv_blocks_copy save of the source's 8 blocks into a pool of
      8 blocks and load of them into the destinations, two launches;
  (b) the piece size (bytes of a run per workgroup, zl_kv_fork_ex) at 1 and 7 destinations, as in (a);
  (c) admission of one 1024-token prompt as n = 2 / 4 / 8 samples through LLaMA.admit_samples (one encode of 1023 rows, one fork
      launch, one admission launch) next to LLaMA.admit of n copies of the prompt (what a caller does without the fork: n encodes in one
      prefill_batch call), synthetic GPTQ weights: device time (events around the call) and wall time, calls alternated.

usage: python tools/bench_fork.py [--reps 20] [--launches 8] [--skip-model]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zhilight_amd._lib import lib  # noqa: E402

LAYERS, HKV, D, BLOCK, SEQ, TASKS = 32, 8, 128, 128, 1024, 16
TASK_BYTES = LAYERS * 2 * SEQ * HKV * D * 2


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


def _tasks(i, nd):
    """launch i of a graph: its source and nd destinations, rotating through the tasks"""
    src = (i * (nd + 1)) % TASKS
    return src, [(src + 1 + j) % TASKS for j in range(nd)]


def copy_legs(dev, reps, launches):
    f16 = dict(dtype=torch.float16, device=dev)
    kv = [torch.randn((LAYERS, 2, SEQ, HKV, D), **f16) for _ in range(TASKS)]
    pool = torch.randn((SEQ // BLOCK, LAYERS, 2, BLOCK, HKV, D), **f16)
    k_tab = torch.tensor([[t[l, 0].data_ptr() for t in kv] for l in range(LAYERS)], dtype=torch.int64, device=dev)
    v_tab = torch.tensor([[t[l, 1].data_ptr() for t in kv] for l in range(LAYERS)], dtype=torch.int64, device=dev)
    buf_lens = torch.full((TASKS,), SEQ, dtype=torch.int32, device=dev)
    rows4 = [torch.zeros(TASKS, dtype=torch.int32, device=dev) for _ in range(4)]
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    i64 = C.c_int64

    def fork(desc_dev, n, piece=0):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib().zl_kv_fork_ex(p(desc_dev), i64(n), p(k_tab), p(v_tab), p(buf_lens), i64(LAYERS), i64(TASKS), i64(SEQ), i64(HKV), i64(D * 2),
                                   C.c_int(1), *(p(t) for t in rows4), i64(piece), st) == 0

    def blocks(desc_dev, n, to_pool):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib().zl_kv_blocks_copy(p(desc_dev), i64(n), p(k_tab), p(v_tab), p(buf_lens), p(pool), i64(LAYERS), i64(TASKS), i64(BLOCK),
                                       i64(HKV), i64(D * 2), C.c_int(1), C.c_int(to_pool), st) == 0

    def fork_desc(i, nd):
        src, dsts = _tasks(i, nd)
        return torch.tensor([(src, d, SEQ, 7) for d in dsts] + [(src, src, 0, 7)], dtype=torch.int32, device=dev)

    def pool_desc(i, nd):
        src, dsts = _tasks(i, nd)
        nb = SEQ // BLOCK
        return (torch.tensor([(src, j * BLOCK, j) for j in range(nb)], dtype=torch.int32, device=dev),
                torch.tensor([(d, j * BLOCK, j) for d in dsts for j in range(nb)], dtype=torch.int32, device=dev))

    # one fork is what the save + load route gives: the destination's rows are the source's
    d = fork_desc(0, 3)
    fork(d, 4)
    torch.cuda.synchronize()
    src, dsts = _tasks(0, 3)
    assert all(torch.equal(kv[t], kv[src]) for t in dsts) and rows4[0][dsts[0]].item() == 7

    graphs, keep = {}, []
    for nd in (1, 3, 7):
        fd = [fork_desc(i, nd) for i in range(launches)]
        pd = [pool_desc(i, nd) for i in range(launches)]
        keep += [fd, pd]
        graphs[(nd, "fork, one launch")] = _graph(lambda fd=fd, nd=nd: [fork(x, nd + 1) for x in fd])
        graphs[(nd, "save + load, two")] = _graph(lambda pd=pd: [(blocks(s, s.shape[0], 1), blocks(ld, ld.shape[0], 0)) for s, ld in pd])
    t = _alternate(graphs, reps)
    print("# (a) %d rows (%.0f MiB) of one task to nd destinations, 16 tasks; us per fork, median [p10 .. p90] over %d alternated replays of "
          "%d; bytes = what the destinations receive; GB/s = 2 * bytes / median (the save + load route moves 2 * (1 + nd) * %.0f MiB)"
          % (SEQ, TASK_BYTES / 2 ** 20, reps, launches, TASK_BYTES / 2 ** 20))
    print("# nd | %-17s | %-32s | GB/s" % ("how", "captured us"))
    for (nd, how), ms in t.items():
        med, lo, hi = _stats(ms, launches)
        print("  %2d | %-17s | %9.1f [%9.1f .. %9.1f] | %6.0f" % (nd, how, med, lo, hi, 2 * nd * TASK_BYTES / (med * 1e-6) / 1e9), flush=True)
    print("# ratio of the captured medians, save + load / fork")
    for nd in (1, 3, 7):
        a, b = _stats(t[(nd, "fork, one launch")], launches)[0], _stats(t[(nd, "save + load, two")], launches)[0]
        print("  %2d | %6.2f x" % (nd, b / a), flush=True)
    del graphs

    graphs = {}
    for nd in (1, 7):
        fd = [fork_desc(i, nd) for i in range(launches)]
        keep.append(fd)
        for piece in (4096, 8192, 16384, 32768, 65536):
            graphs[(nd, piece)] = _graph(lambda fd=fd, nd=nd, piece=piece: [fork(x, nd + 1, piece) for x in fd])
    t = _alternate(graphs, reps)
    print("# (b) piece size: us per fork, median [p10 .. p90], GB/s")
    print("# nd | piece bytes | workgroups | captured us                      | GB/s")
    for (nd, piece), ms in t.items():
        med, lo, hi = _stats(ms, launches)
        print("  %2d | %11d | %10d | %9.1f [%9.1f .. %9.1f] | %6.0f" % (
            nd, piece, (nd + 1) * LAYERS * 2 * (SEQ * HKV * D * 2 // piece), med, lo, hi, 2 * nd * TASK_BYTES / (med * 1e-6) / 1e9), flush=True)


def model_leg(dev, reps):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.llama3_8b()
    model = LLaMA(cfg, QuantConfig(5, 128), dev)
    model.init_synthetic(seed=1234)
    b, len_buf = 8, SEQ + 64
    prompt = torch.randint(0, cfg.vocab_size, (SEQ,), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    ctx = model.new_context(b, len_buf, 0)
    samp = model.new_sampler(ctx, penalties=True)
    stop = model.new_stopper(ctx, widths=(16, 8, 16))
    reqs = [dict(temperature=0.8, top_p=0.95, seed=100 + j, max_new_tokens=32) for j in range(b)]
    calls = {}
    for n in (2, 4, 8):
        calls[(n, "admit_samples, one encode + fork")] = lambda n=n: model.admit_samples(ctx, [(list(range(n)), prompt, reqs[:n])], samp, stop)
        calls[(n, "admit of n copies, n encodes")] = lambda n=n: model.admit(ctx, list(range(n)), [prompt] * n, reqs[:n], samp, stop)
    dev_ms, wall_ms = {k: [] for k in calls}, {k: [] for k in calls}
    for r in range(2 + reps):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                wall_ms[k].append((time.perf_counter() - t0) * 1e3)
                dev_ms[k].append(e0.elapsed_time(e1))
    print("# (c) synthetic Llama-3-8B GPTQ, one %d-token prompt admitted as n samples into a batch of %d; %d alternated calls" % (SEQ, b, reps))
    print("#  n | call                               | device ms, median [p10 .. p90]   | wall ms, median [p10 .. p90]")
    for k in calls:
        d, w = (tuple(v / 1e3 for v in _stats(x)) for x in (dev_ms[k], wall_ms[k]))
        print("  %2d | %-34s | %8.3f [%8.3f .. %8.3f] | %8.3f [%8.3f .. %8.3f]" % (k + d + w), flush=True)
    print("# wall ratio, n copies / admit_samples")
    for n in (2, 4, 8):
        a, c = (statistics.median(wall_ms[(n, h)]) for h in ("admit_samples, one encode + fork", "admit of n copies, n encodes"))
        print("  %2d | %6.2f x" % (n, c / a), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fork: needs a GPU")
    dev = torch.device("cuda:0")
    copy_legs(dev, a.reps, a.launches)
    torch.cuda.empty_cache()
    if not a.skip_model:
        model_leg(dev, a.reps)


if __name__ == "__main__":
    main()
