"""The host side of forked samples, no device: ops.kv_fork_check, the numpy model of the launch (fork_ref.py), zl_kv_fork's argument
statuses, LLaMA.fork_descriptors, BatchServer.submit's refusals for n / best_of / sample_first and the ranking of the samples."""
import collections
import types

import numpy as np
import pytest

import fork_ref as fr

LENS = (40, 64, 33, 128, 7, 64)


# ---- ops.kv_fork_check ------------------------------------------------------------------------------------------------------------------
def test_kv_fork_check_accepts_and_normalises():
    from zhilight_amd import ops
    desc = [(0, 1, 33, 5), (0, 2, 0, 5), [0, 4, 7, 5], (0, 0, 0, 5), (3, 5, 1, -1), np.array([3, 3, 0, -1], np.int32)]
    out, max_rows = ops.kv_fork_check(desc, LENS, 6)
    assert out == [(0, 1, 33, 5), (0, 2, 0, 5), (0, 4, 7, 5), (0, 0, 0, 5), (3, 5, 1, -1), (3, 3, 0, -1)] and max_rows == 33
    assert all(type(x) is int for d in out for x in d)
    assert ops.kv_fork_check(np.asarray(out, np.int32), np.asarray(LENS), 6) == (out, 33)
    assert ops.kv_fork_check([], LENS, 6) == ([], 0)
    # a self-descriptor without an override leaves its other descriptors free; rows = the whole of both buffers
    assert ops.kv_fork_check([(1, 5, 64, 9), (1, 1, 0, -1)], LENS, 6, vocab=10)[1] == 64
    # an override that every other descriptor of the source names
    ops.kv_fork_check([(1, 5, 3, 9), (1, 2, 3, 9), (1, 1, 0, 9)], LENS, 6, vocab=10)


@pytest.mark.parametrize("desc,match", [
    ([(0, 1, 3)], "four integers"), ([(0, 1, 3, 4, 5)], "four integers"), ([(0, 1, 3.0, 4)], "four integers"),
    ([(0, 1, True, 4)], "four integers"), ([7], "four integers"),
    ([(6, 1, 0, 0)], "outside the batch"), ([(0, -1, 0, 0)], "outside the batch"), ([(0, 6, 0, 0)], "outside the batch"),
    ([(0, 1, -1, 0)], "outside a buffer"), ([(0, 1, 41, 0)], "outside a buffer"), ([(1, 4, 8, 0)], "outside a buffer"),
    ([(0, 1, 3, 0), (2, 1, 3, 0)], "destination twice"), ([(0, 1, 3, 0), (0, 1, 4, 0)], "destination twice"),
    ([(0, 0, 0, 1), (0, 0, 0, 2)], "destination twice"),
    ([(0, 1, 3, 0), (1, 2, 3, 0)], "a destination and a source"), ([(1, 2, 3, 0), (0, 1, 3, 0)], "a destination and a source"),
    ([(0, 1, 3, 0), (1, 1, 0, 4)], "destination twice"), ([(1, 1, 0, 4), (0, 1, 3, 0)], "destination twice"),
    ([(0, 1, 3, 5), (0, 0, 0, 6)], "overrides its token"), ([(0, 0, 0, 6), (0, 1, 3, -1)], "overrides its token"),
    ([(0, 1, 3, 1 << 31)], "outside the vocabulary"),
])
def test_kv_fork_check_refuses(desc, match):
    from zhilight_amd import ops
    with pytest.raises(ops.ZLError, match=match):
        ops.kv_fork_check(desc, LENS, 6)


def test_kv_fork_check_vocab_and_lengths():
    from zhilight_amd import ops
    ops.kv_fork_check([(0, 1, 3, 9)], LENS, 6, vocab=10)
    with pytest.raises(ops.ZLError, match="outside the vocabulary"):
        ops.kv_fork_check([(0, 1, 3, 10)], LENS, 6, vocab=10)
    with pytest.raises(ops.ZLError, match="one buffer length per task"):
        ops.kv_fork_check([(0, 1, 3, 9)], LENS, 5)


# ---- the numpy model --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bshd", [True, False])
def test_fork_ref_copies_rows_sets_bookkeeping_and_drops(bshd):
    rng = np.random.default_rng(1)
    hkv, rb = 2, 8
    bufs = [rng.integers(0, 256, (3, 2, n, hkv, rb) if bshd else (3, 2, hkv, n, rb), dtype=np.uint8) for n in LENS]
    old = [x.copy() for x in bufs]
    ctx = {f: rng.integers(0, 1000, 6).astype(np.int32) for f in fr.CTX}
    old_ctx = {f: v.copy() for f, v in ctx.items()}
    desc = [(0, 1, 33, 77), (0, 4, 7, -1), (0, 0, 0, -1), (3, 3, 0, 11), (3, 5, 1, 11),
            (0, 6, 1, 0), (3, 2, 34, 0), (3, 2, 40, 0), (-1, 2, 1, 0)]       # dropped: dst = b, rows > buf_lens[dst], rows > max_rows, src < 0
    done = fr.fork(desc, bufs, LENS, bshd, 33, ctx)
    assert done == desc[:5]
    rows = (lambda t, n: t[:, :, :n]) if bshd else (lambda t, n: t[:, :, :, :n])
    rest = (lambda t, n: t[:, :, n:]) if bshd else (lambda t, n: t[:, :, :, n:])
    for dst, src, n in ((1, 0, 33), (4, 0, 7), (5, 3, 1)):
        assert np.array_equal(rows(bufs[dst], n), rows(old[src], n)) and np.array_equal(rest(bufs[dst], n), rest(old[dst], n))
    for t in (0, 2, 3):
        assert np.array_equal(bufs[t], old[t])
    assert ctx["tokens"].tolist() == [old_ctx["tokens"][0], 77, old_ctx["tokens"][2], 11, old_ctx["tokens"][0], 11]
    for f in fr.CTX[1:]:
        o = old_ctx[f]
        assert ctx[f].tolist() == [o[0], o[0], o[2], o[3], o[0], o[3]]
    assert fr.fork(desc, [x.copy() for x in old], LENS, bshd, 33, None) == desc[:5]


def test_fork_launcher_argument_statuses_without_a_launch():
    """zl_kv_fork's argument checks return before any launch, so they run without a device"""
    import ctypes as C
    from zhilight_amd._lib import lib
    i64, one = C.c_int64, C.c_void_p(16)                         # a non-null stand-in: never dereferenced

    def call(n=1, desc=one, tab=one, layers=2, b=3, max_rows=16, hkv=2, row_bytes=256, piece=0, rows4=(None,) * 4):
        return lib().zl_kv_fork_ex(desc, i64(n), tab, one, one, i64(layers), i64(b), i64(max_rows), i64(hkv), i64(row_bytes), C.c_int(1),
                                   *rows4, i64(piece), None)
    assert call(n=0, desc=None, tab=None) == 0                   # n == 0: ZL_OK, nothing is read
    assert lib().zl_kv_fork(None, i64(0), None, None, None, i64(2), i64(3), i64(0), i64(2), i64(256), C.c_int(0), None, None, None, None, None) == 0
    assert call(n=-1) == -1 and call(desc=None) == -1 and call(tab=None) == -1 and call(layers=0) == -1 and call(row_bytes=0) == -1
    assert call(max_rows=-1) == -1 and call(hkv=0) == -1
    for rows4 in ((one, None, None, None), (one, one, one, None), (None, one, one, one)):        # the bookkeeping pointers given in part
        assert call(rows4=rows4) == -1 and call(n=0, rows4=rows4) == -1
    assert call(row_bytes=6) == -2 and call(piece=24) == -2      # ZL_ESHAPE
    assert call(layers=1 << 20) == -4 and call(n=1 << 31) == -4 and call(row_bytes=1 << 30) == -4      # ZL_ELIMIT
    assert call(n=1 << 20, layers=65535, max_rows=1 << 20, hkv=1, row_bytes=1 << 20, piece=16) == -4     # beyond the grid


# ---- LLaMA.fork_descriptors ---------------------------------------------------------------------------------------------------------------
def test_fork_descriptors_of_two_groups_one_of_them_a_single_slot():
    import torch
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA
    groups = [([2, 0, 5], torch.tensor([4, 8, 15, 16, 23], dtype=torch.int32)), ([3], np.array([42, 7], np.int32))]
    desc = LLaMA.fork_descriptors(groups)
    assert desc == [(2, 0, 4, 23), (2, 5, 4, 23), (2, 2, 0, 23), (3, 3, 0, 7)]
    assert ops.kv_fork_check(desc, [16] * 6, 6, vocab=64) == (desc, 4)
    # the model of the launch: slots 0 and 5 stand where slot 2 stands, every slot of a group holds the re-fed token
    ctx = {f: np.arange(6, dtype=np.int32) * 10 + i for i, f in enumerate(fr.CTX)}
    bufs = [np.full((1, 2, 16, 1, 4), t, np.uint8) for t in range(6)]
    fr.fork(desc, bufs, [16] * 6, True, 4, ctx)
    assert ctx["tokens"].tolist() == [23, 10, 23, 7, 40, 23] and ctx["positions"].tolist() == [21, 11, 21, 31, 41, 21]
    assert all((bufs[t][:, :, :4] == 2).all() and (bufs[t][:, :, 4:] == t).all() for t in (0, 2, 5)) and (bufs[3] == 3).all()


# ---- BatchServer.submit and the ranking ---------------------------------------------------------------------------------------------------
def _server(batch=4, len_buf=32, vocab=100):
    """a BatchServer with the fields submit() reads and no device behind it"""
    from zhilight_amd.llama import LLaMA
    from zhilight_amd.serving import BatchServer
    srv = object.__new__(BatchServer)
    srv.b, srv.len_buf, srv.k, srv.lookup = batch, len_buf, 0, None
    srv.sampler = types.SimpleNamespace(fsm=None, seen=None, bias_ids=None)
    srv.stop = types.SimpleNamespace(stop_ids=np.zeros((batch, 16)), stop_seqs=np.zeros((batch, 8, 16)))
    srv.model = types.SimpleNamespace(cfg=types.SimpleNamespace(vocab_size=vocab), slot_widths=LLaMA.slot_widths)
    srv.queue, srv.requests, srv.meta = collections.deque(), {}, {}
    return srv


def test_submit_takes_n_best_of_and_sample_first():
    srv = _server()
    p = list(range(10))
    assert srv.submit(p) == 0 and srv.submit(p, n=3, seed=5) == 1 and srv.submit(p, n=2, best_of=4) == 2
    assert srv.submit(p, sample_first=True) == 3 and srv.submit(p[:2], n=2) == 4 and srv.submit(p[:1]) == 5
    assert srv.submit(p, n=2, seed=(1 << 64) - 2) == 6 and srv.submit(p, n=2, seed=-(1 << 63)) == 7
    assert [srv.meta[r] for r in range(8)] == [(1, 1, False), (3, 3, True), (2, 4, True), (1, 1, True), (2, 2, True), (1, 1, False),
                                               (2, 2, True), (2, 2, True)]
    assert list(srv.queue) == list(range(8)) and srv.requests[1][1] == dict(seed=5)
    assert srv.submit(list(range(30)), max_new_tokens=1) == 8 and srv.submit(list(range(31)), n=2) == 9      # 30 rows encoded: room for one


@pytest.mark.parametrize("kw,match", [
    (dict(n=0), "1 <= n <= best_of <= batch"), (dict(n=5), "1 <= n <= best_of <= batch"), (dict(n=2, best_of=5), "1 <= n <= best_of <= batch"),
    (dict(n=3, best_of=2), "1 <= n <= best_of <= batch"), (dict(best_of=0), "1 <= n <= best_of <= batch"),
    (dict(n=2.0), "1 <= n <= best_of <= batch"), (dict(n=True), "1 <= n <= best_of <= batch"),
    (dict(n=2, seed=(1 << 64) - 1), "seeds"), (dict(n=2, best_of=4, seed=(1 << 64) - 3), "seeds"), (dict(n=2, seed=-(1 << 63) - 1), "seeds"),
    (dict(n=2, seed=1.5), "seeds"),
])
def test_submit_refuses_samples_out_of_range(kw, match):
    from zhilight_amd import ops
    srv = _server()
    with pytest.raises(ops.ZLError, match=match):
        srv.submit(list(range(10)), **kw)
    assert not srv.queue and not srv.requests and not srv.meta


def test_submit_refuses_a_one_token_prompt_on_the_refeed_route():
    from zhilight_amd import ops
    srv = _server()
    for kw in (dict(n=2), dict(best_of=2), dict(sample_first=True)):
        with pytest.raises(ops.ZLError, match="two with a grammar, n > 1 or sample_first"):
            srv.submit([3], **kw)
    with pytest.raises(ops.ZLError, match="does not fit"):
        srv.submit(list(range(33)), n=2)
    with pytest.raises(ops.ZLError, match="does not fit"):
        srv.submit(list(range(32)))
    assert not srv.queue


def test_rank_samples_orders_by_cum_logprob_ties_to_the_lower_index():
    from zhilight_amd.serving import rank_samples
    mk = lambda *lp: dict(logprobs=list(lp), tokens=list(range(len(lp))))                                   # noqa: E731
    samples = [mk(-1.0, -2.0), mk(-0.5), mk(-1.5, -1.5), mk(-0.25, -0.25), mk()]
    ids = {id(s): j for j, s in enumerate(samples)}
    got = rank_samples(samples, 5)                                # best_of == n: by sample index
    assert [ids[id(s)] for s in got] == [0, 1, 2, 3, 4]
    assert [s["cum_logprob"] for s in got] == [-3.0, -0.5, -3.0, -0.5, 0.0]
    assert [ids[id(s)] for s in rank_samples(samples, 3)] == [4, 1, 3]       # -0.5 twice: the lower index first
    assert [ids[id(s)] for s in rank_samples(samples, 4)] == [4, 1, 3, 0]    # -3.0 twice: sample 0, not sample 2
    assert [ids[id(s)] for s in rank_samples(samples, 1)] == [4]
    one = [mk(-0.125, -0.375)]
    assert rank_samples(one, 1) == one and one[0]["cum_logprob"] == -0.5
