"""The prompt prefix cache on the device.

Kernel: zl_kv_blocks_copy (ops.kv_blocks_copy) against a numpy model of the copy over the WHOLE buffers and the WHOLE pool, both
pre-filled with distinct random bytes: every byte outside the copied slices must be unchanged.  Both directions, both layouts,
16-bit rows, u8 code rows, the fp32 scale plane and 8-byte slices that only the dword path can move.

Model: LLaMA.prefill_cached on the two-layer GPTQ geometry of test_gpu_prefill_batch against the same continuation without the cache
-- a task whose prefix rows are filled by a torch slice copy and continued with prefill_batch(pos0=...) -- bit for bit: logits, K/V
rows, context fields and three greedy steps.  That bar rests on the prompt kernels giving the same bits for the same inputs at the
same shape, as the bit-identity tests of prefill_batch assume."""
import numpy as np
import pytest
import torch

from test_gpu_model import _ThreadTP, _hf_state

pytestmark = pytest.mark.gpu

LAYERS, LEN_BUFS, NUM_BLOCKS = 2, (48, 64, 80), 6


# ---- the copy launch ---------------------------------------------------------------------------------------------------------
def _descs(block):
    """five descriptors: a block ending exactly at len_buf (twice), pool ids 0 and NUM_BLOCKS - 1, two blocks of task 2, and a first
    slot (33) that is no multiple of anything"""
    return [(0, LEN_BUFS[0] - block, 0), (1, 0, NUM_BLOCKS - 1), (2, block, 2), (2, LEN_BUFS[2] - block, 3), (1, 33, 1)]


def _setup(dev, rng, block, hkv, row_bytes, bshd):
    bufs = [rng.integers(0, 256, (LAYERS, 2, n, hkv, row_bytes) if bshd else (LAYERS, 2, hkv, n, row_bytes), dtype=np.uint8)
            for n in LEN_BUFS]
    pool = rng.integers(0, 256, (NUM_BLOCKS, LAYERS, 2, block, hkv, row_bytes) if bshd else (NUM_BLOCKS, LAYERS, 2, hkv, block, row_bytes),
                        dtype=np.uint8)
    d_bufs = [torch.from_numpy(b).to(dev) for b in bufs]
    tables = [torch.tensor([[t[l, kv].data_ptr() for t in d_bufs] for l in range(LAYERS)], dtype=torch.int64, device=dev) for kv in (0, 1)]
    buf_lens = torch.tensor(LEN_BUFS, dtype=torch.int32, device=dev)
    return bufs, pool, d_bufs, torch.from_numpy(pool).to(dev), tables, buf_lens


def _model_copy(bufs, pool, descs, block, bshd, to_pool):
    bufs, pool = [b.copy() for b in bufs], pool.copy()
    for task, slot, pb in descs:
        rows = bufs[task][:, :, slot:slot + block] if bshd else bufs[task][:, :, :, slot:slot + block]
        if to_pool:
            pool[pb] = rows
        else:
            rows[...] = pool[pb]
    return bufs, pool


@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("block,hkv,row_bytes", [(16, 2, 256), (16, 2, 128), (16, 2, 4), (2, 1, 4)])
def test_kv_blocks_copy_is_exact_over_whole_buffers_and_pool(dev, block, hkv, row_bytes, bshd):
    from zhilight_amd import ops
    rng = np.random.default_rng(block * 1000 + row_bytes + hkv)
    descs = _descs(block)
    for to_pool in (True, False):
        bufs, pool, d_bufs, d_pool, (k_tab, v_tab), buf_lens = _setup(dev, rng, block, hkv, row_bytes, bshd)
        ops.kv_blocks_copy(descs, k_tab, v_tab, buf_lens, d_pool, block, hkv, row_bytes, to_pool, bshd=bshd)
        want_bufs, want_pool = _model_copy(bufs, pool, descs, block, bshd, to_pool)
        assert np.array_equal(d_pool.cpu().numpy(), want_pool), ("pool", to_pool)
        assert (want_pool != pool).any() == to_pool
        for t in range(3):
            assert np.array_equal(d_bufs[t].cpu().numpy(), want_bufs[t]), ("buffer", t, to_pool)
        # the host's buffer lengths instead of a read-back, and another piece size: the same bytes
        bufs2, pool2, d_bufs2, d_pool2, (k2, v2), lens2 = _setup(dev, np.random.default_rng(7), block, hkv, row_bytes, bshd)
        ops.kv_blocks_copy(descs, k2, v2, lens2, d_pool2, block, hkv, row_bytes, to_pool, bshd=bshd, buf_lens_host=LEN_BUFS, piece_bytes=48)
        want_bufs2, want_pool2 = _model_copy(bufs2, pool2, descs, block, bshd, to_pool)
        assert np.array_equal(d_pool2.cpu().numpy(), want_pool2)
        assert all(np.array_equal(d_bufs2[t].cpu().numpy(), want_bufs2[t]) for t in range(3))


@pytest.mark.parametrize("bshd", [True, False])
def test_save_then_load_into_another_task_reproduces_the_rows(dev, bshd):
    from zhilight_amd import ops
    block, hkv, rb = 16, 2, 256
    bufs, pool, d_bufs, d_pool, (k_tab, v_tab), buf_lens = _setup(dev, np.random.default_rng(11), block, hkv, rb, bshd)
    ops.kv_blocks_copy([(0, 16, 4), (0, 32, 1)], k_tab, v_tab, buf_lens, d_pool, block, hkv, rb, True, bshd=bshd)
    # one launch loads pool block 4 into two tasks (two prompts that share a prefix)
    ops.kv_blocks_copy([(2, 64, 4), (1, 0, 1), (1, 32, 4)], k_tab, v_tab, buf_lens, d_pool, block, hkv, rb, False, bshd=bshd)
    rows = (lambda t, a: t[:, :, a:a + block]) if bshd else (lambda t, a: t[:, :, :, a:a + block])
    assert np.array_equal(rows(d_bufs[2].cpu().numpy(), 64), rows(bufs[0], 16))
    assert np.array_equal(rows(d_bufs[1].cpu().numpy(), 32), rows(bufs[0], 16))
    assert np.array_equal(rows(d_bufs[1].cpu().numpy(), 0), rows(bufs[0], 32))
    assert np.array_equal(d_bufs[0].cpu().numpy(), bufs[0])


def test_kv_blocks_copy_accepts_nothing_and_refuses_bad_descriptors(dev):
    from zhilight_amd import ops
    block, hkv, rb = 16, 2, 128
    bufs, pool, d_bufs, d_pool, (k_tab, v_tab), buf_lens = _setup(dev, np.random.default_rng(13), block, hkv, rb, True)
    args = (k_tab, v_tab, buf_lens, d_pool, block, hkv, rb)
    for to_pool in (True, False):
        assert ops.kv_blocks_copy([], *args, to_pool) is None                       # n == 0
    for descs in ([(0, 33, 0)],                                                     # rows 33 .. 48 of a 48-row buffer
                  [(1, 0, 0), (0, -1, 1)],
                  [(3, 0, 0)],                                                      # no such task
                  [(1, 0, NUM_BLOCKS)], [(1, 0, -1)]):                              # pool block out of range
        for to_pool in (True, False):
            with pytest.raises(ops.ZLError):
                ops.kv_blocks_copy(descs, *args, to_pool)
    # a destination twice in one call: a pool block when saving, rows of a task when loading (one block MAY be loaded into two tasks)
    with pytest.raises(ops.ZLError):
        ops.kv_blocks_copy([(1, 0, 2), (2, 0, 2)], *args, True)
    with pytest.raises(ops.ZLError):
        ops.kv_blocks_copy([(1, 0, 2), (1, 15, 3)], *args, False)
    with pytest.raises(ops.ZLError):
        ops.kv_blocks_copy([(1, 0, 0)], k_tab, v_tab, buf_lens, d_pool, block, hkv, 126, True)      # row_bytes % 4
    with pytest.raises(ops.ZLError):
        ops.kv_blocks_copy([(1, 0, 0)], k_tab, v_tab, buf_lens, d_pool[:, :1], block, hkv, rb, True)  # not the pool's shape
    torch.cuda.synchronize()
    assert np.array_equal(d_pool.cpu().numpy(), pool)
    assert all(np.array_equal(d_bufs[t].cpu().numpy(), bufs[t]) for t in range(3))


# ---- LLaMA.prefill_cached ----------------------------------------------------------------------------------------------------
BS, LEN_BUF = 16, 64


@pytest.fixture(scope="module")
def gptq(dev):
    """the two-layer GPTQ model of test_gpu_prefill_batch._gptq_model"""
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    rng = np.random.default_rng(3)
    cfg = ModelConfig(num_layers=2, dim_model=1024, num_heads=8, dim_head=128, dim_ff=2048, vocab_size=512, num_kv_heads=2, eps=1e-5,
                      rope_theta=5e5, rope_scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                                    "original_max_position_embeddings": 8192})
    sd = {k: torch.from_numpy(v) for k, v in _hf_state(rng, cfg, 128).items()}
    return cfg, sd, LLaMA(cfg, QuantConfig(5, 128), dev).load_state_dict(sd)


def _prompt(seed, n, vocab=512):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, vocab, n).astype(np.int32))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _planes(ctx, task):
    return [ctx.kv[task]] + ([ctx.kv_scales[task]] if ctx.kv_quant else [])


def _copy_rows(dst, dst_task, src, src_task, rows):
    """the control's prefix: a torch slice copy of rows 0 .. rows - 1, every layer, K and V (codes and scales on an INT8 cache)"""
    for d, s in zip(_planes(dst, dst_task), _planes(src, src_task)):
        d[:, :, :rows].copy_(s[:, :, :rows])


def _assert_same_task(a, b, task, lo, hi, what):
    for pa, pb in zip(_planes(a, task), _planes(b, task)):
        assert _same(pa[:, :, lo:hi], pb[:, :, lo:hi]), (what, task, "K/V rows", lo, hi)
    for f in ("tokens", "positions", "placement", "valid_lens"):
        assert int(getattr(a, f)[task]) == int(getattr(b, f)[task]), (what, task, f)


def _assert_same_steps(model, a, b, what, steps=3):
    assert a.steps_left == b.steps_left, what
    for step in range(steps):
        la, ta = model.step_greedy(a)
        lb, tb = model.step_greedy(b)
        assert torch.equal(ta, tb), (what, step)
        assert _same(la, lb), (what, step)


def _hit_against_control(model, ctx_kw, kv_history):
    """(i), (ii), (iii) for one kind of context -> the cache and the context, for more"""
    p = _prompt(50, 50)
    ctx = model.new_context(3, LEN_BUF, 0, **ctx_kw)
    cache = model.new_prefix_cache(ctx, 8, block_size=BS)
    kw = dict(kv_history=kv_history) if kv_history else {}
    # (i) a miss is prefill_batch
    logits0, matched = model.prefill_cached(ctx, cache, [0], [p], **kw)
    assert matched == [0]
    ctl = model.new_context(3, LEN_BUF, 0, **ctx_kw)
    ref0 = model.prefill_batch(ctl, [0], [p], **kw)
    assert _same(logits0, ref0)
    _assert_same_task(ctx, ctl, 0, 0, 50, "miss")
    planes = 2 if ctx.kv_quant else 1
    assert (cache.load_launches, cache.save_launches) == (0, planes)
    assert len(cache.index) == 3 and cache.index.counters() == dict(lookups=1, hits=0, tokens_matched=0, blocks_saved=3, evictions=0)
    # (ii) the same prompt again: 48 tokens from the cache, ONE load launch per plane, nothing new to save
    logits1, matched = model.prefill_cached(ctx, cache, [1], [p], **kw)
    assert matched == [48]
    assert (cache.load_launches, cache.save_launches) == (planes, planes)
    for pa, pb in zip(_planes(ctx, 1), _planes(ctx, 0)):
        assert _same(pa[:, :, :48], pb[:, :, :48])
    assert cache.index.counters() == dict(lookups=2, hits=1, tokens_matched=48, blocks_saved=3, evictions=0)
    # (iii) the control: rows 0 .. 47 by a slice copy, the rest by prefill_batch(pos0=[48])
    _copy_rows(ctl, 1, ctl, 0, 48)
    ref1 = model.prefill_batch(ctl, [1], [p[48:]], pos0=[48], **kw)
    assert _same(logits1, ref1)
    _assert_same_task(ctx, ctl, 1, 0, 50, "hit")
    _assert_same_steps(model, ctx, ctl, "hit")
    return cache, ctx


def test_prefill_cached_miss_hit_and_control_fp16(dev, gptq):
    _, _, model = gptq
    cache, _ = _hit_against_control(model, {}, None)
    assert cache.pool.dtype == torch.float16 and cache.pool_scales is None
    assert tuple(cache.pool.shape) == (8, 2, 2, BS, 2, 128)


def test_prefill_cached_int8_cache_codes_and_scales(dev, gptq):
    from zhilight_amd import ops
    _, _, model = gptq
    p = _prompt(50, 50)
    ctx = model.new_context(3, LEN_BUF, 0, kv_cache_dtype="int8")
    cache = model.new_prefix_cache(ctx, 8, block_size=BS)
    assert cache.pool.dtype == torch.uint8 and cache.pool_scales.dtype == torch.float32
    before = (cache.index.state(), [t.clone() for t in ctx.kv + ctx.kv_scales], ctx.positions.tolist(), ctx.tokens.tolist())
    with pytest.raises(ops.ZLError):                                 # without the keyword, whether or not anything would match
        model.prefill_cached(ctx, cache, [0], [p])
    assert cache.index.state() == before[0] and (ctx.positions.tolist(), ctx.tokens.tolist()) == before[2:]
    assert all(_same(a, b) for a, b in zip(ctx.kv + ctx.kv_scales, before[1]))
    assert (cache.load_launches, cache.save_launches) == (0, 0)
    cache, _ = _hit_against_control(model, dict(kv_cache_dtype="int8"), "cache")
    assert (cache.load_launches, cache.save_launches) == (2, 2)


def test_prefill_cached_three_tasks_full_hit_partial_hit_and_miss(dev, gptq):
    _, _, model = gptq
    p = _prompt(50, 50)
    q = torch.cat([p[:32], _prompt(51, 20)])                          # shares the first two blocks only
    r = _prompt(52, 30)
    assert not torch.equal(q[32:48], p[32:48])
    seed = model.new_context(1, LEN_BUF, 0)
    cache = model.new_prefix_cache(seed, 8, block_size=BS)
    model.prefill_cached(seed, cache, [0], [p])
    ctx, ctl = model.new_context(3, LEN_BUF, 0), model.new_context(3, LEN_BUF, 0)
    logits, matched = model.prefill_cached(ctx, cache, [0, 1, 2], [p, q, r])
    assert matched == [48, 32, 0]
    assert (cache.load_launches, cache.save_launches) == (1, 2)       # five blocks in ONE load launch; one save launch per call
    _copy_rows(ctl, 0, seed, 0, 48)
    _copy_rows(ctl, 1, seed, 0, 32)
    ref = model.prefill_batch(ctl, [0, 1, 2], [p[48:], q[32:], r], pos0=[48, 32, 0])
    assert _same(logits, ref)
    for task, n in enumerate((50, 52, 30)):
        _assert_same_task(ctx, ctl, task, 0, n, "three tasks")
    _assert_same_steps(model, ctx, ctl, "three tasks")
    # q's third block (behind p's first two) and r's one full block are new
    assert cache.index.counters() == dict(lookups=4, hits=2, tokens_matched=80, blocks_saved=5, evictions=0)
    # two tasks of one call with a common uncached prefix: its blocks are saved once, from the first
    u = _prompt(53, 40)
    ctx2 = model.new_context(3, LEN_BUF, 0)
    _, matched = model.prefill_cached(ctx2, cache, [2, 0], [u, torch.cat([u[:32], _prompt(54, 20)])])
    assert matched == [0, 0] and cache.index.blocks_saved == 5 + 2 + 1
    ids = cache.index.match(u)
    assert len(ids) == 2 and all(_same(cache.pool[b], ctx2.kv[2][:, :, i * BS:(i + 1) * BS]) for i, b in enumerate(ids))


def test_prefill_cached_block_identity_is_the_whole_prefix(dev, gptq):
    """prompts [X, Y, t] and [Z, Y, t]: the second never receives the first one's block for Y"""
    _, _, model = gptq
    x, y, z, t = _prompt(60, BS), _prompt(61, BS), _prompt(62, BS), _prompt(63, 3)
    ctx = model.new_context(3, LEN_BUF, 0)
    cache = model.new_prefix_cache(ctx, 8, block_size=BS)
    _, m0 = model.prefill_cached(ctx, cache, [0], [torch.cat([x, y, t])])
    _, m1 = model.prefill_cached(ctx, cache, [1], [torch.cat([z, y, t])])
    assert m0 == [0] and m1 == [0]                                    # Y behind Z is not Y behind X
    _, m2 = model.prefill_cached(ctx, cache, [2], [torch.cat([z, y, t])])
    assert m2 == [32]
    own, other = ctx.kv[1][:, :, BS:2 * BS], ctx.kv[0][:, :, BS:2 * BS]
    assert not _same(own[1], other[1])                                # layer 1's rows for Y depend on what came before
    assert _same(ctx.kv[2][:, :, :2 * BS], ctx.kv[1][:, :, :2 * BS])
    assert len(cache.index) == 4


def test_prefill_cached_pool_smaller_than_the_prompts(dev, gptq):
    _, _, model = gptq
    len_buf = 128
    a, b = _prompt(70, 85), _prompt(71, 85)                           # five full blocks each, a pool of three
    ctx, ctl = model.new_context(2, len_buf, 0), model.new_context(2, len_buf, 0)
    cache = model.new_prefix_cache(ctx, 3, block_size=BS)
    la, ma = model.prefill_cached(ctx, cache, [0], [a])
    assert ma == [0] and _same(la, model.prefill_batch(ctl, [0], [a]))
    assert len(cache.index) == 3 and cache.index.evictions == 0       # a prompt's own chain is never evicted for its tail
    lb, mb = model.prefill_cached(ctx, cache, [1], [b])
    assert mb == [0] and _same(lb, model.prefill_batch(ctl, [1], [b]))
    assert len(cache.index) == 3 and cache.index.evictions == 3
    _assert_same_task(ctx, ctl, 0, 0, 85, "small pool")
    _assert_same_task(ctx, ctl, 1, 0, 85, "small pool")
    ctx2 = model.new_context(2, len_buf, 0)
    l2, m2 = model.prefill_cached(ctx2, cache, [0], [b])
    assert m2 == [48]
    _copy_rows(ctl, 0, ctl, 1, 48)
    assert _same(l2, model.prefill_batch(ctl, [0], [b[48:]], pos0=[48]))


def test_prefill_cached_refusals_leave_index_and_context_alone(dev, gptq):
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, QuantConfig
    from zhilight_amd.prefix_cache import PrefixCache
    cfg, sd, model = gptq
    p = _prompt(50, 50)
    ctx = model.new_context(3, LEN_BUF, 0)
    cache = model.new_prefix_cache(ctx, 8, block_size=BS)
    model.prefill_cached(ctx, cache, [0], [p])
    state = cache.index.state()
    snap = ([t.clone() for t in ctx.kv], ctx.positions.tolist(), ctx.tokens.tolist(), cache.pool.clone())
    other_geometry = PrefixCache(dev, cfg.num_layers + 1, cfg.num_kv_heads, cfg.dim_head, cfg.torch_dtype, False, 8, BS)
    other_heads = PrefixCache(dev, cfg.num_layers, cfg.num_kv_heads * 2, cfg.dim_head, cfg.torch_dtype, False, 8, BS)
    int8_cache = model.new_prefix_cache(model.new_context(1, LEN_BUF, 0, kv_cache_dtype="int8"), 8, block_size=BS)
    for c in (other_geometry, other_heads, int8_cache):
        s = c.index.state()
        with pytest.raises(ops.ZLError):
            model.prefill_cached(ctx, c, [1], [p])
        assert c.index.state() == s and (c.load_launches, c.save_launches) == (0, 0)
    for tasks, prompts in (([1], [_prompt(1, LEN_BUF)]),               # does not fit the buffer
                           ([1, 1], [p, p]), ([3], [p]), ([1], [p[:0]]), ([1, 2], [p])):
        with pytest.raises(ops.ZLError):
            model.prefill_cached(ctx, cache, tasks, prompts)
    with pytest.raises(ops.ZLError):
        model.prefill_cached(ctx, cache, [1], [p], kv_history="rows")
    tp_model = LLaMA(cfg, QuantConfig(5, 128), dev, tp=_ThreadTP(2).view(0)).load_state_dict(sd)
    with pytest.raises(ops.ZLError, match="tensor parallelism is not supported"):
        tp_model.prefill_cached(tp_model.new_context(3, LEN_BUF, 0), cache, [1], [p])
    assert cache.index.state() == state and (cache.load_launches, cache.save_launches) == (0, 1)
    assert (ctx.positions.tolist(), ctx.tokens.tolist()) == snap[1:3] and _same(cache.pool, snap[3])
    assert all(_same(a, b) for a, b in zip(ctx.kv, snap[0]))
