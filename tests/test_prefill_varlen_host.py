"""Host-side checks of the varlen prompt attention (zl_prefill_attn_varlen): argument checks return before any device call, and the
work planner lists every (task, query tile) once, longest first.  No GPU needed."""
import ctypes as C

import pytest

LENS = [1, 63, 64, 65, 200]
POS0 = [0, 0, 37, 0, 100]
ZL_EINVAL, ZL_ESHAPE, ZL_EDTYPE = -1, -2, -3


def _call(d=128, h=8, hkv=2, b=5, dtype=0, work=True, groups=0):
    from zhilight_amd import _lib
    fake = C.c_void_p(1 << 20)                      # never dereferenced: the checks return first
    return _lib.lib().zl_prefill_attn_varlen(fake, fake, fake, fake, fake, fake, fake, fake if work else C.c_void_p(0),
                                             C.c_int64(10), C.c_int64(b), C.c_int64(393), C.c_int64(h), C.c_int64(hkv),
                                             C.c_int64(d), C.c_float(0.1), C.c_int(1), C.c_int(dtype), C.c_int(groups),
                                             C.c_void_p(0))


def test_varlen_argument_checks_without_device():
    assert _call(d=64) == ZL_ESHAPE
    assert _call(h=8, hkv=3) == ZL_ESHAPE
    assert _call(work=False) == ZL_EINVAL
    assert _call(b=0) == ZL_EINVAL
    assert _call(dtype=2) == ZL_EDTYPE
    assert _call(groups=3) == ZL_EINVAL


def _key_tiles(t, qt):
    return (POS0[t] + min((qt + 1) * 64, LENS[t]) + 63) // 64


def test_work_planner_lists_every_tile_once_longest_first():
    from zhilight_amd import ops
    items = ops.prefill_work_items(LENS, POS0)
    expect = {(t, qt) for t, s in enumerate(LENS) for qt in range((s + 63) // 64)}
    assert len(items) == len(expect) and set(items) == expect
    cost = [_key_tiles(t, qt) for t, qt in items]
    assert cost == sorted(cost, reverse=True)
    assert items[0] == (4, 3)                        # 100 + 200 keys: 5 key tiles
    # one task: the order of the one-task launch's own map (query tiles descending)
    assert ops.prefill_work_items([200], [0]) == [(0, 3), (0, 2), (0, 1), (0, 0)]


def test_varlen_plan_tables_and_refusals():
    import torch
    from zhilight_amd import ops
    plan = ops.prefill_varlen_plan(LENS, POS0, [320] * 5, "cpu")
    assert plan.b == 5 and plan.total_q == sum(LENS) and plan.n_work == len(plan.work_items)
    assert plan.cu_seqlens_q.tolist() == [0, 1, 64, 128, 193, 393]
    assert plan.pos0_dev.tolist() == POS0 and plan.buf_lens_dev.tolist() == [320] * 5
    assert plan.work.view(-1, 2).tolist() == [list(w) for w in plan.work_items]
    assert plan.tables.dtype == torch.int32
    with pytest.raises(ops.ZLError):
        ops.prefill_varlen_plan(LENS, POS0, [299] * 5, "cpu")          # task 4 needs 300 rows
    with pytest.raises(ops.ZLError):
        ops.prefill_varlen_plan([0, 5], [0, 0], [64, 64], "cpu")
    with pytest.raises(ops.ZLError):
        ops.prefill_varlen_plan([5], [0, 0], [64], "cpu")
