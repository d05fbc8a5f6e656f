"""The window / sink attention entry points without a GPU: their argument checks return before any device call (fake pointers, the
call form of test_decode_attn_host.py), their names are in _lib.SYMBOLS, and the ops wrappers refuse head sizes other than 64."""
import ctypes as C

import pytest
import torch

FAKE, NULL, I64 = C.c_void_p(1 << 20), C.c_void_p(0), C.c_int64
TAIL = lambda dt, window: (C.c_int(1), C.c_int(dt), I64(window), NULL, NULL)      # bshd, dtype, window, sinks, stream
CALLS = {
    "zl_decode_attn_window": lambda f, q, hkv, dt, w: f(q, *[FAKE] * 6, I64(4), I64(1), I64(8), I64(hkv), C.c_float(0.125), I64(1088), *TAIL(dt, w)),
    "zl_prefill_attn_d64_window": lambda f, q, hkv, dt, w: f(q, *[FAKE] * 3, I64(10), I64(5), I64(8), I64(hkv), C.c_float(0.125), I64(64), *TAIL(dt, w)),
    "zl_prefill_attn_d64_varlen_window": lambda f, q, hkv, dt, w: f(q, *[FAKE] * 7, I64(10), I64(5), I64(393), I64(8), I64(hkv), C.c_float(0.125),
                                                                   *TAIL(dt, w)),
}


@pytest.mark.parametrize("name", CALLS)
def test_argument_checks(name):
    from zhilight_amd import _lib
    assert name in _lib.SYMBOLS
    call = lambda q=FAKE, hkv=2, dt=0, w=128: CALLS[name](getattr(_lib.lib(), name), q, hkv, dt, w)
    assert (call(q=NULL), call(hkv=3), call(dt=2), call(w=-1)) == (-1, -2, -3, -1)


def test_wrappers_refuse_head_size_128():
    from zhilight_amd import ops
    q, t = torch.zeros(2, 1, 8, 128, dtype=torch.float16), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ops.ZLError, match="head size 64"):
        ops.multi_query_attention_rag_buffer(q, t.int(), t, t, None, 0.1, 64, 2, valid_lens=t.int(), window=16)
    with pytest.raises(ops.ZLError, match="head size 64"):
        ops.prefill_attention(q[0], q[0], q[0], 0, 8, 0.1, sinks=torch.zeros(8))
    with pytest.raises(ops.ZLError, match="head size 64"):
        ops.prefill_attention_varlen(q[:, 0], [1, 1], [0, 0], t, t, [64, 64], 2, 0.1, window=16)
