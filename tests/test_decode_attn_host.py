"""Host-side checks of the decode attention launchers (attention.hip): which status each entry point returns for which bad argument,
and which one wins when two are bad.  Every case is refused before any device call -- no case here passes a valid argument set, the
pointers are fakes that are never dereferenced.  No GPU needed."""
import ctypes as C

import pytest

ZL_EINVAL, ZL_ESHAPE, ZL_EDTYPE, ZL_ELIMIT = -1, -2, -3, -4
BASE = dict(b=2, len_q=1, h=8, hkv=2, d=128, max_len_buf=1024, dtype=0, algo=0, split_len=128, half_partials=0,
            ws=True, mask=False, valid_lens=True)
MHA = dict(h=8, hkv=8)                              # one query row per kv head: never the matrix-core route of _ex / _quant_ex

# per entry point: its arguments in ABI order.  A lower-case name is a pointer (fake, or null where the case says so),
# i64 / i32 / f32 are scalars taken from the case.  `mask` is the optional one (null in BASE), `maskp` the required one of _splits_h_mask
ABI = {
    "zl_decode_attn": "q buf_lens k_bufs v_bufs mask valid_lens out ws "
                      "i64:b i64:len_q i64:h i64:hkv i64:d f32:scale i64:max_len_buf i32:bshd i32:dtype stream",
    "zl_decode_attn_ex": "q buf_lens k_bufs v_bufs mask valid_lens out ws "
                         "i64:b i64:len_q i64:h i64:hkv i64:d f32:scale i64:max_len_buf i32:bshd i32:dtype i32:algo stream",
    "zl_decode_attn_causal": "q buf_lens k_bufs v_bufs valid_lens out ws "
                             "i64:b i64:len_q i64:h i64:hkv i64:d f32:scale i64:max_len_buf i32:bshd i32:dtype stream",
    "zl_decode_attn_splits": "q buf_lens k_bufs v_bufs valid_lens ws "
                             "i64:b i64:h i64:hkv i64:d f32:scale i64:max_len_buf i32:bshd i32:dtype stream",
    "zl_decode_attn_splits_h": "q buf_lens k_bufs v_bufs valid_lens ws "
                               "i64:b i64:h i64:hkv i64:d f32:scale i64:max_len_buf i32:bshd stream",
    "zl_decode_attn_splits_h_mask": "q buf_lens k_bufs v_bufs maskp ws "
                                    "i64:b i64:h i64:hkv i64:d f32:scale i64:max_len_buf i32:bshd stream",
    "zl_decode_attn_combine_h": "ws buf_lens valid_lens out i64:b i64:h i64:hkv i64:max_len_buf stream",
    "zl_decode_attn_la": "q buf_lens k_bufs v_bufs valid_lens out ws i64:b i64:h i64:hkv i64:d f32:scale i64:max_len_buf "
                         "i32:bshd i32:dtype i64:split_len i32:half_partials stream",
    "zl_decode_attn_fused": "cosv sinv qkv placement buf_lens valid_lens k_bufs v_bufs out ws "
                            "i64:b i64:h i64:hkv i64:d f32:scale i64:max_len_buf i32:neox i32:bshd i32:dtype stream",
    "zl_decode_attn_quant": "q buf_lens k_bufs v_bufs k_scales v_scales mask valid_lens out ws "
                            "i64:b i64:len_q i64:h i64:hkv i64:d f32:scale i64:max_len_buf i32:bshd i32:dtype stream",
    "zl_decode_attn_quant_ex": "q buf_lens k_bufs v_bufs k_scales v_scales mask valid_lens out ws "
                               "i64:b i64:len_q i64:h i64:hkv i64:d f32:scale i64:max_len_buf i32:bshd i32:dtype i32:algo stream",
}
ALL = [n for n in ABI if n not in ("zl_decode_attn", "zl_decode_attn_quant")]     # the two forwarders have cases of their own
EX, QEX, CAUSAL, SPLITS, SPLITS_H, SPLITS_HM, COMBINE_H, LA, FUSED = (
    "zl_decode_attn_ex", "zl_decode_attn_quant_ex", "zl_decode_attn_causal", "zl_decode_attn_splits", "zl_decode_attn_splits_h",
    "zl_decode_attn_splits_h_mask", "zl_decode_attn_combine_h", "zl_decode_attn_la", "zl_decode_attn_fused")
MFMA_ONLY = [SPLITS, SPLITS_H, SPLITS_HM, LA]


def _call(name, **over):
    from zhilight_amd import _lib
    a = dict(BASE, scale=0.1, bshd=1, neox=1, **over)
    fake, null = C.c_void_p(1 << 20), C.c_void_p(0)             # never dereferenced: the checks return first
    args = []
    for spec in ABI[name].split():
        kind, _, key = spec.rpartition(":")
        if kind == "i64":
            args.append(C.c_int64(a[key]))
        elif kind == "i32":
            args.append(C.c_int(a[key]))
        elif kind == "f32":
            args.append(C.c_float(a[key]))
        elif key == "stream":
            args.append(null)
        else:                                                   # a pointer: only these three are ever null
            args.append(fake if a.get(key, True) else null)
    return getattr(_lib.lib(), name)(*args)


CASES = []
for n in ALL:
    CASES += [(n, dict(ws=False), ZL_EINVAL), (n, dict(b=0), ZL_EINVAL)]
    if n != COMBINE_H:
        CASES.append((n, dict(h=8, hkv=3), ZL_ESHAPE))
for n in (EX, QEX):
    CASES.append((n, dict(mask=False, valid_lens=False), ZL_EINVAL))
    CASES.append((n, dict(d=96, **MHA), ZL_ESHAPE))             # falls through to the head-size switch
CASES.append((FUSED, dict(d=96, **MHA), ZL_ESHAPE))
for n in (EX, CAUSAL, SPLITS, LA, FUSED, QEX):
    CASES.append((n, dict(dtype=2), ZL_EDTYPE))
CASES.append((LA, dict(dtype=1, half_partials=1), ZL_EDTYPE))
for n in [CAUSAL] + MFMA_ONLY:
    CASES.append((n, dict(d=64), ZL_ESHAPE))
for n in (EX, FUSED, QEX, CAUSAL):
    CASES.append((n, dict(b=70000, **MHA), ZL_ELIMIT))          # grid limits of these four: ELIMIT ...
for n in MFMA_ONLY:
    CASES.append((n, dict(b=70000), ZL_ESHAPE))                 # ... of these four: ESHAPE (a known inconsistency, pinned as it is)
    CASES.append((n, dict(h=64, hkv=2), ZL_ESHAPE))
CASES += [
    (CAUSAL, dict(len_q=33), ZL_ELIMIT),
    (LA, dict(split_len=100), ZL_EINVAL),
    (LA, dict(split_len=32, max_len_buf=8192), ZL_ELIMIT),      # 256 splits, the last-arriver merge holds 64
    # two violations at once: the order of the checks
    (EX, dict(h=8, hkv=3, dtype=2), ZL_ESHAPE),
    (LA, dict(dtype=2, split_len=100), ZL_EDTYPE),              # _la looks at split_len after its dtype checks
]


@pytest.mark.parametrize("name,over,status", CASES, ids=["%s-%s" % (n[15:], "-".join("%s=%s" % kv for kv in o.items()))
                                                           for n, o, _ in CASES])
def test_launcher_refuses_with_the_status(name, over, status):
    assert _call(name, **over) == status


@pytest.mark.parametrize("fwd,ex", [("zl_decode_attn", EX), ("zl_decode_attn_quant", QEX)])
def test_forwarders_give_the_statuses_of_their_ex_forms(fwd, ex):
    for over, status in ((dict(ws=False), ZL_EINVAL), (dict(h=8, hkv=3), ZL_ESHAPE), (dict(dtype=2), ZL_EDTYPE),
                         (dict(b=70000, **MHA), ZL_ELIMIT)):
        assert _call(fwd, **over) == _call(ex, **over) == status


def test_size_queries_refuse_without_device():
    from zhilight_amd import _lib
    l = _lib.lib()
    i64 = C.c_int64
    assert l.zl_decode_attn_workspace_bytes(i64(0), i64(1), i64(8), i64(128), i64(1024)) == ZL_EINVAL
    assert l.zl_decode_attn_split_len(i64(0), i64(2), i64(1024)) == ZL_EINVAL
    assert l.zl_decode_attn_la_split_len(i64(0), i64(2), i64(1024)) == ZL_EINVAL
    assert l.zl_decode_attn_la_workspace_bytes(i64(2), i64(8), i64(2), i64(1024), i64(100)) == ZL_EINVAL
    assert l.zl_decode_attn_la_workspace_bytes(i64(2), i64(8), i64(2), i64(8192), i64(32)) == ZL_ELIMIT
