"""Host-side checks of the W4A16 matrix-core entry points (w4_mfma.hip): which status each one returns for which bad argument, and
which one wins when two are bad.  Every case is refused before any device call and before any launcher of the family is reached --
no case here is a valid argument set, the pointers are fakes that are never dereferenced.  No GPU needed."""
import ctypes as C

import pytest

ZL_EINVAL, ZL_ESHAPE, ZL_EDTYPE, ZL_ELIMIT = -1, -2, -3, -4
EPI_BIAS, EPI_ADD_C, EPI_RESIDUAL, EPI_SILU_MUL, EPI_SILU_MUL_F32 = 1, 2, 4, 8, 16
BASE = dict(m=1, n=4096, k=4096, ldx=4096, g=128, eps=1e-5, epi=0, bshd=1, h=8, hkv=2, d=128, split_len=128, max_splits=8,
            norm_w=False, opts=False, x_addr=1 << 20)

# per entry point: its arguments in ABI order.  A lower-case name is a pointer (fake, or null where the case says so; norm_w and opts
# are null in BASE), i64 / i32 / f32 are scalars taken from the case
ABI = {
    "zl_w4a16_gemm_mfma": "x i64:ldx qw meta bias residual y i64:m i64:n i64:k i64:g norm_w f32:eps i32:epi stream",
    "zl_w4a16_gemm_mfma_ex": "x i64:ldx qw meta bias residual y i64:m i64:n i64:k i64:g norm_w f32:eps i32:epi opts stream",
    "zl_w4a16_qkv_rope_scatter": "x i64:ldx qw meta bias norm_w f32:eps cosv sinv placement buf_lens k_bufs v_bufs q_out "
                                 "i64:m i64:h i64:hkv i64:d i64:k i64:g i32:bshd stream",
    "zl_w4a16_qkv_rope_scatter_ex": "x i64:ldx qw meta bias norm_w f32:eps cosv sinv placement buf_lens k_bufs v_bufs q_out "
                                    "i64:m i64:h i64:hkv i64:d i64:k i64:g i32:bshd opts stream",
    "zl_w4a16_gemm_attn_merge": "ws buf_lens valid_lens i64:split_len i64:max_splits qw meta bias residual y "
                                "i64:m i64:n i64:k i64:g i32:epi stream",
    "zl_w4a16_gemm_attn_merge_h": "ws buf_lens valid_lens i64:split_len i64:max_splits qw meta bias residual y "
                                  "i64:m i64:n i64:k i64:g i32:epi stream",
    "zl_w4a16_gemm_attn_merge_h_ex": "ws buf_lens valid_lens i64:split_len i64:max_splits qw meta bias residual y "
                                     "i64:m i64:n i64:k i64:g i32:epi opts stream",
}
GEMM, ROPE, MERGE, MERGE_H = ("zl_w4a16_gemm_mfma_ex", "zl_w4a16_qkv_rope_scatter_ex", "zl_w4a16_gemm_attn_merge",
                              "zl_w4a16_gemm_attn_merge_h_ex")


def _call(name, **over):
    from zhilight_amd import _lib
    a = dict(BASE, **over)
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
        elif key == "x":
            args.append(C.c_void_p(a["x_addr"]) if a.get("x", True) else null)
        else:
            args.append(fake if a.get(key, True) else null)
    return getattr(_lib.lib(), name)(*args)


def _layout(n, k, g, out=True):
    from zhilight_amd import _lib
    L = _lib.W4Layout()
    return _lib.lib().zl_w4m_layout(C.c_int64(n), C.c_int64(k), C.c_int64(g), C.byref(L) if out else C.c_void_p(0))


# (n, k, group_size), the status
LAYOUT_CASES = [
    ((0, 4096, 128), ZL_EINVAL), ((4096, 0, 128), ZL_EINVAL), ((4096, 4096, 0), ZL_EINVAL), ((-16, 4096, 128), ZL_EINVAL),
    ((4096, 4100, 128), ZL_ESHAPE),                             # K % 8
    ((4096, 4096, 64), ZL_ESHAPE), ((4096, 4096, 192), ZL_ESHAPE),   # the group is a multiple of the 128-k tile ...
    ((4096, 384, 256), ZL_ESHAPE),                              # ... and divides K
    ((0, 4096, 64), ZL_EINVAL),                                 # two at once: the sizes come first
]


@pytest.mark.parametrize("nkg,status", LAYOUT_CASES, ids=["n=%d-k=%d-g=%d" % c for c, _ in LAYOUT_CASES])
def test_layout_refuses_with_the_status(nkg, status):
    assert _layout(*nkg) == status


def test_layout_refuses_a_null_result():
    assert _layout(4096, 4096, 128, out=False) == ZL_EINVAL


BIG = dict(h=448, hkv=32, d=128, k=131072, ldx=131072)         # n = 65536 columns x K = 131072: 4 GiB of packed weights
CASES = []
# ---- zl_w4a16_gemm_mfma_ex: what is refused before the first route is asked, and the normalising launch of 9..32 rows
CASES += [(GEMM, {p: False}, ZL_EINVAL) for p in ("x", "qw", "meta", "y")]
CASES += [(GEMM, {s: 0}, ZL_EINVAL) for s in ("m", "n", "k")]
CASES += [
    (GEMM, dict(ldx=4088), ZL_ESHAPE), (GEMM, dict(ldx=4100), ZL_ESHAPE), (GEMM, dict(x_addr=(1 << 20) + 8), ZL_ESHAPE),
    (GEMM, dict(epi=EPI_RESIDUAL, residual=False), ZL_EINVAL),
    (GEMM, dict(g=64), ZL_ESHAPE), (GEMM, dict(g=0), ZL_EINVAL), (GEMM, dict(k=4100, ldx=4104), ZL_ESHAPE),
    (GEMM, dict(n=4095, epi=EPI_SILU_MUL), ZL_ESHAPE), (GEMM, dict(n=4095, epi=EPI_SILU_MUL_F32), ZL_ESHAPE),
    (GEMM, dict(m=9, norm_w=True), ZL_ESHAPE), (GEMM, dict(m=32, norm_w=True), ZL_ESHAPE),   # the deferred norm: on request only
    # two at once: the order of the checks
    (GEMM, dict(x=False, ldx=4088), ZL_EINVAL),
    (GEMM, dict(ldx=4088, epi=EPI_RESIDUAL, residual=False), ZL_ESHAPE),
    (GEMM, dict(epi=EPI_RESIDUAL, residual=False, g=64), ZL_EINVAL),
    (GEMM, dict(g=0, n=4095, epi=EPI_SILU_MUL), ZL_EINVAL),
]
# ---- zl_w4a16_qkv_rope_scatter_ex without options (the slab route is not asked)
CASES += [(ROPE, {p: False}, ZL_EINVAL) for p in ("x", "qw", "meta", "cosv", "sinv", "placement", "buf_lens", "k_bufs", "v_bufs", "q_out")]
CASES += [(ROPE, {s: 0}, ZL_EINVAL) for s in ("m", "h", "hkv", "d", "k")]
CASES += [
    (ROPE, dict(ldx=4088), ZL_ESHAPE), (ROPE, dict(ldx=4100), ZL_ESHAPE), (ROPE, dict(x_addr=(1 << 20) + 8), ZL_ESHAPE),
    (ROPE, dict(g=64), ZL_ESHAPE), (ROPE, dict(g=0), ZL_EINVAL),
    (ROPE, dict(m=33), ZL_ESHAPE), (ROPE, dict(d=48), ZL_ESHAPE),
    (ROPE, dict(m=17, k=8320, ldx=8320), ZL_ESHAPE),            # more than 16 rows: K <= 8192
    (ROPE, BIG, ZL_ELIMIT),
    (ROPE, dict(norm_w=True, m=4, k=8192, ldx=8192), ZL_ESHAPE),   # fused norm up to 8 rows: K <= 4096
    (ROPE, dict(norm_w=True, m=9), ZL_ESHAPE),                  # 9..32 rows: the deferred norm, on request only
    (ROPE, dict(cosv=False, m=0), ZL_EINVAL),
    (ROPE, dict(m=0, ldx=4088), ZL_EINVAL),
    (ROPE, dict(ldx=4088, g=0), ZL_ESHAPE),
    (ROPE, dict(m=33, **BIG), ZL_ESHAPE),                       # the shape is looked at before the size of the weights
    (ROPE, dict(norm_w=True, m=4, **BIG), ZL_ELIMIT),           # ... and that before the norm's own limits
]
# ---- the two attention-merge projections
for n in (MERGE, MERGE_H):
    CASES += [(n, {p: False}, ZL_EINVAL) for p in ("ws", "buf_lens", "valid_lens", "qw", "meta", "y")]
    CASES += [(n, {s: 0}, ZL_EINVAL) for s in ("m", "n", "k", "split_len", "max_splits")]
    CASES += [
        (n, dict(epi=EPI_BIAS, bias=False), ZL_EINVAL),
        (n, dict(epi=EPI_RESIDUAL, residual=False), ZL_EINVAL), (n, dict(epi=EPI_ADD_C, residual=False), ZL_EINVAL),
        (n, dict(m=5), ZL_ESHAPE), (n, dict(k=8192), ZL_ESHAPE), (n, dict(k=4000), ZL_ESHAPE), (n, dict(max_splits=17), ZL_ESHAPE),
        (n, dict(epi=EPI_SILU_MUL), ZL_ESHAPE), (n, dict(epi=EPI_SILU_MUL_F32), ZL_ESHAPE),
        (n, dict(g=64), ZL_ESHAPE), (n, dict(g=0), ZL_EINVAL),
        (n, dict(n=1 << 21), ZL_ELIMIT),                        # 2^21 columns x K = 4096: 4 GiB of packed weights
        (n, dict(m=5, epi=EPI_BIAS, bias=False), ZL_EINVAL),
        (n, dict(m=5, epi=EPI_SILU_MUL), ZL_ESHAPE),
        (n, dict(epi=EPI_SILU_MUL, g=0), ZL_ESHAPE),             # the epilogue is looked at before the layout
        (n, dict(m=5, n=1 << 21), ZL_ESHAPE),
    ]


@pytest.mark.parametrize("name,over,status", CASES, ids=["%s-%s" % (n[9:], "-".join("%s=%s" % kv for kv in o.items()))
                                                           for n, o, _ in CASES])
def test_entry_point_refuses_with_the_status(name, over, status):
    assert _call(name, **over) == status


@pytest.mark.parametrize("fwd,ex,cases", [
    ("zl_w4a16_gemm_mfma", GEMM, ((dict(y=False), ZL_EINVAL), (dict(ldx=4088), ZL_ESHAPE), (dict(m=9, norm_w=True), ZL_ESHAPE))),
    ("zl_w4a16_qkv_rope_scatter", ROPE, ((dict(q_out=False), ZL_EINVAL), (dict(m=33), ZL_ESHAPE), (BIG, ZL_ELIMIT))),
    ("zl_w4a16_gemm_attn_merge_h", MERGE_H, ((dict(ws=False), ZL_EINVAL), (dict(m=5), ZL_ESHAPE), (dict(n=1 << 21), ZL_ELIMIT))),
])
def test_forwarders_give_the_statuses_of_their_ex_forms(fwd, ex, cases):
    for over, status in cases:
        assert _call(fwd, **over) == _call(ex, **over) == status
