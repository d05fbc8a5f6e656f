"""Host-side checks of the fused lm_head scoring (zl_lm_head_score, ops.lm_head_score, LLaMA.score): workspace arithmetic, argument
refusals that return before any launch, the label builder, and the error bound B(N) of the kernel's log-sum-exp derived from a numpy
restatement of its reduction in the worst (sequential) order.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

ZL_EINVAL, ZL_ESHAPE, ZL_EDTYPE = -1, -2, -3


def bound(n, bn=128):
    """B(N): one fp32 rounding per addition in the longest chain of a block sum (bn) plus of the merge over ceil(N / bn) blocks,
    relative to a sum >= 1, plus one rounding of the exponent's scaled argument over the fp32 exp range"""
    return (bn + -(-n // bn)) * 2.0 ** -24 + 88 * 2.0 ** -23


def test_workspace_bytes_arithmetic_and_refusals():
    from zhilight_amd import _lib
    f = _lib.lib().zl_lm_head_score_ws_bytes
    ws = lambda m, n: int(f(C.c_int64(m), C.c_int64(n)))
    assert ws(1, 1) == 16 + 16                                   # one record + the label logits rounded up to 16 bytes
    assert ws(5, 1000) == 5 * 8 * 16 + 32
    assert ws(2048, 128256) == 2048 * 1002 * 16 + 2048 * 4
    assert ws(300, 128) == 300 * 16 + 1200 and ws(300, 129) == 300 * 2 * 16 + 1200
    assert ws(0, 512) == ZL_EINVAL and ws(4, 0) == ZL_EINVAL and ws(-1, 5) == ZL_EINVAL
    assert ws(1 << 31, 512) == ZL_ESHAPE and ws(4, 1 << 31) == ZL_ESHAPE


def _call(x=1 << 20, w=1 << 20, ws=1 << 20, m=8, n=512, k=1024, ldx=None, dtype=0, col0=0):
    from zhilight_amd import _lib
    fake = C.c_void_p(1 << 20)                                   # never dereferenced: the checks return first
    return _lib.lib().zl_lm_head_score(C.c_void_p(x), C.c_int64(k if ldx is None else ldx), C.c_void_p(w), fake, C.c_int(-100),
                                       C.c_int(col0), fake, fake, fake, fake, fake, C.c_void_p(ws), C.c_int64(m), C.c_int64(n),
                                       C.c_int64(k), C.c_int(dtype), C.c_void_p(0))


def test_score_argument_checks_without_device():
    assert _call(x=0) == ZL_EINVAL
    assert _call(w=0) == ZL_EINVAL
    assert _call(ws=0) == ZL_EINVAL
    assert _call(m=0) == ZL_EINVAL and _call(n=0) == ZL_EINVAL
    assert _call(k=1000) == ZL_ESHAPE                            # K % 128
    assert _call(k=1024, ldx=1016) == ZL_ESHAPE                  # ldx < K
    assert _call(k=1024, ldx=1028) == ZL_ESHAPE                  # ldx % 8
    assert _call(x=(1 << 20) + 8) == ZL_ESHAPE                   # misaligned pointers
    assert _call(w=(1 << 20) + 2) == ZL_ESHAPE
    assert _call(ws=(1 << 20) + 4) == ZL_ESHAPE
    assert _call(col0=-1) == ZL_ESHAPE
    assert _call(dtype=2) == ZL_EDTYPE
    from zhilight_amd import _lib
    fake = C.c_void_p(1 << 20)
    for order, want in ((2, ZL_EINVAL), (-2, ZL_EINVAL), (-1, ZL_ESHAPE), (1, ZL_ESHAPE)):   # launch order: -1, 0, 1 (then K % 128 refuses)
        assert _lib.lib().zl_lm_head_score_ex(fake, C.c_int64(1000), fake, fake, C.c_int(-100), C.c_int(0), fake, fake, fake, fake, fake,
                                              fake, C.c_int64(8), C.c_int64(512), C.c_int64(1000), C.c_int(0), C.c_int(order),
                                              C.c_void_p(0)) == want


def test_label_builder():
    import torch
    from zhilight_amd import ops
    a, b = torch.tensor([5, 6, 7, 8], dtype=torch.int32), np.array([1, 2], np.int64)
    assert ops.score_labels([a, b]) == [6, 7, 8, -100, 2, -100]          # next-token shift, the last row of each task ignored
    assert ops.score_labels([a[:1]]) == [-100]
    assert ops.score_labels([a, b], [[9, -100, 3, 4], torch.tensor([-100, 0])]) == [9, -100, 3, 4, -100, 0]
    with pytest.raises(ops.ZLError):
        ops.score_labels([a, b], [[9, 1, 3], [1, 0]])                    # length mismatch
    with pytest.raises(ops.ZLError):
        ops.score_labels([a, b], [[9, 1, 3, 4]])


def _kernel_lse(y, bn=128):
    """The kernel's log-sum-exp of one row of (already rounded) logits in fp32, every sum in the WORST order: per bn-column block
    max and a sequential sum of exp(y - max); over the blocks a sequential merge that rescales the running sum whenever the
    maximum grows.  The kernel's own order (lane pairs, butterflies, four waves; a strided two-pass merge) has shorter chains."""
    f = np.float32
    run_m, run_s = f(-np.inf), f(0)
    for a in range(0, len(y), bn):
        blk = y[a:a + bn].astype(f)
        m = blk.max()
        s = f(0)
        for e in np.exp(blk - m, dtype=f):
            s = f(s + e)
        if m > run_m:
            run_s = f(f(run_s * np.exp(f(run_m - m), dtype=f)) + s) if run_m > -np.inf else s
            run_m = m
        else:
            run_s = f(run_s + f(s * np.exp(f(m - run_m), dtype=f)))
    return f(run_m + np.log(run_s, dtype=f))


@pytest.mark.parametrize("n", [512, 32000, 128256, 151936])
def test_log_sum_exp_bound_is_derived_not_fitted(n):
    rng = np.random.default_rng(n)
    for sigma in (0.5, 3.0, 8.0):
        y = (rng.standard_normal(n) * sigma).astype(np.float16)
        y64 = y.astype(np.float64)
        ref = y64.max() + np.log(np.exp(y64 - y64.max()).sum())
        err = abs(float(_kernel_lse(y)) - ref)
        print(n, sigma, err, bound(n))
        assert err <= bound(n), (n, sigma, err)
