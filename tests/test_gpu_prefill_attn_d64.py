"""Prompt attention at head size 64 (zl_prefill_attn_d64 / zl_prefill_attn_d64_varlen through ops.prefill_attention[_varlen]) against
float64 causal softmax attention on the same rounded inputs; the varlen launch against the one-task launch, bit for bit; and a
task's rows against the same task in a longer buffer (a row depends on the keys it sees only).  Rows behind a task's last visible
key hold NaN in K and V."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# one row; one row short of a query tile; a tile plus one row behind a history; one key past a 128-key tile; three key tiles with a
# partial last one behind a history; a two-row chunk that straddles the 128-key boundary
LENS = [1, 63, 65, 129, 200, 2]
POS0 = [0, 0, 37, 0, 100, 127]
D = 64


def _reference(q, k, v, p0, hkv, scale):
    """q (s, h, D), k / v (rows, hkv, D) float64 -> (s, h, D): causal softmax attention, query i at position p0 + i"""
    s, h, _ = q.shape
    out = np.empty_like(q)
    for head in range(h):
        hk = head // (h // hkv)
        sc = scale * q[:, head] @ k[:p0 + s, hk].T
        sc[np.arange(p0 + s)[None, :] > (p0 + np.arange(s))[:, None]] = -np.inf
        w = np.exp(sc - sc.max(axis=1, keepdims=True))
        out[:, head] = (w / w.sum(axis=1, keepdims=True)) @ v[:p0 + s, hk]
    return out


@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("h,hkv", [(8, 2), (4, 4)])
def test_prefill_attention_d64_against_float64_and_across_launches(dev, h, hkv, dtype, bshd):
    from zhilight_amd import _lib, ops
    g = torch.Generator().manual_seed(h + int(bshd))
    scale = 1.0 / np.sqrt(D)
    q = (torch.randn(sum(LENS), h, D, generator=g) * 1.5).to(dtype)
    ks, vs, longer, len_bufs, refs = [], [], [], [], []
    cu = np.concatenate([[0], np.cumsum(LENS)])

    def lay(x):                                           # (rows, hkv, D) -> the launch's layout, on the device
        return (x if bshd else x.transpose(0, 1)).contiguous().to(dev)

    for i, (s, p0) in enumerate(zip(LENS, POS0)):
        lb = (p0 + s + 63) // 64 * 64 + 64
        k, v = torch.randn(lb, hkv, D, generator=g).to(dtype), torch.randn(lb, hkv, D, generator=g).to(dtype)
        refs.append(_reference(q[cu[i]:cu[i + 1]].double().numpy(), k.double().numpy(), v.double().numpy(), p0, hkv, scale))
        k[p0 + s:], v[p0 + s:] = float("nan"), float("nan")           # behind the task's visible keys: must not leak
        nan = torch.full((64, hkv, D), float("nan"), dtype=dtype)
        ks.append(lay(k)); vs.append(lay(v)); len_bufs.append(lb)
        longer.append((lay(torch.cat([k, nan])), lay(torch.cat([v, nan]))))
    qd = q.to(dev)
    out = ops.prefill_attention_varlen(qd, LENS, POS0, ops.make_ptr_table(ks), ops.make_ptr_table(vs), len_bufs, hkv, scale, bshd)
    bar = 1.5e-2 if dtype == torch.bfloat16 else 2e-3
    for i, p0 in enumerate(POS0):
        qi, got = qd[cu[i]:cu[i + 1]].contiguous(), out[cu[i]:cu[i + 1]]
        assert torch.isfinite(got).all(), i
        err = np.abs(got.double().cpu().numpy() - refs[i]).max() / np.abs(refs[i]).max()
        print(f"task {i} (s {LENS[i]}, pos0 {p0}): max |got - ref| / max |ref| = {err:.3e}")
        assert err <= bar, (i, err)
        assert torch.equal(got.view(torch.int16), ops.prefill_attention(qi, ks[i], vs[i], p0, hkv, scale, bshd).view(torch.int16)), i
        assert torch.equal(got.view(torch.int16), ops.prefill_attention(qi, *longer[i], p0, hkv, scale, bshd).view(torch.int16)), i
    # the wrappers' refusals: another head size, wave groups at head size 64
    with pytest.raises(ops.ZLError, match="64 and 128"):
        ops.prefill_attention(torch.zeros(4, h, 96, dtype=dtype, device=dev), ks[0], vs[0], 0, hkv, scale, bshd)
    with pytest.raises(ops.ZLError, match="groups"):
        ops.prefill_attention(qd[:1], ks[0], vs[0], 0, hkv, scale, bshd, groups=2)
    # the C entry point's argument checks return before any device call (the call form of test_prefill_varlen_host.py)
    fake, i64 = C.c_void_p(1 << 20), C.c_int64

    def call(work=fake, hkv_=2, dt=0):
        return _lib.lib().zl_prefill_attn_d64_varlen(fake, fake, fake, fake, fake, fake, fake, work, i64(10), i64(5), i64(393), i64(8),
                                                     i64(hkv_), C.c_float(0.1), C.c_int(1), C.c_int(dt), C.c_void_p(0))
    assert (call(work=C.c_void_p(0)), call(hkv_=3), call(dt=2)) == (-1, -2, -3)
