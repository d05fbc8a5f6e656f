"""Sliding-window attention with sinks at head size 64 (zl_decode_attn_window, zl_prefill_attn_d64[_varlen]_window through the
`window` / `sinks` arguments of ops.multi_query_attention_rag_buffer and ops.prefill_attention[_varlen]) against float64 attention on
the same rounded inputs, with NaN in every K / V slot outside the keys a launch may see; the variants against their parents and
across launches bit for bit, and the prompt kernel's last row against the decode kernel's step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, SCALE, LEN_BUF = 64, 0.125, 1088
DT = [torch.float16, torch.bfloat16]
# the parents' bars -- tests/test_gpu_decode_attn_d64.py: of max(1, max |exact|); tests/test_gpu_prefill_attn_d64.py: of max |ref| per task
DECODE_BAR, PROMPT_BAR = {torch.float16: 1e-3, torch.bfloat16: 5e-3}, {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}
# the existing D = 64 prompt test's tasks, and 300 rows behind 150: several key tiles, the window's edge crossing tiles and 32-key groups
LENS = [1, 63, 65, 129, 200, 2, 300]
POS0 = [0, 0, 37, 0, 100, 127, 150]


def _reference(q, k, v, pos, window, sinks, hkv):
    """q (s, h, D), k / v (n, hkv, D) float64; the row at position pos[i] sees the keys max(0, pos[i] - window + 1) .. pos[i]
    (window 0: from key 0); sinks (h) or None: one logit per head in the normaliser"""
    s, h, _ = q.shape
    j = np.arange(k.shape[0])[None, :]
    hidden = (j > pos[:, None]) | ((j <= pos[:, None] - window) if window else False)
    out = np.empty_like(q)
    for head in range(h):
        hk = head // (h // hkv)
        sc = SCALE * q[:, head] @ k[:, hk].T
        sc[hidden] = -np.inf
        sink = -np.inf if sinks is None else sinks[head]
        m = np.maximum(sc.max(axis=1), sink)
        w = np.exp(sc - m[:, None])
        out[:, head] = (w @ v[:, hk]) / (w.sum(axis=1) + np.exp(sink - m))[:, None]
    return out


def _sinks(h, g):
    """at the scale of the scores; head 0 swamps its row (output almost zero), head 1 has no effect"""
    return torch.cat([torch.tensor([30.0, -30.0]), torch.randn(h - 2, generator=g) * 1.5])


def _poisoned(x, lo, hi, bshd, dev):
    """(n, hkv, D) -> the launch's layout on the device, NaN in front of slot lo and from slot hi on"""
    x = x.clone()
    x[:lo], x[hi:] = float("nan"), float("nan")
    return (x if bshd else x.transpose(0, 1)).contiguous().to(dev)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("window", [128, 100, 320, 0])        # one workgroup writes `out`; no multiple of a chunk; 3 splits + merge; sinks alone
@pytest.mark.parametrize("h,hkv,len_q", [(8, 2, 1), (14, 2, 1), (32, 2, 1), (8, 2, 2), (4, 4, 1)])
def test_decode_against_float64_and_the_parent(dev, h, hkv, len_q, window, bshd, dtype):
    from zhilight_amd import ops
    g = torch.Generator().manual_seed(h + len_q + window)
    w = window or 128
    valid = [1, w - 1, w, w + 1, w + 63, 2 * w + 5, LEN_BUF]    # lo = 0, 1, inside a 64-key chunk, unaligned to everything
    b = len(valid)
    assert ops.decode_attn_split_len(b, hkv, w) == 128
    q = (torch.randn(b, len_q, h, D, generator=g) * 1.5).to(dtype)
    sinks = _sinks(h, g)
    k, v = (torch.randn(b, LEN_BUF, hkv, D, generator=g).to(dtype) for _ in range(2))
    los = [max(0, n - window) if window else 0 for n in valid]
    dk, dv = ([_poisoned(x[i], los[i], valid[i], bshd, dev) for i in range(b)] for x in (k, v))
    args = (q.to(dev), torch.full((b,), LEN_BUF, dtype=torch.int32, device=dev), ops.make_ptr_table(dk), ops.make_ptr_table(dv), None,
            SCALE, LEN_BUF, hkv)
    kw = dict(valid_lens=torch.tensor(valid, dtype=torch.int32, device=dev), bshd=bshd)
    for sk in (sinks, None) if window else (sinks,):
        got = ops.multi_query_attention_rag_buffer(*args, window=window, sinks=None if sk is None else sk.to(dev), **kw).double().cpu().numpy()
        assert np.isfinite(got).all()
        for i in range(b):
            exact = _reference(q[i].double().numpy(), k[i].double().numpy(), v[i].double().numpy(), np.full(len_q, valid[i] - 1), window,
                               None if sk is None else sk.double().numpy(), hkv)
            err, bar = np.abs(got[i] - exact).max(), DECODE_BAR[dtype] * max(1.0, np.abs(exact).max())
            print(f"decode window {window} sinks {sk is not None} task {i} (valid {valid[i]}): max |got - exact| {err:.3e}, bar {bar:.3e}")
            assert err <= bar, (i, err, bar)
    if not window and len_q * h // hkv >= 2:
        # a window over the whole buffer, no sinks: the parent's bits (with one row per kv head the parent runs the VALU kernel)
        parent = ops.multi_query_attention_rag_buffer(*args, **kw)
        for over in (LEN_BUF, 5000):
            assert torch.equal(ops.multi_query_attention_rag_buffer(*args, window=over, **kw).view(torch.int16), parent.view(torch.int16))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("window", [128, 100, 33])
def test_prompt_against_float64_across_launches_and_the_decode_step(dev, window, bshd, dtype):
    from zhilight_amd import ops
    h, hkv = 8, 2
    g = torch.Generator().manual_seed(window + int(bshd))
    q = (torch.randn(sum(LENS), h, D, generator=g) * 1.5).to(dtype)
    len_bufs = [((p0 + s + 63) // 64 * 64 + 64) for s, p0 in zip(LENS, POS0)]
    k, v = ([torch.randn(n, hkv, D, generator=g).to(dtype) for n in len_bufs] for _ in range(2))
    sinks, cu, qd = _sinks(h, g), np.concatenate([[0], np.cumsum(LENS)]), q.to(dev)
    # the tasks' buffers, NaN outside the keys each task may see
    r = [(max(0, p0 - window + 1), p0 + s) for s, p0 in zip(LENS, POS0)]
    ks, vs = ([_poisoned(x, *r[i], bshd, dev) for i, x in enumerate(kv)] for kv in (k, v))
    kt, vt = ops.make_ptr_table(ks), ops.make_ptr_table(vs)
    for sk in (None, sinks):
        kw = dict(window=window, sinks=None if sk is None else sk.to(dev))
        out = ops.prefill_attention_varlen(qd, LENS, POS0, kt, vt, len_bufs, hkv, SCALE, bshd, **kw)
        assert torch.isfinite(out).all()
        for i, (s, p0) in enumerate(zip(LENS, POS0)):
            ref = _reference(q[cu[i]:cu[i + 1]].double().numpy(), k[i].double().numpy(), v[i].double().numpy(), p0 + np.arange(s), window,
                             None if sk is None else sk.double().numpy(), hkv)
            got = out[cu[i]:cu[i + 1]]
            err = np.abs(got.double().cpu().numpy() - ref).max() / np.abs(ref).max()
            print(f"prompt window {window} sinks {sk is not None} task {i} (s {s}, pos0 {p0}): max |got - ref| / max |ref| = {err:.3e}")
            assert err <= PROMPT_BAR[dtype], (i, err)
            one = ops.prefill_attention(qd[cu[i]:cu[i + 1]].contiguous(), ks[i], vs[i], p0, hkv, SCALE, bshd, **kw)
            assert torch.equal(got.view(torch.int16), one.view(torch.int16)), i
    # (from here on with sinks)  every workgroup alone -- a work table of one (task, 64-row tile) -- over buffers with NaN in front of
    # ITS first visible key and behind its last: the same bits as in the full launch
    for task, qt in ops.prefill_work_items(LENS, POS0):
        r0, r1 = 64 * qt, min(64 * qt + 64, LENS[task])
        lo, hi = max(0, POS0[task] + r0 - window + 1), POS0[task] + r1
        ks1, vs1 = list(ks), list(vs)                     # (kept alive: the tables hold addresses)
        ks1[task], vs1[task] = _poisoned(k[task], lo, hi, bshd, dev), _poisoned(v[task], lo, hi, bshd, dev)
        plan = ops.prefill_varlen_plan(LENS, POS0, len_bufs, dev)
        plan.work[:2], plan.n_work = torch.tensor([task, qt], dtype=torch.int32), 1
        alone = ops.prefill_attention_varlen(qd, LENS, POS0, ops.make_ptr_table(ks1), ops.make_ptr_table(vs1), len_bufs, hkv, SCALE, bshd,
                                             plan=plan, out=torch.zeros_like(qd), **kw)
        rows = slice(cu[task] + r0, cu[task] + r1)
        assert torch.equal(alone[rows].view(torch.int16), out[rows].view(torch.int16)), (task, qt)
    # the last row of the 200-row chunk against a decode step over the same buffer: two kernels, two orders of summation -- the sum
    # of their bars, not bit equality
    i32 = dict(dtype=torch.int32, device=dev)
    step = ops.multi_query_attention_rag_buffer(qd[cu[5] - 1].view(1, 1, h, D), torch.tensor(len_bufs[4:5], **i32), kt[4:5], vt[4:5], None,
                                                SCALE, len_bufs[4], hkv, valid_lens=torch.tensor([POS0[4] + LENS[4]], **i32), bshd=bshd, **kw)
    top = np.abs(_reference(q[cu[5] - 1:cu[5]].double().numpy(), k[4].double().numpy(), v[4].double().numpy(), np.array([POS0[4] + LENS[4] - 1]),
                            window, sinks.double().numpy(), hkv)).max()
    diff = (out[cu[5] - 1].double() - step.view(h, D).double()).abs().max().item()
    print(f"prompt row against decode step: max |difference| {diff:.3e}")
    assert diff <= PROMPT_BAR[dtype] * top + DECODE_BAR[dtype] * max(1.0, top)
    # a window over the whole prefix, no sinks: the parents' bits, varlen and one task
    if window == 128:                                     # (the parent reads every key up to a row's position: it needs all of them finite)
        ck, cv = ([_poisoned(x, 0, e, bshd, dev) for x, (_, e) in zip(kv, r)] for kv in (k, v))
        tabs = (ops.make_ptr_table(ck), ops.make_ptr_table(cv), len_bufs, hkv, SCALE, bshd)
        assert torch.equal(ops.prefill_attention_varlen(qd, LENS, POS0, *tabs, window=max(len_bufs)).view(torch.int16),
                           ops.prefill_attention_varlen(qd, LENS, POS0, *tabs).view(torch.int16))
        one = (qd[cu[6]:].contiguous(), ck[6], cv[6], POS0[6], hkv, SCALE, bshd)
        assert torch.equal(ops.prefill_attention(*one, window=len_bufs[6]).view(torch.int16), ops.prefill_attention(*one).view(torch.int16))
