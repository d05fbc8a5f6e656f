"""The two kernels of the speculative verify step through the C ABI: zl_decode_attn_causal (the staircase form of the matrix-core
decode attention) against the fp64 oracle and the VALU mask route, and zl_spec_accept against the numpy reference, bit for bit."""
import numpy as np
import pytest
import torch

import spec_ref

pytestmark = pytest.mark.gpu

LENS = [64, 64, 160, 160, 1088, 1088, 640]


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.view(dtype)


def _bits(t):
    return t.detach().view(torch.int16).cpu().numpy().view(np.uint16)


def _to_bits(x, dtype, oracle):
    return oracle.f32_to_bf16(x.astype(np.float32)) if dtype else oracle.h2u(x.astype(np.float16))


def _staircase_valid(split, len_q):
    """first-row visible lengths of the seven tasks, from the launch's split length"""
    valid = [1,                          # the staircase starts at one key
             30,                         # straddles a 32-key chunk
             split - 1,                  # straddles a split: the early rows have an empty second split
             split - len_q + 1,          # ends at a split
             1025 - len_q,               # deep into a long buffer
             LENS[5] - len_q + 1,        # fills the buffer
             2 * split - 2]              # straddles the second split boundary
    for L, v in zip(LENS, valid):
        assert v >= 1 and v + len_q - 1 <= L, (L, v, len_q)
    return valid


@pytest.mark.parametrize("h,hkv,len_q", [(32, 8, 4), (8, 2, 2), (16, 4, 3), (28, 4, 2), (8, 8, 5), (24, 8, 5), (32, 8, 8), (32, 4, 3)])
@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("dtype", [0, 1])
def test_causal_decode_attention(oracle, dev, h, hkv, len_q, bshd, dtype):
    """row qi of a task sees valid + qi keys: against the fp64 oracle with causal_step_mask (1e-3 / 5e-3 of max(1, |exact|max), the
    matrix-core test's bar) and against the VALU mask route (twice that); K and V of every slot no row sees are NaN"""
    from zhilight_amd import ops
    rng = np.random.default_rng(41)
    d, b = 128, len(LENS)
    tdt = torch.bfloat16 if dtype else torch.float16
    split = ops.decode_attn_split_len(b, hkv, max(LENS))
    valid = _staircase_valid(split, len_q)
    kb, vb = [], []
    for L in LENS:
        shape = (L, hkv, d) if bshd else (hkv, L, d)
        kb.append(_to_bits(rng.standard_normal(shape), dtype, oracle))
        vb.append(_to_bits(rng.standard_normal(shape), dtype, oracle))
    dk = [_t(a.view(np.int16), dev, tdt) for a in kb]
    dv = [_t(a.view(np.int16), dev, tdt) for a in vb]
    q = _to_bits(rng.standard_normal((b, len_q, h, d)), dtype, oracle)
    qd = _t(q.view(np.int16), dev, tdt)
    scale = 1.0 / np.sqrt(d)
    lens_np, lens_d, valid_d = np.array(LENS, np.int32), _t(np.array(LENS, np.int32), dev), _t(np.array(valid, np.int32), dev)
    mask = ops.causal_step_mask(LENS, valid, len_q)
    exact = oracle.mqa_rag_buffer(q, lens_np, kb, vb, mask.numpy(), hkv, scale, bshd, dtype=dtype, exact=True)
    k_tab, v_tab = ops.make_ptr_table(dk), ops.make_ptr_table(dv)
    # the VALU mask route first: it walks the whole buffer, so its tail stays finite
    valu = ops.multi_query_attention_rag_buffer(qd, lens_d, k_tab, v_tab, mask.to(dev), scale, max(LENS), hkv, bshd=bshd)
    valu = oracle.to_f32(_bits(valu), dtype).astype(np.float64)
    nan = np.uint16(0x7fc0 if dtype else 0x7e00)
    for bi, (L, v) in enumerate(zip(LENS, valid)):               # device copies only: what no row sees must not reach the result
        end = v + len_q - 1
        if end < L:
            pk, pv = kb[bi].copy(), vb[bi].copy()
            if bshd:
                pk[end:], pv[end:] = nan, nan
            else:
                pk[:, end:], pv[:, end:] = nan, nan
            dk[bi].copy_(_t(pk.view(np.int16), dev, tdt))
            dv[bi].copy_(_t(pv.view(np.int16), dev, tdt))
    got = ops.decode_attention_causal(qd, lens_d, k_tab, v_tab, valid_d, scale, max(LENS), hkv, bshd=bshd)
    g = oracle.to_f32(_bits(got), dtype).astype(np.float64)
    assert g.shape == exact.shape and np.isfinite(g).all()
    tol = (5e-3 if dtype else 1e-3) * max(1.0, np.abs(exact).max())
    err = np.abs(g - exact).reshape(b, -1).max(axis=1)
    print("max |got - exact| per task:", err, "bar", tol, "vs VALU mask route:", np.abs(g - valu).max())
    assert err.max() < tol, err
    assert np.abs(g - valu).max() < 2 * tol


@pytest.mark.parametrize("h,hkv", [(32, 8), (28, 4), (8, 8)])
@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("dtype", [0, 1])
def test_causal_one_row_is_the_prefix_form(oracle, dev, h, hkv, bshd, dtype):
    """len_q == 1: zl_decode_attn(mask = NULL, valid_lens) bit for bit"""
    from zhilight_amd import ops
    rng = np.random.default_rng(42)
    d, b = 128, len(LENS)
    tdt = torch.bfloat16 if dtype else torch.float16
    valid = [1, 33, 128, 129, 1025, 1088, 517]
    dk = [_t(_to_bits(rng.standard_normal((L, hkv, d) if bshd else (hkv, L, d)), dtype, oracle).view(np.int16), dev, tdt) for L in LENS]
    dv = [_t(_to_bits(rng.standard_normal((L, hkv, d) if bshd else (hkv, L, d)), dtype, oracle).view(np.int16), dev, tdt) for L in LENS]
    qd = _t(_to_bits(rng.standard_normal((b, 1, h, d)), dtype, oracle).view(np.int16), dev, tdt)
    lens_d, valid_d = _t(np.array(LENS, np.int32), dev), _t(np.array(valid, np.int32), dev)
    k_tab, v_tab = ops.make_ptr_table(dk), ops.make_ptr_table(dv)
    ref = ops.multi_query_attention_rag_buffer(qd, lens_d, k_tab, v_tab, None, 0.088, max(LENS), hkv, valid_lens=valid_d, bshd=bshd)
    got = ops.decode_attention_causal(qd, lens_d, k_tab, v_tab, valid_d, 0.088, max(LENS), hkv, bshd=bshd)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


def test_causal_refusals(dev):
    from zhilight_amd import ops
    i32 = dict(dtype=torch.int32, device=dev)
    lens, valid = torch.full((2,), 64, **i32), torch.full((2,), 3, **i32)

    def call(d=128, len_q=2, h=8, hkv=2, dt=torch.float16, **kw):
        kv = [torch.zeros((64, hkv, d), dtype=dt, device=dev) for _ in range(2)]
        tab = ops.make_ptr_table(kv)
        a = dict(buf_lens=lens, k_addrs=tab, v_addrs=tab, valid_lens=valid)
        a.update(kw)
        return ops.decode_attention_causal(torch.zeros((2, len_q, h, d), dtype=dt, device=dev), a["buf_lens"], a["k_addrs"], a["v_addrs"],
                                           a["valid_lens"], 0.088, 64, hkv, workspace=a.get("workspace"))
    call()
    with pytest.raises(ops.ZLError):
        call(d=64)
    with pytest.raises(ops.ZLError):
        call(len_q=33)
    with pytest.raises(ops.ZLError):
        call(h=9)
    with pytest.raises(ops.ZLError):
        call(dt=torch.float32)
    with pytest.raises(ops.ZLError):
        call(valid_lens=valid.to(torch.int64))
    with pytest.raises(ops.ZLError):
        call(buf_lens=lens[:1])
    with pytest.raises(ops.ZLError):
        call(workspace=torch.zeros(16, dtype=torch.float32, device=dev))


# ---------------------------------------------------------------------------------------------------------------- zl_spec_accept
@pytest.mark.parametrize("b,k,n", [(1, 1, 512), (3, 3, 512), (8, 3, 4099), (4, 7, 128256)])
@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16, torch.float32])
def test_spec_accept_bit_for_bit(dev, b, k, n, tdt):
    """picks, accepted, out_tokens and the four state vectors against the numpy reference; rows with two equal maxima (the lowest
    column wins), a row stride beyond n, drafts built so that every count from 0 to K occurs in every task"""
    from zhilight_amd import ops
    rng = np.random.default_rng(b * 1000 + k)
    len_q, ld = k + 1, n + 24
    m = b * len_q
    store = torch.from_numpy(rng.standard_normal((m, ld)).astype(np.float32)).to(tdt)
    store[:, n:] = 100.0                                         # beyond the row: must not be looked at
    for r in range(0, m, 2):                                     # forced ties above everything else in the row
        c0, c1 = sorted(rng.choice(n, 2, replace=False))
        store[r, c0] = store[r, c1] = 50.0
    logits = store.to(dev)[:, :n]
    picks = spec_ref.argmax_rows(store[:, :n].float().numpy()).reshape(b, len_q)
    for r in range(0, m, 2):
        assert store[r, picks.reshape(-1)[r]] == 50.0 and (store[r, :picks.reshape(-1)[r]] < 50.0).all()
    state = [rng.integers(0, 1000, b).astype(np.int32) for _ in range(4)]
    for shift in range(len_q):
        want = [(t + shift) % len_q for t in range(b)]           # accepted drafts of task t in this call
        drafts = picks[:, :k].copy()
        for t, w in enumerate(want):
            if w < k:
                drafts[t, w] = (drafts[t, w] + 1) % n
        acc_ref, out_ref = spec_ref.accept(picks, drafts)
        assert acc_ref.tolist() == want
        dev_state = [torch.from_numpy(v).to(dev) for v in state]
        acc, out = ops.spec_accept(logits, torch.from_numpy(drafts).to(dev), *dev_state)
        assert acc.dtype == torch.int32 and out.dtype == torch.int32 and out.shape == (b, len_q)
        assert np.array_equal(acc.cpu().numpy(), acc_ref) and np.array_equal(out.cpu().numpy(), out_ref)
        for got, ref in zip(dev_state, spec_ref.advance(acc_ref, out_ref, *state)):
            assert np.array_equal(got.cpu().numpy(), ref)
    # no bookkeeping pointers at all, and one of the four
    drafts = torch.from_numpy(picks[:, :k].copy()).to(dev)
    acc, out = ops.spec_accept(logits, drafts)
    assert acc.tolist() == [k] * b and np.array_equal(out.cpu().numpy(), picks)
    only = torch.zeros(b, dtype=torch.int32, device=dev)
    ops.spec_accept(logits, drafts, valid_lens=only)
    assert only.tolist() == [k + 1] * b


def test_spec_accept_nan_counts_as_largest(dev):
    from zhilight_amd import ops
    x = torch.randn((4, 300), dtype=torch.float32)
    x[1, 7] = x[1, 200] = float("nan")
    x[3, 299] = float("inf")
    picks = spec_ref.argmax_rows(x.numpy()).reshape(2, 2)
    assert picks[0, 1] == 7 and picks[1, 1] == 299
    drafts = torch.tensor([[int(picks[0, 0])], [int(picks[1, 0]) + 1]], dtype=torch.int32)
    acc, out = ops.spec_accept(x.to(dev), drafts.to(dev))
    assert acc.tolist() == [1, 0] and out.tolist() == [[int(picks[0, 0]), 7], [int(picks[1, 0]), -1]]


def test_spec_accept_device_refusals(dev):
    from zhilight_amd import ops
    logits = torch.zeros((8, 16), dtype=torch.float16, device=dev)
    drafts = torch.zeros((2, 3), dtype=torch.int32, device=dev)
    ops.spec_accept(logits, drafts)
    with pytest.raises(ops.ZLError, match="on the logits' device"):
        ops.spec_accept(logits, drafts.cpu())
    with pytest.raises(ops.ZLError, match="drafts are"):                          # the host-side cases again, with device logits
        ops.spec_accept(logits, drafts.to(torch.int64))
    with pytest.raises(ops.ZLError, match="drafts are"):
        ops.spec_accept(logits, torch.zeros((2, 0), dtype=torch.int32, device=dev))
    with pytest.raises(ops.ZLError, match="one logit row per task"):
        ops.spec_accept(logits, torch.zeros((3, 3), dtype=torch.int32, device=dev))
    with pytest.raises(ops.ZLError, match="unsupported logits dtype"):
        ops.spec_accept(logits.to(torch.float64), drafts)
    with pytest.raises(ops.ZLError, match="unit column stride"):
        ops.spec_accept(torch.zeros((16, 8), dtype=torch.float16, device=dev).t(), drafts)
    with pytest.raises(ops.ZLError):
        ops.spec_accept(logits, drafts, tokens=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ops.ZLError):
        ops.spec_accept(logits, drafts, positions=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(ops.ZLError):
        ops.spec_accept(logits, drafts, out_tokens=torch.zeros((2, 3), dtype=torch.int32, device=dev))
