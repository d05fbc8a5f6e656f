"""Decode attention at head size 64 on the matrix cores (decode_attn_d64.hip, through ops.multi_query_attention_rag_buffer and
ops.decode_attention_fused): which shapes take it, the prefix form against float64 attention on the same rounded inputs with NaN in
every slot behind a task's visible keys, and the fused form against the oracle's rope + copy (KV buffers, bit for bit), float64
attention, and the unfused sequence on the same kernel (bit for bit: the injected row against the loaded one)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 64
SCALE = 0.125
SHAPES = [(4, 4, 1), (8, 2, 1), (14, 2, 1), (32, 2, 1), (8, 2, 2), (4, 2, 1)]   # (h, hkv, len_q): 1, 4, 7, 16, 2 x 4 and 2 rows per kv head
LENS = [64, 64, 160, 160, 1088, 1088, 640]
# 32 tasks x 8 kv heads of 1088 slots take 384-key splits: wave w of a workgroup walks the chunks t0 + 64 w and, for w < 2,
# t0 + 64 w + 256 -- the prefetched chunk, the softmax carry, the reuse of the V staging and waves 2 and 3 in the merge.  Visible
# lengths: full; either side of a split; either side of wave 0's and wave 1's second chunk; short ones; then a spread
LONG = (32, 8, 32)                                                         # (h, hkv, tasks)
LONG_VALID = [1088, 384, 383, 385, 257, 256, 321, 320, 129, 193, 1, 65, 700, 769, 1025, 1087] + list(range(40, 1088, 66))
# the new row in wave 0's second chunk; in wave 1's, second split; a buffer's last slot (a second chunk's last key); a split's first
# slot; wave 1's second chunk's first key; slot 0; a slot whose owning split has no visible key; then a spread
LONG_POS = [300, 710, 1087, 384, 320, 0, 900, 639] + list(range(17, 1088, 45))
BAR = {0: 1e-3, 1: 5e-3}                                                   # the matrix-core tests' bars, of max(1, |exact| max)
TORCH_T = {0: torch.float16, 1: torch.bfloat16}


def _bits(oracle, x, dtype):
    return oracle.f32_to_bf16(x.astype(np.float32)) if dtype else oracle.h2u(x.astype(np.float16))


def _dev(bits, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(TORCH_T[dtype])


def _kv(oracle, rng, lens, hkv, bshd, dtype):
    shape = (lambda n: (n, hkv, D)) if bshd else (lambda n: (hkv, n, D))
    return [_bits(oracle, rng.standard_normal(shape(n)), dtype) for n in lens]


def _hide(bits, visible, bshd, dtype):
    """a copy with NaN in every slot from `visible` on"""
    out = bits.copy()
    nan = 0x7fc0 if dtype else 0x7e00
    if bshd:
        out[visible:] = nan
    else:
        out[:, visible:] = nan
    return out


@pytest.mark.parametrize("h,hkv,len_q", SHAPES)
def test_which_shapes_take_the_matrix_cores(dev, h, hkv, len_q):
    from zhilight_amd import ops
    # one query row per kv head, (4, 4, 1), stays on the VALU kernel: measured ahead there (profiles/decode_attn_d64.txt)
    assert ops.decode_attn_kernel(len_q, h, hkv, 64, algo=0) == int(len_q * h // hkv >= 2)
    assert ops.decode_attn_kernel(len_q, h, hkv, 64, masked=True, algo=0) == 0
    assert ops.decode_attn_kernel(len_q, h, hkv, 64, algo=1) == 0
    assert ops.decode_attn_kernel(17, hkv, hkv, 64, algo=0) == 0                      # 17 rows per kv head
    # D = 128: prefix lengths, or a mask alone at one query row per task
    assert ops.decode_attn_kernel(len_q, h, hkv, 128, algo=0) == 1
    assert ops.decode_attn_kernel(len_q, h, hkv, 128, masked=True, algo=0) == int(len_q == 1)
    assert ops.decode_attn_kernel(len_q, h, hkv, 128, masked=True, valid_lens=True, algo=0) == 0
    assert ops.decode_attn_kernel(len_q, h, hkv, 128, algo=1) == 0
    assert ops.decode_attn_kernel(len_q, h, hkv, 256, algo=0) == 0


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("h,hkv,len_q,b", [s + (len(LENS),) for s in SHAPES] + [(LONG[0], LONG[1], 1, LONG[2])])
def test_prefix_form_against_float64(oracle, dev, monkeypatch, h, hkv, len_q, b, bshd, dtype):
    from zhilight_amd import ops
    rng = np.random.default_rng(h + 2 * len_q + int(bshd))
    split = ops.decode_attn_split_len(b, hkv, max(LENS))
    if b == len(LENS):
        assert split == 128
        # one key; either side of a wave's first 64-key chunk; one short of a split; a split; a full buffer; two splits less two keys
        lens_l, valid = LENS, np.array([1, 30, 65, split - 1, split, 1088, 2 * split - 2], np.int32)
    else:
        assert split == 384
        lens_l, valid = [max(LENS)] * b, np.array(LONG_VALID, np.int32)
    lens = np.array(lens_l, np.int32)
    q = _bits(oracle, rng.standard_normal((b, len_q, h, D)) * 1.5, dtype)
    kb, vb = _kv(oracle, rng, lens_l, hkv, bshd, dtype), _kv(oracle, rng, lens_l, hkv, bshd, dtype)
    mask = np.concatenate([np.tile((np.arange(n) < v).astype(np.int8), len_q) for n, v in zip(lens_l, valid)])
    exact = oracle.mqa_rag_buffer(q, lens, kb, vb, mask, hkv, SCALE, bshd, dtype=dtype, exact=True)
    dk = [_dev(_hide(a, v, bshd, dtype), dev, dtype) for a, v in zip(kb, valid)]
    dv = [_dev(_hide(a, v, bshd, dtype), dev, dtype) for a, v in zip(vb, valid)]
    args = (_dev(q, dev, dtype), torch.from_numpy(lens).to(dev), ops.make_ptr_table(dk), ops.make_ptr_table(dv), None, SCALE, max(LENS), hkv)
    kw = dict(valid_lens=torch.from_numpy(valid).to(dev), bshd=bshd)
    assert ops.decode_attn_kernel(len_q, h, hkv, D) == int(len_q * h // hkv >= 2)
    got = ops.multi_query_attention_rag_buffer(*args, **kw).double().cpu().numpy()
    monkeypatch.setenv("ZL_ATTN_MFMA", "0")
    valu = ops.multi_query_attention_rag_buffer(*args, **kw).double().cpu().numpy()
    assert np.isfinite(got).all()
    bar = BAR[dtype] * max(1.0, np.abs(exact).max())
    err, dist = np.abs(got - exact).max(axis=(1, 2, 3)), np.abs(got - valu).max()
    print(f"decode d64 h {h} hkv {hkv} len_q {len_q} bshd {bshd} dtype {dtype}: max |got - exact| per task {err}, bar {bar:.3e}; "
          f"max |got - valu| {dist:.3e}")
    assert err.max() <= bar and dist <= 2 * bar


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("bshd", [True, False])
@pytest.mark.parametrize("neox", [True, False])
@pytest.mark.parametrize("h,hkv,b", [(8, 2, 4), (4, 4, 4), LONG])
def test_fused_form_against_oracle_and_unfused_sequence(oracle, dev, h, hkv, b, neox, bshd, dtype):
    from zhilight_amd import ops
    rng = np.random.default_rng(h + int(neox) + 2 * int(bshd))
    split = ops.decode_attn_split_len(b, hkv, 1088)
    if b == 4:
        assert split == 128
        lens_l = [64, 192, 1088, 256]
        # slot 0; a buffer's last slot; the first slot of a split; a slot whose owning split (the second) has no visible key
        pos = np.array([0, 191, split, 200], np.int32)
        valid = np.array([1, 192, split + 1, 100], np.int32)
    else:
        assert split == 384
        lens_l = [1088] * b
        pos = np.array(LONG_POS, np.int32)
        valid = pos + 1
        valid[6] = 500                                # slot 900 belongs to the third split, which sees nothing
    lens = np.array(lens_l, np.int32)
    kb, vb = _kv(oracle, rng, lens_l, hkv, bshd, dtype), _kv(oracle, rng, lens_l, hkv, bshd, dtype)
    qkv = _bits(oracle, rng.standard_normal((b, (h + 2 * hkv) * D)), dtype)
    cs, sn = oracle.rope_cos_sin(pos, D, 1e4, neox)
    # the device copies hold NaN where the new row goes: what the launch stores must reach the product from registers
    nan = 0x7fc0 if dtype else 0x7e00
    dks, dvs = [], []
    for _ in range(2):
        for src, dst in ((kb, dks), (vb, dvs)):
            bufs = [a.copy() for a in src]
            for a, p in zip(bufs, pos):
                a[(p,) if bshd else (slice(None), p)] = nan
            dst.append([_dev(a, dev, dtype) for a in bufs])
    rq, rk, rv = oracle.rope_qk_cache(cs, sn, qkv, h, hkv, D, neox, dtype=dtype)
    oracle.copy_to_rag_buffer2(pos.reshape(b, 1), lens, rk.reshape(b, 1, hkv, D), rv.reshape(b, 1, hkv, D), kb, vb, bshd)
    mask = np.concatenate([(np.arange(n) < v).astype(np.int8) for n, v in zip(lens_l, valid)])
    exact = oracle.mqa_rag_buffer(rq.reshape(b, 1, h, D), lens, kb, vb, mask, hkv, SCALE, bshd, dtype=dtype, exact=True).reshape(b, -1)
    t = lambda a: torch.from_numpy(a).to(dev)
    got = ops.decode_attention_fused(t(cs), t(sn), _dev(qkv, dev, dtype), t(pos), t(lens), t(valid), ops.make_ptr_table(dks[0]),
                                     ops.make_ptr_table(dvs[0]), h, hkv, D, SCALE, max(lens_l), neox, bshd)
    gq = ops.rope_scatter_decode(t(cs), t(sn), _dev(qkv, dev, dtype), t(pos), t(lens), ops.make_ptr_table(dks[1]),
                                 ops.make_ptr_table(dvs[1]), h, hkv, D, neox, bshd)
    assert ops.decode_attn_kernel(1, h, hkv, D) == int(h // hkv >= 2)       # (4, 4): both sides on the VALU kernel
    ref = ops.multi_query_attention_rag_buffer(gq.view(b, 1, h, D), t(lens), ops.make_ptr_table(dks[1]), ops.make_ptr_table(dvs[1]), None,
                                               SCALE, max(lens_l), hkv, valid_lens=t(valid), bshd=bshd)
    for i in range(b):
        for dbuf, want in ((dks[0][i], kb[i]), (dvs[0][i], vb[i]), (dks[1][i], kb[i]), (dvs[1][i], vb[i])):
            assert np.array_equal(dbuf.view(torch.int16).cpu().numpy().view(np.uint16), want), i
    err = np.abs(got.double().cpu().numpy() - exact).max()
    print(f"fused d64 h {h} hkv {hkv} neox {neox} bshd {bshd} dtype {dtype}: max |got - exact| {err:.3e}")
    assert err <= BAR[dtype] * max(1.0, np.abs(exact).max())
    assert torch.equal(got.view(torch.int16), ref.view(b, -1).view(torch.int16))
