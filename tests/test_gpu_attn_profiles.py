"""The attention kernels on peaked, drifting and offset score profiles (tests/attn_profiles.py) instead of i.i.d. normals: the
data-dependent code of the online softmax -- the "rescale only if a maximum moved" shortcuts, merges of partials whose maxima differ
by tens, the last visible key, finite data behind the mask, scores far from zero -- against the fp64 oracle at every kernel's EXISTING
bar (tests/test_attn_profiles_host.py shows on the CPU that an fp32 kernel has room inside it on every workload here, and that every
defect the profiles are built for exceeds it).

All decode routes run b = 6 tasks in one launch over buffers of 640 slots with 1, 31, 33, 129, 517 and 640 visible keys; the profile
lies over each task's visible keys, so the spike / the end of the ramp sits on a ragged chunk, a split boundary and the buffer end.
Every case prints "ATTNPROF route profile dtype layout max|got - exact| / bar" (docs/lab/attn_score_profiles.md is filled from it).
"""
import functools

import numpy as np
import pytest
import torch

import attn_profiles as ap

pytestmark = pytest.mark.gpu

DT = [pytest.param(0, id="fp16"), pytest.param(1, id="bf16")]
LAYOUT = [pytest.param(True, id="bshd"), pytest.param(False, id="bhsd")]


def _tdt(dtype):
    return torch.bfloat16 if dtype else torch.float16


def _dev_bits(bits, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(_tdt(dtype))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _vals(t, dtype):
    return ap.from_bits(t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16), dtype)


def _lay(arrs, bshd):
    return arrs if bshd else [np.ascontiguousarray(np.moveaxis(a, 1, 0)) for a in arrs]


@functools.lru_cache(maxsize=32)
def _decode(geom, name, dtype, long=False):
    return ap.decode_case(geom, name, dtype, long=long)


@functools.lru_cache(maxsize=8)
def _prefill(geom, name, dtype):
    return ap.prefill_case(geom, name, dtype)


def _report(route, name, dtype, bshd, g, exact, bar):
    assert g.shape == exact.shape and np.isfinite(g).all(), route
    err = np.abs(g - exact).max()
    print(f"ATTNPROF {route} {name} {'bf16' if dtype else 'fp16'} {'bshd' if bshd else 'bhsd'} {err / bar:.4f}")
    assert err < bar, (route, name, err, bar)


class _Dec:
    """a decode case on the device: q, the K / V pointer tables, lengths, the mask, the oracle's exact rows"""

    def __init__(self, oracle, dev, c, bshd, hkv):
        from zhilight_amd import ops
        dtype = c.dtype
        self.k, self.v = _lay(c.k, bshd), _lay(c.v, bshd)
        self.dk = [_dev_bits(a, dev, dtype) for a in self.k]
        self.dv = [_dev_bits(a, dev, dtype) for a in self.v]
        self.ka, self.va = ops.make_ptr_table(self.dk), ops.make_ptr_table(self.dv)
        self.q = _dev_bits(c.q, dev, dtype)
        self.lens = _t(np.array(c.buf_lens, np.int32), dev)
        self.valid = _t(np.array(c.valid, np.int32), dev)
        self.mask = _t(c.mask, dev)
        self.max_len = max(c.buf_lens)
        self.exact = oracle.mqa_rag_buffer(c.q, np.array(c.buf_lens, np.int32), self.k, self.v, c.mask, hkv, c.scale, bshd, dtype=dtype, exact=True)
        assert np.abs(self.exact - c.ref).max() <= 1e-6


# ---- routes 1-3: multi_query_attention_rag_buffer ---------------------------------------------------------------------------------
# (route id, geometry of DECODE_GEOMS [hidden_spike: its form with holes], mask or valid_lens, ZL_ATTN_MFMA=0)
RAG_ROUTES = [
    ("valu_d64", "d64", "mask", False),                         # route 1: the VALU split-KV kernel
    ("valu_d128", "h8", "mask", True),
    ("valu_d128_q2", "h8_q2", "mask", False),                   # (two rows with a mask: the VALU kernel by shape)
    ("mfma_prefix_h8", "h8", "valid", False),                   # route 2: the matrix-core prefix form
    ("mfma_prefix_h16_q4", "h16_q4", "valid", False),           # 16 rows per kv head
    ("mfma_prefix_h28", "h28", "valid", False),                 # 7 rows: a ragged tile
    ("mfma_mask_h8", "h8_holes", "mask", False),                # route 3: the matrix-core mask form, masks with holes
]


@pytest.mark.parametrize("bshd", LAYOUT)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", ap.PROFILES)
@pytest.mark.parametrize("route,geom,form,valu", RAG_ROUTES, ids=[r[0] for r in RAG_ROUTES])
def test_rag_buffer_attention_on_score_profiles(oracle, dev, monkeypatch, route, geom, form, valu, name, dtype, bshd):
    from zhilight_amd import ops
    if valu:
        monkeypatch.setenv("ZL_ATTN_MFMA", "0")
    if form == "mask" and name == "hidden_spike" and not geom.endswith("_holes"):
        geom = {"d64": "d64_holes", "h8": "h8_holes", "h8_q2": "h8_q2_holes"}[geom]     # finite spikes in holes inside the visible range too
    d, h, hkv, len_q, _ = ap.DECODE_GEOMS[geom]
    c = _decode(geom, name, dtype)
    x = _Dec(oracle, dev, c, bshd, hkv)
    got = ops.multi_query_attention_rag_buffer(x.q, x.lens, x.ka, x.va, x.mask if form == "mask" else None, c.scale, x.max_len, hkv,
                                               valid_lens=x.valid if form == "valid" else None, bshd=bshd)
    # bar: test_decode_attention_matrix_core_path / _mask_form (1e-3, bf16 5e-3 of max(1, max|exact|)); test_decode_attention has the same 1e-3
    _report(route, name, dtype, bshd, _vals(got, dtype), x.exact, ap.decode_bar(x.exact, dtype))


# ---- route 4: decode_attention_causal -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bshd", LAYOUT)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", ap.PROFILES)
@pytest.mark.parametrize("geom", ["causal_h8_q4", "causal_h32_q3"])          # 16 rows; 24 rows per kv head = two tiles
def test_causal_attention_on_score_profiles(oracle, dev, geom, name, dtype, bshd):
    """row qi sees valid + qi keys; the profile lies over the keys of the last row (late_spike: a ladder, every row ends on a spike),
    under hidden_spike the slots no row sees are finite and 125 above"""
    from zhilight_amd import ops
    d, h, hkv, len_q, _ = ap.DECODE_GEOMS[geom]
    c = _decode(geom, name, dtype)
    x = _Dec(oracle, dev, c, bshd, hkv)
    assert np.array_equal(c.mask, ops.causal_step_mask(c.buf_lens, c.valid, len_q).numpy())
    got = ops.decode_attention_causal(x.q, x.lens, x.ka, x.va, x.valid, c.scale, x.max_len, hkv, bshd=bshd)
    # bar: test_causal_decode_attention (the matrix-core test's bar)
    _report(geom, name, dtype, bshd, _vals(got, dtype), x.exact, ap.decode_bar(x.exact, dtype))


# ---- route 5: decode_attention_la ---------------------------------------------------------------------------------------------------
_LA_WS = {}


@pytest.mark.parametrize("bshd", LAYOUT)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", ap.PROFILES)
@pytest.mark.parametrize("split_len", [32, 128, 0])
def test_last_arriver_attention_on_score_profiles(oracle, dev, split_len, name, dtype, bshd):
    """the merge by the last-arriving workgroup: fp32 and (fp16) half records; ONE workspace, zeroed once, for every case here"""
    from zhilight_amd import ops
    d, h, hkv, len_q, _ = ap.DECODE_GEOMS["h8"]
    c = _decode("h8", name, dtype)
    x = _Dec(oracle, dev, c, bshd, hkv)
    if "ws" not in _LA_WS:
        _LA_WS["ws"] = ops.decode_attn_la_workspace(len(c.valid), h, hkv, x.max_len, dev)
    ws = _LA_WS["ws"]
    for half in ((False, True) if dtype == 0 else (False,)):
        got = ops.decode_attention_la(x.q, x.lens, x.ka, x.va, x.valid, c.scale, x.max_len, hkv, ws, bshd=bshd, split_len=split_len, half=half)
        # bar: test_last_arriver_attention_against_the_oracle
        _report(f"la_split{split_len}{'_half' if half else ''}", name, dtype, bshd, _vals(got, dtype), x.exact, ap.decode_bar(x.exact, dtype))
        torch.cuda.synchronize()
        assert int(ws.view(torch.int32)[:len(c.valid) * hkv].abs().sum()) == 0      # every pair's arrival word is back to zero


# ---- route 6: half records + their stand-alone merge --------------------------------------------------------------------------------
@pytest.mark.parametrize("bshd", LAYOUT)
@pytest.mark.parametrize("name", ap.PROFILES)
@pytest.mark.parametrize("form", ["prefix", "mask"])
def test_half_record_merge_on_score_profiles(oracle, dev, form, name, bshd):
    """decode_attention_splits + decode_attention_combine_h, and the mask form's records of EVERY split merged with valid_lens = None"""
    from zhilight_amd import ops
    geom = "h8" if form == "prefix" else "h8_holes"
    d, h, hkv, len_q, _ = ap.DECODE_GEOMS[geom]
    c = _decode(geom, name, 0)
    x = _Dec(oracle, dev, c, bshd, hkv)
    b = len(c.valid)
    ws = ops.decode_attn_workspace(b, 1, h, d, x.max_len, dev)
    ws.fill_(float("nan"))                                      # nothing stale may be read
    if form == "prefix":
        ops.decode_attention_splits(x.q, x.lens, x.ka, x.va, x.valid, c.scale, x.max_len, hkv, ws, bshd=bshd)
        att = ops.decode_attention_combine_h(ws, x.lens, x.valid, b, h, hkv, x.max_len)
    else:
        ops.decode_attention_splits_mask(x.q, x.lens, x.ka, x.va, x.mask, c.scale, x.max_len, hkv, ws, bshd=bshd)
        att = ops.decode_attention_combine_h(ws, x.lens, None, b, h, hkv, x.max_len)
    # bar: test_attention_mask_form_split_records_merge ((1e-3 + 2^-10) * max(1, max|exact|): the records pass through fp16 once)
    _report(f"half_records_{form}", name, 0, bshd, _vals(att, 0), x.exact, ap.half_record_bar(x.exact))


# ---- route 7: the INT8 KV cache -----------------------------------------------------------------------------------------------------
Q8_ROUTES = [("q8_valu_d64", "d64", 0), ("q8_valu_d64", "d64", 1), ("q8_mfma_h8", "h8", 0), ("q8_mfma_h16_q4", "h16_q4", 0)]


@pytest.mark.parametrize("bshd", LAYOUT)
@pytest.mark.parametrize("name", ap.PROFILES)
@pytest.mark.parametrize("route,geom,dtype", Q8_ROUTES, ids=[f"{r[0]}-{'bf16' if r[2] else 'fp16'}" for r in Q8_ROUTES])
def test_int8_cache_attention_on_score_profiles(oracle, dev, route, geom, dtype, name, bshd):
    """the built rows quantised by the project's row quantiser (the oracle's, bit for bit the device's: test_quant_calc_scale_zp_bit_exact),
    every score evaluated on the dequantised values; d = 64: the VALU kernel with a mask (hidden_spike: with holes), d = 128: the
    matrix-core kernel's prefix form"""
    from zhilight_amd import ops
    masked = geom == "d64"
    if masked and name == "hidden_spike":
        geom = "d64_holes"
    d, h, hkv, len_q, _ = ap.DECODE_GEOMS[geom]
    c = ap.decode_case(geom, name, dtype, quant=lambda r: oracle.quant_calc_scale_zp(r, dtype=dtype))
    lens_np = np.array(c.buf_lens, np.int32)
    host = [_lay(a, bshd) for a in (c.k, c.v, c.ks, c.vs)]
    exact = oracle.mqa_rag_buffer_quant(c.q, lens_np, *host, c.mask, hkv, c.scale, bshd, dtype=dtype)
    assert np.abs(exact - c.ref).max() <= 1e-6 * max(1.0, np.abs(c.ref).max())
    devt = [[_t(a, dev) for a in arrs] for arrs in host]
    got = ops.multi_query_attention_rag_buffer_quant(_dev_bits(c.q, dev, dtype), _t(lens_np, dev), *[ops.make_ptr_table(t) for t in devt],
                                                     _t(c.mask, dev) if masked else None, c.scale, max(c.buf_lens), hkv,
                                                     valid_lens=None if masked else _t(np.array(c.valid, np.int32), dev), bshd=bshd)
    # bar: test_decode_attention_quant / _quant_matrix_core_path (1e-3), test_decode_attention_quant_valid_lens_bf16_and_garbage_tail (bf16 5e-3)
    _report(route, name, dtype, bshd, _vals(got, dtype), exact, ap.decode_bar(exact, dtype))


# ---- route 8: more than 16 splits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", ["stairs", "late_spike"])
@pytest.mark.parametrize("form", ["mfma_prefix", "valu_mask"])
def test_many_splits_on_score_profiles(oracle, dev, monkeypatch, form, name, dtype):
    """one task, 4161 visible keys of 4224: 33 splits of 128 keys (the merge's ns > 16 form), 4-wave workgroups"""
    from zhilight_amd import ops
    geom = "h8" if form == "mfma_prefix" else "h8_holes"
    d, h, hkv, len_q, _ = ap.DECODE_GEOMS[geom]
    assert ops.decode_attn_split_len(1, hkv, ap.LONG_BUF) == 128
    if form == "valu_mask":
        monkeypatch.setenv("ZL_ATTN_MFMA", "0")
    c = _decode(geom, name, dtype, True)
    x = _Dec(oracle, dev, c, True, hkv)
    got = ops.multi_query_attention_rag_buffer(x.q, x.lens, x.ka, x.va, x.mask if form == "valu_mask" else None, c.scale, x.max_len, hkv,
                                               valid_lens=x.valid if form == "mfma_prefix" else None)
    # bar: test_decode_attention_matrix_core_path
    _report(f"splits33_{form}", name, dtype, True, _vals(got, dtype), x.exact, ap.decode_bar(x.exact, dtype))


# ---- route 9: prefill_attention -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", ap.PROFILES)
@pytest.mark.parametrize("geom", list(ap.PREFILL_GEOMS))
@pytest.mark.parametrize("groups", [1, 2, 4, 0])
def test_prefill_attention_on_score_profiles(oracle, dev, groups, geom, name, dtype):
    """row i sees the keys 0 .. pos0 + i of a profile laid over 0 .. pos0 + s_q - 1: under `rise` every row's maximum is its own last key,
    inside the diagonal tile; late_spike's spike is the chunk's last key (the last row's); under hidden_spike the slots behind the
    chunk -- the rest of the last diagonal tile -- are finite and 125 above.  Rows of one 16-row tile have gains 1, -1, 0, 0.5, ..."""
    from zhilight_amd import ops
    s_q, pos0, h, hkv = ap.PREFILL_GEOMS[geom]
    c = _prefill(geom, name, dtype)
    exact = oracle.mqa_rag_buffer(c.q[None], np.array([c.len_buf], np.int32), [c.k], [c.v], c.mask, hkv, c.scale, True, dtype=dtype, exact=True)[0]
    assert np.abs(exact - c.ref).max() <= 1e-6
    got = ops.prefill_attention(_dev_bits(c.q, dev, dtype), _dev_bits(c.k, dev, dtype), _dev_bits(c.v, dev, dtype), pos0, hkv, c.scale, True, groups=groups)
    # bar: test_prefill_attention (2e-3, bf16 1.5e-2 of max|ref|)
    _report(f"prefill_{geom}_g{groups}", name, dtype, True, _vals(got, dtype), exact, ap.prefill_bar(exact, dtype))


# ---- route 10: MLA decode attention -------------------------------------------------------------------------------------------------
MLA_ROUTES = [("h16", 0), ("h16", 1), ("h20", 0), ("h128_b3", 2), ("h128_b32", 0)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", ap.PROFILES)
@pytest.mark.parametrize("geom,algo", MLA_ROUTES, ids=[f"{g}_algo{a}" for g, a in MLA_ROUTES])
def test_mla_attention_on_score_profiles(oracle, dev, geom, algo, name, dtype):
    """h = 16 on the matrix-core and the VALU kernel, h = 20 (a ragged head group), the wide kernel at 3 tasks, and 32 tasks x 128 heads
    over 1088-slot buffers: 256 head groups, ONE split, no combine launch -- with a task without keys, whose rows must be zero there
    too.  Reference: the oracle's flavour E (the fp64 statement rounded once to T); at 128 heads the numpy fp64 statement itself,
    which test_attn_profiles_host.py holds within half an ulp of E."""
    from zhilight_amd import ops
    h, buf, vis = ap.MLA_GEOMS[geom]
    c = ap.mla_case(geom, name, dtype)
    b = len(vis)
    dbufs = [_dev_bits(a, dev, dtype) for a in c.kv]
    addrs = torch.tensor([t.data_ptr() for t in dbufs], dtype=torch.int64, device=dev)
    buf_lens = torch.tensor([buf] * b, dtype=torch.int32, device=dev)
    valid = torch.tensor(vis, dtype=torch.int32, device=dev)
    got = ops.mla_decode_attention(_dev_bits(c.q, dev, dtype), buf_lens, addrs, ap.MLA_SCALE, buf, valid, algo=algo)
    g = _vals(got, dtype)
    if h <= 20:
        E = ap.from_bits(oracle.mla_decode_attn(c.q, [buf] * b, vis, c.kv, scale=ap.MLA_SCALE, dtype=dtype, flavour="E"), dtype)
    else:
        E = c.ref
    assert np.isfinite(g).all()
    for t, n in enumerate(vis):
        if n == 0:
            assert not g[t].any()                                # a task without keys: zero rows on every route
    # bar: test_mla_decode_attention_over_the_latent_cache (ulp * |E| + 2e-5 * max|E|, elementwise)
    bar = ap.mla_bar(E, dtype)
    ratio = (np.abs(g - E) / bar).max()
    print(f"ATTNPROF mla_{geom}_algo{algo} {name} {'bf16' if dtype else 'fp16'} - {ratio:.4f}")
    assert ratio <= 1.0, (geom, algo, name, ratio)
