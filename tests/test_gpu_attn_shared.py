"""zl_decode_attn_shared (two-segment decode attention: a prompt's K / V rows shared between tasks) through ops and the C ABI, against
tests/shared_ref.py (fp64) and against zl_decode_attn on buffers that hold the prefix as a copy.

Random normal fp16 / bf16 data, BSHD and BHSD.  Every row the rule says is unread is NaN: own rows below P, own rows from `valid` on,
prefix rows from prefix_lens on.  `out` and the workspace sit between poisoned guards.

Bars.  attn_profiles.decode_bar against shared_ref: the kernel is k_decode_attn_mfma's chunk body and k_decode_attn_combine's merge
arithmetic, only with more records per row.  A float32 restatement of the two-segment merge (shared_ref.restate_f32: an online softmax
per split of either segment + one merge; tests/test_shared_host.py) stays below 0.4 of that bar at these shapes.  Against zl_decode_attn on materialised buffers:
twice decode_bar (two kernels, each within one bar of the exact result), as tests/test_gpu_spec_attn.py does for its two routes."""
import ctypes as C

import numpy as np
import pytest
import torch

import shared_ref
from attn_profiles import decode_bar, from_bits, to_bits

pytestmark = pytest.mark.gpu

D = 128
SCALE = 1.0 / np.sqrt(D)
GUARD = 512                     # elements on either side of out and of the workspace
OUT_POISON, WS_POISON = 0x7b7b, 12345.0

# name -> h, hkv, caps, prefix_lens, prefix_of, valid, buf_lens, max_len_buf (None: max(buf_lens))
CASES = {
    "mixed-8-2": (8, 2, (96, 64), (70, 33), [0, 0, -1, 1, 0], [71, 115, 50, 233, 73], [128, 128, 64, 256, 80], None),
    "mixed-32-8": (32, 8, (96, 64), (70, 33), [0, 0, -1, 1, 0], [71, 115, 50, 233, 73], [128, 128, 64, 256, 80], None),
    # nine members of one prefix: 36 rows = tiles of 16, 16, 4
    "many-rows": (8, 2, (96,), (70,), [0] * 9, [71, 80, 75, 90, 100, 71, 128, 77, 99], [128] * 9, None),
    # n_rep 1: every row of a tile belongs to another task (18 members: tiles of 16 and 2)
    "n-rep-1": (4, 4, (64,), (45,), [0] * 18, [46 + 3 * i for i in range(18)], [128] * 18, None),
    # several splits on both sides
    "long": (8, 2, (1152,), (1100,), [0, 0, 0], [1101, 1164, 1800], [2048, 1280, 2048], 2048),
    # prefix_lens 0; valid == P; prefix_of = G and = -7; prefix_lens > cap; a task with valid 0; valid < prefix_lens; valid > buf_len
    "edges": (8, 2, (64, 48, 32), (0, 60, 20), [0, 1, 3, -7, 1, 2, 1, 1, 2], [40, 48, 33, 20, 90, 20, 0, 30, 70],
              [64, 64, 64, 32, 128, 64, 64, 64, 40], None),
}


def _nan(dtype):
    return np.uint16(0x7fc0 if dtype else 0x7e00)


def _rand_bits(rng, shape, dtype):
    return to_bits(rng.standard_normal(shape), dtype)


class Case:
    """the operands of one call, as uint16 bit arrays on the host (what is unread poisoned with NaN) and tensors on the device"""

    def __init__(self, dev, rng, dtype, bshd, h, hkv, caps, plens, prefix_of, valid, buf_lens, max_len_buf=None, poison=True):
        self.dev, self.dtype, self.bshd, self.h, self.hkv = dev, dtype, bshd, h, hkv
        self.tdt = torch.bfloat16 if dtype else torch.float16
        self.caps, self.plens, self.prefix_of, self.valid, self.buf_lens = list(caps), list(plens), list(prefix_of), list(valid), list(buf_lens)
        self.b, self.g = len(valid), len(caps)
        self.max_prefix_len, self.max_len_buf = max(caps), max_len_buf or max(buf_lens)
        shape = (lambda n: (n, hkv, D)) if bshd else (lambda n: (hkv, n, D))
        self.pk, self.pv = [_rand_bits(rng, shape(c), dtype) for c in caps], [_rand_bits(rng, shape(c), dtype) for c in caps]
        self.ok, self.ov = [_rand_bits(rng, shape(n), dtype) for n in buf_lens], [_rand_bits(rng, shape(n), dtype) for n in buf_lens]
        self.q = _rand_bits(rng, (self.b, h, D), dtype)
        if poison:
            ps = shared_ref.prefix_rows(prefix_of, plens, caps, valid, buf_lens)
            for g in range(self.g):
                for a in (self.pk[g], self.pv[g]):
                    self._rows(a, max(0, min(plens[g], caps[g])), caps[g])[...] = _nan(dtype)
            for b in range(self.b):
                for a in (self.ok[b], self.ov[b]):
                    self._rows(a, 0, ps[b])[...] = _nan(dtype)
                    self._rows(a, max(ps[b], min(valid[b], buf_lens[b])), buf_lens[b])[...] = _nan(dtype)
        self.upload()

    def _rows(self, a, lo, hi):
        return a[lo:hi] if self.bshd else a[:, lo:hi]

    def _t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(self.dev).view(self.tdt)

    def upload(self):
        from zhilight_amd import ops
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.dev)                     # noqa: E731
        self.d_pk, self.d_pv = [self._t(a) for a in self.pk], [self._t(a) for a in self.pv]
        self.d_ok, self.d_ov = [self._t(a) for a in self.ok], [self._t(a) for a in self.ov]
        self.pk_tab, self.pv_tab = ops.make_ptr_table(self.d_pk), ops.make_ptr_table(self.d_pv)
        self.k_tab, self.v_tab = ops.make_ptr_table(self.d_ok), ops.make_ptr_table(self.d_ov)
        self.d_q = self._t(self.q)
        self.d_buf_lens, self.d_valid, self.d_prefix_of = i32(self.buf_lens), i32(self.valid), i32(self.prefix_of)
        self.d_plens, self.d_caps = i32(self.plens), i32(self.caps)

    def values(self, arrays):
        return [from_bits(a, self.dtype).reshape(a.shape) for a in arrays]

    def exact(self):
        q = from_bits(self.q, self.dtype).reshape(self.q.shape)
        return shared_ref.shared_attention(q, self.values(self.ok), self.values(self.ov), self.valid, self.buf_lens, self.prefix_of,
                                           self.plens, self.caps, self.values(self.pk), self.values(self.pv), self.hkv, SCALE, self.bshd)

    def run(self, guarded=True, **kw):
        """the call through ops -> (values fp64 (B, H, D), bits); guarded: out and the workspace between poisoned guards, checked"""
        from zhilight_amd import ops
        n_out = self.b * self.h * D
        need = ops.decode_attn_shared_workspace_bytes(self.b, self.g, self.h, self.hkv, D, self.max_prefix_len, self.max_len_buf) // 4
        out_big = torch.full((n_out + 2 * GUARD,), OUT_POISON, dtype=torch.int16, device=self.dev)
        ws_big = torch.full((need + 2 * GUARD,), WS_POISON, dtype=torch.float32, device=self.dev)
        out = out_big[GUARD:GUARD + n_out].view(self.tdt).view(self.b, self.h, D)
        ops.decode_attention_shared(self.d_q, self.d_buf_lens, self.k_tab, self.v_tab, self.d_valid, self.d_prefix_of, self.d_plens, self.d_caps,
                                    self.pk_tab, self.pv_tab, SCALE, self.max_prefix_len, self.max_len_buf, self.hkv, bshd=self.bshd, out=out,
                                    workspace=ws_big[GUARD:GUARD + need], **kw)
        torch.cuda.synchronize()
        if guarded:
            assert (out_big[:GUARD] == OUT_POISON).all() and (out_big[GUARD + n_out:] == OUT_POISON).all()
            assert (ws_big[:GUARD] == WS_POISON).all() and (ws_big[GUARD + need:] == WS_POISON).all()
        bits = out.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        return from_bits(bits, self.dtype).reshape(bits.shape), bits

    def materialised(self):
        """zl_decode_attn(mask = NULL, valid_lens) over buffers that hold each task's prefix as a copy -> values (B, H, D)"""
        from zhilight_amd import ops
        mk = shared_ref.materialise(self.ok, self.valid, self.buf_lens, self.prefix_of, self.plens, self.caps, self.pk, self.bshd, fill=0)
        mv = shared_ref.materialise(self.ov, self.valid, self.buf_lens, self.prefix_of, self.plens, self.caps, self.pv, self.bshd, fill=0)
        dk, dv = [self._t(a) for a in mk], [self._t(a) for a in mv]
        out = ops.multi_query_attention_rag_buffer(self.d_q.view(self.b, 1, self.h, D), self.d_buf_lens, ops.make_ptr_table(dk),
                                                   ops.make_ptr_table(dv), None, SCALE, self.max_len_buf, self.hkv,
                                                   valid_lens=self.d_valid, bshd=self.bshd)
        bits = out.view(torch.int16).cpu().numpy().view(np.uint16)
        return from_bits(bits, self.dtype).reshape(self.b, self.h, D)


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("bshd", [True, False], ids=["bshd", "bhsd"])
@pytest.mark.parametrize("name", list(CASES))
def test_shared_attention_against_the_rule(dev, name, bshd, dtype):
    """within decode_bar of shared_ref, within twice that of zl_decode_attn on materialised buffers; NaN in every unread row; guards"""
    h, hkv, caps, plens, prefix_of, valid, buf_lens, max_len_buf = CASES[name]
    case = Case(dev, np.random.default_rng(7), dtype, bshd, h, hkv, caps, plens, prefix_of, valid, buf_lens, max_len_buf)
    exact = case.exact()
    got, _ = case.run()
    assert got.shape == exact.shape and np.isfinite(got).all()
    bar = decode_bar(exact, dtype)
    err = np.abs(got - exact).reshape(case.b, -1).max(axis=1)
    twin = np.abs(got - case.materialised()).max()
    print("max |got - exact| per task:", err, "bar", bar, "vs zl_decode_attn on copies:", twin)
    assert err.max() < bar, err
    assert twin < 2 * bar
    for b in range(case.b):                                          # a task without a visible key: a zero row
        if min(valid[b], buf_lens[b]) <= 0:
            assert not got[b].any()


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])
def test_explicit_split_lengths(dev, dtype):
    """_ex's split lengths: other splits on either side, the same bar"""
    h, hkv, caps, plens, prefix_of, valid, buf_lens, max_len_buf = CASES["long"]
    case = Case(dev, np.random.default_rng(8), dtype, True, h, hkv, caps, plens, prefix_of, valid, buf_lens, max_len_buf)
    exact = case.exact()
    for sh, own in ((128, 128), (160, 224), (1152, 2048)):
        got, _ = case.run(shared_split_len=sh, own_split_len=own)
        err = np.abs(got - exact).max()
        print(sh, own, err, decode_bar(exact, dtype))
        assert err < decode_bar(exact, dtype)


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("h,hkv", [(8, 2), (4, 4)])
def test_member_independence(dev, h, hkv, dtype):
    """a member's output bits do not change with the number of other members of its prefix (1 against 9; same b, same launch
    arguments), nor with its slot index"""
    b = 10
    valid, buf_lens = [71 + 5 * i for i in range(b)], [128] * b
    full = Case(dev, np.random.default_rng(9), dtype, True, h, hkv, (96,), (70,), [0] * 9 + [-1], valid, buf_lens, poison=False)
    _, bits9 = full.run()
    for member in (0, 4, 8):
        alone = Case(dev, np.random.default_rng(9), dtype, True, h, hkv, (96,), (70,), [0 if i == member else -1 for i in range(b)], valid,
                     buf_lens, poison=False)
        _, bits1 = alone.run()
        assert np.array_equal(bits1[member], bits9[member])
    # slot 0's task moved to slot 7: operands swapped, tables swapped
    moved = Case(dev, np.random.default_rng(9), dtype, True, h, hkv, (96,), (70,), [0] * 9 + [-1], valid, buf_lens, poison=False)
    for arr in (moved.ok, moved.ov, moved.valid):
        arr[0], arr[7] = arr[7], arr[0]
    moved.q[[0, 7]] = moved.q[[7, 0]]
    moved.upload()
    _, bits_m = moved.run()
    assert np.array_equal(bits_m[7], bits9[0]) and np.array_equal(bits_m[0], bits9[7])


def test_graph_replay_follows_the_tables(dev):
    """a captured call replayed after prefix_of, prefix_lens and valid_lens were rewritten in place gives the eager call's bits"""
    from zhilight_amd import ops
    h, hkv, b = 8, 2, 6
    buf_lens = [160] * b
    first = dict(plens=(70, 33), prefix_of=[0, 0, -1, 1, 0, 1], valid=[71, 115, 50, 140, 73, 34])
    second = dict(plens=(64, 50), prefix_of=[1, -1, 0, 0, 0, 2], valid=[90, 30, 65, 160, 100, 77])
    case = Case(dev, np.random.default_rng(10), 0, True, h, hkv, (96, 64), first["plens"], first["prefix_of"], first["valid"], buf_lens,
                poison=False)
    out = torch.empty_like(case.d_q)
    ws = ops.decode_attn_shared_workspace(b, 2, h, hkv, D, case.max_prefix_len, case.max_len_buf, dev)

    def call(o):
        return ops.decode_attention_shared(case.d_q, case.d_buf_lens, case.k_tab, case.v_tab, case.d_valid, case.d_prefix_of, case.d_plens,
                                           case.d_caps, case.pk_tab, case.pv_tab, SCALE, case.max_prefix_len, case.max_len_buf, hkv, out=o,
                                           workspace=ws)
    call(out)                                                        # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(out)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    case.d_plens.copy_(i32(second["plens"]))
    case.d_prefix_of.copy_(i32(second["prefix_of"]))
    case.d_valid.copy_(i32(second["valid"]))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = call(torch.empty_like(case.d_q))
    assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
    case.plens, case.prefix_of, case.valid = list(second["plens"]), second["prefix_of"], second["valid"]
    exact = case.exact()
    got = from_bits(out.view(torch.int16).cpu().numpy().view(np.uint16), 0).reshape(exact.shape)
    assert np.abs(got - exact).max() < decode_bar(exact, 0)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp16", "bf16"])
def test_prompt_attention_on_a_history(dev, dtype, groups):
    """zl_prefill_attn_varlen_hist equals zl_prefill_attn_varlen on buffers that hold history and own rows, bit for bit; history rows
    from pos0 on are NaN (never read), a task without history has no history buffer at all"""
    from zhilight_amd import ops
    rng = np.random.default_rng(12)
    h, hkv = 8, 2
    tdt = torch.bfloat16 if dtype else torch.float16
    pos0, lens, hist_lens, buf_lens = [0, 50, 130], [5, 70, 17], [0, 64, 130], [64, 160, 192]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev).view(tdt)     # noqa: E731
    total = sum(lens)
    q, k_new, v_new = (_rand_bits(rng, (total, n, D), dtype) for n in (h, hkv, hkv))
    hist_k, hist_v = ([_rand_bits(rng, (n, hkv, D), dtype) for n in hist_lens] for _ in range(2))
    full_k, full_v = [], []
    row = 0
    for i, (p0, n, cap) in enumerate(zip(pos0, lens, buf_lens)):
        for full, hist, new in ((full_k, hist_k, k_new), (full_v, hist_v, v_new)):
            buf = np.full((cap, hkv, D), _nan(dtype), np.uint16)
            buf[:p0] = hist[i][:p0]
            buf[p0:p0 + n] = new[row:row + n]
            full.append(buf)
            hist[i][p0:] = _nan(dtype)
        row += n
    d_q, d_kn, d_vn = t(q), t(k_new), t(v_new)
    d_fk, d_fv = [t(a) for a in full_k], [t(a) for a in full_v]
    d_hk, d_hv = [t(a) for a in hist_k[1:]], [t(a) for a in hist_v[1:]]
    null = torch.zeros(1, dtype=torch.int64, device=dev)
    hk_tab, hv_tab = torch.cat([null, ops.make_ptr_table(d_hk)]), torch.cat([null, ops.make_ptr_table(d_hv)])
    ref = ops.prefill_attention_varlen(d_q, lens, pos0, ops.make_ptr_table(d_fk), ops.make_ptr_table(d_fv), buf_lens, hkv, SCALE, groups=groups)
    got = ops.prefill_attention_varlen_hist(d_q, lens, pos0, d_kn, d_vn, hk_tab, hv_tab, hist_lens, buf_lens, hkv, SCALE, groups=groups)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    for bad in (dict(hist_lens=[0, 49, 130]), dict(hist_lens=[0, 64]), dict(k_new=d_kn[:-1]), dict(hk=hk_tab[:2]), dict(q=d_q.float())):
        a = dict(q=d_q, k_new=d_kn, hk=hk_tab, hist_lens=hist_lens)
        a.update(bad)
        with pytest.raises(ops.ZLError):
            ops.prefill_attention_varlen_hist(a["q"], lens, pos0, a["k_new"], d_vn, a["hk"], hv_tab, a["hist_lens"], buf_lens, hkv, SCALE)


def test_refusals_before_any_launch(dev):
    """ops raises ZLError and the C entries answer with their codes; the guards of out and of the workspace stay intact"""
    from zhilight_amd import _lib, ops
    h, hkv, caps, plens, prefix_of, valid, buf_lens, _ = CASES["mixed-8-2"]
    case = Case(dev, np.random.default_rng(11), 0, True, h, hkv, caps, plens, prefix_of, valid, buf_lens)
    case.run()                                                       # the operands are good

    def call(**kw):
        a = dict(q=case.d_q, buf_lens=case.d_buf_lens, valid=case.d_valid, prefix_of=case.d_prefix_of, plens=case.d_plens, caps=case.d_caps,
                 hkv=hkv, workspace=None, sh=0, own=0)
        a.update(kw)
        return ops.decode_attention_shared(a["q"], a["buf_lens"], case.k_tab, case.v_tab, a["valid"], a["prefix_of"], a["plens"], a["caps"],
                                           case.pk_tab, case.pv_tab, SCALE, case.max_prefix_len, case.max_len_buf, a["hkv"],
                                           workspace=a["workspace"], shared_split_len=a["sh"], own_split_len=a["own"])
    call()
    for bad in (dict(q=case.d_q.float()), dict(q=case.d_q[:, :, :64].contiguous()), dict(hkv=3), dict(q=case.d_q.view(1, case.b, h, D)),
                dict(valid=case.d_valid.long()), dict(prefix_of=case.d_prefix_of[:2]), dict(caps=case.d_caps[:1]),
                dict(buf_lens=case.d_buf_lens.cpu()), dict(workspace=torch.zeros(16, dtype=torch.float32, device=dev)), dict(sh=100),
                dict(own=64), dict(q=torch.zeros((case.b, 34, D), dtype=torch.float16, device=dev), hkv=2)):
        with pytest.raises(ops.ZLError):
            call(**bad)
    # the C entries, with out and the workspace between guards
    n_out = case.b * h * D
    need = ops.decode_attn_shared_workspace_bytes(case.b, 2, h, hkv, D, case.max_prefix_len, case.max_len_buf) // 4
    out_big = torch.full((n_out + 2 * GUARD,), OUT_POISON, dtype=torch.int16, device=dev)
    ws_big = torch.full((need + 2 * GUARD,), WS_POISON, dtype=torch.float32, device=dev)
    p, i64 = ops._p, C.c_int64

    def centry(b=case.b, g=2, hh=h, kv=hkv, d=D, mp=case.max_prefix_len, ml=case.max_len_buf, dtype=0, sh=0, own=0, q=case.d_q):
        return _lib.lib().zl_decode_attn_shared_ex(
            p(q), p(case.d_buf_lens), p(case.k_tab), p(case.v_tab), p(case.d_valid), p(case.d_prefix_of), p(case.d_plens), p(case.d_caps),
            p(case.pk_tab), p(case.pv_tab), p(out_big[GUARD:]), p(ws_big[GUARD:]), i64(b), i64(g), i64(hh), i64(kv), i64(d),
            C.c_float(SCALE), i64(mp), i64(ml), C.c_int(1), C.c_int(dtype), i64(sh), i64(own), None)
    einval, eshape, edtype, elimit = -1, -2, -3, -4
    assert centry(q=None) == einval and centry(b=0) == einval and centry(g=0) == einval and centry(mp=0) == einval
    assert centry(sh=100) == einval and centry(own=96) == einval and centry(sh=-128) == einval and centry(own=-128) == einval
    assert centry(kv=3) == eshape and centry(d=64) == eshape and centry(hh=34, kv=2) == eshape
    assert centry(dtype=2) == edtype
    assert centry(sh=128, own=128, mp=40000, ml=40000) == elimit      # 626 record slots, the merge holds 512
    assert centry(b=70000) == elimit
    assert centry(kv=3, dtype=2) == eshape                            # the order of the checks
    assert _lib.lib().zl_decode_attn_shared_workspace_bytes(i64(0), i64(1), i64(8), i64(2), i64(128), i64(64), i64(64)) == einval
    torch.cuda.synchronize()
    assert (out_big == OUT_POISON).all() and (ws_big == WS_POISON).all()
