"""Host-side pieces of the device sampler: the Philox4x32-10 of tests/sample_ref.py against the Random123 known answers, the
sampling rule's invariants on hand cases, the kernel's sort-free procedure against the sorting rule, and every argument check of
ops.sample_advance and LLaMA.new_sampler that needs no device."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import sample_ref


def test_philox_known_answers():
    kat = [
        ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ]
    for ctr, key, expect in kat:
        assert " ".join(f"{w:08x}" for w in sample_ref.philox4x32_10(ctr, key)) == expect


def test_uniforms():
    u = sample_ref.uniforms([0, 0, -1, 5 + (7 << 32)], [0, 1, (1 << 64) - 1, 3 + (9 << 32)])
    assert u.dtype == np.float32 and ((u >= 0) & (u < 1)).all()
    assert u[0] == np.float32((0x6627E8D5 >> 8) * 2.0 ** -24)
    assert u[1] == np.float32((sample_ref.philox4x32_10([1, 0, 0, 0], [0, 0])[0] >> 8) * 2.0 ** -24)
    # the halves of seed and counter land where the kernel puts them
    assert u[3] == np.float32((sample_ref.philox4x32_10([3, 9, 0, 0], [5, 7])[0] >> 8) * 2.0 ** -24)
    assert u[2] == np.float32((sample_ref.philox4x32_10([0xFFFFFFFF, 0xFFFFFFFF, 0, 0], [0xFFFFFFFF] * 2)[0] >> 8) * 2.0 ** -24)
    assert len(set(sample_ref.uniforms([3] * 64, range(64)).tolist())) > 60


def test_rule_invariants():
    rng = np.random.default_rng(3)
    last = np.float32(1 - 2.0 ** -24)
    for n in (1, 2, 7, 64, 1000):
        for _ in range(20):
            x = rng.standard_normal(n).astype(np.float16).astype(np.float64) * 2
            x[rng.integers(0, n)] = x.max()                                 # a tied maximum now and then
            am = int(np.argmax(x))
            for u in (0.0, 0.37, last):
                assert sample_ref.sample(x, 0.0, 0, 1.0, u)[0] == am        # T <= 0
                assert sample_ref.sample(x, 0.8, 1, 1.0, u)[0] == am        # top_k = 1
                assert sample_ref.sample(x, 0.8, 0, 0.0, u)[0] == am        # top_p = 0
                assert 0 <= sample_ref.sample(x, 1.3, 5, 0.9, u)[0] < n
            assert sample_ref.sample(x, 0.8, 40, 0.9, 0.0)[0] == am         # u = 0
    # ties go to the lower index; -0.0 and +0.0 are one value
    x = np.array([1.0, 3.0, 3.0, -0.0, 0.0, 3.0])
    pick, pos, c, v, order = sample_ref.sample(x, 1.0, 0, 1.0, 0.5)
    assert order.tolist() == [1, 2, 5, 0, 3, 4] and pick == order[pos] and c[pos] >= v and (pos == 0 or c[pos - 1] < v)
    # a masked class is never picked, whatever u; the fallback is the last class with p > 0
    x = np.array([-np.inf, 0.5, -np.inf, 0.25, -np.inf])
    for u in (0.0, 0.5, last, 1.0):
        assert sample_ref.sample(x, 1.0, 0, 1.0, u)[0] in (1, 3)
        assert sample_ref.sample(x, 1.0, 4, 1.0, u)[0] in (1, 3)
    # all-equal rows: the ceil(u * cap * n)-th class in index order
    for n in (5, 64):
        x = np.full(n, 0.75)
        for top_k, top_p, u in ((0, 1.0, 0.5), (3, 1.0, 0.9), (0, 0.5, 0.7), (0, 1.0, float(last)), (2, 0.25, 0.99)):
            cap = min(top_p, top_k / n) if 0 < top_k < n else top_p
            assert sample_ref.sample(x, 1.0, top_k, top_p, u)[0] == max(math.ceil(u * cap * n), 1) - 1
    # NaN / +inf / all -inf rows: the arg-max, NaN largest
    assert sample_ref.sample(np.array([1.0, np.nan, 5.0, np.nan]), 1.0, 0, 1.0, 0.9)[0] == 1
    assert sample_ref.sample(np.array([1.0, np.inf, 5.0, np.inf]), 1.0, 0, 1.0, 0.9)[0] == 1
    assert sample_ref.sample(np.full(4, -np.inf), 1.0, 0, 1.0, 0.9)[0] == 0
    # probabilities() is the distribution of sample() over u
    x = rng.standard_normal(12)
    pr = sample_ref.probabilities(x, 0.9, 5, 0.8)
    us = (np.arange(20000) + 0.5) / 20000
    freq = np.bincount([sample_ref.sample(x, 0.9, 5, 0.8, u)[0] for u in us], minlength=12) / us.size
    assert abs(pr.sum() - 1) < 1e-12 and np.abs(freq - pr).max() < 1e-4
    assert abs(sample_ref.logprob(x, 0.0, 3) - (x[3] - np.log(np.exp(x).sum()))) < 1e-12


def _rows(rng, n, kind, bf16):
    if kind == "ties":
        x = rng.choice(np.array([-1.5, 0.0, 0.25, 2.0]), n)
    else:
        x = rng.standard_normal(n) * kind
    if bf16:
        return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    bits = x.astype(np.float16).view(np.uint16).copy()
    bits[(bits & 0x7FFF) == 0] = rng.choice(np.array([0, 0x8000], np.uint16), int(((bits & 0x7FFF) == 0).sum()))   # both zeros
    return bits


def test_sort_free_procedure_equals_the_sorting_rule():
    """the kernel's procedure: exactly the sorting rule over the same integer masses, and the float64 rule's pick up to the fixed
    point's resolution (2^-45 of the largest probability at 128 k classes: equal in at least 98 % of the cases, and always within the
    GPU test's mass tolerance)"""
    rng = np.random.default_rng(17)
    last = float(np.float32(1 - 2.0 ** -24))
    cases = equal = 0
    for n in (1, 2, 7, 65, 257, 1025, 4097):
        for kind in (0.05, 0.5, 2, 8, "ties"):
            for bf16 in (False, True):
                bits = _rows(rng, n, kind, bf16)
                if n > 7:
                    bits[rng.random(n) < 0.3] = 0xFC00 if not bf16 else 0xFF80             # -inf masks
                    bits[rng.integers(0, n)] = 0x3C00 if not bf16 else 0x3F80              # at least one finite class
                x = sample_ref.values_of(bits, bf16)
                for _ in range(3):
                    T = float(rng.choice([0.3, 0.7, 1.0, 1.5]))
                    top_k = int(rng.choice([0, 1, 2, 5, 40, n - 1, n + 7]))
                    top_p = float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0]))
                    u = float(rng.choice([0.0, last, float(np.float32(rng.random()))]))
                    got = sample_ref.sample_sort_free(bits, bf16, T, top_k, top_p, u)
                    assert got == sample_ref.sample_sorted_fixed(bits, bf16, T, top_k, top_p, u), (n, kind, bf16, T, top_k, top_p, u)
                    pick, pos, c, v, order = sample_ref.sample(x, T, top_k, top_p, u)
                    gpos = int(np.flatnonzero(order == got)[0])
                    tol = 2.0 ** -15 * c[-1]
                    assert (c[gpos - 1] if gpos else 0.0) - tol <= v <= c[gpos] + tol
                    assert x[got] > -np.inf
                    cases += 1
                    equal += got == pick
    print(f"sort-free == float64 rule in {equal} of {cases} cases")
    assert equal >= 0.98 * cases


def test_sample_advance_argument_checks():
    """every ZLError of ops.sample_advance that is decided before a device is touched, each by its own message; the host tensors
    used here are refused LAST, so a deleted check surfaces as the wrong message"""
    from zhilight_amd import ops
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    logits = torch.zeros((2, 8), dtype=torch.float16)
    t, k, p = torch.ones(2, dtype=f32), torch.zeros(2, dtype=i32), torch.ones(2, dtype=f32)
    seeds, draws, u = torch.zeros(2, dtype=i64), torch.zeros(2, dtype=i64), torch.zeros(2, dtype=f32)
    tok = torch.zeros(2, dtype=i32)
    bad = [
        (dict(logits=logits.tolist()), "are tensors"),
        (dict(temperature=[1.0, 1.0]), "are tensors"),
        (dict(top_k=[0, 0]), "are tensors"),
        (dict(top_p=1.0), "are tensors"),
        (dict(logits=logits.view(-1)), "unit column stride"),
        (dict(logits=torch.zeros((2, 16), dtype=torch.float16)[:, ::2]), "unit column stride"),
        (dict(logits=torch.zeros((8, 2), dtype=torch.float16).t()), "unit column stride"),
        (dict(logits=torch.zeros((0, 8), dtype=torch.float16)), "unit column stride"),
        (dict(logits=torch.zeros((2, 0), dtype=torch.float16)), "unit column stride"),
        (dict(logits=logits.float()), "fp16 or bf16"),
        (dict(logits=logits.double()), "fp16 or bf16"),
        (dict(logits=torch.empty((1, 1 << 31), dtype=torch.float16, device="meta")), "fewer than 2\\^31"),
        (dict(temperature=t.double()), "temperature:"),
        (dict(temperature=torch.ones(3, dtype=f32)), "temperature:"),
        (dict(temperature=torch.ones(4, dtype=f32)[::2]), "temperature:"),
        (dict(temperature=torch.ones((2, 1), dtype=f32)), "temperature:"),
        (dict(top_k=k.to(i64)), "top_k:"),
        (dict(top_k=torch.zeros(1, dtype=i32)), "top_k:"),
        (dict(top_p=p.half()), "top_p:"),
        (dict(top_p=torch.ones(3, dtype=f32)), "top_p:"),
        (dict(seeds=None), "seeds and draws, or u"),
        (dict(draws=None), "seeds and draws, or u"),
        (dict(seeds=seeds.to(i32)), "seeds:"),
        (dict(draws=torch.zeros(3, dtype=i64)), "draws:"),
        (dict(seeds=None, draws=None, u=u.double()), "u:"),
        (dict(u=torch.zeros(3, dtype=f32)), "u:"),
        (dict(u=u, seeds=seeds.to(i32)), "seeds:"),                         # checked even where u makes them unused
        (dict(tokens=None), "tokens or next_tokens"),
        (dict(tokens=tok.to(i64)), "tokens:"),
        (dict(tokens=torch.zeros(3, dtype=i32)), "tokens:"),
        (dict(positions=torch.zeros(2, dtype=i64)), "positions:"),
        (dict(placement=torch.zeros(4, dtype=i32)[::2]), "placement:"),
        (dict(valid_lens=torch.zeros((2, 1), dtype=i32)), "valid_lens:"),
        (dict(next_tokens=torch.zeros(2, dtype=i32)), "next_tokens:"),
        (dict(logprobs=torch.zeros(2, dtype=torch.float64)), "logprobs:"),
        (dict(u_out=torch.zeros(3, dtype=f32)), "u_out:"),
        (dict(), "CUDA logits"),                                            # everything right but the device
        (dict(seeds=None, draws=None, u=u, tokens=None, next_tokens=torch.zeros(2, dtype=i64), logprobs=torch.zeros(2, dtype=f32),
              u_out=torch.zeros(2, dtype=f32), positions=tok, placement=tok, valid_lens=tok), "CUDA logits"),
    ]
    for change, msg in bad:
        kw = dict(logits=logits, temperature=t, top_k=k, top_p=p, seeds=seeds, draws=draws, tokens=tok)
        kw.update(change)
        with pytest.raises(ops.ZLError, match=msg):
            ops.sample_advance(**kw)


def test_entry_point_refusals_without_a_launch():
    """zl_sample_advance's own argument checks: every one returns before anything is launched, so no GPU is needed"""
    import ctypes as C
    from zhilight_amd import _lib
    f = _lib.lib().zl_sample_advance
    P = 0x1000                                                              # a non-null pointer that is never dereferenced

    def call(logits=P, type=2, rows=2, n=8, ld=8, t=P, k=P, p=P, seeds=P, draws=P, u=None, tokens=P, nxt=None):
        return f(logits, type, rows, n, ld, t, k, p, seeds, draws, u, tokens, None, None, None, nxt, None, None, None)

    EINVAL, ESHAPE, EDTYPE = -1, -2, -3
    assert call(logits=None) == EINVAL and call(t=None) == EINVAL and call(k=None) == EINVAL and call(p=None) == EINVAL
    assert call(seeds=None) == EINVAL and call(draws=None) == EINVAL and call(tokens=None) == EINVAL
    assert call(rows=0) == ESHAPE and call(n=0) == ESHAPE and call(ld=7) == ESHAPE and call(n=1 << 31, ld=1 << 31) == ESHAPE
    assert call(type=1) == EDTYPE and call(type=0) == EDTYPE and call(type=5) == EDTYPE
    assert call(seeds=None, draws=None, u=P, type=1) == EDTYPE              # u alone is a complete generator: past the EINVAL checks
    assert call(tokens=None, nxt=P, type=1) == EDTYPE


def test_sample_opts_refusals_without_a_launch():
    """zl_sample_opts_t through zl_sample_advance_ex / zl_spec_sample_accept_ex: every refusal of the penalty, bias / top-N and
    automaton groups with its code, and every field set alone.  Each returns before anything is launched, so no GPU is needed."""
    from zhilight_amd import _lib
    lib, SampleOpts = _lib.lib(), _lib.SampleOpts
    P = 0x1000                                                              # a non-null pointer that is never dereferenced
    EINVAL, ESHAPE, EDTYPE = -1, -2, -3

    def advance(n, type=2, **fields):
        return lib.zl_sample_advance_ex(P, type, 2, n, n, P, P, P, None, None, P, P, None, None, None, None, None, None, C.byref(SampleOpts(**fields)), None)

    def spec(n, type=2, **fields):
        return lib.zl_spec_sample_accept_ex(P, type, 1, 2, n, n, P, P, P, P, None, None, P, None, None, None, None, P, P, None, None, None,
                                            C.byref(SampleOpts(**fields)), None)

    def both(n, **fields):
        a, s = advance(n, **fields), spec(n, **fields)
        assert a == s, fields
        return a

    # the penalty group (tests/test_gpu_sample_penalty.py), n = 40
    assert both(40, presence=P, seen=P, seen_ld=2) == EINVAL and both(40, rep_penalty=P, seen=P, seen_ld=2) == EINVAL
    assert both(40, rep_penalty=P, presence=P, seen=P, seen_ld=1) == ESHAPE
    # the bias / top-N group (tests/test_gpu_sample_opts.py), n = 40
    bias = dict(bias_ids=P, bias_vals=P, bias_cnt=P, bias_ld=1, bias_bits=P, bias_bits_ld=2)
    assert both(40, **{**bias, "bias_vals": None}) == EINVAL and both(40, bias_vals=P, bias_ld=1, bias_bits_ld=2) == EINVAL
    assert both(40, **{**bias, "bias_bits": None}) == EINVAL
    assert both(40, top_n=4, top_ids=P) == EINVAL and both(40, top_n=4, top_logprobs=P) == EINVAL
    assert both(40, **{**bias, "bias_ld": 1025}) == ESHAPE and both(40, **{**bias, "bias_ld": 0}) == ESHAPE
    assert both(40, **{**bias, "bias_bits_ld": 1}) == ESHAPE
    assert both(40, top_n=-1, top_ids=P, top_logprobs=P) == ESHAPE and both(40, top_n=33, top_ids=P, top_logprobs=P) == ESHAPE
    assert both(40, top_n=(1 << 32) + 4, top_ids=P, top_logprobs=P) == ESHAPE                      # all 64 bits of top_n count
    # the automaton group (tests/test_gpu_fsm.py), n = 70: three mask words
    six = ("fsm_mask", "fsm_default", "fsm_exc_off", "fsm_exc_tok", "fsm_exc_next", "fsm_state")
    fsm = dict({name: P for name in six}, fsm_mask_ld=3, fsm_states=3, fsm_exceptions=1, fsm_row_states=P)
    for drop in six:                                                        # some but not all of the six
        assert both(70, **{**fsm, drop: None}) == EINVAL, drop
    assert both(70, fsm_state=P, fsm_mask_ld=3, fsm_states=3, fsm_exceptions=1) == EINVAL
    assert spec(70, **{**fsm, "fsm_row_states": None}) == EINVAL            # tables without row_states: the speculative call alone
    assert advance(70, type=1, **{**fsm, "fsm_row_states": None}) == EDTYPE  # ... zl_sample_advance_ex does not ask for them
    for change in (dict(fsm_states=0), dict(fsm_mask_ld=2), dict(fsm_states=1 << 31), dict(fsm_exceptions=1 << 31), dict(fsm_exceptions=-1)):
        assert both(70, **{**fsm, **change}) == ESHAPE, change
    # every field alone: a pointer of a group is refused by its group's check (type = 2, so the dtype check is passed); a field that
    # is legal alone -- a leading dimension or a count without its pointers, an output without top_n, parameters without seen --
    # reaches the dtype check, which type = 1 fails
    alone = dict(rep_penalty=EDTYPE, presence=EDTYPE, seen=EINVAL, seen_ld=EDTYPE, bias_ids=EINVAL, bias_vals=EINVAL, bias_cnt=EINVAL,
                 bias_ld=EDTYPE, bias_bits=EINVAL, bias_bits_ld=EDTYPE, top_n=EINVAL, top_ids=EDTYPE, top_logprobs=EDTYPE, fsm_mask=EINVAL,
                 fsm_mask_ld=EDTYPE, fsm_default=EINVAL, fsm_exc_off=EINVAL, fsm_exc_tok=EINVAL, fsm_exc_next=EINVAL, fsm_states=EDTYPE,
                 fsm_exceptions=EDTYPE, fsm_state=EINVAL, fsm_row_states=EDTYPE)
    assert list(alone) == [name for name, _ in SampleOpts._fields_] and len(alone) == 23
    for (name, ctype), code in zip(SampleOpts._fields_, alone.values()):
        value = {name: P if ctype is C.c_void_p else 4}
        type = 1 if code == EDTYPE else 2
        assert advance(40, type=type, **value) == code and spec(40, type=type, **value) == code, name
    # NULL opts and a zeroed struct are the plain call: past every option's check, to the dtype's
    assert advance(40, type=1) == EDTYPE and spec(40, type=1) == EDTYPE
    assert lib.zl_sample_advance_ex(P, 1, 2, 40, 40, P, P, P, None, None, P, P, None, None, None, None, None, None, None, None) == EDTYPE


def test_option_struct_layouts_match_the_header():
    """the ctypes mirrors of zl_sample_opts_t and zl_w4_opts_t against the C compiler's sizeof / offsetof (zl_internals.struct_layouts):
    a mirror that disagrees would hand the launchers wild pointers"""
    from zhilight_amd import _lib, zl_internals
    layouts = zl_internals.struct_layouts()
    assert sorted(layouts) == ["zl_sample_opts_t", "zl_w4_opts_t"]
    for name, mirror in (("zl_sample_opts_t", _lib.SampleOpts), ("zl_w4_opts_t", _lib.W4Opts)):
        size, fields = layouts[name]
        assert [f for f, _ in fields] == [f for f, _ in mirror._fields_], name
        assert [(f, off) for f, off in fields] == [(f, getattr(mirror, f).offset) for f, _ in mirror._fields_], name
        assert C.sizeof(mirror) == size, name
    assert layouts["zl_sample_opts_t"][0] == 184 and len(_lib.SampleOpts._fields_) == 23


def test_new_sampler_argument_checks():
    from zhilight_amd import ops
    from zhilight_amd.llama import LLaMA, SamplerState
    ctx = types.SimpleNamespace(tokens=torch.zeros(3, dtype=torch.int32))
    new = lambda **kw: LLaMA.new_sampler(None, ctx, **kw)
    bad = [
        (dict(temperature=-0.1), "temperature >= 0"),
        (dict(temperature=[1.0, float("nan"), 1.0]), "temperature >= 0"),
        (dict(temperature=[1.0, 1.0]), "3 tasks, 2 values of temperature"),
        (dict(top_k=-1), "top_k is an integer >= 0"),
        (dict(top_k=[1, 2, 2.5]), "top_k is an integer >= 0"),
        (dict(top_k=[1, 2, 3, 4]), "3 tasks, 4 values of top_k"),
        (dict(top_p=1.01), "top_p in \\[0, 1\\]"),
        (dict(top_p=[0.5, -0.01, 1.0]), "top_p in \\[0, 1\\]"),
        (dict(top_p=float("nan")), "top_p in \\[0, 1\\]"),
        (dict(top_p=[0.5]), "3 tasks, 1 values of top_p"),
        (dict(seed=[1, 2]), "3 tasks, 2 values of seed"),
        (dict(seed=1.5), "seed is an integer"),
    ]
    for kw, msg in bad:
        with pytest.raises(ops.ZLError, match=msg):
            new(**kw)
    s = new(temperature=[0.0, 0.7, 1.5], top_k=torch.tensor([0, 5, 40]), top_p=0.9, seed=11)
    assert isinstance(s, SamplerState)
    assert s.temperature.tolist() == pytest.approx([0.0, 0.7, 1.5]) and s.top_k.tolist() == [0, 5, 40] and s.top_k.dtype == torch.int32
    assert s.top_p.tolist() == pytest.approx([0.9] * 3) and s.seeds.tolist() == [11, 12, 13] and s.draws.tolist() == [0, 0, 0]
    assert s.seeds.dtype == s.draws.dtype == torch.int64 and s.logprobs.dtype == s.u.dtype == torch.float32
    assert new(seed=[7, 7, (1 << 64) - 1]).seeds.tolist() == [7, 7, -1]     # given seeds are taken as they are, 64 bits of key
