"""Token automata on the host: zhilight_amd/grammar.py (the dict form, pack(), the two builders, the refusals) and the grammar side
array of ops.slots_pack.  No GPU: the kernels' side is tests/test_gpu_fsm.py."""
import itertools

import numpy as np
import pytest

import fsm_ref
import slot_ref as sl


def _random_automaton(rng, vocab, states, free=False):
    from zhilight_amd.grammar import TokenAutomaton
    trans = []
    for s in range(states):
        toks = rng.choice(vocab, int(rng.integers(1, vocab + 1)), replace=False)
        lo = -2 if free else 0
        if s % 3 == 0:                                                      # one dominant target and a few exceptions
            t = {int(k): (int(rng.integers(lo, states)) if rng.random() < 0.2 else s) for k in toks}
        else:
            t = {int(k): int(rng.integers(lo, states)) for k in toks}
        trans.append(t)
    return TokenAutomaton(vocab, trans, int(rng.integers(0, states)))


@pytest.mark.parametrize("vocab", [1, 31, 32, 33, 70])
def test_pack_round_trips_the_dict_form(vocab):
    """delta from the packed arrays (grammar.packed_step and fsm_ref.delta, written apart) equals the dict lookup for every
    (state, token), tokens outside the vocabulary and states outside the automaton included"""
    from zhilight_amd import grammar
    rng = np.random.default_rng(vocab)
    for states in (1, 2, 7):
        a = _random_automaton(rng, vocab, states, free=states > 1)
        p = a.pack()
        tb = fsm_ref.Tables(*p)
        assert p.mask.shape == (states, (vocab + 31) // 32) and p.mask.dtype == np.uint32
        assert p.exc_off[0] == 0 and p.exc_off[-1] == p.exc_tok.size == p.exc_next.size and (np.diff(p.exc_off) >= 0).all()
        for s in range(states):
            lst = p.exc_tok[p.exc_off[s]:p.exc_off[s + 1]]
            assert (np.diff(lst) > 0).all()                                 # ascending and distinct
            targets = list(a.transitions[s].values())
            assert targets.count(int(p.default[s])) == max(targets.count(v) for v in set(targets))        # the most frequent target
            assert lst.size == len(targets) - targets.count(int(p.default[s]))
            bits = [t for t in range(vocab) if fsm_ref.allowed(tb, s, t)]
            assert bits == sorted(a.transitions[s])
        if vocab & 31:
            assert not (p.mask[:, -1] >> np.uint32(vocab & 31)).any()       # nothing at or above the vocabulary
        for s, t in itertools.product(range(-2, states + 2), range(-2, vocab + 2)):
            want = a.step(s, t)
            assert grammar.packed_step(p, s, t, vocab) == want == fsm_ref.delta(tb, s, t, vocab), (s, t)


def test_from_choices_accepts_exactly_the_listed_sequences():
    from zhilight_amd.grammar import from_choices
    vocab, eos = 6, 5
    choices = [[1, 2], [1, 2, 3], [4], [0, 0, 1]]
    a = from_choices(vocab, choices, eos)
    p = a.pack()
    tb = fsm_ref.Tables(*p)
    final = a.states - 1
    got = set()
    for ln in range(1, 5):
        for seq in itertools.product(range(vocab), repeat=ln):
            # a full output: every token allowed where it arrives, and the walk ends in the final state (behind eos)
            s, ok = a.start, True
            for t in seq:
                ok = ok and fsm_ref.allowed(tb, s, t)
                s = fsm_ref.delta(tb, s, t, vocab)
            if ok and s == final and seq.count(eos) == 1:
                got.add(seq)
    assert got == {tuple(c) + (eos,) for c in choices}
    assert sorted(a.transitions[final]) == [eos] and a.transitions[final][eos] == final
    assert a.accepts([1, 2, eos]) and a.accepts([1, 2, 3, eos]) and not a.accepts([1, eos]) and not a.accepts([2])


def test_from_char_dfa_against_a_brute_force_walk():
    """a 3-state digit / sign DFA ([+-]?[0-9]+) over a 40-string vocabulary"""
    from zhilight_amd.grammar import from_char_dfa
    digits = "0123456789"
    dfa = [dict({"+": 1, "-": 1}, **{d: 2 for d in digits}), {d: 2 for d in digits}, {d: 2 for d in digits}]
    strings = (list(digits) + ["+", "-", "+1", "-7", "12", "007", "1+", "+-", "a", "1a", " ", "", "42", "-0", "9-9", "+12", "--", "3.", "100",
                               "-12", "0x", "5", "55", "+", "-", "00", "x", None, "1 ", "<eos>"])
    assert len(strings) == 40
    eos = 39
    a = from_char_dfa(strings, dfa, 0, [2], eos)
    assert a.states == 4 and a.start == 0
    for q in range(3):
        want = {}
        for i, text in enumerate(strings):
            if i == eos or not text:
                continue
            s = q
            for ch in text:
                s = dfa[s].get(ch) if s is not None else None
            if s is not None:
                want[i] = s
        if q == 2:
            want[eos] = 3
        assert a.transitions[q] == want, q
    assert a.transitions[3] == {eos: 3}
    tok = strings.index
    assert a.accepts([tok("-7"), tok("42"), eos]) and a.accepts([tok("+"), tok("007"), eos])
    assert not a.accepts([tok("+"), eos]) and not a.accepts([tok("12"), tok("-7")]) and not a.accepts([tok("1a")])


def test_refusals():
    from zhilight_amd._lib import ZLError
    from zhilight_amd.grammar import TokenAutomaton, from_char_dfa, from_choices
    for bad in (dict(vocab=4, transitions=[{0: 0}, {}]),                     # a state with no allowed token
                dict(vocab=4, transitions=[{4: 0}]), dict(vocab=4, transitions=[{-1: 0}]),                 # ids outside the vocabulary
                dict(vocab=4, transitions=[{0: 1}]), dict(vocab=4, transitions=[{0: 2}, {1: 0}]),          # targets at or above S
                dict(vocab=4, transitions=[]), dict(vocab=0, transitions=[{0: 0}]), dict(vocab=4, transitions=[{0: 0}], start=1),
                dict(vocab=4, transitions=[{0: 0.5}]), dict(vocab=4, transitions=5)):
        with pytest.raises(ZLError):
            TokenAutomaton(**bad)
    TokenAutomaton(4, [{0: -1, 1: 0}])                                       # a negative target: unconstrained from here
    for bad in (dict(sequences=[], eos=3), dict(sequences=[[]], eos=3), dict(sequences=[[1, 3]], eos=3), dict(sequences=[[1]], eos=4),
                dict(sequences=[[7]], eos=3)):
        with pytest.raises(ZLError):
            from_choices(4, **bad)
    with pytest.raises(ZLError):
        from_char_dfa(["a", "b"], [{"a": 0}], 0, [0], 2)
    with pytest.raises(ZLError):
        from_char_dfa(["a", "b"], [{"a": 0}], 1, [0], 1)
    with pytest.raises(ZLError):
        from_char_dfa(["a", "b"], [{"a": 1}, {"z": 0}], 0, [0], 1)        # state 1 is a dead end: no token leaves it


# ---- ops.slots_pack: the grammar side array --------------------------------------------------------------------------------------------
def _requests():
    return [(3, dict(temperature=0.7, top_k=5, seed=11, penalty_tokens=[4, 9], logit_bias={7: -1.0}, stop_ids=[2], max_new_tokens=9,
                     history=[5, 6, 7])),
            (0, None),
            (5, dict(top_p=0.9, stop_sequences=[[1, 2]], history=[1]))]


def test_slots_pack_without_a_grammar_request_is_todays_blob():
    from zhilight_amd import ops
    base = dict(penalties=True, bias_ld=4, n_ids=2, n_seqs=1, seq_ld=3, hist_cap=16)
    blob0, h0 = ops.slots_pack(_requests(), 100, ops.slot_widths(**base))
    blob1, h1 = ops.slots_pack(_requests(), 100, ops.slot_widths(**base, grammar=True))
    assert blob0.tobytes() == blob1.tobytes() and h0 == h1 == sl.header(blob0)
    assert not blob1[12:16].any() and not h1["flags"] & 16 and "grammar" not in h1


def test_slots_pack_writes_the_side_array():
    from zhilight_amd import ops
    from zhilight_amd._lib import ZLError
    base = dict(penalties=True, bias_ld=4, n_ids=2, n_seqs=1, seq_ld=3, hist_cap=16)
    reqs = _requests()
    blob0, h0 = ops.slots_pack(reqs, 100, ops.slot_widths(**base, grammar=True))
    reqs[0][1]["grammar"] = (6, 42)
    reqs[2][1]["grammar"] = 2
    blob, h = ops.slots_pack(reqs, 100, ops.slot_widths(**base, grammar=True))
    assert h["flags"] == h0["flags"] | 16 and h["grammar"] == int(blob[12]) == h0["total"] and h["total"] == h0["total"] + 6
    assert blob[h["grammar"]:].reshape(3, 2).tolist() == [[6, 42], [-1, -1], [2, -1]]
    same = np.ones(h0["total"], bool)
    same[[3, 10, 12]] = False                                               # flags, total, the offset
    assert np.array_equal(blob[:h0["total"]][same], blob0[same]) and not blob[13:16].any()
    assert ops.slots_header(blob) == h and sl.header(blob)["total"] == blob.size
    # the reference reads it: the override becomes the pending token everywhere, the state follows the record
    b = 8
    ctx = {k: np.arange(b, dtype=np.int32) + 50 for k in sl.CTX}
    state = np.full(b, 77, np.int32)
    draft_new = np.zeros(b, np.int32)
    fsm_ref.admit(blob, ctx, draft_new=draft_new, fsm_state=state)
    assert ctx["tokens"][3] == 42 and ctx["tokens"][5] == 55 and ctx["tokens"][0] == 0
    assert state.tolist() == [-1, 77, 77, 6, 77, 2, 77, 77] and draft_new.tolist() == [-1, -1, -1, 42, -1, 55, -1, -1]
    for bad in (7.5, (1,), (1, 2, 3), -1, (0, 100), (0, -2), "x"):
        with pytest.raises(ZLError):
            ops.slots_pack([(0, dict(grammar=bad))], 100, ops.slot_widths(grammar=True))
    with pytest.raises(ZLError, match="no automaton"):
        ops.slots_pack([(0, dict(grammar=1))], 100, ops.slot_widths())
    assert "grammar" in ops.SLOT_REQUEST_KEYS
