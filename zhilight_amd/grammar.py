"""Token automata for constrained output (numpy only): the host half of zl_sample_opts_t's automaton group
(zl_sample_advance_ex / zl_spec_sample_accept_ex).

A TokenAutomaton is a DFA over token ids.  pack() turns it into the five device tables of include/zhilight_amd.h -- per state a dense
allow-bitmap over the vocabulary, a default next state and an ascending exception list in CSR form -- which LLaMA.load_grammar copies
into a sampler once; from then on the sampling launch masks every row by its task's state and advances the state over the pick, with
no host round trip.  How an automaton is obtained is host work outside the step: two small builders are here, a regex or JSON-schema
compiler is not."""
import collections

import numpy as np

from ._lib import ZLError

PackedAutomaton = collections.namedtuple("PackedAutomaton", "mask default exc_off exc_tok exc_next")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class TokenAutomaton:
    """A DFA over the token ids [0, vocab): transitions[s] = {token: next state}; the allowed set of state s is its key set.  A next
    state >= 0 is a state of this automaton; a negative one means "unconstrained from here".  Refused (ZLError): a state with no
    allowed token, ids outside the vocabulary, targets at or above the number of states, a start outside the states."""

    def __init__(self, vocab, transitions, start=0):
        if not _is_int(vocab) or not 1 <= int(vocab) < 1 << 31:
            raise ZLError("TokenAutomaton: 1 <= vocab < 2^31")
        self.vocab = int(vocab)
        try:
            self.transitions = [dict(t) for t in transitions]
        except (TypeError, ValueError):
            raise ZLError("TokenAutomaton: transitions is a list of {token: next state} dicts") from None
        ns = len(self.transitions)
        if ns < 1:
            raise ZLError("TokenAutomaton: at least one state")
        if not _is_int(start) or not 0 <= int(start) < ns:
            raise ZLError(f"TokenAutomaton: start in [0, {ns})")
        self.start = int(start)
        for s, t in enumerate(self.transitions):
            if not t:
                raise ZLError(f"TokenAutomaton: state {s} allows no token")
            for tok, nxt in t.items():
                if not _is_int(tok) or not 0 <= int(tok) < self.vocab:
                    raise ZLError(f"TokenAutomaton: state {s}: token {tok!r} outside [0, {self.vocab})")
                if not _is_int(nxt) or int(nxt) >= ns or int(nxt) < -(1 << 31):
                    raise ZLError(f"TokenAutomaton: state {s}: target {nxt!r} at or above the {ns} states")

    @property
    def states(self):
        return len(self.transitions)

    def step(self, state, token):
        """delta(state, token) in the dict form: an unconstrained state, a token outside the vocabulary and a disallowed token leave
        the state where it is"""
        if not 0 <= state < self.states:
            return state
        return int(self.transitions[state].get(int(token), state)) if 0 <= token < self.vocab else state

    def accepts(self, tokens):
        """every token is allowed where it arrives (the walk starts at start and goes on while it is constrained)"""
        s = self.start
        for tok in tokens:
            if not 0 <= s < self.states:
                return True
            if int(tok) not in self.transitions[s]:
                return False
            s = int(self.transitions[s][int(tok)])
        return True

    def pack(self):
        """-> PackedAutomaton(mask (S, ceil(vocab / 32)) uint32, default (S) int32, exc_off (S + 1) int32, exc_tok (E) int32,
        exc_next (E) int32).  A state's default is its most frequent target (the lowest one among equals); every allowed token with
        another target is an exception, ascending by token."""
        ns, words = self.states, (self.vocab + 31) // 32
        mask = np.zeros((ns, words), np.uint32)
        default = np.zeros(ns, np.int32)
        off = np.zeros(ns + 1, np.int64)
        toks, nexts = [], []
        for s, t in enumerate(self.transitions):
            tk = np.fromiter(t.keys(), np.int64, len(t))
            nx = np.fromiter(t.values(), np.int64, len(t))
            order = np.argsort(tk, kind="stable")
            tk, nx = tk[order], nx[order]
            np.bitwise_or.at(mask[s], tk >> 5, (np.uint32(1) << (tk & 31).astype(np.uint32)))
            vals, counts = np.unique(nx, return_counts=True)
            default[s] = vals[np.argmax(counts)]
            exc = nx != default[s]
            toks.append(tk[exc])
            nexts.append(nx[exc])
            off[s + 1] = off[s] + int(exc.sum())
        if off[-1] >= 1 << 31:
            raise ZLError("TokenAutomaton.pack: fewer than 2^31 exception entries")
        return PackedAutomaton(mask, default, off.astype(np.int32), np.concatenate(toks).astype(np.int32),
                               np.concatenate(nexts).astype(np.int32))


def packed_step(packed, state, token, vocab):
    """delta(state, token) from the packed arrays, the device's rule word for word"""
    ns = packed.default.shape[0]
    if not 0 <= state < ns or not 0 <= token < vocab:
        return int(state)
    if not (int(packed.mask[state, token >> 5]) >> (token & 31)) & 1:
        return int(state)
    lo, hi = int(packed.exc_off[state]), int(packed.exc_off[state + 1])
    at = lo + int(np.searchsorted(packed.exc_tok[lo:hi], token))
    if at < hi and int(packed.exc_tok[at]) == token:
        return int(packed.exc_next[at])
    return int(packed.default[state])


def from_choices(vocab, sequences, eos):
    """The automaton whose output is exactly one of the token sequences and then eos: a trie over the sequences; a node where a
    sequence ends allows eos, which leads to a final state that allows eos alone (the task stops on it: eos is one of its stop
    ids).  Refused: no sequence, an empty one, ids outside the vocabulary, eos inside a sequence."""
    seqs = [[int(t) for t in q] for q in sequences]
    if not seqs or any(not q for q in seqs):
        raise ZLError("from_choices: at least one sequence, none of them empty")
    if not _is_int(eos) or not 0 <= int(eos) < int(vocab):
        raise ZLError("from_choices: eos inside the vocabulary")
    eos = int(eos)
    if any(t == eos for q in seqs for t in q):
        raise ZLError("from_choices: eos ends a choice, it is not part of one")
    trans = [{}]
    ends = set()
    for q in seqs:
        s = 0
        for t in q:
            if t not in trans[s]:
                trans.append({})
                trans[s][t] = len(trans) - 1
            s = trans[s][t]
        ends.add(s)
    final = len(trans)
    trans.append({eos: final})
    for s in ends:
        trans[s][eos] = final
    return TokenAutomaton(vocab, trans, 0)


def from_char_dfa(vocab_strings, char_transitions, start, accepting, eos):
    """The token-index construction: vocab_strings[i] = the text of token i (None or "" = never allowed, eos included),
    char_transitions[q] = {character: next q} of a character DFA, start its start state, accepting its accepting states.  Token i is
    allowed in q where the walk of its whole string from q stays inside the DFA, and leads to where the walk ends; eos is allowed in
    the accepting states and leads to a final state that allows eos alone.  States that no token leaves (dead ends) are refused."""
    vocab = len(vocab_strings)
    nq = len(char_transitions)
    if not _is_int(eos) or not 0 <= int(eos) < vocab:
        raise ZLError("from_char_dfa: eos inside the vocabulary")
    if not 0 <= int(start) < nq or any(not 0 <= int(a) < nq for a in accepting):
        raise ZLError("from_char_dfa: start and accepting states inside the character DFA")
    eos, final = int(eos), nq
    trans = [{} for _ in range(nq)] + [{eos: final}]
    for q in range(nq):
        for i, text in enumerate(vocab_strings):
            if i == eos or not text:
                continue
            s = q
            for ch in text:
                s = char_transitions[s].get(ch)
                if s is None:
                    break
            if s is not None:
                trans[q][i] = int(s)
    for a in accepting:
        trans[int(a)][eos] = final
    return TokenAutomaton(vocab, trans, int(start))
