"""numpy statement of the token automaton of zl_sample_advance_fsm / zl_spec_sample_accept_fsm / zl_slots_admit_fsm, written from the
rule of include/zhilight_amd.h and shared by test_fsm_host.py and test_gpu_fsm.py.  It holds no probability arithmetic: delta, the
draft chain and `masked` (the row a constrained task sees) are all there is; the expected picks come from the existing statements
(sample_ref / sample_opts_ref / spec_sample_ref / slot_ref) applied to the masked copy."""
import numpy as np

import slot_ref

NEG_INF = {False: 0xFC00, True: 0xFF80}


class Tables:
    """the five arrays as the kernel gets them; mask may be wider than ceil(n / 32) words and hold bits at or above n"""

    def __init__(self, mask, default, exc_off, exc_tok, exc_next):
        self.mask = np.asarray(mask, np.uint32)
        self.default = np.asarray(default, np.int32)
        self.exc_off = np.asarray(exc_off, np.int32)
        self.exc_tok = np.asarray(exc_tok, np.int32)
        self.exc_next = np.asarray(exc_next, np.int32)
        self.S = self.default.size

    def arrays(self):
        return self.mask, self.default, self.exc_off, self.exc_tok, self.exc_next


def allowed(tb, s, tok):
    return bool((int(tb.mask[s, tok >> 5]) >> (tok & 31)) & 1)


def delta(tb, s, tok, n):
    """a state outside [0, S), a token outside [0, n) and a disallowed token leave the state; else the exception's target where the
    list of s holds the token (a linear walk: the lists are ascending, nothing here depends on it), else the default"""
    s, tok = int(s), int(tok)
    if not 0 <= s < tb.S or not 0 <= tok < n or not allowed(tb, s, tok):
        return s
    for e in range(int(tb.exc_off[s]), int(tb.exc_off[s + 1])):
        if int(tb.exc_tok[e]) == tok:
            return int(tb.exc_next[e])
    return int(tb.default[s])


def chain(tb, s, drafts, n):
    """[s_0, s_1, ..., s_K]: the state of every row of a speculative step, s_{j+1} = delta(s_j, drafts[j])"""
    out = [int(s)]
    for d in drafts:
        out.append(delta(tb, out[-1], int(d), n))
    return out


def masked(bits, tb, s, bf16):
    """the row a task in state s sees: the stored patterns where the state's bit is set, -inf of the type everywhere else (whatever
    is stored there, a NaN included); a state outside [0, S): the row as stored.  The input is left alone"""
    out = np.array(bits, np.uint16, copy=True)
    s = int(s)
    if 0 <= s < tb.S:
        i = np.arange(out.size)
        keep = (tb.mask[s, i >> 5] >> (i & 31).astype(np.uint32)) & 1
        out[keep == 0] = NEG_INF[bool(bf16)]
    return out


def spec_states(tb, state, drafts, picks, accepted, n):
    """-> (row_states (b, len_q), fsm_state (b)) of a speculative call: picks (b, len_q) = every row's pick BEFORE the padding"""
    b, len_q = picks.shape
    rows = np.empty((b, len_q), np.int32)
    for t in range(b):
        s = chain(tb, state[t], drafts[t], n)
        for i in range(len_q):
            rows[t, i] = delta(tb, s[i], picks[t, i], n)
    return rows, rows[np.arange(b), np.asarray(accepted)].copy()


def admit(blob, ctx, sampler=None, stop=None, lookup=None, draft_new=None, fsm_state=None):
    """zl_slots_admit_fsm, in place: the pending-token overrides of the blob's side array (header flag 16, header word 12) go into
    ctx["tokens"] first, the rest IS slot_ref.admit; then the states: the start state of an admitted slot (-1 without the array),
    -1 for a parked one"""
    h = slot_ref.header(blob)
    recs = blob[slot_ref.HDR:h["var"]].reshape(h["n"], h["rec"])
    side = None
    if fsm_state is not None and h["flags"] & 16:
        side = blob[blob[12]:blob[12] + 2 * h["n"]].reshape(h["n"], 2)
    b = ctx["tokens"].size
    for j, r in enumerate(recs):
        s = int(r[0])
        if not 0 <= s < b:
            continue
        if r[1] != 0 and side is not None and 0 <= side[j, 1] < h["vocab"]:
            ctx["tokens"][s] = side[j, 1]
    slot_ref.admit(blob, ctx, sampler, stop, lookup, draft_new)
    if fsm_state is not None:
        for j, r in enumerate(recs):
            s = int(r[0])
            if 0 <= s < b:
                fsm_state[s] = -1 if r[1] == 0 or side is None else side[j, 0]
