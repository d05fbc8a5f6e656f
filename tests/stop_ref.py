"""Pure-Python / numpy statement of zl_stop_advance (the stop conditions of a decode step: stop ids, multi-token stop sequences and a
length limit per task, applied to the ids a step emitted, with the cut of the step's results and the roll-back of the batch state),
written from the rule of include/zhilight_amd.h and shared by test_stop_host.py and the GPU tests."""
import numpy as np

TAIL = 15                                    # ids a task remembers: a stop sequence has at most 16 ids, one of them new
LIVE, STOP_ID, STOP_SEQ, LENGTH = 0, 1, 2, 3


def new_state(b, pending=None):
    """the state of b live tasks that have emitted nothing; pending (b ids): the token each task feeds next -- it seeds the tail's last
    entry and last_token and is neither tested nor counted"""
    st = dict(gen_lens=np.zeros(b, np.int32), tail=np.full((b, TAIL), -1, np.int32), last_token=np.full(b, -1, np.int32),
              finished=np.zeros(b, np.int32))
    if pending is not None:
        st["tail"][:, TAIL - 1] = st["last_token"][:] = np.asarray(pending, np.int32)
    return st


def emitted(row):
    """the ids of a row before its first negative one"""
    out = []
    for v in row:
        if v < 0:
            break
        out.append(int(v))
    return out


def hit(ids, seqs, max_new, tail, e, j, g):
    """the reason position j of the emitted ids e is a hit for, 0 = none.  ids: the task's stop ids (-1 = unused); seqs: its stop
    sequences as lists (an empty one = unused); tail: the TAIL ids in front of e, -1 = none; g: ids the task has emitted up to and
    including e[j]"""
    if e[j] in [i for i in ids if i >= 0]:
        return STOP_ID
    window = list(tail) + list(e[:j + 1])
    for s in seqs:
        if len(s) and window[-len(s):] == list(s) and min(window[-len(s):]) >= 0:
            return STOP_SEQ
    if max_new > 0 and g >= max_new:
        return LENGTH
    return LIVE


def stop_advance(stop_ids, stop_seqs, seq_lens, max_new, state, new_tokens, accepted=None, next_tokens=None, tokens=None,
                 positions=None, placement=None, valid_lens=None):
    """One call, in place on numpy arrays: state = new_state()'s dict; new_tokens (B, n_new) the step's rows; the optional results and
    batch state as the C call takes them (None = absent; new_tokens may be tokens.reshape(B, 1) itself).  stop_ids (B, n_ids) / stop_seqs
    (B, n_seqs, ld) / seq_lens (B, n_seqs) / max_new (B) may each be None.  Returns (emit_lens (B) int32, live)"""
    b, n_new = new_tokens.shape
    emit = np.zeros(b, np.int32)
    ctx = [a for a in (positions, placement, valid_lens) if a is not None]
    for t in range(b):
        e = emitted(new_tokens[t].tolist())                # the row is read before anything of the task is written
        m = len(e)
        if m == 0:
            continue
        if state["finished"][t] != LIVE:                   # frozen: the step is undone, the task re-feeds its last token
            new_tokens[t, :] = -1
            if accepted is not None:
                accepted[t] = -1
            if next_tokens is not None:
                next_tokens[t] = -1
            for a in ctx:
                a[t] -= m
            if tokens is not None:
                tokens[t] = state["last_token"][t]
            continue
        ids = [] if stop_ids is None else stop_ids[t].tolist()
        seqs = [] if stop_seqs is None else [stop_seqs[t, q, :max(int(seq_lens[t, q]), 0)].tolist() for q in range(stop_seqs.shape[1])]
        lim = 0 if max_new is None else int(max_new[t])
        tail, g0 = state["tail"][t].tolist(), int(state["gen_lens"][t])
        c, reason = m, LIVE
        for j in range(m):
            r = hit(ids, seqs, lim, tail, e, j, g0 + j + 1)
            if r:
                c, reason = j + 1, r
                break
        new_tokens[t, c:] = -1
        emit[t] = c
        state["gen_lens"][t] = g0 + c
        state["tail"][t] = (tail + e[:c])[-TAIL:]
        if accepted is not None:
            accepted[t] = c - 1
        for a in ctx:
            a[t] -= m - c
        if tokens is not None:
            tokens[t] = e[c - 1]
        if next_tokens is not None:
            next_tokens[t] = e[c - 1]
        state["last_token"][t] = e[c - 1]
        state["finished"][t] = reason
    return emit, int((state["finished"] == LIVE).sum())


def pack(stops, n_ids=None, n_seqs=None, ld=None):
    """per-task (stop ids, stop sequences) -> the padded int32 arrays (stop_ids (B, n_ids), stop_seqs (B, n_seqs, ld), seq_lens (B, n_seqs))
    with -1 / length 0 in the unused entries; widths default to the longest list, at least 1"""
    n_ids = n_ids or max([1] + [len(i) for i, _ in stops])
    n_seqs = n_seqs or max([1] + [len(s) for _, s in stops])
    ld = ld or max([1] + [len(q) for _, s in stops for q in s])
    ids = np.full((len(stops), n_ids), -1, np.int32)
    seqs = np.full((len(stops), n_seqs, ld), -1, np.int32)
    lens = np.zeros((len(stops), n_seqs), np.int32)
    for t, (i, s) in enumerate(stops):
        ids[t, :len(i)] = i
        for q, sq in enumerate(s):
            seqs[t, q, :len(sq)], lens[t, q] = sq, len(sq)
    return ids, seqs, lens
