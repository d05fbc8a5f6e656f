"""Host-side pieces of the stop conditions: the reference statement of zl_stop_advance (tests/stop_ref.py) is invariant under the
partition of a task's id stream into steps -- which is what makes speculation change the speed and not the output --, hand-written cases
of the rule, ops.stop_pack's layout and refusals, and the C entry point's argument checks (every check precedes the launch: nothing
runs, so they hold without a GPU)."""
import ctypes as C

import numpy as np
import pytest

import stop_ref as sr

ALPHABET = 6


def random_stops(rng, b, alphabet=ALPHABET, p_ids=0.5, p_seqs=0.7, p_max=0.5, max_hi=60, max_seq_len=16):
    """per task: up to 2 stop ids, up to 3 sequences of 2 .. max_seq_len ids (long ones rarely hit, short ones often), a length limit"""
    stops, max_new = [], np.zeros(b, np.int32)
    for t in range(b):
        ids = rng.integers(0, alphabet, rng.integers(1, 3)).tolist() if rng.random() < p_ids else []
        seqs = []
        if rng.random() < p_seqs:
            for _ in range(int(rng.integers(1, 4))):
                n = int(rng.choice([2, 2, 3, 3, 4, 5, max_seq_len]))
                seqs.append(rng.integers(0, alphabet, n).tolist())
        if rng.random() < p_max:
            max_new[t] = rng.integers(1, max_hi)
        stops.append((ids, seqs))
    return stops, max_new


def run_stream(stops, max_new, stream, pieces, pending=None, n_new=32):
    """feed one task's stream in the given pieces -> (concatenated output, state, [emit_lens per call])"""
    ids, seqs, lens = sr.pack(stops)
    st = sr.new_state(1, pending)
    out, at, emits = [], 0, []
    for p in pieces:
        row = np.full((1, n_new), -1, np.int32)
        row[0, :p] = stream[at:at + p]
        at += p
        emit, _ = sr.stop_advance(ids, seqs, lens, max_new, st, row)
        assert (row[0, emit[0]:] == -1).all()
        out += row[0, :emit[0]].tolist()
        emits.append(int(emit[0]))
    return out, st, emits


def test_partition_invariance():
    """2 400 random cases over a 6-symbol alphabet: a stream fed in pieces of 1 .. 32 ids gives the cut, the reason, gen_lens and the
    tail of the same stream fed one id at a time; every reason and the never-finishing task occur often"""
    rng = np.random.default_rng(5)
    reasons = np.zeros(4, np.int64)
    cut_inside = 0
    for case in range(2400):
        stops, max_new = random_stops(rng, 1)
        n = int(rng.integers(1, 80))
        stream = rng.integers(0, ALPHABET, n).astype(np.int32)
        pending = [int(rng.integers(0, ALPHABET))] if case % 2 else None
        pieces = []
        while sum(pieces) < n:
            pieces.append(int(min(rng.integers(1, 33), n - sum(pieces))))
        one, st1, _ = run_stream(stops, max_new, stream, [1] * n, pending)
        got, st, emits = run_stream(stops, max_new, stream, pieces, pending)
        assert got == one, case
        for name in ("gen_lens", "tail", "last_token", "finished"):
            assert np.array_equal(st[name], st1[name]), (case, name)
        assert st["gen_lens"][0] == len(got) and got == stream[:len(got)].tolist()
        reasons[st["finished"][0]] += 1
        cut_inside += any(0 < e < p for e, p in zip(emits, pieces))
        assert sum(emits) == len(got)
    print("reasons 0 .. 3:", reasons.tolist(), "cases cut inside a piece:", cut_inside)
    assert (reasons >= 100).all() and cut_inside >= 300


def _one(stops, max_new, rows, pending=None, extra=False):
    """feed the rows (lists, -1 padded by the caller or not) of ONE task one call each -> [(row after, emit, finished)], state"""
    ids, seqs, lens = sr.pack([stops])
    st = sr.new_state(1, pending)
    res = []
    width = max(len(r) for r in rows)
    for r in rows:
        row = np.full((1, max(width, 1)), -1, np.int32)
        row[0, :len(r)] = r
        emit, live = sr.stop_advance(ids, seqs, lens, np.array([max_new], np.int32), st, row)
        res.append((row[0].tolist(), int(emit[0]), int(st["finished"][0])))
        assert live == int(st["finished"][0] == 0)
    return res, st


def test_sequence_spanning_three_steps():
    res, st = _one(([], [[4, 5, 1, 2]]), 0, [[3, 4], [5, 1], [2, 0, 3]])
    assert res[0] == ([3, 4, -1], 2, 0) and res[1] == ([5, 1, -1], 2, 0) and res[2] == ([2, -1, -1], 1, sr.STOP_SEQ)
    assert st["gen_lens"][0] == 5 and st["tail"][0].tolist() == [-1] * 10 + [3, 4, 5, 1, 2] and st["last_token"][0] == 2


def test_sixteen_ids_against_a_full_tail_and_one_new_id():
    seq = [(i * 5) % 7 for i in range(16)]
    res, st = _one(([], [seq]), 0, [seq[:8], seq[8:15], [seq[15], 1]])
    assert [r[2] for r in res] == [0, 0, sr.STOP_SEQ] and res[2][:2] == ([seq[15], -1, -1, -1, -1, -1, -1, -1], 1)
    assert st["tail"][0].tolist() == seq[1:]
    # one id short of the sequence in the window: 15 matching ids behind a hole never match
    res, _ = _one(([], [seq]), 0, [seq[1:8], seq[8:15], [seq[15], 1]])
    assert [r[2] for r in res] == [0, 0, 0]


def test_two_sequences_ending_at_the_same_id_and_the_order_of_reasons():
    # both sequences end at j = 2; the rule takes the lowest index -- either way the cut and the reason are the same
    res, _ = _one(([], [[1, 2, 3], [2, 3]]), 0, [[0, 1, 2, 3, 4]])
    assert res[0] == ([0, 1, 2, 3, -1], 4, sr.STOP_SEQ)
    # the later-listed sequence ends EARLIER in the row: the first hit position decides, not the sequence's index
    res, _ = _one(([], [[1, 2, 3], [0, 1]]), 0, [[0, 1, 2, 3, 4]])
    assert res[0] == ([0, 1, -1, -1, -1], 2, sr.STOP_SEQ)
    # a stop id and a sequence at the same j: reason 1; with the length limit there too: still 1; sequence + limit: 2
    res, _ = _one(([3], [[2, 3]]), 4, [[0, 1, 2, 3, 4]])
    assert res[0] == ([0, 1, 2, 3, -1], 4, sr.STOP_ID)
    res, _ = _one(([], [[2, 3]]), 4, [[0, 1, 2, 3, 4]])
    assert res[0] == ([0, 1, 2, 3, -1], 4, sr.STOP_SEQ)


def test_length_limit_inside_a_row_and_an_empty_row():
    res, st = _one(([], []), 5, [[1, 2, 3], [], [4, 5, 0, 1], [2, 3, 4, 5]])
    assert res[0] == ([1, 2, 3, -1], 3, 0)
    assert res[1] == ([-1, -1, -1, -1], 0, 0)                          # m = 0 changes nothing
    assert res[2] == ([4, 5, -1, -1], 2, sr.LENGTH)
    assert res[3] == ([-1, -1, -1, -1], 0, sr.LENGTH)                  # frozen
    assert st["gen_lens"][0] == 5 and st["last_token"][0] == 5 and st["tail"][0].tolist() == [-1] * 10 + [1, 2, 3, 4, 5]


def test_the_pending_token_starts_a_match_but_is_not_tested():
    res, st = _one(([7], [[7, 2]]), 0, [[2, 3]], pending=[7])
    assert res[0] == ([2, -1], 1, sr.STOP_SEQ) and st["gen_lens"][0] == 1
    res, _ = _one(([7], [[7, 2]]), 0, [[2, 3]])                       # without the seed the tail's -1 matches nothing
    assert res[0] == ([2, 3], 2, 0)
    res, st = _one(([7], []), 3, [[1], [2], [7]], pending=[7])          # the pending stop id itself did not finish the task
    assert [r[2] for r in res] == [0, 0, sr.STOP_ID] and st["gen_lens"][0] == 3


def test_batch_state_and_a_frozen_task():
    """the optional results: a cut row takes the context back by m - c, a frozen task by m and re-feeds its last token; the aliased
    one-token form ends in tokens = last_token"""
    ids, seqs, lens = sr.pack([([5], []), ([], [])])
    st = sr.new_state(2, [9, 9])
    rows = np.array([[1, 5, 2, -1], [1, 2, 3, 4]], np.int32)
    acc, nxt = np.array([2, 3], np.int32), np.zeros(2, np.int64)
    tok, pos, plc, val = (np.array(v, np.int32) for v in ([2, 4], [13, 24], [13, 24], [14, 25]))
    emit, live = sr.stop_advance(ids, seqs, lens, None, st, rows, acc, nxt, tok, pos, plc, val)
    assert emit.tolist() == [2, 4] and live == 1 and rows.tolist() == [[1, 5, -1, -1], [1, 2, 3, 4]]
    assert acc.tolist() == [1, 3] and nxt.tolist() == [5, 4] and tok.tolist() == [5, 4]
    assert pos.tolist() == [12, 24] and plc.tolist() == [12, 24] and val.tolist() == [13, 25]
    rows = np.array([[0, 1, -1, -1], [5, -1, -1, -1]], np.int32)
    tok[:], pos[:], plc[:], val[:] = [1, 5], pos + [2, 1], plc + [2, 1], val + [2, 1]
    emit, live = sr.stop_advance(ids, seqs, lens, None, st, rows, acc, nxt, tok, pos, plc, val)
    assert emit.tolist() == [0, 1] and live == 1 and rows.tolist() == [[-1] * 4, [5, -1, -1, -1]]
    assert acc.tolist() == [-1, 0] and nxt.tolist() == [-1, 5] and tok.tolist() == [5, 5]
    assert pos.tolist() == [12, 25] and val.tolist() == [13, 26] and st["finished"].tolist() == [sr.STOP_ID, 0]
    tok[:] = [3, 3]                                                     # the row IS tokens
    emit, _ = sr.stop_advance(ids, seqs, lens, None, st, tok.reshape(2, 1), None, nxt, tok, pos, plc, val)
    assert emit.tolist() == [0, 1] and tok.tolist() == [5, 3] and nxt.tolist() == [-1, 3] and pos.tolist() == [11, 25]


def test_stop_pack_layout_and_refusals():
    from zhilight_amd import ops
    ids, seqs, lens = ops.stop_rows([([3, 1], [[1, 2, 3], [4]]), None, (None, [[5, 5]]), ([], [])], 10)
    assert ids.tolist() == [[3, 1], [-1, -1], [-1, -1], [-1, -1]] and lens.tolist() == [[3, 1], [0, 0], [2, 0], [0, 0]]
    assert seqs.shape == (4, 2, 3) and seqs[0].tolist() == [[1, 2, 3], [4, -1, -1]] and seqs[2, 0].tolist() == [5, 5, -1]
    for a, b in zip((ids, seqs, lens), sr.pack([([3, 1], [[1, 2, 3], [4]]), ([], []), ([], [[5, 5]]), ([], [])])):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    empty = ops.stop_rows([None, None], 10)                             # nothing set: still a valid state, widths of 1
    assert [a.shape for a in empty] == [(2, 1), (2, 1, 1), (2, 1)] and (empty[0] == -1).all() and (empty[2] == 0).all()
    t = ops.stop_pack([([1], [[2, 3]])], 10, "cpu")
    assert [tuple(x.shape) for x in t] == [(1, 1), (1, 1, 2), (1, 1)] and all(str(x.dtype) == "torch.int32" for x in t)
    ops.stop_rows([(list(range(16)), [[1] * 16] * 8)], 16)              # the limits themselves are fine
    for match, stops in (("17 stop ids", [(list(range(17)), [])]), ("9 stop sequences", [([], [[1]] * 9)]),
                         ("1 .. 16 ids", [([], [[]])]), ("1 .. 16 ids", [([], [[1] * 17])]),
                         ("outside", [([10], [])]), ("outside", [([-1], [])]), ("outside", [([], [[1, 10]])]), ("outside", [None, ([], [[-2]])]),
                         ("per task", [(["a"], [])]), ("per task", [5]), ("per task", [])):
        with pytest.raises(ops.ZLError, match=match):
            ops.stop_rows(stops, 10)
    with pytest.raises(ops.ZLError, match="vocab"):
        ops.stop_rows([None], 0)


def test_c_entry_point_refuses_before_any_launch():
    """the header's ZL_EINVAL / ZL_ESHAPE cases on host memory: every one returns before the launch, so nothing runs"""
    from zhilight_amd import _lib
    lib = _lib.lib()
    b, n_new = 3, 4
    arr = lambda *shape: np.zeros(shape, np.int32)                                               # noqa: E731
    full = dict(stop_ids=arr(b, 2), stop_seqs=arr(b, 2, 3), seq_lens=arr(b, 2), max_new=arr(b), gen_lens=arr(b), tail=arr(b, 15),
                last_token=arr(b), finished=arr(b), new_tokens=arr(b, n_new), accepted=arr(b), next_tokens=np.zeros(b, np.int64),
                tokens=arr(b), positions=arr(b), placement=arr(b), valid_lens=arr(b), emit_lens=arr(b), live=arr(1))

    def status(n_ids=2, n_seqs=2, ld=3, nn=n_new, bb=b, **change):
        a = {**full, **change}
        p = lambda m: C.c_void_p(None if a[m] is None else a[m].ctypes.data)                    # noqa: E731
        return lib.zl_stop_advance(p("stop_ids"), n_ids, p("stop_seqs"), p("seq_lens"), n_seqs, ld, p("max_new"), p("gen_lens"), p("tail"),
                                   p("last_token"), p("finished"), p("new_tokens"), nn, bb, p("accepted"), p("next_tokens"), p("tokens"),
                                   p("positions"), p("placement"), p("valid_lens"), p("emit_lens"), p("live"), C.c_void_p(None))

    EINVAL, ESHAPE = -1, -2
    for m in ("gen_lens", "tail", "last_token", "finished", "new_tokens", "emit_lens", "live"):
        assert status(**{m: None}) == EINVAL, m
    for kw in (dict(bb=0), dict(nn=0), dict(n_ids=-1), dict(n_ids=0), dict(stop_ids=None), dict(n_seqs=0), dict(ld=0), dict(stop_seqs=None),
               dict(seq_lens=None), dict(n_seqs=0, ld=0, stop_seqs=None), dict(new_tokens=full["tokens"], nn=2)):
        assert status(**kw) == EINVAL, kw
    for kw in (dict(n_ids=17), dict(n_seqs=9), dict(ld=17), dict(nn=33), dict(bb=1 << 31)):
        assert status(**kw) == ESHAPE, kw
    assert status(nn=33, gen_lens=None) == EINVAL                       # the order of the checks
