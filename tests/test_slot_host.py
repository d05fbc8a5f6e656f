"""Slot admission on the host: tests/slot_ref.py (the numpy statement of zl_slots_admit) against the rows that new_sampler's,
new_stopper's and new_lookup's packing code builds for the same requests -- ops.logit_bias_rows, ops.stop_rows, penalty_ref.pack and
stop_ref.new_state --, rows of other slots untouched, live recounted, the park rule, the blob's layout, every refusal of
ops.slots_pack, the clamp of a slot's length limit, and the C entry point's refusals.  Also the generators the GPU tests share."""
import ctypes as C

import numpy as np
import pytest

import penalty_ref as pr
import slot_ref as sl
import stop_ref as sr

FULL = dict(penalties=True, bias_ld=6, n_ids=16, n_seqs=8, seq_ld=16, hist_cap=24)
TOP_N = 5


def widths_of(groups, full=FULL):
    """full with the groups that are not named switched off; groups is a subset of {"pen", "bias", "top", "stop", "lookup"}"""
    w = dict(full)
    if "pen" not in groups:
        w["penalties"] = False
    if "bias" not in groups:
        w["bias_ld"] = 0
    if "stop" not in groups:
        w["n_ids"] = w["n_seqs"] = w["seq_ld"] = 0
    if "lookup" not in groups:
        w["hist_cap"] = 0
    return w


ALL = ("pen", "bias", "top", "stop", "lookup")


def garbage_states(rng, b, vocab, w, groups, ld_extra=0):
    """(ctx, sampler, stop, lookup) dicts of numpy arrays full of random garbage (valid where a kernel reads: finished is 0 .. 3);
    ld_extra: words a bitmap row is wider than ceil(vocab / 32)"""
    words = pr.words(vocab) + ld_extra
    i32 = lambda *shape: rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)          # noqa: E731
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)                                        # noqa: E731
    ctx = dict(tokens=rng.integers(0, vocab, b).astype(np.int32), positions=rng.integers(1, 99, b).astype(np.int32),
               placement=rng.integers(1, 99, b).astype(np.int32), valid_lens=rng.integers(1, 99, b).astype(np.int32))
    ctx["tokens"][rng.random(b) < 0.2] = -7                                # a pending id outside the vocabulary is skipped by the bitmap
    sampler = dict(temperature=f32(b), top_k=i32(b), top_p=f32(b), seeds=rng.integers(-(1 << 62), 1 << 62, b), draws=rng.integers(1, 999, b),
                   logprobs=f32(b), u=f32(b))
    if "pen" in groups:
        sampler.update(repetition_penalty=f32(b), presence_penalty=f32(b), seen=i32(b, words))
    if "bias" in groups:
        sampler.update(bias_ids=i32(b, w["bias_ld"]), bias_vals=f32(b, w["bias_ld"]), bias_cnt=i32(b), bias_bits=i32(b, words))
    if "top" in groups:
        sampler.update(top_ids=i32(b, TOP_N), top_logprobs=f32(b, TOP_N))
    stop = lookup = None
    if "stop" in groups:
        stop = dict(stop_ids=i32(b, w["n_ids"]), stop_seqs=i32(b, w["n_seqs"], w["seq_ld"]), seq_lens=i32(b, w["n_seqs"]), max_new=i32(b),
                    gen_lens=i32(b), tail=i32(b, sr.TAIL), last_token=i32(b), finished=rng.integers(0, 4, b).astype(np.int32),
                    emit_lens=i32(b), live=i32(1))
    if "lookup" in groups:
        lookup = dict(history=i32(b, w["hist_cap"]), hist_lens=i32(b))
    return ctx, sampler, stop, lookup


def request(rng, vocab, w, shape):
    """a request in one of the row shapes the kernel can go wrong at; shape 0 .. 3:
    0: everything empty (no penalty ids, no bias, no stops, history length 0);  1: everything full (duplicates and id vocab - 1 among the
    penalty ids, bias count = ld with a -inf value, stop rows at full widths, history length cap - 1);  2, 3: random in between"""
    rq = dict(temperature=float(rng.random() * 2), top_k=int(rng.integers(0, 50)), top_p=float(rng.random()),
              seed=int(rng.integers(-(1 << 63), 1 << 63)))
    some = lambda hi: int(rng.integers(1, hi + 1))                                                            # noqa: E731
    if w["penalties"]:
        rq.update(repetition_penalty=float(1 + rng.random()), presence_penalty=float(rng.random() - 0.5))
        if shape == 1:
            ids = rng.integers(0, vocab, 300).tolist()
            rq["penalty_tokens"] = ids + ids[:40] + [vocab - 1, 0, vocab - 1]
        elif shape == 0:
            rq["penalty_tokens"] = []
        elif shape == 2:
            rq["penalty_tokens"] = rng.integers(0, vocab, some(70)).tolist()
    if w["bias_ld"] and shape:
        cnt = w["bias_ld"] if shape == 1 else some(w["bias_ld"])
        ids = rng.choice(vocab, cnt, replace=False).tolist()
        rq["logit_bias"] = {int(i): float(rng.standard_normal() * 3) for i in ids}
        rq["logit_bias"][int(ids[0])] = -float("inf")
    if w["n_ids"]:
        if shape == 1:
            rq.update(stop_ids=rng.integers(0, vocab, w["n_ids"]).tolist(),
                      stop_sequences=[rng.integers(0, vocab, w["seq_ld"]).tolist() for _ in range(w["n_seqs"])], max_new_tokens=(1 << 31) - 1)
        elif shape >= 2:
            rq.update(stop_ids=rng.integers(0, vocab, some(w["n_ids"]) - 1).tolist(),
                      stop_sequences=[rng.integers(0, vocab, some(w["seq_ld"])).tolist() for _ in range(some(w["n_seqs"]) - 1)],
                      max_new_tokens=int(rng.integers(0, 100)))
    if w["hist_cap"]:
        n = (0, w["hist_cap"] - 1, some(w["hist_cap"] - 1), some(w["hist_cap"] - 1))[shape]
        rq["history"] = rng.integers(0, vocab, n).tolist()
    return rq


def poison_penalty_ids(blob, entries, vocab, words):
    """Overwrite words of the blob's packed penalty id lists, in place, with ids the kernel must skip -- what ops.slots_pack never
    packs: -1 padding (first and last word of a list), vocab itself, the last id of the vocabulary's partly used bitmap word (1023 at
    1003 ids), the last bit of a row of `words` words (in the extra word of a wider row), INT32_MAX and INT32_MIN.
    -> (entries with penalty_tokens = the lists as they now stand in the blob, lists touched)"""
    from zhilight_amd import ops
    bad = [-1, vocab, max(vocab, (vocab + 31) // 32 * 32 - 1), max(vocab, words * 32 - 1), (1 << 31) - 1, -(1 << 31), vocab + 1]
    recs, out, touched = ops.slots_records(blob), [], 0
    for r, (s, rq) in zip(recs, entries):
        assert r[0] == s
        if rq is not None and r[11] > 0:
            off, cnt = int(r[10]), int(r[11])
            blob[off:off + min(cnt, len(bad))] = bad[:cnt]
            blob[off + cnt - 1] = -1
            rq = dict(rq, penalty_tokens=blob[off:off + cnt].tolist())
            touched += 1
        out.append((s, rq))
    return out, touched


def expected(ctx, sampler, stop, lookup, entries, vocab, w):
    """The states after the admission, built WITHOUT slot_ref: copies of the inputs whose admitted rows are replaced by what the packing
    code of new_sampler / new_stopper / new_lookup builds for the request alone, parked rows by the park rule, live recounted"""
    from zhilight_amd import ops
    cp = lambda d: None if d is None else {k: v.copy() for k, v in d.items()}                                 # noqa: E731
    ctx, sampler, stop, lookup = cp(ctx), cp(sampler), cp(stop), cp(lookup)
    for s, rq in entries:
        if rq is None:
            ctx["tokens"][s] = ctx["positions"][s] = ctx["placement"][s] = 0
            ctx["valid_lens"][s] = 1
            if stop is not None:
                stop["last_token"][s], stop["emit_lens"][s] = 0, 0
                stop["tail"][s] = -1
            continue
        pending = int(ctx["tokens"][s])
        sampler["temperature"][s], sampler["top_k"][s] = np.float32(rq["temperature"]), rq["top_k"]
        sampler["top_p"][s], sampler["seeds"][s] = np.float32(rq["top_p"]), rq["seed"]
        sampler["draws"][s] = 0
        sampler["logprobs"][s] = sampler["u"][s] = 0
        if "seen" in sampler:
            sampler["repetition_penalty"][s] = np.float32(rq["repetition_penalty"])
            sampler["presence_penalty"][s] = np.float32(rq["presence_penalty"])
            ids = [i for i in [pending] + list(rq.get("penalty_tokens") or []) if 0 <= i < vocab]
            sampler["seen"][s] = pr.pack([ids], vocab, sampler["seen"].shape[1])[0].view(np.int32)
        if "bias_ids" in sampler:
            ids, vals, cnt, bits = ops.logit_bias_rows([rq.get("logit_bias")], vocab)
            ld = sampler["bias_ids"].shape[1]
            sampler["bias_ids"][s], sampler["bias_vals"][s] = -1, 0
            sampler["bias_ids"][s, :cnt[0]], sampler["bias_vals"][s, :cnt[0]] = ids[0, :cnt[0]], vals[0, :cnt[0]]
            assert cnt[0] <= ld
            sampler["bias_cnt"][s] = cnt[0]
            sampler["bias_bits"][s] = 0
            sampler["bias_bits"][s, :bits.shape[1]] = bits[0].view(np.int32)
        if "top_ids" in sampler:
            sampler["top_ids"][s], sampler["top_logprobs"][s] = -1, np.nan
        if stop is not None:
            ids, seqs, lens = ops.stop_rows([(rq.get("stop_ids"), rq.get("stop_sequences"))], vocab)
            stop["stop_ids"][s], stop["stop_seqs"][s], stop["seq_lens"][s] = -1, -1, 0
            stop["stop_ids"][s, :ids.shape[1]] = ids[0]
            stop["stop_seqs"][s, :seqs.shape[1], :seqs.shape[2]] = seqs[0]
            stop["seq_lens"][s, :lens.shape[1]] = lens[0]
            stop["max_new"][s] = rq.get("max_new_tokens", 0)
            fresh = sr.new_state(1, [pending])
            for k in ("gen_lens", "tail", "last_token", "finished"):
                stop[k][s] = fresh[k][0]
            stop["emit_lens"][s] = 0
        if lookup is not None:
            h = np.asarray(rq.get("history") or [], np.int32)
            lookup["history"][s, :h.size], lookup["hist_lens"][s] = h, h.size
    if stop is not None:
        stop["live"][0] = (stop["finished"] == 0).sum()
    return ctx, sampler, stop, lookup


def same(got, want, what):
    """bit equality of every array of two state dicts"""
    if want is None:
        assert got is None
        return
    assert got.keys() == want.keys()
    for k in want:
        g, x = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == x.dtype and g.shape == x.shape, (what, k)
        assert g.tobytes() == x.tobytes(), (what, k)


def scenario(rng, b, vocab, groups, which):
    """(entries, widths): which = "one" slot, "all" slots, "scattered" (slots 0 and b - 1 and some between, one of them parked when the
    stop group is on and the batch has room)"""
    w = widths_of(groups)
    if which == "one":
        slots = [int(rng.integers(0, b))]
    elif which == "all":
        slots = rng.permutation(b).tolist()
    else:
        slots = sorted({0, b - 1} | set(rng.choice(b, max(1, b // 3), replace=False).tolist()))
        slots = [slots[i] for i in rng.permutation(len(slots))]
    entries = [(s, request(rng, vocab, w, (i + (which == "one")) % 4)) for i, s in enumerate(slots)]   # a single slot: the full shape
    if which == "scattered" and len(entries) >= 3:
        entries[1] = (entries[1][0], None)
    return entries, w


@pytest.mark.parametrize("groups", [ALL] + [tuple(g for g in ALL if g != off) for off in ALL], ids=["all"] + ["no-" + g for g in ALL])
@pytest.mark.parametrize("poison", [False, True], ids=["packed", "ids-to-skip"])
@pytest.mark.parametrize("vocab,ld_extra", [(1003, 0), (1003, 1), (128256, 0)], ids=["1003", "1003-odd-rows", "128256"])
@pytest.mark.parametrize("b,which", [(1, "one"), (5, "all"), (5, "scattered"), (33, "scattered"), (33, "one")])
def test_reference_builds_the_rows_of_the_packing_code(b, which, vocab, ld_extra, groups, poison):
    """ids-to-skip: the blob's penalty lists are overwritten with -1 padding and ids at and beyond the vocabulary (poison_penalty_ids);
    `expected` drops them by its own filter and packs the rest with penalty_ref.pack"""
    from zhilight_amd import ops
    rng = np.random.default_rng(b * 7 + vocab + len(groups) + sum(map(ord, which)) + ld_extra)
    entries, w = scenario(rng, b, vocab, groups, which)
    ctx, sampler, stop, lookup = garbage_states(rng, b, vocab, w, groups, ld_extra)
    for s, rq in entries:
        if rq is None and stop is not None:
            stop["finished"][s] = 2                                         # the host parks finished slots only
    blob, hdr = ops.slots_pack(entries, vocab, w)
    if poison:
        entries, touched = poison_penalty_ids(blob, entries, vocab, pr.words(vocab) + ld_extra)
        assert touched or "pen" not in groups or (b == 1 and which != "one")                # a lone slot of the empty shape
    want = expected(ctx, sampler, stop, lookup, entries, vocab, w)
    before = [None if d is None else {k: v.copy() for k, v in d.items()} for d in (ctx, sampler, stop, lookup)]
    draft_new = np.full(b, 12345, np.int32)
    sl.admit(blob, ctx, sampler, stop, lookup, draft_new)
    for got, x, what in zip((ctx, sampler, stop, lookup), want, ("ctx", "sampler", "stop", "lookup")):
        same(got, x, what)
    touched = {s for s, _ in entries}
    rest = [t for t in range(b) if t not in touched]
    for got, old in zip((ctx, sampler, stop, lookup), before):              # rows that are not admitted are unchanged
        if got is not None:
            for k in got:
                if k != "live":
                    assert got[k][rest].tobytes() == old[k][rest].tobytes(), k
    admitted = {s for s, rq in entries if rq is not None}
    assert draft_new.tolist() == [int(ctx["tokens"][t]) if t in admitted else -1 for t in range(b)]
    if stop is not None:
        assert stop["live"][0] == len(admitted) + sum(before[2]["finished"][t] == 0 for t in range(b) if t not in admitted)
        for s, rq in entries:                                               # the park rule
            if rq is None:
                assert stop["finished"][s] == 2 and (ctx["tokens"][s], ctx["positions"][s], ctx["placement"][s], ctx["valid_lens"][s]) == (0, 0, 0, 1)
                assert stop["last_token"][s] == 0 and (stop["tail"][s] == -1).all() and stop["emit_lens"][s] == 0
                assert stop["gen_lens"][s] == before[2]["gen_lens"][s]
                assert sampler["draws"][s] == before[1]["draws"][s]


def test_blob_round_trip():
    from zhilight_amd import ops
    w = dict(penalties=True, bias_ld=4, n_ids=3, n_seqs=2, seq_ld=4, hist_cap=16)
    rq = dict(temperature=0.5, top_k=7, top_p=0.25, seed=-3, repetition_penalty=1.5, presence_penalty=-0.25, penalty_tokens=[1, 1, 5],
              logit_bias={4: -float("inf"), 1: 2.0}, stop_ids=[7], stop_sequences=[[1, 2, 3]], max_new_tokens=9, history=[3, 4])
    blob, h = ops.slots_pack([(2, rq), (0, None)], 100, w)
    assert blob.dtype == np.int32 and blob.flags.c_contiguous and blob.ndim == 1
    rec = 16 + 3 + 2 + 2 * 4
    assert h == dict(magic=ops.SLOT_MAGIC, n=2, vocab=100, flags=15, bias_ld=4, n_ids=3, n_seqs=2, seq_ld=4, rec=rec, var=16 + 2 * rec,
                     total=blob.size, hist_cap=16)
    assert ops.slots_header(blob) == h == sl.header(blob) and not blob[12:16].any()
    r, park = ops.slots_records(blob)
    f = lambda word: np.array([word], np.int32).view(np.float32)[0]                                           # noqa: E731
    assert (r[0], r[1], f(r[2]), r[3], f(r[4]), f(r[7]), f(r[8]), r[9]) == (2, 1, 0.5, 7, 0.25, 1.5, -0.25, 9)
    assert np.array([r[5], r[6]], np.int32).view(np.int64)[0] == -3
    assert blob[r[10]:r[10] + r[11]].tolist() == [1, 1, 5]
    assert blob[r[12]:r[12] + r[13]].tolist() == [1, 4] and blob[r[12] + 2:r[12] + 4].view(np.float32).tolist() == [2.0, -np.inf]
    assert blob[r[14]:r[14] + r[15]].tolist() == [3, 4] and r[14] + r[15] == blob.size
    assert r[16:19].tolist() == [7, -1, -1] and r[19:21].tolist() == [3, 0]                                   # -1 padding, length 0
    assert r[21:].reshape(2, 4).tolist() == [[1, 2, 3, -1], [-1, -1, -1, -1]]
    assert park[0] == 0 and park[1] == 0 and not park[2:16].any() and park[16:19].tolist() == [-1] * 3
    assert ops.slots_pack([(0, {})], 100, ops.slot_widths())[1]["rec"] == 16                                  # the defaults, no option at all
    for bad in (blob[:-1], blob.astype(np.int64), np.zeros(40, np.int32), blob.reshape(1, -1)):
        with pytest.raises(ops.ZLError, match="slots_pack's contiguous int32 array"):
            ops.slots_header(bad)


def test_refusals_of_slots_pack():
    from zhilight_amd import ops
    full = dict(penalties=True, bias_ld=3, n_ids=2, n_seqs=2, seq_ld=3, hist_cap=8)
    bare = ops.slot_widths()
    ok = lambda rq, w=full, slot=0, vocab=50: ops.slots_pack([(slot, rq)], vocab, w)                          # noqa: E731
    ok(dict(temperature=0, penalty_tokens=[49], logit_bias={1: 1.0, 2: 2.0, 3: 3.0}, stop_ids=[1, 2], stop_sequences=[[1, 2, 3], [4]],
            history=list(range(7))))
    cases = [
        (dict(temperature=-1), full, r"temperature >= 0"), (dict(temperature=float("nan")), full, r"temperature >= 0"),
        (dict(top_k=-1), full, r"top_k is an integer >= 0"), (dict(top_k=1.5), full, r"top_k is an integer >= 0"),
        (dict(top_p=1.5), full, r"top_p in \[0, 1\]"), (dict(seed=0.5), full, r"seed is an integer"),
        (dict(repetition_penalty=0), full, r"repetition_penalty > 0 and finite"),
        (dict(presence_penalty=float("inf")), full, r"presence_penalty is finite"),
        (dict(temperature="x"), full, r"are numbers"),
        (dict(penalty_tokens=[50]), full, r"penalty_tokens outside \[0, 50\)"), (dict(penalty_tokens=[-1]), full, r"penalty_tokens outside"),
        (dict(logit_bias={50: 1.0}), full, r"ids outside \[0, 50\)"), (dict(logit_bias={1: float("nan")}), full, r"not NaN or \+inf"),
        (dict(logit_bias={1: 1e39}), full, r"within float32's range"), (dict(logit_bias=[1]), full, r"logit_bias is one dict"),
        (dict(logit_bias={i: 1.0 for i in range(4)}), full, r"4 bias ids, the sampler state holds 3"),
        (dict(stop_ids=[50]), full, r"ids outside \[0, 50\)"), (dict(stop_sequences=[[]]), full, r"a stop sequence has 1 .. 16 ids"),
        (dict(stop_ids=[1, 2, 3]), full, r"beyond the stop state's widths"),
        (dict(stop_sequences=[[1]] * 3), full, r"beyond the stop state's widths"),
        (dict(stop_sequences=[[1, 2, 3, 4]]), full, r"beyond the stop state's widths"),
        (dict(stop_ids=list(range(17))), full, r"17 stop ids, at most 16"),
        (dict(max_new_tokens=-1), full, r"max_new_tokens is an integer >= 0"), (dict(max_new_tokens=1.0), full, r"max_new_tokens is an integer"),
        (dict(history=list(range(8))), full, r"8 ids and the pending token do not fit cap = 8"),
        (dict(history=[50]), full, r"history ids outside \[0, 50\)"),
        (dict(colour=1), full, r"a request is a dict over"),
        # an option the states lack
        (dict(repetition_penalty=1.1), bare, r"the sampler state has no bitmap"), (dict(presence_penalty=0.1), bare, r"no bitmap"),
        (dict(penalty_tokens=[]), bare, r"no bitmap"), (dict(logit_bias={1: 1.0}), bare, r"the sampler state has no bias rows"),
        (dict(stop_ids=[1]), bare, r"there is no stop state"), (dict(stop_sequences=[[1]]), bare, r"no stop state"),
        (dict(max_new_tokens=4), bare, r"no stop state"), (dict(history=[1]), bare, r"there is no lookup state"),
    ]
    for rq, w, msg in cases:
        with pytest.raises(ops.ZLError, match=msg):
            ok(rq, w)
    with pytest.raises(ops.ZLError, match=r"entries, at most 1024"):
        ops.slots_pack([(0, dict(logit_bias={i: 0.5 for i in range(1025)}))], 5000, dict(full, bias_ld=1024))
    ops.slots_pack([(0, dict(logit_bias={i: 0.5 for i in range(1024)}))], 5000, dict(full, bias_ld=1024))
    with pytest.raises(ops.ZLError, match="slot 3 is given twice"):
        ops.slots_pack([(3, {}), (1, None), (3, None)], 50, full)
    for slot in (-1, 1.0, True, 1 << 31):
        with pytest.raises(ops.ZLError, match="a slot is an integer >= 0"):
            ok({}, slot=slot)
    for entries in ([], [3], [(1, 2, 3)]):
        with pytest.raises(ops.ZLError, match="entry"):
            ops.slots_pack(entries, 50, full)
    for vocab in (0, 1 << 31):
        with pytest.raises(ops.ZLError, match="1 <= vocab < 2\\^31"):
            ok({}, vocab=vocab)
    for w in (dict(bias_ld=1025), dict(n_ids=1), dict(n_ids=17, n_seqs=1, seq_ld=1), dict(n_ids=1, n_seqs=9, seq_ld=1),
              dict(n_ids=1, n_seqs=1, seq_ld=17), dict(hist_cap=1)):
        with pytest.raises(ops.ZLError, match="slots_pack"):
            ops.slot_widths(**w)


def test_the_clamp_of_a_slots_length_limit():
    from zhilight_amd import ops
    for prompt_len, max_new, len_buf, k in [(5, 0, 128, 0), (5, 10, 128, 0), (5, 200, 128, 0), (5, 122, 128, 0), (5, 123, 128, 0),
                                            (5, 0, 128, 3), (5, 119, 128, 3), (5, 120, 128, 3), (126, 0, 128, 0), (127, 0, 128, 0),
                                            (123, 7, 128, 3), (124, 7, 128, 3)]:
        lim = ops.slot_max_new(prompt_len, max_new, len_buf, k)
        assert lim == sl.clamp_max_new(prompt_len, max_new, len_buf, k)
        if lim >= 1:
            # the rows a task can touch: its pending token's at prompt_len, one per emitted id, the frozen re-feed at prompt_len + lim,
            # and k draft rows behind any of them
            assert prompt_len + lim + k <= len_buf - 1 and (max_new == 0 or lim <= max_new)
            assert lim == max_new or prompt_len + lim + k + 1 == len_buf                                      # cut no further than needed
    assert ops.slot_max_new(5, 200, 128, 0) == 122 and ops.slot_max_new(5, 0, 128, 3) == 119
    assert ops.slot_max_new(127, 0, 128, 0) == 0 and ops.slot_max_new(124, 7, 128, 3) == 0                    # no room: admit refuses


def test_c_entry_point_refuses_before_any_launch():
    """the header's ZL_EINVAL / ZL_ESHAPE cases on host memory: every one returns before the launch, so nothing runs"""
    from zhilight_amd import _lib
    lib = _lib.lib()
    b = 3
    i32, f32, i64 = (lambda *s: np.zeros(s, np.int32)), (lambda *s: np.zeros(s, np.float32)), (lambda *s: np.zeros(s, np.int64))
    full = dict(blob=i32(64), tokens=i32(b), positions=i32(b), placement=i32(b), valid_lens=i32(b), temperature=f32(b), top_k=i32(b),
                top_p=f32(b), seeds=i64(b), draws=i64(b), logprobs=f32(b), u=f32(b), rep=f32(b), pres=f32(b), seen=i32(b, 4),
                bias_ids=i32(b, 2), bias_vals=f32(b, 2), bias_cnt=i32(b), bias_bits=i32(b, 4), top_ids=i32(b, 2), top_logprobs=f32(b, 2),
                stop_ids=i32(b, 2), stop_seqs=i32(b, 2, 3), seq_lens=i32(b, 2), max_new=i32(b), gen_lens=i32(b), tail=i32(b, 15),
                last_token=i32(b), finished=i32(b), emit_lens=i32(b), live=i32(1), history=i32(b, 8), hist_lens=i32(b), draft_new=i32(b))

    def status(n=1, rec=16 + 2 + 2 + 6, bb=b, vocab=100, seen_ld=4, bias_ld=2, bits_ld=4, top_n=2, n_ids=2, n_seqs=2, ld=3, cap=8, **change):
        a = {**full, **change}
        p = lambda m: C.c_void_p(None if a[m] is None else a[m].ctypes.data)                                  # noqa: E731
        return lib.zl_slots_admit(p("blob"), n, rec, bb, vocab, p("tokens"), p("positions"), p("placement"), p("valid_lens"),
                                  p("temperature"), p("top_k"), p("top_p"), p("seeds"), p("draws"), p("logprobs"), p("u"), p("rep"), p("pres"),
                                  p("seen"), seen_ld, p("bias_ids"), p("bias_vals"), p("bias_cnt"), p("bias_bits"), bias_ld, bits_ld,
                                  p("top_ids"), p("top_logprobs"), top_n, p("stop_ids"), p("stop_seqs"), p("seq_lens"), n_ids, n_seqs, ld,
                                  p("max_new"), p("gen_lens"), p("tail"), p("last_token"), p("finished"), p("emit_lens"), p("live"),
                                  p("history"), cap, p("hist_lens"), p("draft_new"), C.c_void_p(None))

    EINVAL, ESHAPE = -1, -2
    for m in ("blob", "tokens", "positions", "placement", "valid_lens", "top_k", "seeds", "u", "rep", "pres", "bias_vals", "bias_cnt",
              "bias_bits", "top_logprobs", "stop_ids", "stop_seqs", "seq_lens", "max_new", "gen_lens", "last_token", "finished",
              "emit_lens", "live", "hist_lens"):
        assert status(**{m: None}) == EINVAL, m                             # a group given in part
    for kw in (dict(n=0), dict(bb=0), dict(vocab=0), dict(seen_ld=0), dict(bias_ld=0), dict(bits_ld=0), dict(top_n=0), dict(n_ids=0),
               dict(ld=0), dict(rec=16), dict(rec=27), dict(cap=0), dict(n_ids=-1),
               dict(temperature=None, top_k=None, top_p=None, seeds=None, draws=None, logprobs=None, u=None)):        # a bitmap without a sampler
        assert status(**kw) == EINVAL, kw
    for kw in (dict(bb=131073), dict(n=4), dict(vocab=1 << 31), dict(bias_ld=1025), dict(top_n=33), dict(n_ids=17, rec=16 + 17 + 2 + 6),
               dict(n_seqs=9, rec=16 + 2 + 9 + 27), dict(ld=17, rec=16 + 2 + 2 + 34), dict(vocab=129), dict(seen_ld=3), dict(bits_ld=3)):
        assert status(**kw) == ESHAPE, kw
