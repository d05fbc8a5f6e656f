"""Host-side pieces of the speculative sampling step: tests/spec_sample_ref.py against a plain per-task loop, the sequence property --
a speculative run emits exactly the tokens of the plain sampling run under the same seeds, whatever the drafter proposes -- on a toy
model, and the conditions the inputs of the GPU distribution test must meet before a GPU ever runs them."""
import numpy as np
import pytest

import sample_ref
import spec_sample_ref as ssr

LAST = ssr.LAST


def _params(rng, rows, n):
    """test_gpu_sample._params, restated here: this file runs without a device"""
    T = rng.choice(np.array([0.3, 0.7, 1.0, 1.5], np.float32), rows)
    T[rng.random(rows) < 0.125] = rng.choice(np.array([0.0, -1.0], np.float32))
    k = rng.choice(np.array([0, 1, 2, 5, 40, n - 1, n + 7], np.int32), rows)
    p = rng.choice(np.array([0.0, 0.1, 0.5, 0.9, 1.0], np.float32), rows)
    u = rng.random(rows).astype(np.float32)
    pick = rng.integers(0, 3, rows)
    u[pick == 0], u[pick == 1] = 0.0, LAST
    return T, k, p, u


def _loop(x, drafts, T, k, p, u, seeds, draws, state):
    """one task at a time, one row at a time, as a sampling loop that stops at the first pick the draft did not foresee"""
    b, len_q = drafts.shape[0], drafts.shape[1] + 1
    out = []
    for t in range(b):
        emitted, lps, d = [], [], int(draws[t])
        for i in range(len_q):
            uu = float(u[t, i]) if u is not None else float(sample_ref.uniforms([seeds[t]], [d])[0])
            row = x[t * len_q + i]
            tok = sample_ref.sample(row, float(T[t]), int(k[t]), float(p[t]), uu)[0]
            emitted.append(tok)
            lps.append(sample_ref.logprob(row, T[t], tok))
            d += 1
            if i == len_q - 1 or int(drafts[t, i]) != tok:
                break
        a = len(emitted) - 1
        out.append(dict(accepted=a, tokens=emitted + [-1] * (len_q - a - 1), lps=lps, draws=d if u is None else int(draws[t]),
                        state=(emitted[-1],) + tuple(int(s[t]) + a + 1 for s in state[1:])))
    return out


@pytest.mark.parametrize("len_q", [2, 4, 32])
@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_reference_against_a_loop(n, len_q):
    rng = np.random.default_rng(100 * n + len_q)
    for b in (1, 3, 8):
        for given in (False, True):
            x = (rng.standard_normal((b * len_q, n)) * rng.choice([0.05, 0.5, 2.0, 8.0], (b * len_q, 1))).astype(np.float16).astype(np.float64)
            T, k, p, _ = _params(rng, b, n)
            u = np.stack([_params(rng, len_q, n)[3] for _ in range(b)]) if given else None
            seeds, draws = rng.integers(-2 ** 62, 2 ** 62, b), rng.integers(0, 1000, b)
            # drafts from the picks themselves, cut at every length 0 .. K, with a -1 and an id >= n among the wrong ones
            full = ssr.spec_sample(x, np.zeros((b, len_q - 1), np.int64), T, k, p, u=u, seeds=seeds, draws=draws)["picks"]
            drafts = full[:, :-1].astype(np.int64).copy()
            for t in range(b):
                cut = int(rng.integers(0, len_q))
                if cut < len_q - 1:
                    drafts[t, cut] = (-1, n, (full[t, cut] + 1) % n if n > 1 else n + 3)[int(rng.integers(0, 3))]
            state = tuple(rng.integers(0, 1000, b).astype(np.int32) for _ in range(4))
            res = ssr.spec_sample(x, drafts, T, k, p, u=u, seeds=seeds, draws=draws, state=state)
            ref = _loop(x, drafts, T, k, p, u, seeds, draws, state)
            for t in range(b):
                a = ref[t]["accepted"]
                assert res["accepted"][t] == a and res["out_tokens"][t].tolist() == ref[t]["tokens"], (b, given, t)
                assert np.array_equal(res["out_logprobs"][t, :a + 1], np.array(ref[t]["lps"])) and np.isnan(res["out_logprobs"][t, a + 1:]).all()
                assert res["logprobs"][t] == ref[t]["lps"][-1] and res["draws"][t] == ref[t]["draws"]
                assert tuple(int(s[t]) for s in res["state"]) == ref[t]["state"]
            assert ((res["picks"] >= 0) & (res["picks"] < n)).all()
            if not given:
                assert np.array_equal(res["u"][:, 0], sample_ref.uniforms(seeds, draws))
                assert np.array_equal(res["u"][:, len_q - 1], sample_ref.uniforms(seeds, draws + len_q - 1))


# ---- the sequence property on a toy model -------------------------------------------------------------------------------------------
TOY_N, TOY_TASKS, TOY_TOKENS, TOY_K = 64, 4, 24, 3
TOY_T = np.array([0.7, 1.0, 1.5, 0.0], np.float32)
TOY_TOPK = np.array([0, 8, 20, 5], np.int32)
TOY_TOPP = np.array([1.0, 0.9, 0.95, 0.5], np.float32)
TOY_SEEDS = np.array([11, 12, -5, 2 ** 40], np.int64)
TOY_FIRST = np.array([3, 60, 17, 33], np.int32)


def toy_table():
    """the toy model: the (64, 64) fp16 logits of the next token, indexed by the previous one"""
    return (np.random.default_rng(64).standard_normal((TOY_N, TOY_N)) * 2.0).astype(np.float16)


def toy_drafters(plain):
    """drafter(task, tokens emitted so far) -> K drafts.  wrong: never the plain run's token; right: the plain run's own continuation;
    random: anything, the drafter's -1 and an id past the vocabulary included"""
    rng = np.random.default_rng(5)
    ahead = lambda t, d: np.array([plain[t][d + i] for i in range(TOY_K)], np.int64)            # noqa: E731
    return {"wrong": lambda t, d: (ahead(t, d) + 1) % TOY_N, "right": ahead,
            "random": lambda t, d: rng.integers(-1, TOY_N + 1, TOY_K)}


def test_sequence_property_on_a_toy_model():
    table = toy_table().astype(np.float64)
    total = TOY_TOKENS + TOY_K + 1                                     # the plain run goes on past the cut: the right drafter looks ahead
    plain = []
    for t in range(TOY_TASKS):
        prev, seq = int(TOY_FIRST[t]), []
        for s in range(total):
            prev = sample_ref.sample(table[prev], float(TOY_T[t]), int(TOY_TOPK[t]), float(TOY_TOPP[t]), sample_ref.uniforms([TOY_SEEDS[t]], [s])[0])[0]
            seq.append(prev)
        plain.append(seq)
    assert all(len(set(seq[:TOY_TOKENS])) > 3 for seq in plain)        # not a constant sequence
    for name, drafter in toy_drafters(plain).items():
        prev, draws = TOY_FIRST.astype(np.int64).copy(), np.zeros(TOY_TASKS, np.int64)
        emitted, steps, all_accepted = [[] for _ in range(TOY_TASKS)], 0, True
        while min(len(e) for e in emitted) < TOY_TOKENS:
            drafts = np.stack([drafter(t, min(int(draws[t]), TOY_TOKENS)) for t in range(TOY_TASKS)])
            fed = np.concatenate([prev[:, None], np.clip(drafts, 0, TOY_N - 1)], axis=1)       # row i sees the draft before it as its input
            res = ssr.spec_sample(table[fed.reshape(-1)], drafts, TOY_T, TOY_TOPK, TOY_TOPP, seeds=TOY_SEEDS, draws=draws)
            for t in range(TOY_TASKS):
                a = int(res["accepted"][t])
                emitted[t] += res["out_tokens"][t, :a + 1].tolist()
                prev[t] = res["out_tokens"][t, a]
                all_accepted &= a == TOY_K or draws[t] >= TOY_TOKENS
            draws = res["draws"]
            assert draws.tolist() == [len(e) for e in emitted]
            steps += 1
        for t in range(TOY_TASKS):
            assert emitted[t][:TOY_TOKENS] == plain[t][:TOY_TOKENS], (name, t)
        if name == "right":
            assert all_accepted and steps == TOY_TOKENS // (TOY_K + 1)
        if name == "wrong":
            assert steps == TOY_TOKENS


# ---- the GPU distribution test's inputs ---------------------------------------------------------------------------------------------
def test_distribution_inputs_meet_their_conditions():
    """before a GPU runs them: under seeds base .. base + 4 095 the REFERENCE's own picks have an acceptance frequency within
    5 sqrt(p (1 - p) / 4096) of p(draft) and every class of row 0 within the same bound of its probability (binomial bounds: a
    correct sampler fails one of the ~10 with probability < 1e-5); the exact fixed-point picks are the float64 rule's; and no
    threshold u cap Z lies within 2^-21 Z of a class boundary, where 2 ulp of an fp32 exponential (2^-22 relative per mass) could move
    a pick between the host's float64 masses and the device's"""
    bits, draft, seeds, prob0 = ssr.distribution_case()
    assert seeds[0] == ssr.DIST_SEED_BASE and seeds.size == ssr.DIST_B == 4096
    assert 2 <= (prob0 > 0).sum() <= 8 and 0.05 < prob0[draft] < 0.5 and prob0[draft] == np.sort(prob0)[-2]
    picks, accepted, u = ssr.distribution_reference(bits, draft, seeds)
    bound = 5 * np.sqrt(prob0 * (1 - prob0) / ssr.DIST_B)
    freq = np.bincount(picks[:, 0], minlength=ssr.DIST_N) / ssr.DIST_B
    assert (np.abs(freq - prob0) <= bound).all()
    assert abs(accepted.mean() - prob0[draft]) <= bound[draft]
    assert np.array_equal(accepted == 1, picks[:, 0] == draft)
    for i in range(2):
        x = sample_ref.values_of(bits[i], False)
        for t in range(ssr.DIST_B):
            pick, pos, c, v, order = sample_ref.sample(x, ssr.DIST_T, ssr.DIST_K, ssr.DIST_P, u[t, i])
            assert pick == picks[t, i]
            assert np.abs(c[:ssr.DIST_K] - v).min() > 2.0 ** -21 * c[-1], (i, t)
    # FixedRow is sample_ref.sample_sorted_fixed, call by call
    row = ssr.FixedRow(bits[0], False, ssr.DIST_T)
    for t in range(0, ssr.DIST_B, 64):
        assert row.pick(ssr.DIST_K, ssr.DIST_P, float(u[t, 0])) == sample_ref.sample_sorted_fixed(bits[0], False, ssr.DIST_T, ssr.DIST_K, ssr.DIST_P, float(u[t, 0]))
