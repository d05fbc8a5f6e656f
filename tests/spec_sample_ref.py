"""numpy statement of zl_spec_sample_accept (the acceptance of a speculative step under sampling and the roll-back of the batch state),
shared by test_spec_sample_host.py (against a per-task loop) and the GPU tests.  It sits on sample_ref (the pick, the uniforms, the
log-probability) and spec_ref (the prefix match, the state's advance) and adds what is the call's own: per-task parameters expanded
over a task's rows, the counter draws[t] + i of row (t, i), the NaN padding and the draws' advance by accepted + 1."""
import numpy as np

import sample_ref
import spec_ref

LAST = float(np.float32(1 - 2.0 ** -24))


def rule_pick(x, T, top_k, top_p, u):
    """the float64 rule on one row of values"""
    return sample_ref.sample(x, T, top_k, top_p, u)[0]


class FixedRow:
    """sample_ref.sample_sorted_fixed on ONE row of 16-bit patterns for many (top_k, top_p, u) at one temperature: the integer masses,
    the order and the running sums are computed once.  pick() equals sample_ref.sample_sorted_fixed(bits, bf16, T, ...) call by call"""

    def __init__(self, bits, bf16, T):
        self.bits, self.bf16, self.T = sample_ref.bits_of(bits), bf16, float(T)
        self.n = self.bits.size
        self.x = sample_ref.values_of(self.bits, bf16)
        q, _ = sample_ref.fixed_masses(self.bits, bf16, T)
        keys = sample_ref.keys_of(self.bits)
        self.order = np.lexsort((np.arange(self.n), -keys.astype(np.int64)))
        self.c = [int(v) for v in np.cumsum(q[self.order])]

    def pick(self, top_k, top_p, u):
        v = sample_ref._threshold(u, top_p, self.c[-1], self.c[top_k - 1] if 0 < top_k < self.n else None)
        return int(self.order[next(i for i in range(self.n) if self.c[i] >= v)])


def row_uniforms(seeds, draws, len_q):
    """(b, len_q) float32: row (t, i) draws the Philox word of key seeds[t] at counter draws[t] + i"""
    seeds, draws = np.asarray(seeds, np.int64), np.asarray(draws, np.int64)
    return np.stack([sample_ref.uniforms(seeds, [int(d) + i for d in draws]) for i in range(len_q)], axis=1)


def spec_sample(logits, drafts, T, top_k, top_p, u=None, seeds=None, draws=None, state=None, pick=rule_pick):
    """logits (b * len_q, n) values, task-major; drafts (b, len_q - 1); T / top_k / top_p / seeds / draws per task (b); u per row
    (b, len_q) or None (then seeds and draws give the uniforms); state = (tokens, positions, placement, valid_lens) per task or None.
    pick(x_row, T, top_k, top_p, u) -> class: the rule for rows that have a distribution (T <= 0 and NaN / infinite rows take the
    arg-max here).  Returns a dict: picks (b, len_q) before the padding, accepted (b), out_tokens (b, len_q), out_logprobs (b, len_q)
    float64 (NaN behind the bonus token), logprobs (b), u (b, len_q) as used, draws (b) afterwards (None where u was given and no
    draws), state afterwards (None without one)"""
    x = np.asarray(logits, np.float64)
    drafts = np.asarray(drafts, np.int64)
    b, len_q = drafts.shape[0], drafts.shape[1] + 1
    assert x.shape[0] == b * len_q and len_q >= 2
    generated = u is None
    u = row_uniforms(seeds, draws, len_q) if generated else np.asarray(u, np.float32).reshape(b, len_q)
    picks = np.empty((b, len_q), np.int64)
    lp = np.empty((b, len_q), np.float64)
    for t in range(b):
        for i in range(len_q):
            row = x[t * len_q + i]
            uu = float(u[t, i])
            uu = (uu if uu < 1.0 else LAST) if uu >= 0.0 else 0.0                      # the kernel's clamps: u into [0, 1), top_p into [0, 1]
            pp = float(top_p[t])
            pp = (pp if pp < 1.0 else 1.0) if pp >= 0.0 else 0.0
            if not T[t] > 0 or sample_ref.is_plain(row):
                picks[t, i] = sample_ref.argmax(row)
            else:
                picks[t, i] = pick(row, float(T[t]), int(top_k[t]), pp, uu)
            with np.errstate(all="ignore"):
                lp[t, i] = np.nan if sample_ref.is_plain(row) else sample_ref.logprob(row, T[t], int(picks[t, i]))
    accepted, out = spec_ref.accept(picks, drafts)
    out_lp = np.where(np.arange(len_q)[None, :] <= accepted[:, None], lp, np.nan)
    res = dict(picks=picks.astype(np.int32), accepted=accepted, out_tokens=out, out_logprobs=out_lp, row_logprobs=lp,
               logprobs=lp[np.arange(b), accepted], u=u, draws=None, state=None)
    if draws is not None:
        res["draws"] = np.asarray(draws, np.int64) + (accepted.astype(np.int64) + 1 if generated else 0)
    if state is not None:
        res["state"] = spec_ref.advance(accepted, out, *state)
    return res


# ---- the inputs of the distribution test, shared by the host conditions and the GPU run --------------------------------------------
# the seed base: bases 0 and 4 096 meet the binomial bounds too, but each has one threshold within 2^-21 Z of a class boundary (0.38 and
# 0.15 of that margin), where the device's fp32 exponentials may tip the pick; under 8 192 the closest is 2.4 margins away
DIST_B, DIST_N, DIST_T, DIST_K, DIST_P, DIST_SEED_BASE = 4096, 257, 1.0, 8, 0.9, 8192


def distribution_case():
    """one (2, 257) fp16 row pair shared by 4 096 tasks of len_q = 2 -> (bits (2, 257) uint16, draft = the second most probable class
    of row 0, seeds (4 096) int64, prob0 = the exact class probabilities of row 0 under T = 1, top_k = 8, top_p = 0.9)"""
    rng = np.random.default_rng(41)
    bits = (rng.standard_normal((2, DIST_N)) * 1.0).astype(np.float16).view(np.uint16)
    prob0 = sample_ref.probabilities(sample_ref.values_of(bits[0], False), DIST_T, DIST_K, DIST_P)
    draft = int(np.argsort(-prob0, kind="stable")[1])
    seeds = DIST_SEED_BASE + np.arange(DIST_B, dtype=np.int64)
    return bits, draft, seeds, prob0


def distribution_reference(bits, draft, seeds):
    """spec_sample over the 4 096 tasks with the pick in its exact fixed-point form -> (picks (4 096, 2), accepted (4 096), u)"""
    rows = [FixedRow(bits[i], False, DIST_T) for i in range(2)]
    u = row_uniforms(seeds, np.zeros(len(seeds), np.int64), 2)
    picks = np.array([[rows[i].pick(DIST_K, DIST_P, float(u[t, i])) for i in range(2)] for t in range(len(seeds))], np.int32)
    accepted, _ = spec_ref.accept(picks, np.full((len(seeds), 1), draft))
    return picks, accepted, u
