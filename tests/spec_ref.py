"""numpy statement of zl_spec_accept (the greedy acceptance of a speculative step and the roll-back of the batch state), shared by
test_spec_host.py (against a brute-force loop) and the GPU tests."""
import numpy as np


def argmax_rows(logits):
    """per-row arg-max under zl_argmax_advance's rule: the lowest index of the largest value, a NaN counting as largest"""
    x = np.asarray(logits, np.float64)
    x = np.where(np.isnan(x), np.inf, x)
    nan_first = np.isnan(np.asarray(logits, np.float64))
    picks = np.argmax(x, axis=1)
    any_nan = nan_first.any(axis=1)
    picks[any_nan] = np.argmax(nan_first[any_nan], axis=1)
    return picks.astype(np.int32)


def accept(picks, drafts):
    """picks (B, K + 1), drafts (B, K) -> (accepted (B) int32, out_tokens (B, K + 1) int32): accepted = length of the longest prefix
    of the drafts that the picks confirm, out_tokens = picks[:, :accepted + 1], -1 behind them"""
    picks, drafts = np.asarray(picks, np.int64), np.asarray(drafts, np.int64)
    b, len_q = picks.shape
    assert drafts.shape == (b, len_q - 1)
    confirmed = np.cumprod(picks[:, :-1] == drafts, axis=1)
    accepted = confirmed.sum(axis=1).astype(np.int32)
    out = np.where(np.arange(len_q)[None, :] <= accepted[:, None], picks, -1).astype(np.int32)
    return accepted, out


def advance(accepted, out_tokens, tokens, positions, placement, valid_lens):
    """the state after the step: tokens = the pick behind the accepted drafts, the three counters += accepted + 1"""
    accepted = np.asarray(accepted, np.int32)
    new_tokens = np.asarray(out_tokens)[np.arange(accepted.size), accepted].astype(np.int32)
    return (new_tokens,) + tuple((np.asarray(v, np.int32) + accepted + 1).astype(np.int32) for v in (positions, placement, valid_lens))
