"""Pure-Python / numpy statement of zl_lookup_draft (the prompt-lookup drafter: append the step's tokens to a task's history, then
propose what followed the latest earlier occurrence of the history's last n-gram), shared by test_lookup_host.py (against a brute-force
maximisation) and the GPU tests."""
import numpy as np


def append(row, length, new_tokens, cap):
    """row: a list of cap ids (changed in place), length: tokens fed so far.  The ids of new_tokens before the first negative one go
    to row[length + j] where that index is below cap and are dropped otherwise; returns the new length, which counts them all"""
    for t in new_tokens:
        if t < 0:
            break
        if 0 <= length < cap:
            row[length] = int(t)
        length += 1
    return length


def draft(h, k, max_ngram, min_ngram):
    """h: the history (a list of L ids) -> (drafts: k ids, -1 padded; (n, s)): for n from min(max_ngram, L - 1) down to min_ngram a
    match is a start s with s + n <= L - 1 and h[s:s+n] == h[L-n:L]; the first n with a match decides, among its matches the largest s
    with k tokens behind it, else the smallest s"""
    L = len(h)
    for n in range(min(max_ngram, L - 1), min_ngram - 1, -1):
        tail = h[L - n:]
        starts = [s for s in range(0, L - n) if h[s:s + n] == tail]
        if not starts:
            continue
        full = [s for s in starts if s + n + k <= L]
        s = max(full) if full else min(starts)
        cont = h[s + n:s + n + k]
        return cont + [-1] * (k - len(cont)), (n, s)
    return [-1] * k, (0, -1)


def lookup(history, hist_lens, k, max_ngram=3, min_ngram=1, new_tokens=None):
    """history (B, cap), hist_lens (B), new_tokens (B, n_new) or None -> (history, hist_lens, drafts (B, k), match (B, 2)) after the
    call, int32 arrays; the inputs are left alone.  A task whose length exceeds cap has overflowed: no drafts, match (0, -1)"""
    hist = np.array(history, np.int32)
    lens = np.array(hist_lens, np.int64)
    b, cap = hist.shape
    drafts, match = np.full((b, k), -1, np.int32), np.zeros((b, 2), np.int32)
    for t in range(b):
        row = hist[t].tolist()
        if new_tokens is not None:
            lens[t] = append(row, int(lens[t]), [int(v) for v in new_tokens[t]], cap)
            hist[t] = row
        d, m = ([-1] * k, (0, -1)) if lens[t] > cap else draft(row[:max(int(lens[t]), 0)], k, max_ngram, min_ngram)
        drafts[t], match[t] = d, m
    return hist, lens.astype(np.int32), drafts, match
