"""Host-side pieces of the prompt-lookup drafter: the reference statement of zl_lookup_draft (tests/lookup_ref.py) against a brute-force
maximisation of the kernel's key and hand cases, and the argument checks of ops.lookup_draft that need no device."""
import numpy as np
import pytest
import torch

import lookup_ref


def _brute(h, k, max_ngram, min_ngram):
    """over all (s, n): the largest (n, c = min(k, L - s - n), s if c == k else -s)"""
    L, best = len(h), None
    for n in range(min_ngram, min(max_ngram, L - 1) + 1):
        for s in range(0, L - n):
            if h[s:s + n] != h[L - n:]:
                continue
            c = min(k, L - s - n)
            key = (n, c, s if c == k else -s)
            if best is None or key > best[0]:
                best = (key, s)
    if best is None:
        return [-1] * k, (0, -1)
    (n, c, _), s = best
    return h[s + n:s + n + c] + [-1] * (k - c), (n, s)


def test_reference_against_brute_force():
    rng = np.random.default_rng(11)
    matched = partial = 0
    for _ in range(4000):
        alphabet = int(rng.integers(2, 6))
        h = rng.integers(0, alphabet, int(rng.integers(1, 41))).tolist()
        k, max_ngram = int(rng.integers(1, 7)), int(rng.integers(1, 5))
        min_ngram = int(rng.integers(1, max_ngram + 1))
        got = lookup_ref.draft(h, k, max_ngram, min_ngram)
        assert got == _brute(h, k, max_ngram, min_ngram), (h, k, max_ngram, min_ngram)
        matched += got[1][0] > 0
        partial += got[1][0] > 0 and got[0][-1] == -1
    assert matched > 2000 and partial > 100            # both branches of the choice are exercised


def test_hand_cases():
    assert lookup_ref.draft([7, 1, 2, 3, 9, 9, 7], 3, 3, 1) == ([1, 2, 3], (1, 0))
    # a a a a: no match has 3 tokens behind it, so the earliest one wins (n = 3: s = 0 only; n = 1: s = 0, 1, 2 -> 0)
    assert lookup_ref.draft([5, 5, 5, 5], 3, 3, 1) == ([5, -1, -1], (3, 0))
    assert lookup_ref.draft([5, 5, 5, 5], 3, 1, 1) == ([5, 5, 5], (1, 0))
    assert lookup_ref.draft([5, 5, 5, 5], 4, 1, 1) == ([5, 5, 5, -1], (1, 0))
    # the latest match with a full continuation beats an earlier one; a later one without it does not count
    assert lookup_ref.draft([1, 2, 3, 1, 4, 5, 1, 6, 1], 3, 1, 1) == ([4, 5, 1], (1, 3))
    assert lookup_ref.draft([1, 2, 3, 1, 4, 5, 1, 6, 1], 2, 1, 1) == ([6, 1], (1, 6))          # (one token short of full / just full)
    # the longer n-gram decides before any continuation is looked at
    assert lookup_ref.draft([1, 2, 9, 8, 7, 2, 6, 6, 6, 1, 2], 3, 2, 1) == ([9, 8, 7], (2, 0))
    assert lookup_ref.draft([1, 2, 3], 2, 3, 2) == ([-1, -1], (0, -1))            # a match of one id is below min_ngram
    assert lookup_ref.draft([4], 2, 3, 1) == ([-1, -1], (0, -1))                  # L = 1
    assert lookup_ref.draft([], 2, 3, 1) == ([-1, -1], (0, -1))
    assert lookup_ref.draft([4, 4], 2, 3, 1) == ([4, -1], (1, 0))                 # L = 2: the continuation is the suffix itself


def test_append_and_overflow():
    hist = np.full((3, 6), 77, np.int32)
    hist[0, :4], hist[1, :5], hist[2, :2] = [1, 2, 1, 2], [1, 2, 3, 1, 2], [9, 9]
    new = np.array([[1, -1, 5], [3, 1, -1], [-1, 3, 3]], np.int32)
    h, lens, drafts, match = lookup_ref.lookup(hist, [4, 5, 2], 2, 2, 1, new)
    assert lens.tolist() == [5, 7, 2]
    assert h[0].tolist() == [1, 2, 1, 2, 1, 77] and drafts[0].tolist() == [2, 1] and match[0].tolist() == [2, 1]   # 5 behind the -1: not fed
    assert h[1].tolist() == [1, 2, 3, 1, 2, 3]          # the seventh token is dropped, the length counts it
    assert drafts[1].tolist() == [-1, -1] and match[1].tolist() == [0, -1]                                        # the overflow row
    assert h[2].tolist() == hist[2].tolist() and drafts[2].tolist() == [9, -1] and match[2].tolist() == [1, 0]     # nothing appended
    assert hist[1, 5] == 77                              # the inputs are left alone
    # cap reached exactly is no overflow
    h, lens, drafts, match = lookup_ref.lookup(hist, [4, 5, 2], 2, 2, 1, np.array([[1, 2], [3, -1], [-1, -1]], np.int32))
    assert lens.tolist() == [6, 6, 2] and drafts[1].tolist() == [1, 2] and match[1].tolist() == [2, 1]
    # without new tokens the call only drafts
    h, lens, drafts, match = lookup_ref.lookup(hist, [4, 5, 2], 2, 2, 1)
    assert lens.tolist() == [4, 5, 2] and np.array_equal(h, hist) and drafts[1].tolist() == [3, 1]


def test_lookup_draft_argument_checks():
    """every ZLError of ops.lookup_draft that is decided before a device is touched, each by its own message: the checks run in this
    order, and the host tensors used here are refused LAST, so a deleted check would surface as the wrong message"""
    from zhilight_amd import ops
    i32 = torch.int32
    hist, lens = torch.zeros((2, 8), dtype=i32), torch.zeros(2, dtype=i32)
    new = torch.zeros((2, 4), dtype=i32)
    bad = [
        (dict(history=hist.tolist()), "are tensors"),
        (dict(hist_lens=[0, 0]), "are tensors"),
        (dict(history=hist.view(-1)), "history is"),                                              # 1-D
        (dict(history=hist.to(torch.int64)), "history is"),                                       # dtype
        (dict(history=torch.zeros((2, 16), dtype=i32)[:, ::2]), "history is"),                    # not contiguous
        (dict(history=torch.zeros((2, 1), dtype=i32)), "history is"),                             # cap < 2
        (dict(history=torch.zeros((0, 8), dtype=i32), hist_lens=torch.zeros(0, dtype=i32)), "history is"),   # B = 0
        (dict(history=torch.empty((2, 1 << 31), dtype=i32, device="meta")), "fewer than 2\\^31"),
        (dict(hist_lens=lens.to(torch.int64)), "hist_lens is"),
        (dict(hist_lens=torch.zeros(3, dtype=i32)), "hist_lens is"),
        (dict(hist_lens=torch.zeros((2, 1), dtype=i32)), "hist_lens is"),
        (dict(hist_lens=torch.zeros(4, dtype=i32)[::2]), "hist_lens is"),
        (dict(k=0), "1 <= k <= 31"),
        (dict(k=32), "1 <= k <= 31"),
        (dict(min_ngram=0), "min_ngram <= max_ngram"),
        (dict(max_ngram=2, min_ngram=3), "min_ngram <= max_ngram"),
        (dict(max_ngram=17), "min_ngram <= max_ngram"),
        (dict(new_tokens=new.tolist()), "new_tokens is"),
        (dict(new_tokens=new.to(torch.int64)), "new_tokens is"),
        (dict(new_tokens=new.view(-1)), "new_tokens is"),
        (dict(new_tokens=torch.zeros((3, 4), dtype=i32)), "new_tokens is"),                       # another batch
        (dict(new_tokens=torch.zeros((2, 0), dtype=i32)), "new_tokens is"),                       # n_new = 0
        (dict(new_tokens=torch.zeros((2, 33), dtype=i32)), "new_tokens is"),                      # n_new > 32
        (dict(new_tokens=torch.zeros((2, 8), dtype=i32)[:, ::2]), "new_tokens is"),
        (dict(drafts=torch.zeros((2, 3), dtype=torch.int64)), "drafts:"),
        (dict(drafts=torch.zeros((2, 4), dtype=i32)), "drafts:"),                                 # k = 3 asked
        (dict(drafts=torch.zeros((2, 6), dtype=i32)[:, ::2]), "drafts:"),
        (dict(match=torch.zeros((2, 2), dtype=torch.int64)), "match:"),
        (dict(match=torch.zeros((2, 3), dtype=i32)), "match:"),
        (dict(match=torch.zeros((2, 4), dtype=i32)[:, ::2]), "match:"),
        (dict(), "CUDA history"),                                                                 # everything right but the device
        (dict(new_tokens=new, drafts=torch.zeros((2, 3), dtype=i32), match=torch.zeros((2, 2), dtype=i32)), "CUDA history"),
    ]
    for change, msg in bad:
        kw = dict(history=hist, hist_lens=lens, k=3, max_ngram=3, min_ngram=1)
        kw.update(change)
        with pytest.raises(ops.ZLError, match=msg):
            ops.lookup_draft(**kw)
