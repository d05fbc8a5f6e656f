"""Host-side pieces of the speculative verify step: ops.causal_step_mask and the numpy accept reference (tests/spec_ref.py) against
brute-force loops, and the argument checks of ops.spec_accept that need no device."""
import numpy as np
import pytest
import torch

import spec_ref


def test_causal_step_mask_against_triple_loop():
    from zhilight_amd import ops
    lens = [1, 5, 64, 33, 130, 7]
    valid = [1, 2, 61, 33, 1, 0]
    for len_q in (1, 2, 4, 7):
        ref = []
        for L, v in zip(lens, valid):
            for qi in range(len_q):
                for j in range(L):
                    ref.append(1 if j < min(L, v + qi) else 0)
        for args in ((lens, valid), (torch.tensor(lens, dtype=torch.int32), np.array(valid, np.int32))):
            got = ops.causal_step_mask(args[0], args[1], len_q)
            assert got.dtype == torch.int8 and got.dim() == 1
            assert got.tolist() == ref
    with pytest.raises(ops.ZLError):
        ops.causal_step_mask([4, 4], [1], 2)
    with pytest.raises(ops.ZLError):
        ops.causal_step_mask([4], [1], 0)


def _accept_loop(picks, drafts):
    b, len_q = len(picks), len(picks[0])
    acc, out = [], []
    for t in range(b):
        n = 0
        while n < len_q - 1 and drafts[t][n] == picks[t][n]:
            n += 1
        acc.append(n)
        out.append([picks[t][j] if j <= n else -1 for j in range(len_q)])
    return acc, out


@pytest.mark.parametrize("k", [1, 3, 7])
def test_accept_reference_against_loop(k):
    rng = np.random.default_rng(k)
    b = 64
    picks = rng.integers(0, 4, (b, k + 1))
    drafts = rng.integers(0, 4, (b, k))
    drafts[0] = picks[0, :k]                      # all accepted
    drafts[1] = (picks[1, :k] + 1) % 4            # none accepted
    drafts[2] = picks[2, :k]
    drafts[2, k - 1] = (picks[2, k - 1] + 1) % 4  # all but the last
    if k > 1:
        drafts[3] = picks[3, :k]
        drafts[3, 0] = (picks[3, 0] + 1) % 4      # a match BEHIND a mismatch does not count
    for n in range(k + 1):                        # every count from 0 to K, by construction
        drafts[4 + n] = picks[4 + n, :k]
        if n < k:
            drafts[4 + n, n] = (picks[4 + n, n] + 1) % 4
    acc, out = spec_ref.accept(picks, drafts)
    racc, rout = _accept_loop(picks.tolist(), drafts.tolist())
    assert acc.dtype == np.int32 and out.dtype == np.int32
    assert acc.tolist() == racc and out.tolist() == rout
    assert acc[0] == k and (out[0] == picks[0]).all()
    assert acc[1] == 0 and out[1, 0] == picks[1, 0] and (out[1, 1:] == -1).all()
    assert acc[2] == k - 1 and out[2, k] == -1
    assert acc[4:5 + k].tolist() == list(range(k + 1))
    tok, pos, plc, val = spec_ref.advance(acc, out, np.zeros(b), np.arange(b), np.arange(b) + 1, np.arange(b) + 2)
    for t in range(b):
        assert tok[t] == picks[t, racc[t]] and pos[t] == t + racc[t] + 1 and plc[t] == t + racc[t] + 2 and val[t] == t + racc[t] + 3


def test_argmax_reference_ties_and_nan():
    x = np.array([[1.0, 3.0, 3.0, 0.0], [2.0, np.nan, 5.0, np.nan], [-0.0, 0.0, -1.0, 0.0], [np.inf, np.nan, np.inf, 0.0]])
    assert spec_ref.argmax_rows(x).tolist() == [1, 1, 0, 1]


def test_spec_accept_argument_checks():
    """every ZLError of ops.spec_accept that is decided before a device is touched, each by its own message: the checks run in
    this order, and the host logits used here are refused LAST, so a deleted check would surface as the wrong message"""
    from zhilight_amd import ops
    logits = torch.zeros((8, 16), dtype=torch.float16)
    drafts = torch.zeros((2, 3), dtype=torch.int32)
    bad = [
        (logits, [[0, 0, 0], [0, 0, 0]], "are tensors"),                                   # not a tensor
        (logits.view(-1), drafts, "unit column stride"),                                   # not 2-D
        (logits.t(), drafts, "unit column stride"),                                        # column stride
        (logits.to(torch.float64), drafts, "unsupported logits dtype"),                    # dtype
        (logits.to(torch.int32), drafts, "unsupported logits dtype"),
        (logits, drafts.to(torch.int64), "drafts are"),                                    # drafts dtype
        (logits, drafts.view(-1), "drafts are"),                                           # drafts 1-D
        (logits, torch.zeros((2, 0), dtype=torch.int32), "drafts are"),                    # K = 0
        (logits, torch.zeros((4, 6), dtype=torch.int32)[:, ::2], "drafts are"),            # not contiguous
        (logits, torch.zeros((3, 3), dtype=torch.int32), "one logit row per task"),        # rows != B * (K + 1)
        (logits, torch.zeros((4, 3), dtype=torch.int32), "one logit row per task"),
        (logits, drafts, "CUDA logits"),                                                   # everything right but the device
    ]
    for lg, dr, msg in bad:
        with pytest.raises(ops.ZLError, match=msg):
            ops.spec_accept(lg, dr)
