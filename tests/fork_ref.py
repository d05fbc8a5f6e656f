"""A numpy model of zl_kv_fork (include/zhilight_amd.h): the copy rule, the bookkeeping rule and the dropped descriptors.

bufs: one uint8 array per task, (layers, 2, len, hkv, row_bytes) under BSHD and (layers, 2, hkv, len, row_bytes) under BHSD; ctx: a
dict of the four (B) int32 vectors tokens / positions / placement / valid_lens, or None for a call without bookkeeping.  Both are
changed in place.  The caller keeps the C call's promises (no task a destination twice, no destination a source, the override rule), so
the order in which the descriptors are applied does not matter."""
import numpy as np

CTX = ("tokens", "positions", "placement", "valid_lens")


def dropped(d, buf_lens, max_rows):
    src, dst, rows, _ = (int(x) for x in d)
    b = len(buf_lens)
    return (not 0 <= src < b or not 0 <= dst < b or rows < 0 or rows > max_rows or rows > buf_lens[src] or rows > buf_lens[dst])


def fork(desc, bufs, buf_lens, bshd, max_rows, ctx=None):
    """-> the descriptors that were carried out"""
    done = []
    old_tokens = None if ctx is None else ctx["tokens"].copy()              # a destination reads what the launch found
    for d in desc:
        if dropped(d, buf_lens, max_rows):
            continue
        src, dst, rows, token = (int(x) for x in d)
        done.append((src, dst, rows, token))
        if src != dst:
            if bshd:
                bufs[dst][:, :, :rows] = bufs[src][:, :, :rows]
            else:
                bufs[dst][:, :, :, :rows] = bufs[src][:, :, :, :rows]
        if ctx is not None:
            if src != dst:
                for f in CTX[1:]:
                    ctx[f][dst] = ctx[f][src]
                ctx["tokens"][dst] = token if token >= 0 else old_tokens[src]
            elif token >= 0:
                ctx["tokens"][src] = token
    return done
