"""PrefixIndex (zhilight_amd/prefix_cache.py), the host side of the prompt prefix cache: match lengths, the chained identity of a
block (its whole token prefix), digest collisions, LRU order and eviction, reserve under a full pool, the counters.  No device."""
import pytest

from zhilight_amd import prefix_cache
from zhilight_amd.prefix_cache import PrefixIndex

BS = 4


def _blk(tag, bs=BS):
    """one block of tokens that differs from every other tag's in every position"""
    return [tag * 100 + i for i in range(bs)]


X, Y, Z, W = _blk(1), _blk(2), _blk(3), _blk(4)


def test_imports_without_torch_or_device():
    import subprocess
    import sys
    code = ("import sys, importlib.util as u; s = u.spec_from_file_location('pc', %r); m = u.module_from_spec(s); s.loader.exec_module(m); "
            "m.PrefixIndex(2, 4, 2); assert 'torch' not in sys.modules" % prefix_cache.__file__)
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0


@pytest.mark.parametrize("extra,want", [(0, 0), (1, 1)])
def test_match_lengths_keep_one_token_to_encode(extra, want):
    idx = PrefixIndex(8, BS, 8)
    long = X + Y + Z + [7]
    assert [i for i, _ in idx.put(long)] == [0, 1, 2]
    # block_size (+1) tokens: the block is matched only if a token is left behind it
    assert len(idx.match((X + [7])[:BS + extra])) == want
    # 2 * block_size (+1)
    assert len(idx.match((X + Y + [7])[:2 * BS + extra])) == 1 + want
    assert idx.match([]) == [] and idx.match(X[:1]) == []


def test_match_and_reserve_respect_max_blocks():
    idx = PrefixIndex(8, BS, 2)
    long = X + Y + Z + W + [7]
    assert [i for i, _ in idx.put(long)] == [0, 1]               # only the first max_blocks blocks are stored
    assert len(idx.match(long)) == 2
    assert len(idx) == 2
    idx0 = PrefixIndex(8, BS, 0)
    assert idx0.put(long) == [] and idx0.match(long) == []


def test_put_of_an_exact_multiple_stores_the_last_block_and_match_leaves_it():
    idx = PrefixIndex(8, BS, 8)
    assert [i for i, _ in idx.put(X + Y)] == [0, 1]
    assert len(idx.match(X + Y)) == 1                            # (8 - 1) // 4
    assert len(idx.match(X + Y + [5])) == 2
    assert idx.put(X + Y + [5]) == []                            # nothing new


def test_a_block_is_identified_by_the_whole_prefix():
    """after put [X, Y, t] and put [Z, Y, t] the two Y blocks are different pool blocks, and each prompt gets its own"""
    idx = PrefixIndex(8, BS, 8)
    a = dict(idx.put(X + Y + [9]))
    b = dict(idx.put(Z + Y + [9]))
    assert sorted(a) == sorted(b) == [0, 1]
    assert len({a[0], a[1], b[0], b[1]}) == 4
    assert idx.match(Z + Y + [9]) == [b[0], b[1]]
    assert idx.match(X + Y + [9]) == [a[0], a[1]]
    assert idx.match(W + Y + [9]) == []                          # Y behind an unknown block is nobody's
    assert idx.match(Y + [9]) == []                              # nor is Y as block 0


def test_forced_digest_collisions_return_only_equal_tokens(monkeypatch):
    monkeypatch.setattr(prefix_cache, "_digest", lambda prev, block_tokens: 42)
    idx = PrefixIndex(16, BS, 8)
    a = dict(idx.put(X + Y + Z + [9]))
    b = dict(idx.put(Z + Y + X + [9]))
    c = dict(idx.put(X + Z + [9]))                               # shares block 0 with a
    assert sorted(c) == [1] and len(set(a.values()) | set(b.values()) | set(c.values())) == 7
    assert idx.match(X + Y + Z + [9]) == [a[0], a[1], a[2]]
    assert idx.match(Z + Y + X + [9]) == [b[0], b[1], b[2]]
    assert idx.match(X + Z + [9]) == [a[0], c[1]]
    assert idx.match(X + Y + X + [9]) == [a[0], a[1]]            # the third block's tokens differ: a miss there, not b's block
    assert idx.match(Y + X + [9]) == []
    assert idx.match(W + [9]) == []


def test_lru_order_across_two_chains():
    idx = PrefixIndex(4, BS, 8)
    a = dict(idx.put(X + Y + [9]))
    b = dict(idx.put(Z + W + [9]))
    # each chain is touched deepest block first: least recent first is a's tail, a's head, b's tail, b's head
    assert idx.lru_order() == [a[1], a[0], b[1], b[0]]
    assert idx.match(X + Y + [9]) == [a[0], a[1]]                # a hit makes chain a the more recent one
    assert idx.lru_order() == [b[1], b[0], a[1], a[0]]
    c = dict(idx.put(_blk(5) + [9]))                             # full pool: the least recent block goes, chain b's tail
    assert c[0] == b[1] and idx.evictions == 1
    assert idx.match(Z + W + [9]) == [b[0]]
    assert idx.match(X + Y + [9]) == [a[0], a[1]]


def test_a_chain_loses_its_tail_first():
    idx = PrefixIndex(3, BS, 8)
    a = dict(idx.put(X + Y + Z + [9]))
    idx.put(_blk(5) + [9])
    assert idx.match(X + Y + Z + [9]) == [a[0], a[1]]
    idx.put(_blk(6) + [9])                                       # the least recent now is block 5's, not a's: the hit refreshed a
    assert idx.match(X + Y + Z + [9]) == [a[0], a[1]]
    idx.put(_blk(7) + [9])
    idx.put(_blk(8) + _blk(9) + [9])
    assert idx.match(X + Y + Z + [9]) in ([a[0]], [])            # whatever is left of a is a head, never a tail without it
    assert len(idx) == 3


def test_matched_blocks_survive_the_same_calls_reserve():
    idx = PrefixIndex(3, BS, 8)
    a = dict(idx.put(X + Y + [9]))
    idx.put(_blk(5) + [9])                                       # pool full: X, Y, 5
    prompt = X + Y + Z + W + [9]
    hit = idx.match(prompt)
    assert hit == [a[0], a[1]]
    pairs = idx.reserve(prompt)                                  # needs two blocks, only block 5's may go
    assert [i for i, _ in pairs] == [2] and pairs[0][1] not in hit
    assert idx.evictions == 1
    assert idx.match(prompt) == hit                              # the reserved block is pending: not matched before commit
    idx.commit([pairs[0][1]])
    assert idx.match(prompt) == hit + [pairs[0][1]]
    # `keep`: ids another prompt of the same step matched are not evicted either
    idx2 = PrefixIndex(2, BS, 8)
    k = dict(idx2.put(X + [9]))
    idx2.put(Y + [9])
    assert idx2.reserve(Z + W + [9], keep=set(idx2.lru_order())) == []
    got = idx2.reserve(Z + W + [9], keep={k[0]})
    assert [i for i, _ in got] == [0] and got[0][1] != k[0]      # one block could go; the second has nowhere to be placed


def test_reserve_stops_at_the_first_block_it_cannot_place():
    idx = PrefixIndex(3, BS, 8)
    prompt = X + Y + Z + W + _blk(5) + [9]
    pairs = idx.put(prompt)
    assert [i for i, _ in pairs] == [0, 1, 2] and idx.evictions == 0      # a prompt never evicts its own chain
    assert idx.match(prompt) == [p for _, p in pairs]
    assert idx.put(prompt) == []                                 # block 3 still has no place: everything else is its own chain
    other = Y + X + [9]
    got = idx.put(other)
    assert [i for i, _ in got] == [0, 1] and idx.evictions == 2
    assert [p for _, p in got] == [pairs[2][1], pairs[1][1]]     # the old chain's tail went first
    assert idx.match(prompt) == [pairs[0][1]]


def test_pending_blocks_are_shared_and_abort_returns_them():
    idx = PrefixIndex(4, BS, 8)
    first = idx.reserve(X + Y + [9])
    assert [i for i, _ in first] == [0, 1]
    assert idx.reserve(X + Y + [9]) == []                        # the second task of a call: the blocks are saved once
    third = idx.reserve(X + Y + Z + [9])                         # chains onto the pending blocks
    assert [i for i, _ in third] == [2]
    assert idx.match(X + Y + Z + [9]) == [] and len(idx) == 0 and idx.blocks_saved == 0
    idx.abort([p for _, p in third])
    idx.commit([p for _, p in first])
    assert idx.match(X + Y + Z + [9]) == [p for _, p in first]
    assert idx.blocks_saved == 2 and len(idx) == 2
    assert [i for i, _ in idx.put(X + Y + Z + [9])] == [2]


def test_counters_and_state():
    idx = PrefixIndex(2, BS, 8)
    s0 = idx.state()
    assert idx.counters() == dict(lookups=0, hits=0, tokens_matched=0, blocks_saved=0, evictions=0)
    idx.match(X + [9])
    idx.put(X + Y + [9])
    idx.match(X + Y + [9])
    idx.match(X + [9])
    idx.match(Z + [9])
    idx.put(Z + [9])
    assert idx.counters() == dict(lookups=4, hits=2, tokens_matched=3 * BS, blocks_saved=3, evictions=1)
    assert idx.state() != s0
    s1 = idx.state()
    assert idx.state() == s1
    import numpy as np
    assert idx.match(np.array(Z + [9], dtype=np.int32)) != []    # anything with tolist() is accepted


def test_copy_launcher_argument_statuses_without_a_launch():
    """zl_kv_blocks_copy's argument checks return before any launch, so they run without a device"""
    import ctypes as C
    from zhilight_amd._lib import lib
    i64, one = C.c_int64, C.c_void_p(16)                         # a non-null, 16-byte aligned stand-in: never dereferenced

    def call(n=1, desc=one, pool=one, layers=2, b=3, block=16, hkv=2, row_bytes=256, piece=0):
        return lib().zl_kv_blocks_copy_ex(desc, i64(n), one, one, one, pool, i64(layers), i64(b), i64(block), i64(hkv), i64(row_bytes),
                                          C.c_int(1), C.c_int(1), i64(piece), None)
    assert call(n=0, desc=None, pool=None) == 0                  # n == 0: ZL_OK, nothing is read
    assert lib().zl_kv_blocks_copy(None, i64(0), None, None, None, None, i64(2), i64(3), i64(16), i64(2), i64(256), C.c_int(1), C.c_int(0), None) == 0
    assert call(n=-1) == -1 and call(desc=None) == -1 and call(pool=None) == -1 and call(layers=0) == -1 and call(row_bytes=0) == -1
    assert call(row_bytes=6) == -2 and call(piece=24) == -2      # ZL_ESHAPE
    assert call(layers=1 << 20) == -4 and call(n=1 << 31) == -4 and call(row_bytes=1 << 30) == -4      # ZL_ELIMIT
    assert call(n=1 << 20, layers=65535, block=1 << 20, hkv=1, row_bytes=1 << 20, piece=16) == -4       # beyond the grid


def test_constructor_refuses_nonsense():
    for args in ((0, 4, 2), (2, 0, 2), (2, 4, -1)):
        with pytest.raises(ValueError):
            PrefixIndex(*args)
