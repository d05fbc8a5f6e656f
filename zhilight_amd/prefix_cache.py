"""Prompt prefix cache: a pool of K/V blocks and an index from token prefixes to pool blocks (the reference's
generator::PrefixCache, src/generator/prefix_cache.hpp, as its scheduler uses it: batch_generator.cpp:626-648, 1033-1045).

PrefixIndex is the host side: pure Python, no device.  PrefixCache holds the pool tensors and moves blocks between the pool and a
context's ragged buffers with ops.kv_blocks_copy, one launch per direction and plane.  LLaMA.new_prefix_cache builds one and
LLaMA.prefill_cached uses it.

Identity.  Block i of a prompt is identified by the prompt's first (i + 1) * block_size tokens: K/V rows depend on every token
before them.  The reference keys a block by its OWN tokens and its index (to_blocks, prefix_cache.hpp:35-46), so after the prompts
[X, Y, ..] and [Z, Y, ..] its block (Y, 1) holds rows computed behind X and is handed to a prompt that starts with Z; that rule is
deliberately not reproduced here.
"""
import collections

_ROOT = 0            # the chain id in front of block 0


def _digest(prev, block_tokens):
    """chained digest of a block: of its predecessor's digest and its own tokens.  It only narrows the search: a lookup compares the
    tokens themselves and the predecessor's identity, so a collision costs a comparison, never a wrong block."""
    return hash((prev, block_tokens))


def _token_list(tokens):
    tokens = tokens.tolist() if hasattr(tokens, "tolist") else list(tokens)
    return [int(t) for t in tokens]


class _Block:
    __slots__ = ("uid", "parent", "tokens", "digest", "ready")

    def __init__(self, uid, parent, tokens, digest):
        self.uid, self.parent, self.tokens, self.digest, self.ready = uid, parent, tokens, digest, False


class PrefixIndex:
    """Token prefixes -> pool block ids, for a pool of num_blocks blocks of block_size tokens; at most max_blocks blocks of a prompt
    are looked up or stored.

    A cached block records its own tokens and the identity of the block before it (a serial number that is never reused, so a block
    whose predecessor was evicted can never be reached again and simply ages out).  A lookup walks the prompt block by block: the
    chained digest finds candidates, and a candidate is taken only if its predecessor is the block matched one step earlier and its
    tokens equal the prompt's -- by induction the whole prefix is equal.

    Recency: a hit or a put touches its chain deepest block first, so block 0 ends up the most recent, a block is never older than
    the blocks behind it, and eviction (least recent first) takes a chain's tail before its head -- the reference's put walks
    backwards for the same reason.

    reserve() hands out ids for a prompt's uncached full blocks and commit() makes them visible to match(): between the two the
    blocks are pending -- a later reserve() chains onto them and does not reserve them again, match() does not see them, and nothing
    evicts them.  put() is both steps.  abort() gives pending ids back."""

    def __init__(self, num_blocks, block_size, max_blocks):
        num_blocks, block_size, max_blocks = int(num_blocks), int(block_size), int(max_blocks)
        if num_blocks < 1 or block_size < 1 or max_blocks < 0:
            raise ValueError("PrefixIndex: num_blocks >= 1, block_size >= 1, max_blocks >= 0")
        self.num_blocks, self.block_size, self.max_blocks = num_blocks, block_size, max_blocks
        self._free = list(range(num_blocks - 1, -1, -1))        # pop() hands out 0, 1, 2, ..
        self._blocks = {}                                        # id -> _Block
        self._by_digest = {}                                     # digest -> [ids]
        self._lru = collections.OrderedDict()                    # id -> None, least recent first
        self._serial = _ROOT
        self.lookups = self.hits = self.tokens_matched = self.blocks_saved = self.evictions = 0

    def __len__(self):
        return sum(1 for b in self._blocks.values() if b.ready)

    def counters(self):
        return dict(lookups=self.lookups, hits=self.hits, tokens_matched=self.tokens_matched, blocks_saved=self.blocks_saved,
                    evictions=self.evictions)

    def state(self):
        """everything a call may change, as one comparable value (tests: "the index is unchanged")"""
        return (tuple(self._lru), tuple(sorted((i, b.uid, b.parent, b.tokens, b.ready) for i, b in self._blocks.items())),
                tuple(self._free), tuple(sorted(self.counters().items())))

    def lru_order(self):
        """cached and pending block ids, least recent first"""
        return list(self._lru)

    def _walk(self, tokens, limit, pending_too):
        """ids of the longest chain of the prompt's first `limit` blocks, and the (uid, digest) it ends on"""
        bs, ids, parent, digest = self.block_size, [], _ROOT, _ROOT
        for i in range(limit):
            blk = tuple(tokens[i * bs:(i + 1) * bs])
            d = _digest(digest, blk)
            for cand in self._by_digest.get(d, ()):
                b = self._blocks[cand]
                if b.parent == parent and b.tokens == blk and (b.ready or pending_too):
                    break
            else:
                break
            ids.append(cand)
            parent, digest = b.uid, d
        return ids, parent, digest

    def _touch(self, ids):
        for i in reversed(ids):                                  # deepest first: block 0 becomes the most recent
            self._lru[i] = None
            self._lru.move_to_end(i)

    def match(self, tokens):
        """Pool block ids of the longest cached chain among the prompt's first min((len - 1) // block_size, max_blocks) blocks.
        At least one token is always left to encode: prefill_batch needs a row to produce logits from.  (The reference looks up
        (len - 2) / block_size blocks, one token more in reserve, because its scheduler holds the prompt's last token back as the
        search token.)  A hit touches the chain and counts."""
        tokens = _token_list(tokens)
        limit = min(max(len(tokens) - 1, 0) // self.block_size, self.max_blocks)
        ids, _, _ = self._walk(tokens, limit, False)
        self._touch(ids)
        self.lookups += 1
        if ids:
            self.hits += 1
            self.tokens_matched += len(ids) * self.block_size
        return ids

    def _evict(self, protected):
        for cand in self._lru:                                   # least recent first
            if cand not in protected and self._blocks[cand].ready:
                self._drop(cand)
                self.evictions += 1
                return cand
        return None

    def _drop(self, i):
        b = self._blocks.pop(i)
        bucket = self._by_digest[b.digest]
        bucket.remove(i)
        if not bucket:
            del self._by_digest[b.digest]
        self._lru.pop(i, None)

    def reserve(self, tokens, keep=()):
        """(block index, pool block id) pairs for the prompt's full blocks, among its first min(len // block_size, max_blocks), that
        are neither cached nor pending.  Ids come from the free list first, then from evicting the least recently used block; the
        prompt's own chain, the blocks reserved by this call, every pending block and the ids in `keep` (what the caller matched or
        reserved earlier in the same step) are never evicted.  A block is reserved only behind a predecessor that is cached or
        reserved, so reserve stops at the first block it cannot place.  The whole chain is touched.  The new blocks are pending
        until commit()."""
        tokens = _token_list(tokens)
        bs = self.block_size
        full = min(len(tokens) // bs, self.max_blocks)
        chain, parent, digest = self._walk(tokens, full, True)
        protected, out = set(keep) | set(chain), []
        for i in range(len(chain), full):
            new = self._free.pop() if self._free else self._evict(protected)
            if new is None:
                break
            blk = tuple(tokens[i * bs:(i + 1) * bs])
            digest = _digest(digest, blk)
            self._serial += 1
            self._blocks[new] = _Block(self._serial, parent, blk, digest)
            self._by_digest.setdefault(digest, []).append(new)
            parent = self._serial
            protected.add(new)
            chain.append(new)
            out.append((i, new))
        self._touch(chain)
        return out

    def commit(self, ids):
        """the pending blocks `ids` hold their rows now: match() sees them from here on"""
        for i in ids:
            b = self._blocks[i]
            if not b.ready:
                b.ready = True
                self.blocks_saved += 1

    def abort(self, ids):
        """give pending blocks back (their rows were never written); blocks chained behind them become unreachable and age out"""
        for i in ids:
            b = self._blocks.get(i)
            if b is not None and not b.ready:
                self._drop(i)
                self._free.append(i)

    def put(self, tokens, keep=()):
        """reserve() and commit() in one step -> the (block index, id) pairs that were new"""
        pairs = self.reserve(tokens, keep)
        self.commit([i for _, i in pairs])
        return pairs


class PrefixCache:
    """The device side: the pool and its PrefixIndex (LLaMA.new_prefix_cache builds it from a context).

    pool: (num_blocks, layers, 2, block_size, Hkv, D) in the context's element type -- the model dtype, or the INT8 cache's u8 codes
    with a second plane pool_scales (num_blocks, layers, 2, block_size, Hkv) fp32.  Inside a block the rows keep the buffers' BSHD
    order, so a (layer, K/V) slice of a block is one contiguous run on both sides and one block's bytes are contiguous.

    A cache serves contexts of its own kind -- the same layers, KV heads, head size, element type (INT8 or not) -- on its own device,
    and on the stream that was current when it was built: its load and save launches and the prompt encode between them are ordered
    by that stream alone, no event is recorded.  fits() states the conditions; LLaMA.prefill_cached refuses anything else."""

    def __init__(self, device, layers, hkv, dim_head, dtype, quant, num_blocks, block_size=128, max_prefix=4096):
        import torch
        self.device, self.layers, self.hkv, self.dim_head, self.dtype, self.quant = device, layers, hkv, dim_head, dtype, bool(quant)
        self.num_blocks, self.block_size = int(num_blocks), int(block_size)
        self.index = PrefixIndex(num_blocks, block_size, int(max_prefix) // int(block_size))
        shape = (self.num_blocks, layers, 2, self.block_size, hkv, dim_head)
        self.pool = torch.zeros(shape, dtype=torch.uint8 if quant else dtype, device=device)
        self.pool_scales = torch.zeros(shape[:-1], dtype=torch.float32, device=device) if quant else None
        self.stream = torch.cuda.current_stream(device)
        self.load_launches = self.save_launches = 0

    def fits(self, ctx):
        """None if this cache serves ctx, else the reason it does not"""
        import torch
        if bool(ctx.kv_quant) != self.quant:
            return "the cache and the context differ in the KV element type (INT8 or not)"
        if not ctx.kv or ctx.kv[0].device != self.pool.device:
            return "the cache and the context live on different devices"
        if tuple(ctx.k_addrs.shape) != (self.layers, ctx.tokens.numel()) or any(
                t.dtype != self.pool.dtype or t.dim() != 5 or t.shape[0] != self.layers or tuple(t.shape[3:]) != (self.hkv, self.dim_head)
                for t in ctx.kv):
            return "the cache was built for another geometry (layers, KV heads, head size or element type)"
        if torch.cuda.current_stream(self.pool.device) != self.stream:
            return "the cache is used on another stream than the one it was built on"
        return None

    def _copy(self, ctx, desc, to_pool):
        from . import ops
        lens = [ctx.max_len_buf] * ctx.tokens.numel()
        ops.kv_blocks_copy(desc, ctx.k_addrs, ctx.v_addrs, ctx.buf_lens, self.pool, self.block_size, self.hkv,
                           self.dim_head * self.pool.element_size(), to_pool, buf_lens_host=lens)
        if self.quant:
            ops.kv_blocks_copy(desc, ctx.ks_addrs, ctx.vs_addrs, ctx.buf_lens, self.pool_scales, self.block_size, self.hkv, 4, to_pool,
                               buf_lens_host=lens)
        return 2 if self.quant else 1

    def load(self, ctx, desc):
        """pool -> buffers for the (task, first slot, pool block) triples of desc: ONE launch (two on an INT8 cache: codes, scales)"""
        if desc:
            self.load_launches += self._copy(ctx, desc, False)

    def save(self, ctx, desc):
        """buffers -> pool, ONE launch (two on an INT8 cache)"""
        if desc:
            self.save_launches += self._copy(ctx, desc, True)
