"""A small serving loop that keeps a decode batch full: requests wait in a queue, LLaMA.admit puts them into the slots that finished
tasks leave, and the steps between two looks at the device are the captured-or-eager steps of LLaMA.step_sample / step_lookup.

The reference's scheduler (src/generator/batch_generator.cpp: BatchGenerator::run moves tasks from its queue into max_batch_active as
slots free up, SearcherImplV1 keeps the per-task state on the host) does this per step on the host; here the per-task state lives on
the device, a request's whole life runs inside the step, and the host looks once every `poll` steps."""
import collections

import torch

from . import ops

REASONS = {1: "stop id", 2: "stop sequence", 3: "length"}
SEED_MIN, SEED_END = -(1 << 63), 1 << 64       # the seeds ops.slots_pack keeps apart: the 64 bits of the key, read signed or unsigned


# Rows of a prompt (without its re-fed last token) from which submit(n=, best_of=) shares the prompt's K/V between the samples instead
# of copying it, when a prefix buffer is free: the smallest measured P at which TWO members of 8 slots beat the copies on the same
# context (tools/bench_shared.py (b), profiles/shared_prefix.txt, DESIGN 4 "Shared prefix"; captured step_sample, Llama-3-8B geometry):
# 2.660 [2.652 .. 2.665] ms against 2.711 [2.702 .. 2.720] at 2048 rows; the intervals overlap at 512 and 1024 rows, sharing loses at
# 256 rows, and for two members it loses again at 4096 (3.372 against 3.195).  Eight members of 8 win from 1024 rows on (2.241 / 2.405).
SHARE_MIN_ROWS = 2048
# ... and the rows from which a group of TWO goes back to copying: the 4096-row line of the same table.  Larger groups have no upper
# bound (8 of 8 and 32 of 32 gain most at 4096 rows); groups of 3 .. 7 were not measured.
SHARE_PAIR_MAX_ROWS = 4096


class PrefixPool:
    """Who holds the G shared prefix buffers of a BatchServer, host only.  A buffer is free, pinned (a loaded prompt that requests name
    by handle until drop()) or a group's (the samples of one request read it).  A slot STOPS reading its buffer when it is parked or
    re-admitted, not when its request finishes: a finished slot keeps re-feeding its last token over the same keys.  A group's buffer
    is free again when its last slot has been released."""

    def __init__(self, count, rows):
        self.count, self.rows = int(count), int(rows)
        self.pinned, self.group = set(), set()
        self.lens = [0] * self.count
        self.of = {}                                     # slot -> buffer it reads

    def free(self):
        return [g for g in range(self.count) if g not in self.pinned and g not in self.group]

    def users(self, g):
        return sorted(s for s, v in self.of.items() if v == g)

    def pin(self, rows):
        """a free buffer for a loaded prompt of `rows` rows -> its handle, None when none is free"""
        free = self.free()
        if not free or not 1 <= rows <= self.rows:
            return None
        self.pinned.add(free[0])
        self.lens[free[0]] = int(rows)
        return free[0]

    def drop(self, g):
        """give a pinned buffer back; refused (False) while a slot reads it or when g is not pinned"""
        if g not in self.pinned or self.users(g):
            return False
        self.pinned.discard(g)
        self.lens[g] = 0
        return True

    def take_group(self, rows, min_rows=None, members=None):
        """a free buffer for the `members` samples of one prompt of `rows` shared rows -> its index, or None: the copying route (none
        free, the prompt shorter than SHARE_MIN_ROWS or longer than a buffer, or a pair from SHARE_PAIR_MAX_ROWS rows on); min_rows:
        the caller's threshold, which also lifts the pair's bound"""
        free = self.free()
        low = SHARE_MIN_ROWS if min_rows is None else min_rows
        if not free or not low <= rows <= self.rows or (min_rows is None and members == 2 and rows >= SHARE_PAIR_MAX_ROWS):
            return None
        self.group.add(free[0])
        self.lens[free[0]] = int(rows)
        return free[0]

    def attach(self, g, slots):
        if g not in self.pinned and g not in self.group:
            raise ops.ZLError(f"PrefixPool: buffer {g} is neither pinned nor a group's")
        for s in slots:
            self.of[int(s)] = g

    def release(self, slots):
        """the slots were parked or are being re-admitted: they read no buffer any more -> the group buffers that became free"""
        freed = []
        for s in slots:
            g = self.of.pop(int(s), None)
            if g is not None and g in self.group and not self.users(g):
                self.group.discard(g)
                self.lens[g] = 0
                freed.append(g)
        return freed


def rank_samples(samples, n):
    """The samples a request with best_of = len(samples) returns, host only: every dict gains cum_logprob = the sum of its
    logprobs; best_of > n: the n samples of largest cum_logprob, largest first, ties to the lower sample index; best_of == n: all of
    them by sample index."""
    for sm in samples:
        sm["cum_logprob"] = float(sum(sm["logprobs"]))
    if len(samples) <= n:
        return list(samples)
    order = sorted(range(len(samples)), key=lambda j: (-samples[j]["cum_logprob"], j))
    return [samples[j] for j in order[:n]]


class BatchServer:
    """BatchServer(model, batch, len_buf, ...) owns ONE context of `batch` slots with len_buf KV rows each and the full-width states:
    a sampler with the penalty bitmap (penalties=True), bias rows of bias_ld ids (0 = no logit bias) and top_logprobs alternatives, a
    stop state of the widths (16, 8, 16), and with lookup_k = K > 0 the prompt-lookup drafter (steps are step_lookup(sampler=)).
    prefix_blocks = N > 0: the server builds a prompt prefix cache of N blocks for its context (LLaMA.new_prefix_cache(ctx, N,
    prefix_block_size)) and the prompts go through it; prefix_cache: a PrefixCache made elsewhere instead -- one cache may serve several
    servers -- which must fit this server's context (PrefixCache.fits: geometry, KV element type, device, stream); build it
    with LLaMA.new_prefix_cache from any context of the same model and KV cache type.  capture=True: the steps are replays of one graph
    captured after the first eager step.  poll: steps between two read-backs.  grammar_states = S / grammar_edges = E: the sampler carries
    token-automaton tables of that capacity (LLaMA.new_sampler); load_grammar(automaton) copies a grammar.TokenAutomaton into them --
    before run() or between two runs, the captured graph stays valid -- and returns the handle that submit(..., grammar=handle) names.

    submit(prompt, **request) -> id; request = ops.SLOT_REQUEST_KEYS (temperature, top_k, top_p, seed, repetition_penalty,
    presence_penalty, penalty_tokens, logit_bias, stop_ids, stop_sequences, max_new_tokens, history, grammar).  A request is checked when
    it is submitted, against the states' widths and the buffer's length.  A request with a grammar needs a prompt of two tokens at
    least: its last token is re-fed so that the first generated token is drawn under the grammar (LLaMA.admit); its first_token is None
    and tokens holds every generated id.

    submit(prompt, n=, best_of=, sample_first=): n samples of one prompt for ONE prompt encode (LLaMA.admit_samples: the prompt without
    its last token is encoded into one slot, one launch copies its K/V rows into best_of - 1 other slots, every slot re-feeds the last
    token and draws its first token under its own sampler row).  best_of (default n) samples run, sample j with seed + j; 1 <= n <=
    best_of <= batch.  best_of > 1 or sample_first=True takes that route and needs a prompt of two tokens at least; with best_of == 1
    the result is the plain one, first_token None as for a grammar.  With best_of > 1 results[id] = dict(samples=[...], round=...): n
    dicts of the plain shape plus seed and cum_logprob (rank_samples has the order).  Admission is FIFO and all-or-nothing: the head of
    the queue waits until best_of slots are free and nothing overtakes it.

    shared_prefixes = G, shared_rows = L (no drafter): the context carries G prefix buffers of L rows (LLaMA.new_shared_prefixes) that
    slots read in place of a copy; PrefixPool keeps who holds them.  load_prefix(tokens) -> handle encodes a prompt that many requests
    share (a system prompt) into a free buffer and pins it until drop_prefix(handle), which is refused while a slot reads it;
    submit(prompt, prefix=handle) admits a request whose prompt is the part behind it (LLaMA.admit(prefixes=)).  submit(n=, best_of=)
    with best_of > 1 takes a free unpinned buffer when there is one and SHARE_MIN_ROWS <= len(prompt) - 1 <= L (share_min_rows=
    overrides the constant): the samples then share the prompt's rows and nothing is copied (LLaMA.admit_samples(share=)); otherwise
    it takes the copying route.  A group's buffer is released when its last slot is parked or re-admitted, not when it finishes: a
    finished slot keeps re-feeding its last token and still reads the prefix.  stats["shared_groups"] counts the sharing groups,
    stats["forks"] keeps its meaning (destinations copied).

    run() serves the queue until it and the batch are empty and returns {id: dict(tokens, logprobs, reason, round, first_token,
    clamped, [top_ids, top_logprobs])}: tokens = the ids emitted behind first_token (the greedy pick the prompt encode leaves
    pending, LLaMA.admit's convention), logprobs = their tempered log-probabilities, reason = 1 (stop id) / 2 (stop sequence) / 3 (length),
    round = the admission round, clamped = the length limit the slot ran under.  self.log = the admission groups (round, [(slot, id),
    ...]), the samples of one request in sample order; self.matched = {id: tokens the prefix cache supplied}; self.stats counts steps,
    slot-steps and forks (destinations copied)."""

    def __init__(self, model, batch, len_buf, penalties=True, bias_ld=0, top_logprobs=0, lookup_k=0, prefix_cache=None, capture=False,
                 poll=8, kv_history=None, prefix_blocks=0, prefix_block_size=128, grammar_states=0, grammar_edges=0, shared_prefixes=0,
                 shared_rows=0, share_min_rows=None):
        if int(poll) < 1 or int(batch) < 1:
            raise ops.ZLError("BatchServer: batch >= 1 and poll >= 1")
        if int(shared_prefixes) and (int(lookup_k) or int(shared_rows) < 1):
            raise ops.ZLError("BatchServer: shared_prefixes needs shared_rows >= 1 and no drafter (lookup_k = 0)")
        self.model, self.b, self.len_buf, self.poll, self.capture = model, int(batch), int(len_buf), int(poll), bool(capture)
        self.cache, self.kv_history = prefix_cache, kv_history
        self.ctx = ctx = model.new_context(self.b, self.len_buf, 0)
        if int(prefix_blocks):
            if prefix_cache is not None:
                raise ops.ZLError("BatchServer: prefix_blocks builds the cache, prefix_cache brings one: give one of them")
            self.cache = model.new_prefix_cache(ctx, int(prefix_blocks), int(prefix_block_size))
        self.sampler = model.new_sampler(ctx, penalties=bool(penalties), bias_ld=int(bias_ld), top_logprobs=int(top_logprobs),
                                         grammar_states=int(grammar_states), grammar_edges=int(grammar_edges))
        self.stop = model.new_stopper(ctx, widths=(ops.STOP_IDS_MAX, ops.STOP_SEQS_MAX, ops.STOP_SEQ_LEN_MAX))
        self.pool, self.share_min_rows, self.prefix_req = None, share_min_rows, {}     # prefix_req: id -> handle of submit(prefix=)
        if int(shared_prefixes):
            model.new_shared_prefixes(ctx, int(shared_prefixes), int(shared_rows))
            self.pool = PrefixPool(int(shared_prefixes), int(shared_rows))
        self.lookup = model.new_lookup(ctx, [[] for _ in range(self.b)], int(lookup_k)) if int(lookup_k) else None
        self.k = int(lookup_k)
        self.width = self.k + 1                                            # ids a step emits per slot at most
        self.stop.finished.fill_(3)                                        # nothing runs yet: every slot is a finished one
        self.stop.live.zero_()
        self.finished = [3] * self.b                                       # the host's copy of stop.finished
        self.queue = collections.deque()
        self.requests, self.results, self.log, self.matched = {}, {}, [], {}
        self.active, self.parked = {}, set()                               # slot -> id; slots parked since they finished
        self.meta, self.sample_of, self._pending = {}, {}, {}              # id -> (n, best_of, re-fed); slot -> sample index; id -> samples running
        self.round = 0
        self.graph = self._graph_out = None
        self.stats = dict(steps=0, live_slot_steps=0, finished_slot_steps=0, parked_slot_steps=0, admissions=0, parks=0, forks=0,
                          shared_groups=0)
        n, w, top = self.poll * self.b * self.width, self.width, int(top_logprobs)
        # one read-back: the rounds' token rows, their log-probabilities (as bits), finished and the first tokens, in ONE int32 buffer
        self._rb = torch.empty(2 * n + 2 * self.b + 2 * n * top, dtype=torch.int32, device=model.device)
        self._tok = self._rb[:n].view(self.poll, self.b, w)
        self._lp = self._rb[n:2 * n].view(torch.float32).view(self.poll, self.b, w)
        self._fin = self._rb[2 * n:2 * n + self.b]
        self._first = self._rb[2 * n + self.b:2 * n + 2 * self.b]
        self._first.zero_()
        self._tid = self._rb[2 * n + 2 * self.b:2 * n + 2 * self.b + n * top].view(self.poll, self.b, w, top) if top else None
        self._tlp = self._rb[2 * n + 2 * self.b + n * top:].view(torch.float32).view(self.poll, self.b, w, top) if top else None
        self.top = top

    # ---- the queue --------------------------------------------------------------------------------------------------------------
    def load_grammar(self, automaton):
        """-> the handle of submit's grammar= (LLaMA.load_grammar on the server's sampler)"""
        return self.model.load_grammar(self.sampler, automaton)

    def load_prefix(self, tokens):
        """encode `tokens` into a free prefix buffer and pin it -> the handle that submit(..., prefix=handle) names, until drop_prefix"""
        if self.pool is None:
            raise ops.ZLError("load_prefix: the server has no shared prefixes (shared_prefixes=, shared_rows=)")
        tokens = torch.as_tensor(tokens).reshape(-1).to(torch.int32).cpu()
        g = self.pool.pin(int(tokens.numel()))
        if g is None:
            raise ops.ZLError(f"load_prefix: no free prefix buffer, or not 1 .. {self.pool.rows} tokens")
        try:
            self.model.load_prefix(self.ctx, g, tokens)
        except Exception:
            self.pool.drop(g)
            raise
        return g

    def drop_prefix(self, handle):
        """unpin a loaded prefix; refused while a slot reads it or a queued request names it"""
        if self.pool is None or handle in [self.prefix_req.get(r) for r in self.queue] or not self.pool.drop(handle):
            raise ops.ZLError("drop_prefix: not a loaded prefix, or still in use")

    def _prompt_len(self, prompt, request, refed=False):
        """the tokens the prompt encode sees: all of them, or all but the re-fed last one of a request with a grammar or of one that
        goes through admit_samples"""
        return int(prompt.numel()) - (1 if refed or request.get("grammar") is not None else 0)

    def submit(self, prompt, n=1, best_of=None, sample_first=False, prefix=None, **request):
        prompt = torch.as_tensor(prompt).reshape(-1).to(torch.int32).cpu()
        base = 0                                                             # rows of a loaded prefix in front of the prompt
        if prefix is not None:
            if self.pool is None or prefix not in self.pool.pinned or isinstance(prefix, bool):
                raise ops.ZLError("submit: prefix is a handle of this server's load_prefix")
            if best_of not in (None, 1) or n != 1 or sample_first:
                raise ops.ZLError("submit: prefix= takes one sample per request")
            base = self.pool.lens[prefix]
        ints = lambda v: isinstance(v, int) and not isinstance(v, bool)                                      # noqa: E731
        best_of = n if best_of is None else best_of
        if not (ints(n) and ints(best_of) and 1 <= n <= best_of <= self.b):
            raise ops.ZLError(f"submit: 1 <= n <= best_of <= batch ({self.b}), integers")
        samples, refed = (n, best_of), best_of > 1 or bool(sample_first)
        if best_of > 1:
            seed = request.get("seed", 0)
            if not (isinstance(seed, int) and SEED_MIN <= seed and seed + best_of - 1 < SEED_END):
                raise ops.ZLError(f"submit: seeds seed .. seed + {best_of - 1} of the samples within [-2^63, 2^64)")
        n = self._prompt_len(prompt, request, refed) + base
        if n - base < 1 or n + 1 > self.len_buf:
            raise ops.ZLError(f"submit: a prompt of {int(prompt.numel())} tokens does not fit the KV buffer of {self.len_buf}"
                              if n - base >= 1 else "submit: a prompt of one token at least, two with a grammar, n > 1 or sample_first")
        if request.get("grammar") is not None and not (self.sampler.fsm is not None and isinstance(request["grammar"], int)
                                                      and 0 <= request["grammar"] < self.sampler.fsm_used[0]):
            raise ops.ZLError("submit: grammar is a handle of this server's load_grammar")
        probe = dict(request)
        if self.lookup is not None and probe.get("history") is None:
            probe["history"] = prompt
        ops.slots_pack([(0, probe)], self.model.cfg.vocab_size, self.model.slot_widths(self.sampler, self.stop, self.lookup))
        if ops.slot_max_new(n, request.get("max_new_tokens", 0), self.len_buf, self.k) < 1:
            raise ops.ZLError(f"submit: a prompt of {n} tokens leaves no room for one generated token")
        rid = len(self.requests)
        self.requests[rid] = (prompt, dict(request))
        self.meta[rid] = samples + (refed,)
        if prefix is not None:
            self.prefix_req[rid] = prefix
        self.queue.append(rid)
        return rid

    # ---- one step ---------------------------------------------------------------------------------------------------------------
    def _step(self):
        if self.lookup is not None:
            res = self.model.step_lookup(self.ctx, self.lookup, sampler=self.sampler, stop=self.stop)
            out = [res.tokens, self.sampler.row_logprobs]
            return out + ([self.sampler.row_top_ids, self.sampler.row_top_logprobs] if self.top else [])
        _, nxt = self.model.step_sample(self.ctx, self.sampler, stop=self.stop)
        out = [nxt, self.sampler.logprobs]
        return out + ([self.sampler.top_ids, self.sampler.top_logprobs] if self.top else [])

    def _run_step(self, i):
        if self.graph is not None:
            self.graph.replay()
            out = self._graph_out
        else:
            out = self._step()
            if self.capture:                                                # the first eager step has allocated what a step allocates
                torch.cuda.synchronize()
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self._graph_out = self._step()
                # the capture enqueued nothing: `out` is still the eager step's, in the buffers the replays will write
        self._tok[i].copy_(out[0].view(self.b, self.width))
        self._lp[i].copy_(out[1].view(self.b, self.width))
        if self.top:
            self._tid[i].copy_(out[2].view(self.b, self.width, self.top))
            self._tlp[i].copy_(out[3].view(self.b, self.width, self.top))

    # ---- the loop ---------------------------------------------------------------------------------------------------------------
    def _admit(self):
        free = [s for s in range(self.b) if s not in self.active]
        group = []
        while self.queue and len(free) >= self.meta[self.queue[0]][1]:      # FIFO, all-or-nothing: the head waits, nothing overtakes it
            rid = self.queue.popleft()
            group += [(free.pop(0), rid) for _ in range(self.meta[rid][1])]
        if not group:
            return
        self.round += 1
        if self.pool is not None:                                           # re-admission: the slots let go of the buffers they read
            self.pool.release([s for s, _ in group])
            self.model.release_prefix(self.ctx, [s for s, _ in group])
        behind = [(s, r) for s, r in group if r in self.prefix_req]
        if behind:
            self.model.admit(self.ctx, [s for s, _ in behind], [self.requests[r][0] for _, r in behind],
                             [self.requests[r][1] for _, r in behind], self.sampler, self.stop, self.lookup,
                             prefixes=[self.prefix_req[r] for _, r in behind])
            for s, r in behind:
                self.pool.attach(self.prefix_req[r], [s])
        plain = [(s, r) for s, r in group if not self.meta[r][2] and r not in self.prefix_req]
        forked = {}
        for s, r in group:
            if self.meta[r][2]:
                forked.setdefault(r, []).append(s)
        if plain:
            out = self.model.admit(self.ctx, [s for s, _ in plain], [self.requests[r][0] for _, r in plain],
                                   [self.requests[r][1] for _, r in plain], self.sampler, self.stop, self.lookup, cache=self.cache,
                                   kv_history=self.kv_history)
            if self.cache is not None:
                for (_, r), m in zip(plain, out[1]):
                    self.matched[r] = int(m)
        shared = {}                                                         # id -> prefix buffer: the samples that share their prompt
        for r, slots in forked.items():
            g = self.pool.take_group(int(self.requests[r][0].numel()) - 1, self.share_min_rows, len(slots)) if self.pool is not None and len(slots) > 1 else None
            if g is not None:
                shared[r] = g
        if shared:
            self.model.admit_samples(self.ctx, [(forked[r], self.requests[r][0], [dict(self.requests[r][1], seed=self.requests[r][1].get("seed", 0) + j)
                                                                                for j in range(len(forked[r]))]) for r in shared],
                                     self.sampler, self.stop, self.lookup, share=[shared[r] for r in shared])
            for r, g in shared.items():
                self.pool.attach(g, forked[r])
            self.stats["shared_groups"] += len(shared)
            forked = {r: slots for r, slots in forked.items() if r not in shared}
        if forked:
            groups = [(slots, self.requests[r][0], [dict(self.requests[r][1], seed=self.requests[r][1].get("seed", 0) + j)
                                                    if len(slots) > 1 else self.requests[r][1] for j in range(len(slots))])
                      for r, slots in forked.items()]
            out = self.model.admit_samples(self.ctx, groups, self.sampler, self.stop, self.lookup, cache=self.cache,
                                           kv_history=self.kv_history)
            if self.cache is not None:
                for r, m in zip(forked, out[1]):
                    self.matched[r] = int(m)
            self.stats["forks"] += sum(len(slots) - 1 for slots in forked.values())
        self._first.copy_(self.ctx.tokens)
        self.log.append((self.round, list(group)))
        self.stats["admissions"] += 1
        seen = {}
        for s, r in group:
            self.active[s] = r
            self.parked.discard(s)
            self.finished[s] = 0
            prompt, request = self.requests[r]
            res = dict(tokens=[], logprobs=[], reason=0, round=self.round, first_token=None,
                       clamped=ops.slot_max_new(self._prompt_len(prompt, request, self.meta[r][2]) + (self.pool.lens[self.prefix_req[r]] if r in self.prefix_req else 0),
                                                request.get("max_new_tokens", 0) or 0,
                                                self.len_buf, self.k))
            if self.top:
                res.update(top_ids=[], top_logprobs=[])
            if self.meta[r][1] > 1:                                         # a sample: its dict lives in the request's list until all are done
                j = seen[r] = seen.get(r, -1) + 1
                self.sample_of[s] = j
                res["seed"] = request.get("seed", 0) + j
                if j == 0:
                    self.results[r] = dict(samples=[], round=self.round)
                    self._pending[r] = self.meta[r][1]
                self.results[r]["samples"].append(res)
            else:
                self.results[r] = res

    def _res(self, s):
        """the result dict that slot s fills"""
        res = self.results[self.active[s]]
        return res["samples"][self.sample_of[s]] if s in self.sample_of else res

    def _park(self, last=False):
        idle = [s for s in range(self.b) if s not in self.active and s not in self.parked]
        # nothing active: the loop is about to end, and only a server with prefix buffers parks then (last) -- its finished slots
        # would otherwise stay readers of their buffers until some later request happened to reuse them
        if idle and (self.active or (last and self.pool is not None and any(s in self.pool.of for s in idle))):
            self.model.park(self.ctx, idle, self.sampler, self.stop, self.lookup, finished=self.finished)
            self.parked.update(idle)
            self.stats["parks"] += 1
            if self.pool is not None:
                self.pool.release(idle)

    def run(self):
        while self.queue or self.active:
            self._admit()
            self._park()
            for i in range(self.poll):
                self._run_step(i)
            self._fin.copy_(self.stop.finished)
            rb = self._rb.cpu()                                             # the one read-back of the round
            n, bw = self.poll * self.b * self.width, self.b
            tok = rb[:n].view(self.poll, self.b, self.width).tolist()
            lp = rb[n:2 * n].view(torch.float32).view(self.poll, self.b, self.width).tolist()
            fin = rb[2 * n:2 * n + bw].tolist()
            first = rb[2 * n + bw:2 * n + 2 * bw].tolist()
            if self.top:
                t0 = 2 * n + 2 * bw
                tid = rb[t0:t0 + n * self.top].view(self.poll, self.b, self.width, self.top).tolist()
                tlp = rb[t0 + n * self.top:].view(torch.float32).view(self.poll, self.b, self.width, self.top).tolist()
            self.stats["steps"] += self.poll
            for i in range(self.poll):
                for s in range(self.b):
                    row = tok[i][s]
                    m = next((j for j, v in enumerate(row) if v < 0), len(row))
                    if s in self.parked:
                        self.stats["parked_slot_steps"] += 1
                    elif m == 0:
                        self.stats["finished_slot_steps"] += 1
                    else:
                        self.stats["live_slot_steps"] += 1
                    if m == 0:
                        continue
                    if s not in self.active:
                        raise ops.ZLError(f"BatchServer: slot {s} emitted ids without a request")
                    res = self._res(s)
                    res["tokens"] += row[:m]
                    res["logprobs"] += lp[i][s][:m]
                    if self.top:
                        res["top_ids"] += tid[i][s][:m]
                        res["top_logprobs"] += tlp[i][s][:m]
            for s in list(self.active):
                rid = self.active[s]
                res = self._res(s)
                if res["first_token"] is None and self.requests[rid][1].get("grammar") is None and not self.meta[rid][2]:
                    res["first_token"] = first[s]
                self.finished[s] = fin[s]
                if fin[s]:
                    res["reason"] = fin[s]
                    del self.active[s]
                    if self.sample_of.pop(s, None) is not None:
                        self._pending[rid] -= 1
                        if self._pending[rid] == 0:                       # the request's last sample: rank them
                            del self._pending[rid]
                            self.results[rid]["samples"] = rank_samples(self.results[rid]["samples"], self.meta[rid][0])
        self._park(last=True)
        return self.results
