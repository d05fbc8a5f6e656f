"""Pure-Python / numpy statement of zl_slots_admit (slot admission: one call re-initialises the rows of a set of slots in the sampler's,
the stop state's and the lookup drafter's tensors for new requests, or parks a slot), written from the rule of include/zhilight_amd.h
and shared by test_slot_host.py and the GPU tests.  It reads the packed blob itself, word by word, and builds every row from the ids in
it -- not through ops.logit_bias_rows / ops.stop_rows, which the tests hold it against."""
import numpy as np

HDR, REC, TAIL = 16, 16, 15
MAGIC = 0x534C4F54
NAN_BITS = 0x7FC00000
CTX = ("tokens", "positions", "placement", "valid_lens")
SAMPLER = ("temperature", "top_k", "top_p", "seeds", "draws", "logprobs", "u")
PENALTY = ("repetition_penalty", "presence_penalty", "seen")
BIAS = ("bias_ids", "bias_vals", "bias_cnt", "bias_bits")
TOP = ("top_ids", "top_logprobs")
STOP = ("stop_ids", "stop_seqs", "seq_lens", "max_new", "gen_lens", "tail", "last_token", "finished", "emit_lens", "live")
LOOKUP = ("history", "hist_lens")


def header(blob):
    names = ("magic", "n", "vocab", "flags", "bias_ld", "n_ids", "n_seqs", "seq_ld", "rec", "var", "total", "hist_cap")
    h = dict(zip(names, (int(v) for v in blob[:12])))
    assert h["magic"] == MAGIC and h["total"] == blob.size and h["var"] == HDR + h["n"] * h["rec"]
    assert h["rec"] == REC + h["n_ids"] + h["n_seqs"] + h["n_seqs"] * h["seq_ld"]
    return h


def _f32(word):
    return np.array([word], np.int32).view(np.float32)[0]


def _bits(row, ids, vocab):
    """row (ld) uint32 <- exactly the bits of the ids in [0, vocab)"""
    row[:] = 0
    for i in ids:
        if 0 <= i < vocab:
            row[i >> 5] |= np.uint32(1 << (i & 31))


def admit(blob, ctx, sampler=None, stop=None, lookup=None, draft_new=None):
    """One call, in place on dicts of numpy arrays named as LLaMA's DynBatchContext / SamplerState / StopState / LookupState fields
    (seen and the bias bitmap as uint32 or int32 words).  ctx is required (tokens holds the pending tokens; a park writes all four);
    sampler / stop / lookup = None skips the group, and inside the sampler the penalty, bias and top-N tensors may be absent.
    draft_new (B) int32: the drafter's new-token column.  A record whose slot is outside [0, B) is dropped."""
    h = header(blob)
    b, vocab = ctx["tokens"].size, h["vocab"]
    recs = blob[HDR:h["var"]].reshape(h["n"], h["rec"])
    admitted = set()
    for r in recs:
        s = int(r[0])
        if not 0 <= s < b:
            continue
        if r[1] == 0:                                                       # park
            ctx["tokens"][s] = ctx["positions"][s] = ctx["placement"][s] = 0
            ctx["valid_lens"][s] = 1
            if stop is not None:
                stop["last_token"][s] = 0
                stop["tail"][s] = -1
                stop["emit_lens"][s] = 0
            continue
        admitted.add(s)
        pending = int(ctx["tokens"][s])
        if sampler is not None:
            sampler["temperature"][s], sampler["top_k"][s], sampler["top_p"][s] = _f32(r[2]), r[3], _f32(r[4])
            sampler["seeds"][s] = np.array([r[5], r[6]], np.int32).view(np.int64)[0]
            sampler["draws"][s] = 0
            sampler["logprobs"][s] = sampler["u"][s] = 0.0
            if sampler.get("seen") is not None:
                sampler["repetition_penalty"][s], sampler["presence_penalty"][s] = _f32(r[7]), _f32(r[8])
                _bits(sampler["seen"][s].view(np.uint32), [pending] + blob[r[10]:r[10] + r[11]].tolist(), vocab)
            if sampler.get("bias_ids") is not None:
                cnt = int(r[13])
                ids = blob[r[12]:r[12] + cnt]
                sampler["bias_ids"][s] = -1
                sampler["bias_ids"][s, :cnt] = ids
                sampler["bias_vals"][s] = 0.0
                sampler["bias_vals"][s, :cnt] = blob[r[12] + cnt:r[12] + 2 * cnt].view(np.float32)
                sampler["bias_cnt"][s] = cnt
                _bits(sampler["bias_bits"][s].view(np.uint32), ids.tolist(), vocab)
            if sampler.get("top_ids") is not None:
                sampler["top_ids"][s] = -1
                sampler["top_logprobs"][s].view(np.uint32)[:] = NAN_BITS
        if stop is not None:
            q = REC
            stop["stop_ids"][s] = r[q:q + h["n_ids"]]
            q += h["n_ids"]
            stop["seq_lens"][s] = r[q:q + h["n_seqs"]]
            q += h["n_seqs"]
            stop["stop_seqs"][s] = r[q:].reshape(h["n_seqs"], h["seq_ld"])
            stop["max_new"][s] = r[9]
            stop["gen_lens"][s] = stop["finished"][s] = stop["emit_lens"][s] = 0
            stop["tail"][s] = -1
            stop["tail"][s, TAIL - 1] = stop["last_token"][s] = pending
        if lookup is not None:
            n = int(r[15])
            lookup["history"][s, :n] = blob[r[14]:r[14] + n]
            lookup["hist_lens"][s] = n
    if stop is not None:
        stop["live"][0] = int((stop["finished"] == 0).sum())
    if draft_new is not None:
        draft_new[:] = -1
        for s in admitted:
            draft_new[s] = ctx["tokens"][s]


def clamp_max_new(prompt_len, max_new, len_buf, k=0):
    """LLaMA.admit's length limit of a slot: the request's (0 = none) cut so that prompt_len + max_new + k + 1 <= len_buf, k = the
    drafter's K or 0 -- the device-side length stop then keeps the task inside its buffer.  < 1: the prompt leaves no room."""
    room = len_buf - prompt_len - k - 1
    return room if max_new <= 0 else min(max_new, room)
