"""Score-profile builders for the attention tests (plain numpy, no GPU, no oracle).

Every other attention test draws q, K and V as i.i.d. normals: the scores are N(0, ~1), the softmax is flat and the running maximum
of an online-softmax kernel settles in its first chunk.  The builders here make q and K so that the REALISED fp64 scores
scale * q . K_j -- computed from the rounded fp16 / bf16 (or dequantised INT8) values, exactly what a kernel sees -- follow a designed
profile a_j over the visible keys:

    q_head = g_head * C * w + 0.05 * noise        K_j = a_j / (scale * C) * w + 0.3 * noise        (w: a unit direction per kv head)

The query rows that share a kv head get different gains g (1, -1, 0, 0.5, ...): a rise is a fall for the row with g = -1 and nothing
for the row with g = 0, so one 16-row matrix-core tile holds rows whose maxima move in different chunks.  (sparse_spikes adds a
second direction u, orthogonal to w, that every q carries WITHOUT a gain: q += C * u, K_j += b_j / (scale * C) * u, so that its
non-spike keys score -110 for every row.)  Each builder asserts the
profile's defining property (span, margin, offset) and the fp64 softmax mass it claims on the rows with g = 1, and carries the plain
numpy fp64 attention of its data as `ref`.

Also here: a float32 restatement of the attention (`attend(..., dt=np.float32)`, the noise floor of any fp32 kernel) and a small
float32 online-softmax restatement with one switch per kernel defect (`online_softmax`, tests/test_attn_profiles_host.py).
"""
import numpy as np

PROFILES = ("rise", "fall", "late_spike", "early_spike", "stairs", "offset_pos", "offset_neg", "equal", "hidden_spike", "sparse_spikes")
GAINS = (1.0, -1.0, 0.0, 0.5, 1.0, -0.5)        # gain of query row r of a kv head: GAINS[r % 6]
C = 8.0                                         # |q| along w
BLOCK = 64                                      # keys per `stairs` level: the smallest MLA split / key tile, divides the 128-key decode split
# neighbouring block levels alternate in sign and differ by 30 .. 110 (the wrap-around included)
STAIR_LEVELS = (-55.0, 55.0, -15.0, 40.0, -55.0, 25.0, -5.0, 55.0)
HIDDEN_LIFT = 125.0                             # designed score of an invisible key above the visible maximum (asserted: >= 100 realised)
HIDDEN_V = 1e4
# MLA only: the ramps run from -110 to 0 instead of -55 to +55 (a gain-free shift along u, as sparse_spikes').  At +-55 the float32
# restatement's noise on the keys that carry the mass reached 0.25 .. 0.27 of the MLA bar's absolute term (2e-5 of max|E|; fp16, 16
# and 128 heads): the span and the shape stay, the scores that matter move towards 0, where fp32 resolves them better.
MLA_SHIFT, MLA_SHIFTED = -55.0, ("rise", "fall", "hidden_spike")
SPIKE_STEP = 37                                 # sparse_spikes: coprime to every chunk / tile / split length


def to_bits(x, dtype):
    """float array -> uint16 raw bits of fp16 (dtype 0) or bf16 (1), round to nearest even"""
    if dtype == 0:
        return np.ascontiguousarray(x, dtype=np.float64).astype(np.float16).view(np.uint16)
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bits(u, dtype):
    u = np.ascontiguousarray(u, dtype=np.uint16)
    if dtype == 0:
        return u.view(np.float16).astype(np.float64)
    return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def designed(name, n, rng, ladder=1):
    """the designed scores a_j of the n visible keys (ladder > 1, causal form: the last `ladder` keys are spikes 12 apart, so that
    every row of the staircase ends on a dominant key)"""
    noise = rng.standard_normal(n)
    if n == 0:
        return np.zeros(0)
    if name in ("rise", "hidden_spike"):
        return np.linspace(-55.0, 55.0, n) if n > 1 else np.array([55.0])
    if name == "fall":
        return np.linspace(55.0, -55.0, n) if n > 1 else np.array([55.0])
    if name == "late_spike":
        a = noise
        for i in range(min(ladder, n)):
            a[n - 1 - i] = 40.0 + 12.0 * (min(ladder, n) - 1 - i)
        return a
    if name == "early_spike":
        noise[0] = 40.0
        return noise
    if name == "stairs":
        return np.array([STAIR_LEVELS[(j // BLOCK) % len(STAIR_LEVELS)] for j in range(n)])
    if name == "offset_pos":
        return noise + 60.0
    if name == "offset_neg":
        return noise - 60.0
    if name == "equal":
        return np.zeros(n)
    if name == "sparse_spikes":
        # every 37th key is a spike, 2 at key 0 rising to 12 at the end (times the row's gain); every other key scores -110 for EVERY
        # row (`fixed_part`: a second direction u, orthogonal to w, that q carries with no gain): the maximum moves at (almost) every
        # spike while every lane that has not met a spike yet holds a partial sum of exactly 0 -- the one state in which "rescale
        # only if alpha != 1 and the lane's own sum is > 0" is wrong without the wave ballot.  No row sees a large positive score,
        # so the fp32 noise floor stays far below the MLA bar's absolute term.
        a = np.zeros(n)
        idx = np.arange(0, n, SPIKE_STEP)
        a[idx] = 2.0 + 10.0 * idx / max(n - 1, 1)
        return a
    raise ValueError(name)


def fixed_part(name, a):
    """the part of the designed score that does not scale with the row's gain (sparse_spikes: -110 off the spikes)"""
    return np.where(a > 0.0, 0.0, -110.0) if name == "sparse_spikes" else np.zeros(len(a))


def attend(q, k, v, vis, scale, dt=np.float64):
    """plain softmax attention of one unit: q (R, d), k (L, d), v (L, dv), vis (R, L) bool -> (out (R, dv), scores (R, L)) in dt;
    a row without a visible key gives zeros (Z = 1e-20)"""
    q, k, v = (np.asarray(x, dtype=dt) for x in (q, k, v))
    s = (q @ k.T) * dt(scale)
    sm = np.where(vis, s, -np.inf)
    m = np.where(vis.any(1), sm.max(1, initial=-np.inf), 0.0).astype(dt)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(vis, np.exp(sm - m[:, None]), 0).astype(dt)
    # (invisible V may be huge: 0 * 1e4 is fine, NaN never appears here)
    out = (p @ np.where(vis.any(0)[:, None], v, 0).astype(dt)) / (p.sum(1, dtype=dt)[:, None] + dt(1e-20))
    return out.astype(dt), s


MUTANTS = ("drop_last", "no_rescale", "lane_skip", "hidden_in_max", "no_max", "merge_no_max", "drop_first_split")


def online_softmax(q, k, v, vis, scale, mutant=None, chunk=32, split=128, lanes=8):
    """float32 restatement of the split-KV online-softmax kernels: chunks of `chunk` keys, splits of `split`, a record (max, sum, O)
    per split, then the merge.  A "lane" owns 4 consecutive keys of every chunk (its own partial sum) and 1 / lanes of the output
    columns of the shared accumulator, as in the matrix-core kernels; exp flushes denormals as the device's does.  mutant:
      drop_last         the last visible key of every row is skipped
      no_rescale        the accumulator is not rescaled when the maximum moves
      lane_skip         a lane rescales its accumulator columns only if ITS OWN partial sum is > 0 (the shortcut without the ballot)
      hidden_in_max     invisible keys enter the running maximum (their probability is zeroed)
      no_max            no maximum subtraction
      merge_no_max      the split merge ignores the split maxima
      drop_first_split  the first split's record is dropped
    """
    f = np.float32
    q, k, v = (np.asarray(x, dtype=f) for x in (q, k, v))
    vis = np.array(vis, dtype=bool)
    R, L, dv = q.shape[0], k.shape[0], v.shape[1]
    if mutant == "drop_last":
        for r in range(R):
            idx = np.nonzero(vis[r])[0]
            if len(idx):
                vis[r, idx[-1]] = False
    colgrp = (np.arange(dv) * lanes) // dv
    tiny = np.finfo(f).tiny
    recs = []
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        s_all = (q @ k.T) * f(scale)
        for t0 in range(0, L, split):
            m = np.full(R, -1e20, f)
            lsum = np.zeros((R, lanes), f)
            acc = np.zeros((R, dv), f)
            for c0 in range(t0, min(L, t0 + split), chunk):
                c1 = min(L, c0 + chunk)
                s, vz = s_all[:, c0:c1], vis[:, c0:c1]
                sm = np.where(vz, s, f(-np.inf))
                mloc = (s if mutant == "hidden_in_max" else sm).max(1)
                m_new = np.maximum(m, mloc)
                if mutant == "no_max":
                    m_new = np.zeros(R, f)
                    alpha = np.ones(R, f)
                else:
                    alpha = np.exp(m - m_new)
                p = np.where(vz, np.exp(sm - m_new[:, None]), f(0)).astype(f)
                p[np.abs(p) < tiny] = 0
                lane = (np.arange(c1 - c0) // 4) % lanes
                pl = np.stack([p[:, lane == g].sum(1, dtype=f) for g in range(lanes)], axis=1)
                if mutant == "no_rescale":
                    a_cols = np.ones((R, dv), f)
                elif mutant == "lane_skip":
                    a_cols = np.where((lsum > 0)[:, colgrp], alpha[:, None], f(1))
                else:
                    a_cols = np.broadcast_to(alpha[:, None], (R, dv))
                acc = (acc * a_cols + p @ np.where(vz.any(0)[:, None], v[c0:c1], f(0))).astype(f)
                lsum = (lsum * alpha[:, None] + pl).astype(f)
                m = m_new
            recs.append((m, lsum.sum(1, dtype=f), acc))
        if mutant == "drop_first_split" and len(recs) > 1:
            recs = recs[1:]
        M = np.max([r[0] for r in recs], axis=0)
        o, z = np.zeros((R, dv), f), np.zeros(R, f)
        for m_s, l_s, a_s in recs:
            w = np.ones(R, f) if mutant == "merge_no_max" else np.exp(m_s - M).astype(f)
            o = (o + a_s * w[:, None]).astype(f)
            z = (z + l_s * w).astype(f)
        return o / (z[:, None] + f(1e-20))


class Case:
    """One built workload.  units: list of dicts (q, k, v, vis, gains, where) with the float64 VALUES of the bits, one per
    (task, kv head) -- what `attend` / `online_softmax` take; ref: the fp64 attention in the op's output shape."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def restate(self, fn):
        """apply fn(q, k, v, vis) -> (R, dv) to every unit and scatter the rows into an array of ref's shape"""
        out = np.zeros(self.ref.shape, np.float64)
        for u in self.units:
            out[u["where"]] = np.asarray(fn(u["q"], u["k"], u["v"], u["vis"]), dtype=np.float64).reshape(out[u["where"]].shape)
        return out


def _check_profile(name, s, vis, hidden, gains, a_vis_idx, a):
    """s (R, L) realised scores, vis (R, L); rows with gain 1 carry the profile.  a_vis_idx: buffer index of every designed key, a:
    its designed score.  Returns nothing; raises AssertionError when the data does not have the property its name promises."""
    rows = [r for r in range(s.shape[0]) if gains[r] == 1.0]
    assert rows, "no query row with gain 1"
    n = len(a_vis_idx)
    if name == "equal":
        assert not s[:, a_vis_idx].any()
        return
    for r in rows:
        idx = np.nonzero(vis[r])[0]
        if len(idx) == 0:
            continue
        sv = s[r, idx]
        p = np.exp(sv - sv.max())
        p /= p.sum()
        full = len(idx) == n                                   # this row sees every designed key (the last row of a staircase)
        if name in ("rise", "fall", "hidden_spike") and full and n >= 2:
            assert sv.max() - sv.min() >= 104.0, (name, sv.max() - sv.min())
            m = -(-n // 16)
            assert (p[-m:] if name != "fall" else p[:m]).sum() > 0.99
        if name == "stairs" and full and n > BLOCK:
            assert sv.max() - sv.min() >= 104.0, (name, sv.max() - sv.min())
            top = a[np.searchsorted(a_vis_idx, idx)] == a.max()
            assert p[top].sum() > 0.999
            assert np.float32(np.exp(sv.min() - sv.max())) == 0.0      # (some block's merge weight is exactly 0 in fp32)
        if name == "late_spike" and len(idx) >= 2:
            designed_here = a[np.searchsorted(a_vis_idx, idx)]
            plain = designed_here < 20.0
            if plain[-1]:
                continue                                       # (a prefill row before the last: the spike is not among its keys)
            if plain.any():
                assert sv[-1] - sv[plain].max() >= 30.0, (name, sv[-1] - sv[plain].max())
            assert p[-1] > 0.999, (name, p[-1])
        if name == "early_spike" and len(idx) >= 2:
            assert sv[0] - sv[1:].max() >= 30.0
            assert p[0] > 0.999
        if name in ("offset_pos", "offset_neg"):
            assert (np.abs(sv).min() >= 50.0) and (np.sign(sv) == (1 if name == "offset_pos" else -1)).all()
        if name == "sparse_spikes":
            spk = a[np.searchsorted(a_vis_idx, idx)] > 0.0
            if (~spk).any():
                assert sv[spk].min() - sv[~spk].max() >= 104.0, (name, sv[spk].min() - sv[~spk].max())
                assert np.float32(np.exp(sv[~spk].max() - sv[spk].min())) == 0.0      # (exactly 0 in fp32, denormals or not)
            if spk.sum() >= 2:                                     # the running maximum keeps moving
                moves = (sv[spk][1:] > np.maximum.accumulate(sv[spk])[:-1]).sum()
                assert moves >= max(1, (spk.sum() - 1) // 4), (name, moves)
        if name == "hidden_spike" and hidden.any():
            assert s[r, hidden].min() - sv.max() >= 100.0, (name, s[r, hidden].min() - sv.max())


def _unit_dir(rng, d):
    """(w, u): two orthonormal directions"""
    w, u = rng.standard_normal(d), rng.standard_normal(d)
    w /= np.linalg.norm(w)
    u -= (u @ w) * w
    return np.stack([w, u / np.linalg.norm(u)])


def build_decode(name, rng, buf_lens, valid, h, hkv, d, len_q, dtype, scale, bshd=True, causal=False, holes=False, quant=None):
    """The rag-buffer decode ops.  Task t has a buffer of buf_lens[t] slots; row qi sees the keys j < valid[t] (+ qi when causal),
    minus the holes of a mask form (holes=True: about one key in eight of the visible range, never the first or the last).  The
    profile lies over the visible keys in order.  quant: a function (rows (M, d) bits) -> (codes u8 (M, d), scales f32 (M,)), the
    project's INT8 row quantiser; K and V are then codes + scales and every score is evaluated on the dequantised values.
    Returns a Case: q (b, len_q, h, d) bits, k / v lists of per-task bit (or code) arrays in the bshd / bhsd layout, ks / vs scale
    lists (quant), mask (the concatenated int8 mask), ref (b, len_q, h, d) fp64."""
    rep, b = h // hkv, len(buf_lens)
    q_bits = np.zeros((b, len_q, h, d), np.uint16)
    ks, vs, kscales, vscales, masks, units = [], [], [], [], [], []
    ref = np.zeros((b, len_q, h, d), np.float64)
    for t, (L, n0) in enumerate(zip(buf_lens, valid)):
        vis = np.zeros((len_q, L), bool)
        for qi in range(len_q):
            vis[qi, :min(L, n0 + (qi if causal else 0))] = True
        if holes and n0 > 2:
            hole = np.zeros(L, bool)
            hole[1:n0 - 1] = rng.random(n0 - 2) < 0.125
            vis[:, hole] = False
        seen = vis.any(0)
        idx = np.nonzero(seen)[0]
        a = designed(name, len(idx), rng, ladder=len_q if causal else 1)
        A = np.zeros(L)
        A[idx] = a
        hidden = ~seen
        if name == "hidden_spike":
            A[hidden] = (a.max() if len(a) else 0.0) + HIDDEN_LIFT
        Bf = np.zeros(L)
        Bf[idx] = fixed_part(name, a)
        wu = np.stack([_unit_dir(rng, d) for _ in range(hkv)])                    # (hkv, 2, d)
        w, u = wu[:, 0], wu[:, 1] * (name == "sparse_spikes")
        K = (A[:, None, None] * w[None] + Bf[:, None, None] * u[None]) / (scale * C) + 0.3 * rng.standard_normal((L, hkv, d))
        V = rng.standard_normal((L, hkv, d))
        if name == "hidden_spike":
            V[hidden] = HIDDEN_V
        gains = np.array([[GAINS[(r + qi) % len(GAINS)] for r in range(rep)] for qi in range(len_q)])     # (len_q, rep)
        Q = np.zeros((len_q, h, d))
        for hk in range(hkv):
            Q[:, hk * rep:(hk + 1) * rep] = gains[:, :, None] * C * w[hk] + C * u[hk] + 0.05 * rng.standard_normal((len_q, rep, d))
        if name == "equal":
            Q[:] = 0.0
        qb = to_bits(Q, dtype)
        q_bits[t] = qb
        Qv = from_bits(qb, dtype)
        if quant is None:
            kb, vb = to_bits(K, dtype), to_bits(V, dtype)
            Kv, Vv = from_bits(kb, dtype), from_bits(vb, dtype)
            ksc = vsc = None
        else:
            kb, ksc = quant(to_bits(K, dtype).reshape(L * hkv, d))
            vb, vsc = quant(to_bits(V, dtype).reshape(L * hkv, d))
            kb, vb, ksc, vsc = kb.reshape(L, hkv, d), vb.reshape(L, hkv, d), ksc.reshape(L, hkv), vsc.reshape(L, hkv)
            Kv = (kb.astype(np.float64) - 128.0) * ksc.astype(np.float64)[:, :, None]
            Vv = (vb.astype(np.float64) - 128.0) * vsc.astype(np.float64)[:, :, None]
        for hk in range(hkv):
            uq = Qv[:, hk * rep:(hk + 1) * rep].reshape(len_q * rep, d)
            uvis = np.repeat(vis, rep, axis=0)
            out, s = attend(uq, Kv[:, hk], Vv[:, hk], uvis, scale)
            _check_profile(name, s, uvis, hidden, gains.reshape(-1), idx, a)
            ref[t][:, hk * rep:(hk + 1) * rep] = out.reshape(len_q, rep, d)
            units.append(dict(q=uq, k=Kv[:, hk], v=Vv[:, hk], vis=uvis, gains=gains.reshape(-1), scores=s,
                              where=(t, slice(None), slice(hk * rep, (hk + 1) * rep))))
        lay = (lambda x: np.ascontiguousarray(x)) if bshd else (lambda x: np.ascontiguousarray(np.moveaxis(x, 1, 0)))
        ks.append(lay(kb))
        vs.append(lay(vb))
        if quant is not None:
            kscales.append(lay(ksc))
            vscales.append(lay(vsc))
        masks.append(vis.astype(np.int8).reshape(-1))
    return Case(name=name, q=q_bits, k=ks, v=vs, ks=kscales, vs=vscales, mask=np.concatenate(masks), ref=ref, units=units,
                buf_lens=list(buf_lens), valid=list(valid), scale=scale, dtype=dtype)


def build_prefill(name, rng, s_q, pos0, h, hkv, d, dtype, scale):
    """prefill_attention: one task, q (s_q, h, d), buffers (len_buf, hkv, d) holding the chunk at pos0 .. pos0 + s_q - 1; row i sees
    the keys 0 .. pos0 + i.  The profile lies over the keys 0 .. pos0 + s_q - 1 (every row sees a prefix of it, so under `rise` each
    row's maximum is its own last key); the slots behind the chunk are invisible to every row and lie in the last query tile's
    diagonal key tile -- under hidden_spike they are finite, 125 above the visible maximum and carry V = 1e4.  Row i of head r of a
    kv head has gain GAINS[(r + i) % 6]."""
    rep = h // hkv
    n = pos0 + s_q
    L = (n + 63) // 64 * 64 + 64
    vis = np.arange(L)[None, :] <= (pos0 + np.arange(s_q))[:, None]
    a = designed(name, n, rng)
    A = np.zeros(L)
    A[:n] = a
    hidden = np.arange(L) >= n
    if name == "hidden_spike":
        A[hidden] = a.max() + HIDDEN_LIFT
    Bf = np.zeros(L)
    Bf[:n] = fixed_part(name, a)
    wu = np.stack([_unit_dir(rng, d) for _ in range(hkv)])
    w, u = wu[:, 0], wu[:, 1] * (name == "sparse_spikes")
    K = (A[:, None, None] * w[None] + Bf[:, None, None] * u[None]) / (scale * C) + 0.3 * rng.standard_normal((L, hkv, d))
    V = rng.standard_normal((L, hkv, d))
    if name == "hidden_spike":
        V[hidden] = HIDDEN_V
    gains = np.array([[GAINS[(r + i) % len(GAINS)] for r in range(rep)] for i in range(s_q)])             # (s_q, rep)
    Q = np.zeros((s_q, h, d))
    for hk in range(hkv):
        Q[:, hk * rep:(hk + 1) * rep] = gains[:, :, None] * C * w[hk] + C * u[hk] + 0.05 * rng.standard_normal((s_q, rep, d))
    if name == "equal":
        Q[:] = 0.0
    qb, kb, vb = to_bits(Q, dtype), to_bits(K, dtype), to_bits(V, dtype)
    Qv, Kv, Vv = from_bits(qb, dtype), from_bits(kb, dtype), from_bits(vb, dtype)
    ref = np.zeros((s_q, h, d))
    units = []
    idx = np.arange(n)
    for hk in range(hkv):
        uq = Qv[:, hk * rep:(hk + 1) * rep].reshape(s_q * rep, d)
        uvis = np.repeat(vis, rep, axis=0)
        out, s = attend(uq, Kv[:, hk], Vv[:, hk], uvis, scale)
        _check_profile(name, s, uvis, hidden, gains.reshape(-1), idx, a)
        ref[:, hk * rep:(hk + 1) * rep] = out.reshape(s_q, rep, d)
        units.append(dict(q=uq, k=Kv[:, hk], v=Vv[:, hk], vis=uvis, gains=gains.reshape(-1), scores=s,
                          where=(slice(None), slice(hk * rep, (hk + 1) * rep))))
    return Case(name=name, q=qb, k=kb, v=vb, mask=vis.astype(np.int8), ref=ref, units=units, len_buf=L, scale=scale, dtype=dtype)


def build_mla(name, rng, buf_len, vis_lens, h, dtype, scale, rank=512, rope=64):
    """MLA decode over the latent cache: task t has a (buf_len, 576) buffer of latent rows (key = the whole row, value = its first
    512 entries) and sees the keys j < vis_lens[t].  The profile's direction w lives in the 64 rope entries, so the value part stays
    i.i.d. (0.6 sigma, as the other MLA tests); head r has gain GAINS[r % 6].  Under hidden_spike the invisible rows are finite,
    score 125 above the visible maximum and have a value part of 1e4 (q's value part is zero there, so that this does not swamp the
    designed score).  Returns a Case: q (b, h, 576) bits, kv (list of (buf_len, 576) bit arrays), ref (b, h, 512) fp64."""
    b, cd = len(vis_lens), rank + rope
    q_bits = np.zeros((b, h, cd), np.uint16)
    kv, units = [], []
    ref = np.zeros((b, h, rank))
    gains = np.array([GAINS[r % len(GAINS)] for r in range(h)])
    for t, n in enumerate(vis_lens):
        a = designed(name, n, rng)
        A = np.zeros(buf_len)
        A[:n] = a
        hidden = np.arange(buf_len) >= n
        if name == "hidden_spike":
            A[hidden] = (a.max() if n else 0.0) + HIDDEN_LIFT
        Bf = np.zeros(buf_len)
        Bf[:n] = fixed_part(name, a)
        w, u = _unit_dir(rng, rope)
        if name in MLA_SHIFTED:
            Bf[:n] += MLA_SHIFT
        elif name != "sparse_spikes":
            u = 0.0 * u
        row = np.concatenate([0.6 * rng.standard_normal((buf_len, rank)),
                              (A[:, None] * w[None] + Bf[:, None] * u[None]) / (scale * C) + 0.3 * rng.standard_normal((buf_len, rope))], axis=1)
        Q = np.concatenate([0.4 * rng.standard_normal((h, rank)),
                            gains[:, None] * C * w[None] + C * u[None] + 0.05 * rng.standard_normal((h, rope))], axis=1)
        if name == "hidden_spike":
            row[hidden, :rank] = HIDDEN_V
            Q[:, :rank] = 0.0
        if name == "equal":
            Q[:] = 0.0
        qb, rb = to_bits(Q, dtype), to_bits(row, dtype)
        q_bits[t] = qb
        kv.append(rb)
        Qv, Rv = from_bits(qb, dtype), from_bits(rb, dtype)
        vis = np.broadcast_to(~hidden, (h, buf_len))
        out, s = attend(Qv, Rv, Rv[:, :rank], vis, scale)
        if n:
            _check_profile(name, s, vis, hidden, gains, np.arange(n), a)
        ref[t] = out
        units.append(dict(q=Qv, k=Rv, v=Rv[:, :rank], vis=vis, gains=gains, scores=s, where=(t,)))
    return Case(name=name, q=q_bits, kv=kv, ref=ref, units=units, vis_lens=list(vis_lens), buf_len=buf_len, scale=scale, dtype=dtype)


# ---- the bars of the existing tests, by kernel --------------------------------------------------------------------------------------
def decode_bar(exact, dtype):
    """tests/test_gpu_ops.py test_decode_attention_matrix_core_path (and the causal, last-arriver, mask-form and INT8 tests):
    1e-3 (fp16) / 5e-3 (bf16: output rounding is 2^-9 relative) of max(1, max|exact|)"""
    return (5e-3 if dtype else 1e-3) * max(1.0, np.abs(exact).max())


def half_record_bar(exact):
    """tests/test_gpu_w4.py test_attention_mask_form_split_records_merge: the records pass through fp16 once"""
    return (1e-3 + 2.0 ** -10) * max(1.0, np.abs(exact).max())


def prefill_bar(ref, dtype):
    """tests/test_gpu_ops.py test_prefill_attention: 2e-3 (fp16) / 1.5e-2 (bf16) of max|ref|"""
    return (1.5e-2 if dtype else 2e-3) * np.abs(ref).max()


def mla_bar(E, dtype):
    """tests/test_gpu_f4.py test_mla_decode_attention_over_the_latent_cache: ulp * |E| + 2e-5 * max|E|, elementwise"""
    return 2.0 ** (-7 if dtype else -10) * np.abs(E) + 2e-5 * np.abs(E).max()


# ---- the workloads of tests/test_gpu_attn_profiles.py (tests/test_attn_profiles_host.py checks the fp32 noise floor on each) --------
VALID = [1, 31, 33, 129, 517, 640]              # visible lengths of the six decode tasks: a ragged chunk, a split boundary, the buffer end
BUF = 640
# (d, h, hkv, len_q, visibility): every decode geometry a route below uses; "holes": a mask with holes, "causal": the staircase
DECODE_GEOMS = {
    "d64": (64, 8, 2, 1, "prefix"),
    "h8": (128, 8, 2, 1, "prefix"),
    "h8_holes": (128, 8, 2, 1, "holes"),
    "h8_q2": (128, 8, 2, 2, "prefix"),
    "h8_q2_holes": (128, 8, 2, 2, "holes"),
    "d64_holes": (64, 8, 2, 1, "holes"),
    "h16_q4": (128, 16, 4, 4, "prefix"),
    "h28": (128, 28, 4, 1, "prefix"),
    "causal_h8_q4": (128, 8, 2, 4, "causal"),
    "causal_h32_q3": (128, 32, 4, 3, "causal"),
}
LONG_BUF, LONG_VALID = 4224, 4161                # route 8: 33 splits of 128 keys
PREFILL_GEOMS = {"s200_p440": (200, 440, 8, 2), "s65_p0": (65, 0, 4, 1)}
MLA_SCALE = 0.1147
MLA_GEOMS = {                                    # (h, buffer, visible lengths)
    "h16": (16, 768, [1, 65, 700, 767]),
    "h20": (20, 768, [1, 65, 700, 767]),
    "h128_b3": (128, 768, [1, 700, 767]),
    # 32 tasks x 8 head groups: one split, every wave walks up to 17 pieces.  One key (three waves without any), none, the whole buffer,
    # and long ragged lengths; lengths of 16 .. 130 keys are left to h16 / h20: over 128 heads x 32 tasks the fp32 noise of a flat
    # softmax over that few keys at scores of +-60 reaches 0.3 .. 0.4 of the MLA bar's absolute term (test_attn_profiles_host.py)
    "h128_b32": (128, 1088, [1, 0, 1088, 1087, 1086, 1025, 545, 513] + [400 + 27 * i for i in range(24)]),
}


def seed_of(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


def decode_case(geom, name, dtype, quant=None, long=False):
    d, h, hkv, len_q, visib = DECODE_GEOMS[geom]
    rng = np.random.default_rng(seed_of("decode", geom, name, dtype, bool(quant), long))
    lens, valid = ([LONG_BUF], [LONG_VALID]) if long else ([BUF] * len(VALID), VALID)
    if visib == "causal":
        valid = [min(v, L - len_q + 1) for v, L in zip(valid, lens)]
    return build_decode(name, rng, lens, valid, h, hkv, d, len_q, dtype, 1.0 / np.sqrt(d), causal=visib == "causal",
                        holes=visib == "holes", quant=quant)


def prefill_case(geom, name, dtype):
    s_q, pos0, h, hkv = PREFILL_GEOMS[geom]
    return build_prefill(name, np.random.default_rng(seed_of("prefill", geom, name, dtype)), s_q, pos0, h, hkv, 128, dtype, 1.0 / np.sqrt(128))


def mla_case(geom, name, dtype):
    h, buf, vis = MLA_GEOMS[geom]
    return build_mla(name, np.random.default_rng(seed_of("mla", geom, name, dtype)), buf, vis, h, dtype, MLA_SCALE)
