"""A numpy (fp64) statement of the two-segment decode attention (zl_decode_attn_shared, include/zhilight_amd.h), on top of
attn_profiles.attend.

A call carries G prefix buffers of prefix_caps[g] rows, prefix_lens[g] of them valid.  Task b names g = prefix_of[b] (outside [0, G):
none).  With P = min(prefix_lens[g], prefix_caps[g], valid_lens[b], buf_lens[b]) (0 for "none", never below 0) the task's key j is row j
of prefix buffer g for j < P and row j of its own buffer for P <= j < min(valid_lens[b], buf_lens[b]).  Only those rows are touched
here: whatever else the buffers hold (NaN in the tests) cannot reach the result.  A task without a visible key gets a zero row."""
import numpy as np

from attn_profiles import attend


def prefix_rows(prefix_of, prefix_lens, prefix_caps, valid_lens, buf_lens):
    """P of every task"""
    g_n = len(prefix_lens)
    out = []
    for b, g in enumerate(prefix_of):
        g = int(g)
        if not 0 <= g < g_n:
            out.append(0)
            continue
        out.append(max(0, min(int(prefix_lens[g]), int(prefix_caps[g]), int(valid_lens[b]), int(buf_lens[b]))))
    return out


def _rows(buf, hk, lo, hi, bshd):
    """rows [lo, hi) of kv head hk of a (L, Hkv, D) / (Hkv, L, D) buffer"""
    return buf[lo:hi, hk] if bshd else buf[hk, lo:hi]


def task_keys(b, hk, own_k, own_v, valid_lens, buf_lens, prefix_of, prefix_lens, prefix_caps, prefix_k, prefix_v, bshd=True):
    """(K, V) of task b and kv head hk under the rule: the prefix rows, then the own rows from P on"""
    p = prefix_rows(prefix_of, prefix_lens, prefix_caps, valid_lens, buf_lens)[b]
    end = max(p, min(int(valid_lens[b]), int(buf_lens[b])))
    ks, vs = [_rows(own_k[b], hk, p, end, bshd)], [_rows(own_v[b], hk, p, end, bshd)]
    if p:
        g = int(prefix_of[b])
        ks.insert(0, _rows(prefix_k[g], hk, 0, p, bshd))
        vs.insert(0, _rows(prefix_v[g], hk, 0, p, bshd))
    return np.concatenate(ks, axis=0), np.concatenate(vs, axis=0)


def shared_attention(q, own_k, own_v, valid_lens, buf_lens, prefix_of, prefix_lens, prefix_caps, prefix_k, prefix_v, hkv, scale,
                     bshd=True, dt=np.float64):
    """q (B, H, D) values; own_k / own_v: B arrays, prefix_k / prefix_v: G arrays, all in the layout `bshd` names -> out (B, H, D)"""
    q = np.asarray(q, dtype=np.float64)
    b_n, h, d = q.shape
    n_rep = h // hkv
    out = np.zeros((b_n, h, d), dtype=dt)
    for b in range(b_n):
        for hk in range(hkv):
            k, v = task_keys(b, hk, own_k, own_v, valid_lens, buf_lens, prefix_of, prefix_lens, prefix_caps, prefix_k, prefix_v, bshd)
            rows = q[b, hk * n_rep:(hk + 1) * n_rep]
            out[b, hk * n_rep:(hk + 1) * n_rep] = attend(rows, k, v, np.ones((n_rep, len(k)), dtype=bool), scale, dt=dt)[0]
    return out


def restate_f32(q, k_pre, v_pre, k_own, v_own, scale, shared_split=128, own_split=128, chunk=32):
    """float32 restatement of the kernel's arithmetic for the rows q (R, d) of one (task, kv head): an online softmax over chunks of
    32 keys, one (max, sum, acc) record per split of the prefix segment and per split of the own segment, then ONE merge over all
    records (max init -1e20, Z init 1e-20) -> (R, dv) float32.  The noise floor of any fp32 kernel of this structure."""
    f = np.float32
    q = np.asarray(q, dtype=f)
    recs = []
    with np.errstate(over="ignore", under="ignore"):
        for k, v, split in ((k_pre, v_pre, shared_split), (k_own, v_own, own_split)):
            k, v = np.asarray(k, dtype=f), np.asarray(v, dtype=f)
            for t0 in range(0, len(k), split):
                m, l, acc = np.full(len(q), -1e20, f), np.zeros(len(q), f), np.zeros((len(q), v.shape[1]), f)
                for c0 in range(t0, min(len(k), t0 + split), chunk):
                    s = ((q @ k[c0:c0 + chunk].T) * f(scale)).astype(f)[:, :min(len(k), t0 + split) - c0]
                    m_new = np.maximum(m, s.max(1))
                    alpha, p = np.exp(m - m_new).astype(f), np.exp(s - m_new[:, None]).astype(f)
                    acc = (acc * alpha[:, None] + p @ v[c0:c0 + s.shape[1]]).astype(f)
                    l, m = (l * alpha + p.sum(1, dtype=f)).astype(f), m_new
                recs.append((m, l, acc))
        big = np.max([r[0] for r in recs], axis=0) if recs else np.full(len(q), -1e20, f)
        o, z = np.zeros((len(q), np.asarray(v_own).shape[1]), f), np.zeros(len(q), f)
        for m, l, acc in recs:
            w = np.exp(m - big).astype(f)
            o, z = (o + acc * w[:, None]).astype(f), (z + l * w).astype(f)
        return o / (z[:, None] + f(1e-20))


def materialise(own, valid_lens, buf_lens, prefix_of, prefix_lens, prefix_caps, prefix, bshd=True, fill=0.0):
    """the buffers a task would hold WITHOUT sharing: its prefix rows copied in front of its own rows from P on, `fill` elsewhere"""
    ps = prefix_rows(prefix_of, prefix_lens, prefix_caps, valid_lens, buf_lens)
    out = []
    for b, buf in enumerate(own):
        m = np.full(buf.shape, fill, dtype=buf.dtype)
        end = max(ps[b], min(int(valid_lens[b]), int(buf_lens[b])))
        if bshd:
            m[ps[b]:end] = buf[ps[b]:end]
            if ps[b]:
                m[:ps[b]] = prefix[int(prefix_of[b])][:ps[b]]
        else:
            m[:, ps[b]:end] = buf[:, ps[b]:end]
            if ps[b]:
                m[:, :ps[b]] = prefix[int(prefix_of[b])][:, :ps[b]]
        out.append(m)
    return out
