"""The load-time glue kernels (csrc/tensor_ops.hip; zl_rope_rotate / zl_mask_valid_lens of misc_ops.hip) against the plain float64 /
numpy references of tests/glue_ref.py, through the C ABI as ops.py calls it: raw device pointers, the current stream, the status
checked.  Bit-exact means equal bit patterns (a NaN has to be a NaN on both sides, its payload is not compared); every random input is
seeded; assertion messages name the worst element.  Lines starting "glue_ops_errors:" (pytest -s) are the figures kept in
profiles/glue_ops_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import glue_ref as G

pytestmark = pytest.mark.gpu

# zl_elem_t codes and the numpy carrier of the raw elements
CODE = {"f64": 0, "f32": 1, "f16": 2, "i8": 3, "i16": 4, "i32": 5, "bf16": 6}
RAW = {"f64": np.float64, "f32": np.float32, "f16": np.uint16, "bf16": np.uint16, "i8": np.int8, "i16": np.int16, "i32": np.int32}
FLOATS, INTS = ("f64", "f32", "f16", "bf16"), ("i8", "i16", "i32")
_SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
CANARY = 0x5A


def _call(name, *args):
    from zhilight_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args), name)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, byte_offset=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + byte_offset)


def _i(v):
    return C.c_int64(int(v))


def _up(a, dev):
    """numpy array -> device tensor of the same bytes (signed integer view: torch has no uint16 / uint32 arithmetic, none is needed)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED[a.dtype.itemsize])).to(dev)


def _down(t, dtype):
    return t.cpu().numpy().view(dtype)


def _canary(nbytes, dev):
    return torch.full((int(nbytes),), CANARY, dtype=torch.uint8, device=dev)


def _decode(raw, t):
    """raw elements of type t -> exact float64 values"""
    if t in ("f16", "bf16"):
        with np.errstate(invalid="ignore"):
            return G.bits_to_f64(raw, t)
    return np.asarray(raw).astype(np.float64)


def _encode(x64, t):
    """float64 -> raw elements of the float type t (one rounding)"""
    if t == "f64":
        return np.ascontiguousarray(x64, dtype=np.float64)
    bits = G.round_to(x64, t)
    return bits.view(np.float32) if t == "f32" else bits


def _bits(raw):
    raw = np.ascontiguousarray(raw)
    return raw.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[raw.dtype.itemsize])


def _isnan(raw, t):
    if t in ("f16", "bf16"):
        return G.is_nan_bits(raw, t)
    return np.isnan(raw) if t in ("f64", "f32") else np.zeros(np.shape(raw), bool)


def _assert_bits(got, want, t, what, src=None):
    """equal bit patterns; where the reference is a NaN any NaN will do"""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nw, ng = _isnan(want, t), _isnan(got, t)
    bad = np.nonzero(np.where(nw, ~ng, _bits(got) != _bits(want)))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ; first at {i}: got {_bits(got)[i]:#x} want {_bits(want)[i]:#x}"
                             + (f" input {(src[i] if src.ndim == 2 else src.reshape(-1)[i])!r}" if src is not None else ""))


def _all16():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def _normals(rng, n, scales=(1e-7, 1e-3, 1.0, 300.0, 6e4)):
    return rng.standard_normal(n) * rng.choice(np.array(scales), n)


# ======================================================================================================================== zl_cast
# the reference's typecast.cu pairs, the int8 <-> half pair that carries bytes across RCCL, every same-type pair, and the
# int <-> float pairs the ABI accepts besides
CAST_PAIRS = ([(a, b) for a in FLOATS for b in FLOATS if a != b] + [(a, b) for a in INTS for b in INTS if a != b]
              + [("i8", "f16"), ("f16", "i8")] + [(t, t) for t in FLOATS + INTS]
              + [("i32", "f32"), ("i32", "f64"), ("i32", "bf16"), ("i32", "f16"), ("i16", "f32"), ("i16", "bf16"), ("f32", "i32"),
                 ("f64", "i32"), ("f64", "i16"), ("bf16", "i32"), ("f32", "i8")])
INT_RANGE = {"i8": (-128, 127), "i16": (-32768, 32767), "i32": (-2 ** 31, 2 ** 31 - 1)}
FLOAT_MAX = {"f16": 65504.0, "bf16": (2 - 2.0 ** -7) * 2.0 ** 127, "f32": (2 - 2.0 ** -23) * 2.0 ** 127, "f64": np.inf}


def _cast_pool(src, dst, rng):
    """raw source elements: the union the pair has to survive (see the module's issue list: random normals over several scales, all
    16-bit patterns, the target's ties and their neighbours in the source format, double-rounding vectors, the target's edges)"""
    if src in INTS:
        lo, hi = INT_RANGE[src]
        if dst in INTS or dst == "f64" or (dst == "f32" and src != "i32"):
            edge = [0, 1, -1, 44, 127, 128, -128, -129, 255, 256, 300, -300, 32767, 32768, -32768, -32769, 65535, 65536, 16777216,
                    16777217, -16777217, 2 ** 31 - 1, -2 ** 31, 2 ** 24 + 2 ** 16 + 1]
            vals = np.concatenate([np.array([e for e in edge if lo <= e <= hi], np.int64), rng.integers(lo, hi + 1, 70000)])
        else:
            # int -> float, tested IN RANGE of the target only (beyond its largest finite value nothing is asked): exact where
            # representable, else one round-to-nearest-even -- so ties of the target and their neighbours, e.g. 2^30 + 2^22 (+1)
            top = int(min(hi, FLOAT_MAX[dst]))
            ties = []
            if src == "i32" and dst in ("bf16", "f32"):
                p = 8 if dst == "bf16" else 24
                for e in range(p, 31):
                    base, ulp = 1 << e, 1 << (e - p + 1)
                    for k in (0, 1, 2, 3, (1 << (p - 1)) - 1):
                        tie = base + k * ulp + ulp // 2
                        ties += [tie - 1, tie, tie + 1, -tie, -tie - 1, -tie + 1] if ulp >= 2 else [tie]
            vals = np.concatenate([np.array([t for t in ties if -top <= t <= top] + [0, 1, -1, top, -top], np.int64),
                                   rng.integers(max(lo, -top), top + 1, 70000),
                                   rng.integers(-2048, 2049, 5000)])
        return vals.astype(RAW[src])
    if dst in INTS:
        # float -> int truncates towards zero; only values whose truncation lies in the target's range are tested (outside it the
        # conversion is undefined in C as well)
        lo, hi = INT_RANGE[dst]
        top = min(float(hi), FLOAT_MAX[src])
        x = np.concatenate([rng.uniform(-min(top, 300.0), min(top, 300.0), 50000), rng.uniform(max(lo, -top), top, 50000),
                            [0.0, -0.0, 0.5, -0.5, 0.999, -0.999, 1.5, -1.5, 2.5, -2.5, 126.99, -127.99, float(lo), 1e-30, -1e-30]])
        raw = _encode(x, src)
        keep = np.trunc(_decode(raw, src))
        return raw[(keep >= lo) & (keep <= hi)]
    parts = []
    if src in ("f16", "bf16"):
        parts.append(_all16())                                    # every pattern: subnormals, zeros, infinities, NaNs
    else:
        parts.append(_encode(np.concatenate([_normals(rng, 60000), _normals(rng, 20000, (1e-42, 1e-30, 1e30, 3e38))]), src))
    if dst != src and dst != "f64":
        parts.append(_encode(G.special_values(dst), src))
        for v in (1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -11, 1 + 2.0 ** -8, 1 + 2.0 ** -24 + 2.0 ** -50):
            parts.append(_encode(np.array([v, -v]), src))
        if src in ("f64", "f32") and G.FORMATS[dst][1] < (52 if src == "f64" else 23):
            mid = _encode(G.halfway_cases(dst, rng), src)         # the target's exact ties, then the source's neighbours of each
            parts += [mid, np.nextafter(mid, RAW[src](np.inf)), np.nextafter(mid, RAW[src](-np.inf))]
    else:
        parts.append(_encode(np.concatenate([G.special_values("f16"), G.special_values("bf16"), G.special_values("f32")]), src))
    return np.concatenate(parts)


def _cast_want(raw, src, dst):
    if src == dst:
        return raw
    if src in INTS and dst in INTS:
        return raw.astype(RAW[dst])                               # numpy's integer narrowing is C's modular one
    if dst in INTS:
        return np.trunc(_decode(raw, src)).astype(RAW[dst])
    return _encode(_decode(raw, src), dst)


def _run_cast(raw, src, dst, dev, what):
    n = raw.size
    x = _up(raw, dev)
    item = np.dtype(RAW[dst]).itemsize
    out = _canary((n + 64) * item, dev)
    _call("zl_cast", _p(x), C.c_int(CODE[src]), _p(out), C.c_int(CODE[dst]), _i(n), _s())
    got = _down(out, RAW[dst])
    assert (_down(out, np.uint8)[n * item:] == CANARY).all(), (what, "wrote past n")
    _assert_bits(got[:n], _cast_want(raw, src, dst), dst, what, raw)


@pytest.mark.parametrize("src,dst", CAST_PAIRS, ids=[f"{a}-{b}" for a, b in CAST_PAIRS])
def test_cast(dev, src, dst):
    """out[i] = OutT(in[i]) converted directly: int -> int as C (narrowing modular), to a wider float exact, to a narrower float ONE
    round-to-nearest-even of the source value (f64 -> half / bf16 not through a rounded fp32), same type a bit copy"""
    rng = np.random.default_rng([CODE[src], CODE[dst], 77])
    pool = _cast_pool(src, dst, rng)
    _run_cast(pool, src, dst, dev, f"cast {src}->{dst} pool")
    for n in (1, 255, 256, 257, 1_000_003):
        start = int(rng.integers(0, pool.size))
        raw = np.resize(np.roll(pool, -start), n)
        if n > pool.size:
            raw = raw.copy()
            rng.shuffle(raw[pool.size:])
        _run_cast(raw, src, dst, dev, f"cast {src}->{dst} n={n}")


def test_cast_hand_vectors(dev):
    """the cases a conversion through fp32 gets wrong, written out"""
    def one(vals, src, dst):
        raw = np.array(vals, RAW[src])
        x = _up(raw, dev)
        out = _canary(raw.size * np.dtype(RAW[dst]).itemsize, dev)
        _call("zl_cast", _p(x), C.c_int(CODE[src]), _p(out), C.c_int(CODE[dst]), _i(raw.size), _s())
        return _down(out, RAW[dst]).tolist()
    assert one([300, -129, 16777217, -16777217, 2 ** 31 - 1], "i32", "i8") == [44, 127, 1, -1, -1]
    assert one([16777217, 65536 + 5, -32769, 2 ** 31 - 1], "i32", "i16") == [1, 5, 32767, -1]
    assert one([300, -129, 32767], "i16", "i8") == [44, 127, -1]
    assert one([16777217, -(2 ** 31), 2 ** 31 - 1, 33554433], "i32", "i32") == [16777217, -(2 ** 31), 2 ** 31 - 1, 33554433]
    assert one([16777217, 2 ** 31 - 1, -(2 ** 31 - 1)], "i32", "f64") == [16777217.0, 2.0 ** 31 - 1, -(2.0 ** 31 - 1)]
    assert one([16777217.0, 2.0 ** 31 - 1, -2.0 ** 31, 0.99], "f64", "i32") == [16777217, 2 ** 31 - 1, -(2 ** 31), 0]
    d = [1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -30, 0.1]
    assert one(d, "f64", "f64") == d
    assert [hex(v) for v in one(d[:2], "f64", "f16")] == ["0x3c01", "0x3c04"]
    assert [hex(v) for v in one(d[:2], "f64", "bf16")] == ["0x3f80", "0x3f81"]
    assert [hex(v) for v in one([2 ** 30 + 2 ** 22 + 1, 2 ** 30 + 2 ** 22], "i32", "bf16")] == ["0x4e81", "0x4e80"]


def test_cast_past_the_grid_cap(dev):
    """65535 * 8 * 256 + 12345 elements, half -> bf16: more than the capped grid covers in one trip, so the grid-stride step runs
    (about 540 MB of device memory in plus out)"""
    n = 65535 * 8 * 256 + 12345
    rng = np.random.default_rng(4)
    raw = rng.integers(0, 65536, n, dtype=np.uint16)
    raw[:65536] = _all16()
    raw[-65536:] = _all16()[::-1]
    table = _cast_want(_all16(), "f16", "bf16")
    nan_table = G.is_nan_bits(table, "bf16")
    x = _up(raw, dev)
    out = torch.full((n + 64,), 0x5A5A, dtype=torch.int16, device=dev)
    _call("zl_cast", _p(x), C.c_int(CODE["f16"]), _p(out), C.c_int(CODE["bf16"]), _i(n), _s())
    got = _down(out, np.uint16)
    del x, out
    assert (got[n:] == 0x5A5A).all()
    got = got[:n]
    ok = got == table[raw]
    ok |= nan_table[raw] & G.is_nan_bits(got, "bf16")
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (bad.size, int(bad[0]), hex(raw[bad[0]]), hex(got[bad[0]]), hex(table[raw[bad[0]]]))


# ======================================================================================================================== zl_copy_2d
# (source offset, destination offset, source pitch, destination pitch, width): all multiples of 16; a multiple of 4 but not of 16 in
# each of the five in turn; an odd width; a pointer at +1; src_pitch == width < dst_pitch and the other way round, in every lane width
COPY_CASES = [(0, 0, 64, 80, 48), (16, 32, 48, 48, 48),
              (4, 0, 64, 80, 48), (0, 4, 64, 80, 48), (0, 0, 68, 80, 48), (0, 0, 64, 84, 48), (0, 0, 64, 80, 44),
              (0, 0, 64, 80, 45), (1, 0, 64, 80, 48), (0, 1, 64, 80, 48), (0, 0, 63, 80, 48), (3, 5, 7, 9, 7),
              (0, 0, 48, 64, 48), (0, 0, 64, 48, 48), (0, 0, 44, 52, 44), (0, 0, 52, 44, 44), (0, 0, 45, 51, 45), (0, 0, 51, 45, 45),
              (0, 0, 16, 16, 16), (0, 0, 4, 4, 4), (0, 0, 1, 1, 1), (0, 0, 4096, 6144, 2048)]


@pytest.mark.parametrize("rows", [1, 7, 4099])
def test_copy_2d(dev, rows):
    """bytes against numpy slicing; the destination's pitch gaps, the bytes in front of it and everything past the last row keep the
    canary"""
    rng = np.random.default_rng(rows)
    for so, do, sp, dp, w in COPY_CASES:
        src = rng.integers(0, 256, so + rows * sp + 64, dtype=np.uint8)
        src[src == CANARY] = 0                                    # so that a copied byte is never mistaken for an untouched one
        dsz = do + rows * dp + 64
        want = np.full(dsz, CANARY, np.uint8)
        r, c = np.arange(rows)[:, None], np.arange(w)[None, :]
        want[do + r * dp + c] = src[so + r * sp + c]
        s_t, d_t = _up(src, dev), _canary(dsz, dev)
        assert s_t.data_ptr() % 16 == 0 and d_t.data_ptr() % 16 == 0
        _call("zl_copy_2d", _p(s_t, so), _i(sp), _p(d_t, do), _i(dp), _i(w), _i(rows), _s())
        got = _down(d_t, np.uint8)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, ((so, do, sp, dp, w, rows), bad.size, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


# ======================================================================================================================== zl_index_select
@pytest.mark.parametrize("outer", [1, 3])
def test_index_select(dev, outer):
    """out[o, j, :] = in[o, index[j], :] against np.take; an index of -1 or dim_in gives a zero run (the kernel's documented guard)"""
    rng = np.random.default_rng(outer)
    dim_in = 7
    index = np.array([3, 3, 0, 6, -1, 2, 6, dim_in, 5, 1, 1, 4, 0, 6, 2, 2, 3, 5, 0], np.int32)      # 19 > dim_in, repeats, two outside
    ok = (index >= 0) & (index < dim_in)
    # (inner bytes, byte offset of in, byte offset of out): 16-, 4-, 2- and 1-byte kernels; a base pointer at +2 forces the 2-byte one
    for inner, off_in, off_out in [(32, 0, 0), (16, 0, 0), (4096, 0, 0), (20, 0, 0), (4, 0, 0), (16, 4, 0), (6, 0, 0), (2, 0, 0), (16, 2, 0),
                                   (16, 0, 2), (32, 2, 2), (5, 0, 0), (1, 0, 0), (16, 1, 0), (33, 0, 3)]:
        src = rng.integers(1, 256, (outer, dim_in, inner), dtype=np.uint8)
        want = np.take(src, np.where(ok, index, 0), axis=1)
        want[:, ~ok, :] = 0
        s_t = _up(np.concatenate([np.zeros(off_in, np.uint8), src.reshape(-1)]), dev)
        o_t, i_t = _canary(off_out + want.size + 64, dev), _up(index, dev)
        _call("zl_index_select", _p(s_t, off_in), _p(o_t, off_out), _p(i_t), _i(outer), _i(dim_in), _i(index.size), _i(inner), _s())
        got = _down(o_t, np.uint8)
        assert (got[:off_out] == CANARY).all() and (got[off_out + want.size:] == CANARY).all(), (inner, off_in, off_out, "canary")
        bad = np.nonzero(got[off_out:off_out + want.size] != want.reshape(-1))[0]
        assert bad.size == 0, ((inner, off_in, off_out), bad.size, int(bad[0]), int(got[off_out + bad[0]]), int(want.reshape(-1)[bad[0]]))


# ======================================================================================================================== zl_reduce_abs_max
@pytest.mark.parametrize("t", ["f16", "bf16", "f32"])
def test_reduce_abs_max(dev, t):
    """per row max |x| from the reference's start -1e4, as T: an element's magnitude, so bit-exact.  The maximum in the first, the
    last and column 1024; negative rows; a NaN ignored (fmaxf); an all-NaN row gives the start value; an infinity gives inf"""
    rng = np.random.default_rng(CODE[t])

    def run(x64, what):
        raw = _encode(x64, t)
        rows, cols = raw.shape
        x, out = _up(raw, dev), _canary((rows + 8) * raw.dtype.itemsize, dev)
        _call("zl_reduce_abs_max", _p(x), _p(out), _i(rows), _i(cols), C.c_int(CODE[t]), _s())
        got = _down(out, raw.dtype)
        assert (_down(out, np.uint8)[rows * raw.dtype.itemsize:] == CANARY).all(), what
        _assert_bits(got[:rows], _encode(G.abs_max_rows(_decode(raw, t)), t), t, what)

    for cols in (1, 63, 64, 65, 1023, 1024, 1025, 14336):
        rowsets = []
        for pos in sorted({0, cols - 1, min(1024, cols - 1)}):
            for peak in (300.0, -300.0):
                r = rng.standard_normal(cols)
                r[pos] = peak
                rowsets.append(r)
        rowsets.append(-np.abs(rng.standard_normal(cols)) - 0.5)                    # negative values only
        one_nan = rng.standard_normal(cols)
        one_nan[cols // 2] = np.nan
        rowsets.append(one_nan)
        rowsets.append(np.full(cols, np.nan))                                       # nothing but NaN: the start value -1e4 as T
        for inf in (np.inf, -np.inf):
            r = rng.standard_normal(cols)
            r[cols - 1] = inf
            rowsets.append(r)
        rowsets.append(rng.standard_normal(cols) * 1e-7)                            # subnormals of half; 0 < max
        rowsets.append(np.zeros(cols))
        i, step = 0, 1
        while i < len(rowsets):                                                     # launches of 1, 2, 3, 1, ... rows
            run(np.stack(rowsets[i:i + step]), f"abs_max {t} cols={cols} rows {i}..{i + step}")
            i, step = i + step, step % 3 + 1
    many = rng.standard_normal((70000, 8))
    many[5] = np.nan
    many[69999, 7] = -77.0
    run(many, f"abs_max {t} 70000 x 8")


# ======================================================================================================================== zl_binary_op
def _edges(t):
    eb, mb, _ = G.FORMATS[t]
    bias = (1 << (eb - 1)) - 1
    tiny, big = 2.0 ** (1 - bias - mb), (2.0 - 2.0 ** -mb) * 2.0 ** bias
    return np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, 2.0 ** (1 - bias) - tiny, big, -big, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.0])


def _binary_want(x, y, op):
    with np.errstate(all="ignore"):
        return [x + y, x - y, x * y, x / y, G.max_gt(x, y)][op]


@pytest.mark.parametrize("t", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("bmode", [0, 1, 2])
def test_binary_op(dev, t, bmode):
    """c = a (op) b, b of the same shape / one value per row / one row: bit-exact against the float64 result rounded ONCE to T (the
    fp32 intermediate of 16-bit operands has more than 2p + 2 bits, so its second rounding changes nothing; for fp32 it is the IEEE
    operation, the division correctly rounded).  Signed zeros, subnormals, overflow, x / 0, 0 / 0, NaN on either side."""
    rng = np.random.default_rng([CODE[t], bmode])
    edges = _edges(t)

    def operand(n):
        v = _normals(rng, n, (1e-6, 1e-2, 1.0, 50.0))
        pick = rng.random(n) < 0.3
        v[pick] = rng.choice(edges, int(pick.sum()))
        return v

    for rows, cols in ((1, 1), (3, 5), (7, 4096), (300, 257)):
        nb = {0: rows * cols, 1: rows, 2: cols}[bmode]
        a64, b64 = operand(rows * cols), operand(nb)
        k = min(rows * cols, edges.size ** 2)
        a64[:k] = np.repeat(edges, edges.size)[:k]                                  # every edge against every edge where b allows
        if bmode == 0:
            b64[:k] = np.tile(edges, edges.size)[:k]
        a_raw, b_raw = _encode(a64, t), _encode(b64, t)
        x = _decode(a_raw, t).reshape(rows, cols)
        yb = _decode(b_raw, t)
        y = yb.reshape(rows, cols) if bmode == 0 else yb[:, None] if bmode == 1 else yb[None, :]
        for op in range(5):
            want = _encode(_binary_want(x, np.broadcast_to(y, x.shape), op), t)
            a_t, b_t = _up(a_raw, dev), _up(b_raw, dev)
            c_t = _canary((rows * cols + 16) * a_raw.dtype.itemsize, dev)
            _call("zl_binary_op", _p(a_t), _p(b_t), _p(c_t), _i(rows), _i(cols), C.c_int(op), C.c_int(bmode), C.c_int(CODE[t]), _s())
            got = _down(c_t, a_raw.dtype)
            assert (_down(c_t, np.uint8)[rows * cols * a_raw.dtype.itemsize:] == CANARY).all()
            what = f"binary {t} op={op} bmode={bmode} {rows}x{cols}"
            _assert_bits(got[:rows * cols], want, t, what, np.stack([x.reshape(-1), np.broadcast_to(y, x.shape).reshape(-1)], 1))
            if bmode == 0:                                                          # in place (BinaryElementwiseOp::inplace): c == a
                _call("zl_binary_op", _p(a_t), _p(b_t), _p(a_t), _i(rows), _i(cols), C.c_int(op), C.c_int(0), C.c_int(CODE[t]), _s())
                _assert_bits(_down(a_t, a_raw.dtype), want, t, what + " in place")


# ======================================================================================================================== zl_scale
@pytest.mark.parametrize("t", ["f16", "bf16", "f32"])
def test_scale(dev, t):
    """T(float(x) * float(T(factor))), the factor a C float: bit-exact (the product of two 16-bit-format values is exact in fp32, the
    fp32 product is the IEEE one)"""
    rng = np.random.default_rng(CODE[t] + 100)
    pool = _all16() if t != "f32" else _encode(np.concatenate([_normals(rng, 70000), _normals(rng, 5000, (1e-42, 1e-36, 1e34)),
                                                               G.special_values("f32")]), t)
    for factor in (0.1, 1.0 / 3.0, -2.5, 1e-4, 65504.0):
        f_t = _decode(_encode(np.array([np.float64(np.float32(factor))]), t), t)[0]
        for n in (pool.size, 1, 255, 256, 257):
            raw = np.roll(pool, -int(rng.integers(0, pool.size)))[:n]
            with np.errstate(all="ignore"):
                want = _encode(_decode(raw, t) * f_t, t)
            x, out = _up(raw, dev), _canary((n + 16) * raw.dtype.itemsize, dev)
            _call("zl_scale", _p(x), _p(out), _i(n), C.c_float(factor), C.c_int(CODE[t]), _s())
            assert (_down(out, np.uint8)[n * raw.dtype.itemsize:] == CANARY).all()
            _assert_bits(_down(out, raw.dtype)[:n], want, t, f"scale {t} factor={factor} n={n}", raw)
            _call("zl_scale", _p(x), _p(x), _i(n), C.c_float(factor), C.c_int(CODE[t]), _s())
            _assert_bits(_down(x, raw.dtype), want, t, f"scale {t} factor={factor} n={n} in place", raw)


# ======================================================================================================================== zl_act_inplace
ACTS = {"silu": (0, G.silu), "gelu": (1, G.gelu_tanh)}


def _ulp_report(name, t, got, want, finite):
    """worst ulp distance and the share of differing elements among `finite`; both sides non-NaN there"""
    d = G.ulp_diff(got[finite], want[finite], t)
    worst, share = int(d.max()), float((d != 0).mean())
    at = int(np.nonzero(finite)[0][int(d.argmax())])
    print(f"glue_ops_errors: {name} {t}: worst {worst} ulp, {share * 100:.4f} % of {int(finite.sum())} elements differ")
    return worst, share, at


@pytest.mark.parametrize("t", ["f16", "bf16"])
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_act_inplace_16bit(dev, act, t):
    """all 65536 patterns against the float64 evaluation rounded to T: at most 1 ulp of T, and at most 1 % of the finite inputs
    differing at all -- an fp32 evaluation within 8 fp32 ulps can flip a 16-bit rounding for about 16 x 2^-24 / 2^-11 = 0.2 % of the
    inputs at most; 1 % leaves a factor five.  NaN stays NaN; +-inf give what float64 gives (silu(-inf) taken as its limit -0)."""
    code, f = ACTS[act]
    raw = _all16()
    x64 = _decode(raw, t)
    want = _encode(f(x64), t)
    buf = _up(raw, dev)
    _call("zl_act_inplace", _p(buf), _i(raw.size), C.c_int(code), C.c_int(CODE[t]), _s())
    got = _down(buf, np.uint16)
    nan_w, nan_g = G.is_nan_bits(want, t), G.is_nan_bits(got, t)
    bad = np.nonzero(nan_w != nan_g)[0]
    assert bad.size == 0, (act, t, "NaN-ness", bad.size, hex(raw[bad[0]]), hex(got[bad[0]]), hex(want[bad[0]]))
    inf_in = np.isinf(x64) & ~nan_w
    assert (G.ulp_diff(got[inf_in], want[inf_in], t) == 0).all(), (act, t, "infinite input", got[inf_in], want[inf_in])
    finite = np.isfinite(x64)
    assert not nan_w[finite].any()
    worst, share, at = _ulp_report(act, t, got, want, finite)
    assert worst <= 1, (act, t, worst, "input", float(x64[at]), hex(raw[at]), "got", hex(got[at]), "want", hex(want[at]))
    assert share <= 0.01, (act, t, share)


@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_act_inplace_f32(dev, act):
    """|got - f64| <= 16 * 2^-24 * max(|f64|, |x| / 2, 2^-126): five to seven fp32 operations at half an ulp each plus expf / tanhf at
    4 ulp; the |x| / 2 term covers the cancellation in 1 + tanh(.) for negative x in gelu.  A dense sweep of [-20, 20], +-88, +-1e4,
    zeros, subnormals; NaN and the infinities as float64 has them."""
    code, f = ACTS[act]
    rng = np.random.default_rng(code)
    x = np.concatenate([np.linspace(-20.0, 20.0, 2_000_001), rng.uniform(-20, 20, 100_000), rng.uniform(-90, 90, 100_000),
                        [88.0, -88.0, 1e4, -1e4, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 2.0 ** -126, -2.0 ** -126, 1e-30, -1e-30,
                         np.inf, -np.inf, np.nan]]).astype(np.float32)
    x64 = x.astype(np.float64)
    want = f(x64)
    buf = _up(x, dev)
    _call("zl_act_inplace", _p(buf), _i(x.size), C.c_int(code), C.c_int(CODE["f32"]), _s())
    got = _down(buf, np.float32).astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (act, x[np.isnan(got) != np.isnan(want)][:5])
    special = ~np.isfinite(want) | ~np.isfinite(x64)
    ok = ~np.isnan(want) & special
    assert np.array_equal(got[ok], want[ok]), (act, x[ok], got[ok], want[ok])
    fin = ~special
    bound = 16 * 2.0 ** -24 * np.maximum(np.maximum(np.abs(want[fin]), np.abs(x64[fin]) / 2), 2.0 ** -126)
    ratio = np.abs(got[fin] - want[fin]) / bound
    at = int(ratio.argmax())
    print(f"glue_ops_errors: {act} f32: worst ratio to the bound {ratio.max():.4f} at x = {x64[fin][at]!r} "
          f"(got {got[fin][at]!r}, float64 {want[fin][at]!r}), {fin.sum()} elements")
    assert ratio.max() <= 1.0, (act, float(ratio.max()), float(x64[fin][at]), float(got[fin][at]), float(want[fin][at]))


# ======================================================================================================================== zl_count_nonfinite
@pytest.mark.parametrize("t", ["f16", "bf16", "f32"])
def test_count_nonfinite(dev, t):
    """*counter += the number of NaN / +inf / -inf elements; the largest finite value and subnormals are finite.  4096 x 256 x 3 + 7
    elements are past the launcher's grid cap: the stride loop and one atomic per thread"""
    rng = np.random.default_rng(CODE[t] + 9)
    eb, mb, _ = G.FORMATS[t]
    bias = (1 << (eb - 1)) - 1
    big, tiny = (2.0 - 2.0 ** -mb) * 2.0 ** bias, 2.0 ** (1 - bias - mb)

    def count(x64):
        raw = _encode(x64, t)
        assert np.array_equal(_isnan(raw, t) | np.isinf(_decode(raw, t)), ~np.isfinite(x64))
        x, counter = _up(raw, dev), torch.full((3,), 5, dtype=torch.int32, device=dev)
        _call("zl_count_nonfinite", _p(x), _i(raw.size), C.c_int(CODE[t]), _p(counter, 4), _s())
        assert counter[0].item() == 5 and counter[2].item() == 5
        return counter[1].item() - 5

    for n in (1, 257, 4096 * 256 * 3 + 7):
        x = rng.standard_normal(n)
        x[rng.integers(0, n, 4)] = [big, -big, tiny, -tiny][:4]
        x[0] = big
        assert count(x) == 0, (t, n, "finite tensor")
        for bad in (np.nan, np.inf, -np.inf):
            y = x.copy()
            y[n - 1] = bad
            assert count(y) == 1, (t, n, bad)
        if n > 1:
            y = x.copy()
            where = rng.choice(n, min(n // 2, 100_000), replace=False)
            y[where] = rng.choice(np.array([np.nan, np.inf, -np.inf]), where.size)
            assert count(y) == where.size, (t, n, where.size)
            assert count(np.full(n, np.nan)) == n


# ======================================================================================================================== permutations
@pytest.mark.parametrize("k", [1, 8, 4096, 65536])
def test_perm_narrow_and_reverse(dev, k):
    """narrow: perm.astype(uint16); reverse: out[perm[i]] = i, reverse(reverse(p)) == p; an entry of -1 or k is dropped (its slot keeps
    the canary) and nothing is written outside the k slots"""
    rng = np.random.default_rng(k)
    perm = rng.permutation(k).astype(np.int32)

    def run(name, p):
        src, out = _up(p, dev), torch.full((k + 64,), 0x5A5A, dtype=torch.int16, device=dev)
        _call(name, _p(src), _p(out, 64), _i(k), _s())
        got = _down(out, np.uint16)
        assert (got[:32] == 0x5A5A).all() and (got[32 + k:] == 0x5A5A).all(), (name, k, "wrote outside")
        return got[32:32 + k]

    assert np.array_equal(run("zl_perm_narrow_u16", perm), perm.astype(np.uint16))
    inv = run("zl_perm_reverse_u16", perm)
    assert np.array_equal(inv, G.perm_reverse(perm, k))
    assert np.array_equal(inv.astype(np.int64)[perm], np.arange(k))
    assert np.array_equal(run("zl_perm_reverse_u16", inv.astype(np.int32)), perm.astype(np.uint16))
    if k >= 8:
        holes = perm.copy()
        holes[1], holes[k - 2] = -1, k
        got = run("zl_perm_reverse_u16", holes)
        want = G.perm_reverse(holes, k, fill=0x5A5A)
        assert (want == 0x5A5A).sum() >= 2
        assert np.array_equal(got, want), (k, np.nonzero(got != want)[0][:5])


@pytest.mark.parametrize("k,n", [(128, 8), (4096, 272), (11008, 100)])
def test_gptq_permute_rows(dev, k, n):
    """nibble row i of the output is nibble row perm[i] of the (K/8, N) input: unpack, take rows, repack.  Valid permutations only (the
    kernel has no guard): random, the argsort of a shuffled group index, the identity"""
    rng = np.random.default_rng(k + n)
    q = rng.integers(0, 2 ** 32, (k // 8, n), dtype=np.uint64).astype(np.uint32)
    g_idx = np.repeat(np.arange(k // 128), 128)
    rng.shuffle(g_idx)
    for name, perm in (("random", rng.permutation(k)), ("argsort(g_idx)", np.argsort(g_idx, kind="stable")), ("identity", np.arange(k))):
        assert np.array_equal(np.sort(perm), np.arange(k))
        out = torch.full((k // 8 * n + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        q_t, p_t = _up(q, dev), _up(perm.astype(np.int32), dev)
        _call("zl_gptq_permute_rows", _p(q_t), _p(out), _p(p_t), _i(k // 8), _i(n), _s())
        got = _down(out, np.uint32)
        assert (got[k // 8 * n:] == 0x5A5A5A5A).all()
        want = G.gptq_permute_rows(q, perm)
        if name == "identity":
            assert np.array_equal(want, q)
        bad = np.nonzero(got[:k // 8 * n] != want.reshape(-1))[0]
        assert bad.size == 0, (name, k, n, bad.size, int(bad[0]), hex(got[bad[0]]), hex(want.reshape(-1)[bad[0]]))


@pytest.mark.parametrize("k", [8, 4096, 65536])
@pytest.mark.parametrize("rows", [1, 5, 33])
def test_permute_input_u16(dev, rows, k):
    """out[r, i] = x[r, perm[i]] with a row stride larger than k; k = 65536 uses the index 65535"""
    rng = np.random.default_rng(rows * 7 + k)
    ldx = k + 24
    x = rng.integers(0, 65536, (rows, ldx), dtype=np.uint16)
    perm = rng.permutation(k)
    out = torch.full((rows * k + 16,), 0x5A5A, dtype=torch.int16, device=dev)
    x_t, p_t = _up(x, dev), _up(perm.astype(np.uint16), dev)
    _call("zl_permute_input_u16", _p(x_t), _i(ldx), _p(p_t), _p(out), _i(rows), _i(k), _s())
    got = _down(out, np.uint16)
    assert (got[rows * k:] == 0x5A5A).all()
    want = x[:, :k][:, perm]
    bad = np.nonzero(got[:rows * k] != want.reshape(-1))[0]
    assert bad.size == 0, (rows, k, bad.size, int(bad[0]), int(got[bad[0]]), int(want.reshape(-1)[bad[0]]))


# ======================================================================================================================== zl_scatter_update_dim0
@pytest.mark.parametrize("row_bytes,dst_off", [(6, 0), (16, 2), (16, 0), (34, 0), (32, 2)])
@pytest.mark.parametrize("with_src_index", [False, True])
def test_scatter_update_dim0_narrow_path(dev, row_bytes, dst_off, with_src_index):
    """dst[dst_index[i], :] = src[src_index ? src_index[i] : i, :] where the rows are not 16-byte material (6 bytes; 16 bytes at a
    destination 2 bytes off): the 2-byte path.  An index of -1 or dst_rows is dropped, every other row keeps the canary."""
    rng = np.random.default_rng([row_bytes, dst_off, int(with_src_index)])
    dst_rows, src_rows, n_index = 41, 29, 23
    src = rng.integers(0, 256, (src_rows, row_bytes), dtype=np.uint8)
    src[src == CANARY] = 1
    di = rng.permutation(dst_rows)[:n_index].astype(np.int32)
    di[3], di[17] = -1, dst_rows
    si = rng.integers(0, src_rows, n_index).astype(np.int32) if with_src_index else None
    want = np.full((dst_rows, row_bytes), CANARY, np.uint8)
    for i in range(n_index):
        if 0 <= di[i] < dst_rows:
            want[di[i]] = src[si[i] if with_src_index else i]
    dst = _canary(dst_off + dst_rows * row_bytes + 64, dev)
    di_t, src_t, si_t = _up(di, dev), _up(src, dev), _up(si, dev) if with_src_index else None
    _call("zl_scatter_update_dim0", _p(dst, dst_off), _p(di_t), _p(src_t), _p(si_t),
          _i(n_index), _i(row_bytes), _i(dst_rows), _i(src_rows), _s())
    got = _down(dst, np.uint8)
    assert (got[:dst_off] == CANARY).all() and (got[dst_off + want.size:] == CANARY).all()
    bad = np.nonzero(got[dst_off:dst_off + want.size] != want.reshape(-1))[0]
    assert bad.size == 0, (bad.size, divmod(int(bad[0]), row_bytes), int(got[dst_off + bad[0]]), int(want.reshape(-1)[bad[0]]))


# ======================================================================================================================== zl_rope_rotate
@pytest.mark.parametrize("t,code", [("f16", 0), ("bf16", 1)])
@pytest.mark.parametrize("neox", [True, False])
@pytest.mark.parametrize("n,heads,d", [(5, 16, 64), (3, 2, 128), (1, 1, 2)])
def test_rope_rotate(oracle, dev, n, heads, d, neox, t, code):
    """the d rope dimensions inside a 192-wide head (MLA's layout) into a dense output and IN PLACE: bit-exact with the oracle's
    rope_qk_cache on the gathered slices (the kernel claims the fused kernels' expression), within 1 ulp of T of the float64 rotation
    (at most 1 % differing: the cap of the activations), and in place nothing outside the slices changes"""
    rng = np.random.default_rng([n, heads, d, int(neox), code])
    wide, lead = 192, 128 if d <= 64 else 64                                       # the slice starts `lead` elements into each head
    pos = rng.integers(0, 4000, n).astype(np.int32)
    cos, sin = oracle.rope_cos_sin(pos, d, 10000.0, neox=neox)
    full = _encode(rng.standard_normal((n, heads, wide)), t)
    x = np.ascontiguousarray(full[:, :, lead:lead + d])
    want_q, _, _ = oracle.rope_qk_cache(cos, sin, np.concatenate([x.reshape(n, heads * d)] * 3, axis=1), heads, heads, d, neox=neox, dtype=code)
    want = want_q.reshape(n, heads, d)
    cs_t, sn_t = _up(cos, dev), _up(sin, dev)

    def check(got, what):
        _assert_bits(got, want, t, what + ": against the oracle's rope_qk_cache")
        ref = _encode(G.rope_rotate(_decode(x, t), cos, sin, neox), t)
        worst, share, at = _ulp_report(f"rope_rotate {'neox' if neox else 'interleaved'} ({n}, {heads}, {d})", t, got.reshape(-1), ref.reshape(-1),
                                       np.ones(got.size, bool))
        assert worst <= 1, (what, worst, at, hex(got.reshape(-1)[at]), hex(ref.reshape(-1)[at]))
        assert share <= 0.01, (what, share)

    src = _up(full, dev)
    out = torch.full((n * heads * d + 16,), 0x5A5A, dtype=torch.int16, device=dev)
    _call("zl_rope_rotate", _p(cs_t), _p(sn_t), _p(src, 2 * lead), _p(out), _i(n), _i(heads), _i(d), _i(heads * wide), _i(wide), _i(heads * d), _i(d),
          C.c_int(int(neox)), C.c_int(code), _s())
    got = _down(out, np.uint16)
    assert (got[n * heads * d:] == 0x5A5A).all()
    assert np.array_equal(_down(src, np.uint16).reshape(full.shape), full)         # the source is untouched
    check(got[:n * heads * d].reshape(n, heads, d), f"rope_rotate {t} neox={neox} ({n},{heads},{d}) dense output")
    _call("zl_rope_rotate", _p(cs_t), _p(sn_t), _p(src, 2 * lead), _p(src, 2 * lead), _i(n), _i(heads), _i(d), _i(heads * wide), _i(wide),
          _i(heads * wide), _i(wide), C.c_int(int(neox)), C.c_int(code), _s())
    after = _down(src, np.uint16).reshape(full.shape)
    check(after[:, :, lead:lead + d], f"rope_rotate {t} neox={neox} ({n},{heads},{d}) in place")
    keep = np.ones(wide, bool)
    keep[lead:lead + d] = False
    assert np.array_equal(after[:, :, keep], full[:, :, keep]), "in place: an element outside the rotated slices changed"


# ======================================================================================================================== zl_mask_valid_lens
@pytest.mark.parametrize("len_q", [1, 3], ids=["len_q1", "len_q3"])
def test_mask_valid_lens(dev, len_q):
    """1 + the last visible key of every task's LAST query row (0 if none) over ragged tasks; earlier rows see a LATER key than the
    last row, so a wrong row gives a wrong length; any nonzero mask value counts as visible"""
    rng = np.random.default_rng(len_q)
    buf_lens = [1, 33, 256, 257, 1088, 300]
    for variant in range(4):
        parts = []
        for b, lb in enumerate(buf_lens):
            m = np.zeros((len_q, lb), np.int8)
            kind = (b + variant) % 6
            if kind == 0:                                        # a prefix
                m[-1, :max(1, lb // 2)] = 1
            elif kind == 1:                                      # holes
                m[-1] = rng.random(lb) < 0.3
                m[-1, max(0, lb - 1 - lb // 3):] = 0
            elif kind == 2:                                      # nothing visible in the whole task
                pass
            elif kind == 3:                                      # only the last key
                m[-1, lb - 1] = 1
            elif kind == 4:                                      # values other than 1
                m[-1, :max(1, lb // 3)] = rng.choice(np.array([2, -1, 127, -128], np.int8), max(1, lb // 3))
            else:                                                # only the first key
                m[-1, 0] = 1
            if len_q > 1 and m[-1].any():                        # the earlier rows reach further than the last one
                last = int(np.nonzero(m[-1])[0][-1])
                if last + 1 < lb:
                    m[:-1, :last + 1] = 1
                    m[0, lb - 1] = 1
                    m[-2, min(lb - 1, last + 1 + (lb - last) // 2)] = 1
            parts.append(m.reshape(-1))
        mask = np.concatenate(parts)
        want = G.mask_valid_lens(mask, buf_lens, len_q)
        out = torch.full((len(buf_lens) + 4,), -7, dtype=torch.int32, device=dev)
        m_t, l_t = _up(mask, dev), _up(np.array(buf_lens, np.int32), dev)
        _call("zl_mask_valid_lens", _p(m_t), _p(l_t), _p(out), _i(len(buf_lens)), _i(len_q), _s())
        got = _down(out, np.int32)
        assert (got[len(buf_lens):] == -7).all()
        assert np.array_equal(got[:len(buf_lens)], want), (len_q, variant, got[:len(buf_lens)].tolist(), want.tolist())
    single = np.zeros(1088, np.int8)                             # one task, last key alone (beyond the block's first trips)
    single[1087] = 1
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    m_t, l_t = _up(np.concatenate([np.zeros(1088 * (len_q - 1), np.int8), single]), dev), _up(np.array([1088], np.int32), dev)
    _call("zl_mask_valid_lens", _p(m_t), _p(l_t), _p(out), _i(1), _i(len_q), _s())
    assert out.item() == 1088


# ======================================================================================================================== zl_argmax_advance
@pytest.mark.parametrize("dt", ["float16", "bfloat16", "float32"])
def test_argmax_advance_signed_zeros(dev, dt):
    """-0.0 and +0.0 are one value: the FIRST zero of either sign wins, as torch.argmax([-0.0, 0.0]) == 0.  Aligned rows (the
    16-byte lanes of the 16-bit types) and rows starting 2 bytes off an aligned address (the scalar loop)"""
    from zhilight_amd import ops
    tdt = getattr(torch, dt)
    assert int(torch.argmax(torch.tensor([-0.0, 0.0]))) == 0

    def pick(x):
        tokens = torch.full((x.shape[0],), -1, dtype=torch.int32, device=dev)
        nxt = torch.full((x.shape[0],), -1, dtype=torch.int64, device=dev)
        ops.argmax_advance(x, tokens=tokens, next_tokens=nxt)
        assert torch.equal(tokens.long(), nxt)
        return nxt.tolist()

    assert pick(torch.tensor([[-0.0, 0.0]], dtype=tdt, device=dev)) == [0]
    assert pick(torch.tensor([[0.0, -0.0]], dtype=tdt, device=dev)) == [0]
    assert pick(torch.tensor([[-1.0, -0.0, 0.0, -0.0]], dtype=tdt, device=dev)) == [1]
    n = 128256
    rng = np.random.default_rng(3)
    host = (-np.abs(rng.standard_normal((3, n + 16))) - 0.01).astype(np.float32)
    for shift, what in ((0, "aligned rows"), (1, "rows one element off")):
        base = torch.from_numpy(host).to(dev).to(tdt)
        x = base[:, shift:shift + n]                              # row stride n + 16 elements: every row as (mis)aligned as the first
        assert (x.data_ptr() % 16 == 0) == (shift == 0)
        x[0, 9], x[0, 4000], x[0, 100000] = -0.0, 0.0, 0.0
        x[1, 4000], x[1, 100000] = 0.0, -0.0
        x[2, 100000], x[2, n - 1] = -0.0, 0.0
        assert bool(torch.signbit(x[0, 9])) and not bool(torch.signbit(x[0, 4000]))
        assert pick(x) == [9, 4000, 100000], (dt, what, pick(x))
