"""Host-side checks of the quantised-history prompt attention (zl_prefill_attn_varlen_q8): the library exports it, the header
declares it, its argument checks return before any device call, and the keyword that reaches it refuses wrong values.  No GPU
needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZL_EINVAL, ZL_ESHAPE, ZL_EDTYPE = -1, -2, -3


def test_symbol_exported_and_declared():
    from zhilight_amd import _lib
    _lib.lib()
    assert "zl_prefill_attn_varlen_q8" in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.SO_PATH), "zl_prefill_attn_varlen_q8")
    hdr = open(os.path.join(ROOT, "include", "zhilight_amd.h")).read()
    decl = re.search(r"\bint\s+zl_prefill_attn_varlen_q8\s*\(([^;]*)\)\s*;", hdr)
    assert decl, "include/zhilight_amd.h does not declare zl_prefill_attn_varlen_q8"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert len(args) == 22
    for name in ("k_codes", "v_codes", "k_scales", "v_scales", "k_new", "v_new", "work", "groups"):
        assert any(re.search(r"\b%s$" % name, a) for a in args), name
    assert not any(re.search(r"\bbshd$", a) for a in args)          # BSHD only: no layout switch


def _call(d=128, h=8, hkv=2, b=5, dtype=0, work=True, groups=0, k_new=True, codes=True):
    from zhilight_amd import _lib
    fake, null = C.c_void_p(1 << 20), C.c_void_p(0)                 # never dereferenced: the checks return first
    return _lib.lib().zl_prefill_attn_varlen_q8(fake, fake, fake, fake, fake if codes else null, fake, fake, fake,
                                                fake if k_new else null, fake, fake, fake if work else null, C.c_int64(10),
                                                C.c_int64(b), C.c_int64(393), C.c_int64(h), C.c_int64(hkv), C.c_int64(d),
                                                C.c_float(0.1), C.c_int(dtype), C.c_int(groups), C.c_void_p(0))


def test_q8_argument_checks_without_device():
    assert _call(d=64) == ZL_ESHAPE
    assert _call(h=8, hkv=3) == ZL_ESHAPE
    assert _call(work=False) == ZL_EINVAL
    assert _call(k_new=False) == ZL_EINVAL
    assert _call(codes=False) == ZL_EINVAL                          # the TABLE may not be null (its entries may, at pos0 = 0)
    assert _call(b=0) == ZL_EINVAL
    assert _call(dtype=2) == ZL_EDTYPE
    assert _call(groups=3) == ZL_EINVAL
