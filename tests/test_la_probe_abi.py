"""CPU tests of the ABI of the test export xm_la_probe (include/xm_amd.h): the prototype and the struct compile from the header, the symbol
is exported, the ABI revision stays where it was (an added export), the binding's struct and argument list agree with the header, and what
the export refuses is refused before any device call, with every output as it was."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("struct_size", "op", "m", "n", "k", "nrhs", "ta", "tb", "lower_only", "info", "lda", "ldb", "ldc", "q", "A", "B", "C")
OPS = ("XM_LA_GEMM_SUB", "XM_LA_CHOLESKY", "XM_LA_SUBSTITUTE", "XM_LA_INVERSE", "XM_LA_LAYOUT", "XM_LA_RANK1_SUB")
PROTO = " int (*f)(xm_la_probe_t *) = xm_la_probe; (void)f;"


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %d %d", sizeof(xm_la_probe_t), XM_ABI_REVISION, XM_LA_PROBE_MAX_N);\n'
           + "".join(f' printf(" %d", {o});\n' for o in OPS)
           + "".join(f' printf(" %zu", offsetof(xm_la_probe_t, {f}));\n' for f in FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declaration must match the signature above (the executable never calls it, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    size, rev, cap, *rest = _c_values()
    ops, offs = rest[:len(OPS)], rest[len(OPS):]
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # an added export: the revision stays
    assert cap == xmamd.LA_PROBE_MAX_N == 4096
    assert ops == [xmamd.LA_OPS[o[len("XM_LA_"):].lower()] for o in OPS] and len(xmamd.LA_OPS) == len(OPS)
    assert ctypes.sizeof(xmamd.LaProbe) == size
    assert [getattr(xmamd.LaProbe, f).offset for f in FIELDS] == offs and xmamd.LaProbe.struct_size.offset == 0
    assert [f for f, _ in xmamd.LaProbe._fields_] == list(FIELDS)


def test_probe_is_exported(xmamd):
    assert "xm_la_probe" in xmamd.EXPORTS and hasattr(xmamd.lib(), "xm_la_probe")
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert "xm_la_probe" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_wrapper_arguments(xmamd):
    sig = inspect.signature(xmamd.la_probe)
    assert list(sig.parameters) == ["op", "a", "b", "c", "m", "n", "k", "nrhs", "ta", "tb", "lower_only", "info", "lda", "ldb", "ldc", "q"]
    with pytest.raises(xmamd.XmError, match="unknown op"):
        xmamd.la_probe("lu")
    with pytest.raises(xmamd.XmError, match="float64"):
        xmamd.la_probe("cholesky", a=np.zeros((2, 2), dtype=np.float32), n=2, lda=2)


def _refused(xmamd, op, arrays, **kw):
    before = {k: v.copy() for k, v in arrays.items() if v is not None}
    with pytest.raises(xmamd.XmError, match="error -2"):
        xmamd.la_probe(op, **arrays, **kw)
    for k, v in before.items():
        assert np.array_equal(arrays[k], v)


def test_bad_arguments_are_refused_before_the_device(xmamd):
    """XM_ERR_ARG (-2) also where there is no device: the arguments are checked first, and nothing is written"""
    a = lambda r, c: np.arange(float(r * c)).reshape(r, c, order="F")
    cap = xmamd.LA_PROBE_MAX_N
    gemm = dict(a=a(4, 3), b=a(3, 5), c=a(4, 5))
    good = dict(m=4, n=5, k=3, lda=4, ldb=3, ldc=4)
    for bad in (dict(m=-1), dict(n=0), dict(k=-3), dict(m=cap + 1), dict(k=cap + 1), dict(lda=3), dict(ldb=2), dict(ldc=3), dict(ta=2), dict(tb=-1),
                dict(lower_only=2), dict(ta=1, lda=2), dict(tb=1, ldb=4), dict(ldc=2 * cap + 1)):
        _refused(xmamd, "gemm_sub", gemm, **{**good, **bad})
    for missing in ("a", "b", "c"):
        _refused(xmamd, "gemm_sub", {**gemm, missing: None}, **good)
    _refused(xmamd, "cholesky", dict(a=a(4, 4)), n=4, lda=3)
    _refused(xmamd, "cholesky", dict(a=a(4, 4)), n=-4, lda=4)
    _refused(xmamd, "cholesky", dict(a=a(4, 4)), n=cap + 1, lda=cap + 1)
    _refused(xmamd, "cholesky", dict(a=None), n=4, lda=4)
    _refused(xmamd, "substitute", dict(a=a(4, 4), c=a(4, 2)), n=4, lda=4, ldc=3, nrhs=2)
    _refused(xmamd, "substitute", dict(a=a(4, 4), c=a(4, 2)), n=4, lda=4, ldc=4, nrhs=0)
    _refused(xmamd, "substitute", dict(a=a(4, 4), c=None), n=4, lda=4, ldc=4, nrhs=2)
    _refused(xmamd, "inverse", dict(a=a(4, 4), c=a(4, 4)), n=4, lda=5, ldc=4)
    _refused(xmamd, "inverse", dict(a=a(4, 4), c=a(4, 4)), n=4, lda=4, ldc=5)
    _refused(xmamd, "layout", dict(a=a(4, 4), c=a(4, 4)), n=4, lda=4, ldc=3)
    _refused(xmamd, "rank1_sub", dict(a=a(4, 4), b=None), n=4, lda=4, q=1.0)
    _refused(xmamd, "rank1_sub", dict(a=a(4, 4), b=a(4, 1)), n=4, lda=5, q=1.0)
    # a wrong struct_size and an unknown op, below the wrapper
    p = xmamd.LaProbe(struct_size=ctypes.sizeof(xmamd.LaProbe) - 8, op=1, n=4, lda=4, info=5, A=gemm["a"].ctypes.data_as(ctypes.c_void_p))
    assert xmamd.lib().xm_la_probe(ctypes.byref(p)) == -2 and p.info == 5
    p = xmamd.LaProbe(struct_size=ctypes.sizeof(xmamd.LaProbe), op=6, n=4, lda=4, info=5, A=gemm["a"].ctypes.data_as(ctypes.c_void_p))
    assert xmamd.lib().xm_la_probe(ctypes.byref(p)) == -2 and p.info == 5
    assert xmamd.lib().xm_la_probe(None) == -2
