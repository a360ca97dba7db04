"""CPU tests of the ABI of the test export xm_symw_probe (include/xm_amd.h): the prototype and the struct compile from the header, the symbol
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
FIELDS = ("struct_size", "ntot", "nloc", "cam0", "world", "o", "K", "nt", "scal_status", "nitems", "nfull", "alpha", "pad_value", "Q", "W", "cs_all",
          "Prow", "Pcol", "csum", "Y")
PROTO = " int (*f)(xm_symw_probe_t *) = xm_symw_probe; (void)f;"
MARK = -12345.5


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %d %d", sizeof(xm_symw_probe_t), XM_ABI_REVISION, XM_SYMW_PROBE_MAX_NTOT);\n'
           + "".join(f' printf(" %zu", offsetof(xm_symw_probe_t, {f}));\n' for f in FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declaration must match the signature above (the executable never calls it, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    size, rev, cap, *offs = _c_values()
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # an added export: the revision stays
    assert cap == xmamd.SYMW_PROBE_MAX_NTOT == 4096
    assert ctypes.sizeof(xmamd.SymwProbe) == size
    assert [getattr(xmamd.SymwProbe, f).offset for f in FIELDS] == offs and xmamd.SymwProbe.struct_size.offset == 0
    assert [f for f, _ in xmamd.SymwProbe._fields_] == list(FIELDS)


def test_probe_is_exported(xmamd):
    assert "xm_symw_probe" in xmamd.EXPORTS and hasattr(xmamd.lib(), "xm_symw_probe")
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert "xm_symw_probe" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_wrapper_arguments(xmamd):
    sig = inspect.signature(xmamd.symw_probe)
    assert list(sig.parameters) == ["Q", "W", "ntot", "nloc", "cam0", "world", "o", "alpha", "K", "nt", "scal_status", "pad_value", "cs_all"]
    assert list(inspect.signature(xmamd.symw_product).parameters) == ["Q", "W", "world", "o", "alpha", "K", "nt", "scal_status", "pad_value"]
    with pytest.raises(xmamd.XmError, match="3 nloc x 3 ntot"):
        xmamd.symw_probe(np.zeros((6, 11)), np.zeros((12, 3)), 4, 2, 0, 2, 3)
    with pytest.raises(xmamd.XmError, match="cs_all"):
        xmamd.symw_probe(np.zeros((6, 12)), np.zeros((12, 3)), 4, 2, 0, 2, 3, cs_all=np.zeros((2, 12, 3), dtype=np.float32))
    with pytest.raises(xmamd.XmError, match="world divides"):
        xmamd.symw_product(np.zeros((12, 12)), np.zeros((12, 3)), 3, 3)


def _call(xmamd, drop=(), size_delta=0, **kw):
    """the export below the wrapper, every array filled with a mark -> (return code, were all arrays and in/out fields left as they were)"""
    a = dict(ntot=8, nloc=4, cam0=4, world=2, o=3, K=0, nt=-1, scal_status=-1, alpha=1.0, pad_value=0.0)
    a.update(kw)
    sh = dict(Q=(12, 24), W=(24, 3), cs_all=(2, 24, 3), Prow=(1, 12, 3), Pcol=(4, 256, 3), csum=(24, 3), Y=(12, 3))
    arr = {k: np.full(v, MARK) for k, v in sh.items()}
    V = lambda k: None if k in drop else arr[k].ctypes.data_as(ctypes.c_void_p)
    p = xmamd.SymwProbe(struct_size=ctypes.sizeof(xmamd.SymwProbe) + size_delta, nitems=-7, nfull=-9, **a, **{k: V(k) for k in sh})
    rc = xmamd.lib().xm_symw_probe(ctypes.byref(p))
    same = all(np.all(v == MARK) for v in arr.values()) and (p.K, p.nt, p.nitems, p.nfull) == (a["K"], a["nt"], -7, -9)
    return rc, same


def test_bad_arguments_are_refused_before_the_device(xmamd):
    """XM_ERR_ARG (-2) also where there is no device: the arguments are checked first, and nothing is written"""
    bad = [dict(o=2), dict(o=6), dict(o=0), dict(o=-1), dict(nloc=3, world=2), dict(nloc=3, cam0=3, ntot=6), dict(cam0=1), dict(cam0=3),
           dict(ntot=7), dict(ntot=9, nloc=3, cam0=0, world=3), dict(cam0=6),                     # cam0 + nloc > ntot
           dict(world=3), dict(world=1), dict(world=0), dict(nloc=2, cam0=4, world=2),            # world * nloc != ntot
           dict(cam0=2), dict(cam0=-4),                                                           # not a rank's first camera
           dict(ntot=0, nloc=0, cam0=0), dict(ntot=4100, nloc=2050, cam0=0, world=2),    # above XM_SYMW_PROBE_MAX_NTOT only
           dict(nt=2), dict(nt=-2), dict(scal_status=2), dict(scal_status=-2),
           dict(pad_value=np.nan), dict(pad_value=np.inf), dict(pad_value=-np.inf), dict(alpha=np.nan), dict(alpha=np.inf)]
    for kw in bad:
        assert _call(xmamd, **kw) == (-2, True), kw
    for k in ("Q", "W", "cs_all"):
        assert _call(xmamd, drop=(k,)) == (-2, True), k
    for d in (-8, 8, -ctypes.sizeof(xmamd.SymwProbe)):
        assert _call(xmamd, size_delta=d) == (-2, True), d
    assert xmamd.lib().xm_symw_probe(None) == -2
    # what is in order passes the checks: with a device it runs (the outputs are optional), without one it is the device that is missing
    rc, same = _call(xmamd, drop=("Prow", "Pcol", "csum", "Y"))
    assert rc in (0, -3) and (rc == 0) != same
    # and through the wrapper
    with pytest.raises(xmamd.XmError, match="error -2"):
        xmamd.symw_probe(np.zeros((12, 24)), np.zeros((24, 2)), 8, 4, 4, 2, 2)
    with pytest.raises(xmamd.XmError, match="error -2"):
        xmamd.symw_probe(np.zeros((9, 18)), np.zeros((18, 3)), 6, 3, 3, 2, 3)
    with pytest.raises(xmamd.XmError, match="error -2"):
        xmamd.symw_probe(np.zeros((12, 24)), np.zeros((24, 3)), 8, 4, 4, 2, 3, pad_value=np.nan)
