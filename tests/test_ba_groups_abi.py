"""CPU tests of the focal groups' ABI (include/xm_amd.h: xm_ctx_bundle_adjust_focal_groups, xm_ctx_ba_probe_focal_groups): the header's
declarations against the Python binding, no struct grown and the ABI revision left as it was, the two exports, and the refusals that need
no device: those Python raises before any call, and those the library makes before it touches its context."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = (" int (*f)(xm_ctx_t *, const xm_ba_options_t *, double *, double *, double *, int64_t, const int32_t *, double *, const uint8_t *,"
         " xm_ba_result_t *) = xm_ctx_bundle_adjust_focal_groups; (void)f;"
         " int (*h)(xm_ctx_t *, const double *, const double *, const double *, int64_t, const int32_t *, const double *, const uint8_t *,"
         " xm_ba_probe_t *, double *) = xm_ctx_ba_probe_focal_groups; (void)h;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n'
           'int main(){printf("%u %zu %zu %zu %d\\n", XM_BA_REFINE_FOCAL, sizeof(xm_ba_options_t), sizeof(xm_ba_probe_t),'
           ' sizeof(xm_ba_result_t), XM_ABI_REVISION);' + DECLS + ' return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(DECLS, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_the_header_declares_what_the_binding_calls_and_no_struct_grew(xmamd):
    flag, so, sp, sr, rev = _c_values()
    assert flag == xmamd.BA_REFINE_FOCAL == 128
    assert so == 80 == ctypes.sizeof(xmamd.BaOptions)
    assert sp == 280 == ctypes.sizeof(xmamd.BaProbe) and sr == ctypes.sizeof(xmamd.BaResult)
    assert rev == 4 == xmamd.lib().xm_abi_revision()


def test_the_new_symbols_are_exported_and_bound(xmamd):
    names = ("xm_ctx_bundle_adjust_focal_groups", "xm_ctx_ba_probe_focal_groups")
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm
    out = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = xmamd.lib()
    for s in names:
        assert s in xmamd.EXPORTS and s in defined and hasattr(L, s)
    assert len(L.xm_ctx_bundle_adjust_focal_groups.argtypes) == 10 and len(L.xm_ctx_ba_probe_focal_groups.argtypes) == 10
    assert L.xm_ctx_bundle_adjust_focal_groups.argtypes[5] is ctypes.c_int64 and L.xm_ctx_ba_probe_focal_groups.argtypes[4] is ctypes.c_int64


def _no_device(xmamd, n=4, m=5):
    ctx = xmamd.Context.__new__(xmamd.Context)   # no device and no handle: a call that got as far as the library would fail on ctx.h
    ctx.n, ctx.n_landmarks = n, m
    return ctx, (np.tile(np.eye(3), (1, n)), np.zeros((3, n)), np.ones((3, m)))


@pytest.mark.parametrize("kw, word", [
    (dict(focal_group=[0, 1, 0, 1], preconditioner="two_level"), "two_level"),
    (dict(focal_group=[0, 1, 0, 1], preconditioner="blocks"), "blocks"),
    (dict(focal_group=[0, 1, 0, 1], focal=[1.0, 0.0]), "> 0"),
    (dict(focal_group=[0, 1, 0, 1], focal=[1.0, float("nan")]), "> 0"),
    (dict(focal_group=[0, 1, 0, 1], focal=[1.0, float("inf")]), "> 0"),
    (dict(focal_group=[0, 1, 0, 2], focal=[1.0, 1.0]), "outside"),
    (dict(focal_group=[0, -1, 0, 1], focal=[1.0, 1.0]), "outside"),
    (dict(focal_group=[0, 1, 0], focal=[1.0, 1.0]), "per camera"),
    (dict(focal_group=[0.0, 1.0, 0.0, 1.0]), "integer"),
    (dict(focal_group=[0, 1, 0, 1], focal=np.ones(5)), "5 groups"),
    (dict(focal_group=[0, 1, 0, 1], focal=[]), "0 groups"),
    (dict(focal_group=[0, 1, 0, 1], focal=[1.0, 1.0], focal_free=[1, 0, 1]), "3 values"),
])
def test_python_refuses_before_the_device(xmamd, kw, word):
    ctx, (rot, t, P) = _no_device(xmamd)
    with pytest.raises(xmamd.XmError, match=word):
        ctx.bundle_adjust(rot, t, P, refine_focal=True, **kw)
    with pytest.raises(xmamd.XmError, match=word):
        ctx.ba_probe_focal(rot, t, P, 1.0, **kw)


def test_groups_need_the_option(xmamd):
    ctx, (rot, t, P) = _no_device(xmamd)
    with pytest.raises(xmamd.XmError, match="refine_focal"):
        ctx.bundle_adjust(rot, t, P, focal_group=[0, 1, 0, 1])


def test_the_exact_block_constant(xmamd):
    src = '#include "xm_amd.h"\n#include <stdio.h>\nint main(){printf("%d\\n", XM_BA_FOCAL_GROUPS_EXACT); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        assert int(subprocess.check_output([os.path.join(d, "t")])) == 16 == xmamd.BA_FOCAL_GROUPS_EXACT


def test_the_library_refuses_null_arguments_without_a_device(xmamd):
    """XM_ERR_ARG from both entry points before the context is touched"""
    L = xmamd.lib()
    opt, res, q = xmamd.BaOptions(), xmamd.BaResult(), xmamd.BaProbe()
    a = np.zeros(9)
    v = a.ctypes.data_as(ctypes.c_void_p)
    g = np.zeros(1, dtype=np.int32).ctypes.data_as(ctypes.c_void_p)
    assert L.xm_ctx_bundle_adjust_focal_groups(None, ctypes.byref(opt), v, v, v, 1, g, v, None, ctypes.byref(res)) == -2              # XM_ERR_ARG
    assert L.xm_ctx_ba_probe_focal_groups(None, v, v, v, 1, g, v, None, ctypes.byref(q), None) == -2              # XM_ERR_ARG
