"""CPU tests of the radial refinement's ABI (include/xm_amd.h: XM_BA_REFINE_RADIAL, xm_ctx_bundle_adjust_radial,
xm_ctx_reprojection_errors_radial, xm_ctx_ba_probe_radial): the header constants against the Python binding, no struct grown and the ABI
revision left as it was, the three exports, and the refusals that Python raises before any device call."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = (" int (*f)(xm_ctx_t *, const xm_ba_options_t *, double *, double *, double *, double *, const uint8_t *, double *, const uint8_t *,"
         " xm_ba_result_t *) = xm_ctx_bundle_adjust_radial; (void)f;"
         " int (*g)(xm_ctx_t *, const double *, const double *, const double *, const double *, const double *, double *) ="
         " xm_ctx_reprojection_errors_radial; (void)g;"
         " int (*h)(xm_ctx_t *, const double *, const double *, const double *, const double *, const uint8_t *, const double *, const uint8_t *,"
         " xm_ba_probe_t *, double *, double *) = xm_ctx_ba_probe_radial; (void)h;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n'
           'int main(){printf("%u %u %zu %zu %zu %d %u %u %u %u %u\\n", XM_BA_REFINE_RADIAL, XM_BA_REFINE_FOCAL, sizeof(xm_ba_options_t),'
           ' sizeof(xm_ba_probe_t), sizeof(xm_ba_result_t), XM_ABI_REVISION, XM_BA_FIX_ROTATIONS, XM_BA_NONMONOTONIC, XM_BA_DENSE_SCHUR,'
           ' XM_BA_PRECOND_TWO_LEVEL, XM_BA_PRECOND_BLOCKS);' + DECLS + ' return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(DECLS, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_constants_match_the_binding(xmamd):
    flag, focal, so, sp, sr, rev, fix, nonmono, dense, two, blocks = _c_values()
    assert flag == xmamd.BA_REFINE_RADIAL == 256 and focal == xmamd.BA_REFINE_FOCAL == 128
    assert flag & (focal | fix | nonmono | dense | two | blocks | 4 | 8) == 0    # a bit of its own; 4 and 8 stay unknown flags
    assert so == 80 == ctypes.sizeof(xmamd.BaOptions)                            # no struct grew
    assert sp == 280 == ctypes.sizeof(xmamd.BaProbe) and sr == ctypes.sizeof(xmamd.BaResult)
    assert rev == 4 == xmamd.lib().xm_abi_revision()


def test_the_new_symbols_are_exported_and_declared(xmamd):
    names = ("xm_ctx_bundle_adjust_radial", "xm_ctx_reprojection_errors_radial", "xm_ctx_ba_probe_radial")
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm
    out = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = xmamd.lib()
    for s in names:
        assert s in xmamd.EXPORTS and s in defined and hasattr(L, s)
        assert getattr(L, s).argtypes is not None, s
    assert len(L.xm_ctx_bundle_adjust_radial.argtypes) == 10 and len(L.xm_ctx_reprojection_errors_radial.argtypes) == 7
    assert len(L.xm_ctx_ba_probe_radial.argtypes) == 11


def _no_device(xmamd, n=4, m=5):
    ctx = xmamd.Context.__new__(xmamd.Context)   # no device and no handle: a call that got as far as the library would fail on ctx.h
    ctx.n, ctx.n_landmarks = n, m
    return ctx, (np.tile(np.eye(3), (1, n)), np.zeros((3, n)), np.ones((3, m)))


@pytest.mark.parametrize("kw, word", [
    (dict(preconditioner="two_level"), "two_level"),
    (dict(preconditioner="blocks"), "blocks"),
    (dict(focal=[1.0, 0.0, 1.0, 1.0]), "> 0"),
    (dict(focal=[1.0, 1.0, 1.0]), "4 cameras"),
    (dict(focal_free=[1, 0, 1]), "4 cameras"),
    (dict(distortion=[0.0, float("nan"), 0.0, 0.0]), "finite"),
    (dict(distortion=[0.0, float("inf"), 0.0, 0.0]), "finite"),
    (dict(distortion=[0.0, 0.1, 0.0]), "4 cameras"),
    (dict(distortion_free=[1, 0, 1]), "4 cameras"),
])
def test_python_refuses_before_the_device(xmamd, kw, word):
    ctx, (rot, t, P) = _no_device(xmamd)
    with pytest.raises(xmamd.XmError, match=word):
        ctx.bundle_adjust(rot, t, P, refine_distortion=True, **kw)
    with pytest.raises(xmamd.XmError, match=word):
        ctx.ba_probe_radial(rot, t, P, 1.0, **kw)
    if "distortion" in kw:
        with pytest.raises(xmamd.XmError, match=word):
            ctx.reprojection_errors(rot, t, P, distortion=kw["distortion"])


def test_distortion_with_focal_groups_is_refused_before_the_device(xmamd):
    ctx, (rot, t, P) = _no_device(xmamd)
    with pytest.raises(xmamd.XmError, match="focal_group"):
        ctx.bundle_adjust(rot, t, P, refine_distortion=True, focal_group=[0, 0, 1, 1])
    with pytest.raises(xmamd.XmError, match="focal_group"):
        ctx.bundle_adjust(rot, t, P, refine_focal=True, refine_distortion=True, focal_group=[0, 0, 1, 1], focal=[1.0, 1.0])


def test_distortion_arguments_need_the_option(xmamd):
    ctx, (rot, t, P) = _no_device(xmamd)
    for kw in (dict(distortion=np.zeros(4)), dict(distortion_free=np.ones(4)), dict(refine_focal=True, distortion=np.zeros(4))):
        with pytest.raises(xmamd.XmError, match="refine_distortion"):
            ctx.bundle_adjust(rot, t, P, **kw)
