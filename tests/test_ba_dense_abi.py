"""CPU tests of the dense Schur solver of xm_ctx_bundle_adjust and of xm_spd_solve (include/xm_amd.h): the header constants against the
Python binding, the options struct and ABI revision left as they were, and the new export."""
import ctypes
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n'
           'int main(){printf("%u %d %zu %u %d %u %u\\n", XM_BA_DENSE_SCHUR, XM_BA_DENSE_MAX_ROWS, sizeof(xm_ba_options_t), XM_BA_OPTIONS_SIZE_V1,'
           ' XM_ABI_REVISION, XM_BA_FIX_ROTATIONS, XM_BA_NONMONOTONIC);'
           ' int (*f)(int64_t, int64_t, const double *, double *) = xm_spd_solve; (void)f; return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declaration must match the signature above (the executable never calls it, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        src2 = src.replace(" int (*f)(int64_t, int64_t, const double *, double *) = xm_spd_solve; (void)f;", "")
        open(os.path.join(d, "t2.c"), "w").write(src2)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_constants_match_the_binding(xmamd):
    flag, rows, so, v1, rev, fix, nonmono = _c_values()
    assert flag == xmamd.BA_DENSE_SCHUR == 16 and rows == xmamd.BA_DENSE_MAX_ROWS == 32768
    assert xmamd.BA_LINEAR_SOLVERS == {"iterative_schur": 0, "dense_schur": 16}
    assert flag & (fix | nonmono | 4 | 8) == 0                                   # 4 and 8 stay unknown flags
    assert so == 80 == ctypes.sizeof(xmamd.BaOptions) and v1 == 64 and rev == 4  # no struct grew
    assert xmamd.lib().xm_abi_revision() == 4


def test_spd_solve_is_declared_and_exported(xmamd):
    assert "xm_spd_solve" in xmamd.EXPORTS and hasattr(xmamd.lib(), "xm_spd_solve")
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm
    out = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    assert "xm_spd_solve" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_unknown_linear_solver_is_refused_before_the_device(xmamd):
    import numpy as np
    ctx = xmamd.Context.__new__(xmamd.Context)   # no device: the name is checked before anything else is looked at
    ctx.n, ctx.n_landmarks = 1, 1
    try:
        ctx.bundle_adjust(np.eye(3), np.zeros((3, 1)), np.zeros((3, 1)), linear_solver="sparse_schur")
    except xmamd.XmError as e:
        assert "sparse_schur" in str(e)
    else:
        raise AssertionError("an unknown linear solver was accepted")
