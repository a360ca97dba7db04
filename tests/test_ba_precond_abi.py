"""CPU tests of the ABI of the opt-in PCG preconditioners of xm_ctx_bundle_adjust (include/xm_amd.h): the four defines, the structs left at
their sizes with coarse_fallbacks in the result's former tail padding, the ABI revision, and the binding's agreement with the header."""
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%u %u %d %d %zu %zu %zu %d %u %u %u\\n", XM_BA_PRECOND_TWO_LEVEL, XM_BA_PRECOND_BLOCKS, XM_BA_AGG_CAMS,'
           ' XM_BA_MAX_AGGREGATES, sizeof(xm_ba_options_t), sizeof(xm_ba_result_t), offsetof(xm_ba_result_t, coarse_fallbacks), XM_ABI_REVISION,'
           ' XM_BA_FIX_ROTATIONS, XM_BA_NONMONOTONIC, XM_BA_DENSE_SCHUR);'
           ' int (*f)(int64_t, int64_t, const int32_t *, const int32_t *, const uint8_t *, int, int32_t *) = xm_ba_aggregate_plan; (void)f; return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declaration must match the signature above (the executable never calls it, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        src2 = src.replace(" int (*f)(int64_t, int64_t, const int32_t *, const int32_t *, const uint8_t *, int, int32_t *) = xm_ba_aggregate_plan; (void)f;", "")
        open(os.path.join(d, "t2.c"), "w").write(src2)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_defines_and_struct_sizes(xmamd):
    two, blocks, agg, nmax, so, sr, off, rev, fix, nonmono, dense = _c_values()
    assert (two, blocks, agg, nmax) == (32, 64, 16, 4096)
    assert so == 80 and sr == 72 and off == 68 and rev == 4                       # no struct grew; the new field fills the tail padding
    for f in (two, blocks):
        assert f & (1 | 2 | 4 | 8 | 16) == 0 and f & (fix | nonmono | dense) == 0
    assert two & blocks == 0


def test_binding_agrees_with_the_header(xmamd):
    two, blocks, agg, nmax, so, sr, off, rev, _, _, _ = _c_values()
    assert xmamd.BA_PRECOND_TWO_LEVEL == two and xmamd.BA_PRECOND_BLOCKS == blocks and xmamd.BA_AGG_CAMS == agg and xmamd.BA_MAX_AGGREGATES == nmax
    assert xmamd.BA_PRECONDITIONERS == {"jacobi": 0, "blocks": blocks, "two_level": two}
    assert ctypes.sizeof(xmamd.BaOptions) == so and ctypes.sizeof(xmamd.BaResult) == sr
    assert xmamd.BaResult.coarse_fallbacks.offset == off and xmamd.BaResult.trace_len.offset == 64
    assert xmamd.lib().xm_abi_revision() == rev
    assert "xm_ba_aggregate_plan" in xmamd.EXPORTS and hasattr(xmamd.lib(), "xm_ba_aggregate_plan")


def test_unknown_preconditioner_is_refused_before_the_device(xmamd):
    import numpy as np
    ctx = xmamd.Context.__new__(xmamd.Context)   # no device: the name is checked before anything else is looked at
    ctx.n, ctx.n_landmarks = 1, 1
    try:
        ctx.bundle_adjust(np.eye(3), np.zeros((3, 1)), np.zeros((3, 1)), preconditioner="multigrid")
    except xmamd.XmError as e:
        assert "multigrid" in str(e)
    else:
        raise AssertionError("an unknown preconditioner was accepted")
