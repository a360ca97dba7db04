"""CPU tests of the ABI of the global positioning (xm_ctx_global_positioning, xm_ctx_gp_probe, xm_gp_limits; include/xm_amd.h): the sizes
and offsets of the new structs against ctypes, the exports, the host-only limits and the random start, and the ABI revision left as it was."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import xm_gp_numpy as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("xm_ctx_global_positioning", "xm_ctx_gp_probe", "xm_gp_limits")


def _c_sizes():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(xm_gp_options_t), sizeof(xm_gp_result_t), sizeof(xm_gp_probe_t),'
           ' offsetof(xm_gp_options_t, trace), offsetof(xm_gp_options_t, loss_scale), offsetof(xm_gp_result_t, trace_len),'
           ' offsetof(xm_gp_probe_t, s), offsetof(xm_gp_probe_t, step2), offsetof(xm_gp_probe_t, M), offsetof(xm_gp_probe_t, s1)); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_struct_sizes_match_ctypes(xmamd):
    so, sr, sp, o_trace, o_scale, o_len, o_s, o_step2, o_M, o_s1 = _c_sizes()
    assert (ctypes.sizeof(xmamd.GpOptions), ctypes.sizeof(xmamd.GpResult), ctypes.sizeof(xmamd.GpProbe)) == (so, sr, sp)
    assert xmamd.GpOptions.trace.offset == o_trace and xmamd.GpOptions.loss_scale.offset == o_scale
    assert xmamd.GpResult.trace_len.offset == o_len
    assert (xmamd.GpProbe.s.offset, xmamd.GpProbe.step2.offset, xmamd.GpProbe.M.offset, xmamd.GpProbe.s1.offset) == (o_s, o_step2, o_M, o_s1)
    assert xmamd.lib().xm_abi_revision() == 4                      # new entries only: the revision does not change
    assert ctypes.sizeof(xmamd.BaOptions) == 80 and ctypes.sizeof(xmamd.BaResult) == 72      # the bundle adjustment's structs as they were


def test_entries_are_exported(xmamd):
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm
    out = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in SYMBOLS:
        assert hasattr(xmamd.lib(), s) and s in xmamd.EXPORTS and s in names, s


def test_limits_and_random_start(xmamd):
    lim = xmamd.gp_limits()
    assert lim == dict(light_max=64, cam_pass=64, threads=1024)
    assert xmamd.lib().xm_gp_limits(None) == -2                    # XM_ERR_ARG
    t, P = xmamd.gp_random_start(7, 11, seed=3)
    t2, P2 = gp.random_start(7, 11, seed=3)
    assert t.shape == (3, 7) and P.shape == (3, 11) and np.array_equal(t, t2) and np.array_equal(P, P2)
    assert np.abs(t).max() <= 100 and np.abs(P).max() <= 100 and np.abs(P).max() > 50
    assert not np.array_equal(xmamd.gp_random_start(7, 11, seed=4)[0], t)
