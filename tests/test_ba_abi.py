"""CPU tests of the reprojection bundle adjustment (xm_ctx_bundle_adjust, include/xm_amd.h): the numpy restatement's Jacobian against
central differences, the ABI of the new structs, the export, and the revision-4 structs left as they were."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import xm_ba_numpy as ba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_sizes():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(xm_ba_options_t), sizeof(xm_ba_result_t),'
           ' offsetof(xm_ba_options_t, trace), offsetof(xm_ba_result_t, trace_len), sizeof(xm_tuning_t), sizeof(xm_problem_t),'
           ' sizeof(xm_options_t), sizeof(xm_result_t), sizeof(xm_xm2_info_t)); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def _numeric_jacobian(pr, Rcw, tcw, P, h=1e-6):
    nx = pr.cd * pr.n + 3 * pr.m
    cols = []
    for k in range(nx):
        d = np.zeros(nx); d[k] = h
        rp = pr.residuals(*pr.plus(Rcw, tcw, P, d))
        rm = pr.residuals(*pr.plus(Rcw, tcw, P, -d))
        cols.append((rp - rm) / (2 * h))
    return np.stack(cols, axis=1)


def test_numpy_jacobian_matches_central_differences():
    S = ba.ring_scene(n_cams=5, n_pts=12, seed=3, noise=1e-3)
    rot, t, P = ba.perturb(S["rot"], S["t"], S["P"], seed=4)
    for fix in (False, True):
        pr = ba.Problem(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], fix_rotations=fix)
        Rcw, tcw = ba.to_world_to_camera(rot, t)
        X = P.T.copy()
        r, J = pr.jacobian(Rcw, tcw, X)
        assert np.allclose(r, pr.residuals(Rcw, tcw, X), rtol=0, atol=1e-15)
        Jn = _numeric_jacobian(pr, Rcw, tcw, X)
        err = np.abs(J.toarray() - Jn).max() / np.abs(Jn).max()
        assert err < 1e-7, (fix, err)


def test_numpy_lm_converges_on_a_noise_free_scene():
    S = ba.ring_scene(n_cams=8, n_pts=60, seed=5)
    rot, t, P = ba.perturb(S["rot"], S["t"], S["P"], seed=6)
    _, _, _, info = ba.lm(S["cam"], S["lm"], S["p"], S["w"], rot, t, P, gradient_tol=1e-14, parameter_tol=1e-16)
    assert info["final_cost"] < 1e-20 * max(1.0, info["initial_cost"]) and info["accepted"] > 0


def test_scenes_have_positive_depths():
    for S in (ba.ring_scene(seed=1), ba.sequential_scene(n_cams=40, seed=2), ba.ring_scene(n_cams=70, n_pts=40, frac=1.0, seed=3)):
        assert np.all(S["p"][:, 2] > 0.5)


def test_struct_sizes_match_ctypes(xmamd):
    so, sr, off_trace, off_len, st, sp_, sopt, sres, sx2 = _c_sizes()
    assert ctypes.sizeof(xmamd.BaOptions) == so and ctypes.sizeof(xmamd.BaResult) == sr
    assert xmamd.BaOptions.trace.offset == off_trace and xmamd.BaResult.trace_len.offset == off_len
    # the revision-4 structs are untouched
    assert xmamd.lib().xm_abi_revision() == 4
    assert (ctypes.sizeof(xmamd.Tuning), ctypes.sizeof(xmamd.Problem), ctypes.sizeof(xmamd.Options), ctypes.sizeof(xmamd.Result),
            ctypes.sizeof(xmamd.Xm2Info)) == (st, sp_, sopt, sres, sx2)
    assert (st, sp_, sopt, sres, sx2) == (112, 184, 80, 192, 80)


def test_bundle_adjust_is_exported(xmamd):
    assert hasattr(xmamd.lib(), "xm_ctx_bundle_adjust") and "xm_ctx_bundle_adjust" in xmamd.EXPORTS
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm
    out = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    assert "xm_ctx_bundle_adjust" in {line.split()[-1] for line in out.splitlines() if line.strip()}
