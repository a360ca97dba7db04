"""CPU tests of the robust losses and non-monotonic steps of xm_ctx_bundle_adjust and of xm_ctx_reprojection_errors (include/xm_amd.h):
the numpy restatement in xm_ba_loss_numpy.py (derivatives, corrected gradient, Ceres's step evaluator), the grown options struct against
the header, and the new export."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_ba_loss_numpy as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBUST = ("huber", "soft_l1", "cauchy", "arctan")


@pytest.mark.parametrize("loss", ROBUST)
def test_loss_derivatives_match_central_differences(loss):
    a = 0.3
    s = np.concatenate([np.geomspace(1e-4, 1e2, 40), [0.5 * a * a, 2.0 * a * a]])
    h, h2 = 1e-6 * s, 1e-4 * s          # rho' is close to 1 at small s: its difference needs the larger step
    r0, r1, r2 = rl.rho(loss, s, a)
    rp, rm = rl.rho(loss, s + h, a)[0], rl.rho(loss, s - h, a)[0]
    r1p, r1m = rl.rho(loss, s + h2, a)[1], rl.rho(loss, s - h2, a)[1]
    assert np.allclose(r1, (rp - rm) / (2 * h), rtol=1e-6, atol=0)
    assert np.allclose(r2, (r1p - r1m) / (2 * h2), rtol=1e-5, atol=0)
    assert np.all(r2 <= 0) and np.all(r1 > 0) and np.all(r1 <= 1)
    # small s: every loss is the trivial one to first order
    assert np.allclose(rl.rho(loss, np.array([1e-12]), a)[0], 1e-12, rtol=1e-6)


def test_huber_is_trivial_below_the_scale():
    s = np.linspace(0.0, 0.09, 10)
    r0, r1, r2 = rl.rho("huber", s, 0.3)
    assert np.array_equal(r0, s) and np.all(r1 == 1.0) and np.all(r2 == 0.0)


def test_rho_prime_is_clamped_at_the_smallest_normal():
    with np.errstate(over="ignore", invalid="ignore"):           # s^2 and a^2 leave the double range here: only rho' is looked at
        for loss in ROBUST:
            assert rl.rho(loss, np.array([1e300]), 1e-150)[1][0] >= np.finfo(np.float64).tiny


@pytest.mark.parametrize("loss", ROBUST)
def test_corrected_gradient_is_the_gradient_of_the_robust_cost(loss):
    S, _ = rl.outlier_scene(n_cams=5, n_pts=12, seed=3, noise=1e-2, frac_out=0.2)
    rot, t, P = ba.perturb(S["rot"], S["t"], S["P"], seed=4)
    pr = rl.RobustProblem(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], loss=loss, a=0.02)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    X = P.T.copy()
    F, r, J = pr.corrected(Rcw, tcw, X)
    assert F == pytest.approx(pr.cost(Rcw, tcw, X), rel=1e-14)
    g = J.T @ r
    nx = pr.cd * pr.n + 3 * pr.m
    h = 1e-6
    gn = np.zeros(nx)
    for k in range(nx):
        d = np.zeros(nx); d[k] = h
        gn[k] = (pr.cost(*pr.plus(Rcw, tcw, X, d)) - pr.cost(*pr.plus(Rcw, tcw, X, -d))) / (2 * h)
    assert np.abs(g - gn).max() <= 1e-6 * np.abs(gn).max()


def test_step_evaluator_on_a_scripted_sequence():
    ev = rl.StepEvaluator(10.0, max_nonmonotonic=2)
    assert ev.quality(9.0, 2.0) == pytest.approx(0.5)
    assert ev.accepted(9.0, 2.0)                               # new minimum: candidate = reference bookkeeping restarts
    assert (ev.minimum, ev.reference, ev.dm_ref, ev.dm_cand, ev.steps) == (9.0, 10.0, 2.0, 0.0, 0)
    # a step up: its own ratio is negative, the historical one (against the reference 10) accepts it
    q = ev.quality(9.5, 1.0)
    assert (9.0 - 9.5) / 1.0 < 0 and q == pytest.approx((10.0 - 9.5) / 3.0)
    assert not ev.accepted(9.5, 1.0)
    assert (ev.steps, ev.candidate, ev.dm_cand, ev.reference) == (1, 9.5, 0.0, 10.0)
    assert not ev.accepted(9.2, 0.5)                           # still above the minimum: second non-monotonic step -> reset
    assert ev.steps == 2 and ev.candidate == 9.5 and ev.dm_cand == 0.5
    assert ev.reference == 9.5 and ev.dm_ref == 0.5
    assert ev.quality(9.4, 1.0) == pytest.approx(max((9.2 - 9.4) / 1.0, (9.5 - 9.4) / 1.5))
    assert ev.accepted(8.0, 1.0) and ev.steps == 0 and ev.minimum == 8.0


def test_nonmonotonic_lm_returns_the_least_cost_point():
    # the scene of the GPU test: steps 5 and 6 go up and are accepted; after 6 iterations the current point is not the best one
    S, _ = rl.outlier_scene(n_cams=16, n_pts=150, seed=215, noise=5e-3, frac_out=0.1, out_size=0.5)
    obs = (S["cam"], S["lm"], S["p"], S["w"])
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=216, deg=40.0, rel=0.4)
    rot, t, P, info = rl.lm(*obs, rot0, t0, P0, nonmonotonic=True, function_tol=1e-12, max_iters=6)
    tr = info["trace"]
    assert info["nonmonotonic_accepts"] >= 1 and np.any((tr[:, 3] == 1) & (tr[:, 1] > tr[:, 0]))
    costs = np.concatenate([tr[:, 0], tr[tr[:, 3] == 1, 1]])
    assert info["final_cost"] == pytest.approx(costs.min(), rel=1e-12) and costs.min() < tr[-1, 0]
    assert rl.robust_cost(*obs, rot, t, P) == pytest.approx(info["final_cost"], rel=1e-12)
    _, _, _, mono = rl.lm(*obs, rot0, t0, P0, function_tol=1e-12, max_iters=6)
    assert not np.array_equal(mono["trace"][:, 3], tr[:, 3])


def test_trivial_restatement_is_xm_ba_numpy():
    S = ba.ring_scene(n_cams=8, n_pts=60, seed=5, noise=2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=6)
    obs = (S["cam"], S["lm"], S["p"], S["w"])
    _, _, _, a = ba.lm(*obs, rot0, t0, P0)
    _, _, _, b = rl.lm(*obs, rot0, t0, P0)
    assert np.array_equal(a["trace"][:, 3], b["trace"][:, 3]) and b["final_cost"] == pytest.approx(a["final_cost"], rel=1e-12)


def test_sq_errors_mark_unused_observations():
    S = ba.ring_scene(n_cams=6, n_pts=20, seed=7, noise=1e-3)
    w = S["w"].copy(); w[3] = 0.0
    p = S["p"].copy(); p[5, 2] = -1.0
    s = rl.sq_errors(S["cam"], S["lm"], p, w, S["rot"], S["t"], S["P"])
    assert s[3] == -1.0 and s[5] == -1.0 and np.all(s[np.r_[0:3, 4, 6:len(s)]] >= 0)


def _c_layout():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu %zu %zu %d %d %u %u\\n", sizeof(xm_ba_options_t), offsetof(xm_ba_options_t, loss),'
           ' offsetof(xm_ba_options_t, max_nonmonotonic), offsetof(xm_ba_options_t, loss_scale), sizeof(xm_ba_result_t),'
           ' XM_BA_LOSS_HUBER + 10 * XM_BA_LOSS_SOFT_L1 + 100 * XM_BA_LOSS_CAUCHY + 1000 * XM_BA_LOSS_ARCTAN, XM_BA_LOSS_TRIVIAL,'
           ' XM_BA_NONMONOTONIC, XM_BA_OPTIONS_SIZE_V1); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_grown_options_struct_matches_ctypes(xmamd):
    so, off_loss, off_maxnm, off_scale, sr, losses, trivial, flag, v1 = _c_layout()
    assert ctypes.sizeof(xmamd.BaOptions) == so == 80 and ctypes.sizeof(xmamd.BaResult) == sr
    assert (xmamd.BaOptions.loss.offset, xmamd.BaOptions.max_nonmonotonic.offset, xmamd.BaOptions.loss_scale.offset) == (off_loss, off_maxnm, off_scale)
    assert off_loss == v1 == xmamd.BA_OPTIONS_SIZE_V1 == 64                      # the first version of the struct ends at trace
    assert xmamd.BaOptions.trace.offset + ctypes.sizeof(ctypes.c_void_p) == v1
    assert losses == 4321 and trivial == 0 and flag == xmamd.BA_NONMONOTONIC == 2
    assert xmamd.BA_LOSS == {"trivial": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}
    assert xmamd.lib().xm_abi_revision() == 4


def test_reprojection_errors_is_exported(xmamd):
    assert hasattr(xmamd.lib(), "xm_ctx_reprojection_errors") and "xm_ctx_reprojection_errors" in xmamd.EXPORTS
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm
    out = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    assert "xm_ctx_reprojection_errors" in {line.split()[-1] for line in out.splitlines() if line.strip()}
