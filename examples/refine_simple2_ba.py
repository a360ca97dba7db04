#!/usr/bin/env python3
"""The reference's last step (5_test_ceres.py:610-616, utils/ceresforXM.py: a Ceres reprojection bundle adjustment of the XM solution)
on the GPU, after the rest of its pipeline on the SIMPLE2 observation list:

    reference:  R_real, s_real, p_est, t_est = recover_XM(Q, R, s, Abar, lam)
                landmarks_2D = landmarks[:, :2] / landmarks[:, 2]
                R_real, t_est, p_est, ... = XM_Ceres_interface(edges, landmarks_2D, R_real, t_est, p_est)
    here:       ctx = xmamd.Context(obs=(cam, lm, p, w))                         (XM_STORAGE_SCHUR)
                R, s, info = ctx.solve(5, tol, lam)
                rot, scale, _ = xmamd.recover_rotations(R, s);  t, P = ctx.recover_tp(rot, scale)
                rot, t, P, ba_info = ctx.bundle_adjust(rot, t, P)                 (the 2D observations are p[:2] / p[2] of the context)

    python examples/refine_simple2_ba.py [--precond jacobi|blocks|two_level]
--precond: the PCG's preconditioner (Context.bundle_adjust(preconditioner=...)); "two_level" is meant for sequential captures, on a scene
like this one (every camera sees much of the scene) the default is the cheaper choice.

Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
import numpy as np            # noqa: E402
import xmamd                  # noqa: E402

G = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(G, "obs.npz"))
ctx = xmamd.Context(obs=(Z["cam"], Z["lm"], Z["p"], Z["w"]))
R, s, info = ctx.solve(5, 1e-10, 0.0)
rot, scale, _ = xmamd.recover_rotations(R, s)
t, P = ctx.recover_tp(rot, scale)
precond = sys.argv[sys.argv.index("--precond") + 1] if "--precond" in sys.argv else "jacobi"
rot2, t2, P2, ba = ctx.bundle_adjust(rot, t, P, preconditioner=precond)
ctx.close()
print(f"XM solve: rank {info['rank']}, status {info['status']}, {info['seconds'] * 1e3:.1f} ms")
print(f"bundle adjustment: {ba['n_used']} observations, reprojection cost {ba['initial_cost']:.6e} -> {ba['final_cost']:.6e} "
      f"({ba['iters']} LM iterations, {ba['accepted']} accepted, {ba['pcg_iters']} PCG iterations, {ba['seconds'] * 1e3:.1f} ms, "
      f"stop: {ba['status_name']}, |J^T r|_inf {ba['gradient_max']:.2e}; preconditioner {precond}, coarse fallbacks {ba['coarse_fallbacks']})")
