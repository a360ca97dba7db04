#!/usr/bin/env python3
"""The reference's second driver (2_test_creatematrix.py) with its dense Q built ON THE DEVICE from the observation list:

    reference:  create_matrix(weights, edges, landmarks, path)   -> Q.bin + Abar.bin (process pool per camera, dense solve on the host)
                XM.solve(path, 5, 1e-1, lam, 1000);  recover_XM(Q, R, s, Abar, lam)
    here:       ctx = xmamd.Context(obs=(cam, lm, p, w), tuning=dict(schur_dense_q=1))
                    the observation lists stay (residuals, recovery, XM^2, cleaning, bundle adjustment) and the context also owns the dense Q:
                    every product of the solve is the dense kernel's (72 N^2 bytes, independent of the number of observations)
                R, s, info = ctx.solve(5, tol, lam)
                rot, scale, _ = xmamd.recover_rotations(R, s);  t, P = ctx.recover_tp(rot, scale)

xmamd.create_matrix(weight, edges, landmarks, path) is the drop-in for the reference's function itself (writes Q.bin and Abar.bin).
The observation list is the one the reference's pipeline hands to create_matrix for assets/SIMPLE2 (tests/golden/simple2/obs.npz).
Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
import numpy as np            # noqa: E402
import xmamd                  # noqa: E402

G = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(G, "obs.npz"))
ref = np.load(os.path.join(G, "tp.npz"))
ctx = xmamd.Context(obs=(Z["cam"], Z["lm"], Z["p"], Z["w"]), tuning=dict(schur_dense_q=1))
Q = ctx.dense_q()
print(f"dense Q {Q.shape[0]} x {Q.shape[1]} built on the device, symmetric bit for bit: {np.array_equal(Q, Q.T)}; product kernel: {ctx.product_kind(3)}")
R, s, info = ctx.solve(5, 1e-10, 0.0)
rot, scale, nneg = xmamd.recover_rotations(R, s)
t, P = ctx.recover_tp(rot, scale)
ctx.close()
print(f"cameras {scale.size}, landmarks {P.shape[1]}, observations {Z['cam'].size}: rank {info['rank']}, status {info['status']}, "
      f"primal {info['primal']:.6e}, min eig {info['min_eig']:.2e}, {info['tcg_iters']} tCG iterations, {info['qw_bytes'] / 1e6:.2f} MB per product")
print("against the reference's own run (solved to tol 1e-1 only): rotations", float(np.abs(rot - ref['R_real']).max()),
      "translations", float(np.abs(t - ref['t_est']).max()), "landmarks", float(np.abs(P - ref['p_est']).max()))
