#!/usr/bin/env python3
"""Refining per-camera focal lengths in the bundle adjustment (GLOMAP's optimize_intrinsics, estimators/bundle_adjustment.h:16), on the
SIMPLE2 observation list seen with wrong focal priors: each camera's first two coordinates are scaled by a ratio drawn from
[0.9, 1.1], which is what a focal prior off by that ratio does to the normalised observations.

    ctx = xmamd.Context(obs=(cam, lm, p, w))                                     (XM_STORAGE_SCHUR)
    R, s, info = ctx.solve(5, tol, lam);  rot, scale, _ = xmamd.recover_rotations(R, s);  t, P = ctx.recover_tp(rot, scale)
    ctx.bundle_adjust(rot, t, P)                                                  (every focal taken as exact)
    rot, t, P, info = ctx.bundle_adjust(rot, t, P, refine_focal=True)             (info["focal"]: one scale per camera)
    p2 = xmamd.rescale_observations(p, cam, info["focal"]);  ctx2 = xmamd.Context(obs=(cam, lm, p2, w))
    ctx2.filter_tracks(rot, t, P)                                                 (everything without a focal argument now sees the refined calibration)

Printed for both adjustments: the cost, the focal errors and the median rotation error against the recorded ground truth gtR.bin; then
the track filter's verdict on the original and on the rescaled observations.

    python examples/refine_focal_simple2.py [--spread 0.1] [--seed 0]

Needs an MI355X."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
import numpy as np            # noqa: E402
import xmamd                  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def read_bin(fn):
    """int32 rows, int32 cols, float64 column-major"""
    with open(fn, "rb") as f:
        r, c = struct.unpack("<ii", f.read(8))
        return np.frombuffer(f.read(), dtype="<f8").reshape(c, r).T.copy()


def rotation_error(rot, gt, fi):
    """median over the cameras of |R_0^T R_i - G_f(0) G_f(i)^T|_F, f = frame_index (gtR.bin holds world-to-camera rotations per frame)"""
    return float(np.median([np.linalg.norm(rot[:, :3].T @ rot[:, 3 * i:3 * i + 3] - gt[:, 3 * fi[0]:3 * fi[0] + 3] @ gt[:, 3 * fi[i]:3 * fi[i] + 3].T)
                            for i in range(fi.size)]))


G = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(G, "obs.npz"))
gt = read_bin(os.path.join(G, "gtR.bin"))
fi = np.load(os.path.join(G, "frame_index.npy"))
cam, lm, w = Z["cam"], Z["lm"], Z["w"].reshape(-1)
n = int(cam.max()) + 1
spread = arg("--spread", 0.1)
ratio = np.random.default_rng(arg("--seed", 0)).uniform(1.0 - spread, 1.0 + spread, n)     # true focal / prior
p = Z["p"].copy()
p[:, :2] *= ratio[cam][:, None]

ctx = xmamd.Context(obs=(cam, lm, p, w))
R, s, info = ctx.solve(5, 1e-10, 0.0)
rot, scale, _ = xmamd.recover_rotations(R, s)
t, P = ctx.recover_tp(rot, scale)
print(f"XM solve on {cam.size} observations of {n} cameras whose focal priors are off by up to {100 * spread:.0f} %: rank {info['rank']}, "
      f"status {info['status']}, rotation error {rotation_error(rot, gt, fi):.4e}")
rot_a, t_a, P_a, a = ctx.bundle_adjust(rot, t, P)
print(f"bundle_adjust, focals taken as exact: cost {a['initial_cost']:.6e} -> {a['final_cost']:.6e} ({a['iters']} LM iterations, "
      f"{a['status_name']}), focal error max {np.abs(1.0 / ratio - 1.0).max():.3e} (not modelled), rotation error {rotation_error(rot_a, gt, fi):.4e}")
rot_f, t_f, P_f, f = ctx.bundle_adjust(rot, t, P, refine_focal=True)
g = f["focal"]
err = np.abs(g / ratio - 1.0)
print(f"bundle_adjust, refine_focal=True:     cost {f['initial_cost']:.6e} -> {f['final_cost']:.6e} ({f['iters']} LM iterations, "
      f"{f['status_name']}), focal error max {err.max():.3e} median {np.median(err):.3e}, rotation error {rotation_error(rot_f, gt, fi):.4e}")
k0 = ctx.filter_tracks(rot_f, t_f, P_f)
ctx.close()
ctx2 = xmamd.Context(obs=(cam, lm, xmamd.rescale_observations(p, cam, g), w))
k1 = ctx2.filter_tracks(rot_f, t_f, P_f)
sq = ctx2.reprojection_errors(rot_f, t_f, P_f)
ctx2.close()
print(f"filter_tracks at the refined geometry: {int(k0.dropped.sum())} observations dropped on the observations as given, "
      f"{int(k1.dropped.sum())} on those rescaled by the refined focals (cost there at g = 1: {0.5 * sq[sq >= 0].sum():.6e})")
