#!/usr/bin/env python3
"""Refining one radial distortion coefficient per camera beside the focal scale in the bundle adjustment (COLMAP's SIMPLE_RADIAL; GLOMAP
optimises the camera's whole parameter vector but the principal point, estimators/bundle_adjustment.cc:72-84, :163-175), on the SIMPLE2
observation list seen through distorting lenses with wrong focal priors: with u = (p0, p1) / p2 each camera's first two coordinates
become ratio (1 + k |u|^2) u p2, ratio drawn from [0.9, 1.1] and k from [-0.15, 0.15].

    ctx = xmamd.Context(obs=(cam, lm, p, w))                                     (XM_STORAGE_SCHUR)
    R, s, info = ctx.solve(5, tol, lam);  rot, scale, _ = xmamd.recover_rotations(R, s);  t, P = ctx.recover_tp(rot, scale)
    ctx.bundle_adjust(rot, t, P)                                                  (pinhole: every focal taken as exact, no distortion)
    ctx.bundle_adjust(rot, t, P, refine_focal=True)                               (a focal scale per camera)
    rot, t, P, info = ctx.bundle_adjust(rot, t, P, refine_distortion=True)        (info["focal"], info["distortion"]: one of each per camera)
    p2, no_root = xmamd.undistort_observations(p, cam, info["focal"], info["distortion"]);  ctx2 = xmamd.Context(obs=(cam, lm, p2, w))
    ctx2.filter_tracks(rot, t, P)                                                 (everything without a distortion argument now sees the refined calibration)

Printed for the three models: the cost, the rotation error against the recorded ground truth gtR.bin and how many observations the
track filter drops at the refined geometry on the observations as that model normalises them.

    python examples/refine_radial_simple2.py [--spread 0.1] [--k 0.15] [--seed 0]

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
spread, kmax = arg("--spread", 0.1), arg("--k", 0.15)
rng = np.random.default_rng(arg("--seed", 0))
ratio = rng.uniform(1.0 - spread, 1.0 + spread, n)         # true focal / prior
k = rng.uniform(-kmax, kmax, n)                            # true radial coefficient
p = Z["p"].copy()
u = p[:, :2] / p[:, 2:3]
rho2 = np.sum(u * u, axis=1)
p[:, :2] *= (ratio[cam] * (1.0 + k[cam] * rho2))[:, None]

ctx = xmamd.Context(obs=(cam, lm, p, w))
R, s, info = ctx.solve(5, 1e-10, 0.0)
rot, scale, _ = xmamd.recover_rotations(R, s)
t, P = ctx.recover_tp(rot, scale)
print(f"XM solve on {cam.size} observations of {n} cameras (rays up to rho = {np.sqrt(rho2[p[:, 2] > 0].max()):.2f} off the axis) whose focal priors are off "
      f"by up to {100 * spread:.0f} % and whose lenses have |k| <= {kmax:g}: rank {info['rank']}, status {info['status']}, rotation error "
      f"{rotation_error(rot, gt, fi):.4e}")
out = {}
for name, kw in (("pinhole", {}), ("focal", dict(refine_focal=True)), ("radial", dict(refine_distortion=True))):
    out[name] = ctx.bundle_adjust(rot, t, P, **kw)
ctx.close()
for name, (rot_m, t_m, P_m, a) in out.items():
    g = a.get("focal", np.ones(n))
    kd = a.get("distortion", np.zeros(n))
    q, no_root = xmamd.undistort_observations(p, cam, g, kd)
    c2 = xmamd.Context(obs=(cam, lm, q, w))
    plan = c2.filter_tracks(rot_m, t_m, P_m)
    c2.close()
    line = (f"bundle_adjust, {name:7s}: cost {a['initial_cost']:.6e} -> {a['final_cost']:.6e} ({a['iters']} LM iterations, {a['status_name']}), "
            f"rotation error {rotation_error(rot_m, gt, fi):.4e}, filter_tracks drops {int(plan.dropped.sum())} of {int((w > 0).sum())} observations")
    if name != "pinhole":
        line += f", focal error max {np.abs(g / ratio - 1.0).max():.3e}"
    if name == "radial":
        line += f", k error max {np.abs(kd - k).max():.3e} median {np.median(np.abs(kd - k)):.3e}, {int(no_root.sum())} observations beyond a fold"
    print(line)
