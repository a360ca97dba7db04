#!/usr/bin/env python3
"""Refining ONE focal length per physical camera in the bundle adjustment (GLOMAP shares a Camera among its images:
estimators/bundle_adjustment.cc:72-84), on the SIMPLE2 observation list seen with wrong focal priors.  Two captures are made up:
  (a) one camera took every image: every image's first two coordinates are scaled by the same ratio (a prior off by that ratio);
  (b) three cameras took them in turn (image i by camera i mod 3), each with a ratio of its own.

    rot, t, P, info = ctx.bundle_adjust(rot, t, P)                                              (every focal taken as exact)
    rot, t, P, info = ctx.bundle_adjust(rot, t, P, refine_focal=True)                           (info["focal"]: one scale per image)
    rot, t, P, info = ctx.bundle_adjust(rot, t, P, refine_focal=True, focal_group=group_of)     (info["focal"]: one scale per camera)
    p2 = xmamd.rescale_observations(p, cam, info["focal"][group_of]);  ctx2 = xmamd.Context(obs=(cam, lm, p2, w));  ctx2.filter_tracks(rot, t, P)

Printed for the three forms: the cost, the focal errors and the median rotation error against the recorded ground truth gtR.bin; then
the track filter's verdict on the observations rescaled by the shared focals.

    python examples/refine_shared_focal_simple2.py [--ratio 1.08] [--seed 0]

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
    """median over the images of |R_0^T R_i - G_f(0) G_f(i)^T|_F, f = frame_index (gtR.bin holds world-to-camera rotations per frame)"""
    return float(np.median([np.linalg.norm(rot[:, :3].T @ rot[:, 3 * i:3 * i + 3] - gt[:, 3 * fi[0]:3 * fi[0] + 3] @ gt[:, 3 * fi[i]:3 * fi[i] + 3].T)
                            for i in range(fi.size)]))


G = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(G, "obs.npz"))
gt = read_bin(os.path.join(G, "gtR.bin"))
fi = np.load(os.path.join(G, "frame_index.npy"))
cam, lm, w = Z["cam"], Z["lm"], Z["w"].reshape(-1)
n = int(cam.max()) + 1
one = arg("--ratio", 1.08)
three = np.random.default_rng(arg("--seed", 0)).uniform(0.9, 1.1, 3)

for label, group_of, ratio in (("(a) one camera", np.zeros(n, dtype=np.int32), np.array([one])),
                               ("(b) three cameras", (np.arange(n) % 3).astype(np.int32), three)):
    p = Z["p"].copy()
    p[:, :2] *= ratio[group_of][cam][:, None]
    ctx = xmamd.Context(obs=(cam, lm, p, w))
    R, s, info = ctx.solve(5, 1e-10, 0.0)
    rot, scale, _ = xmamd.recover_rotations(R, s)
    t, P = ctx.recover_tp(rot, scale)
    print(f"{label}: true focal / prior = {np.array2string(ratio, precision=4)}; XM solve: rank {info['rank']}, rotation error {rotation_error(rot, gt, fi):.4e}")
    rot_a, _, _, a = ctx.bundle_adjust(rot, t, P)
    print(f"  focals taken as exact:   cost {a['initial_cost']:.6e} -> {a['final_cost']:.6e} ({a['iters']} LM iterations, {a['status_name']}), "
          f"rotation error {rotation_error(rot_a, gt, fi):.4e}")
    rot_f, _, _, f = ctx.bundle_adjust(rot, t, P, refine_focal=True)
    err = np.abs(f["focal"] / ratio[group_of] - 1.0)
    print(f"  one focal per image:     cost {f['initial_cost']:.6e} -> {f['final_cost']:.6e} ({f['iters']} LM iterations, {f['status_name']}), "
          f"focal error max {err.max():.3e} median {np.median(err):.3e}, rotation error {rotation_error(rot_f, gt, fi):.4e}")
    rot_g, t_g, P_g, g = ctx.bundle_adjust(rot, t, P, refine_focal=True, focal_group=group_of)
    err = np.abs(g["focal"] / ratio - 1.0)
    print(f"  one focal per camera:    cost {g['initial_cost']:.6e} -> {g['final_cost']:.6e} ({g['iters']} LM iterations, {g['pcg_iters']} PCG, "
          f"{g['status_name']}), focal error max {err.max():.3e}, rotation error {rotation_error(rot_g, gt, fi):.4e}")
    ctx.close()
    ctx2 = xmamd.Context(obs=(cam, lm, xmamd.rescale_observations(p, cam, g["focal"][group_of]), w))
    k = ctx2.filter_tracks(rot_g, t_g, P_g)
    ctx2.close()
    print(f"  filter_tracks on the observations rescaled by the shared focals: {int(k.dropped.sum())} of {cam.size} observations dropped")
