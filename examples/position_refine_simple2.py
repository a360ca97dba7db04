#!/usr/bin/env python3
"""Step 5 of GLOMAP's pipeline (controllers/global_mapper.cc:188-231) and the refinement after it on the GPU, on the SIMPLE2 observation
list with the depths thrown away -- rotations and plain 2-D tracks in, cameras and points out, no XM solve and no initial value:

    ctx = xmamd.Context(obs=(cam, lm, p / |p|, w))                                (XM_STORAGE_SCHUR; only the bearings are kept)
    t, P, info = ctx.global_positioning(rot, seed=1)                              (random start, global_positioning.cc)
    plan = ctx.filter_tracks(rot, t, P, reprojection=None, angle=1.0)             (global_mapper.cc:219-225)
    ctx.set_edge_weights(plan.weights(w));  rot, t, P, info = ctx.bundle_adjust(rot, t, P)

The rotations are those of the recorded ground truth gtR.bin.  Printed: the median distance of the camera centres from those of the
reference's own recovery (tp.npz: t_est; the data set records no ground-truth centres) after a similarity alignment, relative to their
extent, after the positioning and after the adjustment, and the median rotation error against gtR.bin after the adjustment (the
positioning leaves the rotations as they are).

    python examples/position_refine_simple2.py [--seed 1]

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


def centre_error(t, ref):
    """median distance of the centres from ref after the best similarity (Umeyama), relative to ref's extent"""
    ma, mb = t.mean(axis=1, keepdims=True), ref.mean(axis=1, keepdims=True)
    A, B = t - ma, ref - mb
    U, sv, Vt = np.linalg.svd(B @ A.T)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    al = float(np.sum(sv * np.diag(D)) / np.sum(A * A)) * (U @ D @ Vt @ A) + mb
    return float(np.median(np.linalg.norm(al - ref, axis=0)) / np.linalg.norm(ref.max(axis=1) - ref.min(axis=1)))


G = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(G, "obs.npz"))
ref = np.load(os.path.join(G, "tp.npz"))
gt = read_bin(os.path.join(G, "gtR.bin"))
fi = np.load(os.path.join(G, "frame_index.npy"))
cam, lm, w = Z["cam"], Z["lm"], Z["w"].reshape(-1)
p = Z["p"] / np.linalg.norm(Z["p"], axis=1, keepdims=True)                       # the depth is thrown away
rot = np.concatenate([gt[:, 3 * f:3 * f + 3].T for f in fi], axis=1)             # camera to world

ctx = xmamd.Context(obs=(cam, lm, p, w))
t, P, g = ctx.global_positioning(rot, seed=arg("--seed", 1))
print(f"global positioning of {ctx.n} cameras and {ctx.n_landmarks} points from {g['n_used']} of {cam.size} bearings, random start: cost "
      f"{g['initial_cost']:.6e} -> {g['final_cost']:.6e} ({g['iters']} LM iterations, {g['pcg_iters']} PCG, {g['status_name']}, {g['seconds']:.3f} s); "
      f"centre error {centre_error(t, ref['t_est']):.4e} (the rotations are the ground truth's)")
plan = ctx.filter_tracks(rot, t, P, reprojection=None, angle=1.0)
ctx.set_edge_weights(plan.weights(w))
print(f"angle filter at 1 degree: kept {plan.info['obs_kept']} of {plan.info['obs_used']} observations, {plan.info['tracks_kept']} of "
      f"{plan.info['tracks_total']} tracks")
rot_b, t_b, P_b, b = ctx.bundle_adjust(rot, t, P)
print(f"bundle_adjust: cost {b['initial_cost']:.6e} -> {b['final_cost']:.6e} ({b['iters']} LM iterations, {b['status_name']}, {b['seconds']:.3f} s); "
      f"rotation error {rotation_error(rot_b, gt, fi):.4e}, centre error {centre_error(t_b, ref['t_est']):.4e}")
ctx.close()
