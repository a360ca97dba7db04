#!/usr/bin/env python3
"""The four constraint types of GLOMAP's global positioning (estimators/global_positioning.cc:53-60) and its fixed-centre point pass
(controllers/global_mapper.cc:205-217) on the GPU, on SIMPLE2 with the depths thrown away:

    t, P, info = ctx.global_positioning(rot, t0, P0, pairs=(pi, pj, trel), constraint=...)

The rotations are those of gtR.bin.  The reference positions are those of an ONLY_POINTS run from a random start on the whole observation
list.  The camera pairs are every camera with its next ten, their relative translations trel (cam2_from_cam1) computed from the rotations
and these positions with a noise of 1e-3 on the unit vector.  Then every third camera is stripped of its tracks (its bearings are
turned behind it, which the positioning does not use), the start is the reference moved by a tenth of its extent, and each type is run
from it.  Printed per type: how many cameras it positions, how many of the stripped ones, and the largest distance of the positioned
centres from the reference after a similarity alignment, relative to the extent.

    python examples/position_pairs_simple2.py

Needs an MI355X."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
import numpy as np            # noqa: E402
import xmamd                  # noqa: E402


def read_bin(fn):
    """int32 rows, int32 cols, float64 column-major"""
    with open(fn, "rb") as f:
        r, c = struct.unpack("<ii", f.read(8))
        return np.frombuffer(f.read(), dtype="<f8").reshape(c, r).T.copy()


def aligned_error(t, ref, sel):
    """largest distance of the centres sel from ref after the best similarity over them (Umeyama), relative to ref's extent"""
    A0, B0 = t[:, sel], ref[:, sel]
    ma, mb = A0.mean(axis=1, keepdims=True), B0.mean(axis=1, keepdims=True)
    A, B = A0 - ma, B0 - mb
    U, sv, Vt = np.linalg.svd(B @ A.T)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    al = float(np.sum(sv * np.diag(D)) / np.sum(A * A)) * (U @ D @ Vt @ A) + mb
    return float(np.linalg.norm(al - B0, axis=0).max() / np.linalg.norm(ref.max(axis=1) - ref.min(axis=1)))


G = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(G, "obs.npz"))
gt = read_bin(os.path.join(G, "gtR.bin"))
fi = np.load(os.path.join(G, "frame_index.npy"))
cam, lm, w = Z["cam"], Z["lm"], Z["w"].reshape(-1)
p = Z["p"] / np.linalg.norm(Z["p"], axis=1, keepdims=True)                       # the depth is thrown away
rot = np.concatenate([gt[:, 3 * f:3 * f + 3].T for f in fi], axis=1)             # camera to world

ctx = xmamd.Context(obs=(cam, lm, p, w))
n = ctx.n
t_ref, P_ref, g = ctx.global_positioning(rot, seed=1)
print(f"reference: only_points from a random start on all {cam.size} bearings, cost {g['final_cost']:.4e} in {g['iters']} LM iterations")

rng = np.random.default_rng(7)
pi, pj = np.array([(i, j) for i in range(n) for j in range(i + 1, min(n, i + 11))], dtype=np.int32).T
R = np.stack([rot[:, 3 * i:3 * i + 3] for i in range(n)])
d = (t_ref[:, pi] - t_ref[:, pj]).T
trel = np.einsum("kba,kb->ka", R[pj], d / np.linalg.norm(d, axis=1, keepdims=True)) + 1e-3 * rng.standard_normal((pi.size, 3))
trel /= np.linalg.norm(trel, axis=1, keepdims=True)
pairs = (np.ascontiguousarray(pi), np.ascontiguousarray(pj), trel)

stripped = np.arange(n) % 3 == 1
ctx.close()
ctx = xmamd.Context(obs=(cam, lm, np.where(stripped[cam][:, None], -p, p), w))   # behind the camera: not used (weight 0 would cut the graph)
extent = np.linalg.norm(t_ref.max(axis=1) - t_ref.min(axis=1))
t0 = t_ref + 0.1 * extent * rng.uniform(-1, 1, t_ref.shape)
P0 = P_ref + 0.1 * extent * rng.uniform(-1, 1, P_ref.shape)
print(f"{n} cameras, {pi.size} pairs; {int(stripped.sum())} cameras stripped of their tracks; start: the reference moved by up to 0.1 of its extent")
for constraint in ("only_points", "only_cameras", "points_and_cameras_balanced", "points_and_cameras"):
    t, P, info = ctx.global_positioning(rot, t0, P0, pairs=pairs, constraint=constraint)
    moved = np.any(t != t0, axis=0)
    pts = f", then {int(np.any(P != P0, axis=0).sum())} points against the fixed centres" if "points" in info else ""
    print(f"{constraint:28s} positions {int(moved.sum()):3d} cameras ({int((moved & stripped).sum())} of the stripped ones){pts}: cost "
          f"{info['initial_cost']:.4e} -> {info['final_cost']:.4e}, {info['iters']} LM iterations, {info['pcg_iters']} PCG, {info['status_name']}; "
          f"pairs used {info['pairs_used']}, weight_scale_pt {info['weight_scale_pt']:.4g}; centre error {aligned_error(t, t_ref, moved):.3e}")
ctx.close()
