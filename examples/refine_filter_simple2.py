#!/usr/bin/env python3
"""GLOMAP's alternation of bundle adjustment and track filtering (controllers/global_mapper.cc:243-317, processors/track_filter.cc) on the
GPU, on the SIMPLE2 observation list with a seeded share of its observed points displaced:

    ctx = xmamd.Context(obs=(cam, lm, p, w))                                     (XM_STORAGE_SCHUR)
    R, s, info = ctx.solve(5, tol, lam);  rot, scale, _ = xmamd.recover_rotations(R, s);  t, P = ctx.recover_tp(rot, scale)
    rot, t, P, info = ctx.refine_filtered(rot, t, P)                              (BA with fixed rotations, full BA, filter; repeated)

and, next to it, a plain ctx.bundle_adjust(rot, t, P) from the same start.  Printed: the share of the displaced observations that the loop
removed and the median rotation error against the recorded ground truth gtR.bin before and after either refinement.

    python examples/refine_filter_simple2.py [--share 0.05] [--size 0.05] [--seed 0]

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
cam, lm, w = Z["cam"], Z["lm"], Z["w"]
rng = np.random.default_rng(arg("--seed", 0))
hit = rng.random(cam.size) < arg("--share", 0.05)
ang = rng.uniform(0, 2 * np.pi, cam.size)
p = Z["p"].copy()
size = arg("--size", 0.05)
p[hit, 0] += size * np.cos(ang[hit]) * p[hit, 2]; p[hit, 1] += size * np.sin(ang[hit]) * p[hit, 2]

ctx = xmamd.Context(obs=(cam, lm, p, w))
R, s, info = ctx.solve(5, 1e-10, 0.0)
rot, scale, _ = xmamd.recover_rotations(R, s)
t, P = ctx.recover_tp(rot, scale)
print(f"XM solve on {cam.size} observations, {int(hit.sum())} of them displaced by {size}: rank {info['rank']}, status {info['status']}, "
      f"rotation error {rotation_error(rot, gt, fi):.4e}")
rot_b, t_b, P_b, b = ctx.bundle_adjust(rot, t, P)
print(f"plain bundle_adjust: cost {b['initial_cost']:.6e} -> {b['final_cost']:.6e} ({b['iters']} LM iterations, {b['status_name']}), "
      f"rotation error {rotation_error(rot_b, gt, fi):.4e}")
rot_f, t_f, P_f, f = ctx.refine_filtered(rot, t, P)
dropped = ~f["keep"]
for r in f["rounds"]:
    print(f"  round {r['ite']}: BA fixed rotations {r['ba_fixed']['initial_cost']:.6e} -> {r['ba_fixed']['final_cost']:.6e}, full "
          f"{r['ba_full']['initial_cost']:.6e} -> {r['ba_full']['final_cost']:.6e}; filters "
          + ", ".join(f"{q['scaling']}x: {q['dropped']} observations / {q['tracks_changed']} of {q['tracks_total']} tracks" for q in r["filters"]))
print("  closing filters: " + ", ".join(f"{'reprojection' if q['reprojection'] is not None else 'triangulation'}: {q['dropped']} observations"
                                        for q in f["final"]))
print(f"refine_filtered: removed {int(dropped.sum())} observations, {int((dropped & hit).sum())} of the {int(hit.sum())} displaced ones "
      f"({100.0 * (dropped & hit).sum() / max(1, hit.sum()):.1f} %), rotation error {rotation_error(rot_f, gt, fi):.4e}"
      f"{' (stopped by the 0.1 % rule)' if f['stopped_early'] else ''}")
ctx.close()
