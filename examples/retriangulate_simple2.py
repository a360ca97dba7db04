#!/usr/bin/env python3
"""GLOMAP's retriangulation step (controllers/global_mapper.cc:322-375) on the GPU, behind the alternation of bundle adjustment and track
filtering, on the SIMPLE2 observation list with a seeded share of its observed points displaced:

    ctx = xmamd.Context(obs=(cam, lm, p, w))                                     (XM_STORAGE_SCHUR)
    R, s, info = ctx.solve(5, tol, lam);  rot, scale, _ = xmamd.recover_rotations(R, s);  t, P = ctx.recover_tp(rot, scale)
    rot, t, P, f = ctx.refine_filtered(rot, t, P)                                 (BA and filter, repeated: only removes observations)
    rot, t, P, r = ctx.retriangulate(rot, t, P, weights=w)                        (triangulate at the refined poses with every observation
                                                                                   of the list a candidate again, BA, filter, BA, filters)

Printed: the observations refine_filtered dropped, those the triangulation re-admitted, the displaced ones that are kept at the end, and
the median rotation error against the recorded ground truth gtR.bin before and after.

    python examples/retriangulate_simple2.py [--share 0.05] [--size 0.05] [--seed 0] [--rounds 1]

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
rot, t, P, f = ctx.refine_filtered(rot, t, P)
kept_f = f["keep"]
print(f"refine_filtered: dropped {int((~kept_f).sum())} observations ({int((~kept_f & hit).sum())} of the {int(hit.sum())} displaced ones, "
      f"{int((~kept_f & ~hit).sum())} clean ones), rotation error {rotation_error(rot, gt, fi):.4e}")
plan = ctx.triangulate_tracks(rot, t, P, candidates=w > 0)
print(f"triangulate_tracks at the refined poses, every observation a candidate: {plan.info['lm_accepted']} of {plan.P.shape[1]} landmarks accepted, "
      f"{plan.info['obs_kept']} observations kept, {plan.info['obs_readmitted']} re-admitted ({int((plan.keep & ~kept_f & hit).sum())} of them displaced), "
      f"{plan.info['obs_lost']} lost; {plan.info['hypotheses_scored']} hypotheses scored of {plan.info['pairs_tested']} pairs tested; "
      f"{(plan.info['seconds_kernels'] + plan.info['seconds_download']) * 1e3:.2f} ms")
acc = plan.status == xmamd.TRI_LM_ACCEPTED
rel = np.linalg.norm(plan.P[:, acc] - P[:, acc], axis=0) / np.linalg.norm(P[:, acc], axis=0)
print(f"  median relative distance of the triangulated points from the adjusted ones: {float(np.median(rel)):.2e}")
rot, t, P, r = ctx.retriangulate(rot, t, P, rounds=arg("--rounds", 1), weights=w)
for q in r["rounds"]:
    print(f"  round {q['ite']}: re-admitted {q['triangulation']['obs_readmitted']}, lost {q['triangulation']['obs_lost']}; BA "
          f"{q['ba_first']['initial_cost']:.6e} -> {q['ba_first']['final_cost']:.6e}; filter dropped {q['filter']['dropped']}; BA "
          f"{q['ba_second']['initial_cost']:.6e} -> {q['ba_second']['final_cost']:.6e}")
print("  closing filters: " + ", ".join(f"{'reprojection' if q['reprojection'] is not None else 'triangulation'}: {q['dropped']} observations"
                                        for q in r["final"]))
keep = r["keep"]
print(f"retriangulate: ends with {int(keep.sum())} observations ({int((keep & ~kept_f).sum())} that refine_filtered had dropped, "
      f"{int((kept_f & ~keep).sum())} fewer of those it had kept); displaced and kept {int((keep & hit).sum())} of {int(hit.sum())}; clean and out "
      f"{int((~keep & ~hit).sum())} of {int((~hit).sum())}; rotation error {rotation_error(rot, gt, fi):.4e}")
ctx.close()
