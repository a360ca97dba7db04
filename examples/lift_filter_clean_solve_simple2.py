#!/usr/bin/env python3
"""The reference's last pipeline (5_test_ceres.py) from the depth network's output to the recovered rotations, every stage on the device:

    reference:  matches = matches[unique rows of (camera, track)]               :191-204, host
                for i in range(N): depth.cpu().numpy(), confidence.cpu().numpy()  every H x W map to the host; margin, np.percentile,
                    K^-1 (u, v, 1) d, w ** 2                                       :244-296, one Python pass per camera
                the pairwise filter, checklandmarks, create_matrix, XM.solve, recover_XM
    here:       lift = xmamd.lift_observations(cam, lm, xy, depth, conf, K)     xm_lift_observations: the maps stay where they are
                plan = xmamd.pair_filter(lift.cam, lift.lm, lift.p, ...)        xm_pair_filter
                clean = xmamd.clean_observations(...)                           xm_clean_observations
                ctx = xmamd.Context(obs=clean.apply(...)); ctx.solve(...); xmamd.recover_rotations(...); ctx.recover_tp(...)

Neither images nor a depth network are part of the repository, so the maps are RENDERED: every observation of the list the reference's
pipeline hands on for assets/SIMPLE2 (tests/golden/simple2/obs.npz: camera-frame point and weight) is projected through a pinhole K into
its camera's 768 x 1024 depth map (the point's z) and confidence map (the root of its weight); the match table holds the projected pixel
positions, and 2 % of the rows are listed twice.  The maps are uploaded once, as a network would leave them, and the lift reads them on the
device.  What it returns differs from obs.npz by the pixel quantisation (the reference back-projects the integer pixel), by the border and
the depth percentile, and where two tracks fall on one pixel.  The relative rotations of the pair filter come from the committed ground
truth (gtR.bin).  Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
import numpy as np            # noqa: E402
import xmamd                  # noqa: E402

G = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(G, "obs.npz"))
cam, lm, p, w = Z["cam"].astype(np.int32), Z["lm"].astype(np.int32), Z["p"], Z["w"].reshape(-1)
n, m = int(cam.max()) + 1, int(lm.max()) + 1
H, W = 768, 1024

# a pinhole camera per view whose field of view holds nearly all of its points
K = np.zeros((n, 3, 3)); xy = np.zeros((cam.size, 2)); depth, conf = [], []
for c in range(n):
    e = np.flatnonzero(cam == c)
    q = p[e]
    front = q[:, 2] > 0
    tx, ty = np.abs(q[front, 0] / q[front, 2]), np.abs(q[front, 1] / q[front, 2])
    f = 0.95 * min((W / 2 - 12) / np.percentile(tx, 99), (H / 2 - 12) / np.percentile(ty, 99))
    K[c] = [[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]]
    z = np.where(front, q[:, 2], 1.0)
    xy[e, 0] = np.where(front, f * q[:, 0] / z + W / 2.0, -5.0); xy[e, 1] = np.where(front, f * q[:, 1] / z + H / 2.0, -5.0)
    D = np.zeros((H, W), dtype=np.float32); Cf = np.zeros((H, W), dtype=np.float32)
    u, v = xy[e, 0].astype(int), xy[e, 1].astype(int)
    ok = front & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    D[v[ok], u[ok]] = q[ok, 2]; Cf[v[ok], u[ok]] = np.sqrt(w[e][ok])
    depth.append((xmamd.DevArray(D), H, W)); conf.append((xmamd.DevArray(Cf), H, W))
rng = np.random.default_rng(0)
twice = rng.choice(cam.size, cam.size // 50, replace=False)
cam2, lm2, xy2 = np.concatenate([cam, cam[twice]]), np.concatenate([lm, lm[twice]]), np.concatenate([xy, xy[twice] + 3.0])

lift = xmamd.lift_observations(cam2, lm2, xy2, depth, conf, K, m=m)
i = lift.info
back = np.linalg.norm(lift.p - p[lift.row % cam.size], axis=1) / np.linalg.norm(p[lift.row % cam.size], axis=1)
print(f"lift: {cam2.size} rows -> {lift.cam.size} observations ({i['rows_duplicate']} duplicate, {i['rows_border']} border, {i['rows_depth']} depth), "
      f"cameras by kernel size {i['cams_small']} / {i['cams_large']} / {i['cams_workspace']}; median |p - p of obs.npz| / |p| {np.median(back):.2e}; "
      f"{1e3 * (i['seconds_index'] + i['seconds_kernels'] + i['seconds_download']):.2f} ms ({1e3 * i['seconds_kernels']:.2f} ms of kernels)")

with open(os.path.join(G, "gtR.bin"), "rb") as f:                # int32 rows, int32 columns, float64 column-major
    rows, cols = (int(x) for x in np.fromfile(f, dtype="<i4", count=2))
    gt = np.fromfile(f, dtype="<f8", count=rows * cols).reshape((rows, cols), order="F")
fi = np.load(os.path.join(G, "frame_index.npy"))                 # camera index -> frame of the ground truth
Gc = np.stack([gt[:, 3 * fi[c]:3 * fi[c] + 3] for c in range(n)])
pairs_i, pairs_j = np.triu_indices(n, 1)
R = np.einsum("kab,kcb->kac", Gc[pairs_j], Gc[pairs_i])          # p_j ~ scale * (G_j G_i^T) p_i + t
plan = xmamd.pair_filter(lift.cam, lift.lm, lift.p, pairs_i, pairs_j, R, n=n, m=m)
print(f"pair filter: {plan.info['pairs_used']} of {pairs_i.size} pairs used, {plan.info['nobs_flagged']} observations flagged")
c1, l1, p1, w1 = plan.apply(lift.cam, lift.lm, lift.p, lift.w)
clean = xmamd.clean_observations(c1, l1, w1, n, m)               # thresholds 10 and 1: checklandmarks
print(f"cleaning: {clean.info['nobs_new']} of {c1.size} observations, {clean.info['n_new']} cameras and {clean.info['m_new']} landmarks stay")
c2, l2, p2, w2 = clean.apply(c1, l1, p1, w1)

ctx = xmamd.Context(obs=(c2, l2, p2, w2))
Rs, s, info = ctx.solve(5, 1e-8, 0.0)
rot, scale, _ = xmamd.recover_rotations(Rs, s)
t, P = ctx.recover_tp(rot, scale)
ctx.close()
# camera -> world rotations against the ground truth's world -> camera ones, up to one global rotation (the chordal mean of R_c G_c)
kept = np.flatnonzero(clean.cam_index >= 0)
Rc = np.stack([rot[:, 3 * clean.cam_index[c]:3 * clean.cam_index[c] + 3] for c in kept])
U, _, Vt = np.linalg.svd(np.einsum("cab,cbd->ad", Rc, Gc[kept]))
A = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
cosang = (np.einsum("cba,bd,cad->c", Rc, A, Gc[kept]) - 1.0) / 2.0     # trace(R_c^T A G_c^T)
ang = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0)))
print(f"solve on {c2.size} observations: rank {info['rank']}, status {info['status']}, primal {info['primal']:.6e}; rotation error against gtR.bin: "
      f"median {np.median(ang):.3f} deg, largest {ang.max():.3f} deg over {kept.size} cameras")
