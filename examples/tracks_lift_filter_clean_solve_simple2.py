#!/usr/bin/env python3
"""The reference's last pipeline from COLMAP's verified two-view matches to the recovered rotations, every stage on the device:

    reference:  GLOMAP's track establishment (its fork: track_establishment.cc, union_find.h), one thread over hash maps, writes
                    assets/tempdata/output.txt                                       global_mapper.cc:113-156
                5_test_ceres.py reads it back, de-duplicates, lifts, filters, cleans, builds Q, solves, recovers
    here:       t = xmamd.build_tracks(foff, xy, pi, pj, (moff, f1, f2))          xm_build_tracks: the match table on the device
                lift = xmamd.lift_observations(t.cam, t.track, t.xy, depth, conf, K, n=n, m=t.m)
                plan = xmamd.pair_filter(...); clean = xmamd.clean_observations(...); ctx = xmamd.Context(obs=...); ctx.solve(...)

Neither images, a COLMAP database nor a depth network are part of the repository.  The features are the observations of the list the
reference's pipeline hands on for assets/SIMPLE2 (tests/golden/simple2/obs.npz), ordered by (camera, landmark), at the pixel their point
projects to; the matches are generated from them (tests/xm_tracks_numpy.py, simple2_case: every co-visible pair of a landmark's features
with probability 0.6, 0.1 % wrong matches); the maps are rendered as in lift_filter_clean_solve_simple2.py.  The same downstream stages
run a second time from the TRUE tracks (the landmark numbers of obs.npz), which is the figure lift_filter_clean_solve_simple2.py prints
without its duplicated rows, so the two rotation errors stand next to each other.  Needs an MI355X.
    --split-device   the conflicted components are split on the device (conflict="split_device", XM_TRACKS_SPLIT_DEVICE) instead of on the
                     host: the same tracks bit for bit, so every number printed is the one of the plain run; only the times differ"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np            # noqa: E402
import xmamd                  # noqa: E402
import xm_tracks_numpy as tn  # noqa: E402

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

with open(os.path.join(G, "gtR.bin"), "rb") as f:                # int32 rows, int32 columns, float64 column-major
    rows, cols = (int(x) for x in np.fromfile(f, dtype="<i4", count=2))
    gt = np.fromfile(f, dtype="<f8", count=rows * cols).reshape((rows, cols), order="F")
fi = np.load(os.path.join(G, "frame_index.npy"))                 # camera index -> frame of the ground truth
Gc = np.stack([gt[:, 3 * fi[c]:3 * fi[c] + 3] for c in range(n)])
pairs_i, pairs_j = np.triu_indices(n, 1)
R = np.einsum("kab,kcb->kac", Gc[pairs_j], Gc[pairs_i])          # p_j ~ scale * (G_j G_i^T) p_i + t


def downstream(what, ocam, otrack, oxy, mm):
    lift = xmamd.lift_observations(ocam, otrack, oxy, depth, conf, K, n=n, m=mm)
    i = lift.info
    print(f"{what}: lift: {ocam.size} rows -> {lift.cam.size} observations ({i['rows_duplicate']} duplicate, {i['rows_border']} border, {i['rows_depth']} depth)")
    plan = xmamd.pair_filter(lift.cam, lift.lm, lift.p, pairs_i, pairs_j, R, n=n, m=mm)
    c1, l1, p1, w1 = plan.apply(lift.cam, lift.lm, lift.p, lift.w)
    clean = xmamd.clean_observations(c1, l1, w1, n, mm)               # thresholds 10 and 1: checklandmarks
    c2, l2, p2, w2 = clean.apply(c1, l1, p1, w1)
    print(f"{what}: pair filter: {plan.info['pairs_used']} of {pairs_i.size} pairs used, {plan.info['nobs_flagged']} observations flagged; cleaning: "
          f"{clean.info['nobs_new']} of {c1.size} observations, {clean.info['n_new']} cameras and {clean.info['m_new']} landmarks stay")
    ctx = xmamd.Context(obs=(c2, l2, p2, w2))
    Rs, s, info = ctx.solve(5, 1e-8, 0.0)
    rot, scale, _ = xmamd.recover_rotations(Rs, s)
    ctx.recover_tp(rot, scale)
    ctx.close()
    # camera -> world rotations against the ground truth's world -> camera ones, up to one global rotation (the chordal mean of R_c G_c)
    kept = np.flatnonzero(clean.cam_index >= 0)
    Rc = np.stack([rot[:, 3 * clean.cam_index[c]:3 * clean.cam_index[c] + 3] for c in kept])
    U, _, Vt = np.linalg.svd(np.einsum("cab,cbd->ad", Rc, Gc[kept]))
    A = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    cosang = (np.einsum("cba,bd,cad->c", Rc, A, Gc[kept]) - 1.0) / 2.0     # trace(R_c^T A G_c^T)
    ang = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0)))
    print(f"{what}: solve on {c2.size} observations: rank {info['rank']}, status {info['status']}, primal {info['primal']:.6e}; rotation error against "
          f"gtR.bin: median {np.median(ang):.3f} deg, largest {ang.max():.3f} deg over {kept.size} cameras")


# the features in (camera, landmark) order, the generated matches over them
order = np.lexsort((lm, cam))
case = tn.simple2_case()
assert case["foff"][-1] == cam.size
fxy = xy[order]
SPLIT = "split_device" if "--split-device" in sys.argv[1:] else "split"
for policy in (SPLIT, "drop", "glomap"):
    t = xmamd.build_tracks(case["foff"], fxy, case["pi"], case["pj"], (case["moff"], case["f1"], case["f2"]), conflict=policy)
    i = t.info
    # how the tracks sit on the true landmarks: a track is pure when all its rows carry one landmark
    true_lm = lm[order][t.feature]
    o = np.lexsort((true_lm, t.track))
    mixed = np.unique(t.track[o][1:][(t.track[o][1:] == t.track[o][:-1]) & (true_lm[o][1:] != true_lm[o][:-1])]).size
    print(f"tracks ({policy}): {i['matches']} matches over {i['features_touched']} of {cam.size} features -> {i['components']} components, "
          f"{i['components_conflicted']} conflicted ({i['rows_conflicted']} features, {i['edges_split']} edges split on the {'device' if policy == 'split_device' else 'host'}, {i['unions_refused']} unions refused); "
          f"{t.m} tracks, {t.cam.size} rows, {mixed} tracks mix landmarks; dropped: {i['tracks_short']} short, {i['tracks_conflict']} by the policy; "
          f"{i['rounds']} hooking rounds, images by kernel size {i['images_small']} / {i['images_large']} / {i['images_workspace']}; "
          f"{1e3 * (i['seconds_index'] + i['seconds_kernels'] + i['seconds_split'] + i['seconds_download']):.2f} ms "
          f"({1e3 * i['seconds_kernels']:.2f} ms of kernels, {1e3 * i['seconds_split']:.2f} ms {'device' if policy == 'split_device' else 'host'} split)")
    if policy == SPLIT:
        table = t
downstream(f"from the matches ({SPLIT})", table.cam, table.track, table.xy, table.m)
downstream("from the true tracks", cam[order], lm[order], fxy, m)
