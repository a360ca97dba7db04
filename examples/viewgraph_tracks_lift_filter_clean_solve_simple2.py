#!/usr/bin/env python3
"""The reference's pipeline from COLMAP's two-view geometries to the recovered rotations, every stage on the device:

    reference:  GLOMAP scores every match against its pair's geometry, drops pairs by inlier number and ratio, keeps the largest connected
                component, averages rotations, drops pairs whose relative rotation disagrees, prunes again       global_mapper.cc:56-111
                then track establishment, 5_test_ceres.py, ...
    here:       A = xmamd.view_graph_filter(foff, xy, pi, pj, model, matches, focal=, Kinv=, Rrel=, trel=, FH=, valid_in=)        pass A
                ctx = xmamd.Context(vg=(pi, pj, 1, Rrel^T)) over A.pairs(); ctx.solve; xmamd.recover_rotations   rotation averaging, certified
                B = xmamd.view_graph_filter(..., A.matches, valid_in=A.valid, registered_in=A.registered, rot=, score=False)      pass B
                t = xmamd.build_tracks(foff, xy, pi, pj, B.matches, registered=B.registered)
                lift_observations, pair_filter over B.pairs(), clean_observations, Context(obs=...), solve, recover

The scene is the recorded case of tests/xm_viewgraph_numpy.py (simple2_case): the features, pixels, cameras and matches of
tracks_lift_filter_clean_solve_simple2.py, relative poses from tests/golden/simple2/tp.npz, some of them spoiled with a seed.  The view-graph
solve's model is Y_i = M_e Y_j; with M_e = Rrel_e^T its blocks are Y_i = C_i G (C: cam_from_world), recover_rotations returns C_0 C_i^T, and
cam_from_world is the transpose of a recovered block (tests/test_gpu_viewgraph.py checks this with planted rotations).  Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np               # noqa: E402
import xmamd                     # noqa: E402
import xm_viewgraph_numpy as vn  # noqa: E402

c = vn.simple2_case()
n = c["foff"].size - 1
args, kw = vn.call_args(c)
ms = lambda i: 1e3 * (i["seconds_index"] + i["seconds_kernels"] + i["seconds_download"])


def report(what, g):
    i = g.info
    print(f"{what}: {i['matches']} matches, {i['inliers']} inliers; pairs: {i['pairs_valid']} valid, {i['pairs_invalid_in']} invalid at input, "
          f"{i['pairs_few_inliers']} few inliers, {i['pairs_low_ratio']} low ratio, {i['pairs_rotation']} rotation, {i['pairs_outside']} outside; "
          f"{i['largest']} of {n} images registered ({i['components']} components); {i['matches_out']} matches written; {ms(i):.2f} ms "
          f"({1e3 * i['seconds_kernels']:.2f} ms of kernels)")


A = xmamd.view_graph_filter(*args, **kw)
report("pass A", A)

# rotation averaging over the surviving pairs, on the registered images
img = np.flatnonzero(A.registered)
index = np.full(n, -1, dtype=np.int32); index[img] = np.arange(img.size, dtype=np.int32)
vi, vj, vR = A.pairs()
ctx = xmamd.Context(vg=(index[vi], index[vj], np.ones(vi.size), np.ascontiguousarray(np.transpose(vR, (0, 2, 1)))), n=img.size)
Rs, s, info = ctx.solve(5, 1e-8, 20.0)
rot, scale, _ = xmamd.recover_rotations(Rs, s)
ctx.close()
cam_from_world = np.tile(np.eye(3), (n, 1, 1))
cam_from_world[img] = np.stack([rot[:, 3 * k:3 * k + 3].T for k in range(img.size)])
cs = vn.rotation_cosine(cam_from_world[vi], cam_from_world[vj], vR)
print(f"view-graph solve over {vi.size} pairs of {img.size} images: rank {info['rank']}, status {info['status']}; "
      f"{int(np.sum(cs < np.cos(np.radians(10.0))))} pairs disagree with it by more than 10 degrees")

kw_b = dict(kw, valid_in=A.valid, registered_in=A.registered, rot=cam_from_world, score=False)
B = xmamd.view_graph_filter(c["foff"], c["xy"], c["pi"], c["pj"], c["model"], A.matches, **kw_b)
report("pass B", B)
print("images that left the largest component in pass B:", np.flatnonzero((A.registered != 0) & (B.registered == 0)).tolist(), "(planted:", sorted(c["gone"].tolist()), ")")

t = xmamd.build_tracks(c["foff"], c["xy"], c["pi"], c["pj"], B.matches, registered=B.registered)
i = t.info
print(f"tracks: {i['matches']} matches over {i['features_touched']} features -> {i['components']} components, {i['components_conflicted']} conflicted; "
      f"{t.m} tracks, {t.cam.size} rows")

# the depth and confidence maps, rendered from the observation list as in lift_filter_clean_solve_simple2.py
Z = np.load(os.path.join(ROOT, "tests", "golden", "simple2", "obs.npz"))
cam, lm, p, w = Z["cam"].astype(np.int32), Z["lm"].astype(np.int32), Z["p"], Z["w"].reshape(-1)
order = np.lexsort((lm, cam))
K = np.linalg.inv(c["Kinv"])
depth, conf = [], []
for k in range(n):
    e = order[c["foff"][k]:c["foff"][k + 1]]
    D = np.zeros((vn.H_IMG, vn.W_IMG), dtype=np.float32); Cf = np.zeros((vn.H_IMG, vn.W_IMG), dtype=np.float32)
    x = c["xy"][c["foff"][k]:c["foff"][k + 1]]
    u, v = x[:, 0].astype(int), x[:, 1].astype(int)
    ok = (p[e, 2] > 0) & (x[:, 0] >= 0) & (u < vn.W_IMG) & (x[:, 1] >= 0) & (v < vn.H_IMG)
    D[v[ok], u[ok]] = p[e[ok], 2]; Cf[v[ok], u[ok]] = np.sqrt(w[e[ok]])
    depth.append((xmamd.DevArray(D), vn.H_IMG, vn.W_IMG)); conf.append((xmamd.DevArray(Cf), vn.H_IMG, vn.W_IMG))
lift = xmamd.lift_observations(t.cam, t.track, t.xy, depth, conf, K, n=n, m=t.m)
li = lift.info
print(f"lift: {t.cam.size} rows -> {lift.cam.size} observations ({li['rows_duplicate']} duplicate, {li['rows_border']} border, {li['rows_depth']} depth)")
fi_, fj_, fR = B.pairs()
plan = xmamd.pair_filter(lift.cam, lift.lm, lift.p, fi_, fj_, fR, n=n, m=t.m)
c1, l1, p1, w1 = plan.apply(lift.cam, lift.lm, lift.p, lift.w)
clean = xmamd.clean_observations(c1, l1, w1, n, t.m)
c2, l2, p2, w2 = clean.apply(c1, l1, p1, w1)
print(f"pair filter: {plan.info['pairs_used']} of {fi_.size} pairs used, {plan.info['nobs_flagged']} observations flagged; cleaning: "
      f"{clean.info['nobs_new']} of {c1.size} observations, {clean.info['n_new']} cameras and {clean.info['m_new']} landmarks stay")
ctx = xmamd.Context(obs=(c2, l2, p2, w2))
Rs, s, info = ctx.solve(5, 1e-8, 0.0)
rot, scale, _ = xmamd.recover_rotations(Rs, s)
ctx.close()
# camera -> world rotations against the cam_from_world rotations the relative poses were made from, up to one global rotation
kept = np.flatnonzero(clean.cam_index >= 0)
Rc = np.stack([rot[:, 3 * clean.cam_index[k]:3 * clean.cam_index[k] + 3] for k in kept])
Gc = c["rot_true"][kept]
U, _, Vt = np.linalg.svd(np.einsum("cab,cbd->ad", Rc, Gc))
Aa = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
ang = np.degrees(np.arccos(np.clip((np.einsum("cba,bd,cad->c", Rc, Aa, Gc) - 1.0) / 2.0, -1.0, 1.0)))
print(f"solve on {c2.size} observations: rank {info['rank']}, status {info['status']}, primal {info['primal']:.6e}; rotation error against the rotations of "
      f"tp.npz: median {np.median(ang):.3f} deg, largest {ang.max():.3f} deg over {kept.size} cameras")
