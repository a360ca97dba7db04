#!/usr/bin/env python3
"""The loop of examples/refine_filter_simple2.py, then GLOMAP's step 8, PruneWeaklyConnectedImages (processors/reconstruction_pruning.cc), on
the GPU, on the SIMPLE2 observation list:

    ctx = xmamd.Context(obs=(cam, lm, p, w))                                     (XM_STORAGE_SCHUR)
    R, s, info = ctx.solve(5, tol, lam);  rot, scale, _ = xmamd.recover_rotations(R, s);  t, P = ctx.recover_tp(rot, scale)
    rot, t, P, info = ctx.refine_filtered(rot, t, P, prune=True)                  (BA, filters, then the covisibility clusters)
    plan = info["prune"]                                                          (cluster_id per camera: 0 stays, -1 is pruned)
    clean = xmamd.clean_observations(cam, lm, w=info["weights"], min_cam_obs=0)   (the next context's list without the pruned cameras)

--thin K leaves the last K cameras with their first 4 observations only (the others get weight 0), so that the output shows pruned
images; without it the recorded case is one cluster of all 93 cameras.

    python examples/refine_filter_prune_simple2.py [--thin 5] [--min-obs 0]

Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
import numpy as np            # noqa: E402
import xmamd                  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


Z = np.load(os.path.join(ROOT, "tests", "golden", "simple2", "obs.npz"))
cam, lm, p = Z["cam"], Z["lm"], Z["p"]
n = int(cam.max()) + 1
w = np.ones(cam.size)
thin = arg("--thin", 0)
for c in range(n - thin, n):
    w[np.flatnonzero(cam == c)[4:]] = 0.0

ctx = xmamd.Context(obs=(cam, lm, p, np.ones(cam.size)))
R, s, info = ctx.solve(5, 1e-10, 0.0)
rot, scale, _ = xmamd.recover_rotations(R, s)
t, P = ctx.recover_tp(rot, scale)
print(f"XM solve on {cam.size} observations of {n} cameras: rank {info['rank']}, status {info['status']}")
if thin:
    ctx.set_edge_weights(w)
    print(f"the last {thin} cameras keep 4 observations each: {int((w > 0).sum())} observations used")
rot, t, P, f = ctx.refine_filtered(rot, t, P, weights=w, prune=True)
for r in f["rounds"]:
    print(f"  round {r['ite']}: BA fixed rotations {r['ba_fixed']['initial_cost']:.6e} -> {r['ba_fixed']['final_cost']:.6e}, full "
          f"{r['ba_full']['initial_cost']:.6e} -> {r['ba_full']['final_cost']:.6e}; filters "
          + ", ".join(f"{q['scaling']}x: {q['dropped']} observations" for q in r["filters"]))
plan = f["prune"]
i = plan.info
print(f"pruning: {i['pairs_covisible']} pairs with 5 or more common landmarks, {i['n_edges']} edges; median {i['median']:.0f}, MAD {i['mad']:.0f}, "
      f"threshold {i['threshold']:.0f}; largest component {i['component_images']} images in {i['strong_clusters']} strong clusters, "
      f"{i['rounds']} merge round(s) over {i['weak_edges']} edges; {i['n_clusters']} cluster(s) with {i['images_clustered']} images "
      f"({i['seconds_kernels'] * 1e3:.2f} ms)")
pruned = np.flatnonzero(plan.cluster_id != 0)
print(f"pruned images: {pruned.tolist() if pruned.size else 'none'}" + (f" with {plan.obs_count[pruned].tolist()} observations" if pruned.size else ""))
if arg("--min-obs", 0):
    q = ctx.prune_weakly_connected(min_num_observations=arg("--min-obs", 0))
    print(f"with min_num_observations = {arg('--min-obs', 0)}: {q.info['n_edges']} edges, threshold {q.info['threshold']:.0f}, "
          f"{int((q.cluster_id == 0).sum())} images in cluster 0, pruned {np.flatnonzero(q.cluster_id != 0).tolist()}")
clean = xmamd.clean_observations(cam, lm, w=f["weights"], n=n, min_cam_obs=0, min_lm_obs=1)
print(f"the next context's list: {clean.info['n_new']} cameras, {clean.info['m_new']} landmarks, {clean.info['nobs_new']} observations")
ctx.close()
