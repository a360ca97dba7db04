#!/usr/bin/env python3
"""The reference's own filter -> checklandmarks -> create_matrix -> solve (5_test_ceres.py:316-431, :482, :520-560) on the device, for
assets/SIMPLE2:

    reference:  for (i, j) in itertools.combinations(range(N), 2): ...      one Python pass per camera pair with a relative rotation:
                    trim_mean x 10, np.percentile x 3, error_sum[i, ...] += 1  dense rows of length M, a dense N x M error_sum
                edges = edges[~is_outlier]; ...                              rows that any pair flagged are deleted
                checklandmarks(edges, ...)                                   networkx on the host
                create_matrix(...); XM.solve(...)
    here:       plan = xmamd.pair_filter(cam, lm, p, pairs_i, pairs_j, R)    xm_pair_filter: one workgroup per pair
                cam, lm, p, w = plan.apply(cam, lm, p, w)
                clean = xmamd.clean_observations(cam, lm, w)                 xm_clean_observations
                xmamd.Context(obs=clean.apply(cam, lm, p, w)).solve(...)

The observation list is the one the reference's pipeline hands on (tests/golden/simple2/obs.npz).  The front end's pairwise rotations are
not part of the repository: the relative rotations come from the committed ground truth (gtR.bin), and 3 % of the camera-frame points are
scaled by 1 + 0.3 N(0, 1) so that there is something to find.  Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
import numpy as np            # noqa: E402
import xmamd                  # noqa: E402

G = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(G, "obs.npz"))
cam, lm, p, w = Z["cam"], Z["lm"], Z["p"].copy(), Z["w"].reshape(-1)
n = int(cam.max()) + 1

rng = np.random.default_rng(0)
bad = rng.random(cam.size) < 0.03
p[bad] *= (1.0 + 0.3 * rng.standard_normal(int(bad.sum())))[:, None]

with open(os.path.join(G, "gtR.bin"), "rb") as f:                # int32 rows, int32 columns, float64 column-major
    rows, cols = (int(x) for x in np.fromfile(f, dtype="<i4", count=2))
    gt = np.fromfile(f, dtype="<f8", count=rows * cols).reshape((rows, cols), order="F")
fi = np.load(os.path.join(G, "frame_index.npy"))                 # camera index -> frame of the ground truth
Gc = np.stack([gt[:, 3 * fi[c]:3 * fi[c] + 3] for c in range(n)])
pairs_i, pairs_j = np.triu_indices(n, 1)
R = np.einsum("kab,kcb->kac", Gc[pairs_j], Gc[pairs_i])          # p_j ~ scale * (G_j G_i^T) p_i + t

plan = xmamd.pair_filter(cam, lm, p, pairs_i, pairs_j, R)
i = plan.info
used = plan.stats["status"] == xmamd.PAIR_USED
print(f"pair filter: {pairs_i.size} pairs, {i['pairs_used']} used ({i['pairs_skipped']} share fewer than 20 landmarks), largest joint set {i['max_joint']}; "
      f"median of the pairs' median residual {np.median(plan.stats['median'][used]):.4f}; {i['nobs_flagged']} of {cam.size} observations flagged, "
      f"{int((plan.outlier & bad).sum())} of the {int(bad.sum())} perturbed ones among them; "
      f"{1e3 * (i['seconds_index'] + i['seconds_kernels'] + i['seconds_download']):.2f} ms ({1e3 * i['seconds_kernels']:.2f} ms of kernels)")

cam, lm, p, w = plan.apply(cam, lm, p, w)
clean = xmamd.clean_observations(cam, lm, w, n)                  # thresholds 10 and 1: checklandmarks
print(f"cleaning: {clean.info['nobs_new']} of {cam.size} observations, {clean.info['n_new']} cameras and {clean.info['m_new']} landmarks stay, "
      f"{clean.info['components']} component(s)")
cam, lm, p, w = clean.apply(cam, lm, p, w)

ctx = xmamd.Context(obs=(cam, lm, p, w))
Rs, s, info = ctx.solve(5, 1e-6, 0.0)
ctx.close()
print(f"solve on {cam.size} observations: rank {info['rank']}, status {info['status']}, primal {info['primal']:.6e}")
