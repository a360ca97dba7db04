#!/usr/bin/env python3
"""The reference's solve -> XM^2 filter -> checklandmarks -> solve (5_test_ceres.py:482-600) on the device, for assets/SIMPLE2:

    reference:  checklandmarks(edges, ...)                 networkx on the host (before the first create_matrix and after the filter)
                create_matrix(...); XM.solve(...)          first solve
                error > np.percentile(error, 90) deleted   the XM^2 filter
                checklandmarks(edges, ...)                 drops what the filter left weakly observed or detached, renumbers
                create_matrix(...); XM.solve(...)          second solve
    here:       ctx = xmamd.Context(obs=(cam, lm, p, w));  R, s, info = ctx.solve(...)
                ctx.xm2_filter(rot, scale, 90)             weights of the outliers -> 0, on the device
                plan = ctx.clean_observations()            xm_ctx_clean_observations: the filtered list, no upload
                new list = plan.apply(cam, lm, p, w_new)   compacted and renumbered on the host
                xmamd.Context(obs=new list).solve(...)     second solve

The observation list is the one the reference's pipeline hands to create_matrix (tests/golden/simple2/obs.npz).  Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
import numpy as np            # noqa: E402
import xmamd                  # noqa: E402

Z = np.load(os.path.join(ROOT, "tests", "golden", "simple2", "obs.npz"))
cam, lm, p, w = Z["cam"], Z["lm"], Z["p"], Z["w"].reshape(-1)

first = xmamd.clean_observations(cam, lm, w)                     # before the first solve (a list from the reference's pipeline is clean already)
print(f"input list: {first.info['nobs_new']} of {cam.size} observations stay, {first.info['components']} component(s)")
cam, lm, p, w = first.apply(cam, lm, p, w)

ctx = xmamd.Context(obs=(cam, lm, p, w))
R, s, info = ctx.solve(5, 1e-6, 0.0)
rot, scale, _ = xmamd.recover_rotations(R, s)
thr, removed, w_new = ctx.xm2_filter(rot, scale, 90.0)
plan = ctx.clean_observations()                                  # thresholds 10 and 1: checklandmarks
ctx.close()
i = plan.info
live = w_new > 0
print(f"first solve: rank {info['rank']}, status {info['status']}, primal {info['primal']:.6e}; filter: threshold {thr:.3e}, {removed} removed")
print(f"cleaning the filtered list: {i['nobs_live'] - i['nobs_new']} more observations, {np.unique(cam[live]).size - i['n_new']} cameras and "
      f"{np.unique(lm[live]).size - i['m_new']} landmarks go ({i['rounds']} rounds, {i['components']} component(s)); camera {i['first_camera']} "
      f"becomes camera 0")

cam2, lm2, p2, w2 = plan.apply(cam, lm, p, w_new)
ctx2 = xmamd.Context(obs=(cam2, lm2, p2, w2))
R2, s2, info2 = ctx2.solve(5, 1e-6, 0.0)
ctx2.close()
print(f"second solve on {cam2.size} observations, {i['n_new']} cameras, {i['m_new']} landmarks: rank {info2['rank']}, status {info2['status']}, "
      f"primal {info2['primal']:.6e}")
