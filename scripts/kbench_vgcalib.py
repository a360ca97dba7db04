#!/usr/bin/env python3
"""What xmamd.view_graph_calibrate costs: the whole call with the host index, the kernels and the download split out (the best of --reps
calls), the iteration counts, and the numpy contract (tests/xm_vgcalib_numpy.py: calibrate_contract) on the same node.  Sizes: the
SIMPLE2-derived case (93 images, 4182 participating pairs, one camera per image); 2 000 images with 2.0 M pairs (every pair of images but a
few), one camera per image, where the contract's set-up is a Python loop over the pairs and takes minutes: --no-contract leaves it out.
   python scripts/kbench_vgcalib.py [--small-only] [--no-contract] [--reps 3] [--out profiles/...txt]
Needs an MI355X."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import xmamd
import xm_vgcalib_numpy as vc


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path = arg("--out", "")
reps = arg("--reps", 3)
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def large(n=2000, npairs=2000000, seed=1):
    """n images, one camera each, npairs pairs, F = K_j^-T [t]x R K_i^-1 from random poses, vectorised"""
    rng = np.random.default_rng(seed)
    truth = rng.uniform(600.0, 1500.0, n)
    pp = np.stack([rng.uniform(450.0, 550.0, n), rng.uniform(350.0, 450.0, n)], axis=1)
    q = rng.standard_normal((n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    cw = rng.standard_normal((n, 3)) * 3.0
    iu, ju = np.triu_indices(n, 1)
    sel = np.sort(rng.permutation(iu.size)[:npairs])
    pi, pj = iu[sel].astype(np.int32), ju[sel].astype(np.int32)
    Rrel = np.einsum("kab,kcb->kac", R[pj], R[pi])
    t = np.einsum("kab,kb->ka", R[pj], cw[pi] - cw[pj]); t /= np.linalg.norm(t, axis=1, keepdims=True)
    T = np.zeros((pi.size, 3, 3))
    T[:, 0, 1], T[:, 0, 2], T[:, 1, 0], T[:, 1, 2], T[:, 2, 0], T[:, 2, 1] = -t[:, 2], t[:, 1], t[:, 2], -t[:, 0], -t[:, 1], t[:, 0]
    Kinv = np.zeros((n, 3, 3)); Kinv[:, 0, 0] = Kinv[:, 1, 1] = 1.0 / truth; Kinv[:, 2, 2] = 1.0
    Kinv[:, 0, 2] = -pp[:, 0] / truth; Kinv[:, 1, 2] = -pp[:, 1] / truth
    F = np.einsum("kba,kbc,kcd->kad", Kinv[pj], T @ Rrel, Kinv[pi])
    F /= np.linalg.norm(F.reshape(-1, 9), axis=1)[:, None, None]
    return dict(focal0=truth * rng.uniform(0.7, 1.4, n), pp=pp, has_prior=np.zeros(n, dtype=np.uint8), cam_of_image=np.arange(n, dtype=np.int32), pi=pi, pj=pj,
                model=np.full(pi.size, vc.MODEL_F, dtype=np.int32), F=F, valid_in=None, truth=truth)


def bench(what, g, contract):
    best = None
    for _ in range(reps + 1):                      # the first call loads the code objects
        t0 = time.perf_counter()
        r = xmamd.view_graph_calibrate(**vc.call_inputs(g))
        wall = time.perf_counter() - t0
        if best is None or wall < best[0]:
            best = (wall, r.info)
    wall, i = best
    log(f"{what}: {i['pairs']} pairs, {i['cams_free']} free cameras, {i['cams_heavy']} heavy, most incidences {i['max_incidences']}; "
        f"{i['iterations']} LM iterations, {i['pcg_iterations']} PCG iterations, stop: {i['stop']}, cost {i['initial_cost']:.3e} -> {i['final_cost']:.3e}, "
        f"relative focal error {np.max(np.abs(r.focal_est - g['truth']) / g['truth']):.2e}")
    log(f"{what}: call {1e3 * wall:.2f} ms wall (with the binding's copies): host index and upload {1e3 * i['seconds_index']:.2f} ms, kernels "
        f"{1e3 * i['seconds_kernels']:.2f} ms, download {1e3 * i['seconds_download']:.2f} ms")
    if contract:
        t0 = time.perf_counter()
        b = vc.calibrate_contract(g)
        log(f"{what}: numpy contract {1e3 * (time.perf_counter() - t0):.1f} ms ({b['iterations']} LM iterations, {b['pcg_iterations']} PCG iterations)")


xmamd.require_gpu()
g, _ = vc.simple2_case()
bench("SIMPLE2-derived", g, "--no-contract" not in sys.argv)
if "--small-only" not in sys.argv:
    t0 = time.perf_counter()
    G = large()
    log(f"2 000 images: generated in {time.perf_counter() - t0:.1f} s")
    bench("2 000 images, 2.0 M pairs", G, "--no-contract" not in sys.argv)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
