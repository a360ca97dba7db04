#!/usr/bin/env python3
"""What xmamd.view_graph_rotations costs: the whole call with the host index, the kernels and the download split out (the best of --reps
calls), the IRLS and PCG iteration counts, the numpy contract (tests/xm_rotavg_numpy.py: irls_contract) on the same node, and next to it one
pass-B call of xmamd.view_graph_filter and one view-graph solve of the same graph (whose rotations are the start).  Sizes: the
SIMPLE2-derived view graph after pass A (93 images, 2317 participating pairs); 2 000 images with all 1 999 000 pairs, 1 degree of noise, a
tenth of the pairs off the chain replaced by random rotations.  Last, the three median errors of examples/robust_rotations_simple2.py.
   python scripts/kbench_rotavg.py [--small-only] [--no-contract] [--reps 3] [--out profiles/...txt]
Needs an MI355X."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import xmamd
import xm_rotavg_numpy as rn


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path = arg("--out", "")
reps = arg("--reps", 3)
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def large(n=2000, seed=1, noise_deg=1.0, outliers=0.1):
    """n images and every pair of them, vectorised; the chain (i, i + 1) is kept clean"""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    iu, ju = np.triu_indices(n, 1)
    pi, pj = iu.astype(np.int32), ju.astype(np.int32)
    noise = rn.exp_batch(rng.standard_normal((pi.size, 3)) * np.radians(noise_deg) / np.sqrt(3.0))
    Rrel = rn.mul_batch(noise, np.einsum("kab,kcb->kac", R[pj], R[pi]))
    free = np.flatnonzero(pj != pi + 1)
    wrong = np.zeros(pi.size, dtype=bool); wrong[rng.choice(free, int(round(outliers * free.size)), replace=False)] = True
    k = np.flatnonzero(wrong)
    a = rng.standard_normal((k.size, 3)); a *= (rng.uniform(0.0, np.pi, k.size) / np.linalg.norm(a, axis=1))[:, None]
    Rrel[k] = rn.exp_batch(a)
    return dict(pi=pi, pj=pj, Rrel=np.ascontiguousarray(Rrel), truth=R, wrong=wrong, registered=None, valid_in=None)


def solve(n, registered, pi, pj, Rrel):
    """one view-graph solve over the given pairs -> cam_from_world (identity where unregistered), seconds"""
    img = np.flatnonzero(registered)
    index = np.full(n, -1, dtype=np.int32); index[img] = np.arange(img.size, dtype=np.int32)
    t0 = time.perf_counter()
    ctx = xmamd.Context(vg=(index[pi], index[pj], np.ones(pi.size), np.ascontiguousarray(np.transpose(Rrel, (0, 2, 1)))), n=img.size)
    Rs, s, info = ctx.solve(5, 1e-8, 20.0)
    rot, _, _ = xmamd.recover_rotations(Rs, s)
    ctx.close()
    sec = time.perf_counter() - t0
    cam_from_world = np.tile(np.eye(3), (n, 1, 1))
    cam_from_world[img] = np.stack([rot[:, 3 * k:3 * k + 3].T for k in range(img.size)])
    return cam_from_world, sec, info


def bench(what, g, pass_b, contract):
    best = None
    for _ in range(reps + 1):                      # the first call loads the code objects
        t0 = time.perf_counter()
        r = xmamd.view_graph_rotations(**rn.call_inputs(g))
        wall = time.perf_counter() - t0
        if best is None or wall < best[0]:
            best = (wall, r)
    wall, r = best
    i = r.info
    img = np.arange(g["rot0"].shape[0]) if g.get("registered") is None else np.flatnonzero(g["registered"])
    k = np.flatnonzero(r.weight > 0)
    log(f"{what}: {i['pairs']} pairs of {i['registered']} images, {i['cams_heavy']} heavy cameras, most incidences {i['max_incidences']}; "
        f"{i['irls_iterations']} IRLS iterations, {i['pcg_iterations']} PCG iterations ({i['pcg_capped']} capped), stop: {i['stop']}; median error against "
        f"the truth {np.median(rn.errors_deg(g['rot0'], g['truth'], img)):.4f} -> {np.median(rn.errors_deg(r.rot, g['truth'], img)):.4f} deg; "
        f"{int(np.sum(r.weight[k] < 1.0))} pairs with a weight below 1, {int(np.sum(r.weight[k] > 10.0))} above 10")
    log(f"{what}: call {1e3 * wall:.2f} ms wall (with the binding's copies): host index and upload {1e3 * i['seconds_index']:.2f} ms, kernels "
        f"{1e3 * i['seconds_kernels']:.2f} ms, download {1e3 * i['seconds_download']:.2f} ms")
    tb = min(pass_b(r.rot)[0] for _ in range(reps))
    log(f"{what}: one pass-B call of view_graph_filter with these rotations {1e3 * tb:.2f} ms wall; {pass_b(r.rot)[1]}")
    if contract:
        t0 = time.perf_counter()
        b = rn.irls_contract(g)
        log(f"{what}: numpy contract {1e3 * (time.perf_counter() - t0):.1f} ms ({b['iters']} IRLS iterations, {b['pcg_iters']} PCG iterations)")


xmamd.require_gpu()
contract = "--no-contract" not in sys.argv

# the SIMPLE2-derived view graph: pass A on the device, the view-graph solve as the start
import xm_viewgraph_numpy as vn
c = vn.simple2_case()
n = c["foff"].size - 1
args, kw = vn.call_args(c)
A = xmamd.view_graph_filter(*args, **kw)
vi, vj, vR = A.pairs()
rot0, sec, info = solve(n, A.registered, vi, vj, vR)
rot0, sec, info = solve(n, A.registered, vi, vj, vR)      # (the second call: code objects loaded)
log(f"SIMPLE2-derived: one view-graph solve over {vi.size} pairs {1e3 * sec:.2f} ms wall with the context (rank {info['rank']}, status {info['status']})")
g = dict(rot0=rot0, pi=c["pi"], pj=c["pj"], Rrel=c["Rrel"], truth=c["rot_true"], registered=A.registered, valid_in=A.valid)


def pass_b_simple2(rot):
    t0 = time.perf_counter()
    B = xmamd.view_graph_filter(c["foff"], c["xy"], c["pi"], c["pj"], c["model"], A.matches,
                                **dict(kw, valid_in=A.valid, registered_in=A.registered, rot=rot, score=False))
    return time.perf_counter() - t0, f"{B.info['pairs_rotation']} pairs dropped by the rotation test, {B.info['largest']} images stay"


bench("SIMPLE2-derived", g, pass_b_simple2, contract)

if "--small-only" not in sys.argv:
    t0 = time.perf_counter()
    G = large()
    N = G["truth"].shape[0]
    log(f"2 000 images: generated in {time.perf_counter() - t0:.1f} s")
    G["rot0"], sec, info = solve(N, np.ones(N, dtype=np.uint8), G["pi"], G["pj"], G["Rrel"])
    log(f"2 000 images, all pairs: one view-graph solve over {G['pi'].size} pairs {1e3 * sec:.1f} ms wall with the context (rank {info['rank']}, status {info['status']})")
    # pass B looks at rotations only: no feature, no match (N + 1 zeros are the feature offsets of N images)
    none = (np.zeros(N + 1, dtype=np.int64), np.zeros((0, 2)), (np.zeros(G["pi"].size + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)))

    def pass_b_large(rot):
        t0 = time.perf_counter()
        B = xmamd.view_graph_filter(none[0], none[1], G["pi"], G["pj"], np.zeros(G["pi"].size, dtype=np.int32), none[2], Rrel=G["Rrel"], rot=rot, score=False)
        return time.perf_counter() - t0, (f"{B.info['pairs_rotation']} pairs dropped by the rotation test ({int(G['wrong'].sum())} planted), "
                                          f"{B.info['largest']} images stay")

    bench("2 000 images, all pairs", G, pass_b_large, contract)

ex = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "robust_rotations_simple2.py")], capture_output=True, text=True, timeout=300)
if ex.returncode != 0:
    log(f"examples/robust_rotations_simple2.py failed with {ex.returncode}: {ex.stderr.strip().splitlines()[-1:]}")
for line in ex.stdout.splitlines():
    if line.startswith(("median rotation error", "pass B with", "pair statuses", "second view-graph solve")):
        log("example: " + line)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
