#!/usr/bin/env python3
"""What Context.prune_weakly_connected costs: per-call wall time (host clock around the call), the phase times the call reports (kernels with
their host waits and the merge rounds, download of the visibility graph) and, from the same run on the same node, the numpy contract
(tests/xm_prune_numpy.py:run_numpy), the host-array form on the same list and one call of Context.filter_tracks on the same context.
Scenes: the SIMPLE2 observation list; with --sphere the sphere scene of scripts/kbench_trackfilter.py (13 682 cameras, 6.44 M observations,
three landmarks seen by every camera).  --no-hubs times that scene again without the three landmarks, which shows what their sum of L^2 costs.
   python scripts/kbench_prune.py [--sphere] [--no-hubs] [--no-contract-large] [--reps K] [--out profiles/...txt]
Needs an MI355X."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import xmamd
import xm_prune_numpy as pr


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


REPS = int(arg("--reps", 5))
out_path = arg("--out", None)
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)
    if out_path:                                            # kept as it grows: a run that is cut short leaves what it measured
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def sphere_scene(N, M, views, seed, hubs=3, noise=1e-3):
    """the scene of scripts/kbench_trackfilter.py (its list and points; the geometry is made up there and not needed here)"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((N, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    C = 30.0 * d
    z = -d
    up = np.where(np.abs(z[:, 2:3]) < 0.9, np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    x = np.cross(up, z); x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(z, x)
    Rcw = np.stack([x, y, z], axis=1)
    tcw = -np.einsum("iab,ib->ia", Rcw, C)
    P = rng.uniform(-1, 1, (M, 3)) * 4.0
    cam = np.concatenate([np.repeat(np.arange(N), hubs), rng.integers(0, N, M * views)])
    lm = np.concatenate([np.tile(np.arange(hubs), N), np.repeat(np.arange(M), views)])
    _, idx = np.unique(cam.astype(np.int64) * M + lm, return_index=True)
    idx = np.sort(idx)
    cam, lm = cam[idx], lm[idx]
    X = np.einsum("kab,kb->ka", Rcw[cam], P[lm]) + tcw[cam]
    u = X[:, :2] / X[:, 2:3] + noise * rng.standard_normal((X.shape[0], 2))
    p = np.concatenate([u, np.ones((X.shape[0], 1))], axis=1) * X[:, 2:3]
    import xm_ba_numpy as ba
    rot, t = ba.to_camera_to_world(Rcw, tcw)
    return dict(cam=cam.astype(np.int32), lm=lm.astype(np.int32), p=p, w=np.ones(cam.size), n=N, m=M, rot=rot, t=t, P=P.T.copy(), opt={})


def timed(call):
    call()                                                  # warm-up: code objects
    wall, kern, down = [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        plan = call()
        wall.append(time.perf_counter() - t0); kern.append(plan.info["seconds_kernels"]); down.append(plan.info["seconds_download"])
    return plan, np.median(wall), np.median(kern), np.median(down), min(wall)


def bench(name, S, contract=True, geometry=None):
    t0 = time.perf_counter()
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"])
    t_ctx = time.perf_counter() - t0
    deg = np.bincount(S["lm"], minlength=S["m"]).astype(np.int64)
    lim = xmamd.prune_limits()
    log(f"{name}: {S['n']} cameras, {S['m']} landmarks, {S['cam'].size} observations; sum of L^2 over the landmarks {int((deg * deg).sum())}, "
        f"of which {int((deg[deg > lim['group_max']] ** 2).sum())} in the {int((deg > lim['group_max']).sum())} landmarks above {lim['group_max']} "
        f"observations (longest {int(deg.max())}); {-(-S['n'] // lim['tile'])} tiles of {lim['tile']} bins; context created in {t_ctx:.2f} s")
    for label, call in (("context form, clusters only", lambda: ctx.prune_weakly_connected()),
                        ("context form with the visibility graph (second call sized by the first: two calls)", lambda: ctx.prune_weakly_connected(pairs=True)),
                        ("host-array form, clusters only (builds and uploads the lists)",
                         lambda: xmamd.prune_weakly_connected(S["cam"], S["lm"], n=S["n"], m=S["m"], w=S["w"]))):
        plan, wall, kern, down, best = timed(call)
        i = plan.info
        log(f"  {label}: {wall * 1e3:9.3f} ms per call (median of {REPS}; best {best * 1e3:.3f}), kernels, waits and merge rounds {kern * 1e3:9.3f} ms, "
            f"download {down * 1e3:8.3f} ms")
    log(f"    {i['pairs_covisible']} pairs, {i['n_edges']} edges, median {i['median']:.0f}, mad {i['mad']:.0f}, threshold {i['threshold']:.0f}, "
        f"largest component {i['component_images']}, {i['strong_clusters']} strong clusters, {i['weak_edges']} edges for the merge rounds, "
        f"{i['rounds']} rounds, {i['n_clusters']} clusters with {i['images_clustered']} images")
    if contract:
        plan = ctx.prune_weakly_connected(pairs=True)
        t0 = time.perf_counter()
        ref = pr.run_numpy(S)
        t_np = time.perf_counter() - t0
        got = dict(plan.info, cluster_id=plan.cluster_id, obs_count=plan.obs_count, pairs_i=plan.pairs[0], pairs_j=plan.pairs[1], pairs_count=plan.pairs[2])
        log(f"    numpy contract on this node: {t_np * 1e3:9.1f} ms; outputs {'identical' if pr.same(got, ref) == [] else 'DIFFER in ' + ', '.join(pr.same(got, ref))}")
    if geometry is not None:
        rot, t, P = geometry
        ctx.filter_tracks(rot, t, P, reprojection=1e-2, triangulation=1.0)
        best = min(_timed_once(lambda: ctx.filter_tracks(rot, t, P, reprojection=1e-2, triangulation=1.0)) for _ in range(3))
        log(f"  one call of filter_tracks on the same context (reprojection 1e-2 + triangulation 1.0 deg, best of 3): {best * 1e3:9.3f} ms")
    ctx.close()


def _timed_once(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


xmamd.require_gpu()
log(f"# kbench_prune: {xmamd.lib().xm_version().decode()}, reps {REPS}")
S2 = pr.simple2(os.path.join(ROOT, "tests", "golden"))
g = np.load(os.path.join(ROOT, "tests", "golden", "simple2", "tp.npz"))
bench("SIMPLE2", S2, geometry=(np.ascontiguousarray(g["R_real"]), np.ascontiguousarray(g["t_est"]), np.ascontiguousarray(g["p_est"])))
if "--sphere" in sys.argv:
    S = sphere_scene(13682, 800000, 8, seed=13682)
    bench("sphere scene of Final-13682 size", S, contract="--no-contract-large" not in sys.argv, geometry=(S["rot"], S["t"], S["P"]))
    if "--no-hubs" in sys.argv:
        keep = S["lm"] >= 3
        H = dict(S, cam=S["cam"][keep], lm=S["lm"][keep] - 3, p=S["p"][keep], w=S["w"][keep], m=S["m"] - 3)
        bench("the same scene without the three landmarks that every camera sees", H, contract=False)
