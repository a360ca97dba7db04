#!/usr/bin/env python3
"""What Context.triangulate_tracks costs: per-call wall time (host clock around the call, which ends in the download), the share of the call
that is upload + kernels, and, from the same run on the same node, the numpy contract (tests/xm_triangulate_numpy.py:run_numpy) and one
Context.filter_tracks call for scale.  Scenes: the SIMPLE2 observation list at the reference's solution; with --sphere the sphere scene of
scripts/kbench_trackfilter.py (13 682 cameras, 6.44 M observations, three landmarks seen by every camera: the workgroup form).
   python scripts/kbench_triangulate.py [--sphere] [--reps K] [--out profiles/...txt]
Needs an MI355X."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import xmamd
import xm_ba_numpy as ba
import xm_trackfilter_numpy as tf
import xm_triangulate_numpy as tri


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


REPS = int(arg("--reps", 10))
out_path = arg("--out", None)
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def sphere_scene(N, M, views, seed, hubs=3, noise=1e-3):
    """the scene of scripts/kbench_trackfilter.py: cameras on a sphere looking at the landmark cloud, `hubs` landmarks seen by every camera"""
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
    rot, t = ba.to_camera_to_world(Rcw, tcw)
    return dict(cam=cam.astype(np.int32), lm=lm.astype(np.int32), p=p, w=np.ones(cam.size), n=N, m=M, rot=rot, t=t, P=P.T.copy())


def bench(name, S, contract=True):
    t0 = time.perf_counter()
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"])
    t_ctx = time.perf_counter() - t0
    deg = np.bincount(S["lm"], minlength=S["m"])
    lim = xmamd.triangulate_limits()
    log(f"{name}: {S['n']} cameras, {S['m']} landmarks, {S['cam'].size} observations; {int((deg > lim['light_max']).sum())} landmarks above "
        f"{lim['light_max']} observations (longest {int(deg.max())}); context created in {t_ctx:.2f} s")
    ctx.triangulate_tracks(S["rot"], S["t"], P=S["P"])                  # warm-up: code objects
    wall, kern, down = [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        plan = ctx.triangulate_tracks(S["rot"], S["t"], P=S["P"])
        wall.append(time.perf_counter() - t0); kern.append(plan.info["seconds_kernels"]); down.append(plan.info["seconds_download"])
    w_, k_, d_ = np.median(wall), np.median(kern), np.median(down)
    log(f"  triangulate_tracks (defaults): {w_ * 1e3:9.3f} ms per call (median of {REPS}; best {min(wall) * 1e3:.3f}), upload + kernels {k_ * 1e3:9.3f} ms "
        f"({100.0 * k_ / w_:.0f} % of the call), download {d_ * 1e3:8.3f} ms; accepted {plan.info['lm_accepted']} of {S['m']} landmarks, kept "
        f"{plan.info['obs_kept']} of {plan.info['obs_candidates']} candidates; {plan.info['hypotheses_scored']} hypotheses scored of "
        f"{plan.info['pairs_tested']} pairs tested")
    if contract:
        t0 = time.perf_counter()
        ref = tri.run_numpy(S, cos_min_angle=plan.info["cos_min_angle"], cos_create=plan.info["cos_create"])
        t_np = time.perf_counter() - t0
        got = dict(plan.info, p=plan.P, keep=plan.keep, reason=plan.reason, lm_views=plan.views, lm_status=plan.status, lm_support=plan.support,
                   lm_hypothesis=plan.hypothesis)
        log(f"    numpy contract on this node: {t_np * 1e3:9.1f} ms ({t_np / w_:.0f} x the call); outputs "
            f"{'identical' if tri.same(got, ref) == [] else 'DIFFER in ' + ', '.join(tri.same(got, ref))}")
    ctx.filter_tracks(S["rot"], S["t"], S["P"], reprojection=1e-2, triangulation=1.0)
    best = min(_timed(lambda: ctx.filter_tracks(S["rot"], S["t"], S["P"], reprojection=1e-2, triangulation=1.0)) for _ in range(3))
    log(f"  one call of filter_tracks on the same context (reprojection 1e-2 + triangulation 1.0 deg, best of 3): {best * 1e3:9.3f} ms")
    ctx.close()


def _timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


xmamd.require_gpu()
log(f"# kbench_triangulate: {xmamd.lib().xm_version().decode()}, reps {REPS}")
bench("SIMPLE2 at the reference's solution", tf.simple2(os.path.join(ROOT, "tests", "golden")))
if "--sphere" in sys.argv:
    bench("sphere scene of Final-13682 size", sphere_scene(13682, 800000, 8, seed=13682), contract="--no-contract" not in sys.argv)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
