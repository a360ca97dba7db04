#!/usr/bin/env python3
"""What Context.filter_tracks costs: per-call wall time (host clock around the call, which ends in the download), the phase times the call
reports (upload + kernels, download) and, from the same run on the same node, the numpy contract (tests/xm_trackfilter_numpy.py:run_numpy)
and one LM iteration of Context.bundle_adjust at the same size.  Scenes: the SIMPLE2 observation list at the reference's solution; a sphere
scene with 16 landmarks seen by every camera (heavy tracks); with --sphere the sphere scene of scripts/kbench_ba.py (13 682 cameras, 6.44 M
observations, three landmarks seen by every camera).  Per scene: GLOMAP's closing pair of filters in one call (reprojection 1e-2 and
triangulation 1.0 degree), all three filters, and the triangulation filter alone at 179.9 degrees: hardly any pair qualifies, so a short
landmark visits every pair and a landmark seen by every camera searches deep into its list (cameras on a sphere do have a few nearly
antipodal pairs: the kept tracks in the output are the landmarks that still found one).
   python scripts/kbench_trackfilter.py [--sphere] [--reps K] [--out profiles/...txt]
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


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


REPS = int(arg("--reps", 10))
out_path = arg("--out", None)
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def sphere_scene(N, M, views, seed, hubs=3, noise=1e-3):
    """the scene of scripts/kbench_ba.py: cameras on a sphere looking at the landmark cloud, `hubs` landmarks seen by every camera"""
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


def timed(ctx, S, **kw):
    ctx.filter_tracks(S["rot"], S["t"], S["P"], **kw)                 # warm-up: code objects
    wall, kern, down = [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        plan = ctx.filter_tracks(S["rot"], S["t"], S["P"], **kw)
        wall.append(time.perf_counter() - t0); kern.append(plan.info["seconds_kernels"]); down.append(plan.info["seconds_download"])
    return plan, np.median(wall), np.median(kern), np.median(down), min(wall)


def bench(name, S, contract=True):
    t0 = time.perf_counter()
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"])
    t_ctx = time.perf_counter() - t0
    deg = np.bincount(S["lm"], minlength=S["m"])
    lim = xmamd.track_filter_limits()
    log(f"{name}: {S['n']} cameras, {S['m']} landmarks, {S['cam'].size} observations; {int((deg > lim['light_max']).sum())} landmarks above "
        f"{lim['light_max']} observations (longest {int(deg.max())}); context created in {t_ctx:.2f} s")
    for label, kw in (("reprojection 1e-2 + triangulation 1.0 deg", dict(reprojection=1e-2, triangulation=1.0)),
                      ("reprojection 1e-2 + angle 1.0 deg + triangulation 1.0 deg", dict(reprojection=1e-2, angle=1.0, triangulation=1.0)),
                      ("triangulation 179.9 deg alone (hardly any pair qualifies: the pair search runs deep)", dict(reprojection=None, triangulation=179.9))):
        plan, wall, kern, down, best = timed(ctx, S, **kw)
        log(f"  {label}: {wall * 1e3:9.3f} ms per call (median of {REPS}; best {best * 1e3:.3f}), upload + kernels {kern * 1e3:9.3f} ms, "
            f"download {down * 1e3:8.3f} ms; kept {plan.info['obs_kept']} of {plan.info['obs_used']} observations, "
            f"{plan.info['tracks_kept']} of {plan.info['tracks_total']} tracks")
        if contract and kw.get("triangulation") != 179.9:
            t0 = time.perf_counter()
            ref = tf.run_numpy(S, cos_angle=plan.info["cos_angle"], cos_triangulation=plan.info["cos_triangulation"],
                               **dict(dict(reprojection=1e-2, angle=None, triangulation=None), **kw))
            t_np = time.perf_counter() - t0
            got = dict(plan.info, keep=plan.keep, reason=plan.reason, lm_views=plan.lm_views, lm_status=plan.lm_status)
            log(f"    numpy contract on this node: {t_np * 1e3:9.1f} ms ({t_np / wall:.0f} x the call); outputs "
                f"{'identical' if tf.same(got, ref) == [] else 'DIFFER in ' + ', '.join(tf.same(got, ref))}")
    ctx.bundle_adjust(S["rot"], S["t"], S["P"], max_iters=1)          # warm-up
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        _, _, _, info = ctx.bundle_adjust(S["rot"], S["t"], S["P"], max_iters=1, eta=0.1)
        dt = time.perf_counter() - t0
        best = (dt, info) if best is None or dt < best[0] else best
    log(f"  one LM iteration of bundle_adjust (eta 0.1, {best[1]['pcg_iters']} PCG iterations, best of 3): {best[0] * 1e3:9.3f} ms")
    ctx.close()


xmamd.require_gpu()
log(f"# kbench_trackfilter: {xmamd.lib().xm_version().decode()}, reps {REPS}")
bench("SIMPLE2 at the reference's solution", tf.simple2(os.path.join(ROOT, "tests", "golden")))
bench("sphere scene with heavy tracks", sphere_scene(2000, 100000, 8, seed=2000, hubs=16))
if "--sphere" in sys.argv:
    bench("sphere scene of Final-13682 size", sphere_scene(13682, 800000, 8, seed=13682))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
