#!/usr/bin/env python3
"""What Context.global_positioning costs: the whole call from a random start (LM and PCG iteration counts, wall time), the time of one
LM iteration and of one PCG iteration (two one-iteration calls from the same start, eta 0.1 and eta 1e-6: the difference of their times
over the difference of their PCG iterations), the same two figures for one LM iteration of Context.bundle_adjust(fix_rotations=True)
(the same 3 x 3 camera blocks) measured in the same run at the scene's own geometry, and the numpy restatement (tests/xm_gp_numpy.py) on
the same node.  Scenes: a ring scene of 30 cameras x 400 points (the largest size of the tests); the SIMPLE2 observation list with the
ground-truth rotations; with --sphere the sphere scene of scripts/kbench_ba.py (13 682 cameras, 6.44 M observations, three landmarks
seen by every camera), where the restatement is not run: the camera block of its sparse factor alone is dense with 41 046 rows, 13 GB.
   python scripts/kbench_gp.py [--sphere] [--out profiles/...txt]
Needs an MI355X."""
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import xmamd
import xm_ba_numpy as ba
import xm_gp_numpy as gp


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


out_path = arg("--out", None)
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def read_bin(fn):
    with open(fn, "rb") as f:
        r, c = struct.unpack("<ii", f.read(8))
        return np.frombuffer(f.read(), dtype="<f8").reshape(c, r).T.copy()


def simple2():
    G = os.path.join(ROOT, "tests", "golden", "simple2")
    Z, ref = np.load(os.path.join(G, "obs.npz")), np.load(os.path.join(G, "tp.npz"))
    gt, fi = read_bin(os.path.join(G, "gtR.bin")), np.load(os.path.join(G, "frame_index.npy"))
    cam, lm = Z["cam"].astype(np.int32), Z["lm"].astype(np.int32)
    return dict(cam=cam, lm=lm, p=Z["p"], w=Z["w"].reshape(-1), n=int(cam.max()) + 1, m=int(lm.max()) + 1,
                rot=np.concatenate([gt[:, 3 * f:3 * f + 3].T for f in fi], axis=1), ba=(ref["R_real"], ref["t_est"], ref["p_est"]))


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
    return dict(cam=cam.astype(np.int32), lm=lm.astype(np.int32), p=p, w=np.ones(cam.size), n=N, m=M, rot=rot, ba=(rot, t, P.T.copy()))


def one_iteration(call):
    """(seconds of an LM iteration at eta 0.1, its PCG iterations, seconds per PCG iteration) from one-iteration calls, best of 3 each"""
    best = {}
    for eta in (0.1, 1e-6):
        call(eta)                                              # warm-up: code objects
        for _ in range(3):
            t0 = time.perf_counter()
            info = call(eta)
            dt = time.perf_counter() - t0
            if eta not in best or dt < best[eta][0]:
                best[eta] = (dt, info["pcg_iters"])
    (ta, pa), (tb, pb) = best[0.1], best[1e-6]
    return ta, pa, (tb - ta) / max(1, pb - pa), pb


def bench(name, S, restate):
    t0 = time.perf_counter()
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"])
    log(f"{name}: {S['n']} cameras, {S['m']} landmarks, {S['cam'].size} observations; context created in {time.perf_counter() - t0:.2f} s")
    t_s, P_s = xmamd.gp_random_start(S["n"], S["m"], 1)
    ctx.global_positioning(S["rot"], t_s, P_s, max_iters=1)    # warm-up
    t0 = time.perf_counter()
    _, _, g = ctx.global_positioning(S["rot"], t_s, P_s)
    wall = time.perf_counter() - t0
    log(f"  global_positioning from gp_random_start(seed 1), defaults: {g['iters']} LM iterations ({g['accepted']} accepted), {g['pcg_iters']} PCG "
        f"iterations, cost {g['initial_cost']:.6e} -> {g['final_cost']:.6e}, {g['status_name']}, {wall:.3f} s ({wall / max(1, g['iters']) * 1e3:.3f} ms per "
        f"LM iteration over the call)")
    lm_t, lm_p, pcg_t, pcg_hi = one_iteration(lambda eta: ctx.global_positioning(S["rot"], t_s, P_s, max_iters=1, eta=eta)[2])
    log(f"  one LM iteration of global_positioning (eta 0.1, {lm_p} PCG iterations, best of 3): {lm_t * 1e3:9.3f} ms; per PCG iteration "
        f"{pcg_t * 1e6:9.1f} us (from a call with eta 1e-6: {pcg_hi} iterations)")
    rot_b, t_b, P_b = S["ba"]
    lm_t, lm_p, pcg_t, pcg_hi = one_iteration(lambda eta: ctx.bundle_adjust(rot_b, t_b, P_b, fix_rotations=True, max_iters=1, eta=eta)[3])
    log(f"  one LM iteration of bundle_adjust(fix_rotations=True) (eta 0.1, {lm_p} PCG iterations, best of 3): {lm_t * 1e3:9.3f} ms; per PCG "
        f"iteration {pcg_t * 1e6:9.1f} us (from a call with eta 1e-6: {pcg_hi} iterations)")
    ctx.close()
    if restate:
        t0 = time.perf_counter()
        _, _, r1 = gp.lm(S["cam"], S["lm"], S["p"], S["w"], S["rot"], t_s, P_s, max_iters=1)
        t1 = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, _, r = gp.lm(S["cam"], S["lm"], S["p"], S["w"], S["rot"], t_s, P_s)
        tr = time.perf_counter() - t0
        log(f"  numpy restatement on this node (exact sparse solves): one LM iteration {t1:.3f} s; the whole run {r['iters']} LM iterations, cost "
            f"{r['final_cost']:.6e}, {tr:.3f} s")
    else:
        log("  numpy restatement: not run at this size (the dense camera block of its factor)")


xmamd.require_gpu()
log(f"# kbench_gp: {xmamd.lib().xm_version().decode()}")
R = ba.ring_scene(n_cams=30, n_pts=400, seed=10, noise=2e-3)
bench("ring scene 30 x 400, noise 2e-3", dict(R, ba=(R["rot"], R["t"], R["P"])), True)
bench("SIMPLE2 with the ground-truth rotations", simple2(), True)
if "--sphere" in sys.argv:
    bench("sphere scene of Final-13682 size", sphere_scene(13682, 800000, 8, seed=13682), False)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
