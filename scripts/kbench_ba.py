"""Time per LM iteration and per PCG iteration of the reprojection bundle adjustment (xm_ctx_bundle_adjust) and the bytes one PCG iteration
streams (a model of the kernels' loads and stores), at two sizes:
   SIMPLE2 (tests/golden/simple2: the reference's own recovered solution as the start, what its Ceres step would get)
   a scene of gen_scene Final-13682 size (13 682 cameras, 800 000 landmarks, 8 random views each + 3 landmarks seen by every camera) whose
   cameras sit on a sphere looking at the landmark cloud, so every depth is positive
   python scripts/kbench_ba.py [--out profiles/<name>.txt] [--iters K] [--loss NAME --scale A] [--nonmonotonic]
(--loss: one of xmamd.BA_LOSS with its scale A in normalised image units; --nonmonotonic: Ceres's non-monotonic steps.)
Per LM iteration: runs of exactly K LM iterations (stop tolerances 1e-300) at eta = 0.1 and 1e-4.  Per PCG iteration: ONE LM iteration
from the same start at eta = 0.1 and at eta = 1e-10 (identical work apart from the PCG), best of three each; (time difference) / (PCG
iteration difference).
   python scripts/kbench_ba.py --solver dense [--seq 500,1000,2000,5000] [--iters K] [--no-converge] [--out ...]
compares the dense Schur solver (linear_solver="dense_schur") with the PCG at eta 0.1 and 1e-6 on SIMPLE2 and on sequential captures
(xm_ba_numpy.sequential_scene, seeds 62 / 63 as in the tests) instead: time per LM iteration over K iterations, then LM iterations, wall
time and final cost of a run to function_tol 1e-8 (at most 200 iterations or 120 s).  The sphere scene is above XM_BA_DENSE_MAX_ROWS.
   python scripts/kbench_ba.py --precond {jacobi,blocks,two_level} [--seq 500,1000,...] [--sphere] [--no-simple2] [--iters K] [--no-converge] [--out ...]
the same comparison for one preconditioner of the PCG (Context.bundle_adjust(preconditioner=...)) at eta 0.1 and 1e-6, with the PCG
iterations of every step; --sphere adds the Final-13682-size sphere scene.  Without --seq / --sphere the option only selects the
preconditioner of the default benchmark above.
   python scripts/kbench_ba.py --refine-focal [--out ...]
runs the default benchmark on each scene twice in turn in one process -- without and with focal scales (Context.bundle_adjust(
refine_focal=True): camera blocks of 7 instead of 6, records of 22 doubles per observation instead of 20) -- and prints the ratios per LM
iteration and per PCG iteration."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import xmamd
import xm_ba_numpy as ba


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


K = int(arg("--iters", 10))
out_path = arg("--out", None)
LOSS = dict(loss=arg("--loss", "trivial"), loss_scale=float(arg("--scale", 0.0)), nonmonotonic="--nonmonotonic" in sys.argv)
PRECOND = arg("--precond", None)
if PRECOND is not None:
    if PRECOND not in xmamd.BA_PRECONDITIONERS:
        sys.exit(f"--precond: one of {', '.join(xmamd.BA_PRECONDITIONERS)}")
    LOSS["preconditioner"] = PRECOND
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def sphere_scene(N, M, views, seed, hubs=3, noise=1e-3):
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


def pcg_bytes(n, m, nobs, cd=6):
    planes = 2 * cd + 6                               # J_c and J_P of an observation, read by both list passes
    per_obs = 2 * planes * 8 + 2 * 4 + (cd + 3) * 8   # + the two index arrays + the gathered x_i / y_l records
    per_cam = cd * cd * 8 * 2 + cd * 8 * 12           # U*, S_ii^-1 and the vector traffic of the flat kernels
    return nobs * per_obs + n * per_cam + m * (6 + 3) * 8


def bench(name, obs, n, m, rot0, t0, P0, cd=6):
    """returns (ms per LM iteration at eta 0.1, seconds per PCG iteration or None when it is not resolved); cd = 7: with focal scales"""
    LOSS = dict(globals()["LOSS"], refine_focal=True) if cd == 7 else globals()["LOSS"]
    name = f"{name}, focal scales (CD = 7)" if cd == 7 else name
    ctx = xmamd.Context(obs=obs, n=n)
    ctx.bundle_adjust(rot0, t0, P0, max_iters=1, **LOSS)      # warm-up: code objects, allocations
    r = {}
    for eta in (0.1, 1e-4):
        t = time.time()
        _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, max_iters=K, eta=eta, trace=K, function_tol=1e-300, gradient_tol=1e-300,
                                             parameter_tol=1e-300, **LOSS)
        r[eta] = (time.time() - t, info)
    one = {}
    for eta in (0.1, 1e-10):
        best = None
        for _ in range(3):
            t = time.time()
            _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, max_iters=1, eta=eta, **LOSS)
            dt = time.time() - t
            best = (dt, info) if best is None or dt < best[0] else best
        one[eta] = best
    ctx.close()
    (ta, ia), (tb, ib) = one[0.1], one[1e-10]
    nobs = obs[0].size
    per_pcg = (tb - ta) / max(1, ib["pcg_iters"] - ia["pcg_iters"])
    by = pcg_bytes(n, m, nobs, cd)
    log(f"{name}: {n} cameras, {m} landmarks, {nobs} observations ({ia['n_used']} used)")
    for eta, (tt, inf) in r.items():
        log(f"  eta {eta:g}: {inf['iters']} LM iterations ({inf['accepted']} accepted), {inf['pcg_iters']} PCG iterations, {tt * 1e3:9.2f} ms wall, "
            f"{inf['seconds'] * 1e3:9.2f} ms in the call, {inf['seconds'] * 1e3 / max(1, inf['iters']):8.3f} ms per LM iteration; "
            f"cost {inf['initial_cost']:.6e} -> {inf['final_cost']:.6e} ({inf['status_name']})")
    log(f"  one LM iteration: eta 0.1 {ta * 1e3:.2f} ms ({ia['pcg_iters']} PCG), eta 1e-10 {tb * 1e3:.2f} ms ({ib['pcg_iters']} PCG)")
    if tb - ta < 0.1 * ta:   # the rest of the LM iteration (with a preconditioner: its set-up) hides the PCG: the difference is noise
        log(f"  per PCG iteration: not resolved (the two single iterations differ by {(tb - ta) * 1e3:.2f} ms, less than a tenth of either)")
    else:
        log(f"  per PCG iteration: {per_pcg * 1e6:9.1f} us; modelled traffic {by / 1e6:9.1f} MB -> {by / per_pcg / 1e9:7.1f} GB/s")
    return r[0.1][1]["seconds"] * 1e3 / max(1, r[0.1][1]["iters"]), (None if tb - ta < 0.1 * ta else per_pcg)


def bench_both(name, *a):
    """the scene without and, with --refine-focal, with focal scales, alternating, two rounds (the second shows the spread); the ratios"""
    if "--refine-focal" not in sys.argv:
        bench(name, *a)
        return
    by = pcg_bytes(a[1], a[2], a[0][0].size, 7) / pcg_bytes(a[1], a[2], a[0][0].size, 6)
    for rnd in (1, 2):
        lm6, pcg6 = bench(f"{name}, round {rnd}", *a)
        lm7, pcg7 = bench(f"{name}, round {rnd}", *a, cd=7)
        log(f"  round {rnd}, focal scales / without: {lm7 / lm6:.3f} x per LM iteration (eta 0.1)" +
            (f", {pcg7 / pcg6:.3f} x per PCG iteration" if pcg6 and pcg7 else ", per PCG iteration not resolved") +
            f"; modelled PCG traffic {by:.3f} x")


SOLVERS = [("dense", dict(linear_solver="dense_schur")), ("eta 0.1", dict(eta=0.1)), ("eta 1e-6", dict(eta=1e-6))]
PRECOND_MODE = PRECOND is not None and ("--seq" in sys.argv or "--sphere" in sys.argv)
if PRECOND_MODE:
    SOLVERS = SOLVERS[1:]


def bench_solvers(name, obs, n, m, rot0, t0, P0):
    ctx = xmamd.Context(obs=obs, n=n)
    log(f"{name}: {n} cameras ({6 * n} rows in the reduced camera system), {m} landmarks, {obs[0].size} observations")
    for label, kw in SOLVERS:
        ctx.bundle_adjust(rot0, t0, P0, max_iters=1, **kw, **LOSS)      # warm-up: code objects, allocations
        t = time.time()
        _, _, _, inf = ctx.bundle_adjust(rot0, t0, P0, max_iters=K, trace=K, function_tol=1e-300, gradient_tol=1e-300, parameter_tol=1e-300,
                                         **kw, **LOSS)
        tt = time.time() - t
        log(f"  {label:9s} K = {inf['iters']}: {inf['seconds'] * 1e3 / max(1, inf['iters']):9.3f} ms per LM iteration ({tt * 1e3:9.2f} ms wall), "
            f"{inf['pcg_iters']} PCG iterations, max per step {int(inf['trace'][:, 4].max())}, largest |b - S dc| / |b| {inf['trace'][:, 5].max():.2e}")
        if PRECOND_MODE:
            log(f"            PCG iterations per step {inf['trace'][:, 4].astype(int).tolist()}, coarse fallbacks {inf['coarse_fallbacks']}")
    if "--no-converge" not in sys.argv:
        for label, kw in SOLVERS:
            t = time.time()
            _, _, _, inf = ctx.bundle_adjust(rot0, t0, P0, max_iters=200, max_time=120.0, function_tol=1e-8, **kw, **LOSS)
            tt = time.time() - t
            log(f"  {label:9s} to function_tol 1e-8: {inf['iters']:4d} LM iterations ({inf['accepted']} accepted), {tt:8.3f} s wall, "
                f"{inf['pcg_iters']} PCG iterations, cost {inf['initial_cost']:.6e} -> {inf['final_cost']:.12e} ({inf['status_name']})")
    ctx.close()


log(f"kbench_ba: {time.strftime('%Y-%m-%d %H:%M:%S')}  K = {K} LM iterations per run; loss {LOSS['loss']} (scale {LOSS['loss_scale']:g})"
    f"{', non-monotonic steps' if LOSS['nonmonotonic'] else ''}")
G = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(G, "obs.npz"))
ref = np.load(os.path.join(G, "tp.npz"))
if PRECOND_MODE:
    log(f"preconditioner {PRECOND}")
if arg("--solver", "iterative") == "dense" or PRECOND_MODE:
    if "--no-simple2" not in sys.argv:
        bench_solvers("SIMPLE2 (the reference's R_real, t_est, p_est)", (Z["cam"], Z["lm"], Z["p"], Z["w"].reshape(-1)), ref["t_est"].shape[1],
                      ref["p_est"].shape[1], ref["R_real"], ref["t_est"], ref["p_est"])
    for nc in [int(v) for v in arg("--seq", "" if PRECOND_MODE else "500,1000,2000,5000").split(",") if v]:
        S = ba.sequential_scene(n_cams=nc, seed=62, noise=1e-3)
        rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=63, deg=0.5, rel=2e-4)
        bench_solvers(f"sequential capture of {nc} cameras", (S["cam"], S["lm"], S["p"], S["w"]), S["n"], S["m"], rot0, t0, P0)
    if PRECOND_MODE and "--sphere" in sys.argv:
        S = sphere_scene(13682, 800000, 8, seed=13682)
        rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=0.5, rel=1e-3)
        bench_solvers("sphere scene of Final-13682 size", (S["cam"], S["lm"], S["p"], S["w"]), S["n"], S["m"], rot0, t0, P0)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
bench_both("SIMPLE2 (the reference's R_real, t_est, p_est)", (Z["cam"], Z["lm"], Z["p"], Z["w"].reshape(-1)), ref["t_est"].shape[1], ref["p_est"].shape[1],
      ref["R_real"], ref["t_est"], ref["p_est"])
t = time.time()
S = sphere_scene(13682, 800000, 8, seed=13682)
rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=0.5, rel=1e-3)
log(f"(scene generated in {time.time() - t:.1f} s)")
bench_both("sphere scene of Final-13682 size", (S["cam"], S["lm"], S["p"], S["w"]), S["n"], S["m"], rot0, t0, P0)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
