"""Time per PCG iteration and per LM iteration of the bundle adjustment with a focal scale and a radial coefficient per camera
(Context.bundle_adjust(refine_distortion=True), CD = 8) against the focal form (refine_focal=True, CD = 7) in the same process, by the
protocol of scripts/kbench_ba_groups.py (profiles/r38_kbench_ba_groups.txt): ONE LM iteration from the same start at eta = 0.1 and at
eta = 1e-10, best of three each; (time difference) / (PCG iteration difference) is the cost of a PCG iteration.  Also K LM iterations at
eta = 0.1 and 1e-6 for both forms: PCG iterations and milliseconds per LM iteration.  The focal form's kernels are the parent commit's
(profiles/r42_ba_radial_kernel_resources.txt), so its figures are the parent's.  Scenes: SIMPLE2 (tests/golden/simple2) and the sphere
scene of Final-13682 size of kbench_ba_groups.py, both as given (k = 0 is the truth; the width of the block is what is timed).
   python scripts/kbench_ba_radial.py [--out profiles/<name>.txt] [--iters K] [--no-sphere]"""
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
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def sphere_scene(N, M, views, seed, hubs=3, noise=1e-3):
    """kbench_ba.py's scene: cameras on a sphere looking at the landmark cloud, so every depth is positive"""
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


def one_form(ctx, label, rot0, t0, P0, **kw):
    """(seconds per PCG iteration or None, milliseconds per LM iteration at eta 0.1 and 1e-6)"""
    ctx.bundle_adjust(rot0, t0, P0, max_iters=1, **kw)      # warm-up: code objects, allocations
    one = {}
    for eta in (0.1, 1e-10):
        best = None
        for _ in range(3):
            t = time.time()
            _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, max_iters=1, eta=eta, **kw)
            dt = time.time() - t
            best = (dt, info) if best is None or dt < best[0] else best
        one[eta] = best
    (ta, ia), (tb, ib) = one[0.1], one[1e-10]
    per = None if tb - ta < 0.1 * ta else (tb - ta) / max(1, ib["pcg_iters"] - ia["pcg_iters"])
    its = {}
    for eta in (0.1, 1e-6):
        _, _, _, inf = ctx.bundle_adjust(rot0, t0, P0, max_iters=K, eta=eta, trace=K, function_tol=1e-300, gradient_tol=1e-300, parameter_tol=1e-300, **kw)
        its[eta] = (inf["pcg_iters"], inf["iters"], inf["seconds"], inf["final_cost"])
    log(f"  {label:22s} one LM iteration: eta 0.1 {ta * 1e3:8.2f} ms ({ia['pcg_iters']} PCG), eta 1e-10 {tb * 1e3:8.2f} ms ({ib['pcg_iters']} PCG); per PCG iteration "
        + (f"{per * 1e6:9.1f} us" if per else "not resolved"))
    for eta, (pi, li, sec, fc) in its.items():
        log(f"  {'':22s} eta {eta:g}: {pi} PCG iterations in {li} LM iterations ({pi / max(1, li):.1f} each), {sec * 1e3 / max(1, li):8.3f} ms per LM iteration, cost -> {fc:.6e}")
    return per, {eta: v[2] * 1e3 / max(1, v[1]) for eta, v in its.items()}


def bench(name, obs, n, m, rot0, t0, P0):
    log(f"{name}: {n} cameras, {m} landmarks, {obs[0].size} observations")
    ctx = xmamd.Context(obs=obs, n=n)
    for rnd in (1, 2):                                     # the second round shows the spread
        base, lm7 = one_form(ctx, f"round {rnd}, focal (CD = 7)", rot0, t0, P0, refine_focal=True)
        per, lm8 = one_form(ctx, f"round {rnd}, radial (CD = 8)", rot0, t0, P0, refine_distortion=True)
        if base and per:
            log(f"  {'':22s} CD = 8 / CD = 7: {per / base:.3f} x per PCG iteration ({(per - base) * 1e6:+.1f} us)")
        for eta in lm7:
            log(f"  {'':22s} CD = 8 / CD = 7: {lm8[eta] / lm7[eta]:.3f} x per LM iteration at eta {eta:g} (the PCG iteration counts differ: another problem)")
    ctx.close()


log(f"kbench_ba_radial: {time.strftime('%Y-%m-%d %H:%M:%S')}  K = {K} LM iterations per run; one run")
log("CD = 7 is timed in this process: its kernels have the parent commit's resource figures (profiles/r42_ba_radial_kernel_resources.txt)")
Gd = os.path.join(ROOT, "tests", "golden", "simple2")
Z = np.load(os.path.join(Gd, "obs.npz"))
ref = np.load(os.path.join(Gd, "tp.npz"))
bench("SIMPLE2 (the reference's R_real, t_est, p_est)", (Z["cam"], Z["lm"], Z["p"], Z["w"].reshape(-1)), ref["t_est"].shape[1], ref["p_est"].shape[1],
      ref["R_real"], ref["t_est"], ref["p_est"])
if "--no-sphere" not in sys.argv:
    S = sphere_scene(13682, 800000, 8, seed=13682)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=0.5, rel=1e-3)
    bench("sphere scene of Final-13682 size", (S["cam"], S["lm"], S["p"], S["w"]), S["n"], S["m"], rot0, t0, P0)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
