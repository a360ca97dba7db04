#!/usr/bin/env python3
"""What Context.global_positioning costs with camera-to-camera constraints: for the four constraint types and the fixed-centre pass, the
whole call from a perturbed truth (LM and PCG iterations, wall time) and the time per PCG iteration (two one-iteration calls, eta 0.1 and
1e-6: the difference of their times over the difference of their PCG iterations).  Scenes: SIMPLE2 with the ground-truth rotations and
every camera paired with its next ten; a sphere scene of 2 000 cameras with ALL 1 999 000 pairs, where every camera's incidence list is
walked by a workgroup of its own.

The one claim: ONLY_POINTS through xm_ctx_global_positioning_pairs costs no more than through xm_ctx_global_positioning, and neither
more than the parent commit's library.  Measured in turn in one run, each in a fresh child process (--child), ROUNDS rounds:
    parent library, old entry   (only with --parent-lib PATH: lib/libxm_amd.so of a built checkout of the parent commit, whose
                                 xmamd.py beside lib/ is the binding the child then uses)
    this library, old entry
    this library, new entry (pairs=(), constraint only_points)
each child: the median and the minimum of CALLS whole default calls on SIMPLE2 from gp_random_start(seed 1).  The spread between the
rounds of one configuration is printed beside the differences between configurations.

   python scripts/kbench_gp_pairs.py [--parent-lib PATH] [--out profiles/...txt]
Needs an MI355X."""
import json
import os
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a child that times another library (XMAMD_LIB) takes the binding beside it: PARENT/xm-code_amd/{xmamd.py, lib/libxm_amd.so}
_lib = os.environ.get("XMAMD_LIB") if "--child" in sys.argv else None
PKG = os.path.dirname(os.path.dirname(os.path.abspath(_lib))) if _lib else os.path.join(ROOT, "xm-code_amd")
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, PKG)
import numpy as np
import xmamd
import xm_ba_numpy as ba

ROUNDS, CALLS = 3, 9
TYPES = ("only_points", "only_cameras", "points_and_cameras_balanced", "points_and_cameras", "fixed")


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


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
    Z = np.load(os.path.join(G, "obs.npz"))
    gt, fi = read_bin(os.path.join(G, "gtR.bin")), np.load(os.path.join(G, "frame_index.npy"))
    cam, lm = Z["cam"].astype(np.int32), Z["lm"].astype(np.int32)
    return dict(cam=cam, lm=lm, p=Z["p"], w=Z["w"].reshape(-1), n=int(cam.max()) + 1, m=int(lm.max()) + 1,
                rot=np.concatenate([gt[:, 3 * f:3 * f + 3].T for f in fi], axis=1))


def sphere_scene(N, M, views, seed, noise=1e-3):
    """cameras on a sphere looking at a landmark cloud (the scene of scripts/kbench_gp.py without its hub landmarks)"""
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
    cam, lm = rng.integers(0, N, M * views), np.repeat(np.arange(M), views)
    _, idx = np.unique(cam.astype(np.int64) * M + lm, return_index=True)
    idx = np.sort(idx)
    cam, lm = cam[idx], lm[idx]
    X = np.einsum("kab,kb->ka", Rcw[cam], P[lm]) + tcw[cam]
    u = X[:, :2] / X[:, 2:3] + noise * rng.standard_normal((X.shape[0], 2))
    p = np.concatenate([u, np.ones((X.shape[0], 1))], axis=1) * X[:, 2:3]
    rot, t = ba.to_camera_to_world(Rcw, tcw)
    return dict(cam=cam.astype(np.int32), lm=lm.astype(np.int32), p=p, w=np.ones(cam.size), n=N, m=M, rot=rot, t=t, P=P.T.copy())


def translations(rot, t, pi, pj, noise, seed):
    n = t.shape[1]
    R = np.stack([rot[:, 3 * i:3 * i + 3] for i in range(n)])
    d = (t[:, pi] - t[:, pj]).T
    tr = np.einsum("kba,kb->ka", R[pj], d / np.linalg.norm(d, axis=1, keepdims=True)) + noise * np.random.default_rng(seed).standard_normal((pi.size, 3))
    return tr / np.linalg.norm(tr, axis=1, keepdims=True)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def bench(name, S, pairs, t_true, P_true):
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"])
    rng = np.random.default_rng(3)
    ext = np.linalg.norm(t_true.max(axis=1) - t_true.min(axis=1))
    t0, P0 = t_true + 0.05 * ext * rng.uniform(-1, 1, t_true.shape), P_true + 0.05 * ext * rng.uniform(-1, 1, P_true.shape)
    log(f"{name}: {S['n']} cameras, {S['m']} landmarks, {S['cam'].size} observations, {pairs[0].size} pairs; start: the truth moved by up to 0.05 of its extent")
    for ty in TYPES:
        kw = dict(fix_centres=True) if ty == "fixed" else dict(pairs=pairs, constraint=ty, points=False)
        call = lambda **o: ctx.global_positioning(S["rot"], t0, P0, **kw, **o)[2]
        call(max_iters=1)                                          # warm-up: code objects
        wall, g = min((timed(call) for _ in range(3)), key=lambda r: r[0])
        best = {}
        for eta in (0.1, 1e-6):
            best[eta] = min((timed(lambda: call(max_iters=1, eta=eta)) for _ in range(3)), key=lambda r: r[0])
        (ta, ia), (tb, ib) = best[0.1], best[1e-6]
        dp = ib["pcg_iters"] - ia["pcg_iters"]
        per = f"{(tb - ta) / dp * 1e6:9.1f} us per PCG iteration ({ia['pcg_iters']} and {ib['pcg_iters']} iterations)" if dp > 0 else "no PCG"
        log(f"  {ty:28s} {g['iters']:3d} LM iterations ({g['accepted']} accepted), {g['pcg_iters']:4d} PCG, cost {g['initial_cost']:.4e} -> {g['final_cost']:.4e}, "
            f"{g['status_name']}, {wall * 1e3:9.3f} ms per call (best of 3); one-iteration call {ta * 1e3:8.3f} ms; {per}; heavy cameras {g.get('cams_heavy', 0)}")
    ctx.close()


def child(entry):
    S = simple2()
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"])
    ts, Ps = xmamd.gp_random_start(S["n"], S["m"], 1)
    none = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3)))
    call = (lambda: ctx.global_positioning(S["rot"], ts, Ps)) if entry == "old" else (lambda: ctx.global_positioning(S["rot"], ts, Ps, pairs=none))
    call(); call()
    times = [timed(call)[0] for _ in range(CALLS)]
    g = call()[2]
    ctx.close()
    print(json.dumps(dict(median=float(np.median(times)), min=float(min(times)), iters=g["iters"], pcg=g["pcg_iters"], cost=g["final_cost"])))


def ab(parent_lib):
    configs = [("this library, old entry", None, "old"), ("this library, new entry", None, "new")]
    if parent_lib:
        configs.insert(0, ("parent library, old entry", parent_lib, "old"))
    res = {c[0]: [] for c in configs}
    for _ in range(ROUNDS):
        for label, libp, entry in configs:
            env = dict(os.environ)
            if libp:
                env["XMAMD_LIB"] = os.path.abspath(libp)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", entry], env=env, capture_output=True, text=True, timeout=120)
            if out.returncode != 0:
                raise SystemExit(f"child {label} failed ({out.returncode}):\n{out.stderr[-2000:]}")
            res[label].append(json.loads(out.stdout.strip().splitlines()[-1]))
    log(f"ONLY_POINTS on SIMPLE2 from gp_random_start(seed 1), whole default calls, {ROUNDS} rounds in turn, {CALLS} calls per child process:")
    for label, rs in res.items():
        med = [r["median"] * 1e3 for r in rs]
        log(f"  {label:28s} median per round {', '.join(f'{v:.3f}' for v in med)} ms (spread {max(med) - min(med):.3f} ms), minimum "
            f"{min(r['min'] for r in rs) * 1e3:.3f} ms; {rs[0]['iters']} LM iterations, {rs[0]['pcg']} PCG, cost {rs[0]['cost']:.12e}")
    costs = {r["cost"] for rs in res.values() for r in rs}
    log(f"  final costs of all runs identical: {len(costs) == 1}")


if "--child" in sys.argv:
    child(arg("--child", "old"))
    sys.exit(0)
xmamd.require_gpu()
log(f"# kbench_gp_pairs: {xmamd.lib().xm_version().decode()}")
ab(arg("--parent-lib", None))
S = simple2()
ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"])
t_ref, P_ref, _ = ctx.global_positioning(S["rot"], seed=1)
ctx.close()
pi, pj = np.array([(i, j) for i in range(S["n"]) for j in range(i + 1, min(S["n"], i + 11))], dtype=np.int32).T
pi, pj = np.ascontiguousarray(pi), np.ascontiguousarray(pj)
bench("SIMPLE2 with the ground-truth rotations, every camera with its next ten", S, (pi, pj, translations(S["rot"], t_ref, pi, pj, 1e-3, 5)), t_ref, P_ref)
B = sphere_scene(2000, 60000, 8, seed=2000)
i, j = np.triu_indices(2000, 1)
pi, pj = i.astype(np.int32), j.astype(np.int32)
bench("sphere scene, all pairs", B, (pi, pj, translations(B["rot"], B["t"], pi, pj, 1e-3, 6)), B["t"], B["P"])
out_path = arg("--out", None)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
