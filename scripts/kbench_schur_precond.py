"""Jacobi (xm_tuning_t.schur_solver = 2) against the two-level preconditioner (schur_solver = 3) of the matrix-free CG form: set-up time,
ms per product and inner CG iterations per product, on a sequential capture and on a random co-visibility scene;
   python scripts/kbench_schur_precond.py [--seq N] [--scene N M views] [--products K]
(default: a 20 000-camera sequential scene and the Final-13682-size gen_scene(13682, 800000, 8)).  Products are xm_ctx_qw calls (host to
host, inner tolerance 1e-13: the gradient / cost / certificate kind); o = 3."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import xmamd
import xm_seqscene as sq
import xm_testlib as tl


def arg(name, n, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        return [int(x) for x in sys.argv[i + 1:i + 1 + n]]
    return default


K = arg("--products", 1, [5])[0]
scenes = []
if "--scene" not in sys.argv or "--seq" in sys.argv:
    (n,) = arg("--seq", 1, [20000])
    scenes.append((f"sequential {n} cameras (20 landmarks per camera, 2-5 views each)", lambda n=n: sq.gen_sequential(n, seed=n)))
if "--seq" not in sys.argv or "--scene" in sys.argv:
    n, m, v = arg("--scene", 3, [13682, 800000, 8])
    scenes.append((f"gen_scene({n}, {m}, {v})", lambda n=n, m=m, v=v: tl.gen_scene(n, m, v, seed=n)))

for name, make in scenes:
    S = make()
    obs = (S["cam"], S["lm"], S["p"], S["w"])
    N = S["n"]
    W = np.random.default_rng(0).standard_normal((3 * N, 3))
    print(f"{name}: {S['cam'].size} observations", flush=True)
    Y = {}
    for solver in (2, 3):
        t0 = time.time()
        ctx = xmamd.Context(obs=obs, tuning=dict(schur_solver=solver))
        t_setup = time.time() - t0
        Y[solver] = ctx.qw(W)                                   # warm-up (first batch guess, allocations)
        a = ctx.schur_info()
        t0 = time.time()
        for _ in range(K):
            ctx.qw(W)
        ms = (time.time() - t0) * 1e3 / K
        b = ctx.schur_info()
        ctx.close()
        it = (b["inner_iters"] - a["inner_iters"]) / K
        print(f"  {b['precond']:9s} set-up {t_setup:7.2f} s  {ms:9.2f} ms per product  {it:7.1f} inner iterations per product  "
              f"capped {b['capped'] - a['capped']}/{K}  last relres {b['last_relres']:.1e}  aggregates {b['aggregates']}", flush=True)
    print(f"  products two-level vs Jacobi: rel {tl.rel_fro(Y[3], Y[2]):.2e}", flush=True)
