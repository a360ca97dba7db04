"""dense Q built on the device from the observation list (xm_tuning_t.schur_dense_q) against the matrix-free context of the same build:
set-up time by phase, time per o = 3 Hessian product (HIP events around the launches of a rank-3 solve), certified solve both ways;
   python scripts/kbench_schur_dense.py [simple2] [N ...]        default: simple2 500 1778 4000 8000
A scene is tl.gen_scene(N, 112 N, 6, seed=2) (112 landmarks per camera: the Venice-size scene of the tests at N = 1778).  The phase lines
("schur set-up:", "spd_inverse:", "schur dense Q:") are the library's own trace on stderr (schur_trace = 1): run with 2>&1."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, xmamd, xm_testlib as tl
CASES = sys.argv[1:] or ["simple2", "500", "1778", "4000", "8000"]
MAX_TIME = float(os.environ.get("XM_KB_MAX_TIME", "120"))


def say(*a):
    print(*a, flush=True)


def one(name, obs, tuning):
    say(f"-- {name}: {'dense Q from observations (schur_dense_q = 1)' if tuning.get('schur_dense_q') else 'matrix-free (factor chain)'}")
    t0 = time.time(); ctx = xmamd.Context(obs=obs, tuning=dict(tuning, schur_trace=1)); t_setup = time.time() - t0
    t0 = time.time(); ctx.set_edge_weights(obs[3]); t_again = time.time() - t0          # what a re-weighting costs: everything but the host lists
    t0 = time.time(); R, s, i = ctx.solve(5, 1e-6, 0.0, max_time=MAX_TIME, flags=xmamd.FLAG_PROFILE_QW); t_solve = time.time() - t0
    kind = ctx.product_kind(3)
    _, _, i3 = ctx.solve(3, 1e-6, 0.0, max_time=MAX_TIME, mode=xmamd.MODE_RANK3, flags=xmamd.FLAG_PROFILE_QW)   # the rank-3 stage alone: o = 3 products only
    ctx.close()
    qw_us = i["qw_ms_sum"] / max(i["qw_ms_count"], 1) * 1e3
    o3_us = i3["qw_ms_sum"] / max(i3["qw_ms_count"], 1) * 1e3
    say(f"   context {t_setup * 1e3:9.1f} ms (lists on the host + everything below), re-weighting {t_again * 1e3:9.1f} ms | product kind {kind}, "
        f"o = 3 Hessian product {o3_us:8.1f} us (mean over the staircase's levels {qw_us:8.1f} us) | solve {t_solve * 1e3:9.1f} ms: rank {i['rank']} status {i['status']} tcg {i['tcg_iters']} "
        f"({i['tcg_iters'] / max(i['tr_seconds'], 1e-9):.0f} it/s), sym_product {i['sym_product']}, bytes per product {i['qw_bytes'] / 1e6:.1f} MB")
    return dict(setup=t_again, qw=o3_us, solve=t_solve, rank=i["rank"], status=i["status"], R=R, s=s)


for case in CASES:
    if case == "simple2":
        Z = np.load(os.path.join(ROOT, "tests", "golden", "simple2", "obs.npz"))
        obs = (Z["cam"], Z["lm"], Z["p"], Z["w"].reshape(-1)); N = int(Z["cam"].max()) + 1; M = int(Z["lm"].max()) + 1
    else:
        N = int(case)
        S = tl.gen_scene(N, 112 * N, 6, seed=2)
        obs = (S["cam"], S["lm"], S["p"], S["w"]); M = S["m"]
    say(f"== {case}: {N} cameras, {M} landmarks, {obs[0].size} observations; dense Q {72.0 * N * N / 1e6:.1f} MB")
    mf = one(case, obs, {})
    dq = one(case, obs, dict(schur_dense_q=1))
    extra = dq["setup"] - mf["setup"]
    gain = (mf["qw"] - dq["qw"]) * 1e-6
    say(f"   o = 3 Hessian product: matrix-free {mf['qw']:.1f} us / dense {dq['qw']:.1f} us = {mf['qw'] / max(dq['qw'], 1e-9):.2f} x; solve {mf['solve'] * 1e3:.1f} / {dq['solve'] * 1e3:.1f} ms = "
        f"{mf['solve'] / max(dq['solve'], 1e-9):.2f} x; building Q costs {extra * 1e3:.1f} ms more per (re-)weighting: pays from "
        f"{(extra / gain) if gain > 0 else float('inf'):.0f} products on; rotation parity of the two solutions {tl.rotation_parity(dq['R'], dq['s'], mf['R'], mf['s']) if dq['rank'] == mf['rank'] else float('nan'):.2e}")
