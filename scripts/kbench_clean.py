"""timing of observation cleaning (xm_clean_observations / xm_ctx_clean_observations, xm-code_amd/csrc/xm_clean.hip) beside its numpy / scipy
restatement (tests/xm_clean_numpy.py) on the same node:
   python scripts/kbench_clean.py [simple2] [final] [chain] [--calls-only]
simple2: the reference's SIMPLE2 list after the recorded XM^2 filter; final: gen_scene at Final-13682 size (13 682 cameras, 800 000 landmarks,
about 6.4 M observations) plus a detached group and a weak camera; chain: a sequential capture of 20 000 cameras with shuffled numbering.
Per scene: rounds, the list call (with the upload of its arrays timed separately), the context call (no upload), the restatement.
--calls-only: three calls of each entry point and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats -- python ... --calls-only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, xmamd, xm_testlib as tl, xm_clean_numpy as cn

CALLS_ONLY = "--calls-only" in sys.argv
names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["simple2", "final", "chain"]


def scene(name):
    """-> cam, lm, p, w at creation, w for the cleaning (None: the same), n, m, thresholds, tuning of the context"""
    if name == "simple2":
        c = cn.load_case(os.path.join(ROOT, "tests", "golden"), "a")
        o = np.load(os.path.join(ROOT, "tests", "golden", "simple2", "obs.npz"))
        return c["cam"], c["lm"], o["p"], o["w"], c["w"], c["n"], c["m"], (10, 1), None
    if name == "final":
        S = tl.gen_scene(13682, 800000, 8, seed=13682)
        # what cleaning is for: a camera with 10 observations that holds a detached group of 30 cameras to the scene
        rng = np.random.default_rng(1)
        n, m = S["n"], S["m"]
        gc = np.repeat(np.arange(n + 1, n + 31), 40); gl = m + rng.integers(0, 200, gc.size)
        _, idx = np.unique(gc.astype(np.int64) * 1000 + (gl - m), return_index=True)
        gc, gl = gc[idx], gl[idx]
        wc = np.full(10, n); wl = np.concatenate([rng.choice(m, 5, replace=False), m + np.arange(5)])
        cam = np.concatenate([S["cam"], wc, gc]).astype(np.int32); lm = np.concatenate([S["lm"], wl, gl]).astype(np.int32)
        p = np.concatenate([S["p"], rng.standard_normal((cam.size - S["cam"].size, 3))]); w = np.concatenate([S["w"], np.ones(cam.size - S["w"].size)])
        return cam, lm, p, w, None, n + 31, m + 200, (10, 1), dict(schur_solver=2)
    if name == "chain":
        cam, lm, n, m = cn.chain_scene(20000, 5)
        rng = np.random.default_rng(2)
        return cam, lm, rng.standard_normal((cam.size, 3)), rng.uniform(0.5, 1.5, cam.size), None, n, m, (0, 1), dict(schur_solver=2)
    raise SystemExit("unknown scene " + name)


def best(f, reps=7):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts)), r


for name in names:
    cam, lm, p, w0, wc, n, m, thr, tuning = scene(name)
    ctx = xmamd.Context(obs=(cam, lm, p, w0), n=n, tuning=tuning)
    if wc is not None:
        ctx.set_edge_weights(wc)
    wl = w0 if wc is None else wc
    if CALLS_ONLY:
        for _ in range(3):
            xmamd.clean_observations(cam, lm, wl, n, m, *thr); ctx.clean_observations(*thr)
        ctx.close()
        continue
    t_list, plan = best(lambda: xmamd.clean_observations(cam, lm, wl, n, m, *thr))
    t_ctx, plan_c = best(lambda: ctx.clean_observations(*thr))
    live = (wl > 0).astype(np.uint8)

    def upload():   # the bytes the list call sends: two int32 and a flag per observation
        bufs = [xmamd.DevArray(a) for a in (cam, lm, live)]
        for b in bufs:
            b.free()
    t_up, _ = best(upload)
    t0 = time.perf_counter(); ref = cn.clean_numpy(cam, lm, wl, n, m, *thr); t_np = 1e3 * (time.perf_counter() - t0)
    ok = all(np.array_equal(getattr(q, k)[: ref[k].size], ref[k]) for q in (plan, plan_c) for k in ("keep", "cam_index")) and \
        np.array_equal(plan.lm_index, ref["lm_index"])
    i = plan.info
    print(f"{name}: {cam.size} observations, {n} cameras, {m} landmarks, thresholds {thr} -> {i['nobs_new']} / {i['n_new']} / {i['m_new']} kept, "
          f"{i['components']} components, rounds {i['rounds']} (context call {plan_c.info['rounds']}), equal to the restatement: {ok}\n"
          f"    list call {t_list:9.2f} ms (allocating and uploading its {cam.size * 9 / 1e6:.1f} MB alone: {t_up:.2f} ms) | context call {t_ctx:9.2f} ms | "
          f"numpy / scipy restatement {t_np:9.1f} ms", flush=True)
    ctx.close()
