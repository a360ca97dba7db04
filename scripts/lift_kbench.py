"""timing of the depth lift (xm_lift_observations, xm-code_amd/csrc/xm_lift.hip) with device maps and with host maps, beside its numpy
restatement (tests/xm_lift_numpy.py) on the same node; writes profiles/r20_kbench_lift.txt (or --out FILE):
   python scripts/lift_kbench.py [simple2] [large] [--out FILE] [--calls-only]
simple2: 93 cameras with the per-camera row counts of the reference's SIMPLE2 list (tests/golden/simple2/obs.npz, 64 549 rows); large:
2 000 cameras x 3 200 rows.  Maps are 768 x 1024 float32 (depths on a 2^-10 grid, confidences in (0, 1)); the cameras share a pool of 16
distinct depth and confidence maps (2 000 distinct ones would be 12.6 GB), which changes nothing for the call: it gets one pointer per
camera.  2 % of the rows are named twice, pixels are uniform over the image (so about 4.5 % fall inside the border of 10), rows shuffled.
Per scene: 9 calls of each transport after 2 warm-up calls, alternating; median, smallest and largest wall clock of the Python call, and the
call's own split (xm_lift_result_t.seconds_*: medians).  The device -> host copy of one depth and one confidence map, which the reference
pays per camera before it can sample, is timed beside it.
--calls-only: three calls per scene and transport and nothing else, for a kernel trace."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, xmamd, xm_lift_numpy as ln

CALLS_ONLY = "--calls-only" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r20_kbench_lift.txt")
names = [a for a in sys.argv[1:] if not a.startswith("--") and a != OUT] or ["simple2", "large"]
H, W, POOL, WARM, REPS = 768, 1024, 16, 2, 9
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def scene(name):
    if name == "simple2":
        sizes = np.bincount(np.load(os.path.join(ROOT, "tests", "golden", "simple2", "obs.npz"))["cam"])
    else:
        sizes = np.full(2000, 3200)
    rng = np.random.default_rng(sizes.size)
    n, m = sizes.size, int(sizes.max()) * 4
    cam = np.repeat(np.arange(n), sizes)
    lm = np.concatenate([rng.choice(m, k, replace=False) for k in sizes])
    xy = np.stack([rng.uniform(0.0, W, cam.size), rng.uniform(0.0, H, cam.size)], axis=1)
    twin = rng.choice(cam.size, cam.size // 50, replace=False)
    cam, lm = np.concatenate([cam, cam[twin]]), np.concatenate([lm, lm[twin]])
    xy = np.concatenate([xy, np.stack([rng.uniform(0.0, W, twin.size), rng.uniform(0.0, H, twin.size)], axis=1)])
    perm = rng.permutation(cam.size)
    pool_d = [ln.grid_depth(rng, H, W) for _ in range(POOL)]
    pool_c = [rng.uniform(0.05, 1.0, (H, W)).astype(np.float32) for _ in range(POOL)]
    return dict(cam=cam[perm].astype(np.int32), lm=lm[perm].astype(np.int32), xy=xy[perm], depth=[pool_d[c % POOL] for c in range(n)],
                conf=[pool_c[c % POOL] for c in range(n)], pool=(pool_d, pool_c), K=ln.intrinsics(n, [(H, W)] * n), n=n, m=m)


say("Depth lift on the device (xm_lift_observations, xm-code_amd/csrc/xm_lift.hip), one MI355X.\n"
    "  python scripts/lift_kbench.py " + " ".join(names) + "\n"
    f"Call times: {REPS} calls of each transport after {WARM} warm-up calls, the two transports alternating; `call` is the wall clock of the Python\n"
    "call (argument marshalling and the inversion of K included) as median [smallest .. largest]; index (checks, sampling of host maps,\n"
    "upload, binning), kernels and download are the call's own figures (xm_lift_result_t.seconds_*), medians.  The restatement is\n"
    "tests/xm_lift_numpy.py (numpy: lexsort, fancy indexing, np.sort per camera) on the same node, host maps, run once.\n")
for name in names:
    c = scene(name)
    lim = xmamd.lift_limits()
    dev_d = [(xmamd.DevArray(D), H, W) for D in c["pool"][0]]; dev_c = [(xmamd.DevArray(D), H, W) for D in c["pool"][1]]
    on_dev = ([dev_d[i % POOL] for i in range(c["n"])], [dev_c[i % POOL] for i in range(c["n"])])
    run = {"device maps": lambda: xmamd.lift_observations(c["cam"], c["lm"], c["xy"], on_dev[0], on_dev[1], c["K"], m=c["m"]),
           "host maps": lambda: xmamd.lift_observations(c["cam"], c["lm"], c["xy"], c["depth"], c["conf"], c["K"], m=c["m"])}
    if CALLS_ONLY:
        for f in run.values():
            for _ in range(3):
                f()
        continue
    ts = {k: [] for k in run}; infos = {k: [] for k in run}; plans = {}
    for r in range(WARM + REPS):
        for k, f in run.items():
            t = time.perf_counter(); plan = f(); dt = time.perf_counter() - t
            if r >= WARM:
                ts[k].append(dt); infos[k].append(plan.info)
            plans[k] = plan
    a, b = plans["device maps"], plans["host maps"]
    same_bits = all(np.array_equal(getattr(a, f).view(np.uint8), getattr(b, f).view(np.uint8)) for f in ("cam", "lm", "row", "p", "w", "threshold"))
    t0 = time.perf_counter(); ref = ln.lift_numpy(c["cam"], c["lm"], c["xy"], c["depth"], c["conf"], c["K"], m=c["m"], limits=lim); t_np = time.perf_counter() - t0
    equal = bool(all(np.array_equal(getattr(a, f), ref[f]) for f in ("cam", "lm", "row", "w")) and np.all(np.abs(a.p - ref["p"]) <= ref["p_bound"])
                 and np.array_equal(a.threshold.view(np.uint64), ref["threshold"].view(np.uint64)) and {k: a.info[k] for k in ln.INFO_FIELDS} == ref["info"])
    tc = []
    for _ in range(WARM + REPS):
        t = time.perf_counter(); dev_d[0][0].get(np.float32); dev_c[0][0].get(np.float32); tc.append(time.perf_counter() - t)
    t_copy = 1e3 * float(np.median(tc[WARM:]))
    i = a.info
    say(f"{name}: {c['cam'].size} rows, {c['n']} cameras, {H} x {W} maps -> {a.cam.size} observations; dropped: {i['rows_duplicate']} duplicate, {i['rows_border']} border, "
        f"{i['rows_depth']} depth; cameras by kernel size: {i['cams_small']} small, {i['cams_large']} large, {i['cams_workspace']} workspace; most rows of a camera {i['max_rows']}")
    for k in run:
        med = lambda f: 1e3 * float(np.median([x[f] for x in infos[k]]))
        t = 1e3 * np.array(ts[k])
        say(f"    {k:12s} call {np.median(t):9.2f} ms [{t.min():9.2f} .. {t.max():9.2f}] = index {med('seconds_index'):8.2f} + kernels {med('seconds_kernels'):8.2f} + download "
            f"{med('seconds_download'):8.2f} ms (+ marshalling) | {c['cam'].size / (np.median(t) * 1e-3):12.0f} rows/s by the call")
    say(f"    the two transports give the same bits: {same_bits}\n"
        f"    numpy restatement {1e3 * t_np:10.1f} ms; every output equal to it (p within its bound): {equal}\n"
        f"    device -> host copy of one depth and one confidence map: {t_copy:.3f} ms, so {1e-3 * t_copy * c['n']:.3f} s for the {c['n']} cameras of this scene")
    for d, _, _ in dev_d + dev_c:
        d.free()
if not CALLS_ONLY:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
