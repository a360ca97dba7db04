"""timing of the pairwise relative-rotation filter (xm_pair_filter, xm-code_amd/csrc/xm_pair.hip) beside its numpy / scipy restatement
(tests/xm_pair_numpy.py) on the same node; writes profiles/r16_kbench_pair_filter.txt (or --out FILE):
   python scripts/kbench_pair_filter.py [simple2] [scene500] [scene2000] [--out FILE] [--calls-only]
simple2: the reference's SIMPLE2 list with 2 % of the points perturbed, all 4 278 camera pairs (tests/golden/pair, case a); scene500 /
scene2000: gen_scene with 500 / 2 000 cameras, 2 % of the points perturbed, every pair that shares at least 20 landmarks, rotations from the
scene's ground truth.  Per scene: the call (median of 5 after a warm-up) split into index + upload, kernels and download as the call itself
reports them, pairs per second, and the restatement -- on all pairs where that takes seconds, else on a random sample of the pairs, scaled.
--calls-only: three calls per scene and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats -- python ... --calls-only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, xmamd, xm_testlib as tl, xm_pair_numpy as pn
from scipy.sparse import coo_matrix

CALLS_ONLY = "--calls-only" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r16_kbench_pair_filter.txt")
names = [a for a in sys.argv[1:] if not a.startswith("--") and a != OUT] or ["simple2", "scene500", "scene2000"]
SAMPLE = 4000          # pairs of the restatement's sample on the generated scenes
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def scene(name):
    if name == "simple2":
        return pn.case_a_inputs()
    N, M, views = {"scene500": (500, 20000, 30), "scene2000": (2000, 40000, 60)}[name]
    S = tl.gen_scene(N, M, views, seed=N)
    rng = np.random.default_rng(N + 1)
    p = S["p"].copy()
    hit = rng.random(p.shape[0]) < 0.02
    p[hit] *= (1.0 + 0.3 * rng.standard_normal(int(hit.sum())))[:, None]
    V = coo_matrix((np.ones(S["cam"].size, dtype=np.int32), (S["cam"], S["lm"])), shape=(S["n"], S["m"])).tocsr()
    common = (V @ V.T).toarray()
    pi, pj = np.nonzero(np.triu(common >= 20, 1))
    R = np.einsum("kba,kbc->kac", S["R_star"][pj], S["R_star"][pi])      # p_c = R_c^T (P - t_c): dst ~ R_j^T R_i src
    return dict(cam=S["cam"], lm=S["lm"], p=p, n=S["n"], m=S["m"], pi=pi.astype(np.int32), pj=pj.astype(np.int32), R=R)


say("Pairwise relative-rotation filter on the device (xm_pair_filter, xm-code_amd/csrc/xm_pair.hip), one MI355X.\n"
    "  python scripts/kbench_pair_filter.py " + " ".join(names) + "\n"
    "Call times are medians of 5 calls after one warm-up call: `call` is the wall clock of the Python call (argument marshalling included);\n"
    "index + upload (the host's index of the list by camera and landmark, the check for a pair named twice, allocation and copies), kernels\n"
    "and download are the call's own figures (xm_pair_result_t.seconds_*).  The restatement is tests/xm_pair_numpy.py (numpy, scipy.stats.\n"
    "trim_mean, np.percentile; one Python pass per pair over the same camera index) on the same node.  The reference's own loop\n"
    "(5_test_ceres.py:316-431, dense rows of length M per pair) was NOT run on this node: 3.6-4.9 s for the simple2 case is a figure from\n"
    "the build machine's CPU.\n")
for name in names:
    c = scene(name)
    run = lambda: xmamd.pair_filter(c["cam"], c["lm"], c["p"], c["pi"], c["pj"], c["R"], c["n"], c["m"])
    if CALLS_ONLY:
        for _ in range(3):
            run()
        continue
    run()
    ts, infos = [], []
    for _ in range(5):
        t = time.perf_counter(); plan = run(); ts.append(time.perf_counter() - t); infos.append(plan.info)
    med = lambda k: 1e3 * float(np.median([i[k] for i in infos]))
    t_call = 1e3 * float(np.median(ts))
    npairs = c["pi"].size
    if npairs <= 2 * SAMPLE:
        t0 = time.perf_counter(); ref = pn.pair_filter_numpy(c["cam"], c["lm"], c["p"], c["pi"], c["pj"], c["R"], c["n"], c["m"]); t_np = time.perf_counter() - t0
        same = bool(np.array_equal(plan.count, ref["count"]) and np.array_equal(plan.stats["n_flagged"], ref["stats"]["n_flagged"]))
        how = f"numpy / scipy restatement, all pairs {1e3 * t_np:10.1f} ms; counts equal to it: {same}, decision margin {ref['margin']:.1e}"
    else:
        pick = np.sort(np.random.default_rng(0).choice(npairs, SAMPLE, replace=False))
        t0 = time.perf_counter(); ref = pn.pair_filter_numpy(c["cam"], c["lm"], c["p"], c["pi"][pick], c["pj"][pick], c["R"][pick], c["n"], c["m"])
        t_np = time.perf_counter() - t0
        same = all(np.array_equal(plan.stats[f][pick], ref["stats"][f]) for f in ("n_joint", "n_kept", "n_flagged", "status"))
        how = (f"numpy / scipy restatement on {SAMPLE} of the pairs {1e3 * t_np:10.1f} ms, scaled to all pairs {t_np * npairs / SAMPLE:8.1f} s; the sample's integer "
               f"stats equal to it: {same}, decision margin {ref['margin']:.1e}")
    i = plan.info
    say(f"{name}: {c['cam'].size} observations, {c['n']} cameras, {c['m']} landmarks, {npairs} pairs -> {i['pairs_used']} used, {i['pairs_skipped']} with too few "
        f"common landmarks, {i['pairs_degenerate']} degenerate, largest joint set {i['max_joint']}, {i['pairs_on_workspace_path']} on the workspace path, "
        f"{i['nobs_flagged']} observations flagged\n"
        f"    call {t_call:9.2f} ms = index + upload {med('seconds_index'):8.2f} + kernels {med('seconds_kernels'):8.2f} + download {med('seconds_download'):8.2f} ms "
        f"(+ marshalling) | {npairs / (t_call * 1e-3):12.0f} pairs/s by the call, {npairs / max(med('seconds_kernels') * 1e-3, 1e-9):12.0f} by the kernels\n"
        f"    {how}")
if not CALLS_ONLY:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
