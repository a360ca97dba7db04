"""timing of the two-view match verification and view-graph pruning (xm_view_graph_filter, xm-code_amd/csrc/xm_viewgraph.hip) beside the
contract's numpy restatement (tests/xm_viewgraph_numpy.py, run_numpy) on the same node; writes profiles/r22_kbench_viewgraph.txt (or --out FILE):
   python scripts/viewgraph_kbench.py [simple2] [large] [--out FILE] [--calls-only]
simple2: the recorded SIMPLE2-derived case of the tests (93 images, 64 549 features, 261 680 matches of 4 210 pairs; E, F and H pairs); pass
B is fed with pass A's output and the true rotations.  large: the ring of scripts/tracks_kbench.py (2 000 images x 3 200 features, every
image paired with the next three, 11.5 M matches, 0.1 % wrong matches listed as pairs of their own) with a geometry under it: a track's
feature moves 12 px along x from image to image (0.3 px noise), all cameras share K (f = 800) and the identity rotation, so a pair d images
apart is an x-translation: its E, its F and its H are known, and the pairs take the three models in turn; the one-match pairs are NONE.
Pass B gets identity rotations and Rrel turned by 20 degrees in 2 % of the pairs.  Per scene and pass: 7 calls after 2 warm-up calls;
median, smallest and largest wall clock of the Python call, and the call's own split (xm_vg_result_t.seconds_*: medians).
--calls-only: three calls per scene and pass and nothing else, for a kernel trace."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, xmamd, xm_viewgraph_numpy as vn

CALLS_ONLY = "--calls-only" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r22_kbench_viewgraph.txt")
names = [a for a in sys.argv[1:] if not a.startswith("--") and a != OUT] or ["simple2", "large"]
WARM, REPS = 2, 7
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def ring(n=2000, per_start=400, length=8, reach=3, p_match=0.8, wrong=0.001, seed=7, step=12.0, focal=800.0):
    rng = np.random.default_rng(seed)
    nf = per_start * length
    foff = np.arange(n + 1, dtype=np.int64) * nf
    pi, pj, cnt, f1, f2, gap = [], [], [], [], [], []
    for d in range(1, reach + 1):
        o, j = np.meshgrid(np.arange(length - d), np.arange(per_start), indexing="ij")
        a = (o * per_start + j).reshape(-1).astype(np.int32); b = ((o + d) * per_start + j).reshape(-1).astype(np.int32)
        for i in range(n):
            on = rng.random(a.size) < p_match
            pi.append(i); pj.append((i + d) % n); cnt.append(int(on.sum())); f1.append(a[on]); f2.append(b[on]); gap.append(d)
    real = len(pi)
    nw = int(round(wrong * sum(cnt)))
    wk = rng.integers(0, real, nw)
    pi = np.concatenate([np.array(pi), np.array(pi)[wk]]).astype(np.int32); pj = np.concatenate([np.array(pj), np.array(pj)[wk]]).astype(np.int32)
    gap = np.concatenate([np.array(gap), np.array(gap)[wk]]).astype(np.float64)
    f1 = np.concatenate(f1 + [rng.integers(0, nf, nw).astype(np.int32)]); f2 = np.concatenate(f2 + [rng.integers(0, nf, nw).astype(np.int32)])
    moff = np.concatenate([[0], np.cumsum(cnt + [1] * nw)]).astype(np.int64)
    # feature (o, j) of image i is the o-th view of the track that starts at image i - o
    base = np.stack([rng.uniform(100, 900, (n, per_start)), rng.uniform(50, 700, (n, per_start))], axis=2)
    xy = np.zeros((n, length, per_start, 2))
    for o in range(length):
        xy[:, o] = np.roll(base, o, axis=0) + [o * step, 0.0]
    xy = xy.reshape(n * nf, 2) + rng.normal(scale=0.3, size=(n * nf, 2))
    npairs = pi.size
    model = np.where(np.arange(npairs) < real, 1 + np.arange(npairs) % 3, vn.NONE).astype(np.int32)
    K = np.array([[focal, 0.0, 512.0], [0.0, focal, 384.0], [0.0, 0.0, 1.0]])
    Kinv = np.linalg.inv(K)
    Rrel = np.tile(np.eye(3), (npairs, 1, 1)); trel = np.tile([1.0, 0.0, 0.0], (npairs, 1))
    FH = np.tile(np.eye(3), (npairs, 1, 1))
    FH[model == vn.F_] = Kinv.T @ vn.essential(np.eye(3), [1.0, 0.0, 0.0]) @ Kinv
    FH[model == vn.H_, 0, 2] = gap[model == vn.H_] * step
    c = dict(foff=foff, xy=xy, focal=np.full(n, focal), Kinv=np.tile(Kinv, (n, 1, 1)), bearing=None, pi=pi, pj=pj, model=model, Rrel=Rrel, trel=trel, FH=FH,
             valid_in=None, registered_in=None, rot=None, moff=moff, f1=f1, f2=f2, options={})
    c["rot_true"] = np.tile(np.eye(3), (n, 1, 1))
    turned = np.flatnonzero(rng.random(npairs) < 0.02)
    c["Rrel_b"] = Rrel.copy(); c["Rrel_b"][turned] = vn.rot_axis([0.1, 1.0, 0.2], 20.0)
    return c


def run(c):
    a, k = vn.call_args(c)
    return xmamd.view_graph_filter(*a, **k)


def as_result(g):
    return dict(inlier=g.inlier, pair_inliers=g.pair_inliers, pair_status=g.pair_status, registered=g.registered, moff_out=g.matches[0], f1_out=g.matches[1],
                f2_out=g.matches[2])


say("Two-view match verification and view-graph pruning on the device (xm_view_graph_filter, xm-code_amd/csrc/xm_viewgraph.hip), one MI355X.\n"
    "  python scripts/viewgraph_kbench.py " + " ".join(names) + "\n"
    f"Call times: {REPS} calls per pass after {WARM} warm-up calls; `call` is the wall clock of the Python call (argument marshalling and the\n"
    "output arrays included) as median [smallest .. largest]; index (checks, lists, upload), kernels and download are the call's own figures\n"
    "(xm_vg_result_t.seconds_*), medians.  The restatement is tests/xm_viewgraph_numpy.py, run_numpy (numpy, a Python union-find) on the same\n"
    "node, run once per pass.  Pass A scores (XM_VG_SCORE); pass B reads pass A's compacted matches and applies the rotation rule.\n")
lim = xmamd.view_graph_limits()
for name in names:
    a = vn.simple2_case() if name == "simple2" else ring()
    ga = run(a)
    b = vn.next_pass(dict(a, Rrel=a.get("Rrel_b", a["Rrel"])), as_result(ga), a["rot_true"])
    if CALLS_ONLY:
        for c in (a, b):
            for _ in range(3):
                run(c)
        continue
    say(f"{name}: {a['foff'].size - 1} images, {int(a['foff'][-1])} features, {a['pi'].size} pairs, {a['f1'].size} matches")
    for what, c in (("pass A", a), ("pass B", b)):
        ts, infos = [], []
        for r in range(WARM + REPS):
            t = time.perf_counter(); g = run(c); dt = time.perf_counter() - t
            if r >= WARM:
                ts.append(dt); infos.append(g.info)
        t0 = time.perf_counter(); ref = vn.run_numpy(c, lim); t_np = time.perf_counter() - t0
        got = as_result(g)
        equal = bool(all(np.array_equal(got[f], ref[f]) for f in got) and {q: g.info[q] for q in vn.INFO_FIELDS} == ref["info"])
        med = lambda f: 1e3 * float(np.median([i[f] for i in infos]))
        i = g.info
        say(f"  {what} call {1e3 * np.median(ts):9.2f} ms [{1e3 * min(ts):.2f} .. {1e3 * max(ts):.2f}] = index {med('seconds_index'):.2f} / kernels {med('seconds_kernels'):.2f} / "
            f"download {med('seconds_download'):.2f}; restatement {1e3 * t_np:.0f} ms; every output equal: {equal}")
        say(f"         {i['matches']} matches, {i['inliers']} inliers, {i['matches_out']} written; pairs E / F / H / NONE {i['pairs_E']} / {i['pairs_F']} / {i['pairs_H']} / "
            f"{i['pairs_none']}; valid {i['pairs_valid']}, invalid at input {i['pairs_invalid_in']}, few inliers {i['pairs_few_inliers']}, low ratio {i['pairs_low_ratio']}, "
            f"rotation {i['pairs_rotation']}, outside {i['pairs_outside']}; {i['components']} components, the largest of {i['largest']} images; {i['rounds']} hooking rounds; "
            f"pairs by kernel form {i['pairs_wave']} / {i['pairs_group']} / {i['pairs_workspace']}, at most {i['max_matches']} matches in one")
if not CALLS_ONLY:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
