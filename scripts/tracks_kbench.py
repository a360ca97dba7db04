"""timing of the track establishment (xm_build_tracks, xm-code_amd/csrc/xm_tracks.hip) beside the contract's numpy / scipy restatement
(tests/xm_tracks_numpy.py, run_numpy) on the same node; writes profiles/r24_kbench_tracks_split.txt (or --out FILE; profiles/r21_kbench_tracks.txt
is the run from before the device split):
   python scripts/tracks_kbench.py [simple2] [large] [--out FILE] [--calls-only]
simple2: the SIMPLE2-derived case of the tests (93 images, 64 549 features, 261 680 matches of 4 210 pairs, 0.1 % of them wrong); large:
2 000 images x 3 200 features in a ring: 400 tracks start at every image and run over 8 consecutive images, every image is paired with the
next three, a match of two features of a track is listed with probability 0.8, and 0.1 % wrong matches between random features of random
pairs are listed as pairs of their own.  Per scene and policy: 7 calls after 2 warm-up calls; median, smallest and largest wall clock of
the Python call, and the call's own split (xm_tracks_result_t.seconds_*: medians).  "split" (the host splitter) and "split_device"
(XM_TRACKS_SPLIT_DEVICE) are called in turn, one after the other in every repetition, so that both see the same machine; the second row
adds the split's time with its range and what each form took (xm_tracks_split_stats).
--calls-only: three calls per scene and policy and nothing else, for a kernel trace."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, xmamd, xm_tracks_numpy as tn

CALLS_ONLY = "--calls-only" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r24_kbench_tracks_split.txt")
names = [a for a in sys.argv[1:] if not a.startswith("--") and a != OUT] or ["simple2", "large"]
WARM, REPS = 2, 7
POLICIES = ("split", "split_device", "drop", "glomap")
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def ring(n=2000, per_start=400, length=8, reach=3, p_match=0.8, wrong=0.001, seed=7):
    rng = np.random.default_rng(seed)
    nf = per_start * length
    foff = np.arange(n + 1, dtype=np.int64) * nf
    pi, pj, cnt, f1, f2 = [], [], [], [], []
    for d in range(1, reach + 1):
        o, j = np.meshgrid(np.arange(length - d), np.arange(per_start), indexing="ij")
        a = (o * per_start + j).reshape(-1).astype(np.int32); b = ((o + d) * per_start + j).reshape(-1).astype(np.int32)
        for i in range(n):
            on = rng.random(a.size) < p_match
            pi.append(i); pj.append((i + d) % n); cnt.append(int(on.sum())); f1.append(a[on]); f2.append(b[on])
    nw = int(round(wrong * sum(cnt)))
    wk = rng.integers(0, len(pi), nw)
    pi = np.concatenate([np.array(pi), np.array(pi)[wk]]).astype(np.int32); pj = np.concatenate([np.array(pj), np.array(pj)[wk]]).astype(np.int32)
    f1 = np.concatenate(f1 + [rng.integers(0, nf, nw).astype(np.int32)]); f2 = np.concatenate(f2 + [rng.integers(0, nf, nw).astype(np.int32)])
    moff = np.concatenate([[0], np.cumsum(cnt + [1] * nw)]).astype(np.int64)
    xy = np.stack([rng.uniform(0, 1024, n * nf), rng.uniform(0, 768, n * nf)], axis=1)
    return dict(foff=foff, xy=xy, pi=pi, pj=pj, moff=moff, f1=f1, f2=f2, registered=None, options={}, nwrong=nw)


say("Track establishment on the device (xm_build_tracks, xm-code_amd/csrc/xm_tracks.hip), one MI355X.\n"
    "  python scripts/tracks_kbench.py " + " ".join(names) + "\n"
    f"Call times: {REPS} calls per policy after {WARM} warm-up calls; `call` is the wall clock of the Python call (argument marshalling and the\n"
    "output arrays included) as median [smallest .. largest]; index (checks, upload), kernels, split (split: download of the conflicted\n"
    "components' edges, the sequential host split, upload of the labels; split_device: from the first launch of the device split until the\n"
    "labels are final) and download are the call's own figures (xm_tracks_result_t.seconds_*), medians; split and split_device are called in\n"
    "turn.  The restatement is tests/xm_tracks_numpy.py, run_numpy (scipy's connected_components, numpy, a Python loop for the split) on\n"
    "the same node, run once per policy.\n")
for name in names:
    c = tn.simple2_case() if name == "simple2" else ring()
    lim = xmamd.tracks_limits()
    a, k = tn.call_args(c)
    if CALLS_ONLY:
        for p in POLICIES:
            for _ in range(3):
                xmamd.build_tracks(*a, conflict=p, **k)
        continue
    say(f"{name}: {c['foff'].size - 1} images, {int(c['foff'][-1])} features, {c['pi'].size} pairs, {c['f1'].size} matches ({c['nwrong']} wrong)")
    runs = {p: ([], [], []) for p in POLICIES}                 # call times, infos, split statistics
    tabs, refs = {}, {}
    for group in (("split", "split_device"), ("drop",), ("glomap",)):
        for r in range(WARM + REPS):
            for p in group:                                     # the two splits alternate
                t = time.perf_counter(); tabs[p] = xmamd.build_tracks(*a, conflict=p, **k); dt = time.perf_counter() - t
                if r >= WARM:
                    runs[p][0].append(dt); runs[p][1].append(tabs[p].info); runs[p][2].append(xmamd.tracks_split_stats())
    for p in POLICIES:
        ts, infos, stats = runs[p]
        tab = tabs[p]
        word = "split" if p == "split_device" else p
        if word not in refs:
            t0 = time.perf_counter(); r_np = tn.run_numpy(c, word, lim); refs[word] = (r_np, time.perf_counter() - t0)
        ref, t_np = refs[word]
        equal = bool(all(np.array_equal(getattr(tab, f), ref[f]) for f in ("cam", "feat", "track", "label")) and tab.m == ref["m"]
                     and np.array_equal(tab.xy.view(np.uint64), ref["xy"].view(np.uint64)) and {q: tab.info[q] for q in tn.INFO_FIELDS} == ref["info"])
        med = lambda f: 1e3 * float(np.median([i[f] for i in infos]))
        i = tab.info
        say(f"  {p:12s} call {1e3 * np.median(ts):9.2f} ms [{1e3 * min(ts):.2f} .. {1e3 * max(ts):.2f}] = index {med('seconds_index'):.2f} / kernels {med('seconds_kernels'):.2f} / "
            f"split {med('seconds_split'):.2f} / download {med('seconds_download'):.2f}; restatement {1e3 * t_np:.0f} ms; every output equal: {equal}")
        if p == "split_device":
            sp = [1e3 * q["seconds_split"] for q in infos]
            same = bool(all(np.array_equal(getattr(tab, f), getattr(tabs["split"], f)) for f in ("cam", "feat", "track", "label"))
                        and np.array_equal(tab.xy.view(np.uint64), tabs["split"].xy.view(np.uint64)) and all(q == stats[0] for q in stats))
            z = stats[0]
            say(f"         split {np.median(sp):.2f} ms [{min(sp):.2f} .. {max(sp):.2f}]; components by form: {z['wave']} wavefront / {z['group']} workgroup / {z['host']} host; "
                f"raw edges {z['edges_device']} to the device / {z['edges_host']} to the host; every output equal to the split row's, every call the same statistics: {same}")
        if p == "split":
            sp = [1e3 * q["seconds_split"] for q in infos]
            say(f"         split {np.median(sp):.2f} ms [{min(sp):.2f} .. {max(sp):.2f}]")
        say(f"         {i['components']} components, {i['components_conflicted']} conflicted ({i['rows_conflicted']} features, {i['edges_split']} distinct edges split, "
            f"{i['unions_refused']} unions refused); {tab.m} tracks, {tab.cam.size} rows; {i['rounds']} hooking rounds; images by kernel size "
            f"{i['images_small']} / {i['images_large']} / {i['images_workspace']}, at most {i['max_touched']} touched features in one")
if not CALLS_ONLY:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
