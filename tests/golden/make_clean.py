#!/usr/bin/env python3
"""tests/golden/clean/*.npz: what the reference's observation cleaning returns, recorded by EXECUTING the reference (read from
/root/reference at generation time, never copied into this repository).  Runs only in the build container (needs networkx).

Two sequences per case:
  "10_1"  utils/checkconnection.py:checklandmarks, imported and called unchanged (thresholds 10 and 1, 5_test_ceres.py:482 / :578)
  "0_1"   the inline variant of 2_test_creatematrix.py (from `def delete_thereshold` to the line in front of `create_matrix(...)`), executed
          on the case's variables.  Its indices_all is not recorded: the script composes the exchanged index map with itself (lines 101-105),
          which is the identity after an exchange and no longer describes the rows it kept; and it has no stage that drops a camera
          emptied by the landmark threshold.  Kept rows, kept landmarks and their numbering are what both sequences define alike.

Per case and sequence: keep_* (the kept-row mask over the INPUT list, np.packbits), lm_index_* (new number of every landmark, -1 = dropped),
counts_* (cameras, landmarks, observations that remain), sha_* (SHA-256 of the returned arrays edges - 1 as int64, landmarks, weights as
float64, in that order -- what CleanPlan.apply must reproduce); for "10_1" also indices_all.  Cases (b)-(d) carry their input (cam, lm, n,
m; every observation live; points and weights: tests/xm_clean_numpy.py:fixture_points); (a) is tests/golden/simple2/obs.npz after the
recorded XM^2 filter (xm2.npz: error <= its 90-percentile).

  a   SIMPLE2 after the filter                                                        58 065 observations, 93 cameras, 5 998 landmarks
  b   12 cameras / 77 landmarks, shuffled; every stage acts: a main component of 6 cameras, a second of 3, a camera with exactly 10
      observations, five single-view landmarks, a camera whose 11 observations are all single-view, an unobserved camera and landmark
  c1  two components with the same number of nodes, the first one's observations first
  c2  the same with the second one's observations first (the tie goes to the earliest observation)
  d   a (camera, landmark) pair named twice lifts the landmark from one observation to two
"""
import hashlib
import os
import sys

import numpy as np
import networkx as nx

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REF)
from utils.checkconnection import checklandmarks   # noqa: E402  (the reference's function, unchanged)
from xm_clean_numpy import fixture_points          # noqa: E402

src = open(os.path.join(REF, "2_test_creatematrix.py")).read().splitlines()
first = next(i for i, l in enumerate(src) if l.startswith("def delete_thereshold"))
last = next(i for i, l in enumerate(src) if l.startswith("# interface to create the matrix"))
INLINE = "\n".join(src[first:last])
print("executing %s lines %d-%d for the (0, 1) sequence" % (os.path.join(REF, "2_test_creatematrix.py"), first + 1, last))


def sha(edges, landmarks, weights):
    h = hashlib.sha256()
    for a, t in ((np.asarray(edges) - 1, np.int64), (landmarks, np.float64), (weights, np.float64)):
        h.update(np.ascontiguousarray(a, dtype=t).tobytes())
    return h.hexdigest()


def record(tag, rows, edges, landmarks, weights, lm_in, nobs, m, out):
    """rows: the input rows that remain (carried through the reference as a per-observation array)"""
    keep = np.zeros(nobs, dtype=bool); keep[rows] = True
    assert keep.sum() == rows.size and np.all(np.diff(rows) > 0)
    lm_index = np.full(m, -1, dtype=np.int32)
    lm_index[lm_in[rows]] = edges[:, 1] - 1
    assert np.array_equal(lm_index[lm_in[rows]], edges[:, 1] - 1)
    out["keep_" + tag] = np.packbits(keep)
    out["lm_index_" + tag] = lm_index
    out["counts_" + tag] = np.array([np.unique(edges[:, 0]).size, np.unique(edges[:, 1]).size, edges.shape[0]], dtype=np.int64)
    out["sha_" + tag] = sha(edges, landmarks, weights)


def run_case(name, cam, lm, p, w, n, m, store_input):
    nobs = cam.size
    edges = np.stack([cam + 1, lm + 1], axis=1).astype(np.int64)
    rows = np.arange(nobs)
    out = dict(nobs=np.int64(nobs))
    if store_input:
        out.update(cam=cam.astype(np.int16), lm=lm.astype(np.int16), n=np.int64(n), m=np.int64(m))
    e, l, ww, r, ia = checklandmarks(edges.copy(), p.copy(), w.copy(), rows.copy(), n, m)   # rgbs carries the row numbers
    record("10_1", r, e, l, ww, lm, nobs, m, out)
    out["indices_all_10_1"] = np.asarray(ia, dtype=np.int32)
    # the inline variant indexes three arrays; its `weights` carries the row numbers, the real weights are taken from them afterwards
    ns = dict(np=np, nx=nx, print=print, edges=edges.copy(), weights=rows.copy(), landmarks=p.copy(), N=n, M=m)
    exec(INLINE, ns)
    r2 = np.asarray(ns["weights"])
    record("0_1", r2, np.asarray(ns["edges"]), np.asarray(ns["landmarks"]), w[r2], lm, nobs, m, out)
    os.makedirs(os.path.join(HERE, "clean"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "clean", name + ".npz"), **out)
    print(name, "10_1:", out["counts_10_1"], "indices_all", out["indices_all_10_1"][:12], "| 0_1:", out["counts_0_1"])
    return out


def scene_b():
    cam, lm = [], []
    def see(c, ls):
        for l in ls:
            cam.append(c); lm.append(l)
    see(2, range(40))                                         # the camera with the most observations: it becomes index 0
    for k, c in enumerate((0, 1, 3, 4, 5)):                   # main component: landmarks 0 .. 39, every one seen at least twice
        see(c, [(8 * k + j) % 40 for j in range(28)])
        see(c, [40 + k])                                      # five single-view landmarks 40 .. 44
    see(9, range(10))                                         # exactly 10 observations: not more than the threshold
    see(10, range(45, 56))                                    # 11 observations, all single-view: stage 2 empties it
    for c in (6, 7, 8):                                       # second component: landmarks 56 .. 75
        see(c, range(56, 76))
    cam, lm = np.array(cam), np.array(lm)                     # camera 11 and landmark 76 are never named
    order = np.random.default_rng(12).permutation(cam.size)
    return cam[order], lm[order], 12, 77


def scene_c(second_first):
    a = [(c, l) for l in range(12) for c in (0, 1)]
    b = [(c, l) for l in range(12, 24) for c in (2, 3)]
    obs = np.array(b + a if second_first else a + b)
    return obs[:, 0], obs[:, 1], 4, 24


def scene_d():
    obs = [(c, l) for c in (0, 1) for l in range(12)] + [(0, 12), (1, 13), (0, 12)]   # landmark 12: one pair named twice; 13: seen once
    obs = np.array(obs)
    return obs[:, 0], obs[:, 1], 2, 14


if __name__ == "__main__":
    o = np.load(os.path.join(HERE, "simple2", "obs.npz")); x = np.load(os.path.join(HERE, "simple2", "xm2.npz"))
    err = x["error"]
    kept = err <= np.percentile(err, 90)
    print("SIMPLE2: kept by the recorded filter", int(kept.sum()), "of", kept.size)
    n, m = int(o["cam"].max()) + 1, int(o["lm"].max()) + 1
    # the reference deletes the filtered rows (3_test_colmap_glomap.py:323-338) and cleans what is left: rows of the FULL list are recorded
    full = np.flatnonzero(kept)
    out = run_case("a_tmp", o["cam"][kept].astype(np.int64), o["lm"][kept].astype(np.int64), o["p"][kept], o["w"][kept], n, m, False)
    os.remove(os.path.join(HERE, "clean", "a_tmp.npz"))
    for tag in ("10_1", "0_1"):
        k = np.unpackbits(out["keep_" + tag])[: full.size].astype(bool)
        big = np.zeros(kept.size, dtype=bool); big[full[k]] = True
        out["keep_" + tag] = np.packbits(big)
    out["nobs"] = np.int64(kept.size)
    np.savez_compressed(os.path.join(HERE, "clean", "a.npz"), **out)
    for name, (cam, lm, n, m) in (("b", scene_b()), ("c1", scene_c(False)), ("c2", scene_c(True)), ("d", scene_d())):
        p, w = fixture_points(name, cam.size)
        run_case(name, cam.astype(np.int64), lm.astype(np.int64), p, w, n, m, True)
    print("bytes:", sum(os.path.getsize(os.path.join(HERE, "clean", f)) for f in os.listdir(os.path.join(HERE, "clean"))))
