#!/usr/bin/env python3
"""tests/golden/pair/*.npz: what the reference's pairwise relative-rotation filter returns, recorded by EXECUTING the reference's own lines
(5_test_ceres.py, the body of `if run_filter:` up to its last print, read from /root/reference at generation time, never copied into this
repository) on the case's variables.  Runs only in the build container.

The lines read glomap_pose.pkl from output_path (written here to a temporary directory: {(i + 1, j + 1): (R, t)} for i < j), index
`landmarks`, `weights` and `rgbs` by the rows they keep (rgbs carries the row numbers) and leave is_outlier and error_sum behind; tqdm is
replaced by the identity.

Per case: outlier (np.packbits of is_outlier over the input rows), count (error_sum at every observation: the pairs that flagged it), nobs.
  a   SIMPLE2 (tests/golden/simple2/obs.npz), 2 % of the points scaled by 1 + 0.3 N(0, 1) (tests/xm_pair_numpy.py:case_a_inputs), every
      pair i < j with the rotation G_j G_i^T of the committed ground truth
  b   12 cameras / 80 landmarks, hand-built: camera 0 shares 19 landmarks with camera 2, 20 with camera 3 and 21 with camera 4; the pair
      (5, 6) has no pose; input row 0 is camera 0's observation of a landmark that cameras 3 and 4 see as well, so the reference (which
      never sees row 0) has 19 and 20 common landmarks there.  The file carries its input (cam, lm, p, n, m, pi, pj, R)."""
import itertools
import os
import pickle
import sys
import tempfile
import textwrap

import numpy as np
from scipy.sparse import coo_matrix
from scipy.stats import trim_mean

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
import xm_pair_numpy as pn   # noqa: E402

src = open(os.path.join(REF, "5_test_ceres.py")).read().splitlines()
first = next(i for i, l in enumerate(src) if l.startswith("if run_filter:")) + 1
last = next(i for i, l in enumerate(src) if "Total delete observations after glomap pose" in l)
BLOCK = textwrap.dedent("\n".join(src[first:last + 1]))
print("executing %s lines %d-%d" % (os.path.join(REF, "5_test_ceres.py"), first + 1, last + 1))


def run_case(name, c, store_input):
    cam, lm, p, n, m = c["cam"].astype(np.int64), c["lm"].astype(np.int64), c["p"], c["n"], c["m"]
    nobs = cam.size
    pose = {(int(i) + 1, int(j) + 1): (R, np.zeros(3)) for i, j, R in zip(c["pi"], c["pj"], c["R"])}
    assert all(i < j for i, j in pose)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "glomap_pose.pkl"), "wb") as f:
            pickle.dump(pose, f)
        ns = dict(np=np, pickle=pickle, coo_matrix=coo_matrix, itertools=itertools, trim_mean=trim_mean, tqdm=lambda it, **kw: it, print=print,
                  output_path=d, visualization_glomap_filter=False, edges=np.stack([cam + 1, lm + 1], axis=1), landmarks=p.copy(),
                  weights=np.ones(nobs), rgbs=np.arange(nobs), N=n, M=m)
        exec(BLOCK, ns)
    out_rows = np.ones(nobs, dtype=bool); out_rows[np.asarray(ns["rgbs"])] = False
    assert np.array_equal(out_rows, ns["is_outlier"])
    count = ns["error_sum"][cam, lm]
    assert np.array_equal(count, np.round(count)) and count.max() < 256
    out = dict(outlier=np.packbits(ns["is_outlier"]), count=count.astype(np.uint8), nobs=np.int64(nobs))
    if store_input:
        out.update(cam=cam.astype(np.int16), lm=lm.astype(np.int16), p=p, n=np.int64(n), m=np.int64(m), pi=c["pi"].astype(np.int16),
                   pj=c["pj"].astype(np.int16), R=c["R"])
    os.makedirs(os.path.join(HERE, "pair"), exist_ok=True)
    fn = os.path.join(HERE, "pair", name + ".npz")
    np.savez_compressed(fn, **out)
    ours = pn.pair_filter_numpy(c["cam"], c["lm"], p, c["pi"], c["pj"], c["R"], n, m, skip_row0=True)
    print(name, "reference flags", int(ns["is_outlier"].sum()), "of", nobs, "| restatement", ours["info"], "margin %.3e" % ours["margin"],
          "equal", bool(np.array_equal(ours["outlier"], ns["is_outlier"]) and np.array_equal(ours["count"], count)), "|", os.path.getsize(fn), "bytes")


def scene_b(seed=3):
    rng = np.random.default_rng(seed)
    n, m = 12, 80
    sees = {0: range(40), 1: range(30), 2: list(range(21, 40)) + list(range(40, 50)), 3: list(range(20, 40)) + list(range(50, 56)),
            4: range(19, 40)}
    for c in range(5, 12):
        sees[c] = sorted(rng.choice(m, 44, replace=False).tolist())
    P = rng.uniform(-5.0, 5.0, (m, 3))
    A = rng.standard_normal((n, 3, 3)); Q, _ = np.linalg.qr(A); Q = Q * np.sign(np.linalg.det(Q))[:, None, None]
    t = rng.uniform(-2.0, 2.0, (n, 3)); s = rng.uniform(0.5, 2.0, n)
    cam = np.concatenate([np.full(len(sees[c]), c) for c in range(n)]); lm = np.concatenate([np.asarray(sees[c]) for c in range(n)])
    p = np.einsum("eba,eb->ea", Q[cam], P[lm] - t[cam]) / s[cam, None] + 0.01 * rng.standard_normal((cam.size, 3))
    hit = rng.random(cam.size) < 0.08
    p[hit] *= (1.0 + 0.4 * rng.standard_normal(int(hit.sum())))[:, None]
    order = rng.permutation(cam.size)
    r0 = int(np.flatnonzero((cam == 0) & (lm == 25))[0])     # input row 0: camera 0, landmark 25 (cameras 1, 2, 3 and 4 see it too)
    order = np.concatenate([[r0], order[order != r0]])
    pairs = [(i, j) for i, j in itertools.combinations(range(n), 2) if (i, j) != (5, 6)]
    pi, pj = np.array(pairs).T
    R = np.einsum("kba,kbc->kac", Q[pj], Q[pi])              # p_j ~ R_j^T R_i p_i
    return dict(cam=cam[order].astype(np.int32), lm=lm[order].astype(np.int32), p=p[order], n=n, m=m, pi=pi.astype(np.int32), pj=pj.astype(np.int32), R=R)


if __name__ == "__main__":
    run_case("a", pn.case_a_inputs(), False)
    run_case("b", scene_b(), True)
