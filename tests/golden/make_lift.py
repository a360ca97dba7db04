#!/usr/bin/env python3
"""tests/golden/lift/*.npz: what the reference's depth lift returns, recorded by EXECUTING the reference's own lines (5_test_ceres.py: the
de-duplication block from "# this edges is 1-base" to the landmarky matrix, and the loop over the cameras from `for i in tqdm(range(N)`
to `rgbs = np.array(rgbs)`, read from a checkout of the reference at generation time, never copied into this repository) on the case's
variables:   python tests/golden/make_lift.py <directory of the reference>

The lines read an image per camera and ask a depth network for its maps.  Both are stubs here: cv2.imread returns an image whose pixel
(v, u) holds (u, v, camera), so the `rgbs` the lines collect tell which pixel every output was sampled at, and with it which input row it
came from; model.infer returns the case's depth and confidence maps as CPU tensors (a 1-D tensor for a camera without a map, which the
lines skip).  tqdm is the identity.

Per case, the input (cam, lm, xy, n, m, K, hw, has_map, depth and conf as the concatenated float32 maps of the cameras that have one) and
the reference's output: ref_cam, ref_lm (0-based), ref_p (landmarks), ref_w (weights), ref_row (the input row, from rgbs) and
ref_rows_duplicate (what the lines print as "delete same observation").
  a   12 cameras, maps of 48 x 64 and two other sizes: a camera without a map, one without rows, one with every row outside the border,
      one with zeros and negatives among its depths; twins whose two rows lie at different pixels; rows shuffled
  b   5 cameras with 257, 300, 64, 700 and 21 rows (several tracks per pixel, so ties among the depths), a tenth of them outside the border"""
import os
import sys
import textwrap

import numpy as np
import torch
from scipy.sparse import coo_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
import xm_lift_numpy as ln   # noqa: E402

src = open(os.path.join(REF, "5_test_ceres.py")).read().splitlines()
d0 = next(i for i, l in enumerate(src) if "# this edges is 1-base" in l)
d1 = next(i for i, l in enumerate(src) if l.strip().startswith("landmarky = coo_matrix("))
l0 = next(i for i, l in enumerate(src) if l.strip().startswith("for i in tqdm(range(N)"))
l1 = next(i for i, l in enumerate(src) if l.strip() == "rgbs = np.array(rgbs)")
DEDUP = textwrap.dedent("\n".join(src[d0:d1 + 1]))
LOOP = textwrap.dedent("\n".join(src[l0:l1 + 1]))
print("executing %s lines %d-%d and %d-%d" % (os.path.join(REF, "5_test_ceres.py"), d0 + 1, d1 + 1, l0 + 1, l1 + 1))


class Cv2:
    def __init__(self, hw):
        self.hw = hw

    def imread(self, path):
        c = int(os.path.basename(path))
        h, w = self.hw[c]
        img = np.zeros((h, w, 3), dtype=np.int64)
        img[:, :, 0] = np.arange(w)[None, :]; img[:, :, 1] = np.arange(h)[:, None]; img[:, :, 2] = c
        return img


class Model:
    def __init__(self, case):
        self.case = case

    def infer(self, rgb_torch):
        c = int(rgb_torch[2, 0, 0])
        D, Cf = self.case["depth"][c], self.case["conf"][c]
        if D is None:
            return dict(depth=torch.zeros(1, 3), confidence=torch.zeros(1, 3))      # squeezes to one dimension: the lines skip the camera
        return dict(depth=torch.from_numpy(D)[None, None], confidence=torch.from_numpy(Cf)[None, None])


def run_case(name, c):
    cam, lm, xy, n, m = c["cam"].astype(np.int64), c["lm"].astype(np.int64), c["xy"], c["n"], c["m"]
    hw = np.array([(1, 1) if D is None else D.shape for D in c["depth"]], dtype=np.int32)
    # the match table of the front end: camera (1-based), x, y, track (1-based); the last camera and the last track must be named (N, M = max)
    matches = np.stack([cam + 1.0, xy[:, 0], xy[:, 1], lm + 1.0], axis=1)
    assert cam.max() == n - 1
    ns = dict(np=np, coo_matrix=coo_matrix, print=print, matches=matches)
    exec(DEDUP, ns)
    ns.update(torch=torch, cv2=Cv2(hw), tqdm=lambda it, **kw: it, model=Model(c), N=n, image_dir="", filename=[str(i) for i in range(n)],
              gt={str(i): dict(K=c["K"][i]) for i in range(n)}, points_3d=np.zeros((0, 3)), weights=np.array([]), edges=np.zeros((0, 2)),
              rgbs=np.zeros((0, 3)))
    exec(LOOP, ns)
    e = np.asarray(ns["edges"]) - 1
    rgbs = np.asarray(ns["rgbs"]).astype(np.int64)
    assert np.array_equal(rgbs[:, 2], e[:, 0])
    uv = np.trunc(xy).astype(np.int64)
    row = np.zeros(e.shape[0], dtype=np.int64)
    for k in range(e.shape[0]):     # the input row of (camera, track) whose pixel the lines sampled: exactly one
        hit = np.flatnonzero((cam == e[k, 0]) & (lm == e[k, 1]) & (uv[:, 0] == rgbs[k, 0]) & (uv[:, 1] == rgbs[k, 1]))
        assert hit.size == 1, (k, hit)
        row[k] = hit[0]
    has = np.array([D is not None for D in c["depth"]])
    out = dict(cam=cam.astype(np.int16), lm=lm.astype(np.int16), xy=xy, n=np.int64(n), m=np.int64(m), K=c["K"], hw=hw, has_map=has.astype(np.uint8),
               depth=np.concatenate([D.ravel() for D in c["depth"] if D is not None]), conf=np.concatenate([D.ravel() for D in c["conf"] if D is not None]),
               ref_cam=e[:, 0].astype(np.int16), ref_lm=e[:, 1].astype(np.int16), ref_p=np.asarray(ns["landmarks"]), ref_w=np.asarray(ns["weights"]),
               ref_row=row.astype(np.int32), ref_rows_duplicate=np.int64(ns["delete_observation"]))
    os.makedirs(ln.GOLDEN, exist_ok=True)
    fn = os.path.join(ln.GOLDEN, name + ".npz")
    np.savez_compressed(fn, **out)
    ours = ln.run_numpy(c)
    same = all(np.array_equal(ours[k], v) for k, v in (("cam", e[:, 0]), ("lm", e[:, 1]), ("row", row), ("w", out["ref_w"])))
    err = np.abs(ours["p"] - out["ref_p"]) / ours["p_bound"] if row.size else np.zeros(1)
    print(name, "reference keeps", row.size, "of", cam.size, "rows, duplicates", int(out["ref_rows_duplicate"]), "| restatement", ours["info"], "equal", same,
          "largest |p - ref| / bound %.3f" % err.max(), "|", os.path.getsize(fn), "bytes")


def case_a():
    hws = [(48, 64)] * 9 + [(33, 47), (40, 29), (48, 64)]
    c = ln.scene([40, 0, 57, 33, 80, 21, 64, 100, 12, 45, 38, 50], 101, hw=hws, outside=0.1, twins=0.2, no_map=(3,))
    in2 = c["cam"] == 2                                               # camera 2: every row outside the border
    c["xy"][in2, 1] = np.where(np.arange(int(in2.sum())) % 2 == 0, 4.5, 44.5)
    rng = np.random.default_rng(102)
    d4 = c["depth"][4]
    d4[rng.random(d4.shape) < 0.2] = 0.0
    d4[rng.random(d4.shape) < 0.15] = -0.75
    return c


def case_b():
    return ln.scene([257, 300, 64, 700, 21], 103, outside=0.1, twins=0.05)


if __name__ == "__main__":
    run_case("a", case_a())
    run_case("b", case_b())
