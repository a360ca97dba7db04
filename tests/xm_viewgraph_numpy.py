"""Restatements of the two-view match verification and view-graph pruning (include/xm_amd.h: xm_view_graph_filter), the block in front of
track establishment in the reference's fork of GLOMAP (deps/glomap/glomap/controllers/global_mapper.cc:56-111).

NOTHING HERE WAS COMPARED WITH THE REFERENCE'S COMPILED CODE: it needs COLMAP, Eigen and glog.  Two restatements stand in for it:
  (a) sequential(c)   the C++ line by line in plain Python loops over Python floats (IEEE doubles, every operation rounded on its own), one
                      pair and one match at a time, with the lines it restates cited: image_pair_inliers.cc (ipi), two_view_geometry.cc
                      (tvg), relpose_filter.cc (rpf), view_graph.cc (vg), image_undistorter.cc
  (b) run_numpy(c)    the vectorised contract the device is tested against
Where the contract fixes what the C++ leaves open (the order of a sum of three, the rotation as a matrix, the cosine test of rule 6, the
tie of rule 7) both follow the contract; the header says where that departs from the reference."""
import hashlib
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "viewgraph")

NONE, E_, F_, H_ = 0, 1, 2, 3
VALID, INVALID_IN, FEW_INLIERS, LOW_RATIO, ROTATION, OUTSIDE = 0, 1, 2, 3, 4, 5
# the header's literals (XM_VG_*), read by test_viewgraph_abi.py against math
EPS = 9.9999999999999998e-13
MIN_DEPTH = 1.0000000000000000e-02
MAX_DEPTH = 1.0000000000000000e+02
COS_EPIPOLE = 9.9863053475457386e-01
COS_PARALLEL = 1.0000009999999999e+00
COS_10DEG = 9.8480775301220802e-01
DEFAULTS = dict(max_epipolar_error_E=1.0, max_epipolar_error_F=4.0, max_epipolar_error_H=4.0, min_inlier_num=30, min_inlier_ratio=0.25,
                max_rotation_error_deg=10.0)
INFO_FIELDS = ("matches", "inliers", "matches_out", "pairs_valid", "pairs_invalid_in", "pairs_few_inliers", "pairs_low_ratio", "pairs_rotation",
               "pairs_outside", "pairs_none", "pairs_E", "pairs_F", "pairs_H", "largest", "components", "pairs_wave", "pairs_group", "pairs_workspace",
               "max_matches")
LIMITS = dict(wave_matches=256, group_matches=8192)


# ------------------------------------------------------------------------------------------------ cases
def make_case(counts, xy, pairs, focal=None, Kinv=None, bearing=None, valid_in=None, registered_in=None, rot=None, **options):
    """counts: features per image; xy: features x 2; pairs: [dict(i, j, model, m=[(a, b), ...], R=, t=, FH=), ...]"""
    counts = np.asarray(counts, dtype=np.int64)
    n = counts.size
    foff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    per = [np.asarray(p.get("m", []), dtype=np.int32).reshape(-1, 2) for p in pairs]
    moff = np.concatenate([[0], np.cumsum([m.shape[0] for m in per])]).astype(np.int64)
    cat = np.concatenate(per, axis=0) if per else np.zeros((0, 2), dtype=np.int32)
    k = len(pairs)
    return dict(foff=foff, xy=np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2), focal=np.ones(n) if focal is None else np.asarray(focal, dtype=np.float64),
                Kinv=np.tile(np.eye(3), (n, 1, 1)) if Kinv is None else np.asarray(Kinv, dtype=np.float64), bearing=bearing,
                pi=np.array([p["i"] for p in pairs], dtype=np.int32), pj=np.array([p["j"] for p in pairs], dtype=np.int32),
                model=np.array([p.get("model", NONE) for p in pairs], dtype=np.int32),
                Rrel=np.array([p.get("R", np.eye(3)) for p in pairs], dtype=np.float64).reshape(k, 3, 3),
                trel=np.array([p.get("t", [1.0, 0.0, 0.0]) for p in pairs], dtype=np.float64).reshape(k, 3),
                FH=np.array([p.get("FH", np.eye(3)) for p in pairs], dtype=np.float64).reshape(k, 3, 3),
                valid_in=None if valid_in is None else np.asarray(valid_in, dtype=np.uint8),
                registered_in=None if registered_in is None else np.asarray(registered_in, dtype=np.uint8),
                rot=None if rot is None else np.asarray(rot, dtype=np.float64).reshape(n, 3, 3),
                moff=moff, f1=np.ascontiguousarray(cat[:, 0]), f2=np.ascontiguousarray(cat[:, 1]), options=dict(options))


def options_of(c):
    """the library's options of a case: score, the three errors, the two inlier rules and the cosine of rule 6"""
    o = dict(score=True, max_epipolar_error_E=1.0, max_epipolar_error_F=4.0, max_epipolar_error_H=4.0, min_inlier_num=30, min_inlier_ratio=0.25,
             cos_max_rotation_error=COS_10DEG)
    o.update(c["options"])
    return o


def call_args(c):
    """-> positional and keyword arguments of xmamd.view_graph_filter"""
    kw = {k: c[k] for k in ("focal", "Kinv", "bearing", "Rrel", "trel", "FH", "valid_in", "registered_in", "rot")}
    kw.update(options_of(c))
    return (c["foff"], c["xy"], c["pi"], c["pj"], c["model"], (c["moff"], c["f1"], c["f2"])), kw


def next_pass(c, r, rot, **options):
    """pass B's case from pass A's case and result: the compacted matches, the validity and the registered images as they came out"""
    d = dict(c)
    d["moff"], d["f1"], d["f2"] = r["moff_out"], r["f1_out"], r["f2_out"]
    d["valid_in"] = (r["pair_status"] == VALID).astype(np.uint8)
    d["registered_in"] = r["registered"]
    d["rot"] = None if rot is None else np.asarray(rot, dtype=np.float64).reshape(-1, 3, 3)
    d["options"] = dict(c["options"], score=False, **options)
    return d


def permuted(c, seed):
    """the pairs in another order, each carrying its matches; -> the case and the order"""
    order = np.random.default_rng(seed).permutation(c["pi"].size)
    d = dict(c)
    for k in ("pi", "pj", "model", "Rrel", "trel", "FH"):
        d[k] = np.ascontiguousarray(c[k][order])
    if c["valid_in"] is not None:
        d["valid_in"] = np.ascontiguousarray(c["valid_in"][order])
    cnt = np.diff(c["moff"])[order]
    d["moff"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    idx = np.concatenate([np.arange(c["moff"][k], c["moff"][k + 1]) for k in order]) if order.size else np.zeros(0, dtype=np.int64)
    d["f1"] = np.ascontiguousarray(c["f1"][idx.astype(np.int64)]); d["f2"] = np.ascontiguousarray(c["f2"][idx.astype(np.int64)])
    return d, order, idx.astype(np.int64)


def rot_axis(axis, deg):
    """Rodrigues: the rotation by deg degrees about axis"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def essential(R, t):
    """E = [t]x R as rule 2 rounds it"""
    R = np.asarray(R, dtype=np.float64); t = np.asarray(t, dtype=np.float64)
    return np.stack([t[1] * R[2] - t[2] * R[1], t[2] * R[0] - t[0] * R[2], t[0] * R[1] - t[1] * R[0]])


def _check(c):
    n, npairs = c["foff"].size - 1, c["pi"].size
    cnt = np.diff(c["moff"])
    k_of = np.repeat(np.arange(npairs), cnt)
    na = np.diff(c["foff"])
    bad = (c["f1"] < 0) | (c["f1"] >= na[c["pi"][k_of]]) | (c["f2"] < 0) | (c["f2"] >= na[c["pj"][k_of]])
    if bad.any():
        raise ValueError(f"feature index out of range at match {int(np.flatnonzero(bad)[0])}")
    return n, npairs, cnt, k_of


# ------------------------------------------------------------------------------------------------ (a) the C++ in plain loops
def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _bearing_seq(K, x, y):
    """image_undistorter.cc:33-36: camera.CamFromImg(feature).homogeneous().normalized(), for a pinhole camera Kinv * (x, y, 1)"""
    h = [(K[r][0] * x + K[r][1] * y) + K[r][2] for r in range(3)]
    nrm = math.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
    return [_div(h[0], nrm), _div(h[1], nrm), _div(h[2], nrm)]


def _score_essential(R, t, fi, fj, max_E, x1s, x2s):
    """ipi:20-92 -> the inlier flag of every match"""
    # tvg:41-45, EssentialFromMotion: [t]x * R
    E = [[t[1] * R[2][c] - t[2] * R[1][c] for c in range(3)], [t[2] * R[0][c] - t[0] * R[2][c] for c in range(3)],
         [t[0] * R[1][c] - t[1] * R[0][c] for c in range(3)]]
    e12 = list(t)                                                                   # ipi:27
    e21 = [-_dot([R[0][r], R[1][r], R[2][r]], t) for r in range(3)]                 # ipi:28, Inverse(pose).translation = -(R^T t)
    if e12[2] < 0:                                                                  # ipi:30
        e12 = [-v for v in e12]
    if e21[2] < 0:                                                                  # ipi:31
        e21 = [-v for v in e21]
    thres = (max_E * 0.5) * (_div(1.0, fi) + _div(1.0, fj))                         # ipi:43-45
    sq = thres * thres                                                              # ipi:48
    out = []
    for x1, x2 in zip(x1s, x2s):                                                    # ipi:58
        # tvg:71-83, SampsonError on bearings
        d1, d2 = EPS + x1[2], EPS + x2[2]
        Ex1 = [_div(_dot(E[r], x1), d1) for r in range(3)]
        Etx2 = [_div(_dot([E[0][r], E[1][r], E[2][r]], x2), d2) for r in range(3)]
        C = _dot(Ex1, x2)
        Cx = Ex1[0] * Ex1[0] + Ex1[1] * Ex1[1]
        Cy = Etx2[0] * Etx2[0] + Etx2[1] * Etx2[1]
        r2 = _div(C * C, Cx + Cy)
        if not r2 < sq:                                                             # ipi:64
            out.append(0)
            continue
        # tvg:5-29, CheckCheirality(pose, x1, x2, 1e-2, 100)
        Rx1 = [_dot(R[r], x1) for r in range(3)]
        a = -_dot(Rx1, x2)
        b1 = -_dot(Rx1, t)
        b2 = _dot(x2, t)
        l1 = b1 - a * b2
        l2 = (-a) * b1 + b2
        mn = MIN_DEPTH * (1.0 - a * a)
        mx = MAX_DEPTH * (1.0 - a * a)
        cheir = l1 > mn and l2 > mn and l1 < mx and l2 < mx
        Rtx2 = [_dot([R[0][r], R[1][r], R[2][r]], x2) for r in range(3)]            # ipi:72, rotation.inverse() * pt2
        ok = _dot(x1, Rtx2) < COS_PARALLEL                                          # ipi:73
        ok = ok and _dot(x1, e21) < COS_EPIPOLE and _dot(x2, e12) < COS_EPIPOLE     # ipi:76-79
        out.append(1 if cheir and ok else 0)                                        # ipi:81-83
    return out


def _score_fundamental(F, max_F, p1s, p2s):
    """ipi:94-164"""
    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    ep = cross(F[0], F[2])                                                          # ipi:99
    if not any(v > EPS or v < -EPS for v in ep):                                    # ipi:101-110
        ep = cross(F[1], F[2])
    sq = max_F * max_F                                                              # ipi:121
    pre, sign = [], []
    pos = neg = 0
    for k, ((x1, y1), (x2, y2)) in enumerate(zip(p1s, p2s)):
        # tvg:57-69, SampsonError on pixels
        Fx1 = [(F[r][0] * x1 + F[r][1] * y1) + F[r][2] for r in range(3)]
        Ftx2 = [(F[0][r] * x2 + F[1][r] * y2) + F[2][r] for r in range(3)]
        C = (Fx1[0] * x2 + Fx1[1] * y2) + Fx1[2]
        r2 = _div(C * C, (Fx1[0] * Fx1[0] + Fx1[1] * Fx1[1]) + (Ftx2[0] * Ftx2[0] + Ftx2[1] * Ftx2[1]))
        if r2 < sq:                                                                 # ipi:133
            s1 = (F[0][0] * x2 + F[1][0] * y2) + F[2][0]                            # tvg:36
            s2 = ep[1] - ep[2] * y1                                                 # tvg:37
            sign.append(s1 * s2)
            if sign[-1] > 0:                                                        # ipi:135-139
                pos += 1
            else:
                neg += 1
            pre.append(k)
    out = [0] * len(p1s)
    if pos == neg:                                                                  # ipi:150
        return out
    is_positive = pos > neg                                                         # ipi:147
    for k, s in zip(pre, sign):                                                     # ipi:154-161
        if (s > 0) == is_positive:
            out[k] = 1
    return out


def _score_homography(H, max_H, p1s, p2s):
    """ipi:166-198, tvg:85-93"""
    sq = max_H * max_H
    out = []
    for (x1, y1), (x2, y2) in zip(p1s, p2s):
        Hx = [(H[r][0] * x1 + H[r][1] * y1) + H[r][2] for r in range(3)]
        d = EPS + Hx[2]
        u, v = _div(Hx[0], d) - x2, _div(Hx[1], d) - y2
        out.append(1 if u * u + v * v < sq else 0)
    return out


def sequential(c, limits=LIMITS):
    """restatement (a): global_mapper.cc:56-111 for one call, pair by pair and match by match"""
    o = options_of(c)
    n, npairs, cnt, _ = _check(c)
    foff, moff = c["foff"].tolist(), c["moff"].tolist()
    xy = c["xy"].tolist()
    Kinv = None if c["Kinv"] is None else c["Kinv"].tolist()
    bearing = None if c["bearing"] is None else np.asarray(c["bearing"], dtype=np.float64).tolist()
    valid = [True] * npairs if c["valid_in"] is None else [bool(v) for v in c["valid_in"]]
    status = [VALID if v else INVALID_IN for v in valid]
    inlier = [0] * moff[-1]
    ninl = [0] * npairs

    def bear(g):
        return bearing[g] if bearing is not None else _bearing_seq(Kinv[img_of[g]], xy[g][0], xy[g][1])
    img_of = np.repeat(np.arange(n), np.diff(c["foff"])).tolist()
    for k in range(npairs):                                                         # ipi:205
        i, j = int(c["pi"][k]), int(c["pj"][k])
        ms = range(moff[k], moff[k + 1])
        g1 = [foff[i] + int(c["f1"][e]) for e in ms]
        g2 = [foff[j] + int(c["f2"][e]) for e in ms]
        if not o["score"]:                                                          # pass B: the listed matches are the inliers
            flags = [1 if valid[k] else 0] * len(g1)
        elif not valid[k]:                                                          # ipi:207-209
            flags = [0] * len(g1)
        elif c["model"][k] == E_:                                                   # ipi:15-16
            flags = _score_essential(c["Rrel"][k].tolist(), c["trel"][k].tolist(), float(c["focal"][i]), float(c["focal"][j]), o["max_epipolar_error_E"],
                                     [bear(g) for g in g1], [bear(g) for g in g2])
        elif c["model"][k] == F_:                                                   # ipi:13-14
            flags = _score_fundamental(c["FH"][k].tolist(), o["max_epipolar_error_F"], [xy[g] for g in g1], [xy[g] for g in g2])
        elif c["model"][k] == H_:                                                   # ipi:9-12
            flags = _score_homography(c["FH"][k].tolist(), o["max_epipolar_error_H"], [xy[g] for g in g1], [xy[g] for g in g2])
        else:                                                                       # ipi:17
            flags = [0] * len(g1)
        inlier[moff[k]:moff[k + 1]] = flags
        ninl[k] = sum(flags)
    if o["score"]:
        for k in range(npairs):                                                     # rpf:35-48
            if status[k] == VALID and ninl[k] < o["min_inlier_num"]:
                status[k] = FEW_INLIERS
        for k in range(npairs):                                                     # rpf:50-65
            if status[k] == VALID and _div(float(ninl[k]), float(moff[k + 1] - moff[k])) < o["min_inlier_ratio"]:
                status[k] = LOW_RATIO
    if c["rot"] is not None:                                                        # rpf:7-33
        reg = [True] * n if c["registered_in"] is None else [bool(v) for v in c["registered_in"]]
        rot = c["rot"].tolist()
        for k in range(npairs):
            i, j = int(c["pi"][k]), int(c["pj"][k])
            if status[k] != VALID or not reg[i] or not reg[j]:                      # rpf:13-20
                continue
            Q = c["Rrel"][k].tolist()
            s = None
            for a in range(3):                                                      # rpf:22-24 with the contract's cosine: trace((R_j R_i^T)^T Rrel)
                for b in range(3):
                    prod = _dot(rot[j][a], rot[i][b]) * Q[a][b]
                    s = prod if s is None else s + prod
            cs = (s - 1.0) / 2.0
            if cs > 1.0:
                cs = 1.0
            if cs < -1.0:
                cs = -1.0
            if cs < o["cos_max_rotation_error"]:                                    # rpf:25
                status[k] = ROTATION
    # vg:9-46, KeepLargestConnectedComponents: adjacency over the valid pairs, BFS, the largest component
    adj = {}
    for k in range(npairs):
        if status[k] == VALID:
            i, j = int(c["pi"][k]), int(c["pj"][k])
            adj.setdefault(i, []).append(j); adj.setdefault(j, []).append(i)
    seen, comps = set(), []
    for root in sorted(adj):                                                        # ascending: a tie goes to the smaller first image
        if root in seen:
            continue
        comp, queue = {root}, [root]
        seen.add(root)
        while queue:
            cur = queue.pop(0)
            for nb in adj[cur]:
                if nb not in seen:
                    seen.add(nb); comp.add(nb); queue.append(nb)
        comps.append(comp)
    best = set()
    for comp in comps:                                                              # vg:17-22, strictly larger
        if len(comp) > len(best):
            best = comp
    registered = np.array([1 if i in best else 0 for i in range(n)], dtype=np.uint8)
    for k in range(npairs):                                                         # vg:36-40
        if status[k] == VALID and not (int(c["pi"][k]) in best and int(c["pj"][k]) in best):
            status[k] = OUTSIDE
    return _finish(c, np.array(inlier, dtype=np.uint8), np.array(ninl, dtype=np.int32), np.array(status, dtype=np.int32), registered, len(best), len(comps),
                   cnt, limits)


def _finish(c, inlier, ninl, status, registered, largest, components, cnt, limits):
    """rule 8 and the counters, shared by both restatements (pure bookkeeping)"""
    npairs = c["pi"].size
    k_of = np.repeat(np.arange(npairs), cnt)
    keep = (inlier != 0) & (status[k_of] == VALID)
    kept = np.where(status == VALID, ninl, 0).astype(np.int64)
    info = dict(matches=int(cnt.sum()), inliers=int(ninl.sum()), matches_out=int(keep.sum()), largest=int(largest), components=int(components),
                max_matches=int(cnt.max()) if npairs else 0)
    for name, code in (("valid", VALID), ("invalid_in", INVALID_IN), ("few_inliers", FEW_INLIERS), ("low_ratio", LOW_RATIO), ("rotation", ROTATION),
                       ("outside", OUTSIDE)):
        info["pairs_" + name] = int(np.sum(status == code))
    for name, code in (("none", NONE), ("E", E_), ("F", F_), ("H", H_)):
        info["pairs_" + name] = int(np.sum(c["model"] == code))
    info["pairs_wave"] = int(np.sum((cnt > 0) & (cnt <= limits["wave_matches"])))
    info["pairs_group"] = int(np.sum((cnt > limits["wave_matches"]) & (cnt <= limits["group_matches"])))
    info["pairs_workspace"] = int(np.sum(cnt > limits["group_matches"]))
    return dict(inlier=inlier, pair_inliers=ninl, pair_status=status, registered=registered,
                moff_out=np.concatenate([[0], np.cumsum(kept)]).astype(np.int64), f1_out=np.ascontiguousarray(c["f1"][keep]),
                f2_out=np.ascontiguousarray(c["f2"][keep]), info=info)


# ------------------------------------------------------------------------------------------------ (b) the vectorised contract
def _d3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def bearings(c):
    """rule 0 for every feature"""
    if c["bearing"] is not None:
        return np.asarray(c["bearing"], dtype=np.float64).reshape(-1, 3)
    img = np.repeat(np.arange(c["foff"].size - 1), np.diff(c["foff"]))
    K = c["Kinv"][img]
    x, y = c["xy"][:, 0], c["xy"][:, 1]
    h = [(K[:, r, 0] * x + K[:, r, 1] * y) + K[:, r, 2] for r in range(3)]
    nrm = np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
    return np.stack([h[0] / nrm, h[1] / nrm, h[2] / nrm], axis=1)


def rotation_cosine(rot_i, rot_j, Q):
    """rule 6's c for arrays of pairs (k x 3 x 3 each)"""
    s = None
    for a in range(3):
        for b in range(3):
            prod = _d3(rot_j[:, a, 0], rot_j[:, a, 1], rot_j[:, a, 2], rot_i[:, b, 0], rot_i[:, b, 1], rot_i[:, b, 2]) * Q[:, a, b]
            s = prod if s is None else s + prod
    cs = (s - 1.0) / 2.0
    cs = np.where(cs > 1.0, 1.0, cs)
    return np.where(cs < -1.0, -1.0, cs)


def run_numpy(c, limits=LIMITS):
    """restatement (b): every output of xm_view_graph_filter and its integer counters (info, in the order of INFO_FIELDS; `rounds` is the
    device's own and is not restated)"""
    o = options_of(c)
    n, npairs, cnt, k_of = _check(c)
    E = int(c["moff"][-1])
    valid = np.ones(npairs, dtype=bool) if c["valid_in"] is None else c["valid_in"] != 0
    u = c["foff"][c["pi"][k_of]] + c["f1"]; v = c["foff"][c["pj"][k_of]] + c["f2"]
    code = np.zeros(E, dtype=np.uint8)
    with np.errstate(all="ignore"):
        if not o["score"]:
            code[valid[k_of]] = 1
        else:
            md = np.where(valid, c["model"], NONE)[k_of]
            e = np.flatnonzero(md == E_)
            if e.size:
                B = bearings(c)
                R, t = c["Rrel"], c["trel"]
                Em = np.stack([t[:, 1, None] * R[:, 2] - t[:, 2, None] * R[:, 1], t[:, 2, None] * R[:, 0] - t[:, 0, None] * R[:, 2],
                               t[:, 0, None] * R[:, 1] - t[:, 1, None] * R[:, 0]], axis=1)
                thr = (o["max_epipolar_error_E"] * 0.5) * (1.0 / c["focal"][c["pi"]] + 1.0 / c["focal"][c["pj"]])
                sq = thr * thr
                e12 = t.copy()
                e21 = np.stack([-_d3(R[:, 0, r], R[:, 1, r], R[:, 2, r], t[:, 0], t[:, 1], t[:, 2]) for r in range(3)], axis=1)
                e12 = np.where(e12[:, 2:3] < 0, -e12, e12); e21 = np.where(e21[:, 2:3] < 0, -e21, e21)
                k = k_of[e]
                x1, x2 = B[u[e]], B[v[e]]
                Ek, Rk, tk = Em[k], R[k], t[k]
                d1, d2 = EPS + x1[:, 2], EPS + x2[:, 2]
                Ex1 = [_d3(Ek[:, r, 0], Ek[:, r, 1], Ek[:, r, 2], x1[:, 0], x1[:, 1], x1[:, 2]) / d1 for r in range(3)]
                Etx2 = [_d3(Ek[:, 0, r], Ek[:, 1, r], Ek[:, 2, r], x2[:, 0], x2[:, 1], x2[:, 2]) / d2 for r in range(3)]
                C = _d3(Ex1[0], Ex1[1], Ex1[2], x2[:, 0], x2[:, 1], x2[:, 2])
                r2 = (C * C) / ((Ex1[0] * Ex1[0] + Ex1[1] * Ex1[1]) + (Etx2[0] * Etx2[0] + Etx2[1] * Etx2[1]))
                Rx1 = [_d3(Rk[:, r, 0], Rk[:, r, 1], Rk[:, r, 2], x1[:, 0], x1[:, 1], x1[:, 2]) for r in range(3)]
                Rtx2 = [_d3(Rk[:, 0, r], Rk[:, 1, r], Rk[:, 2, r], x2[:, 0], x2[:, 1], x2[:, 2]) for r in range(3)]
                a = -_d3(Rx1[0], Rx1[1], Rx1[2], x2[:, 0], x2[:, 1], x2[:, 2])
                b1 = -_d3(Rx1[0], Rx1[1], Rx1[2], tk[:, 0], tk[:, 1], tk[:, 2])
                b2 = _d3(x2[:, 0], x2[:, 1], x2[:, 2], tk[:, 0], tk[:, 1], tk[:, 2])
                l1 = b1 - a * b2; l2 = (-a) * b1 + b2
                f = 1.0 - a * a
                mn, mx = MIN_DEPTH * f, MAX_DEPTH * f
                ok = (r2 < sq[k]) & (l1 > mn) & (l2 > mn) & (l1 < mx) & (l2 < mx)
                ok &= _d3(x1[:, 0], x1[:, 1], x1[:, 2], Rtx2[0], Rtx2[1], Rtx2[2]) < COS_PARALLEL
                ok &= _d3(x1[:, 0], x1[:, 1], x1[:, 2], e21[k, 0], e21[k, 1], e21[k, 2]) < COS_EPIPOLE
                ok &= _d3(x2[:, 0], x2[:, 1], x2[:, 2], e12[k, 0], e12[k, 1], e12[k, 2]) < COS_EPIPOLE
                code[e] = ok
            e = np.flatnonzero(md == F_)
            if e.size:
                Fm = c["FH"]
                ep = _cross(Fm[:, 0], Fm[:, 2])
                alt = _cross(Fm[:, 1], Fm[:, 2])
                ok0 = ((ep > EPS) | (ep < -EPS)).any(axis=1)
                ep = np.where(ok0[:, None], ep, alt)
                Fk, epk = Fm[k_of[e]], ep[k_of[e]]
                x1, y1, x2, y2 = c["xy"][u[e], 0], c["xy"][u[e], 1], c["xy"][v[e], 0], c["xy"][v[e], 1]
                a_ = [(Fk[:, r, 0] * x1 + Fk[:, r, 1] * y1) + Fk[:, r, 2] for r in range(3)]
                b_ = [(Fk[:, 0, r] * x2 + Fk[:, 1, r] * y2) + Fk[:, 2, r] for r in range(2)]
                C = (a_[0] * x2 + a_[1] * y2) + a_[2]
                r2 = (C * C) / ((a_[0] * a_[0] + a_[1] * a_[1]) + (b_[0] * b_[0] + b_[1] * b_[1]))
                sig = b_[0] * (epk[:, 1] - epk[:, 2] * y1)
                pre = r2 < o["max_epipolar_error_F"] * o["max_epipolar_error_F"]
                cf = np.where(pre, np.where(sig > 0, 1, 2), 0).astype(np.uint8)
                pos = np.bincount(k_of[e][cf == 1], minlength=npairs); neg = np.bincount(k_of[e][cf == 2], minlength=npairs)
                side = np.where(pos == neg, 0, np.where(pos > neg, 1, 2))
                code[e] = (cf != 0) & (cf == side[k_of[e]])
            e = np.flatnonzero(md == H_)
            if e.size:
                Hk = c["FH"][k_of[e]]
                x1, y1, x2, y2 = c["xy"][u[e], 0], c["xy"][u[e], 1], c["xy"][v[e], 0], c["xy"][v[e], 1]
                h = [(Hk[:, r, 0] * x1 + Hk[:, r, 1] * y1) + Hk[:, r, 2] for r in range(3)]
                d = EPS + h[2]
                uu, vv = h[0] / d - x2, h[1] / d - y2
                code[e] = uu * uu + vv * vv < o["max_epipolar_error_H"] * o["max_epipolar_error_H"]
        ninl = np.bincount(k_of, weights=code, minlength=npairs).astype(np.int32)
        status = np.where(valid, VALID, INVALID_IN).astype(np.int32)
        if o["score"]:
            status[(status == VALID) & (ninl < o["min_inlier_num"])] = FEW_INLIERS
            status[(status == VALID) & (ninl.astype(np.float64) / cnt.astype(np.float64) < o["min_inlier_ratio"])] = LOW_RATIO
        if c["rot"] is not None:
            reg = np.ones(n, dtype=bool) if c["registered_in"] is None else c["registered_in"] != 0
            cs = rotation_cosine(c["rot"][c["pi"]], c["rot"][c["pj"]], c["Rrel"])
            status[(status == VALID) & reg[c["pi"]] & reg[c["pj"]] & (cs < o["cos_max_rotation_error"])] = ROTATION
    # rule 7 by union-find over the valid pairs, the smaller root on top: a component's label is its smallest image
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    linked = np.zeros(n, dtype=bool)
    for k in np.flatnonzero(status == VALID):
        a, b = find(int(c["pi"][k])), find(int(c["pj"][k]))
        linked[c["pi"][k]] = linked[c["pj"][k]] = True
        if a != b:
            parent[max(a, b)] = min(a, b)
    label = np.array([find(i) for i in range(n)], dtype=np.int64)
    sizes = np.bincount(label[linked], minlength=n) if n else np.zeros(0, dtype=np.int64)
    components = int(np.sum(sizes > 0))
    largest = int(sizes.max()) if components else 0
    best = int(np.argmax(sizes)) if components else -1          # (the first maximum: the smallest label)
    registered = (linked & (label == best)).astype(np.uint8)
    status[(status == VALID) & ~((registered[c["pi"]] != 0) & (registered[c["pj"]] != 0))] = OUTSIDE
    return _finish(c, code, ninl, status, registered, largest, components, cnt, limits)


# ------------------------------------------------------------------------------------------------ the recorded case
SIMPLE2 = dict(seed=7, f_share=0.15, f_turned=0.1, h_pairs=8, invalid=20, tilted=12)
H_IMG, W_IMG = 768, 1024


def simple2_case():
    """pass A's inputs of the recorded case: the features, pixels, per-view pinhole K and matches of xm_tracks_numpy.simple2_case() exactly as
    examples/tracks_lift_filter_clean_solve_simple2.py builds them; relative poses from tests/golden/simple2/tp.npz (Rrel = R_j^T R_i,
    trel = R_j^T (t_i - t_j) normalised; a pair with a baseline below 1e-6 is NONE).  With SIMPLE2's seed: a share of the pairs become F pairs
    (F = K_j^-T E K_i^-1), a few H pairs (H = K_j Rrel K_i^-1, the homography of a pure rotation: most of their matches are no inliers), some
    pairs are invalid at input, trel of the pairs with the most matches is tilted by 0.2 .. 3 degrees (few inliers or a low ratio), Rrel of a
    tenth of the F pairs is turned by 15 .. 40 degrees and so is Rrel of every pair (made an F pair) of two images but their own, which pass A
    does not look at and pass B drops: the two leave the largest component and their own pair ends outside it.  -> the case; c["rot_true"]: the cam_from_world rotations of tp.npz for pass B"""
    import xm_tracks_numpy as tn
    G = os.path.join(ROOT, "tests", "golden", "simple2")
    Z = np.load(os.path.join(G, "obs.npz"))
    cam, lm, p = Z["cam"].astype(np.int32), Z["lm"].astype(np.int32), Z["p"]
    n = int(cam.max()) + 1
    K = np.zeros((n, 3, 3)); xy = np.zeros((cam.size, 2))
    for cc in range(n):
        e = np.flatnonzero(cam == cc)
        q = p[e]
        front = q[:, 2] > 0
        tx, ty = np.abs(q[front, 0] / q[front, 2]), np.abs(q[front, 1] / q[front, 2])
        f = 0.95 * min((W_IMG / 2 - 12) / np.percentile(tx, 99), (H_IMG / 2 - 12) / np.percentile(ty, 99))
        K[cc] = [[f, 0.0, W_IMG / 2.0], [0.0, f, H_IMG / 2.0], [0.0, 0.0, 1.0]]
        z = np.where(front, q[:, 2], 1.0)
        xy[e, 0] = np.where(front, f * q[:, 0] / z + W_IMG / 2.0, -5.0); xy[e, 1] = np.where(front, f * q[:, 1] / z + H_IMG / 2.0, -5.0)
    order = np.lexsort((lm, cam))
    base = tn.simple2_case()
    assert base["foff"][-1] == cam.size
    fxy = np.ascontiguousarray(xy[order])
    pi, pj, moff = base["pi"], base["pj"], base["moff"]
    npairs = pi.size
    T = np.load(os.path.join(G, "tp.npz"))
    Rw = np.stack([T["R_real"][:, 3 * i:3 * i + 3] for i in range(n)]); tw = T["t_est"].T
    Rrel = np.einsum("kba,kbc->kac", Rw[pj], Rw[pi])
    base_line = np.einsum("kba,kb->ka", Rw[pj], tw[pi] - tw[pj])
    norm = np.linalg.norm(base_line, axis=1)
    model = np.where(norm < 1e-6, NONE, E_).astype(np.int32)
    trel = np.where(norm[:, None] < 1e-6, 0.0, base_line / np.maximum(norm, 1e-300)[:, None])
    focal = K[:, 0, 0].copy()
    Kinv = np.linalg.inv(K)
    rng = np.random.default_rng(SIMPLE2["seed"])
    cnt = np.diff(moff)
    big = np.flatnonzero((cnt >= 60) & (model == E_))
    # the two images that pass B unregisters: the ends of the large pair whose images have the fewest large pairs.  Their own pair is left
    # as it is, so pass B finds it valid and outside the largest component
    deg = np.bincount(np.concatenate([pi[big], pj[big]]), minlength=n)
    own = big[np.argmin(deg[pi[big]] + deg[pj[big]])]
    gone = np.array([pi[own], pj[own]])
    of_gone = np.isin(pi, gone) | np.isin(pj, gone)
    is_f = (rng.random(npairs) < SIMPLE2["f_share"]) | of_gone
    is_f &= model == E_
    of_gone[own] = False
    turned = is_f & ((rng.random(npairs) < SIMPLE2["f_turned"]) | of_gone)
    rest = np.flatnonzero(~is_f & (model == E_))
    is_h = np.zeros(npairs, dtype=bool); is_h[rng.choice(rest, SIMPLE2["h_pairs"], replace=False)] = True
    FH = np.tile(np.eye(3), (npairs, 1, 1))
    for k in np.flatnonzero(is_f):
        FH[k] = Kinv[pj[k]].T @ essential(Rrel[k], trel[k]) @ Kinv[pi[k]]
    for k in np.flatnonzero(is_h):
        FH[k] = K[pj[k]] @ Rrel[k] @ Kinv[pi[k]]
    model[is_f] = F_; model[is_h] = H_
    for k in np.flatnonzero(turned):
        axis = rng.normal(size=3)
        Rrel[k] = rot_axis(axis, rng.uniform(15.0, 40.0)) @ Rrel[k]
    valid_in = np.ones(npairs, dtype=np.uint8)
    valid_in[rng.choice(np.flatnonzero(~of_gone), SIMPLE2["invalid"], replace=False)] = 0
    tilt = [k for k in np.argsort(-cnt, kind="stable") if model[k] == E_ and valid_in[k]][:SIMPLE2["tilted"]]
    for x, k in enumerate(tilt):
        axis = np.cross(trel[k], [0.3, -0.5, 0.8])
        trel[k] = rot_axis(axis, 0.2 + 2.8 * x / (len(tilt) - 1)) @ trel[k]
    c = dict(foff=base["foff"], xy=fxy, focal=focal, Kinv=np.ascontiguousarray(Kinv), bearing=None, pi=pi, pj=pj, model=model,
             Rrel=np.ascontiguousarray(Rrel), trel=np.ascontiguousarray(trel), FH=np.ascontiguousarray(FH), valid_in=valid_in, registered_in=None, rot=None,
             moff=moff, f1=base["f1"], f2=base["f2"], options={})
    c["rot_true"] = np.ascontiguousarray(np.transpose(Rw, (0, 2, 1)))
    c["gone"] = gone
    return c


def digest(c):
    h = hashlib.sha256()
    for k in ("foff", "xy", "focal", "Kinv", "pi", "pj", "model", "Rrel", "trel", "FH", "valid_in", "moff", "f1", "f2", "rot_true"):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    return h.hexdigest()


def digest_matches(r):
    h = hashlib.sha256()
    for k in ("moff_out", "f1_out", "f2_out"):
        h.update(np.ascontiguousarray(r[k]).tobytes())
    return h.hexdigest()


_CASE = None


def load_case():
    """-> pass A's case, run_numpy of it, pass B's case (fed with the true rotations), run_numpy of it, and the recorded file; computed once"""
    global _CASE
    if _CASE is None:
        a = simple2_case()
        ra = run_numpy(a)
        b = next_pass(a, ra, a["rot_true"])
        rb = run_numpy(b)
        _CASE = (a, ra, b, rb, np.load(os.path.join(GOLDEN, "simple2.npz")))
    return _CASE


# ------------------------------------------------------------------------------------------------ seeded small cases
def random_case(seed):
    """a small scene with planted geometry: random cameras looking at random points (some on a plane), E, F and H pairs with their true
    geometry and with spoiled geometry, NONE pairs, invalid pairs, wrong matches, thresholds small enough that every rule fires somewhere"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(3, 8))
    npts = int(rng.integers(8, 40))
    X = np.concatenate([rng.uniform(-1, 1, (npts, 2)), rng.uniform(4, 6, (npts, 1))], axis=1)
    X[: npts // 3, 2] = 5.0                                                     # a plane z = 5 in the world
    Rw = np.stack([rot_axis(rng.normal(size=3), rng.uniform(0, 12)) for _ in range(n)])      # cam_from_world
    tw = rng.uniform(-0.6, 0.6, (n, 3))
    f = rng.uniform(400, 900, n)
    K = np.stack([np.array([[f[i], 0, 320.0], [0, f[i], 240.0], [0, 0, 1.0]]) for i in range(n)])
    xy = np.zeros((n * npts, 2))
    for i in range(n):
        q = X @ Rw[i].T + tw[i]
        xy[i * npts:(i + 1) * npts] = (q[:, :2] / q[:, 2:3]) * f[i] + [320.0, 240.0]
    xy += rng.normal(scale=0.3, size=xy.shape)
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            if rng.random() < 0.25:
                continue
            a, b = (i, j) if rng.random() < 0.7 else (j, i)
            R = Rw[b] @ Rw[a].T
            t = tw[b] - R @ tw[a]
            t = t / np.linalg.norm(t)
            if rng.random() < 0.2:
                t = -t                                                          # the points are behind: cheirality
            model = int(rng.choice([NONE, E_, E_, F_, F_, H_]))
            idx = rng.permutation(npts)[: int(rng.integers(0, npts + 1))]
            if model == H_:
                idx = idx[idx < npts // 3]
            m = np.stack([idx, idx], axis=1)
            wrong = rng.random(idx.size) < 0.15
            m[wrong, 1] = rng.integers(0, npts, int(wrong.sum()))
            FH = np.eye(3)
            if model == F_:
                FH = np.linalg.inv(K[b]).T @ essential(R, t) @ np.linalg.inv(K[a])
                if rng.random() < 0.15:
                    FH = -FH
                if rng.random() < 0.1:
                    FH[0] = 0.0                                                 # row 0 x row 2 vanishes: the other epipole
            elif model == H_:                                                   # the plane z = 5 of the world seen by a and b
                nw, dw = np.array([0.0, 0.0, 1.0]), 5.0
                na = Rw[a] @ nw; da = dw + na @ tw[a]
                Hn = R + np.outer(tw[b] - R @ tw[a], na) / da
                FH = K[b] @ Hn @ np.linalg.inv(K[a])
            if rng.random() < 0.15:
                R = rot_axis(rng.normal(size=3), rng.uniform(5, 30)) @ R
            pairs.append(dict(i=a, j=b, model=model, m=m, R=R, t=t, FH=FH))
    valid_in = None if rng.random() < 0.3 else (rng.random(len(pairs)) < 0.85).astype(np.uint8)
    c = make_case([npts] * n, xy, pairs, focal=f, Kinv=np.linalg.inv(K), valid_in=valid_in,
                  min_inlier_num=int(rng.integers(0, 6)), min_inlier_ratio=float(rng.choice([0.0, 0.25, 0.5, 0.8])),
                  max_epipolar_error_E=float(rng.choice([1.0, 2.0])), max_epipolar_error_F=float(rng.choice([1.0, 4.0])),
                  max_epipolar_error_H=float(rng.choice([1.5, 4.0])))
    c["rot_true"] = Rw
    if rng.random() < 0.1 and len(pairs):
        c["trel"][0, 1] = np.nan
    return c


# ------------------------------------------------------------------------------------------------ hand-made cases
def plant(R, t, X):
    """the unit bearings of the points X (cam1 frame) in both cameras of the pose (R, t): x2 ~ R X + t"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    X2 = X @ np.asarray(R).T + np.asarray(t)
    return X / np.linalg.norm(X, axis=1, keepdims=True), X2 / np.linalg.norm(X2, axis=1, keepdims=True)


def sizes_case(limits, seed=3):
    """four cameras over points on a plane; E, F and H pairs of every size at which the kernels change their form: 0, 1, 63, 64, 65, 255,
    256, 257 matches, each limit and the limit plus one, and two chunks plus one; 10 % wrong matches, 0.4 px noise"""
    rng = np.random.default_rng(seed)
    wave, group = limits["wave_matches"], limits["group_matches"]
    sizes = sorted({0, 1, 63, 64, 65, 255, 256, 257, wave, wave + 1, group, group + 1, 2 * group + 1})
    npts, n = 2 * group + 1, 4
    X = np.concatenate([rng.uniform(-1.5, 1.5, (npts, 2)), np.full((npts, 1), 5.0)], axis=1)
    Rw = np.stack([rot_axis(rng.normal(size=3), rng.uniform(2, 10)) for _ in range(n)])
    tw = rng.uniform(-0.5, 0.5, (n, 3))
    f = np.array([500.0, 650.0, 800.0, 720.0])
    K = np.stack([np.array([[f[i], 0, 320.0], [0, f[i], 240.0], [0, 0, 1.0]]) for i in range(n)])
    xy = np.zeros((n * npts, 2))
    for i in range(n):
        q = X @ Rw[i].T + tw[i]
        xy[i * npts:(i + 1) * npts] = (q[:, :2] / q[:, 2:3]) * f[i] + [320.0, 240.0]
    xy += rng.normal(scale=0.4, size=xy.shape)
    combos = [(0, 1), (2, 0), (1, 2), (3, 1), (0, 3), (3, 2)]
    pairs = []
    for x, (sz, model) in enumerate((s, m) for s in sizes for m in (E_, F_, H_)):
        a, b = combos[x % len(combos)]
        R = Rw[b] @ Rw[a].T
        t = tw[b] - R @ tw[a]
        t = t / np.linalg.norm(t)
        idx = rng.permutation(npts)[:sz]
        m = np.stack([idx, idx], axis=1)
        wrong = rng.random(sz) < 0.1
        m[wrong, 1] = rng.integers(0, npts, int(wrong.sum()))
        FH = np.eye(3)
        if model == F_:
            FH = np.linalg.inv(K[b]).T @ essential(R, t) @ np.linalg.inv(K[a])
            if x % 2:
                FH = -FH
        elif model == H_:
            na = Rw[a] @ np.array([0.0, 0.0, 1.0]); da = 5.0 + na @ tw[a]
            FH = K[b] @ (R + np.outer(tw[b] - R @ tw[a], na) / da) @ np.linalg.inv(K[a])
        pairs.append(dict(i=a, j=b, model=model, m=m, R=R, t=t, FH=FH))
    c = make_case([npts] * n, xy, pairs, focal=f, Kinv=np.linalg.inv(K), max_epipolar_error_E=2.0)
    c["rot_true"] = Rw
    return c


def essential_edges_case():
    """E pairs between two images, read through `bearing`: a control, the same points with the translation reversed (all behind), trel with
    negative z and matches 2 and 4 degrees from the epipole, depths on either side of 1e-2 * (1 - a^2) and of 100 * (1 - a^2), rays that
    are parallel, a NaN in the rotation and a NaN in the translation.  -> the case and the inlier flags it is built to give"""
    rng = np.random.default_rng(5)
    b1, b2, pairs, want = [], [], [], []

    def add(R, t, x1, x2, flags):
        m = [(len(b1) + k, len(b2) + k) for k in range(len(x1))]
        b1.extend(x1); b2.extend(x2); want.extend(flags)
        pairs.append(dict(i=0, j=1, model=E_, m=m, R=R, t=t))
    R0 = rot_axis([0.2, 1.0, 0.1], 6.0)
    t0 = np.array([1.0, 0.1, 0.2]) / np.linalg.norm([1.0, 0.1, 0.2])
    X = np.concatenate([rng.uniform(-1, 1, (6, 2)), rng.uniform(4, 6, (6, 1))], axis=1)
    x1, x2 = plant(R0, t0, X)
    add(R0, t0, x1, x2, [1] * 6)                                       # the control
    add(R0, -t0, x1, x2, [0] * 6)                                      # the same rays with the baseline reversed: every point is behind
    t1 = np.array([0.2, 0.0, -0.98]) / np.linalg.norm([0.2, 0.0, -0.98])   # e12 = t has a negative z and is flipped; e21 = -t
    side = np.cross(-t1, [0.0, 1.0, 0.0]); side /= np.linalg.norm(side)
    Y = [1.5 * (np.cos(np.radians(d)) * -t1 + np.sin(np.radians(d)) * side) for d in (2.0, 4.0)]
    x1, x2 = plant(np.eye(3), t1, Y)
    add(np.eye(3), t1, x1, x2, [0, 1])                                 # 2 degrees from e21: too close; 4 degrees: an inlier
    ts = np.array([1e-3, 0.0, 0.0])                                    # trel is used as given: a baseline of 1e-3
    x1, x2 = plant(np.eye(3), ts, [[0.0, 0.001, 0.0095], [0.0, 0.001, 0.0105]])
    add(np.eye(3), ts, x1, x2, [0, 1])                                 # depths 0.0095 and 0.0105 around XM_VG_MIN_DEPTH
    tu = np.array([1.0, 0.0, 0.0])
    x1, x2 = plant(np.eye(3), tu, [[0.0, 1.0, 99.0], [0.0, 1.0, 101.0]])
    add(np.eye(3), tu, x1, x2, [1, 0])                                 # depths 99 and 101 around XM_VG_MAX_DEPTH
    x1, _ = plant(np.eye(3), tu, [[0.1, 0.2, 1.0]])
    add(np.eye(3), tu, x1, x1, [0])                                    # the same ray twice: a = -1, no depth
    x1, x2 = plant(R0, t0, X)
    Rn = R0.copy(); Rn[1, 1] = np.nan
    add(Rn, t0, x1, x2, [0] * 6)
    tn_ = t0.copy(); tn_[2] = np.nan
    add(R0, tn_, x1, x2, [0] * 6)
    nf = max(len(b1), len(b2))
    bearing = np.concatenate([np.array(b1), np.array(b2)])
    c = make_case([nf, nf], np.zeros((2 * nf, 2)), pairs, bearing=bearing, min_inlier_num=0, min_inlier_ratio=0.0)
    c["Kinv"] = None
    return c, np.array(want, dtype=np.uint8)


def fundamental_edges_case():
    """F pairs with F = [t]x, t = (0.5, 1, 1): the epipole is (0.5, 1) in both images, a match p1 = e + r1 d, p2 = e + r2 d lies on its
    epipolar line and its signum is positive when r1 and r2 have one sign.  A tie (2 against 2): no inliers; three negative against one
    positive: the three; the opposite; no pre-inlier at all (0 against 0); F = [x]x, whose row 0 vanishes: the epipole of rows 1 and 2, whose
    y and z are 0: every signum is 0, an all-negative majority.  -> the case and the inlier flags it is built to give"""
    e = np.array([0.5, 1.0])
    Ft = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -0.5], [-1.0, 0.5, 0.0]])
    Fx = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    p1, p2, pairs, want = [], [], [], []

    def add(F, rs, flags):
        m = []
        for k, (r1, r2) in enumerate(rs):
            d = np.array([np.cos(0.7 + k), np.sin(0.7 + k)])
            m.append((len(p1), len(p2)))
            p1.append(e + r1 * d); p2.append(e + r2 * d)
        want.extend(flags)
        pairs.append(dict(i=0, j=1, model=F_, m=m, FH=F))
    add(Ft, [(3, 5), (2, 7), (4, -6), (-3, 8)], [0, 0, 0, 0])
    add(Ft, [(3, -5), (-2, 7), (4, -6), (3, 8)], [1, 1, 1, 0])
    add(Ft, [(3, 5), (-2, -7), (4, 6), (3, -8)], [1, 1, 1, 0])
    m = [(len(p1), len(p2)), (len(p1) + 1, len(p2) + 1)]
    p1.extend([e + [30.0, 0.0], e + [0.0, 40.0]]); p2.extend([e + [0.0, 35.0], e + [45.0, 0.0]])   # far from their epipolar lines
    want.extend([0, 0]); pairs.append(dict(i=0, j=1, model=F_, m=m, FH=Ft))
    m = [(len(p1) + k, len(p2) + k) for k in range(3)]
    p1.extend([[10.0, 20.0], [15.0, 7.0], [3.0, 9.0]]); p2.extend([[40.0, 20.0], [-5.0, 7.5], [8.0, 30.0]])   # y2 = y1 is the epipolar line
    want.extend([1, 1, 0]); pairs.append(dict(i=0, j=1, model=F_, m=m, FH=Fx))
    nf = len(p1)
    c = make_case([nf, nf], np.concatenate([np.array(p1), np.array(p2)]), pairs, min_inlier_num=0, min_inlier_ratio=0.0)
    return c, np.array(want, dtype=np.uint8)


def _identity_pairs(spec, n=2, **kw):
    """H = identity pairs over images whose feature a sits at (10 a, 0), plus a last feature far away: a match (a, a) is an inlier, a match
    (a, far) is none.  spec: [(i, j, inliers, outliers, model), ...]"""
    nf = 1 + max([s[2] for s in spec] + [1])
    xy = np.tile(np.stack([np.arange(nf) * 10.0, np.zeros(nf)], axis=1), (n, 1))
    xy[nf - 1::nf] = [5000.0, 5000.0]
    pairs = [dict(i=i, j=j, model=md, m=[(a, a) for a in range(good)] + [(a % (nf - 1), nf - 1) for a in range(bad)]) for i, j, good, bad, md in spec]
    return make_case([nf] * n, xy, pairs, **kw)


def rules_case(min_inlier_num=30):
    """29 against 30 inliers; 30 of 120 (a ratio of exactly 0.25, which stays) against 30 of 121; a NONE pair; a pair invalid at input; a
    pair without matches (FEW_INLIERS, or valid under min_inlier_num = 0: the ratio is NaN)"""
    spec = [(0, 1, 29, 0, H_), (1, 2, 30, 0, H_), (2, 3, 30, 90, H_), (3, 4, 30, 91, H_), (4, 5, 40, 0, NONE), (5, 6, 40, 0, H_), (6, 7, 0, 0, H_),
            (7, 8, 35, 5, H_)]
    valid_in = np.ones(len(spec), dtype=np.uint8); valid_in[5] = 0
    return _identity_pairs(spec, n=9, valid_in=valid_in, min_inlier_num=min_inlier_num)


def rotation_case(with_rot=True):
    """pass B over five images in a ring with planted rotations: exact relative rotations but a pair turned by 20 degrees, whose cosine IS
    the threshold (it stays), a pair turned by 25 degrees (ROTATION), and a pair turned by 40 degrees with an unregistered end (skipped)"""
    rng = np.random.default_rng(9)
    n = 6
    rot = np.stack([rot_axis(rng.normal(size=3), rng.uniform(0, 90)) for _ in range(n)])
    ring = [(0, 1, 0.0), (1, 2, 20.0), (2, 3, 25.0), (3, 0, 0.0), (0, 2, 0.0), (3, 4, 40.0), (4, 0, 0.0), (1, 3, 0.0)]
    pairs = [dict(i=i, j=j, model=E_, R=rot_axis([0.3, -0.2, 0.9], d) @ rot[j] @ rot[i].T) for i, j, d in ring]
    reg = np.array([1, 1, 1, 1, 0, 1], dtype=np.uint8)
    c = make_case([1] * n, np.zeros((n, 2)), pairs, registered_in=reg, rot=rot if with_rot else None, score=False)
    c["options"]["cos_max_rotation_error"] = float(rotation_cosine(rot[[1]], rot[[2]], c["Rrel"][[1]])[0])
    return c


def graph_case(n, edges, valid_in=None):
    """pass B without rotations over images that have no feature: rule 7 alone"""
    return make_case([0] * n, np.zeros((0, 2)), [dict(i=i, j=j, model=E_) for i, j in edges], valid_in=valid_in, score=False)


def gpu_cases(limits):
    """name -> case, for tests/test_gpu_viewgraph.py (and, against restatement (a), tests/test_viewgraph_numpy.py)"""
    rng = np.random.default_rng(2)
    chain = rng.permutation(1500)
    return {
        "sizes": sizes_case(limits),
        "essential_edges": essential_edges_case()[0],
        "fundamental_edges": fundamental_edges_case()[0],
        "homography": _identity_pairs([(0, 1, 12, 3, H_), (1, 0, 5, 5, H_)], min_inlier_num=0),
        "rules": rules_case(),
        "rules_no_minimum": rules_case(0),
        "rotation": rotation_case(),
        "rotation_off": rotation_case(False),
        "chain": graph_case(1500, [(int(chain[k]), int(chain[k + 1])) for k in range(1499)]),
        "two_equal": graph_case(9, [(5, 6), (6, 7), (1, 3), (3, 8), (0, 2)]),
        "none_valid": graph_case(4, [(0, 1), (2, 3)], valid_in=[0, 0]),
        "isolated_twice": graph_case(7, [(1, 4), (4, 1), (1, 4), (5, 6), (4, 2)]),
    }
