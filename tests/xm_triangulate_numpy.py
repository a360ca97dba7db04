"""The contract of the track triangulation (include/xm_amd.h at xm_ctx_triangulate_tracks; xm-code_amd/csrc/xm_triangulate.hip), twice:

(a) run_sequential   plain Python loops over one landmark at a time, on Python floats, candidates picked out of the list one by one;
(b) run_numpy        the same operations on arrays, all landmarks of one list length at a time, non-candidates carried as NaN rays.
                     The GPU tests compare with this, exactly.

NOTHING HERE WAS COMPARED WITH THE REFERENCE'S COMPILED CODE: the reference's fork of GLOMAP only calls COLMAP's
IncrementalMapper::TriangulateImage and CompleteAndMergeTracks (controllers/track_retriangulation.cc), and COLMAP's sources are not part of
it.  The contract is this project's own, modelled on the structure of COLMAP's triangulator as GLOMAP configures it: create from two-view
samples under an angular error, refine linearly, complete under a reprojection error, require a minimum triangulation angle.

Every product and sum is rounded on its own, x . y = (x0 y0 + x1 y1) + x2 y2, |x| = sqrt(x . x), and a sum over a landmark's list is the
pairwise tree over the positions padded with +0.0 to a power of two, adjacent pairs first (tree_sum).  The scenes are those of
tests/xm_trackfilter_numpy.py."""
import numpy as np

from xm_trackfilter_numpy import EPS, _nan_div, _sqrt, cos_deg

LM_ACCEPTED, LM_UNUSED, LM_NO_HYPOTHESIS, LM_DEGENERATE, LM_MIN_VIEWS, LM_ANGLE = 0, 1, 2, 3, 4, 5
REASON_NOT_CANDIDATE, REASON_NOT_MEMBER, REASON_LANDMARK = 1, 2, 4
COUNTS = ("lm_accepted", "lm_unused", "lm_no_hypothesis", "lm_degenerate", "lm_min_views", "lm_angle", "obs_candidates", "obs_kept",
          "obs_readmitted", "obs_lost", "pairs_tested", "hypotheses_scored")
ARRAYS = ("p", "keep", "reason", "lm_views", "lm_status", "lm_support", "lm_hypothesis")
DEFAULTS = dict(max_hypotheses=64, min_angle=1.0, create_angle=2.0, complete_reprojection=1e-2, min_views=2, refine_rounds=2)


def schedule(L, max_hypotheses=None):
    """the unordered pairs of positions 0 .. L-1 in the order they are tried: d = 1 .. L // 2, a = 0 .. L-1, (a, (a + d) mod L); for
    2 d = L only a < L / 2; cut at max_hypotheses"""
    out = []
    for d in range(1, L // 2 + 1):
        for a in range(L):
            if 2 * d == L and a >= L // 2:
                break
            if max_hypotheses is not None and len(out) >= max_hypotheses:
                return out
            out.append((a, (a + d) % L))
    return out


def pair_of(h, L):
    """entry h of schedule(L) in closed form (what the kernels compute)"""
    d = h // L + 1
    a = h - (d - 1) * L
    return a, (a + d) % L


def n_pairs(L, max_hypotheses):
    return min(int(max_hypotheses), L * (L - 1) // 2)


def tree_sum(x):
    """x: list of floats -> the pairwise tree over the list padded with +0.0 to a power of two, adjacent pairs first"""
    x = list(x)
    n = 1
    while n < len(x):
        n *= 2
    x += [0.0] * (n - len(x))
    while len(x) > 1:
        x = [x[i] + x[i + 1] for i in range(0, len(x), 2)]
    return x[0]


def tree_sum_axis1(x):
    """the same along axis 1 of an array"""
    n = 1
    while n < x.shape[1]:
        n *= 2
    if n != x.shape[1]:
        x = np.concatenate([x, np.zeros((x.shape[0], n - x.shape[1]) + x.shape[2:])], axis=1)
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _options(kw):
    o = dict(DEFAULTS)
    o.update(kw)
    cos_min = o.pop("cos_min_angle", None); cos_create = o.pop("cos_create", None)
    o["cos_min"] = cos_deg(o["min_angle"]) if cos_min is None else cos_min
    o["cos_create"] = cos_deg(o["create_angle"]) if cos_create is None else cos_create
    return o


def _candidates(S, candidates):
    if candidates is None:
        mask = S["w"] > 0
    else:
        c = np.asarray(candidates).reshape(-1)
        mask = c if c.dtype == bool else c > 0
    return mask & (S["p"][:, 2] > 0)


def _finish(S, out, P, keep, cand, status, views, support, hyp):
    lm = S["lm"]
    used = (S["w"] > 0) & (S["p"][:, 2] > 0)
    reason = np.zeros(lm.size, dtype=np.uint8)
    reason[~cand] = REASON_NOT_CANDIDATE
    acc = status[lm] == LM_ACCEPTED
    reason[cand & acc & ~keep] = REASON_NOT_MEMBER
    reason[cand & ~acc] = REASON_LANDMARK
    for k, v in (("lm_accepted", LM_ACCEPTED), ("lm_unused", LM_UNUSED), ("lm_no_hypothesis", LM_NO_HYPOTHESIS), ("lm_degenerate", LM_DEGENERATE),
                 ("lm_min_views", LM_MIN_VIEWS), ("lm_angle", LM_ANGLE)):
        out[k] = int((status == v).sum())
    out["obs_candidates"] = int(cand.sum()); out["obs_kept"] = int(keep.sum())
    out["obs_readmitted"] = int((keep & ~(S["w"] > 0)).sum()); out["obs_lost"] = int((used & ~keep).sum())
    out.update(p=P, keep=keep, reason=reason, lm_views=views, lm_status=status, lm_support=support, lm_hypothesis=hyp)
    return out


# ------------------------------------------------------------------------------------------------ (a) sequential
def _ray(S, e):
    """(b, c, R^T as rows, u, v) of observation e"""
    i = int(S["cam"][e])
    p = [float(x) for x in S["p"][e]]
    u, v = _nan_div(p[0], p[2]), _nan_div(p[1], p[2])
    R = [[float(S["rot"][r, 3 * i + c]) for c in range(3)] for r in range(3)]
    g = [(R[r][0] * u + R[r][1] * v) + R[r][2] for r in range(3)]
    ng = _sqrt(_dot(g, g))
    return dict(b=[_nan_div(x, ng) for x in g], c=[float(S["t"][r, i]) for r in range(3)], R=R, u=u, v=v)


def _two_view(ra, rb, cos_min):
    """the midpoint of the two closest points of two rays, or None when the pair is no hypothesis"""
    b1, c1, b2, c2 = ra["b"], ra["c"], rb["b"], rb["c"]
    cs = _dot(b1, b2)
    if not cs < cos_min:
        return None
    w = [c2[k] - c1[k] for k in range(3)]
    d1, d2 = _dot(b1, w), _dot(b2, w)
    den = 1.0 - cs * cs
    if not den > 0.0:
        return None
    s = (d1 - cs * d2) / den; t = (cs * d1 - d2) / den
    if not (s > 0.0 and t > 0.0):
        return None
    return [0.5 * ((c1[k] + s * b1[k]) + (c2[k] + t * b2[k])) for k in range(3)]


def _supports(r, X, cos_create):
    dx = [X[k] - r["c"][k] for k in range(3)]
    return _nan_div(_dot(dx, r["b"]), _sqrt(_dot(dx, dx))) > cos_create


def _is_member(r, X, thr):
    d = [X[k] - r["c"][k] for k in range(3)]
    q = [(r["R"][0][a] * d[0] + r["R"][1][a] * d[1]) + r["R"][2][a] * d[2] for a in range(3)]
    if not q[2] >= EPS:
        return False
    uu = q[0] / q[2] - r["u"]; vv = q[1] / q[2] - r["v"]
    return _sqrt(uu * uu + vv * vv) < thr


def _solve(rays, members, L):
    """X = A^-1 r over the members (positions of the list; the others are +0.0 terms), or None"""
    terms = [[0.0] * L for _ in range(9)]
    for k in members:
        b, c = rays[k]["b"], rays[k]["c"]
        sc = _dot(b, c)
        vals = (1.0 - b[0] * b[0], 0.0 - b[0] * b[1], 0.0 - b[0] * b[2], 1.0 - b[1] * b[1], 0.0 - b[1] * b[2], 1.0 - b[2] * b[2],
                (c[0] - b[0] * sc) + 0.0, (c[1] - b[1] * sc) + 0.0, (c[2] - b[2] * sc) + 0.0)
        for j in range(9):
            terms[j][k] = vals[j]
    A00, A01, A02, A11, A12, A22, r0, r1, r2 = (tree_sum(t) for t in terms)
    k00 = A11 * A22 - A12 * A12; k01 = A02 * A12 - A01 * A22; k02 = A01 * A12 - A02 * A11
    k11 = A00 * A22 - A02 * A02; k12 = A01 * A02 - A00 * A12; k22 = A00 * A11 - A01 * A01
    det = (A00 * k00 + A01 * k01) + A02 * k02
    if not (det > 0.0 and det < float("inf")):
        return None
    return [((k00 * r0 + k01 * r1) + k02 * r2) / det, ((k01 * r0 + k11 * r1) + k12 * r2) / det, ((k02 * r0 + k12 * r1) + k22 * r2) / det]


def run_sequential(S, candidates=None, **kw):
    o = _options(kw)
    lm, m = S["lm"], S["P"].shape[1]
    cand = _candidates(S, candidates)
    P = np.array(S["P"], dtype=np.float64, order="C", copy=True)
    keep = np.zeros(lm.size, dtype=bool)
    status = np.full(m, LM_UNUSED, dtype=np.uint8); views = np.zeros(m, dtype=np.int32)
    support = np.zeros(m, dtype=np.int32); hyp = np.full(m, -1, dtype=np.int32)
    out = {k: 0 for k in COUNTS}
    lists = [[] for _ in range(m)]
    for e in range(lm.size):
        lists[int(lm[e])].append(e)                       # the by-landmark list: input order
    for l in range(m):
        obs = lists[l]; L = len(obs)
        rays = {k: _ray(S, e) for k, e in enumerate(obs) if cand[e]}
        if not rays:
            continue
        status[l] = LM_NO_HYPOTHESIS
        if len(rays) < 2:
            continue
        best, best_h, best_X = -1, -1, None
        for h, (a, b) in enumerate(schedule(L, o["max_hypotheses"])):
            out["pairs_tested"] += 1
            if a not in rays or b not in rays:
                continue
            X = _two_view(rays[a], rays[b], o["cos_min"])
            if X is None:
                continue
            out["hypotheses_scored"] += 1
            n = sum(1 for r in rays.values() if _supports(r, X, o["cos_create"]))
            if n > best:
                best, best_h, best_X = n, h, X
        if best_h < 0:
            continue
        support[l], hyp[l] = best, best_h
        if best < 2:
            continue
        members = [k for k, r in rays.items() if _supports(r, best_X, o["cos_create"])]
        X, st = None, LM_ACCEPTED
        for _ in range(o["refine_rounds"]):
            if len(members) < 2:
                st = LM_MIN_VIEWS
                break
            X = _solve(rays, members, L)
            if X is None:
                st = LM_DEGENERATE
                break
            members = [k for k, r in rays.items() if _is_member(r, X, o["complete_reprojection"])]
        if st == LM_ACCEPTED and len(members) < max(o["min_views"], 2):
            st = LM_MIN_VIEWS
        if st == LM_ACCEPTED and not any(_dot(rays[i]["b"], rays[j]["b"]) < o["cos_min"] for i in members for j in members if i < j):
            st = LM_ANGLE
        status[l] = st
        if st == LM_ACCEPTED:
            P[:, l] = X
            views[l] = len(members)
            for k in members:
                keep[obs[k]] = True
    return _finish(S, out, P, keep, cand, status, views, support, hyp)


# ------------------------------------------------------------------------------------------------ (b) vectorised
def _vdot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _group(S, cand, idx, o, P, keep, status, views, support, hyp, ls, out):
    """all landmarks ls (G of them) with L observations each; idx: (G, L) observations by position"""
    G, L = idx.shape
    cam = S["cam"][idx]
    p = S["p"][idx]
    ok = cand[idx]
    with np.errstate(all="ignore"):
        u = p[..., 0] / p[..., 2]; v = p[..., 1] / p[..., 2]
        R = np.ascontiguousarray(S["rot"].T).reshape(-1, 3, 3)[cam]          # R[g, k, c, r] = R_i[r][c]
        g = np.stack([(R[..., 0, r] * u + R[..., 1, r] * v) + R[..., 2, r] for r in range(3)], axis=-1)
        B = g / np.sqrt(_vdot(g, g))[..., None]
        B[~ok] = np.nan
        C = np.ascontiguousarray(S["t"].T)[cam]
        ncand = ok.sum(axis=1)
        status[ls[ncand > 0]] = LM_NO_HYPOTHESIS
        go = ncand >= 2
        H = n_pairs(L, o["max_hypotheses"])
        out["pairs_tested"] += int(go.sum()) * H
        best = np.full(G, -1, dtype=np.int64); best_h = np.full(G, -1, dtype=np.int64); best_X = np.zeros((G, 3))
        for h in range(H):
            a, b = pair_of(h, L)
            b1, c1, b2, c2 = B[:, a], C[:, a], B[:, b], C[:, b]
            cs = _vdot(b1, b2)
            w = c2 - c1
            d1, d2 = _vdot(b1, w), _vdot(b2, w)
            den = 1.0 - cs * cs
            s = (d1 - cs * d2) / den; t = (cs * d1 - d2) / den
            valid = go & (cs < o["cos_min"]) & (den > 0.0) & (s > 0.0) & (t > 0.0)
            if not valid.any():
                continue
            X = 0.5 * ((c1 + s[:, None] * b1) + (c2 + t[:, None] * b2))
            dx = X[:, None, :] - C
            n = ((_vdot(dx, B) / np.sqrt(_vdot(dx, dx))) > o["cos_create"]).sum(axis=1)
            out["hypotheses_scored"] += int(valid.sum())
            better = valid & (n > best)
            best[better] = n[better]; best_h[better] = h; best_X[better] = X[better]
        have = best_h >= 0
        support[ls[have]] = best[have]; hyp[ls[have]] = best_h[have]
        act = have & (best >= 2)
        dx = best_X[:, None, :] - C
        mem = ((_vdot(dx, B) / np.sqrt(_vdot(dx, dx))) > o["cos_create"]) & act[:, None]
        st = np.full(G, LM_ACCEPTED, dtype=np.uint8)
        X = np.zeros((G, 3))
        for _ in range(o["refine_rounds"]):
            few = act & (mem.sum(axis=1) < 2)
            st[few] = LM_MIN_VIEWS; act = act & ~few
            sc = _vdot(B, C)
            terms = np.stack([1.0 - B[..., 0] * B[..., 0], 0.0 - B[..., 0] * B[..., 1], 0.0 - B[..., 0] * B[..., 2], 1.0 - B[..., 1] * B[..., 1],
                              0.0 - B[..., 1] * B[..., 2], 1.0 - B[..., 2] * B[..., 2], (C[..., 0] - B[..., 0] * sc) + 0.0,
                              (C[..., 1] - B[..., 1] * sc) + 0.0, (C[..., 2] - B[..., 2] * sc) + 0.0], axis=-1)
            terms = np.where(mem[..., None], terms, 0.0)
            A00, A01, A02, A11, A12, A22, r0, r1, r2 = tree_sum_axis1(terms).T
            k00 = A11 * A22 - A12 * A12; k01 = A02 * A12 - A01 * A22; k02 = A01 * A12 - A02 * A11
            k11 = A00 * A22 - A02 * A02; k12 = A01 * A02 - A00 * A12; k22 = A00 * A11 - A01 * A01
            det = (A00 * k00 + A01 * k01) + A02 * k02
            bad = act & ~((det > 0.0) & (det < np.inf))
            st[bad] = LM_DEGENERATE; act = act & ~bad
            X = np.stack([((k00 * r0 + k01 * r1) + k02 * r2) / det, ((k01 * r0 + k11 * r1) + k12 * r2) / det,
                          ((k02 * r0 + k12 * r1) + k22 * r2) / det], axis=1)
            d = X[:, None, :] - C
            q = [(R[..., a, 0] * d[..., 0] + R[..., a, 1] * d[..., 1]) + R[..., a, 2] * d[..., 2] for a in range(3)]
            uu = q[0] / q[2] - u; vv = q[1] / q[2] - v
            mem = ok & (q[2] >= EPS) & (np.sqrt(uu * uu + vv * vv) < o["complete_reprojection"]) & act[:, None]
        nm = mem.sum(axis=1)
        few = act & (nm < max(o["min_views"], 2))
        st[few] = LM_MIN_VIEWS; act = act & ~few
        found = np.zeros(G, dtype=bool)
        for i in range(L - 1):
            dots = _vdot(B[:, i:i + 1], B[:, i + 1:])
            found |= (mem[:, i:i + 1] & mem[:, i + 1:] & (dots < o["cos_min"])).any(axis=1)
        flat = act & ~found
        st[flat] = LM_ANGLE; act = act & ~flat
    decided = have & (best >= 2)
    status[ls[decided]] = st[decided]
    P[:, ls[act]] = X[act].T
    views[ls[act]] = nm[act]
    keep[idx[mem & act[:, None]]] = True


def run_numpy(S, candidates=None, **kw):
    """the contract; cos_min_angle / cos_create: the thresholds themselves where the caller has them (the library returns the ones it used)"""
    o = _options(kw)
    lm, m = S["lm"], S["P"].shape[1]
    cand = _candidates(S, candidates)
    P = np.array(S["P"], dtype=np.float64, order="C", copy=True)
    keep = np.zeros(lm.size, dtype=bool)
    status = np.full(m, LM_UNUSED, dtype=np.uint8); views = np.zeros(m, dtype=np.int32)
    support = np.zeros(m, dtype=np.int32); hyp = np.full(m, -1, dtype=np.int32)
    out = {k: 0 for k in COUNTS}
    deg = np.bincount(lm, minlength=m)
    pos = np.argsort(lm, kind="stable")                       # the by-landmark lists: input order within a landmark
    start = np.concatenate([[0], np.cumsum(deg)])
    for L in np.unique(deg[deg > 0]):
        ls = np.nonzero(deg == L)[0]
        idx = pos[start[ls][:, None] + np.arange(L)[None, :]]
        _group(S, cand, idx, o, P, keep, status, views, support, hyp, ls, out)
    return _finish(S, out, P, keep, cand, status, views, support, hyp)


def same(a, b):
    """every output and counter of two runs, exactly (p by its bytes); returns the names that differ"""
    bad = [k for k in COUNTS if int(a[k]) != int(b[k])]
    for k in ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad.append(k)
    return bad
