"""Restatements of the track filter (include/xm_amd.h at xm_ctx_filter_tracks; xm-code_amd/csrc/xm_trackfilter.hip) and of the loop that
drives it (Context.refine_filtered), and the scenes the tests run them on.

(a) run_sequential   Python loops that follow the reference's deps/glomap/glomap/processors/track_filter.cc line by line (the line numbers
                     stand in the comments) over dict-of-lists tracks, with the `counter` each filter returns.
(b) run_numpy        the vectorised contract with the operation order of the header: every product and sum rounded on its own, rows of
                     R^T d left to right, x . y = (x0 y0 + x1 y1) + x2 y2, |x| = sqrt(x . x).  The GPU tests compare with this, exactly.
    refine_loop      the control flow of controllers/global_mapper.cc:243-317 over injected callables.

NOTHING HERE WAS COMPARED WITH THE REFERENCE'S COMPILED CODE (it needs COLMAP, Eigen and glog).  Departures, as the header lists them: the
observed point is p / p_2 without `+ EPS` in the denominator (:29); every camera counts as calibrated (:73-75); a track is a landmark with a
used observation (weight > 0 and p_2 > 0, the bundle adjustment's rule)."""
import math

import numpy as np

EPS = 1e-12                      # glomap/math (track_filter.cc:20, :70)
REASON_DEPTH, REASON_REPROJECTION, REASON_ANGLE, REASON_TRIANGULATION, REASON_MIN_VIEWS = 1, 2, 4, 8, 16
LM_KEPT, LM_UNUSED, LM_TRIANGULATION, LM_MIN_VIEWS = 0, 1, 2, 3
COUNTS = ("tracks_total", "tracks_kept", "obs_used", "obs_kept", "dropped_depth", "dropped_reprojection", "dropped_angle", "dropped_triangulation",
          "dropped_min_views", "tracks_changed_reprojection", "tracks_changed_angle", "tracks_changed_triangulation", "tracks_changed_min_views")
LIGHT_MAX = 64                   # xm_track_filter_limits()[0]: longer landmarks get a workgroup (the GPU test checks the two against the library)
TILE = 256                       # ... [1]: rays per LDS tile


def cos_deg(angle):
    """cos(DegToRad(angle)) as the library computes it on the host (xm_capi.hip): the threshold the kernels compare against"""
    return None if angle is None else math.cos(angle * (3.14159265358979323846 / 180.0))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


# ------------------------------------------------------------------------------------------------ (a) sequential
def _cam_from_world(S, i, l):
    """d = P_l - t_i and q = R_i^T d (image.cam_from_world * track.xyz, :19, :69)"""
    rot, t, P = S["rot"], S["t"], S["P"]
    d = [float(P[c, l]) - float(t[c, i]) for c in range(3)]
    q = [(float(rot[0, 3 * i + a]) * d[0] + float(rot[1, 3 * i + a]) * d[1]) + float(rot[2, 3 * i + a]) * d[2] for a in range(3)]
    return d, q


def _nan_div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan


def _by_reprojection(S, tracks, reason, thr):
    counter = 0                                                                  # :14
    for l, obs in tracks.items():                                                # :15
        new = []                                                                 # :16
        for e in obs:                                                            # :17
            _, q = _cam_from_world(S, int(S["cam"][e]), l)                       # :18-19
            if q[2] < EPS:                                                       # :20
                reason[e] = REASON_DEPTH
                continue
            p = [float(x) for x in S["p"][e]]
            u = _nan_div(q[0], q[2]) - _nan_div(p[0], p[2])                      # :27-29 (no + EPS: the bundle adjustment's observed point)
            v = _nan_div(q[1], q[2]) - _nan_div(p[1], p[2])
            err = _sqrt(u * u + v * v)                                           # :30
            if err < thr:                                                        # :39
                new.append(e)                                                    # :40
            else:
                reason[e] = REASON_REPROJECTION
        if len(new) != len(obs):                                                 # :43
            counter += 1                                                         # :44
            tracks[l] = new                                                      # :45
    return counter                                                               # :50


def _by_angle(S, tracks, reason, thres):
    counter = 0                                                                  # :59  (thres = cos(DegToRad(max_angle_error)), :60)
    for l, obs in tracks.items():                                                # :62
        new = []                                                                 # :63
        for e in obs:                                                            # :64
            _, q = _cam_from_world(S, int(S["cam"][e]), l)                       # :65-69
            if q[2] < EPS:                                                       # :70
                reason[e] = REASON_DEPTH
                continue
            nq = _sqrt(_dot(q, q))                                               # :72
            qn = [_nan_div(x, nq) for x in q]
            p = [float(x) for x in S["p"][e]]
            npn = _sqrt(_dot(p, p))                                              # features_undist holds unit vectors (:67-68)
            pn = [_nan_div(x, npn) for x in p]
            if _dot(qn, pn) > thres:                                             # :77 (every camera calibrated: thres, never thres_uncalib)
                new.append(e)                                                    # :78
            else:
                reason[e] = REASON_ANGLE
        if len(new) != len(obs):                                                 # :81
            counter += 1                                                         # :82
            tracks[l] = new                                                      # :83
    return counter                                                               # :88


def _by_triangulation(S, tracks, reason, status, thres):
    counter = 0                                                                  # :96  (thres = cos(DegToRad(min_angle)), :97)
    for l, obs in tracks.items():                                                # :98
        pts = []                                                                 # :100
        for e in obs:                                                            # :102
            d, _ = _cam_from_world(S, int(S["cam"][e]), l)                       # :104 (track.xyz - image.Center())
            nd = _sqrt(_dot(d, d))
            pts.append([_nan_div(x, nd) for x in d])                             # .normalized(), :105
        ok = False                                                               # :107
        for i in range(len(obs)):                                                # :108
            for j in range(i + 1, len(obs)):                                     # :109
                if _dot(pts[i], pts[j]) < thres:                                 # :110
                    ok = True                                                    # :111
                    break                                                        # :112
            if ok:
                break            # (the reference goes on with the next i; the status cannot change any more)
        if not ok:                                                               # :118
            counter += 1                                                         # :119 (also for a track that is empty already)
            for e in obs:
                reason[e] = REASON_TRIANGULATION
            tracks[l] = []                                                       # :120
            status[l] = LM_TRIANGULATION
    return counter                                                               # :125


def run_sequential(S, reprojection=None, angle=None, triangulation=None, min_views=0):
    """the filters that are switched on, one after the other in the order of the header; angle / triangulation in degrees"""
    nobs, m = S["cam"].size, S["P"].shape[1]
    used = (S["w"] > 0) & (S["p"][:, 2] > 0)
    tracks = {}
    for e in range(nobs):                                    # a track: the used observations of a landmark, in input order
        if used[e]:
            tracks.setdefault(int(S["lm"][e]), []).append(e)
    reason = np.zeros(nobs, dtype=np.uint8)
    status = np.full(m, LM_UNUSED, dtype=np.uint8)
    status[list(tracks)] = LM_KEPT
    out = {k: 0 for k in COUNTS}
    out["tracks_total"] = len(tracks); out["obs_used"] = int(used.sum())
    if reprojection is not None:
        out["tracks_changed_reprojection"] = _by_reprojection(S, tracks, reason, reprojection)
    if angle is not None:
        out["tracks_changed_angle"] = _by_angle(S, tracks, reason, cos_deg(angle))
    if triangulation is not None:
        out["tracks_changed_triangulation"] = _by_triangulation(S, tracks, reason, status, cos_deg(triangulation))
    if min_views > 0:
        for l, obs in tracks.items():
            if 0 < len(obs) < min_views:
                out["tracks_changed_min_views"] += 1
                for e in obs:
                    reason[e] = REASON_MIN_VIEWS
                tracks[l] = []
                status[l] = LM_MIN_VIEWS
    views = np.zeros(m, dtype=np.int32)
    for l, obs in tracks.items():
        views[l] = len(obs)
    return _finish(out, used, reason, views, status)


def _finish(out, used, reason, views, status):
    keep = used & (reason == 0)
    out["obs_kept"] = int(keep.sum()); out["tracks_kept"] = int((views > 0).sum())
    for name, bit in (("depth", REASON_DEPTH), ("reprojection", REASON_REPROJECTION), ("angle", REASON_ANGLE), ("triangulation", REASON_TRIANGULATION),
                      ("min_views", REASON_MIN_VIEWS)):
        out["dropped_" + name] = int((reason == bit).sum())
    out.update(keep=keep, reason=reason, lm_views=views, lm_status=status)
    return out


# ------------------------------------------------------------------------------------------------ (b) vectorised
def _vdot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def geometry(S):
    """d (nobs x 3), q = R^T d (nobs x 3) in the contract's operation order, and the used flags"""
    cam, lm = S["cam"], S["lm"]
    d = np.ascontiguousarray(S["P"].T)[lm] - np.ascontiguousarray(S["t"].T)[cam]
    RT = np.ascontiguousarray(S["rot"].T).reshape(-1, 3, 3)[cam]     # RT[e, a, c] = R_i[c][a]
    q = np.stack([(RT[:, a, 0] * d[:, 0] + RT[:, a, 1] * d[:, 1]) + RT[:, a, 2] * d[:, 2] for a in range(3)], axis=1)
    return d, q, (S["w"] > 0) & (S["p"][:, 2] > 0)


def reprojection_error(S, q):
    p = S["p"]
    with np.errstate(all="ignore"):
        u = q[:, 0] / q[:, 2] - p[:, 0] / p[:, 2]; v = q[:, 1] / q[:, 2] - p[:, 1] / p[:, 2]
        return np.sqrt(u * u + v * v)


def angle_cosine(S, q):
    p = S["p"]
    with np.errstate(all="ignore"):
        return _vdot(q / np.sqrt(_vdot(q, q))[:, None], p / np.sqrt(_vdot(p, p))[:, None])


def rays(d):
    with np.errstate(all="ignore"):
        return d / np.sqrt(_vdot(d, d))[:, None]


def _pair_found(r, idx, thr, budget=1 << 22):
    """idx: (L, k) positions of the survivors of L landmarks with k of them each -> bool per landmark: some pair i < j with r_i . r_j < thr"""
    L, k = idx.shape
    found = np.zeros(L, dtype=bool)
    if k < 2:
        return found
    with np.errstate(all="ignore"):
        if k * k <= budget:
            upper = np.triu(np.ones((k, k), dtype=bool), 1)
            step = max(1, budget // (k * k))
            for a in range(0, L, step):
                x, y, z = (r[idx[a:a + step], c] for c in range(3))
                G = (x[:, :, None] * x[:, None, :] + y[:, :, None] * y[:, None, :]) + z[:, :, None] * z[:, None, :]
                found[a:a + step] = ((G < thr) & upper).any(axis=(1, 2))
        else:                                                # one long landmark at a time, a block of rows at a time
            rows = max(1, budget // k)
            for a in range(L):
                x, y, z = (r[idx[a], c] for c in range(3))
                for i0 in range(0, k, rows):
                    i1 = min(k, i0 + rows)
                    G = (x[i0:i1, None] * x[None, :] + y[i0:i1, None] * y[None, :]) + z[i0:i1, None] * z[None, :]
                    if ((G < thr) & (np.arange(k)[None, :] > np.arange(i0, i1)[:, None])).any():
                        found[a] = True
                        break
    return found


def run_numpy(S, reprojection=None, angle=None, triangulation=None, min_views=0, cos_angle=None, cos_triangulation=None):
    """the contract.  angle / triangulation in degrees; cos_angle / cos_triangulation: the thresholds themselves where the caller has them
    (the library returns the ones it used)"""
    nobs, m = S["cam"].size, S["P"].shape[1]
    lm = S["lm"]
    d, q, used = geometry(S)
    ca = cos_angle if cos_angle is not None else cos_deg(angle)
    ct = cos_triangulation if cos_triangulation is not None else cos_deg(triangulation)
    reason = np.zeros(nobs, dtype=np.uint8)
    alive = used.copy()
    out = {k: 0 for k in COUNTS}
    n_used = np.bincount(lm[used], minlength=m)
    out["tracks_total"] = int((n_used > 0).sum()); out["obs_used"] = int(used.sum())
    if reprojection is not None or angle is not None:
        depth = alive & (q[:, 2] < EPS)
        reason[depth] = REASON_DEPTH
        alive &= ~depth
    else:
        depth = np.zeros(nobs, dtype=bool)
    if reprojection is not None:
        bad = alive & ~(reprojection_error(S, q) < reprojection)
        reason[bad] = REASON_REPROJECTION
        alive &= ~bad
        out["tracks_changed_reprojection"] = int((np.bincount(lm[bad | depth], minlength=m) > 0).sum())
    if angle is not None:
        bad = alive & ~(angle_cosine(S, q) > ca)
        reason[bad] = REASON_ANGLE
        alive &= ~bad
        first = bad | depth if reprojection is None else bad
        out["tracks_changed_angle"] = int((np.bincount(lm[first], minlength=m) > 0).sum())
    status = np.where(n_used > 0, LM_KEPT, LM_UNUSED).astype(np.uint8)
    views = np.bincount(lm[alive], minlength=m).astype(np.int32)
    if triangulation is not None:
        r = rays(d)
        found = np.zeros(m, dtype=bool)
        pos = np.nonzero(alive)[0]
        pos = pos[np.argsort(lm[pos], kind="stable")]        # the survivors by landmark, in input order within one
        start = np.concatenate([[0], np.cumsum(views)])
        for k in np.unique(views[views >= 2]):
            ls = np.nonzero(views == k)[0]
            idx = pos[start[ls][:, None] + np.arange(k)[None, :]]
            found[ls] = _pair_found(r, idx, ct)
        fail = (n_used > 0) & ~found
        out["tracks_changed_triangulation"] = int(fail.sum())
        status[fail] = LM_TRIANGULATION
        hit = alive & fail[lm]
        reason[hit] = REASON_TRIANGULATION
        alive &= ~hit
        views[fail] = 0
    if min_views > 0:
        fail = (views > 0) & (views < min_views)
        out["tracks_changed_min_views"] = int(fail.sum())
        status[fail] = LM_MIN_VIEWS
        hit = alive & fail[lm]
        reason[hit] = REASON_MIN_VIEWS
        views[fail] = 0
    return _finish(out, used, reason, views, status)


def same(a, b):
    """every output and counter of two runs, exactly; returns the names that differ"""
    bad = [k for k in COUNTS if int(a[k]) != int(b[k])]
    bad += [k for k in ("keep", "reason", "lm_views", "lm_status") if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
    return bad


# ------------------------------------------------------------------------------------------------ the loop
def refine_loop(ba, filt, rounds=3, reprojection=1e-2, triangulation=1.0):
    """global_mapper.cc:243-317.  ba(fix_rotations) runs one adjustment; filt(reprojection, triangulation, scaling) runs one filter (one of
    the two thresholds is None) and returns (tracks_changed, tracks_total).  Returns the list of calls made, as tuples."""
    calls = []
    ite = 0
    while ite < rounds:                                                          # :243
        ba(True); calls.append(("ba", True))                                     # :250-253
        ba(False); calls.append(("ba", False))                                   # :260-265
        status, filtered_num = True, 0                                           # :282-283
        while status and ite < rounds:                                           # :284
            scaling = max(3 - ite, 1)                                            # :285
            changed, total = filt(scaling * reprojection, None, scaling)         # :286-291
            calls.append(("filter", scaling * reprojection, None))
            filtered_num += changed
            if filtered_num > 1e-3 * total:                                      # :293
                status = False                                                   # :294
            else:
                ite += 1                                                         # :296
        if status:                                                               # :298
            break                                                                # :300
        ite += 1                                                                 # :243
    filt(reprojection, None, 1); calls.append(("filter", reprojection, None))    # :307-312
    if triangulation is not None:
        filt(None, triangulation, 1); calls.append(("filter", None, triangulation))   # :313-317
    return calls


# ------------------------------------------------------------------------------------------------ scenes
def _rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def scene_from(cam, lm, p, w, R, C, P):
    """R: n camera-to-world rotations (n x 3 x 3), C: n centres, P: m points"""
    n = len(R)
    rot = np.concatenate([np.asarray(R[i], dtype=np.float64) for i in range(n)], axis=1)
    return dict(cam=np.asarray(cam, np.int32), lm=np.asarray(lm, np.int32), p=np.ascontiguousarray(p, dtype=np.float64),
                w=np.ascontiguousarray(w, dtype=np.float64), n=n, m=len(P), rot=np.ascontiguousarray(rot), t=np.ascontiguousarray(np.asarray(C, float).T),
                P=np.ascontiguousarray(np.asarray(P, float).T))


def observe(R, C, P, cam, lm):
    """the camera-frame points R_i^T (P_l - t_i) of the observations listed"""
    return np.stack([R[i].T @ (np.asarray(P[l]) - np.asarray(C[i])) for i, l in zip(cam, lm)])


def fan_scene(degrees, n_cams=12, seed=0, spread=0.5, noise=0.0, base=None):
    """cameras on an arc looking down +z at points about 6 away; landmark l has degrees[l] observations, taken from the cameras in turn
    (a degree above n_cams names (camera, landmark) pairs several times).  Ground-truth geometry; noise on the observed points.
    A connected list: every camera sees landmark 0 when degrees[0] >= n_cams."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(-spread, spread, n_cams)
    C = np.stack([6.0 * np.sin(ang), 0.3 * rng.standard_normal(n_cams), 6.0 - 6.0 * np.cos(ang)], axis=1)
    R = [np.array([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]]) @ _rot_z(0.1 * rng.standard_normal()) for a in ang]
    P = np.stack([rng.uniform(-1, 1, len(degrees)), rng.uniform(-1, 1, len(degrees)), 6.0 + rng.uniform(-1, 1, len(degrees))], axis=1)
    cam, lm = [], []
    for l, k in enumerate(degrees):
        first = int(rng.integers(n_cams))
        cam += [(first + j) % n_cams for j in range(k)]; lm += [l] * k
    p = observe(R, C, P, cam, lm)
    p[:, :2] += noise * rng.standard_normal((len(cam), 2)) * p[:, 2:3]
    return scene_from(cam, lm, p, np.ones(len(cam)), R, C, P)


def boundary_scene(seed=3):
    """landmark degrees around the light / heavy boundary (0 has none: the landmark exists only as an index), noise that puts part of the
    observations beyond the thresholds of TIGHT"""
    degrees = [24, 0, 1, 2, 3, LIGHT_MAX - 1, LIGHT_MAX, LIGHT_MAX + 1, LIGHT_MAX + 2, 5, 7, 12]
    return fan_scene(degrees, n_cams=12, seed=seed, noise=2e-3)


def tile_scene(seed=4):
    """one heavy landmark each of TILE - 1, TILE, TILE + 1 and 2 TILE + 1 observations on 9 cameras"""
    return fan_scene([12, TILE - 1, TILE, TILE + 1, 2 * TILE + 1], n_cams=9, seed=seed, noise=2e-3)


TIGHT = dict(reprojection=2.5e-3, angle=0.12, triangulation=8.0)      # inside the distributions of the two scenes above


def pair_scene(k, where, deg=1.0):
    """landmark 1 with k observations from k cameras whose rays all lie within `deg` degrees of each other, except the pair named by
    `where`: "first": rays 0 and 1; "last": rays k-2 and k-1; "split": rays 0 and k-1 (for k > TILE: two different tiles); "none": no wide
    pair.  The rays are e_z turned about x in steps that span 0.2 deg in all; the two partners of the wide pair are turned by +-0.6 deg
    about y as well: partner to partner 1.2 deg, a partner to any other ray at most 0.64 deg.  Landmark 0 ties the cameras together
    (identity rotations, each camera placed 5 away from landmark 1 against its ray)."""
    tilt = np.zeros(k)
    pair = {"first": (0, 1), "last": (k - 2, k - 1), "split": (0, k - 1), "none": None}[where]
    if pair is not None:
        tilt[pair[0]] = np.deg2rad(0.6 * deg); tilt[pair[1]] = -np.deg2rad(0.6 * deg)
    ang = np.deg2rad(np.arange(k) * (0.2 * deg / max(k, 2)))
    dirs = np.stack([np.sin(tilt), np.sin(ang) * np.cos(tilt), np.cos(ang) * np.cos(tilt)], axis=1)      # unit rays camera -> point
    Pl = np.array([0.0, 0.0, 5.0])
    C = Pl[None, :] - 5.0 * dirs
    R = [np.eye(3)] * k
    P = np.stack([np.array([0.3, -0.2, 6.0]), Pl])
    cam = list(range(k)) + list(range(k)); lm = [0] * k + [1] * k
    p = observe(R, C, P, cam, lm)
    return scene_from(cam, lm, p, np.ones(len(cam)), R, C, P)


def flags_scene():
    """weight 0, p_2 <= 0, a (camera, landmark) pair named twice, an unused camera (3: p_2 <= 0 throughout), a landmark with no used
    observation (2), depths just below and above EPS and negative, and a landmark (4) whose only wide pair contains an observation the
    reprojection filter drops"""
    R = [np.eye(3)] * 5
    C = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [3.0, 0, 0], [0.02, 0, 0]])
    P = np.array([[0.5, 0.1, 5.0], [1.0, -0.2, 6.0], [1.5, 0.3, 4.0], [0.5, 0.0, 0.0], [0.0, 0.0, 8.0]])
    cam = [0, 1, 2, 4, 0, 1, 1, 2, 3, 3, 0, 1, 0, 1, 2, 0, 4, 1]
    lm_ = [0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 2, 2, 3, 3, 3, 4, 4, 4]
    p = observe(R, C, P, cam, lm_)
    w = np.ones(len(cam))
    p[8, 2] = -p[8, 2]; p[9, 2] = -p[9, 2]  # camera 3 is unused: p_2 <= 0 in both its observations
    w[10] = 0.0; p[11, 2] = 0.0             # landmark 2: one observation of weight 0, one with p_2 = 0
    p[12] = [0.5, 0.0, 1.0]; p[13] = [-0.5, 0.0, 1.0]; p[14] = [-1.5, 0.0, 1.0]   # landmark 3 lies in the plane of the cameras: q_2 = 0 < EPS
    S = scene_from(cam, lm_, p, w, R, C, P)
    S["p"][17, 0] += 0.05 * S["p"][17, 2]   # landmark 4: cameras 0 and 4 are 0.02 apart, camera 1 gives the only wide pair and is displaced
    return S


def depth_scene():
    """landmark 1 at depths EPS / 2, 2 EPS and -1 from three cameras (identity rotations at z = -EPS/2, -2 EPS, +1), observed points given"""
    R = [np.eye(3)] * 3
    C = np.array([[0.0, 0.0, -0.5 * EPS], [0.0, 0.0, -2 * EPS], [0.0, 0.0, 1.0]])
    P = np.array([[0.1, 0.1, 5.0], [0.0, 0.0, 0.0]])
    cam = [0, 1, 2, 0, 1, 2]; lm_ = [0, 0, 0, 1, 1, 1]
    p = observe(R, C, P, cam, lm_)
    p[3:] = [0.0, 0.0, 1.0]
    return scene_from(cam, lm_, p, np.ones(6), R, C, P)


def permuted(S, seed=0):
    perm = np.random.default_rng(seed).permutation(S["cam"].size)
    T = dict(S)
    for k in ("cam", "lm", "p", "w"):
        T[k] = np.ascontiguousarray(S[k][perm])
    return T, perm


def threshold_cases():
    """(scene, kwargs, observation or landmark, kept at the threshold?) with a test value EXACTLY equal to the threshold double.
    reprojection: the threshold is the error itself.  angle / triangulation: the angle in degrees is searched so that the cosine the
    library computes equals a dot product the geometry gives exactly: a ray (s, 0, c) with c = cos_deg(angle), s = sqrt(1 - c c) whose norm
    rounds to 1, against e_z."""
    out = []
    S = fan_scene([6, 4], n_cams=6, seed=9, noise=1e-3)
    _, q, _ = geometry(S)
    err = reprojection_error(S, q)
    e = int(np.argmax(err))
    out.append(("reprojection", S, dict(reprojection=float(err[e])), e))
    for a in np.arange(1.0, 40.0, 0.25):
        c = cos_deg(float(a)); s = math.sqrt(1.0 - c * c)
        if math.sqrt((s * s + 0.0) + c * c) == 1.0:
            break
    else:
        raise AssertionError("no angle whose ray has norm 1 exactly")
    # angle: camera 0 at the origin, identity; the point straight ahead; the observed point (s, 0, c)
    R = [np.eye(3)] * 2
    C = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    P = np.array([[0.0, 0.0, 4.0]])
    p = observe(R, C, P, [0, 1], [0, 0])
    p[0] = [s, 0.0, c]
    out.append(("angle", scene_from([0, 1], [0, 0], p, np.ones(2), R, C, P), dict(reprojection=None, angle=float(a)), 0))
    # triangulation: rays e_z and (s, 0, c) from two cameras at -e_z and -(s, 0, c)
    C = np.array([[0.0, 0.0, -1.0], [-s, 0.0, -c]])
    P = np.array([[0.0, 0.0, 0.0]])
    p = observe(R, C, P, [0, 1], [0, 0])
    out.append(("triangulation", scene_from([0, 1], [0, 0], p, np.ones(2), R, C, P), dict(reprojection=None, triangulation=float(a)), 0))
    return out


def simple2(golden):
    """the recorded case: the observation list of SIMPLE2 at the reference's recovered solution"""
    import os
    o = np.load(os.path.join(golden, "simple2", "obs.npz")); g = np.load(os.path.join(golden, "simple2", "tp.npz"))
    return dict(cam=o["cam"], lm=o["lm"], p=o["p"], w=o["w"], n=g["t_est"].shape[1], m=g["p_est"].shape[1],
                rot=np.ascontiguousarray(g["R_real"]), t=np.ascontiguousarray(g["t_est"]), P=np.ascontiguousarray(g["p_est"]))


SIMPLE2_TIGHT = dict(reprojection=1.2e-3, angle=0.07, triangulation=10.0)


def displaced(S, share=0.05, size=0.05, seed=0):
    """a copy of S with a seeded share of the observed points moved by `size` in normalised image units; -> (scene, bool per observation)"""
    rng = np.random.default_rng(seed)
    hit = rng.random(S["cam"].size) < share
    ang = rng.uniform(0, 2 * np.pi, S["cam"].size)
    T = dict(S); p = S["p"].copy()
    p[hit, 0] += size * np.cos(ang[hit]) * p[hit, 2]; p[hit, 1] += size * np.sin(ang[hit]) * p[hit, 2]
    T["p"] = p
    return T, hit
