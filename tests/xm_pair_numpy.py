"""The pairwise relative-rotation filter restated with numpy and scipy (include/xm_amd.h at xm_pair_filter has the definition; the reference
computes it in 5_test_ceres.py:316-431) -- independent of the library: per pair, whole-array operations in the order of the definition, with
scipy.stats.trim_mean and np.percentile / np.median themselves.  The reference for tests/test_gpu_pair_filter.py; tests/test_pair_numpy.py
holds it against outputs recorded from the reference's own lines (tests/golden/pair).

pair_filter_numpy also returns the DECISION MARGIN: the smallest |x - thr| / thr over every value compared with a threshold (steps 4 and 10)
over all used pairs; values bit-equal to their threshold (the rank decisions of an interpolation weight 0) are left out.  Summation orders
differ by ~1e-15, so above a margin of 1e-10 every implementation of the definition takes the same decisions."""
import os

import numpy as np
from scipy.stats import trim_mean

STAT_DTYPE = np.dtype([("n_joint", "<i4"), ("n_kept", "<i4"), ("n_flagged", "<i4"), ("status", "<i4"), ("scale1", "<f8"), ("scale2", "<f8"),
                       ("translation", "<f8", (3,)), ("median", "<f8"), ("p95", "<f8"), ("percentage", "<f8")])
USED, TOO_FEW, DEGENERATE = 0, 1, 2
FLOATS = ("scale1", "scale2", "translation", "median", "p95")
MIN_MARGIN = 1e-10


class F64:
    """the operations of the definition with scipy / numpy themselves"""
    dtype = np.float64

    @staticmethod
    def tmean(a, trim):                      # a: (rows, k) -> per row
        return trim_mean(a, proportiontocut=trim, axis=-1)

    @staticmethod
    def pct(a, q):
        return np.percentile(a, q)

    @staticmethod
    def median(a):
        return np.median(a)


def _margin(x, thr):
    x = x[x != thr]
    return float(np.min(np.abs(x - thr) / np.abs(thr))) if x.size and thr != 0 else np.inf


def one_pair(src, dst, R, opt, ops=F64):
    """steps 2-10 for one pair: src, dst 3 x k.  -> dict(status, n_kept, flagged (bool, k) and the float stats, margin)"""
    T = ops.dtype
    src = np.asarray(src, dtype=T); dst = np.asarray(dst, dtype=T); R = np.asarray(R, dtype=T)
    trim = opt["trim"]
    k = src.shape[1]
    out = dict(status=DEGENERATE, n_kept=0, flagged=np.zeros(k, dtype=bool), scale1=T(0), scale2=T(0), translation=np.zeros(3, dtype=T), median=T(0),
               p95=T(0), percentage=0.0, margin=np.inf, dst_max=float(np.abs(dst).max()))
    with np.errstate(all="ignore"):
        dst_avg = ops.tmean(dst, trim); src_avg = ops.tmean(src, trim)
        dst_dis = np.linalg.norm(dst - dst_avg.reshape(3, 1), axis=0); src_dis = np.linalg.norm(src - src_avg.reshape(3, 1), axis=0)
        ts, td = ops.pct(src_dis, opt["dist_pct"]), ops.pct(dst_dis, opt["dist_pct"])
        index = (src_dis < ts) & (dst_dis < td)
        out["n_kept"] = int(index.sum())
        if not index.any():
            return out
        src_n, dst_n = src[:, index], dst[:, index]
        dst_avg = ops.tmean(dst_n, trim); src_avg = ops.tmean(src_n, trim)
        scale1 = ops.tmean(np.linalg.norm(dst_n - dst_avg.reshape(3, 1), axis=0)[None, :], trim)[0]
        scale2 = ops.tmean(np.linalg.norm(src_n - src_avg.reshape(3, 1), axis=0)[None, :], trim)[0]
        out["scale1"], out["scale2"] = scale1, scale2
        if not (np.isfinite(scale1) and np.isfinite(scale2)) or scale2 == 0:
            return out
        src = src / scale2 * scale1
        src_noR = R @ src
        translation = ops.tmean(dst - src_noR, trim)
        out["translation"] = translation
        target = src_noR + translation.reshape(3, 1)
        error = np.linalg.norm(target - dst, axis=0) / scale1
        if not np.all(np.isfinite(error)) or not np.all(np.isfinite(translation)):
            return out
        med, p95 = ops.median(error), ops.pct(error, opt["err_pct"])
        out["median"], out["p95"] = med, p95
        thr = max(T(opt["mad_factor"]) * med, p95)
        if not np.isfinite(thr):
            return out
    out["flagged"] = error - thr > 0
    out["percentage"] = float(np.sum(error < 0.05) / k)
    out["status"] = USED
    out["margin"] = min(_margin(src_dis, ts), _margin(dst_dis, td), _margin(error, thr))
    return out


def camera_index(cam, lm, n, skip_row0):
    """-> (camptr, landmarks, rows): every camera's observations in increasing landmark order; a pair named twice is a ValueError"""
    rows = np.lexsort((lm, cam))
    key = cam[rows].astype(np.int64) * (int(lm.max()) + 1 if lm.size else 1) + lm[rows]
    if np.any(np.diff(key) == 0):
        raise ValueError("the observation list names a (camera, landmark) pair twice")
    if skip_row0:
        rows = rows[rows != 0]
    return np.searchsorted(cam[rows], np.arange(n + 1)), lm[rows], rows


def pair_filter_numpy(cam, lm, p, pairs_i, pairs_j, R, n=None, m=None, min_joint=20, trim=0.05, dist_pct=90, err_pct=95, mad_factor=3.0, min_flags=1,
                      skip_row0=False, ops=F64):
    """-> dict(count (int32 per observation), outlier (bool), stats (STAT_DTYPE per pair; with ops other than F64 the float fields are in
    `floats`), info (the integer fields of xm_pair_result_t), margin, dst_max (per pair: the largest |coordinate| of dst))"""
    cam = np.asarray(cam, dtype=np.int64).reshape(-1); lm = np.asarray(lm, dtype=np.int64).reshape(-1); p = np.asarray(p, dtype=np.float64)
    pairs_i = np.asarray(pairs_i, dtype=np.int64).reshape(-1); pairs_j = np.asarray(pairs_j, dtype=np.int64).reshape(-1)
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    n = (int(cam.max()) + 1 if cam.size else 0) if n is None else int(n)
    opt = dict(trim=trim, dist_pct=dist_pct, err_pct=err_pct, mad_factor=mad_factor)
    camptr, slm, rows = camera_index(cam, lm, n, skip_row0)
    count = np.zeros(cam.size, dtype=np.int32)
    stats = np.zeros(pairs_i.size, dtype=STAT_DTYPE)
    floats = {f: np.zeros((pairs_i.size, 3) if f == "translation" else pairs_i.size, dtype=ops.dtype) for f in FLOATS}
    dst_max = np.zeros(pairs_i.size)
    margin, max_joint = np.inf, 0
    for q, (i, j) in enumerate(zip(pairs_i, pairs_j)):
        li, lj = slm[camptr[i]:camptr[i + 1]], slm[camptr[j]:camptr[j + 1]]
        _, ai, aj = np.intersect1d(li, lj, assume_unique=True, return_indices=True)      # in increasing landmark order
        k = ai.size
        max_joint = max(max_joint, k)
        st = stats[q]
        st["n_joint"] = k
        if k < min_joint or k < 1:
            st["status"] = TOO_FEW
            continue
        ri, rj = rows[camptr[i] + ai], rows[camptr[j] + aj]
        r = one_pair(p[ri].T, p[rj].T, R[q], opt, ops)
        st["n_kept"], st["status"], st["n_flagged"], st["percentage"] = r["n_kept"], r["status"], int(r["flagged"].sum()), r["percentage"]
        for f in FLOATS:
            floats[f][q] = r[f]
            st[f] = np.asarray(r[f], dtype=np.float64)
        dst_max[q] = r["dst_max"]
        margin = min(margin, r["margin"])
        np.add.at(count, ri[r["flagged"]], 1)
        np.add.at(count, rj[r["flagged"]], 1)
    outlier = count >= min_flags
    status = stats["status"]
    info = dict(pairs_used=int((status == USED).sum()), pairs_skipped=int((status == TOO_FEW).sum()), pairs_degenerate=int((status == DEGENERATE).sum()),
                nobs_flagged=int(outlier.sum()), max_joint=int(max_joint))
    return dict(count=count, outlier=outlier, stats=stats, floats=floats, info=info, margin=margin, dst_max=dst_max)


# ------------------------------------------------------------------------------------------------ the inputs of the recorded cases
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("a", "b")


def load_bin(fn):
    with open(fn, "rb") as f:
        r, c = (int(x) for x in np.fromfile(f, dtype="<i4", count=2))
        return np.fromfile(f, dtype="<f8", count=r * c).reshape((r, c), order="F")


def case_a_inputs(seed=5, share=0.02, sigma=0.3):
    """SIMPLE2's observation list with `share` of the points scaled by 1 + sigma N(0, 1), every camera pair i < j, and the relative rotations
    from the committed ground truth: camera-frame points are p = R_c^T (P - t_c) / s_c with R_c^T the ground-truth block of camera c, so
    dst ~ G_j G_i^T src (G_c = gtR[:, 3 f_c : 3 f_c + 3], f = frame_index).  -> dict(cam, lm, p, n, m, pi, pj, R)"""
    d = os.path.join(GOLDEN, "simple2")
    o = np.load(os.path.join(d, "obs.npz"))
    cam, lm, p = o["cam"].astype(np.int32), o["lm"].astype(np.int32), o["p"].astype(np.float64).copy()
    n, m = int(cam.max()) + 1, int(lm.max()) + 1
    rng = np.random.default_rng(seed)
    hit = rng.random(cam.size) < share
    p[hit] *= (1.0 + sigma * rng.standard_normal(int(hit.sum())))[:, None]
    gt = load_bin(os.path.join(d, "gtR.bin")); fi = np.load(os.path.join(d, "frame_index.npy"))
    G = np.stack([gt[:, 3 * fi[c]:3 * fi[c] + 3] for c in range(n)])
    pi, pj = np.triu_indices(n, 1)
    R = np.einsum("kab,kcb->kac", G[pj], G[pi])
    return dict(cam=cam, lm=lm, p=p, n=n, m=m, pi=pi.astype(np.int32), pj=pj.astype(np.int32), R=R)


def load_case(name):
    """a case of tests/golden/pair with its input: dict(cam, lm, p, n, m, pi, pj, R, fx)"""
    fx = np.load(os.path.join(GOLDEN, "pair", name + ".npz"))
    if name == "a":
        c = case_a_inputs()
    else:
        c = dict(cam=fx["cam"].astype(np.int32), lm=fx["lm"].astype(np.int32), p=fx["p"], n=int(fx["n"]), m=int(fx["m"]), pi=fx["pi"].astype(np.int32),
                 pj=fx["pj"].astype(np.int32), R=fx["R"])
    c["fx"] = fx
    return c


def fixture_outlier(fx):
    return np.unpackbits(fx["outlier"])[: int(fx["nobs"])].astype(bool)


def two_camera_scene(k, seed, shuffle, extra=(7, 11), bad=0.08, noise=0.01):
    """two cameras that share exactly k landmarks (and see `extra` more each on their own), a similarity between them, `bad` of the common
    points displaced; rows in camera-then-landmark order or shuffled.  -> dict(cam, lm, p, n, m, pi, pj, R)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((3, 3)); Q, _ = np.linalg.qr(A); Q *= np.sign(np.linalg.det(Q))
    m = k + sum(extra)
    P = rng.uniform(-4.0, 4.0, (m, 3)) * np.array([1.0, 0.7, 1.3])
    lperm = rng.permutation(m)                                # landmark numbers: the common ones are spread over the range
    l0 = np.concatenate([np.arange(k), k + np.arange(extra[0])]); l1 = np.concatenate([np.arange(k), k + extra[0] + np.arange(extra[1])])
    p0 = P[l0] + noise * rng.standard_normal((l0.size, 3))
    p1 = (1.7 * (P[l1] @ Q.T) + np.array([0.3, -2.0, 1.1])) + noise * rng.standard_normal((l1.size, 3))
    nb = max(1, int(bad * k))
    p1[rng.choice(k, nb, replace=False)] += rng.uniform(0.5, 2.0, (nb, 3))
    cam = np.concatenate([np.zeros(l0.size), np.ones(l1.size)]).astype(np.int32); lm = lperm[np.concatenate([l0, l1])].astype(np.int32)
    p = np.concatenate([p0, p1])
    order = rng.permutation(cam.size) if shuffle else np.lexsort((lm, cam))
    return dict(cam=cam[order], lm=lm[order], p=p[order], n=2, m=m, pi=np.array([0], dtype=np.int32), pj=np.array([1], dtype=np.int32), R=Q[None])


# the shapes and option sets of tests/test_gpu_pair_filter.py (tests/test_pair_numpy.py asserts the decision margin of every one)
JOINT_SIZES = (19, 20, 21, 40, 41, 63, 64, 65, 101, 255, 256, 257, "limit-1", "limit", "limit+1")
OPTION_SETS = (dict(min_flags=2), dict(min_flags=0), dict(dist_pct=80, err_pct=90, mad_factor=2.5), dict(trim=0.1, min_joint=10),
               dict(dist_pct=100, err_pct=50, mad_factor=0.0, trim=0.0), dict(min_joint=25, skip_row0=True))


def joint_size(k, limit):
    return limit + {"limit-1": -1, "limit": 0, "limit+1": 1}[k] if isinstance(k, str) else k


def doubled_pairs(c):
    """the pair list of c, its first ten pairs once more, and every pair reversed with the transposed rotation"""
    return dict(pi=np.concatenate([c["pi"], c["pi"][:10], c["pj"]]), pj=np.concatenate([c["pj"], c["pj"][:10], c["pi"]]),
                R=np.concatenate([c["R"], c["R"][:10], c["R"].transpose(0, 2, 1)]))
