"""Observation cleaning restated with numpy and scipy (include/xm_amd.h at xm_clean_observations has the definition; the reference's
utils/checkconnection.py:checklandmarks computes it) -- independent of the library: whole-array operations in the order of the definition
and scipy.sparse.csgraph.connected_components for stage 4.  The reference for tests/test_gpu_clean.py; tests/test_clean_reference.py holds
it against outputs recorded from the reference's own function (tests/golden/clean)."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

COUNTS = ("nobs_live", "n_new", "m_new", "nobs_new", "components", "cams_weak", "lms_weak", "cams_emptied", "cams_off_component",
          "lms_off_component", "first_camera")


def clean_numpy(cam, lm, w=None, n=None, m=None, min_cam_obs=10, min_lm_obs=1, swap_first=True):
    """-> dict(keep (bool, per observation), cam_index (n), lm_index (m), info (the counts of xm_clean_result_t without `rounds`))"""
    cam = np.asarray(cam, dtype=np.int64).reshape(-1); lm = np.asarray(lm, dtype=np.int64).reshape(-1)
    n = (int(cam.max()) + 1 if cam.size else 0) if n is None else int(n)
    m = (int(lm.max()) + 1 if lm.size else 0) if m is None else int(m)
    live = np.ones(cam.size, dtype=bool) if w is None else np.asarray(w, dtype=np.float64).reshape(-1) > 0
    # 1: cameras by their live observations
    d1 = np.bincount(cam[live], minlength=n)
    cam1 = d1 > min_cam_obs
    first = int(np.argmax(d1)) if n else -1
    # 2: landmarks by their observations from surviving cameras
    on2 = live & cam1[cam]
    lm2 = np.bincount(lm[on2], minlength=m) > min_lm_obs
    # 3: what is left; a camera without any of it goes
    on3 = on2 & lm2[lm]
    cam3 = np.bincount(cam[on3], minlength=n) > 0
    # 4: components of the bipartite graph of the remaining observations; cameras are the vertices 0 .. n-1, landmarks n .. n+m-1
    node = np.concatenate([cam3, lm2])
    e3 = np.flatnonzero(on3)
    graph = coo_matrix((np.ones(e3.size, dtype=np.int8), (cam[e3], n + lm[e3])), shape=(n + m, n + m))
    _, label = connected_components(graph, directed=False) if n + m else (0, np.zeros(0, dtype=np.int64))
    size = np.bincount(label[node], minlength=label.max() + 1 if label.size else 0)       # nodes per component; vertices outside the graph do not count
    earliest = np.full(size.size, cam.size, dtype=np.int64)
    np.minimum.at(earliest, label[cam[e3]], e3)
    keep = np.zeros(cam.size, dtype=bool)
    camk = np.zeros(n, dtype=bool); lmk = np.zeros(m, dtype=bool)
    ncomp = int(np.count_nonzero(size))
    if ncomp:
        tied = np.flatnonzero(size == size.max())
        best = tied[np.argmin(earliest[tied])]
        keep[e3] = label[cam[e3]] == best
        camk = cam3 & (label[:n] == best); lmk = lm2 & (label[n:] == best)
    # index maps
    idx1 = np.where(cam1, np.cumsum(cam1) - 1, -1)
    if swap_first and n and cam1[first] and idx1[first] != 0:
        zero = int(np.flatnonzero(idx1 == 0)[0])
        idx1[zero], idx1[first] = idx1[first], 0
    order = np.argsort(np.where(cam1, idx1, n + np.arange(n)), kind="stable")   # cameras by stage-1 index, the dropped ones behind
    before = np.zeros(n, dtype=np.int64)
    before[order] = np.cumsum(camk[order]) - camk[order]
    cam_index = np.where(camk, before, -1).astype(np.int32)
    lm_index = np.where(lmk, np.cumsum(lmk) - 1, -1).astype(np.int32)
    info = dict(nobs_live=int(live.sum()), n_new=int(camk.sum()), m_new=int(lmk.sum()), nobs_new=int(keep.sum()), components=ncomp,
                cams_weak=int((~cam1).sum()), lms_weak=int((~lm2).sum()), cams_emptied=int((cam1 & ~cam3).sum()),
                cams_off_component=int((cam3 & ~camk).sum()), lms_off_component=int((lm2 & ~lmk).sum()), first_camera=first)
    return dict(keep=keep, cam_index=cam_index, lm_index=lm_index, info=info)


def apply_numpy(plan, cam, lm, *arrays):
    """the compacted, re-indexed list (what CleanPlan.apply returns)"""
    k = plan["keep"]
    return (plan["cam_index"][np.asarray(cam)[k]], plan["lm_index"][np.asarray(lm)[k]]) + tuple(np.asarray(a)[k] for a in arrays)


def fixture_points(name, nobs):
    """camera-frame points and weights of the synthetic cases of tests/golden/clean (make_clean.py records hashes of what the reference
    returns for them)"""
    rng = np.random.default_rng(len(name) + nobs)
    return rng.standard_normal((nobs, 3)), rng.uniform(0.5, 1.5, nobs)


def load_case(golden, name):
    """a case of tests/golden/clean with its input: dict(cam, lm, p, w, n, m, fx) -- w holds 0 where the input row counts as deleted"""
    import os
    fx = np.load(os.path.join(golden, "clean", name + ".npz"))
    if name == "a":   # SIMPLE2 after the recorded XM^2 filter
        o = np.load(os.path.join(golden, "simple2", "obs.npz")); err = np.load(os.path.join(golden, "simple2", "xm2.npz"))["error"]
        cam, lm, p = o["cam"], o["lm"], o["p"]
        w = np.where(err <= np.percentile(err, 90), o["w"], 0.0)
        n, m = int(cam.max()) + 1, int(lm.max()) + 1
    else:
        cam, lm, n, m = fx["cam"].astype(np.int32), fx["lm"].astype(np.int32), int(fx["n"]), int(fx["m"])
        p, w = fixture_points(name, cam.size)
    return dict(cam=cam, lm=lm, p=p, w=w, n=n, m=m, fx=fx)


def fixture_keep(fx, tag):
    return np.unpackbits(fx["keep_" + tag])[: int(fx["nobs"])].astype(bool)


CASES = ("a", "b", "c1", "c2", "d")


def chain_scene(ncams, seed, cut=None):
    """a sequential capture with shuffled numbering: camera i of the trajectory sees the landmarks 3 i .. 3 i + 5, so neighbours share three;
    cut: no landmark is shared across the boundary between trajectory positions cut - 1 and cut (two components).  -> cam, lm, n, m"""
    rng = np.random.default_rng(seed)
    pos = np.repeat(np.arange(ncams), 6)
    l = 3 * pos + np.tile(np.arange(6), ncams)
    m = 3 * ncams + 3
    if cut is not None:   # the first half's last camera loses the three landmarks it shares with the second half
        drop = (pos == cut - 1) & (l >= 3 * cut)
        pos, l = pos[~drop], l[~drop]
    cperm = rng.permutation(ncams); lperm = rng.permutation(m)
    order = rng.permutation(pos.size)
    return cperm[pos][order].astype(np.int32), lperm[l][order].astype(np.int32), ncams, m
