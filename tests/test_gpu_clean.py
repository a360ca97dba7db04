"""GPU tests of observation cleaning (xm_clean_observations / xm_ctx_clean_observations, include/xm_amd.h): both entry points against the
outputs recorded from the reference (tests/golden/clean) and against the numpy / scipy restatement (tests/xm_clean_numpy.py), EXACTLY --
keep, both index maps and every count are integers.

A context can only hold a list whose graph is connected and whose cameras all carry weight (anything else is refused at creation), so the
context variant sees the lists that need cleaning inside a connected superset: rows appended for one more camera that has so few
observations that stage 1 drops it (_bridge).  With the thresholds at which that camera is weak the answer on the original rows is the
answer for the original list; at every threshold the answer for the superset is held against the restatement."""
import os

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import xm_clean_numpy as cn
import xm_testlib as tl

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THRESHOLDS = ((10, 1), (0, 1), (0, 0), (3, 2))


def _same(plan, ref, what=""):
    assert plan.keep.dtype == bool and plan.cam_index.dtype == np.int32 and plan.lm_index.dtype == np.int32
    assert np.array_equal(plan.keep, ref["keep"]), what
    assert np.array_equal(plan.cam_index, ref["cam_index"]), what
    assert np.array_equal(plan.lm_index, ref["lm_index"]), what
    assert {k: plan.info[k] for k in cn.COUNTS} == ref["info"], what
    assert 1 <= plan.info["rounds"] <= 64 or plan.info["nobs_new"] == 0, what


def _bridge(cam, lm, n, m):
    """rows for one more camera (number n) that sees one landmark of every component of the list's graph, unobserved landmarks included, and
    a row for every unobserved camera on the first of those landmarks: with them the graph is connected and every camera is observed"""
    g = coo_matrix((np.ones(cam.size, dtype=np.int8), (cam, n + lm)), shape=(n + m, n + m))
    _, label = connected_components(g, directed=False)
    reps = [int(np.flatnonzero(label[n:] == c)[0]) for c in np.unique(label[n:])]
    lonely = [c for c in range(n) if not np.any(cam == c)]
    bc = np.array([n] * len(reps) + lonely, dtype=np.int32); bl = np.array(reps + [reps[0]] * len(lonely), dtype=np.int32)
    return np.concatenate([cam, bc]).astype(np.int32), np.concatenate([lm, bl]).astype(np.int32), n + 1, len(reps)


def _context(xmamd, cam, lm, n, seed, w=None):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((cam.size, 3))
    w = rng.uniform(0.5, 1.5, cam.size) if w is None else w
    ctx = xmamd.Context(obs=(cam, lm, p, w), n=n)
    return ctx


# ------------------------------------------------------------------------------------------------ the recorded cases
@pytest.fixture(scope="module", params=cn.CASES)
def case(request):
    return cn.load_case(GOLDEN, request.param)


def _fixture_plan(case, tag):
    fx = case["fx"]
    return cn.fixture_keep(fx, tag), fx["lm_index_" + tag], list(fx["counts_" + tag])


def test_list_call_equals_the_reference(xmamd, case):
    for tag, thr in (("10_1", (10, 1)), ("0_1", (0, 1))):
        plan = xmamd.clean_observations(case["cam"], case["lm"], case["w"], case["n"], case["m"], *thr)
        keep, lmi, counts = _fixture_plan(case, tag)
        assert np.array_equal(plan.keep, keep) and np.array_equal(plan.lm_index, lmi)
        assert [plan.info[k] for k in ("n_new", "m_new", "nobs_new")] == counts
        if tag == "10_1":
            assert np.array_equal(plan.cam_index, case["fx"]["indices_all_10_1"])
        _same(plan, cn.clean_numpy(case["cam"], case["lm"], case["w"], case["n"], case["m"], *thr), tag)


def test_context_call_equals_the_reference(xmamd, case):
    cam, lm, n, m, fx = case["cam"], case["lm"], case["n"], case["m"], case["fx"]
    if fx is not None and "cam" not in fx.files:          # (a): SIMPLE2, filtered through set_edge_weights
        o = np.load(os.path.join(GOLDEN, "simple2", "obs.npz"))
        ctx = xmamd.Context(obs=(cam, lm, o["p"], o["w"]))
        ctx.set_edge_weights(case["w"])
        for tag, thr in (("10_1", (10, 1)), ("0_1", (0, 1))):
            plan = ctx.clean_observations(*thr)
            keep, lmi, counts = _fixture_plan(case, tag)
            assert np.array_equal(plan.keep, keep) and np.array_equal(plan.lm_index, lmi)
            assert [plan.info[k] for k in ("n_new", "m_new", "nobs_new")] == counts
            if tag == "10_1":
                assert np.array_equal(plan.cam_index, fx["indices_all_10_1"])
            _same(plan, cn.clean_numpy(cam, lm, case["w"], n, m, *thr), tag)
        ctx.close()
        return
    cam2, lm2, n2, nbridge = _bridge(cam, lm, n, m)
    assert nbridge <= 10                                   # the added camera is weak at checklandmarks' threshold
    ctx = _context(xmamd, cam2, lm2, n2, seed=cam.size)
    assert ctx.n_landmarks == m
    plan = ctx.clean_observations(10, 1)
    keep, lmi, counts = _fixture_plan(case, "10_1")
    assert np.array_equal(plan.keep[: cam.size], keep) and not plan.keep[cam.size:].any()
    assert np.array_equal(plan.lm_index, lmi) and np.array_equal(plan.cam_index[:n], fx["indices_all_10_1"]) and plan.cam_index[n] == -1
    assert [plan.info[k] for k in ("n_new", "m_new", "nobs_new")] == counts
    for thr in THRESHOLDS:
        _same(ctx.clean_observations(*thr), cn.clean_numpy(cam2, lm2, None, n2, m, *thr), str(thr))
    ctx.close()


# ------------------------------------------------------------------------------------------------ random scenes
def _scene(seed, n, m_extra=0, degs=()):
    """two groups of cameras with their own landmarks, each held together by a landmark that all its cameras see (with 72 cameras in the
    first group that is more than 64 observations: a heavy slot of the context), joined only through a camera with four observations that
    sees both of them; cameras with few observations, single-view landmarks, landmarks of the degrees `degs`, m_extra unobserved ones.
    Connected and every camera observed: a context can hold it.  Shuffled rows, shuffled camera and landmark numbers."""
    rng = np.random.default_rng(seed)
    na = max(4, (2 * n) // 3); nb = n - na - 1
    assert nb >= 2
    rows = []
    ma, mb = 3 * na + 10, 3 * nb + 10
    for c in range(na):
        k = min(int(rng.integers(2, 20)), ma - 1)         # some at or below every camera threshold
        rows += [(c, 0)] + [(c, int(l)) for l in rng.choice(np.arange(1, ma), size=k, replace=False)]
    for c in range(na, na + nb):
        k = min(int(rng.integers(2, 20)), mb - 1)
        rows += [(c, ma)] + [(c, ma + int(l)) for l in rng.choice(np.arange(1, mb), size=k, replace=False)]
    weak = na + nb
    rows += [(weak, 0), (weak, 1), (weak, ma), (weak, ma + 1)]
    mtot = ma + mb
    for d in degs:                                        # a landmark seen by exactly d cameras of the first group
        rows += [(int(c), mtot) for c in rng.choice(na, size=d, replace=False)]
        mtot += 1
    for _ in range(5):                                    # single-view landmarks
        rows.append((int(rng.integers(0, n)), mtot)); mtot += 1
    mtot += m_extra
    obs = np.array(rows)
    cperm, lperm = rng.permutation(n), rng.permutation(mtot)
    order = rng.permutation(obs.shape[0])
    return cperm[obs[order, 0]].astype(np.int32), lperm[obs[order, 1]].astype(np.int32), n, mtot


SCENES = [dict(seed=s, n=int(np.random.default_rng(100 + s).integers(8, 201))) for s in range(15)] + [
    dict(seed=15, n=109),                                 # first group: 72 cameras, the landmark they all see is a heavy slot
    dict(seed=16, n=109, degs=(63, 64, 65)),
    dict(seed=17, n=60, m_extra=3000 - (3 * 40 + 10 + 3 * 19 + 10 + 5)),       # m = 3000
    dict(seed=18, n=90, m_extra=2049 - 90 - (3 * 60 + 10 + 3 * 29 + 10 + 5)),  # n + m = 2049
    dict(seed=19, n=8)]


def test_scenes_are_what_they_say():
    c16 = _scene(**SCENES[16]); c17 = _scene(**SCENES[17]); c18 = _scene(**SCENES[18])
    deg = np.bincount(c16[1], minlength=c16[3])
    assert {63, 64, 65, 73} <= set(deg.tolist())             # 73: the 72 cameras of the first group and the joining camera
    assert c17[3] == 3000 and c18[2] + c18[3] == 2049
    assert sorted(s["n"] for s in SCENES)[0] == 8 and max(s["n"] for s in SCENES) <= 200


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_random_scenes_equal_the_restatement(xmamd, k):
    cam, lm, n, m = _scene(**SCENES[k])
    rng = np.random.default_rng(1000 + k)
    w = np.where(rng.random(cam.size) < 0.15, 0.0, rng.uniform(0.5, 1.5, cam.size))     # weight 0: deleted rows
    for j, thr in enumerate(THRESHOLDS):
        swap = (k + j) % 3 != 0                           # XM_CLEAN_NO_SWAP on a third of the calls
        for ww in (None, w):                              # NULL weights: all live
            plan = xmamd.clean_observations(cam, lm, ww, n, m, *thr, swap_first=swap)
            _same(plan, cn.clean_numpy(cam, lm, ww, n, m, *thr, swap_first=swap), f"scene {k} thresholds {thr} swap {swap} w {ww is not None}")
    first, second = (xmamd.clean_observations(cam, lm, w, n, m) for _ in range(2))      # two calls: the same bytes
    assert all(getattr(first, a).tobytes() == getattr(second, a).tobytes() for a in ("keep", "cam_index", "lm_index"))
    # the same list inside a context, at its weights (all positive: only such a list is sure to be connected) ...
    ctx = _context(xmamd, cam, lm, n, seed=k)
    m = ctx.n_landmarks                                   # (unobserved landmarks behind the last observed one are not the context's)
    plans = [ctx.clean_observations(*thr, swap_first=(k % 2 == 0)) for thr in THRESHOLDS]
    for thr, plan in zip(THRESHOLDS, plans):
        _same(plan, cn.clean_numpy(cam, lm, None, n, m, *thr, swap_first=(k % 2 == 0)), f"context, scene {k} thresholds {thr}")
    # ... and two calls give the same bytes
    again = ctx.clean_observations(*THRESHOLDS[0], swap_first=(k % 2 == 0))
    for a, b in ((again.keep, plans[0].keep), (again.cam_index, plans[0].cam_index), (again.lm_index, plans[0].lm_index)):
        assert a.tobytes() == b.tobytes()
    assert {k2: v for k2, v in again.info.items() if k2 != "rounds"} == {k2: v for k2, v in plans[0].info.items() if k2 != "rounds"}
    ctx.close()


def test_everything_dropped(xmamd):
    cam, lm, n, m = cn.chain_scene(8, 0)                  # six observations per camera: none has more than 10
    for plan in (xmamd.clean_observations(cam, lm, None, n, m), xmamd.clean_observations(cam, lm, np.zeros(cam.size), n, m, 0, 0),
                 xmamd.clean_observations(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), None, 3, 4)):
        assert not plan.keep.any() and np.all(plan.cam_index == -1) and np.all(plan.lm_index == -1)
        assert [plan.info[k] for k in ("n_new", "m_new", "nobs_new", "components", "cams_off_component", "lms_off_component")] == [0] * 6
    _same(xmamd.clean_observations(cam, lm, None, n, m), cn.clean_numpy(cam, lm, None, n, m))


# ------------------------------------------------------------------------------------------------ rounds
def test_chain_converges_in_few_rounds(xmamd):
    """a sequential capture of 4096 cameras with shuffled numbering: plain label propagation needs about as many rounds as the trajectory
    is long.  The cap of 64 is a condition of the design (hooking with pointer jumping; an emulation took 15), not a measurement."""
    cam, lm, n, m = cn.chain_scene(4096, 7)
    assert cam.size == 24576
    plan = xmamd.clean_observations(cam, lm, None, n, m, 0, 1)
    print("chain of 4096 cameras: rounds", plan.info["rounds"])
    _same(plan, cn.clean_numpy(cam, lm, None, n, m, 0, 1))
    assert plan.info["components"] == 1 and plan.info["n_new"] == 4096 and plan.info["rounds"] <= 64
    # cut in the middle: two components with the same number of nodes; the half with the earlier observation stays
    cam, lm, n, m = cn.chain_scene(4096, 7, cut=2048)
    plan = xmamd.clean_observations(cam, lm, None, n, m, 0, 1)
    print("the same cut in the middle: rounds", plan.info["rounds"])
    _same(plan, cn.clean_numpy(cam, lm, None, n, m, 0, 1))
    assert plan.info["components"] == 2 and plan.info["n_new"] == 2048 == plan.info["cams_off_component"] and plan.info["rounds"] <= 64
    assert plan.info["m_new"] == plan.info["lms_off_component"]
    graph_rows = (np.bincount(lm, minlength=m) > 1)[lm]
    assert plan.keep[int(np.flatnonzero(graph_rows)[0])]


# ------------------------------------------------------------------------------------------------ the context stays as it was; end to end
def _junk_scene():
    """gen_scene (40 cameras) plus the junk of fixture (b): a camera with 10 observations, single-view landmarks, a detached group of three
    cameras.  -> the whole list (shuffled), and which rows are the clean scene's"""
    S = tl.gen_scene(40, 400, 5, seed=21)
    rng = np.random.default_rng(22)
    n, m = S["n"], S["m"]
    jc = [40] * 10 + [int(c) for c in rng.integers(0, 40, 6)] + [c for c in (41, 42, 43) for _ in range(15)]
    jl = [int(l) for l in rng.choice(m, 10, replace=False)] + list(range(m, m + 6)) + [m + 6 + l for _ in range(3) for l in range(15)]
    cam = np.concatenate([S["cam"], np.array(jc, dtype=np.int32)]); lm = np.concatenate([S["lm"], np.array(jl, dtype=np.int32)])
    p = np.concatenate([S["p"], rng.standard_normal((len(jc), 3))]); w = np.concatenate([S["w"], rng.uniform(0.5, 1.5, len(jc))])
    clean = np.arange(cam.size) < S["cam"].size
    order = rng.permutation(cam.size)
    return S, cam[order], lm[order], p[order], w[order], clean[order], 44, m + 21


def test_clean_apply_solve(xmamd):
    S, cam, lm, p, w, clean, n, m = _junk_scene()
    assert np.bincount(S["cam"]).min() > 10
    plan = xmamd.clean_observations(cam, lm, w, n, m)
    _same(plan, cn.clean_numpy(cam, lm, w, n, m))
    assert np.array_equal(plan.keep, clean) and plan.info["n_new"] == 40 and plan.info["m_new"] == S["m"] and plan.info["components"] == 2
    assert (plan.info["cams_weak"], plan.info["cams_off_component"], plan.info["lms_off_component"]) == (1, 3, 15)
    c2, l2, p2, w2 = plan.apply(cam, lm, p, w)
    # the compacted arrays are the clean scene's under the returned maps: cameras renumbered (the one with the most observations first),
    # landmarks in their order, rows in input order
    cmap, lmap = plan.cam_index[:40], plan.lm_index[: S["m"]]
    assert sorted(cmap.tolist()) == list(range(40)) and cmap[plan.info["first_camera"]] == 0 and np.array_equal(lmap, np.arange(S["m"]))
    assert np.array_equal(c2, cmap[cam[clean]]) and np.array_equal(l2, lm[clean]) and np.array_equal(p2, p[clean]) and np.array_equal(w2, w[clean])
    lam = 1.5 * float(np.sum(w2 * np.sum(p2 ** 2, axis=1)) / (3 * 40))
    ctx = xmamd.Context(obs=(c2, l2, p2, w2))
    R, s, info = ctx.solve(5, 1e-6, lam)
    assert info["status"] == 1                            # certified
    # the cleaned list needs no more cleaning, and asking changes nothing in the context: the next solve gives the same bits
    again = ctx.clean_observations()
    assert again.keep.all() and again.info["components"] == 1 and np.array_equal(again.lm_index, np.arange(S["m"]))
    R1, s1, info1 = ctx.solve(5, 1e-6, lam)
    ctx.clean_observations(0, 1)
    R2, s2, info2 = ctx.solve(5, 1e-6, lam)
    assert R1.tobytes() == R2.tobytes() and s1.tobytes() == s2.tobytes() and info1["primal"] == info2["primal"]
    ctx.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_usable(xmamd):
    S = tl.gen_scene(40, 400, 5, seed=21)
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]))
    ref = ctx.clean_observations()
    import ctypes as C
    L = xmamd.lib()
    keep = np.zeros(ctx.ne, dtype=np.uint8); ci = np.zeros(ctx.n, dtype=np.int32); li = np.zeros(ctx.n_landmarks, dtype=np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)

    def fresh():
        o = xmamd.CleanOptions(); r = xmamd.CleanResult()
        o.struct_size, r.struct_size, o.min_cam_obs, o.min_lm_obs = C.sizeof(o), C.sizeof(r), 10, 1
        return o, r
    for change in (lambda o, r: setattr(o, "struct_size", 8), lambda o, r: setattr(r, "struct_size", 100), lambda o, r: setattr(o, "min_lm_obs", -1),
                   lambda o, r: setattr(o, "flags", 4)):
        o, r = fresh(); change(o, r)
        assert L.xm_ctx_clean_observations(ctx.h, C.byref(o), P(keep), P(ci), P(li), C.byref(r)) == -2
    o, r = fresh()
    assert L.xm_ctx_clean_observations(ctx.h, C.byref(o), None, P(ci), P(li), C.byref(r)) == -2
    assert L.xm_ctx_clean_observations(ctx.h, C.byref(o), P(keep), P(ci), None, C.byref(r)) == -2
    # an index out of range (list call)
    cam = S["cam"].copy(); cam[5] = 40
    with pytest.raises(xmamd.XmError, match="out of range"):
        xmamd.clean_observations(cam, S["lm"], None, 40, S["m"])
    with pytest.raises(xmamd.XmError, match="out of range"):
        xmamd.clean_observations(S["cam"], S["lm"], None, 40, S["m"] - 1)
    with pytest.raises(xmamd.XmError, match="2\\^31"):
        xmamd.clean_observations(S["cam"], S["lm"], None, 2 ** 30, 2 ** 30)
    # another storage, several ranks
    V = tl.gen_vg(40, deg=3, sigma=0.1, seed=1)
    dense = xmamd.Context(Q=V["Q"])
    with pytest.raises(xmamd.XmError, match="XM_STORAGE_SCHUR"):
        dense.clean_observations()
    dense.close()
    two = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n_gpus=2, gpu_map=1)
    two.ne, two.n_landmarks = S["cam"].size, S["m"]
    with pytest.raises(xmamd.XmError, match="single-GPU"):
        two.clean_observations()
    two.close()
    after = ctx.clean_observations()                      # still usable, same answer
    assert np.array_equal(after.keep, ref.keep) and np.array_equal(after.cam_index, ref.cam_index) and after.info["nobs_new"] == ref.info["nobs_new"]
    ctx.close()
