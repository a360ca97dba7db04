"""GPU tests of the pairwise relative-rotation filter (xm_pair_filter, include/xm_amd.h): against the outputs recorded from the reference's
own lines (tests/golden/pair) and against the numpy / scipy restatement (tests/xm_pair_numpy.py) EXACTLY -- count, outlier and the integer
stats are integers, and every case used here has a decision margin of at least 1e-10 (asserted in tests/test_pair_numpy.py), four orders
above what summation orders can move a value -- and, for the float stats, against the longdouble restatement (tests/xm_pair_exact.py) within
the project's bound e_gpu <= max(16 e_ref, 64 eps), e_ref being the f64 restatement's own error (computed here).

Shapes: the two recorded cases, and two-camera scenes whose joint size sits at every place where the code changes its path: the min_joint
threshold, the steps of int(trim k), full wavefronts and workgroups, an integral percentile position, and the LDS limit."""
import numpy as np
import pytest

import xm_pair_exact as pe
import xm_pair_numpy as pn

pytestmark = pytest.mark.gpu
INTS = ("n_joint", "n_kept", "n_flagged", "status")


def _run(xmamd, c, **kw):
    return xmamd.pair_filter(c["cam"], c["lm"], c["p"], c["pi"], c["pj"], c["R"], c["n"], c["m"], **kw)


def _ref(c, ops=None, **kw):
    extra = {} if ops is None else dict(ops=ops)
    return pn.pair_filter_numpy(c["cam"], c["lm"], c["p"], c["pi"], c["pj"], c["R"], c["n"], c["m"], **kw, **extra)


def _same(plan, ref, what=""):
    assert plan.count.dtype == np.int32 and plan.outlier.dtype == bool
    assert np.array_equal(plan.count, ref["count"]), what
    assert np.array_equal(plan.outlier, ref["outlier"]), what
    for f in INTS:
        assert np.array_equal(plan.stats[f], ref["stats"][f]), (what, f)
    assert {k: plan.info[k] for k in ref["info"]} == ref["info"], what


def _floats(plan, c, label, **kw):
    exact = _ref(c, ops=pe.Exact, **kw)
    e_ref = pe.float_errors(_ref(c, **kw)["stats"], exact)
    e_gpu = pe.float_errors(plan.stats, exact)
    for f in pn.FLOATS:
        print(f"PAIR_ERR {label} {f}: e_ref {e_ref[f]:.3e}, e_gpu {e_gpu[f]:.3e}, ratio {e_gpu[f] / pe.bound(e_ref[f]):.3f}")
    for f in pn.FLOATS:
        assert e_gpu[f] <= pe.bound(e_ref[f]), (label, f, e_gpu[f], e_ref[f])
    used = exact["stats"]["status"] == pn.USED
    assert np.allclose(plan.stats["percentage"][used], exact["stats"]["percentage"][used], rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ the recorded cases
@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in pn.CASES:
        c = pn.load_case(name)
        c["ref"] = _ref(c, skip_row0=True)
        out[name] = c
    return out


@pytest.mark.parametrize("name", pn.CASES)
def test_equals_the_reference_and_the_restatement(xmamd, cases, name):
    c = cases[name]
    plan = _run(xmamd, c, skip_row0=True)
    assert np.array_equal(plan.count > 0, pn.fixture_outlier(c["fx"]))
    assert np.array_equal(plan.count, c["fx"]["count"].astype(np.int32))
    _same(plan, c["ref"], name)
    assert plan.info["pairs_on_workspace_path"] == 0 and plan.info["max_joint"] <= xmamd.pair_filter_limits()["lds_joint"]
    print(f"case {name}: {plan.info}")


def test_float_stats_of_case_b(xmamd, cases):
    _floats(_run(xmamd, cases["b"], skip_row0=True), cases["b"], "b", skip_row0=True)


def test_row0_takes_part_by_default(xmamd, cases):
    c = cases["b"]
    plan = _run(xmamd, c)
    ref = _ref(c)
    _same(plan, ref)
    q03 = int(np.flatnonzero((c["pi"] == 0) & (c["pj"] == 3))[0])
    assert plan.stats["n_joint"][q03] == 20 and c["ref"]["stats"]["n_joint"][q03] == 19 and plan.stats["status"][q03] == pn.USED


# ------------------------------------------------------------------------------------------------ two cameras, k common landmarks
@pytest.mark.parametrize("k", pn.JOINT_SIZES)
def test_two_cameras(xmamd, k):
    LIMIT = xmamd.pair_filter_limits()["lds_joint"]
    k = pn.joint_size(k, LIMIT)
    counts = []
    for shuffle in (False, True):
        c = pn.two_camera_scene(k, 1000 + k, shuffle)
        plan = _run(xmamd, c)
        _same(plan, _ref(c), f"k {k} shuffled {shuffle}")
        assert plan.info["max_joint"] == k and plan.info["pairs_on_workspace_path"] == (1 if k > LIMIT else 0)
        assert plan.info["pairs_used"] == (1 if k >= 20 else 0) and plan.info["pairs_skipped"] == (0 if k >= 20 else 1)
        _floats(plan, c, f"k={k} {'shuffled' if shuffle else 'sorted'}")
        by_key = np.lexsort((c["lm"], c["cam"]))
        counts.append((plan.count[by_key], plan.stats.tobytes()))
    # the same scene in another input order: the same counts per (camera, landmark) and the same bits in the stats
    assert np.array_equal(counts[0][0], counts[1][0]) and counts[0][1] == counts[1][1]


# ------------------------------------------------------------------------------------------------ options, pair lists, refusals
def test_options(xmamd, cases):
    c = cases["b"]
    for kw in pn.OPTION_SETS:
        ref = _ref(c, **kw)
        _same(_run(xmamd, c, **kw), ref, str(kw))
    two = _run(xmamd, c, min_flags=2)
    assert 0 < two.outlier.sum() < (two.count > 0).sum()


def test_pairs_listed_twice_and_reversed(xmamd, cases):
    c = dict(cases["b"])
    base = _run(xmamd, c)
    c.update(pn.doubled_pairs(c))
    plan = _run(xmamd, c)
    _same(plan, _ref(c))
    npairs = base.stats.size
    assert plan.stats[npairs:npairs + 10].tobytes() == base.stats[:10].tobytes()         # a pair listed twice: the same answer, counted twice
    assert np.all(plan.count >= base.count) and plan.count.sum() > base.count.sum()
    assert np.array_equal(plan.stats["n_joint"][npairs + 10:], base.stats["n_joint"])      # (j, i, R^T): accepted, a pair of its own


def test_refusals(xmamd, cases):
    c = dict(cases["b"])
    dup = dict(c)
    dup["cam"] = np.concatenate([c["cam"], c["cam"][5:6]]); dup["lm"] = np.concatenate([c["lm"], c["lm"][5:6]]); dup["p"] = np.concatenate([c["p"], c["p"][5:6]])
    with pytest.raises(xmamd.XmError, match="error -2.*twice"):
        _run(xmamd, dup)
    for change, word in ((dict(pi=c["pj"]), "one camera twice"), (dict(pj=np.where(np.arange(c["pj"].size) == 3, 12, c["pj"])), "out of range"),
                         (dict(n=11), "out of range"), (dict(m=79), "out of range")):
        bad = dict(c); bad.update(change)
        with pytest.raises(xmamd.XmError, match="error -2.*" + word):
            _run(xmamd, bad)
    _same(_run(xmamd, c), _ref(c))                        # still usable


def test_degenerate_pair(xmamd):
    c = pn.two_camera_scene(50, 7, True)
    c["p"][c["cam"] == 0] = np.array([0.5, -1.0, 2.0])    # all src points equal: scale2 = 0
    plan = _run(xmamd, c)
    assert plan.stats["status"][0] == xmamd.PAIR_DEGENERATE and plan.stats["n_joint"][0] == 50 and plan.stats["scale2"][0] == 0.0
    assert not plan.count.any() and not plan.outlier.any() and plan.info["pairs_degenerate"] == 1 and plan.info["pairs_used"] == 0
    _same(plan, _ref(c))
    c = pn.two_camera_scene(50, 7, True)
    common = np.flatnonzero((c["cam"] == 1) & np.isin(c["lm"], c["lm"][c["cam"] == 0]))
    c["p"][common[3], 1] = np.nan                         # a common point that is not a number: the same
    plan = _run(xmamd, c)
    assert plan.stats["status"][0] == xmamd.PAIR_DEGENERATE and not plan.count.any()


def test_empty_inputs(xmamd):
    z = np.zeros(0, dtype=np.int32)
    plan = xmamd.pair_filter(z, z, np.zeros((0, 3)), z, z, np.zeros((0, 3, 3)), n=3, m=4)
    assert plan.count.size == 0 and plan.stats.size == 0 and plan.info["pairs_used"] == 0
    c = pn.two_camera_scene(30, 2, False)
    plan = xmamd.pair_filter(c["cam"], c["lm"], c["p"], z, z, np.zeros((0, 3, 3)))
    assert not plan.count.any() and plan.info["max_joint"] == 0


# ------------------------------------------------------------------------------------------------ determinism
def test_two_calls_and_a_permuted_list(xmamd, cases):
    LIMIT = xmamd.pair_filter_limits()["lds_joint"]
    for c in (cases["b"], pn.two_camera_scene(LIMIT + 1, 1000 + LIMIT + 1, True)):
        first, second = _run(xmamd, c), _run(xmamd, c)
        for a in ("count", "outlier", "stats"):
            assert getattr(first, a).tobytes() == getattr(second, a).tobytes()
        perm = np.random.default_rng(4).permutation(c["cam"].size)
        d = dict(c); d["cam"], d["lm"], d["p"] = c["cam"][perm], c["lm"][perm], c["p"][perm]
        third = _run(xmamd, d)
        assert np.array_equal(third.count, first.count[perm]) and third.stats.tobytes() == first.stats.tobytes()


# ------------------------------------------------------------------------------------------------ end to end
def test_filter_clean_solve(xmamd, cases):
    import os
    c = cases["a"]
    w = np.load(os.path.join(pn.GOLDEN, "simple2", "obs.npz"))["w"].reshape(-1)
    plan = _run(xmamd, c)
    cam, lm, p, w = plan.apply(c["cam"], c["lm"], c["p"], w)
    assert cam.size == c["cam"].size - plan.info["nobs_flagged"] and 0 < plan.info["nobs_flagged"] < c["cam"].size // 2
    clean = xmamd.clean_observations(cam, lm, w, c["n"], c["m"])
    cam, lm, p, w = clean.apply(cam, lm, p, w)
    ctx = xmamd.Context(obs=(cam, lm, p, w))
    R, s, info = ctx.solve(5, 1e-6, 0.0)
    ctx.close()
    print(f"pair filter: {plan.info}; cleaning keeps {clean.info['nobs_new']} observations, {clean.info['n_new']} cameras; solve: rank {info['rank']}, "
          f"status {info['status']}, primal {info['primal']:.6e}")
    assert info["status"] == 1                            # certified
