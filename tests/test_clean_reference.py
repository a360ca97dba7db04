"""CPU tests of the definition of observation cleaning (include/xm_amd.h at xm_clean_observations): the numpy / scipy restatement
(tests/xm_clean_numpy.py) against what the reference's own code returned (tests/golden/clean, recorded by tests/golden/make_clean.py), exactly,
for checklandmarks (thresholds 10, 1) and for the inline sequence of 2_test_creatematrix.py (0, 1); and CleanPlan.apply against the arrays
the reference returned."""
import hashlib
import os

import numpy as np
import pytest

import xm_clean_numpy as cn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", params=cn.CASES)
def case(request):
    return cn.load_case(GOLDEN, request.param)


def _sha(cam, lm, p, w):
    h = hashlib.sha256()
    for a, t in ((np.stack([cam, lm], axis=1), np.int64), (p, np.float64), (w, np.float64)):
        h.update(np.ascontiguousarray(a, dtype=t).tobytes())
    return h.hexdigest()


def test_restatement_equals_checklandmarks(case):
    fx = case["fx"]
    r = cn.clean_numpy(case["cam"], case["lm"], case["w"], case["n"], case["m"], 10, 1)
    assert np.array_equal(r["keep"], cn.fixture_keep(fx, "10_1"))
    assert np.array_equal(r["cam_index"], fx["indices_all_10_1"])
    assert np.array_equal(r["lm_index"], fx["lm_index_10_1"])
    assert [r["info"][k] for k in ("n_new", "m_new", "nobs_new")] == list(fx["counts_10_1"])


def test_restatement_equals_inline_sequence(case):
    """thresholds (0, 1).  The script's own indices_all is not a fixture (make_clean.py says why); the camera numbering is pinned through the
    arrays it returned, in test_apply_gives_the_reference_arrays."""
    fx = case["fx"]
    r = cn.clean_numpy(case["cam"], case["lm"], case["w"], case["n"], case["m"], 0, 1)
    assert np.array_equal(r["keep"], cn.fixture_keep(fx, "0_1"))
    assert np.array_equal(r["lm_index"], fx["lm_index_0_1"])
    assert [r["info"][k] for k in ("n_new", "m_new", "nobs_new")] == list(fx["counts_0_1"])


def test_recorded_numbers():
    """the figures of the reference on its own data and on the scene in which every stage acts"""
    a = np.load(os.path.join(GOLDEN, "clean", "a.npz")); b = np.load(os.path.join(GOLDEN, "clean", "b.npz"))
    assert list(a["counts_10_1"]) == [93, 5998, 58065] and a["indices_all_10_1"][0] == 10 and a["indices_all_10_1"][10] == 0
    assert list(b["indices_all_10_1"]) == [2, 1, 0, 3, 4, 5, -1, -1, -1, -1, -1, -1] and list(b["counts_10_1"]) == [6, 40, 180]
    r = cn.clean_numpy(b["cam"], b["lm"], None, int(b["n"]), int(b["m"]))["info"]
    assert (r["cams_weak"], r["cams_emptied"], r["cams_off_component"], r["lms_off_component"], r["components"]) == (2, 1, 3, 20, 2)
    assert r["lms_weak"] == 77 - 40 - 20 and r["first_camera"] == 2


@pytest.mark.parametrize("tag,thr", [("10_1", (10, 1)), ("0_1", (0, 1))])
def test_apply_gives_the_reference_arrays(xmamd, case, tag, thr):
    r = cn.clean_numpy(case["cam"], case["lm"], case["w"], case["n"], case["m"], *thr)
    plan = xmamd.CleanPlan(r["keep"], r["cam_index"], r["lm_index"], r["info"])
    cam, lm, p, w = plan.apply(case["cam"], case["lm"], case["p"], case["w"])
    assert cam.size == r["info"]["nobs_new"] and cam.min() == 0 and lm.min() == 0
    assert cam.max() + 1 == r["info"]["n_new"] and lm.max() + 1 == r["info"]["m_new"] and np.all(w > 0)
    assert _sha(cam, lm, p, w) == str(case["fx"]["sha_" + tag])
    for got, want in zip((cam, lm, p, w), cn.apply_numpy(r, case["cam"], case["lm"], case["p"], case["w"])):
        assert np.array_equal(got, want)


def test_apply_refuses_another_list(xmamd):
    plan = xmamd.CleanPlan(np.ones(3, dtype=bool), np.arange(2, dtype=np.int32), np.arange(2, dtype=np.int32), {})
    with pytest.raises(xmamd.XmError):
        plan.apply(np.zeros(4, dtype=int), np.zeros(4, dtype=int))
    with pytest.raises(xmamd.XmError):
        plan.apply(np.zeros(3, dtype=int), np.zeros(3, dtype=int), np.zeros(2))


def test_nothing_survives():
    cam, lm, n, m = cn.chain_scene(8, 0)
    r = cn.clean_numpy(cam, lm, None, n, m)      # six observations per camera: none has more than 10
    assert not r["keep"].any() and np.all(r["cam_index"] == -1) and np.all(r["lm_index"] == -1)
    assert [r["info"][k] for k in ("n_new", "m_new", "nobs_new", "components")] == [0, 0, 0, 0]


def test_chain_tie_goes_to_the_earlier_observation():
    for seed in (1, 2, 3, 4):
        cam, lm, n, m = cn.chain_scene(64, seed, cut=32)
        r = cn.clean_numpy(cam, lm, None, n, m, 0, 1)
        assert r["info"]["components"] == 2 and r["info"]["n_new"] == 32 == r["info"]["cams_off_component"]
        assert r["info"]["m_new"] == r["info"]["lms_off_component"]          # the tie
        graph_rows = (np.bincount(lm, minlength=m) > 1)[lm]                  # cameras all pass at threshold 0: the rows of the stage-3 graph
        assert r["keep"][int(np.flatnonzero(graph_rows)[0])]
