"""CPU tests of the aggregate plan of the bundle adjustment's opt-in preconditioners (xm_ba_aggregate_plan) against its numpy restatement,
and of the numpy model itself (xm_ba_precond_numpy.py): its coarse space by what defines it, and its PCG iteration counts."""
import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_ba_precond_numpy as bp

B = bp.AGG_CAMS


def _both(xmamd, cam, lm, n, used=None, Bk=B):
    lib = xmamd.ba_aggregate_plan(cam, lm, n=n, used=used, B=Bk)
    ref, order = bp.aggregate_plan(cam, lm, n, used, Bk)
    assert np.array_equal(lib, ref)
    return lib, order


def test_sequential_scene_gives_runs_of_consecutive_cameras(xmamd):
    S = ba.sequential_scene(n_cams=150, seed=62)
    agg, order = _both(xmamd, S["cam"], S["lm"], S["n"])
    assert np.array_equal(agg, np.arange(150) // B)
    assert np.array_equal(order, np.arange(150))


def test_ring_scene_with_heavy_landmarks(xmamd):
    S = ba.ring_scene(n_cams=72, n_pts=120, seed=60, frac=0.93)
    assert (np.bincount(S["lm"]) > 64).sum() > 10
    agg, _ = _both(xmamd, S["cam"], S["lm"], S["n"])
    assert agg.min() == 0 and np.array_equal(np.bincount(agg), [16, 16, 16, 16, 8])


def test_shuffled_camera_numbers_follow_the_trajectory(xmamd):
    S = ba.sequential_scene(n_cams=200, seed=5)
    perm = np.random.default_rng(6).permutation(200)          # frame f carries camera number perm[f]
    cam = perm[S["cam"]].astype(np.int32)
    agg, _ = _both(xmamd, cam, S["lm"], S["n"])
    frame_of = np.argsort(perm)
    for a in range(agg.max() + 1):
        fr = frame_of[np.nonzero(agg == a)[0]]
        assert fr.max() - fr.min() <= 2 * B, (a, fr)


def test_camera_without_a_used_observation_and_trailing_single(xmamd):
    S = ba.sequential_scene(n_cams=34, seed=7)
    used = np.ones(S["cam"].size, dtype=np.uint8)
    used[S["cam"] == 9] = 0
    agg, order = _both(xmamd, S["cam"], S["lm"], S["n"], used)
    assert agg[9] == -1 and (agg >= 0).sum() == 33 and 9 not in order
    assert np.array_equal(np.bincount(agg[agg >= 0]), [16, 16, 1])                  # a last aggregate of one camera
    assert bp.coarse_ranges(33) == [(0, 16), (16, 33)]                               # ... joins its predecessor's coarse columns
    agg17, _ = _both(xmamd, S["cam"][S["cam"] < 17], S["lm"][S["cam"] < 17], 17)
    assert np.array_equal(np.bincount(agg17), [16, 1])
    assert np.array_equal(xmamd.ba_aggregate_plan(S["cam"], S["lm"], n=S["n"], used=None), bp.aggregate_plan(S["cam"], S["lm"], S["n"])[0])


def test_the_limit_of_4096_aggregates(xmamd):
    n = B * bp.MAX_AGGREGATES
    cam = np.repeat(np.arange(n + 1, dtype=np.int32), 2)
    lm = (np.arange(2 * (n + 1), dtype=np.int32) + 1) // 2                            # a chain: camera i sees landmarks i and i + 1
    ok = xmamd.ba_aggregate_plan(cam[:2 * n], lm[:2 * n], n=n)
    assert ok.max() == bp.MAX_AGGREGATES - 1 and np.array_equal(ok, np.arange(n) // B)
    with pytest.raises(xmamd.XmError):
        xmamd.ba_aggregate_plan(cam, lm, n=n + 1)
    assert "XM_BA_MAX_AGGREGATES" in xmamd.lib().xm_last_error().decode()


@pytest.mark.parametrize("fix", [False, True])
def test_coarse_columns_are_null_vectors_of_the_noise_free_system(fix):
    # at the true parameters of a noise-free scene a rigid motion or a scaling of everything changes no residual: the columns of P for ONE
    # aggregate holding all cameras are null vectors of S (up to the damping mu = 1e-13); unit vectors per coordinate are not
    S = ba.sequential_scene(n_cams=60, noise=0.0)
    A, _, Rcw, tcw = bp.reduced_system(S["cam"], S["lm"], S["p"], S["w"], S["rot"], S["t"], S["P"], 1e-13, fix)
    P, dropped = bp.rigid_basis(Rcw, tcw, np.arange(60), B=60, fix_rotations=fix, scale=False)
    assert P.shape[1] == (4 if fix else 7) and not dropped
    norm_inf = abs(A).sum(axis=1).max()
    P = P.toarray()
    for k in range(P.shape[1]):
        res = np.linalg.norm(A @ P[:, k])
        print(f"column {k}: |S P_k| = {res:.2e}, bound {1e-12 * norm_inf * np.linalg.norm(P[:, k]):.2e}")
        assert res <= 1e-12 * norm_inf * np.linalg.norm(P[:, k])
    cd = 3 if fix else 6
    for k in range(cd):
        e = np.zeros(cd * 60); e[k::cd] = 1.0
        assert np.linalg.norm(A @ e) > 1e-7 * norm_inf * np.linalg.norm(e)


def test_the_model_reproduces_the_iteration_counts_of_the_issue():
    # sequential_scene(600) from the start of test_harder_scenes_reach_the_numpy_optimum[sequential], PCG to 1e-6: B = 16 + rigid coarse
    # space 28 (mu = 1e-4) and 73 (mu = 1e-8), 6 x 6 Jacobi 304 (mu = 1e-4); +-20 %: CG counts at a fixed threshold move by a few iterations
    # with the summation order of the BLAS
    S = ba.sequential_scene(n_cams=600, seed=62, noise=1e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=63, deg=0.5, rel=2e-4)
    obs = (S["cam"], S["lm"], S["p"], S["w"])
    got = {(kind, mu): bp.first_step_iterations(*obs, rot0, t0, P0, mu, 1e-6, kind, cap=3000)
           for kind, mu in (("two_level", 1e-4), ("two_level", 1e-8), ("jacobi", 1e-4))}
    print(got)
    for key, want in ((("two_level", 1e-4), 28), (("two_level", 1e-8), 73), (("jacobi", 1e-4), 304)):
        assert abs(got[key] - want) <= 0.2 * want, (key, got[key], want)
