"""CPU tests of the restatements behind the focal refinement (xm_ctx_bundle_adjust_focal, include/xm_amd.h): the f64 restatement
xm_ba_focal_numpy.py against central differences and against the longdouble statement xm_ba_focal_exact.py; what the model buys on a
scene whose focal priors are wrong; the rule for focals that would turn non-positive; and, for every case of the GPU stage test
(test_gpu_ba_focal_stages.py), that the f64 restatement lies within MAX_E_REF of the longdouble reference and that the stage bound rejects
the restatement damaged as a bug would damage it."""
import numpy as np
import pytest

import xm_ba_focal_exact as fx
import xm_ba_focal_numpy as bf
import xm_ba_focal_stages as fs
import xm_ba_numpy as ba
import xm_ba_stages as st


def _small(seed=3):
    S = ba.ring_scene(n_cams=6, n_pts=20, seed=seed, noise=1e-2)
    rot, t, P = ba.perturb(S["rot"], S["t"], S["P"], seed=seed + 1, deg=5.0, rel=0.05)
    focal = np.random.default_rng(seed + 2).uniform(0.8, 1.25, 6)
    return S, rot, t, P, focal


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask"])
def test_jacobian_against_central_differences_and_longdouble(fix, masked):
    S, rot, t, P, focal = _small()
    free = np.array([1, 0, 1, 1, 0, 1], dtype=bool) if masked else None
    pr = bf.FocalProblem(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], fix, free=free)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    r, J = pr.jacobian(Rcw, tcw, P.T.copy(), focal)
    J = J.toarray()
    cd, n, m, k = pr.cd, S["n"], S["m"], pr.cam.size
    assert cd == (4 if fix else 7) and J.shape == (2 * k, cd * n + 3 * m)
    E = fx.FocalExact(S["cam"], S["lm"], S["p"], S["w"], n, m, rot, t, P, focal, 1.0, fix, free=free)
    Jx = np.zeros(J.shape, dtype=fx.LD)
    for e in range(k):
        Jx[2 * e:2 * e + 2, cd * E.cam[e]:cd * E.cam[e] + cd] = E.Jc[e]
        Jx[2 * e:2 * e + 2, cd * n + 3 * E.lm[e]:cd * n + 3 * E.lm[e] + 3] = E.JP[e]
    scale = float(np.abs(Jx).max())
    assert float(np.abs(J - Jx).max()) <= 1e-9 * scale
    assert float(np.abs(r - E.r.reshape(-1)).max()) <= 1e-9
    # central differences in longdouble, h = 1e-7: truncation ~ h^2, rounding ~ eps_longdouble / h, both far below the tolerance
    Jd = fx.central_difference(S["cam"], S["lm"], S["p"], S["w"], n, m, rot, t, P, focal, fix, free, h=fx.LD(1e-7))
    assert float(np.abs(Jx - Jd).max()) <= 1e-9 * scale
    assert float(np.abs(J - Jd).max()) <= 1e-9 * scale
    fcols = cd * np.arange(n) + cd - 1
    held = np.zeros(n, dtype=bool) if free is None else ~free
    assert not J[:, fcols[held]].any() and all(J[:, c].any() for c in fcols[~held])


def _wrong_priors(n_cams=20, n_pts=200):
    """the noiseless ring scene seen with focal priors that are off by a ratio in [0.8, 1.25], and a near start"""
    S0 = ba.ring_scene(n_cams=n_cams, n_pts=n_pts, seed=0, noise=0)
    ratio = bf.focal_ratios(n_cams, 5)
    S = bf.scale_observations(S0, ratio)
    return S, ratio, ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=1.0, rel=0.005)


def test_wrong_focal_priors_are_recovered_where_the_pose_only_model_stalls():
    S, ratio, (rot0, t0, P0) = _wrong_priors()
    args = (S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0)
    tight = dict(function_tol=0.0, gradient_tol=0.0, parameter_tol=0.0, max_iters=5)     # five LM iterations, no other stop
    _, _, _, g, info = bf.lm(*args, **tight)
    print(f"focal model: cost {info['final_cost']:.3e} after {info['iters']} iterations, focal error {np.abs(g - ratio).max():.3e}")
    assert info["final_cost"] <= 1e-18 and np.abs(g - ratio).max() <= 1e-8
    _, _, _, plain = ba.lm(*args, **{**tight, "max_iters": 50})
    print(f"pose-only model: cost {plain['final_cost']:.3e} after {plain['iters']} iterations")
    assert plain["final_cost"] > 1e-4


def test_held_focals_come_back_bit_identical():
    S, ratio, (rot0, t0, P0) = _wrong_priors()
    free = np.ones(20, dtype=bool); free[::3] = False
    f0 = np.where(free, 1.0, ratio)                        # the held ones at the truth, so that the scene stays consistent
    _, _, _, g, info = bf.lm(S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0, focal=f0, focal_free=free, function_tol=0.0, gradient_tol=0.0, parameter_tol=0.0,
                             max_iters=5)
    assert g[~free].tobytes() == f0[~free].tobytes()
    assert info["final_cost"] <= 1e-18 and np.abs(g - ratio).max() <= 1e-8


def test_a_start_far_below_ends_at_the_truth_with_positive_focals():
    S, ratio, (rot0, t0, P0) = _wrong_priors()
    _, _, _, g, info = bf.lm(S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0, focal=np.full(20, 0.05))
    print(f"g = 0.05 start: {info['iters']} iterations, {info['accepted']} accepted, {info['invalid']} invalid, least accepted focal {info['min_focal']:.3g}")
    assert info["min_focal"] > 0 and (g > 0).all()
    assert info["final_cost"] <= 1e-15 and np.abs(g - ratio).max() <= 1e-6


def test_a_candidate_with_a_focal_that_is_not_positive_is_rejected():
    """from a start far off (rotations turned by up to 60 degrees) some steps take a focal below zero: each such iteration is rejected
    whatever its cost, the damping grows as after a step without model decrease (radius /= nu), and every accepted focal is positive"""
    S, ratio, _ = _wrong_priors()
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=21, deg=60.0, rel=0.6)
    _, _, _, g, info = bf.lm(S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0, max_iters=60)
    tr = info["trace"]
    print(f"far start: {info['iters']} iterations, {info['accepted']} accepted, {info['invalid']} invalid, least accepted focal {info['min_focal']:.3g}")
    assert info["invalid"] > 0 and info["min_focal"] > 0 and (g > 0).all()
    for k in info["invalid_at"]:
        assert tr[k, 3] == 0
        if k + 1 < len(tr):
            assert tr[k + 1, 2] > tr[k, 2]                 # mu = 1 / radius


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("name", fs.CASES)
def test_restatement_agrees_with_longdouble(name, fix):
    """the MAX_E_REF rule of xm_ba_stages on every case the GPU stage test uses"""
    c = fs.case(name, fix)
    for mu in c["mus"]:
        kw = fs.stage_args(c, mu)
        E = fs.exact_stages(c["S"], **kw)
        e_ref = fs.reference_errors(c["S"], E, c["keys"], **kw)
        assert max(e_ref.values()) <= st.MAX_E_REF, e_ref


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("damage, keys", [("focal_unmasked", ("ustar", "b", "S")), ("pose_unscaled", ("ustar", "b", "model")),
                                          ("x2_without_g", ("x2",))])
def test_the_bound_rejects_a_damaged_restatement(damage, keys, fix):
    c = fs.case("base", fix)
    S, mu = c["S"], 1.0
    kw = fs.stage_args(c, mu)
    E = fs.exact_stages(S, **kw)
    e_ref = fs.reference_errors(S, E, fs.ALL_KEYS, **kw)
    sound = st.compare("sound", S, fs.f64_stages(S, **kw), E, e_ref, fs.ALL_KEYS, who="f64")
    assert not sound
    bad = st.compare(damage, S, fs.f64_stages(S, damage=(damage,), **kw), E, e_ref, fs.ALL_KEYS, who="f64")
    assert set(keys) <= {k for k, *_ in bad}, bad
