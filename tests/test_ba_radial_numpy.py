"""CPU tests of the restatements behind the radial refinement (xm_ctx_bundle_adjust_radial, include/xm_amd.h): the f64 restatement
xm_ba_radial_numpy.py against central differences and against the longdouble statement xm_ba_radial_exact.py; that with k = 0 held it is
the focal restatement; what the coefficient buys on a scene seen through distorting lenses; for every case of the GPU stage test
(test_gpu_ba_radial_stages.py), that the f64 restatement lies within MAX_E_REF of the longdouble reference and that the stage bound
rejects the restatement damaged as a bug would damage it; and xmamd.undistort_observations (host numpy)."""
import numpy as np
import pytest

import xm_ba_focal_numpy as bf
import xm_ba_numpy as ba
import xm_ba_radial_exact as rx
import xm_ba_radial_numpy as br
import xm_ba_radial_stages as rs
import xm_ba_stages as st


def _small(seed=3):
    S = ba.ring_scene(n_cams=6, n_pts=20, seed=seed, noise=1e-2)
    rot, t, P = ba.perturb(S["rot"], S["t"], S["P"], seed=seed + 1, deg=5.0, rel=0.05)
    focal = np.random.default_rng(seed + 2).uniform(0.8, 1.25, 6)
    dist = np.array([0.12, -0.15, 0.05, -0.03, 0.15, -0.09])
    return S, rot, t, P, focal, dist


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask"])
def test_jacobian_against_central_differences_and_longdouble(fix, masked):
    S, rot, t, P, focal, dist = _small()
    free = np.array([1, 0, 1, 1, 0, 1], dtype=bool) if masked else None
    kfree = np.array([1, 1, 0, 1, 0, 0], dtype=bool) if masked else None
    pr = br.RadialProblem(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], fix, free=free, kfree=kfree)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    r, J = pr.jacobian(Rcw, tcw, P.T.copy(), focal, dist)
    J = J.toarray()
    cd, n, m, k = pr.cd, S["n"], S["m"], pr.cam.size
    assert cd == (5 if fix else 8) and J.shape == (2 * k, cd * n + 3 * m)
    E = rx.RadialExact(S["cam"], S["lm"], S["p"], S["w"], n, m, rot, t, P, focal, dist, 1.0, fix, free=free, kfree=kfree)
    Jx = np.zeros(J.shape, dtype=rx.LD)
    for e in range(k):
        Jx[2 * e:2 * e + 2, cd * E.cam[e]:cd * E.cam[e] + cd] = E.Jc[e]
        Jx[2 * e:2 * e + 2, cd * n + 3 * E.lm[e]:cd * n + 3 * E.lm[e] + 3] = E.JP[e]
    scale = float(np.abs(Jx).max())
    assert float(np.abs(J - Jx).max()) <= 1e-9 * scale
    assert float(np.abs(r - E.r.reshape(-1)).max()) <= 1e-9
    # central differences in longdouble, h = 1e-7: truncation ~ h^2, rounding ~ eps_longdouble / h, both far below the tolerance
    Jd = rx.central_difference(S["cam"], S["lm"], S["p"], S["w"], n, m, rot, t, P, focal, dist, fix, free, kfree, h=rx.LD(1e-7))
    assert float(np.abs(Jx - Jd).max()) <= 1e-9 * scale
    assert float(np.abs(J - Jd).max()) <= 1e-9 * scale
    fcols, kcols = cd * np.arange(n) + cd - 2, cd * np.arange(n) + cd - 1
    held = np.zeros(n, dtype=bool) if free is None else ~free
    kheld = np.zeros(n, dtype=bool) if kfree is None else ~kfree
    assert not J[:, fcols[held]].any() and all(J[:, c].any() for c in fcols[~held])
    assert not J[:, kcols[kheld]].any() and all(J[:, c].any() for c in kcols[~kheld])


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
def test_with_k_zero_held_the_trace_is_the_focal_restatement_s(fix):
    """k = 0 and every dist_free = 0: s = 1 and the factor in front of the pinhole rows is g I in every bit, the distortion column is
    zero and its unknown is decoupled (diagonal mu 1e-6, right-hand side 0), so every iteration is the focal model's"""
    S0 = ba.ring_scene(n_cams=8, n_pts=40, seed=11, noise=1e-2)
    S = bf.scale_observations(S0, bf.focal_ratios(8, 12))
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=13, deg=10.0, rel=0.1)
    args = (S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0)
    free = np.ones(8, dtype=bool); free[2] = False
    kw = dict(focal_free=free, fix_rotations=fix, function_tol=0.0, max_iters=8)
    *_, gf, ref = bf.lm(*args, **kw)
    *_, gr, kr, got = br.lm(*args, dist=np.zeros(8), dist_free=np.zeros(8, dtype=bool), **kw)
    assert got["trace"].shape == ref["trace"].shape and got["trace"].tobytes() == ref["trace"].tobytes()
    assert gr.tobytes() == gf.tobytes() and not kr.any()


def _lenses(n_cams=20, n_pts=200, seed=0):
    """the noiseless ring scene, its point cloud twice as wide as the default (rays up to rho = 0.69 off the axis), seen through lenses
    with focal ratios in [0.8, 1.25] and k in [-0.15, 0.15], and a near start.  With the default cloud the rays stay within rho = 0.4,
    k rho^2 is at most 0.024 and a focal scale absorbs most of it (focal-only optimum 1.8e-5 .. 1.1e-4 over the seeds 0 .. 119); with
    this one the focal model's optimum lies at 1.1e-3 .. 2.3e-3 over the seeds 0 .. 5"""
    S0 = ba.ring_scene(n_cams=n_cams, n_pts=n_pts, seed=seed, noise=0, cloud=4.0)
    ratio, k = bf.focal_ratios(n_cams, seed + 5), br.dist_coefficients(n_cams, seed + 6)
    S = br.distort_observations(S0, ratio, k)
    return S, ratio, k, ba.perturb(S["rot"], S["t"], S["P"], seed=seed + 1, deg=1.0, rel=0.005)


def test_distorting_lenses_are_recovered_where_the_focal_model_stalls():
    """the statements of test_gpu_ba_radial.py::test_noise_free_scene_is_solved_exactly_where_the_focal_model_stalls, on the CPU"""
    S, ratio, k, (rot0, t0, P0) = _lenses()
    args = (S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0)
    tight = dict(function_tol=0.0, gradient_tol=0.0, parameter_tol=0.0, max_iters=8)
    _, _, _, g, kd, info = br.lm(*args, **tight)
    print(f"radial model: cost {info['final_cost']:.3e} after {info['iters']} iterations, focal error {np.abs(g - ratio).max():.3e}, "
          f"k error {np.abs(kd - k).max():.3e}")
    assert info["final_cost"] <= 1e-18 and np.abs(g / ratio - 1.0).max() <= 1e-6 and np.abs(kd - k).max() <= 1e-6
    _, _, _, _, focal_only = bf.lm(*args, **{**tight, "max_iters": 50})
    print(f"focal model: cost {focal_only['final_cost']:.3e} after {focal_only['iters']} iterations")
    assert focal_only["final_cost"] > 1e-4


def test_held_values_come_back_bit_identical():
    S, ratio, k, (rot0, t0, P0) = _lenses()
    free = np.ones(20, dtype=bool); free[::3] = False
    kfree = np.ones(20, dtype=bool); kfree[1::4] = False
    f0, k0 = np.where(free, 1.0, ratio), np.where(kfree, 0.0, k)       # the held ones at the truth, so that the scene stays consistent
    _, _, _, g, kd, info = br.lm(S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0, focal=f0, focal_free=free, dist=k0, dist_free=kfree, function_tol=0.0,
                                 gradient_tol=0.0, parameter_tol=0.0, max_iters=8)
    assert g[~free].tobytes() == f0[~free].tobytes() and kd[~kfree].tobytes() == k0[~kfree].tobytes()
    assert info["final_cost"] <= 1e-18 and np.abs(kd - k).max() <= 1e-6


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("name", rs.CASES)
def test_restatement_agrees_with_longdouble(name, fix):
    """the MAX_E_REF rule of xm_ba_stages on every case the GPU stage test uses"""
    c = rs.case(name, fix)
    for mu in c["mus"]:
        kw = rs.stage_args(c, mu)
        E = rs.exact_stages(c["S"], **kw)
        e_ref = rs.reference_errors(c["S"], E, c["keys"], **kw)
        assert max(e_ref.values()) <= st.MAX_E_REF, e_ref
        assert abs(float(E["fold_min"])) > 1e-3            # whether the candidate folds does not hang on rounding
        print(f"{name} mu {mu:g}: positive {E['positive']}, least 1 + 3 k rho^2 at the candidate {float(E['fold_min']):.3g}")
    assert E["positive"] or "cost1" not in c["keys"]       # at the last mu an ordinary candidate wherever cost1 is compared
    if name == "on_axis":
        J = E["_E"].Jc[E["_E"].cam == rs.ON_AXIS_CAM]
        assert J.shape[0] == 4 and not J[:, :, -2:].any() and J[:, :, :-2].any()


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("damage, keys", [("dist_unmasked", ("ustar", "b", "S")), ("pose_pinhole", ("ustar", "b", "model")),
                                          ("x2_without_k", ("x2",))])
def test_the_bound_rejects_a_damaged_restatement(damage, keys, fix):
    c = rs.case("base", fix)
    S, mu = c["S"], 1.0
    kw = rs.stage_args(c, mu)
    E = rs.exact_stages(S, **kw)
    e_ref = rs.reference_errors(S, E, rs.ALL_KEYS, **kw)
    sound = st.compare("sound", S, rs.f64_stages(S, **kw), E, e_ref, rs.ALL_KEYS, who="f64")
    assert not sound
    bad = st.compare(damage, S, rs.f64_stages(S, damage=(damage,), **kw), E, e_ref, rs.ALL_KEYS, who="f64")
    assert set(keys) <= {k for k, *_ in bad}, bad


# ---- xmamd.undistort_observations
def _rays(nobs, seed, rho_max=0.8):
    rng = np.random.default_rng(seed)
    rho = rho_max * np.sqrt(rng.uniform(0.0, 1.0, nobs))
    rho[:3] = (0.0, rho_max, 1e-9)
    ang = rng.uniform(0.0, 2.0 * np.pi, nobs)
    return np.stack([rho * np.cos(ang), rho * np.sin(ang)], axis=1), rng.uniform(0.5, 3.0, nobs)


def test_undistort_observations_inverts_the_distortion(xmamd):
    """k in [-0.2, 0.3], rho <= 0.8: 1 + 3 k rho^2 >= 0.616, every observation lies on the monotone branch.  Newton ends within an ulp or
    two of the root of the rounded equation; the equation's own rounding (a few ulp of c) is divided by the slope >= 0.616: 32 ulp of the
    largest coordinate is a bound with room"""
    n, nobs = 11, 4000
    u, p2 = _rays(nobs, 5)
    cam = np.random.default_rng(6).integers(0, n, nobs)
    g = np.random.default_rng(7).uniform(0.8, 1.25, n)
    k = np.linspace(-0.2, 0.3, n)
    s = 1.0 + k[cam] * np.sum(u * u, axis=1)
    p = np.concatenate([(g[cam] * s)[:, None] * u * p2[:, None], p2[:, None]], axis=1)
    q, bad = xmamd.undistort_observations(p, cam, g, k)
    assert not bad.any() and bad.dtype == bool and bad.shape == (nobs,)
    assert np.array_equal(q[:, 2], p2)
    err = np.abs(q[:, :2] / q[:, 2:3] - u).max()
    print(f"undistort: max error {err:.3e}")
    assert err <= 32 * np.finfo(np.float64).eps * 0.8
    qt, badt = xmamd.undistort_observations(p.T, cam, g, k)                   # both layouts
    assert np.array_equal(qt, q.T) and np.array_equal(badt, bad)


def test_undistort_observations_at_k_zero_is_rescale_observations(xmamd):
    rng = np.random.default_rng(0)
    p = rng.uniform(-2.0, 2.0, (500, 3)); p[:, 2] = np.abs(p[:, 2]) + 0.1
    cam = rng.integers(0, 5, 500)
    g = rng.uniform(0.5, 2.0, 5)
    q, bad = xmamd.undistort_observations(p, cam, g, np.zeros(5))
    assert not bad.any() and q.tobytes() == xmamd.rescale_observations(p, cam, g).tobytes()
    p[:7, 2] = (0.0, -1.0, 0.0, np.inf, 0.0, -0.0, 1e-310)                       # and on degenerate rows: k = 0 has nothing to solve
    p[2, :2] = 0.0
    with np.errstate(all="ignore"):
        q, bad = xmamd.undistort_observations(p, cam, g, np.zeros(5))
    assert not bad.any() and q.tobytes() == xmamd.rescale_observations(p, cam, g).tobytes()
    with pytest.raises(xmamd.XmError):
        xmamd.undistort_observations(p, cam, [1.0, 0.0, 1.0, 1.0, 1.0], np.zeros(5))
    with pytest.raises(xmamd.XmError):
        xmamd.undistort_observations(p, cam, g, [0.0, np.nan, 0.0, 0.0, 0.0])


def test_undistort_observations_flags_what_lies_beyond_the_fold(xmamd):
    """k = -0.3: rho (1 + k rho^2) has its maximum 2 rho_f / 3 at rho_f = 1 / sqrt(-3 k) = 1.054; an observation with |z| / g at or above
    it has no pre-image on the monotone branch.  Exactly those are flagged and left as given; camera 1 (k > 0) has a root everywhere"""
    g, k = np.array([1.1, 0.9]), np.array([-0.3, 0.2])
    top = 2.0 / (3.0 * np.sqrt(0.9))
    c = np.array([0.0, 0.3, 0.99 * top, 1.01 * top, 5.0])
    cam = np.repeat([0, 1], c.size)
    z = np.tile(c, 2) * g[cam]
    p = np.stack([0.6 * z, 0.8 * z, np.ones(z.size)], axis=1)
    q, bad = xmamd.undistort_observations(p, cam, g, k)
    assert np.array_equal(bad, np.array([0, 0, 0, 1, 1, 0, 0, 0, 0, 0], dtype=bool))
    assert np.array_equal(q[bad], p[bad])
    rho = np.hypot(q[:, 0], q[:, 1])[~bad]
    assert np.abs(rho * (1.0 + k[cam][~bad] * rho * rho) - np.tile(c, 2)[~bad]).max() <= 1e-14
    assert (1.0 + 3.0 * k[cam][~bad] * rho * rho > 0).all()
