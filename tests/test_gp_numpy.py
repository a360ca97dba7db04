"""CPU tests of the restatement of the global positioning (tests/xm_gp_numpy.py; xm_ctx_global_positioning, include/xm_amd.h): the
Jacobian against central differences, the closed-form elimination of the scales against the restatement's own Schur complement of the full
system, the active-set rule, and convergence from random starts.  Nothing here was compared with the reference's compiled code.

Measured with this restatement (min_views = 3, Huber 0.1 unless said otherwise):
  noise-free 8 x 40 (seed 0: 153 observations), starts 1-3:  10, 11, 12 iterations, final cost 1.5e-30, 9.7e-31, 7.2e-31, recovery error
      (centres and points after a similarity, relative to the extent) 1.4e-16, 1.2e-16, 2.5e-16
  20 x 200, noise 2e-3, function_tol 1e-14, starts 1-3:  10 iterations each, final costs equal to 1.6e-15 relative
  12 x 80 (seed 32) with 5 % random bearings, starts 1, 2:  Huber centre error 3.0e-2 and 3.0e-2 of the extent (25 and 29 iterations),
      trivial loss 2.8e-1 and 2.9e-1"""
import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_gp_numpy as gp

TIGHT = dict(gradient_tol=1e-14, parameter_tol=1e-16)          # test_gpu_ba.py


def _obs(S):
    return S["cam"], S["lm"], S["p"], S["w"]


def _point(S, seed, spread=0.05):
    """a point near the scene (so that no loss is saturated everywhere) with scales on both sides of 1"""
    rng = np.random.default_rng(seed)
    t = S["t"] + spread * rng.standard_normal(S["t"].shape)
    P = S["P"] + spread * rng.standard_normal(S["P"].shape)
    depth = np.linalg.norm(S["P"][:, S["lm"]] - S["t"][:, S["cam"]], axis=0)
    return t, P, (1.0 / depth) * rng.uniform(0.8, 1.25, depth.size)


def test_jacobian_matches_central_differences():
    S = ba.ring_scene(n_cams=5, n_pts=12, seed=3, noise=1e-3)
    t, P, s_all = _point(S, 4)
    for loss, a in (("trivial", 0.0), ("huber", 0.02)):
        pr = gp.Problem(*_obs(S), S["rot"], S["n"], S["m"], loss=loss, a=a)
        c, X, s = t.T.copy(), P.T.copy(), s_all[pr.idx]
        B = pr.blocks(c, X, s)
        J = pr.jacobian(B).toarray()
        sw = np.sqrt(B["w"])
        h = 1e-6
        cols = []
        for k in range(J.shape[1]):
            d = np.zeros(J.shape[1]); d[k] = h
            dc, dP, ds = pr.split(d)
            rp = pr.residuals(c + dc, X + dP, s + ds); rm = pr.residuals(c - dc, X - dP, s - ds)
            cols.append((sw[:, None] * (rp - rm) / (2 * h)).reshape(-1))          # Corrector: the weights are those of the point itself
        Jn = np.stack(cols, axis=1)
        assert np.abs(J - Jn).max() <= 1e-7 * np.abs(Jn).max(), loss


@pytest.mark.parametrize("loss,a", [("trivial", 0.0), ("huber", 0.02), ("cauchy", 0.05)])
def test_closed_form_elimination_is_the_schur_complement_of_the_full_system(loss, a):
    S = ba.ring_scene(n_cams=6, n_pts=20, seed=5, noise=1e-3)
    t, P, s_all = _point(S, 6)
    P, s_all = gp.bound_point(S, t, P, s_all)                               # some at the bound: frozen where g_s > 0, free elsewhere
    pr = gp.Problem(*_obs(S), S["rot"], S["n"], S["m"], loss=loss, a=a)
    n, m, k = pr.n, pr.m, pr.k
    mu = 1e-2
    rng = np.random.default_rng(7)
    dc = 1e-2 * rng.standard_normal((n, 3))
    E = gp.stages(pr, t, P, s_all, mu, dc=dc)
    B, s = E["_B"], E["_s"]
    assert B["frozen"].any() and (~B["frozen"] & (s <= gp.S_MIN)).any()
    # the formulas of include/xm_amd.h, observation by observation
    M, q, hs = gp.closed_form(B, s, mu)
    Mfull = np.zeros((pr.nobs, 6)); Mfull[pr.idx] = M[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    assert np.allclose(Mfull, E["M"], rtol=1e-12, atol=1e-14 * np.abs(E["M"]).max())
    assert np.allclose(q, E["q"][pr.idx], rtol=1e-12, atol=1e-14 * np.abs(q).max())
    # the full damped system, solved with dc imposed: (dP, ds) = -[H_PP H_Ps; H_sP H_ss]*^-1 (g + H_.c dc)
    J = pr.jacobian(B).toarray()
    r = B["r"].reshape(-1)
    H = J.T @ J
    Hs = H + mu * np.diag(np.clip(np.diag(H), 1e-6, 1e32))
    g = J.T @ r
    rest = slice(3 * n, None)
    y = -np.linalg.solve(Hs[rest, rest], g[rest] + Hs[rest, :3 * n] @ dc.reshape(-1))
    dP, ds = y[:3 * m].reshape(m, 3), y[3 * m:]
    assert np.allclose(E["dP"], dP, rtol=1e-9, atol=1e-12 * np.abs(dP).max())
    assert np.allclose(E["ds"][pr.idx], ds, rtol=1e-9, atol=1e-12 * np.abs(ds).max())
    assert not E["ds"][pr.idx][B["frozen"]].any()
    # S and b are the Schur complement and right-hand side of the same system on the cameras
    Sc = Hs[:3 * n, :3 * n] - Hs[:3 * n, rest] @ np.linalg.solve(Hs[rest, rest], Hs[rest, :3 * n])
    bc = -g[:3 * n] + Hs[:3 * n, rest] @ np.linalg.solve(Hs[rest, rest], g[rest])
    assert np.allclose(E["S"], Sc, rtol=1e-9, atol=1e-11 * np.abs(Sc).max())
    assert np.allclose(E["b"].reshape(-1), bc, rtol=1e-9, atol=1e-11 * np.abs(bc).max())
    d = np.concatenate([dc.reshape(-1), dP.reshape(-1), ds])
    Jd = J @ d
    assert np.isclose(E["model"], r @ Jd + 0.5 * Jd @ Jd, rtol=1e-9)
    assert np.isclose(E["gmax"], np.abs(g).max(), rtol=1e-12)


def test_longdouble_evaluation_agrees():
    S = ba.ring_scene(n_cams=6, n_pts=20, seed=5, noise=1e-3)
    t, P, s_all = _point(S, 6)
    X = np.random.default_rng(8).standard_normal((18, 2))
    out = []
    for dt in (np.float64, gp.LD):
        pr = gp.Problem(*_obs(S), S["rot"], S["n"], S["m"], dtype=dt)
        out.append(gp.stages(pr, t, P, s_all, 1e-3, X=X, dc=X[:, 0] * 1e-2))
    for k in ("M", "q", "vinv", "g_l", "ustar", "sinv", "b", "SX", "dP", "ds"):
        e = np.abs(np.asarray(out[0][k], dtype=gp.LD) - out[1][k]).max() / np.abs(out[1][k]).max()
        assert e < 1e-10, (k, float(e))


def test_min_views_and_masks():
    S = ba.ring_scene(n_cams=8, n_pts=30, seed=9, min_views=2)
    deg = np.bincount(S["lm"], minlength=S["m"])
    w = S["w"].copy()
    first = np.nonzero(S["lm"] == np.argmax(deg >= 3))[0]
    w[first[:-2]] = 0.0                                                     # a landmark left with two weighted observations
    u = gp.used_mask(S["lm"], S["p"], w, S["m"], 3)
    assert not u[first].any() and u.sum() < (w > 0).sum()
    assert gp.used_mask(S["lm"], S["p"], w, S["m"], 2)[first[-2:]].all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_free_scene_is_recovered_from_a_random_start(seed):
    S = ba.ring_scene(n_cams=8, n_pts=40, seed=0)
    t0, P0 = gp.random_start(S["n"], S["m"], seed)
    t, P, info = gp.lm(*_obs(S), S["rot"], t0, P0, **TIGHT)
    print(f"start {seed}: {info['iters']} iterations, cost {info['initial_cost']:.3e} -> {info['final_cost']:.3e}, error {gp.recovery_error(S, t, P):.2e}")
    assert 8 <= info["iters"] <= 12
    assert info["final_cost"] < 1e-20
    assert gp.recovery_error(S, t, P) < 1e-9
    assert info["scales"].min() > gp.S_MIN


def test_starts_reach_the_same_minimum_on_a_noisy_scene():
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=2e-3)
    F = []
    for seed in (1, 2, 3):
        t0, P0 = gp.random_start(S["n"], S["m"], seed)
        _, _, info = gp.lm(*_obs(S), S["rot"], t0, P0, function_tol=1e-14)
        F.append(info["final_cost"])
    print("final costs", F)
    assert (max(F) - min(F)) <= 1e-8 * min(F)


def _centre_error(S, t):
    Bm = S["t"]
    return float(np.sqrt(np.sum((gp.align(t, Bm) - Bm) ** 2, axis=0)).max() / np.linalg.norm(Bm.max(axis=1) - Bm.min(axis=1)))


@pytest.mark.parametrize("seed", [1, 2])
def test_huber_resists_random_bearings(seed):
    S = gp.bearing_scene(12, 80, seed=32, outliers=0.05)
    assert 3 <= S["bad"].sum() <= 0.1 * S["bad"].size
    t0, P0 = gp.random_start(S["n"], S["m"], seed)
    th, _, ih = gp.lm(*_obs(S), S["rot"], t0, P0)
    tt, _, it = gp.lm(*_obs(S), S["rot"], t0, P0, loss="trivial", a=0.0)
    eh, et = _centre_error(S, th), _centre_error(S, tt)
    print(f"start {seed}: Huber {eh:.3e} ({ih['iters']} it), trivial {et:.3e} ({it['iters']} it)")
    assert ih["status"] in (1, 2, 3)
    assert eh < 0.25 * et


def test_scale_at_the_bound_is_frozen_only_while_its_gradient_points_outward():
    S = ba.ring_scene(n_cams=5, n_pts=12, seed=3)
    pr = gp.Problem(*_obs(S), S["rot"], S["n"], S["m"], loss="trivial", a=0.0)
    c, X = S["t"].T.copy(), S["P"].T.copy()
    s = np.full(pr.k, gp.S_MIN)
    B = pr.blocks(c, X, s)                                                  # d.v > 0 at the true geometry: the gradient points inward, nothing freezes
    assert not B["frozen"].any()
    P2, _ = gp.bound_point(S, S["t"], S["P"], np.ones(S["cam"].size))       # a landmark behind the cameras on its side: d.v < 0 there
    B = pr.blocks(c, P2.T.copy(), s)
    assert B["frozen"].any() and not B["frozen"].all()
    assert not B["Js"][B["frozen"]].any() and not B["gs"][B["frozen"]].any() and B["Js"][~B["frozen"]].any(axis=1).all()
    # the candidate never leaves the bound, whatever the step
    _, _, s1 = pr.plus(c, X, s, -np.ones(3 * pr.n + 3 * pr.m + pr.k))
    assert s1.min() == gp.S_MIN
