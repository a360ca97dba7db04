"""CPU tests of the restatements behind the focal groups (xm_ctx_bundle_adjust_focal_groups, include/xm_amd.h): the f64 restatement
xm_ba_groups_numpy.py (J_shared = J_7 E, the LM of xm_ba_focal_numpy with the damping on the shared parameter, the preconditioner
M = blockdiag(pose blocks, F)) against its own definitions, against xm_ba_focal_numpy.lm where every group is a singleton, and against
the longdouble statement xm_ba_groups_exact.py on every case of the GPU stage test (test_gpu_ba_groups_stages.py)."""
import numpy as np
import pytest

import xm_ba_focal_numpy as bf
import xm_ba_groups_numpy as bg
import xm_ba_groups_stages as gs
import xm_ba_numpy as ba
import xm_ba_stages as st

FIX = pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])


def _small(fix, seed=3, G=3):
    S = ba.ring_scene(n_cams=8, n_pts=30, seed=seed, noise=1e-2)
    rot, t, P = ba.perturb(S["rot"], S["t"], S["P"], seed=seed + 1, deg=5.0, rel=0.05)
    group_of = np.arange(8) % G
    focal = np.random.default_rng(seed + 2).uniform(0.8, 1.25, G)
    pr = bg.GroupProblem(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], group_of, G, fix)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    return S, pr, (Rcw, tcw, P.T.copy()), focal


@FIX
def test_the_contracted_system_is_the_schur_complement_of_the_shared_normal_equations(fix):
    """E^T S_7 E + mu diag(D_c) (S_7: the 7-column reduced system with the members' focal diagonal undamped) equals the Schur complement of
    (J_7 E)^T (J_7 E) + mu D to rounding: the landmark elimination commutes with E"""
    S, pr, (Rcw, tcw, X), focal = _small(fix)
    F, r, J, J7 = pr.shared(Rcw, tcw, X, focal)
    for mu in (1e-4, 1.0, 1e3):
        q = bg.reduced(pr, J, J7, J.T @ r, mu)
        Ec = pr.E[:pr.cd * pr.n, :pr.ncam]
        Sc = (Ec.T @ q["S7"] @ Ec).toarray()
        gi = pr.cp * pr.n + np.arange(pr.G)
        Sc[gi, gi] += mu * q["Dc"]
        Sd = q["S"].toarray()
        assert np.abs(Sc - Sd).max() <= 1e-12 * np.abs(Sd).max()
        assert np.allclose(q["Dc"], np.clip(np.bincount(pr.group_of, weights=(J7.T @ J7).diagonal()[pr.cd * np.arange(pr.n) + pr.cp]), 1e-6, 1e32),
                           rtol=1e-14, atol=0)


@FIX
def test_the_numerical_gradient_agrees_with_the_shared_jacobian(fix):
    S, pr, (Rcw, tcw, X), focal = _small(fix)
    F, r, J, _ = pr.shared(Rcw, tcw, X, focal)
    g = J.T @ r
    nd = pr.ncam + 3 * pr.m
    h = 1e-6
    num = np.zeros(nd)
    for j in range(nd):
        d = np.zeros(nd); d[j] = h
        num[j] = (pr.cost_g(*pr.plus_g(Rcw, tcw, X, focal, d)) - pr.cost_g(*pr.plus_g(Rcw, tcw, X, focal, -d))) / (2 * h)
    assert np.abs(num - g).max() <= 1e-6 * np.abs(g).max()      # truncation h^2 |f'''| and rounding eps F / h, both ~1e-10 relative


@FIX
def test_singleton_groups_reproduce_the_per_image_trace(fix):
    S = ba.ring_scene(n_cams=10, n_pts=60, seed=0, noise=1e-2)
    ratio = bf.focal_ratios(10, 5)
    S = bf.scale_observations(S, ratio)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=2.0, rel=0.01)
    args = (S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0)
    perm = np.random.default_rng(2).permutation(10)
    free = np.ones(10, dtype=bool); free[3] = False
    _, _, _, g1, i1 = bf.lm(*args, focal_free=free, fix_rotations=fix, max_iters=12)
    fg = np.ones(10, dtype=bool); fg[perm[3]] = False
    _, _, _, g2, i2 = bg.lm(*args, perm, focal=np.ones(10), focal_free=fg, fix_rotations=fix, max_iters=12)
    assert np.array_equal(i1["trace"][:, 3], i2["trace"][:, 3]) and i1["trace"].shape == i2["trace"].shape
    assert np.allclose(i1["trace"][:, :3], i2["trace"][:, :3], rtol=1e-9, atol=0)
    assert np.allclose(g1, g2[perm], rtol=1e-9, atol=0) and g2[perm[3]] == 1.0


def test_one_true_ratio_per_group_is_recovered():
    S0 = ba.ring_scene(n_cams=18, n_pts=150, seed=0, noise=0)
    group_of = np.arange(18) % 3
    ratio = np.array([0.85, 1.0, 1.2])
    S = bf.scale_observations(S0, ratio[group_of])
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=1.0, rel=0.005)
    for eta in (None, 0.1):
        _, _, _, g, info = bg.lm(S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0, group_of, focal=np.ones(3), eta=eta)
        print(f"eta {eta}: cost {info['final_cost']:.3e} after {info['iters']} iterations, ratio error {np.abs(g - ratio).max():.3e}")
        assert np.abs(g - ratio).max() <= 1e-6 and info["final_cost"] <= 1e-12


def test_held_and_unused_groups_come_back_bit_identical():
    S0 = ba.ring_scene(n_cams=18, n_pts=150, seed=0, noise=0)
    group_of = np.arange(18) % 3
    ratio = np.array([0.85, 1.0, 1.2])
    S = bf.scale_observations(S0, ratio[group_of])
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=1.0, rel=0.005)
    f0 = np.array([1.0, 1.0, 1.2, 0.777])                  # group 2 held at the truth, group 3 empty
    free = np.array([1, 1, 0, 1], dtype=bool)
    _, _, _, g, info = bg.lm(S["cam"], S["lm"], S["p"], S["w"], rot0, t0, P0, group_of, focal=f0, focal_free=free)
    assert g[2:].tobytes() == f0[2:].tobytes() and np.abs(g[:3] - ratio).max() <= 1e-6


@FIX
@pytest.mark.parametrize("name", gs.CASES)
def test_restatement_agrees_with_longdouble_and_m_is_spd(name, fix):
    """the MAX_E_REF rule of xm_ba_stages on every case the GPU stage test uses; M = blockdiag(pose blocks, F) is symmetric positive definite"""
    c = gs.case(name, fix)
    for mu in c["mus"]:
        kw = gs.stage_args(c, mu)
        E = gs.exact_stages(c["S"], **kw)
        e_ref = gs.reference_errors(c["S"], E, gs.KEYS, c["G"], **kw)
        assert max(e_ref.values()) <= st.MAX_E_REF, e_ref
        X = E["_E"]
        if X.F.ndim == 2:                                  # G <= 16: the exact focal block
            Ff = np.asarray(X.F, dtype=np.float64)
            assert c["G"] <= 16 and np.linalg.eigvalsh(0.5 * (Ff + Ff.T)).min() > 0
        else:
            assert c["G"] > 16 and (X.F > 0).all()
        for Pi in np.asarray(X.Pinv, dtype=np.float64):
            assert np.abs(Pi - Pi.T).max() <= 1e-12 * np.abs(Pi).max() and np.linalg.eigvalsh(0.5 * (Pi + Pi.T)).min() > 0
    if name == "clamp_member":
        uff = np.zeros(c["S"]["n"])
        np.add.at(uff, X.E7.cam, np.asarray(np.sum(X.E7.Jc[:, :, -1] ** 2, axis=1), dtype=np.float64))
        assert 0 < uff[7] < 1e-6 and uff[np.arange(c["S"]["n"]) != 7].min() > 1e-6
    if name == "sizes":
        assert tuple(np.bincount(c["group_of"])) == gs.SIZES


@FIX
@pytest.mark.parametrize("name", ["clamp_member", "unused_member"])
def test_the_bound_rejects_the_sum_of_the_members_clamped_terms(name, fix):
    """the trap of the model: summing mu clamp(U_ff,i) over the members is not mu clamp(sum U_ff,i) when a member's clamp is active"""
    c = gs.case(name, fix)
    mu = c["mus"][0]
    kw = gs.stage_args(c, mu)
    E = gs.exact_stages(c["S"], **kw)
    e_ref = gs.reference_errors(c["S"], E, gs.KEYS, c["G"], **kw)
    assert not gs.compare("sound", c["S"], gs.f64_stages(c["S"], **kw), E, e_ref, gs.KEYS, c["G"], who="f64")
    bad = gs.compare("member_clamp", c["S"], gs.f64_stages(c["S"], damage=("member_clamp",), **kw), E, e_ref, gs.KEYS, c["G"], who="f64")
    assert {"D", "F"} <= {k for k, *_ in bad}, bad
