"""The restatement of the robust rotation averaging (tests/xm_rotavg_numpy.py) against itself: the two maps of rules 3 and 4, (a) against (b),
the explicit matrix against the Laplacian form, what IRLS does to outliers, the stops and the refusals.  No device."""
import numpy as np
import pytest

import xm_rotavg_numpy as rn

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


def _axes(rng, count):
    fixed = [s * np.eye(3)[k] for k in range(3) for s in (1.0, -1.0)]
    rnd = [u / np.linalg.norm(u) for u in rng.standard_normal((count, 3))]
    return fixed + rnd


def test_exp_log_are_inverse_on_every_branch():
    """Log(Exp(a)) = a for |a| < pi.  Each of the two maps is a dozen rounded operations whose errors stay relative to |a| (the quaternion
    form has no acos near 1): 16 eps |a| is asked for; all four quaternion branches and w < 0 must have been taken"""
    rng = np.random.default_rng(0)
    seen = set()
    for angle in (1e-9, 1e-3, 0.5, 1.5, 2.2, 2.6, 3.0, np.pi - 1e-3):
        for u in _axes(rng, 60):
            a = angle * u
            R = rn.aa_to_rot(a)
            q, branch = rn.rot_to_quat(R)
            seen.add((branch, bool(q[3] < 0)))
            assert np.max(np.abs(rn.rot_to_aa(R) - a)) <= 16 * EPS * angle
            assert np.max(np.abs(R @ R.T - np.eye(3))) <= 16 * EPS
            Rl = rn.aa_to_rot(a.astype(LD), LD)
            assert np.max(np.abs(R - Rl)) <= 8 * EPS
    assert {b for b, _ in seen} == {0, 1, 2, 3}
    assert {b for b, neg in seen if neg} == {1, 2, 3}          # (the trace branch has w = sqrt(.) / 2 > 0)


def test_exp_log_at_zero_and_on_the_first_order_branch():
    assert np.array_equal(rn.aa_to_rot(np.zeros(3)), np.eye(3))
    assert np.array_equal(rn.rot_to_aa(np.eye(3)), np.zeros(3))
    rng = np.random.default_rng(1)
    for u in _axes(rng, 20):
        a = 1e-13 * u
        R = rn.aa_to_rot(a)
        assert np.array_equal(R, np.array([[1.0, -a[2], a[1]], [a[2], 1.0, -a[0]], [-a[1], a[0], 1.0]]))   # rigid3d.cc:59-69
        assert np.max(np.abs(rn.rot_to_aa(R) - a)) <= 8 * EPS * 1e-13
    a = np.array([1e-12, 0.0, 0.0])                            # at the threshold: still first order (the test is norm > EPS)
    assert rn.aa_to_rot(a)[0, 0] == 1.0 and rn.aa_to_rot(a)[2, 1] == 1e-12
    b = np.array([2e-12, 0.0, 0.0])                            # above it: Rodrigues
    assert rn.aa_to_rot(b)[2, 1] == np.sin(2e-12)


def test_batch_maps_equal_the_scalar_ones():
    rng = np.random.default_rng(2)
    a = np.concatenate([rng.standard_normal((50, 3)), 1e-13 * rng.standard_normal((5, 3)), np.zeros((1, 3))])
    R = rn.exp_batch(a)
    assert np.array_equal(R, np.stack([rn.aa_to_rot(v) for v in a]))
    A, B = R[:28], R[28:]
    assert np.array_equal(rn.mul_batch(A, B), np.stack([rn.mul3(x, y) for x, y in zip(A, B)]))
    big = np.stack([rn.aa_to_rot(angle * u) for angle in (0.0, 1e-13, 0.7, 2.3, 2.9, np.pi - 1e-3) for u in _axes(rng, 10)])
    assert {rn.rot_to_quat(M)[1] for M in big} == {0, 1, 2, 3}
    assert np.array_equal(rn.log_batch(big), np.stack([rn.rot_to_aa(M) for M in big]))


def test_stages_equal_the_explicit_matrix():
    """stages_sequential forms A^T W r and (A^T W A) x row by row: the same numbers as with the matrix of :205-270"""
    g = rn.make_graph(12, 40, 3, 1.0, 0.2)
    rng = np.random.default_rng(4)
    aa = np.stack([rn.rot_to_aa(R) for R in g["rot0"]]) + 0.05 * rng.standard_normal((12, 3))
    x = 0.05 * rng.standard_normal((12, 3))
    s = rn.stages_sequential(g, aa, x, fixed_image=3)
    p = rn.problem(g, fixed_image=3)
    A = rn.explicit_A(p)
    wrow = np.concatenate([np.repeat(s["weight"][p["k"]], 3), np.ones(3)])
    r = np.concatenate([s["residual"][p["k"]].reshape(-1), s["gauge"]])
    S = (A.T * wrow) @ A
    assert np.allclose(s["rhs"].reshape(-1), (A.T * wrow) @ r, rtol=1e-12, atol=1e-13)
    assert np.allclose(s["product"].reshape(-1), S @ x.reshape(-1), rtol=1e-12, atol=1e-13)
    assert np.allclose(s["diagonal"], np.diag(S)[::3], rtol=1e-13, atol=0.0)
    assert np.allclose(S, rn.laplacian_normal(p, s["weight"][p["k"]]), rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("n,npairs,seed,outliers", [(20, 100, 1, 0.15), (20, 100, 1, 0.25), (60, 400, 1, 0.2)])
def test_sequential_equals_contract_within_the_pcg_tolerance(n, npairs, seed, outliers):
    """(b) leaves a relative residual of 1e-12 in every solve where (a) solves exactly; with the preconditioned system's condition number
    below 1e3 on these graphs the steps, and with them the rotations, agree to 1e-9"""
    g = rn.make_graph(n, npairs, seed, 1.0, outliers)
    a, b = rn.irls_sequential(g), rn.irls_contract(g)
    assert a["iters"] == b["iters"] and a["stop"] == b["stop"] == rn.STOP_STEP and b["pcg_capped"] == 0
    assert np.max(np.abs(a["step_trace"] - b["step_trace"])) <= 1e-9
    for k in ("rot", "angle_axis", "residual"):
        assert np.max(np.abs(a[k] - b[k])) <= 1e-9
    assert np.max(np.abs(a["weight"] - b["weight"]) / a["weight"].max()) <= 1e-9


def test_explicit_matrix_gives_the_laplacian_form():
    g = rn.make_graph(12, 40, 3, 1.0, 0.2)
    g["registered"] = np.ones(12, dtype=np.uint8)
    p = rn.problem(g, fixed_image=4)
    rng = np.random.default_rng(3)
    w = rng.uniform(0.01, 130.0, p["k"].size)
    A = rn.explicit_A(p)
    wrow = np.concatenate([np.repeat(w, 3), np.ones(3)])
    S = (A.T * wrow) @ A
    assert np.allclose(S, rn.laplacian_normal(p, w), rtol=1e-13, atol=0.0)
    assert S[3 * 4, 3 * 4] == pytest.approx(1.0 + w[(p["ca"] == 4) | (p["cb"] == 4)].sum(), rel=1e-13)
    # the right-hand side of rule 8 from the same matrix
    r = rng.standard_normal(3 * p["k"].size + 3)
    b = (A.T * wrow) @ r
    ref = np.zeros((12, 3))
    for m in range(p["k"].size):
        ref[p["cb"][m]] += w[m] * r[3 * m:3 * m + 3]; ref[p["ca"][m]] -= w[m] * r[3 * m:3 * m + 3]
    ref[4] += r[-3:]
    assert np.allclose(b.reshape(12, 3), ref, rtol=1e-12, atol=1e-12)


def test_noise_free_start_is_a_fixed_point():
    g = rn.make_graph(20, 100, 5, 0.0, 0.0)
    for run in (rn.irls_sequential, rn.irls_contract):
        r = run(g)
        assert r["iters"] == 1 and r["stop"] == rn.STOP_STEP and r["step_trace"][0] < 1e-12
        assert np.max(np.abs(r["rot"] - g["rot0"])) < 1e-12


@pytest.mark.parametrize("seed,outliers", [(1, 0.15), (1, 0.25)])
def test_outliers_lose_their_weight(seed, outliers):
    g = rn.make_graph(20, 100, seed, 1.0, outliers)
    assert g["wrong"].sum() == round(outliers * 81)
    a = rn.irls_sequential(g)
    before, after = np.median(rn.errors_deg(g["rot0"], g["truth"])), np.median(rn.errors_deg(a["rot"], g["truth"]))
    print(f"median rotation error against the truth: start {before:.3f} deg, after {a['iters']} IRLS iterations {after:.3f} deg; "
          f"largest weight of a wrong pair {a['weight'][g['wrong']].max():.3g}, smallest of a good pair {a['weight'][~g['wrong']].min():.3g}; "
          f"steps {np.array2string(a['step_trace'], precision=5)}")
    assert after <= 0.5 * before
    assert (a["weight"][g["wrong"]] < 1.0).all() and (a["weight"][~g["wrong"]] > 10.0).all()
    assert a["stop"] == rn.STOP_STEP and (np.abs(a["step_trace"] - 1e-3) > 0.01 * 1e-3).all()     # the seed keeps every step clear of the threshold


def _identity_graph():
    return dict(rot0=np.tile(np.eye(3), (4, 1, 1)), pi=np.array([0, 1, 2, 0], dtype=np.int32), pj=np.array([1, 2, 3, 3], dtype=np.int32),
                Rrel=np.tile(np.eye(3), (4, 1, 1)), registered=None, valid_in=None)


def test_half_norm_with_a_zero_residual_stops():
    g = _identity_graph()
    for run in (rn.irls_sequential, rn.irls_contract):
        r = run(g, weight_type=rn.HALF_NORM)
        assert r["stop"] == rn.STOP_NONFINITE and r["iters"] == 0 and not r["weight"].any()
        assert np.array_equal(r["rot"], g["rot0"]) and not r["residual"].any()
        ok = run(g)                                  # Geman-McClure is finite there: w = 1 / sigma^2
        assert ok["stop"] == rn.STOP_STEP and ok["iters"] == 1 and ok["weight"] == pytest.approx(1.0 / np.radians(5.0) ** 2, rel=1e-14)
    h = rn.make_graph(10, 30, 2, 1.0, 0.1)
    r = rn.irls_sequential(h, weight_type=rn.HALF_NORM, max_iters=5)
    assert r["stop"] in (rn.STOP_STEP, rn.STOP_ITERATIONS) and np.isfinite(r["weight"]).all()


def test_refusals_and_no_pair():
    g = rn.make_graph(8, 16, 4, 1.0, 0.0)
    two = dict(g, valid_in=((g["pi"] < 4) == (g["pj"] < 4)).astype(np.uint8))          # cameras 0 .. 3 and 4 .. 7 fall apart
    with pytest.raises(rn.Refused):
        rn.irls_sequential(two)
    reg = np.ones(8, dtype=np.uint8); reg[5] = 0
    with pytest.raises(rn.Refused):
        rn.irls_sequential(dict(g, registered=reg), fixed_image=5)
    assert rn.irls_sequential(dict(g, registered=reg), fixed_image=6)["fixed"] == 6
    assert rn.irls_sequential(dict(g, registered=reg))["fixed"] == 0
    for bad in (dict(g, pi=g["pj"]), dict(g, pi=np.where(np.arange(16) == 3, 8, g["pi"]).astype(np.int32))):
        with pytest.raises(rn.Refused):
            rn.irls_contract(bad)
    none = rn.irls_sequential(dict(g, valid_in=np.zeros(16, dtype=np.uint8)))
    assert none["stop"] == rn.STOP_NOTHING and none["iters"] == 0 and np.array_equal(none["rot"], g["rot0"]) and not none["weight"].any()


def test_star_ring_and_simple2_generators():
    s = rn.star_ring(300, 7, 1.0, 0.1)
    p = rn.problem(s)
    inc = np.bincount(np.concatenate([p["ca"], p["cb"]]))
    assert inc[0] == 300 and (inc[1:] == 5).all() and s["wrong"].sum() == 60
    assert np.bincount(np.concatenate([rn.problem(rn.star(65, 1))[k] for k in ("ca", "cb")])).tolist() == [65] + [1] * 65
    g = rn.simple2_graph()
    p = rn.problem(g)
    assert p["img"].size == 93 and p["k"].size == int(g["valid_in"].sum())
    b = rn.irls_contract(g)
    before, after = np.median(rn.errors_deg(g["rot0"], g["truth"], p["img"])), np.median(rn.errors_deg(b["rot"], g["truth"], p["img"]))
    print(f"SIMPLE2-derived: {p['k'].size} pairs of {p['img'].size} images, median error {before:.3f} -> {after:.3f} deg in {b['iters']} iterations")
    assert b["stop"] == rn.STOP_STEP and after < before


def test_chain_caps_the_pcg():
    """a chain of 600 cameras: both solves of two IRLS iterations run into the PCG's cap.  The relative residual there is orders of magnitude
    above the tolerance 1e-12, so rounding cannot turn a capped solve into one that converged (tests/test_gpu_rotavg.py asks the device for
    the same counts)"""
    b = rn.irls_contract(rn.chain(600, 3), max_iters=2)
    print(f"chain of 600: relative residual of the two capped solves {b['pcg_relres'][0]:.3e}, {b['pcg_relres'][1]:.3e}")
    assert b["iters"] == 2 and b["pcg_iters"] == 2 * rn.PCG_CAP == 1000 and b["pcg_capped"] == 2 and b["stop"] == rn.STOP_ITERATIONS
    assert min(b["pcg_relres"]) > 1e-8
