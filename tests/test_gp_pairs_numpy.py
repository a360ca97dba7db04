"""CPU tests of the restatement tests/xm_gp_pairs_numpy.py (the reference of tests/test_gpu_gp_pairs*.py).

1. Its closed-form elimination -- reduced camera system S, right-hand side b, back-substituted dP, ds, d sigma -- against a brute-force
   computation: the full dense Jacobian over (c, P, s, sigma) in longdouble, the damped normal equations H = J^T J + mu clamp(diag) and a
   dense Schur complement onto the cameras by Gauss-Jordan inverses (xm_ba_exact.gj_inverse).  Agreement to 1e-10 relative (per array,
   against its largest entry), for every constraint type, mixed `calibrated`, a frozen sigma and fixed centres.
2. Its LM on the scenes of tests/test_gpu_gp_pairs.py with the same seeds converges: the reference alone gets there.

Start points.  From the reference's random start 100 U(-1, 1) the pair terms alone mostly do NOT converge to the scene: a scipy
least-squares trial of ONLY_CAMERAS failed in 11 of 12 runs on rings of 8 to 70 cameras; from the truth moved by up to half the ring's
radius it converged every time, with a largest centre error after similarity alignment of 4 to 6e-3 for 1e-3 noise on tau.  So the pair
tests start from a perturbed truth (xm_gp_pairs_numpy.perturbed_start) and a random start is used with only_points alone."""
import numpy as np
import pytest

import xm_ba_exact as ex
import xm_ba_numpy as ba
import xm_gp_numpy as gp
import xm_gp_pairs_numpy as gpp

LD = gpp.LD
TOL = 1e-10


def small_scene(n, seed):
    S = ba.ring_scene(n_cams=n, n_pts=14, seed=seed, noise=2e-3)
    pi, pj = gpp.all_pairs(n)
    trel = gpp.relative_translations(S, pi, pj, noise=1e-3, seed=seed + 1)
    valid = np.ones(pi.size, dtype=np.uint8)
    valid[1::5] = 0
    return S, (pi, pj, trel, valid)


def point(S, pairs, seed):
    rng = np.random.default_rng(seed)
    t = S["t"] + 0.05 * rng.standard_normal(S["t"].shape)
    P = S["P"] + 0.05 * rng.standard_normal(S["P"].shape)
    depth = np.linalg.norm(S["P"][:, S["lm"]] - S["t"][:, S["cam"]], axis=0)
    dist = np.linalg.norm(S["t"][:, pairs[1]] - S["t"][:, pairs[0]], axis=0)
    return t, P, (1.0 / depth) * rng.uniform(0.8, 1.25, depth.size), (1.0 / dist) * rng.uniform(0.8, 1.25, dist.size)


def dense_jacobian(pr, B, Bp):
    """(3k + 3M) x (3n + 3m + k + M) in longdouble, entry by entry from the residual's definition: d r / d c = s I, d r / d P = -s I,
    d r / d s = -v, each times sqrt(w); a frozen scale's column is zero"""
    n, m, k, M = pr.n, pr.m, pr.k, pr.M
    J = np.zeros((3 * k + 3 * M, 3 * n + 3 * m + k + M), dtype=LD)
    for e in range(k):
        for a in range(3):
            J[3 * e + a, 3 * pr.cam[e] + a] = B["jc"][e]
            J[3 * e + a, 3 * n + 3 * pr.lm[e] + a] = -B["jc"][e]
            J[3 * e + a, 3 * n + 3 * m + e] = B["Js"][e, a]
    for q in range(M):
        for a in range(3):
            J[3 * k + 3 * q + a, 3 * pr.ci[q] + a] = Bp["jc"][q]
            J[3 * k + 3 * q + a, 3 * pr.cj[q] + a] = -Bp["jc"][q]
            J[3 * k + 3 * q + a, 3 * n + 3 * m + k + q] = Bp["Js"][q, a]
    return J


def rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    den = np.abs(b).max(initial=0)
    return float(np.abs(a - b).max(initial=0) / den) if den > 0 else float(np.abs(a).max(initial=0))


CASES = [(c, n, cal, fz) for c, n, cal, fz in (("only_points", 5, False, False), ("only_points", 6, True, False), ("only_cameras", 8, False, False),
                                               ("only_cameras", 6, False, True), ("points_and_cameras", 7, True, False),
                                               ("points_and_cameras", 5, False, True), ("points_and_cameras_balanced", 6, True, False),
                                               ("points_and_cameras_balanced", 8, False, True), ("fixed", 6, True, False))]


@pytest.mark.parametrize("constraint,n,mixed,freeze", CASES)
@pytest.mark.parametrize("mu", [1e-4, 3.0])
def test_closed_form_elimination_equals_the_dense_schur_complement(constraint, n, mixed, freeze, mu):
    S, pairs = small_scene(n, seed=10 + n)
    fix = constraint == "fixed"
    cal = (np.arange(n) % 3 != 1) if mixed else None
    pr = gpp.Problem(S["cam"], S["lm"], S["p"], S["w"], S["rot"], n, S["m"], pairs, "only_points" if fix else constraint, cal, 2.5, fix,
                     loss="huber", a=0.05, dtype=LD)
    t, P, s, sg = point(S, pairs, 3)
    if freeze:                                   # two scales at the bound: one pair too far apart (outward gradient: frozen), one too close
        q0, q1 = pr.pidx[0], pr.pidx[1]
        sg[[q0, q1]] = gpp.S_MIN
        t[:, pairs[1][q0]] = t[:, pairs[0][q0]] - 3.0 * (S["t"][:, pairs[1][q0]] - S["t"][:, pairs[0][q0]])   # c_j - c_i against tau
    out = gpp.stages(pr, t, P, s, sg, mu)
    if freeze:
        fz = out["pfrozen"][pr.pidx]
        assert fz[0] == 1 and fz[1] == 0
    B, Bp = out["_B"], out["_Bp"]
    J = dense_jacobian(pr, B, Bp)
    r = np.concatenate([B["r"].reshape(-1), Bp["r"].reshape(-1)])
    H = J.T @ J
    H = H + np.diag(LD(mu) * ex.clipd(np.diag(H)))
    g = J.T @ r
    nc = 3 * n
    if fix:
        d_o = -ex.gj_inverse(H[nc:, nc:]) @ g[nc:]
        dc = np.zeros(nc, dtype=LD)
    else:
        Hoo_inv = ex.gj_inverse(H[nc:, nc:])
        Sd = H[:nc, :nc] - H[:nc, nc:] @ Hoo_inv @ H[nc:, :nc]
        bd = -(g[:nc] - H[:nc, nc:] @ Hoo_inv @ g[nc:])
        assert rel(out["S"], Sd) <= TOL and rel(out["b"].reshape(-1), bd) <= TOL
        d = -ex.gj_inverse(H) @ g
        dc, d_o = d[:nc], d[nc:]
    step = gpp.stages(pr, t, P, s, sg, mu, dc=dc)
    m, k = S["m"], pr.k
    assert rel(step["dP"].reshape(-1), d_o[:3 * m]) <= TOL
    assert rel(step["ds"][pr.idx], d_o[3 * m:3 * m + k]) <= TOL
    assert rel(step["dsigma"][pr.pidx], d_o[3 * m + k:]) <= TOL
    if pr.M:                                     # a frozen sigma does not move; the model of the full step is the sum of the two shares
        assert np.all(step["dsigma"][pr.pidx][Bp["frozen"]] == 0)
    Jd = J @ np.concatenate([dc, d_o])
    assert abs(float(step["model"] + step["pmodel"]) - float(r @ Jd + 0.5 * (Jd @ Jd))) <= TOL * abs(float(r @ Jd))


def test_weights_and_refusals():
    S, pairs = small_scene(6, seed=3)
    args = (S["cam"], S["lm"], S["p"], S["w"], S["rot"], 6, S["m"])
    cal = np.array([1, 0, 1, 1, 0, 1])
    pr = gpp.Problem(*args, pairs, "points_and_cameras_balanced", cal, 2.5)
    assert pr.weight_scale_pt == 2.5 * pr.M / S["m"] and pr.M == int(pairs[3].sum())
    assert np.array_equal(pr.ae, np.where(cal[pr.cam] != 0, 1.0, 0.5) * pr.weight_scale_pt)
    assert gpp.Problem(*args, pairs, "points_and_cameras", cal, 2.5).weight_scale_pt == 1.0
    assert gpp.Problem(*args, pairs, "only_cameras").k == 0
    none = (pairs[0], pairs[1], pairs[2], np.zeros_like(pairs[3]))
    for kw in (dict(pairs=none, constraint="only_cameras"), dict(pairs=None, constraint="points_and_cameras"),
               dict(pairs=pairs, constraint="only_cameras", fix_centres=True), dict(pairs=(pairs[0], pairs[0], pairs[2]), constraint="only_points"),
               dict(pairs=(pairs[0], pairs[1] + 6, pairs[2]), constraint="only_points")):
        with pytest.raises(ValueError):
            gpp.Problem(*args, **kw)


# ------------------------------------------------------------------------------------------------ the scenes of tests/test_gpu_gp_pairs.py
def ring20():
    S = ba.ring_scene(n_cams=20, n_pts=120, seed=20, noise=2e-3)
    S = gpp.strip_long_tracks(S, STRIPPED)
    pi, pj = gpp.all_pairs(20)
    return S, (pi, pj, gpp.relative_translations(S, pi, pj, noise=1e-3, seed=21))


STRIPPED = (1, 4, 8, 11, 15, 18)
OPTS = dict(function_tol=1e-10)


def test_only_points_leaves_the_stripped_cameras_and_the_mixed_type_positions_all():
    S, pairs = ring20()
    t0, P0 = gpp.perturbed_start(S, 22)
    obs = (S["cam"], S["lm"], S["p"], S["w"])
    t, _, info = gpp.lm(*obs, S["rot"], t0, P0, **OPTS)
    assert info["status"] in (1, 2, 3)
    assert t[:, list(STRIPPED)].tobytes() == np.ascontiguousarray(t0[:, list(STRIPPED)]).tobytes()
    t, _, info = gpp.lm(*obs, S["rot"], t0, P0, pairs=pairs, constraint="points_and_cameras", **OPTS)
    err = gpp.aligned_centre_error(S, t)
    print(f"points_and_cameras: {info['iters']} iterations, status {info['status']}, aligned centre error {err:.3e}")
    assert info["status"] in (1, 2, 3) and err < 2e-2 and info["sigma"].min() > gpp.S_MIN


@pytest.mark.parametrize("constraint", gpp.CONSTRAINTS[1:])
def test_the_reference_converges_from_the_perturbed_start(constraint):
    S, pairs = ring20()
    t0, P0 = gpp.perturbed_start(S, 22)
    t, P, info = gpp.lm(S["cam"], S["lm"], S["p"], S["w"], S["rot"], t0, P0, pairs=pairs, constraint=constraint, **OPTS)
    err = gpp.aligned_centre_error(S, t)
    print(f"{constraint}: {info['iters']} iterations ({info['accepted']} accepted), status {info['status']}, cost {info['initial_cost']:.3e} -> "
          f"{info['final_cost']:.3e}, aligned centre error {err:.3e}")
    assert info["status"] in (1, 2, 3) and err < 2e-2
    if constraint == "only_cameras":             # then the fixed-centre pass: the centres stay, the points land
        assert P.tobytes() == np.ascontiguousarray(P0).tobytes() and np.all(info["scales"] == -1)
        t2, P2, i2 = gpp.lm(S["cam"], S["lm"], S["p"], S["w"], S["rot"], t, P0, fix_centres=True, **OPTS)
        assert t2.tobytes() == t.tobytes() and i2["status"] in (1, 2, 3)
        used = np.bincount(S["lm"], minlength=S["m"]) >= 3
        A = np.concatenate([t2, P2[:, used]], axis=1); Bm = np.concatenate([S["t"], S["P"][:, used]], axis=1)
        perr = float(np.sqrt(np.sum((gp.align(A, Bm) - Bm) ** 2, axis=0)).max())
        print(f"fixed-centre pass: {i2['iters']} iterations, point error {perr:.3e}")
        assert perr < 5e-2
