"""GPU tests of the dense Schur solver of xm_ctx_bundle_adjust (XM_BA_DENSE_SCHUR, linear_solver="dense_schur") and of xm_spd_solve
(xm-code_amd/csrc/xm_ba.hip, xm_dense_la.hip) against the exact-solve numpy restatements xm_ba_numpy.lm and xm_ba_loss_numpy.lm."""
import ctypes as C

import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_ba_loss_numpy as rl

pytestmark = pytest.mark.gpu

ERR_ARG = -2
DENSE = dict(linear_solver="dense_schur")


def _ctx(xmamd, S, **kw):
    return xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"], **kw)


def _obs(S, w=None):
    return S["cam"], S["lm"], S["p"], S["w"] if w is None else w


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _bits(*xs):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in xs)


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 200, 257, 1000])
def test_spd_solve_matches_numpy(xmamd, n):
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    A = M @ M.T / n + np.eye(n)                       # eigenvalues in [1, ~5]
    for k in (1, 3):
        B = rng.standard_normal((n, k))
        ref = np.linalg.solve(A, B)
        junk = A.copy()
        junk[np.triu_indices(n, 1)] = np.nan               # only the lower triangle is read
        X = xmamd.spd_solve(junk, B)
        err = _rel(X, ref)
        print(f"n {n} k {k}: relative error {err:.2e}")
        assert X.shape == (n, k) and err <= 1e-12
    x1 = xmamd.spd_solve(A, B[:, 0])
    assert x1.shape == (n,) and _rel(x1, ref[:, 0]) <= 1e-12


def test_spd_solve_refuses_an_indefinite_matrix(xmamd):
    n = 130
    A = np.eye(n)
    A[100, 100] = -1.0                                  # the pivot of the second 64-row block's 37th row
    with pytest.raises(xmamd.XmError, match="error -2"):
        xmamd.spd_solve(A, np.ones(n))
    assert _rel(xmamd.spd_solve(np.eye(n) * 2.0, np.ones(n)), np.full(n, 0.5)) <= 1e-15   # the library is still usable


def test_trace_follows_the_numpy_lm_at_the_default_eta(xmamd):
    # the scene of test_gpu_ba.py::test_trace_follows_the_numpy_lm, which needs eta = 1e-12 for the PCG: the exact solve needs no eta
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=0.05)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=21, deg=40.0, rel=0.4)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, function_tol=1e-12, max_iters=10, trace=20, **DENSE)
    ctx.close()
    _, _, _, ref = ba.lm(*_obs(S), rot0, t0, P0, function_tol=1e-12, max_iters=10)
    g, gr = info["trace"], ref["trace"]
    np.set_printoptions(linewidth=200)
    print("GPU trace\n", g, "\nnumpy trace\n", gr)
    assert g.shape[0] == gr.shape[0] == 10 and info["pcg_iters"] == 0
    assert np.array_equal(g[:, 3], gr[:, 3])
    assert np.allclose(g[:, 0], gr[:, 0], rtol=1e-9, atol=0) and np.allclose(g[:, 1], gr[:, 1], rtol=1e-9, atol=0)
    assert np.allclose(g[:, 2], gr[:, 2], rtol=1e-6, atol=0)
    assert np.all(g[:, 4] == 0)
    assert np.all((g[:, 5] >= 0) & (g[:, 5] <= 1e-8))             # |b - S dc| / |b| by the matrix-free product


@pytest.mark.parametrize("n_cams", [150, 1000])
def test_sequential_captures_reach_the_numpy_optimum(xmamd, n_cams):
    S = ba.sequential_scene(n_cams=n_cams, seed=62, noise=1e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=63, deg=0.5, rel=2e-4)
    opts = dict(function_tol=1e-8, max_iters=30)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, trace=40, **opts, **DENSE)
    it = None
    if n_cams == 1000:
        _, _, _, it = ctx.bundle_adjust(rot0, t0, P0, eta=1e-6, trace=40, **opts)
    ctx.close()
    _, _, _, ref = ba.lm(*_obs(S), rot0, t0, P0, **opts)
    print(f"{n_cams} cameras: dense {info['final_cost']:.15e} ({info['status_name']}, {info['iters']} it, {info['seconds']:.2f} s), numpy "
          f"{ref['final_cost']:.15e} ({ref['iters']} it); residuals of the dense solves {info['trace'][:, 5]}")
    assert info["status"] == ref["status"] and info["iters"] == ref["iters"]
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
    assert np.array_equal(info["trace"][:, 3], ref["trace"][:, 3])
    if it is not None:
        print(f"iterative at eta 1e-6: {it['final_cost']:.15e} ({it['iters']} it, {it['seconds']:.2f} s), PCG iterations per step {it['trace'][:, 4]}")
        assert it["trace"][:, 4].max() == 500                          # a step at the PCG's cap


def test_fixed_rotations_match_numpy(xmamd):
    S = ba.ring_scene(n_cams=16, n_pts=150, seed=40, noise=2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=41)
    opts = dict(function_tol=1e-10, max_iters=30)
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0, fix_rotations=True, **opts, **DENSE)
    ctx.close()
    _, t_r, P_r, ref = ba.lm(*_obs(S), rot0, t0, P0, fix_rotations=True, **opts)
    print(f"fixed rotations: dense {info['final_cost']:.15e} ({info['iters']} it), numpy {ref['final_cost']:.15e} ({ref['iters']} it)")
    assert rot.tobytes() == np.asfortranarray(rot0).tobytes()
    assert info["status"] == ref["status"] and info["iters"] == ref["iters"]
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
    assert _rel(t, t_r) <= 1e-7 and _rel(P, P_r) <= 1e-7


def test_huber_with_nonmonotonic_steps_follows_the_numpy_evaluator(xmamd):
    S, _ = rl.outlier_scene(n_cams=16, n_pts=150, seed=215, noise=5e-3, frac_out=0.1, out_size=0.5)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=216, deg=40.0, rel=0.4)
    opts = dict(function_tol=1e-10, max_iters=25)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, loss="huber", loss_scale=0.02, nonmonotonic=True, trace=40, **opts, **DENSE)
    ctx.close()
    _, _, _, ref = rl.lm(*_obs(S), rot0, t0, P0, loss="huber", a=0.02, nonmonotonic=True, **opts)
    g, gr = info["trace"], ref["trace"]
    print("GPU trace\n", g, "\nnumpy trace\n", gr)
    assert np.array_equal(g[:, 3], gr[:, 3])
    assert info["status"] == ref["status"] and info["iters"] == ref["iters"]
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]


def test_duplicates_heavy_landmarks_masks_and_an_unused_camera(xmamd):
    S = ba.ring_scene(n_cams=72, n_pts=120, seed=60, noise=2e-3, frac=0.93)
    n, m = S["n"], S["m"]
    deg = np.bincount(S["lm"])
    assert (deg > 64).sum() > 10 and (deg <= 64).sum() > 0
    rng = np.random.default_rng(64)
    dup = rng.choice(S["cam"].size, 40, replace=False)              # (camera, landmark) pairs named twice, with their own noise
    E = dict(S)
    # plus: camera n and landmark m seen only behind the camera (p2 < 0), landmark m + 1 seen once with weight 0 afterwards
    E["cam"] = np.concatenate([S["cam"], S["cam"][dup], [n, 0, 1]]).astype(np.int32)
    E["lm"] = np.concatenate([S["lm"], S["lm"][dup], [m, m, m + 1]]).astype(np.int32)
    pd = S["p"][dup] + 1e-3 * rng.standard_normal((dup.size, 3)) * np.array([1.0, 1.0, 0.0])
    E["p"] = np.concatenate([S["p"], pd, [[0.1, 0.2, -3.0], [0.2, 0.1, -2.0], [0.1, -0.1, 4.0]]])
    E["w"] = np.ones(E["cam"].size)
    E["n"], E["m"] = n + 1, m + 2
    w_set = E["w"].copy(); w_set[-1] = 0.0
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=61)
    rotE = np.concatenate([rot0, np.eye(3)], axis=1)
    tE = np.concatenate([t0, [[0.3], [-0.7], [1.1]]], axis=1)
    PE = np.concatenate([P0, [[0.5, -0.25], [0.125, 0.75], [-1.5, 2.0]]], axis=1)
    opts = dict(function_tol=1e-10, max_iters=30)
    ctx = _ctx(xmamd, E)
    ctx.set_edge_weights(w_set)
    rot, t, P, info = ctx.bundle_adjust(rotE, tE, PE, trace=40, **opts, **DENSE)
    ctx.close()
    rot_r, t_r, P_r, ref = ba.lm(*_obs(E, w_set), rotE, tE, PE, **opts)
    print(f"duplicates / heavy / masked: dense {info['final_cost']:.15e} ({info['status_name']}, {info['iters']} it), numpy "
          f"{ref['final_cost']:.15e} ({ref['iters']} it); residuals {info['trace'][:, 5]}")
    assert info["n_used"] == S["cam"].size + dup.size
    assert info["status"] == ref["status"] and info["iters"] == ref["iters"]
    assert np.array_equal(info["trace"][:, 3], ref["trace"][:, 3])
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
    assert rot[:, 3 * n:].tobytes() == np.asfortranarray(rotE[:, 3 * n:]).tobytes()
    assert t[:, n:].tobytes() == np.ascontiguousarray(tE[:, n:]).tobytes()
    assert P[:, m:].tobytes() == np.ascontiguousarray(PE[:, m:]).tobytes()


def test_repeatable_and_leaves_the_context_unchanged(xmamd):
    S = ba.ring_scene(n_cams=24, n_pts=250, seed=70, noise=2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=71)
    a, b = _ctx(xmamd, S), _ctx(xmamd, S)
    Ra1, sa1, _ = a.solve(5, 1e-8, 0.0)
    Rb1, sb1, _ = b.solve(5, 1e-8, 0.0)
    out1 = a.bundle_adjust(rot0, t0, P0, trace=40, **DENSE)
    out2 = a.bundle_adjust(rot0, t0, P0, trace=40, **DENSE)
    assert _bits(*out1[:3]) == _bits(*out2[:3]) and out1[3]["trace"].tobytes() == out2[3]["trace"].tobytes()
    assert out1[3]["final_cost"] == out2[3]["final_cost"] and out1[3]["iters"] == out2[3]["iters"]
    Ra2, sa2, ia = a.solve(5, 1e-8, 0.0)
    Rb2, sb2, ib = b.solve(5, 1e-8, 0.0)
    a.close(); b.close()
    assert Ra2.tobytes() == Rb2.tobytes() and sa2.tobytes() == sb2.tobytes() and ia["primal"] == ib["primal"]


def test_above_the_row_limit_is_refused_and_the_context_stays_usable(xmamd):
    S = ba.sequential_scene(n_cams=5462, per_cam=2, seed=66, noise=1e-3)     # 6 x 5462 = 32772 rows
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=67, deg=0.1, rel=1e-5)
    ctx = xmamd.Context(obs=_obs(S), n=S["n"], tuning=dict(schur_solver=2))
    assert 6 * S["n"] > xmamd.BA_DENSE_MAX_ROWS >= 3 * S["n"]
    with pytest.raises(xmamd.XmError, match="error -2"):
        ctx.bundle_adjust(rot0, t0, P0, **DENSE)
    assert "XM_BA_DENSE_MAX_ROWS" in xmamd.lib().xm_last_error().decode()
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, max_iters=2)
    sq = ctx.reprojection_errors(rot0, t0, P0)
    ctx.close()
    print(f"after the refusal: {info['iters']} iterations, cost {info['initial_cost']:.6e} -> {info['final_cost']:.6e}")
    assert info["iters"] == 2 and info["final_cost"] < info["initial_cost"]
    assert info["initial_cost"] == pytest.approx(0.5 * sq[sq >= 0].sum(), rel=1e-12)
