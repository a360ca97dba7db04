"""GPU tests of the bundle adjustment with focal scales (xm_ctx_bundle_adjust_focal, xm_ctx_reprojection_errors_focal;
xm-code_amd/csrc/xm_ba.hip at CD = 7 / 4) against the numpy restatement xm_ba_focal_numpy.py (same problem, same Levenberg-Marquardt
rules, exact linear solves).  The tolerances are those of test_gpu_ba.py / test_gpu_ba_dense.py.

Scenes: the ring scenes of xm_ba_numpy.py seen with focal priors that are off by a ratio in [0.8, 1.25] per camera (every camera's
observations scaled by its ratio: the true focal scale of camera i is ratio[i])."""
import ctypes as C

import numpy as np
import pytest

import xm_ba_focal_numpy as bf
import xm_ba_numpy as ba
import xm_testlib as tl

pytestmark = pytest.mark.gpu

TIGHT = dict(gradient_tol=1e-14, parameter_tol=1e-16)


def _ctx(xmamd, S, w=None, **kw):
    return xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"] if w is None else w), n=S["n"], **kw)


def _obs(S, w=None):
    return S["cam"], S["lm"], S["p"], S["w"] if w is None else w


def _relative_poses(rot, t):
    """gauge-free pose description: R_0^T R_i and R_0^T (t_i - t_0) normalised by their overall size"""
    n = t.shape[1]
    R0 = rot[:, :3]
    rr = np.stack([R0.T @ rot[:, 3 * i:3 * i + 3] for i in range(n)])
    tt = R0.T @ (t - t[:, :1])
    return rr, tt / np.linalg.norm(tt)


def _scene(n_cams, n_pts, seed, noise, **kw):
    S0 = ba.ring_scene(n_cams=n_cams, n_pts=n_pts, seed=seed, noise=noise, **kw)
    ratio = bf.focal_ratios(n_cams, seed + 5)
    return bf.scale_observations(S0, ratio), ratio


def test_noise_free_scene_is_solved_exactly_where_the_pose_only_model_stalls(xmamd):
    S, ratio = _scene(20, 200, 0, 0.0)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=1.0, rel=0.005)
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0, refine_focal=True, **TIGHT)
    _, _, _, plain = ctx.bundle_adjust(rot0, t0, P0, **TIGHT)
    ctx.close()
    g = info["focal"]
    rms = np.sqrt(info["final_cost"] / info["n_used"])
    print(f"noise-free: {info['iters']} iterations ({info['accepted']} accepted), {info['pcg_iters']} PCG, cost {info['initial_cost']:.3e} -> "
          f"{info['final_cost']:.3e}, focal error {np.abs(g - ratio).max():.3e}, status {info['status_name']}; without the focal scales "
          f"{plain['final_cost']:.3e}")
    assert rms <= 1e-10
    assert np.abs(g / ratio - 1.0).max() <= 1e-6
    rr, tt = _relative_poses(rot, t)
    rr0, tt0 = _relative_poses(S["rot"], S["t"])
    assert np.abs(rr - rr0).max() < 1e-8 and np.abs(tt - tt0).max() < 1e-8
    assert plain["final_cost"] > 1e-4


@pytest.mark.parametrize("solver", ["iterative_schur", "dense_schur"])
def test_trace_follows_the_numpy_lm(xmamd, solver):
    """ring 20 / 200, noise 0.05, seed 28, start 40 degrees and 40 % of the scene away with g = 1.  The seed was chosen on the CPU: the
    restatement in float64 (xm_ba_focal_numpy.lm) and in longdouble (xm_ba_focal_exact.lm_trace) give the same accept sequence over these
    10 iterations and candidate costs that agree to 7e-12, so the sequence does not hang on rounding."""
    S, _ = _scene(20, 200, 28, 0.05)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=29, deg=40.0, rel=0.4)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, function_tol=1e-12, max_iters=10, trace=20, refine_focal=True, linear_solver=solver)
    ctx.close()
    _, _, _, _, ref = bf.lm(*_obs(S), rot0, t0, P0, function_tol=1e-12, max_iters=10)
    g, gr = info["trace"], ref["trace"]
    print("GPU trace\n", g, "\nnumpy trace\n", gr)
    assert g.shape[0] == gr.shape[0] == 10
    assert np.array_equal(g[:, 3], gr[:, 3])                                            # the same accept / reject sequence
    assert np.allclose(g[:, 0], gr[:, 0], rtol=1e-9, atol=0) and np.allclose(g[:, 1], gr[:, 1], rtol=1e-9, atol=0)
    assert np.allclose(g[:, 2], gr[:, 2], rtol=1e-6, atol=0)                           # mu follows rho, a ratio of cost differences
    assert np.all(g[:, 5] <= (1e-12 if solver == "iterative_schur" else 1e-8))          # the PCG reached eta | as test_gpu_ba_dense.py


def test_steps_to_a_focal_that_is_not_positive_are_rejected(xmamd):
    """ring 20 / 200, noise 0.05, seed 24, the same far start: in the restatement (float64 and longdouble alike) two of the first ten
    candidates have a focal <= 0.  The device rejects the same iterations, the damping grows after each as after a step without model
    decrease, and the returned focals are positive."""
    S, _ = _scene(20, 200, 24, 0.05)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=25, deg=40.0, rel=0.4)
    _, _, _, _, ref = bf.lm(*_obs(S), rot0, t0, P0, function_tol=1e-12, max_iters=10)
    assert ref["invalid"] >= 1
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, function_tol=1e-12, max_iters=10, trace=20, refine_focal=True)
    ctx.close()
    g, gr = info["trace"], ref["trace"]
    print("GPU trace\n", g, "\nnumpy trace\n", gr, "\ninvalid at", ref["invalid_at"])
    assert np.array_equal(g[:, 3], gr[:, 3])
    for k in ref["invalid_at"]:
        assert g[k, 3] == 0 and (k + 1 >= len(g) or g[k + 1, 2] > g[k, 2])
    assert (info["focal"] > 0).all()


def test_default_eta_reaches_the_numpy_optimum(xmamd):
    """ring 24 / 300, noise 2e-3, seed 30, near start with g = 1.  With noise the focal is weakly determined on so shallow a scene (it is
    recovered to about 5 %), so the optimum is flat along it; checked on the CPU: the numpy LM with exact solves and the numpy LM with the
    restated block-Jacobi PCG at eta = 0.1 end at costs that agree to 4e-10 relative on this scene (default tolerances)."""
    S, _ = _scene(24, 300, 30, 2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=31)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, refine_focal=True)
    ctx.close()
    _, _, _, _, ref = bf.lm(*_obs(S), rot0, t0, P0)
    print(f"GPU {info['final_cost']:.12e} ({info['status_name']}, {info['iters']} it, {info['pcg_iters']} PCG) numpy {ref['final_cost']:.12e}")
    assert info["status"] in xmamd.BA_CONVERGED
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]


def test_fixed_rotations(xmamd):
    S, _ = _scene(16, 150, 40, 2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=41)
    f0 = np.ones(16)
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0, fix_rotations=True, eta=1e-10, function_tol=1e-14, parameter_tol=1e-14, refine_focal=True)
    ctx.close()
    assert np.array_equal(rot, rot0) and rot.tobytes() == np.asfortranarray(rot0).tobytes()
    g0 = np.abs(bf.gradient_at(*_obs(S), rot0, t0, P0, f0, fix_rotations=True)).max()
    g1 = np.abs(bf.gradient_at(*_obs(S), rot, t, P, info["focal"], fix_rotations=True)).max()
    print(f"fixed rotations: cost {info['initial_cost']:.3e} -> {info['final_cost']:.3e}, |g| {g0:.3e} -> {g1:.3e}")
    assert g1 <= 1e-8 * g0 and info["final_cost"] < info["initial_cost"]


def test_held_and_unused_cameras_come_back_bit_identical(xmamd):
    S, ratio = _scene(20, 200, 50, 2e-3)
    n, m = S["n"], S["m"]
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=51)
    # camera n is seen only behind the camera (p2 < 0): no used observation
    E = dict(S)
    E["cam"] = np.concatenate([S["cam"], [n, n]]).astype(np.int32)
    E["lm"] = np.concatenate([S["lm"], [0, 1]]).astype(np.int32)
    E["p"] = np.concatenate([S["p"], [[0.1, 0.2, -3.0], [0.2, 0.1, -2.0]]])
    E["w"] = np.ones(E["cam"].size)
    E["n"] = n + 1
    rotE = np.concatenate([rot0, np.eye(3)], axis=1)
    tE = np.concatenate([t0, [[0.3], [-0.7], [1.1]]], axis=1)
    free = np.ones(n + 1, dtype=bool); free[::3] = False
    f0 = np.random.default_rng(52).uniform(0.9, 1.1, n + 1)
    ctx = _ctx(xmamd, E)
    rot, t, P, info = ctx.bundle_adjust(rotE, tE, P0, eta=1e-6, function_tol=1e-10, refine_focal=True, focal=f0, focal_free=free)
    ctx.close()
    g = info["focal"]
    still = ~free; still[n] = True
    assert info["n_used"] == S["cam"].size
    assert g[still].tobytes() == f0[still].tobytes() and (g[~still] != f0[~still]).all() and (g > 0).all()
    assert rot[:, 3 * n:].tobytes() == np.asfortranarray(rotE[:, 3 * n:]).tobytes() and t[:, n:].tobytes() == np.ascontiguousarray(tE[:, n:]).tobytes()
    assert info["final_cost"] < info["initial_cost"]


def test_repeatable_and_leaves_the_context_unchanged(xmamd):
    S, _ = _scene(24, 250, 70, 2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=71)
    a, b = _ctx(xmamd, S), _ctx(xmamd, S)
    a.solve(5, 1e-8, 0.0); b.solve(5, 1e-8, 0.0)
    out1 = a.bundle_adjust(rot0, t0, P0, refine_focal=True)
    out2 = a.bundle_adjust(rot0, t0, P0, refine_focal=True)
    for x, y in zip(out1[:3], out2[:3]):
        assert x.tobytes() == y.tobytes()
    assert out1[3]["focal"].tobytes() == out2[3]["focal"].tobytes()
    assert out1[3]["final_cost"] == out2[3]["final_cost"] and out1[3]["iters"] == out2[3]["iters"]
    Ra2, sa2, ia = a.solve(5, 1e-8, 0.0)                   # after the calls against a context that never saw one: the same bits
    Rb2, sb2, ib = b.solve(5, 1e-8, 0.0)
    a.close(); b.close()
    assert Ra2.tobytes() == Rb2.tobytes() and sa2.tobytes() == sb2.tobytes() and ia["primal"] == ib["primal"]


def test_reprojection_errors_with_focal_scales(xmamd):
    S, ratio = _scene(20, 200, 60, 2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=61)
    w = S["w"].copy(); w[::7] = 0.0
    p = S["p"].copy(); p[3::11] *= -1.0
    S = dict(S, p=p)
    f0 = np.random.default_rng(62).uniform(0.8, 1.25, 20)
    ctx = _ctx(xmamd, S)
    ctx.set_edge_weights(w)
    sq = ctx.reprojection_errors(rot0, t0, P0, focal=f0)
    ref = bf.sq_errors(S["cam"], S["lm"], S["p"], w, rot0, t0, P0, f0)
    assert np.array_equal(sq < 0, ref < 0) and (sq[ref < 0] == -1.0).all() and (ref < 0).sum() > 20
    u = ref >= 0
    assert np.abs(sq[u] - ref[u]).max() <= 1e-12 * ref[u].max()
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, refine_focal=True, focal=f0, max_iters=1)
    assert abs(0.5 * sq[u].sum() - info["initial_cost"]) <= 1e-12 * info["initial_cost"]
    # the same observations as the focal scales normalise them, in a context of their own: at g = 1 the errors are those above / g^2
    ctx2 = xmamd.Context(obs=(S["cam"], S["lm"], xmamd.rescale_observations(S["p"], S["cam"], f0), S["w"]), n=S["n"])
    ctx2.set_edge_weights(w)
    sq1 = ctx2.reprojection_errors(rot0, t0, P0)
    ctx.close(); ctx2.close()
    assert np.array_equal(sq1 < 0, sq < 0)
    g2 = f0[S["cam"]] ** 2
    assert np.abs(sq1[u] - sq[u] / g2[u]).max() <= 1e-12 * (sq[u] / g2[u]).max()


def test_a_start_far_below_returns_positive_focals_at_the_truth(xmamd):
    S, ratio = _scene(20, 200, 0, 0.0)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=1.0, rel=0.005)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, refine_focal=True, focal=np.full(20, 0.05), eta=1e-6, function_tol=1e-12)
    ctx.close()
    g = info["focal"]
    print(f"g = 0.05 start: {info['iters']} iterations ({info['accepted']} accepted), cost {info['final_cost']:.3e}, focal error {np.abs(g - ratio).max():.3e}")
    assert (g > 0).all() and np.abs(g / ratio - 1.0).max() <= 1e-6


def _raw(xmamd, ctx, n, m, flags=None, focal=None, null_focal=False, entry="focal", eta=0.1, free=None):
    opt, res = xmamd.BaOptions(), xmamd.BaResult()
    opt.struct_size, res.struct_size = C.sizeof(opt), C.sizeof(res)
    opt.eta, opt.max_iters = eta, 2
    opt.flags = xmamd.BA_REFINE_FOCAL if flags is None else flags
    rot = np.asfortranarray(np.tile(np.eye(3), (1, n))); t = np.zeros((3, n), order="F"); P = np.zeros((3, max(m, 1)), order="F")
    P[2] = 10.0
    f = np.ones(n) if focal is None else np.asarray(focal, dtype=np.float64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    if entry == "plain":
        return xmamd.lib().xm_ctx_bundle_adjust(ctx.h, C.byref(opt), ptr(rot), ptr(t), ptr(P), C.byref(res))
    return xmamd.lib().xm_ctx_bundle_adjust_focal(ctx.h, C.byref(opt), ptr(rot), ptr(t), ptr(P), None if null_focal else ptr(f),
                                                  None if free is None else ptr(free), C.byref(res))


def test_refusals_leave_contexts_usable(xmamd):
    ERR_ARG = -2
    V = tl.gen_vg(40, deg=6, sigma=0.05, seed=80)
    c = xmamd.Context(Q=V["Q"])
    assert _raw(xmamd, c, c.n, 1) == ERR_ARG and "XM_STORAGE_SCHUR" in xmamd.lib().xm_last_error().decode()
    assert c.solve(5, 1e-8, 0.0)[2]["status"] == 1
    c.close()
    S = ba.ring_scene(n_cams=12, n_pts=80, seed=82, noise=1e-3)
    n, m = S["n"], S["m"]
    ctx = _ctx(xmamd, S)
    _, _, i0 = ctx.solve(5, 1e-8, 0.0)
    F = xmamd.BA_REFINE_FOCAL
    bad = lambda v: np.where(np.arange(n) == 3, v, 1.0)
    for kw in (dict(flags=0), dict(flags=xmamd.BA_FIX_ROTATIONS),                      # the flag missing on the _focal entry point
               dict(flags=F | xmamd.BA_PRECOND_TWO_LEVEL), dict(flags=F | xmamd.BA_PRECOND_BLOCKS), dict(flags=F | 4), dict(flags=F | 8),
               dict(null_focal=True), dict(focal=bad(0.0)), dict(focal=bad(-1.0)), dict(focal=bad(np.nan)), dict(focal=bad(np.inf)),
               dict(eta=0.0), dict(eta=1.0),
               dict(entry="plain", flags=F), dict(entry="plain", flags=F | xmamd.BA_FIX_ROTATIONS)):   # xm_ctx_bundle_adjust: an unknown flag
        assert _raw(xmamd, ctx, n, m, **kw) == ERR_ARG, kw
    assert _raw(xmamd, ctx, n, m) == 0 and _raw(xmamd, ctx, n, m, flags=F | xmamd.BA_FIX_ROTATIONS | xmamd.BA_DENSE_SCHUR) == 0
    assert _raw(xmamd, ctx, n, m, free=np.zeros(n, dtype=np.uint8)) == 0
    rot = np.asfortranarray(np.tile(np.eye(3), (1, n))); t = np.zeros((3, n), order="F"); P = np.zeros((3, m), order="F"); P[2] = 10.0
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros(len(S["cam"]))
    L = xmamd.lib()
    assert L.xm_ctx_reprojection_errors_focal(ctx.h, ptr(rot), ptr(t), ptr(P), None, ptr(out)) == ERR_ARG
    assert L.xm_ctx_reprojection_errors_focal(ctx.h, ptr(rot), ptr(t), ptr(P), ptr(bad(0.0)), ptr(out)) == ERR_ARG
    assert L.xm_ctx_reprojection_errors_focal(ctx.h, ptr(rot), ptr(t), ptr(P), ptr(np.ones(n)), ptr(out)) == 0
    q = xmamd.BaProbe(); q.struct_size = C.sizeof(q); q.mu = 1.0
    for flags, f, rc in ((0, np.ones(n), ERR_ARG), (F | xmamd.BA_PRECOND_BLOCKS, np.ones(n), ERR_ARG), (F, bad(np.nan), ERR_ARG), (F, None, ERR_ARG),
                         (F, np.ones(n), 0)):
        q.flags = flags
        assert L.xm_ctx_ba_probe_focal(ctx.h, ptr(rot), ptr(t), ptr(P), None if f is None else ptr(f), None, C.byref(q), None) == rc, flags
    q.flags = F
    assert L.xm_ctx_ba_probe(ctx.h, ptr(rot), ptr(t), ptr(P), C.byref(q)) == ERR_ARG       # the plain probe does not know the flag
    _, _, i1 = ctx.solve(5, 1e-8, 0.0)
    ctx.close()
    assert i0["status"] == i1["status"] == 1 and i0["primal"] == i1["primal"]
