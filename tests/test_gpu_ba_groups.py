"""GPU tests of the bundle adjustment with focal groups (xm_ctx_bundle_adjust_focal_groups; xm-code_amd/csrc/xm_ba.hip at CD = 7 / 4 in
its grouped mode) against the numpy restatement xm_ba_groups_numpy.py (same problem, same Levenberg-Marquardt rules, exact linear solves).
The tolerances are those of test_gpu_ba_focal.py.

Scenes: the ring scenes of xm_ba_numpy.py seen with focal priors that are off by one ratio in [0.8, 1.25] per GROUP (camera i in group
i mod G; every camera's observations scaled by its group's ratio: the true focal scale of group c is ratio[c])."""
import numpy as np
import pytest

import xm_ba_focal_numpy as bf
import xm_ba_groups_numpy as bg
import xm_ba_numpy as ba

pytestmark = pytest.mark.gpu

TIGHT = dict(gradient_tol=1e-14, parameter_tol=1e-16)


def _ctx(xmamd, S, w=None, **kw):
    return xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"] if w is None else w), n=S["n"], **kw)


def _obs(S):
    return S["cam"], S["lm"], S["p"], S["w"]


def _scene(n_cams, n_pts, seed, noise, G=3, **kw):
    S0 = ba.ring_scene(n_cams=n_cams, n_pts=n_pts, seed=seed, noise=noise, **kw)
    group_of = np.arange(n_cams) % G
    ratio = np.random.default_rng(seed + 5).uniform(0.8, 1.25, G)
    return bf.scale_observations(S0, ratio[group_of]), ratio, group_of


def test_noise_free_scene_with_three_groups_is_solved_exactly(xmamd):
    S, ratio, group_of = _scene(20, 200, 0, 0.0)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=1, deg=1.0, rel=0.005)
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0, refine_focal=True, focal_group=group_of, **TIGHT)
    ctx.close()
    g = info["focal"]
    rms = np.sqrt(info["final_cost"] / info["n_used"])
    print(f"noise-free, 3 groups: {info['iters']} iterations ({info['accepted']} accepted), {info['pcg_iters']} PCG, cost "
          f"{info['initial_cost']:.3e} -> {info['final_cost']:.3e}, ratio error {np.abs(g / ratio - 1).max():.3e}, status {info['status_name']}")
    assert g.shape == (3,)
    assert rms <= 1e-10
    assert np.abs(g / ratio - 1.0).max() <= 1e-6


@pytest.mark.parametrize("solver", ["iterative_schur", "dense_schur"])
def test_trace_follows_the_numpy_lm(xmamd, solver):
    """ring 20 / 200, noise 0.05, seed 32, three groups, start 40 degrees and 40 % of the scene away with g = 1.  The seed was chosen on
    the CPU: the restatement in float64 (xm_ba_groups_numpy.lm) and in longdouble (xm_ba_groups_exact.lm_trace) give the same accept
    sequence over these 10 iterations and candidate costs that agree to 5.1e-12, so the sequence does not hang on rounding; and the
    restatement with its PCG run to eta = 1e-12 (the exact focal block in M, the library's rule at G = 3) stays within 6.8e-12 of the one
    with exact solves.  On other seeds that restated PCG itself leaves the 1e-9: 8.3e-9 on seed 26, 1.5e-8 on seed 24, at the second
    iteration, where mu is 3e-5 -- a residual of 1e-12 does not bound the step's error by 1e-9 there, whatever runs the PCG."""
    S, _, group_of = _scene(20, 200, 32, 0.05)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=33, deg=40.0, rel=0.4)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, function_tol=1e-12, max_iters=10, trace=20, refine_focal=True, focal_group=group_of,
                                      focal=np.ones(3), linear_solver=solver)
    ctx.close()
    _, _, _, _, ref = bg.lm(*_obs(S), rot0, t0, P0, group_of, focal=np.ones(3), function_tol=1e-12, max_iters=10)
    g, gr = info["trace"], ref["trace"]
    print("GPU trace\n", g, "\nnumpy trace\n", gr)
    assert g.shape[0] == gr.shape[0] == 10
    assert np.array_equal(g[:, 3], gr[:, 3])                                            # the same accept / reject sequence
    assert np.allclose(g[:, 0], gr[:, 0], rtol=1e-9, atol=0) and np.allclose(g[:, 1], gr[:, 1], rtol=1e-9, atol=0)
    assert np.allclose(g[:, 2], gr[:, 2], rtol=1e-6, atol=0)                           # mu follows rho, a ratio of cost differences
    assert np.all(g[:, 5] <= (1e-12 if solver == "iterative_schur" else 1e-8))          # the PCG reached eta | as test_gpu_ba_dense.py
    assert info["coarse_fallbacks"] == 0                                                # the exact focal block was factored every time


def test_steps_to_a_group_focal_that_is_not_positive_are_rejected(xmamd):
    """ring 20 / 200, noise 0.05, seed 24 with one ratio per camera, twenty singleton groups in a shuffled order, the far start: the scene
    of test_gpu_ba_focal.py's test of the same name, on which the restatement -- float64 with exact solves, float64 with its PCG at eta =
    1e-12, and longdouble alike (checked on the CPU) -- rejects iterations 8 and 9 because a candidate focal is <= 0, with the accept
    sequence 1 0 0 0 0 0 1 1 0 0.  (With three or five groups on seeds 20 .. 31 the restatement never meets such a candidate: a shared
    focal is too well determined.)  The device rejects the same iterations, the damping grows after each, the returned focals are positive."""
    n = 20
    S = bf.scale_observations(ba.ring_scene(n_cams=n, n_pts=200, seed=24, noise=0.05), bf.focal_ratios(n, 29))
    group_of = np.random.default_rng(7).permutation(n)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=25, deg=40.0, rel=0.4)
    _, _, _, _, ref = bg.lm(*_obs(S), rot0, t0, P0, group_of, focal=np.ones(n), function_tol=1e-12, max_iters=10)
    assert ref["invalid_at"] == [8, 9]
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, function_tol=1e-12, max_iters=10, trace=20, refine_focal=True, focal_group=group_of)
    ctx.close()
    g, gr = info["trace"], ref["trace"]
    print("GPU trace\n", g, "\nnumpy trace\n", gr, "\ninvalid at", ref["invalid_at"])
    assert np.array_equal(g[:, 3], gr[:, 3])
    for k in ref["invalid_at"]:
        assert g[k, 3] == 0 and (k + 1 >= len(g) or g[k + 1, 2] > g[k, 2])
    assert (info["focal"] > 0).all()


def test_default_eta_reaches_the_numpy_optimum(xmamd):
    """ring 24 / 300, noise 2e-3, seed 31, three groups, near start with g = 1.  Checked on the CPU: the numpy LM with exact solves and the
    numpy LM with the restated PCG (M = blockdiag(pose blocks, the exact focal block)) at eta = 0.1 end at costs that agree to 4.3e-10
    relative on this scene (default tolerances)."""
    S, _, group_of = _scene(24, 300, 31, 2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=32)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, refine_focal=True, focal_group=group_of)
    ctx.close()
    _, _, _, _, ref = bg.lm(*_obs(S), rot0, t0, P0, group_of, focal=np.ones(3))
    print(f"GPU {info['final_cost']:.12e} ({info['status_name']}, {info['iters']} it, {info['pcg_iters']} PCG) numpy {ref['final_cost']:.12e}")
    assert info["status"] in xmamd.BA_CONVERGED
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]


def test_singleton_groups_end_at_the_per_image_cost(xmamd):
    S, _, _ = _scene(16, 150, 40, 2e-3, G=16)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=41)
    perm = np.random.default_rng(42).permutation(16)
    kw = dict(eta=1e-10, function_tol=1e-12, refine_focal=True)
    ctx = _ctx(xmamd, S)
    _, _, _, a = ctx.bundle_adjust(rot0, t0, P0, **kw)
    _, _, _, b = ctx.bundle_adjust(rot0, t0, P0, focal_group=perm, **kw)
    ctx.close()
    print(f"per image {a['final_cost']:.12e} ({a['iters']} it), singleton groups {b['final_cost']:.12e} ({b['iters']} it)")
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-9 * a["final_cost"]
    assert np.allclose(b["focal"][perm], a["focal"], rtol=1e-6, atol=0)


def test_fixed_rotations(xmamd):
    S, _, group_of = _scene(16, 150, 40, 2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=41)
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0, fix_rotations=True, eta=1e-10, function_tol=1e-14, parameter_tol=1e-14, refine_focal=True,
                                        focal_group=group_of)
    ctx.close()
    assert rot.tobytes() == np.asfortranarray(rot0).tobytes()
    pr = bg.GroupProblem(*_obs(S), S["n"], S["m"], group_of, 3, True)

    def grad(rot, t, P, g):
        Rcw, tcw = ba.to_world_to_camera(rot, t)
        _, r, J, _ = pr.shared(Rcw, tcw, P.T.copy(), g)
        return np.abs(J.T @ r).max()
    g0, g1 = grad(rot0, t0, P0, np.ones(3)), grad(rot, t, P, info["focal"])
    print(f"fixed rotations: cost {info['initial_cost']:.3e} -> {info['final_cost']:.3e}, |g| {g0:.3e} -> {g1:.3e}")
    assert g1 <= 1e-8 * g0 and info["final_cost"] < info["initial_cost"]


def test_held_unused_and_empty_groups_come_back_bit_identical(xmamd):
    S, ratio, _ = _scene(20, 200, 50, 2e-3)
    n = S["n"]
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=51)
    # camera n is seen only behind the camera (p2 < 0): no used observation; it is group 3's only member.  Group 4 is empty, group 1 held
    E = dict(S)
    E["cam"] = np.concatenate([S["cam"], [n, n]]).astype(np.int32)
    E["lm"] = np.concatenate([S["lm"], [0, 1]]).astype(np.int32)
    E["p"] = np.concatenate([S["p"], [[0.1, 0.2, -3.0], [0.2, 0.1, -2.0]]])
    E["w"] = np.ones(E["cam"].size)
    E["n"] = n + 1
    rotE = np.concatenate([rot0, np.eye(3)], axis=1)
    tE = np.concatenate([t0, [[0.3], [-0.7], [1.1]]], axis=1)
    group_of = np.concatenate([np.arange(n) % 3, [3]])
    f0 = np.array([1.0, ratio[1], 1.0, 0.9123, 1.0771])
    free = np.array([1, 0, 1, 1, 1], dtype=bool)
    ctx = _ctx(xmamd, E)
    rot, t, P, info = ctx.bundle_adjust(rotE, tE, P0, eta=1e-6, function_tol=1e-10, refine_focal=True, focal_group=group_of, focal=f0, focal_free=free)
    rot2, t2, P2, info2 = ctx.bundle_adjust(rotE, tE, P0, eta=1e-6, function_tol=1e-10, refine_focal=True, focal_group=group_of, focal=f0,
                                            focal_free=free)
    ctx.close()
    g = info["focal"]
    assert g[[1, 3, 4]].tobytes() == f0[[1, 3, 4]].tobytes()
    assert (g[[0, 2]] != 1.0).all() and np.abs(g[[0, 2]] / ratio[[0, 2]] - 1).max() < 0.1
    assert rot[:, 3 * n:].tobytes() == np.asfortranarray(rotE)[:, 3 * n:].tobytes() and t[:, n].tobytes() == np.asfortranarray(tE)[:, n].tobytes()
    # two calls give the same bytes
    assert g.tobytes() == info2["focal"].tobytes() and rot.tobytes() == rot2.tobytes() and t.tobytes() == t2.tobytes() and P.tobytes() == P2.tobytes()
    assert info["final_cost"] == info2["final_cost"] and info["pcg_iters"] == info2["pcg_iters"]


def test_nonmonotonic_steps_with_a_loss(xmamd):
    S, _, group_of = _scene(20, 200, 60, 0.02)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=61, deg=10.0, rel=0.1)
    ctx = _ctx(xmamd, S)
    kw = dict(refine_focal=True, focal_group=group_of, loss="huber", loss_scale=0.05, eta=1e-8)
    _, _, _, mono = ctx.bundle_adjust(rot0, t0, P0, **kw)
    _, _, _, non = ctx.bundle_adjust(rot0, t0, P0, nonmonotonic=True, trace=200, **kw)
    ctx.close()
    print(f"monotonic {mono['final_cost']:.9e} ({mono['iters']} it), non-monotonic {non['final_cost']:.9e} ({non['iters']} it)")
    assert mono["status"] in xmamd.BA_CONVERGED and non["status"] in xmamd.BA_CONVERGED
    assert non["final_cost"] <= non["trace"][:, 0].min() * (1 + 1e-12)                 # the least-cost point is returned
    assert non["final_cost"] < non["initial_cost"] and mono["final_cost"] < mono["initial_cost"]
    assert (non["focal"] > 0).all()


def test_refine_filtered_takes_the_groups(xmamd):
    S, ratio, group_of = _scene(20, 200, 70, 2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=71)
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.refine_filtered(rot0, t0, P0, rounds=1, reprojection=0.05, refine_focal=True, focal_group=group_of)
    ctx.close()
    assert info["rounds"] and info["rounds"][0]["ba_full"]["final_cost"] < info["rounds"][0]["ba_fixed"]["initial_cost"]


def test_every_refusal_leaves_the_context_solving_bit_for_bit(xmamd):
    import ctypes as C
    S, _, group_of = _scene(16, 150, 80, 2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=81)
    n = S["n"]
    kw = dict(refine_focal=True, focal_group=group_of, max_iters=5)
    fresh = _ctx(xmamd, S)
    want = fresh.bundle_adjust(rot0, t0, P0, **kw)
    fresh.close()
    ctx = _ctx(xmamd, S)
    L = xmamd.lib()
    V = lambda a: a.ctypes.data_as(C.c_void_p)
    rot = np.array(rot0, order="F"); t = np.array(t0, order="F"); P = np.array(P0, order="F")
    go = np.ascontiguousarray(group_of, dtype=np.int32)

    def call(flags=xmamd.BA_REFINE_FOCAL, G=3, g=go, focal=None, eta=0.1):
        opt, res = xmamd.BaOptions(), xmamd.BaResult()
        opt.struct_size, res.struct_size = C.sizeof(xmamd.BaOptions), C.sizeof(xmamd.BaResult)
        opt.eta, opt.flags = eta, flags
        f = np.ones(max(G, 1)) if focal is None else np.array(focal, dtype=np.float64)
        return L.xm_ctx_bundle_adjust_focal_groups(ctx.h, C.byref(opt), V(rot), V(t), V(P), G, None if g is None else V(g), V(f), None, C.byref(res))
    bad = go.copy(); bad[3] = 3
    neg = go.copy(); neg[0] = -1
    refusals = [call(flags=0), call(G=0), call(G=n + 1, focal=np.ones(n + 1)), call(g=bad), call(g=neg), call(g=None), call(focal=[1.0, 0.0, 1.0]),
                call(focal=[1.0, np.nan, 1.0]), call(focal=[1.0, np.inf, 1.0]), call(flags=xmamd.BA_REFINE_FOCAL | xmamd.BA_PRECONDITIONERS["two_level"]),
                call(flags=xmamd.BA_REFINE_FOCAL | xmamd.BA_PRECONDITIONERS["blocks"]),
                call(eta=0.0), call(flags=xmamd.BA_REFINE_FOCAL | 4)]
    assert refusals == [-2] * len(refusals), refusals       # XM_ERR_ARG
    assert rot.tobytes() == np.asfortranarray(rot0).tobytes()
    got = ctx.bundle_adjust(rot0, t0, P0, **kw)
    ctx.close()
    for a, b in zip(want[:3], got[:3]):
        assert a.tobytes() == b.tobytes()
    assert want[3]["focal"].tobytes() == got[3]["focal"].tobytes() and want[3]["final_cost"] == got[3]["final_cost"]


def test_a_shared_focal_is_better_determined_than_per_image_ones(xmamd):
    """The reason for the feature.  Ring 20 / 200, noise 2e-3, seed 60, every camera's prior off by the same ratio 1.1, near start, default
    tolerances.  On the CPU the restatements end at: per-image focals (xm_ba_focal_numpy.lm) median |g_i - 1.1| = 2.10e-2, one shared focal
    (xm_ba_groups_numpy.lm, G = 1) |g - 1.1| = 2.09e-3, a factor 10 (exact solves; the same to three digits with the restated PCG at eta =
    0.1).  The test asserts only that the shared estimate is the better one."""
    n = 20
    S = bf.scale_observations(ba.ring_scene(n_cams=n, n_pts=200, seed=60, noise=2e-3), np.full(n, 1.1))
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=61)
    ctx = _ctx(xmamd, S)
    _, _, _, per = ctx.bundle_adjust(rot0, t0, P0, refine_focal=True)
    _, _, _, one = ctx.bundle_adjust(rot0, t0, P0, refine_focal=True, focal_group=np.zeros(n, dtype=int))
    ctx.close()
    e_per, e_one = float(np.median(np.abs(per["focal"] - 1.1))), float(abs(one["focal"][0] - 1.1))
    print(f"per-image: median focal error {e_per:.3e}, cost {per['final_cost']:.6e}; shared: focal error {e_one:.3e}, cost {one['final_cost']:.6e}")
    assert one["focal"].shape == (1,)
    assert e_one < e_per
