"""GPU tests of the opt-in PCG preconditioners of xm_ctx_bundle_adjust (XM_BA_PRECOND_BLOCKS, XM_BA_PRECOND_TWO_LEVEL; xm-code_amd/csrc/xm_ba.hip)
through Context.bundle_adjust: the LM path is the one of the exact numpy solver, sequential captures no longer run into the PCG's iteration
cap, degenerate inputs, exactness of state and the refusals."""
import ctypes as C

import numpy as np
import pytest

import xm_ba_loss_numpy as rl
import xm_ba_numpy as ba
import xm_ba_precond_numpy as bp

pytestmark = pytest.mark.gpu

KINDS = ("blocks", "two_level")
PCG_CAP = 500


def _ctx(xmamd, S, w=None, **kw):
    return xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"] if w is None else w), n=S["n"], **kw)


def _obs(S, w=None):
    return S["cam"], S["lm"], S["p"], S["w"] if w is None else w


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _same_path(g, gr, n):
    assert g.shape[0] == gr.shape[0] == n
    assert np.array_equal(g[:, 3], gr[:, 3])                                            # the same accept / reject sequence
    assert np.allclose(g[:, 0], gr[:, 0], rtol=1e-9, atol=0) and np.allclose(g[:, 1], gr[:, 1], rtol=1e-9, atol=0)
    assert np.allclose(g[:, 2], gr[:, 2], rtol=1e-6, atol=0)
    assert np.all(g[:, 5] <= 1e-12)                                                     # each PCG reached eta


@pytest.mark.parametrize("kind", KINDS)
def test_trace_follows_the_numpy_lm(xmamd, kind):
    # the scene and options of test_gpu_ba.py::test_trace_follows_the_numpy_lm: the preconditioner must not change what is solved
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=0.05)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=21, deg=40.0, rel=0.4)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, function_tol=1e-12, max_iters=10, trace=20, preconditioner=kind)
    ctx.close()
    _, _, _, ref = ba.lm(*_obs(S), rot0, t0, P0, function_tol=1e-12, max_iters=10)
    print(kind, "GPU trace\n", info["trace"], "\nnumpy trace\n", ref["trace"], "\ncoarse fallbacks", info["coarse_fallbacks"])
    _same_path(info["trace"], ref["trace"], 10)


@pytest.mark.parametrize("kind", KINDS)
def test_trace_with_fixed_rotations(xmamd, kind):
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=0.05)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=21, deg=2.0, rel=0.4)
    ctx = _ctx(xmamd, S)
    rot, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, function_tol=1e-12, max_iters=10, trace=20, preconditioner=kind, fix_rotations=True)
    ctx.close()
    _, _, _, ref = ba.lm(*_obs(S), rot0, t0, P0, function_tol=1e-12, max_iters=10, fix_rotations=True)
    print(kind, "GPU trace\n", info["trace"], "\nnumpy trace\n", ref["trace"])
    _same_path(info["trace"], ref["trace"], ref["trace"].shape[0])
    assert rot.tobytes() == np.asfortranarray(rot0).tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_trace_with_a_robust_loss_and_nonmonotonic_steps(xmamd, kind):
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=0.05)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=21, deg=40.0, rel=0.4)
    opts = dict(function_tol=1e-12, max_iters=10)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, trace=20, preconditioner=kind, loss="huber", loss_scale=0.1, nonmonotonic=True, **opts)
    ctx.close()
    _, _, _, ref = rl.lm(*_obs(S), rot0, t0, P0, loss="huber", a=0.1, nonmonotonic=True, **opts)
    print(kind, "GPU trace\n", info["trace"], "\nnumpy trace\n", ref["trace"])
    _same_path(info["trace"], ref["trace"][:, :4], ref["trace"].shape[0])


def test_sequential_capture_no_longer_hits_the_iteration_cap(xmamd):
    """default / blocks / two-level on sequential_scene(600) from the start of test_harder_scenes_reach_the_numpy_optimum[sequential]"""
    S = ba.sequential_scene(n_cams=600, seed=62, noise=1e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=63, deg=0.5, rel=2e-4)
    opts = dict(eta=1e-6, function_tol=1e-8, trace=1000)
    ctx = _ctx(xmamd, S)
    out = {k: ctx.bundle_adjust(rot0, t0, P0, preconditioner=k, **opts)[3] for k in ("jacobi",) + KINDS}
    ctx.close()
    for k, info in out.items():
        tr = info["trace"]
        print(f"{k}: {info['status_name']}, {info['iters']} LM iterations, {info['pcg_iters']} PCG iterations, final cost {info['final_cost']:.12e}, "
              f"{info['seconds']:.2f} s, coarse fallbacks {info['coarse_fallbacks']}\n  PCG per step {tr[:, 4].astype(int).tolist()}\n"
              f"  worst relative residual {tr[:, 5].max():.2e}")
    model = bp.first_step_iterations(*_obs(S), rot0, t0, P0, 1e-4, 1e-6, "two_level")
    print(f"first LM step: GPU two-level {int(out['two_level']['trace'][0, 4])} PCG iterations, numpy model {model}")
    _, _, _, ref = ba.lm(*_obs(S), rot0, t0, P0, function_tol=1e-8)
    two = out["two_level"]
    print(f"numpy LM with exact solves: {ref['final_cost']:.12e} ({ref['iters']} iterations)")
    assert np.all(two["trace"][:, 4] < PCG_CAP) and np.all(two["trace"][:, 5] <= 1e-6)
    assert two["coarse_fallbacks"] == 0 and out["blocks"]["coarse_fallbacks"] == 0 and out["jacobi"]["coarse_fallbacks"] == 0
    assert abs(two["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]
    assert 4 * two["pcg_iters"] <= out["jacobi"]["pcg_iters"]


def test_a_size_the_dense_solver_cannot_take(xmamd):
    """6000 cameras = 36 000 rows > XM_BA_DENSE_MAX_ROWS.  The numpy LM with exact sparse solves is too slow for a test at this size, so the
    two-level run is compared with the default run from the same start only.  perturb() moves translations and landmarks by rel times the
    scene's size, and this scene is ten times as long as the 600-camera one: rel = 2e-5 displaces them by the same absolute amount (0.02 of
    the 5-unit depth) as rel = 2e-4 does there."""
    S = ba.sequential_scene(n_cams=6000, seed=64, noise=1e-3)
    assert 6 * S["n"] > xmamd.BA_DENSE_MAX_ROWS
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=65, deg=0.5, rel=2e-5)
    opts = dict(eta=1e-6, function_tol=1e-8, max_iters=60, trace=60)
    ctx = _ctx(xmamd, S)
    two = ctx.bundle_adjust(rot0, t0, P0, preconditioner="two_level", **opts)[3]
    dflt = ctx.bundle_adjust(rot0, t0, P0, **opts)[3]
    ctx.close()
    for k, info in (("two_level", two), ("jacobi", dflt)):
        print(f"{k}: {info['status_name']}, {info['iters']} LM iterations, {info['pcg_iters']} PCG iterations, cost {info['initial_cost']:.6e} -> "
              f"{info['final_cost']:.12e}, {info['seconds']:.2f} s, coarse fallbacks {info['coarse_fallbacks']}\n"
              f"  PCG per step {info['trace'][:, 4].astype(int).tolist()}")
    assert two["status"] in xmamd.BA_CONVERGED or two["final_cost"] <= dflt["final_cost"]
    assert np.all(two["trace"][:, 4] < PCG_CAP)


def test_masked_observations_change_nothing(xmamd):
    # the construction of test_gpu_ba.py::test_masked_observations_change_nothing with the two-level preconditioner
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=50, noise=2e-3, min_views=3)
    n, m = S["n"], S["m"]
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=51)
    E = dict(S)
    E["cam"] = np.concatenate([S["cam"], [n, 0, 1]]).astype(np.int32)
    E["lm"] = np.concatenate([S["lm"], [m, m, m + 1]]).astype(np.int32)
    E["p"] = np.concatenate([S["p"], [[0.1, 0.2, -3.0], [0.2, 0.1, -2.0], [0.1, -0.1, 4.0]]])
    E["w"] = np.ones(E["cam"].size)
    E["n"], E["m"] = n + 1, m + 2
    w_set = E["w"].copy(); w_set[-1] = 0.0
    rotE = np.concatenate([rot0, np.eye(3)], axis=1)
    tE = np.concatenate([t0, [[0.3], [-0.7], [1.1]]], axis=1)
    PE = np.concatenate([P0, [[0.5, -0.25], [0.125, 0.75], [-1.5, 2.0]]], axis=1)
    opts = dict(eta=1e-6, function_tol=1e-10, preconditioner="two_level")
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0, **opts)
    ctx.close()
    ctxE = _ctx(xmamd, E)
    ctxE.set_edge_weights(w_set)
    rot2, t2, P2, info2 = ctxE.bundle_adjust(rotE, tE, PE, **opts)
    ctxE.close()
    print(f"base {info['final_cost']:.15e} ({info['iters']} it), extended {info2['final_cost']:.15e} ({info2['iters']} it)")
    assert info["n_used"] == S["cam"].size and info2["n_used"] == S["cam"].size
    assert _rel(rot2[:, :3 * n], rot) <= 1e-12 and _rel(t2[:, :n], t) <= 1e-12 and _rel(P2[:, :m], P) <= 1e-12
    assert rot2[:, 3 * n:].tobytes() == np.asfortranarray(rotE[:, 3 * n:]).tobytes()
    assert t2[:, n:].tobytes() == np.ascontiguousarray(tE[:, n:]).tobytes()
    assert P2[:, m:].tobytes() == np.ascontiguousarray(PE[:, m:]).tobytes()


def test_seventeen_cameras_leave_an_aggregate_of_one(xmamd):
    S = ba.ring_scene(n_cams=17, n_pts=200, seed=90, noise=2e-3)
    assert np.array_equal(np.bincount(xmamd.ba_aggregate_plan(S["cam"], S["lm"], n=17)), [16, 1])
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=91)
    opts = dict(eta=1e-10, function_tol=1e-10)
    ctx = _ctx(xmamd, S)
    a = ctx.bundle_adjust(rot0, t0, P0, **opts)[3]
    b = ctx.bundle_adjust(rot0, t0, P0, preconditioner="two_level", trace=100, **opts)[3]
    c = ctx.bundle_adjust(rot0, t0, P0, preconditioner="two_level", fix_rotations=True, **opts)[3]
    d = ctx.bundle_adjust(rot0, t0, P0, fix_rotations=True, **opts)[3]
    ctx.close()
    print(f"default {a['final_cost']:.12e} ({a['pcg_iters']} PCG), two-level {b['final_cost']:.12e} ({b['pcg_iters']} PCG, fallbacks "
          f"{b['coarse_fallbacks']}); fixed rotations {d['final_cost']:.12e} / {c['final_cost']:.12e}")
    assert b["coarse_fallbacks"] == 0 and np.all(b["trace"][:, 5] <= 1e-10)
    assert abs(b["final_cost"] - a["final_cost"]) <= 1e-6 * a["final_cost"] and abs(c["final_cost"] - d["final_cost"]) <= 1e-6 * d["final_cost"]


def _one_centre_scene():
    """sixteen cameras at distinct places (0..15) and sixteen turning about the origin (16..31, tcw = 0 exactly).  Landmarks 0..14 are seen
    by camera 0 and one other of the first sixteen and come first in the input, so the breadth-first plan lists those sixteen before any
    camera at the origin; every other landmark is seen by two cameras of each kind, so every depth is observable."""
    rng = np.random.default_rng(95)
    yaw = np.linspace(-0.3, 0.3, 16)
    Cc = np.zeros((32, 3))
    Cc[:16] = np.stack([np.linspace(-3, 3, 16), np.full(16, -1.0), rng.uniform(-0.5, 0.5, 16)], axis=1)
    tgt = [np.array([0.0, 6.0, 0.0])] * 16 + [np.array([6 * np.sin(y), 6 * np.cos(y), 0.0]) for y in yaw]
    Rcw = np.stack([ba._look_at(Cc[i], tgt[i], rng, 0.05) for i in range(32)])
    tcw = -np.einsum("iab,ib->ia", Rcw, Cc)
    m = 15 + 600
    Pw = np.stack([rng.uniform(-2, 2, m), rng.uniform(5, 7, m), rng.uniform(-1.5, 1.5, m)], axis=1)
    cams, lms = [], []
    for l in range(15):
        cams += [0, l + 1]; lms += [l, l]
    for l in range(15, m):
        s = np.concatenate([np.sort(rng.choice(16, 2, replace=False)), 16 + np.sort(rng.choice(16, 2, replace=False))])
        cams += list(s); lms += [l] * 4
    cams, lms = np.array(cams), np.array(lms)
    return ba._pack(Rcw, tcw, Pw, cams, lms, ba._observe(Rcw, tcw, Pw, cams, lms, rng, 1e-3))


@pytest.mark.parametrize("fix", [False, True])
def test_cameras_at_one_centre(xmamd, fix):
    # aggregate 1 holds exactly the sixteen cameras at the origin: C_i = c_a = 0 exactly, so its scale column has norm 0 and is dropped in
    # the first LM iteration (the cameras start at their true poses; the centres part once a step is accepted)
    S = _one_centre_scene()
    assert np.all(S["t"][:, 16:] == 0.0) and np.all(S["p"][:, 2] > 0)
    assert np.array_equal(xmamd.ba_aggregate_plan(S["cam"], S["lm"], n=32), [0] * 16 + [1] * 16)
    Rcw, tcw = ba.to_world_to_camera(S["rot"], S["t"])
    _, order = bp.aggregate_plan(S["cam"], S["lm"], 32)
    _, dropped = bp.rigid_basis(Rcw, tcw, order, fix_rotations=fix)
    assert dropped == [7 if fix else 13]                                         # the scale column of aggregate 1, nothing else
    P0 = S["P"] + 0.01 * np.random.default_rng(96).standard_normal(S["P"].shape)
    opts = dict(eta=1e-10, function_tol=1e-10, fix_rotations=fix)
    ctx = _ctx(xmamd, S)
    a = ctx.bundle_adjust(S["rot"], S["t"], P0, **opts)[3]
    b = ctx.bundle_adjust(S["rot"], S["t"], P0, preconditioner="two_level", trace=2000, **opts)[3]
    ctx.close()
    print(f"fixed rotations {fix}: default {a['final_cost']:.12e} ({a['status_name']}, {a['iters']} it, {a['pcg_iters']} PCG), two-level "
          f"{b['final_cost']:.12e} ({b['status_name']}, {b['iters']} it, {b['pcg_iters']} PCG, coarse fallbacks {b['coarse_fallbacks']}); first steps "
          f"{b['trace'][:4, 4].astype(int).tolist()} PCG, relative residuals {b['trace'][:4, 5].tolist()}")
    assert b["status"] in xmamd.BA_CONVERGED and np.all(b["trace"][:, 4] < PCG_CAP)
    assert b["trace"][0, 5] <= 1e-10                                              # the step with the dropped column is solved like any other
    assert 0 <= b["coarse_fallbacks"] <= b["iters"]
    assert abs(b["final_cost"] - a["final_cost"]) <= 1e-6 * a["final_cost"]


def test_a_coarse_operator_that_cannot_be_inverted_is_counted(xmamd):
    """The one input found that makes A_c lose definiteness: twelve cameras and fifteen of the landmarks only they see at ONE centre, so the
    depth of those landmarks is unobservable, V*_l = V_l + mu D_l loses its definiteness in floating point as mu falls, and S with it.  With
    fixed rotations A_c then fails its Cholesky factorisation in many LM iterations: each must run with the blocks alone and be counted,
    and the call must still return a finite, lower cost, the same one in a second call.  (No agreement with the default solver is asked
    for here: on this input eta = 1e-10 is out of reach of either.)"""
    rng = np.random.default_rng(95)
    yaw = np.linspace(-0.3, 0.3, 16)
    Cc = np.zeros((24, 3))
    Cc[16:] = np.stack([np.linspace(-3, 3, 8), np.full(8, -1.0), rng.uniform(-0.5, 0.5, 8)], axis=1)
    tgt = [np.array([6 * np.sin(y), 6 * np.cos(y), 0.0]) for y in yaw] + [np.array([0.0, 6.0, 0.0])] * 8
    Rcw = np.stack([ba._look_at(Cc[i], tgt[i], rng, 0.05) for i in range(24)])
    tcw = -np.einsum("iab,ib->ia", Rcw, Cc)
    m = 15 + 400
    Pw = np.stack([rng.uniform(-2, 2, m), rng.uniform(5, 7, m), rng.uniform(-1.5, 1.5, m)], axis=1)
    cams, lms = [], []
    for l in range(15):
        cams += [0, l + 1]; lms += [l, l]
    for l in range(15, m):
        s = np.concatenate([np.sort(rng.choice(16, 2, replace=False)), 16 + np.sort(rng.choice(8, 2, replace=False))])
        cams += list(s); lms += [l] * 4
    cams, lms = np.array(cams), np.array(lms)
    S = ba._pack(Rcw, tcw, Pw, cams, lms, ba._observe(Rcw, tcw, Pw, cams, lms, rng, 1e-3))
    P0 = S["P"] + 0.01 * np.random.default_rng(96).standard_normal(S["P"].shape)
    opts = dict(eta=1e-10, function_tol=1e-10, fix_rotations=True, preconditioner="two_level", trace=2000)
    ctx = _ctx(xmamd, S)
    r1 = ctx.bundle_adjust(S["rot"], S["t"], P0, **opts)
    r2 = ctx.bundle_adjust(S["rot"], S["t"], P0, **opts)
    ctx.close()
    b = r1[3]
    print(f"{b['status_name']}, {b['iters']} LM iterations, {b['pcg_iters']} PCG iterations, coarse fallbacks {b['coarse_fallbacks']}, cost "
          f"{b['initial_cost']:.6e} -> {b['final_cost']:.12e}")
    assert 1 <= b["coarse_fallbacks"] <= b["iters"] and b["coarse_fallbacks"] == r2[3]["coarse_fallbacks"]
    assert np.isfinite(b["final_cost"]) and b["final_cost"] < b["initial_cost"] and all(np.all(np.isfinite(x)) for x in r1[:3])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r1[:3], r2[:3])) and b["trace"].tobytes() == r2[3]["trace"].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_repeatable_and_leaves_the_context_unchanged(xmamd, kind):
    S = ba.ring_scene(n_cams=24, n_pts=250, seed=70, noise=2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=71)
    a, b = _ctx(xmamd, S), _ctx(xmamd, S)
    a.solve(5, 1e-8, 0.0); b.solve(5, 1e-8, 0.0)
    out1 = a.bundle_adjust(rot0, t0, P0, preconditioner=kind, trace=50)
    out2 = a.bundle_adjust(rot0, t0, P0, preconditioner=kind, trace=50)
    for x, y in zip(out1[:3], out2[:3]):
        assert x.tobytes() == y.tobytes()
    assert out1[3]["final_cost"] == out2[3]["final_cost"] and out1[3]["iters"] == out2[3]["iters"]
    assert out1[3]["trace"].tobytes() == out2[3]["trace"].tobytes() and out1[3]["pcg_iters"] == out2[3]["pcg_iters"]
    Ra2, sa2, ia = a.solve(5, 1e-8, 0.0)
    Rb2, sb2, ib = b.solve(5, 1e-8, 0.0)
    a.close(); b.close()
    assert Ra2.tobytes() == Rb2.tobytes() and sa2.tobytes() == sb2.tobytes() and ia["primal"] == ib["primal"]


def _raw(xmamd, ctx, n, m, flags):
    opt, res = xmamd.BaOptions(), xmamd.BaResult()
    opt.struct_size, res.struct_size = C.sizeof(opt), C.sizeof(res)
    opt.eta, opt.flags, opt.max_iters = 0.1, flags, 2
    rot = np.asfortranarray(np.tile(np.eye(3), (1, n))); t = np.zeros((3, n), order="F"); P = np.zeros((3, max(m, 1)), order="F")
    t[0] = 0.5 * np.arange(n); P[0] = 0.5 * np.arange(max(m, 1)); P[2] = 5.0
    rc = xmamd.lib().xm_ctx_bundle_adjust(ctx.h, C.byref(opt), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                          P.ctypes.data_as(C.c_void_p), C.byref(res))
    return rc, res


def test_refusals_leave_contexts_usable(xmamd):
    ERR_ARG = -2
    S = ba.ring_scene(n_cams=12, n_pts=80, seed=82, noise=1e-3)
    ctx = _ctx(xmamd, S)
    _, _, i0 = ctx.solve(5, 1e-8, 0.0)
    for flags in (xmamd.BA_PRECOND_TWO_LEVEL | xmamd.BA_PRECOND_BLOCKS, xmamd.BA_PRECOND_TWO_LEVEL | xmamd.BA_DENSE_SCHUR,
                  xmamd.BA_PRECOND_BLOCKS | xmamd.BA_DENSE_SCHUR):
        assert _raw(xmamd, ctx, S["n"], S["m"], flags)[0] == ERR_ARG, flags
    _, _, i1 = ctx.solve(5, 1e-8, 0.0)
    ctx.close()
    assert i0["status"] == i1["status"] == 1 and i0["primal"] == i1["primal"]
    # 65 537 cameras in a chain (camera i at (i / 2, 0, 0) sees landmarks i and i + 1 at depth 5): 4097 aggregates
    n = xmamd.BA_AGG_CAMS * xmamd.BA_MAX_AGGREGATES + 1
    cam = np.repeat(np.arange(n, dtype=np.int32), 2)
    lm = ((np.arange(2 * n) + 1) // 2).astype(np.int32)
    p = np.stack([0.5 * (lm - cam), np.zeros(2 * n), np.full(2 * n, 5.0)], axis=1)
    big = xmamd.Context(obs=(cam, lm, p, np.ones(2 * n)), n=n)
    for flags in (xmamd.BA_PRECOND_TWO_LEVEL, xmamd.BA_PRECOND_BLOCKS):
        assert _raw(xmamd, big, n, n + 1, flags)[0] == ERR_ARG
        assert "XM_BA_MAX_AGGREGATES" in xmamd.lib().xm_last_error().decode()
    rc, res = _raw(xmamd, big, n, n + 1, 0)                                        # the default preconditioner takes the same call
    big.close()
    assert rc == 0 and res.n_used == 2 * n and res.coarse_fallbacks == 0
