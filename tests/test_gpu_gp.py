"""GPU tests of the global positioning (xm_ctx_global_positioning, xm-code_amd/csrc/xm_gp.hip) against the numpy restatement in
xm_gp_numpy.py (same problem, same Levenberg-Marquardt rules, same active-set rule, exact linear solves).  Nothing here was compared with
the reference's compiled code."""
import ctypes as C

import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_gp_numpy as gp
import xm_testlib as tl

pytestmark = pytest.mark.gpu

TIGHT = dict(gradient_tol=1e-14, parameter_tol=1e-16)          # test_gpu_ba.py


def _ctx(xmamd, S, **kw):
    return xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"], **kw)


def _obs(S, w=None):
    return S["cam"], S["lm"], S["p"], S["w"] if w is None else w


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_free_scene_is_recovered_from_a_random_start(xmamd, seed):
    S = ba.ring_scene(n_cams=8, n_pts=40, seed=0)
    ctx = _ctx(xmamd, S)
    t, P, info = ctx.global_positioning(S["rot"], seed=seed, **TIGHT)
    ctx.close()
    err = gp.recovery_error(S, t, P)
    print(f"start {seed}: {info['iters']} iterations ({info['accepted']} accepted), {info['pcg_iters']} PCG, cost {info['initial_cost']:.3e} -> "
          f"{info['final_cost']:.3e}, status {info['status_name']}, recovery error {err:.2e}")
    t0, P0 = xmamd.gp_random_start(S["n"], S["m"], seed)
    assert np.isclose(info["initial_cost"], gp.lm(*_obs(S), S["rot"], t0, P0, max_iters=0)[2]["initial_cost"], rtol=1e-12)
    assert info["n_used"] == S["cam"].size and info["final_cost"] < 1e-20 and err < 1e-8
    assert info["scales"].shape == (S["cam"].size,) and info["scales"].min() > gp.S_MIN


def test_trace_follows_the_numpy_lm(xmamd):
    # Noisy bearings (the scene of test_gpu_ba.py's trace test): all of the first 10 iterations are accepted and change the cost by more
    # than 8e-6 of it.  With the gauge free and mu falling to 1e-8 the damped system is ill-conditioned, so the scene is chosen for a
    # restatement that is itself stable: solved with a dense instead of the sparse factorisation its first 10 costs move by 1.5e-10
    # (measured; 6e-10 on the 12 x 80 scene with random bearings, which is too close to the bound to judge a kernel on)
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=0.05)
    t0, P0 = xmamd.gp_random_start(S["n"], S["m"], 1)
    ctx = _ctx(xmamd, S)
    _, _, info = ctx.global_positioning(S["rot"], t0, P0, eta=1e-12, function_tol=1e-14, max_iters=10, trace=20)
    ctx.close()
    _, _, ref = gp.lm(*_obs(S), S["rot"], t0, P0, function_tol=1e-14, max_iters=10)
    g, gr = info["trace"], ref["trace"]
    print("GPU trace\n", g, "\nnumpy trace\n", gr)
    assert g.shape[0] == gr.shape[0] == 10
    print("relative differences (cost, candidate cost, mu)\n", np.abs(g[:, :3] - gr[:, :3]) / np.abs(gr[:, :3]))
    assert np.array_equal(g[:, 3], gr[:, 3])                                            # the same accept / reject sequence
    assert np.allclose(g[:, 0], gr[:, 0], rtol=1e-9, atol=0) and np.allclose(g[:, 1], gr[:, 1], rtol=1e-9, atol=0)
    assert np.allclose(g[:, 2], gr[:, 2], rtol=1e-6, atol=0)                           # mu follows rho, a ratio of cost differences
    assert np.all(g[:, 5] <= 1e-12)                                                     # each PCG reached eta


def test_default_eta_reaches_the_numpy_optimum(xmamd):
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=2e-3)
    t0, P0 = xmamd.gp_random_start(S["n"], S["m"], 2)
    ctx = _ctx(xmamd, S)
    t, P, info = ctx.global_positioning(S["rot"], t0, P0, function_tol=1e-10)
    ctx.close()
    _, _, ref = gp.lm(*_obs(S), S["rot"], t0, P0, function_tol=1e-10)
    print(f"GPU {info['final_cost']:.12e} ({info['status_name']}, {info['iters']} it, {info['pcg_iters']} PCG) numpy {ref['final_cost']:.12e} "
          f"({ref['iters']} it); recovery error {gp.recovery_error(S, t, P):.2e}")
    assert info["status"] in xmamd.BA_CONVERGED
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]


def _extended(S, t0, P0):
    """the scene plus: camera n and landmark m seen only behind the camera (p2 < 0), landmark m + 1 with two observations (below
    min_views), landmark m + 2 with three of which one gets weight 0 afterwards"""
    n, m = S["n"], S["m"]
    E = dict(S)
    E["cam"] = np.concatenate([S["cam"], [n, 0, 1, 0, 1, 2, 3, 4]]).astype(np.int32)
    E["lm"] = np.concatenate([S["lm"], [m, m, m, m + 1, m + 1, m + 2, m + 2, m + 2]]).astype(np.int32)
    E["p"] = np.concatenate([S["p"], [[0.1, 0.2, -3.0], [0.2, 0.1, -2.0], [0.0, 0.1, -2.5], [0.1, -0.1, 4.0], [0.3, 0.2, 5.0], [0.1, 0.0, 6.0],
                                      [-0.2, 0.1, 6.0], [0.0, 0.2, 7.0]]])
    E["w"] = np.ones(E["cam"].size)
    E["n"], E["m"] = n + 1, m + 3
    w_set = E["w"].copy(); w_set[-1] = 0.0
    rotE = np.concatenate([S["rot"], np.eye(3)], axis=1)
    tE = np.concatenate([t0, [[0.3], [-0.7], [1.1]]], axis=1)
    PE = np.concatenate([P0, [[0.5, -0.25, 3.0], [0.125, 0.75, -1.0], [-1.5, 2.0, 0.5]]], axis=1)
    return E, w_set, rotE, tE, PE


def test_unused_cameras_landmarks_and_scales_come_back_bit_identical(xmamd):
    S = ba.ring_scene(n_cams=12, n_pts=80, seed=50, noise=2e-3)
    n, m, k = S["n"], S["m"], S["cam"].size
    t0, P0 = xmamd.gp_random_start(n, m, 5)
    E, w_set, rotE, tE, PE = _extended(S, t0, P0)
    opts = dict(eta=1e-6, function_tol=1e-10)
    ctx = _ctx(xmamd, S)
    t, P, info = ctx.global_positioning(S["rot"], t0, P0, **opts)
    ctx.close()
    ctxE = _ctx(xmamd, E)
    ctxE.set_edge_weights(w_set)
    t2, P2, info2 = ctxE.global_positioning(rotE, tE, PE, **opts)
    ctxE.close()
    print(f"base {info['final_cost']:.15e} ({info['iters']} it), extended {info2['final_cost']:.15e} ({info2['iters']} it)")
    assert info["n_used"] == k and info2["n_used"] == k
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    assert rel(t2[:, :n], t) <= 1e-9 and rel(P2[:, :m], P) <= 1e-9 and rel(info2["scales"][:k], info["scales"]) <= 1e-9
    assert t2[:, n:].tobytes() == np.ascontiguousarray(tE[:, n:]).tobytes()
    assert P2[:, m:].tobytes() == np.ascontiguousarray(PE[:, m:]).tobytes()
    assert np.all(info2["scales"][k:] == -1.0) and np.all(info2["scales"][:k] > 0)


def test_repeatable_and_leaves_the_context_unchanged(xmamd):
    S = ba.ring_scene(n_cams=16, n_pts=150, seed=70, noise=2e-3)
    a, b = _ctx(xmamd, S), _ctx(xmamd, S)
    out1 = a.global_positioning(S["rot"], seed=4)
    out2 = a.global_positioning(S["rot"], seed=4)
    for x, y in zip(out1[:2], out2[:2]):
        assert x.tobytes() == y.tobytes()
    assert out1[2]["scales"].tobytes() == out2[2]["scales"].tobytes()
    assert out1[2]["final_cost"] == out2[2]["final_cost"] and out1[2]["iters"] == out2[2]["iters"] and out1[2]["pcg_iters"] == out2[2]["pcg_iters"]
    Ra, sa, ia = a.solve(5, 1e-8, 0.0)                         # after two calls: the bits of a context that never made one
    Rb, sb, ib = b.solve(5, 1e-8, 0.0)
    a.close(); b.close()
    assert Ra.tobytes() == Rb.tobytes() and sa.tobytes() == sb.tobytes() and ia["primal"] == ib["primal"]


def _raw(xmamd, ctx, n, m, eta=0.1, struct_size=None, nan=False, loss=1, loss_scale=0.1, min_views=0, null=None, res_size=None, trace_cap=0,
         huge=None, ret=False, **settings):
    """one raw call; null: the argument passed as NULL (opt, rot, t, p, res); huge: "t" or "p" scaled to 1e200 (finite input, an infinite
    initial cost); settings: other fields of xm_gp_options_t.  ret: also the arrays before and after the call"""
    opt, res = xmamd.GpOptions(), xmamd.GpResult()
    opt.struct_size = C.sizeof(opt) if struct_size is None else struct_size
    res.struct_size = C.sizeof(res) if res_size is None else res_size
    opt.eta, opt.loss, opt.loss_scale, opt.min_views, opt.trace_cap = eta, loss, loss_scale, min_views, trace_cap
    for k, v in settings.items():
        setattr(opt, k, v)
    rot = np.asfortranarray(np.tile(np.eye(3), (1, n)))
    t, P = xmamd.gp_random_start(n, max(m, 1), 1)
    t, P = np.asfortranarray(t), np.asfortranarray(P)
    if nan:
        P[0, 0] = np.nan
    if huge == "t":
        t *= 1e198
    if huge == "p":
        P *= 1e198
    before = (t.copy(order="F"), P.copy(order="F"))
    ptr = dict(opt=C.byref(opt), rot=rot.ctypes.data_as(C.c_void_p), t=t.ctypes.data_as(C.c_void_p), p=P.ctypes.data_as(C.c_void_p), res=C.byref(res))
    if null:
        ptr[null] = None
    rc = xmamd.lib().xm_ctx_global_positioning(ctx.h, ptr["opt"], ptr["rot"], ptr["t"], ptr["p"], None, ptr["res"])
    return (rc, before, (t, P)) if ret else rc


def test_refusals_leave_contexts_usable(xmamd):
    ERR_ARG = -2
    V = tl.gen_vg(40, deg=6, sigma=0.05, seed=80)
    e, _ = tl.gen_vg_edges(40, 6, 81)
    Mv = np.tile(np.eye(3).reshape(1, 9), (e.shape[0], 1))
    ctxs = [xmamd.Context(Q=V["Q"]), xmamd.Context(bsr=(V["rowptr"], V["colidx"], V["blocks"])),
            xmamd.Context(vg=(e[:, 0].astype(np.int32), e[:, 1].astype(np.int32), np.ones(e.shape[0]), Mv), n=40)]
    for c in ctxs:
        assert _raw(xmamd, c, c.n, 1) == ERR_ARG
        assert "XM_STORAGE_SCHUR" in xmamd.lib().xm_last_error().decode()
        _, _, info = c.solve(5, 1e-8, 0.0)
        assert info["status"] == 1
        c.close()
    S = ba.ring_scene(n_cams=12, n_pts=80, seed=82, noise=1e-3)
    two = _ctx(xmamd, S, n_gpus=2, gpu_map=1)
    assert _raw(xmamd, two, S["n"], S["m"]) == ERR_ARG
    _, _, i2 = two.solve(5, 1e-8, 0.0)
    two.close()
    ctx, twin = _ctx(xmamd, S), _ctx(xmamd, S)
    R0, s0, i0 = ctx.solve(5, 1e-8, 0.0)
    for kw in (dict(struct_size=8), dict(res_size=8), dict(nan=True), dict(eta=0.0), dict(eta=1.0), dict(eta=np.nan), dict(loss=7), dict(loss=-1),
               dict(loss=0, loss_scale=0.1), dict(loss=1, loss_scale=0.0), dict(loss=1, loss_scale=-0.1), dict(loss=1, loss_scale=np.inf),
               dict(min_views=-1), dict(max_iters=-1), dict(max_time=-1.0), dict(max_time=np.inf), dict(function_tol=-1e-6),
               dict(gradient_tol=-1e-10), dict(parameter_tol=-1e-8), dict(parameter_tol=np.nan), dict(trace_cap=-1), dict(trace_cap=4),
               dict(null="opt"), dict(null="rot"), dict(null="t"), dict(null="p"), dict(null="res")):
        assert _raw(xmamd, ctx, S["n"], S["m"], **kw) == ERR_ARG, kw
    # finite input whose initial cost is infinite (|r|^2 overflows): refused from inside the call, after the workspace is made and
    # kernels have run -- t and p keep their bits and the context is as it was
    for loss, a in ((1, 0.1), (0, 0.0), (3, 0.1)):
        for which in ("t", "p"):
            rc, before, after = _raw(xmamd, ctx, S["n"], S["m"], loss=loss, loss_scale=a, huge=which, ret=True)
            assert rc == ERR_ARG and "initial cost is not finite" in xmamd.lib().xm_last_error().decode(), (loss, which)
            assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    assert _raw(xmamd, ctx, S["n"], S["m"]) == 0                # the same call without a fault is accepted
    R1, s1, i1 = ctx.solve(5, 1e-8, 0.0)
    Rt, st_, it = twin.solve(5, 1e-8, 0.0)
    Rt, st_, it = twin.solve(5, 1e-8, 0.0)                      # the twin never saw a refusal: its second solve has the same bits
    ctx.close(); twin.close()
    assert i0["status"] == i1["status"] == i2["status"] == 1 and i0["primal"] == i1["primal"]
    assert R1.tobytes() == Rt.tobytes() and s1.tobytes() == st_.tobytes() and i1["primal"] == it["primal"]


def _raw_probe(xmamd, ctx, S, mu=1.0, struct_size=None, k=0, X=None, s=None, dc=None, loss=1, loss_scale=0.1, min_views=3, null=None, nan_t=False):
    q = xmamd.GpProbe()
    q.struct_size = C.sizeof(q) if struct_size is None else struct_size
    q.mu, q.k, q.loss, q.loss_scale, q.min_views = mu, k, loss, loss_scale, min_views
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (X, s, dc) if a is not None]
    for name, a in (("X", X), ("s", s), ("dc", dc)):
        if a is not None:
            setattr(q, name, keep.pop(0).ctypes.data_as(C.c_void_p))
    rot = np.asfortranarray(S["rot"]); t = np.asfortranarray(S["t"]).copy(order="F"); P = np.asfortranarray(S["P"])
    if nan_t:
        t[1, 2] = np.inf
    ptr = dict(rot=rot.ctypes.data_as(C.c_void_p), t=t.ctypes.data_as(C.c_void_p), p=P.ctypes.data_as(C.c_void_p), probe=C.byref(q))
    if null:
        ptr[null] = None
    return xmamd.lib().xm_ctx_gp_probe(ctx.h, ptr["rot"], ptr["t"], ptr["p"], ptr["probe"]), q


def test_probe_refusals_leave_the_context_usable(xmamd):
    ERR_ARG = -2
    S = ba.ring_scene(n_cams=8, n_pts=40, seed=0, noise=1e-3)
    n, nobs = S["n"], S["cam"].size
    ctx, twin = _ctx(xmamd, S), _ctx(xmamd, S)
    bad = np.ones(3 * n); bad[4] = np.nan
    bad_s = np.ones(nobs); bad_s[-1] = np.inf
    for kw in (dict(struct_size=16), dict(mu=0.0), dict(mu=-1.0), dict(mu=np.inf), dict(mu=np.nan), dict(k=1), dict(k=-1), dict(k=1, X=bad),
               dict(s=bad_s), dict(dc=bad), dict(loss=9), dict(loss=0, loss_scale=0.1), dict(loss=2, loss_scale=0.0), dict(min_views=-2),
               dict(nan_t=True), dict(null="rot"), dict(null="t"), dict(null="p"), dict(null="probe")):
        assert _raw_probe(xmamd, ctx, S, **kw)[0] == ERR_ARG, kw
    V = tl.gen_vg(20, deg=4, sigma=0.05, seed=83)
    other = xmamd.Context(Q=V["Q"])
    assert _raw_probe(xmamd, other, dict(S, rot=np.tile(np.eye(3), (1, 20)), t=np.zeros((3, 20)), P=np.zeros((3, 1))))[0] == ERR_ARG
    assert "XM_STORAGE_SCHUR" in xmamd.lib().xm_last_error().decode()
    other.close()
    rc, q = _raw_probe(xmamd, ctx, S, k=1, X=np.ones(3 * n), s=np.ones(nobs), dc=np.zeros(3 * n))     # the same call without a fault
    assert rc == 0 and q.n_used == nobs and q.cost > 0 and np.isfinite(q.cost1)
    Ra, sa, ia = ctx.solve(5, 1e-8, 0.0)
    Rb, sb, ib = twin.solve(5, 1e-8, 0.0)
    ctx.close(); twin.close()
    assert Ra.tobytes() == Rb.tobytes() and sa.tobytes() == sb.tobytes() and ia["primal"] == ib["primal"]
