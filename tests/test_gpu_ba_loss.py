"""GPU tests of the robust losses and non-monotonic steps of xm_ctx_bundle_adjust and of xm_ctx_reprojection_errors
(xm-code_amd/csrc/xm_ba.hip) against the numpy restatement in xm_ba_loss_numpy.py (same losses, same Levenberg-Marquardt rules and step
evaluator, exact linear solves)."""
import ctypes as C

import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_ba_loss_numpy as rl
import xm_testlib as tl

pytestmark = pytest.mark.gpu

ERR_ARG = -2
A = 0.01          # loss scale of the outlier scenes: inliers have |r| <= 0.008, the injected outliers |r| >= 0.015


def _ctx(xmamd, S, **kw):
    return xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"], **kw)


def _obs(S):
    return S["cam"], S["lm"], S["p"], S["w"]


def _outliers():
    S, bad = rl.outlier_scene(n_cams=20, n_pts=200, seed=90, noise=2e-3, frac_out=0.05, out_size=0.3)
    return S, bad, ba.perturb(S["rot"], S["t"], S["P"], seed=91)


def _nonmonotonic_scene():
    # found on the CPU (test_ba_loss_abi.py::test_nonmonotonic_lm_returns_the_least_cost_point): steps 5 and 6 raise the cost by 1.2 % and
    # 1.8 % and are accepted against the reference cost; every step quality of the first 10 iterations lies in [0.9, 3.3]
    S, _ = rl.outlier_scene(n_cams=16, n_pts=150, seed=215, noise=5e-3, frac_out=0.1, out_size=0.5)
    return S, ba.perturb(S["rot"], S["t"], S["P"], seed=216, deg=40.0, rel=0.4)


def _relative_poses(rot, t):
    """gauge-free pose description (as test_gpu_ba.py): R_0^T R_i and R_0^T (t_i - t_0) normalised by their overall size"""
    n = t.shape[1]
    R0 = rot[:, :3]
    rr = np.stack([R0.T @ rot[:, 3 * i:3 * i + 3] for i in range(n)])
    tt = R0.T @ (t - t[:, :1])
    return rr, tt / np.linalg.norm(tt)


def _pose_error(rot, t, S):
    rr, tt = _relative_poses(rot, t)
    r0, t0 = _relative_poses(S["rot"], S["t"])
    return float(np.abs(rr - r0).max()), float(np.abs(tt - t0).max())


def _bits(*xs):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in xs)


@pytest.mark.parametrize("loss", ["huber", "soft_l1", "cauchy", "arctan"])
def test_robust_losses_reach_the_numpy_optimum(xmamd, loss):
    S, _, (rot0, t0, P0) = _outliers()
    opts = dict(function_tol=1e-10)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-6, loss=loss, loss_scale=A, **opts)
    ctx.close()
    _, _, _, ref = rl.lm(*_obs(S), rot0, t0, P0, loss=loss, a=A, **opts)
    print(f"{loss}: GPU {info['final_cost']:.12e} ({info['status_name']}, {info['iters']} it) numpy {ref['final_cost']:.12e} ({ref['iters']} it); "
          f"initial GPU {info['initial_cost']:.12e} numpy {ref['initial_cost']:.12e}")
    assert info["initial_cost"] == pytest.approx(ref["initial_cost"], rel=1e-12)
    assert info["status"] == ref["status"]
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]


def test_robust_loss_on_heavy_landmarks(xmamd):
    S, _ = rl.outlier_scene(n_cams=72, n_pts=120, seed=60, noise=2e-3, frac=0.93, frac_out=0.05, out_size=0.3)
    deg = np.bincount(S["lm"])
    assert (deg > 64).sum() > 10 and (deg <= 64).sum() > 0          # heavy landmarks (a workgroup each) and light ones
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=61)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-6, function_tol=1e-10, loss="huber", loss_scale=A)
    ctx.close()
    _, _, _, ref = rl.lm(*_obs(S), rot0, t0, P0, loss="huber", a=A, function_tol=1e-10)
    print(f"heavy huber: GPU {info['final_cost']:.12e} ({info['status_name']}) numpy {ref['final_cost']:.12e}")
    assert info["status"] == ref["status"] and abs(info["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]


def test_robust_loss_with_fixed_rotations(xmamd):
    S, _, (rot0, t0, P0) = _outliers()
    ctx = _ctx(xmamd, S)
    rot, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-6, function_tol=1e-10, loss="cauchy", loss_scale=A, fix_rotations=True)
    ctx.close()
    _, _, _, ref = rl.lm(*_obs(S), rot0, t0, P0, loss="cauchy", a=A, function_tol=1e-10, fix_rotations=True)
    print(f"fixed rotations, cauchy: GPU {info['final_cost']:.12e} ({info['status_name']}) numpy {ref['final_cost']:.12e}")
    assert rot.tobytes() == np.asfortranarray(rot0).tobytes()
    assert info["status"] == ref["status"] and abs(info["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]


def test_robust_losses_keep_the_outliers_off_the_poses(xmamd):
    # measured with the numpy restatement on this scene (111 of 1964 observations moved by up to 0.3): largest pose error (rotation
    # entries, normalised translation) trivial 0.158 / 0.0228, Huber 0.0137 / 0.00206, Cauchy 0.0093 / 0.00144
    S, bad, (rot0, t0, P0) = _outliers()
    ctx = _ctx(xmamd, S)
    err = {}
    for loss, a in (("trivial", 0.0), ("huber", A), ("cauchy", A)):
        rot, t, _, info = ctx.bundle_adjust(rot0, t0, P0, loss=loss, loss_scale=a)
        err[loss] = _pose_error(rot, t, S)
        print(f"{loss}: pose error {err[loss][0]:.4e} (rotations) {err[loss][1]:.4e} (translations), cost {info['final_cost']:.6e}")
    ctx.close()
    assert err["trivial"][0] > 0.1
    for loss in ("huber", "cauchy"):
        assert err[loss][0] < 0.25 * err["trivial"][0] and err[loss][1] < 0.25 * err["trivial"][1]


def _raw(xmamd, ctx, rot, t, P, struct_size=None, trace=0, **fields):
    """xm_ctx_bundle_adjust through a BaOptions filled by hand -> (rc, rot, t, P, result, trace)"""
    opt, res = xmamd.BaOptions(), xmamd.BaResult()
    opt.struct_size = C.sizeof(opt) if struct_size is None else struct_size
    res.struct_size = C.sizeof(res)
    opt.eta = 0.1
    for k, v in fields.items():
        setattr(opt, k, v)
    tr = np.zeros((max(trace, 1), 6))
    if trace:
        opt.trace_cap, opt.trace = trace, tr.ctypes.data_as(C.c_void_p)
    rot = np.array(rot, dtype=np.float64, order="F"); t = np.array(t, dtype=np.float64, order="F"); P = np.array(P, dtype=np.float64, order="F")
    rc = xmamd.lib().xm_ctx_bundle_adjust(ctx.h, C.byref(opt), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                          P.ctypes.data_as(C.c_void_p), C.byref(res))
    return rc, rot, t, P, res, tr[:res.trace_len].copy()


def test_trivial_defaults_are_unchanged(xmamd):
    S, _, (rot0, t0, P0) = _outliers()
    ctx = _ctx(xmamd, S)
    a = ctx.bundle_adjust(rot0, t0, P0, trace=50)
    b = ctx.bundle_adjust(rot0, t0, P0, trace=50, loss="trivial", loss_scale=0.0, nonmonotonic=False, max_nonmonotonic=0)
    assert _bits(*a[:3], a[3]["trace"]) == _bits(*b[:3], b[3]["trace"]) and a[3]["final_cost"] == b[3]["final_cost"]
    # a caller of the first version of the struct (64 bytes): what lies behind trace is not read, the run is the new struct's with zeros
    rc1, *o1, r1, tr1 = _raw(xmamd, ctx, rot0, t0, P0, trace=50)
    rc2, *o2, r2, tr2 = _raw(xmamd, ctx, rot0, t0, P0, trace=50, struct_size=xmamd.BA_OPTIONS_SIZE_V1, loss=99, max_nonmonotonic=-3,
                             loss_scale=float("nan"))
    assert rc1 == rc2 == 0
    assert _bits(*o1, tr1) == _bits(*o2, tr2) and r1.final_cost == r2.final_cost and r1.iters == r2.iters
    assert _bits(*o1, tr1) == _bits(*a[:3], a[3]["trace"])
    # Huber with a scale above every residual of the run is the trivial loss
    h = ctx.bundle_adjust(rot0, t0, P0, trace=50, loss="huber", loss_scale=1e3)
    ctx.close()
    print(f"trivial {a[3]['final_cost']:.17e} ({a[3]['iters']} it), huber(1e3) {h[3]['final_cost']:.17e} ({h[3]['iters']} it)")
    assert np.array_equal(h[3]["trace"][:, 3], a[3]["trace"][:, 3])
    assert abs(h[3]["final_cost"] - a[3]["final_cost"]) <= 1e-13 * a[3]["final_cost"]


def test_nonmonotonic_steps_follow_the_numpy_evaluator(xmamd):
    S, (rot0, t0, P0) = _nonmonotonic_scene()
    opts = dict(function_tol=1e-12, max_iters=10)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, nonmonotonic=True, trace=20, **opts)
    _, _, _, ref = rl.lm(*_obs(S), rot0, t0, P0, nonmonotonic=True, **opts)
    g, gr = info["trace"], ref["trace"]
    print("GPU trace\n", g, "\nnumpy trace\n", gr)
    assert g.shape[0] == gr.shape[0] == 10
    assert np.array_equal(g[:, 3], gr[:, 3])
    assert np.any((g[:, 3] == 1) & (g[:, 1] > g[:, 0]))                                 # an accepted step that raised the cost
    assert np.allclose(g[:, :2], gr[:, :2], rtol=1e-7, atol=0)       # the last steps are almost Gauss-Newton: PCG and exact solve drift apart
    # stopped after 6 iterations the current point (after a step up) is not the least-cost one: that one comes back
    rot, t, P, info6 = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, nonmonotonic=True, trace=20, function_tol=1e-12, max_iters=6)
    g6 = info6["trace"]
    costs = np.concatenate([g6[:, 0], g6[g6[:, 3] == 1, 1]])
    sq = ctx.reprojection_errors(rot, t, P)
    ctx.close()
    F_out = 0.5 * float(np.sum(sq[sq >= 0]))
    print(f"6 iterations: final cost {info6['final_cost']:.17e}, least in the trace {costs.min():.17e}, last current {g6[-1, 0]:.17e}, "
          f"at the returned point {F_out:.17e}")
    assert costs.min() < g6[-1, 0] and g6[-1, 3] == 1
    assert info6["final_cost"] == pytest.approx(costs.min(), rel=1e-13)
    assert F_out == pytest.approx(info6["final_cost"], rel=1e-12)


def test_reprojection_errors(xmamd):
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=100, noise=5e-3)
    n, m = S["n"], S["m"]
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=101)
    # plus camera n and landmark m seen only behind the camera (p2 < 0), and landmark m + 1 seen once with its weight set to 0
    E = dict(S)
    E["cam"] = np.concatenate([S["cam"], [n, 0, 1]]).astype(np.int32)
    E["lm"] = np.concatenate([S["lm"], [m, m, m + 1]]).astype(np.int32)
    E["p"] = np.concatenate([S["p"], [[0.1, 0.2, -3.0], [0.2, 0.1, -2.0], [0.1, -0.1, 4.0]]])
    E["w"] = np.ones(E["cam"].size)
    E["n"], E["m"] = n + 1, m + 2
    w_set = E["w"].copy(); w_set[-1] = 0.0; w_set[5] = 0.0
    rotE = np.concatenate([rot0, np.eye(3)], axis=1)
    tE = np.concatenate([t0, [[0.3], [-0.7], [1.1]]], axis=1)
    PE = np.concatenate([P0, [[0.5, -0.25], [0.125, 0.75], [-1.5, 2.0]]], axis=1)
    ctx, ref_ctx = _ctx(xmamd, E), _ctx(xmamd, E)
    for c in (ctx, ref_ctx):
        c.set_edge_weights(w_set)
    s1 = ctx.reprojection_errors(rotE, tE, PE)
    s2 = ctx.reprojection_errors(rotE, tE, PE)
    s_np = rl.sq_errors(E["cam"], E["lm"], E["p"], w_set, rotE, tE, PE)
    off = np.nonzero(s_np < 0)[0]
    print(f"{s1.size} observations, unused {off.tolist()}, |s| in [{s1[s1 >= 0].min():.3e}, {s1.max():.3e}], "
          f"max relative difference to numpy {np.max(np.abs(s1 - s_np)[s_np >= 0] / s_np[s_np >= 0]):.3e}")
    assert s1.tobytes() == s2.tobytes()
    assert off.tolist() == [5, E["cam"].size - 3, E["cam"].size - 2, E["cam"].size - 1]
    assert np.all(s1[off] == -1.0) and np.all(s1[s_np >= 0] >= 0)
    assert np.all(np.abs(s1 - s_np)[s_np >= 0] <= 1e-12 * s_np[s_np >= 0])
    # the context is unchanged: an adjustment and a solve afterwards give the bits of a context that never computed the errors
    out1 = ctx.bundle_adjust(rotE, tE, PE, loss="huber", loss_scale=A)
    out2 = ref_ctx.bundle_adjust(rotE, tE, PE, loss="huber", loss_scale=A)
    assert _bits(*out1[:3]) == _bits(*out2[:3]) and out1[3]["final_cost"] == out2[3]["final_cost"]
    R1, s_1, i1 = ctx.solve(5, 1e-8, 0.0)
    R2, s_2, i2 = ref_ctx.solve(5, 1e-8, 0.0)
    ctx.close(); ref_ctx.close()
    assert R1.tobytes() == R2.tobytes() and s_1.tobytes() == s_2.tobytes() and i1["primal"] == i2["primal"]


def test_refusals_and_repeatability(xmamd):
    S, (rot0, t0, P0) = _nonmonotonic_scene()
    ctx = _ctx(xmamd, S)
    _, _, i0 = ctx.solve(5, 1e-8, 0.0)
    nan, inf = float("nan"), float("inf")
    bad = [dict(loss=5), dict(loss=-1), dict(loss=1, loss_scale=0.0), dict(loss=2, loss_scale=-0.1), dict(loss=3, loss_scale=nan),
           dict(loss=4, loss_scale=inf), dict(loss=0, loss_scale=0.5), dict(loss=1, loss_scale=A, max_nonmonotonic=-1),
           dict(max_nonmonotonic=-2), dict(flags=4), dict(flags=8 | xmamd.BA_NONMONOTONIC), dict(struct_size=8),
           dict(struct_size=C.sizeof(xmamd.BaOptions) - 8)]
    for kw in bad:
        rc = _raw(xmamd, ctx, rot0, t0, P0, **kw)[0]
        assert rc == ERR_ARG, (kw, xmamd.lib().xm_last_error())
    with pytest.raises(xmamd.XmError):
        ctx.bundle_adjust(rot0, t0, P0, loss="tukey", loss_scale=A)
    _, _, i1 = ctx.solve(5, 1e-8, 0.0)
    assert i0["status"] == i1["status"] == 1 and i0["primal"] == i1["primal"]
    o1 = ctx.bundle_adjust(rot0, t0, P0, loss="cauchy", loss_scale=A, nonmonotonic=True, max_nonmonotonic=3, trace=100)
    o2 = ctx.bundle_adjust(rot0, t0, P0, loss="cauchy", loss_scale=A, nonmonotonic=True, max_nonmonotonic=3, trace=100)
    ctx.close()
    print(f"cauchy, non-monotonic: cost {o1[3]['initial_cost']:.6e} -> {o1[3]['final_cost']:.6e}, {o1[3]['iters']} it, {o1[3]['status_name']}")
    assert _bits(*o1[:3], o1[3]["trace"]) == _bits(*o2[:3], o2[3]["trace"]) and o1[3]["final_cost"] == o2[3]["final_cost"]
    assert o1[3]["final_cost"] < o1[3]["initial_cost"]
    # the other storages have no landmarks: refused, context usable
    V = tl.gen_vg(40, deg=6, sigma=0.05, seed=80)
    d = xmamd.Context(Q=V["Q"])
    z = np.zeros((3, 40), order="F")
    rc = xmamd.lib().xm_ctx_reprojection_errors(d.h, np.asfortranarray(np.tile(np.eye(3), (1, 40))).ctypes.data_as(C.c_void_p),
                                                z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p))
    assert rc == ERR_ARG and "XM_STORAGE_SCHUR" in xmamd.lib().xm_last_error().decode()
    _, _, info = d.solve(5, 1e-8, 0.0)
    d.close()
    assert info["status"] == 1
