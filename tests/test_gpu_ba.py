"""GPU tests of the reprojection bundle adjustment (xm_ctx_bundle_adjust, xm-code_amd/csrc/xm_ba.hip) against the numpy restatement in
xm_ba_numpy.py (same problem, same Levenberg-Marquardt rules, exact linear solves)."""
import ctypes as C
import os

import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_testlib as tl

pytestmark = pytest.mark.gpu

TIGHT = dict(gradient_tol=1e-14, parameter_tol=1e-16)


def _ctx(xmamd, S, w=None, **kw):
    return xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"] if w is None else w), n=S["n"], **kw)


def _obs(S, w=None):
    return S["cam"], S["lm"], S["p"], S["w"] if w is None else w


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _relative_poses(rot, t):
    """gauge-free pose description: R_0^T R_i and R_0^T (t_i - t_0) normalised by their overall size"""
    n = t.shape[1]
    R0 = rot[:, :3]
    rr = np.stack([R0.T @ rot[:, 3 * i:3 * i + 3] for i in range(n)])
    tt = R0.T @ (t - t[:, :1])
    return rr, tt / np.linalg.norm(tt)


def test_noise_free_scene_is_solved_exactly(xmamd):
    S = ba.ring_scene(n_cams=30, n_pts=400, seed=10)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=11, deg=2.0, rel=0.01)
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0, **TIGHT)
    ctx.close()
    rms = np.sqrt(info["final_cost"] / info["n_used"])          # F = 1/2 sum |r|^2 over 2 n_used components
    F_np, _ = ba.reprojection_cost(*_obs(S), rot, t, P)
    print(f"noise-free: {info['iters']} iterations ({info['accepted']} accepted), {info['pcg_iters']} PCG, cost {info['initial_cost']:.3e} -> "
          f"{info['final_cost']:.3e} (numpy at the output {F_np:.3e}), status {info['status_name']}")
    assert rms <= 1e-10 and np.sqrt(F_np / info["n_used"]) <= 1e-10
    rr, tt = _relative_poses(rot, t)
    rr0, tt0 = _relative_poses(S["rot"], S["t"])
    assert np.abs(rr - rr0).max() < 1e-8 and np.abs(tt - tt0).max() < 1e-8


def test_trace_follows_the_numpy_lm(xmamd):
    # noisy observations and a start far away (40 degrees, 40 % of the scene): the first 10 iterations all change the cost by more than 1e-8
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=0.05)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=21, deg=40.0, rel=0.4)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, function_tol=1e-12, max_iters=10, trace=20)
    ctx.close()
    _, _, _, ref = ba.lm(*_obs(S), rot0, t0, P0, function_tol=1e-12, max_iters=10)
    g, gr = info["trace"], ref["trace"]
    print("GPU trace\n", g, "\nnumpy trace\n", gr)
    assert g.shape[0] == gr.shape[0] == 10
    assert np.array_equal(g[:, 3], gr[:, 3])                                            # the same accept / reject sequence
    assert np.allclose(g[:, 0], gr[:, 0], rtol=1e-9, atol=0) and np.allclose(g[:, 1], gr[:, 1], rtol=1e-9, atol=0)
    assert np.allclose(g[:, 2], gr[:, 2], rtol=1e-6, atol=0)                           # mu follows rho, a ratio of cost differences
    assert np.all(g[:, 5] <= 1e-12)                                                     # each PCG reached eta


def test_stationary_point_by_the_numpy_jacobian(xmamd):
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=22, noise=2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=23, deg=10.0, rel=0.1)
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-12, function_tol=1e-12)
    ctx.close()
    g0 = np.abs(ba.gradient_at(*_obs(S), rot0, t0, P0)).max()
    g1 = np.abs(ba.gradient_at(*_obs(S), rot, t, P)).max()
    print(f"|J^T r|_inf {g0:.3e} -> {g1:.3e} (GPU {info['gradient_max']:.3e}), status {info['status_name']}, {info['iters']} iterations")
    assert g1 <= 1e-8 * g0 and info["status"] in xmamd.BA_CONVERGED


def test_default_eta_reaches_the_numpy_optimum(xmamd):
    S = ba.ring_scene(n_cams=24, n_pts=300, seed=30, noise=2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=31)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0)
    ctx.close()
    _, _, _, ref = ba.lm(*_obs(S), rot0, t0, P0)
    print(f"GPU {info['final_cost']:.12e} ({info['status_name']}, {info['iters']} it, {info['pcg_iters']} PCG) numpy {ref['final_cost']:.12e}")
    assert info["status"] in xmamd.BA_CONVERGED
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]


def test_fixed_rotations(xmamd):
    S = ba.ring_scene(n_cams=16, n_pts=150, seed=40, noise=2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=41)
    ctx = _ctx(xmamd, S)
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0, fix_rotations=True, eta=1e-10, function_tol=1e-14, parameter_tol=1e-14)
    ctx.close()
    assert np.array_equal(rot, rot0) and rot.tobytes() == np.asfortranarray(rot0).tobytes()
    g0 = np.abs(ba.gradient_at(*_obs(S), rot0, t0, P0, fix_rotations=True)).max()
    g1 = np.abs(ba.gradient_at(*_obs(S), rot, t, P, fix_rotations=True)).max()
    print(f"fixed rotations: cost {info['initial_cost']:.3e} -> {info['final_cost']:.3e}, |g| {g0:.3e} -> {g1:.3e}")
    assert g1 <= 1e-8 * g0 and info["final_cost"] < info["initial_cost"]


def test_masked_observations_change_nothing(xmamd):
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=50, noise=2e-3, min_views=3)
    n, m = S["n"], S["m"]
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=51)
    # the same scene plus: camera n and landmark m seen only behind the camera (p2 < 0, weight 1 so that the XM problem stays connected), and
    # landmark m + 1 seen once with its weight set to 0 afterwards
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
    opts = dict(eta=1e-6, function_tol=1e-10)
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
    # never used: bit-identical
    assert rot2[:, 3 * n:].tobytes() == np.asfortranarray(rotE[:, 3 * n:]).tobytes()
    assert t2[:, n:].tobytes() == np.ascontiguousarray(tE[:, n:]).tobytes() and np.array_equal(P2[:, m:], PE[:, m:])
    assert P2[:, m:].tobytes() == np.ascontiguousarray(PE[:, m:]).tobytes()


@pytest.mark.parametrize("kind", ["heavy", "sequential"])
def test_harder_scenes_reach_the_numpy_optimum(xmamd, kind):
    if kind == "heavy":
        S = ba.ring_scene(n_cams=72, n_pts=120, seed=60, noise=2e-3, frac=0.93)
        deg = np.bincount(S["lm"])
        assert (deg > 64).sum() > 10 and (deg <= 64).sum() > 0          # heavy landmarks (a workgroup each) and light ones
        rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=61)
    else:
        S = ba.sequential_scene(n_cams=150, seed=62, noise=1e-3)
        rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=63, deg=0.5, rel=2e-4)
    opts = dict(function_tol=1e-10 if kind == "heavy" else 1e-8)
    ctx = _ctx(xmamd, S)
    _, _, _, info = ctx.bundle_adjust(rot0, t0, P0, eta=1e-6, **opts)
    ctx.close()
    _, _, _, ref = ba.lm(*_obs(S), rot0, t0, P0, **opts)
    print(f"{kind}: GPU {info['final_cost']:.12e} ({info['status_name']}, {info['iters']} it, {info['pcg_iters']} PCG, "
          f"{info['pcg_iters'] / max(1, info['iters']):.1f} per step, {info['seconds']:.2f} s) numpy {ref['final_cost']:.12e} ({ref['iters']} it)")
    if kind == "sequential":
        assert info["pcg_iters"] >= 10 * info["iters"]
    assert abs(info["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]


def test_repeatable_and_leaves_the_context_unchanged(xmamd):
    S = ba.ring_scene(n_cams=24, n_pts=250, seed=70, noise=2e-3)
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=71)
    a, b = _ctx(xmamd, S), _ctx(xmamd, S)
    Ra1, sa1, _ = a.solve(5, 1e-8, 0.0)
    Rb1, sb1, _ = b.solve(5, 1e-8, 0.0)
    out1 = a.bundle_adjust(rot0, t0, P0)
    out2 = a.bundle_adjust(rot0, t0, P0)
    for x, y in zip(out1[:3], out2[:3]):
        assert x.tobytes() == y.tobytes()
    assert out1[3]["final_cost"] == out2[3]["final_cost"] and out1[3]["iters"] == out2[3]["iters"]
    Ra2, sa2, ia = a.solve(5, 1e-8, 0.0)
    Rb2, sb2, ib = b.solve(5, 1e-8, 0.0)
    a.close(); b.close()
    assert Ra2.tobytes() == Rb2.tobytes() and sa2.tobytes() == sb2.tobytes() and ia["primal"] == ib["primal"]


def test_simple2_from_the_reference_recovery(xmamd):
    G = os.path.join(tl.GOLDEN, "simple2")
    Z = np.load(os.path.join(G, "obs.npz"))
    ref = np.load(os.path.join(G, "tp.npz"))
    obs = (Z["cam"], Z["lm"], Z["p"], Z["w"].reshape(-1))
    ctx = xmamd.Context(obs=obs)
    rot0, t0, P0 = ref["R_real"], ref["t_est"], ref["p_est"]
    rot, t, P, info = ctx.bundle_adjust(rot0, t0, P0)
    ctx.close()
    F0, nu = ba.reprojection_cost(*obs, rot0, t0, P0)
    F1, _ = ba.reprojection_cost(*obs, rot, t, P)
    g0 = np.abs(ba.gradient_at(*obs, rot0, t0, P0)).max()
    g1 = np.abs(ba.gradient_at(*obs, rot, t, P)).max()
    gt = tl.load_bin(os.path.join(G, "gtR.bin"))
    fi = np.load(os.path.join(G, "frame_index.npy"))

    def rot_err(R):
        return np.median([np.linalg.norm(R[:, :3].T @ R[:, 3 * i:3 * i + 3] - gt[:, 3 * fi[0]:3 * fi[0] + 3] @ gt[:, 3 * fi[i]:3 * fi[i] + 3].T)
                          for i in range(fi.size)])
    print(f"SIMPLE2: cost {info['initial_cost']:.6e} -> {info['final_cost']:.6e} (numpy {F0:.6e} -> {F1:.6e}), {info['iters']} iterations, "
          f"{info['pcg_iters']} PCG, {info['seconds']:.3f} s, status {info['status_name']}; |J^T r|_inf {g0:.3e} -> {g1:.3e}; median rotation "
          f"error against gtR {rot_err(rot0):.4e} -> {rot_err(rot):.4e}")
    assert info["n_used"] == nu and info["final_cost"] < info["initial_cost"]
    assert np.isclose(info["initial_cost"], F0, rtol=1e-10) and np.isclose(info["final_cost"], F1, rtol=1e-8)
    assert info["status"] in xmamd.BA_CONVERGED and g1 <= 1e-2 * g0


def _raw(xmamd, ctx, n, m, eta=0.1, struct_size=None, nan=False):
    opt, res = xmamd.BaOptions(), xmamd.BaResult()
    opt.struct_size = C.sizeof(opt) if struct_size is None else struct_size
    res.struct_size = C.sizeof(res)
    opt.eta = eta
    rot = np.asfortranarray(np.tile(np.eye(3), (1, n))); t = np.zeros((3, n), order="F"); P = np.zeros((3, max(m, 1)), order="F")
    P[2] = 10.0
    if nan:
        rot[0, 0] = np.nan
    rc = xmamd.lib().xm_ctx_bundle_adjust(ctx.h, C.byref(opt), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                          P.ctypes.data_as(C.c_void_p), C.byref(res))
    return rc


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
    ctx = _ctx(xmamd, S)
    _, _, i0 = ctx.solve(5, 1e-8, 0.0)
    for kw in (dict(struct_size=8), dict(nan=True), dict(eta=0.0), dict(eta=1.0)):
        assert _raw(xmamd, ctx, S["n"], S["m"], **kw) == ERR_ARG, kw
    _, _, i1 = ctx.solve(5, 1e-8, 0.0)
    ctx.close()
    assert i0["status"] == i1["status"] == i2["status"] == 1 and i0["primal"] == i1["primal"]
