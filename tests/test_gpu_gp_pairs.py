"""GPU tests of the global positioning with camera-to-camera constraints, per-camera weights and the fixed-centre pass
(xm_ctx_global_positioning_pairs, xm-code_amd/csrc/xm_gp.hip) against the numpy restatement tests/xm_gp_pairs_numpy.py (same problem, same
Levenberg-Marquardt rules, exact linear solves; tests/test_gp_pairs_numpy.py runs it alone on these scenes).  The pair tests start from a
perturbed truth: see that file for why.  Nothing here was compared with the reference's compiled code."""
import ctypes as C

import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_gp_numpy as gp
import xm_gp_pairs_numpy as gpp

pytestmark = pytest.mark.gpu

STRIPPED = (1, 4, 8, 11, 15, 18)
MIXED = gpp.CONSTRAINTS[1:]
_cache = {}


def ring20():
    """the 20-camera ring of tests/test_gp_pairs_numpy.py: six cameras see only landmarks below min_views; all 190 pairs"""
    if "ring20" not in _cache:
        S = gpp.strip_long_tracks(ba.ring_scene(n_cams=20, n_pts=120, seed=20, noise=2e-3), STRIPPED)
        pi, pj = gpp.all_pairs(20)
        _cache["ring20"] = (S, (pi, pj, gpp.relative_translations(S, pi, pj, noise=1e-3, seed=21)), gpp.perturbed_start(S, 22))
    return _cache["ring20"]


def reference(key, **kw):
    """the restatement's LM on ring20, computed once per argument set and shared"""
    if key not in _cache:
        S, pairs, (t0, P0) = ring20()
        _cache[key] = gpp.lm(S["cam"], S["lm"], S["p"], S["w"], S["rot"], kw.pop("t0", t0), P0, **kw)
    return _cache[key]


def _ctx(xmamd, S):
    return xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=S["n"])


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2]["scales"].tobytes() == b[2]["scales"].tobytes() and \
        a[2]["final_cost"] == b[2]["final_cost"] and a[2]["iters"] == b[2]["iters"] and a[2]["pcg_iters"] == b[2]["pcg_iters"]


def test_only_points_through_the_new_entry_has_the_old_entrys_bytes(xmamd):
    S, pairs, (t0, P0) = ring20()
    ctx = _ctx(xmamd, S)
    old = ctx.global_positioning(S["rot"], t0, P0)
    none = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3)))
    new = ctx.global_positioning(S["rot"], t0, P0, pairs=none)                    # no pair, ONLY_POINTS, calibrated NULL
    named = ctx.global_positioning(S["rot"], t0, P0, pairs=pairs)                 # pairs that ONLY_POINTS does not read
    ctx.close()
    assert "pairs_used" in new[2] and new[2]["pairs_used"] == 0 and "pairs_used" not in old[2]
    assert _same(old, new) and _same(old, named) and np.all(named[2]["sigma"] == -1.0)
    assert old[0][:, list(STRIPPED)].tobytes() == np.asfortranarray(t0)[:, list(STRIPPED)].tobytes()


@pytest.mark.parametrize("constraint", MIXED + ("fixed",))
def test_two_calls_give_the_same_bytes(xmamd, constraint):
    S, pairs, (t0, P0) = ring20()
    kw = dict(fix_centres=True) if constraint == "fixed" else dict(pairs=pairs, constraint=constraint, points=False)
    cal = np.arange(20) % 4 != 0
    ctx = _ctx(xmamd, S)
    a = ctx.global_positioning(S["rot"], t0, P0, calibrated=cal, reweight_scale=2.5, **kw)
    b = ctx.global_positioning(S["rot"], t0, P0, calibrated=cal, reweight_scale=2.5, **kw)
    ctx.close()
    assert _same(a, b) and a[2]["iters"] > 2
    if constraint != "fixed":
        assert a[2]["sigma"].tobytes() == b[2]["sigma"].tobytes() and a[2]["sigma"].min() > gpp.S_MIN


@pytest.mark.parametrize("constraint", MIXED)
def test_trace_and_centres_follow_the_restatement(xmamd, constraint):
    """the accept sequence is the restatement's, the costs agree to 1e-9 relative (the figure of the bundle adjustment's loops) and the
    centres to 1e-9 of the largest (the figure tests/test_gpu_gp.py holds two runs of one problem to)"""
    S, pairs, (t0, P0) = ring20()
    cal = np.arange(20) % 4 != 0
    ctx = _ctx(xmamd, S)
    t, P, info = ctx.global_positioning(S["rot"], t0, P0, pairs=pairs, constraint=constraint, calibrated=cal, reweight_scale=2.5, points=False,
                                        eta=1e-12, function_tol=1e-14, max_iters=6, trace=10)
    ctx.close()
    tr, Pr, ref = reference(("trace", constraint), pairs=pairs, constraint=constraint, calibrated=cal, reweight_scale=2.5, function_tol=1e-14,
                            max_iters=6)
    g, gr = info["trace"], ref["trace"]
    print("GPU trace\n", g[:, :4], "\nnumpy trace\n", gr)
    dcost = np.abs(g[:, :2] - gr[:, :2]) / np.abs(gr[:, :2])
    dt = float(np.abs(t - tr).max() / np.abs(tr).max())
    ds = float(np.abs(info["sigma"] - ref["sigma"]).max() / np.abs(ref["sigma"]).max())
    print(f"{constraint}: relative cost differences up to {dcost.max():.3e}, centres {dt:.3e}, sigma {ds:.3e}")
    assert g.shape[0] == gr.shape[0] == 6 and np.array_equal(g[:, 3], gr[:, 3])
    assert info["pairs_used"] == ref["pairs_used"] == 190 and info["weight_scale_pt"] == ref["weight_scale_pt"] and info["n_used"] == ref["n_used"]
    assert dcost.max() <= 1e-9
    assert dt <= 1e-9
    assert np.all(g[:, 5] <= 1e-12)                                               # each PCG reached eta


def test_cameras_without_long_tracks_are_positioned_by_their_pairs(xmamd):
    """fails without the pair terms: ONLY_POINTS returns the six stripped centres as they came, POINTS_AND_CAMERAS positions all 20, with
    an aligned centre error of at most twice the f64 restatement's on the same input (the order of summation differs along the LM
    iterations; a factor of two covers that)"""
    S, pairs, (t0, P0) = ring20()
    opts = dict(function_tol=1e-10)
    ctx = _ctx(xmamd, S)
    t_op, _, i_op = ctx.global_positioning(S["rot"], t0, P0, **opts)
    t, P, info = ctx.global_positioning(S["rot"], t0, P0, pairs=pairs, constraint="points_and_cameras", **opts)
    ctx.close()
    tr, _, ref = reference("pac", pairs=pairs, constraint="points_and_cameras", **opts)
    err, err_ref = gpp.aligned_centre_error(S, t), gpp.aligned_centre_error(S, tr)
    moved = np.linalg.norm(t - t0, axis=0)
    print(f"points_and_cameras: {info['iters']} iterations ({info['status_name']}), aligned centre error GPU {err:.6e} restatement {err_ref:.6e}; "
          f"only_points error over the positioned cameras {gpp.aligned_centre_error(S, t_op, np.setdiff1d(np.arange(20), STRIPPED)):.3e}")
    assert t_op[:, list(STRIPPED)].tobytes() == np.asfortranarray(t0)[:, list(STRIPPED)].tobytes()
    assert info["status"] in xmamd.BA_CONVERGED and moved.min() > 0 and info["pairs_used"] == 190
    assert err <= 2.0 * err_ref


def test_only_cameras_then_the_fixed_centre_pass_then_bundle_adjust(xmamd):
    S, pairs, (t0, P0) = ring20()
    opts = dict(function_tol=1e-10)
    ctx = _ctx(xmamd, S)
    t1, P1, i1 = ctx.global_positioning(S["rot"], t0, P0, pairs=pairs, constraint="only_cameras", points=False, **opts)
    assert P1.tobytes() == np.asfortranarray(P0).tobytes() and np.all(i1["scales"] == -1.0) and i1["n_used"] == 0
    t2, P2, i2 = ctx.global_positioning(S["rot"], t1, P0, fix_centres=True, **opts)
    assert t2.tobytes() == t1.tobytes() and i2["pcg_iters"] == 0 and i2["status"] in xmamd.BA_CONVERGED
    t3, P3, i3 = ctx.global_positioning(S["rot"], t0, P0, pairs=pairs, constraint="only_cameras", **opts)   # both calls in one
    assert t3.tobytes() == t1.tobytes() and P3.tobytes() == P2.tobytes() and i3["points"]["final_cost"] == i2["final_cost"]
    tr, _, r1 = reference("oc", pairs=pairs, constraint="only_cameras", **opts)
    _, Pr, r2 = reference("oc_fixed", t0=tr, fix_centres=True, **opts)
    used = np.bincount(S["lm"], minlength=S["m"]) >= 3

    def point_error(tt, PP):
        A, B = np.concatenate([tt, PP[:, used]], axis=1), np.concatenate([S["t"], S["P"][:, used]], axis=1)
        return float(np.sqrt(np.sum((gp.align(A, B) - B) ** 2, axis=0)).max())
    e_c, e_cr, e_p, e_pr = gpp.aligned_centre_error(S, t1), gpp.aligned_centre_error(S, tr), point_error(t2, P2), point_error(tr, Pr)
    print(f"only_cameras: centre error GPU {e_c:.6e} restatement {e_cr:.6e}; fixed-centre pass: point error GPU {e_p:.6e} restatement {e_pr:.6e}")
    assert e_c <= 2.0 * e_cr and e_p <= 2.0 * e_pr
    assert P2[:, ~used].tobytes() == np.asfortranarray(P0)[:, ~used].tobytes()
    _, _, _, ib = ctx.bundle_adjust(S["rot"], t2, P2, max_iters=20)
    ctx.close()
    print(f"bundle_adjust from the result: cost {ib['initial_cost']:.6e} -> {ib['final_cost']:.6e}")
    assert ib["final_cost"] < ib["initial_cost"]


def _raw(xmamd, ctx, S, pairs, constraint=3, flags=0, struct_size=None, reweight=1.0, null=None, valid=None, npairs=None, bad_index=None, nan_trel=False):
    opt, res, g = xmamd.GpOptions(), xmamd.GpResult(), xmamd.GpPairs()
    opt.struct_size, res.struct_size = C.sizeof(opt), C.sizeof(res)
    opt.eta, opt.loss, opt.loss_scale = 0.1, 1, 0.1
    g.struct_size = C.sizeof(g) if struct_size is None else struct_size
    pi, pj, trel = pairs[0].copy(), pairs[1].copy(), np.ascontiguousarray(pairs[2]).copy()
    if bad_index is not None:
        pj[3] = bad_index if bad_index != "same" else pi[3]
    if nan_trel:
        trel[5, 1] = np.nan
    g.constraint, g.flags, g.reweight_scale, g.npairs = constraint, flags, reweight, pi.size if npairs is None else npairs
    g.pi, g.pj, g.trel = (a.ctypes.data_as(C.c_void_p) for a in (pi, pj, trel))
    if valid is not None:
        valid = np.ascontiguousarray(valid, dtype=np.uint8)
        g.valid = valid.ctypes.data_as(C.c_void_p)
    if null and null != "pairs":
        setattr(g, null, None)
    rot = np.asfortranarray(S["rot"]); t = np.asfortranarray(S["t"]).copy(order="F"); P = np.asfortranarray(S["P"]).copy(order="F")
    rc = xmamd.lib().xm_ctx_global_positioning_pairs(ctx.h, C.byref(opt), None if null == "pairs" else C.byref(g), rot.ctypes.data_as(C.c_void_p),
                                                     t.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p), None, C.byref(res))
    return rc, t.tobytes() == np.asfortranarray(S["t"]).tobytes() and P.tobytes() == np.asfortranarray(S["P"]).tobytes()


def test_refusals_leave_the_context_usable(xmamd):
    ERR_ARG = -2
    S, pairs, _ = ring20()
    ctx, twin = _ctx(xmamd, S), _ctx(xmamd, S)
    none = np.zeros(190, dtype=np.uint8)
    for kw in (dict(struct_size=16), dict(constraint=4), dict(constraint=-1), dict(flags=2), dict(flags=1, constraint=1), dict(flags=1, constraint=2),
               dict(flags=1, constraint=3), dict(valid=none, constraint=1), dict(valid=none, constraint=2), dict(valid=none, constraint=3),
               dict(npairs=0, constraint=1), dict(npairs=-1), dict(null="pi"), dict(null="pj"), dict(null="trel"), dict(null="pairs"),
               dict(bad_index=20), dict(bad_index=-1), dict(bad_index="same"), dict(bad_index=20, constraint=0), dict(bad_index="same", valid=none, constraint=0),
               dict(nan_trel=True), dict(reweight=-1.0), dict(reweight=np.nan), dict(reweight=np.inf)):
        rc, untouched = _raw(xmamd, ctx, S, pairs, **kw)
        assert rc == ERR_ARG and untouched, kw
    assert _raw(xmamd, ctx, S, pairs)[0] == 0 and _raw(xmamd, ctx, S, pairs, constraint=0, flags=1)[0] == 0     # the same calls without a fault
    assert _raw(xmamd, ctx, S, pairs, constraint=0, valid=none)[0] == 0 and _raw(xmamd, ctx, S, pairs, nan_trel=True, valid=none, constraint=0)[0] == 0
    V = __import__("xm_testlib").gen_vg(20, deg=4, sigma=0.05, seed=83)
    other = xmamd.Context(Q=V["Q"])
    assert _raw(xmamd, other, S, pairs)[0] == ERR_ARG and "XM_STORAGE_SCHUR" in xmamd.lib().xm_last_error().decode()
    other.close()
    Ra, sa, ia = ctx.solve(5, 1e-8, 0.0)
    Rb, sb, ib = twin.solve(5, 1e-8, 0.0)
    ctx.close(); twin.close()
    assert Ra.tobytes() == Rb.tobytes() and sa.tobytes() == sb.tobytes() and ia["primal"] == ib["primal"]
