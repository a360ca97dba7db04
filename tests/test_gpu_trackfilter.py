"""GPU tests of the track filter (xm_ctx_filter_tracks, include/xm_amd.h; xm-code_amd/csrc/xm_trackfilter.hip) and of the loop that drives
it (Context.refine_filtered).  keep, reason, lm_views, lm_status and every counter are compared with the numpy contract
tests/xm_trackfilter_numpy.py:run_numpy EXACTLY -- no tolerance anywhere; test_trackfilter_numpy.py holds that contract against the
line-by-line restatement of track_filter.cc on the same scenes.  The thresholds the contract compares against are the doubles the library
returns (and those are asserted to be cos_deg of the angles given).

Which kernel a scene pins: the per-observation tests and the codes -> tf_obs_kernel (boundary, tile, flags, depth, thresholds, SIMPLE2);
landmarks of up to 64 observations -> tf_light_kernel (boundary, pair designs of 2, 3 and 64 rays, SIMPLE2); longer ones -> tf_heavy_kernel
(boundary: 65 and 66; tile: one tile less one, one tile, one tile plus one, two tiles plus one; pair designs of 70, TILE + 5 and
2 TILE + 1 rays, the last two with the only wide pair across two tiles); keep, reason and the counters -> tf_emit_kernel, tf_reduce_kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_trackfilter_numpy as tf

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETTINGS = (dict(reprojection=tf.TIGHT["reprojection"]), dict(reprojection=None, angle=tf.TIGHT["angle"]),
            dict(reprojection=None, triangulation=tf.TIGHT["triangulation"]), dict(**tf.TIGHT), dict(min_views=3, **tf.TIGHT),
            dict(reprojection=1e-2, angle=1.0, triangulation=1.0))


def _ctx(xmamd, S):
    """a context on the scene's list; weights that are not all positive arrive through set_edge_weights (creation wants every camera weighted)"""
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], np.ones(S["cam"].size)), n=S["n"])
    assert ctx.n_landmarks == S["m"]
    if not (S["w"] == 1.0).all():
        ctx.set_edge_weights(S["w"])
    return ctx


def _check(ctx, S, **kw):
    """one call against the contract, exactly; -> (plan, contract)"""
    plan = ctx.filter_tracks(S["rot"], S["t"], S["P"], **kw)
    full = dict(reprojection=1e-2, angle=None, triangulation=None, min_views=0); full.update(kw)
    for key, name in (("angle", "cos_angle"), ("triangulation", "cos_triangulation")):
        assert plan.info[name] == (tf.cos_deg(full[key]) if full[key] is not None else 0.0)
    ref = tf.run_numpy(S, cos_angle=plan.info["cos_angle"], cos_triangulation=plan.info["cos_triangulation"], **full)
    got = dict(plan.info, keep=plan.keep, reason=plan.reason, lm_views=plan.lm_views, lm_status=plan.lm_status)
    assert tf.same(got, ref) == [], (kw, tf.same(got, ref), {k: (got[k], ref[k]) for k in tf.COUNTS if got[k] != ref[k]})
    assert plan.keep.dtype == bool and plan.reason.dtype == np.uint8 and plan.lm_views.dtype == np.int32 and plan.lm_status.dtype == np.uint8
    assert plan.info["seconds_kernels"] > 0 and plan.info["seconds_download"] > 0
    return plan, ref


def test_limits_are_those_of_the_scenes(xmamd):
    assert xmamd.track_filter_limits() == dict(light_max=tf.LIGHT_MAX, tile=tf.TILE, threads=256)


# ------------------------------------------------------------------------------------------------ the recorded case
def test_recorded_case(xmamd):
    S = tf.simple2(GOLDEN)
    ctx = _ctx(xmamd, S)
    # the reference's defaults drop nothing at the reference's own solution
    plan, ref = _check(ctx, S, reprojection=1e-2, angle=1.0, triangulation=1.0)
    assert plan.keep.all() and (plan.reason == 0).all() and (plan.lm_status == tf.LM_KEPT).all() and plan.info["tracks_kept"] == S["m"]
    assert plan.info["obs_kept"] == plan.info["obs_used"] == S["cam"].size and np.array_equal(plan.lm_views, np.bincount(S["lm"], minlength=S["m"]))
    assert plan.weights(S["w"]).tobytes() == S["w"].tobytes()
    # thresholds inside the distributions: each filter alone drops between 1 % and 50 % of its population (under the contract)
    T = tf.SIMPLE2_TIGHT
    for kw, key, pop in ((dict(reprojection=T["reprojection"]), "dropped_reprojection", "obs_used"), (dict(reprojection=None, angle=T["angle"]), "dropped_angle", "obs_used"),
                         (dict(reprojection=None, triangulation=T["triangulation"]), "tracks_changed_triangulation", "tracks_total")):
        ref = tf.run_numpy(S, **kw)
        assert 0.01 * ref[pop] < ref[key] < 0.5 * ref[pop], (kw, ref[key], ref[pop])
        plan, _ = _check(ctx, S, **kw)
        assert plan.info[key] == ref[key]
    plan, _ = _check(ctx, S, **T)
    # (in sequence the angle filter sees what the reprojection filter left: at these thresholds that is nothing it would drop)
    assert plan.info["dropped_reprojection"] > 0 and plan.info["dropped_triangulation"] > 0
    plan3, _ = _check(ctx, S, min_views=3, **T)
    assert plan3.info["dropped_min_views"] > 0 and plan3.info["obs_kept"] < plan.info["obs_kept"]
    w = plan3.weights(S["w"])
    assert np.array_equal(w == 0, ~plan3.keep) and [a.shape[0] for a in plan3.apply(S["cam"], S["p"])] == [plan3.info["obs_kept"]] * 2
    ctx.close()


# ------------------------------------------------------------------------------------------------ hand-made scenes
@pytest.mark.parametrize("scene", ["boundary", "tile", "flags", "depth"])
def test_hand_made_scenes(xmamd, scene):
    S = getattr(tf, scene + "_scene")()
    T, perm = tf.permuted(S, seed=5)
    ctx, ctx_p = _ctx(xmamd, S), _ctx(xmamd, T)
    for kw in SETTINGS + (dict(reprojection=1e-2, triangulation=1.0), dict(reprojection=None, angle=1.0)):
        plan, _ = _check(ctx, S, **kw)
        again = ctx.filter_tracks(S["rot"], S["t"], S["P"], **kw)          # two calls, the same bits
        for k in ("keep", "reason", "lm_views", "lm_status"):
            assert getattr(plan, k).tobytes() == getattr(again, k).tobytes()
        assert {k: plan.info[k] for k in tf.COUNTS} == {k: again.info[k] for k in tf.COUNTS}
        # a permuted observation order: the same answer per observation and per landmark
        pp, _ = _check(ctx_p, T, **kw)
        assert np.array_equal(plan.keep[perm], pp.keep) and np.array_equal(plan.reason[perm], pp.reason)
        assert np.array_equal(plan.lm_views, pp.lm_views) and np.array_equal(plan.lm_status, pp.lm_status)
    ctx.close(); ctx_p.close()


@pytest.mark.parametrize("k", [2, 3, tf.LIGHT_MAX, tf.LIGHT_MAX + 6, tf.TILE + 5, 2 * tf.TILE + 1])
def test_pair_designs(xmamd, k):
    """the only qualifying pair is the first, the last, one across the list (two different tiles for the two longest), or there is none"""
    for where in ("first", "last", "split", "none"):
        S = tf.pair_scene(k, where)
        ctx = _ctx(xmamd, S)
        plan, _ = _check(ctx, S, reprojection=None, triangulation=1.0)
        assert plan.lm_status[1] == (tf.LM_TRIANGULATION if where == "none" else tf.LM_KEPT) and plan.lm_views[1] == (0 if where == "none" else k)
        ctx.close()


def test_a_value_equal_to_the_threshold_does_not_pass(xmamd):
    for name, S, kw, i in tf.threshold_cases():
        ctx = _ctx(xmamd, S)
        plan, _ = _check(ctx, S, **kw)
        if name == "reprojection":
            assert plan.reason[i] == tf.REASON_REPROJECTION                                   # err == threshold: strict <
            assert ctx.filter_tracks(S["rot"], S["t"], S["P"], reprojection=float(np.nextafter(kw["reprojection"], 1.0))).keep[i]
        elif name == "angle":
            _, q, _ = tf.geometry(S)
            assert tf.angle_cosine(S, q)[i] == plan.info["cos_angle"] and plan.reason[i] == tf.REASON_ANGLE          # strict >
        else:
            r = tf.rays(tf.geometry(S)[0])
            assert (r[0, 0] * r[1, 0] + r[0, 1] * r[1, 1]) + r[0, 2] * r[1, 2] == plan.info["cos_triangulation"]
            assert plan.lm_status[i] == tf.LM_TRIANGULATION and (plan.reason == tf.REASON_TRIANGULATION).all()       # strict <
        ctx.close()


# ------------------------------------------------------------------------------------------------ the context is only read
def _ring(seed=7):
    return ba.ring_scene(n_cams=20, n_pts=300, seed=seed, frac=0.5, min_views=3, noise=5e-4)


def test_the_call_changes_nothing_in_the_context(xmamd):
    S = _ring()
    lam = 1.5 * float(np.sum(S["w"] * np.sum(S["p"] ** 2, axis=1)) / (3 * S["n"]))
    start = ba.perturb(S["rot"], S["t"], S["P"], seed=3, deg=0.5, rel=0.002)
    outs = []
    for with_call in (False, True):
        ctx = _ctx(xmamd, S)
        if with_call:
            ctx.filter_tracks(*start, reprojection=5e-3, angle=0.5, triangulation=2.0, min_views=3)
        R, s, info = ctx.solve(5, 1e-6, lam)
        if with_call:
            ctx.filter_tracks(*start, reprojection=5e-3, triangulation=2.0)
        rot, t, P, binfo = ctx.bundle_adjust(*start, max_iters=10)
        outs.append((R.tobytes(), s.tobytes(), info["primal"], rot.tobytes(), t.tobytes(), P.tobytes(), binfo["final_cost"], binfo["iters"]))
        ctx.close()
    assert outs[0] == outs[1]


def test_refusals_leave_the_context_usable(xmamd):
    S = tf.boundary_scene()
    ctx = _ctx(xmamd, S)
    ref = ctx.filter_tracks(S["rot"], S["t"], S["P"], **tf.TIGHT)
    L = xmamd.lib()
    nobs, m = ctx.ne, ctx.n_landmarks
    keep = np.zeros(nobs, dtype=np.uint8); reason = np.zeros(nobs, dtype=np.uint8); views = np.zeros(m, dtype=np.int32); status = np.zeros(m, dtype=np.uint8)
    rot, t, Pw = (np.asfortranarray(S[k]) for k in ("rot", "t", "P"))
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def fresh():
        o = xmamd.TfOptions(); r = xmamd.TfResult()
        o.struct_size, r.struct_size, o.flags = C.sizeof(o), C.sizeof(r), 7
        o.max_reprojection_error, o.max_angle_error, o.min_triangulation_angle = 1e-2, 1.0, 1.0
        return o, r

    def call(o, r, rot_=rot, t_=t, p_=Pw, keep_=keep, views_=views):
        return L.xm_ctx_filter_tracks(ctx.h, C.byref(o), P(rot_), P(t_), P(p_), P(keep_), P(reason), P(views_), P(status), C.byref(r))
    o, r = fresh()
    assert call(o, r) == 0
    for change in (lambda o, r: setattr(o, "struct_size", 32), lambda o, r: setattr(r, "struct_size", 136), lambda o, r: setattr(o, "flags", 15),
                   lambda o, r: setattr(o, "min_views", -1), lambda o, r: setattr(o, "max_reprojection_error", 0.0),
                   lambda o, r: setattr(o, "max_reprojection_error", -1e-2), lambda o, r: setattr(o, "max_angle_error", 0.0),
                   lambda o, r: setattr(o, "min_triangulation_angle", -1.0)):
        o, r = fresh(); change(o, r)
        assert call(o, r) == -2
    o, r = fresh()
    for kw in (dict(rot_=None), dict(t_=None), dict(p_=None), dict(keep_=None), dict(views_=None)):
        assert call(o, r, **kw) == -2 and "null" in L.xm_last_error().decode()
    for name in ("rot_", "t_", "p_"):
        for bad in (np.nan, np.inf):
            a = dict(rot_=rot, t_=t, p_=Pw)[name].copy(order="F"); a[1, 0] = bad
            assert call(o, r, **{name: a}) == -2 and "not finite" in L.xm_last_error().decode()
    o.flags, o.max_angle_error = 1, 0.0                      # the threshold of a filter that is off is not read
    assert call(o, r) == 0
    # another storage, several ranks
    import xm_testlib as tl
    V = tl.gen_vg(40, deg=3, sigma=0.1, seed=1)
    dense = xmamd.Context(Q=V["Q"])
    with pytest.raises(xmamd.XmError, match="XM_STORAGE_SCHUR"):
        dense.filter_tracks(np.zeros((3, 120)), np.zeros((3, 40)), np.zeros((3, 0)))
    dense.close()
    G = _ring()
    two = xmamd.Context(obs=(G["cam"], G["lm"], G["p"], G["w"]), n_gpus=2, gpu_map=1)
    with pytest.raises(xmamd.XmError, match="single-GPU"):
        two.filter_tracks(G["rot"], G["t"], G["P"])
    two.close()
    after = ctx.filter_tracks(S["rot"], S["t"], S["P"], **tf.TIGHT)      # still usable, same answer
    assert after.keep.tobytes() == ref.keep.tobytes() and after.reason.tobytes() == ref.reason.tobytes() and after.info["obs_kept"] == ref.info["obs_kept"]
    ctx.close()


# ------------------------------------------------------------------------------------------------ the loop
def test_refine_filtered_on_a_ring_with_displaced_observations(xmamd):
    G = _ring()
    S, hit = tf.displaced(G, share=0.05, size=0.05, seed=11)
    # the contract itself flags the displaced points at the ground-truth geometry (and hardly anything else)
    truth = tf.run_numpy(S, reprojection=1e-2, triangulation=1.0)
    assert hit.sum() >= 50 and (truth["reason"][hit] != 0).mean() >= 0.9 and (truth["reason"][~hit] != 0).mean() < 0.02
    lam = 1.5 * float(np.sum(S["w"] * np.sum(S["p"] ** 2, axis=1)) / (3 * S["n"]))
    fresh = _ctx(xmamd, S)
    R0, s0, info0 = fresh.solve(5, 1e-6, lam)
    fresh.close()
    ctx = _ctx(xmamd, S)
    start = ba.perturb(S["rot"], S["t"], S["P"], seed=3, deg=0.5, rel=0.002)
    rot, t, P, info = ctx.refine_filtered(*start, rounds=3, reprojection=1e-2, triangulation=1.0, restore_weights=True, max_iters=50)
    keep = info["keep"]
    dropped = ~keep                                           # (every observation of the scene is used: weight 1, depth > 0)
    print(f"refine_filtered: {len(info['rounds'])} rounds, dropped {dropped.sum()} of {keep.size}, displaced {hit.sum()}, "
          f"displaced and dropped {(dropped & hit).sum()}, costs {[(r['ba_full']['initial_cost'], r['ba_full']['final_cost']) for r in info['rounds']]}")
    assert np.array_equal(info["weights"] == 0, dropped) and 1 <= len(info["rounds"]) <= 3
    # every observation the loop dropped is one the contract drops at the returned point
    at_end = tf.run_numpy(dict(S, rot=rot, t=t, P=P), reprojection=1e-2, triangulation=1.0)
    assert not (dropped & (at_end["reason"] == 0)).any(), int((dropped & (at_end["reason"] == 0)).sum())
    assert (dropped & hit).sum() >= 0.9 * hit.sum()
    # restore_weights=True: the context solves as a fresh one does
    R1, s1, info1 = ctx.solve(5, 1e-6, lam)
    assert R1.tobytes() == R0.tobytes() and s1.tobytes() == s0.tobytes() and info1["primal"] == info0["primal"]
    ctx.close()
