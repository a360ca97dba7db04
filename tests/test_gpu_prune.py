"""GPU tests of the pruning of weakly connected images (xm_prune_weakly_connected / xm_ctx_prune_weakly_connected, include/xm_amd.h;
xm-code_amd/csrc/xm_prune.hip) and of Context.refine_filtered(prune=True).  cluster_id, obs_count, every counter and the visibility graph as
three arrays are compared with the numpy contract tests/xm_prune_numpy.py:run_numpy EXACTLY -- no tolerance anywhere;
test_prune_numpy.py holds that contract against the line-cited restatement of the C++ on the same scenes.

Which kernel a scene pins: the LDS histogram and its tiles -> the tile scenes (one tile less one camera, one tile, one tile plus one, two
tiles plus one; edges across the boundaries; a landmark that every camera sees, walked by the whole workgroup; a camera list of more than
one workgroup's worth of entries); the lane groups -> every hand-made scene (tracks of 3 and 4 entries) and SIMPLE2 (6 to 57); the packed
landmark lists of a context -> the context form; the order statistics -> big_weights and edge_values (second level), SIMPLE2; the
labellings, the compaction of the merge rounds' edges and the rounds -> bridge, ladder, ties, small."""
import os

import numpy as np
import pytest

import xm_prune_numpy as pr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _result(plan):
    i, j, c = plan.pairs
    return dict(plan.info, cluster_id=plan.cluster_id, obs_count=plan.obs_count, pairs_i=i, pairs_j=j, pairs_count=c)


def _check(plan, ref):
    got = _result(plan)
    assert pr.same(got, ref) == [], (pr.same(got, ref), {k: (got[k], ref[k]) for k in pr.COUNTERS if got[k] != ref[k]})
    assert plan.cluster_id.dtype == plan.obs_count.dtype == np.int32 and all(a.dtype == np.int32 for a in plan.pairs)
    assert plan.info["seconds_kernels"] > 0
    return got


def _host(xmamd, S, **kw):
    o = dict(S.get("opt", {})); o.update(kw)
    return xmamd.prune_weakly_connected(S["cam"], S["lm"], n=S["n"], m=S["m"], w=S["w"], pairs=True, **o)


def _same_bits(a, b):
    assert all(x.tobytes() == y.tobytes() for x, y in zip((a.cluster_id, a.obs_count) + a.pairs, (b.cluster_id, b.obs_count) + b.pairs))
    assert {k: a.info[k] for k in pr.COUNTERS} == {k: b.info[k] for k in pr.COUNTERS}


def _ctx(xmamd, S, **kw):
    """a context on the scene's list with made-up camera-frame points; weights that are not all positive arrive through set_edge_weights
    (creation wants every camera weighted)"""
    p = S.get("p")
    if p is None:
        rng = np.random.default_rng(7)
        p = np.column_stack([rng.uniform(-0.5, 0.5, (S["cam"].size, 2)), rng.uniform(1.0, 3.0, S["cam"].size)])
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], p, np.ones(S["cam"].size)), n=S["n"], **kw)
    assert ctx.n_landmarks == S["m"]
    if not (S["w"] == 1.0).all():
        ctx.set_edge_weights(S["w"])
    return ctx


@pytest.fixture(scope="module")
def limits(xmamd):
    return xmamd.prune_limits()


# ------------------------------------------------------------------------------------------------ host form against the contract
@pytest.mark.parametrize("name", [k for k, _ in pr.HAND_MADE])
def test_hand_made_scenes_host_form(xmamd, name):
    S = dict(pr.HAND_MADE)[name]()
    ref = pr.run_numpy(S)
    plan = _host(xmamd, S)
    _check(plan, ref)
    _same_bits(plan, _host(xmamd, S))                          # two calls, the same bits
    T, perm = pr.permuted(S, seed=11)                          # another order of the list, other landmark numbers: the same answer per camera
    _same_bits(plan, _host(xmamd, T))
    if name == "small":                                        # the options change what the scene is about
        for kw in (dict(min_num_images=2), dict(min_num_observations=0), dict(min_covisibility=9, min_threshold=7.0)):
            _check(_host(xmamd, S, **kw), pr.run_numpy(S, **kw))
    if name == "bridge2":                                      # w == NULL: all used
        _same_bits(plan, xmamd.prune_weakly_connected(S["cam"], S["lm"], n=S["n"], m=S["m"], pairs=True))


@pytest.mark.parametrize("which", ["T-1", "T", "T+1", "2T+1"])
def test_tile_scenes_host_form(xmamd, limits, which):
    T = limits["tile"]
    n = dict([("T-1", T - 1), ("T", T), ("T+1", T + 1), ("2T+1", 2 * T + 1)])[which]
    S = pr.tile(n, T)
    assert S["cam"].size < 60000 and np.bincount(S["cam"])[0] > limits["threads"] and np.bincount(S["lm"]).max() == n > limits["group_max"]
    ref = pr.run_numpy(S)
    assert ref["component_images"] == n and ref["n_clusters"] > 1
    bi, bj = ref["pairs_i"] // T, ref["pairs_j"] // T        # edges inside the first tile, across a boundary, and (two tiles) two apart
    assert (bi == bj).any() and (n <= T or (bi != bj).any()) and (n <= 2 * T or (bj - bi == 2).any())
    plan = _host(xmamd, S)
    _check(plan, ref)
    T2, _ = pr.permuted(S, seed=2)
    _same_bits(plan, _host(xmamd, T2))


def test_recorded_case_both_forms(xmamd):
    S = pr.simple2(GOLDEN)
    ref = pr.run_numpy(S)
    assert (ref["n_edges"], ref["median"], ref["mad"], ref["threshold"], ref["n_clusters"], ref["images_clustered"]) == (4105, 65.0, 42.0, 23.0, 1, 93)
    host = _host(xmamd, S)
    _check(host, ref)
    ctx = _ctx(xmamd, S)
    plan = ctx.prune_weakly_connected(pairs=True)
    _check(plan, ref)
    _same_bits(plan, host)
    _same_bits(plan, ctx.prune_weakly_connected(pairs=True))
    ref200 = pr.run_numpy(S, min_num_observations=200)
    assert (ref200["n_edges"], ref200["threshold"], ref200["images_clustered"]) == (3497, 31.0, 85)
    p200 = ctx.prune_weakly_connected(min_num_observations=200, pairs=True)
    _check(p200, ref200)
    assert int((p200.cluster_id == -1).sum()) == 8
    _check(_host(xmamd, S, min_num_observations=200), ref200)
    # the context's CURRENT weights: thinned cameras, then the entry weights again
    thin = pr.simple2(GOLDEN, thin=5)
    ctx.set_edge_weights(thin["w"])
    pt = ctx.prune_weakly_connected(pairs=True)
    _check(pt, pr.run_numpy(thin))
    assert (pt.cluster_id[-5:] == -1).all() and (pt.cluster_id[:-5] == 0).all()
    assert np.array_equal(pt.weights(thin["w"]) > 0, (thin["w"] > 0) & (thin["cam"] < S["n"] - 5))
    ctx.set_edge_weights(S["w"])
    _same_bits(plan, ctx.prune_weakly_connected(pairs=True))
    ctx.close()


@pytest.mark.parametrize("name", ["bridge1", "bridge2", "ladder3", "ladder11", "edge_values", "big_weights", "ties", "small"])
def test_hand_made_scenes_context_form(xmamd, name):
    S = dict(pr.HAND_MADE)[name]()
    G = pr.glued(S)                                            # tracks of length 2 make the list one component: the contract ignores them
    ref = pr.run_numpy(S)
    assert pr.same(ref, pr.run_numpy(G)) == []
    ctx = _ctx(xmamd, G)
    plan = ctx.prune_weakly_connected(pairs=True, **S["opt"])
    _check(plan, ref)
    _same_bits(plan, ctx.prune_weakly_connected(pairs=True, **S["opt"]))
    ctx.close()


def test_context_form_without_a_factorisation(xmamd, limits):
    """above a tile of cameras through the CG form of the context (no (N-1)^2 inverse): the packed landmark lists and a contiguous one"""
    T = limits["tile"]
    S = pr.tile(T + 1, T)
    ctx = _ctx(xmamd, S, tuning=dict(schur_solver=2))
    _check(ctx.prune_weakly_connected(pairs=True), pr.run_numpy(S))
    ctx.close()


# ------------------------------------------------------------------------------------------------ the pairs' capacity
def test_pairs_capacity(xmamd):
    S = pr.bridge(2)
    ref = pr.run_numpy(S)
    E = ref["n_edges"]
    small = xmamd.prune_weakly_connected(S["cam"], S["lm"], n=S["n"], m=S["m"], pairs=E - 1)
    assert small.pairs is None and small.info["n_edges"] == E and np.array_equal(small.cluster_id, ref["cluster_id"])
    L = xmamd.lib()
    import ctypes as C
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    opt = xmamd.PruneOptions(C.sizeof(xmamd.PruneOptions), 5, 2, 0, 20.0); res = xmamd.PruneResult(); res.struct_size = C.sizeof(res)
    cid = np.zeros(S["n"], np.int32); cnt = np.zeros(S["n"], np.int32)
    arrays = [np.full(E, -7, dtype=np.int32) for _ in range(3)]
    pp = xmamd.PrunePairs(E - 1, *[P(a) for a in arrays])
    assert L.xm_prune_weakly_connected(S["n"], S["m"], S["cam"].size, P(S["cam"]), P(S["lm"]), None, C.byref(opt), P(cid), P(cnt), C.byref(pp), C.byref(res)) == 0
    assert res.n_edges == E and all((a == -7).all() for a in arrays)          # too small: nothing is written
    exact = xmamd.prune_weakly_connected(S["cam"], S["lm"], n=S["n"], m=S["m"], pairs=E)
    _check(exact, ref)
    none = xmamd.prune_weakly_connected(S["cam"], S["lm"], n=S["n"], m=S["m"])
    assert none.pairs is None and np.array_equal(none.cluster_id, ref["cluster_id"]) and none.info["n_edges"] == E


# ------------------------------------------------------------------------------------------------ the loop
def test_refine_filtered_prune(xmamd):
    """SIMPLE2 with its last five cameras thinned to 4 observations each: the loop's pruning gives them cluster_id -1 and zero weights.  A
    context refuses weights that leave a camera without an observation (set_edge_weights: the reduced camera Laplacian would be singular),
    so the zeros come back in info["weights"] and go into the next context through clean_observations, and the context keeps the weights
    of the closing filters."""
    thin = pr.simple2(GOLDEN, thin=5)
    g = np.load(os.path.join(GOLDEN, "simple2", "tp.npz"))
    rot, t, P = np.ascontiguousarray(g["R_real"]), np.ascontiguousarray(g["t_est"]), np.ascontiguousarray(g["p_est"])
    kw = dict(rounds=1, max_iters=3)
    last = thin["cam"] >= thin["n"] - 5
    outs = {}
    for prune in (False, True, None):
        ctx = _ctx(xmamd, thin)
        outs[prune] = ctx.refine_filtered(rot, t, P, weights=thin["w"], **kw) if prune is None else \
            ctx.refine_filtered(rot, t, P, weights=thin["w"], prune=prune, **kw)
        if prune:
            info = outs[prune][3]
            plan = info["prune"]
            assert (plan.cluster_id[-5:] == -1).all() and (plan.cluster_id[:-5] == 0).all() and (plan.obs_count[-5:] <= 4).all()
            assert (info["weights"][last] == 0).all() and np.array_equal(info["weights"][~last], outs[False][3]["weights"][~last])
            # the plan is the contract's at the weights the closing filters left, and the context still holds exactly those
            filtered = dict(thin, w=outs[False][3]["weights"])
            assert pr.same(_result(ctx.prune_weakly_connected(pairs=True)), pr.run_numpy(filtered)) == []
            assert np.array_equal(plan.cluster_id, pr.run_numpy(filtered)["cluster_id"])
            # the next context's list: the five cameras are gone and the others renumbered
            clean = xmamd.clean_observations(thin["cam"], thin["lm"], w=info["weights"], n=thin["n"], m=thin["m"], min_cam_obs=0, min_lm_obs=1)
            assert (clean.cam_index[-5:] == -1).all() and clean.info["n_new"] == thin["n"] - 5 and not clean.keep[last].any()
        ctx.close()
    # prune=False is the call without the argument, byte for byte
    for a, b in zip(outs[False][:3], outs[None][:3]):
        assert a.tobytes() == b.tobytes()
    assert outs[False][3]["weights"].tobytes() == outs[None][3]["weights"].tobytes() and "prune" not in outs[False][3]
    for a, b in zip(outs[False][:3], outs[True][:3]):          # the pruning runs behind the last adjustment: the geometry is the same
        assert a.tobytes() == b.tobytes()
    # restore_weights puts the entry weights back as before
    ctx = _ctx(xmamd, thin)
    before = ctx.prune_weakly_connected()
    ctx.refine_filtered(rot, t, P, weights=thin["w"], prune=True, restore_weights=True, **kw)
    after = ctx.prune_weakly_connected()
    assert np.array_equal(before.obs_count, after.obs_count) and np.array_equal(before.cluster_id, after.cluster_id)
    ctx.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_argument_errors_of_the_context_form(xmamd):
    import ctypes as C
    import xm_testlib as tl
    L = xmamd.lib()
    S = pr.glued(pr.bridge(1))
    ctx = _ctx(xmamd, S)
    n = S["n"]
    cid = np.zeros(n, np.int32); cnt = np.zeros(n, np.int32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)

    def call(h, change=None):
        o = xmamd.PruneOptions(C.sizeof(xmamd.PruneOptions), 5, 2, 0, 20.0); r = xmamd.PruneResult(); r.struct_size = C.sizeof(r)
        if change:
            change(o, r)
        return L.xm_ctx_prune_weakly_connected(h, C.byref(o), P(cid), P(cnt), None, C.byref(r))
    for change, word in ((lambda o, r: setattr(o, "struct_size", 20), "struct_size"), (lambda o, r: setattr(r, "struct_size", 8), "struct_size"),
                         (lambda o, r: setattr(o, "min_covisibility", -1), "negative"), (lambda o, r: setattr(o, "min_num_images", -3), "negative"),
                         (lambda o, r: setattr(o, "min_num_observations", -1), "negative"), (lambda o, r: setattr(o, "min_threshold", float("inf")), "finite"),
                         (lambda o, r: setattr(o, "min_threshold", float("nan")), "finite")):
        assert call(ctx.h, change) == -2 and word in L.xm_last_error().decode()
    assert call(ctx.h) == 0                                    # refused calls leave the context usable
    ref = pr.run_numpy(S)
    assert np.array_equal(cid, ref["cluster_id"]) and np.array_equal(cnt, ref["obs_count"])
    ctx.close()
    dense = xmamd.Context(Q=tl.gen_vg(12, deg=3, sigma=0.1, seed=1)["Q"])         # dense storage holds no observations
    assert call(dense.h) == -2 and "XM_STORAGE_SCHUR" in L.xm_last_error().decode()
    with pytest.raises(xmamd.XmError, match="XM_STORAGE_SCHUR"):
        dense.prune_weakly_connected()
    dense.close()
    with pytest.raises(xmamd.XmError, match="out of range"):
        xmamd.prune_weakly_connected([0, 1, 5], [0, 0, 0], n=3)
