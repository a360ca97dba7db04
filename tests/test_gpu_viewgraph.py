"""GPU tests of the two-view match verification and view-graph pruning (xm_view_graph_filter, include/xm_amd.h) against the contract's numpy
restatement (run_numpy of tests/xm_viewgraph_numpy.py): inlier, pair_inliers, pair_status, registered, the compacted matches and every
integer counter EXACTLY.  tests/test_viewgraph_numpy.py ties the restatement to the sequential restatement of the reference's C++.

Shapes: the recorded SIMPLE2-derived case in both passes (4 210 pairs, 261 680 matches) and hand-made cases of a few matches, except where
the size is the point: pairs with 0, 1, 63, 64, 65, 255, 256, 257 matches, each limit of view_graph_limits() and the limit plus one (the
three forms of the scoring kernels), and a chain of 1 500 images (hooking rounds)."""
import numpy as np
import pytest

import xm_viewgraph_numpy as vn

pytestmark = pytest.mark.gpu
ARRAYS = ("inlier", "pair_inliers", "pair_status", "registered")
DTYPES = dict(inlier=np.uint8, pair_inliers=np.int32, pair_status=np.int32, registered=np.uint8)


def _run(xmamd, c):
    a, k = vn.call_args(c)
    return xmamd.view_graph_filter(*a, **k)


def _as_result(g):
    return dict(inlier=g.inlier, pair_inliers=g.pair_inliers, pair_status=g.pair_status, registered=g.registered, moff_out=g.matches[0],
                f1_out=g.matches[1], f2_out=g.matches[2])


def _same(g, ref, what=""):
    for f in ARRAYS:
        assert getattr(g, f).dtype == DTYPES[f] and np.array_equal(getattr(g, f), ref[f]), (what, f)
    mo, o1, o2 = g.matches
    assert mo.dtype == np.int64 and o1.dtype == np.int32 and o2.dtype == np.int32
    assert np.array_equal(mo, ref["moff_out"]) and np.array_equal(o1, ref["f1_out"]) and np.array_equal(o2, ref["f2_out"]), what
    assert {k: g.info[k] for k in vn.INFO_FIELDS} == ref["info"], what
    assert np.array_equal(g.valid, (ref["pair_status"] == vn.VALID).astype(np.uint8))
    assert 0 <= g.info["rounds"] < 1024
    assert min(g.info["seconds_index"], g.info["seconds_kernels"], g.info["seconds_download"]) >= 0.0


def _identical(a, b, what=""):
    for f in ARRAYS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)
    for x, y in zip(a.matches, b.matches):
        assert np.array_equal(x, y), what
    assert {k: a.info[k] for k in vn.INFO_FIELDS} == {k: b.info[k] for k in vn.INFO_FIELDS}, what


@pytest.fixture(scope="module")
def cases(xmamd):
    """every case with its restatement (computed once) and the library's answer"""
    xmamd.require_gpu()
    lim = xmamd.view_graph_limits()
    out = vn.gpu_cases(lim)
    a, ra, b, rb, rec = vn.load_case()
    out["simple2_a"], out["simple2_b"] = dict(a, ref=ra), dict(b, ref=rb)
    for name, c in out.items():
        if "ref" not in c:
            c["ref"] = vn.run_numpy(c, lim)
        c["got"] = _run(xmamd, c)
    out["record"] = rec
    out["limits"] = lim
    return out


NAMES = ("simple2_a", "simple2_b", "sizes", "essential_edges", "fundamental_edges", "homography", "rules", "rules_no_minimum", "rotation", "rotation_off",
         "chain", "two_equal", "none_valid", "isolated_twice")


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_contract(cases, name):
    _same(cases[name]["got"], cases[name]["ref"], name)


def test_recorded_case(cases):
    """both passes against the file (the device's pass B is fed with the DEVICE's pass A)"""
    rec, a = cases["record"], cases["simple2_a"]
    assert vn.digest(a) == str(rec["digest"])
    ga = a["got"]
    assert np.array_equal(np.packbits(ga.inlier), rec["a_inlier_bits"]) and np.array_equal(np.diff(ga.pair_inliers, prepend=np.int32(0)), rec["a_pair_inliers_diff"])
    assert np.array_equal(ga.pair_status, rec["a_status"]) and np.array_equal(ga.registered, rec["a_registered"])
    assert [ga.info[k] for k in vn.INFO_FIELDS] == rec["a_info"].tolist() and vn.digest_matches(_as_result(ga)) == str(rec["a_matches"])
    gb = cases["simple2_b"]["got"]
    assert np.array_equal(gb.pair_status, rec["b_status"]) and np.array_equal(gb.registered, rec["b_registered"])
    assert [gb.info[k] for k in vn.INFO_FIELDS] == rec["b_info"].tolist() and vn.digest_matches(_as_result(gb)) == str(rec["b_matches"])
    # every status, every model, and an image that leaves the largest component in pass B
    assert set(ga.pair_status.tolist()) | set(gb.pair_status.tolist()) == {0, 1, 2, 3, 4, 5} and {ga.info["pairs_" + m] > 0 for m in ("none", "E", "F", "H")} == {True}
    assert np.any((ga.registered != 0) & (gb.registered == 0))
    assert ga.info["largest"] == 93 and gb.info["largest"] == 91 and gb.info["pairs_outside"] == 1


def test_every_kernel_form_ran(cases):
    c, lim = cases["sizes"], cases["limits"]
    i = c["got"].info
    cnt = np.diff(c["moff"])
    assert {0, 1, 63, 64, 65, 255, 256, 257, lim["wave_matches"], lim["wave_matches"] + 1, lim["group_matches"], lim["group_matches"] + 1,
            2 * lim["group_matches"] + 1} <= set(cnt.tolist())
    assert i["pairs_wave"] == int(np.sum((cnt > 0) & (cnt <= lim["wave_matches"]))) > 0
    assert i["pairs_group"] == int(np.sum((cnt > lim["wave_matches"]) & (cnt <= lim["group_matches"]))) > 0
    assert i["pairs_workspace"] == int(np.sum(cnt > lim["group_matches"])) >= 6 and i["max_matches"] == 2 * lim["group_matches"] + 1
    # every model in every form, with inliers and with matches that are none
    for lo, hi in ((1, lim["wave_matches"]), (lim["wave_matches"] + 1, lim["group_matches"]), (lim["group_matches"] + 1, 10 ** 9)):
        for m in (vn.E_, vn.F_, vn.H_):
            k = np.flatnonzero((cnt >= max(lo, 60)) & (cnt <= hi) & (c["model"] == m))
            assert k.size and np.all(c["got"].pair_inliers[k] > 0) and np.all(c["got"].pair_inliers[k] < cnt[k])


def test_hand_made_cases_give_what_they_are_built_for(cases):
    _, want = vn.essential_edges_case()
    assert np.array_equal(cases["essential_edges"]["got"].inlier, want)
    _, want = vn.fundamental_edges_case()
    assert np.array_equal(cases["fundamental_edges"]["got"].inlier, want)
    assert cases["fundamental_edges"]["got"].pair_inliers.tolist() == [0, 3, 3, 0, 2]
    assert cases["homography"]["got"].pair_inliers.tolist() == [12, 5]
    assert cases["rules"]["got"].pair_status.tolist() == [vn.FEW_INLIERS, vn.VALID, vn.VALID, vn.LOW_RATIO, vn.FEW_INLIERS, vn.INVALID_IN, vn.FEW_INLIERS, vn.OUTSIDE]
    assert cases["rules_no_minimum"]["got"].pair_status.tolist()[6] in (vn.VALID, vn.OUTSIDE) and cases["rules_no_minimum"]["got"].pair_inliers[6] == 0
    assert cases["rules_no_minimum"]["ref"]["pair_status"].tolist()[:4] == [vn.VALID, vn.VALID, vn.VALID, vn.LOW_RATIO]
    # c == the threshold stays; 25 degrees goes; the pair with an unregistered end is skipped; without rot nothing goes
    assert cases["rotation"]["got"].pair_status.tolist() == [0, 0, vn.ROTATION, 0, 0, 0, 0, 0]
    assert cases["rotation_off"]["got"].pair_status.tolist() == [0] * 8
    g = cases["chain"]["got"]
    assert g.info["largest"] == 1500 and g.info["components"] == 1 and g.registered.all() and 1 <= g.info["rounds"] < 1024
    g = cases["two_equal"]["got"]                      # {5, 6, 7} and {1, 3, 8}: the component with image 1 wins
    assert g.registered.tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 1] and g.info["components"] == 3 and g.info["largest"] == 3
    assert g.pair_status.tolist() == [vn.OUTSIDE, vn.OUTSIDE, 0, 0, vn.OUTSIDE]
    g = cases["none_valid"]["got"]
    assert not g.registered.any() and g.info["largest"] == 0 and g.info["components"] == 0 and g.pair_status.tolist() == [1, 1]
    g = cases["isolated_twice"]["got"]
    assert g.registered.tolist() == [0, 1, 1, 0, 1, 0, 0] and g.pair_status.tolist() == [0, 0, 0, vn.OUTSIDE, 0]


def test_feature_index_out_of_range_is_refused(xmamd, cases):
    c = dict(cases["homography"])
    for f, bad in (("f1", -1), ("f2", 10 ** 6)):
        d = dict(c); d[f] = c[f].copy(); d[f][7] = bad
        with pytest.raises(xmamd.XmError, match="feature index out of range at match 7 \\(pair 0\\)"):
            _run(xmamd, d)


def test_two_calls_give_identical_bits(xmamd, cases):
    for name in ("simple2_a", "simple2_b", "sizes"):
        _identical(_run(xmamd, cases[name]), cases[name]["got"], name)


@pytest.mark.parametrize("name", ("simple2_a", "simple2_b", "sizes"))
def test_permuted_pairs_permute_the_outputs(xmamd, cases, name):
    c = cases[name]
    d, order, idx = vn.permuted(c, 21)
    g, h = c["got"], _run(xmamd, d)
    assert np.array_equal(h.registered, g.registered)
    assert np.array_equal(h.pair_status, g.pair_status[order]) and np.array_equal(h.pair_inliers, g.pair_inliers[order])
    assert np.array_equal(h.inlier, g.inlier[idx])
    assert {k: h.info[k] for k in vn.INFO_FIELDS} == {k: g.info[k] for k in vn.INFO_FIELDS}
    mo, o1, o2 = h.matches
    for x, k in enumerate(order):
        a, b = g.matches[0][k], g.matches[0][k + 1]
        assert np.array_equal(o1[mo[x]:mo[x + 1]], g.matches[1][a:b]) and np.array_equal(o2[mo[x]:mo[x + 1]], g.matches[2][a:b])


def _planted_chain(xmamd, turn=None):
    """10 cameras over 60 points, all 45 E pairs with their exact geometry (Rrel of pair `turn` is turned by 30 degrees for pass B only).  Pass A, the
    view-graph solve over the surviving pairs with M_e = Rrel_e^T, recovery, pass B's case.  The solve's model is Y_i = M_e Y_j with Y_i the
    i-th 3 x 3 block of the solution, so Y_i = C_i G for the cam_from_world rotations C and one rotation G of the world, and
    recover_rotations returns the blocks Y_0 Y_i^T = C_0 C_i^T: cam_from_world is the TRANSPOSE of a recovered block"""
    rng = np.random.default_rng(1)
    n, npts = 10, 60
    Rw = np.stack([vn.rot_axis(rng.normal(size=3), rng.uniform(0, 60)) for _ in range(n)])
    X = np.concatenate([rng.uniform(-1, 1, (npts, 2)), rng.uniform(4, 6, (npts, 1))], axis=1)
    tw = rng.uniform(-0.6, 0.6, (n, 3))
    f = rng.uniform(500, 800, n)
    K = np.stack([np.array([[f[i], 0, 320.0], [0, f[i], 240.0], [0, 0, 1.0]]) for i in range(n)])
    xy = np.zeros((n * npts, 2))
    for i in range(n):
        q = X @ Rw[i].T + tw[i]
        xy[i * npts:(i + 1) * npts] = (q[:, :2] / q[:, 2:3]) * f[i] + [320.0, 240.0]
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            R = Rw[j] @ Rw[i].T                                  # exact relative rotations
            t = tw[j] - R @ tw[i]
            idx = rng.permutation(npts)[:45]
            pairs.append(dict(i=i, j=j, model=vn.E_, m=np.stack([idx, idx], axis=1), R=R, t=t / np.linalg.norm(t)))
    c = vn.make_case([npts] * n, xy, pairs, focal=f, Kinv=np.linalg.inv(K))
    Rpass_b = c["Rrel"].copy()
    if turn is not None:
        Rpass_b[turn] = vn.rot_axis([0.5, 0.5, -0.7], 30.0) @ Rpass_b[turn]
    ga = _run(xmamd, c)
    _same(ga, vn.run_numpy(c), "planted, pass A")
    assert ga.valid.all() and ga.registered.all() and ga.info["inliers"] > 35 * len(pairs)
    pi, pj, Rv = ga.pairs()
    ctx = xmamd.Context(vg=(pi, pj, np.ones(pi.size), np.ascontiguousarray(np.transpose(Rv, (0, 2, 1)))), n=n)
    Rs, s, info = ctx.solve(5, 1e-9, 20.0)
    rot, scale, _ = xmamd.recover_rotations(Rs, s)
    ctx.close()
    assert info["status"] == 1 and info["rank"] == 3
    blocks = np.stack([rot[:, 3 * i:3 * i + 3].T for i in range(n)])
    ra = _as_result(ga)
    b = vn.next_pass(dict(c, Rrel=Rpass_b), ra, blocks)
    return c, b, blocks, Rw


def test_planted_chain_drops_nothing_and_then_exactly_the_turned_pair(xmamd):
    c, b, blocks, Rw = _planted_chain(xmamd)
    # the convention: with M_e = Rrel_e^T over (pi, pj) the transposed recovered blocks are cam_from_world up to one rotation of the world
    cs = vn.rotation_cosine(blocks[c["pi"]], blocks[c["pj"]], c["Rrel"])
    assert np.all(cs > np.cos(np.radians(0.01))), cs.min()
    G = blocks[0].T @ Rw[0]
    assert max(np.abs(blocks[i] @ G - Rw[i]).max() for i in range(len(Rw))) < 1e-4
    wrong = np.ascontiguousarray(np.transpose(blocks, (0, 2, 1)))          # the untransposed blocks are NOT: their relative rotations are conjugated
    assert vn.rotation_cosine(wrong[c["pi"]], wrong[c["pj"]], c["Rrel"]).min() < np.cos(np.radians(1.0))
    gb = _run(xmamd, b)
    _same(gb, vn.run_numpy(b), "planted, pass B")
    assert gb.valid.all() and gb.registered.all() and gb.info["pairs_rotation"] == 0
    c, b, blocks, Rw = _planted_chain(xmamd, turn=17)
    gb = _run(xmamd, b)
    rb = vn.run_numpy(b)
    _same(gb, rb, "planted and turned, pass B")
    assert np.flatnonzero(gb.pair_status != vn.VALID).tolist() == [17] and gb.pair_status[17] == vn.ROTATION
    # the tracks of pass B's matches and registered images are those of the same selection made in numpy
    keep = np.flatnonzero(rb["pair_status"] == vn.VALID)
    sel = np.concatenate([np.arange(b["moff"][k], b["moff"][k + 1]) for k in keep])
    moff = np.concatenate([[0], np.cumsum(np.where(rb["pair_status"] == vn.VALID, np.diff(b["moff"]), 0))]).astype(np.int64)
    t1 = xmamd.build_tracks(b["foff"], b["xy"], b["pi"], b["pj"], gb.matches, registered=gb.registered)
    t2 = xmamd.build_tracks(b["foff"], b["xy"], b["pi"], b["pj"], (moff, b["f1"][sel], b["f2"][sel]), registered=rb["registered"])
    assert t1.m == t2.m > 0 and t1.cam.size == t2.cam.size > 0
    for f in ("cam", "feat", "track", "label"):
        assert np.array_equal(getattr(t1, f), getattr(t2, f)), f
    assert np.array_equal(t1.xy.view(np.uint64), t2.xy.view(np.uint64))
