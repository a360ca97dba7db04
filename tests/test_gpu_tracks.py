"""GPU tests of the track establishment (xm_build_tracks, include/xm_amd.h) against the contract's numpy restatement (run_numpy of
tests/xm_tracks_numpy.py): cam, feat, track, label, m and every integer counter EXACTLY, xy bit for bit, under all three conflict
policies.  tests/test_tracks_numpy.py ties the restatement to the sequential restatement of the reference's fork.

Shapes: the recorded SIMPLE2-derived case (64 549 features, 261 680 matches) and hand-made cases of a few features, except where the
size is the point: chains of 1 500 images (hooking rounds) and images with limits[3], limits[3] + 1, limits[0], limits[0] + 1 touched
features (the three kernel sizes), and one image of 2^20 + 4 features (the second pass of the prefix sums' top kernel)."""
import numpy as np
import pytest

import xm_tracks_numpy as tn

pytestmark = pytest.mark.gpu
ARRAYS = ("cam", "feat", "track", "xy", "label")
MAX_ROUNDS = 1024


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _run(xmamd, c, policy, **kw):
    a, k = tn.call_args(c)
    k.update(kw)
    return xmamd.build_tracks(*a, conflict=policy, **k)


def _same(t, ref, what=""):
    assert t.cam.dtype == np.int32 and t.feat.dtype == np.int32 and t.track.dtype == np.int32 and t.label.dtype == np.int32
    assert t.cam.size == ref["cam"].size and t.m == ref["m"], what
    for f in ("cam", "feat", "track", "label"):
        assert np.array_equal(getattr(t, f), ref[f]), (what, f)
    assert np.array_equal(_bits(t.xy), _bits(ref["xy"])), what
    assert {k: t.info[k] for k in tn.INFO_FIELDS} == ref["info"], what
    assert 0 <= t.info["rounds"] < MAX_ROUNDS
    assert min(t.info["seconds_index"], t.info["seconds_kernels"], t.info["seconds_split"], t.info["seconds_download"]) >= 0.0


def _identical(a, b, what=""):
    for f in ARRAYS:
        assert np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))), (what, f)
    assert a.m == b.m and {k: a.info[k] for k in tn.INFO_FIELDS} == {k: b.info[k] for k in tn.INFO_FIELDS}, what


@pytest.fixture(scope="module")
def cases(xmamd):
    """every case with its restatement (computed once) and the library's answer, per policy"""
    xmamd.require_gpu()
    lim = xmamd.tracks_limits()
    out = tn.gpu_cases(lim)
    out["simple2"], out["record"] = tn.load_case()
    for name, c in out.items():
        if name == "record":
            continue
        c["ref"] = {p: tn.run_numpy(c, p, lim) for p in tn.POLICIES}
        c["got"] = {p: _run(xmamd, c, p) for p in tn.POLICIES}
    return out


NAMES = ("simple2", "one_image", "two_images", "triangle", "lengths", "chain", "chain_permuted", "sizes", "conflict_near", "conflict_far",
         "conflict_chain", "duplicate_match", "duplicate_orientation", "duplicate_pair", "coverage", "unregistered", "max_tracks", "scan_second_pass")


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_contract(cases, name):
    for p in tn.POLICIES:
        _same(cases[name]["got"][p], cases[name]["ref"][p], (name, p))


def test_recorded_case(cases):
    c, rec = cases["simple2"], cases["record"]
    assert tn.digest(c) == str(rec["digest"])
    for p in tn.POLICIES:
        t = c["got"][p]
        assert np.array_equal(t.label, rec["label_" + p]), p
        rows = tn.rows_of(c, rec["label_" + p])
        for f in ("cam", "feat", "track"):
            assert np.array_equal(getattr(t, f), rows[f]), (p, f)
        assert np.array_equal(_bits(t.xy), _bits(rows["xy"]))
        assert {k: t.info[k] for k in tn.INFO_FIELDS} == rec["info_" + p]
    assert c["got"]["split"].cam.size > c["got"]["drop"].cam.size            # the policy matters


def test_empty_and_tiny(cases):
    t = cases["one_image"]["got"]["split"]
    assert t.cam.size == 0 and t.m == 0 and (t.label == tn.UNTOUCHED).all() and t.label.size == 3
    t = cases["two_images"]["got"]["split"]
    assert t.cam.size == 0 and t.label.tolist() == [tn.SHORT, tn.UNTOUCHED, tn.UNTOUCHED, tn.SHORT] and t.info["tracks_short"] == 1
    t = cases["triangle"]["got"]["split"]
    assert t.cam.tolist() == [0, 1, 2] and t.feat.tolist() == [0, 0, 0] and t.track.tolist() == [0, 0, 0] and t.m == 1


def test_length_boundaries(cases):
    t = cases["lengths"]["got"]["split"]                       # chains of 2, 3, 5, 6 observations, min_views 3, max_views 5
    assert t.label[:4].tolist() == [tn.SHORT, 0, 1, tn.LONG]
    assert t.info["tracks_short"] == 1 and t.info["tracks_long"] == 1 and t.m == 2 and np.bincount(t.track).tolist() == [3, 5]


def test_long_chains(cases):
    for name in ("chain", "chain_permuted"):
        t = cases[name]["got"]["split"]
        assert t.m == 1 and t.cam.size == 1500 and (t.track == 0).all() and np.array_equal(t.cam, np.arange(1500))
        print(f"TRACKS_ROUNDS {name}: {t.info['rounds']} hooking rounds")
        assert 1 <= t.info["rounds"] < MAX_ROUNDS


def test_every_size_took_its_path(cases, xmamd):
    lim = xmamd.tracks_limits()
    c = cases["sizes"]
    per_image = np.bincount(np.repeat(np.arange(c["foff"].size - 1), np.diff(c["foff"]))[c["got"]["split"].label != tn.UNTOUCHED])
    for k in (lim["small_rows"], lim["small_rows"] + 1, lim["lds_rows"], lim["lds_rows"] + 1):
        assert np.sum(per_image == k) == 1
    for p in tn.POLICIES:
        i = c["got"][p].info
        assert (i["images_large"], i["images_workspace"]) == (2, 1) and i["images_small"] == np.sum(per_image > 0) - 3
        assert i["max_touched"] == lim["lds_rows"] + 1 and i["components_conflicted"] == 4    # one conflict in each of the four images
    assert c["got"]["split"].info["unions_refused"] == 4 and c["got"]["drop"].info["tracks_conflict"] == 4


def test_conflicts(cases):
    near, far = cases["conflict_near"]["got"], cases["conflict_far"]["got"]
    xy = cases["conflict_near"]["xy"]
    assert np.hypot(*(xy[1] - xy[0])) == 10.0
    xy = cases["conflict_far"]["xy"]
    assert xy[1, 1] - xy[0, 1] == 10.0 + 2.0 ** -40 and xy[1, 0] == xy[0, 0]
    # distance exactly 10 is not "> 10": kept with all four rows, two of them in image 0
    assert near["glomap"].cam.tolist() == [0, 0, 1, 2] and near["glomap"].feat.tolist() == [0, 1, 0, 0] and near["glomap"].m == 1
    assert far["glomap"].cam.size == 0 and (far["glomap"].label[:4] == tn.CONFLICT).all() and far["glomap"].info["tracks_conflict"] == 1
    for t in (near, far):
        assert t["drop"].cam.size == 0 and t["drop"].label[:4].tolist() == [tn.CONFLICT] * 4
        # the split refuses (0.1, 1.0): {0.0, 1.0, 2.0} stays, 0.1 is left alone and too short
        assert t["split"].cam.tolist() == [0, 1, 2] and t["split"].feat.tolist() == [0, 0, 0]
        assert t["split"].label.tolist() == [0, tn.SHORT, 0, 0, tn.UNTOUCHED] and t["split"].info["unions_refused"] == 1
    t = cases["conflict_chain"]["got"]["split"]
    assert t.info["unions_refused"] == 3 and t.m == 2 and t.label.tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 1]


def test_duplicates_change_nothing(cases):
    tri = cases["triangle"]["got"]
    for name in ("duplicate_match", "duplicate_orientation", "duplicate_pair"):
        for p in tn.POLICIES:
            t = cases[name]["got"][p]
            for f in ARRAYS:
                assert np.array_equal(_bits(getattr(t, f)), _bits(getattr(tri[p], f))), (name, p, f)
            assert t.info["matches"] == 4 and t.info["components"] == 1


def test_feature_coverage(cases):
    t = cases["coverage"]["got"]["split"]
    assert t.label.tolist() == [0, tn.UNTOUCHED, 0, tn.UNTOUCHED, 0, tn.SHORT, tn.SHORT]
    assert t.cam.tolist() == [0, 1, 2] and t.feat.tolist() == [0, 0, 0]


def test_unregistered_images(cases):
    t = cases["unregistered"]["got"]["split"]
    # track A reaches three views only through image 2; track B keeps images 0, 1, 3 and its feature of image 2 has a label and no row
    assert t.label.tolist() == [tn.FEW_REGISTERED, 0, tn.FEW_REGISTERED, 0, tn.FEW_REGISTERED, 0, 0]
    assert t.cam.tolist() == [0, 1, 3] and t.feat.tolist() == [1, 1, 0] and t.info["tracks_few_registered"] == 1 and t.m == 1


def test_max_tracks(cases):
    t = cases["max_tracks"]["got"]["split"]                    # lengths 3, 5, 3, 4, 3 at the labels 0 .. 4; max_tracks = 2 keeps three
    assert t.label[:5].tolist() == [tn.BEYOND_MAX, 0, tn.BEYOND_MAX, 1, 2] and t.m == 3 and t.info["tracks_beyond_max"] == 2
    assert np.bincount(t.track).tolist() == [5, 4, 3]


def test_two_calls_give_the_same_bits(cases, xmamd):
    for name in ("simple2", "sizes", "conflict_chain"):
        for p in tn.POLICIES:
            _identical(_run(xmamd, cases[name], p), cases[name]["got"][p], (name, p))


def test_input_order_changes_nothing(cases, xmamd):
    for name, seed in (("simple2", 21), ("sizes", 22), ("conflict_chain", 23), ("conflict_near", 24), ("unregistered", 25), ("max_tracks", 26)):
        d = tn.permuted(cases[name], seed)
        for p in tn.POLICIES:
            _identical(_run(xmamd, d, p), cases[name]["got"][p], (name, p))


def test_refusals(cases, xmamd):
    """every XM_ERR_ARG of the header, from the host's checks and from the device's; the outputs stay as they were"""
    c = cases["conflict_chain"]
    one = lambda a, k, v: np.where(np.arange(a.size) == k, v, a).astype(a.dtype)
    for change, word in ((dict(pj=one(c["pj"], 2, c["pi"][2])), "names one image twice"),
                         (dict(pi=one(c["pi"], 1, 6)), "image index out of range"), (dict(pj=one(c["pj"], 1, -1)), "image index out of range"),
                         (dict(f1=one(c["f1"], 3, 2)), "feature index out of range at match 3"), (dict(f2=one(c["f2"], 9, 1)), "feature index out of range at match 9"),
                         (dict(f1=one(c["f1"], 0, -1)), "feature index out of range at match 0"), (dict(f2=one(c["f2"], 5, 2 ** 31 - 1)), "feature index out of range"),
                         (dict(moff=one(c["moff"], 2, 1)), "moff decreases"), (dict(moff=one(c["moff"], 0, 1)), "moff does not start at 0")):
        with pytest.raises(xmamd.XmError, match=word):
            _run(xmamd, dict(c, **change), "split")
    for kw, word in ((dict(thres_inconsistency=-1.0), "thres_inconsistency"), (dict(thres_inconsistency=float("inf")), "thres_inconsistency"),
                     (dict(thres_inconsistency=float("nan")), "thres_inconsistency"), (dict(min_views=0), "min_views"),
                     (dict(min_views=4, max_views=3), "max_views"), (dict(max_tracks=-1), "max_tracks")):
        with pytest.raises(xmamd.XmError, match=word):
            _run(xmamd, c, "split", **kw)
    with pytest.raises(xmamd.XmError, match="unknown conflict policy"):
        _run(xmamd, c, 7)
    # the C call leaves every output as it was when it refuses on the device
    import ctypes as C
    F = int(c["foff"][-1]); P = lambda a: a.ctypes.data_as(C.c_void_p)
    outs = [np.full(F, 77, dtype=np.int32) for _ in range(4)]; oxy = np.full((F, 2), 7.5); nout = C.c_int64(-5)
    o = xmamd.TracksOptions(); r = xmamd.TracksResult(); r.struct_size = C.sizeof(r); r.ntracks = -9
    bad = one(c["f1"], 3, 2)
    rc = xmamd.lib().xm_build_tracks(c["foff"].size - 1, P(c["foff"]), P(c["xy"]), None, c["pi"].size, P(c["pi"]), P(c["pj"]), P(c["moff"]), P(bad), P(c["f2"]),
                                     C.byref(o), P(outs[0]), P(outs[1]), P(outs[2]), P(oxy), C.byref(nout), P(outs[3]), C.byref(r))
    assert rc == -2 and all((a == 77).all() for a in outs) and (oxy == 7.5).all() and nout.value == -5 and r.ntracks == -9
    for p in tn.POLICIES:
        _identical(_run(xmamd, c, p), c["got"][p], "after the refusals")


def test_carry(cases):
    c = cases["unregistered"]
    t = c["got"]["split"]
    colour = np.arange(int(c["foff"][-1]) * 3).reshape(-1, 3)
    got, = t.carry(colour)
    assert np.array_equal(got, colour[c["foff"][t.cam] + t.feat])


def test_hand_off_to_lift_clean_and_context(xmamd):
    """the table goes into lift_observations as it is, and the list from there into clean_observations and Context(obs=...), which solves"""
    import xm_lift_numpy as ln
    rng = np.random.default_rng(9)
    n, m, h, w = 6, 60, 48, 64
    counts = [m + 2] * n                                       # every image sees every point; two more features stay unmatched
    xy = np.stack([rng.integers(10, w - 10, n * (m + 2)) + 0.5, rng.integers(10, h - 10, n * (m + 2)) + 0.5], axis=1)
    same = np.stack([np.arange(m), np.arange(m)], axis=1)
    c = tn.make_case(counts, [(i, i + 1, same) for i in range(n - 1)] + [(0, n - 1, same[::2])], xy=xy)
    t = _run(xmamd, c, "split")
    assert t.m == m and t.cam.size == n * m
    depth = [ln.grid_depth(rng, h, w) for _ in range(n)]; conf = [rng.uniform(0.2, 1.0, (h, w)).astype(np.float32) for _ in range(n)]
    plan = xmamd.lift_observations(t.cam, t.track, t.xy, depth, conf, ln.intrinsics(n, [(h, w)] * n), n=n, m=t.m)
    assert plan.cam.size > n * m * 0.8
    cl = xmamd.clean_observations(plan.cam, plan.lm, plan.w, n=n, m=t.m)
    assert cl.info["n_new"] == n
    c2, l2, p2, w2 = cl.apply(plan.cam, plan.lm, plan.p, plan.w)
    ctx = xmamd.Context(obs=(c2, l2, p2, w2), n=n)
    R, s, info = ctx.solve(max_rank=6, tol=1e-9, lam=3.0)
    ctx.close()
    assert info["status"] == 1 and np.all(np.isfinite(R)) and np.all(np.isfinite(s))
