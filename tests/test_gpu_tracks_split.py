"""GPU tests of the device split (XM_TRACKS_SPLIT_DEVICE, conflict="split_device"; include/xm_amd.h) against the contract's restatement:
split_numpy and run_numpy(c, "split") of tests/xm_tracks_numpy.py, EXACTLY -- labels, counts, rows, xy bit for bit.  The host splitter
(split_host, conflict="split") is the second witness; the device path is never compared with itself alone.

Shapes: hand-made components of a few features, the recorded SIMPLE2-derived case, and components built to sit exactly on the boundaries
between the three forms (tracks_split_limits(): a wavefront, a workgroup, the host) and to stress the walk over the sorted edges."""
import ctypes as C

import numpy as np
import pytest

import xm_tracks_numpy as tn

pytestmark = pytest.mark.gpu
ARRAYS = ("cam", "feat", "track", "xy", "label")
ZERO = dict(wave=0, group=0, host=0, edges_device=0, edges_host=0, distinct=0, refused=0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


# ------------------------------------------------------------------------------------------------ scenes of raw edges
def conflicted(nend, distinct=None, raw=None):
    """one component of nend >= 3 endpoints: 0 and 1 are two features of one image, every other endpoint has an image of its own; the chain
    0 - 2 - 3 - ... - (nend - 1) - 1 would join the two, so at least one union is refused.  distinct: more edges between chain members until
    that many distinct edges are listed; raw: the edge 0 - 2 is listed again, turned round, until that many edges are listed.
    -> (features per image, edges in local ids)"""
    edges = [(0, 2), (1, nend - 1)] + [(k, k + 1) for k in range(2, nend - 1)]
    span = 2
    while distinct is not None and len(edges) < distinct:
        assert span < nend - 2, "not that many pairs"
        edges += [(k, k + span) for k in range(2, nend - span)][:distinct - len(edges)]
        span += 1
    if raw is not None:
        assert raw >= len(edges)
        edges += [(2, 0)] * (raw - len(edges))
    return [2] + [1] * (nend - 2), np.array(edges, dtype=np.int64)


def scene(comps, seed=0):
    """components (features per image, local edges), each on images of its own -> (foff, eu, ev) with the edges shuffled and half of them
    turned round"""
    counts, eu, ev, base = [], [], [], 0
    for c, e in comps:
        counts += list(c)
        eu.append(e[:, 0] + base); ev.append(e[:, 1] + base)
        base += int(np.sum(c))
    foff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    eu = np.concatenate(eu) if eu else np.zeros(0, np.int64); ev = np.concatenate(ev) if ev else np.zeros(0, np.int64)
    rng = np.random.default_rng(seed)
    q = rng.permutation(eu.size); turn = rng.random(eu.size) < 0.5
    eu, ev = eu[q], ev[q]
    return foff, np.where(turn, ev, eu).astype(np.int32), np.where(turn, eu, ev).astype(np.int32)


def _check(xmamd, foff, eu, ev, what=""):
    """split_device == split_numpy == split_host -> (label, distinct, refused, stats)"""
    F = int(foff[-1])
    label, distinct, refused = xmamd.split_device(foff, F, eu, ev)
    stats = xmamd.tracks_split_stats()
    new, d2, r2 = tn.split_numpy(foff, np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64))
    want = np.full(F, -1, dtype=np.int32)
    for g, v in new.items():
        want[g] = v
    assert label.dtype == np.int32 and np.array_equal(label, want), what
    assert (distinct, refused) == (d2, r2), what
    host, d3, r3 = xmamd.split_host(foff, F, eu, ev)
    assert np.array_equal(host, want) and (d3, r3) == (d2, r2), what
    assert (stats["distinct"], stats["refused"]) == (d2, r2) and stats["edges_device"] + stats["edges_host"] == len(eu), what
    return label, distinct, refused, stats


@pytest.fixture(scope="module")
def lim(xmamd):
    xmamd.require_gpu()
    return xmamd.tracks_split_limits()


@pytest.fixture(scope="module")
def hand(xmamd):
    return tn.gpu_cases(xmamd.tracks_limits())


@pytest.fixture(scope="module")
def simple2(xmamd):
    """the recorded case with its restatement and the host-split table, computed once"""
    xmamd.require_gpu()
    c, rec = tn.load_case()
    return dict(case=c, record=rec, ref=tn.run_numpy(c, "split", xmamd.tracks_limits()), host=_run(xmamd, c, "split"))


# ------------------------------------------------------------------------------------------------ xm_tracks_split_device
def test_small_cases(xmamd, hand, lim):
    for name, labels, counts in (("conflict_near", [0, 1, 0, 0, -1], (3, 1)), ("conflict_chain", [0, 1, 0, 1, 0, 1, 0, 1, 1], (10, 3))):
        c = hand[name]
        eu, ev = tn._global_edges(c)
        label, distinct, refused, st = _check(xmamd, c["foff"], eu, ev, name)
        assert label.tolist() == labels and (distinct, refused) == counts
        assert (st["wave"], st["group"], st["host"]) == ((1, 0, 0) if lim["wave_edges"] else (0, 1, 0))
    # duplicate edges in both orientations, in any order: the same sets and the same counts
    c = hand["conflict_chain"]
    eu, ev = tn._global_edges(c)
    q = np.random.default_rng(3).permutation(eu.size + 5)
    again = _check(xmamd, c["foff"], np.concatenate([eu, ev[:4], eu[-1:]])[q], np.concatenate([ev, eu[:4], ev[-1:]])[q])
    assert again[0].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 1] and again[1:3] == (10, 3) and again[3]["edges_device"] == eu.size + 5
    # no edge at all, and a single one
    none, d, r = xmamd.split_device([3], 3, [], [])
    assert none.tolist() == [-1, -1, -1] and (d, r) == (0, 0) and xmamd.tracks_split_stats() == ZERO
    one = _check(xmamd, np.array([0, 2, 4]), [3], [0])
    assert one[0].tolist() == [0, -1, -1, 0] and one[1:3] == (1, 0)


def test_recorded_case(xmamd, simple2):
    c = simple2["case"]
    eu, ev = tn._global_edges(c)
    label, distinct, refused, st = _check(xmamd, c["foff"], eu, ev, "simple2")   # every component, conflict-free ones included
    assert refused > 0 and np.sum(label >= 0) == 64427 and st["host"] == 0 and xmamd.tracks_split_stats()["host"] == 0


NAMES = ("one_image", "two_images", "triangle", "lengths", "chain", "chain_permuted", "sizes", "conflict_near", "conflict_far", "conflict_chain",
         "duplicate_match", "duplicate_orientation", "duplicate_pair", "coverage", "unregistered", "max_tracks", "scan_second_pass")


@pytest.mark.parametrize("name", NAMES)
def test_hand_made_cases(xmamd, hand, name):
    c = hand[name]
    eu, ev = tn._global_edges(c) if c["pi"].size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    _check(xmamd, c["foff"], eu, ev, name)


def test_the_names_are_all_the_cases(hand):
    assert set(NAMES) == set(hand)


def test_form_boundaries(xmamd, lim):
    we, wr, gr = lim["wave_endpoints"], lim["wave_edges"], lim["group_edges"]
    assert we >= 4 and wr >= 8, "the wavefront form is not built: its boundaries cannot be tested"
    small = min(we, 40)                                        # endpoints of the components whose edges are the point
    assert (small - 2) * (small - 3) // 2 >= wr + 1 and 117 * 118 // 2 >= gr + 1
    for what, comp, form in (("wave_endpoints", conflicted(we), "wave"), ("wave_endpoints + 1", conflicted(we + 1), "group"),
                             ("wave_edges", conflicted(small, distinct=wr), "wave"), ("wave_edges + 1", conflicted(small, distinct=wr + 1), "group"),
                             ("group_edges", conflicted(120, distinct=gr), "group"), ("group_edges + 1", conflicted(120, distinct=gr + 1), "host")):
        foff, eu, ev = scene([comp], seed=len(what))
        assert eu.size == {"wave_endpoints": we - 1, "wave_endpoints + 1": we, "wave_edges": wr, "wave_edges + 1": wr + 1, "group_edges": gr,
                           "group_edges + 1": gr + 1}[what]
        label, distinct, refused, st = _check(xmamd, foff, eu, ev, what)
        assert refused >= 1 and distinct == eu.size, what
        assert {k: st[k] for k in ("wave", "group", "host")} == {k: int(k == form) for k in ("wave", "group", "host")}, what
        assert (st["edges_device"], st["edges_host"]) == ((0, eu.size) if form == "host" else (eu.size, 0)), what
    # raw edges above a cap, distinct edges below it (one pair listed three times): equal, whichever form takes it
    for what, comp in (("wave", conflicted(small, distinct=wr - 1, raw=wr + 1)), ("group", conflicted(120, distinct=gr - 1, raw=gr + 1))):
        foff, eu, ev = scene([comp], seed=7)
        label, distinct, refused, st = _check(xmamd, foff, eu, ev, what)
        assert distinct == eu.size - 2 and refused >= 1 and st["wave"] + st["group"] + st["host"] == 1


def test_one_call_mixes_the_three_forms(xmamd, lim):
    we, wr, gr = lim["wave_endpoints"], lim["wave_edges"], lim["group_edges"]
    comps = [conflicted(120, distinct=gr + 1), conflicted(5), conflicted(we + 1), conflicted(3), conflicted(120, distinct=gr), conflicted(we),
             conflicted(130, distinct=gr + 9), conflicted(min(we, 40), distinct=wr)]
    foff, eu, ev = scene(comps, seed=11)
    label, distinct, refused, st = _check(xmamd, foff, eu, ev)
    assert (st["wave"], st["group"], st["host"]) == (4, 2, 2) and refused >= 8
    assert st["edges_host"] == 2 * gr + 10 and st["edges_device"] == eu.size - st["edges_host"]


def test_shapes_that_stress_the_walk(xmamd, lim):
    k, gr = lim["wave_endpoints"], lim["group_edges"]
    # a star: one feature of image 0 matched to k features of image 1
    star = ([1, k], np.stack([np.zeros(k, dtype=np.int64), np.arange(1, k + 1)], axis=1))
    foff, eu, ev = scene([star], seed=1)
    label, distinct, refused, st = _check(xmamd, foff, eu, ev, "star")
    assert (distinct, refused) == (k, k - 1) and label.tolist() == [0, 0] + list(range(2, k + 1))
    # a complete bipartite block between the six features of a hub image and two features in each of 12 images: dense, most edges skipped
    a, b = np.meshgrid(np.arange(6), np.arange(6, 30), indexing="ij")
    block = ([6] + [2] * 12, np.stack([a.reshape(-1), b.reshape(-1)], axis=1))
    foff, eu, ev = scene([block], seed=2)
    label, distinct, refused, st = _check(xmamd, foff, eu, ev, "block")
    assert distinct == 144 and refused > 0 and st["wave"] + st["group"] == 1
    # a path of group_edges edges through images that each appear twice: first the even endpoints, then the odd ones
    order = np.concatenate([np.arange(0, gr + 1, 2), np.arange(1, gr + 1, 2)])
    path = ([2] * (gr // 2) + [1], np.stack([order[:-1], order[1:]], axis=1))
    foff, eu, ev = scene([path], seed=3)
    label, distinct, refused, st = _check(xmamd, foff, eu, ev, "path")
    assert distinct == gr and refused > 0 and (st["wave"], st["group"], st["host"]) == (0, 1, 0)
    # 3 000 components of three endpoints with a conflict each: more teams than one pass over the CUs
    foff, eu, ev = scene([conflicted(3)] * 3000, seed=4)
    label, distinct, refused, st = _check(xmamd, foff, eu, ev, "many")
    assert (distinct, refused) == (6000, 3000) and st["wave"] + st["group"] == 3000 and st["host"] == 0


def test_seeded_random_scenes(xmamd):
    rng = np.random.default_rng(2024)
    comps = []
    for _ in range(2000):
        counts = rng.integers(1, 7, rng.integers(2, 13))
        img = np.repeat(np.arange(counts.size), counts)
        a, b = np.triu_indices(img.size, 1)
        on = (img[a] != img[b]) & (rng.random(a.size) < 0.3)
        comps.append((counts, np.stack([a[on], b[on]], axis=1)))
    foff, eu, ev = scene(comps, seed=5)
    label, distinct, refused, st = _check(xmamd, foff, eu, ev, "random")
    assert refused > 0 and st["host"] == 0 and st["wave"] > 0


# ------------------------------------------------------------------------------------------------ through xm_build_tracks
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
    assert min(t.info["seconds_index"], t.info["seconds_kernels"], t.info["seconds_split"], t.info["seconds_download"]) >= 0.0


def _identical(a, b, what=""):
    for f in ARRAYS:
        assert np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))), (what, f)
    assert a.m == b.m and {k: a.info[k] for k in tn.INFO_FIELDS} == {k: b.info[k] for k in tn.INFO_FIELDS}, what


def _tie_case():
    """tracks of 3, 5, 3, 4 and 3 observations and a conflicted component that the split turns into one of 3 and a part too short; max_tracks = 2
    keeps three, the tie at the cut goes to the larger label"""
    pairs = [(k, k + 1, [(c, c) for c, L in enumerate((3, 5, 3, 4, 3)) if k + 1 < L]) for k in range(4)]
    return tn.make_case([5] * 5 + [2, 1, 2], pairs + [(5, 6, [(0, 0), (1, 0)]), (6, 7, [(0, 0)])], max_tracks=2)


def test_tracks_recorded_case(xmamd, simple2):
    c, ref = simple2["case"], simple2["ref"]
    t = _run(xmamd, c, "split_device")
    st = xmamd.tracks_split_stats()
    _same(t, ref, "simple2")
    _identical(t, simple2["host"], "simple2 against the host split")
    assert np.array_equal(t.label, simple2["record"]["label_split"])
    assert st["wave"] + st["group"] == t.info["components_conflicted"] == 169 and st["host"] == 0
    assert (st["distinct"], st["refused"]) == (t.info["edges_split"], t.info["unions_refused"]) and t.info["seconds_split"] > 0.0
    _identical(_run(xmamd, c, "split_device"), t, "a second call")
    _identical(_run(xmamd, tn.permuted(c, 21), "split_device"), t, "permuted")


@pytest.mark.parametrize("name", NAMES + ("tie",))
def test_tracks_equal_the_contract(xmamd, hand, name):
    c = _tie_case() if name == "tie" else hand[name]
    ref = tn.run_numpy(c, "split", xmamd.tracks_limits())
    t = _run(xmamd, c, "split_device")
    st = xmamd.tracks_split_stats()
    _same(t, ref, name)
    assert st["wave"] + st["group"] + st["host"] == t.info["components_conflicted"]
    _identical(t, _run(xmamd, c, "split"), name)
    assert xmamd.tracks_split_stats() == ZERO                   # the host split leaves them at 0
    _identical(_run(xmamd, c, "split_device"), t, name)
    if c["pi"].size:
        _identical(_run(xmamd, tn.permuted(c, 31), "split_device"), t, name)
    if name == "conflict_near":                                # the split leaves 0.1 alone, and too short
        assert t.label.tolist() == [0, tn.SHORT, 0, 0, tn.UNTOUCHED] and t.info["unions_refused"] == 1 and st["wave"] + st["group"] == 1
    if name == "tie":
        assert t.label[:5].tolist() == [tn.BEYOND_MAX, 0, tn.BEYOND_MAX, 1, tn.BEYOND_MAX] and t.m == 3 and t.info["tracks_beyond_max"] == 3
        assert t.info["tracks_short"] == 1 and t.info["unions_refused"] == 1


def test_no_conflict_launches_no_split(xmamd, hand):
    for name in ("triangle", "chain", "unregistered"):
        t = _run(xmamd, hand[name], "split_device")
        assert xmamd.tracks_split_stats() == ZERO and t.info["seconds_split"] == 0.0 and t.info["components_conflicted"] == 0


def test_refusal_on_the_device_writes_nothing(xmamd, hand):
    c = hand["conflict_chain"]
    F = int(c["foff"][-1]); P = lambda a: a.ctypes.data_as(C.c_void_p)
    outs = [np.full(F, 77, dtype=np.int32) for _ in range(4)]; oxy = np.full((F, 2), 7.5); nout = C.c_int64(-5)
    o = xmamd.TracksOptions(flags=xmamd.TRACKS_SPLIT_DEVICE); r = xmamd.TracksResult(); r.struct_size = C.sizeof(r); r.ntracks = -9
    bad = c["f1"].copy(); bad[3] = 2
    rc = xmamd.lib().xm_build_tracks(c["foff"].size - 1, P(c["foff"]), P(c["xy"]), None, c["pi"].size, P(c["pi"]), P(c["pj"]), P(c["moff"]), P(bad), P(c["f2"]),
                                     C.byref(o), P(outs[0]), P(outs[1]), P(outs[2]), P(oxy), C.byref(nout), P(outs[3]), C.byref(r))
    assert rc == -2 and "feature index out of range at match 3" in xmamd.lib().xm_last_error().decode()
    assert all((a == 77).all() for a in outs) and (oxy == 7.5).all() and nout.value == -5 and r.ntracks == -9
    with pytest.raises(xmamd.XmError, match="feature index out of range at match 3"):
        _run(xmamd, dict(c, f1=bad), "split_device")
    _same(_run(xmamd, c, "split_device"), tn.run_numpy(c, "split", xmamd.tracks_limits()), "after the refusal")


def test_hand_off_to_lift_clean_and_context(xmamd):
    """the table of a scene with a conflict goes into lift_observations as it is, and the list from there into clean_observations and
    Context(obs=...), which solves"""
    import xm_lift_numpy as ln
    rng = np.random.default_rng(9)
    n, m, h, w = 6, 60, 48, 64
    counts = [m + 2] * n                                       # every image sees every point; two more features per image
    xy = np.stack([rng.integers(10, w - 10, n * (m + 2)) + 0.5, rng.integers(10, h - 10, n * (m + 2)) + 0.5], axis=1)
    same = np.stack([np.arange(m), np.arange(m)], axis=1)
    # image 0's feature m is matched into the track of point 0: that component holds two features of image 0
    c = tn.make_case(counts, [(i, i + 1, same) for i in range(n - 1)] + [(0, n - 1, same[::2]), (0, 3, [(m, 0)])], xy=xy)
    t = _run(xmamd, c, "split_device")
    st = xmamd.tracks_split_stats()
    _same(t, tn.run_numpy(c, "split", xmamd.tracks_limits()))
    _identical(t, _run(xmamd, c, "split"))
    assert t.m >= m and t.cam.size >= n * m and t.info["unions_refused"] >= 1 and st["wave"] + st["group"] == 1
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
