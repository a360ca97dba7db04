"""CPU tests of the two restatements of the track filter (tests/xm_trackfilter_numpy.py) -- the sequential one that follows
track_filter.cc line by line and the vectorised contract the GPU tests compare with agree exactly on every scene of the GPU tests -- and of
the loop of global_mapper.cc:243-317: its restatement against hand-traced sequences, and Context.refine_filtered against the restatement
with the context's methods replaced (no GPU)."""
import os

import numpy as np
import pytest

import xm_trackfilter_numpy as tf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETTINGS = (dict(reprojection=tf.TIGHT["reprojection"]), dict(reprojection=None, angle=tf.TIGHT["angle"]),
            dict(reprojection=None, triangulation=tf.TIGHT["triangulation"]), dict(**tf.TIGHT), dict(min_views=3, **tf.TIGHT),
            dict(reprojection=1e-2, angle=1.0, triangulation=1.0))


def _agree(S, **kw):
    a, b = tf.run_sequential(S, **kw), tf.run_numpy(S, **kw)
    assert tf.same(a, b) == [], (kw, tf.same(a, b))
    assert b["obs_kept"] + sum(b["dropped_" + k] for k in ("depth", "reprojection", "angle", "triangulation", "min_views")) == b["obs_used"]
    return b


@pytest.mark.parametrize("scene", ["boundary", "tile", "flags", "depth"])
def test_restatements_agree_on_the_hand_made_scenes(scene):
    S = getattr(tf, scene + "_scene")()
    for kw in SETTINGS:
        _agree(S, **kw)
        T, perm = tf.permuted(S, seed=5)
        a, b = tf.run_numpy(S, **kw), _agree(T, **kw)
        assert np.array_equal(a["keep"][perm], b["keep"]) and np.array_equal(a["reason"][perm], b["reason"])
        assert np.array_equal(a["lm_views"], b["lm_views"]) and np.array_equal(a["lm_status"], b["lm_status"])


def test_the_scenes_hold_what_they_are_named_for():
    S = tf.boundary_scene()
    deg = np.bincount(S["lm"], minlength=S["m"])
    assert set((0, 1, 2, 3, tf.LIGHT_MAX - 1, tf.LIGHT_MAX, tf.LIGHT_MAX + 1, tf.LIGHT_MAX + 2)) <= set(deg.tolist())
    assert set(np.bincount(tf.tile_scene()["lm"]).tolist()) >= {tf.TILE - 1, tf.TILE, tf.TILE + 1, 2 * tf.TILE + 1}
    for S in (tf.boundary_scene(), tf.tile_scene()):                # each filter drops part of the scene, not nothing and not everything
        for kw, key in ((SETTINGS[0], "dropped_reprojection"), (SETTINGS[1], "dropped_angle")):
            b = tf.run_numpy(S, **kw)
            assert 0.01 * b["obs_used"] < b[key] < 0.9 * b["obs_used"]
    b = tf.run_numpy(tf.boundary_scene(), **SETTINGS[2])
    assert 0 < b["tracks_changed_triangulation"] < b["tracks_total"]
    F = tf.flags_scene()
    b = _agree(F, reprojection=1e-2, triangulation=1.0)
    assert b["lm_status"].tolist() == [tf.LM_KEPT, tf.LM_KEPT, tf.LM_UNUSED, tf.LM_TRIANGULATION, tf.LM_TRIANGULATION]
    assert b["reason"][12:15].tolist() == [tf.REASON_DEPTH] * 3 and b["reason"][17] == tf.REASON_REPROJECTION
    assert b["reason"][15:17].tolist() == [tf.REASON_TRIANGULATION] * 2             # triangulation saw only the survivors of landmark 4
    assert tf.run_numpy(F, reprojection=None, triangulation=1.0)["lm_status"][4] == tf.LM_KEPT   # ... with the displaced one it has a wide pair
    assert not b["keep"][[8, 9, 10, 11]].any() and not b["reason"][[8, 9, 10, 11]].any()          # unused: neither kept nor dropped
    D = tf.depth_scene()
    for kw in (dict(reprojection=1e-2), dict(reprojection=None, angle=1.0)):
        assert _agree(D, **kw)["reason"].tolist() == [0, 0, 0, tf.REASON_DEPTH, 0, tf.REASON_DEPTH]   # EPS / 2 and -1 out, 2 EPS in
    assert _agree(D, reprojection=None, triangulation=1.0)["dropped_depth"] == 0                      # no per-observation filter: no depth test


@pytest.mark.parametrize("k", [2, 3, tf.LIGHT_MAX, tf.LIGHT_MAX + 6])
@pytest.mark.parametrize("where", ["first", "last", "split", "none"])
def test_restatements_agree_on_the_pair_designs(k, where):
    b = _agree(tf.pair_scene(k, where), reprojection=None, triangulation=1.0)
    assert b["lm_status"][1] == (tf.LM_TRIANGULATION if where == "none" else tf.LM_KEPT)
    assert b["lm_views"][1] == (0 if where == "none" else k)


def test_a_value_equal_to_the_threshold_does_not_pass():
    for name, S, kw, i in tf.threshold_cases():
        b = _agree(S, **kw)
        _, q, _ = tf.geometry(S)
        if name == "reprojection":
            assert tf.reprojection_error(S, q)[i] == kw["reprojection"] and b["reason"][i] == tf.REASON_REPROJECTION      # strict <
            kw2 = dict(kw, reprojection=float(np.nextafter(kw["reprojection"], 1.0)))
            assert tf.run_numpy(S, **kw2)["keep"][i]
        elif name == "angle":
            assert tf.angle_cosine(S, q)[i] == tf.cos_deg(kw["angle"]) and b["reason"][i] == tf.REASON_ANGLE              # strict >
            assert tf.run_numpy(S, reprojection=None, angle=1.0, cos_angle=float(np.nextafter(tf.cos_deg(kw["angle"]), 0.0)))["keep"][i]
        else:
            r = tf.rays(tf.geometry(S)[0])
            assert (r[0, 0] * r[1, 0] + r[0, 1] * r[1, 1]) + r[0, 2] * r[1, 2] == tf.cos_deg(kw["triangulation"])
            assert b["lm_status"][i] == tf.LM_TRIANGULATION                                                              # strict <
            ct = float(np.nextafter(tf.cos_deg(kw["triangulation"]), 2.0))
            assert tf.run_numpy(S, reprojection=None, triangulation=1.0, cos_triangulation=ct)["lm_status"][i] == tf.LM_KEPT


def test_restatements_agree_on_the_recorded_case():
    S = tf.simple2(GOLDEN)
    b = _agree(S, reprojection=1e-2, angle=1.0, triangulation=1.0)
    assert b["obs_kept"] == b["obs_used"] == S["cam"].size and b["tracks_kept"] == b["tracks_total"]   # GLOMAP's defaults drop nothing here
    _agree(S, min_views=3, **tf.SIMPLE2_TIGHT)


# ------------------------------------------------------------------------------------------------ the loop
def _trace(changed_of, total=1000, rounds=3):
    """refine_loop with a fake filter whose count of changed tracks is changed_of(scaling)"""
    log = []
    calls = tf.refine_loop(lambda fix: log.append(("ba", fix)),
                           lambda rep, tri, sc: (log.append(("filter", rep, tri)) or (changed_of(sc) if rep is not None else 0, total)),
                           rounds=rounds, reprojection=1e-2, triangulation=1.0)
    assert calls == log
    return calls


BA2 = [("ba", True), ("ba", False)]
F = lambda s: ("filter", s * 1e-2, None)
TAIL = [("filter", 1e-2, None), ("filter", None, 1.0)]


def test_loop_against_hand_traced_sequences():
    # never above 0.1 %: one round of adjustments, the filter at 3x, 2x, 1x inside the while (:284-297), then the break (:298-301)
    assert _trace(lambda sc: 0) == BA2 + [F(3), F(2), F(1)] + TAIL
    assert _trace(lambda sc: 1, total=3001) == BA2 + [F(3), F(2), F(1)] + TAIL        # 1 + 1 + 1 = 3 <= 3.001: filtered_num accumulates
    assert _trace(lambda sc: 1, total=2999) == BA2 + [F(3), F(2), F(1)] + TAIL  # ... 3 > 2.999 at the third: status false, ite = 3 ends the for
    # always above: exactly `rounds` rounds with the scalings 3, 2, 1
    assert _trace(lambda sc: 500) == BA2 + [F(3)] + BA2 + [F(2)] + BA2 + [F(1)] + TAIL
    assert _trace(lambda sc: 500, rounds=5) == BA2 + [F(3)] + BA2 + [F(2)] + BA2 + [F(1)] + BA2 + [F(1)] + BA2 + [F(1)] + TAIL
    # above only at scaling 1: the while runs 3x, 2x, 1x in the first round; the third sets status false and the for ends with ite = 3
    assert _trace(lambda sc: 500 if sc == 1 else 0) == BA2 + [F(3), F(2), F(1)] + TAIL
    # above only at scaling 2: one round reaches 2x, the next one filters at 1x
    assert _trace(lambda sc: 500 if sc == 2 else 0) == BA2 + [F(3), F(2)] + BA2 + [F(1)] + TAIL
    assert _trace(lambda sc: 0, rounds=0) == TAIL


class _Plan:
    def __init__(self, nobs, drop, changed, total, tri):
        self.reason = np.zeros(nobs, dtype=np.uint8)
        self.reason[drop] = 1
        self.keep = self.reason == 0
        self.info = dict(tracks_changed_reprojection=0 if tri else changed, tracks_changed_triangulation=changed if tri else 0, tracks_total=total)

    def weights(self, w):
        w = np.array(w, dtype=np.float64)
        w[self.reason != 0] = 0.0
        return w


# (what the 0.1 % rule does at the end: `never` and `only_at_2` leave the while with status still true, :298-301)
@pytest.mark.parametrize("changed_of,early", [(lambda sc: 0, True), (lambda sc: 500, False), (lambda sc: 500 if sc == 1 else 0, False),
                                              (lambda sc: 500 if sc == 2 else 0, True)], ids=["never", "always", "only_at_1", "only_at_2"])
def test_refine_filtered_makes_the_calls_of_the_restatement(xmamd, changed_of, early):
    nobs = 40
    ctx = xmamd.Context.__new__(xmamd.Context)
    ctx.n, ctx.n_landmarks, ctx.ne, ctx.h, ctx._w = 2, 3, nobs, None, np.ones(nobs)
    log, sets, k = [], [], [0]

    def bundle_adjust(rot, t, P, fix_rotations=False, **kw):
        assert kw == dict(max_iters=7)
        log.append(("ba", fix_rotations))
        return rot + 1, t, P, dict(status=1, status_name="function_tolerance", iters=1, initial_cost=1.0, final_cost=0.5, n_used=nobs)

    def filter_tracks(rot, t, P, reprojection=1e-2, angle=None, triangulation=None, min_views=0):
        assert angle is None and min_views == 2
        log.append(("filter", reprojection, triangulation))
        sc = round(reprojection / 1e-2) if reprojection is not None else 1
        changed = changed_of(sc) if reprojection is not None else 0
        k[0] += 1
        return _Plan(nobs, [k[0]] if changed else [], changed, 1000, triangulation is not None)
    ctx.bundle_adjust, ctx.filter_tracks, ctx.set_edge_weights = bundle_adjust, filter_tracks, lambda w: sets.append(np.array(w))
    rot, t, P, info = ctx.refine_filtered(np.zeros((3, 6)), np.zeros((3, 2)), np.zeros((3, 3)), rounds=3, reprojection=1e-2, triangulation=1.0,
                                          min_views=2, restore_weights=True, max_iters=7)
    want = tf.refine_loop(lambda fix: None, lambda rep, tri, sc: (changed_of(sc) if rep is not None else 0, 1000), rounds=3, reprojection=1e-2,
                          triangulation=1.0)
    assert log == want
    n_ba = sum(1 for c in log if c[0] == "ba")
    assert rot[0, 0] == n_ba and len(info["rounds"]) == n_ba // 2
    dropping = sum(1 for c in log if c[0] == "filter" and c[1] is not None and changed_of(round(c[1] / 1e-2)))
    # one set_edge_weights per filter that dropped something, each with one more zero, and the entry weights put back at the end
    assert len(sets) == dropping + (1 if dropping else 0)
    for j in range(dropping):
        assert int((sets[j] == 0).sum()) == j + 1
    if dropping:
        assert np.array_equal(sets[-1], np.ones(nobs)) and int((info["weights"] == 0).sum()) == dropping
    assert info["keep"].shape == (nobs,) and info["stopped_early"] == early
    with pytest.raises(xmamd.XmError, match="fix_rotations"):
        ctx.refine_filtered(np.zeros((3, 6)), np.zeros((3, 2)), np.zeros((3, 3)), fix_rotations=True)
    ctx._w = None
    with pytest.raises(xmamd.XmError, match="weights"):
        ctx.refine_filtered(np.zeros((3, 6)), np.zeros((3, 2)), np.zeros((3, 3)))
    ctx.h = None   # nothing to destroy
