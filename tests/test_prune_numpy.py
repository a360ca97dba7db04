"""CPU tests of the contract of xm_prune_weakly_connected: the vectorised statement tests/xm_prune_numpy.py:run_numpy against the line-cited
restatement of the reference's C++ (run_sequential) on every scene, again after permuting the observations and renumbering the landmarks, and
both against the numbers recorded for SIMPLE2.  Exact everywhere.

The tile scenes are compared here around a tile of 32 bins: the restatement walks every pair of the landmark that all cameras see in a Python
loop (8.4 M pairs at 2 x 2048 + 1 cameras).  The GPU tests run them at the library's tile, against run_numpy."""
import os

import numpy as np
import pytest

import xm_prune_numpy as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_TILE = 32


def _both(S, **kw):
    a, b = pr.run_sequential(S, **kw), pr.run_numpy(S, **kw)
    assert pr.same(a, b) == [], (pr.same(a, b), {k: (a[k], b[k]) for k in pr.COUNTERS if a[k] != b[k]})
    T, perm = pr.permuted(S, seed=3)
    c, d = pr.run_sequential(T, **kw), pr.run_numpy(T, **kw)
    assert pr.same(a, c) == [] and pr.same(a, d) == []       # per camera: nothing depends on the order of the list or the landmark numbers
    return a


@pytest.mark.parametrize("name", [k for k, _ in pr.HAND_MADE])
def test_hand_made_scenes(name):
    S = dict(pr.HAND_MADE)[name]()
    r = _both(S)
    if name != "empty":
        assert (r["median"], r["mad"], r["threshold"]) == ((8.0, 0.0, 20.0) if name != "big_weights" else (6300.0, 2100.0, 4200.0))
    want = dict(
        bridge1=dict(n_clusters=2, rounds=1, weak_edges=1, strong_clusters=2, images_clustered=13),
        bridge2=dict(n_clusters=1, rounds=2, weak_edges=2, strong_clusters=2, images_clustered=13),
        bridge3=dict(n_clusters=1, rounds=2, weak_edges=3, strong_clusters=2, images_clustered=13),
        ladder3=dict(n_clusters=1, rounds=4, images_clustered=5),
        ladder11=dict(n_clusters=1, rounds=10, images_clustered=12),
        edge_values=dict(pairs_covisible=40, n_edges=40, rounds=2, weak_edges=4),
        big_weights=dict(n_clusters=1, images_clustered=7),
        ties=dict(n_clusters=2, component_images=6, images_clustered=6),
        small=dict(pairs_covisible=21, n_edges=19, n_clusters=1, images_clustered=5),
        empty=dict(pairs_covisible=0, n_edges=0, n_clusters=0, threshold=0.0, rounds=0))[name]
    assert {k: r[k] for k in want} == want
    cid = r["cluster_id"].tolist()
    if name == "bridge1":
        assert cid == [0] * 8 + [1] * 5
    if name == "ladder11":
        assert cid[:12] == [0] * 12 and cid[12] == -1        # the cap: ten bodies admit ten images, the eleventh stays out
    if name == "edge_values":
        assert cid[0:4] == [-1] * 4 and cid[16] == cid[17] == cid[19] == 0 and cid[18] == -1
        assert 4 not in r["pairs_count"] and 5 in r["pairs_count"] and r["pairs_count"].max() == 5000
    if name == "ties":
        assert cid == [0, 0, 0, 1, 1, 1] + [-1] * 6          # both ties go to the smallest image
    if name == "small":
        assert cid == [0] * 5 + [-1] * 6 and r["obs_count"][7] == 20
        assert _both(S, min_num_images=2)["cluster_id"].tolist() == [0] * 5 + [1, 1] + [-1] * 4
        assert _both(S, min_num_observations=0)["cluster_id"].tolist() == [0] * 5 + [-1, -1, 0] + [-1] * 3
    if name == "empty":
        assert cid == [-1] * 6


@pytest.mark.parametrize("n", [SMALL_TILE - 1, SMALL_TILE, SMALL_TILE + 1, 2 * SMALL_TILE + 1])
def test_tile_scenes(n):
    r = _both(pr.tile(n, SMALL_TILE))
    assert r["component_images"] == n and r["n_edges"] >= n and r["n_clusters"] > 1


def test_glue_changes_nothing():
    for name in ("bridge2", "ties", "small"):
        S = dict(pr.HAND_MADE)[name]()
        assert pr.same(pr.run_numpy(S), pr.run_numpy(pr.glued(S))) == []


def test_recorded_case():
    S = pr.simple2(GOLDEN)
    L = np.bincount(S["lm"])
    assert (L.size, L.min(), L.max(), int((L * (L - 1) // 2).sum())) == (6033, 6, 57, 435836) and S["n"] == 93
    from scipy.sparse import coo_matrix
    A = coo_matrix((np.ones(S["cam"].size, dtype=np.int64), (S["lm"], S["cam"]))).tocsr()
    C = (A.T @ A).tocoo()
    assert int((C.row < C.col).sum()) == 4234                # covisible pairs at any count
    for run in (pr.run_sequential, pr.run_numpy):
        r = run(S)
        assert {k: r[k] for k in pr.COUNTERS} == dict(pairs_covisible=4105, n_edges=4105, median=65.0, mad=42.0, threshold=23.0, component_images=93,
                                                      strong_clusters=1, rounds=1, weak_edges=0, n_clusters=1, images_clustered=93)
        assert (r["cluster_id"] == 0).all() and r["obs_count"].sum() == S["cam"].size
        # the recorded case also prunes
        r = run(S, min_num_observations=200)
        assert {k: r[k] for k in pr.COUNTERS} == dict(pairs_covisible=4105, n_edges=3497, median=80.0, mad=49.0, threshold=31.0, component_images=85,
                                                      strong_clusters=1, rounds=1, weak_edges=0, n_clusters=1, images_clustered=85)
        assert int((r["cluster_id"] == 0).sum()) == 85 and int((r["cluster_id"] == -1).sum()) == 8
        assert (r["obs_count"][r["cluster_id"] == -1] < 200).all() and (r["obs_count"][r["cluster_id"] == 0] >= 200).all()
    _both(S)
    thin = pr.simple2(GOLDEN, thin=5)
    r = _both(thin)
    assert (r["cluster_id"][-5:] == -1).all() and (r["cluster_id"][:-5] == 0).all() and r["obs_count"][-5:].tolist() == [4] * 5
