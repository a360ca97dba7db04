"""Track establishment restated twice, and the case builders of its tests.

(a) fork_tracks: a sequential, line-cited restatement of the reference's fork of GLOMAP -- deps/glomap/glomap/math/union_find.h:15-53
    (the union-find that refuses to merge two sets sharing an image) and deps/glomap/glomap/controllers/track_establishment.cc:19-63
    (BlindConcatenation), :65-151 (TrackCollection) and :153-227 (FindTracksForProblem with min_num_tracks_per_view = -1), with the pairs
    in a caller-given order (the reference walks an unordered_map).  It is written from a reading of those lines; the reference's C++
    was never built or run (it needs COLMAP, Eigen and glog), so nothing here is a record of its binary.
(b) run_numpy: the contract of xm_build_tracks (include/xm_amd.h, rules 1-8) in numpy / scipy (connected_components), all three conflict
    policies.  This is what the GPU tests compare with, exactly.

What ties the two: in a component of the match graph in which no image occurs twice no Union is ever refused, so (a) in any pair order,
upstream GLOMAP and plain connected components give the same track for it (tests/test_tracks_numpy.py asserts it).  Components that hold
two features of one image ("conflicted") have no order-independent statement in the reference; (b) gives them an explicit policy."""
import hashlib
import os

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tracks")
POLICIES = ("drop", "glomap", "split")
UNTOUCHED, SHORT, LONG, CONFLICT, FEW_REGISTERED, BEYOND_MAX = -1, -2, -3, -4, -5, -6
INFO_FIELDS = ("ntracks", "features_touched", "matches", "components", "components_conflicted", "rows_conflicted", "tracks_short", "tracks_long",
               "tracks_conflict", "tracks_few_registered", "tracks_beyond_max", "images_small", "images_large", "images_workspace", "max_touched",
               "edges_split", "unions_refused")
DEFAULTS = dict(min_views=3, max_views=1000000, max_tracks=10000000, thres_inconsistency=10.0)


# ------------------------------------------------------------------------------------------------ cases
def make_case(counts, pairs, xy=None, registered=None, **options):
    """counts: features per image; pairs: [(i, j, [(a, b), ...]), ...] with a, b the feature indices in image i, j"""
    counts = np.asarray(counts, dtype=np.int64)
    foff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    F = int(foff[-1])
    if xy is None:
        xy = np.stack([np.arange(F) * 3.0 + 0.25, np.arange(F) * 7.0 % 480 + 0.5], axis=1)
    per = [np.asarray(m, dtype=np.int32).reshape(-1, 2) for _, _, m in pairs]
    moff = np.concatenate([[0], np.cumsum([m.shape[0] for m in per])]).astype(np.int64)
    cat = np.concatenate(per, axis=0) if per else np.zeros((0, 2), dtype=np.int32)
    return dict(foff=foff, xy=np.ascontiguousarray(xy, dtype=np.float64), pi=np.array([p[0] for p in pairs], dtype=np.int32),
                pj=np.array([p[1] for p in pairs], dtype=np.int32), moff=moff, f1=np.ascontiguousarray(cat[:, 0]), f2=np.ascontiguousarray(cat[:, 1]),
                registered=None if registered is None else np.asarray(registered, dtype=np.uint8), options=dict(options))


def call_args(c):
    """-> positional and keyword arguments of xmamd.build_tracks (without the policy)"""
    return (c["foff"], c["xy"], c["pi"], c["pj"], (c["moff"], c["f1"], c["f2"])), dict(registered=c["registered"], **c["options"])


def permuted(c, seed):
    """the same matches with the pairs in another order, half of them turned round, and the matches of every pair shuffled"""
    rng = np.random.default_rng(seed)
    np_ = c["pi"].size
    order = rng.permutation(np_)
    flip = rng.random(np_) < 0.5
    pi, pj, f1, f2, cnt = [], [], [], [], []
    for k in order:
        a, b = int(c["moff"][k]), int(c["moff"][k + 1])
        q = rng.permutation(b - a) + a
        x, y = c["f1"][q], c["f2"][q]
        if flip[k]:
            pi.append(c["pj"][k]); pj.append(c["pi"][k]); f1.append(y); f2.append(x)
        else:
            pi.append(c["pi"][k]); pj.append(c["pj"][k]); f1.append(x); f2.append(y)
        cnt.append(b - a)
    d = dict(c)
    d["pi"] = np.array(pi, dtype=np.int32); d["pj"] = np.array(pj, dtype=np.int32)
    d["moff"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    d["f1"] = np.concatenate(f1).astype(np.int32) if f1 else np.zeros(0, np.int32)
    d["f2"] = np.concatenate(f2).astype(np.int32) if f2 else np.zeros(0, np.int32)
    return d


SIMPLE2 = dict(seed=1, p_match=0.6, wrong=0.001)
FORK_ORDERS = (None, 11, 12)      # the pair orders restatement (a) is run in: as listed, and two random ones by their seed


def pair_order(c, seed):
    return None if seed is None else np.random.default_rng(seed).permutation(c["pi"].size)


def simple2_case():
    """matches derived from the SIMPLE2 observation list (tests/golden/simple2/obs.npz): the features are its observations ordered by
    (camera, landmark); every co-visible feature pair of a landmark is a match with probability 0.6; 0.1 % wrong matches are added, each
    joining random features of a random listed pair; pixel positions uniform over 1024 x 768; every 13th image is unregistered"""
    d = np.load(os.path.join(ROOT, "tests", "golden", "simple2", "obs.npz"))
    order = np.lexsort((d["lm"], d["cam"]))
    cam, lm = d["cam"][order].astype(np.int64), d["lm"][order].astype(np.int64)
    n, F = int(cam.max()) + 1, cam.size
    counts = np.bincount(cam, minlength=n)
    foff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rng = np.random.default_rng(SIMPLE2["seed"])
    xy = np.stack([rng.uniform(0, 1024, F), rng.uniform(0, 768, F)], axis=1)
    by_lm = np.argsort(lm, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(lm))])
    us, vs = [], []
    for l in range(start.size - 1):
        g = by_lm[start[l]:start[l + 1]]
        if g.size < 2:
            continue
        a, b = np.triu_indices(g.size, 1)
        us.append(g[a]); vs.append(g[b])
    u, v = np.concatenate(us), np.concatenate(vs)
    on = rng.random(u.size) < SIMPLE2["p_match"]
    u, v = u[on], v[on]                                        # cam[u] < cam[v]: the features are in camera order
    key = cam[u] * n + cam[v]
    o = np.argsort(key, kind="stable")
    u, v, key = u[o], v[o], key[o]
    pairs, first = np.unique(key, return_index=True)
    pi, pj = (pairs // n).astype(np.int32), (pairs % n).astype(np.int32)
    cnt = np.diff(np.concatenate([first, [key.size]]))
    nwrong = int(round(SIMPLE2["wrong"] * u.size))
    wk = rng.integers(0, pairs.size, nwrong)
    wu = foff[pi[wk]] + (rng.random(nwrong) * counts[pi[wk]]).astype(np.int64)
    wv = foff[pj[wk]] + (rng.random(nwrong) * counts[pj[wk]]).astype(np.int64)
    u, v, key = np.concatenate([u, wu]), np.concatenate([v, wv]), np.concatenate([key, pairs[wk]])
    o = np.argsort(key, kind="stable")
    u, v = u[o], v[o]
    cnt = cnt + np.bincount(wk, minlength=pairs.size)
    moff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    k_of = np.repeat(np.arange(pairs.size), cnt)
    f1 = (u - foff[pi[k_of]]).astype(np.int32); f2 = (v - foff[pj[k_of]]).astype(np.int32)
    registered = (np.arange(n) % 13 != 5).astype(np.uint8)
    return dict(foff=foff, xy=xy, pi=pi, pj=pj, moff=moff, f1=f1, f2=f2, registered=registered, options={}, nwrong=nwrong)


def digest(c):
    h = hashlib.sha256()
    for k in ("foff", "xy", "pi", "pj", "moff", "f1", "f2", "registered"):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    return h.hexdigest()


def chain_case(n, perm=None):
    """n images with one feature each, matched as a chain; perm: the chain runs through perm[0], perm[1], ..."""
    at = np.arange(n) if perm is None else np.asarray(perm)
    return make_case([1] * n, [(int(at[k]), int(at[k + 1]), [(0, 0)]) for k in range(n - 1)], max_views=2 * n)


def sizes_case(limits):
    """four images with limits[3], limits[3] + 1, limits[0] and limits[0] + 1 touched features (every one the end of a track through two
    partner images of 128 features), each with a conflict of its own (its features 0 and 1 match the same partner feature) and with a few
    untouched features in between"""
    big = [limits["small_rows"], limits["small_rows"] + 1, limits["lds_rows"], limits["lds_rows"] + 1]
    counts, pairs = [], []
    for T in big:
        x = len(counts)
        counts.append(T + 3)
        feats = np.concatenate([np.arange(0, 5), np.arange(8, T + 3)])[:T]     # (5, 6, 7 untouched)
        for s in range(0, T, 128):
            f = feats[s:s + 128]
            p1, p2 = len(counts), len(counts) + 1
            counts += [128, 128]
            loc = np.arange(f.size)
            pairs.append((x, p1, np.stack([f, loc], axis=1)))
            pairs.append((p2, p1, np.stack([loc, loc], axis=1)))
            if s == 0:
                pairs.append((p1, x, [(0, int(feats[1]))]))    # the partner's feature 0 sees the image's features 0 and 1
    return make_case(counts, pairs), big


def gpu_cases(limits):
    """the hand-made cases of tests/test_gpu_tracks.py by name"""
    P = {}
    P["one_image"] = make_case([3], [])
    P["two_images"] = make_case([2, 2], [(0, 1, [(0, 1)])])
    P["triangle"] = make_case([1, 1, 1], [(0, 1, [(0, 0)]), (1, 2, [(0, 0)]), (0, 2, [(0, 0)])])
    # chains of 2, 3, 5 and 6 observations over six images with four features each: min_views - 1, min_views, max_views, max_views + 1
    P["lengths"] = make_case([4] * 6, [(k, k + 1, [(c, c) for c, L in enumerate((2, 3, 5, 6)) if k + 1 < L]) for k in range(5)], max_views=5)
    P["chain"] = chain_case(1500)
    P["chain_permuted"] = chain_case(1500, np.random.default_rng(5).permutation(1500))
    P["sizes"], _ = sizes_case(limits)
    # image 0 has features 0 and 1 in one component: (0.0 - 1.0, 0.1 - 1.0, 1.0 - 2.0); the split keeps {0.0, 1.0, 2.0} and leaves 0.1 alone
    for name, off in (("conflict_near", (6.0, 8.0)), ("conflict_far", (0.0, 10.0 + 2.0 ** -40))):
        xy = np.array([[100.0, 100.0], [100.0 + off[0], 100.0 + off[1]], [50.0, 60.0], [70.0, 80.0], [1.0, 2.0]])
        P[name] = make_case([2, 1, 2], [(0, 1, [(0, 0), (1, 0)]), (1, 2, [(0, 0)])], xy=xy)
    # a chain of three conflicts: images 0, 1, 2 with two features each, all in one component through image 3
    P["conflict_chain"] = make_case([2, 2, 2, 1, 1, 1], [(0, 3, [(0, 0), (1, 0)]), (1, 3, [(0, 0), (1, 0)]), (2, 3, [(0, 0), (1, 0)]), (0, 4, [(1, 0)]),
                                                         (1, 4, [(1, 0)]), (2, 5, [(1, 0)]), (4, 5, [(0, 0)])])
    tri = [(0, 1, [(0, 0)]), (1, 2, [(0, 0)]), (0, 2, [(0, 0)])]
    P["duplicate_match"] = make_case([1, 1, 1], [(0, 1, [(0, 0), (0, 0)]), tri[1], tri[2]])
    P["duplicate_orientation"] = make_case([1, 1, 1], tri + [(1, 0, [(0, 0)])])
    P["duplicate_pair"] = make_case([1, 1, 1], tri + [tri[0]])
    # features 0.1, 1.1 are untouched; 2.1 - 3.0 is a track of two: matched only inside a dropped track
    P["coverage"] = make_case([2, 2, 2, 1], tri + [(2, 3, [(1, 0)])])
    # image 2 is unregistered: track A = {0.0, 1.0, 2.0} has two registered images; track B = {0.1, 1.1, 3.0, 2.1} has three and one more
    P["unregistered"] = make_case([2, 2, 2, 1], [(0, 1, [(0, 0), (1, 1)]), (1, 2, [(0, 0)]), (1, 3, [(1, 0)]), (3, 2, [(0, 1)])], registered=[1, 1, 0, 1])
    # five tracks of 5, 4, 3, 3 and 3 observations, max_tracks = 2: three stay, the tie at the cut goes to the larger label
    P["max_tracks"] = make_case([5] * 5, [(k, k + 1, [(c, c) for c, L in enumerate((3, 5, 3, 4, 3)) if k + 1 < L]) for k in range(4)], max_tracks=2)
    # more than 1024 x 1024 features: the prefix sums' top kernel makes a second pass over the tile sums.  Three tracks whose smallest
    # features are the global ids 0, F0 - 3 and F0 + 2; the second and third are numbered and placed with the carry of the first pass
    F0 = 2 ** 20 + 4
    P["scan_second_pass"] = make_case([F0, 4, 4, 4], [(0, 1, [(0, 0), (F0 - 3, 1)]), (1, 2, [(0, 0), (1, 1), (2, 2)]), (2, 3, [(2, 2)]), (0, 2, [(0, 0)])])
    return P


# ------------------------------------------------------------------------------------------------ (b) the contract
def _global_edges(c):
    k_of = np.repeat(np.arange(c["pi"].size), np.diff(c["moff"]))
    u = c["foff"][c["pi"][k_of]] + c["f1"]; v = c["foff"][c["pj"][k_of]] + c["f2"]
    return np.minimum(u, v).astype(np.int64), np.maximum(u, v).astype(np.int64)


def split_numpy(foff, eu, ev):
    """rule 4, XM_TRACKS_SPLIT: -> (dict feature -> label, distinct edges, unions refused)"""
    e = np.unique(np.stack([np.minimum(eu, ev), np.maximum(eu, ev)], axis=1).astype(np.int64), axis=0) if len(eu) else np.zeros((0, 2), np.int64)
    img = lambda g: int(np.searchsorted(foff, g, side="right") - 1)
    parent, images, refused = {}, {}, 0

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for g in np.unique(e):
        parent[int(g)] = int(g); images[int(g)] = {img(g)}
    for u, v in e.tolist():                                    # np.unique(axis=0) sorts the rows: (smaller id, larger id) ascending
        ru, rv = find(u), find(v)
        if ru == rv:
            continue
        if images[ru] & images[rv]:
            refused += 1
            continue
        a, b = min(ru, rv), max(ru, rv)
        parent[b] = a
        images[a] |= images.pop(b)
    return {g: find(g) for g in parent}, int(e.shape[0]), refused


def run_numpy(c, conflict="split", limits=None):
    """the contract of xm_build_tracks -> dict(cam, feat, track, xy, m, label, info)"""
    o = dict(DEFAULTS); o.update(c["options"])
    foff = c["foff"]; n = foff.size - 1; F = int(foff[-1])
    reg = np.ones(n, dtype=bool) if c["registered"] is None else c["registered"].astype(bool)
    fimg = np.repeat(np.arange(n), np.diff(foff))
    info = {k: 0 for k in INFO_FIELDS}
    eu, ev = _global_edges(c) if c["pi"].size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    info["matches"] = int(eu.size)
    label = np.full(F, UNTOUCHED, dtype=np.int32)
    empty = dict(cam=np.zeros(0, np.int32), feat=np.zeros(0, np.int32), track=np.zeros(0, np.int32), xy=np.zeros((0, 2)), m=0, label=label, info=info)
    if n == 0 or eu.size == 0:
        return empty
    touched = np.zeros(F, dtype=bool); touched[eu] = True; touched[ev] = True      # rule 1
    ncomp, comp = connected_components(coo_matrix((np.ones(eu.size), (eu, ev)), shape=(F, F)), directed=False)   # rule 2
    smallest = np.full(ncomp, F, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(F))
    root = smallest[comp]
    t = np.flatnonzero(touched)
    info["features_touched"] = int(t.size); info["components"] = int(np.unique(root[t]).size)
    per_image = np.bincount(fimg[t], minlength=n)
    info["max_touched"] = int(per_image.max())
    if limits is not None:
        info["images_small"] = int(np.sum((per_image > 0) & (per_image <= limits["small_rows"])))
        info["images_large"] = int(np.sum((per_image > limits["small_rows"]) & (per_image <= limits["lds_rows"])))
        info["images_workspace"] = int(np.sum(per_image > limits["lds_rows"]))
    # rule 3: two features of one image under one label
    key = root[t] * n + fimg[t]
    ks, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    dup_roots = np.unique(ks[cnt > 1] // n)
    conflicted = np.zeros(F, dtype=bool); conflicted[dup_roots] = True             # (at the root)
    info["components_conflicted"] = int(dup_roots.size); info["rows_conflicted"] = int(np.sum(conflicted[root[t]]))
    discarded = np.zeros(F, dtype=bool)                                              # (at the root)
    if conflict == "drop":
        discarded = conflicted.copy()
    elif conflict == "glomap":
        thres = o["thres_inconsistency"]
        by_key = np.argsort(inv, kind="stable"); first = np.concatenate([[0], np.cumsum(cnt)])
        for k in np.flatnonzero(cnt > 1):
            g = t[by_key[first[k]:first[k + 1]]]
            x, y = c["xy"][g, 0], c["xy"][g, 1]
            dx = x[:, None] - x[None, :]; dy = y[:, None] - y[None, :]
            if np.any(np.sqrt(dx * dx + dy * dy) > thres):
                discarded[ks[k] // n] = True
    elif conflict == "split":
        on = conflicted[root[eu]]
        if on.any():
            new, info["edges_split"], info["unions_refused"] = split_numpy(foff, eu[on], ev[on])
            g = np.fromiter(new.keys(), dtype=np.int64); root = root.copy(); root[g] = np.fromiter(new.values(), dtype=np.int64)
            conflicted[:] = False
    else:
        raise ValueError(conflict)
    # rule 5
    size = np.bincount(root[t], minlength=F)
    kr = np.unique(root[t][reg[fimg[t]]] * n + fimg[t][reg[fimg[t]]])
    regc = np.bincount(kr // n, minlength=F)
    roots = np.unique(root[t])
    status = np.zeros(F, dtype=np.int32)
    for r in roots:
        if discarded[r]: status[r] = CONFLICT
        elif size[r] < o["min_views"]: status[r] = SHORT
        elif size[r] > o["max_views"]: status[r] = LONG
        elif regc[r] < o["min_views"]: status[r] = FEW_REGISTERED
    kept = roots[status[roots] == 0]
    # rule 6
    if kept.size > o["max_tracks"] + 1:
        order = np.lexsort((kept, size[kept]))                  # ascending (size, label): the last max_tracks + 1 stay
        gone = kept[order[:kept.size - (o["max_tracks"] + 1)]]
        status[gone] = BEYOND_MAX
        kept = np.sort(kept[order[kept.size - (o["max_tracks"] + 1):]])
    for name, code in (("tracks_short", SHORT), ("tracks_long", LONG), ("tracks_conflict", CONFLICT), ("tracks_few_registered", FEW_REGISTERED),
                       ("tracks_beyond_max", BEYOND_MAX)):
        info[name] = int(np.sum(status[roots] == code))
    # rule 8 and the output
    number = np.full(F, -1, dtype=np.int64); number[kept] = np.arange(kept.size)
    info["ntracks"] = int(kept.size)
    st = status[root[t]]
    label[t] = np.where(st < 0, st, number[root[t]]).astype(np.int32)
    rows = t[(st == 0) & reg[fimg[t]]]
    return dict(cam=fimg[rows].astype(np.int32), feat=(rows - foff[fimg[rows]]).astype(np.int32), track=label[rows].copy(), xy=c["xy"][rows].copy(),
                m=int(kept.size), label=label, info=info)


def conflict_free_tracks(c):
    """-> (the conflict-free components as frozensets of global feature indices, the number of components)"""
    foff = c["foff"]; n = foff.size - 1; F = int(foff[-1])
    eu, ev = _global_edges(c)
    fimg = np.repeat(np.arange(n), np.diff(foff))
    ncomp, comp = connected_components(coo_matrix((np.ones(eu.size), (eu, ev)), shape=(F, F)), directed=False)
    touched = np.zeros(F, dtype=bool); touched[eu] = True; touched[ev] = True
    t = np.flatnonzero(touched)
    groups = {}
    for g, k in zip(t.tolist(), comp[t].tolist()):
        groups.setdefault(k, []).append(g)
    free = [frozenset(g) for g in groups.values() if len({int(fimg[x]) for x in g}) == len(g)]
    return free, len(groups)


# ------------------------------------------------------------------------------------------------ (a) the fork, sequentially
def fork_tracks(c, pair_order=None, min_views=3, max_views=1000000, max_tracks=10000000, thres_inconsistency=10.0):
    """the fork with the pairs visited in pair_order -> (what TrackCollection leaves, what FindTracksForProblem selects of it), both
    {track id: [(image, feature), ...]}.  Ids are image << 32 | feature as at track_establishment.cc:47-52."""
    foff = c["foff"]; n = foff.size - 1
    reg = np.ones(n, dtype=bool) if c["registered"] is None else c["registered"].astype(bool)
    order = range(c["pi"].size) if pair_order is None else pair_order
    parent, overlap = {}, {}

    def find(x):                                               # union_find.h:15-32 (the recursion unrolled; the path is compressed)
        if x not in parent:                                    # :18-25: a new point is its own root and overlaps its own image
            parent[x] = x; overlap[x] = {x >> 32}
            return x
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:                                  # :28-31
            parent[x], x = r, parent[x]
        return r

    def union(x, y):                                           # union_find.h:34-53
        rx, ry = find(x), find(y)
        if rx == ry:
            return
        if not (overlap[rx] & overlap[ry]):                    # :43-46: no image in common
            parent[rx] = ry                                    # :49
            overlap[ry] |= overlap[rx]                         # :52
    ids = []
    for k in order:                                            # BlindConcatenation, :23-61
        a, b = int(c["moff"][k]), int(c["moff"][k + 1])
        i1, i2 = int(c["pi"][k]) << 32, int(c["pj"][k]) << 32
        for x, y in zip(c["f1"][a:b].tolist(), c["f2"][a:b].tolist()):
            g1, g2 = i1 | x, i2 | y                            # :47-52
            ids.append((g1, g2))
            if g2 < g1: union(g1, g2)                          # :56-59
            else: union(g2, g1)
    track_map = {}
    for g1, g2 in ids:                                         # TrackCollection, :71-107: both ends go to the track of Find(id1)
        tid = find(g1)
        s = track_map.setdefault(tid, set()); s.add(g1); s.add(g2)
    tracks = {}
    for tid, members in track_map.items():                     # :111-145 (the set is walked in ascending order here; the reference's is a hash order)
        seen, obs = {}, []
        for g in sorted(members):
            im, f = g >> 32, g & 0xFFFFFFFF
            p = c["xy"][foff[im] + f]
            if im in seen:                                     # :123-136
                if any(np.sqrt((q[0] - p[0]) * (q[0] - p[0]) + (q[1] - p[1]) * (q[1] - p[1])) > thres_inconsistency for q in seen[im]):
                    obs = []
                    break
            seen.setdefault(im, []).append(p)
            obs.append((im, f))
        tracks[tid] = obs
    lengths = sorted(((len(o), tid) for tid, o in tracks.items() if min_views <= len(o) <= max_views), reverse=True)   # :159-167
    selected = {}
    for _, tid in lengths:                                     # :182-220 with min_num_tracks_per_view = -1: every track that passes is added
        obs = [(im, f) for im, f in tracks[tid] if reg[im]]    # :189-196
        if len({im for im, _ in obs}) < min_views:             # :198
            continue
        selected[tid] = obs
        if len(selected) > max_tracks:                         # :219
            break
    return tracks, selected


def fork_contains(c, free, pair_order):
    """per conflict-free component of `free`: did TrackCollection produce exactly it in this pair order, and does FindTracksForProblem
    select exactly its observations in registered images when rule 5 keeps it (and nothing of it otherwise)"""
    foff = c["foff"]; n = foff.size - 1
    o = dict(DEFAULTS); o.update(c["options"])
    reg = np.ones(n, dtype=bool) if c["registered"] is None else c["registered"].astype(bool)
    fimg = np.repeat(np.arange(n), np.diff(foff))
    full, sel = fork_tracks(c, pair_order, **o)
    as_set = lambda obs: frozenset(int(foff[im] + f) for im, f in obs)
    got_full = {as_set(obs) for obs in full.values()}
    got_sel = {as_set(obs) for obs in sel.values()}
    whole, chosen = [], []
    for s in free:
        whole.append(s in got_full)
        r = frozenset(g for g in s if reg[fimg[g]])
        keeps = o["min_views"] <= len(s) <= o["max_views"] and len(r) >= o["min_views"]      # (conflict-free: one feature per image)
        chosen.append((r in got_sel) == keeps)
    return np.array(whole, dtype=bool), np.array(chosen, dtype=bool)


def load_case():
    """-> (the SIMPLE2-derived case, regenerated; the record of tests/golden/tracks/simple2.npz with the labels restored)"""
    rec = dict(np.load(os.path.join(GOLDEN, "simple2.npz")))
    for pol in ("drop", "split"):
        rec["label_" + pol] = np.cumsum(rec["label_%s_diff" % pol], dtype=np.int64).astype(np.int32)
    rec["label_glomap"] = rec["label_drop"] + rec["label_glomap_minus_drop"]
    for pol in POLICIES:
        rec["info_" + pol] = dict(zip(INFO_FIELDS, rec["info_" + pol].tolist()))
    return simple2_case(), rec


def rows_of(c, label):
    """the output rows that a label array determines: cam, feat, track, xy"""
    foff = c["foff"]; n = foff.size - 1
    fimg = np.repeat(np.arange(n), np.diff(foff))
    reg = np.ones(n, dtype=bool) if c["registered"] is None else c["registered"].astype(bool)
    rows = np.flatnonzero((label >= 0) & reg[fimg])
    return dict(cam=fimg[rows].astype(np.int32), feat=(rows - foff[fimg[rows]]).astype(np.int32), track=label[rows].astype(np.int32), xy=c["xy"][rows])
