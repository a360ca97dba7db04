"""The contract of xm_prune_weakly_connected (include/xm_amd.h) twice, and the scenes its tests run on.

run_sequential  a restatement of the reference's C++ with dicts and a union-find, its lines cited:
                  P   deps/glomap/glomap/processors/reconstruction_pruning.cc:6-84        PruneWeaklyConnectedImages
                  M   deps/glomap/glomap/processors/view_graph_manipulation.cc:68-168     EstablishStrongClusters
                  V   deps/glomap/glomap/scene/view_graph.cc:9-90                         KeepLargestConnectedComponents, MarkConnectedComponents
                with the three departures of the contract: of several largest components the one with the smallest image stays (V:17-22 takes
                the first in hash order), final components of equal size are numbered by smallest image first (V:72-77 sorts (size, index
                into a hash-ordered vector)), and an empty visibility graph gives no cluster (P:62 reads pair_count[0] of an empty vector).
run_numpy       the same contract vectorised: a sparse A^T A for the covisibility, sorts for the order statistics, scipy's connected
                components for the three labellings and for the cluster graph of a merge round.
Both return the same dict; same(a, b) lists the keys in which two of them differ.  Nothing here has a tolerance: every value is an integer or
a double that holds one.

A scene is dict(cam, lm, w, n, m, opt): the observation list (int32, int32, float64), the sizes and the options it is meant to run with.
Covisibility weights are made exactly: a track that names camera i a times and camera j b times adds a b to covis(i, j) and nothing else
(the reference skips image_id1 == image_id2, P:21), and a track [c, c, c] adds 3 to obs_count[c] and no pair at all."""
import numpy as np

DEFAULTS = dict(min_covisibility=5, min_num_images=2, min_num_observations=0, min_threshold=20.0)
COUNTERS = ("pairs_covisible", "n_edges", "median", "mad", "threshold", "component_images", "strong_clusters", "rounds", "weak_edges", "n_clusters",
            "images_clustered")
ARRAYS = ("cluster_id", "obs_count", "pairs_i", "pairs_j", "pairs_count")


def same(a, b):
    """the keys in which two results differ"""
    bad = [k for k in COUNTERS if a[k] != b[k]]
    return bad + [k for k in ARRAYS if not np.array_equal(a[k], b[k])]


def _options(S, kw):
    o = dict(DEFAULTS); o.update(S.get("opt", {})); o.update(kw)
    return o


def _empty(n, obs_count, pairs_covisible):
    z = np.zeros(0, dtype=np.int32)
    return dict(cluster_id=np.full(n, -1, dtype=np.int32), obs_count=obs_count, pairs_i=z, pairs_j=z, pairs_count=z, pairs_covisible=pairs_covisible,
                n_edges=0, median=0.0, mad=0.0, threshold=0.0, component_images=0, strong_clusters=0, rounds=0, weak_edges=0, n_clusters=0,
                images_clustered=0)


# ------------------------------------------------------------------------------------------------ the C++, line by line
class _UnionFind:
    """glomap/math/union_find.h: Find makes an unknown element its own root"""

    def __init__(self):
        self.parent = {}

    def find(self, x):
        self.parent.setdefault(x, x)
        while self.parent[x] != x:
            self.parent[x] = self.parent[self.parent[x]]
            x = self.parent[x]
        return x

    def union(self, x, y):
        rx, ry = self.find(x), self.find(y)
        if rx != ry:
            self.parent[max(rx, ry)] = min(rx, ry)     # (which root stays cannot change a cluster, only its name)


def _components(pairs, valid):
    """V:48-64, V:92-122: the components of the valid pairs, each a set of images"""
    adj = {}
    for k, ok in valid.items():
        if ok:
            i, j = pairs[k]
            adj.setdefault(i, set()).add(j); adj.setdefault(j, set()).add(i)
    seen, comps = set(), []
    for root in sorted(adj):
        if root in seen:
            continue
        comp, queue = {root}, [root]
        seen.add(root)
        while queue:
            cur = queue.pop(0)
            for nb in adj[cur]:
                if nb not in seen:
                    seen.add(nb); comp.add(nb); queue.append(nb)
        comps.append(comp)
    return comps


def run_sequential(S, **kw):
    o = _options(S, kw)
    n = int(S["n"])
    tracks = {}
    for c, l, w in zip(S["cam"].tolist(), S["lm"].tolist(), S["w"].tolist()):
        if w > 0:                                            # a USED observation (the rule of xm_clean_observations)
            tracks.setdefault(l, []).append(c)
    pair_count, image_count = {}, {}
    for track in tracks.values():                            # P:13
        if len(track) <= 2:                                  # P:14
            continue
        for a in range(len(track)):                          # P:16
            image_count[track[a]] = image_count.get(track[a], 0) + 1     # P:17
            for b in range(a + 1, len(track)):               # P:18
                i1, i2 = track[a], track[b]
                if i1 == i2:                                 # P:21
                    continue
                key = (min(i1, i2), max(i1, i2))             # P:22-23
                pair_count[key] = pair_count.get(key, 0) + 1  # P:24-29
    obs_count = np.array([image_count.get(i, 0) for i in range(n)], dtype=np.int32)
    counter, pairs, weight = 0, {}, {}
    for key in sorted(pair_count):                           # P:38 (sorted: the order of the output, not of the reference)
        count = pair_count[key]
        if count >= o["min_covisibility"]:                   # P:41
            counter += 1                                     # P:42
            if image_count.get(key[0], 0) < o["min_num_observations"] or image_count.get(key[1], 0) < o["min_num_observations"]:   # P:46-48
                continue
            pairs[key] = key; weight[key] = count            # P:50-55
    if not pairs:                                            # departure: P:62 would read pair_count[0]
        return _empty(n, obs_count, counter)
    keys = list(pairs)
    pc = sorted(weight.values())                             # P:61
    median = float(pc[len(pc) // 2])                         # P:62
    diff = sorted(abs(v - median) for v in pc)               # P:65-69
    mad = float(diff[len(diff) // 2])                        # P:70
    thr = max(median - mad, o["min_threshold"])              # P:80
    valid = {k: True for k in keys}                          # P:54
    # M:74, V:9-46
    comps = _components(pairs, valid)
    best = max(comps, key=lambda c: (len(c), -min(c)))       # V:17-22; departure: a tie goes to the smallest image
    for k in keys:                                           # V:36-40
        if pairs[k][0] not in best or pairs[k][1] not in best:
            valid[k] = False
    uf = _UnionFind()                                        # M:77
    for k in keys:                                           # M:79-90
        if valid[k] and weight[k] > thr:                     # M:85
            uf.union(*pairs[k])
    strong_clusters = len({uf.find(i) for i in best})
    status, iteration, weak_edges = True, 0, 0               # M:95-96
    thr75 = 0.75 * thr
    while status:                                            # M:97
        status = False
        iteration += 1
        if iteration > 10:                                   # M:101
            break
        num_pairs, looked = {}, 0
        for k in keys:                                       # M:107
            if not valid[k] or weight[k] < thr75:            # M:108, M:115
                continue
            r1, r2 = uf.find(pairs[k][0]), uf.find(pairs[k][1])          # M:121-122
            if r1 == r2:                                     # M:124
                continue
            looked += 1
            num_pairs[(min(r1, r2), max(r1, r2))] = num_pairs.get((min(r1, r2), max(r1, r2)), 0) + 1     # M:134-135
        if iteration == 1:
            weak_edges = looked
        for (r1, r2), count in num_pairs.items():            # M:139-147
            if count >= 2:
                status = True
                uf.union(r1, r2)
    rounds = min(iteration, 10)                              # bodies run
    for k in keys:                                           # M:151-160
        if valid[k] and uf.find(pairs[k][0]) != uf.find(pairs[k][1]):
            valid[k] = False
    comps = _components(pairs, valid)                        # V:66-70
    comps.sort(key=lambda c: (-len(c), min(c)))              # V:72-77; departure: equal sizes by smallest image
    cluster_id = np.full(n, -1, dtype=np.int32)              # V:80
    n_clusters = images = 0
    for comp_id, comp in enumerate(comps):                   # V:82-87
        if len(comp) < o["min_num_images"]:
            break
        for i in comp:
            cluster_id[i] = comp_id
        n_clusters += 1; images += len(comp)
    return dict(cluster_id=cluster_id, obs_count=obs_count, pairs_i=np.array([k[0] for k in keys], dtype=np.int32),
                pairs_j=np.array([k[1] for k in keys], dtype=np.int32), pairs_count=np.array([weight[k] for k in keys], dtype=np.int32),
                pairs_covisible=counter, n_edges=len(keys), median=median, mad=mad, threshold=thr, component_images=len(best),
                strong_clusters=strong_clusters, rounds=rounds, weak_edges=weak_edges, n_clusters=n_clusters, images_clustered=images)


# ------------------------------------------------------------------------------------------------ the contract, vectorised
def _labels(n, i, j):
    """components of the edges (i, j) over n vertices: every vertex carries the smallest vertex of its component"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = coo_matrix((np.ones(i.size, dtype=np.int8), (i, j)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    low = np.full(lab.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(low, lab, np.arange(n))
    return low[lab]


def run_numpy(S, **kw):
    from scipy.sparse import coo_matrix
    o = _options(S, kw)
    n, m = int(S["n"]), int(S["m"])
    cam, lm = S["cam"].astype(np.int64), S["lm"].astype(np.int64)
    used = S["w"] > 0
    L = np.bincount(lm[used], minlength=m)
    act = used & (L[lm] > 2)
    obs_count = np.bincount(cam[act], minlength=n).astype(np.int32)
    A = coo_matrix((np.ones(int(act.sum()), dtype=np.int64), (lm[act], cam[act])), shape=(m, n)).tocsr()      # a_l(i): duplicates add up
    C = (A.T @ A).tocoo()
    up = C.row < C.col
    ci, cj, cc = C.row[up], C.col[up], C.data[up]
    pair = cc >= o["min_covisibility"]
    pairs_covisible = int(pair.sum())
    edge = pair & (obs_count[ci] >= o["min_num_observations"]) & (obs_count[cj] >= o["min_num_observations"])
    order = np.lexsort((cj[edge], ci[edge]))
    ei, ej, ew = ci[edge][order], cj[edge][order], cc[edge][order]
    E = ei.size
    if E == 0:
        return _empty(n, obs_count, pairs_covisible)
    median = int(np.sort(ew)[E // 2])
    mad = int(np.sort(np.abs(ew - median))[E // 2])
    thr = max(float(median - mad), float(o["min_threshold"]))
    thr75 = 0.75 * thr
    # the largest component; a tie goes to the smallest image
    has = np.zeros(n, dtype=bool); has[ei] = True; has[ej] = True
    comp = _labels(n, ei, ej)
    size = np.bincount(comp[has], minlength=n)
    best = int(np.flatnonzero(size == size.max())[0])
    component_images = int(size.max())
    valid = comp[ei] == best
    # strong clusters, then the merge rounds on the cluster labels
    strong = valid & (ew.astype(np.float64) > thr)
    lab = _labels(n, ei[strong], ej[strong])
    strong_clusters = int(np.unique(lab[comp == best]).size)
    weak = valid & ~(ew.astype(np.float64) < thr75)
    wi, wj = ei[weak], ej[weak]
    rounds = weak_edges = 0
    while rounds < 10:
        rounds += 1
        a, b = lab[wi], lab[wj]
        d = a != b
        if rounds == 1:
            weak_edges = int(d.sum())
        key, count = np.unique(np.minimum(a[d], b[d]) * n + np.maximum(a[d], b[d]), return_counts=True)
        join = key[count >= 2]
        if join.size == 0:
            break
        lab = _labels(n, join // n, join % n)[lab]           # all unions of the round at once: the components of the cluster graph
    # final marking
    fin = valid & (lab[ei] == lab[ej])
    has = np.zeros(n, dtype=bool); has[ei[fin]] = True; has[ej[fin]] = True
    comp = _labels(n, ei[fin], ej[fin])
    size = np.bincount(comp[has], minlength=n)
    roots = np.flatnonzero(size > 0)
    roots = roots[np.argsort(-size[roots], kind="stable")]   # by size, descending; equal sizes by smallest image (the root) first
    ids = np.full(n, -1, dtype=np.int32)
    ok = size[roots] >= o["min_num_images"]
    nc = int(ok.size if ok.all() else np.argmin(ok))
    ids[roots[:nc]] = np.arange(nc, dtype=np.int32)
    cluster_id = np.where(has, ids[comp], -1).astype(np.int32)
    return dict(cluster_id=cluster_id, obs_count=obs_count, pairs_i=ei.astype(np.int32), pairs_j=ej.astype(np.int32), pairs_count=ew.astype(np.int32),
                pairs_covisible=pairs_covisible, n_edges=int(E), median=float(median), mad=float(mad), threshold=thr,
                component_images=component_images, strong_clusters=strong_clusters, rounds=rounds,
                weak_edges=weak_edges, n_clusters=nc, images_clustered=int(size[roots[:nc]].sum()))


# ------------------------------------------------------------------------------------------------ scenes
class _Builder:
    def __init__(self, n):
        self.n, self.cam, self.lm, self.w, self.m = n, [], [], [], 0

    def track(self, cams, w=None):
        cams = list(cams)
        self.cam += cams; self.lm += [self.m] * len(cams); self.w += list(w) if w is not None else [1.0] * len(cams)
        self.m += 1

    def edge(self, i, j, weight, w=1.0):
        """covis(i, j) += weight exactly, from tracks {i, i, j} (+2) and {i, i, i, j} (+3): obs_count[i] += weight, obs_count[j] += tracks"""
        assert weight >= 2 and i != j
        if weight % 2:
            self.track([i, i, i, j], [w] * 4); weight -= 3
        for _ in range(weight // 2):
            self.track([i, i, j], [w] * 3)

    def product(self, i, a, j, b):
        """covis(i, j) += a b from one track that names i a times and j b times"""
        assert a + b >= 3 and i != j
        self.track([i] * a + [j] * b)

    def pad(self, c, k=1):
        """obs_count[c] += 3 k and no pair"""
        for _ in range(k):
            self.track([c, c, c])

    def ring(self, cams, weight):
        for a in range(len(cams)):
            self.edge(cams[a], cams[(a + 1) % len(cams)], weight)

    def rest(self, cams, weight, skip=()):
        """every pair of cams that is neither a ring neighbour nor in skip"""
        k = len(cams)
        for a in range(k):
            for b in range(a + 1, k):
                if b - a in (1, k - 1) or (cams[a], cams[b]) in skip:
                    continue
                self.edge(cams[a], cams[b], weight)

    def clique(self, cams, weight):
        for a in range(len(cams)):
            for b in range(a + 1, len(cams)):
                self.edge(cams[a], cams[b], weight)

    def scene(self, **opt):
        return dict(cam=np.array(self.cam, dtype=np.int32), lm=np.array(self.lm, dtype=np.int32), w=np.array(self.w, dtype=np.float64), n=self.n,
                    m=self.m, opt=opt)


# In the hand-made scenes more than half of the edges have weight 8, so median = 8, mad = 0 and threshold = max(8, 20) = 20 with
# 0.75 threshold = 15: a weight of 40 is strong, one in [15, 20] only counts in the merge rounds, 8 and 14 do neither.
def bridge(k):
    """two strong groups of 8 and 5 images joined by k edges inside [0.75 thr, thr]: k = 1 stays two clusters, k = 2 merges in one round"""
    B = _Builder(13)
    ga, gb = list(range(8)), list(range(8, 13))
    B.ring(ga, 40); B.rest(ga, 8); B.ring(gb, 40); B.rest(gb, 8)
    for t, weight in zip(range(k), (15, 20, 18)):            # 15 = 0.75 thr counts (not <), 20 = thr counts and is not strong (strict >)
        B.edge(ga[t], gb[t], weight)
    return B.scene()


def ladder(r):
    """a strong pair, then r images with one edge of weight 18 to each of the two images before them: every round admits exactly one more"""
    n_l = r + 2
    B = _Builder(n_l + 8)
    B.edge(0, 1, 40)
    for t in range(2, n_l):
        B.edge(t - 1, t, 18); B.edge(t - 2, t, 18)
    filler = list(range(n_l, n_l + 8))                       # 29 edges of weight 8 inside the same component: they set the median
    B.clique(filler, 8); B.edge(filler[0], 0, 8)
    return B.scene()


def edge_values():
    """weights exactly at 4 / 5, at thr, at 0.75 thr and one below, and one far above 2^12 (the second level of the order statistics)"""
    B = _Builder(28)
    B.edge(0, 1, 4)                                          # below min_covisibility: no pair
    B.edge(2, 3, 5)                                          # a pair and an edge, outside the largest component
    core = list(range(10, 16))
    B.ring(core, 40); B.rest(core, 8)
    B.edge(10, 16, 20); B.edge(11, 16, 20)                   # == thr: not strong, but two edges that count: 16 merges
    B.edge(10, 17, 15); B.edge(11, 17, 15)                   # == 0.75 thr: counts (not <): 17 merges
    B.edge(10, 18, 14); B.edge(11, 18, 14)                   # below: 18 stays out
    B.edge(10, 19, 21)                                       # strong
    filler = list(range(20, 26))
    B.clique(filler, 8); B.edge(filler[0], 10, 8)
    for _ in range(10):
        B.edge(filler[1], filler[2], 2)                      # more tracks on an existing pair: 8 + 20 = 28, strong
    B.product(26, 50, 20, 100)                               # 5000
    return B.scene()


def big_weights():
    """every weight above 2^12, so the median and the MAD lie in a bucket of their own; threshold = median - mad > 20"""
    B = _Builder(7)
    for a, b in enumerate((59, 70, 90, 100, 120, 128)):
        B.product(a, 70, (a + 1) % 6, b)
    B.product(6, 64, 0, 65); B.product(6, 64, 3, 70)
    return B.scene()


def ties():
    """two components of 6 images with the same edges (step 5: images 0..5 stay), and inside each two clusters of 3 (final: {0,1,2} is 0)"""
    B = _Builder(12)
    for base in (6, 0):                                      # (the component that must lose comes first in the list)
        g = [base + t for t in range(6)]
        B.ring(g[3:], 40); B.ring(g[:3], 40)
        B.edge(g[2], g[3], 18)
        for a in range(3):
            for b in range(3, 6):
                if (a, b) != (2, 3):
                    B.edge(g[a], g[b], 8)
    return B.scene()


def small():
    """a cluster below min_num_images, a camera below min_num_observations, landmarks of length 2, zero weights"""
    B = _Builder(11)
    core = list(range(5))
    B.ring(core, 40); B.rest(core, 8)
    B.edge(5, 6, 40); B.edge(5, 0, 18)                       # a cluster of two behind one counting edge: 2 < min_num_images = 3
    B.edge(0, 7, 21); B.edge(1, 7, 21)                       # camera 7: strong edges, but only 20 observations
    for _ in range(10):
        B.track([8, 9])                                      # length 2: ignored (P:14), however often
    B.edge(8, 0, 40, w=0.0)                                  # not used at all
    B.track([0, 1, 2, 3], [1.0, 1.0, 1.0, 0.0])              # three used: counts for 0, 1, 2 only
    B.track([1, 2, 4], [1.0, 0.0, 1.0])                      # two used: skipped
    B.edge(9, 10, 8); B.edge(9, 0, 8); B.edge(10, 0, 8); B.edge(10, 1, 8); B.edge(9, 1, 8); B.edge(9, 2, 8); B.edge(10, 2, 8)
    for c in range(11):
        if c != 7:
            B.pad(c, 10)
    return B.scene(min_num_images=3, min_num_observations=21)


def empty():
    """no pair reaches 5"""
    B = _Builder(6)
    B.edge(0, 1, 4); B.edge(1, 2, 4); B.edge(3, 4, 3); B.track([0, 2, 4]); B.track([5, 5, 5])
    return B.scene()


def tile(n, T):
    """n cameras around a tile of T bins: a ring and edges that cross the tile boundary, one landmark that every camera sees, a camera with a
    list of more than 256 entries"""
    B = _Builder(n)
    shapes = ((2, 2), (2, 3), (3, 3), (4, 5), (5, 6), (6, 7))   # + 1 from the long landmark: 5, 7, 10, 21, 31, 43
    def link(i, j, k):
        a, b = shapes[k % len(shapes)]
        B.product(min(i, j), a, max(i, j), b)
    for i in range(n):
        link(i, (i + 1) % n, i + (3 if i % 7 else 4))
        if i + T < n and i % 3 == 0:
            link(i, i + T, i)
        if i % 5 == 0 and i + T - 1 < n:
            link(i, i + T - 1, i + 4)
    for i, j in ((T - 2, T), (T - 1, T + 1), (0, n - 1), (1, T), (0, T - 1), (T, 2 * T - 1), (T - 1, 2 * T), (0, 2 * T)):
        if 0 <= i < j < n and j - i not in (1, T, T - 1, n - 1):
            link(i, j, i + j)
    B.pad(0, 100)
    B.track(range(n))
    B.pad(n - 1, 2)
    return B.scene()


HAND_MADE = (("bridge1", lambda: bridge(1)), ("bridge2", lambda: bridge(2)), ("bridge3", lambda: bridge(3)), ("ladder3", lambda: ladder(3)),
             ("ladder11", lambda: ladder(11)), ("edge_values", edge_values), ("big_weights", big_weights), ("ties", ties), ("small", small),
             ("empty", empty))


def glued(S):
    """S with a track of length 2 between every two neighbouring cameras: the contract ignores them (P:14), and they make the list one
    component, which creating a context needs"""
    n = S["n"]
    cam = np.concatenate([S["cam"], np.repeat(np.arange(n - 1), 2) + np.tile([0, 1], n - 1)]).astype(np.int32)
    lm = np.concatenate([S["lm"], S["m"] + np.repeat(np.arange(n - 1), 2)]).astype(np.int32)
    return dict(S, cam=cam, lm=lm, w=np.concatenate([S["w"], np.ones(2 * (n - 1))]), m=S["m"] + n - 1)


def permuted(S, seed=0):
    """S with its observations in another order and its landmarks renumbered; -> (scene, perm) with scene.cam = S.cam[perm]"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(S["cam"].size)
    renum = rng.permutation(S["m"]).astype(np.int32)
    return dict(S, cam=S["cam"][perm], lm=renum[S["lm"][perm]], w=S["w"][perm]), perm


def simple2(golden, thin=0):
    """the recorded case at unit weights; thin > 0: the last `thin` cameras keep only their first 4 observations (the others get weight 0)"""
    import os
    o = np.load(os.path.join(golden, "simple2", "obs.npz"))
    cam, lm = o["cam"].astype(np.int32), o["lm"].astype(np.int32)
    w = np.ones(cam.size)
    n = int(cam.max()) + 1
    for c in range(n - thin, n):
        w[np.flatnonzero(cam == c)[4:]] = 0.0
    return dict(cam=cam, lm=lm, p=o["p"], w=w, n=n, m=int(lm.max()) + 1, opt={})
