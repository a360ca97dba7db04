"""What tests/test_ba_groups_numpy.py (CPU) and tests/test_gpu_ba_groups_stages.py (GPU) share: the cases of one linearisation of the
bundle adjustment with focal groups (xm_ctx_ba_probe_focal_groups), the quantities from the longdouble reference (xm_ba_groups_exact.py)
and from the f64 restatement (xm_ba_groups_numpy.py) under the same keys, and the comparison.  The error function and the bound are
xm_ba_stages's: e <= max(16 e_ref, 64 eps_f64), with e_ref <= MAX_E_REF required of every case.

Vectors of the shared space (b, the columns of SX and MX) are judged in two parts: the cameras' cp entries, one block per camera, and the
G focal entries, one block per group."""
import numpy as np

import xm_ba_groups_exact as gx
import xm_ba_groups_numpy as bg
import xm_ba_numpy as ba
import xm_ba_stages as st

LD = st.LD
SIZES = (1, 2, 63, 64, 65, 257)                            # either side of the thread / workgroup rule of the group sums, and several strides
KEYS = ("cost", "gmax", "b", "D", "F", "g_l", "S", "SX", "MX", "dP", "rot1", "t1", "p1", "focal1", "cost1", "model", "step2", "x2")
CASES = ("base", "one_group", "singletons", "g16", "g17", "unused_member", "unused_group", "clamp_member", "sizes", "loss_huber")


def _axis_member(S, point, k):
    """the scene with camera k left one used observation, and the point with that observation's landmark moved onto k's optical axis (1e-4
    off it at depth 5): the focal column of k is 2e-8 / 25, below the clamp at 1e-6"""
    cam, lm = np.asarray(S["cam"]), np.asarray(S["lm"])
    mine = np.nonzero(cam == k)[0]
    S = dict(S)
    w = np.asarray(S["w"], dtype=np.float64).copy()
    w[mine[1:]] = 0.0
    S["w0"], S["w"] = np.ones(len(w)), w
    rot, t, P = (np.array(v) for v in point)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    P[:, lm[mine[0]]] = Rcw[k].T @ (np.array([5e-4, -5e-4, 5.0]) - tcw[k])
    return S, (rot, t, P)


def case(name, fix):
    """dict: S, point, group_of, G, focal, free, mus, loss, a, X, dc, fix"""
    loss, a, mus = "trivial", 0.0, (1.0,)
    S, point = st.base_scene()
    n = S["n"]
    free = None
    if name == "base":                                     # five groups of four, an empty group, a singleton; one group held
        group_of = np.arange(n) % 5
        group_of[n - 1] = 6
        G, mus = 7, (1e-4, 1.0, 1e6)
        free = np.ones(G, dtype=bool); free[1] = False
    elif name == "one_group":
        group_of, G = np.zeros(n, dtype=int), 1
    elif name == "singletons":
        group_of, G = np.random.default_rng(4).permutation(n), n
    elif name in ("g16", "g17"):
        G = int(name[1:])
        group_of = np.arange(n) % G
    elif name in ("unused_member", "unused_group"):        # camera 5 has no used observation
        S, point = st.mask_scene()
        n = S["n"]
        group_of = np.arange(n) % 4 + 1
        group_of[5] = 1 if name == "unused_member" else 0
        G = 5 + (name == "unused_member")                  # group 0 holds camera 5 alone, or nobody (and then group 5 is a second empty one)
        mus = (1e-2,)
    elif name == "clamp_member":                           # the trap: a member whose own clamp is active
        S, point = _axis_member(S, point, 7)
        group_of, G = np.arange(n) % 3, 3
    elif name == "sizes":
        S = ba.sequential_scene(n_cams=sum(SIZES), per_cam=3, seed=9, noise=1e-3)
        point = ba.perturb(S["rot"], S["t"], S["P"], seed=10, deg=1.0, rel=0.002)
        n = S["n"]
        group_of = np.random.default_rng(11).permutation(np.repeat(np.arange(len(SIZES)), SIZES))
        G = len(SIZES)
    elif name == "loss_huber":
        S, point, a, _ = st.loss_scene("huber")
        n, loss, mus = S["n"], "huber", (1e-2,)
        group_of, G = np.arange(n) % 3, 3
    else:
        raise ValueError(name)
    cp = 3 if fix else 6
    rng = np.random.default_rng(3)
    focal = rng.uniform(0.8, 1.25, G)
    if name == "loss_huber":
        S = bg.bf.scale_observations(S, focal[group_of])
    used = np.bincount(np.asarray(S["cam"])[ba.used_mask(S["p"], S["w"])], minlength=n) > 0
    X = rng.standard_normal((cp * n + G, 4))
    X[:cp * n][np.repeat(~used, cp)] = 0.0
    X[cp * n:][np.bincount(group_of, minlength=G) == 0] = 0.0      # an empty group has no slot on the device
    dc = 1e-2 * rng.standard_normal(cp * n + G)
    return dict(S=S, point=point, group_of=np.asarray(group_of, dtype=np.int32), G=G, focal=focal, free=free, mus=mus, loss=loss, a=a, X=X, dc=dc,
                fix=fix, name=name)


def stage_args(c, mu):
    rot, t, P = c["point"]
    return dict(rot=rot, t=t, P=P, group_of=c["group_of"], focal=c["focal"], free=c["free"], mu=mu, fix=c["fix"], loss=c["loss"], a=c["a"],
                X=c["X"], dc=c["dc"])


def exact_stages(S, rot, t, P, group_of, focal, free, mu, fix=False, loss="trivial", a=0.0, X=None, dc=None):
    E = gx.GroupsExact(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], rot, t, P, group_of, focal, mu, fix, loss, a, free)
    out = dict(cost=E.cost, gmax=E.gmax, b=E.b, D=E.D, F=E.F, S=np.tril(E.S), g_l=E.E7.g_l, _E=E, cused=E.E7.cused, lused=E.E7.lused, n_used=E.E7.n_used,
               moving=E.moving)
    if X is not None:
        X = np.asarray(X, dtype=LD)
        out["SX"] = E.S @ X
        out["MX"] = E.minv(X)
    if dc is not None:
        c = E.candidate(dc)
        out.update(dP=c["dP"], rot1=c["rot1"], t1=c["t1"], p1=c["P1"].T, focal1=c["focal1"], cost1=c["cost1"], model=c["model"],
                   step2=np.array(c["step2"]), x2=np.array(c["x2"], dtype=LD), positive=c["positive"])
    return out


def f64_stages(S, perm=None, **kw):
    kw = dict(kw)
    return bg.stages(S, kw.pop("rot"), kw.pop("t"), kw.pop("P"), kw.pop("group_of"), kw.pop("focal"), kw.pop("free"), kw.pop("mu"), perm=perm, **kw)


def parts(key, v, n, m, cp, G):
    """[(name, blocks x entries)] of a quantity"""
    v = np.asarray(v)
    if key in ("b", "SX", "MX", "S"):
        v = v.reshape(cp * n + G, -1)
        return [(key + ".pose", v[:cp * n].reshape(n, -1)), (key + ".focal", v[cp * n:].reshape(G, -1))]
    if key in ("D", "F", "focal1"):
        return [(key, v.reshape(G, -1))]
    return [(key, st.shape_blocks(key, v, n, m, cp))]


def errors(S, got, exact, keys, G):
    n, m, cp = S["n"], S["m"], exact["_E"].cp
    out = {}
    for k in keys:
        for (name, x), (_, xe) in zip(parts(k, got[k], n, m, cp, G), parts(k, exact[k], n, m, cp, G)):
            out[name] = st.err(x, xe)
    return out


def reference_errors(S, exact, keys, G, seed=0, **kw):
    """e_ref per (part of a) key: the larger of the f64 restatement's errors in the given and in a permuted observation order"""
    perm = np.random.default_rng(seed).permutation(len(S["cam"]))
    runs = [errors(S, f64_stages(S, perm=p, **kw), exact, keys, G) for p in (None, perm)]
    return {k: max(r[k][0] for r in runs) for k in runs[0]}


def compare(label, S, got, exact, e_ref, keys, G, who="gpu"):
    """prints one line per quantity (the table of profiles/r38_ba_groups_stage_errors.txt) and returns those that miss the bound"""
    bad = []
    for k, (e, blk) in errors(S, got, exact, keys, G).items():
        ratio = e / e_ref[k] if e_ref[k] > 0 else (0.0 if e == 0 else float("inf"))
        print(f"STAGE_ERR {label} {k}: e_ref {e_ref[k]:.3e} e_{who} {e:.3e} ratio {ratio:.3g} bound {st.bound(e_ref[k]):.3e} worst block {blk}")
        if not e <= st.bound(e_ref[k]):
            bad.append((k, e, e_ref[k], blk))
    return bad
