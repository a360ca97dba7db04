"""What tests/test_ba_focal_numpy.py (CPU) and tests/test_gpu_ba_focal_stages.py (GPU) share: the cases of one linearisation of the bundle
adjustment with focal scales, on the scenes of xm_ba_stages.py; the quantities from the longdouble reference (xm_ba_focal_exact.py) and
from the f64 restatement (xm_ba_focal_numpy.py) under the keys of xm_ba_stages; the error function, the blocks and the bound are
xm_ba_stages's: e <= max(16 e_ref, 64 eps_f64), with e_ref <= MAX_E_REF required of every case.

Every case: focal scales drawn from U[0.8, 1.25] at the probed point, every third camera's focal held."""
import numpy as np
import scipy.sparse as sp

import xm_ba_focal_exact as fx
import xm_ba_focal_numpy as bf
import xm_ba_numpy as ba
import xm_ba_stages as st

LD = st.LD
CASES = ("base", "degrees", "masks", "clamp") + tuple("loss_" + k for k in st.rl.LOSSES[1:])
ALL_KEYS = ("cost", "gmax", "b", "g_l", "vinv", "ustar", "sinv", "S", "SX", "MX_jacobi", "dP", "rot1", "t1", "p1", "focal1", "cost1", "model",
            "step2", "x2")


def focal_point(n, seed):
    """(focal, free): U[0.8, 1.25], cameras 0, 3, 6, ... held"""
    free = np.ones(n, dtype=bool)
    free[::3] = False
    return np.random.default_rng(seed).uniform(0.8, 1.25, n), free


def _huber_edge(S, point, focal, a):
    """xm_ba_stages._huber_edge with the focal scale in the residual: observations 0 and 1 (p_2 = 1) get s == a * a and
    s == nextafter(a * a, inf) in f64 with the eval kernel's expression g u_0 - q_0 / q_2"""
    Rcw, tcw = ba.to_world_to_camera(*point[:2])
    out = []
    for e, target in ((0, a * a), (1, np.nextafter(a * a, np.inf))):
        i, l = S["cam"][e], S["lm"][e]
        X = Rcw[i] @ point[2][:, l] + tcw[i]
        gu0, gu1 = focal[i] * (X[0] / X[2]), focal[i] * (X[1] / X[2])
        S["p"][e, 1] = gu1                                 # r_1 = 0 exactly
        q = gu0 - np.sqrt(target)
        for _ in range(200):
            s = (gu0 - q) * (gu0 - q)
            if s == target:
                break
            q = np.nextafter(q, np.inf if s > target else -np.inf)
        S["p"][e, 0] = q
        out.append((e, float((gu0 - q) * (gu0 - q))))
    return out


def case(name, fix):
    """dict: S, point, focal, free, mus, loss, a, X, dc, keys, extra, fix"""
    cd = 4 if fix else 7
    loss, a, extra, mus, keys = "trivial", 0.0, {}, (1e-4,), ALL_KEYS
    if name == "base":
        S, point = st.base_scene()
        mus = (1e-4, 1.0, 1e6)
    elif name == "degrees":
        S, point, extra["roles"], extra["degrees"] = st.degree_scene()
        keys = ("vinv", "g_l", "b", "SX", "S", "dP", "MX_jacobi")
    elif name == "masks":
        S, point = st.mask_scene()
        mus = (1e-2,)
    elif name == "clamp":
        S, point = st.clamp_scene()
        mus = (1.0,)
        keys = ("vinv", "S", "b", "ustar", "g_l", "SX", "dP")
    elif name.startswith("loss_"):
        loss = name[5:]
        S, point, a, _ = st.loss_scene(loss)
        mus = (1e-2,)
        keys = ("cost", "b", "g_l", "cost1", "model")
    else:
        raise ValueError(name)
    n = S["n"]
    focal, free = focal_point(n, 7 + len(name))
    if name.startswith("loss_"):
        # the scene's residuals are built at g = 1; seen through the focal scales they keep their sizes relative to a (times g)
        S = bf.scale_observations(S, focal)
        extra["edge"] = _huber_edge(S, point, focal, a) if loss == "huber" else []
    rng = np.random.default_rng(3)
    used = np.bincount(np.asarray(S["cam"])[ba.used_mask(S["p"], S["w"])], minlength=n) > 0
    X = rng.standard_normal((cd * n, 4))
    X[np.repeat(~used, cd)] = 0.0
    dc = 1e-2 * rng.standard_normal(cd * n)
    return dict(S=S, point=point, focal=focal, free=free, mus=mus, loss=loss, a=a, X=X, dc=dc, keys=keys, extra=extra, fix=fix)


def stage_args(c, mu):
    rot, t, P = c["point"]
    return dict(rot=rot, t=t, P=P, focal=c["focal"], free=c["free"], mu=mu, fix=c["fix"], loss=c["loss"], a=c["a"], X=c["X"], dc=c["dc"])


def exact_stages(S, rot, t, P, focal, free, mu, fix=False, loss="trivial", a=0.0, X=None, dc=None):
    E = fx.FocalExact(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], rot, t, P, focal, mu, fix, loss, a, free)
    cd = E.cd
    out = dict(cost=E.cost, gmax=E.gmax, b=E.b, g_l=E.g_l, vinv=E.vinv6(), ustar=E.Ustar, sinv=E.Sinv, S=st.lower_blocks(E.S, cd), _E=E,
               cused=E.cused, lused=E.lused, n_used=E.n_used)
    if X is not None:
        X = np.asarray(X, dtype=LD)
        out["SX"] = E.S @ X
        out["MX_jacobi"] = E.jacobi_inverse() @ X
    if dc is not None:
        c = E.candidate(dc)
        out.update(dP=c["dP"], rot1=c["rot1"], t1=c["t1"], p1=c["P1"].T, focal1=c["focal1"], cost1=c["cost1"], model=c["model"],
                   step2=np.array(c["step2"]), x2=np.array(c["x2"], dtype=LD), positive=c["positive"])
    return out


def f64_stages(S, rot, t, P, focal, free, mu, fix=False, loss="trivial", a=0.0, X=None, dc=None, perm=None, damage=()):
    """the same quantities from the f64 restatement, the observations in the order perm; damage: FocalProblem's deliberate faults"""
    n, m = S["n"], S["m"]
    cam, lm, p, w = (np.asarray(S[k]) for k in ("cam", "lm", "p", "w"))
    if perm is not None:
        cam, lm, p, w = cam[perm], lm[perm], p[perm], w[perm]
    pr = bf.FocalProblem(cam, lm, p, w, n, m, fix, loss, a, free, damage)
    cd = pr.cd
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    Pw = np.asarray(P, dtype=np.float64).T.copy()
    gf = np.asarray(focal, dtype=np.float64)
    F, r, J = pr.corrected(Rcw, tcw, Pw, gf)
    H = (J.T @ J).tocsc()
    g = J.T @ r
    H = (H + sp.diags(mu * np.clip(H.diagonal(), 1e-6, 1e32))).tocsr()
    nc_ = cd * n
    U, W, V = H[:nc_, :nc_], H[:nc_, nc_:], H[nc_:, nc_:].tocoo()
    Vd = np.zeros((m, 3, 3))
    Vd[V.row // 3, V.row % 3, V.col % 3] = V.data
    Vi = np.linalg.inv(Vd)
    Vinv = sp.block_diag(list(Vi), format="csr")
    Ssp = (U - W @ Vinv @ W.T).tocsr()
    b = -g[:nc_] + W @ (Vinv @ g[nc_:])
    Sd, Ud = Ssp.toarray(), U.toarray()
    out = dict(cost=F, gmax=float(np.abs(g).max(initial=0.0)), b=b, g_l=g[nc_:].reshape(m, 3),
               vinv=np.stack([Vi[:, 0, 0], Vi[:, 0, 1], Vi[:, 0, 2], Vi[:, 1, 1], Vi[:, 1, 2], Vi[:, 2, 2]], axis=1),
               ustar=np.stack([Ud[cd * i:cd * i + cd, cd * i:cd * i + cd] for i in range(n)]),
               sinv=np.stack([np.linalg.inv(Sd[cd * i:cd * i + cd, cd * i:cd * i + cd]) for i in range(n)]), S=st.lower_blocks(Sd, cd))
    if X is not None:
        out["SX"] = Ssp @ X
        out["MX_jacobi"] = st.bp.jacobi_inverse(Ssp, cd) @ X
    if dc is not None:
        dc = np.asarray(dc, dtype=np.float64).reshape(-1)
        dP = -(Vinv @ (g[nc_:] + W.T @ dc))
        dP.reshape(m, 3)[~pr.lused] = 0.0
        d = np.concatenate([dc, dP])
        Jd = J @ d
        Rn, tn, Pn, gn = pr.plus(Rcw, tcw, Pw, gf, d)
        rot1, t1 = ba.to_camera_to_world(Rn, tn)
        out.update(dP=dP.reshape(m, 3), rot1=rot1, t1=t1, p1=Pn.T, focal1=gn, cost1=pr.cost(Rn, tn, Pn, gn),
                   model=float(r @ Jd) + 0.5 * float(Jd @ Jd), step2=pr.step2(d), x2=pr.x2(tcw, Pw, gf))
    return out


def reference_errors(S, exact, keys, seed=0, **kw):
    """e_ref per key: the larger of the f64 restatement's errors in the given and in a permuted observation order"""
    n, m, cd = S["n"], S["m"], exact["_E"].cd
    perm = np.random.default_rng(seed).permutation(len(S["cam"]))
    runs = [f64_stages(S, perm=None, **kw), f64_stages(S, perm=perm, **kw)]
    return {k: max(st.err(st.shape_blocks(k, r[k], n, m, cd), st.shape_blocks(k, exact[k], n, m, cd))[0] for r in runs) for k in keys}
