"""What tests/test_ba_radial_numpy.py (CPU) and tests/test_gpu_ba_radial_stages.py (GPU) share: the cases of one linearisation of the
bundle adjustment with a focal scale and a radial coefficient per camera, on the scenes of xm_ba_stages.py; the quantities from the
longdouble reference (xm_ba_radial_exact.py) and from the f64 restatement (xm_ba_radial_numpy.py) under the keys of xm_ba_stages; the
error function, the blocks and the bound are xm_ba_stages's: e <= max(16 e_ref, 64 eps_f64), with e_ref <= MAX_E_REF required of every case.

The focal stage cases: focal scales from U[0.8, 1.25] with every third camera's held (xm_ba_focal_stages.focal_point), coefficients from
U[-0.15, 0.15] (both signs) with every fourth camera's held, from camera 1 on.  Three more:
  k_zero    the base scene with every k = 0 and every coefficient held: the focal model at the same point
  mask_mix  the base scene, camera i with (focal, distortion) free as (1, 0), (0, 1), (0, 0), (1, 1) for i mod 4 = 0, 1, 2, 3
  on_axis   the base ring scene at a near point with camera 2 at (8, 0, 0) looking along -x (a signed permutation for its rotation) and
            seeing only four new landmarks on its axis (integer coordinates, also seen by three other cameras each): u = 0 in any
            arithmetic, so its focal and its distortion column are zero by the formula
Under Huber, SoftL1 and Cauchy the candidate at mu = 1e-2 moves the outliers' landmarks so far that the radial map folds for some
observation (exact_stages' "positive" is False: the device reports cost1 = NaN); those cases are probed at mu = 1e4 too, where the
candidate is an ordinary one and cost1 is compared."""
import numpy as np
import scipy.sparse as sp

import xm_ba_focal_stages as fs
import xm_ba_numpy as ba
import xm_ba_radial_exact as rx
import xm_ba_radial_numpy as br
import xm_ba_stages as st

LD = st.LD
CASES = fs.CASES + ("k_zero", "mask_mix", "on_axis")
ALL_KEYS = ("cost", "gmax", "b", "g_l", "vinv", "ustar", "sinv", "S", "SX", "MX_jacobi", "dP", "rot1", "t1", "p1", "focal1", "dist1", "cost1",
            "model", "step2", "x2")
ON_AXIS_CAM = 2


def radial_point(n, seed):
    """(focal, free, dist, kfree)"""
    focal, free = fs.focal_point(n, seed)
    kfree = np.ones(n, dtype=bool)
    kfree[1::4] = False
    dist = np.random.default_rng(seed + 1000).uniform(-0.15, 0.15, n)
    assert (dist < 0).any() and (dist > 0).any()
    return focal, free, dist, kfree


def _huber_edge(S, point, focal, dist, a):
    """xm_ba_focal_stages._huber_edge with the radial factor in the residual: observations 0 and 1 (p_2 = 1) get s == a * a and
    s == nextafter(a * a, inf) in f64 with the expression g s u_0 - q_0 / q_2"""
    Rcw, tcw = ba.to_world_to_camera(*point[:2])
    out = []
    for e, target in ((0, a * a), (1, np.nextafter(a * a, np.inf))):
        i, l = S["cam"][e], S["lm"][e]
        X = Rcw[i] @ point[2][:, l] + tcw[i]
        u0, u1 = X[0] / X[2], X[1] / X[2]
        gs = focal[i] * (1.0 + dist[i] * (u0 * u0 + u1 * u1))
        gu0, gu1 = gs * u0, gs * u1
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


def on_axis_scene():
    """the ring scene of base_scene at a near point, camera ON_AXIS_CAM replaced: centre (8, 0, 0), Rcw = [[0, -1, 0], [0, 0, 1], [-1, 0, 0]]
    (it looks along -x), its observations dropped but for those of four new landmarks at (1, 0, 0), (0, 0, 0), (-1, 0, 0), (2, 0, 0):
    X = (0, 0, 8 - x), so X_0 = X_1 = 0 in any arithmetic.  Its measurements lie off the axis, so its residuals and pose gradient are
    not zero.  Cameras 5, 9 and 13 see the new landmarks too, where the scene's own cameras project them"""
    S0 = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=0.05)
    n, m = S0["n"], S0["m"]
    rot, t, P = ba.perturb(S0["rot"], S0["t"], S0["P"], seed=21, deg=3.0, rel=0.02)
    S = st._with(S0, np.nonzero(np.asarray(S0["cam"]) != ON_AXIS_CAM)[0])
    Rc = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    rot[:, 3 * ON_AXIS_CAM:3 * ON_AXIS_CAM + 3] = Rc.T
    t[:, ON_AXIS_CAM] = (8.0, 0.0, 0.0)
    new = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    P = np.concatenate([P, new.T], axis=1)
    Rcw, tcw = ba.to_world_to_camera(S0["rot"], S0["t"])
    cams, lms, ps = [], [], []
    for j in range(4):
        cams.append(ON_AXIS_CAM); lms.append(m + j)
        ps.append(((0.03, -0.02, 1.0), (-0.01, 0.04, 1.0), (0.02, 0.02, 1.0), (-0.03, -0.01, 1.0))[j])
        for i in (5, 9, 13):
            X = Rcw[i] @ new[j] + tcw[i]
            assert X[2] > 1.0
            cams.append(i); lms.append(m + j); ps.append((X[0] / X[2] + 0.01 * (j - 1.5), X[1] / X[2] - 0.01, 1.0))
    S["cam"] = np.concatenate([S["cam"], cams]).astype(np.int32)
    S["lm"] = np.concatenate([S["lm"], lms]).astype(np.int32)
    S["p"] = np.concatenate([S["p"], np.array(ps)])
    S["w"] = np.ones(len(S["cam"]))
    S["m"] = m + 4
    return S, (rot, t, P)


def case(name, fix):
    """dict: S, point, focal, free, dist, kfree, mus, loss, a, X, dc, keys, extra, fix"""
    cd = 5 if fix else 8
    loss, a, extra, mus, keys = "trivial", 0.0, {}, (1e-4,), ALL_KEYS
    if name in ("base", "k_zero", "mask_mix"):
        S, point = st.base_scene()
        mus = (1e-4, 1.0, 1e6) if name == "base" else (1.0,)
    elif name == "on_axis":
        S, point = on_axis_scene()
        mus = (1.0,)
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
        mus = (1e-2, 1e4)
        keys = ("cost", "b", "g_l", "cost1", "model")
    else:
        raise ValueError(name)
    n = S["n"]
    focal, free, dist, kfree = radial_point(n, 7 + len(name))
    if name == "k_zero":
        dist, kfree = np.zeros(n), np.zeros(n, dtype=bool)
    if name == "mask_mix":
        i4 = np.arange(n) % 4
        free, kfree = (i4 == 0) | (i4 == 3), (i4 == 1) | (i4 == 3)
    if name.startswith("loss_"):
        # the scene's residuals are built at g = 1, k = 0; seen through the model they keep their sizes relative to a (times g s)
        S = br.distort_observations(S, focal, dist)
        extra["edge"] = _huber_edge(S, point, focal, dist, a) if loss == "huber" else []
    rng = np.random.default_rng(3)
    used = np.bincount(np.asarray(S["cam"])[ba.used_mask(S["p"], S["w"])], minlength=n) > 0
    X = rng.standard_normal((cd * n, 4))
    X[np.repeat(~used, cd)] = 0.0
    dc = 1e-2 * rng.standard_normal(cd * n)
    return dict(S=S, point=point, focal=focal, free=free, dist=dist, kfree=kfree, mus=mus, loss=loss, a=a, X=X, dc=dc, keys=keys, extra=extra,
                fix=fix)


def stage_args(c, mu):
    rot, t, P = c["point"]
    return dict(rot=rot, t=t, P=P, focal=c["focal"], free=c["free"], dist=c["dist"], kfree=c["kfree"], mu=mu, fix=c["fix"], loss=c["loss"],
                a=c["a"], X=c["X"], dc=c["dc"])


def exact_stages(S, rot, t, P, focal, free, dist, kfree, mu, fix=False, loss="trivial", a=0.0, X=None, dc=None):
    E = rx.RadialExact(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], rot, t, P, focal, dist, mu, fix, loss, a, free, kfree)
    cd = E.cd
    out = dict(cost=E.cost, gmax=E.gmax, b=E.b, g_l=E.g_l, vinv=E.vinv6(), ustar=E.Ustar, sinv=E.Sinv, S=st.lower_blocks(E.S, cd), _E=E,
               cused=E.cused, lused=E.lused, n_used=E.n_used)
    if X is not None:
        X = np.asarray(X, dtype=LD)
        out["SX"] = E.S @ X
        out["MX_jacobi"] = E.jacobi_inverse() @ X
    if dc is not None:
        c = E.candidate(dc)
        out.update(dP=c["dP"], rot1=c["rot1"], t1=c["t1"], p1=c["P1"].T, focal1=c["focal1"], dist1=c["dist1"], cost1=c["cost1"],
                   model=c["model"], step2=np.array(c["step2"]), x2=np.array(c["x2"], dtype=LD), positive=c["positive"], fold_min=c["fold_min"])
    return out


def f64_stages(S, rot, t, P, focal, free, dist, kfree, mu, fix=False, loss="trivial", a=0.0, X=None, dc=None, perm=None, damage=()):
    """the same quantities from the f64 restatement, the observations in the order perm; damage: RadialProblem's deliberate faults"""
    n, m = S["n"], S["m"]
    cam, lm, p, w = (np.asarray(S[k]) for k in ("cam", "lm", "p", "w"))
    if perm is not None:
        cam, lm, p, w = cam[perm], lm[perm], p[perm], w[perm]
    pr = br.RadialProblem(cam, lm, p, w, n, m, fix, loss, a, free, kfree, damage)
    cd = pr.cd
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    Pw = np.asarray(P, dtype=np.float64).T.copy()
    gf, kf = np.asarray(focal, dtype=np.float64), np.asarray(dist, dtype=np.float64)
    F, r, J = pr.corrected(Rcw, tcw, Pw, gf, kf)
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
        Rn, tn, Pn, gn, kn = pr.plus(Rcw, tcw, Pw, gf, kf, d)
        rot1, t1 = ba.to_camera_to_world(Rn, tn)
        out.update(dP=dP.reshape(m, 3), rot1=rot1, t1=t1, p1=Pn.T, focal1=gn, dist1=kn, cost1=pr.cost(Rn, tn, Pn, gn, kn),
                   model=float(r @ Jd) + 0.5 * float(Jd @ Jd), step2=pr.step2(d), x2=pr.x2(tcw, Pw, gf, kf))
    return out


def reference_errors(S, exact, keys, seed=0, **kw):
    """e_ref per key: the larger of the f64 restatement's errors in the given and in a permuted observation order"""
    n, m, cd = S["n"], S["m"], exact["_E"].cd
    perm = np.random.default_rng(seed).permutation(len(S["cam"]))
    runs = [f64_stages(S, perm=None, **kw), f64_stages(S, perm=perm, **kw)]
    return {k: max(st.err(st.shape_blocks(k, r[k], n, m, cd), st.shape_blocks(k, exact[k], n, m, cd))[0] for r in runs) for k in keys}
