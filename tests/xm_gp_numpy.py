"""numpy / scipy.sparse restatement of the global positioning behind xm_ctx_global_positioning (include/xm_amd.h, xm_gp.h): GLOMAP's
estimators/global_positioning.cc in its default ONLY_POINTS form, with the full sparse Jacobian over (camera centres, points, scales), the
loss, the Levenberg-Marquardt rules of xm_ctx_bundle_adjust with EXACT sparse solves, and the active-set rule for the bound on the scales.
NOT COMPARED WITH THE REFERENCE'S COMPILED CODE (it needs Ceres, COLMAP, Eigen and glog): the citations say which line a rule comes from.

Layouts are the library's (xm_ba_numpy.py): rot 3 x 3n (R_i, camera to world, read only), t 3 x n (camera centres), P 3 x m; observations
(cam, lm, p, w), of which only the bearing p / |p| is read.

  used         weight > 0, p_2 > 0 (the bundle adjustment's rule) and the landmark has >= min_views such observations
               (global_positioning.h:33, .cc:119, :231)
  direction    d_e = R_i p_e / |p_e|                                     (.cc:265-267; features_undist: image_undistorter.cc:34-35)
  residual     r_e = d_e - s_e (P_l - c_i)                               (cost_function.h:26-29), s_e = 1 at the start (.cc:273), s_e >= 1e-5 (.cc:297)
  cost         F = 1/2 sum rho(|r_e|^2), Huber with a = 0.1 by default   (global_positioning.h:44-45)
  gauge        free                                                      (.cc:337-338)
  bound        DEPARTURE from Ceres (projection + line search): a scale at the bound whose gradient points outward (g_s > 0) is frozen for
               the iteration -- its column of J is zero --, and the candidate is s <- max(s + ds, 1e-5)

Every function takes dtype: float64 (the restatement) or longdouble (the judge of tests/test_gpu_gp_stages.py; numpy.linalg does not take
longdouble, the small inverses are xm_ba_exact.gj_inverse)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import xm_ba_exact as ex
import xm_ba_loss_numpy as rl

LD = ex.LD
S_MIN = 1e-5
STATUS = {"no_convergence": 0, "function_tolerance": 1, "gradient_tolerance": 2, "parameter_tolerance": 3, "max_iterations": 4,
          "time_limit": 5, "no_progress": 6}


def random_start(n, m, seed=1):
    """100 U(-1, 1)^3 for every camera and point (.cc:141, :235), cameras first; xmamd.gp_random_start draws the same numbers"""
    rng = np.random.default_rng(seed)
    return 100.0 * rng.uniform(-1.0, 1.0, (3, n)), 100.0 * rng.uniform(-1.0, 1.0, (3, m))


def used_mask(lm, p, w, m, min_views=3):
    ok = (np.asarray(w) > 0) & (np.asarray(p)[:, 2] > 0)
    cnt = np.bincount(np.asarray(lm)[ok], minlength=m)
    return ok & (cnt[np.asarray(lm)] >= min_views)


def _rho(loss, s, a, dtype):
    if dtype is LD:
        return ex.rho(loss, s, a)
    r0, r1, _ = rl.rho(loss, s, a)
    return r0, r1


def _clip(d, dtype):
    return np.clip(d, dtype(1e-6), dtype(1e32))


def _inv3(A, dtype):
    return ex.gj_inverse(A) if dtype is LD else np.linalg.inv(A)


class Problem:
    """the used observations; unknowns x = (c: 3 per camera, P: 3 per landmark, s: 1 per used observation, in input order)"""

    def __init__(self, cam, lm, p, w, rot, n, m, min_views=3, loss="huber", a=0.1, dtype=np.float64):
        self.dtype = dtype
        self.mask = used_mask(lm, p, w, m, min_views)
        self.idx = np.nonzero(self.mask)[0]
        self.cam, self.lm = np.asarray(cam)[self.idx].astype(np.int64), np.asarray(lm)[self.idx].astype(np.int64)
        q = np.asarray(p, dtype=dtype)[self.idx]
        u = q / np.sqrt(np.sum(q * q, axis=1))[:, None]
        R = np.stack([np.asarray(rot, dtype=dtype)[:, 3 * i:3 * i + 3] for i in range(n)])
        self.d = np.einsum("kab,kb->ka", R[self.cam], u)
        self.n, self.m, self.k = n, m, self.idx.size
        self.nobs = np.asarray(cam).size
        self.cused = np.bincount(self.cam, minlength=n) > 0
        self.lused = np.bincount(self.lm, minlength=m) > 0
        self.loss, self.a = loss, a

    def residuals(self, c, P, s):
        return self.d - s[:, None] * (P[self.lm] - c[self.cam])

    def cost(self, c, P, s):
        r = self.residuals(c, P, s)
        return 0.5 * float(np.sum(_rho(self.loss, np.sum(r * r, axis=1), self.a, self.dtype)[0]))

    def blocks(self, c, P, s):
        """the corrected residual and Jacobian blocks of every used observation: dict of F, r (k x 3), w = rho', v = P_l - c_i, frozen,
        gs = J_s^T r, Jc = sqrt(w) s I, JP = -sqrt(w) s I (as the scalar on the diagonal), Js = -sqrt(w) v (0 where frozen)"""
        v = P[self.lm] - c[self.cam]
        r = self.d - s[:, None] * v
        r0, w = _rho(self.loss, np.sum(r * r, axis=1), self.a, self.dtype)
        sw = np.sqrt(w)
        gs = -w * np.sum(r * v, axis=1)
        frozen = (s <= self.dtype(S_MIN)) & (gs > 0)
        Js = np.where(frozen[:, None], self.dtype(0), -sw[:, None] * v)
        return dict(F=0.5 * float(np.sum(r0)), r=sw[:, None] * r, w=w, v=v, frozen=frozen, gs=np.where(frozen, self.dtype(0), gs), jc=sw * s, Js=Js)

    def jacobian(self, B):
        """sparse 3k x (3n + 3m + k) from blocks()"""
        k, n, m = self.k, self.n, self.m
        rows = np.arange(3 * k)
        ax = np.tile(np.arange(3), k)
        e = np.repeat(np.arange(k), 3)
        jc = np.repeat(np.asarray(B["jc"], dtype=np.float64), 3)
        J = sp.csr_matrix((np.concatenate([jc, -jc, np.asarray(B["Js"], dtype=np.float64).reshape(-1)]),
                           (np.concatenate([rows, rows, rows]),
                            np.concatenate([3 * self.cam[e] + ax, 3 * n + 3 * self.lm[e] + ax, 3 * n + 3 * m + e]))), shape=(3 * k, 3 * n + 3 * m + k))
        return J

    def split(self, d):
        n, m = self.n, self.m
        return d[:3 * n].reshape(n, 3), d[3 * n:3 * n + 3 * m].reshape(m, 3), d[3 * n + 3 * m:]

    def plus(self, c, P, s, d):
        dc, dP, ds = self.split(d)
        return c + dc, P + dP, np.maximum(s + ds, self.dtype(S_MIN))

    def x_norm(self, c, P, s):
        return float(np.sqrt(np.sum(c[self.cused] ** 2) + np.sum(P[self.lused] ** 2) + np.sum(s ** 2)))


def solve_damped(A, b):
    """exact solve of the damped normal equations (symmetric positive definite) by a sparse LU without pivoting in Ceres's elimination
    order (.cc:310-331): the unknowns are (c, P, s), so reversed the scales go first, then the points, the cameras last.  The fill is the
    3 x 3 point blocks and the dense camera block; a fill-reducing ordering of the whole matrix did not finish at 83 000 unknowns"""
    perm = np.arange(A.shape[0])[::-1]
    lu = spla.splu(A[perm][:, perm].tocsc(), permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    x = np.empty(A.shape[0])
    x[perm] = lu.solve(b[perm])
    return x


def lm(cam, lm_, p, w, rot, t, P, min_views=3, loss="huber", a=0.1, max_iters=100, function_tol=1e-5, gradient_tol=1e-10, parameter_tol=1e-8):
    """the LM of xm_ctx_global_positioning with exact solves of the damped normal equations over (c, P, s).  Returns (t, P, info) with
    info: status, iters, accepted, n_used, initial_cost, final_cost, gradient_max, scales (nobs, -1 = unused), trace (cost, candidate
    cost, mu, accepted per iteration)"""
    n, m = t.shape[1], P.shape[1]
    pr = Problem(cam, lm_, p, w, rot, n, m, min_views, loss, a)
    c, X, s = t.T.copy(), P.T.copy(), np.ones(pr.k)                                   # .cc:273
    radius, nu = 1e4, 2.0
    B = pr.blocks(c, X, s)
    J, r, F = pr.jacobian(B), B["r"].reshape(-1), B["F"]
    g = J.T @ r
    info = dict(initial_cost=F, n_used=pr.k)
    trace = []
    iters = accepted = 0
    status = "no_convergence"
    while True:
        if np.max(np.abs(g), initial=0.0) <= gradient_tol:
            status = "gradient_tolerance"; break
        if iters >= max_iters:
            status = "max_iterations"; break
        mu = 1.0 / radius
        A = (J.T @ J).tocsc()
        D = np.clip(A.diagonal(), 1e-6, 1e32)
        d = solve_damped(A + sp.diags(mu * D).tocsc(), -g)
        Jd = J @ d
        model_dec = -(float(r @ Jd) + 0.5 * float(Jd @ Jd))
        cn, Xn, sn = pr.plus(c, X, s, d)
        Fn = pr.cost(cn, Xn, sn)
        iters += 1
        step = float(np.sqrt(np.sum(d * d)))
        valid = np.isfinite(Fn) and model_dec > 0
        rho = (F - Fn) / model_dec if valid else -1.0
        acc = bool(valid and rho > 1e-3)
        trace.append((F, Fn, mu, float(acc)))
        if step <= parameter_tol * (pr.x_norm(c, X, s) + parameter_tol):
            status = "parameter_tolerance"; break
        if acc:
            accepted += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            nu = 2.0
            c, X, s = cn, Xn, sn
            Fold, F = F, Fn
            B = pr.blocks(c, X, s)
            J, r = pr.jacobian(B), B["r"].reshape(-1)
            g = J.T @ r
            if abs(Fold - Fn) <= function_tol * Fold:
                status = "function_tolerance"; break
        else:
            radius /= nu
            nu *= 2.0
            if radius < 1e-32:
                status = "no_progress"; break
    t_o, P_o = t.copy(), P.copy()
    t_o[:, pr.cused] = c.T[:, pr.cused]
    P_o[:, pr.lused] = X.T[:, pr.lused]
    scales = np.full(pr.nobs, -1.0)
    scales[pr.idx] = s
    info.update(status=STATUS[status], iters=iters, accepted=accepted, final_cost=F, gradient_max=float(np.max(np.abs(g), initial=0.0)),
                scales=scales, trace=np.array(trace).reshape(-1, 4))
    return t_o, P_o, info


def closed_form(B, s, mu, dtype=np.float64):
    """the formulas of include/xm_amd.h for one used observation: M_e (k x 3 x 3), q_e (k x 3), h* (k)"""
    w, v, r, gs = B["w"], B["v"], B["r"] / np.sqrt(B["w"])[:, None], B["gs"]
    h = np.where(B["frozen"], dtype(0), w * np.sum(v * v, axis=1))
    hs = h + dtype(mu) * _clip(h, dtype)
    u = np.where(B["frozen"][:, None], dtype(0), (w * s)[:, None] * v)
    M = (w * s * s)[:, None, None] * np.eye(3, dtype=dtype) - u[:, :, None] * u[:, None, :] / hs[:, None, None]
    q = (w * s)[:, None] * r + u * (gs / hs)[:, None]
    return M, q, hs


def stages(pr, t, P, s_all, mu, X=None, dc=None):
    """one linearisation at (t, P, s_all: nobs scales, read where used) with the damping mu, from the Jacobian blocks by Schur complements
    (scales, then landmarks): what xm_ctx_gp_probe returns, under its keys, in pr.dtype.  Per-observation arrays have nobs rows (0 where
    unused).  S is the dense 3n x 3n reduced camera matrix."""
    dt = pr.dtype
    n, m, k = pr.n, pr.m, pr.k
    c, Xp = np.asarray(t, dtype=dt).T.copy(), np.asarray(P, dtype=dt).T.copy()
    s = np.asarray(s_all, dtype=dt)[pr.idx]
    B = pr.blocks(c, Xp, s)
    mu = dt(mu)
    I3 = np.eye(3, dtype=dt)
    jc, Js, r = B["jc"], B["Js"], B["r"]
    # scales: H_ss = |Js|^2 (one per observation), H_cs = jc Js, H_Ps = -jc Js, g_s = Js . r
    h = np.sum(Js * Js, axis=1)
    hs = h + mu * _clip(h, dt)
    gs = np.sum(Js * r, axis=1)
    y = jc[:, None] * Js                                                   # J_c^T J_s
    M = (jc * jc)[:, None, None] * I3 - y[:, :, None] * y[:, None, :] / hs[:, None, None]
    q = jc[:, None] * r - y * (gs / hs)[:, None]
    # damping of c and P: the diagonal of the FULL J^T J
    dcam, dlm = np.zeros(n, dtype=dt), np.zeros(m, dtype=dt)
    np.add.at(dcam, pr.cam, jc * jc)
    np.add.at(dlm, pr.lm, jc * jc)
    U, V = np.zeros((n, 3, 3), dtype=dt), np.zeros((m, 3, 3), dtype=dt)
    gc, gl = np.zeros((n, 3), dtype=dt), np.zeros((m, 3), dtype=dt)
    gfull = np.zeros((n, 3), dtype=dt)
    np.add.at(U, pr.cam, M); np.add.at(V, pr.lm, M)
    np.add.at(gc, pr.cam, q); np.add.at(gl, pr.lm, -q)
    np.add.at(gfull, pr.cam, jc[:, None] * r)
    gPfull = np.zeros((m, 3), dtype=dt)
    np.add.at(gPfull, pr.lm, -jc[:, None] * r)
    Us = U + (mu * _clip(dcam, dt))[:, None, None] * I3
    Vs = V + (mu * _clip(dlm, dt))[:, None, None] * I3
    Vi = _inv3(Vs, dt)
    # W (camera i, landmark l) = -sum of M_e over the observations of the pair
    W = np.zeros((n, m, 3, 3), dtype=dt)
    np.add.at(W, (pr.cam, pr.lm), -M)
    WV = np.einsum("ilab,lbc->ilac", W, Vi)
    S = np.zeros((3 * n, 3 * n), dtype=dt)
    Sb = -np.einsum("ilab,jlcb->iajc", WV, W)
    for i in range(n):
        Sb[i, :, i, :] += Us[i]
    S = Sb.reshape(3 * n, 3 * n)
    b = -gc + np.einsum("ilab,lb->ia", WV, gl)
    sinv = _inv3(np.stack([S[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(n)]), dt)
    out = dict(cost=B["F"], n_used=k, gmax=float(max(np.abs(gfull).max(initial=0), np.abs(gPfull).max(initial=0), np.abs(gs).max(initial=0))),
               vinv=Vi[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], g_l=gl, ustar=Us, sinv=sinv, b=b, S=S, cused=pr.cused, lused=pr.lused)
    full = lambda a: _scatter(pr, a)
    out.update(M=full(M[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]), q=full(q), frozen=full(B["frozen"].astype(np.int32)))
    if X is not None:
        out["SX"] = S @ np.asarray(X, dtype=dt).reshape(3 * n, -1)
    if dc is not None:
        dcv = np.asarray(dc, dtype=dt).reshape(n, 3)
        dP = -np.einsum("lab,lb->la", Vi, gl + np.einsum("ilab,ia->lb", W, dcv))
        dP[~pr.lused] = 0
        dcv = np.where(pr.cused[:, None], dcv, dt(0))
        ds = -(gs + np.sum(y * (dcv[pr.cam] - dP[pr.lm]), axis=1)) / hs
        c1, P1, s1 = c + dcv, Xp + dP, np.maximum(s + ds, dt(S_MIN))
        r1 = pr.residuals(c1, P1, s1)
        Jd = jc[:, None] * (dcv[pr.cam] - dP[pr.lm]) + Js * ds[:, None]
        sc = np.full(pr.nobs, -1, dtype=dt); sc[pr.idx] = s1
        out.update(dP=dP, ds=full(ds), t1=c1.T, p1=P1.T, s1=sc,
                   cost1=0.5 * float(np.sum(_rho(pr.loss, np.sum(r1 * r1, axis=1), pr.a, dt)[0])),
                   model=float(np.sum(r * Jd) + 0.5 * np.sum(Jd * Jd)),
                   step2=np.array([np.sum(dcv * dcv), np.sum(dP * dP), np.sum(ds * ds)], dtype=dt),
                   x2=np.array([np.sum(c[pr.cused] ** 2), np.sum(Xp[pr.lused] ** 2), np.sum(s * s)], dtype=dt))
    out["_B"], out["_s"], out["_hs"] = B, s, hs
    return out


def _scatter(pr, a):
    full = np.zeros((pr.nobs,) + a.shape[1:], dtype=a.dtype)
    full[pr.idx] = a
    return full


def align(A, B):
    """the similarity (scale, rotation, translation) that takes the columns of A (3 x k) closest to those of B, applied to A (Umeyama)"""
    ma, mb = A.mean(axis=1, keepdims=True), B.mean(axis=1, keepdims=True)
    A0, B0 = A - ma, B - mb
    U, sv, Vt = np.linalg.svd(B0 @ A0.T)
    Dg = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ Dg @ Vt
    sc = float(np.sum(sv * np.diag(Dg)) / np.sum(A0 * A0))
    return sc * (R @ A0) + mb


def recovery_error(S, t, P):
    """largest distance of a centre or point from the scene's after the best similarity, relative to the scene's extent"""
    A, Bm = np.concatenate([t, P], axis=1), np.concatenate([S["t"], S["P"]], axis=1)
    ext = float(np.linalg.norm(Bm.max(axis=1) - Bm.min(axis=1)))
    return float(np.sqrt(np.sum((align(A, Bm) - Bm) ** 2, axis=0)).max()) / ext


def bearing_scene(n_cams, n_pts, seed=0, noise=0.0, outliers=0.0, **kw):
    """xm_ba_numpy.ring_scene; with outliers > 0 that fraction of the bearings is replaced by random unit vectors with p_2 > 0"""
    import xm_ba_numpy as ba
    S = ba.ring_scene(n_cams=n_cams, n_pts=n_pts, seed=seed, noise=noise, **kw)
    if outliers > 0:
        rng = np.random.default_rng(seed + 1000)
        bad = rng.random(S["cam"].size) < outliers
        u = rng.standard_normal((int(bad.sum()), 3))
        u[:, 2] = np.abs(u[:, 2]) + 0.05
        S["p"] = S["p"].copy()
        S["p"][bad] = u / np.linalg.norm(u, axis=1)[:, None]
        S["bad"] = bad
    return S


def bound_point(S, t, P, s_all):
    """(P, s) with the landmark of most observations moved far outside the ring of cameras and all its scales put at the bound: the cameras
    on its side look away from it (g_s > 0: frozen), those on the other side towards it (free)"""
    L = int(np.argmax(np.bincount(S["lm"], minlength=S["m"])))
    P, s_all = P.copy(), s_all.copy()
    P[:, L] = (30.0, 1.0, 0.5)
    s_all[S["lm"] == L] = S_MIN
    return P, s_all
