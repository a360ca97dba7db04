"""numpy / scipy.sparse restatement of the bundle adjustment with focal scales behind xm_ctx_bundle_adjust_focal (include/xm_amd.h): one
g_i > 0 per camera, r_e = g_i pi(Rcw_i P_l + tcw_i) - z_e, the focal the LAST column of the camera block (cd = 7, or 4 with fixed
rotations), d r / d g = pi(X), the pose and point Jacobians those of xm_ba_numpy times g_i; a mask of free focals (a held one has a zero
column); the Levenberg-Marquardt rules of xm_ba_numpy.lm with the rule that a candidate with a focal <= 0 is an invalid step; losses
through xm_ba_loss_numpy.  Exact linear solves, or the restated PCG (xm_ba_precond_numpy.pcg) on the reduced camera system.

Layouts are the library's (xm_ba_numpy.py); focal: n."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import xm_ba_loss_numpy as rl
import xm_ba_numpy as ba
import xm_ba_precond_numpy as bp


class FocalProblem(rl.RobustProblem):
    """xm_ba_numpy.Problem (with a loss) plus a focal scale per camera.  free: n booleans (None = all).  damage: deliberate faults for the
    test that the stage bounds bite: "focal_unmasked" (the focal column ignores the mask), "pose_unscaled" (J_pose without the factor g),
    "x2_without_g" (g^2 left out of |x|^2)"""

    def __init__(self, cam, lm, p, w, n, m, fix_rotations=False, loss="trivial", a=0.0, free=None, damage=()):
        super().__init__(cam, lm, p, w, n, m, fix_rotations, loss, a)
        self.cd0 = self.cd                      # the pose columns
        self.cd = self.cd0 + 1
        self.free = np.ones(n, dtype=bool) if free is None else np.asarray(free).astype(bool)
        self.damage = set(damage)

    def project(self, Rcw, tcw, P):
        X = np.einsum("kab,kb->ka", Rcw[self.cam], P[self.lm]) + tcw[self.cam]
        return X[:, :2] / X[:, 2:3]

    def residuals(self, Rcw, tcw, P, g):
        return (g[self.cam, None] * self.project(Rcw, tcw, P) - self.z).reshape(-1)

    def cost(self, Rcw, tcw, P, g):
        return 0.5 * float(np.sum(rl.rho(self.loss, self.sq(self.residuals(Rcw, tcw, P, g)), self.a)[0]))

    def jacobian(self, Rcw, tcw, P, g):
        """(r, J): J sparse 2k x (cd n + 3 m)"""
        R = Rcw[self.cam]
        Y = np.einsum("kab,kb->ka", R, P[self.lm])
        X = Y + tcw[self.cam]
        iz = 1.0 / X[:, 2]
        u = X[:, :2] / X[:, 2:3]
        k = X.shape[0]
        d = np.zeros((k, 2, 3))
        d[:, 0, 0] = iz; d[:, 1, 1] = iz; d[:, 0, 2] = -u[:, 0] * iz; d[:, 1, 2] = -u[:, 1] * iz
        ge = g[self.cam][:, None, None]
        JP = ge * (d @ R)
        Jpose = np.concatenate([d @ (-ba.skew(Y)), d], axis=2) if self.cd0 == 6 else d
        if "pose_unscaled" not in self.damage:
            Jpose = ge * Jpose
        fr = np.ones(k) if "focal_unmasked" in self.damage else self.free[self.cam].astype(np.float64)
        Jc = np.concatenate([Jpose, (fr[:, None] * u)[:, :, None]], axis=2)
        cd = self.cd
        rows = np.repeat(np.arange(2 * k).reshape(k, 2, 1), cd + 3, axis=2)
        cols = np.concatenate([np.broadcast_to((cd * self.cam)[:, None, None] + np.arange(cd)[None, None, :], (k, 2, cd)),
                               np.broadcast_to((cd * self.n + 3 * self.lm)[:, None, None] + np.arange(3)[None, None, :], (k, 2, 3))], axis=2)
        vals = np.concatenate([Jc, JP], axis=2)
        J = sp.csr_matrix((vals.reshape(-1), (rows.reshape(-1), cols.reshape(-1))), shape=(2 * k, cd * self.n + 3 * self.m))
        return (g[self.cam, None] * u - self.z).reshape(-1), J

    def corrected(self, Rcw, tcw, P, g):
        """(F, r~, J~): Ceres's corrector scales the whole record"""
        r, J = self.jacobian(Rcw, tcw, P, g)
        r0, r1, _ = rl.rho(self.loss, self.sq(r), self.a)
        c = np.repeat(np.sqrt(r1), 2)
        return 0.5 * float(np.sum(r0)), c * r, sp.diags(c) @ J

    def moving(self):
        """the cameras whose focal moves: used and free"""
        return self.cused & self.free

    def plus(self, Rcw, tcw, P, g, d):
        cd, cd0, n = self.cd, self.cd0, self.n
        dc = d[:cd * n].reshape(n, cd)
        dP = d[cd * n:].reshape(self.m, 3)
        Rn, tn, Pn, gn = Rcw.copy(), tcw.copy(), P.copy(), g.copy()
        c, lu, mv = self.cused, self.lused, self.moving()
        if cd0 == 6:
            Rn[c] = ba.expmap(dc[c, :3]) @ Rcw[c]
        tn[c] = tcw[c] + dc[c, cd0 - 3:cd0]
        gn[mv] = g[mv] + dc[mv, cd - 1]
        Pn[lu] = P[lu] + dP[lu]
        return Rn, tn, Pn, gn

    def x2(self, tcw, P, g):
        """|x|^2 as (cameras, landmarks)"""
        c = self.cused
        gg = 0.0 if "x2_without_g" in self.damage else np.sum(g[self.moving()] ** 2)
        return np.array([(c.sum() if self.cd0 == 6 else 0) + np.sum(tcw[c] ** 2) + gg, np.sum(P[self.lused] ** 2)])

    def x_norm(self, tcw, P, g):
        return float(np.sqrt(self.x2(tcw, P, g).sum()))

    def step2(self, d):
        """|d|^2 as (cameras, landmarks), over the used ones"""
        n, cd = self.n, self.cd
        return np.array([np.sum(d[:cd * n].reshape(n, cd)[self.cused] ** 2), np.sum(d[cd * n:].reshape(self.m, 3)[self.lused] ** 2)])


def lm(cam, lm_, p, w, rot, t, P, focal=None, focal_free=None, fix_rotations=False, loss="trivial", a=0.0, max_iters=1000, function_tol=1e-6,
       gradient_tol=1e-10, parameter_tol=1e-8, eta=None):
    """the LM of xm_ctx_bundle_adjust_focal.  eta None: exact solves of the damped normal equations; else the reduced camera system by
    block-Jacobi PCG to eta.  Returns (rot, t, P, focal, info); info as xm_ba_numpy.lm plus min_focal (the least focal of any accepted
    point), invalid (iterations whose candidate had a focal <= 0) and invalid_at (which ones)"""
    n, m = t.shape[1], P.shape[1]
    pr = FocalProblem(cam, lm_, p, w, n, m, fix_rotations, loss, a, focal_free)
    cd = pr.cd
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    X = P.T.copy()
    g0 = np.ones(n) if focal is None else np.array(focal, dtype=np.float64)
    gf = g0.copy()
    radius, nu = 1e4, 2.0
    F, r, J = pr.corrected(Rcw, tcw, X, gf)
    g = J.T @ r
    info = dict(initial_cost=F, n_used=pr.n_used)
    trace = []
    iters = accepted = 0
    invalid = []
    min_focal = float(gf[pr.moving()].min(initial=np.inf))
    status = "no_convergence"
    while True:
        if np.max(np.abs(g), initial=0.0) <= gradient_tol:
            status = "gradient_tolerance"; break
        if iters >= max_iters:
            status = "max_iterations"; break
        mu = 1.0 / radius
        A = (J.T @ J).tocsc()
        D = np.clip(A.diagonal(), 1e-6, 1e32)
        if eta is None:
            d = spla.spsolve(A + sp.diags(mu * D).tocsc(), -g)
        else:
            d = _pcg_step(A + sp.diags(mu * D).tocsc(), g, cd * n, m, cd, eta)
        Jd = J @ d
        model_dec = -(float(r @ Jd) + 0.5 * float(Jd @ Jd))
        Rn, tn, Xn, gn = pr.plus(Rcw, tcw, X, gf, d)
        Fn = pr.cost(Rn, tn, Xn, gn)
        iters += 1
        positive = bool((gn[pr.moving()] > 0).all())
        if not positive:
            invalid.append(iters - 1)
        valid = positive and np.isfinite(Fn) and model_dec > 0
        rho = (F - Fn) / model_dec if valid else -1.0
        acc = bool(valid and rho > 1e-3)
        trace.append((F, Fn, mu, float(acc)))
        if positive and np.sqrt(pr.step2(d).sum()) <= parameter_tol * (pr.x_norm(tcw, X, gf) + parameter_tol):
            status = "parameter_tolerance"; break
        if acc:
            accepted += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            nu = 2.0
            Rcw, tcw, X, gf = Rn, tn, Xn, gn
            min_focal = min(min_focal, float(gf[pr.moving()].min(initial=np.inf)))
            Fold = F
            F, r, J = pr.corrected(Rcw, tcw, X, gf)
            g = J.T @ r
            if abs(Fold - Fn) <= function_tol * Fold:
                status = "function_tolerance"; break
        else:
            radius /= nu
            nu *= 2.0
            if radius < 1e-32:
                status = "no_progress"; break
    rot_o, t_o = ba.to_camera_to_world(Rcw, tcw)
    rot_o[:, np.repeat(~pr.cused, 3)] = rot[:, np.repeat(~pr.cused, 3)]
    t_o[:, ~pr.cused] = t[:, ~pr.cused]
    P_o = X.T.copy()
    P_o[:, ~pr.lused] = P[:, ~pr.lused]
    gf[~pr.moving()] = g0[~pr.moving()]                  # never moved: the caller's bits
    info.update(status=ba.STATUS[status], iters=iters, accepted=accepted, final_cost=F, gradient_max=float(np.max(np.abs(g), initial=0.0)),
                trace=np.array(trace).reshape(-1, 4), min_focal=min_focal, invalid=len(invalid), invalid_at=invalid)
    return rot_o, t_o, P_o, gf, info


def _pcg_step(H, g, ncam, m, cd, eta):
    """the step of (H) d = -g with the landmarks eliminated and the reduced camera system solved by block-Jacobi PCG to eta from zero"""
    H = H.tocsr()
    U, W, V = H[:ncam, :ncam], H[:ncam, ncam:], H[ncam:, ncam:].tocoo()
    Vd = np.zeros((m, 3, 3))
    Vd[V.row // 3, V.row % 3, V.col % 3] = V.data
    empty = ~(np.abs(Vd).sum(axis=(1, 2)) > 0)
    Vd[empty] = np.eye(3)
    Vinv = sp.block_diag(list(np.linalg.inv(Vd)), format="csr")
    S = (U - W @ Vinv @ W.T).tocsr()
    b = -g[:ncam] + W @ (Vinv @ g[ncam:])
    Ji = bp.jacobi_inverse(S, cd)
    dc, _, _ = bp.pcg(S, b, lambda v: Ji @ v, eta)
    dP = -(Vinv @ (g[ncam:] + W.T @ dc))
    return np.concatenate([dc, dP])


def sq_errors(cam, lm_, p, w, rot, t, P, focal):
    """|g_i pi(X) - z|^2 of every observation in input order, -1 where it is not used (xm_ctx_reprojection_errors_focal)"""
    n, m = t.shape[1], P.shape[1]
    u = ba.used_mask(p, w)
    pr = FocalProblem(cam, lm_, p, np.ones(len(cam)), n, m)       # every observation with p2 > 0, in input order
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    r = pr.residuals(Rcw, tcw, P.T.copy(), np.asarray(focal, dtype=np.float64))
    full = -np.ones(len(cam))
    full[np.asarray(p)[:, 2] > 0] = r[0::2] ** 2 + r[1::2] ** 2
    out = -np.ones(len(cam))
    out[u] = full[u]
    return out


def scale_observations(S, ratio):
    """the scene S with every camera's observations as a wrong focal prior sees them: the first two coordinates times ratio[cam] (the
    true focal scale of camera i is then ratio[i])"""
    S = dict(S)
    p = np.array(S["p"], dtype=np.float64)
    p[:, :2] *= np.asarray(ratio)[S["cam"]][:, None]
    S["p"] = p
    return S


def focal_ratios(n, seed, lo=0.8, hi=1.25):
    return np.random.default_rng(seed).uniform(lo, hi, n)


def gradient_at(cam, lm_, p, w, rot, t, P, focal, focal_free=None, fix_rotations=False):
    """J^T r at a point given in the library's layouts"""
    pr = FocalProblem(cam, lm_, p, w, t.shape[1], P.shape[1], fix_rotations, free=focal_free)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    r, J = pr.jacobian(Rcw, tcw, P.T.copy(), np.asarray(focal, dtype=np.float64))
    return J.T @ r
