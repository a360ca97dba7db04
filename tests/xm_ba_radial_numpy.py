"""numpy / scipy.sparse restatement of the bundle adjustment with a focal scale and one radial coefficient per camera behind
xm_ctx_bundle_adjust_radial (include/xm_amd.h): with u = pi(Rcw_i P_l + tcw_i), rho^2 = |u|^2, s = 1 + k_i rho^2,
    r_e = g_i s u - z_e,
COLMAP's SIMPLE_RADIAL and BAL's model with k2 = 0.  GLOMAP builds the cost function over the camera's whole parameter vector
(estimators/bundle_adjustment.cc:72-84) and with optimize_intrinsics holds only the principal point (bundle_adjustment.cc:163-175), so a
radial coefficient moves with the focal.  The camera block is (pose columns, dg, dk): cd = 8, or 5 with fixed rotations; d r / d g = s u,
d r / d k = g rho^2 u, d r / d u = g (s I + 2 k u u^T) in front of the pinhole pose and point Jacobians of xm_ba_numpy.  Two independent
masks (a held column is zero).  The Levenberg-Marquardt rules of xm_ba_focal_numpy.lm with one more invalid step: a candidate at which
some used observation has 1 + 3 k rho^2 <= 0 (the radial map folds there).

Layouts are the library's (xm_ba_numpy.py); focal, dist: n."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import xm_ba_focal_numpy as bf
import xm_ba_loss_numpy as rl
import xm_ba_numpy as ba


class RadialProblem(bf.FocalProblem):
    """FocalProblem plus a radial coefficient per camera.  free, kfree: n booleans each (None = all).  damage: deliberate faults for the
    test that the stage bounds bite: "dist_unmasked" (the distortion column ignores its mask), "pose_pinhole" (the pose and point Jacobians
    without the factor s I + 2 k u u^T), "x2_without_k" (k^2 left out of |x|^2)"""

    def __init__(self, cam, lm, p, w, n, m, fix_rotations=False, loss="trivial", a=0.0, free=None, kfree=None, damage=()):
        super().__init__(cam, lm, p, w, n, m, fix_rotations, loss, a, free, damage)
        self.cd = self.cd0 + 2
        self.kfree = np.ones(n, dtype=bool) if kfree is None else np.asarray(kfree).astype(bool)

    def distorted(self, Rcw, tcw, P, g, kd):
        """(g s u, rho^2) per used observation"""
        u = self.project(Rcw, tcw, P)
        rho2 = np.sum(u * u, axis=1)
        return (g[self.cam] * (1.0 + kd[self.cam] * rho2))[:, None] * u, rho2

    def residuals(self, Rcw, tcw, P, g, kd):
        return (self.distorted(Rcw, tcw, P, g, kd)[0] - self.z).reshape(-1)

    def cost(self, Rcw, tcw, P, g, kd):
        return 0.5 * float(np.sum(rl.rho(self.loss, self.sq(self.residuals(Rcw, tcw, P, g, kd)), self.a)[0]))

    def folded(self, Rcw, tcw, P, kd):
        """whether some used observation lies at or past the fold 1 + 3 k rho^2 = 0"""
        u = self.project(Rcw, tcw, P)
        return bool((~(1.0 + 3.0 * kd[self.cam] * np.sum(u * u, axis=1) > 0.0)).any())

    def jacobian(self, Rcw, tcw, P, g, kd):
        """(r, J): J sparse 2k x (cd n + 3 m)"""
        R = Rcw[self.cam]
        Y = np.einsum("kab,kb->ka", R, P[self.lm])
        X = Y + tcw[self.cam]
        iz = 1.0 / X[:, 2]
        u = X[:, :2] / X[:, 2:3]
        k = X.shape[0]
        d = np.zeros((k, 2, 3))
        d[:, 0, 0] = iz; d[:, 1, 1] = iz; d[:, 0, 2] = -u[:, 0] * iz; d[:, 1, 2] = -u[:, 1] * iz
        ge, ke = g[self.cam], kd[self.cam]
        rho2 = np.sum(u * u, axis=1)
        s = 1.0 + ke * rho2
        M = ge[:, None, None] * (s[:, None, None] * np.eye(2)[None] + 2.0 * ke[:, None, None] * u[:, :, None] * u[:, None, :])
        if "pose_pinhole" in self.damage:
            M = ge[:, None, None] * np.broadcast_to(np.eye(2), (k, 2, 2))
        JP = M @ (d @ R)
        Jpose = M @ (np.concatenate([d @ (-ba.skew(Y)), d], axis=2) if self.cd0 == 6 else d)
        fr = self.free[self.cam].astype(np.float64)
        kr = np.ones(k) if "dist_unmasked" in self.damage else self.kfree[self.cam].astype(np.float64)
        Jc = np.concatenate([Jpose, ((fr * s)[:, None] * u)[:, :, None], ((kr * ge * rho2)[:, None] * u)[:, :, None]], axis=2)
        cd = self.cd
        rows = np.repeat(np.arange(2 * k).reshape(k, 2, 1), cd + 3, axis=2)
        cols = np.concatenate([np.broadcast_to((cd * self.cam)[:, None, None] + np.arange(cd)[None, None, :], (k, 2, cd)),
                               np.broadcast_to((cd * self.n + 3 * self.lm)[:, None, None] + np.arange(3)[None, None, :], (k, 2, 3))], axis=2)
        vals = np.concatenate([Jc, JP], axis=2)
        J = sp.csr_matrix((vals.reshape(-1), (rows.reshape(-1), cols.reshape(-1))), shape=(2 * k, cd * self.n + 3 * self.m))
        return ((ge * s)[:, None] * u - self.z).reshape(-1), J

    def corrected(self, Rcw, tcw, P, g, kd):
        """(F, r~, J~): Ceres's corrector scales the whole record"""
        r, J = self.jacobian(Rcw, tcw, P, g, kd)
        r0, r1, _ = rl.rho(self.loss, self.sq(r), self.a)
        c = np.repeat(np.sqrt(r1), 2)
        return 0.5 * float(np.sum(r0)), c * r, sp.diags(c) @ J

    def kmoving(self):
        """the cameras whose coefficient moves: used and free"""
        return self.cused & self.kfree

    def plus(self, Rcw, tcw, P, g, kd, d):
        cd, cd0, n = self.cd, self.cd0, self.n
        dc = d[:cd * n].reshape(n, cd)
        dP = d[cd * n:].reshape(self.m, 3)
        Rn, tn, Pn, gn, kn = Rcw.copy(), tcw.copy(), P.copy(), g.copy(), kd.copy()
        c, lu, mv, kv = self.cused, self.lused, self.moving(), self.kmoving()
        if cd0 == 6:
            Rn[c] = ba.expmap(dc[c, :3]) @ Rcw[c]
        tn[c] = tcw[c] + dc[c, cd0 - 3:cd0]
        gn[mv] = g[mv] + dc[mv, cd - 2]
        kn[kv] = kd[kv] + dc[kv, cd - 1]
        Pn[lu] = P[lu] + dP[lu]
        return Rn, tn, Pn, gn, kn

    def x2(self, tcw, P, g, kd):
        """|x|^2 as (cameras, landmarks)"""
        c = self.cused
        kk = 0.0 if "x2_without_k" in self.damage else np.sum(kd[self.kmoving()] ** 2)
        return np.array([(c.sum() if self.cd0 == 6 else 0) + np.sum(tcw[c] ** 2) + np.sum(g[self.moving()] ** 2) + kk, np.sum(P[self.lused] ** 2)])

    def x_norm(self, tcw, P, g, kd):
        return float(np.sqrt(self.x2(tcw, P, g, kd).sum()))


def lm(cam, lm_, p, w, rot, t, P, focal=None, focal_free=None, dist=None, dist_free=None, fix_rotations=False, loss="trivial", a=0.0,
       max_iters=1000, function_tol=1e-6, gradient_tol=1e-10, parameter_tol=1e-8, eta=None):
    """the LM of xm_ctx_bundle_adjust_radial: xm_ba_focal_numpy.lm statement for statement, with the coefficients beside the focal scales
    and the fold among the invalid candidates.  Returns (rot, t, P, focal, dist, info); info as there (invalid counts both kinds)"""
    n, m = t.shape[1], P.shape[1]
    pr = RadialProblem(cam, lm_, p, w, n, m, fix_rotations, loss, a, focal_free, dist_free)
    cd = pr.cd
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    X = P.T.copy()
    g0 = np.ones(n) if focal is None else np.array(focal, dtype=np.float64)
    k0 = np.zeros(n) if dist is None else np.array(dist, dtype=np.float64)
    gf, kf = g0.copy(), k0.copy()
    radius, nu = 1e4, 2.0
    F, r, J = pr.corrected(Rcw, tcw, X, gf, kf)
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
            d = bf._pcg_step(A + sp.diags(mu * D).tocsc(), g, cd * n, m, cd, eta)
        Jd = J @ d
        model_dec = -(float(r @ Jd) + 0.5 * float(Jd @ Jd))
        Rn, tn, Xn, gn, kn = pr.plus(Rcw, tcw, X, gf, kf, d)
        Fn = pr.cost(Rn, tn, Xn, gn, kn)
        iters += 1
        positive = bool((gn[pr.moving()] > 0).all()) and not pr.folded(Rn, tn, Xn, kn)
        if not positive:
            invalid.append(iters - 1)
        valid = positive and np.isfinite(Fn) and model_dec > 0
        rho = (F - Fn) / model_dec if valid else -1.0
        acc = bool(valid and rho > 1e-3)
        trace.append((F, Fn, mu, float(acc)))
        if positive and np.sqrt(pr.step2(d).sum()) <= parameter_tol * (pr.x_norm(tcw, X, gf, kf) + parameter_tol):
            status = "parameter_tolerance"; break
        if acc:
            accepted += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            nu = 2.0
            Rcw, tcw, X, gf, kf = Rn, tn, Xn, gn, kn
            min_focal = min(min_focal, float(gf[pr.moving()].min(initial=np.inf)))
            Fold = F
            F, r, J = pr.corrected(Rcw, tcw, X, gf, kf)
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
    kf[~pr.kmoving()] = k0[~pr.kmoving()]
    info.update(status=ba.STATUS[status], iters=iters, accepted=accepted, final_cost=F, gradient_max=float(np.max(np.abs(g), initial=0.0)),
                trace=np.array(trace).reshape(-1, 4), min_focal=min_focal, invalid=len(invalid), invalid_at=invalid)
    return rot_o, t_o, P_o, gf, kf, info


def sq_errors(cam, lm_, p, w, rot, t, P, focal, dist):
    """|g_i s u - z|^2 of every observation in input order, -1 where it is not used (xm_ctx_reprojection_errors_radial)"""
    n, m = t.shape[1], P.shape[1]
    u = ba.used_mask(p, w)
    pr = RadialProblem(cam, lm_, p, np.ones(len(cam)), n, m)       # every observation with p2 > 0, in input order
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    r = pr.residuals(Rcw, tcw, P.T.copy(), np.asarray(focal, dtype=np.float64), np.asarray(dist, dtype=np.float64))
    full = -np.ones(len(cam))
    full[np.asarray(p)[:, 2] > 0] = r[0::2] ** 2 + r[1::2] ** 2
    out = -np.ones(len(cam))
    out[u] = full[u]
    return out


def distort_observations(S, ratio, k):
    """the scene S as cameras with the true focal scales ratio and radial coefficients k see it through priors g = 1, k = 0: with
    u = (p0, p1) / p2 the first two coordinates become ratio (1 + k |u|^2) u p2 (xm_ba_focal_numpy.scale_observations at k = 0)"""
    S = dict(S)
    p = np.array(S["p"], dtype=np.float64)
    u = p[:, :2] / p[:, 2:3]
    f = np.asarray(ratio)[S["cam"]] * (1.0 + np.asarray(k)[S["cam"]] * np.sum(u * u, axis=1))
    p[:, :2] *= f[:, None]
    S["p"] = p
    return S


def dist_coefficients(n, seed, lo=-0.15, hi=0.15):
    return np.random.default_rng(seed).uniform(lo, hi, n)


def gradient_at(cam, lm_, p, w, rot, t, P, focal, dist, focal_free=None, dist_free=None, fix_rotations=False):
    """J^T r at a point given in the library's layouts"""
    pr = RadialProblem(cam, lm_, p, w, t.shape[1], P.shape[1], fix_rotations, free=focal_free, kfree=dist_free)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    r, J = pr.jacobian(Rcw, tcw, P.T.copy(), np.asarray(focal, dtype=np.float64), np.asarray(dist, dtype=np.float64))
    return J.T @ r
