"""numpy.longdouble statement of one linearisation of xm_ctx_bundle_adjust_radial: xm_ba_exact.Exact with the focal and the distortion
column, written from the definitions in include/xm_amd.h (u = pi(X), rho^2 = |u|^2, s = 1 + k rho^2, r_e = g_i s u - z_e; tangent
(dtheta, dt, dg, dk) or (dt, dg, dk); d r / d g = s u for a free focal, d r / d k = g rho^2 u for a free coefficient, 0 for held ones;
d r / d u = g (s I + 2 k u u^T) in front of the pinhole pose and point Jacobians; g += dg, k += dk for used cameras with the column
free; |x|^2 adds their g^2 and k^2).  GLOMAP's cost function takes the camera's whole parameter vector
(estimators/bundle_adjustment.cc:72-84) and holds only the principal point (bundle_adjustment.cc:163-175).  Everything after the
per-observation records is xm_ba_exact's code, run on records of width cd = 8 / 5.  The judge of tests/test_gpu_ba_radial_stages.py and of
the f64 restatement xm_ba_radial_numpy.py."""
import numpy as np

import xm_ba_exact as ex

LD = ex.LD


class RadialExact(ex.Exact):
    """Exact at (rot, t, P, focal, dist) with the masks free, kfree (n booleans, None = all).  Attributes as Exact, blocks of cd = 8 / 5."""

    # Exact.__init__ sets self.cd to the pose columns (6 / 3) and sizes every block by it; here the value it stores is two more
    @property
    def cd(self):
        return self._cd

    @cd.setter
    def cd(self, pose_columns):
        self._cd = pose_columns + 2

    def __init__(self, cam, lm, p, w, n, m, rot, t, P, focal, dist, mu, fix_rotations=False, loss="trivial", a=0.0, free=None, kfree=None):
        self.g = np.asarray(focal, dtype=LD)
        self.k = np.asarray(dist, dtype=LD)
        self.free = np.ones(n, dtype=bool) if free is None else np.asarray(free).astype(bool)
        self.kfree = np.ones(n, dtype=bool) if kfree is None else np.asarray(kfree).astype(bool)
        super().__init__(cam, lm, p, w, n, m, rot, t, P, mu, fix_rotations, loss, a)
        self.moving = self.cused & self.free
        self.kmoving = self.cused & self.kfree

    def project(self, Rcw, tcw, P):
        X = np.einsum("kab,kb->ka", Rcw[self.cam], P[self.lm]) + tcw[self.cam]
        return X[:, :2] / X[:, 2:3]

    def linearise(self, Rcw, tcw, P, g=None, k=None):
        g = self.g if g is None else g
        k = self.k if k is None else k
        R = Rcw[self.cam]
        Y = np.einsum("kab,kb->ka", R, P[self.lm])
        X = Y + tcw[self.cam]
        iz = 1 / X[:, 2]
        uu = X[:, :2] * iz[:, None]
        d = np.zeros((X.shape[0], 2, 3), dtype=LD)
        d[:, 0, 0] = iz; d[:, 1, 1] = iz; d[:, 0, 2] = -uu[:, 0] * iz; d[:, 1, 2] = -uu[:, 1] * iz
        ge, ke = g[self.cam], k[self.cam]
        rho2 = np.sum(uu * uu, axis=1)
        s = 1 + ke * rho2
        M = ge[:, None, None] * (s[:, None, None] * np.eye(2, dtype=LD)[None] + 2 * ke[:, None, None] * uu[:, :, None] * uu[:, None, :])
        JP = M @ (d @ R)
        Jpose = M @ (np.concatenate([-(d @ ex.skew(Y)), d], axis=2) if self.cd == 8 else d)
        Jf = np.where(self.free[self.cam][:, None], s[:, None] * uu, LD(0))
        Jk = np.where(self.kfree[self.cam][:, None], (ge * rho2)[:, None] * uu, LD(0))
        Jc = np.concatenate([Jpose, Jf[:, :, None], Jk[:, :, None]], axis=2)
        return (ge * s)[:, None] * uu - self.z, Jc, JP

    def cost_at(self, Rcw, tcw, P, g=None, k=None):
        r, _, _ = self.linearise(Rcw, tcw, P, g, k)
        return LD(0.5) * np.sum(ex.rho(self.loss, np.sum(r * r, axis=1), self.a)[0])

    def candidate(self, dc):
        """as Exact.candidate, plus focal1 and dist1; cost1 is that of the candidate whatever it is, positive says whether all moving
        focals are > 0 and no used observation lies at or past the fold 1 + 3 k rho^2 = 0"""
        n, cd = self.n, self.cd
        dc = np.asarray(dc, dtype=LD).reshape(n, cd)
        dP = self.back_substitute(dc)
        cu, lu, mv, kv = self.cused, self.lused, self.moving, self.kmoving
        R1, t1, P1, g1, k1 = self.Rcw.copy(), self.tcw.copy(), self.P.copy(), self.g.copy(), self.k.copy()
        if cd == 8:
            R1[cu] = ex.expmap(dc[cu, :3]) @ self.Rcw[cu]
        t1[cu] = self.tcw[cu] + dc[cu, cd - 5:cd - 2]
        g1[mv] = self.g[mv] + dc[mv, cd - 2]
        k1[kv] = self.k[kv] + dc[kv, cd - 1]
        P1[lu] = self.P[lu] + dP[lu]
        Jd = np.einsum("kra,ka->kr", self.Jc, dc[self.cam]) + np.einsum("kra,ka->kr", self.JP, dP[self.lm])
        model = np.sum(self.r * Jd) + LD(0.5) * np.sum(Jd * Jd)
        rot1 = np.concatenate([R1[i].T for i in range(n)], axis=1)
        c1 = -np.einsum("iba,ib->ai", R1, t1)
        u1 = self.project(R1, t1, P1)
        fold = 1 + 3 * k1[self.cam] * np.sum(u1 * u1, axis=1)
        return dict(dP=dP, Rcw1=R1, tcw1=t1, rot1=rot1, t1=c1, P1=P1, focal1=g1, dist1=k1, cost1=self.cost_at(R1, t1, P1, g1, k1), model=model,
                    positive=bool((g1[mv] > 0).all()) and bool((fold > 0).all()), fold_min=fold.min(initial=LD(np.inf)),
                    step2=(np.sum(dc[cu] ** 2), np.sum(dP[lu] ** 2)),
                    x2=((cu.sum() if cd == 8 else 0) + np.sum(self.tcw[cu] ** 2) + np.sum(self.g[mv] ** 2) + np.sum(self.k[kv] ** 2),
                        np.sum(self.P[lu] ** 2)))


def central_difference(cam, lm, p, w, n, m, rot, t, P, focal, dist, fix_rotations=False, free=None, kfree=None, h=LD(1e-9)):
    """the dense Jacobian (2k x (cd n + 3 m)) of the UNCORRECTED residuals by central differences in longdouble, in the tangent coordinates
    of the library; the focal and distortion columns of held cameras are 0 by the definition of the tangent, not by differencing"""
    E = RadialExact(cam, lm, p, w, n, m, rot, t, P, focal, dist, 1.0, fix_rotations, free=free, kfree=kfree)
    cd = E.cd
    k = E.cam.size
    J = np.zeros((2 * k, cd * n + 3 * m), dtype=LD)

    def res(dc, dP):
        R1 = E.Rcw.copy()
        if cd == 8:
            R1 = ex.expmap(dc[:, :3]) @ E.Rcw
        t1 = E.tcw + dc[:, cd - 5:cd - 2]
        g1 = E.g + np.where(E.free, dc[:, cd - 2], LD(0))
        k1 = E.k + np.where(E.kfree, dc[:, cd - 1], LD(0))
        return E.linearise(R1, t1, E.P + dP, g1, k1)[0].reshape(-1)

    for j in range(cd * n + 3 * m):
        dc, dP = np.zeros((n, cd), dtype=LD), np.zeros((m, 3), dtype=LD)
        (dc.reshape(-1) if j < cd * n else dP.reshape(-1))[j if j < cd * n else j - cd * n] = h
        J[:, j] = (res(dc, dP) - res(-dc, -dP)) / (2 * h)
    return J


def lm_trace(cam, lm, p, w, rot, t, P, focal, dist, free=None, kfree=None, fix_rotations=False, max_iters=10):
    """the first max_iters iterations of the Levenberg-Marquardt loop of xm_ctx_bundle_adjust_radial in longdouble with exact solves of the
    reduced camera system (no stop rule but the iteration count): rows (cost, candidate cost, mu, accepted).  For choosing scenes whose
    accept sequence does not hang on f64 rounding (test_gpu_ba_radial.py)"""
    n, m = np.asarray(t).shape[1], np.asarray(P).shape[1]
    rot, t, P = np.asarray(rot, dtype=LD), np.asarray(t, dtype=LD), np.asarray(P, dtype=LD)
    g, kd = np.asarray(focal, dtype=LD), np.asarray(dist, dtype=LD)
    radius, nu = LD(1e4), LD(2)
    rows = []
    for _ in range(max_iters):
        mu = 1 / radius
        E = RadialExact(cam, lm, p, w, n, m, rot, t, P, g, kd, mu, fix_rotations, free=free, kfree=kfree)
        dc = ex.gj_inverse(E.S) @ E.b
        c = E.candidate(dc)
        F, Fn, dm = E.cost, c["cost1"], -c["model"]
        valid = c["positive"] and np.isfinite(Fn) and dm > 0
        rho = (F - Fn) / dm if valid else LD(-1)
        acc = bool(valid and rho > 1e-3)
        rows.append((float(F), float(Fn), float(mu), float(acc)))
        if acc:
            radius = min(LD(1e16), radius / max(LD(1) / 3, 1 - (2 * rho - 1) ** 3))
            nu = LD(2)
            cu, lu = E.cused, E.lused
            rot = np.where(np.repeat(cu, 3)[None, :], c["rot1"], rot)
            t = np.where(cu[None, :], c["t1"], t)
            P = np.where(lu[None, :], c["P1"].T, P)
            g, kd = c["focal1"], c["dist1"]
        else:
            radius /= nu
            nu *= 2
    return np.array(rows)
