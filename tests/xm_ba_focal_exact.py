"""numpy.longdouble statement of one linearisation of xm_ctx_bundle_adjust_focal: xm_ba_exact.Exact with the focal column, written from the
definitions in include/xm_amd.h (r_e = g_i pi(X) - z_e; tangent (dtheta, dt, dg) or (dt, dg); d r / d g = pi(X) for a free focal, 0 for a
held one; pose and point Jacobians times g_i; g += dg for used cameras with a free focal; |x|^2 adds their g^2).  Everything after the
per-observation records (V, g, D, V*^-1, U*, S, b, S_ii^-1, dP) is xm_ba_exact's code, run on records of width cd = 7 / 4.  The judge of
tests/test_gpu_ba_focal_stages.py and of the f64 restatement xm_ba_focal_numpy.py."""
import numpy as np

import xm_ba_exact as ex

LD = ex.LD


class FocalExact(ex.Exact):
    """Exact at (rot, t, P, focal) with the mask free (n booleans, None = all).  Attributes as Exact, blocks of cd = 7 / 4."""

    # Exact.__init__ sets self.cd to the pose columns (6 / 3) and sizes every block by it; here the value it stores is one more
    @property
    def cd(self):
        return self._cd

    @cd.setter
    def cd(self, pose_columns):
        self._cd = pose_columns + 1

    def __init__(self, cam, lm, p, w, n, m, rot, t, P, focal, mu, fix_rotations=False, loss="trivial", a=0.0, free=None):
        self.g = np.asarray(focal, dtype=LD)
        self.free = np.ones(n, dtype=bool) if free is None else np.asarray(free).astype(bool)
        super().__init__(cam, lm, p, w, n, m, rot, t, P, mu, fix_rotations, loss, a)
        self.moving = self.cused & self.free

    def linearise(self, Rcw, tcw, P, g=None):
        g = self.g if g is None else g
        R = Rcw[self.cam]
        Y = np.einsum("kab,kb->ka", R, P[self.lm])
        X = Y + tcw[self.cam]
        iz = 1 / X[:, 2]
        uu = X[:, :2] * iz[:, None]
        d = np.zeros((X.shape[0], 2, 3), dtype=LD)
        d[:, 0, 0] = iz; d[:, 1, 1] = iz; d[:, 0, 2] = -uu[:, 0] * iz; d[:, 1, 2] = -uu[:, 1] * iz
        ge = g[self.cam]
        JP = ge[:, None, None] * (d @ R)
        Jpose = np.concatenate([-(d @ ex.skew(Y)), d], axis=2) if self.cd == 7 else d
        Jf = np.where(self.free[self.cam][:, None], uu, LD(0))
        Jc = np.concatenate([ge[:, None, None] * Jpose, Jf[:, :, None]], axis=2)
        return ge[:, None] * uu - self.z, Jc, JP

    def cost_at(self, Rcw, tcw, P, g=None):
        r, _, _ = self.linearise(Rcw, tcw, P, g)
        return LD(0.5) * np.sum(ex.rho(self.loss, np.sum(r * r, axis=1), self.a)[0])

    def candidate(self, dc):
        """as Exact.candidate, plus focal1; cost1 is that of the candidate whatever the sign of its focals, positive says whether all are > 0"""
        n, cd = self.n, self.cd
        dc = np.asarray(dc, dtype=LD).reshape(n, cd)
        dP = self.back_substitute(dc)
        cu, lu, mv = self.cused, self.lused, self.moving
        R1, t1, P1, g1 = self.Rcw.copy(), self.tcw.copy(), self.P.copy(), self.g.copy()
        if cd == 7:
            R1[cu] = ex.expmap(dc[cu, :3]) @ self.Rcw[cu]
        t1[cu] = self.tcw[cu] + dc[cu, cd - 4:cd - 1]
        g1[mv] = self.g[mv] + dc[mv, cd - 1]
        P1[lu] = self.P[lu] + dP[lu]
        Jd = np.einsum("kra,ka->kr", self.Jc, dc[self.cam]) + np.einsum("kra,ka->kr", self.JP, dP[self.lm])
        model = np.sum(self.r * Jd) + LD(0.5) * np.sum(Jd * Jd)
        rot1 = np.concatenate([R1[i].T for i in range(n)], axis=1)
        c1 = -np.einsum("iba,ib->ai", R1, t1)
        return dict(dP=dP, Rcw1=R1, tcw1=t1, rot1=rot1, t1=c1, P1=P1, focal1=g1, cost1=self.cost_at(R1, t1, P1, g1), model=model,
                    positive=bool((g1[mv] > 0).all()),
                    step2=(np.sum(dc[cu] ** 2), np.sum(dP[lu] ** 2)),
                    x2=((cu.sum() if cd == 7 else 0) + np.sum(self.tcw[cu] ** 2) + np.sum(self.g[mv] ** 2), np.sum(self.P[lu] ** 2)))


def central_difference(cam, lm, p, w, n, m, rot, t, P, focal, fix_rotations=False, free=None, h=LD(1e-9)):
    """the dense Jacobian (2k x (cd n + 3 m)) of the UNCORRECTED residuals by central differences in longdouble, in the tangent coordinates
    of the library; the focal column of a held camera is 0 by the definition of the tangent, not by differencing"""
    E = FocalExact(cam, lm, p, w, n, m, rot, t, P, focal, 1.0, fix_rotations, free=free)
    cd = E.cd
    k = E.cam.size
    J = np.zeros((2 * k, cd * n + 3 * m), dtype=LD)

    def res(dc, dP):
        R1, t1, g1 = E.Rcw.copy(), E.tcw.copy(), E.g.copy()
        if cd == 7:
            R1 = ex.expmap(dc[:, :3]) @ E.Rcw
        t1 = E.tcw + dc[:, cd - 4:cd - 1]
        g1 = E.g + np.where(E.free, dc[:, cd - 1], LD(0))
        return E.linearise(R1, t1, E.P + dP, g1)[0].reshape(-1)

    for j in range(cd * n + 3 * m):
        dc, dP = np.zeros((n, cd), dtype=LD), np.zeros((m, 3), dtype=LD)
        (dc.reshape(-1) if j < cd * n else dP.reshape(-1))[j if j < cd * n else j - cd * n] = h
        J[:, j] = (res(dc, dP) - res(-dc, -dP)) / (2 * h)
    return J


def lm_trace(cam, lm, p, w, rot, t, P, focal, free=None, fix_rotations=False, max_iters=10):
    """the first max_iters iterations of the Levenberg-Marquardt loop of xm_ctx_bundle_adjust_focal in longdouble with exact solves of the
    reduced camera system (no stop rule but the iteration count): rows (cost, candidate cost, mu, accepted).  For choosing scenes whose
    accept sequence does not hang on f64 rounding (test_gpu_ba_focal.py)"""
    n, m = np.asarray(t).shape[1], np.asarray(P).shape[1]
    rot, t, P, g = np.asarray(rot, dtype=LD), np.asarray(t, dtype=LD), np.asarray(P, dtype=LD), np.asarray(focal, dtype=LD)
    radius, nu = LD(1e4), LD(2)
    rows = []
    for _ in range(max_iters):
        mu = 1 / radius
        E = FocalExact(cam, lm, p, w, n, m, rot, t, P, g, mu, fix_rotations, free=free)
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
            g = c["focal1"]
        else:
            radius /= nu
            nu *= 2
    return np.array(rows)
