"""numpy.longdouble statement of one linearisation of xm_ctx_bundle_adjust, written from the definitions in include/xm_amd.h and
xm-code_amd/csrc/xm_ba.h (not from the kernels, and not by calling the f64 restatements with another dtype): residuals, per-observation
Jacobians, the four rho and rho', V, g, D = clip(diag(J^T J), 1e-6, 1e32), V*^-1, U*, S, b, S_ii^-1, S_aa^-1 by aggregate, P, A_c, M^-1,
dP, the exponential map, the candidate and the model value.  It is the judge of tests/test_gpu_ba_stages.py and of the f64 restatements
(tests/test_ba_exact.py); numpy.linalg does not take longdouble, so the inverses are a pivoted Gauss-Jordan written here.

Layouts are the library's (xm_ba_numpy.py): rot 3 x 3n, t 3 x n, P 3 x m, observations (cam, lm, p, w)."""
import numpy as np

LD = np.longdouble
# the 80-bit extended type (x86-64); anywhere longdouble is the double a reference built on it would be no better than the code under test
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended type on this platform: xm_ba_exact cannot serve as a reference"

AGG_CAMS = 16
TINY = LD(np.finfo(np.float64).tiny)


def gj_inverse(A):
    """inverse of a stack of square matrices (..., k, k) by Gauss-Jordan elimination with partial pivoting, in longdouble"""
    A = np.array(A, dtype=LD)
    shape = A.shape
    k = shape[-1]
    M = np.concatenate([A.reshape(-1, k, k), np.broadcast_to(np.eye(k, dtype=LD), (A.size // (k * k), k, k))], axis=2)
    ar = np.arange(M.shape[0])
    for j in range(k):
        piv = j + np.argmax(np.abs(M[:, j:, j]), axis=1)
        rowj, rowp = M[ar, j].copy(), M[ar, piv].copy()
        M[ar, piv] = rowj
        M[ar, j] = rowp / rowp[:, j][:, None]
        f = M[:, :, j].copy()
        f[:, j] = 0
        M -= f[:, :, None] * M[:, j][:, None, :]
    return M[:, :, k:].reshape(shape)


def skew(v):
    K = np.zeros(v.shape[:-1] + (3, 3), dtype=LD)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -v[..., 2], v[..., 1], -v[..., 0]
    K[..., 1, 0], K[..., 2, 0], K[..., 2, 1] = v[..., 2], -v[..., 1], v[..., 0]
    return K


def expmap(w):
    """Exp of rotation vectors (k x 3): I + sin(th) / th K + (1 - cos th) / th^2 K^2, the second coefficient as 2 sin^2(th / 2) / th^2 so
    that nothing cancels; th = 0: 1 and 1/2"""
    w = np.asarray(w, dtype=LD)
    th = np.sqrt(np.sum(w * w, axis=1))
    z = th == 0
    ths = np.where(z, LD(1), th)
    A = np.where(z, LD(1), np.sin(ths) / ths)
    h = np.sin(ths / 2) / ths
    B = np.where(z, LD(0.5), 2 * h * h)
    K = skew(w)
    return np.eye(3, dtype=LD) + A[:, None, None] * K + B[:, None, None] * (K @ K)


def rho(loss, s, a):
    """(rho, rho') of Ceres's losses at s = |r|^2 with scale a (xm_amd.h): Huber s | 2 a sqrt(s) - a^2, SoftL1 2 b (sqrt(1 + s / b) - 1),
    Cauchy b log(1 + s / b), Arctan a atan2(s, a); rho' clamped below at the smallest normal double"""
    s = np.asarray(s, dtype=LD)
    a = LD(a)
    b = a * a
    if loss == "trivial":
        return s.copy(), np.ones_like(s)
    if loss == "huber":
        big = s > b
        rt = np.sqrt(np.where(big, s, LD(1)))
        return np.where(big, 2 * a * rt - b, s), np.where(big, np.maximum(TINY, a / rt), LD(1))
    if loss == "soft_l1":
        rt = np.sqrt(1 + s / b)
        return 2 * s / (rt + 1), np.maximum(TINY, 1 / rt)          # 2 b (rt - 1) without the cancellation at small s
    if loss == "cauchy":
        return b * np.log1p(s / b), np.maximum(TINY, 1 / (1 + s / b))
    if loss == "arctan":
        return a * np.arctan2(s, a), np.maximum(TINY, 1 / (1 + s * s / b))
    raise ValueError(loss)


def clipd(d):
    return np.clip(d, LD(1e-6), LD(1e32))


class Exact:
    """one linearisation at (rot, t, P) with damping mu.  Attributes (longdouble): cost, n_used, gmax, cused, lused, V, g_l (m x 3),
    Vinv (m x 3 x 3), Ustar (n x cd x cd), S (cd n square), b (cd n), Sinv (n x cd x cd: the inverted diagonal blocks)"""

    def __init__(self, cam, lm, p, w, n, m, rot, t, P, mu, fix_rotations=False, loss="trivial", a=0.0):
        p = np.asarray(p, dtype=np.float64)
        u = (np.asarray(w) > 0) & (p[:, 2] > 0)
        self.cam, self.lm = np.asarray(cam)[u].astype(np.int64), np.asarray(lm)[u].astype(np.int64)
        q = p[u].astype(LD)
        self.z = q[:, :2] / q[:, 2:3]
        self.n, self.m, self.cd, self.mu, self.loss, self.a = n, m, (3 if fix_rotations else 6), LD(mu), loss, a
        cd = self.cd
        rot, t = np.asarray(rot, dtype=LD), np.asarray(t, dtype=LD)
        self.Rcw = np.stack([rot[:, 3 * i:3 * i + 3].T for i in range(n)])
        self.tcw = -np.einsum("iab,bi->ia", self.Rcw, t)
        self.P = np.asarray(P, dtype=LD).T.copy()
        self.n_used = int(u.sum())
        self.cused = np.bincount(self.cam, minlength=n) > 0
        self.lused = np.bincount(self.lm, minlength=m) > 0
        r, Jc, JP = self.linearise(self.Rcw, self.tcw, self.P)
        s = np.sum(r * r, axis=1)
        r0, r1 = rho(loss, s, a)
        c = np.sqrt(r1)
        self.cost = LD(0.5) * np.sum(r0)
        self.r, self.Jc, self.JP = c[:, None] * r, c[:, None, None] * Jc, c[:, None, None] * JP     # the corrected residuals and Jacobians
        k = r.shape[0]
        self.V = np.zeros((m, 3, 3), dtype=LD); self.g_l = np.zeros((m, 3), dtype=LD)
        U = np.zeros((n, cd, cd), dtype=LD); g_c = np.zeros((n, cd), dtype=LD)
        np.add.at(self.V, self.lm, np.einsum("kra,krb->kab", self.JP, self.JP))
        np.add.at(self.g_l, self.lm, np.einsum("kra,kr->ka", self.JP, self.r))
        np.add.at(U, self.cam, np.einsum("kra,krb->kab", self.Jc, self.Jc))
        np.add.at(g_c, self.cam, np.einsum("kra,kr->ka", self.Jc, self.r))
        self.g_c = g_c
        self.gmax = max(np.abs(g_c).max(initial=0), np.abs(self.g_l).max(initial=0))
        i3, ic = np.arange(3), np.arange(cd)
        self.DV = clipd(self.V[:, i3, i3]); self.DU = clipd(U[:, ic, ic])
        Vs = self.V.copy(); Vs[:, i3, i3] += self.mu * self.DV
        self.Vinv = gj_inverse(Vs)
        self.Ustar = U.copy(); self.Ustar[:, ic, ic] += self.mu * self.DU
        # W_l: the cd n x 3 block column of landmark l, every observation of a (camera, landmark) pair added
        self.Wobs = np.einsum("kra,krb->kab", self.Jc, self.JP)
        S = np.zeros((cd * n, cd * n), dtype=LD)
        for i in range(n):
            S[cd * i:cd * i + cd, cd * i:cd * i + cd] = self.Ustar[i]
        b = -g_c.reshape(-1).copy()
        by_lm = [[] for _ in range(m)]
        for e in range(k):
            by_lm[self.lm[e]].append(e)
        for l in range(m):
            if not by_lm[l]:
                continue
            Wl = {}
            for e in by_lm[l]:
                Wl[self.cam[e]] = Wl.get(self.cam[e], 0) + self.Wobs[e]
            cams = sorted(Wl)
            Wd = np.concatenate([Wl[i] for i in cams], axis=0)                    # (cd |cams|) x 3
            idx = (cd * np.array(cams)[:, None] + ic[None, :]).reshape(-1)
            WV = Wd @ self.Vinv[l]
            S[np.ix_(idx, idx)] -= WV @ Wd.T
            b[idx] += WV @ self.g_l[l]
        self.S, self.b = S, b
        self.Sinv = gj_inverse(np.stack([S[cd * i:cd * i + cd, cd * i:cd * i + cd] for i in range(n)]))

    def linearise(self, Rcw, tcw, P):
        """(r k x 2, J_c k x 2 x cd, J_P k x 2 x 3) of the used observations: r = pi(Rcw P + tcw) - z, pi(X) = (X0, X1) / X2; tangent
        coordinates X = Exp(dtheta) (Rcw P) + tcw + dt"""
        R = Rcw[self.cam]
        Y = np.einsum("kab,kb->ka", R, P[self.lm])
        X = Y + tcw[self.cam]
        iz = 1 / X[:, 2]
        uu = X[:, :2] * iz[:, None]
        d = np.zeros((X.shape[0], 2, 3), dtype=LD)
        d[:, 0, 0] = iz; d[:, 1, 1] = iz; d[:, 0, 2] = -uu[:, 0] * iz; d[:, 1, 2] = -uu[:, 1] * iz
        JP = d @ R
        Jc = np.concatenate([-(d @ skew(Y)), d], axis=2) if self.cd == 6 else d
        return uu - self.z, Jc, JP

    def cost_at(self, Rcw, tcw, P):
        r, _, _ = self.linearise(Rcw, tcw, P)
        return LD(0.5) * np.sum(rho(self.loss, np.sum(r * r, axis=1), self.a)[0])

    def vinv6(self):
        return np.stack([self.Vinv[:, 0, 0], self.Vinv[:, 0, 1], self.Vinv[:, 0, 2], self.Vinv[:, 1, 1], self.Vinv[:, 1, 2], self.Vinv[:, 2, 2]], axis=1)

    def back_substitute(self, dc):
        """dP = -V*^-1 (g_l + W^T dc), 0 for a landmark without a used observation"""
        dc = np.asarray(dc, dtype=LD).reshape(self.n, self.cd)
        acc = self.g_l.copy()
        np.add.at(acc, self.lm, np.einsum("kab,ka->kb", self.Wobs, dc[self.cam]))
        dP = -np.einsum("lab,lb->la", self.Vinv, acc)
        dP[~self.lused] = 0
        return dP

    def candidate(self, dc):
        """dict: dP, Rcw1, tcw1, rot1, t1 (the caller's layouts), P1, cost1, model, step2, x2 (cameras, landmarks)"""
        n, cd = self.n, self.cd
        dc = np.asarray(dc, dtype=LD).reshape(n, cd)
        dP = self.back_substitute(dc)
        cu, lu = self.cused, self.lused
        R1, t1, P1 = self.Rcw.copy(), self.tcw.copy(), self.P.copy()
        if cd == 6:
            R1[cu] = expmap(dc[cu, :3]) @ self.Rcw[cu]
        t1[cu] = self.tcw[cu] + dc[cu, cd - 3:]
        P1[lu] = self.P[lu] + dP[lu]
        Jd = np.einsum("kra,ka->kr", self.Jc, dc[self.cam]) + np.einsum("kra,ka->kr", self.JP, dP[self.lm])
        model = np.sum(self.r * Jd) + LD(0.5) * np.sum(Jd * Jd)
        rot1 = np.concatenate([R1[i].T for i in range(n)], axis=1)
        c1 = -np.einsum("iba,ib->ai", R1, t1)
        return dict(dP=dP, Rcw1=R1, tcw1=t1, rot1=rot1, t1=c1, P1=P1, cost1=self.cost_at(R1, t1, P1), model=model,
                    step2=(np.sum(dc[cu] ** 2), np.sum(dP[lu] ** 2)),
                    x2=((cu.sum() if cd == 6 else 0) + np.sum(self.tcw[cu] ** 2), np.sum(self.P[lu] ** 2)))

    # ---- preconditioners.  order: the members in plan order (xm_ba_aggregate_plan); blocks = runs of 16, a last run of one member joins
    # its predecessor in the coarse space
    def coarse_ranges(self, nmem):
        nagg = (nmem + AGG_CAMS - 1) // AGG_CAMS
        ncoarse = nagg - 1 if (nagg > 1 and nmem - (nagg - 1) * AGG_CAMS < 2) else nagg
        return [(a * AGG_CAMS, nmem if a == ncoarse - 1 else (a + 1) * AGG_CAMS) for a in range(ncoarse)]

    def block_inverse(self, order):
        """blockdiag(S_aa)^-1 as a dense matrix, zero on the cameras that are no members"""
        cd = self.cd
        M = np.zeros_like(self.S)
        for k0 in range(0, len(order), AGG_CAMS):
            idx = (cd * np.asarray(order[k0:k0 + AGG_CAMS])[:, None] + np.arange(cd)[None, :]).reshape(-1)
            M[np.ix_(idx, idx)] = gj_inverse(self.S[np.ix_(idx, idx)])
        return M

    def jacobi_inverse(self):
        cd = self.cd
        M = np.zeros_like(self.S)
        for i in range(self.n):
            M[cd * i:cd * i + cd, cd * i:cd * i + cd] = self.Sinv[i]
        return M

    def rigid_basis(self, order):
        """(P cd n x NC ncoarse, dropped): per coarse aggregate the first-order effect on (dtheta_i, dtcw_i) of the world motion
        X -> X + w x (X - c) + v + s (X - c) about the centroid c of the members' centres C_i = -Rcw_i^T tcw_i (xm_amd.h).  The world turns
        by I + [w]x, so the camera's orientation becomes Rcw (I - [w]x) = Exp(dtheta) Rcw: dtheta = -Rcw w.  Its centre moves by
        dC = w x (C - c) + v + s (C - c), and tcw' = -Rcw (I - [w]x) (C + dC) gives, to first order,
        dtcw = Rcw ([C - c]x - [C]x) w - Rcw v - s Rcw (C - c).  Columns (w, v, s), or (v, s) of the dtcw rows with fixed rotations, scaled
        to unit norm; a column of norm 0 stays zero and is listed"""
        n, cd = self.n, self.cd
        nc = 7 if cd == 6 else 4
        C = -np.einsum("iba,ib->ia", self.Rcw, self.tcw)
        ranges = self.coarse_ranges(len(order))
        Pm = np.zeros((cd * n, nc * len(ranges)), dtype=LD)
        dropped = []
        for a, (k0, k1) in enumerate(ranges):
            mem = np.asarray(order[k0:k1])
            c = np.sum(C[mem], axis=0) / LD(len(mem))
            for i in mem:
                R, d = self.Rcw[i], C[i] - c
                blk = np.zeros((cd, nc), dtype=LD)
                if cd == 6:
                    blk[:3, :3] = -R
                    blk[3:, :3] = R @ (skew(d) - skew(C[i]))
                blk[cd - 3:, nc - 4:nc - 1] = -R
                blk[cd - 3:, nc - 1] = -R @ d
                Pm[cd * i:cd * i + cd, nc * a:nc * a + nc] = blk
            for q in range(nc * a, nc * a + nc):
                nq = np.sqrt(np.sum(Pm[:, q] ** 2))
                if nq > 0:
                    Pm[:, q] /= nq
                else:
                    dropped.append(q)
        return Pm, dropped

    def coarse_operator(self, Pm, dropped=()):
        Ac = Pm.T @ self.S @ Pm
        for q in dropped:
            Ac[q, :] = 0; Ac[:, q] = 0; Ac[q, q] = 1
        return Ac

    def precond(self, kind, order):
        """M^-1 as a dense matrix for kind in jacobi / blocks / two_level"""
        if kind == "jacobi":
            return self.jacobi_inverse()
        M = self.block_inverse(order)
        if kind == "two_level":
            Pm, dropped = self.rigid_basis(order)
            M = M + Pm @ gj_inverse(self.coarse_operator(Pm, dropped)) @ Pm.T
        return M
