"""numpy.longdouble statement of one linearisation of xm_ctx_bundle_adjust_focal_groups, built on xm_ba_focal_exact.FocalExact at the
groups' scales copied to the members: S_7, b_7 are its reduced camera system with the damping of the members' focal diagonal taken out
again; with E the 0/1 expansion, S = E^T S_7 E + mu diag(0, D_c), b = E^T b_7, D_c = clip(sum_{i in c} U_ff,i).  Vectors: cp = cd - 1
entries per camera, then the G focal entries.  The judge of tests/test_gpu_ba_groups_stages.py and of xm_ba_groups_numpy.py."""
import numpy as np

import xm_ba_exact as ex
import xm_ba_focal_exact as fx

LD = ex.LD


class GroupsExact:
    """attributes (longdouble): E7 (the FocalExact), idx (cd n: the shared index of every entry of the 7-column space), D (G), S, b, gmax,
    F (G x G for G <= 16, else G), Pinv (n x cp x cp: the inverted pose blocks), cost, moving (G); expand(v) = E v, contract(v) = E^T v, minv(X) = M^-1 X"""

    def __init__(self, cam, lm, p, w, n, m, rot, t, P, group_of, focal, mu, fix_rotations=False, loss="trivial", a=0.0, free=None):
        self.group_of = np.asarray(group_of, dtype=np.int64)
        self.g = np.asarray(focal, dtype=LD)
        G = self.G = self.g.size
        self.gfree = np.ones(G, dtype=bool) if free is None else np.asarray(free).astype(bool)
        E7 = self.E7 = fx.FocalExact(cam, lm, p, w, n, m, rot, t, P, self.g[self.group_of], mu, fix_rotations, loss, a, self.gfree[self.group_of])
        cd = self.cd = E7.cd
        cp = self.cp = cd - 1
        self.n, self.m, self.mu = n, m, LD(mu)
        idx = np.empty((n, cd), dtype=np.int64)
        idx[:, :cp] = cp * np.arange(n)[:, None] + np.arange(cp)[None, :]
        idx[:, cp] = cp * n + self.group_of
        self.idx = idx = idx.reshape(-1)
        self.ns = cp * n + G
        Uff = np.zeros(n, dtype=LD)
        np.add.at(Uff, E7.cam, np.sum(E7.Jc[:, :, cp] ** 2, axis=1))
        Dsum = np.zeros(G, dtype=LD)
        np.add.at(Dsum, self.group_of, Uff)
        self.D = ex.clipd(Dsum)
        fidx = cd * np.arange(n) + cp
        S7 = E7.S                                           # changed in place: the members' focal diagonal undamped
        S7[fidx, fidx] -= self.mu * E7.DU[:, cp]
        S = np.zeros((self.ns, self.ns), dtype=LD)
        np.add.at(S, (idx[:, None], idx[None, :]), S7)
        gi = cp * n + np.arange(G)
        S[gi, gi] += self.mu * self.D
        self.S, self.b = S, self.contract(E7.b)
        gc = self.contract(E7.g_c.reshape(-1))
        self.gmax = max(np.abs(gc).max(initial=0), np.abs(E7.g_l).max(initial=0))
        self.cost = E7.cost
        self.gused = np.bincount(self.group_of[E7.cused], minlength=G) > 0
        self.moving = self.gfree & self.gused
        Fs = np.zeros(G, dtype=LD)
        np.add.at(Fs, self.group_of, S7[fidx, fidx])
        self.F = S[np.ix_(gi, gi)].copy() if G <= 16 else Fs + self.mu * self.D      # XM_BA_FOCAL_GROUPS_EXACT: the exact block, else diag
        self.Finv = ex.gj_inverse(self.F) if G <= 16 else None
        self.Pinv = ex.gj_inverse(np.stack([S7[cd * i:cd * i + cp, cd * i:cd * i + cp] for i in range(n)]))

    def contract(self, v):
        out = np.zeros((self.ns,) + np.shape(v)[1:], dtype=LD)
        np.add.at(out, self.idx, np.asarray(v, dtype=LD))
        return out

    def expand(self, v):
        return np.asarray(v, dtype=LD)[self.idx]

    def minv(self, X):
        X = np.asarray(X, dtype=LD).reshape(self.ns, -1)
        n, cp = self.n, self.cp
        out = np.empty_like(X)
        out[:cp * n] = np.einsum("iab,ibk->iak", self.Pinv, X[:cp * n].reshape(n, cp, -1)).reshape(cp * n, -1)
        out[cp * n:] = X[cp * n:] / self.F[:, None] if self.Finv is None else self.Finv @ X[cp * n:]
        return out

    def candidate(self, dcs):
        """dcs: the step in the shared space (cp n + G)"""
        E7, n, cp, G = self.E7, self.n, self.cp, self.G
        dcs = np.asarray(dcs, dtype=LD).reshape(-1)
        dc7 = self.expand(dcs).reshape(n, self.cd)
        c = E7.candidate(dc7)                               # dP, the poses and the model are those of the expanded step
        mv, cu, lu = self.moving, E7.cused, E7.lused
        g1 = self.g.copy()
        g1[mv] = self.g[mv] + dcs[cp * n:][mv]
        cost1 = E7.cost_at(c["Rcw1"], c["tcw1"], c["P1"], g1[self.group_of])
        pose = dcs[:cp * n].reshape(n, cp)
        step2 = (np.sum(pose[cu] ** 2) + np.sum(dcs[cp * n:][mv] ** 2), np.sum(c["dP"][lu] ** 2))
        x2 = ((cu.sum() if cp == 6 else 0) + np.sum(E7.tcw[cu] ** 2) + np.sum(self.g[mv] ** 2), np.sum(E7.P[lu] ** 2))
        return dict(dP=c["dP"], rot1=c["rot1"], t1=c["t1"], P1=c["P1"], focal1=g1, cost1=cost1, model=c["model"],
                    positive=bool((g1[mv] > 0).all()), step2=step2, x2=x2)


def lm_trace(cam, lm, p, w, rot, t, P, group_of, focal, free=None, fix_rotations=False, max_iters=10):
    """the first max_iters iterations of the Levenberg-Marquardt loop in longdouble with exact solves of the shared reduced camera system:
    rows (cost, candidate cost, mu, accepted).  For choosing scenes whose accept sequence does not hang on f64 rounding"""
    n, m = np.asarray(t).shape[1], np.asarray(P).shape[1]
    rot, t, P, g = np.asarray(rot, dtype=LD), np.asarray(t, dtype=LD), np.asarray(P, dtype=LD), np.asarray(focal, dtype=LD)
    radius, nu = LD(1e4), LD(2)
    rows = []
    for _ in range(max_iters):
        mu = 1 / radius
        E = GroupsExact(cam, lm, p, w, n, m, rot, t, P, group_of, g, mu, fix_rotations, free=free)
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
            cu, lu = E.E7.cused, E.E7.lused
            rot = np.where(np.repeat(cu, 3)[None, :], c["rot1"], rot)
            t = np.where(cu[None, :], c["t1"], t)
            P = np.where(lu[None, :], c["P1"].T, P)
            g = c["focal1"]
        else:
            radius /= nu
            nu *= 2
    return np.array(rows)
