"""numpy / scipy.sparse restatement of the bundle adjustment with one focal scale per GROUP of cameras behind
xm_ctx_bundle_adjust_focal_groups (include/xm_amd.h): r_e = g_{group_of[i]} pi(Rcw_i P_l + tcw_i) - z_e.  J_7 is the Jacobian of
xm_ba_focal_numpy.FocalProblem at the groups' scales copied to the members; with E the 0/1 matrix that copies a group's unknown into the
focal column of each member, J_shared = J_7 E.  Tangent order: cp = cd - 1 columns per camera (6, or 3 with fixed rotations), then the G
focal entries, then 3 per landmark.  The damping is Ceres's rule on the shared parameter: D = clip(diag(J_shared^T J_shared)), whose focal
entries are D_c = clip(sum_{i in c} (J_7^T J_7)_ff,i).  A group is held when focal_free[c] = 0 or none of its members has a used
observation (an empty group among them): zero column, step exactly 0.  The LM rules are xm_ba_focal_numpy.lm's.  Exact linear solves, or
the restated PCG (xm_ba_precond_numpy.pcg) on the reduced camera system with M = blockdiag(the cameras' pose blocks of S_7, F): for G <=
EXACT = 16 groups F is the exact focal block S[focal, focal]; for more, diag F with F_c = sum_{i in c} S_7,ii[f, f] (the members' focal
diagonal undamped) + mu D_c (exact_block=False: that rule at every G, the ablation).

Layouts are the library's (xm_ba_numpy.py); focal, focal_free: G."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import xm_ba_focal_numpy as bf
import xm_ba_numpy as ba
import xm_ba_precond_numpy as bp


EXACT = 16                                                 # XM_BA_FOCAL_GROUPS_EXACT


def expand_matrix(n, G, group_of, cd, m=0):
    """E: (cd n + 3 m) x ((cd - 1) n + G + 3 m), 0/1"""
    cp = cd - 1
    group_of = np.asarray(group_of, dtype=np.int64)
    i = np.arange(n)
    rows = np.concatenate([(cd * i[:, None] + np.arange(cp)[None, :]).reshape(-1), cd * i + cp, cd * n + np.arange(3 * m)])
    cols = np.concatenate([(cp * i[:, None] + np.arange(cp)[None, :]).reshape(-1), cp * n + group_of, cp * n + G + np.arange(3 * m)])
    return sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(cd * n + 3 * m, cp * n + G + 3 * m))


class GroupProblem(bf.FocalProblem):
    """FocalProblem with the focal scales shared by groups.  free: G booleans (None = all)"""

    def __init__(self, cam, lm, p, w, n, m, group_of, G, fix_rotations=False, loss="trivial", a=0.0, free=None):
        self.group_of = np.asarray(group_of, dtype=np.int64)
        self.G = int(G)
        self.gfree = np.ones(self.G, dtype=bool) if free is None else np.asarray(free).astype(bool)
        super().__init__(cam, lm, p, w, n, m, fix_rotations, loss, a, self.gfree[self.group_of])
        self.cp = self.cd0
        self.E = expand_matrix(n, self.G, self.group_of, self.cd, m)
        self.gused = np.bincount(self.group_of[self.cused], minlength=self.G) > 0
        self.ncam = self.cp * n + self.G                    # columns of the reduced camera system

    def moving_groups(self):
        return self.gfree & self.gused

    def shared(self, Rcw, tcw, P, gg):
        """(F, r~, J~_shared, J~_7) at the groups' scales gg"""
        F, r, J7 = self.corrected(Rcw, tcw, P, np.asarray(gg)[self.group_of])
        return F, r, (J7 @ self.E).tocsr(), J7

    def cost_g(self, Rcw, tcw, P, gg):
        return self.cost(Rcw, tcw, P, np.asarray(gg)[self.group_of])

    def plus_g(self, Rcw, tcw, P, gg, d):
        cp, n, G = self.cp, self.n, self.G
        dc = d[:cp * n].reshape(n, cp)
        dg = d[cp * n:cp * n + G]
        dP = d[cp * n + G:].reshape(self.m, 3)
        Rn, tn, Pn, gn = Rcw.copy(), tcw.copy(), P.copy(), np.array(gg, dtype=np.float64)
        c, lu, mv = self.cused, self.lused, self.moving_groups()
        if cp == 6:
            Rn[c] = ba.expmap(dc[c, :3]) @ Rcw[c]
        tn[c] = tcw[c] + dc[c, cp - 3:cp]
        gn[mv] = gn[mv] + dg[mv]
        Pn[lu] = P[lu] + dP[lu]
        return Rn, tn, Pn, gn

    def x2_g(self, tcw, P, gg):
        """|x|^2 as (cameras and groups, landmarks): g_c^2 once per moving group"""
        c = self.cused
        return np.array([(c.sum() if self.cp == 6 else 0) + np.sum(tcw[c] ** 2) + np.sum(np.asarray(gg)[self.moving_groups()] ** 2),
                         np.sum(P[self.lused] ** 2)])

    def step2_g(self, d):
        cp, n, G = self.cp, self.n, self.G
        return np.array([np.sum(d[:cp * n].reshape(n, cp)[self.cused] ** 2) + np.sum(d[cp * n:cp * n + G][self.moving_groups()] ** 2),
                         np.sum(d[cp * n + G:].reshape(self.m, 3)[self.lused] ** 2)])


def landmark_inverse(V, m):
    """blockdiag(V)^-1 of the landmark corner (sparse, 3 x 3 blocks); a landmark without an entry gets the identity"""
    V = V.tocoo()
    Vd = np.zeros((m, 3, 3))
    Vd[V.row // 3, V.row % 3, V.col % 3] = V.data
    Vd[~(np.abs(Vd).sum(axis=(1, 2)) > 0)] = np.eye(3)
    Vi = np.linalg.inv(Vd)
    return sp.block_diag(list(Vi), format="csr"), Vi


def reduced(pr, J, J7, g, mu, damage=(), exact_block=True):
    """the reduced camera system of the shared problem at damping mu and the pieces of its preconditioner: dict S (sparse, ncam square), b,
    Vinv, W, D (the whole damping vector), Dc (G), S7 (the cd n reduced system of J_7 with the members' focal diagonal UNdamped), F (G),
    Minv (sparse: the inverted pose blocks of S7 and 1 / F).  damage: "member_clamp", a deliberate fault for the test that the stage bound
    bites -- D_c as the sum of the members' clamped terms, which is what the per-image camera pass would leave behind"""
    n, m, cd, cp, G, nc = pr.n, pr.m, pr.cd, pr.cp, pr.G, pr.ncam
    H = (J.T @ J).tocsc()
    D = np.clip(H.diagonal(), 1e-6, 1e32)
    if "member_clamp" in damage:
        uff = (J7.T @ J7).diagonal()[cd * np.arange(n) + cp]
        D[cp * n:nc] = np.maximum(np.bincount(pr.group_of, weights=np.clip(uff, 1e-6, 1e32), minlength=G), 1e-6)   # (an empty group: 1e-6)
    Hs = (H + sp.diags(mu * D)).tocsr()
    U, W, V = Hs[:nc, :nc], Hs[:nc, nc:], Hs[nc:, nc:]
    Vinv, Vi = landmark_inverse(V, m)
    S = (U - W @ Vinv @ W.T).tocsr()
    b = -g[:nc] + W @ (Vinv @ g[nc:])
    # the 7-column system: the damping of the shared problem on the pose and landmark columns, none on the members' focal columns
    H7 = (J7.T @ J7).tocsc()
    d7 = np.zeros(cd * n + 3 * m)
    pose = (cd * np.arange(n)[:, None] + np.arange(cp)[None, :]).reshape(-1)
    d7[pose] = D[:cp * n]
    d7[cd * n:] = D[nc:]
    H7 = (H7 + sp.diags(mu * d7)).tocsr()
    n7 = cd * n
    W7 = H7[:n7, n7:]
    S7 = (H7[:n7, :n7] - W7 @ Vinv @ W7.T).tocsr()
    Dc = D[cp * n:nc]
    fidx = cd * np.arange(n) + cp
    F = np.bincount(pr.group_of, weights=S7.diagonal()[fidx], minlength=G) + mu * Dc
    S7d = S7.toarray() if n7 <= 4096 else None
    blocks = []
    for i in range(n):
        blk = S7d[cd * i:cd * i + cp, cd * i:cd * i + cp] if S7d is not None else S7[cd * i:cd * i + cp, cd * i:cd * i + cp].toarray()
        blocks.append(np.linalg.inv(blk))
    if exact_block and G <= EXACT:
        F = S[cp * n:, cp * n:].toarray()
        Minv = sp.block_diag(blocks + [np.linalg.inv(F)], format="csr")
    else:
        Minv = sp.block_diag(blocks + [sp.diags(1.0 / F)], format="csr")
    return dict(S=S, b=b, Vinv=Vinv, Vi=Vi, W=W, D=D, Dc=Dc, S7=S7, F=F, Minv=Minv)


def lm(cam, lm_, p, w, rot, t, P, group_of, focal=None, focal_free=None, fix_rotations=False, loss="trivial", a=0.0, max_iters=1000,
       function_tol=1e-6, gradient_tol=1e-10, parameter_tol=1e-8, eta=None, exact_block=True):
    """the LM of xm_ctx_bundle_adjust_focal_groups (the rules of xm_ba_focal_numpy.lm).  focal: G (None: ones; then G = max(group_of) + 1).
    eta None: exact solves of the damped normal equations; else the reduced camera system by PCG to eta with the M above.  Returns
    (rot, t, P, focal, info) as xm_ba_focal_numpy.lm"""
    n, m = t.shape[1], P.shape[1]
    G = int(np.max(group_of)) + 1 if focal is None else len(focal)
    pr = GroupProblem(cam, lm_, p, w, n, m, group_of, G, fix_rotations, loss, a, focal_free)
    nc = pr.ncam
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    X = P.T.copy()
    g0 = np.ones(G) if focal is None else np.array(focal, dtype=np.float64)
    gf = g0.copy()
    mv = pr.moving_groups()
    radius, nu = 1e4, 2.0
    F, r, J, J7 = pr.shared(Rcw, tcw, X, gf)
    g = J.T @ r
    info = dict(initial_cost=F, n_used=pr.n_used)
    trace, invalid = [], []
    iters = accepted = pcg_iters = 0
    min_focal = float(gf[mv].min(initial=np.inf))
    status = "no_convergence"
    while True:
        if np.max(np.abs(g), initial=0.0) <= gradient_tol:
            status = "gradient_tolerance"; break
        if iters >= max_iters:
            status = "max_iterations"; break
        mu = 1.0 / radius
        if eta is None:
            A = (J.T @ J).tocsc()
            D = np.clip(A.diagonal(), 1e-6, 1e32)
            d = spla.spsolve(A + sp.diags(mu * D).tocsc(), -g)
        else:
            q = reduced(pr, J, J7, g, mu, exact_block=exact_block)
            dc, it, _ = bp.pcg(q["S"], q["b"], lambda v: q["Minv"] @ v, eta)
            pcg_iters += it
            d = np.concatenate([dc, -(q["Vinv"] @ (g[nc:] + q["W"].T @ dc))])
        Jd = J @ d
        model_dec = -(float(r @ Jd) + 0.5 * float(Jd @ Jd))
        Rn, tn, Xn, gn = pr.plus_g(Rcw, tcw, X, gf, d)
        Fn = pr.cost_g(Rn, tn, Xn, gn)
        iters += 1
        positive = bool((gn[mv] > 0).all())
        if not positive:
            invalid.append(iters - 1)
        valid = positive and np.isfinite(Fn) and model_dec > 0
        rho = (F - Fn) / model_dec if valid else -1.0
        acc = bool(valid and rho > 1e-3)
        trace.append((F, Fn, mu, float(acc)))
        if positive and np.sqrt(pr.step2_g(d).sum()) <= parameter_tol * (np.sqrt(pr.x2_g(tcw, X, gf).sum()) + parameter_tol):
            status = "parameter_tolerance"; break
        if acc:
            accepted += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            nu = 2.0
            Rcw, tcw, X, gf = Rn, tn, Xn, gn
            min_focal = min(min_focal, float(gf[mv].min(initial=np.inf)))
            Fold = F
            F, r, J, J7 = pr.shared(Rcw, tcw, X, gf)
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
    gf[~mv] = g0[~mv]                                      # never moved: the caller's bits
    info.update(status=ba.STATUS[status], iters=iters, accepted=accepted, final_cost=F, gradient_max=float(np.max(np.abs(g), initial=0.0)),
                trace=np.array(trace).reshape(-1, 4), min_focal=min_focal, invalid=len(invalid), invalid_at=invalid, pcg_iters=pcg_iters)
    return rot_o, t_o, P_o, gf, info


def stages(S, rot, t, P, group_of, focal, free, mu, fix=False, loss="trivial", a=0.0, X=None, dc=None, perm=None, damage=()):
    """the quantities of one linearisation that xm_ctx_ba_probe_focal_groups returns, in its layouts (vectors: cp n + G)"""
    n, m = S["n"], S["m"]
    cam, lm_, p, w = (np.asarray(S[k]) for k in ("cam", "lm", "p", "w"))
    if perm is not None:
        cam, lm_, p, w = cam[perm], lm_[perm], p[perm], w[perm]
    G = len(focal)
    pr = GroupProblem(cam, lm_, p, w, n, m, group_of, G, fix, loss, a, free)
    nc = pr.ncam
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    Pw = np.asarray(P, dtype=np.float64).T.copy()
    gg = np.asarray(focal, dtype=np.float64)
    F, r, J, J7 = pr.shared(Rcw, tcw, Pw, gg)
    g = J.T @ r
    q = reduced(pr, J, J7, g, mu, damage)
    out = dict(cost=F, gmax=float(np.abs(g).max(initial=0.0)), b=q["b"], D=q["Dc"], F=q["F"], g_l=g[nc:].reshape(m, 3), S=np.tril(q["S"].toarray()))
    if X is not None:
        out["SX"] = q["S"] @ X
        out["MX"] = q["Minv"] @ X
    if dc is not None:
        dc = np.asarray(dc, dtype=np.float64).reshape(-1)
        dP = -(q["Vinv"] @ (g[nc:] + q["W"].T @ dc))
        dP.reshape(m, 3)[~pr.lused] = 0.0
        d = np.concatenate([dc, dP])
        Jd = J @ d
        Rn, tn, Pn, gn = pr.plus_g(Rcw, tcw, Pw, gg, d)
        rot1, t1 = ba.to_camera_to_world(Rn, tn)
        out.update(dP=dP.reshape(m, 3), rot1=rot1, t1=t1, p1=Pn.T, focal1=gn, cost1=pr.cost_g(Rn, tn, Pn, gn),
                   model=float(r @ Jd) + 0.5 * float(Jd @ Jd), step2=pr.step2_g(d), x2=pr.x2_g(tcw, Pw, gg))
    return out
