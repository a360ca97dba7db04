"""numpy / scipy.sparse restatement of xm_ctx_global_positioning_pairs (include/xm_amd.h, xm_gp.h): GLOMAP's estimators/global_positioning.cc
with its four constraint types, the down-weighting of uncalibrated cameras and the fixed-centre pass of controllers/global_mapper.cc:205-217,
on top of xm_gp_numpy.py (the ONLY_POINTS form, whose rules -- used observations, loss, bound, LM -- are kept word for word).
NOT COMPARED WITH THE REFERENCE'S COMPILED CODE (it needs Ceres, COLMAP, Eigen and glog): the citations say which line a rule comes from.

  pairs        pi, pj = image_id1, image_id2; trel = translation of cam2_from_cam1, used as given; a pair takes part when it is valid
               (.cc:152).  pi == pj or an index out of range is refused.
  residual     r_m = tau_m - sigma_m (c_j - c_i), tau_m = -R_j trel_m with R_j camera-to-world of image_id2; position1 = c_i,
               position2 = c_j (.cc:165-175, cost_function.h:15-41)
  scale        one sigma_m per participating pair, 1 at the start, >= 1e-5 (.cc:163, :177); the bound by the active-set rule of
               xm_gp_numpy.py (frozen when sigma <= 1e-5 and g_sigma > 0; candidate max(sigma + d sigma, 1e-5))
  loss         pairs: the plain loss (options_.loss_function, .cc:172).  Observations: Ceres's ScaledLoss, rho and rho' times a_e
               (.cc:201-228, :283-295): a_e = weight_scale_pt for a calibrated camera and 0.5 weight_scale_pt for an uncalibrated one;
               weight_scale_pt = reweight_scale * (participating pairs) / (ALL landmarks, tracks.size(), .cc:193) for BALANCED with at least
               one participating pair, else 1
  terms        only_points: observations; only_cameras: pairs (no observation is used); the two mixed types: both (.cc:53-60).  A type
               with pair terms and no participating pair is refused (.cc:32-36)
  used         a camera with a used observation (where observation terms exist) or a participating pair (where pair terms exist),
               .cc:108-127
  fixed        fix_centres = optimize_positions false with only_points (global_mapper.cc:209-213, .cc:341-346): the centres are constants

Unknowns x = (c: 3 per camera, P: 3 per landmark, s: 1 per used observation, sigma: 1 per participating pair), each in input order."""
import numpy as np
import scipy.sparse as sp

import xm_gp_numpy as gp

LD = gp.LD
S_MIN = gp.S_MIN
STATUS = gp.STATUS
CONSTRAINTS = ("only_points", "only_cameras", "points_and_cameras_balanced", "points_and_cameras")


class Problem(gp.Problem):
    def __init__(self, cam, lm, p, w, rot, n, m, pairs=None, constraint="only_points", calibrated=None, reweight_scale=1.0, fix_centres=False,
                 min_views=3, loss="huber", a=0.1, dtype=np.float64):
        super().__init__(cam, lm, p, w, rot, n, m, min_views, loss, a, dtype)
        if constraint not in CONSTRAINTS:
            raise ValueError("unknown constraint type")
        self.has_obs, self.has_pairs, self.fix = constraint != "only_cameras", constraint != "only_points", bool(fix_centres)
        if self.fix and constraint != "only_points":
            raise ValueError("fixed centres go with only_points")
        if not self.has_obs:                                                  # .cc:53-60: no observation is used
            self.mask = np.zeros_like(self.mask)
            self.idx = self.idx[:0]
            self.cam, self.lm, self.d, self.k = self.cam[:0], self.lm[:0], self.d[:0], 0
            self.cused, self.lused = np.zeros(n, dtype=bool), np.zeros(m, dtype=bool)
        self.npairs = 0
        self.pidx = np.zeros(0, dtype=np.int64)
        self.ci = self.cj = np.zeros(0, dtype=np.int64)
        self.tau = np.zeros((0, 3), dtype=dtype)
        if pairs is not None:
            pi, pj = np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64)
            trel = np.asarray(pairs[2], dtype=dtype).reshape(pi.size, 3)
            valid = np.ones(pi.size, dtype=bool) if len(pairs) < 4 or pairs[3] is None else np.asarray(pairs[3]).reshape(pi.size) != 0
            if np.any(pi == pj) or np.any((pi < 0) | (pi >= n) | (pj < 0) | (pj >= n)):
                raise ValueError("a pair names a camera outside [0, n) or one camera twice")
            self.npairs = pi.size
            if self.has_pairs:
                self.pidx = np.nonzero(valid)[0]                              # .cc:152
                self.ci, self.cj = pi[self.pidx], pj[self.pidx]
                R = np.stack([np.asarray(rot, dtype=dtype)[:, 3 * i:3 * i + 3] for i in range(n)])
                self.tau = -np.einsum("kab,kb->ka", R[self.cj], trel[self.pidx])   # .cc:165-168
        self.M = self.pidx.size
        if self.has_pairs and self.M == 0:
            raise ValueError("the constraint type has pair terms but no pair takes part")   # .cc:32-36
        self.weight_scale_pt = float(reweight_scale) * self.M / m if constraint == "points_and_cameras_balanced" and self.M > 0 else 1.0   # .cc:193-199
        cal = np.ones(n, dtype=bool) if calibrated is None else np.asarray(calibrated).reshape(n) != 0
        self.ae = np.where(cal[self.cam], dtype(1), dtype(0.5)) * dtype(self.weight_scale_pt)   # .cc:283-295
        self.pcused = np.zeros(n, dtype=bool)
        self.pcused[self.ci] = True; self.pcused[self.cj] = True
        self.cused = self.cused | self.pcused                                 # .cc:108-127

    def _term(self, d, v, s, ae):
        """corrected residual and Jacobian entries of r = d - s v under the loss (scaled by ae where given): the dict of
        xm_gp_numpy.Problem.blocks"""
        dt = self.dtype
        r = d - s[:, None] * v
        r0, w = gp._rho(self.loss, np.sum(r * r, axis=1), self.a, dt)
        if ae is not None:
            r0, w = ae * r0, ae * w                                           # ScaledLoss
        sw = np.sqrt(w)
        gs = -w * np.sum(r * v, axis=1)
        frozen = (s <= dt(S_MIN)) & (gs > 0)
        Js = np.where(frozen[:, None], dt(0), -sw[:, None] * v)
        return dict(F=0.5 * float(np.sum(r0)), r=sw[:, None] * r, w=w, v=v, frozen=frozen, gs=np.where(frozen, dt(0), gs), jc=sw * s, Js=Js)

    def blocks(self, c, P, s):
        return self._term(self.d, P[self.lm] - c[self.cam], s, self.ae)

    def pair_blocks(self, c, sg):
        return self._term(self.tau, c[self.cj] - c[self.ci], sg, None)

    def cost(self, c, P, s):
        r = self.residuals(c, P, s)
        return 0.5 * float(np.sum(self.ae * gp._rho(self.loss, np.sum(r * r, axis=1), self.a, self.dtype)[0]))

    def pair_cost(self, c, sg):
        r = self.tau - sg[:, None] * (c[self.cj] - c[self.ci])
        return 0.5 * float(np.sum(gp._rho(self.loss, np.sum(r * r, axis=1), self.a, self.dtype)[0]))

    def jacobian_all(self, B, Bp):
        """sparse (3k + 3M) x (3n + 3m + k + M): the observations' rows (xm_gp_numpy) over the pairs' (+jc at c_i, -jc at c_j, Js at sigma)"""
        k, M, n, m = self.k, self.M, self.n, self.m
        Jo = sp.hstack([self.jacobian(B), sp.csr_matrix((3 * k, M))]).tocsr() if k else sp.csr_matrix((0, 3 * n + 3 * m + k + M))
        if M == 0:
            return Jo
        rows = np.arange(3 * M)
        ax = np.tile(np.arange(3), M)
        e = np.repeat(np.arange(M), 3)
        jc = np.repeat(np.asarray(Bp["jc"], dtype=np.float64), 3)
        Jp = sp.csr_matrix((np.concatenate([jc, -jc, np.asarray(Bp["Js"], dtype=np.float64).reshape(-1)]),
                            (np.concatenate([rows, rows, rows]), np.concatenate([3 * self.ci[e] + ax, 3 * self.cj[e] + ax, 3 * n + 3 * m + k + e]))),
                           shape=(3 * M, 3 * n + 3 * m + k + M))
        return sp.vstack([Jo, Jp]).tocsr()

    def x_norm2(self, c, P, s, sg):
        cc = 0.0 if self.fix else float(np.sum(c[self.cused] ** 2))
        return cc + float(np.sum(P[self.lused] ** 2) + np.sum(s ** 2) + np.sum(sg ** 2))


def lm(cam, lm_, p, w, rot, t, P, pairs=None, constraint="only_points", calibrated=None, reweight_scale=1.0, fix_centres=False, min_views=3,
       loss="huber", a=0.1, max_iters=100, function_tol=1e-5, gradient_tol=1e-10, parameter_tol=1e-8):
    """xm_gp_numpy.lm over (c, P, s, sigma): the same rules with exact solves of the damped normal equations; with fixed centres the
    cameras' columns are left out.  info also has sigma (npairs, -1 = takes no part), pairs_used, weight_scale_pt"""
    n, m = t.shape[1], P.shape[1]
    pr = Problem(cam, lm_, p, w, rot, n, m, pairs, constraint, calibrated, reweight_scale, fix_centres, min_views, loss, a)
    c, X, s, sg = t.T.copy(), P.T.copy(), np.ones(pr.k), np.ones(pr.M)       # .cc:273, :163
    c0 = 3 * n if pr.fix else 0                                               # the first free column

    def linearise(c, X, s, sg):
        B, Bp = pr.blocks(c, X, s), pr.pair_blocks(c, sg)
        J = pr.jacobian_all(B, Bp)[:, c0:]
        return J, np.concatenate([B["r"].reshape(-1), Bp["r"].reshape(-1)]), B["F"] + Bp["F"]

    def plus(c, X, s, sg, d):
        d = np.concatenate([np.zeros(c0), d])
        dc, dP, rest = d[:3 * n].reshape(n, 3), d[3 * n:3 * n + 3 * m].reshape(m, 3), d[3 * n + 3 * m:]
        return c + dc, X + dP, np.maximum(s + rest[:pr.k], S_MIN), np.maximum(sg + rest[pr.k:], S_MIN)

    radius, nu = 1e4, 2.0
    J, r, F = linearise(c, X, s, sg)
    g = J.T @ r
    info = dict(initial_cost=F, n_used=pr.k, pairs_used=pr.M, weight_scale_pt=pr.weight_scale_pt)
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
        d = gp.solve_damped(A + sp.diags(mu * D).tocsc(), -g)
        Jd = J @ d
        model_dec = -(float(r @ Jd) + 0.5 * float(Jd @ Jd))
        cn, Xn, sn, sgn = plus(c, X, s, sg, d)
        Fn = pr.cost(cn, Xn, sn) + pr.pair_cost(cn, sgn)
        iters += 1
        step = float(np.sqrt(np.sum(d * d)))
        valid = np.isfinite(Fn) and model_dec > 0
        rho = (F - Fn) / model_dec if valid else -1.0
        acc = bool(valid and rho > 1e-3)
        trace.append((F, Fn, mu, float(acc)))
        if step <= parameter_tol * (np.sqrt(pr.x_norm2(c, X, s, sg)) + parameter_tol):
            status = "parameter_tolerance"; break
        if acc:
            accepted += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            nu = 2.0
            c, X, s, sg = cn, Xn, sn, sgn
            Fold, F = F, Fn
            J, r, _ = linearise(c, X, s, sg)
            g = J.T @ r
            if abs(Fold - Fn) <= function_tol * Fold:
                status = "function_tolerance"; break
        else:
            radius /= nu
            nu *= 2.0
            if radius < 1e-32:
                status = "no_progress"; break
    t_o, P_o = t.copy(), P.copy()
    if not pr.fix:
        t_o[:, pr.cused] = c.T[:, pr.cused]
    P_o[:, pr.lused] = X.T[:, pr.lused]
    scales = np.full(pr.nobs, -1.0)
    scales[pr.idx] = s
    sigma = np.full(pr.npairs, -1.0)
    sigma[pr.pidx] = sg
    info.update(status=STATUS[status], iters=iters, accepted=accepted, final_cost=F, gradient_max=float(np.max(np.abs(g), initial=0.0)),
                scales=scales, sigma=sigma, trace=np.array(trace).reshape(-1, 4))
    return t_o, P_o, info


def _eliminate(Bk, mu, dt):
    """the closed-form elimination of one scale per term (include/xm_amd.h): M (k x 3 x 3), q (k x 3), h*, y = J_c^T J_s, g_s"""
    jc, Js, r = Bk["jc"], Bk["Js"], Bk["r"]
    h = np.sum(Js * Js, axis=1)
    hs = h + mu * gp._clip(h, dt)
    gs = np.sum(Js * r, axis=1)
    y = jc[:, None] * Js
    M = (jc * jc)[:, None, None] * np.eye(3, dtype=dt) - y[:, :, None] * y[:, None, :] / hs[:, None, None]
    q = jc[:, None] * r - y * (gs / hs)[:, None]
    return M, q, hs, y, gs


def _sym6(M):
    return M[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]


def stages(pr, t, P, s_all, sigma_all, mu, X=None, dc=None):
    """one linearisation at (t, P, s_all, sigma_all) with the damping mu, by the formulas of the contract: what xm_ctx_gp_probe_pairs
    returns, under the keys of Context.gp_probe_pairs, in pr.dtype.  The observation terms' scalars (cost, cost1, model, step2, x2) and
    the pairs' (pcost, pcost1, pmodel, pstep2, px2) are kept apart as the probe keeps them; S is the dense reduced camera matrix.  With
    fixed centres there is no camera system (no ustar, sinv, b, S) and dc is 0."""
    dt = pr.dtype
    n, m, k, Mp_ = pr.n, pr.m, pr.k, pr.M
    c, Xp = np.asarray(t, dtype=dt).T.copy(), np.asarray(P, dtype=dt).T.copy()
    s = np.asarray(s_all, dtype=dt)[pr.idx]
    sg = (np.ones(pr.npairs, dtype=dt) if sigma_all is None else np.asarray(sigma_all, dtype=dt))[pr.pidx]
    B, Bp = pr.blocks(c, Xp, s), pr.pair_blocks(c, sg)
    mu = dt(mu)
    I3 = np.eye(3, dtype=dt)
    M, q, hs, y, gs = _eliminate(B, mu, dt)
    Mq, qq, hsp, yp, gsp = _eliminate(Bp, mu, dt)
    jc, jcp = B["jc"], Bp["jc"]
    # damping of c and P: the diagonal of the FULL J^T J, one clamp of the sum over observations and pairs
    dcam, dlm = np.zeros(n, dtype=dt), np.zeros(m, dtype=dt)
    np.add.at(dcam, pr.cam, jc * jc); np.add.at(dcam, pr.ci, jcp * jcp); np.add.at(dcam, pr.cj, jcp * jcp)
    np.add.at(dlm, pr.lm, jc * jc)
    U, V = np.zeros((n, 3, 3), dtype=dt), np.zeros((m, 3, 3), dtype=dt)
    gc, gl = np.zeros((n, 3), dtype=dt), np.zeros((m, 3), dtype=dt)
    gfull, gPfull = np.zeros((n, 3), dtype=dt), np.zeros((m, 3), dtype=dt)
    np.add.at(U, pr.cam, M); np.add.at(V, pr.lm, M)
    np.add.at(U, pr.ci, Mq); np.add.at(U, pr.cj, Mq)                          # S_ii += M_m, S_jj += M_m
    np.add.at(gc, pr.cam, q); np.add.at(gl, pr.lm, -q)
    np.add.at(gc, pr.ci, qq); np.add.at(gc, pr.cj, -qq)                       # i: the camera's sign, j: the point's
    np.add.at(gfull, pr.cam, jc[:, None] * B["r"]); np.add.at(gPfull, pr.lm, -jc[:, None] * B["r"])
    np.add.at(gfull, pr.ci, jcp[:, None] * Bp["r"]); np.add.at(gfull, pr.cj, -jcp[:, None] * Bp["r"])
    Us = U + (mu * gp._clip(dcam, dt))[:, None, None] * I3
    Vs = V + (mu * gp._clip(dlm, dt))[:, None, None] * I3
    Vi = gp._inv3(Vs, dt)
    W = np.zeros((n, m, 3, 3), dtype=dt)
    np.add.at(W, (pr.cam, pr.lm), -M)
    WV = np.einsum("ilab,lbc->ilac", W, Vi)
    gparts = [np.abs(gPfull).max(initial=0), np.abs(gs).max(initial=0), np.abs(gsp).max(initial=0)]
    if not pr.fix:
        gparts.append(np.abs(gfull).max(initial=0))
    out = dict(cost=B["F"], pcost=Bp["F"], n_used=k, gmax=float(max(gparts)), pgsmax=float(np.abs(gsp).max(initial=0)),
               vinv=_sym6(Vi), g_l=gl, cused=pr.cused, lused=pr.lused)
    full = lambda a_: gp._scatter(pr, a_)

    def pfull(a_, fill=0):
        o = np.full((pr.npairs,) + a_.shape[1:], fill, dtype=a_.dtype)
        o[pr.pidx] = a_
        return o
    pused = np.zeros(pr.npairs, dtype=np.int32); pused[pr.pidx] = 1
    out.update(M=full(_sym6(M)), q=full(q), frozen=full(B["frozen"].astype(np.int32)),
               Mp=pfull(_sym6(Mq)), qp=pfull(qq), pfrozen=pfull(Bp["frozen"].astype(np.int32)), pused=pused)
    if not pr.fix:
        Sb = -np.einsum("ilab,jlcb->iajc", WV, W)
        for i in range(n):
            Sb[i, :, i, :] += Us[i]
        np.add.at(Sb, (pr.ci, slice(None), pr.cj, slice(None)), -Mq)          # S_ij = S_ji = -M_m
        np.add.at(Sb, (pr.cj, slice(None), pr.ci, slice(None)), -Mq)
        S = Sb.reshape(3 * n, 3 * n)
        b = -gc + np.einsum("ilab,lb->ia", WV, gl)
        sinv = gp._inv3(np.stack([S[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(n)]), dt)
        out.update(ustar=Us, sinv=sinv, b=b, S=S)
        if X is not None:
            out["SX"] = S @ np.asarray(X, dtype=dt).reshape(3 * n, -1)
    if dc is not None or pr.fix:
        dcv = np.zeros((n, 3), dtype=dt) if pr.fix else np.where(pr.cused[:, None], np.asarray(dc, dtype=dt).reshape(n, 3), dt(0))
        dP = -np.einsum("lab,lb->la", Vi, gl + np.einsum("ilab,ia->lb", W, dcv))
        dP[~pr.lused] = 0
        ds = -(gs + np.sum(y * (dcv[pr.cam] - dP[pr.lm]), axis=1)) / hs
        dsg = -(gsp + np.sum(yp * (dcv[pr.ci] - dcv[pr.cj]), axis=1)) / hsp
        c1, P1, s1, sg1 = c + dcv, Xp + dP, np.maximum(s + ds, dt(S_MIN)), np.maximum(sg + dsg, dt(S_MIN))
        Jd = jc[:, None] * (dcv[pr.cam] - dP[pr.lm]) + B["Js"] * ds[:, None]
        Jdp = jcp[:, None] * (dcv[pr.ci] - dcv[pr.cj]) + Bp["Js"] * dsg[:, None]
        sc = np.full(pr.nobs, -1, dtype=dt); sc[pr.idx] = s1
        cu = np.zeros(n, dtype=bool) if pr.fix else pr.cused
        out.update(dP=dP, ds=full(ds), dsigma=pfull(dsg), t1=c1.T, p1=P1.T, s1=sc, sigma1=pfull(sg1, -1),
                   cost1=pr.cost(c1, P1, s1), pcost1=pr.pair_cost(c1, sg1),
                   model=float(np.sum(B["r"] * Jd) + 0.5 * np.sum(Jd * Jd)), pmodel=float(np.sum(Bp["r"] * Jdp) + 0.5 * np.sum(Jdp * Jdp)),
                   step2=np.array([np.sum(dcv * dcv), np.sum(dP * dP), np.sum(ds * ds)], dtype=dt), pstep2=np.sum(dsg * dsg),
                   x2=np.array([np.sum(c[cu] ** 2), np.sum(Xp[pr.lused] ** 2), np.sum(s * s)], dtype=dt), px2=np.sum(sg * sg))
    out["_B"], out["_Bp"] = B, Bp
    return out


# ------------------------------------------------------------------------------------------------ scenes the CPU and the GPU tests share
def all_pairs(n):
    i, j = np.triu_indices(n, 1)
    return i.astype(np.int32), j.astype(np.int32)


def relative_translations(S, pi, pj, noise=0.0, seed=0):
    """trel of cam2_from_cam1 from the scene's geometry, a unit vector: x_2 = R_j^T (R_i x_1 + c_i - c_j), so trel = R_j^T (c_i - c_j) / |.|;
    noise: a normal perturbation of that size before normalising"""
    rng = np.random.default_rng(seed)
    R = np.stack([S["rot"][:, 3 * i:3 * i + 3] for i in range(S["n"])])
    d = (S["t"][:, pi] - S["t"][:, pj]).T
    tr = np.einsum("kba,kb->ka", R[pj], d / np.linalg.norm(d, axis=1)[:, None])
    tr = tr + noise * rng.standard_normal(tr.shape)
    return tr / np.linalg.norm(tr, axis=1)[:, None]


def perturbed_start(S, seed, rel=0.5, radius=8.0):
    """the truth moved by up to rel x the ring's radius per coordinate (the pair terms do not converge from the reference's random start:
    see tests/test_gp_pairs_numpy.py)"""
    rng = np.random.default_rng(seed)
    return S["t"] + rel * radius * rng.uniform(-1, 1, S["t"].shape) / np.sqrt(3), S["P"] + rel * radius * rng.uniform(-1, 1, S["P"].shape) / np.sqrt(3)


def strip_long_tracks(S, cams, min_views=3):
    """the scene with every observation of `cams` replaced by two new landmarks per camera, each seen by it and by one of its two ring
    neighbours (which are not in `cams`): every landmark of theirs is below min_views, so with observation terms alone they are not used,
    while the observation graph stays connected (a context needs that)"""
    cams = list(cams)
    n = S["n"]
    keep = ~np.isin(S["cam"], cams)
    R = np.stack([S["rot"][:, 3 * i:3 * i + 3] for i in range(n)])
    rng = np.random.default_rng(5)
    newP = rng.uniform(-1, 1, (2 * len(cams), 3))
    cam, lm, p = list(S["cam"][keep]), list(S["lm"][keep]), list(S["p"][keep])
    for q, i in enumerate(cams):
        for side, nb in enumerate(((i + 1) % n, (i - 1) % n)):
            assert nb not in cams
            l = 2 * q + side
            for cc in (i, nb):
                cam.append(cc); lm.append(S["m"] + l); p.append(R[cc].T @ (newP[l] - S["t"][:, cc]))
    out = dict(S, cam=np.array(cam, dtype=np.int32), lm=np.array(lm, dtype=np.int32), p=np.array(p), m=S["m"] + 2 * len(cams),
               P=np.concatenate([S["P"], newP.T], axis=1))
    out["w"] = np.ones(out["cam"].size)
    assert np.bincount(out["lm"], minlength=out["m"])[S["m"]:].max() < min_views
    return out


def aligned_centre_error(S, t, cams=None):
    """largest distance of a centre from the scene's after the best similarity over the centres `cams` (all by default)"""
    sel = np.arange(S["n"]) if cams is None else np.asarray(cams)
    return float(np.sqrt(np.sum((gp.align(t[:, sel], S["t"][:, sel]) - S["t"][:, sel]) ** 2, axis=0)).max())
