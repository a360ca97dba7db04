"""Robust losses and non-monotonic steps on top of the numpy restatement of xm_ctx_bundle_adjust (xm_ba_numpy.py, used as it is): Ceres's
loss functions (loss_function.cc), its Corrector for losses with rho'' <= 0 (r and J scaled by sqrt(rho')), its TrustRegionStepEvaluator
(Conn, Gould & Toint, Algorithm 10.1.2), and the exact-solve Levenberg-Marquardt of xm_ba_numpy.lm extended by both.  Plus a scene with
gross 2-D outliers."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import xm_ba_numpy as ba

LOSSES = ("trivial", "huber", "soft_l1", "cauchy", "arctan")
TINY = np.finfo(np.float64).tiny          # Ceres clamps rho' below at the smallest normal double


def rho(loss, s, a=0.0):
    """(rho, rho', rho'') of Ceres's loss with scale a at s = |r|^2 (arrays)"""
    s = np.asarray(s, dtype=np.float64)
    if loss == "trivial":
        return s.copy(), np.ones_like(s), np.zeros_like(s)
    if loss == "huber":
        b = a * a
        big = s > b
        r = np.sqrt(np.where(big, s, 1.0))
        r1 = np.where(big, np.maximum(TINY, a / r), 1.0)
        return np.where(big, 2.0 * a * r - b, s), r1, np.where(big, -r1 / (2.0 * np.where(big, s, 1.0)), 0.0)
    if loss == "soft_l1":
        b = a * a
        c = 1.0 / b
        tot = 1.0 + s * c
        tmp = np.sqrt(tot)
        r1 = np.maximum(TINY, 1.0 / tmp)
        return 2.0 * b * (tmp - 1.0), r1, -(c * r1) / (2.0 * tot)
    if loss == "cauchy":
        b = a * a
        c = 1.0 / b
        tot = 1.0 + s * c
        inv = 1.0 / tot
        return b * np.log(tot), np.maximum(TINY, inv), -c * (inv * inv)
    if loss == "arctan":
        b = 1.0 / (a * a)
        tot = 1.0 + s * s * b
        inv = 1.0 / tot
        return a * np.arctan2(s, a), np.maximum(TINY, inv), -2.0 * s * b * (inv * inv)
    raise ValueError(loss)


class RobustProblem(ba.Problem):
    """xm_ba_numpy.Problem with a loss: cost 1/2 sum rho(|r_e|^2), corrected residuals and Jacobian sqrt(rho'(s_e)) (r_e, J_e)"""

    def __init__(self, cam, lm, p, w, n, m, fix_rotations=False, loss="trivial", a=0.0):
        super().__init__(cam, lm, p, w, n, m, fix_rotations)
        self.loss, self.a = loss, a

    def sq(self, r):
        return r[0::2] ** 2 + r[1::2] ** 2

    def cost(self, Rcw, tcw, P):
        return 0.5 * float(np.sum(rho(self.loss, self.sq(self.residuals(Rcw, tcw, P)), self.a)[0]))

    def corrected(self, Rcw, tcw, P):
        """(F, r~, J~)"""
        r, J = self.jacobian(Rcw, tcw, P)
        r0, r1, _ = rho(self.loss, self.sq(r), self.a)
        c = np.repeat(np.sqrt(r1), 2)
        return 0.5 * float(np.sum(r0)), c * r, sp.diags(c) @ J


class StepEvaluator:
    """Ceres's TrustRegionStepEvaluator: the step quality of a candidate and the bookkeeping of an accepted step"""

    def __init__(self, cost, max_nonmonotonic):
        self.max = max_nonmonotonic
        self.minimum = self.current = self.reference = self.candidate = cost
        self.dm_ref = self.dm_cand = 0.0
        self.steps = 0

    def quality(self, cost, dm):
        return max((self.current - cost) / dm, (self.reference - cost) / (self.dm_ref + dm))

    def accepted(self, cost, dm):
        """returns True when the point is a new minimum"""
        self.current = cost
        self.dm_cand += dm
        self.dm_ref += dm
        new_min = cost < self.minimum
        if new_min:
            self.minimum = self.candidate = cost
            self.steps = 0
            self.dm_cand = 0.0
        else:
            self.steps += 1
            if cost > self.candidate:
                self.candidate = cost
                self.dm_cand = 0.0
        if self.steps == self.max:
            self.reference, self.dm_ref = self.candidate, self.dm_cand
        return new_min


def lm(cam, lm_, p, w, rot, t, P, loss="trivial", a=0.0, nonmonotonic=False, max_nonmonotonic=5, fix_rotations=False, max_iters=1000,
       function_tol=1e-6, gradient_tol=1e-10, parameter_tol=1e-8):
    """xm_ba_numpy.lm with a loss and, optionally, non-monotonic steps (the least-cost point is returned).  info as there, plus
    "nonmonotonic_accepts": accepted steps whose candidate cost exceeded the current one"""
    n, m = t.shape[1], P.shape[1]
    pr = RobustProblem(cam, lm_, p, w, n, m, fix_rotations, loss, a)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    X = P.T.copy()
    radius, nu = 1e4, 2.0
    F, r, J = pr.corrected(Rcw, tcw, X)
    g = J.T @ r
    ev = StepEvaluator(F, max_nonmonotonic)
    best = (Rcw, tcw, X, g)
    info = dict(initial_cost=F, n_used=pr.n_used)
    trace = []
    iters = accepted = up = 0
    status = "no_convergence"
    while True:
        if np.max(np.abs(g), initial=0.0) <= gradient_tol:
            status = "gradient_tolerance"; break
        if iters >= max_iters:
            status = "max_iterations"; break
        mu = 1.0 / radius
        A = (J.T @ J).tocsc()
        D = np.clip(A.diagonal(), 1e-6, 1e32)
        d = spla.spsolve(A + sp.diags(mu * D).tocsc(), -g)
        Jd = J @ d
        model_dec = -(float(r @ Jd) + 0.5 * float(Jd @ Jd))
        Rn, tn, Xn = pr.plus(Rcw, tcw, X, d)
        Fn = pr.cost(Rn, tn, Xn)
        iters += 1
        c = pr.cused
        dc = d[:pr.cd * n].reshape(n, pr.cd)[c]
        step = float(np.sqrt(np.sum(dc ** 2) + np.sum(d[pr.cd * n:].reshape(m, 3)[pr.lused] ** 2)))
        valid = np.isfinite(Fn) and model_dec > 0
        q = -1.0
        if valid:
            q = ev.quality(Fn, model_dec) if nonmonotonic else (F - Fn) / model_dec
        acc = bool(valid and q > 1e-3)
        trace.append((F, Fn, mu, float(acc)))
        if step <= parameter_tol * (pr.x_norm(tcw, X) + parameter_tol):
            status = "parameter_tolerance"; break
        if acc:
            accepted += 1
            up += Fn > F
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * q - 1.0) ** 3))
            nu = 2.0
            Rcw, tcw, X = Rn, tn, Xn
            Fold, F = F, Fn
            F, r, J = pr.corrected(Rcw, tcw, X)
            g = J.T @ r
            if not nonmonotonic or ev.accepted(Fn, model_dec):
                best = (Rcw, tcw, X, g)
            if abs(Fold - Fn) <= function_tol * Fold:
                status = "function_tolerance"; break
        else:
            radius /= nu
            nu *= 2.0
            if radius < 1e-32:
                status = "no_progress"; break
    Rcw, tcw, X, g = best
    F = pr.cost(Rcw, tcw, X)
    rot_o, t_o = ba.to_camera_to_world(Rcw, tcw)
    rot_o[:, np.repeat(~pr.cused, 3)] = rot[:, np.repeat(~pr.cused, 3)]
    t_o[:, ~pr.cused] = t[:, ~pr.cused]
    P_o = X.T.copy()
    P_o[:, ~pr.lused] = P[:, ~pr.lused]
    info.update(status=ba.STATUS[status], iters=iters, accepted=accepted, final_cost=F, gradient_max=float(np.max(np.abs(g), initial=0.0)),
                trace=np.array(trace).reshape(-1, 4), nonmonotonic_accepts=int(up))
    return rot_o, t_o, P_o, info


def robust_cost(cam, lm_, p, w, rot, t, P, loss="trivial", a=0.0):
    pr = RobustProblem(cam, lm_, p, w, t.shape[1], P.shape[1], False, loss, a)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    return pr.cost(Rcw, tcw, P.T.copy())


def sq_errors(cam, lm_, p, w, rot, t, P):
    """|r_e|^2 of every observation in input order, -1 where it is not used (xm_ctx_reprojection_errors)"""
    n, m = t.shape[1], P.shape[1]
    u = ba.used_mask(p, w)
    out = -np.ones(len(cam))
    pr = ba.Problem(cam, lm_, p, np.ones(len(cam)), n, m)      # every observation with p2 > 0, in input order
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    r = pr.residuals(Rcw, tcw, P.T.copy())
    s = r[0::2] ** 2 + r[1::2] ** 2
    pos = np.asarray(p)[:, 2] > 0
    full = -np.ones(len(cam))
    full[pos] = s
    out[u] = full[u]
    return out


def outlier_scene(n_cams=30, n_pts=400, seed=0, noise=2e-3, frac_out=0.05, out_size=0.3, **kw):
    """ring_scene with noise plus gross outliers: a fraction frac_out of the observations moved by up to out_size (normalised units)
    in the image.  Returns (scene, outlier mask)"""
    S = ba.ring_scene(n_cams=n_cams, n_pts=n_pts, seed=seed, noise=noise, **kw)
    rng = np.random.default_rng(seed + 1000)
    k = S["cam"].size
    bad = rng.random(k) < frac_out
    p = S["p"].copy()
    off = rng.uniform(-out_size, out_size, (int(bad.sum()), 2))
    p[bad, :2] += off * p[bad, 2:3]
    S = dict(S)
    S["p"] = p
    return S, bad
