"""numpy / scipy.sparse restatement of the reprojection bundle adjustment behind xm_ctx_bundle_adjust (include/xm_amd.h, xm_ba.h): the
problem, its Jacobian and the Levenberg-Marquardt rules, with EXACT linear solves.  Plus scene generators whose points lie in front of
every camera that sees them.

Layouts are the library's: rot 3 x 3n (R_i, camera to world), t 3 x n (camera centres), P 3 x m; observations (cam, lm, p, w) with p the
depth-lifted camera-frame point, so the measurement is p[:2] / p[2]."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

STATUS = {"no_convergence": 0, "function_tolerance": 1, "gradient_tolerance": 2, "parameter_tolerance": 3, "max_iterations": 4,
          "time_limit": 5, "no_progress": 6}


def to_world_to_camera(rot, t):
    n = t.shape[1]
    Rcw = np.stack([rot[:, 3 * i:3 * i + 3].T for i in range(n)])
    tcw = -np.einsum("iab,bi->ia", Rcw, t)
    return Rcw, tcw


def to_camera_to_world(Rcw, tcw):
    n = Rcw.shape[0]
    rot = np.zeros((3, 3 * n))
    for i in range(n):
        rot[:, 3 * i:3 * i + 3] = Rcw[i].T
    t = -np.einsum("iba,ib->ai", Rcw, tcw)
    return rot, t


def skew(v):
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -v[..., 2], v[..., 1], -v[..., 0]
    K[..., 1, 0], K[..., 2, 0], K[..., 2, 1] = v[..., 2], -v[..., 1], v[..., 0]
    return K


def expmap(w):
    """rotation matrices of rotation vectors w (k x 3), Rodrigues"""
    th2 = np.sum(w * w, axis=1)
    small = th2 < 1e-16
    th = np.sqrt(np.where(small, 1.0, th2))
    A = np.where(small, 1.0 - th2 / 6.0, np.sin(th) / th)
    B = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(th)) / np.where(small, 1.0, th2))
    K = skew(w)
    return np.eye(3) + A[:, None, None] * K + B[:, None, None] * (K @ K)


def used_mask(p, w):
    return (np.asarray(w) > 0) & (np.asarray(p)[:, 2] > 0)


class Problem:
    """observations restricted to the used ones; parameters: CD per camera (rotation vector + translation, or translation only), 3 per
    landmark, all n cameras and m landmarks (unused ones have empty columns)"""

    def __init__(self, cam, lm, p, w, n, m, fix_rotations=False):
        u = used_mask(p, w)
        self.cam, self.lm = np.asarray(cam)[u].astype(np.int64), np.asarray(lm)[u].astype(np.int64)
        q = np.asarray(p, dtype=np.float64)[u]
        self.z = q[:, :2] / q[:, 2:3]
        self.n, self.m, self.cd = n, m, (3 if fix_rotations else 6)
        self.cused = np.bincount(self.cam, minlength=n) > 0
        self.lused = np.bincount(self.lm, minlength=m) > 0
        self.n_used = int(u.sum())

    def residuals(self, Rcw, tcw, P):
        X = np.einsum("kab,kb->ka", Rcw[self.cam], P[self.lm]) + tcw[self.cam]
        return (X[:, :2] / X[:, 2:3] - self.z).reshape(-1)

    def cost(self, Rcw, tcw, P):
        r = self.residuals(Rcw, tcw, P)
        return 0.5 * float(r @ r)

    def jacobian(self, Rcw, tcw, P):
        """(r, J): J sparse 2k x (cd n + 3 m), tangent coordinates of the library (left rotation vector, tcw, P)"""
        R = Rcw[self.cam]
        Y = np.einsum("kab,kb->ka", R, P[self.lm])
        X = Y + tcw[self.cam]
        iz = 1.0 / X[:, 2]
        u = X[:, :2] / X[:, 2:3]
        k = X.shape[0]
        d = np.zeros((k, 2, 3))
        d[:, 0, 0] = iz; d[:, 1, 1] = iz; d[:, 0, 2] = -u[:, 0] * iz; d[:, 1, 2] = -u[:, 1] * iz
        JP = d @ R
        Jc = np.concatenate([d @ (-skew(Y)), d], axis=2) if self.cd == 6 else d
        cd = self.cd
        rows = np.repeat(np.arange(2 * k).reshape(k, 2, 1), cd + 3, axis=2)
        cols = np.concatenate([np.broadcast_to((cd * self.cam)[:, None, None] + np.arange(cd)[None, None, :], (k, 2, cd)),
                               np.broadcast_to((cd * self.n + 3 * self.lm)[:, None, None] + np.arange(3)[None, None, :], (k, 2, 3))], axis=2)
        vals = np.concatenate([Jc, JP], axis=2)
        J = sp.csr_matrix((vals.reshape(-1), (rows.reshape(-1), cols.reshape(-1))), shape=(2 * k, cd * self.n + 3 * self.m))
        return (u - self.z).reshape(-1), J

    def gradient(self, Rcw, tcw, P):
        r, J = self.jacobian(Rcw, tcw, P)
        return J.T @ r

    def plus(self, Rcw, tcw, P, d):
        cd, n = self.cd, self.n
        dc = d[:cd * n].reshape(n, cd)
        dP = d[cd * n:].reshape(self.m, 3)
        Rn, tn, Pn = Rcw.copy(), tcw.copy(), P.copy()
        c, lu = self.cused, self.lused
        if cd == 6:
            Rn[c] = expmap(dc[c, :3]) @ Rcw[c]
            tn[c] = tcw[c] + dc[c, 3:]
        else:
            tn[c] = tcw[c] + dc[c]
        Pn[lu] = P[lu] + dP[lu]
        return Rn, tn, Pn

    def x_norm(self, tcw, P):
        c = self.cused
        return float(np.sqrt((c.sum() if self.cd == 6 else 0) + np.sum(tcw[c] ** 2) + np.sum(P[self.lused] ** 2)))


def lm(cam, lm_, p, w, rot, t, P, fix_rotations=False, max_iters=1000, function_tol=1e-6, gradient_tol=1e-10, parameter_tol=1e-8):
    """the LM of xm_ctx_bundle_adjust with exact solves of the damped normal equations.  Returns (rot, t, P, info) with info: status,
    iters, accepted, initial_cost, final_cost, gradient_max, trace (cost, candidate cost, mu, accepted per iteration)"""
    n, m = t.shape[1], P.shape[1]
    pr = Problem(cam, lm_, p, w, n, m, fix_rotations)
    Rcw, tcw = to_world_to_camera(rot, t)
    X = P.T.copy()
    radius, nu = 1e4, 2.0
    r, J = pr.jacobian(Rcw, tcw, X)
    F = 0.5 * float(r @ r)
    g = J.T @ r
    info = dict(initial_cost=F, n_used=pr.n_used)
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
        rho = (F - Fn) / model_dec if valid else -1.0
        acc = bool(valid and rho > 1e-3)
        trace.append((F, Fn, mu, float(acc)))
        if step <= parameter_tol * (pr.x_norm(tcw, X) + parameter_tol):
            status = "parameter_tolerance"; break
        if acc:
            accepted += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            nu = 2.0
            Rcw, tcw, X = Rn, tn, Xn
            Fold, F = F, Fn
            r, J = pr.jacobian(Rcw, tcw, X)
            g = J.T @ r
            if abs(Fold - Fn) <= function_tol * Fold:
                status = "function_tolerance"; break
        else:
            radius /= nu
            nu *= 2.0
            if radius < 1e-32:
                status = "no_progress"; break
    rot_o, t_o = to_camera_to_world(Rcw, tcw)
    rot_o[:, np.repeat(~pr.cused, 3)] = rot[:, np.repeat(~pr.cused, 3)]
    t_o[:, ~pr.cused] = t[:, ~pr.cused]
    P_o = X.T.copy()
    P_o[:, ~pr.lused] = P[:, ~pr.lused]
    info.update(status=STATUS[status], iters=iters, accepted=accepted, final_cost=F, gradient_max=float(np.max(np.abs(g), initial=0.0)),
                trace=np.array(trace).reshape(-1, 4))
    return rot_o, t_o, P_o, info


def gradient_at(cam, lm_, p, w, rot, t, P, fix_rotations=False):
    """J^T r at a point given in the library's layouts (the numpy Jacobian)"""
    pr = Problem(cam, lm_, p, w, t.shape[1], P.shape[1], fix_rotations)
    Rcw, tcw = to_world_to_camera(rot, t)
    return pr.gradient(Rcw, tcw, P.T.copy())


def reprojection_cost(cam, lm_, p, w, rot, t, P):
    pr = Problem(cam, lm_, p, w, t.shape[1], P.shape[1])
    Rcw, tcw = to_world_to_camera(rot, t)
    return pr.cost(Rcw, tcw, P.T.copy()), pr.n_used


# ------------------------------------------------------------------------------------------------ scenes
def _look_at(c, target, rng, jitter=0.0):
    """world-to-camera rotation of a camera at c looking at target (+z forward), rolled by a random angle of `jitter` radians at most"""
    zc = (target - c) / np.linalg.norm(target - c)
    up = np.array([0.0, 0.0, 1.0]) if abs(zc[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    xc = np.cross(up, zc); xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    Rcw = np.stack([xc, yc, zc])
    if jitter:
        Rcw = expmap(rng.uniform(-jitter, jitter, (1, 3)))[0] @ Rcw
    return Rcw


def _observe(Rcw, tcw, Pw, cams, lms, rng, noise):
    X = np.einsum("kab,kb->ka", Rcw[cams], Pw[lms]) + tcw[cams]
    u = X[:, :2] / X[:, 2:3] + noise * rng.standard_normal((X.shape[0], 2))
    return np.concatenate([u, np.ones((X.shape[0], 1))], axis=1) * X[:, 2:3]


def _pack(Rcw, tcw, Pw, cams, lms, p):
    rot, t = to_camera_to_world(Rcw, tcw)
    return dict(cam=np.asarray(cams, np.int32), lm=np.asarray(lms, np.int32), p=p, w=np.ones(len(cams)), n=Rcw.shape[0], m=Pw.shape[0],
                rot=rot, t=t, P=Pw.T.copy())


def ring_scene(n_cams=30, n_pts=400, seed=0, radius=8.0, cloud=2.0, frac=0.5, min_views=3, noise=0.0):
    """cameras on a ring (varying height) around a point cloud, each looking at its centre; point l is seen by each camera with
    probability frac (at least min_views cameras).  Depths are >= radius - cloud - 1 > 0."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n_cams) / n_cams + rng.uniform(-0.1, 0.1, n_cams)
    C = np.stack([radius * np.cos(ang), radius * np.sin(ang), rng.uniform(-1.0, 1.0, n_cams)], axis=1)
    Rcw = np.stack([_look_at(C[i], rng.uniform(-0.3, 0.3, 3), rng, 0.1) for i in range(n_cams)])
    tcw = -np.einsum("iab,ib->ia", Rcw, C)
    Pw = rng.uniform(-1, 1, (n_pts, 3)) * (cloud / np.sqrt(3))
    cams, lms = [], []
    for l in range(n_pts):
        s = np.nonzero(rng.random(n_cams) < frac)[0]
        if s.size < min_views:
            s = rng.choice(n_cams, min_views, replace=False)
        cams += list(np.sort(s)); lms += [l] * s.size
    cams, lms = np.array(cams), np.array(lms)
    return _pack(Rcw, tcw, Pw, cams, lms, _observe(Rcw, tcw, Pw, cams, lms, rng, noise))


def sequential_scene(n_cams=300, per_cam=12, span=(2, 5), seed=0, noise=1e-3):
    """a side-looking camera moving along a facade: camera i starts per_cam landmarks, each seen by cameras i .. i+k-1 (k from span).
    The reduced camera system is close to a path: PCG needs many iterations.  Depths are about 5."""
    rng = np.random.default_rng(seed)
    C = np.stack([0.5 * np.arange(n_cams), 0.2 * np.sin(0.05 * np.arange(n_cams)), 0.1 * np.cos(0.07 * np.arange(n_cams))], axis=1)
    Rcw = np.stack([_look_at(C[i], C[i] + np.array([0.0, 1.0, 0.0]), rng, 0.05) for i in range(n_cams)])
    tcw = -np.einsum("iab,ib->ia", Rcw, C)
    cams, lms, pts = [], [], []
    for i in range(n_cams):
        for _ in range(per_cam):
            k = int(rng.integers(span[0], span[1] + 1))
            s = np.arange(i, min(n_cams, i + k))
            if s.size < 2:
                s = np.arange(n_cams - 2, n_cams)
            xm = C[s, 0].mean()
            pts.append([xm + rng.uniform(-0.5, 0.5), 5.0 + rng.uniform(-1.0, 1.0), rng.uniform(-1.5, 1.5)])
            cams += list(s); lms += [len(pts) - 1] * s.size
    Pw = np.array(pts)
    cams, lms = np.array(cams), np.array(lms)
    return _pack(Rcw, tcw, Pw, cams, lms, _observe(Rcw, tcw, Pw, cams, lms, rng, noise))


def perturb(rot, t, P, seed=1, deg=2.0, rel=0.01):
    """start point: every rotation turned by up to `deg` degrees, translations and landmarks moved by `rel` of the scene's size"""
    rng = np.random.default_rng(seed)
    n = t.shape[1]
    E = expmap(rng.uniform(-1, 1, (n, 3)) * np.deg2rad(deg) / np.sqrt(3))
    rot2 = rot.copy()
    for i in range(n):
        rot2[:, 3 * i:3 * i + 3] = E[i] @ rot[:, 3 * i:3 * i + 3]
    size = np.max(np.abs(np.concatenate([t, P], axis=1)))
    return rot2, t + rel * size * rng.standard_normal(t.shape) / 3, P + rel * size * rng.standard_normal(P.shape) / 3
