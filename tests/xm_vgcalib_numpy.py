"""View-graph calibration (include/xm_amd.h: xm_view_graph_calibrate) restated for the tests.  Nothing here is compared with the reference's
compiled code (it needs Ceres, COLMAP, Eigen and glog); the C++ is cited by file and line and restated, no line of it is copied.

(a) `calibrate_sequential`: plain Python loops over the pairs and cameras in the order of the C++, in a selectable arithmetic type (float64 or
    longdouble); the normal equations are assembled densely and solved by numpy.linalg.solve (in longdouble: followed by two rounds of
    iterative refinement, numpy's solver being float64).
(b) `calibrate_contract`: the vectorised float64 contract, operation by operation what the device does for the residuals (rule 2), the flags
    (rule 6) and the configuration update (rule 7), and the device's PCG rule for the normal equations.
`jacobi_svd`: a one-sided Jacobi SVD in any type, the higher-precision reference of the set-up.

Files cited: estimators/view_graph_calibration.cc (VGC), estimators/cost_function.h (CF), processors/view_graph_manipulation.cc (VGM),
math/two_view_geometry.cc (TVG), estimators/view_graph_calibration.h and optimization_base.h for the defaults."""
import numpy as np

MODEL_NONE, MODEL_E, MODEL_F, MODEL_H = 0, 1, 2, 3
VALID, INVALID_IN, TWO_VIEW_ERROR = 0, 1, 2
CAM_UNUSED, CAM_CONSTANT, CAM_REFINED, CAM_REJECTED = 0, 1, 2, 3
STOP_NONE, STOP_FUNCTION, STOP_GRADIENT, STOP_PARAMETER, STOP_MAX_ITERATIONS, STOP_NO_PROGRESS = 0, 1, 2, 3, 4, 6
MAX_PCG = 500
PCG_TOL2 = 1e-24

DEFAULTS = dict(thres_loss_function=1e-2, thres_lower_ratio=0.1, thres_higher_ratio=10.0, thres_two_view_error=2.0,   # view_graph_calibration.h:21-23
                max_num_iterations=100, function_tolerance=1e-5,                                                        # optimization_base.h:21-26
                lower_bound=1e-3, gradient_tolerance=1e-10, parameter_tolerance=1e-8)                                   # VGC:113; Ceres's defaults


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


# ---------------------------------------------------------------------------------------------------------------- synthetic graphs
def random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def fundamental(f1, pp1, f2, pp2, R, t):
    """K2^-T [t]x R K1^-1 (TVG:41-55) in plain float64 matrix products: the generator of the test graphs, not the contract of rule 7"""
    T = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    K1 = np.array([[f1, 0, pp1[0]], [0, f1, pp1[1]], [0, 0, 1.0]]); K2 = np.array([[f2, 0, pp2[0]], [0, f2, pp2[1]], [0, 0, 1.0]])
    return np.linalg.inv(K2).T @ (T @ R) @ np.linalg.inv(K1)


def make_graph(ncams, npairs, seed, images_per_camera=1, pairs=None, perturb=(0.6, 1.6), scale_F=True):
    """noise-free synthetic graph: random rotations and centres, focals in 600-1500, principal points near (500, 400), F = K2^-T [t]x R K1^-1
    scaled to unit Frobenius norm (as an estimated F comes).  -> dict with the call's inputs (focal0 = truth times a factor in `perturb`),
    truth, Rrel, trel"""
    rng = np.random.default_rng(seed)
    n = ncams * images_per_camera
    cam = np.repeat(np.arange(ncams, dtype=np.int32), images_per_camera)
    truth = rng.uniform(600.0, 1500.0, ncams)
    pp = np.stack([rng.uniform(450.0, 550.0, ncams), rng.uniform(350.0, 450.0, ncams)], axis=1)
    Rw = [random_rotation(rng) for _ in range(n)]
    cw = rng.standard_normal((n, 3)) * 3.0
    if pairs is None:
        allp = [(i, j) for i in range(n) for j in range(i + 1, n)]
        idx = rng.permutation(len(allp))[:npairs]
        pairs = [allp[k] for k in sorted(idx)]
    pi = np.array([p[0] for p in pairs], dtype=np.int32); pj = np.array([p[1] for p in pairs], dtype=np.int32)
    F = np.zeros((len(pairs), 3, 3)); Rrel = np.zeros((len(pairs), 3, 3)); trel = np.zeros((len(pairs), 3))
    for k, (i, j) in enumerate(pairs):
        R = Rw[j] @ Rw[i].T
        t = Rw[j] @ (cw[i] - cw[j])
        t = t / np.linalg.norm(t)
        Rrel[k], trel[k] = R, t
        Fk = fundamental(truth[cam[i]], pp[cam[i]], truth[cam[j]], pp[cam[j]], R, t)
        F[k] = Fk / np.linalg.norm(Fk) if scale_F else Fk
    focal0 = truth * rng.uniform(perturb[0], perturb[1], ncams)
    return dict(focal0=focal0, pp=pp, has_prior=np.zeros(ncams, dtype=np.uint8), cam_of_image=cam, pi=pi, pj=pj,
                model=np.full(len(pairs), MODEL_F, dtype=np.int32), F=F, valid_in=None, truth=truth, Rrel=Rrel, trel=trel)


def random_rank2(rng):
    U, s, Vt = np.linalg.svd(rng.standard_normal((3, 3)))
    s[2] = 0.0
    M = U @ np.diag(s) @ Vt
    return M / np.linalg.norm(M)


def call_inputs(g):
    return {k: g[k] for k in ("focal0", "pp", "has_prior", "cam_of_image", "pi", "pj", "model", "F", "valid_in")}


# ---------------------------------------------------------------------------------------------------------------- rule 1
def jacobi_svd(G, T=np.longdouble, sweeps=60):
    """one-sided Jacobi (Hestenes) SVD of the 3 x 3 G in the type T: G = U diag(s) V^T, s descending.  A column of U whose singular value
    is 0 is 0 (a rank-2 G: u_2 is not needed by rule 1)"""
    A = np.array(G, dtype=T)
    V = np.eye(3, dtype=T)
    eps = np.finfo(T).eps
    for _ in range(sweeps):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha = A[:, p] @ A[:, p]; beta = A[:, q] @ A[:, q]; gamma = A[:, p] @ A[:, q]
            if gamma == 0 or not abs(gamma) > eps * np.sqrt(alpha * beta):
                continue
            zeta = (beta - alpha) / (2 * gamma)
            t = np.copysign(T(1), zeta) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
            c = 1 / np.sqrt(1 + t * t); s = c * t
            ap, aq = A[:, p].copy(), A[:, q].copy()
            A[:, p] = c * ap - s * aq; A[:, q] = s * ap + c * aq
            vp, vq = V[:, p].copy(), V[:, q].copy()
            V[:, p] = c * vp - s * vq; V[:, q] = s * vp + c * vq
            rotated = True
        if not rotated:
            break
    s = np.sqrt(np.sum(A * A, axis=0))
    order = np.argsort(-s, kind="stable")
    A, V, s = A[:, order], V[:, order], s[order]
    U = np.zeros((3, 3), dtype=T)
    for k in range(3):
        if s[k] > 0:
            U[:, k] = A[:, k] / s[k]
    return U, s, V


def G_of(F, pp0, pp1, T=np.float64):
    """K1^T F K0 with K = [[1,0,px],[0,1,py],[0,0,1]] (CF:107-115), every entry as (a*b + c*d) + e"""
    F = np.array(F, dtype=T).reshape(3, 3)
    px0, py0, px1, py1 = T(pp0[0]), T(pp0[1]), T(pp1[0]), T(pp1[1])
    H = np.zeros((3, 3), dtype=T)
    for i in range(3):
        H[i, 0] = F[i, 0]; H[i, 1] = F[i, 1]
        H[i, 2] = (F[i, 0] * px0 + F[i, 1] * py0) + F[i, 2]
    G = H.copy()
    for j in range(3):
        G[2, j] = (px1 * H[0, j] + py1 * H[1, j]) + H[2, j]
    return G


def fetzer_d(G, T=np.float64, svd="lapack"):
    """d_01 and d_12 of CF:47-100 from the SVD of G: svd = "lapack" (numpy.linalg.svd, float64 only) or "jacobi" (jacobi_svd in T).
    -> 8 values (d_01, d_12); d_02 is computed by the reference and never read"""
    if svd == "lapack":
        U, s, Vt = np.linalg.svd(np.asarray(G, dtype=np.float64))
        V = Vt.T
    else:
        U, s, V = jacobi_svd(G, T)
    U, s, V = U.astype(T), s.astype(T), V.astype(T)
    v0, v1, u0, u1 = V[:, 0], V[:, 1], U[:, 0], U[:, 1]                                                    # CF:68-72
    ai = [s[0] * s[0] * (v0[0] * v0[0] + v0[1] * v0[1]), s[0] * s[1] * (v0[0] * v1[0] + v0[1] * v1[1]),   # CF:74-77
          s[1] * s[1] * (v1[0] * v1[0] + v1[1] * v1[1])]
    aj = [u1[0] * u1[0] + u1[1] * u1[1], -(u0[0] * u1[0] + u0[1] * u1[1]), u0[0] * u0[0] + u0[1] * u0[1]]   # CF:79-81
    bi = [s[0] * s[0] * v0[2] * v0[2], s[0] * s[1] * v0[2] * v1[2], s[1] * s[1] * v1[2] * v1[2]]           # CF:83-85
    bj = [u1[2] * u1[2], -(u0[2] * u1[2]), u0[2] * u0[2]]                                                   # CF:87-88

    def dd(u, v):                                                                                           # CF:47-60
        return [ai[u] * aj[v] - ai[v] * aj[u], ai[u] * bj[v] - ai[v] * bj[u], bi[u] * aj[v] - bi[v] * aj[u], bi[u] * bj[v] - bi[v] * bj[u]]
    return np.array(dd(1, 0) + dd(2, 1), dtype=T)                                                           # CF:90, :92


def normalise_d(d):
    """each of d_01, d_12 scaled to unit max-norm with its largest-magnitude entry positive: d is defined up to a joint sign (rule 1)"""
    d = np.array(d).reshape(-1, 2, 4).copy()
    for k in range(d.shape[0]):
        for h in range(2):
            j = int(np.argmax(np.abs(d[k, h])))
            if d[k, h, j] != 0:
                d[k, h] = d[k, h] / d[k, h, j]
    return d.reshape(-1, 8)


# ---------------------------------------------------------------------------------------------------------------- the problem
def participating(g, model=None):
    """indices of the valid pairs of model E or F in input order (VGC:72-79), their two cameras"""
    model = g["model"] if model is None else model
    valid = np.ones(len(g["pi"]), dtype=bool) if g["valid_in"] is None else np.asarray(g["valid_in"]) != 0
    k = np.flatnonzero(valid & ((model == MODEL_E) | (model == MODEL_F)))
    cam = np.asarray(g["cam_of_image"])
    return k, cam[g["pi"][k]], cam[g["pj"][k]]


def setup_all(g, T=np.float64, svd="lapack", model=None, F=None):
    k, ca, cb = participating(g, model)
    F = g["F"] if F is None else F
    d = np.zeros((len(k), 8), dtype=T)
    for m in range(len(k)):
        d[m] = fetzer_d(G_of(F[k[m]], g["pp"][ca[m]], g["pp"][cb[m]], T), T, svd)
    return d


def setup_contract(g, model=None, F=None):
    """setup_all in float64 with numpy.linalg.svd, vectorised over the pairs (the same formulas in the same order)"""
    k, ca, cb = participating(g, model)
    F = np.asarray(g["F"] if F is None else F, dtype=np.float64).reshape(-1, 3, 3)[k]
    pp = np.asarray(g["pp"], dtype=np.float64)
    px0, py0, px1, py1 = pp[ca, 0], pp[ca, 1], pp[cb, 0], pp[cb, 1]
    H = F.copy()
    H[:, :, 2] = (F[:, :, 0] * px0[:, None] + F[:, :, 1] * py0[:, None]) + F[:, :, 2]
    G = H.copy()
    G[:, 2, :] = (px1[:, None] * H[:, 0, :] + py1[:, None] * H[:, 1, :]) + H[:, 2, :]
    if len(k) == 0:
        return np.zeros((0, 8))
    U, s, Vt = np.linalg.svd(G)
    v0, v1, u0, u1 = Vt[:, 0, :], Vt[:, 1, :], U[:, :, 0], U[:, :, 1]
    s0, s1 = s[:, 0], s[:, 1]
    ai = [s0 * s0 * (v0[:, 0] * v0[:, 0] + v0[:, 1] * v0[:, 1]), s0 * s1 * (v0[:, 0] * v1[:, 0] + v0[:, 1] * v1[:, 1]),
          s1 * s1 * (v1[:, 0] * v1[:, 0] + v1[:, 1] * v1[:, 1])]
    aj = [u1[:, 0] * u1[:, 0] + u1[:, 1] * u1[:, 1], -(u0[:, 0] * u1[:, 0] + u0[:, 1] * u1[:, 1]), u0[:, 0] * u0[:, 0] + u0[:, 1] * u0[:, 1]]
    bi = [s0 * s0 * v0[:, 2] * v0[:, 2], s0 * s1 * v0[:, 2] * v1[:, 2], s1 * s1 * v1[:, 2] * v1[:, 2]]
    bj = [u1[:, 2] * u1[:, 2], -(u0[:, 2] * u1[:, 2]), u0[:, 2] * u0[:, 2]]

    def dd(u, v):
        return [ai[u] * aj[v] - ai[v] * aj[u], ai[u] * bj[v] - ai[v] * bj[u], bi[u] * aj[v] - bi[v] * aj[u], bi[u] * bj[v] - bi[v] * bj[u]]
    return np.stack(dd(1, 0) + dd(2, 1), axis=1)


def residual_one(d, fi, fj, T):
    """CF:132-152 / :189-212 for one pair: -> r0, r1 and what the analytic Jacobian needs"""
    fi2 = fi * fi; fj2 = fj * fj
    di = fj2 * d[0] + d[1]                     # CF:140
    dj = fi2 * d[4] + d[6]                     # CF:141
    di_set = di == 0; dj_set = dj == 0
    if di_set:
        di = T(1e-6)                           # CF:142
    if dj_set:
        dj = T(1e-6)                           # CF:143
    n0 = fj2 * d[2] + d[3]; n1 = fi2 * d[5] + d[7]
    K0 = -(n0 / di); K1 = -(n1 / dj)           # CF:145-146
    r0 = (fi2 - K0) / fi2; r1 = (fj2 - K1) / fj2   # CF:148-149
    dK0 = -((2 * fj * d[2]) * di - n0 * (0 if di_set else 2 * fj * d[0])) / (di * di)
    dK1 = -((2 * fi * d[5]) * dj - n1 * (0 if dj_set else 2 * fi * d[4])) / (dj * dj)
    J = [(2 * K0) / (fi2 * fi), -(dK0 / fi2), -(dK1 / fj2), (2 * K1) / (fj2 * fj)]
    return r0, r1, J


def cauchy(s, a, T):
    """Ceres's CauchyLoss (loss_function.cc): rho(s), rho'(s)"""
    b = a * a
    sm = 1 + s * (1 / b)
    return b * np.log(sm), max(T(np.finfo(np.float64).tiny), 1 / sm)


def _unknowns(g, ca, cb):
    ncams = len(g["focal0"])
    touched = np.zeros(ncams, dtype=bool)
    touched[ca] = True; touched[cb] = True
    free = touched & (np.asarray(g["has_prior"]) == 0)          # VGC:110-117
    slot = np.full(ncams, -1)
    slot[free] = np.arange(int(free.sum()))
    return touched, free, slot


def linearise_sequential(d, ca, cb, slot, f, a, T, dense=True):
    """cost, corrector-scaled records, gradient and J^T J (dense; dense=False: its diagonal alone) at f, pair by pair"""
    nf = int((slot >= 0).sum())
    g = np.zeros(nf, dtype=T); A = np.zeros((nf, nf) if dense else nf, dtype=T)
    cost = T(0); raw = np.zeros((len(ca), 2), dtype=T); rec = np.zeros((len(ca), 6), dtype=T)
    for m in range(len(ca)):
        r0, r1, J = residual_one(d[m], f[ca[m]], f[cb[m]], T)
        if ca[m] == cb[m]:                                       # VGC:89-94: one parameter block
            J = [J[0] + J[1], T(0), J[2] + J[3], T(0)]
        rho, rho1 = cauchy(r0 * r0 + r1 * r1, a, T)
        w = np.sqrt(rho1)
        cost += rho / 2
        raw[m] = (r0, r1)
        rec[m] = (w * r0, w * r1, w * J[0], w * J[1], w * J[2], w * J[3])
        cols = [(slot[ca[m]], rec[m, 2], rec[m, 4])]
        if ca[m] != cb[m]:
            cols.append((slot[cb[m]], rec[m, 3], rec[m, 5]))
        for (u, c0, c1) in cols:
            if u < 0:
                continue
            g[u] += c0 * rec[m, 0] + c1 * rec[m, 1]
            if not dense:
                A[u] += c0 * c0 + c1 * c1
                continue
            for (v, e0, e1) in cols:
                if v >= 0:
                    A[u, v] += c0 * e0 + c1 * e1
    return cost, raw, rec, g, A


def _solve(A, b, T):
    x = np.linalg.solve(A.astype(np.float64), b.astype(np.float64)).astype(T)
    if T is not np.float64:
        for _ in range(2):
            x = x + np.linalg.solve(A.astype(np.float64), (b - A @ x).astype(np.float64)).astype(T)
    return x


def clamp_diag(d):
    return np.minimum(np.maximum(d, d.dtype.type(1e-6)), d.dtype.type(1e32))


def _lm(lin, cost_at, solve, f0, free_cams, opt, T):
    """the Levenberg-Marquardt rules of xm_ba.hip / xm_gp.hip for Ceres, on whatever lin / cost_at / solve are given.
    lin(f) -> cost, g, extra; solve(extra, g, mu) -> dx, model; cost_at(f) -> cost"""
    f = np.array(f0, dtype=T)
    radius, nu = T(1e4), T(2)
    status, iters, accepted, trace, fresh, Fc = STOP_NONE, 0, 0, [], True, None
    pcg_total = 0
    while True:
        mu = 1 / radius
        if fresh:
            Fc, g, extra = lin(f)
            trace.append(Fc)
            fresh = False
            if (np.max(np.abs(g)) if len(g) else 0) <= opt["gradient_tolerance"]:
                status = STOP_GRADIENT
                break
        if iters >= opt["max_num_iterations"]:
            status = STOP_MAX_ITERATIONS
            break
        dx, model, pit = solve(extra, g, mu)
        pcg_total += pit
        fn = f.copy()
        fn[free_cams] = np.maximum(T(opt["lower_bound"]), f[free_cams] + dx)      # VGC:113: the bound, by projection
        Fn = cost_at(fn)
        iters += 1
        step = fn[free_cams] - f[free_cams]
        step_norm = np.sqrt(np.sum(step * step)); x_norm = np.sqrt(np.sum(f[free_cams] * f[free_cams]))
        model_dec = -model
        valid = bool(np.isfinite(Fn)) and model_dec > 0
        rho = (Fc - Fn) / model_dec if valid else -1
        accept = valid and rho > 1e-3
        if step_norm <= opt["parameter_tolerance"] * (x_norm + opt["parameter_tolerance"]):
            status = STOP_PARAMETER
            break
        if accept:
            accepted += 1
            radius = min(T(1e16), radius / max(T(1) / 3, 1 - (2 * rho - 1) ** 3))
            nu = T(2)
            Fold, Fc, f, fresh = Fc, Fn, fn, True
            if abs(Fold - Fn) <= opt["function_tolerance"] * Fold:
                status = STOP_FUNCTION
                break
        else:
            radius = radius / nu
            nu = nu * 2
            if radius < 1e-32:
                status = STOP_NO_PROGRESS
                break
    if fresh:
        Fc, g, extra = lin(f)
        trace.append(Fc)
    return f, dict(stop=status, iterations=iters, accepted=accepted, cost_trace=np.array(trace, dtype=T), final_cost=Fc, pcg_iterations=pcg_total)


def _results(g, k, ca, cb, touched, free, f, raw, opt):
    """rule 6 (VGC:123-186)"""
    ncams, npairs = len(g["focal0"]), len(g["pi"])
    focal0 = np.asarray(g["focal0"], dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    focal_out = focal0.copy(); focal_est = focal0.copy()
    cam_status = np.where(touched, CAM_CONSTANT, CAM_UNUSED).astype(np.int32)
    for c in np.flatnonzero(free):
        focal_est[c] = f[c]
        ratio = f[c] / focal0[c]
        if ratio > opt["thres_higher_ratio"] or ratio < opt["thres_lower_ratio"]:      # VGC:130-131
            cam_status[c] = CAM_REJECTED
        else:
            cam_status[c] = CAM_REFINED
            focal_out[c] = f[c]                                                          # VGC:144-146
    valid = np.ones(npairs, dtype=bool) if g["valid_in"] is None else np.asarray(g["valid_in"]) != 0
    pair_status = np.where(valid, VALID, INVALID_IN).astype(np.int32)
    residual = np.zeros((npairs, 2))
    raw = np.asarray(raw, dtype=np.float64)
    residual[k] = raw
    thr2 = opt["thres_two_view_error"] * opt["thres_two_view_error"]                     # VGC:162-163
    bad = raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1] > thr2                           # VGC:174
    pair_status[k[bad]] = TWO_VIEW_ERROR
    return dict(focal=focal_out, focal_est=focal_est, refined=(cam_status == CAM_REFINED).astype(np.uint8), cam_status=cam_status,
                pair_status=pair_status, residual=residual)


def _nothing(g, model, F):
    """rule 5 (VGC:32-35): the call returns before CopyBackResults and FilterImagePairs"""
    k, ca, cb = participating(g, model)
    touched, free, slot = _unknowns(g, ca, cb)
    out = _results(g, k[:0], ca[:0], cb[:0], touched, free & False, g["focal0"], np.zeros((0, 2)), DEFAULTS)
    out.update(model=model, F=F, stop=STOP_NONE, iterations=0, accepted=0, cost_trace=np.zeros(0), pcg_iterations=0)
    return out


def calibrate_sequential(g, T=np.longdouble, svd="jacobi", d=None, **kw):
    """(a): VGC:12-49 in plain loops in the type T.  d (participating pairs x 8) replaces the set-up"""
    opt = options(**kw)
    model, F = np.array(g["model"]), np.array(g["F"], dtype=np.float64)
    if opt.get("update_config"):
        model, F = update_config(g)
    k, ca, cb = participating(g, model)
    touched, free, slot = _unknowns(g, ca, cb)
    if not free.any():
        return _nothing(g, model, F)
    d = setup_all(g, T, svd, model, F) if d is None else np.asarray(d, dtype=T)
    a = T(opt["thres_loss_function"])
    free_cams = np.flatnonzero(free)

    def lin(f):
        cost, raw, rec, grad, A = linearise_sequential(d, ca, cb, slot, f, a, T)
        return cost, grad, (rec, A)

    def solve(extra, grad, mu):
        rec, A = extra
        Ad = A + np.diag(mu * clamp_diag(np.diag(A)))
        dx = _solve(Ad, -grad, T)
        model_v = T(0)
        for m in range(len(ca)):
            xa = dx[slot[ca[m]]] if slot[ca[m]] >= 0 else T(0)
            xb = dx[slot[cb[m]]] if slot[cb[m]] >= 0 else T(0)
            t0 = rec[m, 2] * xa + rec[m, 3] * xb; t1 = rec[m, 4] * xa + rec[m, 5] * xb
            model_v += (rec[m, 0] * t0 + rec[m, 1] * t1) + (t0 * t0 + t1 * t1) / 2
        return dx, model_v, 0

    def cost_at(f):
        c = T(0)
        for m in range(len(ca)):
            r0, r1, _ = residual_one(d[m], f[ca[m]], f[cb[m]], T)
            c += cauchy(r0 * r0 + r1 * r1, a, T)[0] / 2
        return c

    f, info = _lm(lin, cost_at, solve, np.asarray(g["focal0"], dtype=T), free_cams, opt, T)
    raw = np.array([residual_one(d[m], f[ca[m]], f[cb[m]], T)[:2] for m in range(len(ca))], dtype=T).reshape(-1, 2)
    out = _results(g, k, ca, cb, touched, free, f, raw, opt)
    out.update(info, model=model, F=F, d=d, f_raw=f)
    return out


# ---------------------------------------------------------------------------------------------------------------- (b) the contract
def residuals_contract(d, fi, fj):
    """rule 2, vectorised float64, every product and sum rounded on its own in the order of include/xm_amd.h -> r (pairs x 2) and the
    intermediate values"""
    d = np.asarray(d, dtype=np.float64)
    fi2 = fi * fi; fj2 = fj * fj
    di = fj2 * d[:, 0] + d[:, 1]
    dj = fi2 * d[:, 4] + d[:, 6]
    di_set = di == 0.0; dj_set = dj == 0.0
    di = np.where(di_set, 1e-6, di); dj = np.where(dj_set, 1e-6, dj)
    n0 = fj2 * d[:, 2] + d[:, 3]; n1 = fi2 * d[:, 5] + d[:, 7]
    K0 = -(n0 / di); K1 = -(n1 / dj)
    r = np.stack([(fi2 - K0) / fi2, (fj2 - K1) / fj2], axis=1)
    return r, dict(fi2=fi2, fj2=fj2, di=di, dj=dj, n0=n0, n1=n1, K0=K0, K1=K1, di_set=di_set, dj_set=dj_set)


def flags_contract(r, thres_two_view_error=2.0):
    return r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] > thres_two_view_error * thres_two_view_error


def records_contract(d, ca, cb, f, a):
    """rules 2 and 3 at f -> cost, raw residuals, corrector-scaled records (pairs x 6)"""
    d = np.asarray(d, dtype=np.float64)
    fi, fj = f[ca], f[cb]
    r, v = residuals_contract(d, fi, fj)
    dK0 = -((2.0 * fj * d[:, 2]) * v["di"] - v["n0"] * np.where(v["di_set"], 0.0, 2.0 * fj * d[:, 0])) / (v["di"] * v["di"])
    dK1 = -((2.0 * fi * d[:, 5]) * v["dj"] - v["n1"] * np.where(v["dj_set"], 0.0, 2.0 * fi * d[:, 4])) / (v["dj"] * v["dj"])
    j00 = (2.0 * v["K0"]) / (v["fi2"] * fi); j01 = -(dK0 / v["fi2"]); j10 = -(dK1 / v["fj2"]); j11 = (2.0 * v["K1"]) / (v["fj2"] * fj)
    same = ca == cb
    j00 = np.where(same, j00 + j01, j00); j10 = np.where(same, j10 + j11, j10)
    j01 = np.where(same, 0.0, j01); j11 = np.where(same, 0.0, j11)
    s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    b = a * a
    sm = 1.0 + s * (1.0 / b)
    rho1 = np.maximum(np.finfo(np.float64).tiny, 1.0 / sm)
    w = np.sqrt(rho1)
    rec = np.stack([w * r[:, 0], w * r[:, 1], w * j00, w * j01, w * j10, w * j11], axis=1)
    return float(np.sum(0.5 * (b * np.log(sm)))), r, rec


def camera_sums_contract(rec, ca, cb, slot, nf):
    """gradient and diagonal of J^T J per unknown"""
    g = np.zeros(nf, dtype=rec.dtype); dg = np.zeros(nf, dtype=rec.dtype)
    ua, ub = slot[ca], slot[cb]
    ma = ua >= 0
    np.add.at(g, ua[ma], (rec[:, 2] * rec[:, 0] + rec[:, 4] * rec[:, 1])[ma])
    np.add.at(dg, ua[ma], (rec[:, 2] * rec[:, 2] + rec[:, 4] * rec[:, 4])[ma])
    mb = (ub >= 0) & (ca != cb)
    np.add.at(g, ub[mb], (rec[:, 3] * rec[:, 0] + rec[:, 5] * rec[:, 1])[mb])
    np.add.at(dg, ub[mb], (rec[:, 3] * rec[:, 3] + rec[:, 5] * rec[:, 5])[mb])
    return g, dg


def product_contract(rec, ca, cb, slot, dg, mu, x):
    """(J^T J + mu clamp(diag)) x, in the type of rec"""
    ua, ub = slot[ca], slot[cb]
    x = np.asarray(x, dtype=rec.dtype)
    xa = np.where(ua >= 0, x[np.maximum(ua, 0)], 0); xb = np.where(ub >= 0, x[np.maximum(ub, 0)], 0)
    t0 = rec[:, 2] * xa + rec[:, 3] * xb; t1 = rec[:, 4] * xa + rec[:, 5] * xb
    out = np.zeros(len(x), dtype=rec.dtype)
    ma = ua >= 0
    np.add.at(out, ua[ma], (rec[:, 2] * t0 + rec[:, 4] * t1)[ma])
    mb = (ub >= 0) & (ca != cb)
    np.add.at(out, ub[mb], (rec[:, 3] * t0 + rec[:, 5] * t1)[mb])
    return out + (mu * clamp_diag(dg)) * x


def pcg_contract(apply, b, sinv):
    """the device's PCG rule (xm_lm_shared.h): Jacobi preconditioner, stop at |r|^2 / |b|^2 <= 1e-24 or MAX_PCG iterations"""
    x = np.zeros_like(b); r = b.copy(); z = sinv * r; p = z.copy()
    rz = float(r @ z); bb = float(b @ b); rr = bb
    it = 0
    while True:
        q = rr / bb if bb > 0 else 0.0
        if q <= PCG_TOL2 or it >= MAX_PCG:
            return x, it
        Ap = apply(p)
        pap = float(p @ Ap)
        alpha = rz / pap if (pap > 0 and rz > 0) else 0.0
        x = x + alpha * p
        r = r - alpha * Ap
        z = sinv * r
        rzn = float(r @ z); rr = float(r @ r)
        it += 1
        beta = rzn / rz if rz > 0 else 0.0
        p = z + beta * p
        rz = rzn


def calibrate_contract(g, d=None, svd="lapack", **kw):
    """(b): the vectorised float64 contract with the device's PCG rule.  d (participating pairs x 8) replaces the set-up"""
    opt = options(**kw)
    T = np.float64
    model, F = np.array(g["model"]), np.array(g["F"], dtype=np.float64)
    if opt.get("update_config"):
        model, F = update_config(g)
    k, ca, cb = participating(g, model)
    touched, free, slot = _unknowns(g, ca, cb)
    if not free.any():
        return _nothing(g, model, F)
    if d is None:
        d = setup_contract(g, model, F) if svd == "lapack" else setup_all(g, T, svd, model, F)
    d = np.asarray(d, dtype=T)
    a = opt["thres_loss_function"]
    free_cams = np.flatnonzero(free)
    nf = len(free_cams)

    def lin(f):
        cost, raw, rec = records_contract(d, ca, cb, f, a)
        grad, dg = camera_sums_contract(rec, ca, cb, slot, nf)
        return cost, grad, (rec, dg)

    def solve(extra, grad, mu):
        rec, dg = extra
        dd = dg + mu * clamp_diag(dg)
        sinv = np.where(dd > 0, 1.0 / np.where(dd > 0, dd, 1.0), 0.0)
        dx, it = pcg_contract(lambda p: product_contract(rec, ca, cb, slot, dg, mu, p), -grad, sinv)
        ua, ub = slot[ca], slot[cb]
        xa = np.where(ua >= 0, dx[np.maximum(ua, 0)], 0.0); xb = np.where(ub >= 0, dx[np.maximum(ub, 0)], 0.0)
        t0 = rec[:, 2] * xa + rec[:, 3] * xb; t1 = rec[:, 4] * xa + rec[:, 5] * xb
        return dx, float(np.sum((rec[:, 0] * t0 + rec[:, 1] * t1) + 0.5 * (t0 * t0 + t1 * t1))), it

    def cost_at(f):
        return records_contract(d, ca, cb, f, a)[0]

    f, info = _lm(lin, cost_at, solve, np.asarray(g["focal0"], dtype=T), free_cams, opt, T)
    raw, _ = residuals_contract(d, f[ca], f[cb])
    out = _results(g, k, ca, cb, touched, free, f, raw, opt)
    out.update(info, model=model, F=F, d=d, f_raw=f)
    return out


# ---------------------------------------------------------------------------------------------------------------- rule 7
def update_config(g):
    """VGM:170-231 and TVG:41-55 in float64, every operation rounded on its own in the order of include/xm_amd.h -> model_out, F_out"""
    cam = np.asarray(g["cam_of_image"]); model = np.array(g["model"]).copy(); F = np.array(g["F"], dtype=np.float64).reshape(-1, 3, 3).copy()
    npairs, ncams = len(model), len(g["focal0"])
    valid = np.ones(npairs, dtype=bool) if g["valid_in"] is None else np.asarray(g["valid_in"]) != 0
    prior = np.asarray(g["has_prior"]) != 0
    total = np.zeros(ncams, dtype=np.int64); calibrated = np.zeros(ncams, dtype=np.int64)
    for k in range(npairs):                                                    # VGM:178-198
        if not valid[k]:
            continue
        c1, c2 = cam[g["pi"][k]], cam[g["pj"][k]]
        if not prior[c1] or not prior[c2]:
            continue
        if model[k] == MODEL_E:
            total[c1] += 1; total[c2] += 1; calibrated[c1] += 1; calibrated[c2] += 1
        elif model[k] == MODEL_F:
            total[c1] += 1; total[c2] += 1
    cam_valid = np.array([total[c] > 0 and calibrated[c] * 1.0 / total[c] > 0.5 for c in range(ncams)])   # VGM:203-211
    f0 = np.asarray(g["focal0"], dtype=np.float64); pp = np.asarray(g["pp"], dtype=np.float64)
    for k in range(npairs):                                                    # VGM:213-230
        if not valid[k] or g["model"][k] != MODEL_F:
            continue
        c1, c2 = cam[g["pi"][k]], cam[g["pj"][k]]
        if not (cam_valid[c1] and cam_valid[c2]):
            continue
        model[k] = MODEL_E
        R = np.asarray(g["Rrel"][k], dtype=np.float64).reshape(3, 3); t = np.asarray(g["trel"][k], dtype=np.float64)
        E = np.stack([t[1] * R[2] - t[2] * R[1], t[2] * R[0] - t[0] * R[2], t[0] * R[1] - t[1] * R[0]])     # TVG:41-45
        a2, x2, y2 = 1.0 / f0[c2], -pp[c2, 0] / f0[c2], -pp[c2, 1] / f0[c2]
        a1, x1, y1 = 1.0 / f0[c1], -pp[c1, 0] / f0[c1], -pp[c1, 1] / f0[c1]
        A = np.stack([a2 * E[0], a2 * E[1], (x2 * E[0] + y2 * E[1]) + E[2]])                                # TVG:54: K2^-T E
        F[k] = np.stack([A[:, 0] * a1, A[:, 1] * a1, (A[:, 0] * x1 + A[:, 1] * y1) + A[:, 2]], axis=1)      # ... K1^-1
    return model, F


# ---------------------------------------------------------------------------------------------------------------- shared test cases
def corrupt(g, fraction, seed):
    """a copy of g with `fraction` of the F replaced by random rank-2 matrices -> the copy, the indices replaced"""
    rng = np.random.default_rng(seed)
    h = dict(g)
    h["F"] = g["F"].copy()
    bad = np.sort(rng.permutation(len(g["pi"]))[:max(1, int(round(fraction * len(g["pi"]))))])
    for k in bad:
        h["F"][k] = random_rank2(rng)
    return h, bad


def config_case(seed=5):
    """rule 7 by hand, one image per camera, cameras 0-3, 5, 6 with a prior and 4 without.  Counted (both priors): camera 0 4/4, camera 1
    3/4, camera 2 2/3, camera 5 2/3 (valid); camera 3 1/2, exactly 0.5 (not valid); camera 6 has a prior and no counted pair (its one pair
    is with camera 4); pair 5 = (2, 5) F flips, pair 4 = (1, 3) F has one valid end only, pairs 8 and 9 are not counted"""
    pairs = [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 5), (0, 5), (1, 5), (0, 4), (4, 6)]
    g = make_graph(7, len(pairs), seed, pairs=pairs, perturb=(1.0, 1.0))
    g["model"] = np.array([MODEL_E, MODEL_E, MODEL_E, MODEL_E, MODEL_F, MODEL_F, MODEL_E, MODEL_E, MODEL_F, MODEL_F], dtype=np.int32)
    g["has_prior"] = np.array([1, 1, 1, 1, 0, 1, 1], dtype=np.uint8)
    g["focal0"] = g["truth"] * np.array([1.0, 1.0, 1.0, 1.0, 1.3, 1.0, 1.0])
    return g


def rejection_case(seed=11):
    """priors within 10 % of the truth, except camera 3 whose prior is 20 times its focal"""
    g = make_graph(12, 40, seed, perturb=(0.9, 1.1))
    g["focal0"] = g["focal0"].copy()
    g["focal0"][3] = 20.0 * g["truth"][3]
    return g


def simple2_case(seed=28, perturb=(0.7, 1.4)):
    """the SIMPLE2-derived case: the pairs, relative poses and per-view intrinsics of xm_viewgraph_numpy.simple2_case(), one camera per
    image, F = K_j^-T [t]x R K_i^-1 scaled to unit norm for the E pairs (the F pairs keep theirs), priors off by a factor in `perturb`
    -> the call's inputs (with truth), the view-graph case"""
    import xm_viewgraph_numpy as vg
    c = vg.simple2_case()
    n = len(c["focal"])
    K = np.linalg.inv(c["Kinv"])
    F = np.array(c["FH"])
    for k in np.flatnonzero(c["model"] == vg.E_):
        Fk = c["Kinv"][c["pj"][k]].T @ vg.essential(c["Rrel"][k], c["trel"][k]) @ c["Kinv"][c["pi"][k]]
        F[k] = Fk / np.linalg.norm(Fk)
    rng = np.random.default_rng(seed)
    g = dict(focal0=c["focal"] * rng.uniform(perturb[0], perturb[1], n), pp=np.ascontiguousarray(K[:, :2, 2]), has_prior=np.zeros(n, dtype=np.uint8),
             cam_of_image=np.arange(n, dtype=np.int32), pi=c["pi"], pj=c["pj"], model=c["model"], F=F, valid_in=c["valid_in"], truth=c["focal"].copy(),
             Rrel=c["Rrel"], trel=c["trel"])
    return g, c
