"""Restatement of xm_view_graph_rotations (include/xm_amd.h has the rules): the IRLS stage of the reference's rotation averaging,
deps/glomap/glomap/estimators/global_rotation_averaging.cc (cited below as :line) and math/rigid3d.cc, with skip_initialization = true and
max_num_l1_iterations = 0.

  (a) irls_sequential / stages_sequential: the C++ line by line in plain loops, generic over float64 / longdouble, the linear system built
      from the explicit matrix A of :205-270 and solved exactly (a dense Cholesky solve of the 3 * registered unknowns).  This is the
      reference of every test; nothing in it knows how the device sums.
  (b) irls_contract: the vectorised float64 contract with the device's rules: the Laplacian form of the product, the Jacobi-preconditioned
      CG from zero to a relative residual of 1e-12 or PCG_CAP iterations.

Generators: make_graph (a clean spanning chain, outliers among the other pairs, the start from a chordal least-squares solve), star,
star_ring (one camera in `hub` pairs) and simple2_graph (the SIMPLE2-derived view graph of xm_viewgraph_numpy.simple2_case after pass A)."""
import numpy as np

GEMAN_MCCLURE, HALF_NORM = 0, 1
STOP_NOTHING, STOP_STEP, STOP_ITERATIONS, STOP_NONFINITE = 0, 1, 2, 3
AA_EPS = 1e-12          # glomap/types.h: EPS
PCG_CAP = 500
PCG_TOL2 = 1e-24
LIGHT_INCIDENCES = 64


class Refused(ValueError):
    """what the library answers with XM_ERR_ARG (rule 11)"""


# ------------------------------------------------------------------------------------------------ rules 3 and 4
def aa_to_rot(a, T=np.float64):
    """AngleAxisToRotation (rigid3d.cc:53-71); above the norm 1e-12 Eigen's AngleAxis::toRotationMatrix"""
    a = np.asarray(a, dtype=T)
    n = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    R = np.empty((3, 3), dtype=T)
    if n > T(AA_EPS):                                                  # :55
        u = a / n                                                      # aa_vec.normalized()
        s, c = np.sin(n), np.cos(n)
        su = s * u
        cu = (T(1) - c) * u
        t = cu[0] * u[1]; R[0, 1] = t - su[2]; R[1, 0] = t + su[2]
        t = cu[0] * u[2]; R[0, 2] = t + su[1]; R[2, 0] = t - su[1]
        t = cu[1] * u[2]; R[1, 2] = t - su[0]; R[2, 1] = t + su[0]
        for k in range(3):
            R[k, k] = cu[k] * u[k] + c
    else:                                                              # :59-69, first order, not orthogonal
        R[0, 0] = 1; R[1, 0] = a[2]; R[2, 0] = -a[1]
        R[0, 1] = -a[2]; R[1, 1] = 1; R[2, 1] = a[0]
        R[0, 2] = a[1]; R[1, 2] = -a[0]; R[2, 2] = 1
    return R


def rot_to_quat(R, T=np.float64):
    """Eigen's quaternion from a matrix (the four-branch rule) -> (x, y, z, w) and the branch taken (0: trace, 1 .. 3: diagonal entry)"""
    R = np.asarray(R, dtype=T)
    t = (R[0, 0] + R[1, 1]) + R[2, 2]
    q = np.empty(4, dtype=T)
    if t > 0:
        t = np.sqrt(t + T(1))
        q[3] = T(0.5) * t
        t = T(0.5) / t
        q[0] = (R[2, 1] - R[1, 2]) * t; q[1] = (R[0, 2] - R[2, 0]) * t; q[2] = (R[1, 0] - R[0, 1]) * t
        return q, 0
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j = (i + 1) % 3; k = (j + 1) % 3
    t = np.sqrt(((R[i, i] - R[j, j]) - R[k, k]) + T(1))
    q[i] = T(0.5) * t
    t = T(0.5) / t
    q[3] = (R[k, j] - R[j, k]) * t
    q[j] = (R[j, i] + R[i, j]) * t
    q[k] = (R[k, i] + R[i, k]) * t
    return q, 1 + i


def rot_to_aa(R, T=np.float64):
    """RotationToAngleAxis (rigid3d.cc:47-51): Eigen's AngleAxis from the quaternion; angle * axis"""
    q, _ = rot_to_quat(R, T)
    n = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    if n == 0:
        return np.zeros(3, dtype=T)
    angle = T(2) * np.arctan2(n, abs(q[3]))
    if q[3] < 0:
        n = -n
    return angle * (q[:3] / n)


def mul3(A, B):
    """3 x 3 product, every entry (p0 + p1) + p2 (the order the device uses; longdouble does not care)"""
    C = np.empty((3, 3), dtype=A.dtype)
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    return C


def deg_to_rad(d, T=np.float64):
    """DegToRad (rigid3d.cc:37): degree * pi / 180"""
    pi = T(np.pi) if T is np.float64 else T(4) * np.arctan(T(1))
    return T(d) * pi / T(180)


def weight_of(e2, weight_type, sigma, T=np.float64):
    """:376-381"""
    if weight_type == GEMAN_MCCLURE:
        tmp = e2 + sigma * sigma
        return sigma * sigma / (tmp * tmp)
    if weight_type == HALF_NORM:
        with np.errstate(divide="ignore"):
            return np.power(T(e2), T(-0.75))
    raise Refused("unknown weight type")


# ------------------------------------------------------------------------------------------------ the problem (rules 1 and 11)
def problem(g, fixed_image=-1):
    """participation, the slots of the registered images, the fixed camera; raises Refused as rule 11 does.  -> dict(img, slot, k, ca, cb, fixed)"""
    rot0 = np.asarray(g["rot0"], dtype=np.float64).reshape(-1, 3, 3)
    n = rot0.shape[0]
    pi, pj = np.asarray(g["pi"]), np.asarray(g["pj"])
    Rrel = np.asarray(g["Rrel"], dtype=np.float64).reshape(-1, 3, 3)
    reg = np.ones(n, dtype=bool) if g.get("registered") is None else np.asarray(g["registered"]) != 0
    val = np.ones(pi.size, dtype=bool) if g.get("valid_in") is None else np.asarray(g["valid_in"]) != 0
    if pi.size and (pi.min() < 0 or pj.min() < 0 or pi.max() >= n or pj.max() >= n):
        raise Refused("index out of range")
    if np.any(pi == pj):
        raise Refused("pi == pj")
    if fixed_image < -1 or fixed_image >= n:
        raise Refused("fixed_image out of range")
    if fixed_image >= 0 and not reg[fixed_image]:
        raise Refused("fixed_image is not registered")
    if not np.isfinite(rot0[reg]).all():
        raise Refused("rot0 is not finite")
    img = np.flatnonzero(reg)
    slot = np.full(n, -1, dtype=np.int64); slot[img] = np.arange(img.size)
    part = val & reg[pi] & reg[pj] if pi.size else np.zeros(0, dtype=bool)                # :163-164
    k = np.flatnonzero(part)
    if not np.isfinite(Rrel[k]).all():
        raise Refused("Rrel is not finite")
    ca, cb = slot[pi[k]], slot[pj[k]]
    if k.size:                                                                           # one component (a union-find, smaller root wins)
        parent = np.arange(img.size)

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a
        joins = 0
        for a, b in zip(ca.tolist(), cb.tolist()):
            a, b = find(a), find(b)
            if a != b:
                parent[max(a, b)] = min(a, b); joins += 1
        if joins != img.size - 1:
            raise Refused("the participating pairs do not connect the registered images")
    fixed = fixed_image if fixed_image >= 0 else (int(img[0]) if img.size else -1)         # a departure from :150-156 (hash order)
    return dict(n=n, npairs=pi.size, img=img, slot=slot, k=k, ca=ca, cb=cb, fixed=fixed, rot0=rot0, Rrel=Rrel)


def explicit_A(p, T=np.float64):
    """sparse_matrix_ of :205-270 as a dense array: per participating pair three rows with -1 at image_id1 and +1 at image_id2, then three
    rows with +1 at the fixed camera"""
    M, nr = p["k"].size, p["img"].size
    A = np.zeros((3 * M + 3, 3 * nr), dtype=T)
    for m in range(M):
        for i in range(3):
            A[3 * m + i, 3 * p["ca"][m] + i] = -1                                         # :229-232
            A[3 * m + i, 3 * p["cb"][m] + i] = 1                                          # :241-244
    f = p["slot"][p["fixed"]]
    for i in range(3):
        A[3 * M + i, 3 * f + i] = 1                                                       # :262-265
    return A


def laplacian_normal(p, w, T=np.float64):
    """(L_w + e_f e_f^T) (x) I_3 (rule 8) as a dense array"""
    nr = p["img"].size
    L = np.zeros((nr, nr), dtype=T)
    for m in range(p["k"].size):
        a, b = p["ca"][m], p["cb"][m]
        L[a, a] += w[m]; L[b, b] += w[m]; L[a, b] -= w[m]; L[b, a] -= w[m]
    f = p["slot"][p["fixed"]]
    L[f, f] += 1
    return np.kron(L, np.eye(3, dtype=T))


def cholesky_solve(S, b):
    """dense S x = b for a symmetric positive definite S in S's own precision (numpy's LAPACK has no longdouble): column Cholesky with
    vectorised rank-1 updates, two substitutions"""
    if S.dtype == np.float64:
        return np.linalg.solve(S, b)
    n = S.shape[0]
    L = np.array(S, copy=True)
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
        L[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    y = np.array(b, copy=True)
    for j in range(n):
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


# ------------------------------------------------------------------------------------------------ (a) the sequential restatement
def _residuals_seq(p, est, fixed0, T):
    """ComputeResiduals (:437-483) -> 3M + 3 entries"""
    M = p["k"].size
    R = [aa_to_rot(est[u], T) for u in range(len(est))]
    r = np.zeros(3 * M + 3, dtype=T)
    for m in range(M):
        R_1, R_2 = R[p["ca"][m]], R[p["cb"][m]]                                           # :457-465
        Rr = p["Rrel"][p["k"][m]].astype(T)
        r[3 * m:3 * m + 3] = -rot_to_aa(mul3(R_2.T.copy(), mul3(Rr, R_1)), T)              # :468-469
    f = p["slot"][p["fixed"]]
    r[3 * M:] = rot_to_aa(mul3(aa_to_rot(fixed0, T).T.copy(), R[f]), T)                    # :478-482
    return r, R


def _weights_seq(p, r, weight_type, sigma, T):
    """:362-393 -> the weights of the 3M + 3 rows and of the M pairs"""
    M = p["k"].size
    wrow = np.ones(3 * M + 3, dtype=T)                                                    # :353 the gauge rows
    wp = np.zeros(M, dtype=T)
    for m in range(M):
        e = r[3 * m:3 * m + 3]
        wp[m] = weight_of((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], weight_type, sigma, T)   # :372-381
        wrow[3 * m:3 * m + 3] = wp[m]                                                     # :392
    return wrow, wp


def _update_seq(est, x, T):
    """UpdateGlobalRotations (:418-435)"""
    out = []
    for u in range(len(est)):
        R_ori = aa_to_rot(est[u], T)                                                      # :425-426
        out.append(rot_to_aa(mul3(R_ori, aa_to_rot(-x[3 * u:3 * u + 3], T)), T))          # :428-430
    return out


def _average_step(x, nr, T):
    """ComputeAverageStepSize (:485-499)"""
    total = T(0)
    for u in range(nr):
        v = x[3 * u:3 * u + 3]
        total += np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return total / T(nr)


def _finish(p, T, est, R, r, wp, trace, stop, extra=None):
    n, npairs, M = p["n"], p["npairs"], p["k"].size
    rot = np.array(p["rot0"], dtype=T); aa = np.zeros((n, 3), dtype=T)
    for u, i in enumerate(p["img"]):
        rot[i] = R[u]; aa[i] = est[u]
    residual = np.zeros((npairs, 3), dtype=T); weight = np.zeros(npairs, dtype=T)
    if M:
        residual[p["k"]] = np.asarray(r[:3 * M]).reshape(M, 3)
        if wp is not None:
            weight[p["k"]] = wp
    out = dict(rot=rot, angle_axis=aa, residual=residual, weight=weight, step_trace=np.array(trace, dtype=T), iters=len(trace), stop=stop,
               fixed=p["fixed"], pairs=M)
    out.update(extra or {})
    return out


def irls_sequential(g, T=np.float64, weight_type=GEMAN_MCCLURE, max_iters=100, threshold=1e-3, sigma_deg=5.0, fixed_image=-1):
    """SolveIRLS (:334-416) from the caller's rotations -> dict(rot, angle_axis, residual, weight, step_trace, iters, stop, ...)"""
    if weight_type not in (GEMAN_MCCLURE, HALF_NORM) or not (max_iters > 0) or not (0 < threshold < np.inf) or not (0 < sigma_deg < np.inf):
        raise Refused("options")
    p = problem(g, fixed_image)
    nr, M = p["img"].size, p["k"].size
    est = [rot_to_aa(p["rot0"][i].astype(T), T) for i in p["img"]]                        # :143-144
    if M == 0:
        return _finish(p, T, est, [p["rot0"][i].astype(T) for i in p["img"]], np.zeros(3, dtype=T), None, [], STOP_NOTHING)
    fixed0 = est[p["slot"][p["fixed"]]].copy()                                            # :150-156
    A = explicit_A(p, T)
    sigma = deg_to_rad(sigma_deg, T)                                                      # :344
    r, R = _residuals_seq(p, est, fixed0, T)                                              # :355
    trace, stop, wp_used = [], STOP_ITERATIONS, None
    for _ in range(max_iters):                                                            # :357
        wrow, wp = _weights_seq(p, r, weight_type, sigma, T)
        if not np.isfinite(wp.astype(np.float64)).all():                                  # rule 7 (:383-386 tests for NaN only)
            stop = STOP_NONFINITE
            break
        AtW = A.T * wrow                                                                  # :396
        x = cholesky_solve(AtW @ A, AtW @ r)                                              # :398-402
        est = _update_seq(est, x, T)                                                      # :403
        r, R = _residuals_seq(p, est, fixed0, T)                                          # :404
        wp_used = wp
        trace.append(_average_step(x, nr, T))
        if trace[-1] < T(threshold):                                                      # :407-411
            stop = STOP_STEP
            break
    return _finish(p, T, est, R, r, wp_used, trace, stop)


def stages_sequential(g, angle_axis, x, T=np.float64, weight_in=None, weight_type=GEMAN_MCCLURE, sigma_deg=5.0, fixed_image=-1):
    """what xm_view_graph_rotations_probe returns, by the functions of (a): the quantities of one iteration at the state angle_axis and the
    step x (n x 3 each)"""
    p = problem(g, fixed_image)
    n, npairs, nr, M = p["n"], p["npairs"], p["img"].size, p["k"].size
    est = [np.asarray(angle_axis, dtype=T).reshape(n, 3)[i] for i in p["img"]]
    xs = np.concatenate([np.asarray(x, dtype=T).reshape(n, 3)[i] for i in p["img"]])
    fixed0 = rot_to_aa(p["rot0"][p["fixed"]].astype(T), T)
    r, R = _residuals_seq(p, est, fixed0, T)
    wrow, wp = _weights_seq(p, r, weight_type, deg_to_rad(sigma_deg, T), T)
    w_out = wp.copy()
    if weight_in is not None:
        wp = np.asarray(weight_in, dtype=T)[p["k"]]
        wrow = np.concatenate([np.repeat(wp, 3), np.ones(3, dtype=T)])
    # A^T W r, the diagonal of A^T W A and (A^T W A) x row by row of A (:205-270), without forming the matrix (test_rotavg_numpy.py checks
    # explicit_A against this form)
    rhs = np.zeros(3 * nr, dtype=T); diag = np.zeros(nr, dtype=T); prod = np.zeros(3 * nr, dtype=T)
    f = p["slot"][p["fixed"]]
    for m in range(M):
        a, b = p["ca"][m], p["cb"][m]
        for i in range(3):
            row = wrow[3 * m + i] * r[3 * m + i]
            rhs[3 * a + i] -= row; rhs[3 * b + i] += row
            ax = wrow[3 * m + i] * (xs[3 * b + i] - xs[3 * a + i])
            prod[3 * a + i] -= ax; prod[3 * b + i] += ax
        diag[a] += wp[m]; diag[b] += wp[m]
    for i in range(3):
        rhs[3 * f + i] += r[3 * M + i]; prod[3 * f + i] += xs[3 * f + i]
    diag[f] += 1
    new = _update_seq(est, xs, T)
    out = dict(rot=np.zeros((n, 3, 3), dtype=T), residual=np.zeros((npairs, 3), dtype=T), gauge=r[3 * M:].copy(), weight=np.zeros(npairs, dtype=T),
               rhs=np.zeros((n, 3), dtype=T), diagonal=np.zeros(n, dtype=T), product=np.zeros((n, 3), dtype=T), angle_axis_out=np.zeros((n, 3), dtype=T),
               step=_average_step(xs, nr, T))
    out["residual"][p["k"]] = r[:3 * M].reshape(M, 3); out["weight"][p["k"]] = w_out
    for u, i in enumerate(p["img"]):
        out["rot"][i] = R[u]; out["rhs"][i] = rhs[3 * u:3 * u + 3]; out["diagonal"][i] = diag[u]
        out["product"][i] = prod[3 * u:3 * u + 3]; out["angle_axis_out"][i] = new[u]
    return out


# ------------------------------------------------------------------------------------------------ (b) the vectorised float64 contract
def exp_batch(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    n = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    big = n > AA_EPS
    nn = np.where(big, n, 1.0)
    u = a / nn[:, None]
    s, c = np.sin(n), np.cos(n)
    su = s[:, None] * u; cu = (1.0 - c)[:, None] * u
    R = np.empty((a.shape[0], 3, 3))
    t = cu[:, 0] * u[:, 1]; R[:, 0, 1] = t - su[:, 2]; R[:, 1, 0] = t + su[:, 2]
    t = cu[:, 0] * u[:, 2]; R[:, 0, 2] = t + su[:, 1]; R[:, 2, 0] = t - su[:, 1]
    t = cu[:, 1] * u[:, 2]; R[:, 1, 2] = t - su[:, 0]; R[:, 2, 1] = t + su[:, 0]
    for k in range(3):
        R[:, k, k] = cu[:, k] * u[:, k] + c
    F = np.empty_like(R)
    F[:, 0, 0] = 1; F[:, 1, 0] = a[:, 2]; F[:, 2, 0] = -a[:, 1]
    F[:, 0, 1] = -a[:, 2]; F[:, 1, 1] = 1; F[:, 2, 1] = a[:, 0]
    F[:, 0, 2] = a[:, 1]; F[:, 1, 2] = -a[:, 0]; F[:, 2, 2] = 1
    return np.where(big[:, None, None], R, F)


def log_batch(R):
    """rot_to_aa for many matrices: every branch is computed for every matrix and the one rule 4 takes is selected"""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    d = [R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]]
    tr = (d[0] + d[1]) + d[2]
    i = np.where(d[1] > d[0], 1, 0)
    i = np.where(d[2] > np.where(i == 1, d[1], d[0]), 2, i)
    q = np.zeros((R.shape[0], 4))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sqrt(tr + 1.0)
        f = 0.5 / t
        q0 = np.stack([(R[:, 2, 1] - R[:, 1, 2]) * f, (R[:, 0, 2] - R[:, 2, 0]) * f, (R[:, 1, 0] - R[:, 0, 1]) * f, 0.5 * t], axis=1)
        q = np.where((tr > 0)[:, None], q0, q)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            t = np.sqrt(((d[a] - d[b]) - d[c]) + 1.0)
            f = 0.5 / t
            qa = np.empty_like(q)
            qa[:, a] = 0.5 * t; qa[:, 3] = (R[:, c, b] - R[:, b, c]) * f
            qa[:, b] = (R[:, b, a] + R[:, a, b]) * f; qa[:, c] = (R[:, c, a] + R[:, a, c]) * f
            q = np.where(((tr <= 0) & (i == a))[:, None], qa, q)
        n = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        angle = 2.0 * np.arctan2(n, np.abs(q[:, 3]))
        sn = np.where(q[:, 3] < 0, -n, n)
        out = angle[:, None] * (q[:, :3] / sn[:, None])
    return np.where((n == 0)[:, None], 0.0, out)


def mul_batch(A, B):
    C = np.empty_like(A)
    for i in range(3):
        for j in range(3):
            C[:, i, j] = (A[:, i, 0] * B[:, 0, j] + A[:, i, 1] * B[:, 1, j]) + A[:, i, 2] * B[:, 2, j]
    return C


def pcg_contract(apply, b, dinv, tol2=PCG_TOL2, cap=PCG_CAP):
    """the device's PCG (xm_lm_shared.h) from zero -> x, iterations, capped"""
    x = np.zeros_like(b); r = b.copy(); z = dinv * r; p = z.copy()
    rz = float(r @ z); bb = float(b @ b); rr = bb; rzo = 0.0
    it = 0
    while True:
        if it > 0:
            q = rr / bb if bb > 0.0 else 0.0
            if q <= tol2:
                return x, it, False
            if it >= cap:
                return x, it, True
            beta = rz / rzo if rzo > 0.0 else 0.0
            p = z + beta * p
        Ap = apply(p)
        pap = float(p @ Ap)
        alpha = rz / pap if (pap > 0.0 and rz > 0.0) else 0.0
        x = x + alpha * p; r = r - alpha * Ap; z = dinv * r
        rzo = rz; rz = float(r @ z); rr = float(r @ r)
        it += 1


def irls_contract(g, weight_type=GEMAN_MCCLURE, max_iters=100, threshold=1e-3, sigma_deg=5.0, fixed_image=-1):
    """the device's rules in float64 (rules 5 to 10 vectorised, the camera sums in incidence order) -> as irls_sequential, and pcg_iters, pcg_capped,
    pcg_relres (per solve |b - A x| / |b| of what the PCG returned)"""
    if weight_type not in (GEMAN_MCCLURE, HALF_NORM) or not (max_iters > 0) or not (0 < threshold < np.inf) or not (0 < sigma_deg < np.inf):
        raise Refused("options")
    p = problem(g, fixed_image)
    T = np.float64
    nr, M = p["img"].size, p["k"].size
    est = log_batch(p["rot0"][p["img"]])
    if M == 0:
        return _finish(p, T, est, p["rot0"][p["img"]], np.zeros(3), None, [], STOP_NOTHING, dict(pcg_iters=0, pcg_capped=0, pcg_relres=[]))
    ca, cb, Rrel = p["ca"], p["cb"], p["Rrel"][p["k"]]
    f = int(p["slot"][p["fixed"]])
    R = exp_batch(est)
    Rf0 = R[f].copy()
    sigma = deg_to_rad(sigma_deg)
    sigma2 = sigma * sigma
    cams = np.stack([ca, cb], axis=1).reshape(-1)                     # a camera's incidences in input order

    def scatter(vals):
        """per camera the sum of its incidences' rows, added in input order"""
        return np.stack([np.bincount(cams, weights=vals[:, c], minlength=nr) for c in range(3)], axis=1)

    def evaluate(R):
        Q = mul_batch(np.transpose(R[cb], (0, 2, 1)), mul_batch(Rrel, R[ca]))
        r = -log_batch(Q)
        e2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        if weight_type == GEMAN_MCCLURE:
            tmp = e2 + sigma2
            w = sigma2 / (tmp * tmp)
        else:
            with np.errstate(divide="ignore"):
                w = np.power(e2, -0.75)
        return r, w

    r, w = evaluate(R)
    trace, stop, w_used, pcg_iters, pcg_capped, pcg_relres = [], STOP_ITERATIONS, None, 0, 0, []
    for _ in range(max_iters):
        if not np.isfinite(w).all():
            stop = STOP_NONFINITE
            break
        gauge = rot_to_aa(mul3(Rf0.T.copy(), R[f]))
        wr = w[:, None] * r
        b = scatter(np.stack([-wr, wr], axis=1).reshape(-1, 3))
        d = np.bincount(cams, weights=np.repeat(w, 2), minlength=nr)
        b[f] += gauge; d[f] += 1.0
        dinv = np.repeat(np.where(d > 0.0, 1.0 / np.where(d > 0.0, d, 1.0), 0.0), 3)

        def apply(v):
            v = v.reshape(nr, 3)
            dv = w[:, None] * (v[ca] - v[cb])
            o = scatter(np.stack([dv, -dv], axis=1).reshape(-1, 3))
            o[f] += v[f]
            return o.reshape(-1)
        x, it, capped = pcg_contract(apply, b.reshape(-1), dinv)
        pcg_iters += it; pcg_capped += int(capped)
        pcg_relres.append(float(np.linalg.norm(b.reshape(-1) - apply(x)) / np.linalg.norm(b)))
        x = x.reshape(nr, 3)
        est = log_batch(mul_batch(R, exp_batch(-x)))
        R = exp_batch(est)
        w_used = w
        r, w = evaluate(R)
        trace.append(float(np.sum(np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])) / nr))
        if trace[-1] < threshold:
            stop = STOP_STEP
            break
    return _finish(p, T, est, R, r.reshape(-1), w_used, trace, stop, dict(pcg_iters=pcg_iters, pcg_capped=pcg_capped, pcg_relres=pcg_relres))


# ------------------------------------------------------------------------------------------------ measures
def angle_deg(A, B):
    """angle of A^T B per matrix, in degrees"""
    c = (np.einsum("kab,kab->k", np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)) - 1.0) / 2.0
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def errors_deg(rot, truth, img=None):
    """rotation error per image against the truth after one world rotation G: angle(rot_i G, truth_i).  G is the chordal fit over all
    images, then twice over the images within three medians of it, so that a few images that are wrong as a group (the two SIMPLE2 images
    whose pairs are all spoiled) do not tilt the frame of the others"""
    rot = np.asarray(rot, dtype=np.float64); truth = np.asarray(truth, dtype=np.float64)
    if img is not None:
        rot, truth = rot[img], truth[img]
    keep = np.ones(rot.shape[0], dtype=bool)
    for _ in range(3):
        U, _, Vt = np.linalg.svd(np.einsum("kba,kbc->ac", rot[keep], truth[keep]))
        G = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
        e = angle_deg(rot @ G, truth)
        keep = e <= 3.0 * np.median(e) + 1e-9
    return e


def call_inputs(g):
    """the arguments of xmamd.view_graph_rotations and of its probe"""
    return dict(rot0=g["rot0"], pi=g["pi"], pj=g["pj"], Rrel=g["Rrel"], registered=g.get("registered"), valid_in=g.get("valid_in"))


# ------------------------------------------------------------------------------------------------ generators
def random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def chordal_start(n, pi, pj, Rrel, anchor):
    """the chordal least-squares rotations of the pairs (R_j = Rrel R_i): the three smallest eigenvectors of the block Laplacian, every
    block projected onto SO(3), camera 0 turned onto `anchor`"""
    Mx = np.zeros((3 * n, 3 * n))
    for i, j, Q in zip(pi, pj, Rrel):
        Mx[3 * j:3 * j + 3, 3 * j:3 * j + 3] += np.eye(3); Mx[3 * i:3 * i + 3, 3 * i:3 * i + 3] += np.eye(3)
        Mx[3 * j:3 * j + 3, 3 * i:3 * i + 3] -= Q; Mx[3 * i:3 * i + 3, 3 * j:3 * j + 3] -= Q.T
    _, V = np.linalg.eigh(Mx)
    V = V[:, :3]
    if sum(np.linalg.det(V[3 * i:3 * i + 3]) for i in range(n)) < 0:
        V = -V
    R = np.empty((n, 3, 3))
    for i in range(n):
        U, _, Vt = np.linalg.svd(V[3 * i:3 * i + 3])
        R[i] = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    return R @ (R[0].T @ anchor)


def build_graph(n, pairs, clean, seed, noise_deg=1.0, outliers=0.0, start="chordal"):
    """pairs: (i, j) tuples; clean: a mask of pairs that keep their relative rotation (up to the noise).  Of the others a share `outliers`
    gets a random rotation.  -> dict(rot0, pi, pj, Rrel, truth, wrong, registered=None, valid_in=None)"""
    rng = np.random.default_rng(seed)
    truth = np.stack([random_rotation(rng) for _ in range(n)])
    pi = np.array([p[0] for p in pairs], dtype=np.int32); pj = np.array([p[1] for p in pairs], dtype=np.int32)
    K = pi.size
    Rrel = np.empty((K, 3, 3))
    for k in range(K):
        noise = rng.standard_normal(3) * np.radians(noise_deg) / np.sqrt(3.0)
        Rrel[k] = aa_to_rot(noise) @ truth[pj[k]] @ truth[pi[k]].T
    free = np.flatnonzero(~np.asarray(clean, dtype=bool))
    wrong = np.zeros(K, dtype=bool)
    wrong[rng.choice(free, int(round(outliers * free.size)), replace=False)] = True
    for k in np.flatnonzero(wrong):
        Rrel[k] = random_rotation(rng)
    rot0 = chordal_start(n, pi, pj, Rrel, truth[0]) if start == "chordal" else truth.copy()
    return dict(rot0=np.ascontiguousarray(rot0), pi=pi, pj=pj, Rrel=np.ascontiguousarray(Rrel), truth=truth, wrong=wrong, registered=None, valid_in=None)


def make_graph(n, npairs, seed, noise_deg=1.0, outliers=0.0, start="chordal"):
    """n cameras, a spanning chain (i, i + 1) kept clean, npairs - (n - 1) other pairs drawn without repetition in a random orientation"""
    rng = np.random.default_rng(1000 + seed)
    pairs = [(i, i + 1) for i in range(n - 1)]
    have = set(pairs)
    while len(pairs) < npairs:
        i, j = rng.choice(n, 2, replace=False).tolist()
        if (min(i, j), max(i, j)) in have:
            continue
        have.add((min(i, j), max(i, j)))
        pairs.append((i, j))
    clean = np.arange(len(pairs)) < n - 1
    return build_graph(n, pairs, clean, seed, noise_deg, outliers, start)


def chain(n, seed, noise_deg=1.0):
    """n cameras in one chain (i, i + 1), all pairs clean, from the true rotations: a Laplacian whose condition grows with n^2, so that from
    600 cameras on the PCG runs into its cap"""
    return build_graph(n, [(i, i + 1) for i in range(n - 1)], np.ones(n - 1, dtype=bool), seed, noise_deg, 0.0, start="truth")


def star(leaves, seed, noise_deg=1.0, start="chordal"):
    """camera 0 in every pair, `leaves` other cameras with one pair each (in alternating orientation): incidence counts `leaves` and 1"""
    pairs = [(0, j) if j % 2 else (j, 0) for j in range(1, leaves + 1)]
    return build_graph(leaves + 1, pairs, np.ones(leaves, dtype=bool), seed, noise_deg, 0.0, start)


def star_ring(hub, seed, noise_deg=1.0, outliers=0.0):
    """camera 0 in `hub` pairs, the other cameras in a ring with its second neighbours (five pairs per camera, so that one wrong pair does
    not cost a camera its start): clean are the ring's chain 1 .. hub and the pair (0, 1); outliers among the rest (the star's other pairs,
    the ring's closing pair and the second neighbours)"""
    ring = lambda j: 1 + (j - 1) % hub
    pairs = [(0, j) if j % 2 else (j, 0) for j in range(1, hub + 1)] + [(j, j + 1) for j in range(1, hub)] + [(hub, 1)] + \
            [(j, ring(j + 2)) for j in range(1, hub + 1)]
    clean = np.zeros(len(pairs), dtype=bool)
    clean[0] = True; clean[hub:2 * hub - 1] = True
    return build_graph(hub + 1, pairs, clean, seed, noise_deg, outliers)


_SIMPLE2 = None


def simple2_graph():
    """the SIMPLE2-derived view graph of xm_viewgraph_numpy.simple2_case() with its spoiled pairs, after pass A (the numpy contract's): all
    listed pairs, valid_in and registered as pass A left them, the start from the chordal least-squares solve over the valid pairs.
    -> the graph; g["case"], g["passA"]: the case and pass A's result for a pass B (xm_viewgraph_numpy.next_pass)"""
    global _SIMPLE2
    if _SIMPLE2 is None:
        import xm_viewgraph_numpy as vn
        c = vn.simple2_case()
        A = vn.run_numpy(c)
        valid = (A["pair_status"] == vn.VALID)
        reg = A["registered"] != 0
        n = reg.size
        img = np.flatnonzero(reg)
        index = np.full(n, -1); index[img] = np.arange(img.size)
        k = np.flatnonzero(valid & reg[c["pi"]] & reg[c["pj"]])
        truth = c["rot_true"]
        rot0 = np.tile(np.eye(3), (n, 1, 1))
        rot0[img] = chordal_start(img.size, index[c["pi"][k]], index[c["pj"][k]], c["Rrel"][k], truth[img[0]])
        _SIMPLE2 = dict(rot0=rot0, pi=c["pi"], pj=c["pj"], Rrel=c["Rrel"], truth=truth, registered=reg.astype(np.uint8), valid_in=valid.astype(np.uint8),
                        case=c, passA=A)
    return dict(_SIMPLE2)
