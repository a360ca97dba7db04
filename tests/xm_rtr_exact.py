"""The quantities of the Riemannian trust region on St(3,o)^n x R+^(n-1), stage by stage, restated in plain numpy from the reference's
trustregion.h and checkeig.h (line numbers in the comments).  Every function is written once over a dtype: dt = np.longdouble gives the
reference the GPU stage tests compare with (tests/test_gpu_rtr_stages.py), dt = np.float64 the restatement whose own error against it sets
their bound (xm_rtr_stages.py).  Imports nothing from the library or the oracle.

Layout: R is 3n x o (camera i = rows 3i..3i+2, orthonormal rows), s is n with s[0] = 1 (the anchor, trustregion.h:125-127); a tangent
vector is (pR, ps) with sym(R_i pR_i^T) = 0 and ps[0] = 0; the metric is <u, v> = sum(uR vR) + sum(us vs / s^2) (ProductManifoldInner with
the scale parts divided by s, trustregion.h:565-566, 625-626).

Next to every array the functions return, under the key "<name>~", the magnitude of the terms its blocks are formed from (per camera, or
a scalar): the products' terms are bounded through |Q| |W|, and what is built from them inherits that.  An error is judged against the larger of
the exact block's maximum and this magnitude -- at a critical point, where the exact gradient is 0, the first alone would compare one round-off
with another.

damage= (f64 runs of tests/test_rtr_exact.py only) plants one deliberate fault; the names are those of FAULTS and, for the certificate's
eigen-solver, LZ_FAULTS."""
import numpy as np

LD = np.longdouble
FAULTS = ("no_S0", "no_ps_s_egs", "anchor_egs", "anchor_rhs", "anchor_ps", "nosym", "lam_s2", "rr_est_no_cross", "tau_root", "vp_no_beta", "lam5",
          "dz_row") + ("m_no_scale", "m_metric_s", "anchor_scale", "mgs_raw_row", "rou_sign", "double_any")
# a fault that changes no output, kept apart: `f > loss` dropped from the reject test of trustregion.h:702.  With m < 0 (the only way to the test)
# f > loss makes rou = (f - loss) / m negative (or -0), so rou < 0.1 rejects as well; tests/test_rtr_exact.py pins that over a grid.
EQUIVALENT_FAULTS = ("no_f_gt_loss",)
MAX_INNER = 1000   # trustregion.h:416
PH_TCG, PH_CAND, PH_STOP, PH_INIT = 0, 1, 2, 3   # what a (product, step) pair of the device-driven outer iteration does (xm_common.h: Phase)


class Op:
    """W -> Q W for a dense matrix, in any dtype; absolute() is the same for |Q| (the magnitude of the product's terms)"""

    def __init__(self, Q):
        self.Q = np.asarray(Q)
        self._cache = {}

    def _as(self, dt, absolute=False):
        key = (np.dtype(dt).name, absolute)
        if key not in self._cache:
            M = self.Q.astype(dt)
            self._cache[key] = np.abs(M) if absolute else M
        return self._cache[key]

    def __call__(self, W, dt):
        return self._as(dt) @ W.astype(dt)

    def absolute(self, W, dt):
        return self._as(dt, True) @ np.abs(W).astype(dt)


class BlockOp:
    """the same for a 3x3-block CSR matrix (rows too many to densify)"""

    def __init__(self, rowptr, colidx, blocks):
        self.rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
        self.cols = np.asarray(colidx, dtype=np.int64)
        self.blocks = np.asarray(blocks).reshape(-1, 3, 3)
        self.n = len(rowptr) - 1

    def _apply(self, B, W, dt):
        Wb = W.astype(dt).reshape(self.n, 3, -1)
        out = np.zeros(Wb.shape, dtype=dt)
        np.add.at(out, self.rows, np.einsum("bac,bck->bak", B.astype(dt), Wb[self.cols]))
        return out.reshape(W.shape)

    def __call__(self, W, dt):
        return self._apply(self.blocks, W, dt)

    def absolute(self, W, dt):
        return self._apply(np.abs(self.blocks), np.abs(W), dt)


def blk(A, n):
    return A.reshape(n, 3, -1)


def sym3(M):
    return (M + np.swapaxes(M, 1, 2)) / 2


def inner(uR, us, vR, vs, s):
    """the product metric: trustregion.h:565-566 (ProductManifoldInner with one scale part over s^2)"""
    return (uR * vR).sum() + (us * vs / (s * s)).sum()


def tangent(R, Z, zs):
    """projection of (Z, zs) onto the tangent space at R (trustregion.h:307-317 without the metric factor of the scale part), anchor masked"""
    n = R.shape[0] // 3
    Rb, Zb = blk(R, n), blk(Z, n)
    P = Zb - np.einsum("iab,ibk->iak", sym3(np.einsum("iak,ibk->iab", Rb, Zb)), Rb)
    ps = np.array(zs, dtype=Z.dtype)
    ps[0] = 0
    return P.reshape(R.shape), ps


def point(R, s, dt):
    R = np.asarray(R).astype(dt)
    s = np.asarray(s).astype(dt).copy()
    s[0] = 1                                               # trustregion.h:125-127
    return R, s


def cost(op, R, s, lam, dt=LD):
    """objc, trustregion.h:162-170: <sR, Q sR> + lam sum_{i>=1} (s_i^2 - 1)^2"""
    R, s = point(R, s, dt)
    sR = R * np.repeat(s, 3)[:, None]
    q = s[1:] * s[1:] - 1
    return (sR * op(sR, dt)).sum() + dt(lam) * (q * q).sum()


def grad_stage(op, R, s, lam, dt=LD, damage=None):
    """objc :162-170, grad :186-194, projection :307-317; rr = <rg, rg> (:483-484)"""
    R, s = point(R, s, dt)
    n, lam = s.size, dt(lam)
    s3 = np.repeat(s, 3)[:, None]
    sR = R * s3
    G = 2 * op(sR, dt)                                     # dfdsR, :187
    aG = 2 * op.absolute(sR, dt)
    q = s * s - 1
    anchor = np.arange(n) == 0
    f = (G * sR).sum() / 2 + lam * (q[1:] * q[1:]).sum()
    af = (aG * np.abs(sR)).sum() / 2 + lam * (q[1:] * q[1:]).sum()
    Rb, Gb, aGb = blk(R, n), blk(G, n), blk(aG, n)
    lamterm = 4 * lam * q * s                              # GradLambdaKernal + :191-192
    egs = (Gb * Rb).sum(axis=(1, 2)) + lamterm             # :189
    aegs = (aGb * np.abs(Rb)).sum(axis=(1, 2)) + np.abs(lamterm)
    if damage != "anchor_egs":
        egs = np.where(anchor, 0, egs)
    aegs = np.where(anchor, 0, aegs)
    eg = Gb * s[:, None, None]                             # grad_r, :188
    aeg = (aGb * s[:, None, None]).max(axis=(1, 2))
    M = np.einsum("iak,ibk->iab", Rb, eg)                  # :310
    S0 = M if damage == "nosym" else sym3(M)               # :311
    rgR = eg - np.einsum("iab,ibk->iak", S0, Rb)           # :312-314
    rgs = egs * s * s                                      # :315
    rr = (rgR * rgR).sum() + ((rgs / s) ** 2).sum()
    o = R.shape[1]
    arr = (3 * o * aeg * aeg).sum() + ((aegs * s) ** 2).sum()
    return {"f": f, "f~": af, "rr": rr, "rr~": arr, "G": Gb, "G~": aGb.max(axis=(1, 2)), "egs": egs, "egs~": aegs, "S0": S0, "S0~": aeg,
            "rgR": rgR, "rgR~": aeg, "rgs": rgs, "rgs~": aegs * s * s, "_aG": aGb, "_R": Rb, "_s": s}


def hess_stage(op, g, pR, ps, rR, rs, lam, dt=LD, damage=None):
    """ehess :227-255, ehess2rhess :277-295 at the point of the gradient stage g (op: the operator of the Hessian products, which the fp32 option
    rounds to fp32; G, egs, S0 come from g), and the three inner products the truncated CG takes from it (:565-566, :625-626)"""
    Rb, s = g["_R"], g["_s"]
    n, lam = s.size, dt(lam)
    anchor = np.arange(n) == 0
    Pb, rb = blk(np.asarray(pR).astype(dt), n), blk(np.asarray(rR).astype(dt), n)
    ps, rs = np.asarray(ps).astype(dt).copy(), np.asarray(rs).astype(dt).copy()
    pse = ps.copy()                                        # the scale part as the epilogue sees it: a direction is given with anything at the anchor
    ps[0] = 0                                              # su_ex = [0; su], :204
    rs[0] = 0
    if damage != "anchor_ps":
        pse[0] = 0
    G, aG, egs = g["G"].astype(dt), g["_aG"].astype(dt), g["egs"].astype(dt)
    W = Pb * s[:, None, None] + Rb * ps[:, None, None]     # sRu + suR, :229-234
    aW = np.abs(Pb) * s[:, None, None] + np.abs(Rb) * np.abs(ps)[:, None, None]
    h = blk(2 * op(W.reshape(3 * n, -1), dt), n)           # CsRu, :237
    ah = blk(2 * op.absolute(aW.reshape(3 * n, -1), dt), n)
    c = (s * s - 1) if damage == "lam_s2" else (3 * s * s - 1)
    lamterm = 4 * lam * c * ps                             # HessLambdaKernal, :250-254
    hs = (h * Rb).sum(axis=(1, 2)) + (G * Pb).sum(axis=(1, 2)) + lamterm   # :244-248
    ahs = (ah * np.abs(Rb)).sum(axis=(1, 2)) + (aG * np.abs(Pb)).sum(axis=(1, 2)) + np.abs(lamterm)
    if damage != "anchor_rhs":
        hs = np.where(anchor, 0, hs)
    eh = h * s[:, None, None] + G * pse[:, None, None]     # hr = sCsRu + suCsR, :238-242
    aeh = (ah * s[:, None, None] + aG * np.abs(ps)[:, None, None]).max(axis=(1, 2))
    S0 = g["S0"].astype(dt)
    aS0 = g["S0~"].astype(dt)
    rh = eh if damage == "no_S0" else eh - np.einsum("iab,ibk->iak", S0, Pb)   # :279-283
    M = np.einsum("iak,ibk->iab", Rb, rh)                  # :285
    S1 = M if damage == "nosym" else sym3(M)               # :286
    HpR = rh - np.einsum("iab,ibk->iak", S1, Rb)           # :287
    aHpR = aeh + 3 * aS0 * np.abs(Pb).max(axis=(1, 2))
    Hps = hs * s * s                                       # :288
    if damage != "no_ps_s_egs":
        Hps = Hps + ps * s * egs                           # :289-293
    aHps = ahs * s * s + np.abs(ps) * s * g["egs~"].astype(dt)
    if damage != "anchor_rhs":
        Hps = np.where(anchor, 0, Hps)
    aHps = np.where(anchor, 0, aHps)
    o = Rb.shape[2]
    pHp = (Pb * HpR).sum() + (ps * Hps / (s * s)).sum()
    rHp = (rb * HpR).sum() + (rs * Hps / (s * s)).sum()
    HpHp = (HpR * HpR).sum() + ((Hps / s) ** 2).sum()
    apHp = (np.abs(Pb).sum(axis=(1, 2)) * aHpR).sum() + (np.abs(ps) * aHps / (s * s)).sum()
    arHp = (np.abs(rb).sum(axis=(1, 2)) * aHpR).sum() + (np.abs(rs) * aHps / (s * s)).sum()
    aHH = (3 * o * aHpR * aHpR).sum() + ((aHps / s) ** 2).sum()
    return {"HpR": HpR, "HpR~": aHpR, "Hps": Hps, "Hps~": aHps, "pHp": pHp, "pHp~": apHp, "rHp": rHp, "rHp~": arHp, "HpHp": HpHp, "HpHp~": aHH,
            "W": W, "W~": aW.max(axis=(1, 2))}


def tcg_init_stage(g, delta, dt=LD):
    """start of the truncated CG, trustregion.h:454-458, 476-485: r = rg, p = -rg, v = Hv = 0, the first product input (:229-234)"""
    Rb, s = g["_R"], g["_s"]
    rR, rs = g["rgR"].astype(dt), g["rgs"].astype(dt)
    z, zs = np.zeros(rR.shape, dtype=dt), np.zeros(rs.shape, dtype=dt)
    W = -rR * s[:, None, None] + Rb * (-rs)[:, None, None]
    rr = dt(g["rr"])
    scal = dict(rr=rr, vv=dt(0), vp=dt(0), pp=rr, delta=dt(delta), gradnorm=np.sqrt(rr), last_step=dt(0), model=dt(0), status=0, iter=0)
    return {"rR": rR, "rs": rs, "pR": -rR, "ps": -rs, "vR": z, "vs": zs, "HvR": z, "Hvs": zs, "W": W, "scal": scal}


def cg_step_stage(sc, sums, Hp, p, r, v, Hv, R, s, dt=LD, damage=None, model_rec=False, pHp_scale=None):
    """one iteration of the truncated CG's body, trustregion.h:565-644, from its scalar state sc (rr, vv, vp, pp, delta, gradnorm, model, iter),
    sums = (<p,Hp>, <r,Hp>, <Hp,Hp>, |r|^2 as summed by the previous iteration or None at iter 0) and the vectors.  The residual norm after
    the step is the expansion <r,r> + 2 step <r,Hp> + step^2 <Hp,Hp> of :626; the model value follows m -= step <r,r> - step^2 <p,Hp> / 2.
    Returns the outputs, the branch taken and, under "margins", the relative distance of every comparison a branch depends on (the sign of
    alpha is the sign of <p,Hp>: judged against pHp_scale, the magnitude of that sum's terms)."""
    R, s = point(R, s, dt)
    n = s.size
    Rb = blk(R, n)
    cv = lambda a: np.asarray(a).astype(dt)
    HpR, Hps, pR, ps, rR, rs, vR, vs = blk(cv(Hp[0]), n), cv(Hp[1]), blk(cv(p[0]), n), cv(p[1]), blk(cv(r[0]), n), cv(r[1]), blk(cv(v[0]), n), cv(v[1])
    HvR, Hvs = (None, None) if model_rec else (blk(cv(Hv[0]), n), cv(Hv[1]))
    pHp, rHp, HpHp = (dt(x) for x in sums[:3])
    rr = dt(sc["rr"]) if sc["iter"] == 0 else dt(sums[3])
    vv, vp, pp, delta, gradnorm, model = (dt(sc[k]) for k in ("vv", "vp", "pp", "delta", "gradnorm", "model"))
    out = dict(vR=vR, vs=vs, HvR=HvR, Hvs=Hvs, rR=rR, rs=rs, pR=pR, ps=ps, W=None, rr_parts=None)
    bmax = lambda a: np.abs(a).max(axis=(1, 2))
    nx = dict(rr=rr, vv=vv, vp=vp, pp=pp, delta=delta, gradnorm=gradnorm, last_step=dt(0), model=model, status=0, iter=int(sc["iter"]))
    rel = lambda a, b: float(abs(a - b) / max(abs(a), abs(b))) if max(abs(a), abs(b)) > 0 else 0.0
    margins = {"rr<1e-15": rel(rr, dt(1e-15))}
    if rr < dt(1e-15):                                     # :572-576
        nx["status"] = 5
        return dict(out, scal=nx, branch=5, margins=margins, step=dt(0))
    alpha = rr / pHp                                       # :566
    margins["alpha>0"] = float(abs(pHp) / max(abs(pHp), dt(pHp_scale or 0)))
    vnew2 = vv + 2 * alpha * vp + alpha * alpha * pp       # :589
    neg = alpha <= 0                                       # :577
    if not neg:
        margins["inside"] = rel(vnew2, delta * delta)
    boundary = neg or vnew2 > delta * delta
    if boundary:                                           # :578-579, 590-591
        sq = np.sqrt(vp * vp + pp * (delta * delta - vv))
        step = ((-vp - sq) if damage == "tau_root" else (-vp + sq)) / pp
    else:
        step = alpha
    nx["last_step"] = step
    if model_rec:
        nx["model"] = model - step * rr + step * step * pHp / 2
    out["vR"], out["vs"] = vR + step * pR, vs + step * ps                         # :582-583, 594-595, 605-606
    out["vR~"], out["vs~"] = bmax(vR) + abs(step) * bmax(pR), np.abs(vs) + abs(step) * np.abs(ps)
    out["model~"] = abs(model) + abs(step * rr) + abs(step * step * pHp / 2)
    if not model_rec:
        out["HvR"], out["Hvs"] = HvR + step * HpR, Hvs + step * Hps               # :584-585, 596-597, 609-610
        out["HvR~"], out["Hvs~"] = bmax(HvR) + abs(step) * bmax(HpR), np.abs(Hvs) + abs(step) * np.abs(Hps)
    if boundary:
        nx["status"] = 1 if neg else 2                     # :586, 598
        return dict(out, scal=nx, branch=nx["status"], margins=margins, step=step)
    rRn, rsn = rR + step * HpR, rs + step * Hps            # :607-608
    out["rR"], out["rs"] = rRn, rsn
    out["rR~"], out["rs~"] = bmax(rR) + abs(step) * bmax(HpR), np.abs(rs) + abs(step) * np.abs(Hps)
    out.update({"rr~": rr + abs(2 * step * rHp) + step * step * HpHp, "vv~": vv + abs(2 * alpha * vp) + alpha * alpha * pp})
    out["rr_parts"] = (rRn * rRn).sum() + ((rsn / s) ** 2).sum()                  # :625-626, summed directly: <r,r> of the next iteration
    rr_est = rr + step * step * HpHp
    if damage != "rr_est_no_cross":
        rr_est = rr_est + 2 * step * rHp
    rr_est = max(rr_est, dt(0))
    stop = gradnorm * min(gradnorm, dt(0.1))               # :627
    margins["converged"] = rel(np.sqrt(rr_est), stop)
    beta = rr_est / rr                                     # :634
    nx["rr"] = rr_est
    nx["vv"] = vnew2                                       # :642
    nx["vp"] = (vp + step * pp) if damage == "vp_no_beta" else beta * (vp + step * pp)   # :643
    nx["pp"] = beta * beta * pp + rr_est                   # :644
    out["vp~"] = beta * (abs(vp) + abs(step) * pp)
    if np.sqrt(rr_est) < stop:
        nx["status"] = 3                                   # :628
        return dict(out, scal=nx, branch=3, margins=margins, step=step)
    pRn, psn = beta * pR - rRn, beta * ps - rsn            # :635-638
    out["pR"], out["ps"] = pRn, psn
    out["pR~"], out["ps~"] = beta * bmax(pR) + out["rR~"], beta * np.abs(ps) + out["rs~"]
    out["W~"] = out["pR~"] * s + out["ps~"]
    out["W"] = pRn * s[:, None, None] + Rb * psn[:, None, None]                   # the next :229-234
    nx["iter"] = int(sc["iter"]) + 1
    nx["status"] = 6 if nx["iter"] >= MAX_INNER else 0     # :559
    return dict(out, scal=nx, branch=nx["status"], margins=margins, step=step)


def gj_solve(N, b):
    """N y = b for a batch of small SPD systems, Gauss-Jordan without pivoting (N = <A_g B, A_h B> with B B^T = s^2 I: near diagonal)"""
    N, b = N.copy(), b.copy()
    m = N.shape[1]
    for c in range(m):
        d = N[:, c, c].copy()
        N[:, c, :] /= d[:, None]
        b[:, c] /= d
        for r in range(m):
            if r != c:
                f = N[:, r, c].copy()
                N[:, r, :] -= f[:, None] * N[:, c, :]
                b[:, r] -= f * b[:, c]
    return b


def generators(anchor, dt):
    """constraint matrices of one camera, checkeig.h:71-98 (anchor: the six symmetric unit matrices) and :100-161 (the others: two traceless
    diagonal and three off-diagonal ones)"""
    E = lambda a, b: np.outer(np.eye(3)[a], np.eye(3)[b]).astype(dt)
    h = dt(1) / 2
    if anchor:
        return np.stack([E(0, 0), h * (E(0, 1) + E(1, 0)), h * (E(0, 2) + E(2, 0)), E(1, 1), h * (E(1, 2) + E(2, 1)), E(2, 2)])
    return np.stack([h * (E(0, 0) - E(1, 1)), h * (E(1, 1) - E(2, 2)), h * (E(0, 1) + E(1, 0)), h * (E(0, 2) + E(2, 0)), h * (E(1, 2) + E(2, 1))])


def cert_stage(op, R, s, lam, X=None, dt=LD, damage=None):
    """the dual certificate's multipliers and operator, checkeig.h:56-368: Z = Q + 2 lam (|row 3i of sR|^2 - 1) on the diagonal entries 3i
    (:173-182), y = least squares of [A_g sR] y = Z sR camera by camera (:190-214; the columns of different cameras are orthogonal), Lam_i =
    sum y_g A_g (:263-299), dual = y0 + y3 + y5 + lam sum(1 - xii^2) (:322-332), and S X = Z X - Lam X"""
    R, s = point(R, s, dt)
    n, lam = s.size, dt(lam)
    sR = R * np.repeat(s, 3)[:, None]
    B = blk(sR, n)
    row = 1 if damage == "dz_row" else 0
    xii = (B[:, 0, :] ** 2).sum(axis=1)                    # :324-329
    dz = 2 * lam * (xii - 1)
    adz = 2 * lam * (xii + 1)
    Right = blk(op(sR, dt), n).copy()                      # :181-182
    aRight = blk(op.absolute(sR, dt), n).copy()
    Right[:, row, :] += dz[:, None] * B[:, row, :]
    aRight[:, 0, :] += adz[:, None] * np.abs(B[:, 0, :])
    Lam = np.zeros((n, 3, 3), dtype=dt)
    Mm = np.einsum("iak,ibk->iab", Right, B)
    Pm = np.einsum("iak,ibk->iab", B, B)
    y_anchor = None
    for anchor in (True, False):
        idx = np.array([0]) if anchor else np.arange(1, n)
        if idx.size == 0:
            continue
        A = generators(anchor and damage != "lam5", dt)
        rhs = np.einsum("gab,iab->ig", A, Mm[idx])
        N = np.einsum("gab,ibc,hac->igh", A, Pm[idx], A)
        y = gj_solve(N, rhs)
        Lam[idx] = np.einsum("ig,gab->iab", y, A)
        if anchor:
            y_anchor = y[0]
    aLam = aRight.max(axis=(1, 2)) / s
    if damage == "lam5":
        dual0 = dt(0)
    else:
        dual0 = y_anchor[0] + y_anchor[3] + y_anchor[5]     # :322
    dual1 = lam * (1 - xii * xii).sum()                    # :330-332
    out = {"Lam": Lam, "Lam~": aLam, "dz": dz, "dz~": adz, "dual0": dual0, "dual0~": 3 * aLam[0], "dual1": dual1, "dual1~": lam * (1 + xii * xii).sum()}
    if X is not None:
        out.update(cert_operator(op, out, X, dt, damage))
    return out


def cert_operator(op, C, X, dt=LD, damage=None):
    """S X = Z X - Lam X (checkeig.h:303-318) from the multipliers C = cert_stage(...) of the point"""
    Lam, dz, adz, aLam = C["Lam"].astype(dt), C["dz"].astype(dt), C["dz~"].astype(dt), C["Lam~"].astype(dt)
    n = dz.size
    row = 1 if damage == "dz_row" else 0
    X = np.asarray(X).astype(dt)
    Xb = blk(X, n)
    SX = blk(op(X, dt), n) - np.einsum("iab,ibk->iak", Lam, Xb)
    SX[:, row, :] += dz[:, None] * Xb[:, row, :]
    aSX = blk(op.absolute(X, dt), n).max(axis=(1, 2)) + adz * np.abs(Xb[:, 0, :]).max(axis=1) + 3 * aLam * np.abs(Xb).max(axis=(1, 2))
    return {"SX": SX, "SX~": aSX}


# ---------------------------------------------------------------------------------------------------------------- the certificate's eigen-solver
# Context::lanczos_min restated: Lanczos on S with two classical Gram-Schmidt passes against every earlier column, the smallest eigenpair of the
# tridiagonal matrix by Sturm bisection and inverse iteration, restart cycles from the Ritz vector.  Vectors are in global camera order throughout
# (the device keeps them in the partition's position order, which is the same on one rank).
LZ_FAULTS = ("lz_no_pass2", "lz_skip_last", "lz_alpha_pass1", "lz_beta_no_sqrt", "lz_drop_segment", "lz_y_reversed", "lz_no_unmap")
LZ_STEP_KEYS = ("c1", "c2", "alpha", "beta", "w")


def lanczos_start(n):
    """the start vector, bit for bit: a 64-bit linear congruential generator drawn in global order, 53 bits each, minus 1/2, the squares summed in
    order, every entry divided by the root of the sum (all in f64, whatever dtype the run continues in)"""
    state, mask = 0x9E3779B97F4A7C15, (1 << 64) - 1
    v = np.empty(3 * n)
    for i in range(3 * n):
        state = (state * 6364136223846793005 + 1442695040888963407) & mask
        v[i] = (state >> 11) / 9007199254740992.0 - 0.5
    return v / np.sqrt(np.cumsum(v * v)[-1])               # (cumsum adds in order; sum would add pairwise)


def dots_segments(length):
    """(segments, elements per segment) of a dot product over `length` elements: dots_multi_segments and the launchers' segment length"""
    nseg = min(64, max(1, length // 4096))
    return nseg, (-(-length // nseg) + 255) // 256 * 256


def lanczos_step(op, C, V, dt=LD, damage=None, length=None, scales=True):
    """one step from the columns V[:, 0..j] as given (3n x (j + 1)): w = S v_j, two classical Gram-Schmidt passes against all j + 1 columns with the
    coefficients c1 and c2, alpha_j = c1[j] + c2[j], beta_j = |w|; w is returned un-normalised (n x 3).  Magnitudes: S v_j's from cert_operator
    (per camera) for w; that, summed through |V|, for the coefficients and alpha; its 2-norm for beta.  length: elements of the device's vectors
    (3n rounded up; only the fault "one segment's terms dropped" reads it)"""
    V = np.asarray(V).astype(dt, copy=False)
    j, n = V.shape[1] - 1, C["dz"].size
    o = cert_operator(op, C, V[:, j:j + 1], dt)
    w, a3 = o["SX"].reshape(-1), np.repeat(o["SX~"], 3)
    keep = np.ones(3 * n, dtype=bool)
    if damage == "lz_drop_segment":                        # in every dot product of the step, as a fault of their kernel would; a vector of one segment is left alone
        nseg, seg = dots_segments(length or -(-3 * n // 128) * 128)
        if nseg > 1:
            keep[(nseg - 1) * seg:] = False                # the last segment that holds anything (the short one)
    cols = slice(0, j) if damage == "lz_skip_last" else slice(0, j + 1)
    c1 = V.T @ np.where(keep, w, 0)
    w = w - V[:, cols] @ c1[cols]
    if damage == "lz_no_pass2":
        c2 = np.zeros(j + 1, dtype=dt)
    else:
        c2 = V.T @ np.where(keep, w, 0)
        w = w - V[:, cols] @ c2[cols]
    alpha = c1[j] if damage == "lz_alpha_pass1" else c1[j] + c2[j]
    ww = w @ np.where(keep, w, 0)
    beta = ww if damage == "lz_beta_no_sqrt" else np.sqrt(ww)
    ac = np.abs(V).T @ a3 if scales else np.zeros(j + 1, dtype=dt)
    return {"w": w.reshape(n, 3), "w~": o["SX~"], "c1": c1, "c1~": ac, "c2": c2, "c2~": ac, "alpha": alpha, "alpha~": ac[j], "beta": beta,
            "beta~": np.sqrt(a3 @ a3)}


def sturm_count(a, b, x):
    """eigenvalues below x of the tridiagonal matrix (diagonal a, off-diagonal b)"""
    d = a[0] - x
    cnt = int(d < 0)
    for i in range(1, len(a)):
        if d == 0:
            d = type(d)(1e-300)
        d = (a[i] - x) - b[i - 1] * b[i - 1] / d
        cnt += int(d < 0)
    return cnt


def tridiag_bounds(a, b):
    """Gershgorin interval of the tridiagonal matrix and tmax = the larger of its ends' magnitudes"""
    a, b = np.asarray(a), np.asarray(b)[:len(a) - 1]
    r = np.zeros(len(a), dtype=a.dtype)
    r[:-1] += np.abs(b)
    r[1:] += np.abs(b)
    lo, hi = (a - r).min(), (a + r).max()
    return lo, hi, max(abs(lo), abs(hi))


def tridiag_min(a, b, dt=LD):
    """tridiag_min of xm_solver.hip restated over a dtype: bisection on the Sturm count down to an interval of 4e-16 max(1, tmax), its midpoint
    theta, then three rounds of inverse iteration with the shift theta - 1e-14 max(1, tmax) from the constant vector (here through a dense solve
    in place of the pivoted tridiagonal elimination: the same equations).  -> theta, y (unit norm), tmax"""
    a, b = np.asarray(a).astype(dt), np.asarray(b).astype(dt)[:len(a) - 1]
    m = len(a)
    lo, hi, tmax = tridiag_bounds(a, b)
    unit = max(dt(1), tmax)
    for _ in range(200):
        if not hi - lo > dt(4e-16) * unit:
            break
        mid = (lo + hi) / 2
        if sturm_count(a, b, mid) >= 1:
            hi = mid
        else:
            lo = mid
    theta = (lo + hi) / 2
    if m == 1:
        return theta, np.ones(1, dtype=dt), tmax
    y = np.full(m, 1 / np.sqrt(dt(m)), dtype=dt)
    d, e = a - (theta - dt(1e-14) * unit), b.copy()
    for _ in range(3):
        y = tridiag_solve(d, e, y)
        y = y / np.sqrt(y @ y)
    return theta, y, tmax


def tridiag_solve(d, e, rhs):
    """(tridiagonal with diagonal d, off-diagonal e) x = rhs by elimination with partial pivoting, in the arrays' dtype"""
    m = len(d)
    dd, du, du2, dl, x = d.copy(), np.append(e, 0), np.zeros(m, dtype=d.dtype), np.append(e, 0), rhs.copy()
    for i in range(m - 1):
        if abs(dd[i]) >= abs(dl[i]):
            f = dl[i] / dd[i]
            dd[i + 1] -= f * du[i]
            x[i + 1] -= f * x[i]
        else:
            f = dd[i] / dl[i]
            t_dd, t_du = dd[i + 1], du[i + 1]
            dd[i], old_du = dl[i], du[i]
            du[i] = t_dd
            du2[i] = t_du if i < m - 2 else 0
            dd[i + 1] = old_du - f * t_dd
            if i < m - 2:
                du[i + 1] = -f * t_du
            x[i], x[i + 1] = x[i + 1], x[i] - f * x[i + 1]
    x[m - 1] = x[m - 1] / dd[m - 1]
    x[m - 2] = (x[m - 2] - du[m - 2] * x[m - 1]) / dd[m - 2]
    for i in range(m - 3, -1, -1):
        x[i] = (x[i] - du[i] * x[i + 1] - du2[i] * x[i + 2]) / dd[i]
    return x


def lanczos_stage(op, C, dt=LD, mmax=400, restarts=12, dense_rows=384, damage=None, pos=None, length=None, V=None):
    """V given: lanczos_step, one step from those columns.  Otherwise the whole run of Context::lanczos_min from lanczos_start with its stop rules:
    a cycle takes up to min(3n, max(2, mmax)) steps; with 3n <= dense_rows and 3n <= mmax ("exact") it ends only when the Krylov space is
    exhausted (3n steps, or beta < 1e-13 max(1, tmax)), otherwise also at a Ritz residual |beta_{m-1} y_{m-1}| <= 1e-9 max(1, tmax); the Ritz
    vector starts the next of up to `restarts` cycles; converged (ret 0) means a residual <= 1e-6 max(1, tmax).  pos (camera -> position; only
    the fault "not mapped back" reads it).  -> alpha, beta, V (3n x (m_use + 1)), y, x, theta, resid, ret, eig_exact, m_use, cycles, iters, tmax, c1 and c2 of the last step"""
    if V is not None:
        return lanczos_step(op, C, V, dt, damage, length)
    n = C["dz"].size
    m3 = 3 * n
    mmax = min(m3, max(2, mmax))
    exact = m3 <= dense_rows and m3 <= mmax
    x = lanczos_start(n).astype(dt)
    eig_exact, iters, resid, theta, tmax = False, 0, dt(1e300), dt(0), dt(1)
    for cycle in range(max(1, restarts)):
        V = np.zeros((m3, mmax + 1), dtype=dt)
        V[:, 0] = x
        al, be, done, m_use, y = [], [], False, 0, None
        for j in range(mmax):
            st = step = lanczos_step(op, C, V[:, :j + 1], dt, damage, length, scales=False)
            iters += 1
            al.append(st["alpha"])
            beta = st["beta"]
            V[:, j + 1] = st["w"].reshape(-1) / beta if beta > 0 else 0
            m_use = m = j + 1
            tmax = tridiag_bounds(np.array(al, dtype=dt), np.array(be + [dt(0)], dtype=dt))[2]
            exhausted = m == m3 or beta < dt(1e-13) * max(dt(1), tmax)
            y = None
            if not exact or exhausted or j == mmax - 1:        # (an exact run looks at the residual only when it ends)
                theta, y, tmax = tridiag_min(al, be + [dt(0)], dt)
                resid = abs(beta * y[m - 1])
            if exact and exhausted and np.isfinite(beta):
                eig_exact = True
            if (not exact and resid <= dt(1e-9) * max(dt(1), tmax)) or exhausted or not np.isfinite(beta):
                done = True
                break
            be.append(beta)
        yy = y[::-1] if damage == "lz_y_reversed" else y
        x = V[:, :m_use] @ yy
        x = x / np.sqrt(x @ x)
        if done:
            break
    be = (be + [beta])[:m_use]
    xo = x
    if damage == "lz_no_unmap" and pos is not None:
        xo = np.empty_like(x)
        xo.reshape(n, 3)[np.asarray(pos)] = x.reshape(n, 3)
    return dict(alpha=np.array(al, dtype=dt), beta=np.array(be, dtype=dt), V=V[:, :m_use + 1], y=y, x=xo, theta=theta, resid=resid,
                ret=0 if resid <= dt(1e-6) * max(dt(1), tmax) else 1, eig_exact=eig_exact, m_use=m_use, cycles=cycle + 1, iters=iters, tmax=tmax,
                c1=step["c1"], c2=step["c2"])


def polar_rows(M):
    """the closest matrices with orthonormal rows to a batch of 3 x o blocks: Newton's iteration X <- (X + (X X^T)^-1 X) / 2, the 3x3 inverses
    by cofactors (numpy's factorisations do not work in longdouble)"""
    X = M.copy()
    for _ in range(60):
        A = np.einsum("iak,ibk->iab", X, X)
        C = np.empty_like(A)
        for a in range(3):
            for b in range(3):
                a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
                C[:, b, a] = A[:, a1, b1] * A[:, a2, b2] - A[:, a1, b2] * A[:, a2, b1]
        det = (A[:, 0, :] * C[:, :, 0]).sum(axis=1)
        Xn = (X + np.einsum("iab,ibk->iak", C / det[:, None, None], X)) / 2
        if np.abs(Xn - X).max() == 0:
            break
        X = Xn
    return X


def curve(R, s, pR, ps, t, dt=LD):
    """a second-order curve through (R, s) with velocity (pR, ps): the polar retraction of R + t pR and the geodesic s exp(t ps / s) of the
    metric ds^2 / s^2 (trustregion.h:19-24)"""
    R, s = point(R, s, dt)
    n, t = s.size, dt(t)
    Rt = polar_rows(blk(R + t * np.asarray(pR).astype(dt), n)).reshape(R.shape)
    st = s * np.exp(t * np.asarray(ps).astype(dt) / s)
    return Rt, st


def mgs_rows(M, damage=None):
    """rows of a batch of 3 x o blocks by modified Gram-Schmidt in the order of Dense/batchedQR.h:42-67: normalise row i, then take its
    component out of every later row"""
    q = M.copy()
    for i in range(3):
        raw = q[:, i, :].copy()
        q[:, i, :] = raw / np.sqrt((raw * raw).sum(axis=1))[:, None]
        for j in range(i + 1, 3):
            a = raw if (damage == "mgs_raw_row" and i == 1) else q[:, i, :]
            uu = (a * q[:, j, :]).sum(axis=1)
            q[:, j, :] = q[:, j, :] - uu[:, None] * a
    return q


def retract_stage(R, s, D, ds, t, polar, dt=LD, damage=None):
    """the retraction of trustregion.h:667-678 (and of its line search with ds = None): Rn = rows of R + t D by modified Gram-Schmidt or the
    polar factor, sn = s exp(t ds / s) with the anchor left alone (trustregion.h:19-24), the next product input W = sn .* Rn (:677)"""
    R, s = point(R, s, dt)
    n, t = s.size, dt(t)
    M = blk(R + t * np.asarray(D).astype(dt), n)
    Rn = polar_rows(M) if polar else mgs_rows(M, damage)
    if ds is None:
        sn = s.copy()
    else:
        sn = s * np.exp(t * np.asarray(ds).astype(dt) / s)
        if damage != "anchor_scale":
            sn[0] = s[0]
    one = np.ones(n, dtype=dt)
    return {"Rc": Rn, "Rc~": one, "sc": sn, "sc~": sn, "W": Rn * sn[:, None, None], "W~": sn}


def model_stage(v, Hv, rg, s, dt=LD, damage=None):
    """the model decrease of the step v, m = <v, Hv> / 2 + <v, rg> in the product metric (trustregion.h:667-668), per camera and summed; the
    anchor's scale part of a step is 0.  Hv = None: no such sum is formed (XM_FLAG_MODEL_RECURRENCE)"""
    cv = lambda a: np.asarray(a).astype(dt)
    s = cv(s).copy(); s[0] = 1
    n = s.size
    vR, vs, HvR, Hvs, rgR, rgs = blk(cv(v[0]), n), cv(v[1]).copy(), blk(cv(Hv[0]), n), cv(Hv[1]), blk(cv(rg[0]), n), cv(rg[1])
    vs[0] = 0
    metric = s if damage == "m_metric_s" else s * s
    mR = (vR * (HvR / 2 + rgR)).sum(axis=(1, 2))
    ms = vs / metric * (Hvs / 2 + rgs)
    if damage == "m_no_scale":
        ms = ms * 0
    am = (np.abs(vR) * (np.abs(HvR) / 2 + np.abs(rgR))).sum(axis=(1, 2)) + np.abs(vs) / (s * s) * (np.abs(Hvs) / 2 + np.abs(rgs))
    return {"m_cam": mR + ms, "m": (mR + ms).sum(), "m~": am.sum()}


def outer_decide_stage(sc, os, f, rr_new, m, delta_bar, gradtol, max_outer, time_up, damage=None):
    """what the step launch of the device-driven outer iteration decides between two truncated CGs, in plain f64 scalar code: the trust-region
    update of trustregion.h:680-708 and the stop tests of :527-543 as Context::trust_region has them.  sc: the tCG's scalar block (delta, status,
    iter, phase), os: the trust region's (loss, rr_point, totalite, shrink_count, k, time_up, slots), f / rr_new / m: the candidate's cost and
    squared gradient norm and the model decrease, time_up: the host's stop-request word.  PH_INIT starts the first tCG and decides nothing,
    PH_STOP passes both blocks on.  Returns the next blocks' fields, stop_reason, accept, start and the trace record (None if none is written)."""
    F = np.float64
    phase = int(sc["phase"])
    if phase == PH_STOP:
        return dict(phase=PH_STOP, passed=True, accept=False, start=False, trace=None)
    loss, rr, delta = F(os["loss"]), F(os["rr_point"]), F(sc["delta"])
    shrink, k, totalite, stop = int(os["shrink_count"]), int(os["k"]), int(os["totalite"]), 0
    accept, start, trace = False, True, None
    if phase == PH_CAND:
        f, rr_new, m = F(f), F(rr_new), F(m)
        endreason = 6 if int(sc["status"]) == 0 else int(sc["status"])
        inner_print, trstatus = int(sc["iter"]) + 1, 4
        totalite += int(sc["iter"]) + 1
        if m >= 0:                                         # "loss_qu is larger than 0": the point stays
            stop, start = 12, False
        else:
            rou = (f - loss) / (-m if damage == "rou_sign" else m)    # :680
            if rou < 0.25:
                delta, trstatus, shrink = delta * F(0.25), 1, shrink + 1
            elif rou > 0.75 and (endreason <= 2 or damage == "double_any"):
                delta, trstatus, shrink = min(delta * 2, F(delta_bar)), 2, 0
            else:
                shrink = 0
            stop_delta = False
            if shrink > 3:                                 # :692-700
                delta, shrink = delta * F(1e-3), 0
                stop_delta = bool(delta < 1e-20)
            reject = bool((f > loss and damage != "no_f_gt_loss") or rou < 0.1)   # :702
            accept = stop_delta or not reject
            if stop_delta:                                 # the reference leaves the new point in place but reports loss[k]
                stop, start = 13, False
            else:
                if not reject:
                    loss, rr = f, rr_new
                else:
                    trstatus = 3
                k += 1
                if k >= int(max_outer):
                    stop, start = 14, False
                else:
                    trace = (float(loss), float(np.sqrt(rr)), float(inner_print), float(endreason), float(trstatus), float(delta))
                    if endreason == 5:
                        stop = 5
                    elif np.sqrt(rr) < F(gradtol):
                        stop = 10
                    elif int(os["time_up"]):
                        stop = 11
                    start = stop == 0
    return dict(rr=float(rr), pp=float(rr), delta=float(delta), gradnorm=float(np.sqrt(rr)), vv=0.0, vp=0.0, last_step=0.0, model=0.0, status=0, iter=0,
                seq=int(sc.get("seq", 0)), phase=PH_TCG if start else PH_STOP, loss=float(loss), rr_point=float(rr), totalite=totalite, shrink_count=shrink,
                k=k, stop_reason=stop, time_up=int(os["time_up"]) | int(time_up), slots=int(os.get("slots", 0)) + (1 if phase == PH_CAND else 0),
                accept=accept, start=start, trace=trace, passed=False)
