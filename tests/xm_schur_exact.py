"""The matrix-free Q (xm-code_amd/csrc/xm_schur.hip) in np.longdouble, straight from the observation list (cam, lm, p, w): the set-up factors,
the stages of one product and the pieces of the inner CG, under the keys of the test export xm_ctx_schur_probe.  Reference of
tests/test_schur_exact.py (CPU) and tests/test_gpu_schur_stages.py (GPU); the f64 restatement it judges is xm_schur_stages.py.

    Q1_i = sum w p p^T, c_i = sum w p, q2_i = sum w (per camera);  Q3_l = sum w, q3inv_l = 1 / Q3_l, := 0 where Q3_l = 0 (per landmark)
    VT = diag(q2) - V3 diag(q3inv) V3^T without row and column of camera 0, V3[i, l] = the summed weight of the pair (i, l)
    h_l = -q3inv_l sum w (p . W_i);  r_i = c_i . W_i + sum w h_l;  xc = VT^-1 r;  xl_l = h_l + q3inv_l sum_{i >= 1} w xc_i
    Y_i = alpha (Q1_i W_i - c_i xc_i + sum w p xl_l)

A (camera, landmark) pair named twice is summed wherever a sum runs over observations.  Systems with VT are solved by an f64 factorisation and
iterative refinement with longdouble residuals, until the residual stops falling (VT is applied through the observation list: O(observations)
longdouble operations per column instead of a dense longdouble product)."""
import numpy as np
import scipy.linalg as sla

LD = np.longdouble
AGG = 64


def _add(shape, idx, vals):
    out = np.zeros(shape, dtype=LD)
    np.add.at(out, idx, vals)
    return out


def refine_inverse(A):
    """A^-1 in longdouble for a small symmetric positive definite A (longdouble): f64 inverse, then Newton steps X += X (I - A X)"""
    n = A.shape[0]
    X = np.linalg.inv(A.astype(np.float64)).astype(LD)
    I = np.eye(n, dtype=LD)
    last = np.inf
    for _ in range(6):
        R = I - A @ X
        e = float(np.abs(R).max())
        if not e < last:
            break
        last = e
        X = X + X @ R
    return (X + X.T) / 2


class Exact:
    def __init__(self, cam, lm, p, w, n, m):
        self.cam, self.lm = np.asarray(cam, dtype=np.int64), np.asarray(lm, dtype=np.int64)
        self.p, self.w = np.asarray(p, dtype=LD), np.asarray(w, dtype=LD).reshape(-1)
        self.n, self.m, self.n1 = int(n), int(m), int(n) - 1
        cam, lm, p, w = self.cam, self.lm, self.p, self.w
        self.Q1 = _add((n, 3, 3), cam, w[:, None, None] * p[:, :, None] * p[:, None, :])
        self.c = _add((n, 3), cam, w[:, None] * p)
        self.q2 = _add((n,), cam, w)
        self.Q3 = _add((m,), lm, w)
        self.q3inv = np.where(self.Q3 > 0, 1 / np.where(self.Q3 > 0, self.Q3, 1), LD(0))
        self.deg = np.bincount(lm, minlength=m)
        self.red = cam >= 1                                   # observations of the reduced cameras 1..n-1
        if self.n1 > 0:
            self.VT = self.apply_vt(np.eye(self.n1, dtype=LD))
            self.VT = (self.VT + self.VT.T) / 2
            self._lu = sla.lu_factor(self.VT.astype(np.float64))
            self.dinv = 1 / np.diag(self.VT)

    # ---------------------------------------------------------------------------------------- the reduced camera Laplacian
    def lm_sum(self, X):
        """y_l = q3inv_l sum_{obs of l, camera >= 1} w X_{camera - 1}"""
        e = self.red
        return self.q3inv[:, None] * _add((self.m, X.shape[1]), self.lm[e], self.w[e, None] * X[self.cam[e] - 1])

    def apply_vt(self, X):
        X = np.asarray(X, dtype=LD)
        e = self.red
        y = self.lm_sum(X)
        return self.q2[1:, None] * X - _add(X.shape, self.cam[e] - 1, self.w[e, None] * y[self.lm[e]])

    def solve(self, B):
        """VT^-1 B; self.refine: (steps, last residual relative to |B|)"""
        B = np.asarray(B, dtype=LD)
        x = sla.lu_solve(self._lu, B.astype(np.float64)).astype(LD)
        scale = max(float(np.abs(B).max()), np.finfo(np.float64).tiny)
        last, steps = np.inf, 0
        for steps in range(1, 12):
            res = B - self.apply_vt(x)
            e = float(np.abs(res).max()) / scale
            if not e < 0.5 * last:
                break
            last = e
            x = x + sla.lu_solve(self._lu, res.astype(np.float64)).astype(LD)
        self.refine = (steps, min(e, last))
        return x

    def cond(self):
        ev = np.linalg.eigvalsh(self.VT.astype(np.float64))
        return float(ev[-1] / ev[0])

    def vtinv(self):
        X = self.solve(np.eye(self.n1, dtype=LD))
        return (X + X.T) / 2

    # ---------------------------------------------------------------------------------------- one product
    def chain(self, W, alpha=1.0):
        """dict h, r, xc, xl, Y and the floors of their error denominators (key + "~"): the magnitude of the terms a row is summed from"""
        n, m, cam, lm, p, w = self.n, self.m, self.cam, self.lm, self.p, self.w
        W = np.asarray(W, dtype=LD).reshape(3 * n, -1)
        o = W.shape[1]
        Wc = W.reshape(n, 3, o)
        pw = np.einsum("ea,eak->ek", p, Wc[cam])
        pw_abs = np.einsum("ea,eak->ek", np.abs(p), np.abs(Wc[cam]))
        h = -self.q3inv[:, None] * _add((m, o), lm, w[:, None] * pw)
        h_abs = self.q3inv[:, None] * _add((m, o), lm, w[:, None] * pw_abs)
        r = np.einsum("ia,iak->ik", self.c, Wc) + _add((n, o), cam, w[:, None] * h[lm])
        r_abs = np.einsum("ia,iak->ik", np.abs(self.c), np.abs(Wc)) + _add((n, o), cam, w[:, None] * h_abs[lm])
        xc = np.zeros((n, o), dtype=LD)
        if self.n1 > 0:
            xc[1:] = self.solve(r[1:])
        xl = h + self.q3inv[:, None] * _add((m, o), lm, w[:, None] * xc[cam])
        xl_abs = h_abs + self.q3inv[:, None] * _add((m, o), lm, w[:, None] * np.abs(xc[cam]))
        Y = np.einsum("iab,ibk->iak", self.Q1, Wc) - self.c[:, :, None] * xc[:, None, :] + \
            _add((n, 3, o), cam, w[:, None, None] * p[:, :, None] * xl[lm][:, None, :])
        Y_abs = np.einsum("iab,ibk->iak", np.abs(self.Q1), np.abs(Wc)) + np.abs(self.c)[:, :, None] * np.abs(xc)[:, None, :] + \
            _add((n, 3, o), cam, w[:, None, None] * np.abs(p)[:, :, None] * xl_abs[lm][:, None, :])
        a = LD(alpha)
        xs = np.abs(xc).max() if self.n1 > 0 else LD(0)   # a solve is accurate normwise
        out = {"h": h, "r": r[1:], "xc": xc[1:], "xl": xl, "Y": a * Y.reshape(n, 3 * o)}
        out.update({"h~": h_abs.max(axis=1), "r~": r_abs[1:].max(axis=1), "xc~": np.full(self.n1, xs),
                    "xl~": np.maximum(xl_abs, xs).max(axis=1), "Y~": abs(a) * Y_abs.reshape(n, 3 * o).max(axis=1)})
        return out

    # ---------------------------------------------------------------------------------------- the inner CG's pieces
    def blocks(self, perm):
        """perm (nagg x 64, reduced camera or -1) -> binv (nagg x 64 x 64: VT_aa^-1, identity on the padding rows), Ac = P^T VT P, ainv"""
        perm = np.asarray(perm)
        na = perm.shape[0]
        binv = np.zeros((na, AGG, AGG), dtype=LD)
        P = np.zeros((self.n1, na), dtype=LD)
        for a in range(na):
            rows = np.nonzero(perm[a] >= 0)[0]
            idx = perm[a][rows]
            binv[a] = np.eye(AGG, dtype=LD)
            binv[a][np.ix_(rows, rows)] = refine_inverse(self.VT[np.ix_(idx, idx)])
            P[idx, a] = 1
        Ac = P.T @ self.VT @ P
        return binv, (Ac + Ac.T) / 2, refine_inverse((Ac + Ac.T) / 2), P

    def pieces(self, X, perm=None):
        """dict VX, pAp, MX_jacobi (+ its floors) and, with perm, binv, ainv, MX_two_level"""
        X = np.asarray(X, dtype=LD).reshape(self.n1, -1)
        e = self.red
        y_abs = self.q3inv[:, None] * _add((self.m, X.shape[1]), self.lm[e], self.w[e, None] * np.abs(X)[self.cam[e] - 1])
        VX = self.apply_vt(X)
        VX_abs = self.q2[1:, None] * np.abs(X) + _add(X.shape, self.cam[e] - 1, self.w[e, None] * y_abs[self.lm[e]])
        out = {"VX": VX, "VX~": VX_abs.max(axis=1), "pAp": (X * VX).sum(axis=0)[:, None], "pAp~": (np.abs(X) * VX_abs).sum(axis=0),
               "MX_jacobi": self.dinv[:, None] * X}
        if perm is not None:
            perm = np.asarray(perm)
            binv, Ac, ainv, P = self.blocks(perm)
            Z = np.zeros_like(X)
            for a in range(perm.shape[0]):
                rows = np.nonzero(perm[a] >= 0)[0]
                idx = perm[a][rows]
                Z[idx] = binv[a][np.ix_(rows, rows)] @ X[idx]
            MX = Z + P @ (ainv @ (P.T @ X))
            # A_c = P^T VT P cancels: an aggregate's sum of q2 (hundreds of observations) against the landmarks that lie inside it, what is left
            # is the weight that crosses its border.  To first order an error dA of A_c moves the inverse by -ainv dA ainv, so the floor of
            # ainv's error is |ainv| T |ainv| with T the magnitude of the terms A_c is summed from: P^T (diag q2 + V3 Q3^-1 V3^T) P
            T = P.T @ (2 * np.diag(self.q2[1:]) - self.VT) @ P
            out["ainv~"] = np.array([np.abs(np.abs(ainv) @ T @ np.abs(ainv)).max()])
            out.update({"binv": binv.reshape(perm.shape[0], -1), "ainv": ainv.reshape(1, -1), "Ac": Ac, "MX_two_level": MX,
                        "MX_two_level~": np.full(self.n1, np.abs(MX).max())})
        return out

    def setup(self, dense=False):
        out = {"Q1": self.Q1.reshape(self.n, 9), "c": self.c, "q2": self.q2[:, None], "q3inv": self.q3inv[:, None]}
        if self.n1 > 0:
            out["dinv"] = self.dinv[:, None]
            if dense:
                V = self.vtinv()
                out["VTinv"] = V
                out["VTinv~"] = np.full(self.n1, np.abs(V).max())          # an inverse is accurate normwise
        return out


def perm_from_plan(agg_of):
    """nagg x 64 table of reduced cameras from the aggregate of every camera (xm_schur_aggregate_plan; -1: camera 0), members in index order,
    -1 = padding.  The library orders the members of an aggregate by its breadth-first search: a test that has the probe's table uses that."""
    agg_of = np.asarray(agg_of)
    na = int(agg_of.max()) + 1
    perm = -np.ones((na, AGG), dtype=np.int64)
    for a in range(na):
        mem = np.nonzero(agg_of == a)[0] - 1
        perm[a, :mem.size] = mem
    return perm
