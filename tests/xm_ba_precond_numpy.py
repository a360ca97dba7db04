"""numpy / scipy.sparse restatement of the opt-in PCG preconditioners of xm_ctx_bundle_adjust (XM_BA_PRECOND_BLOCKS, XM_BA_PRECOND_TWO_LEVEL;
include/xm_amd.h, xm_ba.h): the aggregate plan, the damped reduced camera system, the aggregate blocks, the rigid-plus-scale coarse space P,
A_c = P^T S P and the PCG with the library's stop rule.  Written from the formulas of the header, on top of xm_ba_numpy.py."""
import numpy as np
import scipy.sparse as sp

import xm_ba_numpy as ba

AGG_CAMS = 16
MAX_AGGREGATES = 4096
HEAVY = 64


def aggregate_plan(cam, lm, n, used=None, B=AGG_CAMS):
    """(agg_of_camera, order): the cameras with a used observation in breadth-first order over the graph of the used observations
    (landmarks with more than 64 of them are not expanded; lists in input order) from camera 0, or from the camera that search reaches last
    when camera 0 does not lie in the last level of the search from there; members never reached appended in index order, cut into
    runs of B; -1 for a camera without a used observation"""
    cam, lm = np.asarray(cam, dtype=np.int64), np.asarray(lm, dtype=np.int64)
    if used is not None:
        u = np.asarray(used) != 0
        cam, lm = cam[u], lm[u]
    by_cam = [[] for _ in range(n)]
    by_lm = [[] for _ in range(int(lm.max()) + 1 if lm.size else 0)]
    for c, l in zip(cam.tolist(), lm.tolist()):
        by_cam[c].append(l); by_lm[l].append(c)
    member = [len(v) > 0 for v in by_cam]
    if (sum(member) + B - 1) // B > MAX_AGGREGATES:
        raise ValueError("more than MAX_AGGREGATES aggregates")
    def bfs(start):
        seen, lseen, out, level = [False] * n, [False] * len(by_lm), [start], {start: 0}
        seen[start] = True
        h = 0
        while h < len(out):
            for l in by_cam[out[h]]:
                if lseen[l] or len(by_lm[l]) > HEAVY:
                    continue
                lseen[l] = True
                for c2 in by_lm[l]:
                    if not seen[c2]:
                        seen[c2] = True; level[c2] = level[out[h]] + 1; out.append(c2)
            h += 1
        return out, level, seen

    order, seen = [], [False] * n
    if any(member):
        start = member.index(True)
        first, _, seen = bfs(start)
        order, level, _ = bfs(first[-1])               # again from the camera reached last: one front instead of two ...
        if level[start] == level[order[-1]]:           # ... unless the start is an end of the trajectory itself
            order = first
    order += [i for i in range(n) if member[i] and not seen[i]]
    agg = np.full(n, -1, dtype=np.int32)
    agg[order] = np.arange(len(order)) // B
    return agg, np.array(order, dtype=np.int64)


def coarse_ranges(nmem, B=AGG_CAMS):
    """positions [k0, k1) of the members of every coarse aggregate: the runs of B, a last run of one member joined to its predecessor"""
    nagg = (nmem + B - 1) // B
    ncoarse = nagg - 1 if (nagg > 1 and nmem - (nagg - 1) * B < 2) else nagg
    return [(a * B, nmem if a == ncoarse - 1 else (a + 1) * B) for a in range(ncoarse)]


def reduced_system(cam, lm, p, w, rot, t, P, mu, fix_rotations=False):
    """(S, b, Rcw, tcw): the damped reduced camera system S = U* - W V*^-1 W^T, b = -g_c + W V*^-1 g_l at (rot, t, P) with the library's
    D = diag(J^T J) clamped to [1e-6, 1e32]"""
    n, m = t.shape[1], P.shape[1]
    pr = ba.Problem(cam, lm, p, w, n, m, fix_rotations)
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    r, J = pr.jacobian(Rcw, tcw, P.T.copy())
    H = (J.T @ J).tocsc()
    g = J.T @ r
    H = (H + sp.diags(mu * np.clip(H.diagonal(), 1e-6, 1e32))).tocsr()
    nc = pr.cd * n
    U, W, V = H[:nc, :nc], H[:nc, nc:], H[nc:, nc:].tocoo()
    Vd = np.zeros((m, 3, 3))
    Vd[V.row // 3, V.row % 3, V.col % 3] = V.data
    Vinv = sp.block_diag(list(np.linalg.inv(Vd)), format="csr")
    S = (U - W @ Vinv @ W.T).tocsr()
    b = -g[:nc] + W @ (Vinv @ g[nc:])
    return S, b, Rcw, tcw


def rigid_basis(Rcw, tcw, order, B=AGG_CAMS, fix_rotations=False, scale=True):
    """(P, dropped): cd n x NC ncoarse.  Per coarse aggregate a with centroid c_a of its members' centres C_i = -Rcw_i^T tcw_i the effect
    on (dtheta_i, dtcw_i) of X -> X + w x (X - c_a) + v + s (X - c_a):  dtheta_i = -Rcw_i w,
    dtcw_i = Rcw_i ([C_i - c_a]x - [C_i]x) w - Rcw_i v - s Rcw_i (C_i - c_a); columns (w, v, s), or (v, s) of the dtcw rows with fixed
    rotations; columns scaled to unit 2-norm, a column of norm 0 left zero and listed in dropped"""
    n = Rcw.shape[0]
    cd, ncol = (3, 4) if fix_rotations else (6, 7)
    C = -np.einsum("iba,ib->ia", Rcw, tcw)
    ranges = coarse_ranges(len(order), B)
    Pm = np.zeros((cd * n, ncol * len(ranges)))
    dropped = []
    for a, (k0, k1) in enumerate(ranges):
        mem = order[k0:k1]
        c = C[mem].mean(axis=0)
        for i in mem:
            R, d = Rcw[i], C[i] - c
            blk = np.zeros((cd, ncol))
            if not fix_rotations:
                blk[:3, :3] = -R
                blk[3:, :3] = R @ (ba.skew(d) - ba.skew(C[i]))
            blk[cd - 3:, ncol - 4:ncol - 1] = -R
            blk[cd - 3:, ncol - 1] = -R @ d
            Pm[cd * i:cd * i + cd, ncol * a:ncol * a + ncol] = blk
        for k in range(ncol * a, ncol * a + ncol):
            nk = np.linalg.norm(Pm[:, k])
            if nk > 0 and scale:
                Pm[:, k] /= nk
            elif not nk > 0:
                dropped.append(k)
    return sp.csr_matrix(Pm), dropped


def block_inverse(S, order, B=AGG_CAMS, cd=6):
    """blockdiag(S_aa)^-1 over the aggregates (runs of B members), zero on the cameras that are no members, as a sparse matrix"""
    N = S.shape[0]
    rows, cols, vals = [], [], []
    for k0 in range(0, len(order), B):
        idx = (cd * np.asarray(order[k0:k0 + B])[:, None] + np.arange(cd)[None, :]).reshape(-1)
        inv = np.linalg.inv(S[idx][:, idx].toarray())
        rows.append(np.repeat(idx, idx.size)); cols.append(np.tile(idx, idx.size)); vals.append(inv.reshape(-1))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))


def jacobi_inverse(S, cd=6):
    n = S.shape[0] // cd
    return block_inverse(S, np.arange(n), 1, cd)


def coarse_operator(S, P, dropped=()):
    """A_c = P^T S P with the rows and columns of dropped columns set to the identity"""
    Ac = (P.T @ S @ P).toarray()
    for k in dropped:
        Ac[k, :] = 0.0; Ac[:, k] = 0.0; Ac[k, k] = 1.0
    return Ac


def two_level(S, order, P, dropped=(), B=AGG_CAMS, cd=6):
    """r -> blockdiag(S_aa)^-1 r + P A_c^-1 P^T r"""
    Bi = block_inverse(S, order, B, cd)
    Aci = np.linalg.inv(coarse_operator(S, P, dropped))
    return lambda r: Bi @ r + P @ (Aci @ (P.T @ r))


def pcg(S, b, Minv, eta, cap=500):
    """(x, iterations, |r| / |b|): PCG from zero, stopped when |r| <= eta |b| after an update or at cap iterations (the library's rule)"""
    x = np.zeros_like(b); r = b.copy(); z = Minv(r); p = z.copy(); rz = r @ z; nb = np.linalg.norm(b)
    if nb == 0:
        return x, 0, 0.0
    for k in range(1, cap + 1):
        Ap = S @ p
        al = rz / (p @ Ap)
        x += al * p; r -= al * Ap
        if np.linalg.norm(r) <= eta * nb:
            return x, k, float(np.linalg.norm(r) / nb)
        z = Minv(r); rz2 = r @ z; p = z + (rz2 / rz) * p; rz = rz2
    return x, cap, float(np.linalg.norm(r) / nb)


def first_step_iterations(cam, lm, p, w, rot, t, P, mu, eta, kind, fix_rotations=False, cap=500):
    """PCG iterations of one LM step at (rot, t, P) for kind in jacobi / blocks / two_level"""
    cd = 3 if fix_rotations else 6
    S, b, Rcw, tcw = reduced_system(cam, lm, p, w, rot, t, P, mu, fix_rotations)
    _, order = aggregate_plan(cam, lm, t.shape[1], ba.used_mask(p, w))
    if kind == "jacobi":
        Ji = jacobi_inverse(S, cd)
        M = lambda r: Ji @ r
    elif kind == "blocks":
        Bi = block_inverse(S, order, AGG_CAMS, cd)
        M = lambda r: Bi @ r
    else:
        Pm, dropped = rigid_basis(Rcw, tcw, order, AGG_CAMS, fix_rotations)
        M = two_level(S, order, Pm, dropped, AGG_CAMS, cd)
    return pcg(S, b, M, eta, cap)[1]
