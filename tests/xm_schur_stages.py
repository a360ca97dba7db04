"""What tests/test_schur_exact.py (CPU) and tests/test_gpu_schur_stages.py (GPU) share: the scenes, the f64 numpy restatement of the matrix-free
Q's stages (the factors, one product's chain, the inner CG's pieces) under the keys of xm_schur_exact.py, the forms a context can take, the
comparison and the STAGE_ERR table.

Error and bound are those of the bundle adjustment's stage tests (xm_ba_stages.err / bound): per quantity and case e <= max(16 e_ref,
64 eps_f64), e_ref the f64 restatement's own error against the longdouble reference, the larger of two observation orders.  Errors are taken
per block (a landmark row, a camera row, a camera's 3 x 3 block, an aggregate's block) against the larger of the exact block and the magnitude
of the terms it is summed from (the "~" entries of xm_schur_exact.py), so that a row that cancels to nothing does not blow the ratio up."""
import functools

import numpy as np
import scipy.sparse as sp

import xm_ba_stages as st
import xm_schur_exact as ex
import xm_seqscene as sq
import xm_testlib as tl

LD = ex.LD
EPS = st.EPS
MAX_E_REF = st.MAX_E_REF
err, bound = st.err, st.bound
AGG = ex.AGG
PCG_TOL, PCG_CAP = 1e-13, 1000          # relative residual of the inner solve in a plain product, iteration cap (xm_schur.h)

# form of a context -> (xm_tuning_t fields, kind of the reduced solve: which restatement of xc applies)
FORMS = {"dense": (dict(schur_solver=1), "dense"), "sym": (dict(schur_solver=1, sym_min_rows=1), "dense"),
         "jacobi": (dict(schur_solver=2), "jacobi"), "two_level": (dict(schur_solver=3), "two_level"),
         "host": (dict(schur_host_assembly=1), "dense")}
SETUP_KEYS = ("Q1", "c", "q2", "q3inv")
CHAIN_KEYS = ("h", "r", "xc", "xl", "Y")


def keys_of(kind, n1, chain=True, pieces=True):
    if n1 <= 0:
        return SETUP_KEYS + (("h", "xl", "Y") if chain else ())
    k = SETUP_KEYS + (("VTinv",) if kind == "dense" else ("dinv",)) + (CHAIN_KEYS if chain else ())
    if pieces and kind != "dense":
        k += ("VX", "pAp", "MX") + (("binv", "ainv") if kind == "two_level" else ())
    return k


# ------------------------------------------------------------------------------------------------ scenes
def _observe(rng, n, m, cam, lm, noise=0.01):
    Rs = tl.haar_so3(rng, n)
    ts = rng.uniform(-5.0, 5.0, (n, 3))
    P = rng.uniform(-8.0, 8.0, (m, 3))
    pts = np.einsum("eba,eb->ea", Rs[cam], P[lm] - ts[cam]) + noise * rng.standard_normal((cam.size, 3))
    return dict(cam=cam.astype(np.int32), lm=lm.astype(np.int32), p=pts, w=rng.uniform(0.5, 1.5, cam.size), n=n, m=m)


DEGREES = (0, 1, 2, 63, 64, 65, 66, 1023, 1024, 1025, 1030)
DEGREES_N = 1030
DEGREES_LIGHT = 1024 + 64 + 1            # one full workgroup of light landmarks, one full group of the second, a last group of one slot
WITH_CAMERA_0 = {2: True, 63: False, 64: True, 65: False, 66: True, 1023: False, 1024: True, 1025: False, 1030: True}


def degree_scene():
    """1030 cameras; one landmark of every degree in DEGREES (`roles`: their indices; those of degree >= 2 with or without camera 0 as
    WITH_CAMERA_0 says) and fillers of degree 2..9, DEGREES_LIGHT landmarks of at most 64 observations in all; landmark indices shuffled, the
    observations in random order, no (camera, landmark) pair twice"""
    rng = np.random.default_rng(1030)
    n = DEGREES_N
    light = sum(1 for d in DEGREES if d <= 64)
    degs = list(DEGREES) + list(rng.integers(2, 10, DEGREES_LIGHT - light))
    m = len(degs)
    index = rng.permutation(m)
    if degs[int(np.argmax(index))] == 0:                   # the binding takes m = largest index + 1: the degree-0 index is not the last
        j = int(np.argmax(index)); index[[j, (j + 1) % m]] = index[[(j + 1) % m, j]]
    cams, lms = [], []
    for k, d in enumerate(degs):
        if d == 0:
            continue
        if k < len(DEGREES) and d >= 2:
            rest = 1 + rng.choice(n - 1, d - 1 if WITH_CAMERA_0[d] else d, replace=False)
            seen = np.concatenate([[0], rest]) if WITH_CAMERA_0[d] else rest
        else:
            seen = rng.choice(n, d, replace=False)
        cams.append(seen); lms.append(np.full(d, index[k]))
    cam, lm = np.concatenate(cams), np.concatenate(lms)
    e = rng.permutation(cam.size)
    S = _observe(rng, n, m, cam[e], lm[e])
    S["roles"] = {d: int(index[k]) for k, d in enumerate(DEGREES)}
    return S


CAM_COUNTS = (64, 1, 2, 63, 65, 127, 128, 129, 20, 21, 22, 23)


def cam_degree_scene():
    """12 cameras with CAM_COUNTS observations (camera 0: 64) of 140 landmarks: camera i sees a window of consecutive landmarks (mod 140), the
    windows of the three long lists start 47 apart, so that every landmark is seen at least twice"""
    rng = np.random.default_rng(12)
    m = 140
    starts = (0, 5, 70, 30, 100, 0, 47, 94, 10, 50, 90, 120)
    cam = np.concatenate([np.full(c, i) for i, c in enumerate(CAM_COUNTS)])
    lm = np.concatenate([(s + np.arange(c)) % m for s, c in zip(starts, CAM_COUNTS)])
    assert np.bincount(lm, minlength=m).min() >= 2
    e = rng.permutation(cam.size)
    return _observe(rng, len(CAM_COUNTS), m, cam[e], lm[e])


TINY_N = (1, 2, 5, 8, 9)


def tiny_scene(n):
    """n cameras, 5 landmarks, every camera sees every landmark"""
    rng = np.random.default_rng(100 + n)
    cam, lm = np.repeat(np.arange(n), 5), np.tile(np.arange(5), n)
    e = rng.permutation(cam.size)
    return _observe(rng, n, 5, cam[e], lm[e])


def base_scene():
    """the schur-n40 scene of the trust-region stage tests (xm_rtr_stages.matrix("scene", 40, 60))"""
    return tl.gen_scene(40, 60, 4, 840, noise=0.01, hubs=3)


MASK_ZERO_LANDMARKS = (7, 19)


def mask_scene(dup):
    """the base scene with a tenth of the weights 0 and every weight of MASK_ZERO_LANDMARKS 0; dup: one (camera, landmark) pair named a second
    time, with a point and a weight of its own.  S["w1"]: unit weights to create a context with before the real ones are handed over"""
    S = dict(base_scene())
    rng = np.random.default_rng(77)
    w = S["w"].copy()
    w[rng.choice(w.size, w.size // 10, replace=False)] = 0.0
    w[np.isin(S["lm"], MASK_ZERO_LANDMARKS)] = 0.0
    S["w"] = w
    if dup:
        e = int(np.nonzero((w > 0) & (S["lm"] > 10) & (S["cam"] > 0))[0][5])
        S["cam"] = np.append(S["cam"], S["cam"][e]); S["lm"] = np.append(S["lm"], S["lm"][e])
        S["p"] = np.concatenate([S["p"], S["p"][e:e + 1] + 0.01]); S["w"] = np.append(w, 0.8)
    S["w1"] = np.ones(S["w"].size)
    return S


AGG_REDUCED = (64, 65, 129)             # reduced cameras: one full aggregate | + one of a single row | two full + one of a single row


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "base":
        return base_scene()
    if name == "degrees":
        return degree_scene()
    if name == "cam_degrees":
        return cam_degree_scene()
    if name.startswith("tiny"):
        return tiny_scene(int(name[4:]))
    if name in ("masks", "masks_dup"):
        return mask_scene(name == "masks_dup")
    if name.startswith("agg"):
        return sq.gen_sequential(int(name[3:]) + 1, per_cam=6, seed=int(name[3:]))
    raise KeyError(name)


def obs(S):
    return S["cam"], S["lm"], S["p"], S["w"]


O_OF = {"base": (1, 3, 4, 5, 6, 7, 8, 9, 10), "degrees": (3, 4, 5), "cam_degrees": (3, 6), "masks": (3, 4), "masks_dup": (3,)}
FORMS_OF = {"base": tuple(FORMS), "degrees": tuple(FORMS), "masks": tuple(FORMS), "masks_dup": ("dense", "sym", "host"),
            "cam_degrees": ("dense", "jacobi", "two_level")}
CASES = ("base", "degrees", "cam_degrees", "masks", "masks_dup") + tuple(f"tiny{n}" for n in TINY_N) + tuple(f"agg{k}" for k in AGG_REDUCED)


def o_of(case):
    return O_OF.get(case, (3,))


def forms_of(case):
    return ("two_level",) if case.startswith("agg") else FORMS_OF.get(case, ("dense", "jacobi", "two_level"))


def inputs(case, o):
    """W (3n x o), alpha and X (n1 x 8, the same for every o: four identity columns -- the first and the last row of the first aggregate's
    range, the last reduced camera, one in between -- and four random ones; NID = 4)"""
    S = scene(case)
    n = S["n"]
    W = np.random.default_rng(1000 + o).standard_normal((3 * n, o))
    X = None
    if n > 1:
        n1 = n - 1
        X = np.random.default_rng(999).standard_normal((n1, 8))
        X[:, :NID] = 0.0
        for j, i in enumerate((0, min(AGG - 1, n1 - 1), n1 - 1, n1 // 2)):
            X[i, j] = 1.0
    return W, 1.0 + 0.25 * o, X


NID = 4


# ------------------------------------------------------------------------------------------------ the f64 restatement
def pcg(A, M, B, tol=PCG_TOL, cap=PCG_CAP):
    """the inner solve of xm_schur.hip restated: the columns advance together, each with its own alpha and beta; stops when every column has
    |r|^2 / |b|^2 <= tol^2 (tested before the direction update of iterations >= 1) or after cap iterations.  Returns x, iterations, relres"""
    x = np.zeros_like(B); r = B.copy(); z = M(r); p = z.copy()
    rz = (r * z).sum(axis=0); bb = (B * B).sum(axis=0); rr = bb.copy()
    it, worst = 0, 1.0
    while True:
        if it > 0:
            q = np.where(bb > 0, rr / np.where(bb > 0, bb, 1), 0.0)
            worst = float(np.sqrt(q.max()))
            if np.all(q <= tol * tol) or it >= cap:
                break
            p = z + np.where(rzo > 0, rz / np.where(rzo > 0, rzo, 1), 0.0) * p
        Ap = A(p)
        pap = (p * Ap).sum(axis=0)
        ok = (pap > 0) & (rz > 0)
        a = np.where(ok, rz / np.where(ok, pap, 1), 0.0)
        x += a * p; r -= a * Ap
        rr = (r * r).sum(axis=0)
        z = M(r); rzo = rz; rz = (r * z).sum(axis=0)
        it += 1
    return x, it, worst


def f64_stages(S, kind, W=None, alpha=1.0, X=None, perm=None, order=None, damage=None):
    """the quantities of xm_schur_exact.Exact (setup, chain, pieces) in f64, the observations summed in the order `order`; xc as the form does
    it: kind "dense": inv(VT) @ r | "jacobi", "two_level": pcg() with that preconditioner.  perm: the aggregates' table (two_level).  damage: a
    dict of deliberate faults for the test that the bounds bite (test_schur_exact.py):
      h_row = l: h_l off by 1e3 ulp | skip_observation = i: the last observation of camera i is left out of every sum |
      pad_row = a: the padding rows of aggregate a are counted in the coarse operator's diagonal | block_pair = a: one off-diagonal pair of
      aggregate a's block is left out before it is inverted"""
    damage = damage or {}
    n, m = S["n"], S["m"]
    cam, lm, p, w = (np.asarray(S[k]) for k in ("cam", "lm", "p", "w"))
    cam, lm = cam.astype(np.int64), lm.astype(np.int64)
    w = w.astype(np.float64).copy()
    if order is not None:
        cam, lm, p, w = cam[order], lm[order], p[order], w[order]
    if "skip_observation" in damage:
        w[np.nonzero(cam == damage["skip_observation"])[0][-1]] = 0.0
    n1 = n - 1

    def add(shape, idx, vals):
        out = np.zeros(shape)
        np.add.at(out, idx, vals)
        return out
    Q1 = add((n, 3, 3), cam, w[:, None, None] * p[:, :, None] * p[:, None, :])
    c = add((n, 3), cam, w[:, None] * p)
    q2 = add((n,), cam, w)
    Q3 = add((m,), lm, w)
    q3inv = np.where(Q3 > 0, 1.0 / np.where(Q3 > 0, Q3, 1.0), 0.0)
    out = {"Q1": Q1.reshape(n, 9), "c": c, "q2": q2[:, None], "q3inv": q3inv[:, None]}
    VT = None
    if n1 > 0:
        V3b = sp.coo_matrix((w, (cam, lm)), shape=(n, m)).tocsr()[1:]
        VT = np.diag(q2[1:]) - (V3b.multiply(q3inv[None, :]) @ V3b.T).toarray()
        VT = 0.5 * (VT + VT.T)
        dinv = 1.0 / np.diag(VT)
        out["dinv"] = dinv[:, None]
        if kind == "dense":
            VTinv = np.linalg.inv(VT)
            out["VTinv"] = 0.5 * (VTinv + VTinv.T)
    M = None
    if n1 > 0 and kind == "jacobi":
        M = lambda R: dinv[:, None] * R
    if n1 > 0 and kind == "two_level":
        perm = np.asarray(perm)
        na = perm.shape[0]
        binv = np.zeros((na, AGG, AGG)); P = np.zeros((n1, na))
        members = []
        for a in range(na):
            rows = np.nonzero(perm[a] >= 0)[0]
            idx = perm[a][rows]
            members.append((rows, idx))
            blk = VT[np.ix_(idx, idx)].copy()
            if damage.get("block_pair") == a and idx.size > 1:
                blk[0, 1] = blk[1, 0] = 0.0
            binv[a] = np.eye(AGG)
            binv[a][np.ix_(rows, rows)] = np.linalg.inv(blk)
            P[idx, a] = 1.0
        Ac = P.T @ VT @ P
        if "pad_row" in damage:
            a = damage["pad_row"]
            Ac[a, a] += AGG - members[a][0].size
        ainv = np.linalg.inv(0.5 * (Ac + Ac.T))
        ainv = 0.5 * (ainv + ainv.T)
        out.update(binv=binv.reshape(na, -1), ainv=ainv.reshape(1, -1))

        def M(R):
            Z = np.zeros_like(R)
            for a, (rows, idx) in enumerate(members):
                Z[idx] = binv[a][np.ix_(rows, rows)] @ R[idx]
            return Z + P @ (ainv @ (P.T @ R))
    if W is not None:
        W = np.asarray(W, dtype=np.float64).reshape(3 * n, -1)
        o = W.shape[1]
        Wc = W.reshape(n, 3, o)
        h = -q3inv[:, None] * add((m, o), lm, w[:, None] * np.einsum("ea,eak->ek", p, Wc[cam]))
        if "h_row" in damage:
            h[damage["h_row"]] *= 1.0 + 1e3 * EPS
        r = np.einsum("ia,iak->ik", c, Wc) + add((n, o), cam, w[:, None] * h[lm])
        xc = np.zeros((n, o))
        if n1 > 0:
            if kind == "dense":
                xc[1:] = out["VTinv"] @ r[1:]
            else:
                xc[1:], out["pcg_iters"], out["pcg_relres"] = pcg(lambda V: VT @ V, M, r[1:])
        xl = h + q3inv[:, None] * add((m, o), lm, w[:, None] * xc[cam])
        Y = np.einsum("iab,ibk->iak", Q1, Wc) - c[:, :, None] * xc[:, None, :] + add((n, 3, o), cam, w[:, None, None] * p[:, :, None] * xl[lm][:, None, :])
        out.update(h=h, r=r[1:], xc=xc[1:], xl=xl, Y=alpha * Y.reshape(n, 3 * o))
    if X is not None and n1 > 0 and kind != "dense":
        X = np.asarray(X, dtype=np.float64).reshape(n1, -1)
        red = cam >= 1
        y = q3inv[:, None] * add((m, X.shape[1]), lm[red], w[red, None] * X[cam[red] - 1])
        VX = q2[1:, None] * X - add(X.shape, cam[red] - 1, w[red, None] * y[lm[red]])
        out.update(VX=VX, pAp=(X * VX).sum(axis=0)[:, None], MX=M(X))
    return out


# ------------------------------------------------------------------------------------------------ references (computed once, left unchanged)
@functools.lru_cache(maxsize=None)
def exact_op(case):
    S = scene(case)
    return ex.Exact(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"])


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray) and v.flags.owndata:
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def exact_setup(case):
    return _freeze(exact_op(case).setup(dense=True))


@functools.lru_cache(maxsize=None)
def exact_chain(case, o):
    W, alpha, _ = inputs(case, o)
    return _freeze(exact_op(case).chain(W, alpha))


def as_perm(perm):
    return None if perm is None else tuple(map(tuple, np.asarray(perm).tolist()))


@functools.lru_cache(maxsize=None)
def exact_pieces(case, perm):
    """perm: as_perm(table) or None"""
    _, _, X = inputs(case, 3)
    E = exact_op(case).pieces(X, None if perm is None else np.array(perm))
    return _freeze(E)


def exact_all(case, kind, o, perm=None):
    """every compared quantity of (case, kind) at o columns under the probe's keys"""
    E = dict(exact_setup(case))
    E.update(exact_chain(case, o))
    if kind != "dense" and scene(case)["n"] > 1:
        P = exact_pieces(case, as_perm(perm) if kind == "two_level" else None)
        E.update(P)
        E["MX"] = P["MX_" + kind]
        if "MX_" + kind + "~" in P:
            E["MX~"] = P["MX_" + kind + "~"]
    return E


@functools.lru_cache(maxsize=None)
def _reference_errors(case, kind, o, perm):
    S = scene(case)
    W, alpha, X = inputs(case, o)
    pm = None if perm is None else np.array(perm)
    E = exact_all(case, kind, o, pm)
    order = np.random.default_rng(5).permutation(len(S["cam"]))
    runs = [f64_stages(S, kind, W, alpha, X, pm, order=od) for od in (None, order)]
    keys = keys_of(kind, S["n"] - 1)
    e = {k: max(err(r[k], E[k], E.get(k + "~"))[0] for r in runs) for k in keys}
    e["pcg_iters"] = tuple(r.get("pcg_iters", 0) for r in runs)
    return e


def reference_errors(case, kind, o, perm=None):
    """e_ref per key: the larger of the f64 restatement's errors in the given and in a permuted observation order"""
    return _reference_errors(case, kind, o, as_perm(perm) if kind == "two_level" else None)


def plan_perm(xmamd, case):
    """the aggregates' table from the library's host plan (xm_schur_aggregate_plan), members in index order"""
    S = scene(case)
    return ex.perm_from_plan(xmamd.schur_aggregate_plan(S["cam"], S["lm"], S["n"]))


def shape_probe(g, n, m):
    """the probe's arrays as (blocks, entries), under the keys of the exact dict"""
    out = dict(g)
    for k in ("q2", "q3inv", "dinv", "pAp"):
        if k in g:
            out[k] = np.asarray(g[k]).reshape(-1, 1)
    if "Q1" in g:
        out["Q1"] = np.asarray(g["Q1"]).reshape(n, 9)
    if "Y" in g:
        out["Y"] = np.ascontiguousarray(g["Y"]).reshape(n, -1)
    if "binv" in g:
        out["binv"] = np.asarray(g["binv"]).reshape(g["binv"].shape[0], -1)
        out["ainv"] = np.ascontiguousarray(g["ainv"]).reshape(1, -1)
    return out


def compare(label, got, E, e_ref, keys, who="gpu"):
    """prints one line per key (the table of profiles/r19_schur_stage_errors.txt) and returns the keys that miss the bound"""
    bad = []
    for k in keys:
        e, blk = err(got[k], E[k], E.get(k + "~"))
        ratio = e / e_ref[k] if e_ref[k] > 0 else (0.0 if e == 0 else float("inf"))
        print(f"STAGE_ERR {label} {k}: e_ref {e_ref[k]:.3e} e_{who} {e:.3e} ratio {ratio:.3g} bound {bound(e_ref[k]):.3e} worst block {blk}")
        if not e <= bound(e_ref[k]):
            bad.append((k, e, e_ref[k], blk))
    return bad
