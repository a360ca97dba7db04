"""What tests/test_ba_exact.py (CPU) and tests/test_gpu_ba_stages.py (GPU) share: the scenes, the quantities of one linearisation from the
longdouble reference (xm_ba_exact.py) and from the f64 restatements (xm_ba_numpy.py, xm_ba_loss_numpy.py, xm_ba_precond_numpy.py) under
the same keys, the error function and the bound.

Error: max |x - x_exact| / max |x_exact| per natural block (landmark for vinv / g_l / dP, camera block row for b / SX / S / ustar / sinv / Pm,
column for MX and Ac), then the maximum over blocks; a block whose exact value is 0 must be 0.  Bound: with e_ref the f64 restatement's own
error against the longdouble reference at the same point (the larger of two evaluations, the second with the observations permuted), the
code under test must reach e <= max(16 e_ref, 64 eps_f64)."""
import numpy as np
import scipy.sparse as sp

import xm_ba_exact as ex
import xm_ba_loss_numpy as rl
import xm_ba_numpy as ba
import xm_ba_precond_numpy as bp

LD = ex.LD
EPS = float(np.finfo(np.float64).eps)
KINDS = ("jacobi", "blocks", "two_level")
MAX_E_REF = 1e-8          # a scene whose reference is worse than this for a compared quantity is not a scene to judge a kernel on


def err(x, xe, scale=None):
    """(error, index of the worst block); x, xe: (blocks, ...); scale (per block, optional): a lower limit of the denominator -- the magnitude
    of the terms the block is formed from, where the exact block itself may cancel to nothing (xm_rtr_exact.py)"""
    xe = np.asarray(xe, dtype=LD)
    xe = xe.reshape(xe.shape[0] if xe.ndim else 1, -1)
    x = np.asarray(x, dtype=LD).reshape(xe.shape)
    num, den = np.abs(x - xe).max(axis=1), np.abs(xe).max(axis=1)
    if scale is not None:
        den = np.maximum(den, np.asarray(scale, dtype=LD).reshape(-1))
    e = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num > 0, np.inf, 0))
    return float(e.max()), int(e.argmax())


def bound(e_ref):
    return max(16.0 * e_ref, 64.0 * EPS)


def lower_blocks(A, cd):
    """the lower block triangle of a square matrix (blocks of cd), the rest 0"""
    nb = A.shape[0] // cd
    mask = np.kron(np.tril(np.ones((nb, nb))), np.ones((cd, cd))) > 0
    return np.where(mask, A, 0)


def plan_order(S):
    return bp.aggregate_plan(S["cam"], S["lm"], S["n"], ba.used_mask(S["p"], S["w"]))[1]


def compact_basis(Pm, order, n, cd):
    """cd n x NC ncoarse -> cd n x NC: every camera's rows of its own coarse aggregate's columns (the library's storage)"""
    nc = 7 if cd == 6 else 4
    out = np.zeros((cd * n, nc), dtype=Pm.dtype)
    for a, (k0, k1) in enumerate(bp.coarse_ranges(len(order))):
        for i in order[k0:k1]:
            out[cd * i:cd * i + cd] = Pm[cd * i:cd * i + cd, nc * a:nc * a + nc]
    return out


def shape_blocks(key, v, n, m, cd):
    """the array of a quantity as (blocks, entries)"""
    v = np.asarray(v)
    if key in ("b", "ustar", "sinv", "S", "SX", "Pm") or key.startswith("SX"):
        return v.reshape(n, -1) if key in ("b", "ustar", "sinv") else v.reshape(n, cd, -1).reshape(n, -1)
    if key in ("g_l", "vinv", "dP"):
        return v.reshape(m, -1)
    if key.startswith("MX") or key == "Ac":
        return v.T.reshape(v.shape[1], -1)
    if key == "rot1":
        return np.stack([v[:, 3 * i:3 * i + 3].reshape(-1) for i in range(n)])
    if key in ("t1", "p1"):
        return v.T
    return v.reshape(1, -1) if key in ("cost", "cost1", "model", "gmax") else v.reshape(-1, 1)     # scalars; step2 / x2: one block each


def exact_stages(S, rot, t, P, mu, fix=False, loss="trivial", a=0.0, order=None, kinds=(), X=None, dc=None):
    E = ex.Exact(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], rot, t, P, mu, fix, loss, a)
    cd = E.cd
    out = dict(cost=E.cost, gmax=E.gmax, b=E.b, g_l=E.g_l, vinv=E.vinv6(), ustar=E.Ustar, sinv=E.Sinv, S=lower_blocks(E.S, cd), _E=E,
               cused=E.cused, lused=E.lused, n_used=E.n_used)
    if X is not None:
        X = np.asarray(X, dtype=LD)
        out["SX"] = E.S @ X
        for kind in kinds:
            out["MX_" + kind] = E.precond(kind, order) @ X
    if "two_level" in kinds:
        Pm, dropped = E.rigid_basis(order)
        out["Pm"] = compact_basis(Pm, order, E.n, cd)
        out["dropped"] = dropped
        out["Ac"] = lower_blocks(E.coarse_operator(Pm, dropped), Pm.shape[1] // len(bp.coarse_ranges(len(order))))
    if dc is not None:
        c = E.candidate(dc)
        out.update(dP=c["dP"], rot1=c["rot1"], t1=c["t1"], p1=c["P1"].T, cost1=c["cost1"], model=c["model"],
                   step2=np.array(c["step2"]), x2=np.array(c["x2"], dtype=LD))
    return out


def f64_stages(S, rot, t, P, mu, fix=False, loss="trivial", a=0.0, order=None, kinds=(), X=None, dc=None, perm=None, damage=None):
    """the same quantities from the f64 restatements, the observations in the order perm.  damage: a dict of deliberate faults for the
    test that the bounds bite (test_ba_exact.py)"""
    damage = damage or {}
    n, m = S["n"], S["m"]
    cam, lm, p, w = (np.asarray(S[k]) for k in ("cam", "lm", "p", "w"))
    if perm is not None:
        cam, lm, p, w = cam[perm], lm[perm], p[perm], w[perm]
    if "skip_observation" in damage:                       # (landmark, which of its used observations): left out of the landmark's sums
        l, q = damage["skip_observation"]
        w = w.copy()
        w[np.nonzero((lm == l) & ba.used_mask(p, w))[0][q]] = 0.0
    pr = rl.RobustProblem(cam, lm, p, w, n, m, fix, loss, a)
    cd = pr.cd
    Rcw, tcw = ba.to_world_to_camera(rot, t)
    Pw = np.asarray(P, dtype=np.float64).T.copy()
    F, r, J = pr.corrected(Rcw, tcw, Pw)
    H = (J.T @ J).tocsc()
    g = J.T @ r
    D = np.clip(H.diagonal(), 1e-6, 1e32)
    if damage.get("no_clamp"):
        D = H.diagonal()
    H = (H + sp.diags(mu * D)).tocsr()
    nc_ = cd * n
    U, W, V = H[:nc_, :nc_], H[:nc_, nc_:], H[nc_:, nc_:].tocoo()
    Vd = np.zeros((m, 3, 3))
    Vd[V.row // 3, V.row % 3, V.col % 3] = V.data
    Vi = np.linalg.inv(Vd)
    Vinv = sp.block_diag(list(Vi), format="csr")
    Ssp = (U - W @ Vinv @ W.T).tocsr()
    b = -g[:nc_] + W @ (Vinv @ g[nc_:])
    Sd = Ssp.toarray()
    Ud = U.toarray()
    out = dict(cost=F, gmax=float(np.abs(g).max(initial=0.0)), b=b, g_l=g[nc_:].reshape(m, 3),
               vinv=np.stack([Vi[:, 0, 0], Vi[:, 0, 1], Vi[:, 0, 2], Vi[:, 1, 1], Vi[:, 1, 2], Vi[:, 2, 2]], axis=1),
               ustar=np.stack([Ud[cd * i:cd * i + cd, cd * i:cd * i + cd] for i in range(n)]),
               sinv=np.stack([np.linalg.inv(Sd[cd * i:cd * i + cd, cd * i:cd * i + cd]) for i in range(n)]), S=lower_blocks(Sd, cd))
    if X is not None:
        out["SX"] = Ssp @ X
        Sp = Ssp
        if "drop_pair" in damage:                           # one off-diagonal camera pair of one aggregate block
            i, j = damage["drop_pair"]
            Sp = Ssp.tolil()
            Sp[cd * i:cd * i + cd, cd * j:cd * j + cd] = 0.0; Sp[cd * j:cd * j + cd, cd * i:cd * i + cd] = 0.0
            Sp = Sp.tocsr()
        for kind in kinds:
            if kind == "jacobi":
                M = bp.jacobi_inverse(Ssp, cd)
                out["MX_jacobi"] = M @ X
            elif kind == "blocks":
                out["MX_blocks"] = bp.block_inverse(Sp, order, bp.AGG_CAMS, cd) @ X
            else:
                o2 = order
                if damage.get("leave_out_merged"):           # the merged member is missing from the last coarse aggregate
                    o2 = order[:-1]
                Pm, dropped = bp.rigid_basis(Rcw, tcw, o2, bp.AGG_CAMS, fix)
                Bi = bp.block_inverse(Sp, order, bp.AGG_CAMS, cd)
                Ac = bp.coarse_operator(Ssp, Pm, dropped)
                if "swap_coarse" in damage:                  # two columns of P swapped after A_c was formed: the coarse solve no longer fits them
                    q0, q1 = damage["swap_coarse"]
                    Pm = Pm.toarray(); Pm[:, [q0, q1]] = Pm[:, [q1, q0]]; Pm = sp.csr_matrix(Pm)
                out["MX_two_level"] = Bi @ X + Pm @ (np.linalg.inv(Ac) @ (Pm.T @ X))
    if "two_level" in kinds:
        Pm, dropped = bp.rigid_basis(Rcw, tcw, order, bp.AGG_CAMS, fix)
        out["Pm"] = compact_basis(Pm.toarray(), order, n, cd)
        out["dropped"] = dropped
        Ac = bp.coarse_operator(Ssp, Pm, dropped)
        if "swap_coarse" in damage:
            q0, q1 = damage["swap_coarse"]
            Ac[:, [q0, q1]] = Ac[:, [q1, q0]]
        out["Ac"] = lower_blocks(Ac, 7 if cd == 6 else 4)
    if dc is not None:
        dc = np.asarray(dc, dtype=np.float64).reshape(-1)
        dP = -(Vinv @ (g[nc_:] + W.T @ dc))
        dP.reshape(m, 3)[~pr.lused] = 0.0
        d = np.concatenate([dc, dP])
        Jd = J @ d
        Rn, tn, Pn = pr.plus(Rcw, tcw, Pw, d)
        rot1, t1 = ba.to_camera_to_world(Rn, tn)
        cu, lu = pr.cused, pr.lused
        out.update(dP=dP.reshape(m, 3), rot1=rot1, t1=t1, p1=Pn.T, cost1=pr.cost(Rn, tn, Pn), model=float(r @ Jd) + 0.5 * float(Jd @ Jd),
                   step2=np.array([np.sum(dc.reshape(n, cd)[cu] ** 2), np.sum(dP.reshape(m, 3)[lu] ** 2)]),
                   x2=np.array([(cu.sum() if cd == 6 else 0) + np.sum(tcw[cu] ** 2), np.sum(Pw[lu] ** 2)]))
    return out


def reference_errors(S, exact, keys, seed=0, **kw):
    """e_ref per key: the larger of the f64 restatement's errors in the given and in a permuted observation order"""
    n, m, cd = S["n"], S["m"], exact["_E"].cd
    perm = np.random.default_rng(seed).permutation(len(S["cam"]))
    runs = [f64_stages(S, perm=None, **kw), f64_stages(S, perm=perm, **kw)]
    return {k: max(err(shape_blocks(k, r[k], n, m, cd), shape_blocks(k, exact[k], n, m, cd))[0] for r in runs) for k in keys}


def compare(label, S, got, exact, e_ref, keys, who="gpu"):
    """prints one line per key (the table of profiles/r12_ba_stage_errors.txt) and returns the keys that miss the bound"""
    n, m, cd = S["n"], S["m"], exact["_E"].cd
    bad = []
    for k in keys:
        e, blk = err(shape_blocks(k, got[k], n, m, cd), shape_blocks(k, exact[k], n, m, cd))
        ratio = e / e_ref[k] if e_ref[k] > 0 else (0.0 if e == 0 else float("inf"))
        print(f"STAGE_ERR {label} {k}: e_ref {e_ref[k]:.3e} e_{who} {e:.3e} ratio {ratio:.3g} bound {bound(e_ref[k]):.3e} worst block {blk}")
        if not e <= bound(e_ref[k]):
            bad.append((k, e, e_ref[k], blk))
    return bad


# ------------------------------------------------------------------------------------------------ scenes (each: the scene dict and a point)
def _with(S, keep=None, extra=None, **over):
    """a copy of scene S with the observations keep (indices) followed by the observations extra (indices, may repeat)"""
    idx = np.arange(len(S["cam"])) if keep is None else np.asarray(keep)
    if extra is not None:
        idx = np.concatenate([idx, np.asarray(extra, dtype=idx.dtype)])
    out = dict(S)
    for k in ("cam", "lm", "p", "w"):
        out[k] = np.asarray(S[k])[idx].copy()
    out.update(over)
    return out


def base_scene():
    """the scene and far start of test_gpu_ba.py::test_trace_follows_the_numpy_lm"""
    S = ba.ring_scene(n_cams=20, n_pts=200, seed=20, noise=0.05)
    return S, ba.perturb(S["rot"], S["t"], S["P"], seed=21, deg=40.0, rel=0.4)


DEGREES = (1, 2, 63, 64, 65, 66)


def degree_scene():
    """ring_scene(72, 120, frac=0.93) with seven of its landmarks (the ones seen most often, `roles`) changed: roles[k], k = 0..5, cut to
    DEGREES[k] observations and roles[6] brought above 1024 by naming each of its observations 16 times.  Returns (scene, point, roles,
    degrees of the roles)"""
    S0 = ba.ring_scene(n_cams=72, n_pts=120, seed=31, frac=0.93, noise=0.02)
    lm = np.asarray(S0["lm"])
    cnt = np.bincount(lm, minlength=120)
    roles = [int(l) for l in np.argsort(-cnt, kind="stable")[:7]]
    assert cnt[roles].min() >= 66
    keep = []
    for l in range(120):
        e = np.nonzero(lm == l)[0]
        keep += list(e[:DEGREES[roles.index(l)]] if l in roles[:6] else e)
    S = _with(S0, np.sort(np.array(keep)), np.tile(np.nonzero(lm == roles[6])[0], 15))
    deg = np.bincount(S["lm"], minlength=120)
    return S, ba.perturb(S["rot"], S["t"], S["P"], seed=32, deg=3.0, rel=0.02), roles, deg[roles]


def mask_scene():
    """ring scene with duplicated (camera, landmark) pairs, observations of weight 0 (S["w"]; the context is created with S["w0"] = 1
    everywhere, so that the rotation-averaging problem stays connected, and given S["w"] afterwards) and of p_2 <= 0; camera 5 and landmark 7
    have no used observation (every one of theirs lies behind the camera)"""
    S0 = ba.ring_scene(n_cams=24, n_pts=150, seed=41, frac=0.5, noise=0.01)
    rng = np.random.default_rng(42)
    ne = len(S0["cam"])
    S = _with(S0, None, rng.choice(ne, 60, replace=False))
    w, p = S["w"].copy(), S["p"].copy()
    off = rng.choice(ne, 80, replace=False)
    w[off[:40]] = 0.0
    p[off[40:60]] *= -1.0                                  # p_2 < 0
    p[off[60:], 2] = 0.0                                   # p_2 = 0
    gone = (S["cam"] == 5) | (S["lm"] == 7)
    p[gone] = -np.abs(p[gone])
    S["w0"], S["w"], S["p"] = np.ones(len(w)), w, p
    return S, ba.perturb(S["rot"], S["t"], S["P"], seed=43, deg=3.0, rel=0.02)


def clamp_scene():
    """a 12-camera ring scene with every third landmark moved 3e2 .. 1e5 away, so that diag(J_P^T J_P) lies below 1e-6 for some landmarks
    and above for others; only observations in front of their cameras are kept, and they are re-observed from the moved points"""
    S0 = ba.ring_scene(n_cams=12, n_pts=80, seed=51, frac=0.6, noise=0.0)
    rng = np.random.default_rng(52)
    Pw = S0["P"].T.copy()
    far = np.arange(0, 80, 3)
    dirs = rng.standard_normal((far.size, 3)); dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    Pw[far] = dirs * np.exp(rng.uniform(np.log(3e2), np.log(1e5), far.size))[:, None]
    Rcw, tcw = ba.to_world_to_camera(S0["rot"], S0["t"])
    X = np.einsum("kab,kb->ka", Rcw[S0["cam"]], Pw[S0["lm"]]) + tcw[S0["cam"]]
    front = np.nonzero(X[:, 2] > 1.0)[0]
    S = _with(S0, front, P=Pw.T.copy())
    S["p"] = ba._observe(Rcw, tcw, Pw, S["cam"], S["lm"], rng, 1e-3)
    rot, t, _ = ba.perturb(S["rot"], S["t"], S["P"], seed=53, deg=1.0, rel=0.0)
    return S, (rot, t + 0.01 * rng.standard_normal(t.shape), S["P"] * (1.0 + 1e-3 * rng.standard_normal(S["P"].shape)))


def aggregate_scene(n_cams, shuffle=False):
    """a sequential capture of n_cams cameras (16 q + r members); shuffle: the cameras renumbered at random"""
    S = ba.sequential_scene(n_cams=n_cams, per_cam=8, seed=60 + n_cams, noise=1e-3)
    if shuffle:
        rng = np.random.default_rng(7)
        new = rng.permutation(n_cams)                      # new number of camera i
        inv = np.argsort(new)
        S["cam"] = new[S["cam"]].astype(np.int32)
        S["rot"] = np.concatenate([S["rot"][:, 3 * i:3 * i + 3] for i in inv], axis=1)
        S["t"] = S["t"][:, inv].copy()
    return S, ba.perturb(S["rot"], S["t"], S["P"], seed=61, deg=1.0, rel=0.002)


def one_centre_scene():
    """sixteen cameras at distinct places (0..15) and sixteen turning about the origin (16..31, tcw = 0 exactly): the second aggregate's
    scale column has norm 0 and is dropped (the construction of test_gpu_ba_precond.py).  The point is the scene itself, with the landmarks
    moved: the centres must stay where they are"""
    rng = np.random.default_rng(95)
    yaw = np.linspace(-0.3, 0.3, 16)
    Cc = np.zeros((32, 3))
    Cc[:16] = np.stack([np.linspace(-3, 3, 16), np.full(16, -1.0), rng.uniform(-0.5, 0.5, 16)], axis=1)
    tgt = [np.array([0.0, 6.0, 0.0])] * 16 + [np.array([6 * np.sin(y), 6 * np.cos(y), 0.0]) for y in yaw]
    Rcw = np.stack([ba._look_at(Cc[i], tgt[i], rng, 0.05) for i in range(32)])
    tcw = -np.einsum("iab,ib->ia", Rcw, Cc)
    m = 15 + 600
    Pw = np.stack([rng.uniform(-2, 2, m), rng.uniform(5, 7, m), rng.uniform(-1.5, 1.5, m)], axis=1)
    cams, lms = [], []
    for l in range(15):
        cams += [0, l + 1]; lms += [l, l]
    for l in range(15, m):
        s = np.concatenate([np.sort(rng.choice(16, 2, replace=False)), 16 + np.sort(rng.choice(16, 2, replace=False))])
        cams += list(s); lms += [l] * 4
    cams, lms = np.array(cams), np.array(lms)
    S = ba._pack(Rcw, tcw, Pw, cams, lms, ba._observe(Rcw, tcw, Pw, cams, lms, rng, 1e-3))
    return S, (S["rot"], S["t"], S["P"] + 0.01 * rng.standard_normal(S["P"].shape))


LOSS_SCALE = 0.05


def loss_scene(loss):
    """ring scene whose observations have |r|^2 far below a^2 (the first third), about a^2, and 1e6 times above (the last tenth: the measured
    point moved by 1e3 a); for Huber two observations are set so that s == a * a exactly in f64 and s == nextafter(a * a) (returned)"""
    S = ba.ring_scene(n_cams=16, n_pts=120, seed=71, frac=0.5, noise=0.0)
    rng = np.random.default_rng(72)
    ne = len(S["cam"])
    a = LOSS_SCALE
    sig = np.where(np.arange(ne) < ne // 3, 1e-4 * a, a)
    u = S["p"][:, :2] / S["p"][:, 2:3] + sig[:, None] * rng.standard_normal((ne, 2))
    big = np.arange(ne) >= ne - ne // 10
    u[big] += 1e3 * a * np.array([0.6, 0.8])
    S["p"] = np.concatenate([u, np.ones((ne, 1))], axis=1)
    point = (S["rot"], S["t"], S["P"])                    # the generating point: the residuals are the offsets above, up to rounding
    edge = []
    if loss == "huber":
        edge = _huber_edge(S, point, a)
    return S, point, a, edge


def _huber_edge(S, point, a):
    """moves the measurements of observations 0 and 1 (p_2 = 1, so q / q_2 is exact) until the f64 residual, evaluated with the eval
    kernel's expression, has s == a * a and s == nextafter(a * a, inf); returns [(observation, s)]"""
    Rcw, tcw = ba.to_world_to_camera(*point[:2])
    out = []
    for e, target in ((0, a * a), (1, np.nextafter(a * a, np.inf))):
        i, l = S["cam"][e], S["lm"][e]
        X = Rcw[i] @ point[2][:, l] + tcw[i]
        u0, u1 = X[0] / X[2], X[1] / X[2]
        S["p"][e, 1] = u1                                  # r_1 = 0 exactly
        q = u0 - np.sqrt(target)
        for _ in range(200):                               # walk q over neighbouring doubles until (u0 - q)^2 rounds to the target
            s = (u0 - q) * (u0 - q)
            if s == target:
                break
            q = np.nextafter(q, np.inf if s > target else -np.inf)
        S["p"][e, 0] = q
        out.append((e, float((u0 - q) * (u0 - q))))
    return out


STEP_NORMS = (0.0, 1e-200, 9.9e-9, 1e-8, 1.01e-8, 1e-3, 1.0, np.pi - 1e-9, np.pi, 4.0)


def step_vector(n, cd, seed=81):
    """dc whose rotation parts have the norms STEP_NORMS (cameras 0 .. 9, then random small ones), random translations"""
    rng = np.random.default_rng(seed)
    dc = 1e-2 * rng.standard_normal((n, cd))
    if cd == 6:
        for i, nm in enumerate(STEP_NORMS):
            d = rng.standard_normal(3)
            dc[i, :3] = d / np.linalg.norm(d) * nm
    return dc.reshape(-1)


# ------------------------------------------------------------------------------------------------ cases (the CPU and the GPU test run the same ones)
ALL_KEYS = ("cost", "gmax", "b", "g_l", "vinv", "ustar", "sinv", "S", "SX", "MX_jacobi", "MX_blocks", "MX_two_level", "Pm", "Ac", "dP", "rot1", "t1",
            "p1", "cost1", "model", "step2", "x2")
AGG_SIZES = (16, 17, 18, 31, 32, 33, 34, 47)              # 16 q + r for q in 1, 2 and r in 0, 1, 2, 15
CASES = ("base", "degrees", "masks", "clamp") + tuple(f"agg{k}" for k in AGG_SIZES) + ("one_centre", "shuffled33") + \
        tuple("loss_" + k for k in rl.LOSSES[1:]) + ("step",)


def aggregate_columns(order, n, cd, seed=5):
    """the identity columns of the first and of the last block aggregate, then 8 random vectors; returns (X, number of identity columns)"""
    first, last = order[:bp.AGG_CAMS], order[(len(order) - 1) // bp.AGG_CAMS * bp.AGG_CAMS:]
    mem = list(first) + [i for i in last if i not in set(first)]
    rows = (cd * np.asarray(mem)[:, None] + np.arange(cd)[None, :]).reshape(-1)
    X = np.zeros((cd * n, rows.size + 8))
    X[rows, np.arange(rows.size)] = 1.0
    R = np.random.default_rng(seed).standard_normal((cd * n, 8))
    member = np.zeros(n, dtype=bool); member[order] = True
    R[np.repeat(~member, cd)] = 0.0                        # as the PCG's vectors: 0 on cameras without a used observation
    X[:, rows.size:] = R
    return X, rows.size


def case(name, fix):
    """dict: S, point (rot, t, P), mus, loss, a, order, kinds, X, dc, keys (the compared quantities), nid (identity columns of X), extra"""
    cd = 3 if fix else 6
    loss, a, extra, mus, keys, nid = "trivial", 0.0, {}, (1e-4,), ALL_KEYS, 0
    if name == "base":
        S, point = base_scene()
        mus = (1e-4, 1.0, 1e6)
    elif name == "degrees":
        S, point, extra["roles"], extra["degrees"] = degree_scene()
        keys = ("vinv", "g_l", "b", "SX", "S", "dP", "Ac", "MX_jacobi", "MX_blocks", "MX_two_level")
    elif name == "masks":
        S, point = mask_scene()
        mus = (1e-2,)
    elif name == "clamp":
        S, point = clamp_scene()
        mus = (1.0,)
        keys = ("vinv", "S", "b", "ustar", "g_l", "SX", "dP")
    elif name.startswith("agg") or name in ("one_centre", "shuffled33"):
        S, point = one_centre_scene() if name == "one_centre" else aggregate_scene(33, True) if name == "shuffled33" else aggregate_scene(int(name[3:]))
        keys = ("MX_jacobi", "MX_blocks", "MX_two_level", "Pm", "Ac", "S", "b")
    elif name.startswith("loss_"):
        loss = name[5:]
        S, point, a, extra["edge"] = loss_scene(loss)
        mus = (1e-2,)
        keys = ("cost", "b", "g_l", "cost1", "model")
    elif name == "step":
        S, point = base_scene()
        keys = ("rot1", "t1", "p1", "step2", "x2", "model", "cost1", "dP")
    else:
        raise ValueError(name)
    n = S["n"]
    order = plan_order(S)
    rng = np.random.default_rng(3)
    if name.startswith("agg") or name in ("one_centre", "shuffled33"):
        X, nid = aggregate_columns(order, n, cd)
    else:
        X = rng.standard_normal((cd * n, 4))
        X[np.repeat(~np.isin(np.arange(n), order), cd)] = 0.0
    dc = step_vector(n, cd) if name == "step" else 1e-2 * rng.standard_normal(cd * n)
    return dict(S=S, point=point, mus=mus, loss=loss, a=a, order=order, kinds=KINDS, X=X, dc=dc, keys=keys, nid=nid, extra=extra, fix=fix)


def stage_args(c, mu):
    rot, t, P = c["point"]
    return dict(rot=rot, t=t, P=P, mu=mu, fix=c["fix"], loss=c["loss"], a=c["a"], order=c["order"], kinds=c["kinds"], X=c["X"], dc=c["dc"])
