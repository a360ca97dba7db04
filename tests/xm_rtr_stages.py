"""What tests/test_rtr_exact.py (CPU) and tests/test_gpu_rtr_stages.py (GPU) share: the matrices, the points, the paths (which context a case
is run on), the quantities of every stage from the longdouble reference and from its f64 run (xm_rtr_exact.py) under the same keys, and
the comparison.  Error and bound are those of the bundle adjustment's stage tests (xm_ba_stages.err / bound): per quantity and case
e <= max(16 e_ref, 64 eps_f64), e_ref the f64 run's own error against longdouble at the same point; errors are taken per camera block
against the larger of the exact block and the magnitude of the terms it is formed from (the "~" entries of xm_rtr_exact.py)."""
import functools

import numpy as np

import xm_ba_stages as st
import xm_rtr_exact as ex
import xm_testlib as tl

LD = ex.LD
EPS = st.EPS
MAX_E_REF = st.MAX_E_REF
LAMS = (0.0, 10.0, 1000.0)
GRAD_KEYS = ("f", "rr", "G", "egs", "S0", "rgR", "rgs")
HESS_KEYS = ("HpR", "Hps", "pHp", "rHp", "HpHp")
CERT_KEYS = ("Lam", "dz", "dual0", "dual1", "SX")
MARGIN = 1e-6             # relative distance a cg_step case keeps from every comparison a branch depends on


# ---------------------------------------------------------------------------------------------------------------- matrices
def solve_ld(A, B):
    """A^-1 B in longdouble for a symmetric positive definite A (Gauss-Jordan on [A | B]; numpy's solvers stop at f64)"""
    M = np.concatenate([A.astype(LD), B.astype(LD)], axis=1)
    m = A.shape[0]
    for c in range(m):
        M[c] /= M[c, c]
        f = M[:, c].copy()
        f[c] = 0
        M -= f[:, None] * M[c][None, :]
    return M[:, m:]


def schur_dense_ld(cam, lm, p, w):
    """tl.schur_dense in longdouble: the matrix-free storage's operator, by explicit elimination of translations and landmarks"""
    N, M, Q1, c, Q2, Q3 = tl.schur_parts(cam, lm, p, w)
    p, w = np.asarray(p, dtype=LD), np.asarray(w, dtype=LD).reshape(-1)
    Q1l = np.zeros((N, 3, 3), dtype=LD); cl = np.zeros((N, 3), dtype=LD); Q2l = np.zeros(N, dtype=LD); Q3l = np.zeros(M, dtype=LD)
    np.add.at(Q1l, cam, w[:, None, None] * p[:, :, None] * p[:, None, :]); np.add.at(cl, cam, w[:, None] * p)
    np.add.at(Q2l, cam, w); np.add.at(Q3l, lm, w)
    Vtp = np.zeros((3 * N, N + M), dtype=LD)
    for i in range(N):
        Vtp[3 * i:3 * i + 3, i] = cl[i]
    np.add.at(Vtp, (3 * cam[:, None] + np.arange(3)[None, :], N + lm[:, None]), -(w[:, None] * p))
    Qtp = np.zeros((N + M, N + M), dtype=LD)
    Qtp[np.arange(N), np.arange(N)] = Q2l
    Qtp[N + np.arange(M), N + np.arange(M)] = Q3l
    np.add.at(Qtp, (cam, N + lm), -w); np.add.at(Qtp, (N + lm, cam), -w)
    Q = -Vtp[:, 1:] @ solve_ld(Qtp[1:, 1:], Vtp[:, 1:].T)
    for i in range(N):
        Q[3 * i:3 * i + 3, 3 * i:3 * i + 3] += Q1l[i]
    return (Q + Q.T) / 2


def _drop_camera(V, k):
    """the block CSR of a view graph with camera k cut off: an empty row, and no block in column k"""
    rows = np.repeat(np.arange(V["n"]), np.diff(V["rowptr"]))
    keep = (rows != k) & (V["colidx"] != k)
    rowptr = np.zeros(V["n"] + 1, dtype=np.int64)
    np.add.at(rowptr, rows[keep] + 1, 1)
    return np.cumsum(rowptr), V["colidx"][keep], np.ascontiguousarray(V["blocks"][keep])


@functools.lru_cache(maxsize=None)
def matrix(kind, n, arg=0):
    """dict(n, ctx = keyword arguments of xmamd.Context, op / op_f64 = the operator for the longdouble and the f64 run, Q = dense f64 or None)"""
    if kind == "dense":                                    # arg: 0 PSD with planted optimum and noise | 1 the known-answer variant | 2 indefinite
        if arg == 2:
            rng = np.random.default_rng(900 + n)
            A = rng.standard_normal((3 * n, 3 * n)) / np.sqrt(3 * n)
            Q = (A + A.T) / 2
            return dict(n=n, ctx=dict(Q=Q), op=ex.Op(Q), Q=Q)
        P = tl.gen_dense(n, seed=500 + n, noise=0.0 if arg == 1 else 0.3)
        return dict(n=n, ctx=dict(Q=P["Q"]), op=ex.Op(P["Q"]), Q=P["Q"], R_star=P["R_star"].reshape(3 * n, 3))
    if kind == "dense_bsr":                                # the known-answer dense matrix as 3x3-block CSR (every block stored)
        D = matrix("dense", n, 1)
        bsr = tl.dense_to_bsr(D["Q"])
        return dict(D, ctx=dict(bsr=bsr), bsr=bsr)
    if kind == "vg_neg":                                   # a view graph's blocks negated: a negative semidefinite Q (negative curvature for cg_step)
        V = matrix("vg", n, arg)
        bsr = (V["bsr"][0], V["bsr"][1], -V["bsr"][2])
        return dict(n=n, ctx=dict(bsr=bsr), op=ex.BlockOp(*bsr), Q=None, bsr=bsr)
    if kind in ("vg", "vg_empty", "vg_hub"):               # arg: degree
        if kind == "vg_hub":
            H = tl.gen_vg_hubs(n, arg, 1, 0.5, 0.05, 700 + n)
            rowptr, colidx, blocks = tl.vg_from_edges(n, H["ei"], H["ej"], H["w"], H["M"])
        else:
            V = tl.gen_vg(n, deg=arg, sigma=0.05, seed=600 + n, dense=False)
            rowptr, colidx, blocks = _drop_camera(V, n // 2) if kind == "vg_empty" else (V["rowptr"], V["colidx"], V["blocks"])
        return dict(n=n, ctx=dict(bsr=(rowptr, colidx, blocks)), op=ex.BlockOp(rowptr, colidx, blocks), Q=None, bsr=(rowptr, colidx, blocks))
    if kind in ("scene", "scene0"):                        # arg: landmarks; scene0: without noise, the planted rotations are the optimum (f = 0)
        S = tl.gen_scene(n, arg, 4, 800 + n, noise=0.01 if kind == "scene" else 0.0, hubs=3)
        Ql = schur_dense_ld(S["cam"], S["lm"], S["p"], S["w"])
        out = dict(n=n, ctx=dict(obs=(S["cam"], S["lm"], S["p"], S["w"]), n=n), op=ex.Op(Ql), Q=Ql.astype(np.float64))
        if kind == "scene0":                               # anchored at camera 0; the orientation convention is the one that costs nothing
            Ra = np.einsum("ab,ibc->iac", S["R_star"][0].T, S["R_star"])
            cands = [Ra.reshape(3 * n, 3), np.transpose(Ra, (0, 2, 1)).reshape(3 * n, 3)]
            out["R_star"] = min(cands, key=lambda U: float(ex.cost(out["op"], U, np.ones(n), 0.0)))
        return out
    raise KeyError(kind)


def densified(mk):
    M = matrix(*mk)
    return M["Q"] if M["Q"] is not None else tl.bsr_to_dense(M["n"], *M["bsr"])


# ---------------------------------------------------------------------------------------------------------------- points
def make_point(n, o, seed, R_star=None):
    """a random point far from critical: rows of R orthonormal from a QR of Gaussian data, s in [0.6, 1.6] with s[0] given as something the
    solver must replace by 1, a tangent direction and a residual whose scale parts do NOT vanish at the anchor, and a block X for the
    certificate operator.  R_star: the planted optimum instead (rank 3, padded with zero columns; s = 1)."""
    rng = np.random.default_rng(seed)
    if R_star is None:
        R = np.concatenate([np.linalg.qr(rng.standard_normal((o, 3)))[0].T for _ in range(n)], axis=0)
        s = rng.uniform(0.6, 1.6, n)
    else:
        R = np.concatenate([R_star, np.zeros((3 * n, o - 3))], axis=1)
        s = np.ones(n)
    s[0] = 0.8
    sp = s.copy(); sp[0] = 1.0
    pR, ps = ex.tangent(R, rng.standard_normal((3 * n, o)), rng.standard_normal(n) * sp)
    rR, rs = ex.tangent(R, rng.standard_normal((3 * n, o)), rng.standard_normal(n) * sp)
    ps[0], rs[0] = 0.7, -1.3
    return dict(R=R, s=s, p=(pR, ps), r=(rR, rs), X=rng.standard_normal((3 * n, 2)))


def lam_of(n, o):
    return LAMS[(n + o) % 3]


@functools.lru_cache(maxsize=None)
def reference(mk, o, f32=False, optimum=False, cert=True):
    """(point, exact, e_ref) of one matrix at one rank: the longdouble quantities of the grad, hess and cert stages under one dict, and the
    f64 run's error against them per quantity.  f32: the Hessian products' operator is Q rounded to fp32 (the kernel's contract); G, which
    enters the Hessian epilogue, still comes from the f64 Q."""
    M = matrix(*mk)
    n, lam = M["n"], lam_of(M["n"], o)
    pt = make_point(n, o, 1000 * n + o, M.get("R_star") if optimum else None)
    op = M["op"]
    if M["Q"] is not None:
        op64 = ex.Op(M["Q"])
        oph = ex.Op(M["Q"].astype(np.float32).astype(np.float64)) if f32 else op
        oph64 = oph if f32 else op64
    else:
        op64 = oph = oph64 = op
    out = []
    for dt, a, b in ((LD, op, oph), (np.float64, op64, oph64)):
        g = ex.grad_stage(a, pt["R"], pt["s"], lam, dt)
        E = dict(g)
        E.update(ex.hess_stage(b, g, *pt["p"], *pt["r"], lam, dt))
        if cert:
            E.update(ex.cert_stage(a, pt["R"], pt["s"], lam, pt["X"], dt))
        out.append(E)
    E, F = out
    keys = GRAD_KEYS + HESS_KEYS + (CERT_KEYS if cert else ())
    return pt, E, {k: error(F[k], E, k)[0] for k in keys}, lam


def error(x, E, k):
    return st.err(np.asarray(x), E[k], E.get(k + "~"))


def compare(label, got, E, e_ref, keys, who="gpu"):
    """prints STAGE_ERR lines; returns the quantities that miss max(16 e_ref, 64 eps)"""
    bad = []
    for k in keys:
        e, blk = error(got[k], E, k)
        b = st.bound(e_ref[k])
        print(f"STAGE_ERR {label} {k}: e_ref {e_ref[k]:.3e}, e_{who} {e:.3e}, ratio {e / b:.3f}")
        if not e <= b:
            bad.append(f"{label} {k}: {e:.3e} > {b:.3e} (e_ref {e_ref[k]:.3e}, block {blk})")
    return bad


# ---------------------------------------------------------------------------------------------------------------- paths
# (id, matrix key, xm_tuning_t fields, ranks, options): options f32 (hess_f32 contexts), auto (both roles of EPI_AUTO), kind (the product_kind the
# context must report: the kernel family under test), wpad (the tCG keeps the padded copy of its product input), symv_k (forced chunk lengths of
# the symmetric pair), optimum (the point is the planted optimum), split (slices of the column split in effect), gather (sliced-ELL gather mode)
def _paths():
    P = []
    add = lambda *a, **kw: P.append(dict(id=a[0], mk=a[1], tuning=a[2], ranks=a[3], **kw))
    for n in (1, 5, 43, 85, 86, 211):                      # 3n crosses the 256-column tile between 85 and 86
        add(f"dense-n{n}", ("dense", n, 0), dict(sym=-1), (3, 4, 5, 6, 7, 10), kind="dense")
    add("dense-optimum", ("dense", 43, 1), dict(sym=-1), (3, 4), kind="dense", optimum=True)
    # the column split: setup_rank cuts split_k down to the 256-column tiles of a row, so one tile (n = 45) cannot be split on one rank and runs the
    # general kernel (split = 1: listed so that the clamp is pinned, not as a case of the split kernel); 8 slices need 8 tiles (n >= 598)
    for n, k, ks in ((45, 2, 1), (45, 8, 1), (223, 2, 2), (223, 8, 3), (683, 2, 2), (683, 8, 8)):
        add(f"split{k}-n{n}" if ks > 1 else f"split{k}-clamped-n{n}", ("dense", n, 0), dict(sym=-1, split_k=k), (3, 4), kind="dense", split=ks)
    for n in (7, 8, 9, 85, 86, 87, 128, 343):
        add(f"sym-n{n}", ("dense", n, 0), dict(sym=1, sym_min_rows=1), (3, 4, 5), kind="dense_sym")
    add("sym-optimum", ("dense", 43, 1), dict(sym=1, sym_min_rows=1), (3, 4), kind="dense_sym", optimum=True)
    add("sym-finer-cut", ("dense", 128, 0), dict(sym=1, sym_min_rows=1), (3, 5), kind="dense_sym", symv_k=(4, 2))
    for n in (43, 86, 343):
        add(f"f32-n{n}", ("dense", n, 0), dict(sym=-1, hess_f32=1), (3, 4, 5), kind="dense", f32=True)
        add(f"f32-sym-n{n}", ("dense", n, 0), dict(sym=1, sym_min_rows=1, hess_f32=1), (3, 4, 5), kind="dense_sym", f32=True)
    for n, deg in ((1, 2), (7, 3), (17, 4), (200, 8), (300, 20)):
        add(f"bsr-n{n}", ("vg", n, deg), dict(sell=-1), (3, 4, 5, 7, 10), kind="bsr3")
    add("bsr-empty-row", ("vg_empty", 40, 6), dict(sell=-1), (3, 4), kind="bsr3")
    add("bsr-hub-row", ("vg_hub", 120, 4), dict(sell=-1), (3, 5), kind="bsr3")
    for n, deg in ((200, 8), (1000, 12)):
        for gather in (0, 1):                              # the kernels' mode: 0 a record of W per lane | 1 LDS-transposed (xm_tuning_t counts them 1 and 2)
            for codec in (1, 2):
                for wpad in (1, -1):
                    add(f"sell-n{n}-g{gather}-c{codec}-w{wpad}", ("vg", n, deg), dict(sell=1, sell_gather=gather + 1, sell_codec=codec, sell_wpad=wpad, sell_lmax=5),
                        (3, 4, 5), kind="sell" if codec == 1 else "sell_quat", wpad=wpad == 1, gather=gather)
    for n, m in ((40, 60), (130, 150)):
        add(f"schur-n{n}", ("scene", n, m), dict(schur_solver=1), (3, 4, 5), kind="schur")
    # every storage once more at a planted optimum, where the exact gradient vanishes and the errors are judged against the terms' magnitude
    add("f32-optimum", ("dense", 43, 1), dict(sym=1, sym_min_rows=1, hess_f32=1), (3, 4), kind="dense_sym", f32=True, optimum=True)
    add("bsr-optimum", ("dense_bsr", 43, 0), dict(sell=-1), (3, 4), kind="bsr3", optimum=True)
    add("sell-optimum", ("dense_bsr", 43, 0), dict(sell=1, sell_codec=1, sell_lmax=5, sell_wpad=-1), (3, 4), kind="sell", optimum=True)
    add("schur-optimum", ("scene0", 40, 60), dict(schur_solver=1), (3, 4), kind="schur", optimum=True)
    for n in (43, 86):
        add(f"auto-dense-n{n}", ("dense", n, 0), dict(sym=-1), (3, 4, 5), kind="dense", auto=True)
    add("auto-sym-n86", ("dense", 86, 0), dict(sym=1, sym_min_rows=1), (3, 4, 5), kind="dense_sym", auto=True)
    add("auto-f32-n86", ("dense", 86, 0), dict(sym=-1, hess_f32=1), (3, 4, 5), kind="dense", auto=True, f32=True)
    for n, deg in ((17, 4), (200, 8)):
        add(f"auto-bsr-n{n}", ("vg", n, deg), dict(sell=-1), (3, 4, 5), kind="bsr3", auto=True)
    return P


PATHS = _paths()
PATH_IDS = [p["id"] for p in PATHS]


# ---------------------------------------------------------------------------------------------------------------- cg_step
CG_BRANCHES = {"interior0": 0, "interior7": 0, "converged": 3, "boundary": 2, "negative": 1, "tiny": 5, "cap": 6, "interior0-model": 0, "boundary-model": 2}
CG_ARRAYS = ("vR", "vs", "HvR", "Hvs", "rR", "rs", "pR", "ps", "W")
CG_SCALARS = ("rr", "vv", "vp", "pp", "last_step", "model")
# (context: path fields, ranks); the last one has more than one element per thread of cg_step_kernel's grid (3 n pitch > 1024 x 256)
CG_CONTEXTS = (dict(id="cg-dense", mk=("dense", 43, 0), mk_neg=("dense", 43, 2), tuning=dict(sym=-1), ranks=(3, 5), names=tuple(CG_BRANCHES)),
               dict(id="cg-bsr", mk=("vg", 200, 8), mk_neg=("vg_neg", 200, 8), tuning=dict(sell=-1), ranks=(3, 5), names=tuple(CG_BRANCHES)),
               dict(id="cg-bsr-stride", mk=("vg", 30000, 3), mk_neg=None, tuning=dict(sell=-1), ranks=(3,), names=("interior0", "interior7")))


@functools.lru_cache(maxsize=None)
def cg_case(mk, o, name):
    """one launch of cg_step_kernel that takes the branch `name`: the point, a direction p (the first of a few seeded candidates whose <p,Hp>
    has the sign the branch needs), residual r, iterate v, H v, and a scalar state placed around the longdouble values of the Hessian stage's
    sums so that every comparison a branch depends on keeps a wide margin.  Returns also what the longdouble chain expects."""
    M = matrix(*mk)
    n, lam = M["n"], lam_of(M["n"], o)
    base = name.split("-")[0]
    want_neg = base == "negative"
    chosen = None
    if want_neg:                                           # an indefinite (or negative semidefinite) Q, no penalty term, directions along its most negative eigenvectors
        lam = 0.0
        evec = np.linalg.eigh(densified(mk))[1]
    for cand in range(8):
        pt = make_point(n, o, 2000 * n + 10 * o + cand)
        if want_neg:
            Z = np.zeros((3 * n, o)); Z[:, cand % o] = evec[:, cand // o]
            pR, ps = ex.tangent(pt["R"], Z, np.zeros(n))
            ps[0] = 0.7
            pt = dict(pt, p=(pR, ps))
        g = ex.grad_stage(M["op"], pt["R"], pt["s"], lam, LD)
        h = ex.hess_stage(M["op"], g, *pt["p"], *pt["r"], lam, LD)
        if (h["pHp"] < 0) == want_neg and abs(h["pHp"]) > 1e-3 * h["pHp~"]:
            chosen = (pt, g, h)
            break
    assert chosen is not None, f"no direction with the curvature sign of {name} among the candidates"
    pt, g, h = chosen
    rng = np.random.default_rng(77 + n + o)
    s1 = pt["s"].copy(); s1[0] = 1.0
    v = ex.tangent(pt["R"], 0.1 * rng.standard_normal((3 * n, o)), 0.1 * rng.standard_normal(n) * s1)
    Hv = ex.tangent(pt["R"], rng.standard_normal((3 * n, o)), rng.standard_normal(n) * s1)
    rs = pt["r"][1].copy(); rs[0] = 0.0                    # the residual a solve holds: 0 at the anchor
    r = (pt["r"][0], rs)
    rr = float(ex.inner(r[0].astype(LD), rs.astype(LD), r[0].astype(LD), rs.astype(LD), s1.astype(LD)))
    alpha = rr / float(h["pHp"])
    vv, vp, pp = 0.3, 0.1, 2.0
    vnew2 = vv + 2 * alpha * vp + alpha * alpha * pp
    rr_est = max(rr + 2 * alpha * float(h["rHp"]) + alpha * alpha * float(h["HpHp"]), 0.0)
    sc = dict(rr=rr, vv=vv, vp=vp, pp=pp, delta=10.0 * np.sqrt(max(vnew2, 1.0)), gradnorm=1e-2 * min(1.0, np.sqrt(rr_est)), model=-0.25, iter=0)
    if base in ("interior7", "cap"):
        sc["iter"] = 7 if base == "interior7" else ex.MAX_INNER - 1
    elif base == "converged":
        sc["gradnorm"] = 1e6 * max(1.0, np.sqrt(rr_est))
    elif base == "boundary":
        sc["delta"] = float(np.sqrt((vv + vnew2) / 2))
    elif base == "negative":
        sc["delta"] = 1.0
    elif base == "tiny":
        sc["rr"] = 1e-17
    model_rec = name.endswith("-model")
    sums = (h["pHp"], h["rHp"], h["HpHp"], LD(rr))
    expect = ex.cg_step_stage(sc, sums, (h["HpR"], h["Hps"]), pt["p"], r, v, Hv, pt["R"], pt["s"], LD, model_rec=model_rec, pHp_scale=h["pHp~"])
    return dict(pt=pt, r=r, v=v, Hv=Hv, sc=sc, rr_total=rr, lam=lam, model_rec=model_rec, expect=expect, hess=h, grad=g)


def cg_inputs(c, nB):
    """keyword arguments of Context.rtr_probe for the case; for iter > 0 the |r|^2 partial sums the launch before would have left: nB unequal
    shares of the total"""
    w = 1.0 + 0.5 * np.cos(np.arange(nB))
    parts = c["rr_total"] * w / w.sum() if c["sc"]["iter"] > 0 else None
    return dict(p=c["pt"]["p"], r=c["r"], cg_step=dict(c["sc"], v=c["v"], Hv=c["Hv"], partsB=parts), model_recurrence=c["model_rec"]), parts


# ---------------------------------------------------------------------------------------------------------------- the outer iteration's other half
# retract_kernel's shapes: 43 cameras = one partly filled wavefront; 131 = three wavefronts (outer_decide's group of four has an absent member);
# 321 = two workgroups, six wavefronts (two partsM entries, the second with two absent members); ranks with and without the pad column
RETRACT_RANKS = (3, 4, 5, 10)
RETRACTIONS = ("mgs", "polar")
OUTER_CONTEXTS = tuple(dict(id=f"{kind}-n{n}", mk=mk, tuning=tuning, kind=pk)
                       for n in (43, 131, 321)
                       for kind, mk, tuning, pk in (("dense", ("dense", n, 0), dict(sym=-1), "dense"),
                                                    ("sym", ("dense", n, 0), dict(sym=1, sym_min_rows=1), "dense_sym"),
                                                    ("bsr", ("vg", n, 6), dict(sell=-1), "bsr3")))
OUTER_IDS = [c["id"] for c in OUTER_CONTEXTS]
RETRACT_KEYS = ("Rc", "sc", "W")
LS_T = -0.37              # the line search retracts R - alpha D


@functools.lru_cache(maxsize=None)
def retract_case(mk, o):
    """a point, a tangent step v whose scale part has t ds / s spread over -5 .. 5 (the exp is nowhere near 1), H v and a line-search direction D;
    for a tangent D the Gram matrix of a block of R + D is I + D D^T: every block is well conditioned.  -> the longdouble quantities of the
    gradient, the two retractions, the line search's form and the model decrease, and the f64 run's error per quantity"""
    M = matrix(*mk)
    n, lam = M["n"], lam_of(M["n"], o)
    pt = make_point(n, o, 3000 * n + o)
    rng = np.random.default_rng(3100 * n + o)
    s1 = pt["s"].copy(); s1[0] = 1.0
    v = ex.tangent(pt["R"], 0.4 * rng.standard_normal((3 * n, o)), s1 * rng.uniform(-5.0, 5.0, n))
    v[1][0] = 0.9                                          # what a caller leaves at the anchor must not get through
    Hv = ex.tangent(pt["R"], rng.standard_normal((3 * n, o)), rng.standard_normal(n) * s1)
    D = ex.tangent(pt["R"], rng.standard_normal((3 * n, o)), np.zeros(n))[0]
    op64 = ex.Op(M["Q"]) if M["Q"] is not None else M["op"]
    runs = []
    for dt, op in ((LD, M["op"]), (np.float64, op64)):
        g = ex.grad_stage(op, pt["R"], pt["s"], lam, dt)
        E = dict(grad=g, model=ex.model_stage(v, Hv, (g["rgR"], g["rgs"]), pt["s"], dt))
        for name in RETRACTIONS:
            E[name] = ex.retract_stage(pt["R"], pt["s"], v[0], v[1], 1.0, name == "polar", dt)
            E["ls-" + name] = ex.retract_stage(pt["R"], pt["s"], D, None, LS_T, name == "polar", dt)
        runs.append(E)
    E, F = runs
    e_ref = {name: {k: error(F[name][k], E[name], k)[0] for k in RETRACT_KEYS} for name in E if name not in ("grad", "model")}
    e_ref["model"] = {"m": error(F["model"]["m"], E["model"], "m")[0]}
    return dict(pt=pt, v=v, Hv=Hv, D=D, lam=lam, E=E, e_ref=e_ref)


def regroup4(w):
    """per-wavefront partial sums four by four in block_sum256's order (w0 + w1) + (w2 + w3), absent members 0: retract_kernel's per-workgroup sums"""
    w = np.concatenate([np.asarray(w, dtype=np.float64), np.zeros(-len(w) % 4)]).reshape(-1, 4)
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


# the step launch: (context, the indefinite matrix of the negative-curvature branch, ranks); the last is the one size at which the tCG-ending role's
# loop over wavefronts takes a second trip (more than 1024 x 64 cameras)
STEP_CG = ("interior0", "interior7", "interior0-model")
STEP_END = ("converged", "boundary", "negative", "tiny", "cap", "boundary-model")
STEP_CONTEXTS = (dict(id="step-dense-n43", mk=("dense", 43, 0), mk_neg=("dense", 43, 2), tuning=dict(sym=-1), ranks=(3, 4), names=STEP_CG + STEP_END),
                 dict(id="step-sym-n131", mk=("dense", 131, 0), mk_neg=("dense", 131, 2), tuning=dict(sym=1, sym_min_rows=1), ranks=(4, 5), names=STEP_CG + STEP_END),
                 dict(id="step-bsr-n321", mk=("vg", 321, 6), mk_neg=("vg_neg", 321, 6), tuning=dict(sell=-1), ranks=(3, 10), names=STEP_CG + STEP_END),
                 dict(id="step-bsr-n65600", mk=("vg", 65600, 2), mk_neg=None, tuning=dict(sell=-1), ranks=(3,), names=("boundary",)))
STEP_IDS = [c["id"] for c in STEP_CONTEXTS]
DECIDE_CONTEXTS = (dict(id="decide-dense-n43", mk=("dense", 43, 0), tuning=dict(sym=-1), o=4), dict(id="decide-bsr-n131", mk=("vg", 131, 6), tuning=dict(sell=-1), o=3),
                   dict(id="decide-sym-n321", mk=("dense", 321, 0), tuning=dict(sym=1, sym_min_rows=1), o=5))
RHO_TARGETS = (0.05, 0.2, 0.5, 0.9)                      # each keeps a relative distance > MARGIN from 0.1, 0.25 and 0.75


def decide_branches(delta=2.0):
    """(name, changes to the decision's inputs, what must come out): rho = the target the loss is placed for (None: m >= 0), then the tCG's exit
    status and iteration count, the radius, the state of the trust region and the limits"""
    B = []
    add = lambda name, rho, expect, **kw: B.append(dict(dict(name=name, rho=rho, status=2, iter=4, delta=delta, delta_bar=1e3, gradtol=0.0, max_outer=0, shrink=0,
                                                             k=3, time_up=0, stop_req=0), expect=expect, **kw))
    add("reject", 0.05, dict(accept=False, start=True, stop_reason=0, shrink_count=1))
    add("shrink-accept", 0.2, dict(accept=True, start=True, stop_reason=0, shrink_count=1))
    add("accept", 0.5, dict(accept=True, start=True, stop_reason=0, shrink_count=0), shrink=2)
    add("double", 0.9, dict(accept=True, start=True, stop_reason=0, shrink_count=0, delta=2 * delta))
    add("no-double-at-tolerance", 0.9, dict(accept=True, start=True, stop_reason=0, delta=delta), status=3)
    add("delta-bar-cap", 0.9, dict(accept=True, start=True, stop_reason=0, delta=1.5 * delta), delta_bar=1.5 * delta)
    add("fourth-shrink", 0.2, dict(accept=True, start=True, stop_reason=0, shrink_count=0, delta=delta * 0.25 * 1e-3), shrink=3)
    add("fourth-shrink-reject", 0.05, dict(accept=False, start=True, stop_reason=0, shrink_count=0, delta=delta * 0.25 * 1e-3), shrink=3)
    add("stop13", 0.05, dict(accept=True, start=False, stop_reason=13), shrink=3, delta=1e-18)
    add("stop12", None, dict(accept=False, start=False, stop_reason=12))
    add("stop14", 0.5, dict(accept=True, start=False, stop_reason=14), k=6, max_outer=7)
    add("stop14-solve-cap", 0.5, dict(accept=True, start=False, stop_reason=14), k=999)
    add("stop5", 0.5, dict(accept=True, start=False, stop_reason=5), status=5)
    add("stop10", 0.5, dict(accept=True, start=False, stop_reason=10), gradtol=1e30)
    add("stop11", 0.5, dict(accept=True, start=False, stop_reason=11), time_up=1)
    add("time-request-is-passed-on", 0.5, dict(accept=True, start=True, stop_reason=0, time_up=1), stop_req=1)
    add("max-iterations", 0.9, dict(accept=True, start=True, stop_reason=0, delta=delta), status=0, iter=999)
    return B
