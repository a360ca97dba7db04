"""What tests/test_rtr_exact.py (CPU) and tests/test_gpu_cert_stages.py (GPU) share for the certificate's Lanczos eigen-solver: the matrices, the
points, the cases, and the comparison of one run -- the output of the test export xm_ctx_cert_probe, or of the f64 run of the reference in its
place -- with the longdouble reference xm_rtr_exact.lanczos_stage.  Bound: e <= max(16 e_ref, 64 eps) per quantity and case (xm_ba_stages.bound).

A run is compared step by step from its OWN basis: step j of the reference starts from the run's columns V[:, 0..j], so every step is a
well-conditioned stage (a product, two Gram-Schmidt passes, a norm) and not a recurrence that drifts.  What only the whole run shows -- loss of
orthogonality, the Lanczos relation, the Ritz pair -- is compared with the f64 whole run of the reference."""
import functools

import numpy as np

import xm_ba_stages as st
import xm_rtr_exact as ex
import xm_rtr_stages as rs
import xm_testlib as tl

LD = ex.LD
EPS = st.EPS
ORTH_LD_MAX = 300          # columns up to which V^T V is formed in longdouble (beyond: in f64, whose own error per entry is <= 2 eps for unit columns)


@functools.lru_cache(maxsize=None)
def matrix(kind, n, arg=0):
    """rs.matrix, and: vg0 = a noise-free view graph of degree arg (its planted rotations are an optimum with f = 0), vg0_dense = the same as a
    dense matrix, complete = the noise-free complete view graph with unit weights, dense (Q = n I - U U^T, U the stacked planted rotations)"""
    if kind in ("vg0", "vg0_dense"):
        V = tl.gen_vg(n, deg=arg, sigma=0.0, seed=1200 + n, dense=False)
        bsr = (V["rowptr"], V["colidx"], V["blocks"])
        U = V["R_star"].reshape(3 * n, 3)
        if kind == "vg0":
            return dict(n=n, ctx=dict(bsr=bsr), op=ex.BlockOp(*bsr), Q=None, bsr=bsr, R_star=U)
        Q = tl.bsr_to_dense(n, *bsr)
        return dict(n=n, ctx=dict(Q=Q), op=ex.Op(Q), Q=Q, R_star=U)
    if kind == "complete":
        U = tl.haar_so3(np.random.default_rng(1300 + n), n).reshape(3 * n, 3)
        Q = n * np.eye(3 * n) - U @ U.T
        Q = (Q + Q.T) / 2
        return dict(n=n, ctx=dict(Q=Q), op=ex.Op(Q), Q=Q, R_star=U)
    return rs.matrix(kind, n, arg)


def make_point(n, o, seed, R_star=None):
    """R_star: the planted optimum (rank 3, zero columns beyond; s = 1).  Otherwise a random point of the manifold with s spread over 0.5 .. 2"""
    if R_star is not None:
        return np.concatenate([R_star, np.zeros((3 * n, o - 3))], axis=1), np.ones(n)
    rng = np.random.default_rng(seed)
    R = np.concatenate([np.linalg.qr(rng.standard_normal((o, 3)))[0].T for _ in range(n)], axis=0) if n < 5000 else \
        np.transpose(np.linalg.qr(rng.standard_normal((n, o, 3)))[0], (0, 2, 1)).reshape(3 * n, o)
    return R, rng.uniform(0.5, 2.0, n)


# (id, matrix, tuning, o, options): optimum (the planted point, lam = 0), kind (product_kind the context must report), nseg, steps (which steps are
# compared; None = all), expect (what the run must report), eig (theta is held against eigvalsh(S)), unfused (run both forms, equal bits)
def _cases():
    P = []
    add = lambda cid, mk, tuning, o=3, **kw: P.append(dict(id=cid, mk=mk, tuning=tuning, o=o, **kw))
    one = dict(lanczos_restarts=1)
    for n in (5, 43):                                      # len 128: fewer elements than threads; every step of the complete tridiagonalisation
        add(f"single-n{n}", ("dense", n, 0), dict(one, sym=-1), 4, kind="dense", nseg=1, eig=True, expect=dict(m_use=3 * n, eig_exact=1, ret=0))
        add(f"single-n{n}-optimum", ("vg0_dense", n, 3), dict(one, sym=-1), 4, kind="dense", nseg=1, eig=True, optimum=True, expect=dict(eig_exact=1, ret=0))
    m24 = dict(one, lanczos_mmax=24)
    add("dense-n130", ("dense", 130, 0), dict(m24, sym=-1), 4, kind="dense", nseg=1, eig=True, unfused=True)
    add("sym-n130", ("dense", 130, 0), dict(m24, sym=1, sym_min_rows=1), 4, kind="dense_sym", nseg=1, eig=True)
    add("bsr-n130", ("vg", 130, 6), dict(m24, sell=-1), 3, kind="bsr3", nseg=1, eig=True)
    add("bsr-n130-optimum", ("vg0", 130, 6), dict(m24, sell=-1), 5, kind="bsr3", nseg=1, eig=True, optimum=True)
    add("sell-n130", ("vg", 130, 6), dict(m24, sell=1, sell_codec=1, sell_lmax=5, sell_wpad=-1), 3, kind="sell", nseg=1, eig=True)
    add("schur-n130", ("scene", 130, 150), dict(m24, schur_solver=1), 3, kind="schur", nseg=1, eig=True)
    m6 = dict(one, lanczos_mmax=6, sell=-1)
    add("seg2-n2731", ("vg", 2731, 4), m6, 3, kind="bsr3", nseg=2, unfused=True)
    add("seg3-n4097", ("vg", 4097, 4), m6, 3, kind="bsr3", nseg=3)
    add("seg64-n87424", ("vg", 87424, 4), m6, 3, kind="bsr3", nseg=64, steps=(0, 5))
    add("cross1024-n400", ("dense", 400, 0), dict(one, sym=1, sym_min_rows=1, cert_dense_rows=1200, lanczos_mmax=1200), 3, kind="dense_sym", nseg=1, eig=True,
        steps=(0, 1023, 1024, 1199), relation=True, expect=dict(m_use=1200, eig_exact=1, ret=0, steps_fused=1024, steps_unfused=176))
    add("exhaust-n100", ("complete", 100, 0), dict(one, sym=-1), 3, kind="dense", nseg=1, optimum=True, exhaust=True, expect=dict(m_use=2, eig_exact=1, ret=0))
    add("exhaust-n130", ("complete", 130, 0), dict(one, sym=-1), 3, kind="dense", nseg=1, optimum=True, exhaust=True, expect=dict(m_use=2, eig_exact=0, ret=0))
    add("restarts-n130", ("dense", 130, 0), dict(sym=-1, cert_dense_rows=3, lanczos_mmax=8, lanczos_restarts=12), 4, kind="dense", nseg=1, eig=True, restarts=True)
    add("cut-short-n130", ("dense", 130, 0), dict(one, sym=-1, lanczos_mmax=4), 4, kind="dense", nseg=1, eig=True, expect=dict(m_use=4, ret=1))
    return P


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}


def run_settings(case):
    t = case["tuning"]
    return dict(mmax=t.get("lanczos_mmax", 0) or 400, restarts=t.get("lanczos_restarts", 0) or 12, dense_rows=t.get("cert_dense_rows", 0) or 384)


@functools.lru_cache(maxsize=None)
def setup(cid):
    """the point, lam, the multipliers in longdouble and f64 (cert_stage), the operators, and the f64 whole run of the reference"""
    case = BY_ID[cid]
    M = matrix(*case["mk"])
    n, o = M["n"], case["o"]
    optimum = case.get("optimum", False)
    R, s = make_point(n, o, 4000 + n + o, M["R_star"] if optimum else None)
    lam = 0.0 if optimum else 10.0
    op64 = ex.Op(M["Q"]) if M["Q"] is not None else M["op"]
    C = ex.cert_stage(M["op"], R, s, lam, None, LD)
    C64 = ex.cert_stage(op64, R, s, lam, None, np.float64)
    F = ex.lanczos_stage(op64, C64, np.float64, **run_settings(case))
    return dict(n=n, o=o, R=R, s=s, lam=lam, op=M["op"], op64=op64, C=C, C64=C64, F=F, M=M)


def as_run(F):
    """the f64 whole run of the reference in the shape of the probe's output"""
    k = F["m_use"]
    return dict(alpha=F["alpha"], beta=F["beta"], V=F["V"], y=F["y"], x=F["x"], theta=float(F["theta"]), resid=float(F["resid"]), ret=F["ret"],
                eig_exact=int(F["eig_exact"]), m_use=k, steps_dev=k, cycles=F["cycles"], iters=F["iters"], c1=F["c1"], c2=F["c2"])


def dense_S(S, dt=np.float64):
    n = S["n"]
    op, C = (S["op"], S["C"]) if dt is LD else (S["op64"], S["C64"])
    return ex.cert_operator(op, C, np.eye(3 * n), dt)["SX"].reshape(3 * n, 3 * n)


def orthogonality(V, m):
    """max |V^T V - I| over the first m columns"""
    W = V[:, :m].astype(LD if m <= ORTH_LD_MAX else np.float64)
    return float(np.abs(W.T @ W - np.eye(m)).max())


def whole_run_figures(S, run):
    """what only the whole run shows, each as (value, scale): the Ritz vector against V y / |V y|, x^T S x against theta, the reported residual
    against |S x - theta x|, all in longdouble from the run's own V, y, x and theta"""
    n, m = S["n"], run["m_use"]
    V, y, x = run["V"][:, :m].astype(LD), np.asarray(run["y"]).astype(LD), np.asarray(run["x"]).astype(LD)
    xr = V @ y
    xr = xr / np.sqrt(xr @ xr)
    o = ex.cert_operator(S["op"], S["C"], x[:, None], LD)
    Sx, aS = o["SX"].reshape(-1), np.repeat(o["SX~"], 3)
    theta, tmax = LD(run["theta"]), ex.tridiag_bounds(np.asarray(run["alpha"][:m]).astype(LD), np.asarray(run["beta"][:m]).astype(LD))[2]
    ax = np.abs(V) @ np.abs(y)
    out = {"x": (float(np.abs(x - xr).max()), float(max(ax.max(), np.abs(xr).max())))}
    # theta is the midpoint of a bisection interval of 4e-16 max(1, tmax): it is judged against no less than that
    out["xSx"] = (float(abs(x @ Sx - theta)), float(max(np.abs(x) @ aS, tmax, 1)))
    r = Sx - theta * x
    out["resid"] = (float(abs(np.sqrt(r @ r) - LD(run["resid"]))), float(max(np.sqrt(aS @ aS), tmax, 1)))
    return out


def compare_run(label, S, run, case, who="gpu", e_ref_run=None):
    """STAGE_ERR lines for one run; returns what misses the bound.  e_ref_run: the figures of the f64 whole run (None: `run` is that run)"""
    bad, n = [], S["n"]
    m, k = run["m_use"], run["steps_dev"]
    V = np.asarray(run["V"])
    steps = [j for j in (case.get("steps") or range(m)) if j < m]
    worst = {}
    for j in steps:
        E = ex.lanczos_step(S["op"], S["C"], V[:, :j + 1], LD)
        F = ex.lanczos_step(S["op64"], S["C64"], V[:, :j + 1], np.float64)
        got = dict(alpha=run["alpha"][j], beta=run["beta"][j], w=(run["beta"][j] * V[:, j + 1]).reshape(n, 3))
        keys = ["alpha", "beta", "w"]
        if run.get("c1") is not None and j == k - 1:
            got.update(c1=run["c1"], c2=run["c2"])
            keys += ["c1", "c2"]
        for q in keys:
            e_ref, e = rs.error(F[q], E, q)[0], rs.error(got[q], E, q)[0]
            ratio = e / st.bound(e_ref)
            if ratio > worst.get(q, (-1.0,))[0]:
                worst[q] = (ratio, e_ref, e, j)
    for q, (ratio, e_ref, e, j) in worst.items():
        print(f"STAGE_ERR {label} {q}: e_ref {e_ref:.3e}, e_{who} {e:.3e}, ratio {ratio:.3f}")
        if not ratio <= 1:
            bad.append(f"{label} {q} at step {j}: {e:.3e} > {st.bound(e_ref):.3e}")
    ref = as_run(S["F"]) if e_ref_run is None else e_ref_run
    figs = {"orth": (orthogonality(V, m), 1.0)}
    refs = {"orth": (orthogonality(np.asarray(ref["V"]), ref["m_use"]), 1.0)}
    figs.update(whole_run_figures(S, run))
    refs.update(whole_run_figures(S, ref))
    for q, (v, scale) in figs.items():
        e, e_ref = v / scale, refs[q][0] / refs[q][1]
        print(f"STAGE_ERR {label} {q}: e_ref {e_ref:.3e}, e_{who} {e:.3e}, ratio {e / st.bound(e_ref):.3f}")
        if not e <= st.bound(e_ref):
            bad.append(f"{label} {q}: {e:.3e} > {st.bound(e_ref):.3e}")
    return bad


def relation_error(S, run):
    """the Lanczos relation S V_m = V_m T_m + beta_{m-1} v_m e_m^T column by column, in f64 (1200 columns): the largest entry of a column of the
    defect over the magnitude of the terms of S v_j (per camera, the largest)"""
    m = run["m_use"]
    V, a, b = np.asarray(run["V"], dtype=np.float64), np.asarray(run["alpha"], dtype=np.float64)[:m], np.asarray(run["beta"], dtype=np.float64)[:m]
    Sd = dense_S(S)
    D = Sd @ V[:, :m] - V[:, :m] * a[None, :]
    D[:, 1:] -= V[:, :m - 1] * b[None, :m - 1]
    D[:, :m - 1] -= V[:, 1:m] * b[None, :m - 1]
    D[:, m - 1] -= b[m - 1] * V[:, m] if V.shape[1] > m else 0
    scale = np.abs(Sd) @ np.abs(V[:, :m])
    return float((np.abs(D).max(axis=0) / scale.max(axis=0)).max())
