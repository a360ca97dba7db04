"""GPU tests of the trust region's kernels stage by stage through the test export xm_ctx_rtr_probe: one gradient, one Hessian product, one
start and one step of the truncated CG, the certificate's multipliers and operator, at fixed points, every array compared with the longdouble
reference xm_rtr_exact.py.  The probe runs the context's own setup, product dispatch and launchers, so the kernel under test is the one the
storage and xm_tuning_t select (checked through product_kind).

Bound (xm_rtr_stages.py): e_gpu <= max(16 e_ref, 64 eps_f64) per quantity and case, e_ref the f64 run's own error against the same reference at
the same point; errors per camera block against the larger of the exact block and the magnitude of the terms it is formed from.  Nothing is
derived from the GPU's output.  The cases are those of test_rtr_exact.py::test_f64_run_agrees_with_longdouble_on_every_gpu_case (which asserts
e_ref <= 1e-8 for each).  Every comparison prints `STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s); profiles/r14_rtr_stage_errors.txt condenses a run.

Which kernel an output pins: f, rr, G, egs, S0, rgR, rgs -> scale_rows_kernel, the product kernel's EPI_GRAD instantiation (epi_grad; with auto the
EPI_AUTO instantiation in its candidate role, which loads its rows of W late) and outer_finalize_kernel; HpR, Hps -> tcg_init_kernel's product
input (native pitch or the padded copy), the EPI_HESS instantiation (epi_hess; the fp32 launch on hess_f32 contexts; EPI_AUTO in its tCG role);
pHp, rHp, HpHp -> the epilogue's per-workgroup partial sums (qw_tail, the symmetric pair's symv_reduce_kernel, the sliced-ELL reducer, the
column split's last slice) and the summation tree; init_* -> tcg_init_kernel; out_*, scal_out, rr_parts -> cg_step_kernel; Lam, dz, dual ->
cert_prepare_kernel (and the EPI_PLAIN product); SX -> the O = 1 EPI_CERT instantiation of the product kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import xm_ba_stages as st
import xm_rtr_exact as ex
import xm_rtr_stages as rs
import xm_testlib as tl

pytestmark = pytest.mark.gpu

LD = ex.LD
BY_ID = {p["id"]: p for p in rs.PATHS}
_dense_results = {}


def _ctx(xmamd, mk, tuning):
    return xmamd.Context(**rs.matrix(*mk)["ctx"], tuning=tuning)


def _probe(ctx, path, o, pt, lam, **kw):
    got = ctx.rtr_probe(o, lam, pt["R"], pt["s"], p=pt["p"], r=pt["r"], auto=path.get("auto", False), **kw)
    if "dual" in got:
        got["dual0"], got["dual1"] = got["dual"]
    return got


def _dense_kernel(xmamd, mk, optimum):
    """G, rgR, HpR of the general dense kernel on the densified matrix, every rank the paths use on it (one context per matrix, cached)"""
    key = (mk, optimum)
    if key not in _dense_results:
        ranks = sorted({o for p in rs.PATHS if p["mk"] == mk and p.get("optimum", False) == optimum for o in p["ranks"]})
        ctx = xmamd.Context(Q=rs.densified(mk), tuning=dict(sym=-1))
        out = {}
        for o in ranks:
            pt, E, e_ref, lam = rs.reference(mk, o, False, optimum)
            g = ctx.rtr_probe(o, lam, pt["R"], pt["s"], p=pt["p"], r=pt["r"])
            assert g["product_kind"] == "dense"
            out[o] = {k: g[k] for k in ("G", "rgR", "HpR")}
        ctx.close()
        _dense_results[key] = out
    return _dense_results[key]


@pytest.mark.parametrize("pid", rs.PATH_IDS)
def test_stage_outputs_against_the_longdouble_reference(xmamd, pid):
    path = BY_ID[pid]
    mk, f32, optimum = path["mk"], path.get("f32", False), path.get("optimum", False)
    n = rs.matrix(*mk)["n"]
    L = xmamd.lib()
    if "symv_k" in path:                                   # the symmetric pair's chunks cut finer than the plan cuts them at this size
        xmamd._chk(L.xm_bench_symv_k(path["symv_k"][0], 1, path["symv_k"][1]))
        plan = (C.c_int32 * 4)()
        xmamd._chk(L.xm_symv_plan(n, plan))
        assert (plan[0], plan[1]) == path["symv_k"]
    try:
        ctx = _ctx(xmamd, mk, path["tuning"])
        bad = []
        for i, o in enumerate(path["ranks"]):
            pt, E, e_ref, lam = rs.reference(mk, o, f32, optimum)
            assert max(e_ref.values()) <= rs.MAX_E_REF, e_ref
            label = f"{pid}-o{o}"
            got = _probe(ctx, path, o, pt, lam, tcg_init=True, delta=2.5, cert=True, X=pt["X"])
            assert got["product_kind"] == path["kind"], (label, got["product_kind"])
            assert got["wpad"] == path.get("wpad", False) and got["w_native"] != got["wpad"]
            assert got["split_k"] == path.get("split", 1) and got["sell_gather"] == path.get("gather", 1 if path["kind"].startswith("sell") else -1), label
            if got["split_k"] > 1:                         # the role-switching launch has no column-split form
                with pytest.raises(xmamd.XmError, match="XM_RTR_PROBE_AUTO"):
                    ctx.rtr_probe(o, lam, pt["R"], pt["s"], auto=True)
            bad += rs.compare(label, got, E, e_ref, rs.GRAD_KEYS + rs.HESS_KEYS + rs.CERT_KEYS)
            # the anchor: its scale is 1 whatever was given, and nothing of the scale parts given at the anchor gets through
            assert got["egs"][0] == 0.0 and got["rgs"][0] == 0.0 and got["Hps"][0] == 0.0
            # tcg_init: a copy, a negation, zeros -- exact bits; the scalar block; the first product input from the kernel's own rg
            for k, ref in (("init_rR", got["rgR"]), ("init_rs", got["rgs"]), ("init_pR", -got["rgR"]), ("init_ps", -got["rgs"])):
                assert np.array_equal(got[k], ref), (label, k)
            for k in ("init_vR", "init_vs", "init_HvR", "init_Hvs"):
                assert not got[k].any(), (label, k)
            sc = got["init_scal"]
            assert (sc["rr"], sc["pp"], sc["vv"], sc["vp"], sc["delta"], sc["model"], sc["status"], sc["iter"]) == (got["rr"], got["rr"], 0.0, 0.0, 2.5, 0.0, 0, 0)
            assert abs(sc["gradnorm"] - np.sqrt(got["rr"])) <= 2 * st.EPS * sc["gradnorm"]
            s1 = pt["s"].astype(LD); s1[0] = 1
            Rb = ex.blk(pt["R"].astype(LD), n)
            W = -ex.blk(got["rgR"].astype(LD), n) * s1[:, None, None] - got["rgs"].astype(LD)[:, None, None] * Rb
            aW = np.abs(ex.blk(got["rgR"], n)).max(axis=(1, 2)) * s1 + np.abs(got["rgs"])
            OP = o | 1
            Wgot = got["init_W"] if got["w_native"] else got["init_Wpad"][:, :3 * OP].reshape(n, 3, OP)[:, :, :o]
            e, blk = st.err(ex.blk(np.asarray(Wgot), n), W, aW)
            print(f"STAGE_ERR {label} init_W: e_ref 0.000e+00, e_gpu {e:.3e}, ratio {e / st.bound(0.0):.3f}")
            if not e <= st.bound(0.0):
                bad.append(f"{label} init_W: {e:.3e} (block {blk})")
            if got["wpad"]:
                assert not got["init_Wpad"][:, 3 * OP:].any()      # the pad of a record is never written
            # the same G, rgR, HpR as the general dense kernel on the densified matrix: each within its bound of the exact value
            if path["kind"] != "dense" or path.get("split", 1) > 1 or path.get("auto"):
                D = _dense_kernel(xmamd, mk, optimum)[o]
                for k in ("G", "rgR") + (() if f32 else ("HpR",)):
                    e, blk = st.err(ex.blk(got[k], n), ex.blk(D[k], n).astype(LD), E[k + "~"])
                    print(f"STAGE_CONS {label} {k} vs the general dense kernel: {e:.3e}")
                    if not e <= 2 * st.bound(e_ref[k]):
                        bad.append(f"{label} {k} vs dense: {e:.3e} (block {blk})")
            if i == 0:                                     # two calls give identical bytes
                again = _probe(ctx, path, o, pt, lam, tcg_init=True, delta=2.5, cert=True, X=pt["X"])
                for k, v in got.items():
                    same = v.tobytes() == again[k].tobytes() if isinstance(v, np.ndarray) else v == again[k]
                    assert same, (label, k)
        ctx.close()
    finally:
        if "symv_k" in path:
            xmamd._chk(L.xm_bench_symv_k(0, 1, 0))
    assert not bad, bad


SYMV_MK, SYMV_TUNING = ("dense", 128, 0), dict(sym=1, sym_min_rows=1)   # ld = 384: two strips, 64 steps


def _symv_plan(xmamd, n):
    plan = (C.c_int32 * 4)()
    xmamd._chk(xmamd.lib().xm_symv_plan(n, plan))
    return tuple(plan)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "hess_f32"])
def test_symv_plan_does_not_move_under_a_live_context(xmamd, f32):
    """the symmetric pair's chunk plan belongs to the workspace it sized: xm_bench_symv_k between two probes of one context changes no byte of
    any output (gradient, Hessian product -- the fp32 sweep with hess_f32 --, the certificate's o = 1 launch on the same workspace).  The
    override only moves to LONGER chunks here (4 records per column allocated, 2 asked for)."""
    L = xmamd.lib()
    n = rs.matrix(*SYMV_MK)["n"]
    assert _symv_plan(xmamd, n) == (4, 4, 1, 4)            # the default the test stands on: K = Kf = 4, no finer cut, nchunks = 4
    pt, E, e_ref, lam = rs.reference(SYMV_MK, 3, False, False)
    path = dict(auto=False)
    try:
        ctx = _ctx(xmamd, SYMV_MK, dict(SYMV_TUNING, hess_f32=1) if f32 else SYMV_TUNING)
        first = _probe(ctx, path, 3, pt, lam, tcg_init=True, delta=2.5, cert=True, X=pt["X"])
        assert first["product_kind"] == "dense_sym"
        xmamd._chk(L.xm_bench_symv_k(8, 1, 8))
        assert _symv_plan(xmamd, n)[:2] == (8, 8) and _symv_plan(xmamd, n)[3] == 2   # what a workspace made now would get
        again = _probe(ctx, path, 3, pt, lam, tcg_init=True, delta=2.5, cert=True, X=pt["X"])
        for k, v in first.items():
            same = v.tobytes() == again[k].tobytes() if isinstance(v, np.ndarray) else v == again[k]
            assert same, k
        ctx.close()
    finally:
        xmamd._chk(L.xm_bench_symv_k(0, 1, 0))


def test_symv_workspace_made_under_the_override_uses_it(xmamd):
    """a context created after xm_bench_symv_k runs the forced plan: the bounds of the path sym-finer-cut"""
    L = xmamd.lib()
    n = rs.matrix(*SYMV_MK)["n"]
    pt, E, e_ref, lam = rs.reference(SYMV_MK, 3, False, False)
    try:
        xmamd._chk(L.xm_bench_symv_k(8, 1, 8))
        ctx = _ctx(xmamd, SYMV_MK, SYMV_TUNING)
        got = _probe(ctx, dict(auto=False), 3, pt, lam)
        assert got["product_kind"] == "dense_sym"
        bad = rs.compare("sym-override-8-8-o3", got, E, e_ref, rs.GRAD_KEYS + rs.HESS_KEYS)
        assert _symv_plan(xmamd, n)[:2] == (8, 8)
        ctx.close()
    finally:
        xmamd._chk(L.xm_bench_symv_k(0, 1, 0))
    assert not bad, bad


CONS = ["dense-n86", "sym-n87", "f32-sym-n86", "bsr-n200", "sell-n200-g1-c2-w1", "schur-n40", "auto-bsr-n17", "split8-n683"]


@pytest.mark.parametrize("pid", CONS)
def test_outputs_are_consistent_with_each_other(xmamd, pid):
    """without a reference (a layout slip that a shared misunderstanding would hide): the three sums from the partial sums = the same inner
    products formed on the host from the returned HpR, Hps; rr = the metric norm of the returned rg; f = <G, sR> / 2 + lam sum (s^2 - 1)^2;
    <u, H v> = <v, H u> through two calls; S X on identity columns is symmetric.  Each side of an equation is within its bound of the exact value
    (the test above), so two sides differ by at most the sum of the two bounds, times the magnitude of the terms."""
    path = BY_ID[pid]
    mk, f32 = path["mk"], path.get("f32", False)
    o = path["ranks"][-1]
    n = rs.matrix(*mk)["n"]
    pt, E, e_ref, lam = rs.reference(mk, o, f32, False)
    ctx = _ctx(xmamd, mk, path["tuning"])
    rows = np.array([0, 1, 2, 3 * (n // 2), 3 * (n // 2) + 1, 3 * n - 1])
    X = np.zeros((3 * n, rows.size)); X[rows, np.arange(rows.size)] = 1.0
    got = _probe(ctx, path, o, pt, lam, cert=True, X=X)
    s = pt["s"].astype(LD); s[0] = 1
    ps, rsv = pt["p"][1].astype(LD), pt["r"][1].astype(LD)
    ps[0] = rsv[0] = 0
    HpR, Hps = got["HpR"].astype(LD), got["Hps"].astype(LD)
    bH = st.bound(max(e_ref["HpR"], e_ref["Hps"]))
    for k, host in (("pHp", ex.inner(pt["p"][0].astype(LD), ps, HpR, Hps, s)), ("rHp", ex.inner(pt["r"][0].astype(LD), rsv, HpR, Hps, s)),
                    ("HpHp", ex.inner(HpR, Hps, HpR, Hps, s))):
        e = float(abs(got[k] - host) / E[k + "~"])
        print(f"STAGE_CONS {pid}-o{o} {k} from the partial sums vs from HpR, Hps: {e:.3e}")
        assert e <= st.bound(e_ref[k]) + 2 * bH, k
    rr = ex.inner(got["rgR"].astype(LD), got["rgs"].astype(LD), got["rgR"].astype(LD), got["rgs"].astype(LD), s)
    assert float(abs(got["rr"] - rr) / E["rr~"]) <= st.bound(e_ref["rr"]) + 2 * st.bound(max(e_ref["rgR"], e_ref["rgs"]))
    sR = pt["R"].astype(LD) * np.repeat(s, 3)[:, None]
    f = (got["G"].astype(LD) * sR).sum() / 2 + LD(lam) * ((s[1:] ** 2 - 1) ** 2).sum()
    assert float(abs(got["f"] - f) / E["f~"]) <= st.bound(e_ref["f"]) + st.bound(e_ref["G"])
    swapped = ctx.rtr_probe(o, lam, pt["R"], pt["s"], p=pt["r"], r=pt["p"], auto=path.get("auto", False))
    M = rs.matrix(*mk)
    oph = ex.Op(M["Q"].astype(np.float32).astype(np.float64)) if f32 else M["op"]
    Es = ex.hess_stage(oph, E, *pt["r"], *pt["p"], lam, LD)     # <p, H r>: the same terms with the roles of the two vectors exchanged
    e = abs(got["rHp"] - swapped["rHp"]) / float(max(E["rHp~"], Es["rHp~"]))
    print(f"STAGE_CONS {pid}-o{o} <r,Hp> vs <p,Hr>: {e:.3e}")
    assert e <= 2 * st.bound(e_ref["rHp"])
    sub = got["SX"][rows]                                  # X^T S X = S restricted to the rows
    Ec = ex.cert_stage(M["op"], pt["R"], pt["s"], lam, X, LD)
    Fc = ex.cert_stage(ex.Op(M["Q"]) if M["Q"] is not None else M["op"], pt["R"], pt["s"], lam, X, np.float64)
    asym = np.abs(sub - sub.T).max() / float(Ec["SX~"].max())
    print(f"STAGE_CONS {pid}-o{o} asymmetry of S on identity columns: {asym:.3e}")
    assert asym <= 2 * st.bound(rs.error(Fc["SX"], Ec, "SX")[0])
    ctx.close()


def test_certificate_operator_annihilates_a_golden_optimum(xmamd):
    """S sR ~ 0 at the optimum of the golden case simple1.  For lam = 0 the least-squares residual Z sR - Lam sR of camera i is its Riemannian
    gradient over 2 s_i plus, for a free scale, the scale gradient's share: |S sR|_F <= sqrt(rr) / min(s) with rr = <rg, rg> at the point."""
    G = os.path.join(tl.GOLDEN, "simple1")
    Q = tl.load_bin(os.path.join(G, "Q.bin"))
    ctx = xmamd.Context(Q=Q)
    R, s, info = ctx.solve(3, 1e-16, 0.0)
    assert info["status"] == 1 and info["rank"] == 3
    sR = tl.scale_rows(R, s)
    got = ctx.rtr_probe(3, 0.0, R, s, cert=True, X=sR)
    g = ex.grad_stage(ex.Op(Q), R, s, 0.0, LD)
    resid = float(np.linalg.norm(got["SX"]))
    print(f"STAGE_CONS simple1 |S sR| {resid:.3e}, sqrt(rr) {float(np.sqrt(g['rr'])):.3e}, |Q sR| {np.linalg.norm(Q @ sR):.3e}")
    assert resid <= float(np.sqrt(g["rr"])) / s.min() + 64 * st.EPS * float(np.abs(Q).dot(np.abs(sR)).max()) * np.sqrt(sR.size)
    ctx.close()


def _cg_compare(label, got, case, parts, bad):
    """one cg_step launch against the longdouble body fed with the launch's own inputs: Hp and the three sums as the GPU's Hessian stage left them"""
    pt, n = case["pt"], case["pt"]["s"].size
    sums = (got["pHp"], got["rHp"], got["HpHp"], None if parts is None else parts.astype(LD).sum())
    args = (case["sc"], sums, (got["HpR"], got["Hps"]), pt["p"], case["r"], case["v"], case["Hv"], pt["R"], pt["s"])
    E = ex.cg_step_stage(*args, LD, model_rec=case["model_rec"])
    F = ex.cg_step_stage(*args, np.float64, model_rec=case["model_rec"])
    X = case["expect"]
    assert E["branch"] == X["branch"] and got["scal_out"]["status"] == X["scal"]["status"] and got["scal_out"]["iter"] == X["scal"]["iter"], label
    OP = pt["R"].shape[1] | 1
    gpu = {k: got["out_" + k] for k in rs.CG_ARRAYS if k != "W"}
    gpu["W"] = got["out_W"] if got["w_native"] else got["out_Wpad"][:, :3 * OP].reshape(n, 3, OP)[:, :, :pt["R"].shape[1]]
    given = dict(vR=case["v"][0], vs=case["v"][1], HvR=case["Hv"][0], Hvs=case["Hv"][1], rR=case["r"][0], rs=case["r"][1], pR=pt["p"][0], ps=pt["p"][1])
    s1 = pt["s"].astype(LD); s1[0] = 1
    psm = pt["p"][1].astype(LD); psm[0] = 0
    W0 = ex.blk(pt["p"][0].astype(LD), n) * s1[:, None, None] + ex.blk(pt["R"].astype(LD), n) * psm[:, None, None]   # what the Hessian stage multiplied
    for k in rs.CG_ARRAYS:
        if case["model_rec"] and k in ("HvR", "Hvs"):
            continue
        blocks = lambda a: ex.blk(np.asarray(a), n) if k.endswith("R") or k == "W" else np.asarray(a)
        if _untouched(E["branch"], k) and k != "W":        # the input bits come back
            assert np.array_equal(np.asarray(gpu[k]).reshape(given[k].shape), given[k]), (label, k)
            continue
        xe, xf, scale = (W0, W0.astype(np.float64), np.abs(W0).max(axis=(1, 2))) if _untouched(E["branch"], k) else (E[k], F[k], E.get(k + "~"))
        e_ref = st.err(blocks(xf), xe, scale)[0]
        e, blk = st.err(blocks(gpu[k]), xe, scale)
        print(f"STAGE_ERR {label} {k}: e_ref {e_ref:.3e}, e_gpu {e:.3e}, ratio {e / st.bound(e_ref):.3f}")
        if not e <= st.bound(e_ref):
            bad.append(f"{label} {k}: {e:.3e} > {st.bound(e_ref):.3e} (block {blk})")
    for k in rs.CG_SCALARS + (("rr_parts",) if E["rr_parts"] is not None else ()):
        xe, xf, xg = (E[k], F[k], got[k]) if k == "rr_parts" else (E["scal"][k], F["scal"][k], got["scal_out"][k])
        e_ref, e = st.err(np.asarray(xf), xe, E.get(k + "~"))[0], st.err(np.asarray(xg), xe, E.get(k + "~"))[0]
        print(f"STAGE_ERR {label} scal.{k}: e_ref {e_ref:.3e}, e_gpu {e:.3e}, ratio {e / st.bound(e_ref):.3f}")
        if not e <= st.bound(e_ref):
            bad.append(f"{label} scal.{k}: {e:.3e} > {st.bound(e_ref):.3e}")
    if E["rr_parts"] is None:
        assert not got["partsB_out"].any(), label              # only a CG step sums |r|^2
    else:
        assert abs(got["partsB_out"].astype(LD).sum() - LD(got["rr_parts"])) <= 64 * st.EPS * got["rr_parts"]
    assert got["scal_out"]["delta"] == case["sc"]["delta"] and got["scal_out"]["gradnorm"] == case["sc"]["gradnorm"]
    if not case["model_rec"]:
        assert got["scal_out"]["model"] == case["sc"]["model"]


def _untouched(branch, k):
    """the arrays a branch of cg_step_kernel does not write: nothing at rr < 1e-15; r, p and the product input at the boundary and at negative
    curvature; p and the product input at convergence"""
    return branch == 5 or (branch in (1, 2) and k in ("rR", "rs", "pR", "ps", "W")) or (branch == 3 and k in ("pR", "ps", "W"))


@pytest.mark.parametrize("cid", [c["id"] for c in rs.CG_CONTEXTS])
def test_cg_step_against_the_longdouble_reference(xmamd, cid):
    """one launch of cg_step_kernel per branch of trustregion.h:565-644: statuses, iter and the arrays a branch leaves alone exactly, everything
    else within the bound; with and without XM_FLAG_MODEL_RECURRENCE; at iter > 0 <r,r> comes from the partial sums of the launch before; the
    last context has more than one element per thread (the grid-stride loop's second leg)"""
    c = next(x for x in rs.CG_CONTEXTS if x["id"] == cid)
    ctxs = {}
    bad = []
    for o in c["ranks"]:
        for name in c["names"]:
            mk = c["mk_neg"] if name == "negative" else c["mk"]
            if mk not in ctxs:
                ctxs[mk] = _ctx(xmamd, mk, c["tuning"])
            case = rs.cg_case(mk, o, name)
            pt = case["pt"]
            first = ctxs[mk].rtr_probe(o, case["lam"], pt["R"], pt["s"])
            n = pt["s"].size
            if cid == "cg-bsr-stride":
                assert 3 * n * (o | 1) > 1024 * 256 and first["nB"] == 1024
            kw, parts = rs.cg_inputs(case, first["nB"])
            got = ctxs[mk].rtr_probe(o, case["lam"], pt["R"], pt["s"], **kw)
            _cg_compare(f"{cid}-o{o}-{name}", got, case, parts, bad)
    for ctx in ctxs.values():
        ctx.close()
    assert not bad, bad


def _solve_bits(ctx, flags=0):
    R, s, info = ctx.solve(5, 1e-8, 0.0, flags=flags)
    return R.tobytes(), s.tobytes(), info["primal"], info["tcg_iters"], info["status"]


@pytest.mark.parametrize("pid", ["dense-n43", "sym-n86", "bsr-n200", "sell-n200-g1-c1-w1", "schur-n40"])
def test_solve_after_a_probe_gives_the_same_bits(xmamd, pid):
    path = BY_ID[pid]
    a, b = _ctx(xmamd, path["mk"], path["tuning"]), _ctx(xmamd, path["mk"], path["tuning"])
    pt, E, e_ref, lam = rs.reference(path["mk"], 4, False, False)
    case = rs.cg_case(("dense", 43, 0), 3, "interior7") if pid == "dense-n43" else None
    a.rtr_probe(4, lam, pt["R"], pt["s"], p=pt["p"], r=pt["r"], tcg_init=True, cert=True, X=pt["X"])
    if case is not None:
        nB = a.rtr_probe(3, case["lam"], case["pt"]["R"], case["pt"]["s"])["nB"]
        a.rtr_probe(3, case["lam"], case["pt"]["R"], case["pt"]["s"], **rs.cg_inputs(case, nB)[0])
    ra, rb = _solve_bits(a), _solve_bits(b)
    assert ra == rb and ra[4] == 1
    a.rtr_probe(3, lam, *(rs.reference(path["mk"], 3, False, False)[0][k] for k in ("R", "s")))     # between two solves as well
    assert _solve_bits(a) == _solve_bits(b)
    a.close(); b.close()


def _raw(xmamd, ctx, n, o=3, flags=0, struct_size=None, nan=None, s0=1.0, with_p=False, iter_=0, parts=0):
    q = xmamd.RtrProbe()
    q.struct_size = C.sizeof(q) if struct_size is None else struct_size
    q.o, q.lam, q.flags = o, 1.0, flags
    oo = max(o, 3)
    keep = dict(R=np.asfortranarray(np.tile(np.eye(3, oo), (n, 1))), s=np.full(n, s0), pR=np.zeros((3 * n, oo), order="F"), ps=np.zeros(n),
                vR=np.zeros((3 * n, oo), order="F"), vs=np.zeros(n), HvR=np.zeros((3 * n, oo), order="F"), Hvs=np.zeros(n), partsB_in=np.ones(max(parts, 1)))
    if nan:
        keep[nan][-1, ...] = np.nan
    for k in ("R", "s") + (("pR", "ps", "vR", "vs", "HvR", "Hvs", "partsB_in") if with_p else ()):
        setattr(q, k, keep[k].ctypes.data_as(C.c_void_p))
    q.scal_in.rr, q.scal_in.pp, q.scal_in.delta, q.scal_in.iter, q.partsB_in_count = 1.0, 1.0, 1.0, iter_, parts
    return xmamd.lib().xm_ctx_rtr_probe(ctx.h, C.byref(q)), q


def test_refusals_leave_contexts_usable(xmamd):
    ERR_ARG = -2
    err = lambda: xmamd.lib().xm_last_error().decode()
    V = tl.gen_vg(40, deg=6, sigma=0.05, seed=80)
    two = xmamd.Context(Q=V["Q"], n_gpus=2, gpu_map=1)
    assert _raw(xmamd, two, 40)[0] == ERR_ARG and "single" in err()
    two.close()
    dense, sell = xmamd.Context(Q=V["Q"], tuning=dict(sym=-1)), xmamd.Context(bsr=(V["rowptr"], V["colidx"], V["blocks"]), tuning=dict(sell=1))
    assert _raw(xmamd, dense, 40)[0] == 0
    for kw in (dict(o=0), dict(o=1), dict(o=2), dict(o=11), dict(struct_size=8), dict(nan="R"), dict(nan="s"), dict(nan="pR", with_p=True), dict(flags=64),
               dict(s0=0.0), dict(flags=xmamd.RTR_PROBE_CG_STEP), dict(flags=xmamd.RTR_PROBE_CG_STEP, with_p=True, iter_=3, parts=1),
               dict(flags=xmamd.RTR_PROBE_CG_STEP, with_p=True, nan="vs")):
        assert _raw(xmamd, dense, 40, **kw)[0] == ERR_ARG, kw
        assert "xm_ctx_rtr_probe" in err(), (kw, err())
    # the role-switching launch where the device-driven outer iteration does not apply: sliced ELL, the column split, matrix-free storage
    assert _raw(xmamd, sell, 40, flags=xmamd.RTR_PROBE_AUTO)[0] == ERR_ARG and "XM_RTR_PROBE_AUTO" in err()
    split = xmamd.Context(Q=tl.gen_dense(223, seed=5)["Q"], tuning=dict(sym=-1, split_k=2))
    assert _raw(xmamd, split, 223, flags=xmamd.RTR_PROBE_AUTO)[0] == ERR_ARG and _raw(xmamd, split, 223)[0] == 0
    assert _raw(xmamd, dense, 40, flags=xmamd.RTR_PROBE_AUTO)[0] == 0 and _raw(xmamd, sell, 40)[0] == 0
    for c in (dense, sell, split):                         # usable afterwards
        _, _, info = c.solve(4, 1e-8, 0.0)
        assert info["status"] == 1
        c.close()
