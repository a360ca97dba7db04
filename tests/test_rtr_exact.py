"""CPU tests of the longdouble reference of the trust region's stages (xm_rtr_exact.py) and of the bound the GPU stage tests apply
(xm_rtr_stages.py).  The reference cannot be compared with anything compiled, so it is held against first principles -- finite differences
of the cost along curves on the manifold, symmetry of the Hessian -- and the bound against deliberate faults: each of them, planted in the
f64 run, must exceed max(16 e_ref, 64 eps) on at least one case, or the bound would let the same fault through in a kernel."""
import numpy as np
import pytest

import xm_ba_stages as st
import xm_rtr_exact as ex
import xm_rtr_stages as rs

LD = ex.LD


def _fd_case(n, o, lam, seed):
    M = rs.matrix("dense", n, 0)
    pt = rs.make_point(n, o, seed)
    pR, ps = pt["p"][0], pt["p"][1].copy()
    uR, us = pt["r"][0], pt["r"][1].copy()
    ps[0] = us[0] = 0.0
    g = ex.grad_stage(M["op"], pt["R"], pt["s"], lam, LD)
    return M["op"], pt, g, (pR, ps), (uR, us)


def _differences(op, pt, lam, d, h):
    fp, fm = (ex.cost(op, *ex.curve(pt["R"], pt["s"], d[0], d[1], t), lam) for t in (h, -h))
    f0 = ex.cost(op, pt["R"], pt["s"], lam)
    return (fp - fm) / (2 * LD(h)), (fp - 2 * f0 + fm) / (LD(h) * LD(h))


@pytest.mark.parametrize("n,o,lam", [(5, 3, 10.0), (20, 4, 1000.0), (43, 7, 0.0), (86, 5, 10.0)])
def test_gradient_and_hessian_are_the_derivatives_of_the_cost(n, o, lam):
    """central first and second differences of f along the curve t -> (polar retraction of R + t pR, s exp(t ps / s)) in longdouble against
    <rg, p> and <p, H p> in the product metric, and the polarisation (d2(u + p) - d2(u - p)) / 4 against <u, H p>.  The tolerance is the
    scheme's own truncation error estimated from two step sizes: the value at h / 2 lies within 1.5 |D(h) - D(h / 2)| / 3 of the analytic
    one, and halving h quarters the error (ratio within 3.5 .. 4.5).  Observed at h = 1e-3: 2e-6 .. 8e-5 relative for the gradient, 7e-7 .. 4e-6
    for the Hessian, ratios 3.99 .. 4.01."""
    op, pt, g, p, u = _fd_case(n, o, lam, 31 * n + o)
    s = g["_s"]
    cast = lambda d: (d[0].astype(LD), d[1].astype(LD))
    Hp = ex.hess_stage(op, g, *p, *u, lam, LD)
    rgp = ex.inner(g["rgR"].reshape(3 * n, o), g["rgs"], *cast(p), s)
    assert abs(float(Hp["pHp"] - ex.inner(Hp["HpR"].reshape(3 * n, o), Hp["Hps"], *cast(p), s))) <= 1e-17 * float(Hp["pHp~"])
    h = 1e-3
    (a1, a2), (b1, b2) = _differences(op, pt, lam, p, h), _differences(op, pt, lam, p, h / 2)
    for name, exact, Dh, Dh2 in (("gradient", rgp, a1, b1), ("hessian", Hp["pHp"], a2, b2)):
        e1, e2 = float(abs(Dh - exact)), float(abs(Dh2 - exact))
        print(f"FD {name} n={n} o={o}: {e1 / float(abs(exact)):.2e} at h, {e2 / float(abs(exact)):.2e} at h/2, ratio {e1 / e2:.3f}")
        assert e2 <= 1.5 * float(abs(Dh - Dh2)) / 3
        assert 3.5 <= e1 / e2 <= 4.5
    plus, minus = (p[0] + u[0], p[1] + u[1]), (u[0] - p[0], u[1] - p[1])
    mixed = [(_differences(op, pt, lam, plus, t)[1] - _differences(op, pt, lam, minus, t)[1]) / 4 for t in (h, h / 2)]
    e1, e2 = (float(abs(m - Hp["rHp"])) for m in mixed)                # hess_stage's <r, Hp> with r = u
    assert e2 <= 1.5 * float(abs(mixed[0] - mixed[1])) / 3 and 3.5 <= e1 / e2 <= 4.5


@pytest.mark.parametrize("n,o,lam", [(1, 3, 10.0), (9, 3, 0.0), (20, 5, 1000.0), (43, 10, 10.0)])
def test_hessian_is_symmetric(n, o, lam):
    """<u, H v> = <v, H u> in longdouble, to 64 longdouble round-offs of the terms the two sums are formed from -- at a point and for tangent
    vectors that are on the manifold and in its tangent space to longdouble precision (those of make_point are to f64 precision only)"""
    op, pt, g, p, u = _fd_case(n, o, lam, 77 * n + o)
    R = ex.polar_rows(ex.blk(pt["R"].astype(LD), n)).reshape(3 * n, o)
    p, u = ex.tangent(R, p[0].astype(LD), p[1].astype(LD)), ex.tangent(R, u[0].astype(LD), u[1].astype(LD))
    g = ex.grad_stage(op, R, pt["s"], lam, LD)
    a = ex.hess_stage(op, g, *p, *u, lam, LD)
    b = ex.hess_stage(op, g, *u, *p, lam, LD)
    assert abs(float(a["rHp"] - b["rHp"])) <= 64 * float(np.finfo(LD).eps) * float(max(a["rHp~"], b["rHp~"]))


def _all_references():
    for p in rs.PATHS:
        for o in p["ranks"]:
            yield f"{p['id']}-o{o}", rs.reference(p["mk"], o, p.get("f32", False), p.get("optimum", False))


def test_f64_run_agrees_with_longdouble_on_every_gpu_case():
    """e_ref <= MAX_E_REF for every quantity of every case the GPU tests judge (a case that does not is no case to judge a kernel on), and
    for the cg_step cases: the f64 run of the body takes the longdouble run's branch and agrees on every output"""
    worst = {}
    for label, (pt, E, e_ref, lam) in _all_references():
        for k, v in e_ref.items():
            assert v <= rs.MAX_E_REF, (label, k, v)
            worst[k] = max(worst.get(k, 0.0), v)
    print("E_REF worst per quantity: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for c, o, name, case in _cg_cases():
        E, F = case["expect"], _cg_run(case, np.float64)
        assert F["branch"] == E["branch"] and F["scal"]["iter"] == E["scal"]["iter"]
        for k, e in _cg_errors(F, E).items():
            assert e <= rs.MAX_E_REF, (c["id"], o, name, k, e)
    # the outer iteration's other half (test_gpu_outer_stages.py): both retractions, the line search's form and the model decrease
    worst = {}
    for c in rs.OUTER_CONTEXTS:
        for o in rs.RETRACT_RANKS:
            for name, errs in rs.retract_case(c["mk"], o)["e_ref"].items():
                for k, v in errs.items():
                    assert v <= rs.MAX_E_REF, (c["id"], o, name, k, v)
                    worst[name + "." + k] = max(worst.get(name + "." + k, 0.0), v)
    print("E_REF worst per quantity of the retraction: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def _cg_cases(contexts=None):
    for c in contexts or rs.CG_CONTEXTS + rs.STEP_CONTEXTS:
        for o in c["ranks"]:
            for name in c["names"]:
                mk = c["mk_neg"] if name == "negative" else c["mk"]
                yield c, o, name, rs.cg_case(mk, o, name)


def _cg_run(case, dt, damage=None):
    h = case["hess"]
    sums = (h["pHp"], h["rHp"], h["HpHp"], LD(case["rr_total"]))
    return ex.cg_step_stage(case["sc"], sums, (h["HpR"], h["Hps"]), case["pt"]["p"], case["r"], case["v"], case["Hv"], case["pt"]["R"], case["pt"]["s"], dt,
                            damage=damage, model_rec=case["model_rec"], pHp_scale=h["pHp~"])


def _cg_errors(F, E):
    out = {}
    for k in rs.CG_ARRAYS:
        if E[k] is not None:
            out[k] = st.err(np.asarray(F[k]), E[k], E.get(k + "~"))[0]
    for k in rs.CG_SCALARS:
        out["scal." + k] = st.err(np.asarray(F["scal"][k]), E["scal"][k], E.get(k + "~"))[0]
    if E["rr_parts"] is not None:
        out["rr_parts"] = st.err(np.asarray(F["rr_parts"]), E["rr_parts"])[0]
    return out


def test_cg_step_cases_take_their_branch_with_a_margin():
    """every comparison a branch of the tCG body depends on -- the sign of alpha (:577), |v + alpha p|^2 against delta^2 (:589), the stop test
    (:627), rr < 1e-15 (:572) -- keeps a relative distance of at least MARGIN in the longdouble run, so f64 and the GPU must take the same
    branch; and every branch the GPU tests list is taken by some case"""
    seen = set()
    for c, o, name, case in _cg_cases():
        E = case["expect"]
        assert E["branch"] == rs.CG_BRANCHES[name], (c["id"], o, name, E["branch"])
        for what, m in E["margins"].items():
            assert m >= rs.MARGIN, (c["id"], o, name, what, m)
        seen.add(E["branch"])
        if name.startswith("interior7"):
            assert E["scal"]["iter"] == 8
        if name == "cap":
            assert E["scal"]["iter"] == ex.MAX_INNER and E["W"] is not None
    assert seen == {0, 1, 2, 3, 5, 6}


FAULT_CASES = [("dense-n5", 3), ("dense-n43", 4), ("dense-n86", 5), ("bsr-n17", 3), ("sym-n9", 3)]
OUTER_FAULTS = ("m_no_scale", "m_metric_s", "anchor_scale", "mgs_raw_row", "rou_sign", "double_any")


def _decide_inputs(b, f=7.25, m=-0.8, rr_new=3.0):
    """the decision's inputs for one branch of rs.decide_branches around given sums: the loss is placed so that rho hits the branch's target"""
    m = 0.3 if b["rho"] is None else m
    loss = f + 1.0 if b["rho"] is None else f - b["rho"] * m
    sc = dict(delta=b["delta"], status=b["status"], iter=b["iter"], phase=ex.PH_CAND, seq=5)
    os_ = dict(loss=loss, rr_point=4.0, totalite=11, shrink_count=b["shrink"], k=b["k"], time_up=b["time_up"], slots=9)
    return sc, os_, (f, rr_new, m, b["delta_bar"], b["gradtol"], b["max_outer"] or 1000, b["stop_req"])


def _outer_faults(fault):
    """the new faults in the f64 run: the retraction's and the model's against the longdouble reference with the bound, the decision's (plain f64
    code compared exactly) as any output that differs"""
    broken = []
    for c in rs.OUTER_CONTEXTS[:3]:
        for o in (3, 4):
            case = rs.retract_case(c["mk"], o)
            pt, E, e_ref = case["pt"], case["E"], case["e_ref"]
            ds = case["v"][1]                              # (0.9 at the anchor)
            F = ex.retract_stage(pt["R"], pt["s"], case["v"][0], ds, 1.0, False, np.float64, fault)
            broken += [(c["id"], o, k, rs.error(F[k], E["mgs"], k)[0]) for k in rs.RETRACT_KEYS if rs.error(F[k], E["mgs"], k)[0] > st.bound(e_ref["mgs"][k])]
            g = ex.grad_stage(ex.Op(rs.matrix(*c["mk"])["Q"]) if rs.matrix(*c["mk"])["Q"] is not None else rs.matrix(*c["mk"])["op"], pt["R"], pt["s"], case["lam"], np.float64)
            Fm = ex.model_stage(case["v"], case["Hv"], (g["rgR"], g["rgs"]), pt["s"], np.float64, fault)
            e = rs.error(Fm["m"], E["model"], "m")[0]
            if e > st.bound(e_ref["model"]["m"]):
                broken.append((c["id"], o, "m", e))
    for b in rs.decide_branches():
        sc, os_, rest = _decide_inputs(b)
        good, bad = ex.outer_decide_stage(sc, os_, *rest), ex.outer_decide_stage(sc, os_, *rest, damage=fault)
        broken += [("decide-" + b["name"], 0, k, 1.0) for k in good if good[k] != bad[k]]
    return broken


@pytest.mark.parametrize("fault", ex.FAULTS + (None,))
def test_every_deliberate_fault_breaks_the_bound(fault):
    """the faults a trust region survives (it converges to the same certified optimum, only more slowly) planted in the f64 run: no S0 term; no
    ps s egs; the anchor not masked in egs, in hs and rhs, in the direction's scale part; sym replaced by the unsymmetrised product; s^2 - 1 for
    3 s^2 - 1; rr_est without its cross term; tau's other root; the vp recurrence without beta; the anchor's multipliers from five generators;
    dz on the wrong row; the scale term of the model decrease dropped; its metric 1 / s for 1 / s^2; the anchor's scale moved by the retraction;
    the second Gram-Schmidt projection against the unnormalised row; rho with the sign of m flipped; the radius doubled whatever ended the tCG.  (The masks of hs and of rs at the anchor are each covered by a second one -- rhs is masked as well, and rs only ever
    multiplies rhs -- so one of them missing alone changes no output: they are planted together with the mask that covers them.)"""
    broken = []
    if fault in OUTER_FAULTS or fault is None:
        broken += _outer_faults(fault)
    if fault in ("rr_est_no_cross", "tau_root", "vp_no_beta", None):
        for c, o, name, case in _cg_cases(rs.CG_CONTEXTS):
            if c["id"] != "cg-dense":
                continue
            E = case["expect"]
            e_ref, e = _cg_errors(_cg_run(case, np.float64), E), _cg_errors(_cg_run(case, np.float64, fault), E)
            broken += [(name, o, k, e[k]) for k in e if e[k] > st.bound(e_ref[k])]
    if fault not in ("rr_est_no_cross", "tau_root", "vp_no_beta") + OUTER_FAULTS:
        by_id = {p["id"]: p for p in rs.PATHS}
        for pid, o in FAULT_CASES:
            p = by_id[pid]
            pt, E, e_ref, lam = rs.reference(p["mk"], o)
            M = rs.matrix(*p["mk"])
            op = ex.Op(M["Q"]) if M["Q"] is not None else M["op"]
            g = ex.grad_stage(op, pt["R"], pt["s"], lam, np.float64, fault)
            F = dict(g)
            F.update(ex.hess_stage(op, g, *pt["p"], *pt["r"], lam, np.float64, fault))
            F.update(ex.cert_stage(op, pt["R"], pt["s"], lam, pt["X"], np.float64, fault))
            for k in rs.GRAD_KEYS + rs.HESS_KEYS + rs.CERT_KEYS:
                e = rs.error(F[k], E, k)[0]
                if e > st.bound(e_ref[k]):
                    broken.append((pid, o, k, e))
    print(f"FAULT {fault}: " + ", ".join(f"{a}-o{b} {k} {e:.1e}" for a, b, k, e in broken[:6]))
    assert (not broken) if fault is None else broken, (fault, broken[:6])    # None: the control -- the same loop without a fault reports nothing


def test_f_above_loss_in_the_reject_test_changes_nothing():
    """`f > loss` of trustregion.h:702 cannot be reached alone: the test is only looked at with m < 0, where f > loss gives rho = (f - loss) / m
    <= -0 < 0.1.  So the fault "f > loss dropped" (ex.EQUIVALENT_FAULTS) breaks no output, here over every branch and a grid of sums that
    includes f a hair above the loss, equal to it and far from it, and m from tiny to huge -- it is listed apart from ex.FAULTS for that reason,
    and no GPU case can exist for "reject by f > loss with rho >= 0.1"."""
    assert ex.EQUIVALENT_FAULTS == ("no_f_gt_loss",) and not set(ex.EQUIVALENT_FAULTS) & set(ex.FAULTS)
    count = 0
    for b in rs.decide_branches():
        for m in (-1e-300, -1e-12, -0.8, -1e12, -1e300):
            for gap in (0.0, 5e-324, 1e-300, 2.0 ** -52, 1e-3, 1.0, 1e300, -1e-3, -2.0 ** -52):
                sc, os_, rest = _decide_inputs(b)
                os_["loss"] = 7.25
                f = np.nextafter(7.25, np.inf) if gap == 2.0 ** -52 else np.nextafter(7.25, -np.inf) if gap == -2.0 ** -52 else 7.25 + gap
                rest = (f, rest[1], m) + rest[3:]
                with np.errstate(over="ignore"):            # (rho = -inf at the corners of the grid)
                    assert ex.outer_decide_stage(sc, os_, *rest) == ex.outer_decide_stage(sc, os_, *rest, damage="no_f_gt_loss"), (b["name"], m, gap)
                count += 1
    assert count > 500


def test_decision_branches_are_reached_with_a_margin():
    """every branch of rs.decide_branches comes out as listed from the plain f64 restatement, and every target rho keeps a relative distance
    of more than MARGIN from the thresholds 0.1, 0.25 and 0.75, so the kernel's own sums (a few round-offs from any others) take the same branch"""
    for rho in rs.RHO_TARGETS:
        assert min(abs(rho - t) / t for t in (0.1, 0.25, 0.75)) > 1e3 * rs.MARGIN
    seen = set()
    for b in rs.decide_branches():
        sc, os_, rest = _decide_inputs(b)
        out = ex.outer_decide_stage(sc, os_, *rest)
        for k, v in b["expect"].items():
            assert out[k] == v, (b["name"], k, out[k], v)
        assert (out["trace"] is None) == (out["stop_reason"] in (12, 13, 14)), b["name"]
        assert out["phase"] == (ex.PH_TCG if out["start"] else ex.PH_STOP)
        seen.add(out["stop_reason"])
    assert seen == {0, 5, 10, 11, 12, 13, 14}
    init = ex.outer_decide_stage(dict(delta=2.0, status=0, iter=0, phase=ex.PH_INIT, seq=3), dict(loss=1.0, rr_point=4.0, totalite=0, shrink_count=0, k=0, time_up=0), 0, 0, 0, 1, 0, 1000, 0)
    assert (init["phase"], init["rr"], init["gradnorm"], init["delta"], init["k"], init["accept"], init["start"], init["trace"]) == (ex.PH_TCG, 4.0, 2.0, 2.0, 0, False, True, None)
    assert ex.outer_decide_stage(dict(phase=ex.PH_STOP), {}, 0, 0, 0, 1, 0, 1000, 0)["passed"]


@pytest.mark.parametrize("n,o,polar", [(5, 3, False), (20, 4, True), (43, 10, False), (43, 5, True)])
def test_the_retraction_is_a_retraction(n, o, polar):
    """Rn Rn^T = I to longdouble round-off, the anchor's scale stays, and d/dt at 0 is the tangent step: central differences at two step
    sizes, the error quartering (the curve is smooth), for the rows and for s exp(t ds / s)"""
    case = rs.retract_case(("dense", n, 0), o)
    pt, v = case["pt"], case["v"]
    E = ex.retract_stage(pt["R"], pt["s"], v[0], v[1], 1.0, polar, LD)
    gram = np.einsum("iak,ibk->iab", E["Rc"], E["Rc"]) - np.eye(3)
    assert float(np.abs(gram).max()) <= 64 * float(np.finfo(LD).eps)
    assert E["sc"][0] == 1 and float(np.abs(E["W"] - E["Rc"] * E["sc"][:, None, None]).max()) == 0.0
    R1 = ex.polar_rows(ex.blk(pt["R"].astype(LD), n)).reshape(3 * n, o)     # on the manifold to longdouble precision, and v tangent there
    vR, vs = ex.tangent(R1, v[0].astype(LD), v[1].astype(LD))
    errs = []
    for h in (1e-3, 5e-4):
        P, Mn = (ex.retract_stage(R1, pt["s"], vR, vs, t, polar, LD) for t in (h, -h))
        dR, ds = (P["Rc"] - Mn["Rc"]) / (2 * LD(h)), (P["sc"] - Mn["sc"]) / (2 * LD(h))
        errs.append((float(np.abs(dR - ex.blk(vR, n)).max()), float(np.abs(ds - vs).max())))
    for e1, e2 in zip(*errs):
        assert e2 <= 1e-4 and 3.5 <= e1 / e2 <= 4.5, errs


@pytest.mark.parametrize("n,o,lam", [(5, 3, 10.0), (20, 4, 1000.0), (43, 7, 0.0)])
def test_model_decrease_is_the_second_order_expansion_of_the_cost(n, o, lam):
    """m(v) = <v, rg> + <v, Hv> / 2 with Hv from hess_stage against D1 + D2 / 2, the central first and second differences of the cost along
    curve() with velocity v: within the scheme's truncation error estimated from two step sizes, as in the test of the derivatives above"""
    op, pt, g, p, u = _fd_case(n, o, lam, 53 * n + o)
    H = ex.hess_stage(op, g, *p, *u, lam, LD)
    m = ex.model_stage(p, (H["HpR"].reshape(3 * n, o), H["Hps"]), (g["rgR"].reshape(3 * n, o), g["rgs"]), pt["s"], LD)
    assert abs(float(m["m"] - m["m_cam"].sum())) == 0.0
    h = 1e-3
    (a1, a2), (b1, b2) = _differences(op, pt, lam, p, h), _differences(op, pt, lam, p, h / 2)
    e1, e2 = float(abs(a1 + a2 / 2 - m["m"])), float(abs(b1 + b2 / 2 - m["m"]))
    print(f"FD model n={n} o={o}: {e1 / float(abs(m['m'])):.2e} at h, {e2 / float(abs(m['m'])):.2e} at h/2, ratio {e1 / e2:.3f}")
    assert e2 <= 1.5 * (float(abs(a1 - b1)) + float(abs(a2 - b2)) / 2) / 3
    assert e2 <= 1e-4 * float(m["m~"])


# ---------------------------------------------------------------------------------------------------------------- the certificate's eigen-solver
import xm_cert_stages as cs

EPS_LD = float(np.finfo(LD).eps)


@pytest.mark.parametrize("cid", ["single-n5", "single-n43", "single-n43-optimum"])
def test_lanczos_reference_tridiagonalises_S(cid):
    """the whole run in longdouble, taken through all 3n steps (or to an invariant subspace): V^T V = I (column 0 is normalised in f64 as the
    solver's start vector is: 4 eps_f64 on its diagonal entry; everything else to longdouble round-off), S V_m = V_m T_m + beta_{m-1} v_m e_m^T
    entry by entry against the magnitude of the terms, and theta = the smallest eigenvalue of S (numpy's eigvalsh of the f64 matrix, whose own
    error is a few eps |S|; theta is the midpoint of an interval of 4e-16 max(1, tmax))"""
    S = cs.setup(cid)
    n = S["n"]
    E = ex.lanczos_stage(S["op"], S["C"], LD, **cs.run_settings(cs.BY_ID[cid]))
    m, V = E["m_use"], E["V"]
    G = V[:, :m].T @ V[:, :m] - np.eye(m)
    assert abs(float(G[0, 0])) <= 4 * st.EPS
    G[0, 0] = 0
    assert float(np.abs(G).max()) <= 64 * m * EPS_LD, float(np.abs(G).max())
    Sd = cs.dense_S(S, LD)
    T = np.diag(E["alpha"]) + np.diag(E["beta"][:m - 1], 1) + np.diag(E["beta"][:m - 1], -1)
    D = Sd @ V[:, :m] - V[:, :m] @ T
    D[:, m - 1] -= E["beta"][m - 1] * V[:, m]
    scale = np.abs(Sd) @ np.abs(V[:, :m]) + np.abs(V[:, :m + 1]) @ np.abs(np.vstack([T, np.eye(m)[m - 1:] * E["beta"][m - 1]]))
    assert float((np.abs(D) / scale).max()) <= 64 * m * EPS_LD
    assert E["eig_exact"] and E["ret"] == 0
    ev = np.linalg.eigvalsh(Sd.astype(np.float64))
    unit = max(1.0, float(E["tmax"]))
    assert abs(float(E["theta"]) - ev[0]) <= 8e-16 * unit + 16 * st.EPS * np.abs(ev).max()
    x = E["x"]
    r = Sd @ x - E["theta"] * x
    assert float(np.sqrt(r @ r)) <= 1e-6 * unit            # (inverse iteration with a shift 1e-14 away: the vector is far better than theta)


def _critical_point(n, o, lam, seed):
    """a matrix Q for which a random point (R, s) is a critical point of the cost with multipliers that are not zero: Q = L - dz + P A P with
    L block diagonal and symmetric (traceless blocks for every camera but the anchor: the scale's stationarity), dz the diagonal term of the
    certificate, P the projector onto the complement of the columns of s R and A any symmetric matrix; then Z sR = L sR, and S = P A P"""
    rng = np.random.default_rng(seed)
    R, s = cs.make_point(n, o, seed)
    R, s = ex.point(R, s, LD)
    R = ex.polar_rows(ex.blk(R, n)).reshape(3 * n, o)
    Y = R * np.repeat(s, 3)[:, None]
    L = np.zeros((3 * n, 3 * n), dtype=LD)
    for i in range(n):
        B = rng.standard_normal((3, 3)).astype(LD)
        B = (B + B.T) / 2
        if i > 0:
            B -= np.eye(3) * np.trace(B) / 3
        L[3 * i:3 * i + 3, 3 * i:3 * i + 3] = B
    dz = np.zeros(3 * n, dtype=LD)
    dz[0::3] = 2 * LD(lam) * (s * s - 1)
    P = np.eye(3 * n, dtype=LD) - Y @ rs.solve_ld(Y.T @ Y, Y.T)
    A = rng.standard_normal((3 * n, 3 * n)).astype(LD)
    Q = L - np.diag(dz) + P @ ((A + A.T) / 2) @ P
    return ex.Op((Q + Q.T) / 2), R, s, L


@pytest.mark.parametrize("n,o,lam,polar", [(6, 4, 10.0, False), (9, 3, 1000.0, True), (5, 5, 0.0, False)])
def test_ritz_vector_is_the_escape_direction_the_staircase_uses(n, o, lam, polar):
    """at a critical point of rank o, with v = x / s in a new last column, the cost along the line search's retraction of [R 0] + t [0 v] is
    f + t^2 x^T S x + O(t^3) -- for the Ritz pair of the reference's whole run, t^2 theta.  Central second differences at h and h / 2: the
    value at h / 2 within the scheme's truncation error estimated from the two, and the error quartering (ratio 3.5 .. 4.5).  The critical
    point is built, not found: _critical_point."""
    op, R, s, L = _critical_point(n, o, lam, 90 + n)
    C = ex.cert_stage(op, R, s, lam, None, LD)
    assert float(np.abs(C["Lam"] - np.stack([L[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(n)])).max()) <= 1e4 * EPS_LD * float(np.abs(L).max())
    E = ex.lanczos_stage(op, C, LD)
    assert E["eig_exact"] and float(E["theta"]) < -0.1     # a direction of descent
    x, theta = E["x"], E["theta"]
    Rp = np.concatenate([R, np.zeros((3 * n, 1), dtype=LD)], axis=1)
    D = np.zeros_like(Rp)
    D[:, o] = x / np.repeat(s, 3)
    f = lambda t: ex.cost(op, ex.retract_stage(Rp, s, D, None, t, polar, LD)["Rc"].reshape(3 * n, o + 1), s, lam)
    f0 = ex.cost(op, R, s, lam)
    assert abs(float(f(0.0) - f0)) <= 1e3 * EPS_LD * abs(float(f0))
    d2 = [(f(h) - 2 * f0 + f(-h)) / (LD(h) * LD(h)) / 2 for h in (1e-2, 5e-3)]
    e1, e2 = (float(abs(d - theta)) for d in d2)
    print(f"FD escape n={n} o={o}: {e1 / abs(float(theta)):.2e} at h, {e2 / abs(float(theta)):.2e} at h/2, ratio {e1 / e2:.3f}")
    assert e2 <= 1.5 * float(abs(d2[0] - d2[1])) / 3 and 3.5 <= e1 / e2 <= 4.5
    assert e2 <= 1e-3 * abs(float(theta))


LZ_FAULT_CASES = ("single-n43", "dense-n130", "seg2-n2731", "restarts-n130")


def _lz_fault_run(cid, fault):
    case = cs.BY_ID[cid]
    S = cs.setup(cid)
    n = S["n"]
    pos = np.roll(np.arange(n), 1)                         # a partition that moves every camera (one rank keeps the identity)
    F = ex.lanczos_stage(S["op64"], S["C64"], np.float64, damage=fault, pos=pos, **cs.run_settings(case))
    return cs.compare_run(f"{cid}-{fault}", S, cs.as_run(F), case, who="f64", e_ref_run=cs.as_run(S["F"]))


@pytest.mark.parametrize("fault", ex.LZ_FAULTS + (None,))
def test_every_deliberate_lanczos_fault_breaks_the_bound(fault):
    """the faults a certificate survives, planted in the f64 whole run and judged as the GPU's run is (xm_cert_stages.compare_run): the second
    Gram-Schmidt pass dropped; the last column left out of the subtraction; alpha from the first pass alone; beta without the square root; one
    segment's terms dropped from the first pass's dots; y reversed in the Ritz vector; the Ritz vector left in the partition's order.  None: the
    control.  alpha from the first pass alone differs from alpha by c2[j], which from an orthonormal basis is one round-off of the terms: from
    the run's own basis it stays under the bound, so it is planted in the step form as well, from a basis that is orthonormal to 1e-6 only --
    there it must break alpha and nothing else."""
    broken = []
    for cid in LZ_FAULT_CASES:
        broken += _lz_fault_run(cid, fault)
    if fault in ("lz_alpha_pass1", None):
        S = cs.setup("dense-n130")
        rng = np.random.default_rng(5)
        V = np.asarray(S["F"]["V"][:, :9]) + 1e-6 * rng.standard_normal((3 * S["n"], 9))
        E = ex.lanczos_stage(S["op"], S["C"], LD, V=V)
        F, Fd = (ex.lanczos_stage(S["op64"], S["C64"], np.float64, V=V, damage=d) for d in (None, fault))
        hit = [k for k in ex.LZ_STEP_KEYS if rs.error(Fd[k], E, k)[0] > st.bound(rs.error(F[k], E, k)[0])]
        assert hit == (["alpha"] if fault else []), hit
        broken += hit
    print(f"FAULT {fault}: " + "; ".join(broken[:6]))
    assert (not broken) if fault is None else broken, (fault, broken[:6])


def test_lanczos_cases_end_as_the_gpu_tests_expect():
    """the f64 run of the reference ends every case the way tests/test_gpu_cert_stages.py asserts for the GPU, with a margin at each threshold
    the ending depends on: the exhaustion cases stop at m = 2 with beta_1 a factor 10 under 1e-13 max(1, tmax) and beta_0 far above; the run that
    is cut short keeps its residual a factor 1e3 above the convergence limit; the segment counts are those listed"""
    for case in cs.CASES:
        S = cs.setup(case["id"])
        F = S["F"]
        for k, v in case.get("expect", {}).items():
            if k in F:
                assert int(F[k]) == v, (case["id"], k, F[k])
        assert ex.dots_segments(-(-3 * S["n"] // 128) * 128)[0] == case["nseg"], case["id"]
        unit = max(1.0, float(F["tmax"]))
        if case.get("exhaust"):
            assert F["beta"][1] <= 1e-14 * unit and F["beta"][0] >= 1e-3 * unit, (case["id"], F["beta"])
            assert abs(float(F["theta"])) <= 64 * st.EPS * S["n"]
        if case["id"] == "cut-short-n130":
            assert float(F["resid"]) >= 1e-3 * unit
        if case.get("restarts"):
            assert F["cycles"] > 1
    nseg, seg = ex.dots_segments(262272)
    assert (nseg, seg) == (64, 4352) and sum(1 for q in range(64) if q * seg >= 262272) == 3      # the last three segments are empty
    assert ex.dots_segments(8320) == (2, 4352) and ex.dots_segments(12416)[0] == 3
