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


def _cg_cases():
    for c in rs.CG_CONTEXTS:
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


@pytest.mark.parametrize("fault", ex.FAULTS + (None,))
def test_every_deliberate_fault_breaks_the_bound(fault):
    """the faults a trust region survives (it converges to the same certified optimum, only more slowly) planted in the f64 run: no S0 term; no
    ps s egs; the anchor not masked in egs, in hs and rhs, in the direction's scale part; sym replaced by the unsymmetrised product; s^2 - 1 for
    3 s^2 - 1; rr_est without its cross term; tau's other root; the vp recurrence without beta; the anchor's multipliers from five generators;
    dz on the wrong row.  (The masks of hs and of rs at the anchor are each covered by a second one -- rhs is masked as well, and rs only ever
    multiplies rhs -- so one of them missing alone changes no output: they are planted together with the mask that covers them.)"""
    broken = []
    if fault in ("rr_est_no_cross", "tau_root", "vp_no_beta", None):
        for c, o, name, case in _cg_cases():
            if c["id"] != "cg-dense":
                continue
            E = case["expect"]
            e_ref, e = _cg_errors(_cg_run(case, np.float64), E), _cg_errors(_cg_run(case, np.float64, fault), E)
            broken += [(name, o, k, e[k]) for k in e if e[k] > st.bound(e_ref[k])]
    if fault not in ("rr_est_no_cross", "tau_root", "vp_no_beta"):
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
