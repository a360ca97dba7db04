"""GPU tests of the other half of an outer iteration stage by stage through the test export xm_ctx_outer_probe: the retraction with the model
decrease it delivers (retract_kernel<O, POLAR, MV>, the line search's form included) and one step launch of the device-driven outer iteration
(outer_step_kernel) in each of its roles.  test_gpu_rtr_stages.py pins the gradient, the Hessian product and the tCG's start and step; a
wrong model decrease or a wrong trust-region update changes only which steps are accepted and how the radius moves, and every whole solve in
the suite would still certify.

Against the longdouble reference (xm_rtr_exact.py: retract_stage, model_stage, cg_step_stage) the bound is the project's own,
e_gpu <= max(16 e_ref, 64 eps_f64) per quantity and case (xm_rtr_stages.py), errors per camera block; every comparison prints
`STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s; profiles/r17_outer_stage_errors.txt condenses a run).  The reference is fed the
launch's own inputs (the gradient the model decrease is formed with, Hp and the three sums of a tCG step), so an output pins the one launch.
What the kernels' comments claim to be the same arithmetic is compared bit for bit: the step launch's cg role with cg_step_kernel, its tCG-ending
role with cg_step_kernel + retract_kernel (the per-wavefront model partials regrouped four by four giving the per-workgroup ones), its decision
role's start of the next tCG with tcg_init_kernel.  The decision itself is a handful of f64 operations on three sums: compared exactly with
ex.outer_decide_stage fed with those sums.

No case exists for "reject by f > loss with rho >= 0.1": with m < 0, f > loss makes rho negative (test_rtr_exact.py pins that the test changes
no output).

Which kernel an output pins: ret_*, model -> retract_kernel<O, POLAR, MV> (MV = false with model_recurrence) and outer_finalize_kernel; ls_* ->
retract_kernel in the line search's form; the step launch's out_*, scal_out, os_out, progress, trace -> outer_step_kernel by role."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_rtr_stages as base
import xm_ba_stages as st
import xm_rtr_exact as ex
import xm_rtr_stages as rs
import xm_testlib as tl

pytestmark = pytest.mark.gpu

LD = ex.LD
TCG_VECTORS = ("vR", "vs", "HvR", "Hvs", "rR", "rs", "pR", "ps")
SCAL_FIELDS = ("rr", "vv", "vp", "pp", "delta", "gradnorm", "last_step", "model", "status", "iter")


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).reshape(np.asarray(a).shape).tobytes()


def _one(label, k, x, xe, xf, scale, bad):
    """one quantity against its longdouble value, the f64 run's error giving the bound"""
    e_ref, (e, blk) = st.err(xf, xe, scale)[0], st.err(x, xe, scale)
    print(f"STAGE_ERR {label} {k}: e_ref {e_ref:.3e}, e_gpu {e:.3e}, ratio {e / st.bound(e_ref):.3f}")
    if not e <= st.bound(e_ref):
        bad.append(f"{label} {k}: {e:.3e} > {st.bound(e_ref):.3e} (e_ref {e_ref:.3e}, block {blk})")


def _retraction(label, n, o, Rc, sc, W, E, F, bad):
    for k, x in (("Rc", ex.blk(np.asarray(Rc), n)), ("sc", sc), ("W", ex.blk(np.asarray(W), n))):
        if x is not None:
            _one(label, k, x, E[k], F[k], E[k + "~"], bad)


def _wpad_rows(Wpad, n, o):
    OP = o | 1
    return Wpad[:, :3 * OP].reshape(n, 3, OP)[:, :, :o]


def _model(label, parts, model, v, Hv, rg, s, bad):
    """the model decrease from the launch's partial sums against the longdouble sum formed with the launch's own gradient"""
    E, F = (ex.model_stage(v, Hv, rg, s, dt) for dt in (LD, np.float64))
    _one(label, "partsM", parts.astype(LD).sum(), E["m"], F["m"], E["m~"], bad)
    if model is not None:                                  # the result kernel's sum of the same partials
        assert abs(LD(model) - parts.astype(LD).sum()) <= 64 * st.EPS * E["m~"], label
    return E


@pytest.mark.parametrize("cid", rs.OUTER_IDS + ["sell-n131"])
def test_retraction_stage_against_the_longdouble_reference(xmamd, cid):
    """retract_kernel in the three forms a solve launches: with the model decrease (MV), without (XM_FLAG_MODEL_RECURRENCE) and the line search's
    (no scale step, no scales out); both retractions; ranks with and without the pad column; one, three and six wavefronts.  The sliced-ELL
    context is the one that keeps the padded copy of the product input"""
    if cid == "sell-n131":
        c = dict(id=cid, mk=("vg", 131, 6), tuning=dict(sell=1, sell_codec=1, sell_lmax=5, sell_wpad=1), kind="sell")
    else:
        c = next(x for x in rs.OUTER_CONTEXTS if x["id"] == cid)
    n = rs.matrix(*c["mk"])["n"]
    ctx = base._ctx(xmamd, c["mk"], c["tuning"])
    bad = []
    for o in rs.RETRACT_RANKS:
        case = rs.retract_case(c["mk"], o)
        pt, E, lam = case["pt"], case["E"], case["lam"]
        s1 = pt["s"].copy(); s1[0] = 1.0
        fill = np.cos(np.arange(1024.0))
        for name in rs.RETRACTIONS:
            label = f"{cid}-o{o}-{name}"
            F = {k: ex.retract_stage(pt["R"], pt["s"], *a, name == "polar", np.float64)
                 for k, a in (("ret", (case["v"][0], case["v"][1], 1.0)), ("ls", (case["D"], None, rs.LS_T)))}
            got = ctx.outer_probe(o, lam, pt["R"], pt["s"], v=case["v"], Hv=case["Hv"], retract=True, retraction=name, ls=(case["D"], rs.LS_T))
            if o <= 5:
                assert got["product_kind"] == c["kind"], (label, got["product_kind"])
            wpad = cid.startswith("sell") and o <= 5
            assert got["polar"] == (name == "polar") and got["nM"] == (n + 255) // 256 and got["nwave"] == (n + 63) // 64, label
            assert got["wpad"] == wpad and got["w_native"] != got["wpad"], label
            _retraction(label, n, o, got["ret_Rc"], got["ret_sc"], got["ret_W"], E[name], F["ret"], bad)
            if wpad:
                _one(label, "Wpad", _wpad_rows(got["ret_Wpad"], n, o), E[name]["W"], F["ret"]["W"], E[name]["W~"], bad)
                assert not got["ret_Wpad"][:, 3 * (o | 1):].any(), label       # what lies behind a record is never written
            assert got["ret_pad"] == (0, 0, 0 if wpad else -1), (label, got["ret_pad"])   # the pad column of every copy written: exactly 0
            assert got["ret_sc"][0] == 1.0, label                                          # the anchor's scale: untouched, whatever the step holds there
            _model(label, got["ret_partsM"], got["model"], case["v"], case["Hv"], (got["rgR"], got["rgs"]), s1, bad)
            _retraction(label + "-ls", n, o, got["ls_Rc"], None, got["ls_W"], E["ls-" + name], F["ls"], bad)
            assert got["ls_pad"] == (0, 0), (label, got["ls_pad"])
            rec = ctx.outer_probe(o, lam, pt["R"], pt["s"], v=case["v"], retract=True, model_recurrence=True, retraction=name, model=-0.625, partsM_fill=fill)
            _retraction(label + "-rec", n, o, rec["ret_Rc"], rec["ret_sc"], rec["ret_W"], E[name], F["ret"], bad)
            assert rec["ret_pad"] == got["ret_pad"] and rec["ret_sc"][0] == 1.0, label
            assert _same(rec["ret_partsM"], fill[:rec["nM"]]) and rec["model"] == -0.625, label     # no partial sums: the tCG's own model value goes out
    ctx.close()
    assert not bad, bad


def _step_inputs(case, parts, phase, slot, **kw):
    sc = dict(case["sc"], phase=phase, status=0, seq=11, last_step=0.0)
    os_ = dict(loss=1.5, rr_point=case["sc"]["rr"], totalite=17, shrink_count=2, k=5, stop_reason=0, time_up=0, slots=23)
    return dict(dict(scal=sc, os=os_, delta_bar=1e3, gradtol=1e-9, slot=slot, p=case["pt"]["p"], r=case["r"], partsB=parts), **kw)


def _chain(case, got, parts, dt):
    """the tCG body on the launch's own inputs (Hp and the three sums as the GPU's Hessian stage left them)"""
    pt = case["pt"]
    sums = (got["pHp"], got["rHp"], got["HpHp"], None if parts is None else parts.astype(LD).sum())
    return ex.cg_step_stage(case["sc"], sums, (got["HpR"], got["Hps"]), pt["p"], case["r"], case["v"], case["Hv"], pt["R"], pt["s"], dt, model_rec=case["model_rec"])


@pytest.mark.parametrize("cid", rs.STEP_IDS)
def test_step_launch_in_the_tcg_roles(xmamd, cid):
    """outer_step_kernel with phase = PH_TCG, one launch per branch of the tCG body.  A step that goes on: cg_step_kernel's outputs bit for bit.
    A step that ends the tCG: the candidate, its scale and the product input bit for bit those of cg_step_kernel + retract_kernel on the same
    inputs, the per-wavefront model partials regrouped four by four bit for bit retract_kernel's per-workgroup ones, the tCG's vectors left
    alone.  Both also within the bound of the longdouble chain.  The last context is the size at which the tCG-ending role's loop over
    wavefronts takes a second trip (grid 1024, more than 1024 wavefronts)."""
    c = next(x for x in rs.STEP_CONTEXTS if x["id"] == cid)
    ctxs, bad = {}, []
    for io, o in enumerate(c["ranks"]):
        retr = rs.RETRACTIONS[io % 2]
        for name in c["names"]:
            mk = c["mk_neg"] if name == "negative" else c["mk"]
            if mk not in ctxs:
                ctxs[mk] = base._ctx(xmamd, mk, c["tuning"])
            ctx, case = ctxs[mk], rs.cg_case(mk, o, name)
            pt, lam, n, rec = case["pt"], case["lam"], case["pt"]["s"].size, case["model_rec"]
            label = f"{cid}-o{o}-{name}"
            s1 = pt["s"].copy(); s1[0] = 1.0
            nB = ctx.rtr_probe(o, lam, pt["R"], pt["s"], auto=True)["nB"]
            kw, parts = rs.cg_inputs(case, nB)
            host = ctx.rtr_probe(o, lam, pt["R"], pt["s"], auto=True, **kw)        # the Hessian product in its EPI_AUTO form, then cg_step_kernel
            slot = case["sc"]["iter"]                                              # (the same parity copies and sweep direction as the host-driven probe)
            dev = ctx.outer_probe(o, lam, pt["R"], pt["s"], v=case["v"], Hv=case["Hv"], model_recurrence=rec, retraction=retr,
                                  step=_step_inputs(case, parts, xmamd.PH_TCG, slot))
            assert dev["grid"] == nB and dev["nwave"] == (n + 63) // 64, label
            if cid == "step-bsr-n65600":
                assert dev["grid"] == 1024 and dev["nwave"] > 1024, (label, dev["grid"], dev["nwave"])
            for k in ("HpR", "Hps", "pHp", "rHp", "HpHp"):                         # the same launches gave both their inputs
                assert _same(dev[k], host[k]), (label, k)
            X = case["expect"]
            so, oo = dev["scal_out"], dev["os_out"]
            assert (so["status"], so["iter"], so["seq"]) == (X["scal"]["status"], X["scal"]["iter"], 11), (label, so)
            assert oo == dict(loss=1.5, rr_point=case["sc"]["rr"], totalite=17, shrink_count=2, k=5, stop_reason=0, time_up=0, slots=24), (label, oo)
            assert dev["trace"] is None and _same(dev["out_R"], pt["R"]) and _same(dev["out_s"], s1), label
            given = dict(vR=case["v"][0], vs=case["v"][1], HvR=case["Hv"][0], Hvs=case["Hv"][1], rR=case["r"][0], rs=case["r"][1], pR=pt["p"][0], ps=pt["p"][1])
            if name in rs.STEP_CG:
                assert so["phase"] == xmamd.PH_TCG and dev["progress"] == xmamd.pack_prog(dev["run"], slot + 1, xmamd.PH_TCG), label
                for k in TCG_VECTORS + ("W",):
                    if not (rec and k in ("HvR", "Hvs")):
                        assert _same(dev["out_" + k], host["out_" + k]), (label, k)
                assert _same(dev["out_partsB"], host["partsB_out"]), label
                for k in SCAL_FIELDS:
                    assert so[k] == host["scal_out"][k], (label, k, so[k], host["scal_out"][k])
                assert _same(dev["out_Rc"], pt["R"]) and _same(dev["out_sc"], s1) and dev["out_pad"][1] == 0, label    # no candidate yet
                as_host = dict(dev, scal_out={k: so[k] for k in SCAL_FIELDS}, partsB_out=dev["out_partsB"], rr_parts=host["rr_parts"])
                base._cg_compare(label, as_host, case, parts, bad)
                continue
            assert so["phase"] == xmamd.PH_CAND and dev["progress"] == xmamd.pack_prog(dev["run"], slot + 1, xmamd.PH_CAND), label
            for k in TCG_VECTORS:                                                  # not written back: nothing reads them before the next start
                if not (rec and k in ("HvR", "Hvs")):
                    assert _same(dev["out_" + k], given[k]), (label, k)
            assert not dev["out_partsB"].any() and dev["out_pad"] == (0, 0), (label, dev["out_pad"])
            # the host-driven pair on the same inputs: cg_step_kernel's v and H v, then the retraction with the model decrease
            vh = (host["out_vR"], host["out_vs"])
            Hvh = None if rec else (host["out_HvR"], host["out_Hvs"])
            pair = ctx.outer_probe(o, lam, pt["R"], pt["s"], v=vh, Hv=Hvh, retract=True, model_recurrence=rec, retraction=retr, auto=True,
                                   model=host["scal_out"]["model"])
            for k in ("Rc", "sc", "W"):
                assert _same(dev["out_" + k], pair["ret_" + k]), (label, k)
            if not rec:
                assert _same(rs.regroup4(dev["out_partsM"]), pair["ret_partsM"]), label
            # and the longdouble chain: the tCG body, the retraction of its step, the model decrease
            polar = retr == "polar"
            E, F = (_chain(case, dev, parts, dt) for dt in (LD, np.float64))
            assert E["branch"] == X["branch"], label
            Er, Fr = (ex.retract_stage(pt["R"], pt["s"], A["vR"].reshape(3 * n, -1), A["vs"], 1.0, polar, dt) for A, dt in ((E, LD), (F, np.float64)))
            _retraction(label, n, o, dev["out_Rc"], dev["out_sc"], dev["out_W"], Er, Fr, bad)
            for k in ("last_step", "model"):
                _one(label, "scal." + k, so[k], E["scal"][k], F["scal"][k], E.get(k + "~"), bad)
            if not rec:
                Em, Fm = (ex.model_stage((A["vR"].reshape(3 * n, -1), A["vs"]), (A["HvR"].reshape(3 * n, -1), A["Hvs"]), (dev["rgR"], dev["rgs"]), s1, dt)
                          for A, dt in ((E, LD), (F, np.float64)))
                _one(label, "partsM", dev["out_partsM"].astype(LD).sum(), Em["m"], Fm["m"], Em["m~"], bad)
    for ctx in ctxs.values():
        ctx.close()
    assert not bad, bad


def _check_decision(xmamd, label, got, exp, sc_in, os_in, slot):
    so, oo = got["scal_out"], got["os_out"]
    for k in ("rr", "pp", "delta", "gradnorm", "vv", "vp", "last_step", "model", "status", "iter", "seq", "phase"):
        assert so[k] == exp[k], (label, "scal." + k, so[k], exp[k])
    for k in ("loss", "rr_point", "totalite", "shrink_count", "k", "stop_reason", "time_up", "slots"):
        assert oo[k] == exp[k], (label, "os." + k, oo[k], exp[k])
    assert (got["trace"] is None) == (exp["trace"] is None), (label, got["trace"], exp["trace"])
    if exp["trace"] is not None:
        assert tuple(got["trace"]) == exp["trace"], (label, got["trace"], exp["trace"])
    assert got["progress"] == xmamd.pack_prog(got["run"], slot + 1, exp["phase"]), label


@pytest.mark.parametrize("cid", [c["id"] for c in rs.DECIDE_CONTEXTS])
def test_step_launch_in_the_decision_role(xmamd, cid):
    """outer_step_kernel with phase = PH_CAND, PH_INIT and PH_STOP.  The candidate is the retraction of a real tCG step (the boundary case of the
    tCG roles) with the per-wavefront model partials of that launch; a first call gives the kernel's own f, <rg,rg> and m, and the loss is placed
    for a target rho.  Everything the launch decides is exactly ex.outer_decide_stage on those three sums; the point's buffers hold the
    candidate's bits after an accept and the current point's after a reject; a start of the next tCG is tcg_init_kernel's bit for bit."""
    c = next(x for x in rs.DECIDE_CONTEXTS if x["id"] == cid)
    o, mk = c["o"], c["mk"]
    ctx = base._ctx(xmamd, mk, c["tuning"])
    case = rs.cg_case(mk, o, "boundary")
    pt, lam, n = case["pt"], case["lam"], case["pt"]["s"].size
    s1 = pt["s"].copy(); s1[0] = 1.0
    retr = "polar" if o == 4 else "mgs"
    nB = ctx.rtr_probe(o, lam, pt["R"], pt["s"], auto=True)["nB"]
    kw, parts = rs.cg_inputs(case, nB)
    end = ctx.outer_probe(o, lam, pt["R"], pt["s"], v=case["v"], Hv=case["Hv"], retraction=retr, step=_step_inputs(case, parts, xmamd.PH_TCG, 0))
    assert end["scal_out"]["phase"] == xmamd.PH_CAND
    cand, w = (end["out_Rc"], end["out_sc"]), end["out_partsM"]
    if w.astype(LD).sum() > 0:                             # (v and H v of the case are not a tCG's history: the sign of their model value is anybody's)
        w = -w
    cur = ctx.rtr_probe(o, lam, pt["R"], pt["s"], auto=True, tcg_init=True, delta=2.0)             # the current point's state and tcg_init_kernel from it
    nxt = ctx.rtr_probe(o, lam, cand[0], cand[1], auto=True, tcg_init=True, delta=2.0)             # the same at the candidate
    given = dict(vR=case["v"][0], vs=case["v"][1], HvR=case["Hv"][0], Hvs=case["Hv"][1], rR=case["r"][0], rs=case["r"][1], pR=pt["p"][0], ps=pt["p"][1])
    slot, bad = 7, []                                      # (odd: the sweep direction of the symmetric product in the probes compared with)

    def call(sc, os_, b, partsM):
        step = dict(scal=sc, os=os_, delta_bar=b["delta_bar"], gradtol=b["gradtol"], max_outer=b["max_outer"], stop_req=b["stop_req"], slot=slot,
                    p=pt["p"], r=case["r"], cand=cand, partsM=partsM)
        return ctx.outer_probe(o, lam, pt["R"], pt["s"], v=case["v"], Hv=case["Hv"], retraction=retr, step=step)

    def state(got, label, accept, start):
        src, pnt = (nxt, cand) if accept else (cur, (pt["R"], s1))
        assert _same(got["out_R"], pnt[0]) and _same(got["out_s"], pnt[1]), (label, "point")
        for k in ("G", "egs", "S0", "rgR", "rgs"):
            assert _same(got["out_" + k], src[k]), (label, k)
            if accept:
                assert _same(got["out_" + k], got["cand_" + k]), (label, "cand_" + k)
        assert _same(got["out_Rc"], cand[0]) and _same(got["out_sc"], cand[1]), (label, "candidate")
        for k in TCG_VECTORS + ("W",):
            if start:
                assert _same(got["out_" + k], src["init_" + k]), (label, "start", k)
            elif k != "W":
                assert _same(got["out_" + k], given[k]), (label, "left alone", k)

    base_b = rs.decide_branches()[0]
    sc0 = dict(rr=1.0, vv=0.5, vp=0.1, pp=2.0, delta=2.0, gradnorm=1.0, last_step=0.3, model=-0.1, status=2, iter=4, seq=5, phase=xmamd.PH_CAND)
    os0 = dict(loss=0.0, rr_point=4.0, totalite=11, shrink_count=0, k=3, stop_reason=0, time_up=0, slots=9)
    first = call(sc0, os0, base_b, w)
    f, rr_new, m = first["f_cand"], first["rr_cand"], first["m_cand"]
    # the three sums: f and <rg,rg> against the longdouble gradient stage at the candidate, m against the longdouble sum of the partials
    M = rs.matrix(*mk)
    op64 = ex.Op(M["Q"]) if M["Q"] is not None else M["op"]
    Eg, Fg = ex.grad_stage(M["op"], cand[0], cand[1], lam, LD), ex.grad_stage(op64, cand[0], cand[1], lam, np.float64)
    for k, x in (("f", f), ("rr", rr_new)):
        _one(f"{cid}-sums", k, x, Eg[k], Fg[k], Eg[k + "~"], bad)
    _one(f"{cid}-sums", "m", m, w.astype(LD).sum(), w.sum(), np.abs(w).astype(LD).sum(), bad)
    assert m < 0, (cid, m)
    if w.size <= 8:                                        # at most two groups of four: their sum has one order only
        assert m == rs.regroup4(w).sum(), (cid, m)
    for b in rs.decide_branches():
        label = f"{cid}-{b['name']}"
        wb = -w if b["rho"] is None else w
        mb = -m if b["rho"] is None else m
        sc = dict(sc0, delta=b["delta"], status=b["status"], iter=b["iter"])
        os_ = dict(os0, loss=f + 1.0 if b["rho"] is None else f - b["rho"] * m, shrink_count=b["shrink"], k=b["k"], time_up=b["time_up"])
        got = call(sc, os_, b, wb)
        assert (got["f_cand"], got["rr_cand"], got["m_cand"]) == (f, rr_new, mb), label
        exp = ex.outer_decide_stage(sc, os_, f, rr_new, mb, b["delta_bar"], b["gradtol"], b["max_outer"] or 1000, b["stop_req"])
        for k, val in b["expect"].items():
            assert exp[k] == val, (label, k, exp[k], val)
        _check_decision(xmamd, label, got, exp, sc, os_, slot)
        state(got, label, exp["accept"], exp["start"])
    # PH_INIT: the first launch of a run starts the first tCG from the state the host uploaded and decides nothing
    sc = dict(sc0, phase=xmamd.PH_INIT, delta=2.5, status=0, iter=0)
    os_ = dict(os0, loss=cur["f"], rr_point=cur["rr"])
    got = call(sc, os_, base_b, w)
    exp = ex.outer_decide_stage(sc, os_, 0, 0, 0, base_b["delta_bar"], base_b["gradtol"], 1000, 0)
    assert exp["phase"] == xmamd.PH_TCG and exp["trace"] is None and exp["slots"] == 9
    _check_decision(xmamd, f"{cid}-init", got, exp, sc, os_, slot)
    for k in ("G", "egs", "S0", "rgR", "rgs"):
        assert _same(got["out_" + k], cur[k]), k
    assert _same(got["out_R"], pt["R"]) and _same(got["out_s"], s1) and _same(got["out_Rc"], cand[0]) and _same(got["out_sc"], cand[1])
    for k in TCG_VECTORS + ("W",):
        assert _same(got["out_" + k], cur["init_" + k]), ("init", k)
    # PH_STOP: both scalar blocks pass through, nothing else is written, no progress is published
    sc = dict(sc0, phase=xmamd.PH_STOP)
    os_ = dict(os0, loss=3.5, stop_reason=10)
    got = call(sc, os_, base_b, w)
    assert got["scal_out"] == sc and got["os_out"] == os_ and got["progress"] == 0 and got["trace"] is None
    for k in TCG_VECTORS:
        assert _same(got["out_" + k], given[k]), ("stop", k)
    for k in ("G", "egs", "S0", "rgR", "rgs"):
        assert _same(got["out_" + k], cur[k]), ("stop", k)
    assert _same(got["out_R"], pt["R"]) and _same(got["out_s"], s1) and _same(got["out_Rc"], cand[0]) and _same(got["out_sc"], cand[1])
    assert _same(got["out_partsM"], w) and not got["out_partsB"].any()
    ctx.close()
    assert not bad, bad


@pytest.mark.parametrize("pid", ["dense-n43", "bsr-n200"])
def test_solve_after_a_probe_gives_the_same_bits(xmamd, pid):
    path = base.BY_ID[pid]
    a, b = base._ctx(xmamd, path["mk"], path["tuning"]), base._ctx(xmamd, path["mk"], path["tuning"])
    mk = path["mk"]
    case = rs.cg_case(mk, 3, "boundary")
    rc = rs.retract_case(("dense", 43, 0), 4) if pid == "dense-n43" else None
    pt, lam = case["pt"], case["lam"]
    flags = xmamd.FLAG_DEVICE_OUTER if pid == "dense-n43" else 0

    def probes():
        if rc is not None:
            a.outer_probe(4, rc["lam"], rc["pt"]["R"], rc["pt"]["s"], v=rc["v"], Hv=rc["Hv"], retract=True, retraction="polar", ls=(rc["D"], rs.LS_T))
        nB = a.rtr_probe(3, lam, pt["R"], pt["s"], auto=True)["nB"]
        end = a.outer_probe(3, lam, pt["R"], pt["s"], v=case["v"], Hv=case["Hv"], step=_step_inputs(case, rs.cg_inputs(case, nB)[1], xmamd.PH_TCG, 0))
        step = dict(_step_inputs(case, None, xmamd.PH_CAND, 1), cand=(end["out_Rc"], end["out_sc"]), partsM=end["out_partsM"])
        a.outer_probe(3, lam, pt["R"], pt["s"], v=case["v"], Hv=case["Hv"], step=step)

    probes()
    ra, rb = base._solve_bits(a, flags), base._solve_bits(b, flags)
    assert ra == rb and ra[4] == 1
    probes()                                               # between two solves as well
    assert base._solve_bits(a, flags) == base._solve_bits(b, flags)
    assert base._solve_bits(a) == base._solve_bits(b)      # and the host-driven form of dense storage
    a.close(); b.close()


def _raw(xmamd, ctx, n, o=3, flags=1, struct_size=None, nan=None):
    q = xmamd.OuterProbe()
    q.struct_size = C.sizeof(q) if struct_size is None else struct_size
    q.o, q.lam, q.flags, q.t = o, 1.0, flags, 0.5
    oo = max(o, 3)
    zm, zv = (lambda: np.zeros((3 * n, oo), order="F")), (lambda: np.zeros(n))
    keep = dict(R=np.asfortranarray(np.tile(np.eye(3, oo), (n, 1))), s=np.ones(n), vR=zm(), vs=zv(), HvR=zm(), Hvs=zv(), D=zm(), pR=zm(), ps=zv(), rR=zm(), rs=zv())
    if nan:
        keep[nan][-1, ...] = np.nan
    for k, a in keep.items():
        setattr(q, k, a.ctypes.data_as(C.c_void_p))
    q.scal_in.rr, q.scal_in.pp, q.scal_in.delta, q.scal_in.phase = 1.0, 1.0, 1.0, xmamd.PH_INIT
    q.delta_bar = 10.0
    return xmamd.lib().xm_ctx_outer_probe(ctx.h, C.byref(q)), q


def test_refusals_leave_contexts_usable(xmamd):
    ERR_ARG = -2
    err = lambda: xmamd.lib().xm_last_error().decode()
    RET, LS, STEP = xmamd.OUTER_PROBE_RETRACT, xmamd.OUTER_PROBE_RETRACT_LS, xmamd.OUTER_PROBE_STEP
    V = tl.gen_vg(40, deg=6, sigma=0.05, seed=80)
    two = xmamd.Context(Q=V["Q"], n_gpus=2, gpu_map=1)
    assert _raw(xmamd, two, 40)[0] == ERR_ARG and "single" in err()
    two.close()
    S = rs.matrix("scene", 40, 60)
    dense, sell = xmamd.Context(Q=V["Q"], tuning=dict(sym=-1)), xmamd.Context(bsr=(V["rowptr"], V["colidx"], V["blocks"]), tuning=dict(sell=1))
    free = xmamd.Context(**S["ctx"], tuning=dict(schur_solver=1))
    assert _raw(xmamd, dense, 40, flags=RET | LS | STEP)[0] == 0
    for kw in (dict(o=0), dict(o=2), dict(o=11), dict(struct_size=8), dict(nan="R"), dict(nan="s"), dict(nan="vR"), dict(nan="D", flags=LS), dict(flags=1024),
               dict(flags=RET | xmamd.OUTER_PROBE_POLAR | xmamd.OUTER_PROBE_MGS), dict(nan="pR", flags=STEP)):
        assert _raw(xmamd, dense, 40, **kw)[0] == ERR_ARG, kw
        assert "xm_ctx_outer_probe" in err(), (kw, err())
    # the step launch where the device-driven outer iteration does not apply: sliced ELL and matrix-free storage (their retraction stages run)
    for c in (sell, free):
        assert _raw(xmamd, c, 40, flags=STEP)[0] == ERR_ARG and "XM_OUTER_PROBE_STEP" in err()
        assert _raw(xmamd, c, 40, flags=xmamd.OUTER_PROBE_AUTO)[0] == ERR_ARG
        assert _raw(xmamd, c, 40, flags=RET | LS)[0] == 0
    for c in (dense, sell, free):                          # usable afterwards
        _, _, info = c.solve(4, 1e-8, 0.0)
        assert info["status"] == 1
        c.close()
