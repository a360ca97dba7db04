"""GPU tests of the certificate's Lanczos eigen-solver through the test export xm_ctx_cert_probe: Context::lanczos_min itself at fixed points, with
what its last restart cycle left on the device compared with the longdouble reference xm_rtr_exact.lanczos_stage (cases and comparison:
xm_cert_stages.py; test_rtr_exact.py holds the reference against first principles and shows that every planted fault breaks this comparison).

Bound: e_gpu <= max(16 e_ref, 64 eps_f64) per quantity and case.  Every step is compared from the GPU's own basis V[:, 0..j] (alpha_j, beta_j, the
coefficients c1 / c2 of the last step against the magnitude of the dots' terms; beta_j v_{j+1} per camera against the magnitude of the terms of
S v_j); orthogonality, the Ritz vector, x^T S x and the residual against the same figures of the reference's f64 whole run.  Every comparison
prints `STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s); profiles/r18_cert_stage_errors.txt condenses a run.

Which kernel an output pins: alpha, beta, c1, c2, w -> the O = 1 EPI_CERT product, dots_multi_seg_kernel (dots_multi_kernel and
dots_multi_fin_kernel in the un-fused form), sub_vc_fin_kernel / sub_vc_kernel, lz_next_fin_kernel / lz_next_kernel, lz_alpha_kernel; x ->
gemv_n_kernel; theta, y, resid, ret, eig_exact -> the host's tridiag_min and the stop rules."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_rtr_stages as base
import xm_ba_stages as st
import xm_cert_stages as cs
import xm_rtr_exact as ex
import xm_rtr_stages as rs

pytestmark = pytest.mark.gpu

LD = ex.LD
FUSED_KEYS = ("alpha", "beta", "V", "c1", "c2", "x", "y")


def _probe(ctx, case, S, **kw):
    return ctx.cert_probe(S["o"], S["lam"], S["R"], S["s"], mmax=case["tuning"].get("lanczos_mmax"), **kw)


@pytest.mark.parametrize("cid", cs.CASE_IDS)
def test_lanczos_run_against_the_longdouble_reference(xmamd, cid):
    case, S = cs.BY_ID[cid], cs.setup(cid)
    n = S["n"]
    ctx = xmamd.Context(**S["M"]["ctx"], tuning=case["tuning"])
    got = _probe(ctx, case, S)
    twin = _probe(ctx, case, S, unfused=True) if case.get("unfused") else None
    ctx.close()
    m, k = got["m_use"], got["steps_dev"]
    assert got["product_kind"] == case["kind"] and got["nseg"] == case["nseg"] == ex.dots_segments(got["len"])[0], (got["product_kind"], got["nseg"], got["len"])
    assert got["len"] >= 3 * n and got["len"] % 128 == 0
    for key, v in case.get("expect", {}).items():
        assert got[key] == v, (key, got[key], v)
    assert 1 <= m <= k <= got["mmax"] and got["steps_fused"] + got["steps_unfused"] == got["iters"] == (got["cycles"] - 1) * got["mmax"] + k
    # the multipliers, as the trust region's probe compares them
    E = dict(S["C"]); F = S["C64"]
    keys = ("Lam", "dz", "dual0", "dual1")
    bad = rs.compare(cid, dict(Lam=got["Lam"], dz=got["dz"], dual0=got["dual"][0], dual1=got["dual"][1]), E, {q: rs.error(F[q], E, q)[0] for q in keys}, keys)
    # the start vector, bit for bit; after restarts the last cycle's start: the normalised Ritz vector of the cycle before
    if got["cycles"] == 1:
        assert np.array_equal(got["V"][:, 0], ex.lanczos_start(n))
    else:
        v0 = got["V"][:, 0].astype(LD)
        assert abs(float(np.sqrt(v0 @ v0)) - 1.0) <= 4 * st.EPS
    if case.get("restarts"):
        assert got["cycles"] > 1
    bad += cs.compare_run(cid, S, got, case)
    # the stop rules on the GPU's own numbers
    tmax = float(ex.tridiag_bounds(got["alpha"][:m], np.append(got["beta"][:m - 1], 0.0))[2])
    unit = max(1.0, tmax)
    assert abs(got["resid"] - abs(got["beta"][m - 1] * got["y"][m - 1])) <= 2 * st.EPS * got["resid"]
    assert got["ret"] == int(got["resid"] > 1e-6 * unit)
    exact = 3 * n <= (case["tuning"].get("cert_dense_rows", 0) or 384) and 3 * n <= got["mmax"]
    exhausted = m == 3 * n or got["beta"][m - 1] < 1e-13 * unit
    assert got["eig_exact"] == int(exact and exhausted)
    if m < got["mmax"]:
        assert exhausted or (not exact and got["resid"] <= 1e-9 * unit)
    if case.get("eig"):
        ev = np.linalg.eigvalsh(cs.dense_S(S))
        slack = 8e-16 * unit + 64 * st.EPS * max(np.abs(ev).max(), 1.0)
        print(f"STAGE_CONS {cid} theta - eig_min: {got['theta'] - ev[0]:.3e}")
        assert got["theta"] >= ev[0] - slack               # a Ritz value is an upper bound
        if got["ret"] == 0:
            assert got["theta"] - ev[0] <= got["resid"] + slack, (got["theta"], ev[0], got["resid"])
    if case.get("exhaust"):
        Sx = cs.dense_S(S, LD) @ got["x"].astype(LD)
        print(f"STAGE_CONS {cid} |S x|: {float(np.sqrt(Sx @ Sx)):.3e}")
        # |S x| <= |S x - theta x| + |theta|: the reported residual (at exhaustion under the solver's own threshold) and round-off of the n terms of a row
        assert abs(got["theta"]) <= 64 * st.EPS * n and got["resid"] <= 1e-13 * unit
        assert float(np.sqrt(Sx @ Sx)) <= got["resid"] + 128 * st.EPS * n
    if case.get("relation"):
        e, e_ref = cs.relation_error(S, got), cs.relation_error(S, cs.as_run(S["F"]))
        print(f"STAGE_ERR {cid} relation: e_ref {e_ref:.3e}, e_gpu {e:.3e}, ratio {e / st.bound(e_ref):.3f}")
        if not e <= st.bound(e_ref):
            bad.append(f"{cid} relation: {e:.3e} > {st.bound(e_ref):.3e}")
    if twin is not None:                                   # the un-fused form of a step gives the fused form's bits
        assert twin["steps_fused"] == 0 and twin["steps_unfused"] == twin["iters"] == got["iters"] and got["steps_unfused"] == 0
        for key in FUSED_KEYS + ("theta", "resid", "ret", "m_use"):
            assert np.array_equal(np.asarray(twin[key]), np.asarray(got[key])), key
    assert not bad, bad


def test_solve_after_a_probe_gives_the_same_bits(xmamd):
    case, S = cs.BY_ID["single-n43"], cs.setup("single-n43")
    a, b = (xmamd.Context(**S["M"]["ctx"], tuning=case["tuning"]) for _ in range(2))
    _probe(a, case, S)
    _probe(a, case, S, unfused=True)
    ra, rb = base._solve_bits(a), base._solve_bits(b)
    assert ra == rb and ra[4] == 1
    _probe(a, case, S, unfused=True)                       # between two solves as well; the flag does not outlive the call
    assert base._solve_bits(a) == base._solve_bits(b)
    a.close(); b.close()


def _raw(xmamd, ctx, n, o=3, flags=0, struct_size=None, nan=None, lam=1.0, alpha=None):
    q = xmamd.CertProbe()
    q.struct_size = C.sizeof(q) if struct_size is None else struct_size
    q.o, q.lam, q.flags = o, lam, flags
    keep = dict(R=np.asfortranarray(np.tile(np.eye(3, max(o, 3)), (n, 1))), s=np.ones(n))
    if nan:
        keep[nan][-1, ...] = np.nan
    if alpha is not None:
        keep["alpha"], q.cap = alpha, alpha.size
    for key, a in keep.items():
        setattr(q, key, a.ctypes.data_as(C.c_void_p))
    return xmamd.lib().xm_ctx_cert_probe(ctx.h, C.byref(q)), q


def test_refusals_leave_the_context_usable(xmamd):
    ERR_ARG = -2
    err = lambda: xmamd.lib().xm_last_error().decode()
    Q = rs.matrix("dense", 43, 0)["Q"]
    two = xmamd.Context(Q=Q, n_gpus=2, gpu_map=1)
    assert _raw(xmamd, two, 43)[0] == ERR_ARG and "single" in err()
    two.close()
    ctx = xmamd.Context(Q=Q, tuning=dict(sym=-1))
    rc, q = _raw(xmamd, ctx, 43)                           # no output array at all: the scalars alone
    assert rc == 0 and q.m_use == 129 and q.eig_exact == 1 and q.nseg == 1
    small = np.zeros(4)
    rc, q = _raw(xmamd, ctx, 43, alpha=small)               # an array too short for a cycle: refused before anything is written to it
    assert rc == ERR_ARG and "cap" in err() and q.mmax == 129 and not small.any()
    for kw in (dict(o=2), dict(o=11), dict(struct_size=8), dict(nan="R"), dict(nan="s"), dict(flags=2), dict(lam=float("inf"))):
        assert _raw(xmamd, ctx, 43, **kw)[0] == ERR_ARG, kw
        assert "xm_ctx_cert_probe" in err(), (kw, err())
    _, _, info = ctx.solve(4, 1e-8, 0.0)
    assert info["status"] == 1
    ctx.close()
