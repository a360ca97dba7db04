"""GPU tests of the matrix-free Q stage by stage (xm-code_amd/csrc/xm_schur.hip) through the test export xm_ctx_schur_probe: the layout of the
packed landmark lists, the set-up factors, every stage of one product's factor chain (through SchurOp::product itself) and the pieces of the
inner CG (through the members pcg_solve calls), each against the longdouble reference xm_schur_exact.py.

Bound (xm_schur_stages.py): per quantity and case e_gpu <= max(16 e_ref, 64 eps_f64), errors per landmark row / camera row / camera block /
aggregate block, e_ref the f64 numpy restatement's own error (the larger of two observation orders); for xc of the CG forms the restatement
is a numpy PCG with the same preconditioner, the same per-column stop rule and the same cap, so e_ref is the error the stop rule leaves.
Nothing is derived from the GPU's output.  Every comparison prints a STAGE_ERR line (profiles/r19_schur_stage_errors.txt).

Found on the MI355X (profiles/r19_schur_stage_errors.txt): all 1136 comparisons inside the bound, the worst MX of the two-level form at 0.35 of
it; the CG forms stop after the restatement's iteration count (agg129: 11 against 10) with xc at 0.06 of its bound, so 16 x was room enough
for a one-iteration difference.  One quantity needed the denominator's floor the cancelling sums have (xm_schur_stages.py): ainv = (P^T VT P)^-1.
A_c is what is left of an aggregate's sum of Q2 (1 300 on agg64) once the landmarks inside it are taken off (10), tl_coarse_entries_kernel takes
them off one by one in a running sum of that size, and a normwise error of ainv (2.7e-13 on agg64, 17 .. 33 e_ref on base and agg*) measures
that cancellation, not a defect: the floor |ainv| T |ainv| (T: the magnitude of A_c's terms, xm_schur_exact.py) puts it at 0.04 of the bound
while an aggregate's padding rows counted in A_c still miss it by orders of magnitude (test_schur_exact.py).

The kernels are instantiated for o = 1 and 3..10: o = 2 is refused by the probe as it is by every product (asserted below)."""
import ctypes as C

import numpy as np
import pytest

import xm_schur_stages as ss

pytestmark = pytest.mark.gpu
ERR_ARG = -2


def _ctx(xmamd, case, form, w=None):
    S = ss.scene(case)
    return xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"] if w is None else w), n=S["n"], tuning=dict(ss.FORMS[form][0]))


def _probe(ctx, case, o, pieces=True):
    W, alpha, X = ss.inputs(case, o)
    cg = ctx.schur_info()["cg"]
    g = ctx.schur_probe(W=W, alpha=alpha, X=X if (cg and pieces) else None, dense=not cg)
    S = ss.scene(case)
    return g, ss.shape_probe(g, S["n"], S["m"])


def _perm_of(xmamd, g, case):
    """the probe's table of aggregates, checked against the library's host plan: the same members, every reduced camera once"""
    S = ss.scene(case)
    perm = np.asarray(g["perm"])
    plan = xmamd.schur_aggregate_plan(S["cam"], S["lm"], S["n"])
    for a in range(perm.shape[0]):
        mem = perm[a][perm[a] >= 0]
        assert sorted(mem + 1) == list(np.nonzero(plan == a)[0]), a
        assert np.all(perm[a][:mem.size] >= 0)               # members first, padding behind them
    assert np.sort(perm[perm >= 0]).tolist() == list(range(S["n"] - 1))
    return perm


def _check_layout(g, case, form):
    S = ss.scene(case)
    kind = ss.FORMS[form][1]
    deg = np.bincount(S["lm"], minlength=S["m"])
    assert np.array_equal(g["deg"], deg)
    assert g["nheavy"] == int((deg > 64).sum())
    assert bool(g["uses_cg"]) == (kind != "dense") and bool(g["two_level"]) == (kind == "two_level")
    named_twice = np.unique(S["cam"].astype(np.int64) * S["m"] + S["lm"]).size < S["cam"].size
    assert bool(g["dup_pairs"]) == (kind == "dense" and (named_twice or form == "host"))
    # the packed lists: heavy landmarks contiguous, light ones 64 to a group, each group padded to its first (longest) slot
    light = np.sort(deg[deg <= 64])[::-1]
    assert g["lm_total"] == max(1, int(deg[deg > 64].sum()) + 64 * int(light[::64].sum()))
    if kind == "two_level" and S["n"] > 1:
        assert g["nagg"] == -(-(S["n"] - 1) // 64)


def _check_state(g, label):
    print(f"PCG_STATE {label}: done {g['pcg_done']} iters {g['pcg_iters']} relres {g['pcg_relres']:.3e} tol {g['pcg_tol']:.1e} cap {g['pcg_cap']}")
    assert g["pcg_done"] == 1 and g["pcg_iters"] <= g["pcg_cap"] == ss.PCG_CAP and g["pcg_relres"] <= g["pcg_tol"] == ss.PCG_TOL


def _run(xmamd, case, form):
    S = ss.scene(case)
    kind = ss.FORMS[form][1]
    n1 = S["n"] - 1
    ctx = _ctx(xmamd, case, form)
    bad = []
    try:
        for o in ss.o_of(case):
            g, got = _probe(ctx, case, o)
            _check_layout(g, case, form)
            perm = _perm_of(xmamd, g, case) if (kind == "two_level" and n1 > 0) else None
            E = ss.exact_all(case, kind, o, perm)
            e_ref = ss.reference_errors(case, kind, o, perm)
            assert max(e_ref[k] for k in ss.keys_of(kind, n1)) <= ss.MAX_E_REF
            if kind != "dense" and n1 > 0:
                _check_state(g, f"{case} {form} o{o}")
                print(f"PCG_ITERS {case} {form} o{o}: gpu {g['pcg_iters']} numpy {e_ref['pcg_iters']}")
            bad += [(o,) + b for b in ss.compare(f"{case} {form} o{o}", got, E, e_ref, ss.keys_of(kind, n1))]
            if kind != "dense" and n1 > 0:                   # the operator and the preconditioner are symmetric on the identity columns
                for key in ("VX", "MX"):
                    A = np.asarray(got[key])[[0, min(63, n1 - 1), n1 - 1, n1 // 2], :ss.NID]
                    asym = float(np.abs(A - A.T).max() / np.abs(A).max())
                    print(f"STAGE_SYM {case} {form} {key}: {asym:.3e} bound {ss.bound(e_ref[key]):.3e}")
                    assert asym <= ss.bound(e_ref[key]), (key, asym)
    finally:
        ctx.close()
    assert not bad, bad


CASE_FORMS = [(c, f) for c in ss.CASES for f in ss.forms_of(c)]


@pytest.mark.parametrize("case,form", CASE_FORMS, ids=[f"{c}-{f}" for c, f in CASE_FORMS])
def test_stages_match_the_longdouble_reference(xmamd, case, form):
    _run(xmamd, case, form)


def test_degree_scene_has_the_edges_it_is_for(xmamd):
    """the counts of the `degrees` case on the probe's own layout: six heavy landmarks (65, 66, 1023, 1024, 1025, 1030 observations),
    1024 + 64 + 1 light ones, every degree of xm_schur_stages.DEGREES at its landmark, with and without camera 0 as the scene says"""
    S = ss.scene("degrees")
    ctx = _ctx(xmamd, "degrees", "jacobi")
    try:
        g = ctx.schur_probe()
    finally:
        ctx.close()
    assert g["nheavy"] == 6 and S["m"] - g["nheavy"] == ss.DEGREES_LIGHT == 1089
    for d, l in S["roles"].items():
        assert g["deg"][l] == d
        if d >= 2:
            assert bool(np.any(S["cam"][S["lm"] == l] == 0)) == ss.WITH_CAMERA_0[d]
    fill = np.delete(g["deg"], list(S["roles"].values()))
    assert fill.min() == 2 and fill.max() == 9 and len(set(fill[:64])) > 1
    assert sorted(np.bincount(ss.scene("cam_degrees")["cam"])) == sorted(ss.CAM_COUNTS)


@pytest.mark.parametrize("form", tuple(ss.FORMS))
def test_zero_weight_landmarks_drop_out(xmamd, form):
    """a landmark whose weights are all 0: q3inv, h and xl are exactly 0 (the kernels set 1 / Q3 := 0)"""
    ctx = _ctx(xmamd, "masks", form)
    try:
        g, _ = _probe(ctx, "masks", 3, pieces=False)
    finally:
        ctx.close()
    for l in ss.MASK_ZERO_LANDMARKS:
        assert g["q3inv"][l] == 0.0 and not np.any(g["h"][l]) and not np.any(g["xl"][l])
    assert np.count_nonzero(g["q3inv"] == 0.0) == len(ss.MASK_ZERO_LANDMARKS)


BIT_KEYS = ("Q1", "c", "q2", "q3inv", "dinv", "VTinv", "binv", "ainv", "h", "r", "xc", "xl", "Y", "VX", "pAp", "MX")


def _same_bits(a, b, what):
    for k in BIT_KEYS:
        if k in a or k in b:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


@pytest.mark.parametrize("form", tuple(ss.FORMS))
def test_weights_handed_over_later_give_the_same_bits(xmamd, form):
    """created with unit weights and given the real ones through set_edge_weights: every factor and stage bit-equal to a context created
    with the real weights"""
    S = ss.scene("masks")
    a = _ctx(xmamd, "masks", form)
    b = _ctx(xmamd, "masks", form, w=S["w1"])
    try:
        b.set_edge_weights(S["w"])
        _same_bits(_probe(a, "masks", 4)[0], _probe(b, "masks", 4)[0], form)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("form", tuple(ss.FORMS))
def test_changing_o_on_one_context_gives_a_fresh_contexts_bits(xmamd, form):
    """the row pitch of r and xc changes with o and only those two vectors are cleared: the sequence o = 5, 3, 4, 3 on one context against a
    fresh context per o; and the probe leaves the context as it found it: products before and after it are bit-equal, the statistics of the CG
    form count the products alone"""
    fresh = {}
    for o in (3, 4, 5):
        c = _ctx(xmamd, "base", form)
        try:
            fresh[o] = _probe(c, "base", o)[0]
        finally:
            c.close()
    ctx = _ctx(xmamd, "base", form)
    try:
        W = ss.inputs("base", 4)[0]
        Y0, s0 = ctx.qw(W), ctx.schur_info()
        for o in (5, 3, 4, 3):
            _same_bits(_probe(ctx, "base", o)[0], fresh[o], (form, o))
        s1 = ctx.schur_info()
        assert np.array_equal(ctx.qw(W), Y0)
        assert (s1["products"], s1["inner_iters"], s1["capped"], s1["last_relres"]) == (s0["products"], s0["inner_iters"], s0["capped"], s0["last_relres"])
    finally:
        ctx.close()


def test_padding_rows_of_an_aggregate_stay_inside_it(xmamd):
    """agg65: the second aggregate has one member and 63 padding rows (perm = -1); its block inverse is 1 / VT_ii in the corner, the identity
    on the padding and 0 between them, and M^-1 X of a vector that is 0 on the member is what the coarse term alone gives"""
    ctx = _ctx(xmamd, "agg65", "two_level")
    try:
        g, _ = _probe(ctx, "agg65", 3)
    finally:
        ctx.close()
    perm, B = np.asarray(g["perm"]), np.asarray(g["binv"])[1]
    assert perm.shape == (2, 64) and np.all(perm[0] >= 0) and perm[1, 0] >= 0 and np.all(perm[1, 1:] == -1)
    assert np.array_equal(B[1:, 1:], np.eye(63)) and not np.any(B[0, 1:]) and not np.any(B[1:, 0])
    assert B[0, 0] == pytest.approx(float(g["dinv"][perm[1, 0]]), rel=1e-14)


def _raw(xmamd, ctx, **kw):
    q = xmamd.SchurProbe()
    q.struct_size = C.sizeof(xmamd.SchurProbe)
    keep = []
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            keep.append(v); v = v.ctypes.data_as(C.c_void_p)
        setattr(q, k, v)
    return xmamd.lib().xm_ctx_schur_probe(ctx.h, C.byref(q))


def test_refusals(xmamd):
    import xm_testlib as tl
    S = ss.scene("base")
    n = S["n"]
    err = lambda: xmamd.lib().xm_last_error().decode()
    W = np.zeros((3 * n, 3), order="F")
    d = xmamd.Context(Q=tl.gen_dense(8, seed=1)["Q"])
    try:
        assert _raw(xmamd, d) == ERR_ARG and "XM_STORAGE_SCHUR" in err()
    finally:
        d.close()
    ctx = _ctx(xmamd, "base", "dense")
    try:
        assert _raw(xmamd, ctx, struct_size=8) == ERR_ARG and "struct_size" in err()
        assert _raw(xmamd, ctx, flags=1) == ERR_ARG and "flag" in err()
        assert _raw(xmamd, ctx, o=2, W=np.zeros((3 * n, 2), order="F")) == ERR_ARG and "3..10" in err()
        assert _raw(xmamd, ctx, o=11, W=np.zeros((3 * n, 11), order="F")) == ERR_ARG
        assert _raw(xmamd, ctx, o=3) == ERR_ARG and "go together" in err()
        assert _raw(xmamd, ctx, o=3, W=np.full((3 * n, 3), np.nan, order="F")) == ERR_ARG and "finite" in err()
        assert _raw(xmamd, ctx, h=np.zeros(S["m"])) == ERR_ARG and "need W" in err()
        assert _raw(xmamd, ctx, dinv=np.zeros(n)) == ERR_ARG and "CG form" in err()
        assert _raw(xmamd, ctx, k=3, X=np.zeros((n - 1, 3), order="F")) == ERR_ARG and "CG form" in err()
        assert _raw(xmamd, ctx, perm=np.zeros(64, dtype=np.int32)) == ERR_ARG and "two-level" in err()
        with pytest.raises(xmamd.XmError, match="3..10"):
            ctx.qw(np.zeros((3 * n, 2)))                   # the product's own refusal of o = 2
        assert _raw(xmamd, ctx, o=3, W=W) == 0             # and the context is still usable
    finally:
        ctx.close()
    cg = _ctx(xmamd, "base", "jacobi")
    try:
        assert _raw(xmamd, cg, VTinv=np.zeros((n - 1) ** 2)) == ERR_ARG and "VTinv" in err()
        assert _raw(xmamd, cg, binv=np.zeros(64 * 64)) == ERR_ARG and "two-level" in err()
    finally:
        cg.close()
    two = xmamd.Context(obs=ss.obs(S), n=n, n_gpus=2, gpu_map=1, tuning=dict(schur_solver=1))   # a row-partitioned context
    try:
        assert _raw(xmamd, two) == ERR_ARG and "single" in err()
    finally:
        two.close()
    import xm_seqscene as sq
    B = sq.gen_sequential(xmamd.SCHUR_PROBE_DENSE_MAX_ROWS + 2, per_cam=3, seed=9)   # VTinv above its row cap
    big = xmamd.Context(obs=ss.obs(B), n=B["n"], tuning=dict(schur_solver=1))
    try:
        assert _raw(xmamd, big, VTinv=np.zeros(1)) == ERR_ARG and "XM_SCHUR_PROBE_DENSE_MAX_ROWS" in err()
        with pytest.raises(xmamd.XmError, match="SCHUR_PROBE_DENSE_MAX_ROWS"):
            big.schur_probe(dense=True)
    finally:
        big.close()
