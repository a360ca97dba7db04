"""GPU tests of the bundle adjustment's kernels with a focal and a distortion column (CD = 8, and 5 with fixed rotations;
xm-code_amd/csrc/xm_ba.hip) stage by stage through the test export xm_ctx_ba_probe_radial (Context.ba_probe_radial): one linearisation at
a fixed point, fixed focal scales and radial coefficients and a fixed mu, no LM loop, every array compared elementwise with the longdouble
reference xm_ba_radial_exact.py.

Bound (xm_ba_stages.py): e_gpu <= max(16 e_ref, 64 eps_f64) with e_ref the f64 restatement's own error against the same reference at the
same point, evaluated here per quantity and case (the larger of two observation orders).  Nothing is derived from the GPU's output.  The
cases are those of test_ba_radial_numpy.py::test_restatement_agrees_with_longdouble (which asserts e_ref <= 1e-8 for each): the focal
stage cases with k in [-0.15, 0.15] of both signs, and k_zero, mask_mix and on_axis (xm_ba_radial_stages.py).
Every comparison prints a line `STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s): the table of
profiles/r42_ba_radial_stage_errors.txt.

Which kernel an output pins: cost, n_used -> ba_eval, ba_reduce; g_l, vinv, lused -> ba_lm; b, ustar, sinv, cused -> ba_cam; gmax -> both;
SX -> ba_lmx, ba_camx; S -> ba_schur_dense; MX_jacobi -> ba_pcg_init; dP -> ba_lmx (sign -1, with g_l); rot1, t1, focal1, dist1, step2[0],
x2[0] -> ba_cand_cam; p1, step2[1], x2[1] -> ba_cand_vec; cost1, model -> ba_cost, all at CD = 8 / 5."""
import numpy as np
import pytest

import xm_ba_radial_stages as rs
import xm_ba_stages as st

pytestmark = pytest.mark.gpu

FIX = pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])


def _ctx(xmamd, S, **kw):
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S.get("w0", S["w"])), n=S["n"], **kw)
    if "w0" in S:
        ctx.set_edge_weights(S["w"])
    return ctx


def _probe(ctx, c, mu, dc=None):
    rot, t, P = c["point"]
    g = ctx.ba_probe_radial(rot, t, P, mu, focal=c["focal"], focal_free=c["free"], distortion=c["dist"], distortion_free=c["kfree"],
                            fix_rotations=c["fix"], loss=c["loss"], loss_scale=c["a"], X=c["X"], dc=c["dc"] if dc is None else dc, dense=True)
    g["S"], g["MX_jacobi"] = g["Sdense"], g["MX"]
    return g


def _zero_row_and_column(got, still, col, cd, mu):
    """the rows and columns `col` of the cameras `still`: zero off the diagonal in U* and in the assembled S, the diagonal exactly mu 1e-6
    (the clamp of D), the right-hand side 0"""
    U = got["ustar"]
    assert not np.delete(U[still][:, col, :], col, axis=1).any() and not np.delete(U[still][:, :, col], col, axis=1).any()
    assert np.array_equal(U[still][:, col, col], np.full(int(still.sum()), mu * 1e-6))
    assert not got["b"][still, col].any()
    Sd = got["S"]
    for i in np.nonzero(still)[0]:
        row, column = Sd[cd * i + col].copy(), Sd[:, cd * i + col].copy()
        assert row[cd * i + col] == mu * 1e-6
        row[cd * i + col] = column[cd * i + col] = 0.0
        assert not row.any() and not column.any(), i


@FIX
@pytest.mark.parametrize("name", rs.CASES)
def test_stage_outputs_against_the_longdouble_reference(xmamd, name, fix):
    c = rs.case(name, fix)
    S, cd, n = c["S"], 5 if fix else 8, c["S"]["n"]
    rot, t, P = c["point"]
    focal, free, dist, kfree = c["focal"], c["free"], c["dist"], c["kfree"]
    f, kc = cd - 2, cd - 1
    ctx = _ctx(xmamd, S)
    for mu in c["mus"]:
        got = _probe(ctx, c, mu)
        kw = rs.stage_args(c, mu)
        E = rs.exact_stages(S, **kw)
        e_ref = rs.reference_errors(S, E, c["keys"], **kw)
        assert max(e_ref.values()) <= st.MAX_E_REF, e_ref
        keys = c["keys"]
        if not E["positive"]:                              # the radial map folds at the candidate (xm_ba_radial_stages.py): the documented report
            assert not np.isfinite(got["cost1"]) and float(E["fold_min"]) < -1e-3
            keys = tuple(k for k in keys if k != "cost1")
        bad = st.compare(f"radial-{name}-{'fixed' if fix else 'free'}-mu{mu:g}", S, got, E, e_ref, keys)
        # exact comparisons stay exact
        assert got["n_used"] == E["n_used"]
        assert np.array_equal(got["cused"] != 0, E["cused"]) and np.array_equal(got["lused"] != 0, E["lused"])
        still, kstill = ~(E["cused"] & free), ~(E["cused"] & kfree)      # held, or without a used observation: the value does not move
        assert still.any() and not still.all() and (name == "k_zero" or (kstill.any() and not kstill.all()))
        _zero_row_and_column(got, still, f, cd, mu)
        _zero_row_and_column(got, kstill, kc, cd, mu)
        step = c["dc"].reshape(n, cd)
        assert got["focal1"][still].tobytes() == focal[still].tobytes() and got["dist1"][kstill].tobytes() == dist[kstill].tobytes()
        assert np.array_equal(got["focal1"][~still], focal[~still] + step[~still, f])
        assert np.array_equal(got["dist1"][~kstill], dist[~kstill] + step[~kstill, kc])
        assert not bad, bad
        if name == "masks":
            off = ~E["cused"]
            assert off[5] and not E["lused"][7]
            rows = np.repeat(off, cd)
            for k in ("SX", "MX_jacobi"):
                assert not np.asarray(got[k])[rows].any(), k
            assert not got["b"].reshape(-1)[rows].any()
            assert got["rot1"][:, np.repeat(off, 3)].tobytes() == np.asfortranarray(rot)[:, np.repeat(off, 3)].tobytes()
            assert got["t1"][:, off].tobytes() == np.asfortranarray(t)[:, off].tobytes()
            assert got["p1"][:, ~E["lused"]].tobytes() == np.asfortranarray(P)[:, ~E["lused"]].tobytes()
        if name == "degrees":
            deg = c["extra"]["degrees"]
            assert list(deg[:6]) == list(st.DEGREES) and deg[6] > 1024
        if name == "clamp":
            d = E["_E"].V[:, np.arange(3), np.arange(3)][E["lused"]]
            assert (d < 1e-6).any() and (d.min(axis=1) > 1e-6).any()
        if name == "loss_huber":
            assert [s for _, s in c["extra"]["edge"]] == [c["a"] * c["a"], np.nextafter(c["a"] * c["a"], np.inf)]
        if name == "mask_mix":
            i4 = np.arange(n) % 4
            assert np.array_equal(free, (i4 == 0) | (i4 == 3)) and np.array_equal(kfree, (i4 == 1) | (i4 == 3)) and E["cused"].all()
        if name == "on_axis":                              # u = 0 exactly: both columns are zero though both are free, and are handled as held ones
            i = rs.ON_AXIS_CAM
            assert free[i] and kfree[i] and E["cused"][i]
            one = np.arange(n) == i
            _zero_row_and_column(got, one, f, cd, mu)
            _zero_row_and_column(got, one, kc, cd, mu)
        if fix:
            assert got["rot1"].tobytes() == np.asfortranarray(rot).tobytes()
    ctx.close()


@FIX
def test_k_zero_gives_the_bytes_of_the_focal_probe(xmamd, fix):
    """every k = 0 and every dist_free = 0: every output other than the distortion row, column and slot is ba_probe_focal's at the same point.
    (The factor in front of the pinhole rows is g I in every bit then; what else must agree is how the compiler fuses the products of the
    rows the two forms share, which ba_eval_body fixes for CD = 8: profiles/r42_ba_radial_kernel_resources.txt, section 3.)"""
    c = rs.case("k_zero", fix)
    n, cd = c["S"]["n"], 5 if fix else 8
    assert not c["dist"].any() and not c["kfree"].any() and not c["free"].all() and c["free"].any()
    keep = np.arange(cd) != cd - 1
    X7 = c["X"].reshape(n, cd, -1)[:, keep].reshape(n * (cd - 1), -1)
    c["dc"] = np.where(np.tile(keep, n), c["dc"], 0.0)    # a held column's step is 0 in the loop; |d|^2 then has the focal form's terms
    dc7 = c["dc"].reshape(n, cd)[:, keep].reshape(-1)
    rot, t, P = c["point"]
    ctx = _ctx(xmamd, c["S"])
    mu = 1.0
    got = _probe(ctx, c, mu)
    ref = ctx.ba_probe_focal(rot, t, P, mu, focal=c["focal"], focal_free=c["free"], fix_rotations=fix, X=X7, dc=dc7, dense=True)
    ctx.close()
    same = lambda a, b: np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    for k in ("cost", "n_used", "gmax", "cost1", "model"):
        assert got[k] == ref[k], k
    for k in ("g_l", "vinv", "cused", "lused", "dP", "rot1", "t1", "p1", "focal1", "step2", "x2"):
        assert same(got[k], ref[k]), k
    assert same(got["b"][:, keep], ref["b"]) and not got["b"][:, cd - 1].any()
    for k in ("ustar", "sinv"):
        assert same(got[k][:, keep][:, :, keep], ref[k]), k
    assert np.array_equal(got["ustar"][:, cd - 1, cd - 1], np.full(n, mu * 1e-6)) and same(got["dist1"], c["dist"])
    rows = np.repeat(keep[None, :], n, axis=0).reshape(-1)
    assert same(got["Sdense"][rows][:, rows], ref["Sdense"])
    for k in ("SX", "MX"):
        assert same(np.asarray(got[k])[rows], ref[k]), k


@FIX
def test_a_step_past_the_fold_is_reported(xmamd, fix):
    """a step dc whose dk takes one used camera with a free coefficient past 1 + 3 k rho^2 = 0 for its outermost observation (and not for
    all of them): cost1 is not finite (the documented report); the same step with that entry halved is an ordinary candidate.  A held
    camera ignores its entry.  The entry aims at 1.5 times the coefficient at which the outermost observation of the candidate without it
    folds; whether a candidate folds is the longdouble reference's word, with a margin that leaves rounding no say."""
    c = rs.case("base", fix)
    n, cd = c["S"]["n"], 5 if fix else 8
    ctx = _ctx(xmamd, c["S"])
    i, held = 2, 1
    assert c["kfree"][i] and not c["kfree"][held]
    dc = c["dc"].reshape(n, cd).copy()
    dc[i, cd - 1] = dc[held, cd - 1] = 0.0
    E0 = rs.exact_stages(c["S"], **{**rs.stage_args(c, 1.0), "dc": dc.reshape(-1)})
    assert E0["positive"]
    EE = E0["_E"]
    cand = EE.candidate(dc.reshape(-1))
    u = EE.project(cand["Rcw1"], cand["tcw1"], cand["P1"])
    rho2 = np.sort(np.asarray(np.sum(u * u, axis=1)[EE.cam == i], dtype=np.float64))
    kfold = -1.0 / (3.0 * rho2[-1])                       # the coefficient at which camera i's outermost observation folds
    assert rho2[-1] > 2.0 * rho2[0]
    dc[i, cd - 1] = 1.5 * kfold - c["dist"][i]
    dc[held, cd - 1] = -1e3                                # held: no effect
    got = _probe(ctx, c, 1.0, dc.reshape(-1))
    E = rs.exact_stages(c["S"], **{**rs.stage_args(c, 1.0), "dc": dc.reshape(-1)})
    assert not E["positive"] and float(E["fold_min"]) < -1e-3 and not np.isfinite(got["cost1"])
    assert got["dist1"][i] == c["dist"][i] + dc[i, cd - 1] and got["dist1"][held] == c["dist"][held] and (got["focal1"] > 0).all()
    dc[i, cd - 1] *= 0.5
    got = _probe(ctx, c, 1.0, dc.reshape(-1))
    E = rs.exact_stages(c["S"], **{**rs.stage_args(c, 1.0), "dc": dc.reshape(-1)})
    assert E["positive"] and float(E["fold_min"]) > 1e-3 and np.isfinite(got["cost1"])
    assert abs(got["cost1"] - float(E["cost1"])) <= 1e-12 * float(E["cost1"])
    ctx.close()
