"""GPU tests of the bundle adjustment's kernels with a focal column (CD = 7, and 4 with fixed rotations; xm-code_amd/csrc/xm_ba.hip) stage
by stage through the test export xm_ctx_ba_probe_focal (Context.ba_probe_focal): one linearisation at a fixed point, fixed focal scales
and a fixed mu, no LM loop, every array compared elementwise with the longdouble reference xm_ba_focal_exact.py.

Bound (xm_ba_stages.py): e_gpu <= max(16 e_ref, 64 eps_f64) with e_ref the f64 restatement's own error against the same reference at the
same point, evaluated here per quantity and case (the larger of two observation orders).  Nothing is derived from the GPU's output.  The
cases are those of test_ba_focal_numpy.py::test_restatement_agrees_with_longdouble (which asserts e_ref <= 1e-8 for each).
Every comparison prints a line `STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s): the table of
profiles/r37_ba_focal_stage_errors.txt.

Which kernel an output pins: cost, n_used -> ba_eval_focal, ba_reduce; g_l, vinv, lused -> ba_lm; b, ustar, sinv, cused -> ba_cam; gmax ->
both; SX -> ba_lmx, ba_camx; S -> ba_schur_dense; MX_jacobi -> ba_pcg_init; dP -> ba_lmx (sign -1, with g_l); rot1, t1, focal1, step2[0],
x2[0] -> ba_cand_cam_focal; p1, step2[1], x2[1] -> ba_cand_vec; cost1, model -> ba_cost_focal."""
import numpy as np
import pytest

import xm_ba_focal_stages as fs
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
    g = ctx.ba_probe_focal(rot, t, P, mu, focal=c["focal"], focal_free=c["free"], fix_rotations=c["fix"], loss=c["loss"], loss_scale=c["a"],
                           X=c["X"], dc=c["dc"] if dc is None else dc, dense=True)
    g["S"], g["MX_jacobi"] = g["Sdense"], g["MX"]
    return g


@FIX
@pytest.mark.parametrize("name", fs.CASES)
def test_stage_outputs_against_the_longdouble_reference(xmamd, name, fix):
    c = fs.case(name, fix)
    S, cd, n = c["S"], 4 if fix else 7, c["S"]["n"]
    rot, t, P = c["point"]
    focal, free = c["focal"], c["free"]
    ctx = _ctx(xmamd, S)
    for mu in c["mus"]:
        got = _probe(ctx, c, mu)
        kw = fs.stage_args(c, mu)
        E = fs.exact_stages(S, **kw)
        e_ref = fs.reference_errors(S, E, c["keys"], **kw)
        assert max(e_ref.values()) <= st.MAX_E_REF, e_ref
        bad = st.compare(f"focal-{name}-{'fixed' if fix else 'free'}-mu{mu:g}", S, got, E, e_ref, c["keys"])
        # exact comparisons stay exact
        assert got["n_used"] == E["n_used"]
        assert np.array_equal(got["cused"] != 0, E["cused"]) and np.array_equal(got["lused"] != 0, E["lused"])
        still = ~(E["cused"] & free)                       # held, or without a used observation: the focal does not move
        assert still[::3].all() and not still.all()
        f = cd - 1
        U = got["ustar"]
        offdiag = np.delete(U[still][:, f, :], f, axis=1)
        assert not offdiag.any() and not np.delete(U[still][:, :, f], f, axis=1).any()      # the focal row and column of U*, apart from the diagonal
        assert np.array_equal(U[still][:, f, f], np.full(int(still.sum()), mu * 1e-6))       # the clamp of D
        assert not got["b"][still, f].any()
        Sd = got["S"]
        for i in np.nonzero(still)[0]:                     # and of the assembled S
            row, col = Sd[cd * i + f].copy(), Sd[:, cd * i + f].copy()
            row[cd * i + f] = col[cd * i + f] = 0.0
            assert not row.any() and not col.any(), i
        assert got["focal1"][still].tobytes() == focal[still].tobytes()
        assert np.array_equal(got["focal1"][~still], focal[~still] + c["dc"].reshape(n, cd)[~still, f])
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
        if fix:
            assert got["rot1"].tobytes() == np.asfortranarray(rot).tobytes()
    ctx.close()


@FIX
def test_a_step_to_a_focal_that_is_not_positive_is_reported(xmamd, fix):
    """the candidate of a step dc whose focal entry takes one free, used camera's g to 0, and another's below: cost1 is not finite (the
    documented report); the same step with those two entries halved is an ordinary candidate.  A held camera ignores its entry."""
    c = fs.case("base", fix)
    n, cd = c["S"]["n"], 4 if fix else 7
    ctx = _ctx(xmamd, c["S"])
    dc = c["dc"].reshape(n, cd).copy()
    assert c["free"][1] and c["free"][2] and not c["free"][3]
    dc[1, cd - 1] = -c["focal"][1]                         # exactly 0
    dc[2, cd - 1] = -2.0 * c["focal"][2]
    dc[3, cd - 1] = -5.0                                   # held: no effect
    got = _probe(ctx, c, 1.0, dc.reshape(-1))
    assert not np.isfinite(got["cost1"])
    assert got["focal1"][1] == 0.0 and got["focal1"][2] == -c["focal"][2] and got["focal1"][3] == c["focal"][3]
    dc[1, cd - 1] *= 0.5; dc[2, cd - 1] *= 0.25
    got = _probe(ctx, c, 1.0, dc.reshape(-1))
    E = fs.exact_stages(c["S"], **{**fs.stage_args(c, 1.0), "dc": dc.reshape(-1)})
    assert E["positive"] and np.isfinite(got["cost1"]) and (got["focal1"] > 0).all()
    assert abs(got["cost1"] - float(E["cost1"])) <= 1e-12 * float(E["cost1"])
    ctx.close()
