"""GPU tests of the focal groups' kernels (xm-code_amd/csrc/xm_ba.hip: ba_cam<GR>, ba_group_setup, ba_group_expand, ba_group_sum,
ba_group_cand, ba_cand_cam_groups) stage by stage through the test export xm_ctx_ba_probe_focal_groups (Context.ba_probe_focal(...,
focal_group=)): one linearisation at a fixed point, fixed group scales and a fixed mu, no LM loop, every array compared with the longdouble
reference xm_ba_groups_exact.py.

Bound (xm_ba_stages.py): e_gpu <= max(16 e_ref, 64 eps_f64) with e_ref the f64 restatement's own error against the same reference at the
same point, evaluated here per quantity and case (the larger of two observation orders).  Nothing is derived from the GPU's output.  The
cases are those of test_ba_groups_numpy.py::test_restatement_agrees_with_longdouble_and_m_is_spd (which asserts e_ref <= 1e-8 for each).
Every comparison prints a line `STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s): the table of
profiles/r38_ba_groups_stage_errors.txt.

Which kernel an output pins: b, D, F, gmax -> ba_cam<GR>, ba_group_setup; SX -> ba_group_expand, ba_lmx, ba_camx, ba_group_sum; S -> ba_schur_dense and the
ba_group_dense_* contraction; F -> ba_group_unit, the product, ba_group_col; MX -> ba_group_setup (the preconditioner's blocks),
ba_pcg_init, ba_group_precond (the exact block's inverse, G <= 16: every case but singletons and g17); dP -> ba_group_expand, ba_lmx; focal1, step2[0], x2[0] -> ba_group_cand,
ba_cand_cam_groups; cost1, model -> ba_cost_focal on the expanded step."""
import numpy as np
import pytest

import xm_ba_groups_stages as gs
import xm_ba_stages as st

pytestmark = pytest.mark.gpu

FIX = pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])


def _ctx(xmamd, S, **kw):
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S.get("w0", S["w"])), n=S["n"], **kw)
    if "w0" in S:
        ctx.set_edge_weights(S["w"])
    return ctx


def _probe(ctx, c, mu, dc=None, S=None):
    rot, t, P = c["point"]
    g = ctx.ba_probe_focal(rot, t, P, mu, focal=c["focal"], focal_free=c["free"], fix_rotations=c["fix"], loss=c["loss"], loss_scale=c["a"],
                           X=c["X"], dc=c["dc"] if dc is None else dc, focal_group=c["group_of"], dense=True)
    g["S"] = g["Sdense"]
    return g


@FIX
@pytest.mark.parametrize("name", gs.CASES)
def test_stage_outputs_against_the_longdouble_reference(xmamd, name, fix):
    c = gs.case(name, fix)
    S, n, G, cp = c["S"], c["S"]["n"], c["G"], 3 if fix else 6
    rot, t, P = c["point"]
    focal, group_of = c["focal"], c["group_of"]
    ctx = _ctx(xmamd, S)
    for mu in c["mus"]:
        got = _probe(ctx, c, mu)
        again = _probe(ctx, c, mu)
        for k in gs.KEYS:                                  # two calls give the same bytes
            assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k
        kw = gs.stage_args(c, mu)
        E = gs.exact_stages(S, **kw)
        e_ref = gs.reference_errors(S, E, gs.KEYS, G, **kw)
        assert max(e_ref.values()) <= st.MAX_E_REF, e_ref
        bad = gs.compare(f"groups-{name}-{'fixed' if fix else 'free'}-mu{mu:g}", S, got, E, e_ref, gs.KEYS, G)
        # exact comparisons stay exact
        assert got["n_used"] == E["n_used"]
        assert np.array_equal(got["cused"] != 0, E["cused"]) and np.array_equal(got["lused"] != 0, E["lused"])
        still = ~E["moving"]                               # held, empty, or without a used member: the focal does not move
        dg = c["dc"][cp * n:]
        assert got["focal1"][still].tobytes() == focal[still].tobytes()
        assert np.array_equal(got["focal1"][~still], focal[~still] + dg[~still])
        assert not got["b"][cp * n:][still].any()
        assert np.array_equal(got["D"][still], np.full(int(still.sum()), 1e-6))           # the clamp of D
        members = np.bincount(group_of, minlength=G)
        exact = G <= 16                                    # XM_BA_FOCAL_GROUPS_EXACT: F is the G x G block and the preconditioner uses its inverse
        Fd = np.diag(got["F"]) if exact else got["F"]
        assert got["F"].shape == ((G, G) if exact else (G,)) and got["coarse_ok"] == (1 if exact else 0)
        assert np.array_equal(Fd[still], np.full(int(still.sum()), mu * 1e-6))
        if exact:
            off = got["F"] - np.diag(Fd)
            assert not off[still].any() and not off[:, still].any()
        assert not np.asarray(got["SX"])[cp * n:][members == 0].any() and not np.asarray(got["MX"])[cp * n:][members == 0].any()
        # the member blocks the device holds: the focal diagonal of U* undamped, 1 / F in the representative's slot of the preconditioner
        f = cp
        rep = np.full(G, -1)
        rep[group_of[::-1]] = np.arange(n)[::-1]            # the first member
        isrep = np.zeros(n, dtype=bool); isrep[rep[rep >= 0]] = True
        assert not got["sinv"][~isrep, f, f].any()
        assert np.array_equal(got["sinv"][rep[rep >= 0], f, f], np.zeros(int((rep >= 0).sum())) if exact else 1.0 / got["F"][rep >= 0])
        Sg = got["S"]                                      # a held or unused group's row and column of the contracted matrix: the diagonal alone
        for cgrp in np.nonzero(still)[0]:
            row, col = Sg[cp * n + cgrp].copy(), Sg[:, cp * n + cgrp].copy()
            assert row[cp * n + cgrp] == mu * 1e-6
            row[cp * n + cgrp] = col[cp * n + cgrp] = 0.0
            assert not row.any() and not col.any(), cgrp
        assert not np.delete(got["sinv"][:, f, :], f, axis=1).any() and not np.delete(got["sinv"][:, :, f], f, axis=1).any()
        assert not got["ustar"][~E["cused"], f, f].any()   # no mu 1e-6 on an unused member: the damping is the group's
        assert not bad, bad
        if fix:
            assert got["rot1"].tobytes() == np.asfortranarray(rot).tobytes()
    if name == "base":
        assert still[1] and still[5] and int(still.sum()) == 2
    if name == "unused_member":
        assert not E["cused"][5] and group_of[5] == 1 and not still[1] and still[0] and still[5]
    if name == "unused_group":
        assert not E["cused"][5] and group_of[5] == 0 and still[0] and int(still.sum()) == 1
    if name == "sizes":
        assert tuple(members) == gs.SIZES
    ctx.close()


def test_a_permuted_observation_list_stays_within_the_bound(xmamd):
    c = gs.case("base", False)
    S, G = c["S"], c["G"]
    perm = np.random.default_rng(5).permutation(len(S["cam"]))
    Sp = dict(S, cam=np.asarray(S["cam"])[perm], lm=np.asarray(S["lm"])[perm], p=np.asarray(S["p"])[perm], w=np.asarray(S["w"])[perm])
    ctx = _ctx(xmamd, Sp)
    kw = gs.stage_args(c, 1.0)
    got = _probe(ctx, c, 1.0)
    E = gs.exact_stages(S, **kw)
    e_ref = gs.reference_errors(S, E, gs.KEYS, G, **kw)
    bad = gs.compare("groups-base-permuted", S, got, E, e_ref, gs.KEYS, G)
    assert not bad, bad
    ctx.close()


@FIX
def test_a_step_to_a_group_focal_that_is_not_positive_is_reported(xmamd, fix):
    """the candidate of a step whose focal entry takes one moving group's g to 0: cost1 is not finite (the documented report); a held
    group ignores its entry; the same step with that entry halved is an ordinary candidate"""
    c = gs.case("base", fix)
    n, cp = c["S"]["n"], 3 if fix else 6
    ctx = _ctx(xmamd, c["S"])
    dc = c["dc"].copy()
    dc[cp * n + 0] = -c["focal"][0]                        # exactly 0
    dc[cp * n + 1] = -5.0                                  # held: no effect
    got = _probe(ctx, c, 1.0, dc)
    assert not np.isfinite(got["cost1"])
    assert got["focal1"][0] == 0.0 and got["focal1"][1] == c["focal"][1]
    dc[cp * n + 0] *= 0.5
    got = _probe(ctx, c, 1.0, dc)
    E = gs.exact_stages(c["S"], **{**gs.stage_args(c, 1.0), "dc": dc})
    assert E["positive"] and np.isfinite(got["cost1"]) and (got["focal1"] > 0).all()
    assert abs(got["cost1"] - float(E["cost1"])) <= 1e-12 * float(E["cost1"])
    ctx.close()
