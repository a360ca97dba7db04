"""The truncated CG's iteration in two launches against the same iteration in three (XM_FLAG_TCG_THREE_LAUNCH), bit for bit.

On one GPU with the host-driven outer iteration and the f64 symmetric dense pair at ranks 3 and 4, the sweep of iteration i carries cg_step(i - 1)
in its own launch and forms its product input from p, r, Hp of iteration i - 1 instead of reading W.  The step's decision and the expression for W
are the routines cg_step itself uses, no sum changes its order: every solve below must give the same bytes in both forms -- R, s, the trace,
the iteration counts and the primal value -- and info["tcg_two_launch"] must say which form ran.  The shapes are the symmetric stage shapes
of xm_rtr_stages.py (one strip with an absent second half and an odd camera count; around the 256-column tile; a last strip that is half;
several strips and chunks), and the traces must between them contain every way a truncated CG ends that the two forms share."""
import numpy as np
import pytest

import xm_rtr_stages as rs
import xm_testlib as tl

pytestmark = pytest.mark.gpu

TUNING = dict(sym=1, sym_min_rows=1)
SHAPES = (9, 85, 86, 87, 128, 343)
LAM = 1.0
_runs = {}   # case id -> (two, three): every solve runs once, whichever test asks first


def _solve_both(xmamd, mk, max_rank, lam=LAM, tol=1e-8, **kw):
    """one context, the solve in the default form and again with XM_FLAG_TCG_THREE_LAUNCH -> the two (R, s, info)"""
    Q = tl.gen_vg(mk[1], deg=3, sigma=1.5, seed=mk[1])["Q"] if mk[0] == "vg-dense" else rs.matrix(*mk)["Q"]
    ctx = xmamd.Context(Q=Q, tuning=TUNING)
    try:
        flags = kw.pop("flags", 0)
        two = ctx.solve(max_rank, tol, lam, trace=4000, flags=flags, **kw)
        three = ctx.solve(max_rank, tol, lam, trace=4000, flags=flags | xmamd.FLAG_TCG_THREE_LAUNCH, **kw)
    finally:
        ctx.close()
    return two, three


def _finer_cut(xmamd):
    L = xmamd.lib()
    xmamd._chk(L.xm_bench_symv_k(4, 1, 2))   # the plan belongs to the workspace a context makes: set before the context, reset behind it
    try:
        return _solve_both(xmamd, ("dense", 343, 0), 5)
    finally:
        xmamd._chk(L.xm_bench_symv_k(0, 1, 0))


CASES = {f"n{n}": (lambda x, n=n: _solve_both(x, ("dense", n, 0), 5)) for n in SHAPES}
CASES.update({f"grouping{g}": (lambda x, g=g: _solve_both(x, ("dense", 87, 0), 5, grouping=g)) for g in (1, 2)})   # (grouping 0: every other case)
CASES["polar"] = lambda x: _solve_both(x, ("dense", 86, 0), 5, retraction=x.RETRACT_POLAR)
CASES["model-recurrence"] = lambda x: _solve_both(x, ("dense", 128, 0), 5, flags=x.FLAG_MODEL_RECURRENCE)
CASES["finer-cut"] = _finer_cut
# noisy view graphs as dense matrices: staircases that climb to rank 5 -- the stage matrices above are solved at rank 3 -- so that the rank-4 sweep
# carries steps too and the rank-5 trust region, which keeps its three launches, follows two that did not (n = 87: again around the tile)
CASES.update({f"staircase-n{n}": (lambda x, n=n: _solve_both(x, ("vg-dense", n), 5, lam=3.0, tol=1e-9)) for n in (40, 87)})
# the known-answer matrix, solved from the identity stack into its planted optimum: truncated CGs that end in their first iteration
CASES["optimum"] = lambda x: _solve_both(x, ("dense", 43, 1), 4, lam=0.0)


def _case(xmamd, cid):
    if cid not in _runs:
        _runs[cid] = CASES[cid](xmamd)
    return _runs[cid]


def _stages_34(info):
    """trust regions at ranks 3 and 4 of a staircase that ended at info["rank"]: those run in the two-launch form (rank 5 keeps three launches)"""
    return min(info["rank"], 4) - 2


@pytest.mark.parametrize("cid", sorted(CASES))
def test_two_launches_give_the_bits_of_three(xmamd, cid):
    (R2, s2, i2), (R3, s3, i3) = _case(xmamd, cid)
    assert i2["sym_product"] == 1 and i3["sym_product"] == 1
    assert i3["tcg_two_launch"] == 0, i3["tcg_two_launch"]
    assert i2["tcg_two_launch"] == _stages_34(i2), (i2["tcg_two_launch"], i2["rank"])
    assert R2.shape == R3.shape and R2.tobytes() == R3.tobytes()
    assert s2.tobytes() == s3.tobytes()
    assert i2["trace"].tobytes() == i3["trace"].tobytes()
    for k in ("tcg_iters", "outer_iters", "rank", "status", "last_stop_reason"):
        assert i2[k] == i3[k], (k, i2[k], i3[k])
    assert np.float64(i2["primal"]).tobytes() == np.float64(i3["primal"]).tobytes()
    assert i2["tcg_iters"] > 0
    if cid.startswith("staircase"):
        assert i2["rank"] == 5 and i2["tcg_two_launch"] == 2, (i2["rank"], i2["tcg_two_launch"])
    if cid == "optimum":
        assert (i2["trace"][1:, 2] == 1).any(), i2["trace"][:, 2]   # a truncated CG of one iteration: the step rides on launch pair 1


def test_every_shared_ending_was_met(xmamd):
    """interior convergence (3), boundary (2) and negative curvature (1) each ended a truncated CG of the solves above, in the two-launch form"""
    ends = {cid: set(int(e) for e in _case(xmamd, cid)[0][2]["trace"][1:, 3]) for cid in sorted(CASES)}
    assert {1, 2, 3} <= set().union(*ends.values()), {k: sorted(v) for k, v in ends.items()}
