"""The truncated CG behind a rejected step, replayed from the rejected one's history, against the same one recomputed (XM_FLAG_TCG_RECOMPUTE),
bit for bit.

When the host rejects a step it keeps the point, its gradient state, the loss and |r|^2 and shrinks the radius: the next truncated CG starts from
bit-identical inputs and repeats the rejected one's iterations until the smaller radius trips.  The steps of a live truncated CG store p_j, Hp_j
and what they decided from (TcgHist); one launch of tcg_replay_kernel then walks the records with the new radius and rebuilds v and H v -- no
product, no step.  Every solve below runs once by default and once with XM_FLAG_TCG_RECOMPUTE on one context and must give the same bytes: R, s,
the trace, the primal value, the counters.  From the default run's own trace: every stage has a rejection that is followed by a truncated CG, every
one of those was replayed (info["tcg_replays"]) and stands for the iterations the trace shows behind it (info["tcg_replayed_iters"]); with the
history cut to 4 iterations (xm_ctx_set_tcg_history) some are replayed and some fall back to the recomputation."""
import numpy as np
import pytest

import xm_rtr_stages as rs
import xm_testlib as tl

pytestmark = pytest.mark.gpu

SYM = dict(sym=1, sym_min_rows=1)     # the two-launch form: the step's workgroups ride on the symmetric sweep
_runs = {}   # case id -> (replayed, recomputed): every solve runs once, whichever test asks first


def _solve_both(xmamd, mk, tuning, max_rank=5, lam=1.0, tol=1e-8, **kw):
    """one context, the solve in the default form and again with XM_FLAG_TCG_RECOMPUTE -> the two (R, s, info)"""
    Q = tl.gen_vg(mk[1], deg=3, sigma=1.5, seed=mk[1])["Q"] if mk[0] == "vg-dense" else rs.matrix(*mk)["Q"]
    ctx = xmamd.Context(Q=Q, tuning=tuning or None)
    try:
        flags = kw.pop("flags", 0)
        if "history" in kw:
            ctx.set_tcg_history(kw.pop("history"))
        a = ctx.solve(max_rank, tol, lam, trace=4000, flags=flags, **kw)
        b = ctx.solve(max_rank, tol, lam, trace=4000, flags=flags | xmamd.FLAG_TCG_RECOMPUTE, **kw)
    finally:
        ctx.close()
    return a, b


CASES = {}
# the general kernel with three launches per iteration
CASES.update({f"general-n{n}": (lambda x, n=n: _solve_both(x, ("dense", n, 0), {})) for n in (9, 85, 87, 128)})
# the two-launch form, with several partitions of the step's workgroups
CASES.update({f"sym-n{n}": (lambda x, n=n: _solve_both(x, ("dense", n, 0), SYM)) for n in (9, 85, 87, 128, 343)})
# noisy view graphs as dense matrices: staircases to rank 5 with rejections in every stage, one of them in the first outer iteration behind the
# escalation's line search (the stale scaled point of the reference)
for _n in (40, 87):
    CASES[f"general-staircase-n{_n}"] = lambda x, n=_n: _solve_both(x, ("vg-dense", n), {}, lam=3.0, tol=1e-9)
    CASES[f"sym-staircase-n{_n}"] = lambda x, n=_n: _solve_both(x, ("vg-dense", n), SYM, lam=3.0, tol=1e-9)
# a history of 4 iterations: rejected truncated CGs of up to 27 iterations, so that replays stand next to fallbacks
CASES["general-short-history"] = lambda x: _solve_both(x, ("vg-dense", 40), {}, lam=3.0, tol=1e-9, history=4)
CASES["sym-short-history"] = lambda x: _solve_both(x, ("vg-dense", 40), SYM, lam=3.0, tol=1e-9, history=4)
CASES["model-recurrence"] = lambda x: _solve_both(x, ("dense", 87, 0), SYM, flags=x.FLAG_MODEL_RECURRENCE)
CASES["polar"] = lambda x: _solve_both(x, ("dense", 87, 0), SYM, retraction=x.RETRACT_POLAR)
CASES.update({f"grouping{g}": (lambda x, g=g: _solve_both(x, ("dense", 87, 0), SYM, grouping=g)) for g in (1, 2)})


def _case(xmamd, cid):
    if cid not in _runs:
        _runs[cid] = CASES[cid](xmamd)
    return _runs[cid]


def _stages(trace):
    """the trace rows of each trust region: one starts with the row of outer iteration 0 (one inner iteration, end reason 6, status 4)"""
    starts = [i for i in range(len(trace)) if (int(trace[i, 2]), int(trace[i, 3]), int(trace[i, 4])) == (1, 6, 4)]
    return [trace[a:b] for a, b in zip(starts, starts[1:] + [len(trace)])]


def _rejections(trace):
    """per stage: the iterations of the truncated CG behind every rejected step (row with trstatus 3 that is not the last of its trust region)"""
    return [[int(t[i + 1, 2]) for i in range(1, len(t) - 1) if int(t[i, 4]) == 3] for t in _stages(trace)]


@pytest.mark.parametrize("cid", sorted(CASES))
def test_replay_gives_the_bits_of_the_recomputation(xmamd, cid):
    (Ra, sa, ia), (Rb, sb, ib) = _case(xmamd, cid)
    assert Ra.shape == Rb.shape and Ra.tobytes() == Rb.tobytes()
    assert sa.tobytes() == sb.tobytes()
    assert ia["trace"].tobytes() == ib["trace"].tobytes()
    for k in ("tcg_iters", "outer_iters", "rank", "status", "last_stop_reason"):
        assert ia[k] == ib[k], (k, ia[k], ib[k])
    assert np.float64(ia["primal"]).tobytes() == np.float64(ib["primal"]).tobytes()
    assert ia["tcg_two_launch"] == ib["tcg_two_launch"] and (ia["tcg_two_launch"] > 0) == cid.startswith(("sym", "model", "polar", "grouping"))
    if "staircase" in cid or "short-history" in cid:
        assert ia["rank"] == 5, ia["rank"]


@pytest.mark.parametrize("cid", sorted(CASES))
def test_every_rejection_was_replayed(xmamd, cid):
    (_, _, ia), (_, _, ib) = _case(xmamd, cid)
    rej = _rejections(ia["trace"])
    print(cid, "rejections followed by a truncated CG, per stage:", [len(r) for r in rej], "iterations:", [sum(r) for r in rej],
          "replays", ia["tcg_replays"], "replayed iterations", ia["tcg_replayed_iters"], "of", ia["tcg_iters"])
    assert rej and all(len(r) >= 1 for r in rej), [len(r) for r in rej]
    count, iters = sum(len(r) for r in rej), sum(sum(r) for r in rej)
    assert ib["tcg_replays"] == 0 and ib["tcg_replayed_iters"] == 0
    if "short-history" in cid:
        assert 0 < ia["tcg_replays"] < count, (ia["tcg_replays"], count)
    else:
        assert ia["tcg_replays"] == count, (ia["tcg_replays"], count)
        assert ia["tcg_replayed_iters"] == iters, (ia["tcg_replayed_iters"], iters)
    assert ia["qw_products"] < ib["qw_products"], (ia["qw_products"], ib["qw_products"])
