"""GPU tests of the two-level preconditioner of the matrix-free CG form (xm_tuning_t.schur_solver = 3): exact blocks of the reduced camera
Laplacian VT on aggregates of 64 cameras in breadth-first order plus the coarse operator P^T VT P.  On a sequential capture (every landmark
seen by a few consecutive frames) Jacobi needs O(N) inner iterations and stops at the cap of 1000; the two-level form converges in under
150 and gives the products of the dense-inverse form (schur_solver = 1)."""
import numpy as np
import pytest

import xm_seqscene as sq
import xm_testlib as tl

pytestmark = pytest.mark.gpu

O_LIST = (1, 3, 4, 5)


def _obs(S):
    return (S["cam"], S["lm"], S["p"], S["w"])


def _products(xmamd, obs, solver, Ws, **tuning):
    ctx = xmamd.Context(obs=obs, tuning=dict(schur_solver=solver, **tuning))
    try:
        Y = [ctx.qw(W) for W in Ws]
        return Y, ctx.schur_info()
    finally:
        ctx.close()


def _W(n, seed=0):
    return [np.random.default_rng(seed + o).standard_normal((3 * n, o)) for o in O_LIST]


@pytest.fixture(scope="module")
def seq3000():
    return sq.gen_sequential(3000, seed=1)


def test_sequential_products_equal_the_dense_inverse_where_jacobi_caps(xmamd, seq3000):
    S = seq3000
    Ws = _W(S["n"])
    Y1, s1 = _products(xmamd, _obs(S), 1, Ws)
    Y3, s3 = _products(xmamd, _obs(S), 3, Ws)
    assert s1["precond"] is None and not s1["cg"]
    assert s3["cg"] and s3["precond"] == "two-level" and s3["aggregates"] == -(-(S["n"] - 1) // 64)
    for o, a, b in zip(O_LIST, Y1, Y3):
        assert tl.rel_fro(b, a) < 1e-10, o
    assert s3["products"] == len(O_LIST) and s3["capped"] == 0
    assert s3["inner_iters"] / s3["products"] < 150, s3
    # control: the Jacobi form on the same scene stops at the iteration cap (1000) -- the operator is inexact
    _, s2 = _products(xmamd, _obs(S), 2, Ws[1:2])
    assert s2["precond"] == "jacobi" and s2["aggregates"] == 0
    assert s2["capped"] == 1 and s2["inner_iters"] >= 1000, s2
    print(f"3000 sequential cameras: two-level {s3['inner_iters'] / s3['products']:.1f} inner iterations per product, Jacobi {s2['inner_iters']} (capped)")


def test_renumbered_cameras_give_the_same_products(xmamd, seq3000):
    S = seq3000
    T, pi = sq.renumber(S, seed=2)
    Ws = _W(S["n"], seed=10)
    Y, s = _products(xmamd, _obs(S), 3, Ws)
    Yp, sp = _products(xmamd, _obs(T), 3, [sq.permute_rows(W, pi) for W in Ws])
    for a, b in zip(Y, Yp):
        assert tl.rel_fro(b, sq.permute_rows(a, pi)) < 1e-10
    assert sp["capped"] == s["capped"] == 0
    assert sp["inner_iters"] <= 1.5 * s["inner_iters"] and s["inner_iters"] <= 1.5 * sp["inner_iters"], (s, sp)


def test_whole_solve_on_a_sequential_scene_with_loop_closures(xmamd):
    S = sq.gen_sequential(150, loops=6, seed=3)
    n = S["n"]
    lam = 1.5 * float(np.sum(S["w"] * np.sum(S["p"] ** 2, axis=1)) / (3 * n))
    out = {}
    for solver in (1, 3):
        ctx = xmamd.Context(obs=_obs(S), tuning=dict(schur_solver=solver, schur_pcg_hess_digits=13))
        R, s, info = ctx.solve(5, 1e-8, lam)
        out[solver] = (R, s, info, ctx.schur_info())
        ctx.close()
    (R1, s1, i1, _), (R3, s3, i3, q3) = out[1], out[3]
    assert i1["status"] == i3["status"] == 1 and i1["rank"] == i3["rank"]
    assert i3["primal"] == pytest.approx(i1["primal"], rel=1e-8)
    print(f"whole solve: rotation parity {tl.rotation_parity(R3, s3, R1, s1):.2e}, primal rel {abs(i3['primal'] / i1['primal'] - 1):.1e}")
    # measured: 1.0e-7 here (2.7e-7 at 300 cameras, where the Jacobi form is 3.9e-9 from the dense inverse and 5e-13 from this form in the
    # primal): the optimum of a sequential scene is flat along directions the stop rule does not resolve; the bound of the multi-rank tests
    assert tl.rotation_parity(R3, s3, R1, s1) < 1e-6
    assert q3["capped"] == 0 and q3["products"] > 4


def test_random_scene_matches_jacobi_with_few_extra_iterations(xmamd):
    S = tl.gen_scene(600, 60000, 6, seed=5)
    Ws = _W(600, seed=20)
    Y2, s2 = _products(xmamd, _obs(S), 2, Ws)
    Y3, s3 = _products(xmamd, _obs(S), 3, Ws)
    for a, b in zip(Y2, Y3):
        assert tl.rel_fro(b, a) < 1e-10
    assert s2["capped"] == s3["capped"] == 0
    assert s3["inner_iters"] <= s2["inner_iters"] + 3 * s3["products"], (s2, s3)


def test_two_contexts_give_identical_bits(xmamd):
    S = sq.gen_sequential(1500, loops=10, seed=4)
    Ws = _W(S["n"], seed=30)
    Ya, sa = _products(xmamd, _obs(S), 3, Ws)
    Yb, sb = _products(xmamd, _obs(S), 3, Ws)
    for a, b in zip(Ya, Yb):
        assert np.array_equal(a, b)
    assert sa["inner_iters"] == sb["inner_iters"] and sa["capped"] == 0


def test_duplicated_pairs_and_heavy_landmarks(xmamd):
    S = sq.gen_sequential(1200, seed=6, heavy=4, heavy_views=90)
    rng = np.random.default_rng(6)
    dup = rng.choice(S["cam"].size, 300, replace=False)          # (camera, landmark) pairs named twice, with their own point and weight
    cam = np.concatenate([S["cam"], S["cam"][dup]]); lm = np.concatenate([S["lm"], S["lm"][dup]])
    p = np.concatenate([S["p"], S["p"][dup] + 0.01 * rng.standard_normal((dup.size, 3))])
    w = np.concatenate([S["w"], rng.uniform(0.5, 1.5, dup.size)])
    assert np.bincount(lm).max() > 64                             # heavy landmarks: rank-1 terms of the coarse operator
    Ws = _W(S["n"], seed=40)
    Y1, _ = _products(xmamd, (cam, lm, p, w), 1, Ws)
    Y3, s3 = _products(xmamd, (cam, lm, p, w), 3, Ws)
    for a, b in zip(Y1, Y3):
        assert tl.rel_fro(b, a) < 1e-10
    assert s3["capped"] == 0 and s3["inner_iters"] / s3["products"] < 150


def test_reweighting_rebuilds_the_preconditioner(xmamd):
    S = sq.gen_sequential(2000, seed=7)
    w2 = S["w"].copy()
    w2[S["cam"] < S["n"] // 2] *= 100.0                            # half of the trajectory weighs 100 times more
    W = np.random.default_rng(50).standard_normal((3 * S["n"], 3))
    ctx = xmamd.Context(obs=_obs(S), tuning=dict(schur_solver=3))
    ctx.qw(W)
    ctx.set_edge_weights(w2)
    before = ctx.schur_info()
    Y = ctx.qw(W)
    after = ctx.schur_info()
    ctx.close()
    Yf, sf = _products(xmamd, (S["cam"], S["lm"], S["p"], w2), 3, [W])
    assert tl.rel_fro(Y, Yf[0]) < 1e-12
    assert after["inner_iters"] - before["inner_iters"] == sf["inner_iters"]
    assert after["capped"] == sf["capped"] == 0


def test_refusals_leave_the_device_usable(xmamd):
    S = sq.gen_sequential(200, seed=8)
    with pytest.raises(xmamd.XmError, match="schur_solver must be 0, 1, 2 or 3"):
        xmamd.Context(obs=_obs(S), tuning=dict(schur_solver=4))
    with pytest.raises(xmamd.XmError, match="single-rank"):
        xmamd.Context(obs=_obs(S), n_gpus=2, gpu_map=1, tuning=dict(schur_solver=3))
    # (more than 4096 aggregates: the host plan's refusal, tests/test_schur_precond_plan.py)
    W = _W(S["n"], seed=60)[1:2]
    Y1, _ = _products(xmamd, _obs(S), 1, W)
    Y3, s3 = _products(xmamd, _obs(S), 3, W)
    assert tl.rel_fro(Y3[0], Y1[0]) < 1e-10 and s3["capped"] == 0
