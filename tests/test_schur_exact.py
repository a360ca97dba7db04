"""CPU tests of the references of the matrix-free Q's stage tests: the longdouble reference (xm_schur_exact.py) against two independent
statements of the same operator, the f64 numpy restatement (xm_schur_stages.py) against the longdouble reference for every case, kind and
quantity the GPU test compares (e_ref <= MAX_E_REF: a worse scene is a badly chosen scene), and the bound against deliberate damage."""
import os

import numpy as np
import pytest

import xm_rtr_stages as rs
import xm_schur_exact as ex
import xm_schur_stages as ss
import xm_testlib as tl

KINDS = ("dense", "jacobi", "two_level")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simple2")


def _perm(xmamd, case, kind):
    return ss.plan_perm(xmamd, case) if (kind == "two_level" and ss.scene(case)["n"] > 1) else None


@pytest.mark.parametrize("case", ss.CASES)
def test_restatement_agrees_with_the_longdouble_reference(xmamd, case):
    S = ss.scene(case)
    kinds = sorted({ss.FORMS[f][1] for f in ss.forms_of(case)})
    for kind in kinds:
        perm = _perm(xmamd, case, kind)
        for o in ss.o_of(case):
            e = ss.reference_errors(case, kind, o, perm)
            for k in ss.keys_of(kind, S["n"] - 1):
                print(f"E_REF {case} {kind} o{o} {k}: {e[k]:.3e}")
                assert e[k] <= ss.MAX_E_REF, (kind, o, k, e[k])
    E = ss.exact_op(case)
    if S["n"] > 1:
        assert E.refine[1] < 1e-17 and E.cond() < 1e5, (E.refine, E.cond())


def test_scenes_have_the_edges_they_are_for():
    S = ss.scene("degrees")
    deg = np.bincount(S["lm"], minlength=S["m"])
    assert S["n"] == 1030 and int((deg > 64).sum()) == 6 and int((deg <= 64).sum()) == 1024 + 64 + 1
    for d, l in S["roles"].items():
        assert deg[l] == d
        if d >= 2:
            assert bool(np.any(S["cam"][S["lm"] == l] == 0)) == ss.WITH_CAMERA_0[d]
    assert S["roles"][0] < S["m"] - 1
    for name in ("degrees", "cam_degrees", "base", "masks") + tuple(f"tiny{n}" for n in ss.TINY_N):
        T = ss.scene(name)
        assert np.unique(T["cam"].astype(np.int64) * T["m"] + T["lm"]).size == T["cam"].size, name       # no pair named twice
    T = ss.scene("masks_dup")
    assert np.unique(T["cam"].astype(np.int64) * T["m"] + T["lm"]).size == T["cam"].size - 1
    assert tuple(np.bincount(ss.scene("cam_degrees")["cam"])) == ss.CAM_COUNTS and ss.CAM_COUNTS[0] == 64
    M = ss.scene("masks")
    assert np.count_nonzero(M["w"] == 0) >= M["w"].size // 10
    assert list(np.nonzero(ss.exact_op("masks").q3inv == 0)[0]) == list(ss.MASK_ZERO_LANDMARKS)
    for k in ss.AGG_REDUCED:
        assert ss.scene(f"agg{k}")["n"] - 1 == k


def test_exact_product_is_the_dense_longdouble_schur_complement():
    S = ss.scene("base")
    Q = rs.schur_dense_ld(S["cam"], S["lm"], S["p"], S["w"])
    for o in (1, 4):
        W, alpha, _ = ss.inputs("base", o)
        Y = ss.exact_chain("base", o)["Y"].reshape(3 * S["n"], o)
        ref = alpha * (Q @ W.astype(ex.LD))
        assert float(np.abs(Y - ref).max() / np.abs(ref).max()) < 1e-17


def test_exact_chain_reproduces_the_golden_matrix():
    """tests/golden/simple2: the dense Q the reference's create_matrix wrote from the observation list obs.npz (2e-13 |Q| from the chain)"""
    Q = tl.load_bin(os.path.join(GOLD, "Q.bin"))
    Z = np.load(os.path.join(GOLD, "obs.npz"))
    cam, lm, p, w = Z["cam"], Z["lm"], Z["p"], np.asarray(Z["w"]).reshape(-1)
    n, m = Q.shape[0] // 3, int(lm.max()) + 1
    W = np.random.default_rng(2).standard_normal((3 * n, 3))
    Y = ex.Exact(cam, lm, p, w, n, m).chain(W)["Y"].reshape(3 * n, 3)
    assert tl.rel_fro(Y.astype(np.float64), Q @ W) < 1e-11


DAMAGE = {   # damage -> (case, kind, the quantities it must push past the bound)
    "h_row": ("base", "dense", ("h", "xl")),           # a few ulp x 1e3 on one landmark row: r, a sum over ~8 landmarks, stays inside
    "skip_observation": ("base", "two_level", ("Q1", "c", "q2", "q3inv", "dinv", "h", "r", "xc", "xl", "Y", "VX", "pAp", "MX", "binv")),
    "skip_observation_dense": ("base", "dense", ("VTinv", "xc", "Y")),
    "pad_row": ("agg65", "two_level", ("ainv", "MX")),
    "block_pair": ("agg65", "two_level", ("binv", "MX")),
}


@pytest.mark.parametrize("name", tuple(DAMAGE))
def test_a_damaged_restatement_misses_the_bound(xmamd, name):
    case, kind, keys = DAMAGE[name]
    S = ss.scene(case)
    o = 3
    W, alpha, X = ss.inputs(case, o)
    perm = _perm(xmamd, case, kind)
    E = ss.exact_all(case, kind, o, perm)
    e_ref = ss.reference_errors(case, kind, o, perm)
    arg = {"h_row": 11, "skip_observation": 9, "skip_observation_dense": 9, "pad_row": 1, "block_pair": 0}[name]
    bad = ss.f64_stages(S, kind, W, alpha, X, perm, damage={name.replace("_dense", ""): arg})
    missed = {b[0] for b in ss.compare(f"{case} {kind} damage={name}", bad, E, e_ref, ss.keys_of(kind, S["n"] - 1), who="damaged")}
    assert set(keys) <= missed, (name, sorted(set(keys) - missed))
    clean = ss.f64_stages(S, kind, W, alpha, X, perm)
    assert not ss.compare(f"{case} {kind} clean", clean, E, e_ref, ss.keys_of(kind, S["n"] - 1), who="clean")
