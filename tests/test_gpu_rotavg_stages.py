"""The robust rotation averaging's kernels stage by stage through the test export xm_view_graph_rotations_probe, against the sequential
restatement (a) of tests/xm_rotavg_numpy.py in longdouble.  Stage bound: e_gpu <= max(16 e_ref, 64 eps_f64), e_ref being the same
restatement's error in float64 against the same reference; an error is the largest absolute deviation over the array divided by the
array's largest absolute entry.  Every comparison prints `ROTAVG_STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s): the table of
profiles/r30_rotavg_stage_errors.txt.

Which kernel an output pins: rot -> rav_exp_kernel; residual, weight -> rav_pair_kernel; gauge, rhs, diagonal -> rav_cam_kernel (and
rav_log_kernel for the fixed camera's start); product -> rav_camx_kernel; angle_axis_out, step -> rav_update_kernel, ba_reduce_kernel."""
import numpy as np
import pytest

import xm_rotavg_numpy as rn

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


def rel(x, ref):
    ref = np.asarray(ref, dtype=LD); x = np.asarray(x, dtype=LD)
    s = float(np.max(np.abs(ref))) if ref.size else 0.0
    return float(np.max(np.abs(x - ref))) / s if s > 0 else float(np.max(np.abs(x), initial=0.0))


def stage_ok(case, what, gpu_v, f64_v, ref_v):
    e_gpu, e_ref = rel(gpu_v, ref_v), rel(f64_v, ref_v)
    bound = max(16.0 * e_ref, 64.0 * EPS)
    print(f"ROTAVG_STAGE_ERR {case} {what}: e_ref {e_ref:.3e}, e_gpu {e_gpu:.3e}, ratio {e_gpu / bound:.3f}")
    return np.isfinite(np.asarray(gpu_v, dtype=np.float64)).all() and e_gpu <= bound


@pytest.fixture(scope="module")
def gpu(xmamd):
    xmamd.require_gpu()
    return xmamd


def _state(g, seed, spread=0.05):
    """a state that is not the solution: Log of the start plus a perturbation, and a step of the same size"""
    rng = np.random.default_rng(seed)
    n = g["rot0"].shape[0]
    aa = np.stack([rn.rot_to_aa(R) for R in g["rot0"]]) + spread * rng.standard_normal((n, 3))
    return aa, spread * rng.standard_normal((n, 3))


def _compare(gpu, case, g, aa, x, quantities, weight_in=None, weight_type=rn.GEMAN_MCCLURE, fixed_image=-1):
    out = gpu.view_graph_rotations_probe(**rn.call_inputs(g), angle_axis=aa, x=x, weight_in=weight_in, weight_type=weight_type, fixed_image=fixed_image)
    ref = rn.stages_sequential(g, aa, x, LD, weight_in, weight_type, fixed_image=fixed_image)
    f64 = rn.stages_sequential(g, aa, x, np.float64, weight_in, weight_type, fixed_image=fixed_image)
    ok = True
    for q in quantities:
        ok &= bool(stage_ok(case, q, out[q], f64[q], ref[q]))
    return ok, out, ref


ALL = ("rot", "residual", "gauge", "weight", "rhs", "diagonal", "product", "angle_axis_out", "step")


def _edge_vectors():
    """angle-axis vectors on every branch of rules 3 and 4: the trace branch, each diagonal branch with w of either sign, angle 0, the
    first-order branch at norm 1e-13, and up to pi - 1e-3"""
    rng = np.random.default_rng(11)
    out = [np.zeros(3), 1e-13 * np.array([0.6, -0.8, 0.0]), 1e-13 * np.array([0.0, 0.0, -1.0]), np.array([2e-12, 0.0, 0.0])]
    for angle in (1e-6, 0.3, 1.2, 2.2, 2.6, 3.0, np.pi - 1e-3):
        for k in range(3):
            for s in (1.0, -1.0):
                u = s * np.eye(3)[k] + 0.05 * rng.standard_normal(3)
                out.append(angle * u / np.linalg.norm(u))
        u = rng.standard_normal(3)
        out.append(angle * u / np.linalg.norm(u))
    return np.array(out)


def _edge_graph():
    """20 cameras / 100 pairs whose states, pair rotations R_2^T Rrel R_1 and updated states all run through _edge_vectors"""
    E = _edge_vectors()
    g = rn.make_graph(20, 100, 6, 1.0, 0.0)
    aa = np.stack([E[(3 * i) % len(E)] for i in range(20)])
    target = np.stack([E[(3 * i + 1) % len(E)] for i in range(20)])
    R = [rn.aa_to_rot(a.astype(LD), LD) for a in aa]
    Rrel = np.empty((100, 3, 3))
    for m in range(100):
        c = E[m % len(E)].astype(LD)
        Rrel[m] = np.asarray(rn.mul3(R[g["pj"][m]], rn.mul3(rn.aa_to_rot(c, LD), R[g["pi"][m]].T.copy())), dtype=np.float64)
    x = np.stack([-rn.rot_to_aa(rn.mul3(R[i].T.copy(), rn.aa_to_rot(target[i].astype(LD), LD)), LD) for i in range(20)]).astype(np.float64)
    g = dict(g, Rrel=np.ascontiguousarray(Rrel))
    return g, aa, x, E, target


def test_exp_log_edge_cases(gpu):
    g, aa, x, E, target = _edge_graph()
    ok, out, ref = _compare(gpu, "edges", g, aa, x, ALL)
    assert ok
    # the branches were met: residuals run through -E, updated states through the targets
    assert np.max(np.abs(out["residual"] + np.stack([E[m % len(E)] for m in range(100)]))) < 1e-12
    assert np.max(np.abs(out["angle_axis_out"] - target)) < 1e-12
    branches = {rn.rot_to_quat(rn.mul3(out["rot"][g["pj"][m]].T.copy(), rn.mul3(g["Rrel"][m], out["rot"][g["pi"][m]])))[1] for m in range(100)}
    assert branches == {0, 1, 2, 3}
    # near pi the vector itself is compared above; here also through Exp(Log(R)), which does not care on which side of pi a result lands
    near = np.flatnonzero(np.linalg.norm(out["residual"], axis=1) > 2.9)
    assert near.size >= 3
    Rg = np.stack([rn.aa_to_rot(v) for v in out["residual"][near]])
    Rf = np.stack([rn.aa_to_rot(np.asarray(v, dtype=np.float64)) for v in rn.stages_sequential(g, aa, x, np.float64)["residual"][near]])
    Rr = np.stack([np.asarray(rn.aa_to_rot(v, LD)) for v in ref["residual"][near]])
    assert stage_ok("edges", "Exp(residual) near pi", Rg, Rf, Rr)
    # angle 0 and the first-order branch come out exactly as rule 3 states them
    assert np.array_equal(out["rot"][0], np.eye(3))
    a = aa[np.flatnonzero(np.abs(np.linalg.norm(aa, axis=1) - 1e-13) < 1e-15)[0]]
    i = int(np.flatnonzero((aa == a).all(axis=1))[0])
    assert np.array_equal(out["rot"][i], np.array([[1.0, -a[2], a[1]], [a[2], 1.0, -a[0]], [-a[1], a[0], 1.0]]))


@pytest.mark.parametrize("weight_type", [rn.GEMAN_MCCLURE, rn.HALF_NORM])
def test_weights_of_both_types(gpu, weight_type):
    g = rn.make_graph(20, 100, 1, 1.0, 0.15)
    aa, x = _state(g, 3, 0.01)
    ok, out, _ = _compare(gpu, f"graph weight_type {weight_type}", g, aa, x, ALL, weight_type=weight_type)
    assert ok and (out["weight"] > 0).all()


def test_sums_on_the_graph(gpu):
    g = rn.make_graph(20, 100, 1, 1.0, 0.15)
    aa, x = _state(g, 4)
    w = np.random.default_rng(5).uniform(1e-3, 130.0, 100)
    assert _compare(gpu, "graph weight_in", g, aa, x, ALL, weight_in=w)[0]
    ok, out, _ = _compare(gpu, "graph fixed 7", g, aa, x, ALL, weight_in=w, fixed_image=7)
    assert ok
    base = gpu.view_graph_rotations_probe(**rn.call_inputs(g), angle_axis=aa, x=x, weight_in=w)
    assert out["diagonal"][7] == base["diagonal"][7] + 1.0 and base["diagonal"][0] == out["diagonal"][0] + 1.0


def test_sums_by_incidence_count(gpu):
    """a hub with 1 incidence, with the most a thread walks less one, exactly that, one more (a workgroup), and 300"""
    light = gpu.view_graph_rotations_limits()["light_incidences"]
    assert light == 64
    for leaves in (1, light - 1, light, light + 1, 300):
        g = rn.star(leaves, 20 + leaves % 7)
        aa, x = _state(g, leaves)
        w = np.random.default_rng(leaves).uniform(1e-3, 130.0, leaves)
        assert _compare(gpu, f"star {leaves}", g, aa, x, ALL, weight_in=w)[0]
    g = rn.star_ring(300, 7, 1.0, 0.1)
    aa, x = _state(g, 9)
    assert _compare(gpu, "star_ring 300", g, aa, x, ALL)[0]


def test_unregistered_images_and_invalid_pairs_hold_zero(gpu):
    g = rn.make_graph(20, 100, 2, 1.0, 0.1)
    reg = np.ones(20, dtype=np.uint8); reg[[0, 6, 13]] = 0
    val = np.ones(100, dtype=np.uint8); val[[20, 33, 47, 80, 99]] = 0
    g = dict(g, registered=reg, valid_in=val)
    aa, x = _state(g, 6)
    aa[6] = np.nan; x[13] = 7.0                                   # what an unregistered image carries is ignored
    ok, out, ref = _compare(gpu, "partial", g, aa, x, ALL)
    assert ok
    p = rn.problem(g)
    assert p["fixed"] == 1 and p["k"].size < 95
    out_pairs = np.setdiff1d(np.arange(100), p["k"])
    assert not out["residual"][out_pairs].any() and not out["weight"][out_pairs].any()
    for q in ("rot", "rhs", "diagonal", "product", "angle_axis_out"):
        assert not out[q][[0, 6, 13]].any()
    assert (out["diagonal"][reg != 0] > 0).all()


def test_no_pair(gpu):
    g = rn.make_graph(5, 8, 3, 1.0, 0.0)
    g = dict(g, valid_in=np.zeros(8, dtype=np.uint8))
    out = gpu.view_graph_rotations_probe(**rn.call_inputs(g), angle_axis=np.ones((5, 3)), x=np.ones((5, 3)))
    assert all(not np.any(out[k]) for k in ALL)
