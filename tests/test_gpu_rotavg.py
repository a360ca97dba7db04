"""xm_view_graph_rotations as a whole against the restatement of tests/xm_rotavg_numpy.py.  The reference is (a), the sequential form with an
exact solve (longdouble where its dense solve is small, float64 on the 300-pair hub and on SIMPLE2); the device may deviate from it by
max(16 e_b, 64 eps), e_b being the deviation of (b), the float64 contract with the device's PCG rule, from the same reference.  A deviation
is the largest absolute difference over an array divided by the reference's largest absolute entry."""
import functools

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


def within(what, gpu_v, b_v, a_v):
    e_gpu, e_b = rel(gpu_v, a_v), rel(b_v, a_v)
    bound = max(16.0 * e_b, 64.0 * EPS)
    print(f"{what}: e_b {e_b:.3e}, e_gpu {e_gpu:.3e}, ratio {e_gpu / bound:.3f}")
    return e_gpu <= bound


@pytest.fixture(scope="module")
def gpu(xmamd):
    xmamd.require_gpu()
    return xmamd


CASES = {"20/100 15 %": (20, 100, 1, 0.15), "20/100 25 %": (20, 100, 1, 0.25), "60/400 20 %": (60, 400, 1, 0.2)}


@functools.lru_cache(maxsize=None)
def references(case):
    """the graph, (a) in longdouble and (b), once per module"""
    n, npairs, seed, outliers = CASES[case]
    g = rn.make_graph(n, npairs, seed, 1.0, outliers)
    return g, rn.irls_sequential(g, LD), rn.irls_contract(g)


@functools.lru_cache(maxsize=None)
def hub_references():
    g = rn.star_ring(300, 7, 1.0, 0.1)
    return g, rn.irls_sequential(g), rn.irls_contract(g)


def _steps_clear_of_the_threshold(a, threshold=1e-3):
    return bool((np.abs(np.asarray(a["step_trace"], dtype=np.float64) - threshold) > 0.01 * threshold).all())


def _agrees(what, plan, a, b, g=None):
    assert plan.info["irls_iterations"] == a["iters"] == b["iters"] and plan.info["stop_reason"] == a["stop"] == b["stop"]
    assert plan.info["pcg_capped"] == 0 == b["pcg_capped"]
    ok = within(f"{what} step_trace", plan.step_trace, b["step_trace"], a["step_trace"])
    ok &= within(f"{what} rot", plan.rot, b["rot"], a["rot"])
    ok &= within(f"{what} angle_axis", plan.angle_axis, b["angle_axis"], a["angle_axis"])
    ok &= within(f"{what} residual", plan.residual, b["residual"], a["residual"])
    ok &= within(f"{what} weight", plan.weight, b["weight"], a["weight"])
    if g is not None:
        ea = rn.errors_deg(np.asarray(a["rot"], dtype=np.float64), g["truth"])
        ok &= within(f"{what} error against the truth", rn.errors_deg(plan.rot, g["truth"]), rn.errors_deg(b["rot"], g["truth"]), ea)
    return ok


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_the_restatement(gpu, case):
    g, a, b = references(case)
    assert a["stop"] == rn.STOP_STEP and _steps_clear_of_the_threshold(a)
    plan = gpu.view_graph_rotations(**rn.call_inputs(g))
    i = plan.info
    print(f"{case}: {i['irls_iterations']} IRLS iterations, {i['pcg_iterations']} PCG iterations (the contract: {b['pcg_iters']}), median error "
          f"{np.median(rn.errors_deg(g['rot0'], g['truth'])):.3f} -> {np.median(rn.errors_deg(plan.rot, g['truth'])):.3f} deg")
    assert i["pairs"] == g["pi"].size and i["registered"] == g["rot0"].shape[0] and i["fixed_image"] == 0 and i["pcg_capped"] == 0
    assert i["cams_heavy"] == 0 and i["max_incidences"] == int(np.bincount(np.concatenate([g["pi"], g["pj"]])).max())
    assert _agrees(case, plan, a, b, g)
    # the same separation of the weights as (a)'s (tests/test_rotavg_numpy.py), and the error against the truth at least halved
    assert (plan.weight[g["wrong"]] < 1.0).all() and (plan.weight[~g["wrong"]] > 10.0).all()
    assert np.median(rn.errors_deg(plan.rot, g["truth"])) <= 0.5 * np.median(rn.errors_deg(g["rot0"], g["truth"]))
    # the outputs fit together: rot is Exp of angle_axis, and the residuals are those of rot
    assert np.max(np.abs(plan.rot - rn.exp_batch(plan.angle_axis))) <= 8 * EPS
    Q = rn.mul_batch(np.transpose(plan.rot[g["pj"]], (0, 2, 1)), rn.mul_batch(g["Rrel"], plan.rot[g["pi"]]))
    assert np.max(np.abs(plan.residual + rn.log_batch(Q))) <= 64 * EPS * np.pi


def test_noise_free_start_stays(gpu):
    g = rn.make_graph(20, 100, 5, 0.0, 0.0)
    a, b = rn.irls_sequential(g, LD), rn.irls_contract(g)
    plan = gpu.view_graph_rotations(**rn.call_inputs(g))
    assert plan.info["irls_iterations"] == 1 == a["iters"] and plan.info["stop"] == "step_tolerance" and plan.step_trace[0] < 1e-12
    assert within("noise-free rot", plan.rot, b["rot"], a["rot"])
    assert within("noise-free rot against the start", plan.rot, b["rot"], g["rot0"])


def test_heavy_camera(gpu):
    g, a, b = hub_references()
    assert a["stop"] == rn.STOP_STEP and _steps_clear_of_the_threshold(a)
    plan = gpu.view_graph_rotations(**rn.call_inputs(g))
    assert plan.info["cams_heavy"] == 1 and plan.info["max_incidences"] == 300
    assert _agrees("hub of 300", plan, a, b, g)
    assert (plan.weight[g["wrong"]] < 1.0).all() and (plan.weight[~g["wrong"]] > 10.0).all()


@pytest.mark.parametrize("kind", ["graph", "hub"])
def test_two_calls_give_the_same_bytes(gpu, kind):
    g = references("20/100 25 %")[0] if kind == "graph" else hub_references()[0]
    p, q = gpu.view_graph_rotations(**rn.call_inputs(g)), gpu.view_graph_rotations(**rn.call_inputs(g))
    for k in ("rot", "angle_axis", "residual", "weight", "step_trace"):
        assert getattr(p, k).tobytes() == getattr(q, k).tobytes()
    drop = ("seconds_index", "seconds_kernels", "seconds_download")
    assert {k: v for k, v in p.info.items() if k not in drop} == {k: v for k, v in q.info.items() if k not in drop}
    out = [gpu.view_graph_rotations_probe(**rn.call_inputs(g), angle_axis=p.angle_axis, x=0.01 * p.angle_axis) for _ in range(2)]
    assert all(np.asarray(out[0][k]).tobytes() == np.asarray(out[1][k]).tobytes() for k in out[0])


def test_chain_caps_the_pcg(gpu):
    """a chain of 600 cameras, two IRLS iterations: both solves stop at the PCG's cap of 500 iterations (tests/test_rotavg_numpy.py: the
    contract's relative residual there is far above the tolerance), and the call goes on with what the capped solves gave"""
    g = rn.chain(600, 3)
    b = rn.irls_contract(g, max_iters=2)
    plan = gpu.view_graph_rotations(**rn.call_inputs(g), max_num_irls_iterations=2)
    i = plan.info
    print(f"chain of 600: {i['irls_iterations']} IRLS iterations, {i['pcg_iterations']} PCG iterations, {i['pcg_capped']} capped, stop {i['stop']}")
    assert i["irls_iterations"] == 2 and i["pcg_iterations"] == 1000 == b["pcg_iters"] and i["pcg_capped"] == 2 == b["pcg_capped"]
    assert i["stop_reason"] == b["stop"]
    assert all(np.isfinite(getattr(plan, k)).all() for k in ("rot", "angle_axis", "residual", "weight", "step_trace"))


def test_fixed_image_is_honoured(gpu):
    g = references("20/100 15 %")[0]
    a, b = rn.irls_sequential(g, LD, fixed_image=7), rn.irls_contract(g, fixed_image=7)
    plan = gpu.view_graph_rotations(**rn.call_inputs(g), fixed_image=7)
    assert plan.info["fixed_image"] == 7 == a["fixed"]
    assert _agrees("fixed 7", plan, a, b, g)
    # the fixed camera stays at its start (the gauge rows hold it; the pairs' terms do not see a common turn)
    assert within("the fixed camera against its start", plan.rot[7], b["rot"][7], g["rot0"][7])
    default = gpu.view_graph_rotations(**rn.call_inputs(g))
    assert within("camera 0 against its start", default.rot[0], references("20/100 15 %")[2]["rot"][0], g["rot0"][0])
    assert rel(default.rot[7], g["rot0"][7]) > 1e-6             # ... and a camera that is not fixed moves
    reg = np.ones(20, dtype=np.uint8); reg[0] = 0
    assert gpu.view_graph_rotations(**dict(rn.call_inputs(g), registered=reg)).info["fixed_image"] == 1


def test_no_participating_pair_is_a_no_op(gpu):
    g = dict(references("20/100 15 %")[0])
    g["valid_in"] = np.zeros(100, dtype=np.uint8)
    plan = gpu.view_graph_rotations(**rn.call_inputs(g))
    assert plan.info["stop"] == "nothing" and plan.info["irls_iterations"] == 0 and plan.info["pairs"] == 0 and plan.step_trace.size == 0
    assert np.array_equal(plan.rot, g["rot0"]) and not plan.residual.any() and not plan.weight.any()
    assert np.max(np.abs(plan.angle_axis - rn.log_batch(g["rot0"]))) <= 16 * EPS * np.pi


def test_half_norm_runs_and_stops_as_the_restatement(gpu):
    g = references("20/100 15 %")[0]
    a = rn.irls_sequential(g, LD, weight_type=rn.HALF_NORM, max_iters=30)
    b = rn.irls_contract(g, weight_type=rn.HALF_NORM, max_iters=30)
    assert _steps_clear_of_the_threshold(a)
    plan = gpu.view_graph_rotations(**rn.call_inputs(g), weight_type="half_norm", max_num_irls_iterations=30)
    print(f"half norm: {plan.info['irls_iterations']} iterations, stop {plan.info['stop']}, steps {np.array2string(plan.step_trace, precision=6)}")
    assert plan.info["irls_iterations"] == a["iters"] and plan.info["stop_reason"] == a["stop"]
    assert _agrees("half norm", plan, a, b)
    capped = gpu.view_graph_rotations(**rn.call_inputs(g), weight_type="half_norm", max_num_irls_iterations=2)
    assert capped.info["stop"] == "max_iterations" and capped.info["irls_iterations"] == 2
    assert np.array_equal(capped.step_trace, plan.step_trace[:2])
    # an exactly zero residual: the weight is infinite, the call ends before its first solve with the start as it came
    z = dict(rot0=np.tile(np.eye(3), (4, 1, 1)), pi=np.array([0, 1, 2, 0], dtype=np.int32), pj=np.array([1, 2, 3, 3], dtype=np.int32),
             Rrel=np.tile(np.eye(3), (4, 1, 1)))
    stop = gpu.view_graph_rotations(**z, weight_type="half_norm")
    ref = rn.irls_sequential(dict(z, registered=None, valid_in=None), weight_type=rn.HALF_NORM)
    assert stop.info["stop"] == "nonfinite_weight" and stop.info["stop_reason"] == ref["stop"] and stop.info["irls_iterations"] == 0 == ref["iters"]
    assert np.array_equal(stop.rot, z["rot0"]) and not stop.weight.any() and not stop.residual.any() and not stop.angle_axis.any()
    assert gpu.view_graph_rotations(**z).info["stop"] == "step_tolerance"


def test_simple2_rotations_go_into_pass_b(gpu):
    """the SIMPLE2-derived view graph: the plan's rot is pass B's rot as it is, and pass B decides every pair as with (a)'s rotations"""
    import xm_viewgraph_numpy as vn
    g = rn.simple2_graph()
    a, b = rn.irls_sequential(g), rn.irls_contract(g)
    assert a["stop"] == rn.STOP_STEP and _steps_clear_of_the_threshold(a)
    plan = gpu.view_graph_rotations(**rn.call_inputs(g))
    img = np.flatnonzero(g["registered"])
    print(f"SIMPLE2-derived: {plan.info['pairs']} pairs of {plan.info['registered']} images, {plan.info['irls_iterations']} iterations, "
          f"{plan.info['pcg_iterations']} PCG iterations, {plan.info['cams_heavy']} heavy cameras (most incidences {plan.info['max_incidences']}); median "
          f"error {np.median(rn.errors_deg(g['rot0'], g['truth'], img)):.4f} -> {np.median(rn.errors_deg(plan.rot, g['truth'], img)):.4f} deg")
    assert _agrees("SIMPLE2", plan, a, b)
    assert plan.info["cams_heavy"] > 0
    status = []
    for rot in (plan.rot, np.asarray(a["rot"], dtype=np.float64), g["rot0"]):
        args, kw = vn.call_args(vn.next_pass(g["case"], g["passA"], rot))
        status.append(gpu.view_graph_filter(*args, **kw).pair_status)
    assert np.array_equal(status[0], status[1])
    turned = int(np.sum(status[0] == gpu.VG_ROTATION))
    print(f"pass B: {turned} pairs dropped by the rotation test with the refined rotations, {int(np.sum(status[2] == gpu.VG_ROTATION))} with the start")
    assert turned > 0
