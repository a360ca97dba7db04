"""The whole call xm_view_graph_calibrate on the device against the restatement of tests/xm_vgcalib_numpy.py: (a) the sequential longdouble
restatement is the reference, (b) the float64 contract with the device's PCG rule gives the error a float64 implementation may have."""
import numpy as np
import pytest

import xm_vgcalib_numpy as vn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(xmamd):
    xmamd.require_gpu()
    return xmamd


@pytest.fixture(scope="module")
def graph():
    return vn.make_graph(20, 100, 2)


@pytest.fixture(scope="module")
def corrupted(graph):
    """10 % of the F replaced by random rank-2 matrices; thres_two_view_error = 0.5 (tests/test_vgcalib_numpy.py says why and checks on the
    CPU that the restatement alone invalidates exactly the corrupted pairs)"""
    h, bad = vn.corrupt(graph, 0.1, 0)
    return h, bad, dict(thres_two_view_error=0.5)


def run(gpu, g, **kw):
    extra = {k: g[k] for k in ("Rrel", "trel")} if kw.get("update_config") else {}
    return gpu.view_graph_calibrate(**vn.call_inputs(g), **extra, **kw)


def trace_deviation(t, ref):
    """largest difference of two cost traces over their common length, relative to the initial cost"""
    n = min(len(t), len(ref))
    return float(np.max(np.abs(np.asarray(t[:n], dtype=np.longdouble) - ref[:n])) / ref[0])


def rel_err(f, truth):
    return float(np.max(np.abs(f - truth) / truth))


def check_against_restatement(gpu, g, opts, what):
    """cost trace and recovered focals: the device stays within 16 times what (b) deviates from (a), and within 16 times (a)'s own error"""
    a = vn.calibrate_sequential(g, **opts); b = vn.calibrate_contract(g, **opts)
    dev = run(gpu, g, want_d=True, **opts)
    e_b, e_dev = trace_deviation(b["cost_trace"], a["cost_trace"]), trace_deviation(dev.cost_trace, a["cost_trace"])
    err_a, err_b, err_dev = rel_err(a["focal_est"], g["truth"]), rel_err(b["focal_est"], g["truth"]), rel_err(dev.focal_est, g["truth"])
    print(f"{what}: cost trace deviation from the longdouble restatement: contract {e_b:.3e}, device {e_dev:.3e}; trace lengths "
          f"{len(a['cost_trace'])} / {len(b['cost_trace'])} / {len(dev.cost_trace)}; relative focal error: restatement {err_a:.3e}, contract {err_b:.3e}, "
          f"device {err_dev:.3e}; iterations {dev.info['iterations']}, PCG {dev.info['pcg_iterations']}, stop {dev.info['stop']}")
    assert abs(len(dev.cost_trace) - len(a["cost_trace"])) <= 1              # (a stop decided at rounding level may move by one step)
    assert dev.cost_trace[0] == dev.info["initial_cost"] and dev.cost_trace[-1] == dev.info["final_cost"]
    assert e_dev <= 16.0 * e_b
    assert err_dev <= 16.0 * err_a
    # rule 6 from the device's own d and estimates: the contract's bits
    k, ca, cb = vn.participating(g)
    r, _ = vn.residuals_contract(dev.d[k], dev.focal_est[ca], dev.focal_est[cb])
    assert np.array_equal(dev.residual[k], r)
    flags = vn.flags_contract(r, opts.get("thres_two_view_error", 2.0))
    assert np.array_equal(dev.pair_status[k] == gpu.VGC_TWO_VIEW_ERROR, flags) and dev.info["pairs_invalidated"] == int(flags.sum())
    assert np.array_equal(dev.pair_status, a["pair_status"]) and np.array_equal(dev.cam_status, a["cam_status"])
    return dev, a


def test_noise_free_graph(gpu, graph):
    dev, a = check_against_restatement(gpu, graph, {}, "noise-free graph")
    assert dev.refined.all() and dev.valid.all() and np.array_equal(dev.focal, dev.focal_est)
    assert dev.info["pairs"] == 100 and dev.info["cams_free"] == 20 and dev.info["cams_constant"] == 0 and dev.info["pairs_same_camera"] == 0
    assert dev.info["stop"] in ("function_tolerance", "gradient_tolerance", "parameter_tolerance")


def test_corrupted_graph(gpu, corrupted):
    h, bad, opts = corrupted
    dev, a = check_against_restatement(gpu, h, opts, "graph with 10 % random rank-2 F")
    assert np.array_equal(np.flatnonzero(dev.pair_status == gpu.VGC_TWO_VIEW_ERROR), bad)      # every corrupted pair and no clean one


def test_rejection(gpu):
    """tests/test_vgcalib_numpy.py: test_rule6_rejection_and_flags says why function_tolerance is 1e-9 here"""
    g = vn.rejection_case()
    a = vn.calibrate_sequential(g, function_tolerance=1e-9)
    dev = run(gpu, g, function_tolerance=1e-9)
    assert a["cam_status"][3] == vn.CAM_REJECTED
    assert dev.cam_status[3] == gpu.VGC_CAM_REJECTED and dev.focal[3] == g["focal0"][3] and dev.refined[3] == 0 and dev.info["cams_rejected"] == 1
    assert rel_err(dev.focal_est, g["truth"]) <= 16.0 * rel_err(a["focal_est"], g["truth"])
    assert dev.valid.all() and np.abs(dev.residual).max() < 1e-3                  # the residuals use the estimate, not the prior kept
    assert (np.delete(dev.cam_status, 3) == gpu.VGC_CAM_REFINED).all()


def test_lower_bound(gpu, graph):
    """the bound of tests/test_vgcalib_numpy.py: test_bound_case: the restatement's unprojected first step ends below it"""
    one = vn.calibrate_sequential(graph, max_num_iterations=1)
    c = int(np.argmin(one["f_raw"] - graph["focal0"]))
    lb = float(0.5 * (one["f_raw"][c] + graph["focal0"][c]))
    assert one["accepted"] == 1 and one["f_raw"][c] < lb
    a1 = vn.calibrate_sequential(graph, max_num_iterations=1, lower_bound=lb)
    d1 = run(gpu, graph, max_num_iterations=1, lower_bound=lb)
    assert d1.info["accepted"] == a1["accepted"] and d1.info["stop"] == "max_iterations"
    if a1["accepted"]:
        assert d1.focal_est[c] == lb
    full = run(gpu, graph, lower_bound=lb)
    assert (full.focal_est >= lb).all()


def test_early_return(gpu, graph):
    g = dict(graph); g["has_prior"] = np.ones(20, dtype=np.uint8)
    dev = run(gpu, g, want_d=True)
    assert np.array_equal(dev.focal, g["focal0"]) and np.array_equal(dev.focal_est, g["focal0"]) and not dev.refined.any()
    assert dev.valid.all() and not dev.residual.any() and not dev.d.any() and len(dev.cost_trace) == 0
    assert dev.info["iterations"] == 0 and dev.info["cams_free"] == 0 and dev.info["cams_constant"] == 20 and dev.info["pairs_invalidated"] == 0
    assert np.array_equal(dev.F, g["F"]) and np.array_equal(dev.model, g["model"])


def test_priors_stay(gpu, graph):
    g = dict(graph); g["has_prior"] = graph["has_prior"].copy(); g["has_prior"][[0, 7, 13]] = 1
    g["focal0"] = graph["focal0"].copy(); g["focal0"][[0, 7, 13]] = graph["truth"][[0, 7, 13]]
    dev = run(gpu, g)
    a = vn.calibrate_sequential(g)
    assert np.array_equal(dev.focal[[0, 7, 13]], g["focal0"][[0, 7, 13]]) and np.array_equal(dev.focal_est[[0, 7, 13]], g["focal0"][[0, 7, 13]])
    assert (dev.cam_status[[0, 7, 13]] == gpu.VGC_CAM_CONSTANT).all() and not dev.refined[[0, 7, 13]].any()
    assert dev.info["cams_free"] == 17 and dev.info["cams_constant"] == 3
    assert rel_err(dev.focal_est, g["truth"]) <= 16.0 * rel_err(a["focal_est"], g["truth"])


def test_update_config(gpu):
    g = vn.config_case()
    model, F = vn.update_config(g)
    dev = run(gpu, g, update_config=True)
    assert np.array_equal(dev.model, model) and np.array_equal(dev.F, F)          # exactly
    assert dev.info["pairs_flipped"] == 1 and dev.model[5] == gpu.VG_MODEL_E and not np.array_equal(dev.F[5], g["F"][5])
    assert dev.cam_status[4] == gpu.VGC_CAM_REFINED and abs(dev.focal_est[4] - g["truth"][4]) < 1e-6 * g["truth"][4]
    g2 = dict(g); g2["has_prior"] = np.ones(7, dtype=np.uint8)                     # rule 5 behind rule 7: the pair still flips
    m2, F2 = vn.update_config(g2)
    d2 = run(gpu, g2, update_config=True)
    assert np.array_equal(d2.model, m2) and np.array_equal(d2.F, F2) and not d2.refined.any() and d2.info["iterations"] == 0
    plain = run(gpu, g)
    assert np.array_equal(plain.model, g["model"]) and np.array_equal(plain.F, g["F"])


def test_two_calls_same_bytes(gpu, corrupted):
    h, bad, opts = corrupted
    big = vn.make_graph(301, 300, 4, pairs=[(0, j) for j in range(1, 301)])        # a heavy camera
    for g, o in ((h, opts), (big, {})):
        x, y = run(gpu, g, want_d=True, **o), run(gpu, g, want_d=True, **o)
        for k in ("focal", "focal_est", "refined", "cam_status", "pair_status", "residual", "d", "cost_trace"):
            assert getattr(x, k).tobytes() == getattr(y, k).tobytes()
        assert x.info["pcg_iterations"] == y.info["pcg_iterations"] and x.info["iterations"] == y.info["iterations"]
    assert x.info["cams_heavy"] == 1 and x.info["max_incidences"] == 300


def test_simple2_into_view_graph_filter(gpu):
    """the SIMPLE2-derived case: F from its relative poses and intrinsics for the E and F pairs, priors off by 0.7 to 1.4; the call's focals
    and flags go into view_graph_filter pass A, whose pair statuses equal those from the true focals"""
    g, c = vn.simple2_case()
    plan = run(gpu, g)
    print("SIMPLE2-derived:", plan.info, "relative focal error", rel_err(plan.focal_est, c["focal"]))
    assert plan.refined.all() and np.array_equal(plan.valid, c["valid_in"])
    matches = (c["moff"], c["f1"], c["f2"])
    kw = dict(Rrel=c["Rrel"], trel=c["trel"], FH=c["FH"])
    true = gpu.view_graph_filter(c["foff"], c["xy"], c["pi"], c["pj"], c["model"], matches, focal=c["focal"], Kinv=c["Kinv"], valid_in=c["valid_in"], **kw)
    got = gpu.view_graph_filter(c["foff"], c["xy"], c["pi"], c["pj"], c["model"], matches, focal=plan.focal_per_image(), Kinv=plan.Kinv(),
                                valid_in=plan.valid, **kw)
    assert np.array_equal(got.pair_status, true.pair_status) and np.array_equal(got.registered, true.registered)
