"""The restatement of the view-graph calibration (tests/xm_vgcalib_numpy.py) on its own: no library, no GPU."""
import numpy as np
import pytest

import xm_vgcalib_numpy as vn

EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def graph():
    return vn.make_graph(12, 30, 1)


@pytest.fixture(scope="module")
def fits(graph):
    return dict(a=vn.calibrate_sequential(graph), a64=vn.calibrate_sequential(graph, T=np.float64, svd="lapack"), b=vn.calibrate_contract(graph))


def test_jacobi_svd_reconstructs():
    rng = np.random.default_rng(0)
    for _ in range(5):
        G = rng.standard_normal((3, 3))
        U, s, V = vn.jacobi_svd(G)
        assert s[0] >= s[1] >= s[2] >= 0
        assert float(np.abs((U * s) @ V.T - G).max()) < 64 * float(np.finfo(np.longdouble).eps) * float(s[0])
        assert np.allclose(np.asarray(s, dtype=np.float64), np.linalg.svd(G)[1], rtol=1e-13, atol=0)


def test_residual_at_the_truth(graph):
    """noise-free graph: the residual at the true focals is at rounding level.  F is given in float64, so even the longdouble restatement
    sees F's own rounding: its residual is bounded by 1e-9, the float64 one by 1e-6 (the d are differences of products, which cancel
    more the closer G's two leading singular values are); at the perturbed priors the residuals are 0.1 to 1"""
    k, ca, cb = vn.participating(graph)
    for T, svd, bound in ((np.longdouble, "jacobi", 1e-9), (np.float64, "lapack", 1e-6)):
        d = vn.setup_all(graph, T, svd)
        r = np.array([vn.residual_one(d[m], T(graph["truth"][ca[m]]), T(graph["truth"][cb[m]]), T)[:2] for m in range(len(k))], dtype=np.float64)
        print(f"max |r| at the truth in {np.dtype(T).name}: {np.abs(r).max():.3e}")
        assert np.abs(r).max() < bound
    d = vn.setup_all(graph)
    r0, _ = vn.residuals_contract(d, graph["focal0"][ca], graph["focal0"][cb])
    assert np.abs(r0).max() > 1e-2


def test_recovery(graph, fits):
    """the fit from priors off by factors 0.6 to 1.6 recovers the focals; the float64 forms stay within 16 times the longdouble restatement's
    own error"""
    err = {k: float(np.max(np.abs(v["focal_est"] - graph["truth"]) / graph["truth"])) for k, v in fits.items()}
    print("relative focal error:", err)
    assert err["a"] < 1e-6
    assert fits["a"]["stop"] in (vn.STOP_FUNCTION, vn.STOP_GRADIENT, vn.STOP_PARAMETER)
    assert err["a64"] <= 16 * err["a"] and err["b"] <= 16 * err["a"]
    assert fits["a"]["refined"].all() and (fits["a"]["pair_status"] == vn.VALID).all()


def test_sequential_equals_contract_exactly(graph):
    """(a) in float64 and (b) give the same residuals and flags, bit for bit, from the same d and focals"""
    k, ca, cb = vn.participating(graph)
    d = vn.setup_all(graph)
    rng = np.random.default_rng(3)
    for f in (graph["focal0"], graph["truth"], graph["truth"] * rng.uniform(0.05, 20.0, len(graph["truth"]))):
        ra = np.array([vn.residual_one(d[m], np.float64(f[ca[m]]), np.float64(f[cb[m]]), np.float64)[:2] for m in range(len(k))])
        rb, _ = vn.residuals_contract(d, f[ca], f[cb])
        assert np.array_equal(ra, rb)
        fa = np.array([r[0] * r[0] + r[1] * r[1] > 2.0 * 2.0 for r in ra])
        assert np.array_equal(fa, vn.flags_contract(rb))
    # and the records, gradient and product of the contract agree with the sequential linearisation
    slot = np.arange(len(graph["focal0"]))
    cost, raw, rec, g, A = vn.linearise_sequential(d, ca, cb, slot, graph["focal0"], np.float64(1e-2), np.float64)
    cb_, rb, recb = vn.records_contract(d, ca, cb, graph["focal0"], 1e-2)
    assert np.array_equal(rec, recb) and abs(cost - cb_) <= 64 * EPS * cost
    gb, dg = vn.camera_sums_contract(recb, ca, cb, slot, len(slot))
    assert np.allclose(g, gb, rtol=1e-13, atol=0) and np.allclose(np.diag(A), dg, rtol=1e-13, atol=0)
    x = rng.standard_normal(len(slot))
    assert np.allclose(A @ x + 0.5 * vn.clamp_diag(dg) * x, vn.product_contract(recb, ca, cb, slot, dg, 0.5, x), rtol=1e-12, atol=0)


def test_jacobian_is_the_derivative(graph):
    k, ca, cb = vn.participating(graph)
    d = vn.setup_all(graph, np.longdouble, "jacobi")
    T = np.longdouble
    for m in range(0, len(k), 7):
        fi, fj = T(graph["focal0"][ca[m]]), T(graph["focal0"][cb[m]])
        r0, r1, J = vn.residual_one(d[m], fi, fj, T)
        h = T(1e-3)     # truncation h^2 / f^2 = 1e-12 relative, rounding eps / h = 1e-16 absolute
        num = [(vn.residual_one(d[m], fi + h, fj, T)[0] - vn.residual_one(d[m], fi - h, fj, T)[0]) / (2 * h),
               (vn.residual_one(d[m], fi, fj + h, T)[0] - vn.residual_one(d[m], fi, fj - h, T)[0]) / (2 * h),
               (vn.residual_one(d[m], fi + h, fj, T)[1] - vn.residual_one(d[m], fi - h, fj, T)[1]) / (2 * h),
               (vn.residual_one(d[m], fi, fj + h, T)[1] - vn.residual_one(d[m], fi, fj - h, T)[1]) / (2 * h)]
        for a, b in zip(J, num):
            assert abs(a - b) <= 1e-6 * max(abs(a), abs(b)) + 1e-14   # (the entries are 1e-8 to 1e-3)


def test_same_camera_pairs():
    """two images per camera: pairs inside a camera use the one-parameter cost; the fit still recovers the focals"""
    g = vn.make_graph(4, 20, 7, images_per_camera=3)
    k, ca, cb = vn.participating(g)
    assert (ca == cb).any() and (ca != cb).any()
    a = vn.calibrate_sequential(g); b = vn.calibrate_contract(g)
    ea = float(np.max(np.abs(a["focal_est"] - g["truth"]) / g["truth"])); eb = float(np.max(np.abs(b["focal_est"] - g["truth"]) / g["truth"]))
    assert ea < 1e-6 and eb <= 16 * ea


def test_rule5_nothing_free(graph):
    g = dict(graph); g["has_prior"] = np.ones(len(graph["focal0"]), dtype=np.uint8)
    for out in (vn.calibrate_sequential(g), vn.calibrate_contract(g)):
        assert np.array_equal(out["focal"], g["focal0"]) and not out["refined"].any()
        assert (out["pair_status"] == vn.VALID).all() and not out["residual"].any() and out["iterations"] == 0
        assert (out["cam_status"] == vn.CAM_CONSTANT).all()


def test_rule6_rejection_and_flags():
    """a camera whose prior is 20 times its focal: the estimate comes back to the truth, the ratio 1/20 is below thres_lower_ratio, the camera
    keeps its prior and is not refined; the pair residuals use the estimate, so its pairs stay valid.  At 20 times the focal the Cauchy
    loss is nearly flat (r0 is 1 - 1/400) and with the default function_tolerance of 1e-5 the fit stops there after 4 iterations, at a
    ratio of 0.99: the case runs with function_tolerance 1e-9, with which it reaches the truth in 20"""
    g = vn.rejection_case()
    assert vn.calibrate_sequential(g)["cam_status"][3] == vn.CAM_REFINED          # the default tolerance: stalled next to the prior
    for out in (vn.calibrate_sequential(g, function_tolerance=1e-9), vn.calibrate_contract(g, function_tolerance=1e-9)):
        assert out["cam_status"][3] == vn.CAM_REJECTED and out["focal"][3] == g["focal0"][3] and out["refined"][3] == 0
        assert abs(out["focal_est"][3] - g["truth"][3]) < 1e-3 * g["truth"][3]
        assert (np.delete(out["cam_status"], 3) == vn.CAM_REFINED).all()
        assert (out["pair_status"] == vn.VALID).all() and np.abs(out["residual"]).max() < 1e-3
    # untouched camera, invalid and H pairs
    g2 = vn.make_graph(6, 10, 12)
    g2["valid_in"] = np.ones(10, dtype=np.uint8); g2["valid_in"][0] = 0
    g2["model"] = g2["model"].copy(); g2["model"][1] = vn.MODEL_H
    out = vn.calibrate_contract(g2)
    assert out["pair_status"][0] == vn.INVALID_IN and out["pair_status"][1] == vn.VALID and not out["residual"][:2].any()


def test_corrupted_pairs_are_invalidated():
    """10 % of the F replaced by random rank-2 matrices.  The residual of such a pair is of order 1 and seldom above the default
    thres_two_view_error of 2 (of 1200 seeds tried none had all ten above it), so the case sets the option to 0.5: the clean pairs end at
    1e-5 and below.  Exactly the corrupted pairs are invalidated, in the restatement and in the contract"""
    g = vn.make_graph(20, 100, 2)
    h, bad = vn.corrupt(g, 0.1, 0)
    for out in (vn.calibrate_sequential(h, thres_two_view_error=0.5), vn.calibrate_contract(h, thres_two_view_error=0.5)):
        assert np.array_equal(np.flatnonzero(out["pair_status"] == vn.TWO_VIEW_ERROR), bad)
        assert float(np.max(np.abs(out["focal_est"] - g["truth"]) / g["truth"])) < 1e-3


def test_bound_case():
    """the unprojected first step of the camera that moves down most ends below a bound put halfway: the projected candidate sits on the bound"""
    g = vn.make_graph(20, 100, 2)
    one = vn.calibrate_sequential(g, max_num_iterations=1)
    c = int(np.argmin(one["f_raw"] - g["focal0"]))
    assert one["accepted"] == 1 and one["f_raw"][c] < g["focal0"][c]
    lb = float(0.5 * (one["f_raw"][c] + g["focal0"][c]))
    assert one["f_raw"][c] < lb < g["focal0"].min() or lb < g["focal0"][c]
    for fit in (vn.calibrate_sequential, vn.calibrate_contract):
        b1 = fit(g, max_num_iterations=1, lower_bound=lb)
        if b1["accepted"]:
            assert b1["focal_est"][c] == lb
        assert (fit(g, lower_bound=lb)["focal_est"] >= lb).all()


def test_rule7_by_hand():
    g = vn.config_case()
    model, F = vn.update_config(g)
    want = g["model"].copy(); want[5] = vn.MODEL_E
    assert np.array_equal(model, want)
    changed = np.flatnonzero((F != g["F"]).any(axis=(1, 2)))
    assert np.array_equal(changed, [5])
    assert np.abs(F[5] / np.linalg.norm(F[5]) - g["F"][5]).max() < 64 * EPS       # the generator's F, up to its unit scale
    # with the flag the calibration starts from the updated pairs; camera 4 is the one free camera
    out = vn.calibrate_contract(g, update_config=True)
    assert np.array_equal(out["model"], want) and out["cam_status"][4] == vn.CAM_REFINED
    assert abs(out["focal_est"][4] - g["truth"][4]) < 1e-6 * g["truth"][4]
