"""The view-graph calibration's kernels stage by stage through the test export xm_view_graph_calibrate_probe: the set-up's d against a
longdouble Jacobi SVD, residuals bit for bit against the numpy contract, cost, gradient, diagonal and product against the longdouble
restatement.  Stage bound: e_gpu <= max(16 e_ref, 64 eps_f64), e_ref being the float64 restatement's error against the same reference."""
import numpy as np
import pytest

import xm_vgcalib_numpy as vn

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


def stage_ok(what, e_gpu, e_ref):
    print(f"{what}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e}")
    return e_gpu <= max(16.0 * e_ref, 64.0 * EPS)


def rel(x, ref):
    ref = np.asarray(ref, dtype=LD); x = np.asarray(x, dtype=LD)
    s = float(np.max(np.abs(ref))) if ref.size else 0.0
    return float(np.max(np.abs(x - ref))) / s if s > 0 else float(np.max(np.abs(x), initial=0.0))


def star(leaves, seed):
    """camera 0 in every pair, `leaves` other cameras with one pair each: incidence counts `leaves` and 1"""
    return vn.make_graph(leaves + 1, leaves, seed, pairs=[(0, j) for j in range(1, leaves + 1)])


@pytest.fixture(scope="module")
def gpu(xmamd):
    xmamd.require_gpu()
    return xmamd


@pytest.fixture(scope="module")
def graph():
    return vn.make_graph(20, 100, 2)


def _probe(gpu, g, focal=None, **kw):
    return gpu.view_graph_calibrate_probe(**vn.call_inputs(g), focal=g["focal0"] if focal is None else focal, **kw)


def _close_svs():
    """pairs whose two leading singular values are 1 % apart: principal points 0, so G = F = U diag(1, 0.99, 0) V^T"""
    rng = np.random.default_rng(9)
    g = vn.make_graph(4, 6, 9)
    g["pp"] = np.zeros_like(g["pp"])
    for k in range(6):
        U, V = vn.random_rotation(rng), vn.random_rotation(rng)
        g["F"][k] = (U * np.array([1.0, 0.99, 0.0])) @ V.T
    return g


def _scaled(graph, s):
    g = dict(graph)
    g["F"] = graph["F"] * s
    return g


D_CASES = {"graph": lambda graph: graph, "F x 1e-6": lambda graph: _scaled(graph, 1e-6), "F x 1e6": lambda graph: _scaled(graph, 1e6),
           "singular values 1 % apart": lambda graph: _close_svs()}


@pytest.mark.parametrize("case", sorted(D_CASES))
def test_setup_d(gpu, graph, case):
    g = D_CASES[case](graph)
    ref = vn.normalise_d(vn.setup_all(g, LD, "jacobi"))
    lap = vn.normalise_d(vn.setup_all(g, np.float64, "lapack"))
    dev = vn.normalise_d(_probe(gpu, g)["d"])
    assert np.isfinite(dev).all()
    assert stage_ok(f"d ({case})", float(np.max(np.abs(dev.astype(LD) - ref))), float(np.max(np.abs(lap.astype(LD) - ref))))


def test_residuals_bit_for_bit(gpu, graph):
    """the device's own d and the given focals fed to the contract: the same bits, and with them the same flags of rule 6"""
    k, ca, cb = vn.participating(graph)
    rng = np.random.default_rng(4)
    flagged = 0
    for focal in (graph["focal0"], graph["truth"], graph["truth"] * 10.0 ** rng.uniform(-1.5, 1.5, 20), graph["truth"] * rng.uniform(0.5, 2.0, 20)):
        out = _probe(gpu, graph, focal)
        r, _ = vn.residuals_contract(out["d"][k], focal[ca], focal[cb])
        assert np.array_equal(out["residual"][k], r)
        flagged += int(vn.flags_contract(out["residual"][k]).sum())
    assert flagged > 0                            # (a focal at a thirtieth of the truth: r0 near 1 - 900)


def _sums_against_longdouble(gpu, g, what, focal=None, d_in=None, mu=0.37):
    focal = g["focal0"] if focal is None else focal
    rng = np.random.default_rng(8)
    x = rng.standard_normal(len(focal))
    out = _probe(gpu, g, focal, x=x, mu=mu, d_in=d_in)
    k, ca, cb = vn.participating(g)
    touched, free, slot = vn._unknowns(g, ca, cb)
    fc = np.flatnonzero(free)
    d = out["d"][k]
    ref = vn.linearise_sequential(d.astype(LD), ca, cb, slot, focal.astype(LD), LD(1e-2), LD, dense=False)
    f64 = vn.linearise_sequential(d, ca, cb, slot, focal, np.float64(1e-2), np.float64, dense=False)
    r, _ = vn.residuals_contract(d, focal[ca], focal[cb])
    assert np.array_equal(out["residual"][k], r)
    ok = stage_ok(f"{what}: cost", abs(float(LD(out["cost"]) - ref[0])) / float(ref[0]), abs(float(LD(f64[0]) - ref[0])) / float(ref[0]))
    for c in range(6):
        ok &= stage_ok(f"{what}: record {c}", rel(out["record"][k, c], ref[2][:, c]), rel(f64[2][:, c], ref[2][:, c]))
    ok &= stage_ok(f"{what}: gradient", rel(out["gradient"][fc], ref[3]), rel(f64[3], ref[3]))
    ok &= stage_ok(f"{what}: diagonal", rel(out["diagonal"][fc], ref[4]), rel(f64[4], ref[4]))
    pr = vn.product_contract(ref[2], ca, cb, slot, ref[4], LD(mu), x[fc])
    ok &= stage_ok(f"{what}: product", rel(out["product"][fc], pr), rel(vn.product_contract(f64[2], ca, cb, slot, f64[4], mu, x[fc]), pr))
    nf = ~free
    assert not out["gradient"][nf].any() and not out["diagonal"][nf].any() and not out["product"][nf].any()
    return ok, out


def test_sums_on_the_graph(gpu, graph):
    assert _sums_against_longdouble(gpu, graph, "graph")[0]
    g = dict(graph); g["has_prior"] = graph["has_prior"].copy(); g["has_prior"][[1, 5, 6]] = 1       # constant cameras: their x counts as 0
    assert _sums_against_longdouble(gpu, g, "graph with constant cameras")[0]


def test_sums_by_incidence_count(gpu):
    """a camera with 1 incidence (every leaf), with the most a thread walks, one more (a workgroup), and a hub in a few thousand pairs"""
    light = gpu.view_graph_calibrate_limits()["light_incidences"]
    for leaves in (1, light, light + 1, 3000):
        assert _sums_against_longdouble(gpu, star(leaves, 20 + leaves % 7), f"star of {leaves}")[0]


def test_sums_same_camera_and_mixed(gpu):
    one = vn.make_graph(1, 15, 5, images_per_camera=6)
    k, ca, cb = vn.participating(one)
    assert (ca == cb).all() and len(k) == 15
    ok, out = _sums_against_longdouble(gpu, one, "same camera only")
    assert ok and not out["record"][:, 3].any() and not out["record"][:, 5].any()
    mixed = vn.make_graph(4, 20, 7, images_per_camera=3)
    k, ca, cb = vn.participating(mixed)
    assert (ca == cb).any() and (ca != cb).any()
    assert _sums_against_longdouble(gpu, mixed, "both costs")[0]


def test_zero_denominator(gpu, graph):
    """di == 0 and dj == 0 forced by a hand-written d: the denominators become 1e-6 and stop depending on the focal"""
    g = vn.make_graph(5, 8, 3)
    d = vn.setup_all(g)
    d[0, 0] = 0.0; d[0, 1] = 0.0                  # di = fj2 * 0 + 0
    d[1, 4] = 0.0; d[1, 6] = 0.0                  # dj
    d[2, [0, 1, 4, 6]] = 0.0                      # both
    ok, out = _sums_against_longdouble(gpu, g, "zero denominators", d_in=d)
    assert ok and np.array_equal(out["d"], d) and np.isfinite(out["record"]).all()
    k, ca, cb = vn.participating(g)
    _, v = vn.residuals_contract(d, g["focal0"][ca], g["focal0"][cb])
    assert v["di_set"][[0, 2]].all() and v["dj_set"][[1, 2]].all() and v["di_set"].sum() == 2 and v["dj_set"].sum() == 2


def test_no_pair_and_one_pair(gpu):
    g = vn.make_graph(5, 8, 3)
    g["valid_in"] = np.zeros(8, dtype=np.uint8)
    out = _probe(gpu, g)
    assert all(not np.any(out[k]) for k in ("d", "residual", "record", "gradient", "diagonal", "product")) and out["cost"] == 0.0
    g["valid_in"][5] = 1
    ok, out = _sums_against_longdouble(gpu, g, "one pair")
    assert ok and np.flatnonzero(out["record"].any(axis=1)).tolist() == [5]
    h = vn.make_graph(5, 8, 3); h["model"] = np.full(8, vn.MODEL_H, dtype=np.int32)
    assert not np.any(_probe(gpu, h)["d"])
