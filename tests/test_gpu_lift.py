"""GPU tests of the depth lift (xm_lift_observations, include/xm_amd.h) against its numpy restatement (tests/xm_lift_numpy.py), which
tests/test_lift_numpy.py ties to the outputs recorded from the reference's own lines: nout, cam, lm, row, w, threshold and every counter
EXACTLY (w and threshold bit for bit), p componentwise within 8 * 2^-53 * (|Kinv| |(u, v, 1)|) * |d| -- two roundings of a three-term
product sum and one multiply, on each side.

Shapes: maps of at most 48 x 64 pixels; cameras whose row count sits at every place where the code changes its path (an empty camera, one
and two rows, an integral percentile position, full wavefronts and workgroups, both limits of xm_lift_limits()), several tracks sharing a
pixel where a camera needs more rows than the map has pixels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import xm_lift_numpy as ln

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("cam", "lm", "row", "p", "w", "threshold")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _run(xmamd, c, depth=None, conf=None, **kw):
    a, k = ln.call_args(c)
    a = list(a)
    if depth is not None:
        a[3], a[4] = depth, conf
    k.update(kw)
    return xmamd.lift_observations(*a, **k)


def _same(plan, ref, what=""):
    assert plan.cam.dtype == np.int32 and plan.lm.dtype == np.int32 and plan.row.dtype == np.int32
    assert plan.cam.size == ref["cam"].size, what
    for f in ("cam", "lm", "row"):
        assert np.array_equal(getattr(plan, f), ref[f]), (what, f)
    assert np.array_equal(_bits(plan.w), _bits(ref["w"])), what
    assert np.array_equal(_bits(plan.threshold), _bits(ref["threshold"])), what
    assert {k: plan.info[k] for k in ln.INFO_FIELDS} == ref["info"], what
    err = np.abs(plan.p - ref["p"])
    if err.size:
        print(f"LIFT_ERR {what}: largest |p - restatement| / bound {np.max(err / np.maximum(ref['p_bound'], 1e-300)):.3f}")
    assert np.all(err <= ref["p_bound"]), what


def _identical(a, b, what=""):
    for f in ARRAYS:
        assert np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))), (what, f)
    assert {k: a.info[k] for k in ln.INFO_FIELDS} == {k: b.info[k] for k in ln.INFO_FIELDS}, what


def _on_device(xmamd, maps):
    return None if maps is None else [None if D is None else (xmamd.DevArray(D), D.shape[0], D.shape[1]) for D in maps]


@pytest.fixture(scope="module")
def cases(xmamd):
    """every case with its restatement (computed once) and the library's answer for host maps"""
    xmamd.require_gpu()
    lim = xmamd.lift_limits()
    out = ln.gpu_cases(lim)
    out.update({name: ln.load_case(name)[0] for name in ln.CASES})
    for c in out.values():
        c["ref"] = ln.run_numpy(c, limits=lim)
        c["plan"] = _run(xmamd, c)
    return out


@pytest.mark.parametrize("name", ("a", "b", "small", "tiers", "degenerate", "border10", "border0", "duplicates", "no_conf", "mixed"))
def test_equals_the_restatement(cases, name):
    c = cases[name]
    _same(c["plan"], c["ref"], name)
    i = c["plan"].info
    assert c["plan"].cam.size + i["rows_duplicate"] + i["rows_border"] + i["rows_depth"] + i["rows_no_map"] == c["cam"].size
    assert min(i["seconds_index"], i["seconds_kernels"], i["seconds_download"]) >= 0.0


def test_recorded_reference_outputs(cases):
    for name in ln.CASES:
        _, ref = ln.load_case(name)
        plan = cases[name]["plan"]
        for f in ("cam", "lm", "row"):
            assert np.array_equal(getattr(plan, f), ref[f]), (name, f)
        assert np.array_equal(_bits(plan.w), _bits(ref["w"]))
        assert plan.info["rows_duplicate"] == ref["rows_duplicate"]
        assert np.all(np.abs(plan.p - ref["p"]) <= cases[name]["ref"]["p_bound"])


def test_every_size_took_its_path(cases, xmamd):
    lim = xmamd.lift_limits()
    i = cases["tiers"]["plan"].info
    assert (i["cams_small"], i["cams_large"], i["cams_workspace"]) == (1, 3, 2) and i["max_rows"] == 2 * lim["lds_rows"] + 1
    i = cases["small"]["plan"].info
    assert i["cams_large"] == 1 and i["cams_workspace"] == 0 and i["cams_small"] == cases["small"]["n"] - 2      # (one camera has no row)
    t = cases["small"]["plan"].threshold
    per = np.bincount(cases["small"]["cam"], minlength=cases["small"]["n"])
    assert np.isnan(t[per == 0]).all() and np.isfinite(t[per > 0]).all()


def test_two_calls_give_the_same_bits(cases, xmamd):
    for name in ("tiers", "mixed", "duplicates"):
        _identical(_run(xmamd, cases[name]), cases[name]["plan"], name)


def test_input_order_changes_only_row(cases, xmamd):
    for name in ("small", "tiers", "no_conf"):          # no (camera, track) is named twice in these
        c = cases[name]
        perm = np.random.default_rng(3).permutation(c["cam"].size)
        d = dict(c); d["cam"], d["lm"], d["xy"] = c["cam"][perm], c["lm"][perm], c["xy"][perm]
        q, plan = _run(xmamd, d), c["plan"]
        for f in ("cam", "lm", "p", "w", "threshold"):
            assert np.array_equal(_bits(getattr(q, f)), _bits(getattr(plan, f))), (name, f)
        assert np.array_equal(perm[q.row], plan.row)
        assert {k: q.info[k] for k in ln.INFO_FIELDS} == {k: plan.info[k] for k in ln.INFO_FIELDS}


def test_device_maps_give_the_bits_of_host_maps(cases, xmamd):
    for name in ("a", "tiers", "degenerate", "border0", "duplicates", "no_conf"):
        c = cases[name]
        _identical(_run(xmamd, c, _on_device(xmamd, c["depth"]), _on_device(xmamd, c["conf"])), c["plan"], name)
    c = cases["a"]
    with pytest.raises(xmamd.XmError, match="mixed"):
        _run(xmamd, c, _on_device(xmamd, c["depth"]), c["conf"])


TORCH_CHILD = """
import sys
import numpy as np
import torch                                  # first: the process's HIP runtime is the one torch brings
if not torch.cuda.is_available():
    sys.exit(77)
sys.path[:0] = [%r, %r]
import xmamd
import xm_lift_numpy as ln
c = ln.gpu_cases(xmamd.lift_limits())["mixed"]
a, k = ln.call_args(c)
host = xmamd.lift_observations(*a, **k)
dev = lambda maps: [None if D is None else torch.from_numpy(D).to("cuda") for D in maps]
depth, conf = dev(c["depth"]), dev(c["conf"])
torch.cuda.synchronize()
t = xmamd.lift_observations(a[0], a[1], a[2], depth, conf, a[5], **k)
same = all(np.array_equal(np.ascontiguousarray(getattr(host, f)).view(np.uint8), np.ascontiguousarray(getattr(t, f)).view(np.uint8))
           for f in ("cam", "lm", "row", "p", "w", "threshold"))
ints = {f: t.info[f] for f in ln.INFO_FIELDS}
print("LIFT_TORCH", same and ints == {f: host.info[f] for f in ln.INFO_FIELDS}, host.cam.size, ints)
"""


def test_device_tensors(cases):
    """maps as torch tensors on the device, in a process of their own that imports torch first, as a pipeline with a depth network does:
    this process has already initialised the library's HIP runtime, after which torch finds no device"""
    pytest.importorskip("torch")
    child = subprocess.run([sys.executable, "-c", TORCH_CHILD % (os.path.join(ROOT, "xm-code_amd"), os.path.join(ROOT, "tests"))], capture_output=True,
                           text=True, timeout=300)
    if child.returncode == 77:
        pytest.skip("this torch build sees no device")
    assert child.returncode == 0, child.stderr[-2000:]
    line = [x for x in child.stdout.splitlines() if x.startswith("LIFT_TORCH")][-1].split()
    assert line[1] == "True" and int(line[2]) == cases["mixed"]["plan"].cam.size, child.stdout


def test_carry_and_empty_inputs(cases, xmamd):
    c = cases["mixed"]
    colour = np.arange(c["cam"].size * 3).reshape(-1, 3)
    got, = c["plan"].carry(colour)
    assert np.array_equal(got, colour[c["plan"].row])
    none = xmamd.lift_observations(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), c["depth"], c["conf"], c["K"], m=5)
    assert none.cam.size == 0 and np.isnan(none.threshold).all() and none.info["cams_empty"] == c["n"] and none.info["cams_no_map"] == 0
    all_none = xmamd.lift_observations(c["cam"], c["lm"], c["xy"], [None] * c["n"], None, c["K"], m=c["m"])
    assert all_none.cam.size == 0 and all_none.info["cams_no_map"] == c["n"]
    assert all_none.info["rows_no_map"] + all_none.info["rows_duplicate"] == c["cam"].size


def test_hand_off_to_clean_and_context(xmamd):
    """the list goes into clean_observations and Context(obs=...) as it is (construction only)"""
    rng = np.random.default_rng(9)
    n, m, h, w = 6, 60, 48, 64
    cam = np.repeat(np.arange(n), m).astype(np.int32); lm = np.tile(np.arange(m), n).astype(np.int32)
    xy = np.stack([rng.integers(10, w - 10, n * m) + 0.5, rng.integers(10, h - 10, n * m) + 0.5], axis=1)
    depth = [ln.grid_depth(rng, h, w) for _ in range(n)]; conf = [rng.uniform(0.2, 1.0, (h, w)).astype(np.float32) for _ in range(n)]
    plan = xmamd.lift_observations(cam, lm, xy, depth, conf, ln.intrinsics(n, [(h, w)] * n), m=m)
    assert plan.cam.size > n * m * 0.8
    xmamd.Context(obs=(plan.cam, plan.lm, plan.p, plan.w), n=n).close()
    cl = xmamd.clean_observations(plan.cam, plan.lm, plan.w, n=n, m=m)
    assert cl.info["n_new"] == n and cl.keep.all()
    c2, l2, p2, w2 = cl.apply(plan.cam, plan.lm, plan.p, plan.w)
    ctx = xmamd.Context(obs=(c2, l2, p2, w2), n=n)
    ctx.close()


def test_refusals(cases, xmamd):
    """every XM_ERR_ARG of the header that needs a look at the arrays (the others: tests/test_lift_numpy.py)"""
    c = cases["no_conf"]
    bad = lambda **kw: dict(c, **kw)
    for change, word in ((dict(cam=np.where(np.arange(c["cam"].size) == 5, c["n"], c["cam"]).astype(np.int32)), "camera index out of range"),
                         (dict(cam=np.where(np.arange(c["cam"].size) == 5, -1, c["cam"]).astype(np.int32)), "camera index out of range"),
                         (dict(lm=np.where(np.arange(c["cam"].size) == 7, c["m"], c["lm"]).astype(np.int32)), "landmark index out of range"),
                         (dict(lm=np.where(np.arange(c["cam"].size) == 7, -1, c["lm"]).astype(np.int32)), "landmark index out of range"),
                         (dict(xy=np.where(np.arange(c["cam"].size)[:, None] == 3, np.nan, c["xy"])), "not finite"),
                         (dict(xy=np.where(np.arange(c["cam"].size)[:, None] == 3, np.inf, c["xy"])), "not finite"),
                         (dict(xy=np.where(np.arange(c["cam"].size)[:, None] == 3, -2.0 ** 31, c["xy"])), "2\\^31"),
                         (dict(depth=[c["depth"][0], np.zeros((0, 64), dtype=np.float32)]), "height or width")):
        with pytest.raises(xmamd.XmError, match=word):
            _run(xmamd, bad(**change))
    ok = _run(xmamd, bad(xy=np.where(np.arange(c["cam"].size)[:, None] == 3, 2.0 ** 31 - 1.0, c["xy"])))      # the largest position allowed: outside the border
    assert ok.info["rows_border"] == c["plan"].info["rows_border"] + 1
    _identical(_run(xmamd, c), c["plan"], "after the refusals")
