"""CPU tests of the depth lift's restatement and ABI: tests/xm_lift_numpy.py equals the outputs recorded from the reference's own lines
(tests/golden/lift) exactly in cam, lm, row and w, and in p within the bound of include/xm_amd.h's arithmetic; for every case the GPU tests
use, the reference's float32 percentile and the contract's f64 percentile keep the same rows; the header, the binding and the library agree,
and bad arguments are refused before any device is looked at."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

import xm_lift_numpy as ln

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "margin", "flags", "reserved", "depth_pct")
RES_FIELDS = ("struct_size", "reserved") + ln.INFO_FIELDS + ("seconds_index", "seconds_kernels", "seconds_download")


@pytest.mark.parametrize("name", ln.CASES)
def test_restatement_equals_the_reference(name):
    c, ref = ln.load_case(name)
    ours = ln.run_numpy(c)
    assert ref["cam"].size > 300
    for f in ("cam", "lm", "row"):
        assert np.array_equal(ours[f], ref[f]), f
    assert np.array_equal(ours["w"].view(np.uint64), ref["w"].view(np.uint64))
    assert ours["info"]["rows_duplicate"] == ref["rows_duplicate"]
    err = np.abs(ours["p"] - ref["p"])
    print(f"case {name}: {ours['info']}, largest |p - reference| / bound {np.max(err / ours['p_bound']):.3f}")
    assert np.all(err <= ours["p_bound"])
    i = ours["info"]
    assert ref["cam"].size + i["rows_duplicate"] + i["rows_border"] + i["rows_depth"] + i["rows_no_map"] == c["cam"].size
    # the order is camera, then track, and no (camera, track) is named twice
    key = ours["cam"].astype(np.int64) * (c["m"] + 1) + ours["lm"]
    assert np.all(np.diff(key) > 0)


def test_recorded_cases_are_what_they_say():
    a, ra = ln.load_case("a")
    ia = ln.run_numpy(a)["info"]
    assert a["n"] == 12 and ia["cams_no_map"] == 1 and ia["cams_empty"] == 2 and ia["rows_duplicate"] > 50 and ia["rows_border"] > 50
    assert len({d.shape for d in a["depth"] if d is not None}) == 3 and (a["depth"][4] <= 0).sum() > 100
    b, rb = ln.load_case("b")
    assert b["n"] == 5 and ln.run_numpy(b)["info"]["max_rows"] > 700
    # a twin's two rows lie at different pixels, so the recorded p says which of them the reference kept: the earlier one
    for c, r in ((a, ra), (b, rb)):
        first = {}
        for row, (i, l) in enumerate(zip(c["cam"], c["lm"])):
            first.setdefault((int(i), int(l)), row)
        assert all(first[int(i), int(l)] == row for i, l, row in zip(r["cam"], r["lm"], r["row"]))


def test_percentile_is_numpys_in_f64():
    rng = np.random.default_rng(7)
    for k in (1, 2, 20, 21, 41, 64, 257, 1000):
        for pct in (0.0, 37.5, 95.0, 100.0):
            d = ln.grid_depth(rng, 1, k).ravel()
            assert ln.percentile_f64(d, pct) == np.percentile(d.astype(np.float64), pct)
    assert np.isnan(ln.percentile_f64(np.array([1.0, np.nan, 2.0], dtype=np.float32), 95.0))
    # the stated difference: float32 interpolation rounds the threshold onto its lower neighbour, f64 does not
    d = np.array([1.0] * 19 + [np.nextafter(np.float32(1.0), np.float32(2.0))], dtype=np.float32)
    assert ln.percentile_f64(d, 95.0) > 1.0


def test_f32_rule_keeps_the_same_rows_in_every_gpu_case(xmamd):
    """a condition on the INPUTS of tests/test_gpu_lift.py: with depths on the 2^-10 grid the reference's float32 percentile decides every
    row as the contract's f64 percentile does (the camera with a NaN depth yields nothing under both)"""
    cases = ln.gpu_cases(xmamd.lift_limits())
    cases.update({name: ln.load_case(name)[0] for name in ln.CASES})
    for name, c in cases.items():
        f64, f32 = ln.run_numpy(c), ln.run_numpy(c, f32_rule=True)
        for f in ("cam", "lm", "row"):
            assert np.array_equal(f64[f], f32[f]), (name, f)
        assert f64["info"] == f32["info"], name


def test_gpu_cases_are_what_they_say(xmamd):
    lim = xmamd.lift_limits()
    cases = ln.gpu_cases(lim)
    T, S, L = lim["threads"], lim["small_rows"], lim["lds_rows"]
    small = np.bincount(cases["small"]["cam"], minlength=cases["small"]["n"])
    assert {0, 1, 2, 20, 21, 41, 63, 64, 65, T - 1, T, T + 1, S - 1, S, S + 1} == set(small.tolist())
    r = ln.run_numpy(cases["small"], limits=lim)
    assert np.isnan(r["threshold"][small == 0]).all() and not np.isnan(r["threshold"][small > 0]).any()
    assert not np.any(r["cam"] == int(np.flatnonzero(small == 1)[0]))                 # one row: it is the largest depth, nothing survives
    i = ln.run_numpy(cases["tiers"], limits=lim)["info"]
    assert (i["cams_small"], i["cams_large"], i["cams_workspace"], i["max_rows"]) == (1, 3, 2, 2 * L + 1)
    d = ln.run_numpy(cases["degenerate"])
    assert d["info"]["cams_no_map"] == 2 and d["info"]["cams_empty"] == 4 and not np.any(np.isin(d["cam"], (0, 1, 2, 4, 5, 6)))
    assert np.isnan(d["threshold"][[0, 1, 4, 5, 6]]).all() and d["threshold"][2] == 2.5 and np.any(d["cam"] == 3) and np.any(d["cam"] == 7)
    for mg in (10, 0):
        c = cases[f"border{mg}"]
        r = ln.run_numpy(c)
        extra = c["lm"] >= c["m"] - 10
        # per camera: one pixel outside each of the four borders; margin - 0.5 is outside too unless the margin is 0 (-0.5 is pixel 0)
        assert extra.sum() == 30 and r["info"]["rows_border"] == (18 if mg else 12)
        assert mg or np.any(c["xy"][:, 0] == -0.5)
    u = cases["duplicates"]
    r = ln.run_numpy(u)
    assert r["info"]["rows_duplicate"] > 40 and not np.any((r["cam"] == 0) & (r["lm"] == 900))
    k = int(np.flatnonzero((r["cam"] == 1) & (r["lm"] == 901))[0])
    assert r["row"][k] == 0 and u["cam"][-1] == 1 and u["lm"][-1] == 901


# ------------------------------------------------------------------------------------------------ header, binding, library
PROTO = (" int (*f)(int64_t, int64_t, int64_t, const int32_t *, const int32_t *, const double *, const int32_t *, const float *const *,"
         " const float *const *, const double *, const xm_lift_options_t *, int32_t *, int32_t *, double *, double *, int32_t *, int64_t *, double *,"
         " xm_lift_result_t *) = xm_lift_observations; (void)f; int (*g)(int64_t *) = xm_lift_limits; (void)g;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){ xm_lift_options_t o = XM_LIFT_OPTIONS_INIT;\n'
           'printf("%zu %zu %d %u", sizeof(xm_lift_options_t), sizeof(xm_lift_result_t), XM_ABI_REVISION, XM_LIFT_MAPS_ON_DEVICE);\n'
           'printf(" %u %d %u %u %.17g", o.struct_size, o.margin, o.flags, o.reserved, o.depth_pct);\n'
           + "".join(f' printf(" %zu", offsetof(xm_lift_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_lift_result_t, {f}));\n' for f in RES_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return subprocess.check_output([os.path.join(d, "t")]).split()


def test_header_and_binding_agree(xmamd):
    v = _c_values()
    so, sr, rev, on_dev = map(int, v[:4])
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # added exports: the revision stays
    assert on_dev == xmamd.LIFT_MAPS_ON_DEVICE == 1
    assert ctypes.sizeof(xmamd.LiftOptions) == so == 24 and ctypes.sizeof(xmamd.LiftResult) == sr == 112
    # the defaults are the reference's constants (5_test_ceres.py:264, :273), in the header's initialiser and in the binding
    assert [float(x) for x in v[4:9]] == [24, 10, 0, 0, 95.0]
    o = xmamd.LiftOptions()
    assert [getattr(o, f) for f in OPT_FIELDS] == [24, 10, 0, 0, 95.0]
    assert [getattr(xmamd.LiftOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.LiftResult, f).offset for f in RES_FIELDS] == list(map(int, v[9:]))


def test_exports_and_wrapper(xmamd):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_lift_observations", "xm_lift_limits"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    sig = inspect.signature(xmamd.lift_observations).parameters
    assert list(sig) == ["cam", "lm", "xy", "depth", "conf", "K", "n", "m", "margin", "depth_pct"]
    assert [sig[k].default for k in list(sig)[6:]] == [None, None, 10, 95.0]
    lim = xmamd.lift_limits()                             # needs no device
    assert lim["threads"] == 256 and lim["lds_rows"] & (lim["lds_rows"] - 1) == 0 and lim["workspace_groups"] >= 1
    assert 2 <= lim["small_rows"] < lim["lds_rows"]
    cam = np.zeros(4, dtype=np.int32); xy = np.full((4, 2), 20.5); D = np.ones((48, 64), dtype=np.float32); K = np.eye(3)[None]

    class OnDevice:                                       # what a device tensor looks like to the binding
        shape, is_cuda, dtype = (48, 64), True, "float32"

        def data_ptr(self):
            return 4096
    for args, kw, word in (((cam, cam[:3], xy, [D], [D], K), {}, "one entry per row"), ((cam, cam, xy[:, :1], [D], [D], K), {}, "one entry per row"),
                           ((cam, cam, xy, [D, D], [D], np.stack([np.eye(3)] * 2)), {}, "one entry per camera"),
                           ((cam, cam, xy, [D], [D], np.eye(3)), {}, "n x 3 x 3"), ((cam, cam, xy, [D], [D], K), dict(margin=-1), "negative margin"),
                           ((cam, cam, xy, [D], [D], K), dict(depth_pct=100.5), "outside"), ((cam, cam, xy, [D], [D], K), dict(depth_pct=-1), "outside"),
                           ((cam, cam, xy, [D.astype(np.float64)], None, K), {}, "float32"), ((cam, cam, xy, [D[0]], None, K), {}, "2-D"),
                           ((cam, cam, xy, [D], [D[:, :50]], K), {}, "differ in shape"), ((cam, cam, xy, ["x"], None, K), {}, "none of"),
                           ((cam, cam, xy, [D], [OnDevice()], K), {}, "mixed")):
        with pytest.raises(xmamd.XmError, match=word):    # no device: the arguments are checked before anything else is looked at
            xmamd.lift_observations(*args, **kw)
    plan = xmamd.LiftPlan(None, None, None, None, np.array([2, 0], dtype=np.int32), None, {}, 3)
    a, b = plan.carry(np.arange(3) * 10, np.arange(6).reshape(3, 2))
    assert a.tolist() == [20, 0] and b.tolist() == [[4, 5], [0, 1]]
    with pytest.raises(xmamd.XmError, match="another length"):
        plan.carry(np.arange(4))


def test_library_refusals_need_no_device(xmamd):
    """struct sizes, options, flags, sizes and null arrays are looked at before the device (XM_ERR_ARG = -2)"""
    L = xmamd.lib()
    cam = np.zeros(2, dtype=np.int32); xy = np.full((2, 2), 20.5); hw = np.array([48, 64], dtype=np.int32); D = np.ones((48, 64), dtype=np.float32)
    dp = np.array([D.ctypes.data], dtype=np.uint64); K = np.eye(3); oi = np.zeros(2, dtype=np.int32); of = np.zeros(6)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(o, r, n=1, m=1, nrows=2, cam_=cam, xy_=xy, hw_=hw, dp_=dp, K_=K, out_=oi, nout=True):
        no = ctypes.c_int64(0)
        return L.xm_lift_observations(n, m, nrows, P(cam_), P(cam), P(xy_), P(hw_), P(dp_), None, P(K_), None if o is None else ctypes.byref(o), P(out_),
                                      P(oi), P(of), P(of), P(oi), ctypes.byref(no) if nout else None, None, None if r is None else ctypes.byref(r))

    def fresh():
        r = xmamd.LiftResult(); r.struct_size = ctypes.sizeof(r)
        return xmamd.LiftOptions(), r
    for change, word in ((lambda o, r: setattr(o, "struct_size", 16), "struct_size"), (lambda o, r: setattr(r, "struct_size", 0), "struct_size"),
                         (lambda o, r: setattr(o, "margin", -1), "negative margin"), (lambda o, r: setattr(o, "depth_pct", -0.5), "outside"),
                         (lambda o, r: setattr(o, "depth_pct", 100.5), "outside"), (lambda o, r: setattr(o, "depth_pct", float("nan")), "outside"),
                         (lambda o, r: setattr(o, "flags", 2), "unknown flag")):
        o, r = fresh(); change(o, r)
        assert call(o, r) == -2 and word in L.xm_last_error().decode()
    o, r = fresh()
    assert call(None, r) == -2 and call(o, None) == -2 and call(o, r, nout=False) == -2 and "null" in L.xm_last_error().decode()
    assert call(o, r, n=-1) == -2 and call(o, r, nrows=-1) == -2 and "negative size" in L.xm_last_error().decode()
    assert call(o, r, nrows=2 ** 31) == -2 and "2^31" in L.xm_last_error().decode()
    for kw in (dict(cam_=None), dict(xy_=None), dict(out_=None), dict(hw_=None), dict(dp_=None), dict(K_=None)):
        assert call(o, r, **kw) == -2 and "null" in L.xm_last_error().decode()
    assert L.xm_lift_limits(None) == -2
