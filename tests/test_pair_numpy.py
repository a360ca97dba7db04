"""CPU tests of the pairwise relative-rotation filter's restatements and ABI: tests/xm_pair_numpy.py equals the outputs recorded from the
reference's own lines (tests/golden/pair) exactly; every case the GPU tests compare exactly has a decision margin of at least 1e-10; the
longdouble restatement takes the same decisions; the header, the binding and the library agree, and bad arguments are refused before any
device is looked at."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

import xm_pair_exact as pe
import xm_pair_numpy as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "min_joint", "min_flags", "flags", "trim", "dist_pct", "err_pct", "mad_factor")
STAT_FIELDS = ("n_joint", "n_kept", "n_flagged", "status", "scale1", "scale2", "translation", "median", "p95", "percentage")
RES_FIELDS = ("struct_size", "reserved", "pairs_used", "pairs_skipped", "pairs_degenerate", "nobs_flagged", "max_joint", "pairs_on_workspace_path",
              "seconds_index", "seconds_kernels", "seconds_download")


def _ref(c, **kw):
    return pn.pair_filter_numpy(c["cam"], c["lm"], c["p"], c["pi"], c["pj"], c["R"], c["n"], c["m"], **kw)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in pn.CASES:
        c = pn.load_case(name)
        c["ref"] = _ref(c, skip_row0=True)
        out[name] = c
    return out


@pytest.mark.parametrize("name", pn.CASES)
def test_restatement_equals_the_reference(cases, name):
    c = cases[name]
    ref = c["ref"]
    assert np.array_equal(ref["outlier"], pn.fixture_outlier(c["fx"])) and np.array_equal(ref["count"], c["fx"]["count"].astype(np.int32))
    assert np.array_equal(ref["count"] > 0, ref["outlier"])
    print(f"case {name}: {ref['info']}, decision margin {ref['margin']:.3e}")
    assert ref["margin"] >= pn.MIN_MARGIN
    assert ref["info"]["pairs_used"] + ref["info"]["pairs_skipped"] == c["pi"].size and ref["info"]["pairs_degenerate"] == 0


def test_cases_are_what_they_say(cases):
    a, b = cases["a"], cases["b"]
    assert a["cam"].size == 64549 and a["n"] == 93 and a["pi"].size == 93 * 92 // 2 and a["ref"]["info"]["max_joint"] > 1000
    nj = {(int(i), int(j)): int(k) for i, j, k in zip(b["pi"], b["pj"], _ref(b)["stats"]["n_joint"])}
    assert (nj[0, 2], nj[0, 3], nj[0, 4]) == (19, 20, 21) and (5, 6) not in nj and len(nj) == 65
    assert b["cam"][0] == 0 and all(np.any((b["cam"] == c) & (b["lm"] == b["lm"][0])) for c in (3, 4))      # row 0 is among the common points


def test_row0_takes_part_without_the_flag(cases):
    b = cases["b"]
    with_row0, without = _ref(b), b["ref"]
    q03 = int(np.flatnonzero((b["pi"] == 0) & (b["pj"] == 3))[0])
    assert with_row0["stats"]["n_joint"][q03] == 20 and without["stats"]["n_joint"][q03] == 19
    assert with_row0["stats"]["status"][q03] == pn.USED and without["stats"]["status"][q03] == pn.TOO_FEW
    assert with_row0["margin"] >= pn.MIN_MARGIN


def test_margins_of_the_synthetic_cases(cases, xmamd):
    limit = xmamd.pair_filter_limits()["lds_joint"]
    assert limit >= 512
    worst = np.inf
    for k in pn.JOINT_SIZES:
        k = pn.joint_size(k, limit)
        for shuffle in (False, True):
            c = pn.two_camera_scene(k, 1000 + k, shuffle)
            r = _ref(c)
            assert r["info"]["max_joint"] == k and r["info"]["pairs_used"] == (1 if k >= 20 else 0)
            assert r["margin"] >= pn.MIN_MARGIN, (k, shuffle, r["margin"])
            worst = min(worst, r["margin"])
    b = cases["b"]
    for kw in pn.OPTION_SETS:
        r = _ref(b, **kw)
        assert r["margin"] >= pn.MIN_MARGIN, (kw, r["margin"])
        worst = min(worst, r["margin"])
    d = dict(b); d.update(pn.doubled_pairs(b))
    r = _ref(d)
    assert r["margin"] >= pn.MIN_MARGIN
    print(f"smallest decision margin of the synthetic cases: {min(worst, r['margin']):.3e}")
    two = _ref(b, min_flags=2)
    assert np.array_equal(two["outlier"], two["count"] >= 2) and 0 < two["outlier"].sum() < (two["count"] > 0).sum()


def test_longdouble_restatement_takes_the_same_decisions(cases):
    b = cases["b"]
    scenes = [(b, dict(skip_row0=True)), (b, {})] + [(pn.two_camera_scene(k, 1000 + k, True), {}) for k in (20, 41, 101, 257)]
    for c, kw in scenes:
        f64 = _ref(c, **kw)
        ld = pe.pair_filter_exact(c["cam"], c["lm"], c["p"], c["pi"], c["pj"], c["R"], c["n"], c["m"], **kw)
        assert np.array_equal(f64["count"], ld["count"])
        for f in ("n_joint", "n_kept", "n_flagged", "status"):
            assert np.array_equal(f64["stats"][f], ld["stats"][f])
        e = pe.float_errors(f64["stats"], ld)
        assert max(e.values()) < 1e-13, e                  # the f64 restatement's own error: a few units in the last place


def test_input_order_does_not_matter(cases):
    b = cases["b"]
    perm = np.random.default_rng(1).permutation(b["cam"].size)
    d = dict(b); d["cam"], d["lm"], d["p"] = b["cam"][perm], b["lm"][perm], b["p"][perm]
    assert np.array_equal(_ref(d)["count"], _ref(b)["count"][perm])
    with pytest.raises(ValueError, match="twice"):
        pn.camera_index(np.array([0, 1, 0]), np.array([2, 2, 2]), 2, False)


# ------------------------------------------------------------------------------------------------ header, binding, library
PROTO = (" int (*f)(int64_t, int64_t, int64_t, const int32_t *, const int32_t *, const double *, int64_t, const int32_t *, const int32_t *,"
         " const double *, const xm_pair_options_t *, int32_t *, uint8_t *, xm_pair_stat_t *, xm_pair_result_t *) = xm_pair_filter; (void)f;"
         " int (*g)(int64_t *) = xm_pair_filter_limits; (void)g;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){ xm_pair_options_t o = XM_PAIR_OPTIONS_INIT;\n'
           'printf("%zu %zu %zu %d %u %d %d %d", sizeof(xm_pair_options_t), sizeof(xm_pair_stat_t), sizeof(xm_pair_result_t), XM_ABI_REVISION,'
           ' XM_PAIR_SKIP_ROW0, XM_PAIR_USED, XM_PAIR_TOO_FEW, XM_PAIR_DEGENERATE);\n'
           'printf(" %u %d %d %u %.17g %.17g %.17g %.17g", o.struct_size, o.min_joint, o.min_flags, o.flags, o.trim, o.dist_pct, o.err_pct, o.mad_factor);\n'
           + "".join(f' printf(" %zu", offsetof(xm_pair_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_pair_stat_t, {f}));\n' for f in STAT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_pair_result_t, {f}));\n' for f in RES_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return subprocess.check_output([os.path.join(d, "t")]).split()


def test_header_and_binding_agree(xmamd):
    v = _c_values()
    so, ss, sr, rev, skip, used, few, deg = map(int, v[:8])
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # added exports: the revision stays
    assert (skip, used, few, deg) == (xmamd.PAIR_SKIP_ROW0, xmamd.PAIR_USED, xmamd.PAIR_TOO_FEW, xmamd.PAIR_DEGENERATE) == (1, 0, 1, 2)
    assert (pn.USED, pn.TOO_FEW, pn.DEGENERATE) == (used, few, deg)
    assert ctypes.sizeof(xmamd.PairOptions) == so == 48 and ctypes.sizeof(xmamd.PairStat) == ss == 80 == xmamd.PAIR_STAT_DTYPE.itemsize
    assert ctypes.sizeof(xmamd.PairResult) == sr == 80
    # the defaults are the reference's constants (5_test_ceres.py:334, :341, :346, :369-370), in the header's initialiser and in the binding
    assert [float(x) for x in v[8:16]] == [48, 20, 1, 0, 0.05, 90.0, 95.0, 3.0]
    o = xmamd.PairOptions()
    assert [getattr(o, f) for f in OPT_FIELDS] == [48, 20, 1, 0, 0.05, 90.0, 95.0, 3.0]
    offs = list(map(int, v[16:]))
    assert [getattr(xmamd.PairOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.PairStat, f).offset for f in STAT_FIELDS] + \
           [getattr(xmamd.PairResult, f).offset for f in RES_FIELDS] == offs
    assert [xmamd.PAIR_STAT_DTYPE.fields[f][1] for f in STAT_FIELDS] == offs[len(OPT_FIELDS):len(OPT_FIELDS) + len(STAT_FIELDS)]
    assert xmamd.PAIR_STAT_DTYPE == pn.STAT_DTYPE


def test_exports_and_wrapper(xmamd):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_pair_filter", "xm_pair_filter_limits"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    sig = inspect.signature(xmamd.pair_filter).parameters
    assert list(sig) == ["cam", "lm", "p", "pairs_i", "pairs_j", "R", "n", "m", "min_joint", "trim", "dist_pct", "err_pct", "mad_factor", "min_flags", "skip_row0"]
    assert [sig[k].default for k in list(sig)[6:]] == [None, None, 20, 0.05, 90, 95, 3.0, 1, False]
    lim = xmamd.pair_filter_limits()                      # needs no device
    assert lim["threads"] == 256 and lim["lds_joint"] & (lim["lds_joint"] - 1) == 0 and lim["workspace_groups"] >= 1
    assert lim["small_joint"] == 256 and {255, 256, 257} <= set(pn.JOINT_SIZES)      # the GPU tests sit on both sides of it
    cam = np.zeros(4, dtype=np.int32); p = np.zeros((4, 3)); z = np.zeros(1, dtype=np.int32); R = np.eye(3)[None]
    for args, kw, word in (((cam, cam[:3], p, z, z, R), {}, "one entry per observation"), ((cam, cam, p[:, :2], z, z, R), {}, "one entry per observation"),
                           ((cam, cam, p, z, cam, R), {}, "one entry per pair"), ((cam, cam, p, z, z, np.eye(3)[None, :2]), {}, "one entry per pair"),
                           ((cam, cam, p, z, z, R), dict(min_joint=-1), "negative"), ((cam, cam, p, z, z, R), dict(trim=-0.1), "negative"),
                           ((cam, cam, p, z, z, R), dict(mad_factor=-1.0), "negative"), ((cam, cam, p, z, z, R), dict(trim=0.5), "below 0.5"),
                           ((cam, cam, p, z, z, R), dict(err_pct=101), "above 100")):
        with pytest.raises(xmamd.XmError, match=word):    # no device: the arguments are checked before anything else is looked at
            xmamd.pair_filter(*args, **kw)
    plan = xmamd.PairFilterPlan(np.array([0, 2, 0], dtype=np.int32), np.array([False, True, False]), None, {})
    a, b = plan.apply(np.arange(3), np.arange(6).reshape(3, 2))
    assert a.tolist() == [0, 2] and b.tolist() == [[0, 1], [4, 5]]
    with pytest.raises(xmamd.XmError, match="another length"):
        plan.apply(np.arange(4))


def test_library_refusals_need_no_device(xmamd):
    """struct sizes, options, flags, sizes and null arrays are looked at before the device (XM_ERR_ARG = -2)"""
    L = xmamd.lib()
    cam = np.zeros(2, dtype=np.int32); p = np.zeros((2, 3)); R = np.eye(3); count = np.zeros(2, dtype=np.int32); out = np.zeros(2, dtype=np.uint8)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(o, r, n=1, m=1, nobs=2, npairs=1, p_=p, count_=count, R_=R):
        return L.xm_pair_filter(n, m, nobs, P(cam), P(cam), P(p_), npairs, P(cam), P(cam), P(R_), None if o is None else ctypes.byref(o), P(count_), P(out), None,
                                None if r is None else ctypes.byref(r))

    def fresh():
        r = xmamd.PairResult(); r.struct_size = ctypes.sizeof(r)
        return xmamd.PairOptions(), r
    for change, word in ((lambda o, r: setattr(o, "struct_size", 40), "struct_size"), (lambda o, r: setattr(r, "struct_size", 0), "struct_size"),
                         (lambda o, r: setattr(o, "min_joint", -1), "negative"), (lambda o, r: setattr(o, "min_flags", -1), "negative"),
                         (lambda o, r: setattr(o, "trim", -0.01), "negative"), (lambda o, r: setattr(o, "dist_pct", -1.0), "negative"),
                         (lambda o, r: setattr(o, "mad_factor", float("nan")), "negative"), (lambda o, r: setattr(o, "trim", 0.5), "below 0.5"),
                         (lambda o, r: setattr(o, "err_pct", 100.5), "above 100"), (lambda o, r: setattr(o, "flags", 2), "unknown flag")):
        o, r = fresh(); change(o, r)
        assert call(o, r) == -2 and word in L.xm_last_error().decode()
    o, r = fresh()
    assert call(None, r) == -2 and call(o, None) == -2 and "null" in L.xm_last_error().decode()
    assert call(o, r, n=-1) == -2 and call(o, r, npairs=-1) == -2 and "negative size" in L.xm_last_error().decode()
    assert call(o, r, nobs=2 ** 31) == -2 and "2^31" in L.xm_last_error().decode()
    assert call(o, r, p_=None) == -2 and call(o, r, count_=None) == -2 and call(o, r, R_=None) == -2 and "null" in L.xm_last_error().decode()
    assert L.xm_pair_filter_limits(None) == -2
