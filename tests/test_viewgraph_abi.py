"""CPU tests of the view-graph filter's ABI: include/xm_amd.h and the binding agree (sizes, offsets, defaults, constants), the header's
17-digit literals are the reference's constants to 1 ulp and the restatement reads the same literals, the symbols are exported, and every
refusal is made on the host before a device is looked for, with nothing written."""
import ctypes
import inspect
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import xm_viewgraph_numpy as vn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "flags", "max_epipolar_error_E", "max_epipolar_error_F", "max_epipolar_error_H", "min_inlier_num", "reserved", "min_inlier_ratio",
              "cos_max_rotation_error")
RES_FIELDS = ("struct_size", "rounds", "matches", "inliers", "matches_out", "pairs_valid", "pairs_invalid_in", "pairs_few_inliers", "pairs_low_ratio",
              "pairs_rotation", "pairs_outside", "pairs_none", "pairs_E", "pairs_F", "pairs_H", "largest", "components", "pairs_wave", "pairs_group",
              "pairs_workspace", "max_matches", "seconds_index", "seconds_kernels", "seconds_download")
CODES = ("XM_VG_SCORE", "XM_VG_MODEL_NONE", "XM_VG_MODEL_E", "XM_VG_MODEL_F", "XM_VG_MODEL_H", "XM_VG_VALID", "XM_VG_INVALID_IN", "XM_VG_FEW_INLIERS",
         "XM_VG_LOW_RATIO", "XM_VG_ROTATION", "XM_VG_OUTSIDE")
LITERALS = ("XM_VG_EPS", "XM_VG_MIN_DEPTH", "XM_VG_MAX_DEPTH", "XM_VG_COS_EPIPOLE", "XM_VG_COS_PARALLEL", "XM_VG_COS_10DEG")
PROTO = (" int (*f)(int64_t, const int64_t *, const double *, const double *, const double *, const double *, int64_t, const int32_t *, const int32_t *,"
         " const int32_t *, const double *, const double *, const double *, const uint8_t *, const uint8_t *, const double *, const int64_t *, const int32_t *,"
         " const int32_t *, const xm_vg_options_t *, uint8_t *, int32_t *, int32_t *, uint8_t *, int64_t *, int32_t *, int32_t *, xm_vg_result_t *)"
         " = xm_view_graph_filter; (void)f; int (*g)(int64_t *) = xm_view_graph_limits; (void)g;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){ xm_vg_options_t o = XM_VG_OPTIONS_INIT;\n'
           'printf("%zu %zu %d", sizeof(xm_vg_options_t), sizeof(xm_vg_result_t), XM_ABI_REVISION);\n'
           + "".join(f' printf(" %d", (int){c});\n' for c in CODES) + "".join(f' printf(" %.17g", (double){c});\n' for c in LITERALS)
           + 'printf(" %u %u %.17g %.17g %.17g %d %d %.17g %.17g", o.struct_size, o.flags, o.max_epipolar_error_E, o.max_epipolar_error_F,'
             ' o.max_epipolar_error_H, o.min_inlier_num, o.reserved, o.min_inlier_ratio, o.cos_max_rotation_error);\n'
           + "".join(f' printf(" %zu", offsetof(xm_vg_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_vg_result_t, {f}));\n' for f in RES_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return subprocess.check_output([os.path.join(d, "t")]).split()


def test_header_and_binding_agree(xmamd):
    v = _c_values()
    so, sr, rev = map(int, v[:3])
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # added exports: the revision stays
    assert ctypes.sizeof(xmamd.VgOptions) == so == 56 and ctypes.sizeof(xmamd.VgResult) == sr == 184
    codes = list(map(int, v[3:3 + len(CODES)]))
    assert codes == [xmamd.VG_SCORE, xmamd.VG_MODEL_NONE, xmamd.VG_MODEL_E, xmamd.VG_MODEL_F, xmamd.VG_MODEL_H, xmamd.VG_VALID, xmamd.VG_INVALID_IN,
                     xmamd.VG_FEW_INLIERS, xmamd.VG_LOW_RATIO, xmamd.VG_ROTATION, xmamd.VG_OUTSIDE] == [1, 0, 1, 2, 3, 0, 1, 2, 3, 4, 5]
    assert codes[1:] == [vn.NONE, vn.E_, vn.F_, vn.H_, vn.VALID, vn.INVALID_IN, vn.FEW_INLIERS, vn.LOW_RATIO, vn.ROTATION, vn.OUTSIDE]
    at = 3 + len(CODES) + len(LITERALS)
    # the defaults are those of glomap/types.h:18-33, in the header's initialiser and in the binding
    want = [56, 1, 1.0, 4.0, 4.0, 30, 0, 0.25, vn.COS_10DEG]
    assert [float(x) for x in v[at:at + 9]] == want
    o = xmamd.VgOptions()
    assert [getattr(o, f) for f in OPT_FIELDS] == want
    assert vn.DEFAULTS == dict(max_epipolar_error_E=1.0, max_epipolar_error_F=4.0, max_epipolar_error_H=4.0, min_inlier_num=30, min_inlier_ratio=0.25,
                               max_rotation_error_deg=10.0)
    offs = [getattr(xmamd.VgOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.VgResult, f).offset for f in RES_FIELDS]
    assert offs == list(map(int, v[at + 9:]))
    assert tuple(f for f, _ in xmamd.VgResult._fields_) == RES_FIELDS and set(vn.INFO_FIELDS) == set(RES_FIELDS[2:-3])


def test_the_literals_are_the_references_constants():
    """EPS = 1e-12 (glomap/types.h), the depths 1e-2 and 100 (image_pair_inliers.cc:65), cos(DegToRad(3)) + 1e-6 and 1 + 1e-6 (:54-57), the
    cosine of the default max_rotation_error: each 17-digit literal of the header against Python's math to 1 ulp; the restatement reads the
    same text"""
    v = _c_values()
    got = [float(x) for x in v[3 + len(CODES):3 + len(CODES) + len(LITERALS)]]
    want = [1e-12, 1e-2, 100.0, math.cos(math.radians(3.0)) + 1e-6, 1.0 + 1e-6, math.cos(math.radians(10.0))]
    for g, w in zip(got, want):
        assert abs(g - w) <= math.ulp(w), (g, w)
    assert got == [vn.EPS, vn.MIN_DEPTH, vn.MAX_DEPTH, vn.COS_EPIPOLE, vn.COS_PARALLEL, vn.COS_10DEG]
    header = open(os.path.join(ROOT, "include", "xm_amd.h")).read()
    module = open(os.path.join(ROOT, "tests", "xm_viewgraph_numpy.py")).read()
    for name, short in zip(LITERALS, ("EPS", "MIN_DEPTH", "MAX_DEPTH", "COS_EPIPOLE", "COS_PARALLEL", "COS_10DEG")):
        text = re.search(r"#define " + name + r"\s+(\S+)", header).group(1)
        assert re.fullmatch(r"\d\.\d{16}e[+-]\d\d", text), text                   # 17 significant digits
        assert re.search(r"^" + short + r" = " + re.escape(text) + r"$", module, re.M), name


def test_exports_and_wrapper(xmamd):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_view_graph_filter", "xm_view_graph_limits"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    sig = inspect.signature(xmamd.view_graph_filter).parameters
    assert list(sig)[:6] == ["foff_or_counts", "xy", "pi", "pj", "model", "matches"]
    assert {k: sig[k].default for k in vn.DEFAULTS} == vn.DEFAULTS and sig["score"].default is True and sig["rot"].default is None
    lim = xmamd.view_graph_limits()                        # needs no device
    assert lim["threads"] == 256 and lim["max_rounds"] == 1024 and 64 <= lim["wave_matches"] < lim["group_matches"]
    assert lim["wave_matches"] % 64 == 0 and lim["group_matches"] % lim["threads"] == 0
    assert {k: lim[k] for k in vn.LIMITS} == vn.LIMITS
    xy = np.zeros((4, 2)); e = np.zeros(0, dtype=np.int32)
    for args, kw, word in ((([2, 2], xy[:, :1], e, e, e, []), {}, "features x 2"), (([2, 2], xy, [0], [1, 0], [1], []), {}, "one entry per pair"),
                           (([2, 2], xy, [0], [1], [1, 1], ([0, 0], e, e)), {}, "model must have one entry"),
                           (([2, 2], xy, [0], [1], ["Q"], ([0, 0], e, e)), {}, "model must hold"),
                           (([2, 2], xy, [0], [1], ["E"], ([0, 0], e, e)), dict(rot=np.zeros((3, 3, 3))), "rot must be 2 x 3 x 3"),
                           (([2, 2], xy, [0], [1], ["E"], ([0, 0], e, e)), dict(Kinv=np.zeros(9)), "Kinv must be"),
                           (([2, 2], xy, [0], [1], ["E"], ([0, 0], e, e)), dict(valid_in=[1, 1]), "valid_in must be")):
        with pytest.raises(xmamd.XmError, match=word):     # no device: the arguments are checked before anything else is looked at
            xmamd.view_graph_filter(*args, **kw)
    # no pair needs no device: nothing is registered
    g = xmamd.view_graph_filter([2, 2], xy, e, e, e, [])
    assert g.registered.tolist() == [0, 0] and g.matches[0].tolist() == [0] and g.valid.size == 0 and g.info["largest"] == 0
    plan = xmamd.ViewGraphPlan(np.zeros(0, np.uint8), np.zeros(3, np.int32), np.array([0, 4, 0], dtype=np.int32), np.ones(3, np.uint8), None, {},
                               np.array([0, 1, 2], dtype=np.int32), np.array([1, 2, 0], dtype=np.int32), np.arange(27.0).reshape(3, 3, 3))
    a, b, R = plan.pairs()
    assert a.tolist() == [0, 2] and b.tolist() == [1, 0] and R.shape == (2, 3, 3) and R[1, 0, 0] == 18.0 and plan.valid.tolist() == [1, 0, 1]


def test_library_refusals_need_no_device(xmamd):
    """struct sizes, options, sizes, offsets, pairs, models and null arrays are looked at before the device (XM_ERR_ARG = -2), and nothing
    is written"""
    L = xmamd.lib()
    i32, i64, u8 = (lambda *a: np.array(a, dtype=np.int32)), (lambda *a: np.array(a, dtype=np.int64)), (lambda *a: np.array(a, dtype=np.uint8))
    base = dict(n=2, foff=i64(0, 2, 4), xy=np.zeros((4, 2)), focal=np.ones(2), Kinv=np.tile(np.eye(3), (2, 1, 1)), bearing=None, npairs=1, pi=i32(0), pj=i32(1),
                model=i32(1), Rrel=np.eye(3).reshape(1, 3, 3), trel=np.array([[1.0, 0, 0]]), FH=np.eye(3).reshape(1, 3, 3), valid_in=None, registered_in=None,
                rot=None, moff=i64(0, 1), f1=i32(0), f2=i32(0))
    outs = dict(inlier=np.full(1, 55, dtype=np.uint8), pair_inliers=np.full(1, 55, dtype=np.int32), pair_status=np.full(1, 55, dtype=np.int32),
                registered_out=np.full(2, 55, dtype=np.uint8), moff_out=np.full(2, 55, dtype=np.int64), f1_out=np.full(1, 55, dtype=np.int32),
                f2_out=np.full(1, 55, dtype=np.int32))
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(o, r, **kw):
        a = dict(base, **outs); a.update(kw)
        rc = L.xm_view_graph_filter(a["n"], P(a["foff"]), P(a["xy"]), P(a["focal"]), P(a["Kinv"]), P(a["bearing"]), a["npairs"], P(a["pi"]), P(a["pj"]),
                                    P(a["model"]), P(a["Rrel"]), P(a["trel"]), P(a["FH"]), P(a["valid_in"]), P(a["registered_in"]), P(a["rot"]), P(a["moff"]),
                                    P(a["f1"]), P(a["f2"]), None if o is None else ctypes.byref(o), P(a["inlier"]), P(a["pair_inliers"]), P(a["pair_status"]),
                                    P(a["registered_out"]), P(a["moff_out"]), P(a["f1_out"]), P(a["f2_out"]), None if r is None else ctypes.byref(r))
        assert all((x == 55).all() for x in outs.values())
        return rc

    def fresh():
        r = xmamd.VgResult(); r.struct_size = ctypes.sizeof(r)
        return xmamd.VgOptions(), r
    changes = [(lambda o, r: setattr(o, "struct_size", 48), "struct_size"), (lambda o, r: setattr(r, "struct_size", 0), "struct_size"),
               (lambda o, r: setattr(o, "flags", 2), "unknown flag"), (lambda o, r: setattr(o, "flags", 3), "unknown flag"),
               (lambda o, r: setattr(o, "min_inlier_num", -1), "negative min_inlier_num")]
    for f in ("max_epipolar_error_E", "max_epipolar_error_F", "max_epipolar_error_H", "min_inlier_ratio"):
        for bad in (-0.5, float("inf"), float("nan")):
            changes.append((lambda o, r, f=f, bad=bad: setattr(o, f, bad), f + " is negative or not finite"))
    for bad in (float("inf"), float("nan")):
        changes.append((lambda o, r, bad=bad: setattr(o, "cos_max_rotation_error", bad), "cos_max_rotation_error"))
    for change, word in changes:
        o, r = fresh(); change(o, r)
        assert call(o, r) == -2 and word in L.xm_last_error().decode(), word
    o, r = fresh()
    assert call(None, r) == -2 and call(o, None) == -2 and "null" in L.xm_last_error().decode()
    assert call(o, r, n=-1) == -2 and call(o, r, npairs=-1) == -2 and "negative size" in L.xm_last_error().decode()
    assert call(o, r, n=2 ** 31) == -2 and "2^31" in L.xm_last_error().decode() and call(o, r, npairs=2 ** 31) == -2
    for key in ("foff", "xy", "pi", "pj", "model", "moff", "f1", "f2", "inlier", "pair_inliers", "pair_status", "registered_out", "moff_out", "f1_out", "f2_out",
                "focal", "Rrel", "trel"):
        assert call(o, r, **{key: None}) == -2 and "null" in L.xm_last_error().decode(), key
    for kw, word in ((dict(foff=i64(0, 3, 2)), "foff decreases"), (dict(foff=i64(1, 2, 4)), "foff does not start"),
                     (dict(foff=i64(0, 2, 2 ** 31)), "features must stay below 2^31"), (dict(moff=i64(1, 1)), "moff does not start"),
                     (dict(moff=i64(0, -1)), "moff decreases"), (dict(moff=i64(0, 2 ** 31)), "matches must stay below 2^31"),
                     (dict(pj=i32(0)), "names one image twice"), (dict(pi=i32(2)), "image index out of range"), (dict(pj=i32(-1)), "image index out of range"),
                     (dict(model=i32(4)), "unknown model"), (dict(model=i32(-1)), "unknown model"),
                     (dict(model=i32(2), FH=None), "FH is null"), (dict(model=i32(3), FH=None), "FH is null"),
                     (dict(Kinv=None, bearing=None), "Kinv and bearing are both null"), (dict(rot=np.zeros((2, 3, 3)), Rrel=None), "null")):
        assert call(o, r, **kw) == -2 and word in L.xm_last_error().decode(), word
    assert L.xm_view_graph_limits(None) == -2
