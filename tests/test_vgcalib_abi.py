"""CPU tests of the view-graph calibration's ABI: include/xm_amd.h and the binding agree (sizes, offsets, defaults, constants), the symbols
are exported, and every refusal is made on the host, before a device is looked for, and leaves the outputs untouched."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import xm_vgcalib_numpy as vn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "flags", "thres_loss_function", "thres_lower_ratio", "thres_higher_ratio", "thres_two_view_error", "max_num_iterations",
              "reserved", "function_tolerance", "lower_bound")
RES_FIELDS = ("struct_size", "stop_reason", "pairs", "pairs_same_camera", "cams_free", "cams_constant", "cams_rejected", "pairs_invalidated",
              "pairs_flipped", "cams_heavy", "max_incidences", "pcg_iterations", "iterations", "accepted", "trace_len", "reserved", "initial_cost",
              "final_cost", "seconds_index", "seconds_kernels", "seconds_download")
PROBE_FIELDS = ("struct_size", "reserved", "focal", "x", "d_in", "mu", "d", "residual", "record", "cost", "gradient", "diagonal", "product")
CODES = ("XM_VGC_UPDATE_CONFIG", "XM_VGC_VALID", "XM_VGC_INVALID_IN", "XM_VGC_TWO_VIEW_ERROR", "XM_VGC_CAM_UNUSED", "XM_VGC_CAM_CONSTANT",
         "XM_VGC_CAM_REFINED", "XM_VGC_CAM_REJECTED")
PROTO = (" int (*f)(int64_t, const double *, const double *, const uint8_t *, int64_t, const int32_t *, int64_t, const int32_t *, const int32_t *,"
         " const int32_t *, const double *, const uint8_t *, const double *, const double *, const xm_vgc_options_t *, double *, double *, uint8_t *,"
         " int32_t *, int32_t *, double *, double *, int32_t *, double *, double *, xm_vgc_result_t *) = xm_view_graph_calibrate; (void)f;"
         " int (*g)(int64_t, const double *, const double *, const uint8_t *, int64_t, const int32_t *, int64_t, const int32_t *, const int32_t *,"
         " const int32_t *, const double *, const uint8_t *, const xm_vgc_options_t *, xm_vgc_probe_t *) = xm_view_graph_calibrate_probe; (void)g;"
         " int (*h)(int64_t *) = xm_view_graph_calibrate_limits; (void)h;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){ xm_vgc_options_t o = XM_VGC_OPTIONS_INIT;\n'
           'printf("%zu %zu %zu %d", sizeof(xm_vgc_options_t), sizeof(xm_vgc_result_t), sizeof(xm_vgc_probe_t), XM_ABI_REVISION);\n'
           + "".join(f' printf(" %d", (int){c});\n' for c in CODES)
           + 'printf(" %u %u %.17g %.17g %.17g %.17g %d %d %.17g %.17g", o.struct_size, o.flags, o.thres_loss_function, o.thres_lower_ratio,'
             ' o.thres_higher_ratio, o.thres_two_view_error, o.max_num_iterations, o.reserved, o.function_tolerance, o.lower_bound);\n'
           + "".join(f' printf(" %zu", offsetof(xm_vgc_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_vgc_result_t, {f}));\n' for f in RES_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_vgc_probe_t, {f}));\n' for f in PROBE_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return subprocess.check_output([os.path.join(d, "t")]).split()


def test_header_and_binding_agree(xmamd):
    v = _c_values()
    so, sr, sp, rev = map(int, v[:4])
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # added exports: the revision stays
    assert C.sizeof(xmamd.VgcOptions) == so == 64 and C.sizeof(xmamd.VgcResult) == sr and C.sizeof(xmamd.VgcProbe) == sp
    codes = list(map(int, v[4:4 + len(CODES)]))
    assert codes == [xmamd.VGC_UPDATE_CONFIG, xmamd.VGC_VALID, xmamd.VGC_INVALID_IN, xmamd.VGC_TWO_VIEW_ERROR, xmamd.VGC_CAM_UNUSED,
                     xmamd.VGC_CAM_CONSTANT, xmamd.VGC_CAM_REFINED, xmamd.VGC_CAM_REJECTED] == [1, 0, 1, 2, 0, 1, 2, 3]
    assert codes[1:] == [vn.VALID, vn.INVALID_IN, vn.TWO_VIEW_ERROR, vn.CAM_UNUSED, vn.CAM_CONSTANT, vn.CAM_REFINED, vn.CAM_REJECTED]
    # the defaults are view_graph_calibration.h:21-23, optimization_base.h:21-26 and view_graph_calibration.cc:113
    at = 4 + len(CODES)
    want = [64, 0, 1e-2, 0.1, 10.0, 2.0, 100, 0, 1e-5, 1e-3]
    assert [float(x) for x in v[at:at + 10]] == want
    o = xmamd.VgcOptions()
    assert [getattr(o, f) for f in OPT_FIELDS] == want
    assert {k: vn.DEFAULTS[k] for k in OPT_FIELDS[2:6] + OPT_FIELDS[6:7] + OPT_FIELDS[8:]} == dict(zip(OPT_FIELDS[2:7] + OPT_FIELDS[8:], want[2:7] + want[8:]))
    offs = [getattr(xmamd.VgcOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.VgcResult, f).offset for f in RES_FIELDS] + \
           [getattr(xmamd.VgcProbe, f).offset for f in PROBE_FIELDS]
    assert offs == list(map(int, v[at + 10:]))
    assert tuple(f for f, _ in xmamd.VgcResult._fields_) == RES_FIELDS and tuple(f for f, _ in xmamd.VgcProbe._fields_) == PROBE_FIELDS


def test_exports_and_limits(xmamd):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_view_graph_calibrate", "xm_view_graph_calibrate_probe", "xm_view_graph_calibrate_limits"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    lim = xmamd.view_graph_calibrate_limits()                                     # needs no device
    assert lim == dict(light_incidences=64, threads=256, svd_sweeps=30, pcg_iterations=vn.MAX_PCG)
    assert xmamd.lib().xm_view_graph_calibrate_limits(None) == -2


SENTINEL = 7.25


def _raw_call(xmamd, g, opt=None, res_size=None, null=(), Rrel=None, trel=None):
    """xm_view_graph_calibrate through ctypes with outputs full of a sentinel -> the return code and whether every output is untouched"""
    ncams, n, npairs = len(g["focal0"]), len(g["cam_of_image"]), len(g["pi"])
    a = dict(focal0=np.ascontiguousarray(g["focal0"], dtype=np.float64), pp=np.ascontiguousarray(g["pp"], dtype=np.float64),
             has_prior=np.ascontiguousarray(g["has_prior"], dtype=np.uint8), cam=np.ascontiguousarray(g["cam_of_image"], dtype=np.int32),
             pi=np.ascontiguousarray(g["pi"], dtype=np.int32), pj=np.ascontiguousarray(g["pj"], dtype=np.int32),
             model=np.ascontiguousarray(g["model"], dtype=np.int32), F=np.ascontiguousarray(g["F"], dtype=np.float64),
             valid=None if g["valid_in"] is None else np.ascontiguousarray(g["valid_in"], dtype=np.uint8),
             Rrel=None if Rrel is None else np.ascontiguousarray(Rrel, dtype=np.float64), trel=None if trel is None else np.ascontiguousarray(trel, dtype=np.float64))
    outs = dict(focal_out=np.full(ncams, SENTINEL), focal_est=np.full(ncams, SENTINEL), refined=np.full(ncams, 7, dtype=np.uint8),
                cam_status=np.full(ncams, 7, dtype=np.int32), pair_status=np.full(npairs, 7, dtype=np.int32), residual=np.full(2 * npairs, SENTINEL),
                d_out=np.full(8 * npairs, SENTINEL), model_out=np.full(npairs, 7, dtype=np.int32), F_out=np.full(9 * npairs, SENTINEL),
                trace=np.full(101, SENTINEL))
    opt = xmamd.VgcOptions() if opt is None else opt
    res = xmamd.VgcResult()
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    res.struct_size = C.sizeof(res) if res_size is None else res_size
    before = bytes(res)
    P = lambda k, x: None if (x is None or k in null) else x.ctypes.data_as(C.c_void_p)
    rc = xmamd.lib().xm_view_graph_calibrate(ncams, P("focal0", a["focal0"]), P("pp", a["pp"]), P("has_prior", a["has_prior"]), n, P("cam", a["cam"]), npairs,
                                             P("pi", a["pi"]), P("pj", a["pj"]), P("model", a["model"]), P("F", a["F"]), P("valid", a["valid"]),
                                             P("Rrel", a["Rrel"]), P("trel", a["trel"]), None if "opt" in null else C.byref(opt),
                                             *[P(k, outs[k]) for k in ("focal_out", "focal_est", "refined", "cam_status", "pair_status", "residual", "d_out",
                                                                       "model_out", "F_out", "trace")], C.byref(res))
    untouched = all((v == (SENTINEL if v.dtype == np.float64 else 7)).all() for v in outs.values()) and bytes(res) == before
    return rc, untouched


def _base():
    g = vn.make_graph(5, 8, 3)
    g["valid_in"] = np.ones(8, dtype=np.uint8)
    return g


def _mod(key, idx, value):
    g = _base()
    g[key] = np.array(g[key]).copy()
    g[key][idx] = value
    return g


def _opt(xmamd, **kw):
    o = xmamd.VgcOptions()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


REFUSALS = {
    "camera index out of range": lambda x: dict(g=_mod("cam_of_image", 2, 5)),
    "negative camera index": lambda x: dict(g=_mod("cam_of_image", 0, -1)),
    "image index out of range": lambda x: dict(g=_mod("pi", 3, 5)),
    "negative image index": lambda x: dict(g=_mod("pj", 1, -1)),
    "pi == pj": lambda x: dict(g=_mod("pj", 0, int(_base()["pi"][0]))),
    "unknown model": lambda x: dict(g=_mod("model", 2, 4)),
    "negative model": lambda x: dict(g=_mod("model", 2, -1)),
    "unknown flag": lambda x: dict(g=_base(), opt=_opt(x, flags=2)),
    "F is nan": lambda x: dict(g=_mod("F", (4, 1, 2), np.nan)),
    "F is inf": lambda x: dict(g=_mod("F", (0, 0, 0), np.inf)),
    "focal0 is zero": lambda x: dict(g=_mod("focal0", 1, 0.0)),
    "focal0 is negative": lambda x: dict(g=_mod("focal0", 1, -800.0)),
    "focal0 is nan": lambda x: dict(g=_mod("focal0", 4, np.nan)),
    "focal0 is inf": lambda x: dict(g=_mod("focal0", 4, np.inf)),
    "thres_loss_function is zero": lambda x: dict(g=_base(), opt=_opt(x, thres_loss_function=0.0)),
    "thres_lower_ratio is nan": lambda x: dict(g=_base(), opt=_opt(x, thres_lower_ratio=np.nan)),
    "thres_higher_ratio is inf": lambda x: dict(g=_base(), opt=_opt(x, thres_higher_ratio=np.inf)),
    "thres_two_view_error is negative": lambda x: dict(g=_base(), opt=_opt(x, thres_two_view_error=-2.0)),
    "function_tolerance is zero": lambda x: dict(g=_base(), opt=_opt(x, function_tolerance=0.0)),
    "lower_bound is negative": lambda x: dict(g=_base(), opt=_opt(x, lower_bound=-1e-3)),
    "max_num_iterations is zero": lambda x: dict(g=_base(), opt=_opt(x, max_num_iterations=0)),
    "lower ratio above higher ratio": lambda x: dict(g=_base(), opt=_opt(x, thres_lower_ratio=11.0)),
    "update_config without Rrel and trel": lambda x: dict(g=_base(), opt=_opt(x, flags=1)),
    "update_config without trel": lambda x: dict(g=_base(), opt=_opt(x, flags=1), Rrel=_base()["Rrel"]),
    "options struct_size": lambda x: dict(g=_base(), opt=_opt(x, struct_size=56)),
    "result struct_size": lambda x: dict(g=_base(), res_size=8),
    "null options": lambda x: dict(g=_base(), null=("opt",)),
    "null focal0": lambda x: dict(g=_base(), null=("focal0",)),
    "null pp": lambda x: dict(g=_base(), null=("pp",)),
    "null has_prior": lambda x: dict(g=_base(), null=("has_prior",)),
    "null cam_of_image": lambda x: dict(g=_base(), null=("cam",)),
    "null pi": lambda x: dict(g=_base(), null=("pi",)),
    "null model": lambda x: dict(g=_base(), null=("model",)),
    "null F": lambda x: dict(g=_base(), null=("F",)),
    "null focal_out": lambda x: dict(g=_base(), null=("focal_out",)),
    "null cam_status": lambda x: dict(g=_base(), null=("cam_status",)),
    "null pair_status": lambda x: dict(g=_base(), null=("pair_status",)),
    "null residual": lambda x: dict(g=_base(), null=("residual",)),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_leave_the_outputs_untouched(xmamd, case):
    rc, untouched = _raw_call(xmamd, **REFUSALS[case](xmamd))
    assert rc == -2, xmamd.lib().xm_last_error()
    assert untouched


def test_counts_at_2_to_the_31(xmamd):
    """counts >= 2^31 are refused before any array is read (the arrays here are far shorter)"""
    L = xmamd.lib()
    opt = xmamd.VgcOptions(); res = xmamd.VgcResult(); res.struct_size = C.sizeof(res)
    one = np.ones(4); P = lambda a: a.ctypes.data_as(C.c_void_p)
    i32 = np.zeros(4, dtype=np.int32); u8 = np.zeros(4, dtype=np.uint8)
    for ncams, n, npairs in ((1 << 31, 1, 1), (1, 1 << 31, 1), (1, 1, 1 << 31), (-1, 1, 1)):
        rc = L.xm_view_graph_calibrate(ncams, P(one), P(one), P(u8), n, P(i32), npairs, P(i32), P(i32), P(i32), P(one), None, None, None, C.byref(opt),
                                       P(one), P(one), P(u8), P(i32), P(i32), P(one), None, None, None, None, C.byref(res))
        assert rc == -2
    assert (one == 1).all() and not i32.any() and not u8.any()


def test_invalid_pairs_are_not_checked_for_finite_F(xmamd):
    """only a participating pair's F must be finite: the same NaN in an invalid pair or an H pair passes the checks (and then needs a device)"""
    g = _mod("F", (4, 1, 2), np.nan)
    g["valid_in"][4] = 0
    rc, _ = _raw_call(xmamd, g)
    assert rc in (0, -3)
    g = _mod("F", (4, 1, 2), np.nan)
    g["model"] = g["model"].copy(); g["model"][4] = vn.MODEL_H
    rc, _ = _raw_call(xmamd, g)
    assert rc in (0, -3)


def test_probe_refusals(xmamd):
    g = _base()
    with pytest.raises(xmamd.XmError):
        xmamd.view_graph_calibrate_probe(**vn.call_inputs(_mod("pi", 3, 9)), focal=g["focal0"])
    with pytest.raises(xmamd.XmError):
        xmamd.view_graph_calibrate_probe(**vn.call_inputs(g), focal=g["focal0"] * 0.0)
    with pytest.raises(xmamd.XmError):
        xmamd.view_graph_calibrate_probe(**vn.call_inputs(g), focal=g["focal0"], mu=-1.0)
