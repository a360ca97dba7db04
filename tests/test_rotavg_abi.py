"""CPU tests of the robust rotation averaging's ABI: include/xm_amd.h and the binding agree (sizes, offsets, defaults, constants), the
prototypes compile with -Werror, the symbols are exported, and every refusal of rule 11 is made on the host, before a device is looked for,
and leaves the outputs untouched."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import xm_rotavg_numpy as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "weight_type", "max_num_irls_iterations", "fixed_image", "irls_step_convergence_threshold", "irls_loss_parameter_sigma")
RES_FIELDS = ("struct_size", "stop_reason", "irls_iterations", "reserved", "pcg_iterations", "pcg_capped", "pairs", "registered", "fixed_image",
              "cams_heavy", "max_incidences", "seconds_index", "seconds_kernels", "seconds_download")
PROBE_FIELDS = ("struct_size", "reserved", "angle_axis", "x", "weight_in", "rot", "residual", "gauge", "weight", "rhs", "diagonal", "product",
                "angle_axis_out", "step")
CODES = ("XM_VGR_GEMAN_MCCLURE", "XM_VGR_HALF_NORM", "XM_VGR_STOP_NOTHING", "XM_VGR_STOP_STEP", "XM_VGR_STOP_ITERATIONS", "XM_VGR_STOP_NONFINITE")
PROTO = (" int (*f)(int64_t, const uint8_t *, const double *, int64_t, const int32_t *, const int32_t *, const double *, const uint8_t *,"
         " const xm_vgr_options_t *, double *, double *, double *, double *, double *, xm_vgr_result_t *) = xm_view_graph_rotations; (void)f;"
         " int (*g)(int64_t, const uint8_t *, const double *, int64_t, const int32_t *, const int32_t *, const double *, const uint8_t *,"
         " const xm_vgr_options_t *, xm_vgr_probe_t *) = xm_view_graph_rotations_probe; (void)g;"
         " int (*h)(int64_t *) = xm_view_graph_rotations_limits; (void)h;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){ xm_vgr_options_t o = XM_VGR_OPTIONS_INIT;\n'
           'printf("%zu %zu %zu %d", sizeof(xm_vgr_options_t), sizeof(xm_vgr_result_t), sizeof(xm_vgr_probe_t), XM_ABI_REVISION);\n'
           + "".join(f' printf(" %d", (int){c});\n' for c in CODES)
           + 'printf(" %u %d %d %d %.17g %.17g", o.struct_size, o.weight_type, o.max_num_irls_iterations, o.fixed_image,'
             ' o.irls_step_convergence_threshold, o.irls_loss_parameter_sigma);\n'
           + "".join(f' printf(" %zu", offsetof(xm_vgr_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_vgr_result_t, {f}));\n' for f in RES_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_vgr_probe_t, {f}));\n' for f in PROBE_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
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
    assert C.sizeof(xmamd.VgrOptions) == so == 32 and C.sizeof(xmamd.VgrResult) == sr and C.sizeof(xmamd.VgrProbe) == sp
    codes = list(map(int, v[4:4 + len(CODES)]))
    assert codes == [xmamd.VGR_GEMAN_MCCLURE, xmamd.VGR_HALF_NORM, xmamd.VGR_STOP_NOTHING, xmamd.VGR_STOP_STEP, xmamd.VGR_STOP_ITERATIONS,
                     xmamd.VGR_STOP_NONFINITE] == [0, 1, 0, 1, 2, 3]
    assert codes == [rn.GEMAN_MCCLURE, rn.HALF_NORM, rn.STOP_NOTHING, rn.STOP_STEP, rn.STOP_ITERATIONS, rn.STOP_NONFINITE]
    assert sorted(xmamd.VGR_STOP) == [0, 1, 2, 3] and xmamd.VGR_WEIGHT_TYPES == dict(geman_mcclure=0, half_norm=1)
    # the defaults are those of RotationEstimatorOptions (global_rotation_averaging.h); fixed_image -1: the smallest registered index
    at = 4 + len(CODES)
    want = [32, 0, 100, -1, 1e-3, 5.0]
    assert [float(x) for x in v[at:at + 6]] == want
    o = xmamd.VgrOptions()
    assert [getattr(o, f) for f in OPT_FIELDS] == want
    offs = [getattr(xmamd.VgrOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.VgrResult, f).offset for f in RES_FIELDS] + \
           [getattr(xmamd.VgrProbe, f).offset for f in PROBE_FIELDS]
    assert offs == list(map(int, v[at + 6:]))
    assert tuple(f for f, _ in xmamd.VgrOptions._fields_) == OPT_FIELDS and tuple(f for f, _ in xmamd.VgrResult._fields_) == RES_FIELDS
    assert tuple(f for f, _ in xmamd.VgrProbe._fields_) == PROBE_FIELDS


def test_exports_and_limits(xmamd):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_view_graph_rotations", "xm_view_graph_rotations_probe", "xm_view_graph_rotations_limits"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    lim = xmamd.view_graph_rotations_limits()                                     # needs no device
    assert lim == dict(light_incidences=rn.LIGHT_INCIDENCES, threads=256, pcg_iterations=rn.PCG_CAP)
    spare = np.full(4, 7, dtype=np.int64)
    assert xmamd.lib().xm_view_graph_rotations_limits(spare.ctypes.data_as(C.c_void_p)) == 0 and spare[3] == 0
    assert xmamd.lib().xm_view_graph_rotations_limits(None) == -2
    for f in ("view_graph_rotations", "view_graph_rotations_probe", "RotationPlan"):
        assert hasattr(xmamd, f)


SENTINEL = 7.25


def _raw_call(xmamd, g, opt=None, res_size=None, null=(), n=None, npairs=None):
    """xm_view_graph_rotations through ctypes with outputs full of a sentinel -> the return code, whether every output is untouched, the outputs"""
    a = dict(rot0=np.ascontiguousarray(g["rot0"], dtype=np.float64), pi=np.ascontiguousarray(g["pi"], dtype=np.int32),
             pj=np.ascontiguousarray(g["pj"], dtype=np.int32), Rrel=np.ascontiguousarray(g["Rrel"], dtype=np.float64),
             registered=None if g.get("registered") is None else np.ascontiguousarray(g["registered"], dtype=np.uint8),
             valid=None if g.get("valid_in") is None else np.ascontiguousarray(g["valid_in"], dtype=np.uint8))
    ni, nk = a["rot0"].size // 9, a["pi"].size
    outs = dict(rot_out=np.full(9 * ni, SENTINEL), angle_axis_out=np.full(3 * ni, SENTINEL), residual=np.full(3 * nk, SENTINEL),
                weight=np.full(nk, SENTINEL), step_trace=np.full(100, SENTINEL))
    opt = xmamd.VgrOptions() if opt is None else opt
    res = xmamd.VgrResult()
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    res.struct_size = C.sizeof(res) if res_size is None else res_size
    before = bytes(res)
    P = lambda k, x: None if (x is None or k in null) else x.ctypes.data_as(C.c_void_p)
    rc = xmamd.lib().xm_view_graph_rotations(ni if n is None else n, P("registered", a["registered"]), P("rot0", a["rot0"]), nk if npairs is None else npairs,
                                             P("pi", a["pi"]), P("pj", a["pj"]), P("Rrel", a["Rrel"]), P("valid", a["valid"]),
                                             None if "opt" in null else C.byref(opt),
                                             *[P(k, outs[k]) for k in ("rot_out", "angle_axis_out", "residual", "weight", "step_trace")], C.byref(res))
    untouched = all((v == SENTINEL).all() for v in outs.values()) and bytes(res) == before
    return rc, untouched, outs, res


def _base():
    g = rn.make_graph(6, 10, 3, 1.0, 0.0)
    g["valid_in"] = np.ones(10, dtype=np.uint8)
    g["registered"] = np.ones(6, dtype=np.uint8)
    return g


def _mod(key, idx, value):
    g = _base()
    g[key] = np.array(g[key]).copy()
    g[key][idx] = value
    return g


def _opt(xmamd, **kw):
    o = xmamd.VgrOptions()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _apart():
    g = _base()
    g["valid_in"] = ((g["pi"] < 3) == (g["pj"] < 3)).astype(np.uint8)                  # images 0 .. 2 and 3 .. 5 fall apart
    return g


def _islet():
    g = _base()
    g["valid_in"] = ((g["pi"] != 4) & (g["pj"] != 4)).astype(np.uint8)                 # image 4 is registered and in no participating pair
    return g


REFUSALS = {
    "image index out of range": lambda x: dict(g=_mod("pi", 3, 6)),
    "negative image index": lambda x: dict(g=_mod("pj", 1, -1)),
    "index out of range in an invalid pair": lambda x: dict(g=dict(_mod("pi", 9, 7), valid_in=(np.arange(10) != 9).astype(np.uint8))),
    "pi == pj": lambda x: dict(g=_mod("pj", 0, int(_base()["pi"][0]))),
    "unknown weight type": lambda x: dict(g=_base(), opt=_opt(x, weight_type=2)),
    "negative weight type": lambda x: dict(g=_base(), opt=_opt(x, weight_type=-1)),
    "max_num_irls_iterations is zero": lambda x: dict(g=_base(), opt=_opt(x, max_num_irls_iterations=0)),
    "threshold is zero": lambda x: dict(g=_base(), opt=_opt(x, irls_step_convergence_threshold=0.0)),
    "threshold is nan": lambda x: dict(g=_base(), opt=_opt(x, irls_step_convergence_threshold=np.nan)),
    "threshold is inf": lambda x: dict(g=_base(), opt=_opt(x, irls_step_convergence_threshold=np.inf)),
    "sigma is negative": lambda x: dict(g=_base(), opt=_opt(x, irls_loss_parameter_sigma=-5.0)),
    "sigma is nan": lambda x: dict(g=_base(), opt=_opt(x, irls_loss_parameter_sigma=np.nan)),
    "sigma is inf": lambda x: dict(g=_base(), opt=_opt(x, irls_loss_parameter_sigma=np.inf)),
    "rot0 is nan": lambda x: dict(g=_mod("rot0", (4, 1, 2), np.nan)),
    "rot0 is inf": lambda x: dict(g=_mod("rot0", (0, 0, 0), np.inf)),
    "Rrel is nan": lambda x: dict(g=_mod("Rrel", (7, 2, 2), np.nan)),
    "Rrel is inf": lambda x: dict(g=_mod("Rrel", (0, 0, 1), -np.inf)),
    "options struct_size": lambda x: dict(g=_base(), opt=_opt(x, struct_size=24)),
    "result struct_size": lambda x: dict(g=_base(), res_size=8),
    "null options": lambda x: dict(g=_base(), null=("opt",)),
    "null rot0": lambda x: dict(g=_base(), null=("rot0",)),
    "null pi": lambda x: dict(g=_base(), null=("pi",)),
    "null pj": lambda x: dict(g=_base(), null=("pj",)),
    "null Rrel": lambda x: dict(g=_base(), null=("Rrel",)),
    "null rot_out": lambda x: dict(g=_base(), null=("rot_out",)),
    "null angle_axis_out": lambda x: dict(g=_base(), null=("angle_axis_out",)),
    "null residual": lambda x: dict(g=_base(), null=("residual",)),
    "null weight": lambda x: dict(g=_base(), null=("weight",)),
    "null step_trace": lambda x: dict(g=_base(), null=("step_trace",)),
    "images at 2^31": lambda x: dict(g=_base(), n=1 << 31),
    "pairs at 2^31": lambda x: dict(g=_base(), npairs=1 << 31),
    "negative images": lambda x: dict(g=_base(), n=-1),
    "fixed_image unregistered": lambda x: dict(g=_mod("registered", 2, 0), opt=_opt(x, fixed_image=2)),
    "fixed_image out of range": lambda x: dict(g=_base(), opt=_opt(x, fixed_image=6)),
    "fixed_image below -1": lambda x: dict(g=_base(), opt=_opt(x, fixed_image=-2)),
    "two components": lambda x: dict(g=_apart()),
    "a registered image without a pair": lambda x: dict(g=_islet()),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_leave_the_outputs_untouched(xmamd, case):
    kw = REFUSALS[case](xmamd)
    rc, untouched, _, _ = _raw_call(xmamd, **kw)
    assert rc == -2, xmamd.lib().xm_last_error()
    assert untouched
    if not (set(kw) & {"opt", "res_size", "null", "n", "npairs"}):                    # the restatement refuses the same graphs
        with pytest.raises(rn.Refused):
            rn.irls_sequential(kw["g"])


def test_what_takes_no_part_is_not_checked(xmamd):
    """only a registered image's rot0 and a participating pair's Rrel must be finite: the same NaN elsewhere passes the checks (and the
    call then needs a device: XM_ERR_HIP without one)"""
    g = _mod("Rrel", (7, 2, 2), np.nan)
    g["valid_in"][7] = 0
    assert _raw_call(xmamd, g)[0] in (0, -3)
    g = _base()                                      # image 5 leaves; the chain 0 .. 4 still connects the rest
    g["registered"][5] = 0
    g["rot0"] = g["rot0"].copy(); g["rot0"][5, 0, 0] = np.nan
    assert _raw_call(xmamd, g)[0] in (0, -3)


def test_no_participating_pair_needs_no_device(xmamd):
    g = _base()
    g["valid_in"] = np.zeros(10, dtype=np.uint8)
    g["registered"][3] = 0
    rc, untouched, o, res = _raw_call(xmamd, g)
    assert rc == 0 and not untouched
    assert np.array_equal(o["rot_out"].reshape(6, 3, 3), g["rot0"]) and not o["residual"].any() and not o["weight"].any() and not o["step_trace"].any()
    assert res.stop_reason == xmamd.VGR_STOP_NOTHING and res.irls_iterations == 0 and res.pairs == 0 and res.registered == 5 and res.fixed_image == 0
    assert res.pcg_iterations == 0 and res.cams_heavy == 0 and res.max_incidences == 0
    aa = o["angle_axis_out"].reshape(6, 3)
    ref = rn.irls_sequential(g)
    assert not aa[3].any() and np.max(np.abs(aa - ref["angle_axis"])) <= 16 * np.finfo(np.float64).eps * np.pi
    plan = xmamd.view_graph_rotations(**rn.call_inputs(g))
    assert plan.info["stop"] == "nothing" and plan.step_trace.size == 0 and np.array_equal(plan.rot, g["rot0"])
    empty = xmamd.view_graph_rotations(np.zeros((0, 3, 3)), [], [], np.zeros((0, 3, 3)))
    assert empty.rot.shape == (0, 3, 3) and empty.info["fixed_image"] == -1


def test_probe_refusals(xmamd):
    g = _base()
    aa = np.zeros((6, 3))
    with pytest.raises(xmamd.XmError):
        xmamd.view_graph_rotations_probe(**rn.call_inputs(_mod("pi", 3, 9)), angle_axis=aa)
    with pytest.raises(xmamd.XmError):
        xmamd.view_graph_rotations_probe(**rn.call_inputs(g), angle_axis=np.full((6, 3), np.nan))
    with pytest.raises(xmamd.XmError):
        xmamd.view_graph_rotations_probe(**rn.call_inputs(g), angle_axis=aa, x=np.full((6, 3), np.inf))
    with pytest.raises(xmamd.XmError):
        xmamd.view_graph_rotations_probe(**rn.call_inputs(_apart()), angle_axis=aa)
    with pytest.raises(xmamd.XmError):
        xmamd.view_graph_rotations_probe(**rn.call_inputs(g), angle_axis=aa, weight_type="tukey")
    q = xmamd.VgrProbe(8, 0)
    assert xmamd.lib().xm_view_graph_rotations_probe(0, None, None, 0, None, None, None, None, C.byref(xmamd.VgrOptions()), C.byref(q)) == -2
