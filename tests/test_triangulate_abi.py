"""CPU tests of the ABI of xm_ctx_triangulate_tracks / xm_triangulate_limits (include/xm_amd.h): prototypes, structs and constants compile
from the header and agree with the binding, both symbols are exported, the ABI revision stays where it was (added exports), and the
wrappers refuse bad arguments before any device is looked at."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

import xm_trackfilter_numpy as tf
import xm_triangulate_numpy as tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "max_hypotheses", "min_angle", "create_max_angle_error", "complete_max_reproj_error", "min_views", "refine_rounds")
RES_FIELDS = ("struct_size", "reserved") + tri.COUNTS + ("cos_min_angle", "cos_create", "seconds_kernels", "seconds_download")
CONSTANTS = ("XM_TRI_LM_ACCEPTED", "XM_TRI_LM_UNUSED", "XM_TRI_LM_NO_HYPOTHESIS", "XM_TRI_LM_DEGENERATE", "XM_TRI_LM_MIN_VIEWS", "XM_TRI_LM_ANGLE",
             "XM_TRI_REASON_NOT_CANDIDATE", "XM_TRI_REASON_NOT_MEMBER", "XM_TRI_REASON_LANDMARK")
PROTO = (" int (*f)(xm_ctx_t *, const xm_tri_options_t *, const double *, const double *, double *, const uint8_t *, uint8_t *, uint8_t *, int32_t *,"
         " uint8_t *, int32_t *, int32_t *, xm_tri_result_t *) = xm_ctx_triangulate_tracks; (void)f; int (*g)(int64_t *) = xm_triangulate_limits; (void)g;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){xm_tri_options_t d = XM_TRI_OPTIONS_INIT;\n'
           'printf("%zu %zu %d", sizeof(xm_tri_options_t), sizeof(xm_tri_result_t), XM_ABI_REVISION);\n'
           'printf(" %d %d %d %d %d %d", (int)d.struct_size, d.max_hypotheses, d.min_views, d.refine_rounds, (int)(d.min_angle * 100 + d.create_max_angle_error),'
           ' (int)(d.complete_max_reproj_error * 1e6 + 0.5));\n'
           + "".join(f' printf(" %d", (int)({c}));\n' for c in CONSTANTS)
           + "".join(f' printf(" %zu", offsetof(xm_tri_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_tri_result_t, {f}));\n' for f in RES_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    so, sr, rev, *rest = _c_values()
    init, rest = rest[:6], rest[6:]
    consts, offs = rest[:len(CONSTANTS)], rest[len(CONSTANTS):]
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # added exports: the revision stays
    assert ctypes.sizeof(xmamd.TriOptions) == so == 40 and ctypes.sizeof(xmamd.TriResult) == sr == 136
    assert init == [so, 64, 2, 2, 102, 10000]                                     # XM_TRI_OPTIONS_INIT: 64, 1.0, 2.0, 1e-2, 2, 2
    d = tri.DEFAULTS
    assert (d["max_hypotheses"], d["min_angle"], d["create_angle"], d["complete_reprojection"], d["min_views"], d["refine_rounds"]) == (64, 1.0, 2.0, 1e-2, 2, 2)
    assert [getattr(xmamd.TriOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.TriResult, f).offset for f in RES_FIELDS] == offs
    assert consts == [getattr(xmamd, c[3:]) for c in CONSTANTS]
    assert consts == [tri.LM_ACCEPTED, tri.LM_UNUSED, tri.LM_NO_HYPOTHESIS, tri.LM_DEGENERATE, tri.LM_MIN_VIEWS, tri.LM_ANGLE,
                      tri.REASON_NOT_CANDIDATE, tri.REASON_NOT_MEMBER, tri.REASON_LANDMARK] == [0, 1, 2, 3, 4, 5, 1, 2, 4]
    assert xmamd.TRI_COUNTS == tri.COUNTS


def test_both_are_exported_and_the_limits_are_those_of_the_scenes(xmamd):
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_ctx_triangulate_tracks", "xm_triangulate_limits"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    lim = xmamd.triangulate_limits()                                              # host-only
    assert lim == dict(light_max=tf.LIGHT_MAX, tile=tf.TILE, threads=256)
    assert xmamd.lib().xm_triangulate_limits(None) == -2


def test_wrapper_arguments(xmamd):
    sig = inspect.signature(xmamd.Context.triangulate_tracks).parameters
    names = ["self", "rot", "t", "P", "candidates", "max_hypotheses", "min_angle", "create_angle", "complete_reprojection", "min_views", "refine_rounds"]
    assert list(sig) == names and [sig[k].default for k in names[3:]] == [None, None, 64, 1.0, 2.0, 1e-2, 2, 2]
    sig = inspect.signature(xmamd.Context.retriangulate).parameters
    names = ["self", "rot", "t", "P", "rounds", "weights", "restore_weights", "reprojection", "triangulation", "min_views", "bundle_adjust_kwargs"]
    assert list(sig) == names and [sig[k].default for k in names[4:10]] == [1, None, False, 1e-2, 1.0, 0]
    ctx = xmamd.Context.__new__(xmamd.Context)
    ctx.n, ctx.n_landmarks, ctx.ne, ctx.h = 1, 1, 1, None
    g = (np.eye(3), np.zeros((3, 1)))
    for kw, word in ((dict(min_angle=0.0), "min_angle"), (dict(create_angle=-1.0), "create_angle"), (dict(complete_reprojection=float("nan")), "complete_reprojection"),
                     (dict(max_hypotheses=0), "max_hypotheses"), (dict(refine_rounds=0), "refine_rounds"), (dict(min_views=-1), "min_views"),
                     (dict(candidates=np.ones(2, dtype=bool)), "candidates")):
        with pytest.raises(xmamd.XmError, match=word):    # no device: the arguments are checked before anything else is looked at
            ctx.triangulate_tracks(*g, **kw)
    with pytest.raises(xmamd.XmError, match="rounds"):
        ctx.retriangulate(*g, np.zeros((3, 1)), rounds=-1)
    with pytest.raises(xmamd.XmError, match="weights"):   # (this context never learnt its weights)
        ctx.retriangulate(*g, np.zeros((3, 1)))
    ctx.h = None   # nothing to destroy
    plan = xmamd.TriangulationPlan(np.zeros((3, 1)), np.array([True, False, False]), np.array([0, 2, 1], dtype=np.uint8), np.zeros(1, np.int32),
                                   np.zeros(1, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32), {})
    assert plan.weights([3.0, 2.0, 0.0]).tolist() == [3.0, 0.0, 0.0]
    assert [a.tolist() for a in plan.apply(np.arange(3), np.arange(6).reshape(3, 2))] == [[0], [[0, 1]]]
    for bad in (lambda: plan.weights(np.ones(2)), lambda: plan.apply(np.ones(2))):
        with pytest.raises(xmamd.XmError):
            bad()


def test_library_refusals_need_no_device(xmamd):
    """null arguments, struct sizes, counts and thresholds are looked at before the context and the device (XM_ERR_ARG = -2)"""
    L = xmamd.lib()
    a = np.zeros(16); k = np.zeros(4, dtype=np.uint8); v = np.zeros(4, dtype=np.int32)
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(8)     # never dereferenced: every call below is refused before the context is looked at

    def call(o, r, ctx=fake, keep=k, hyp=v):
        return L.xm_ctx_triangulate_tracks(ctx, ctypes.byref(o), P(a), P(a), P(a), None, None if keep is None else P(keep), P(k), P(v), P(k), P(v),
                                           None if hyp is None else P(hyp), ctypes.byref(r))

    def fresh():
        o = xmamd.TriOptions(); r = xmamd.TriResult()
        o.struct_size, r.struct_size = ctypes.sizeof(o), ctypes.sizeof(r)
        o.max_hypotheses, o.min_angle, o.create_max_angle_error, o.complete_max_reproj_error, o.min_views, o.refine_rounds = 64, 1.0, 2.0, 1e-2, 2, 2
        return o, r
    for change, word in ((lambda o, r: setattr(o, "struct_size", 32), "struct_size"), (lambda o, r: setattr(r, "struct_size", 0), "struct_size"),
                         (lambda o, r: setattr(o, "max_hypotheses", 0), "max_hypotheses"), (lambda o, r: setattr(o, "refine_rounds", 0), "refine_rounds"),
                         (lambda o, r: setattr(o, "min_views", -1), "min_views"), (lambda o, r: setattr(o, "min_angle", 0.0), "min_angle"),
                         (lambda o, r: setattr(o, "min_angle", 180.5), "min_angle"), (lambda o, r: setattr(o, "create_max_angle_error", float("nan")), "create_max_angle_error"),
                         (lambda o, r: setattr(o, "create_max_angle_error", -2.0), "create_max_angle_error"),
                         (lambda o, r: setattr(o, "complete_max_reproj_error", 0.0), "complete_max_reproj_error"),
                         (lambda o, r: setattr(o, "complete_max_reproj_error", float("inf")), "complete_max_reproj_error")):
        o, r = fresh(); change(o, r)
        assert call(o, r) == -2 and word in L.xm_last_error().decode()
    o, r = fresh()
    assert call(o, r, ctx=None) == -2 and "null" in L.xm_last_error().decode()
    assert call(o, r, keep=None) == -2 and "null" in L.xm_last_error().decode()
    assert call(o, r, hyp=None) == -2 and "null" in L.xm_last_error().decode()
