"""CPU tests of the ABI of xm_ctx_filter_tracks / xm_track_filter_limits (include/xm_amd.h): prototypes, structs and constants compile
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "flags", "max_reprojection_error", "max_angle_error", "min_triangulation_angle", "min_views", "reserved")
RES_FIELDS = ("struct_size", "reserved") + tf.COUNTS + ("cos_angle", "cos_triangulation", "seconds_kernels", "seconds_download")
CONSTANTS = ("XM_TF_REPROJECTION", "XM_TF_ANGLE", "XM_TF_TRIANGULATION", "XM_TF_REASON_DEPTH", "XM_TF_REASON_REPROJECTION", "XM_TF_REASON_ANGLE",
             "XM_TF_REASON_TRIANGULATION", "XM_TF_REASON_MIN_VIEWS", "XM_TF_LM_KEPT", "XM_TF_LM_UNUSED", "XM_TF_LM_TRIANGULATION", "XM_TF_LM_MIN_VIEWS")
PROTO = (" int (*f)(xm_ctx_t *, const xm_tf_options_t *, const double *, const double *, const double *, uint8_t *, uint8_t *, int32_t *, uint8_t *,"
         " xm_tf_result_t *) = xm_ctx_filter_tracks; (void)f; int (*g)(int64_t *) = xm_track_filter_limits; (void)g;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %d", sizeof(xm_tf_options_t), sizeof(xm_tf_result_t), XM_ABI_REVISION);\n'
           + "".join(f' printf(" %d", (int)({c}));\n' for c in CONSTANTS)
           + "".join(f' printf(" %zu", offsetof(xm_tf_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_tf_result_t, {f}));\n' for f in RES_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    so, sr, rev, *rest = _c_values()
    consts, offs = rest[:len(CONSTANTS)], rest[len(CONSTANTS):]
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # added exports: the revision stays
    assert ctypes.sizeof(xmamd.TfOptions) == so == 40 and ctypes.sizeof(xmamd.TfResult) == sr == 144
    assert [getattr(xmamd.TfOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.TfResult, f).offset for f in RES_FIELDS] == offs
    assert consts == [getattr(xmamd, c[3:]) for c in CONSTANTS]
    assert consts == [1, 2, 4, tf.REASON_DEPTH, tf.REASON_REPROJECTION, tf.REASON_ANGLE, tf.REASON_TRIANGULATION, tf.REASON_MIN_VIEWS,
                      tf.LM_KEPT, tf.LM_UNUSED, tf.LM_TRIANGULATION, tf.LM_MIN_VIEWS]
    assert xmamd.TF_COUNTS == tf.COUNTS


def test_both_are_exported_and_the_limits_are_those_of_the_scenes(xmamd):
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_ctx_filter_tracks", "xm_track_filter_limits"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    lim = xmamd.track_filter_limits()                                             # host-only
    assert lim == dict(light_max=tf.LIGHT_MAX, tile=tf.TILE, threads=256)
    assert xmamd.lib().xm_track_filter_limits(None) == -2


def test_wrapper_arguments(xmamd):
    sig = inspect.signature(xmamd.Context.filter_tracks).parameters
    assert list(sig) == ["self", "rot", "t", "P", "reprojection", "angle", "triangulation", "min_views"]
    assert [sig[k].default for k in ("reprojection", "angle", "triangulation", "min_views")] == [1e-2, None, None, 0]
    sig = inspect.signature(xmamd.Context.refine_filtered).parameters
    assert list(sig)[:8] == ["self", "rot", "t", "P", "rounds", "reprojection", "triangulation", "min_views"] and "restore_weights" in sig
    assert [sig[k].default for k in ("rounds", "reprojection", "triangulation", "min_views", "restore_weights")] == [3, 1e-2, 1.0, 0, False]
    ctx = xmamd.Context.__new__(xmamd.Context)
    ctx.n, ctx.n_landmarks, ctx.ne, ctx.h = 1, 1, 1, None
    g = (np.eye(3), np.zeros((3, 1)), np.zeros((3, 1)))
    for kw, word in ((dict(reprojection=0.0), "reprojection"), (dict(angle=-1.0), "angle"), (dict(triangulation=float("nan")), "triangulation"),
                     (dict(min_views=-1), "min_views")):
        with pytest.raises(xmamd.XmError, match=word):    # no device: the arguments are checked before anything else is looked at
            ctx.filter_tracks(*g, **kw)
    ctx.h = None   # nothing to destroy
    plan = xmamd.TrackFilterPlan(np.array([True, False, False]), np.array([0, 2, 0], dtype=np.uint8), np.zeros(1, np.int32), np.zeros(1, np.uint8), {})
    assert plan.weights([3.0, 2.0, 0.0]).tolist() == [3.0, 0.0, 0.0] and plan.dropped.tolist() == [False, True, False]
    assert [a.tolist() for a in plan.apply(np.arange(3), np.arange(6).reshape(3, 2))] == [[0], [[0, 1]]]
    for bad in (lambda: plan.weights(np.ones(2)), lambda: plan.apply(np.ones(2))):
        with pytest.raises(xmamd.XmError):
            bad()


def test_library_refusals_need_no_device(xmamd):
    """null arguments, struct sizes, flags and thresholds are looked at before the context and the device (XM_ERR_ARG = -2)"""
    L = xmamd.lib()
    a = np.zeros(16); k = np.zeros(4, dtype=np.uint8); v = np.zeros(4, dtype=np.int32)
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(8)     # never dereferenced: every call below is refused before the context is looked at

    def call(o, r, ctx=fake, keep=k):
        return L.xm_ctx_filter_tracks(ctx, ctypes.byref(o), P(a), P(a), P(a), None if keep is None else P(keep), P(k), P(v), P(k), ctypes.byref(r))

    def fresh():
        o = xmamd.TfOptions(); r = xmamd.TfResult()
        o.struct_size, r.struct_size, o.flags = ctypes.sizeof(o), ctypes.sizeof(r), 7
        o.max_reprojection_error, o.max_angle_error, o.min_triangulation_angle = 1e-2, 1.0, 1.0
        return o, r
    for change, word in ((lambda o, r: setattr(o, "struct_size", 32), "struct_size"), (lambda o, r: setattr(r, "struct_size", 0), "struct_size"),
                         (lambda o, r: setattr(o, "flags", 8), "unknown flag"), (lambda o, r: setattr(o, "min_views", -1), "min_views"),
                         (lambda o, r: setattr(o, "max_reprojection_error", 0.0), "max_reprojection_error"),
                         (lambda o, r: setattr(o, "max_reprojection_error", float("inf")), "max_reprojection_error"),
                         (lambda o, r: setattr(o, "max_angle_error", -1.0), "max_angle_error"),
                         (lambda o, r: setattr(o, "min_triangulation_angle", float("nan")), "min_triangulation_angle"),
                         (lambda o, r: setattr(o, "min_triangulation_angle", 181.0), "min_triangulation_angle")):
        o, r = fresh(); change(o, r)
        assert call(o, r) == -2 and word in L.xm_last_error().decode()
    o, r = fresh()
    assert call(o, r, ctx=None) == -2 and "null" in L.xm_last_error().decode()
    assert call(o, r, keep=None) == -2 and "null" in L.xm_last_error().decode()
