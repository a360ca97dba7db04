"""CPU tests of the ABI of xm_clean_observations / xm_ctx_clean_observations (include/xm_amd.h): prototypes and structs compile from the
header and agree with the binding, both symbols are exported, the ABI revision stays where it was (added exports), and the wrappers refuse
bad arguments before any device is looked at."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "min_cam_obs", "min_lm_obs", "flags")
RES_FIELDS = ("struct_size", "rounds", "nobs_live", "n_new", "m_new", "nobs_new", "components", "cams_weak", "lms_weak", "cams_emptied",
              "cams_off_component", "lms_off_component", "first_camera", "reserved")
PROTO = (" int (*f)(int64_t, int64_t, int64_t, const int32_t *, const int32_t *, const double *, const xm_clean_options_t *, uint8_t *, int32_t *,"
         " int32_t *, xm_clean_result_t *) = xm_clean_observations; (void)f;"
         " int (*g)(xm_ctx_t *, const xm_clean_options_t *, uint8_t *, int32_t *, int32_t *, xm_clean_result_t *) = xm_ctx_clean_observations; (void)g;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %d %u", sizeof(xm_clean_options_t), sizeof(xm_clean_result_t), XM_ABI_REVISION, XM_CLEAN_NO_SWAP);\n'
           + "".join(f' printf(" %zu", offsetof(xm_clean_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_clean_result_t, {f}));\n' for f in RES_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    so, sr, rev, noswap, *offs = _c_values()
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # added exports: the revision stays
    assert noswap == xmamd.CLEAN_NO_SWAP == 1
    assert ctypes.sizeof(xmamd.CleanOptions) == so == 16 and ctypes.sizeof(xmamd.CleanResult) == sr == 96
    assert [getattr(xmamd.CleanOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.CleanResult, f).offset for f in RES_FIELDS] == offs


def test_both_are_exported(xmamd):
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_clean_observations", "xm_ctx_clean_observations"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names


def test_wrapper_arguments(xmamd):
    assert list(inspect.signature(xmamd.clean_observations).parameters) == ["cam", "lm", "w", "n", "m", "min_cam_obs", "min_lm_obs", "swap_first"]
    assert list(inspect.signature(xmamd.Context.clean_observations).parameters) == ["self", "min_cam_obs", "min_lm_obs", "swap_first"]
    d = inspect.signature(xmamd.clean_observations).parameters
    assert (d["min_cam_obs"].default, d["min_lm_obs"].default, d["swap_first"].default) == (10, 1, True)
    cam = np.zeros(4, dtype=np.int32)
    for args, kw, word in (((cam, cam[:3]), {}, "one entry per observation"), ((cam, cam, np.ones(3)), {}, "w must have"),
                           ((cam, cam), dict(min_cam_obs=-1), "negative"), ((cam, cam), dict(min_lm_obs=-2), "negative")):
        with pytest.raises(xmamd.XmError, match=word):    # no device: the arguments are checked before anything else is looked at
            xmamd.clean_observations(*args, **kw)
    ctx = xmamd.Context.__new__(xmamd.Context)
    ctx.n, ctx.n_landmarks, ctx.ne, ctx.h = 1, 1, 1, None
    with pytest.raises(xmamd.XmError, match="negative"):
        ctx.clean_observations(min_cam_obs=-1)
    ctx.h = None   # nothing to destroy


def test_library_refusals_need_no_device(xmamd):
    """struct sizes, thresholds, flags and null outputs are looked at before the device (XM_ERR_ARG = -2)"""
    L = xmamd.lib()
    cam = np.zeros(2, dtype=np.int32); keep = np.zeros(2, dtype=np.uint8); ci = np.zeros(1, dtype=np.int32); li = np.zeros(1, dtype=np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(opt, res, keep_=keep, n=1, m=1):
        return L.xm_clean_observations(n, m, 2, P(cam), P(cam), None, ctypes.byref(opt), None if keep_ is None else P(keep_), P(ci), P(li), ctypes.byref(res))

    def fresh():
        o = xmamd.CleanOptions(); r = xmamd.CleanResult()
        o.struct_size, r.struct_size, o.min_cam_obs, o.min_lm_obs = ctypes.sizeof(o), ctypes.sizeof(r), 10, 1
        return o, r
    for change, word in ((lambda o, r: setattr(o, "struct_size", 12), "struct_size"), (lambda o, r: setattr(r, "struct_size", 0), "struct_size"),
                         (lambda o, r: setattr(o, "min_cam_obs", -1), "negative"), (lambda o, r: setattr(o, "flags", 2), "unknown flag")):
        o, r = fresh(); change(o, r)
        assert call(o, r) == -2 and word in L.xm_last_error().decode()
    o, r = fresh()
    assert call(o, r, keep_=None) == -2 and "null" in L.xm_last_error().decode()
    assert call(o, r, n=2 ** 30, m=2 ** 30) == -2 and "2^31" in L.xm_last_error().decode()
    assert call(o, r, n=-1) == -2
    assert L.xm_ctx_clean_observations(None, ctypes.byref(o), P(keep), P(ci), P(li), ctypes.byref(r)) == -2
