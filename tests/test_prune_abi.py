"""CPU tests of the ABI of xm_prune_weakly_connected / xm_ctx_prune_weakly_connected / xm_prune_limits (include/xm_amd.h): prototypes and
structs compile from the header and agree with the binding, the symbols are exported, the ABI revision stays where it was (added exports),
and the library and the wrappers refuse bad arguments before any device is looked at."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

import xm_prune_numpy as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "min_covisibility", "min_num_images", "min_num_observations", "min_threshold")
PAIRS_FIELDS = ("capacity", "i", "j", "count")
RES_FIELDS = ("struct_size", "rounds", "pairs_covisible", "n_edges", "median", "mad", "threshold", "component_images", "strong_clusters", "weak_edges",
              "n_clusters", "images_clustered", "seconds_kernels", "seconds_download")
PROTO = (" int (*f)(int64_t, int64_t, int64_t, const int32_t *, const int32_t *, const double *, const xm_prune_options_t *, int32_t *, int32_t *,"
         " const xm_prune_pairs_t *, xm_prune_result_t *) = xm_prune_weakly_connected; (void)f;"
         " int (*g)(xm_ctx_t *, const xm_prune_options_t *, int32_t *, int32_t *, const xm_prune_pairs_t *, xm_prune_result_t *)"
         " = xm_ctx_prune_weakly_connected; (void)g; int (*h)(int64_t *) = xm_prune_limits; (void)h;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){xm_prune_options_t o = XM_PRUNE_OPTIONS_INIT;\n'
           'printf("%zu %zu %zu %d", sizeof(xm_prune_options_t), sizeof(xm_prune_pairs_t), sizeof(xm_prune_result_t), XM_ABI_REVISION);\n'
           'printf(" %u %d %d %d %d", o.struct_size, o.min_covisibility, o.min_num_images, o.min_num_observations, (int)o.min_threshold);\n'
           + "".join(f' printf(" %zu", offsetof(xm_prune_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_prune_pairs_t, {f}));\n' for f in PAIRS_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_prune_result_t, {f}));\n' for f in RES_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    so, sp, sr, rev, *rest = _c_values()
    init, offs = rest[:5], rest[5:]
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # added exports: the revision stays
    assert ctypes.sizeof(xmamd.PruneOptions) == so == 24 and ctypes.sizeof(xmamd.PrunePairs) == sp == 32 and ctypes.sizeof(xmamd.PruneResult) == sr == 104
    assert [getattr(xmamd.PruneOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.PrunePairs, f).offset for f in PAIRS_FIELDS] + \
           [getattr(xmamd.PruneResult, f).offset for f in RES_FIELDS] == offs
    d = pr.DEFAULTS                                                               # GLOMAP's defaults: header, binding and contract agree
    assert init == [so, d["min_covisibility"], d["min_num_images"], d["min_num_observations"], int(d["min_threshold"])] == [24, 5, 2, 0, 20]
    sig = inspect.signature(xmamd.prune_weakly_connected).parameters
    assert {k: sig[k].default for k in d} == d
    sig = inspect.signature(xmamd.Context.prune_weakly_connected).parameters
    assert {k: sig[k].default for k in d} == d and list(sig)[-1] == "pairs"
    sig = inspect.signature(xmamd.Context.refine_filtered).parameters
    assert sig["prune"].default is False and sig["restore_weights"].default is False


def test_all_are_exported_and_the_limits(xmamd):
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_prune_weakly_connected", "xm_ctx_prune_weakly_connected", "xm_prune_limits"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    lim = xmamd.prune_limits()                                                    # host-only
    assert set(lim) == {"tile", "threads", "group_max", "group", "select_bits"} and lim["threads"] == 256
    assert lim["tile"] % lim["threads"] == 0 and lim["threads"] % lim["group"] == 0 and 256 <= lim["tile"] <= 4096
    assert xmamd.lib().xm_prune_limits(None) == -2


def test_plan(xmamd):
    cam = np.array([0, 1, 2, 2, 3], dtype=np.int32)
    plan = xmamd.PrunePlan(np.array([0, 1, -1, 0], dtype=np.int32), np.zeros(4, np.int32), {}, None, cam)
    assert plan.weights([5.0, 4.0, 3.0, 2.0, 1.0]).tolist() == [5.0, 0.0, 0.0, 0.0, 1.0]
    assert plan.weights(np.ones(5), cluster=1).tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]
    assert [a.tolist() for a in plan.apply(cam, np.arange(10).reshape(5, 2))] == [[0, 3], [[0, 1], [8, 9]]]
    assert [a.tolist() for a in plan.apply(cam, cluster=-1)] == [[2, 2]]
    for bad in (lambda: plan.weights(np.ones(4)), lambda: plan.apply(np.ones(3)), lambda: xmamd.PrunePlan(plan.cluster_id, None, {}).weights(np.ones(5))):
        with pytest.raises(xmamd.XmError):
            bad()


def test_wrapper_arguments(xmamd):
    cam = np.zeros(3, dtype=np.int32)
    for kw, word in ((dict(min_covisibility=-1), "negative"), (dict(min_num_images=-1), "negative"), (dict(min_num_observations=-2), "negative"),
                     (dict(min_threshold=float("nan")), "finite"), (dict(min_threshold=float("inf")), "finite")):
        with pytest.raises(xmamd.XmError, match=word):        # no device: the arguments are checked before anything else is looked at
            xmamd.prune_weakly_connected(cam, cam, **kw)
        ctx = xmamd.Context.__new__(xmamd.Context)
        ctx.n, ctx.h = 1, None
        with pytest.raises(xmamd.XmError, match=word):
            ctx.prune_weakly_connected(**kw)
    with pytest.raises(xmamd.XmError, match="one entry per observation"):
        xmamd.prune_weakly_connected(cam, cam[:2])
    with pytest.raises(xmamd.XmError, match="one entry per observation"):
        xmamd.prune_weakly_connected(cam, cam, w=np.ones(2))


def test_library_refusals_need_no_device(xmamd):
    """null arguments, struct sizes, options, the pairs struct and the sizes are looked at before the context and the device (XM_ERR_ARG = -2)"""
    L = xmamd.lib()
    v = np.zeros(4, dtype=np.int32)
    P = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(8)     # never dereferenced: every call below is refused before the context is looked at

    def fresh():
        o = xmamd.PruneOptions(); r = xmamd.PruneResult()
        o.struct_size, r.struct_size = ctypes.sizeof(o), ctypes.sizeof(r)
        o.min_covisibility, o.min_num_images, o.min_num_observations, o.min_threshold = 5, 2, 0, 20.0
        return o, r

    def ctx_call(o, r, ctx=fake, cid=v, pairs=None):
        return L.xm_ctx_prune_weakly_connected(ctx, ctypes.byref(o), P(cid), P(v), pairs, ctypes.byref(r))

    def host_call(o, r, n=2, m=2, nobs=4, cam=v, cid=v, pairs=None):
        return L.xm_prune_weakly_connected(n, m, nobs, P(cam), P(v), None, ctypes.byref(o), P(cid), P(v), pairs, ctypes.byref(r))
    changes = ((lambda o, r: setattr(o, "struct_size", 16), "struct_size"), (lambda o, r: setattr(r, "struct_size", 0), "struct_size"),
               (lambda o, r: setattr(o, "min_covisibility", -1), "negative"), (lambda o, r: setattr(o, "min_num_images", -1), "negative"),
               (lambda o, r: setattr(o, "min_num_observations", -1), "negative"), (lambda o, r: setattr(o, "min_threshold", float("nan")), "finite"),
               (lambda o, r: setattr(o, "min_threshold", float("-inf")), "finite"))
    for call in (ctx_call, host_call):
        for change, word in changes:
            o, r = fresh(); change(o, r)
            assert call(o, r) == -2 and word in L.xm_last_error().decode()
        o, r = fresh()
        assert call(o, r, cid=None) == -2 and "null" in L.xm_last_error().decode()
        bad = xmamd.PrunePairs(-1, None, None, None)
        assert call(o, r, pairs=ctypes.byref(bad)) == -2 and "capacity" in L.xm_last_error().decode()
        bad = xmamd.PrunePairs(4, P(v), None, P(v))
        assert call(o, r, pairs=ctypes.byref(bad)) == -2 and "null array" in L.xm_last_error().decode()
    o, r = fresh()
    assert ctx_call(o, r, ctx=None) == -2 and "null" in L.xm_last_error().decode()
    assert host_call(o, r, n=-1) == -2 and "negative size" in L.xm_last_error().decode()
    assert host_call(o, r, n=1 << 31) == -2 and "2^31" in L.xm_last_error().decode()
    assert host_call(o, r, cam=None) == -2 and "null observation" in L.xm_last_error().decode()
