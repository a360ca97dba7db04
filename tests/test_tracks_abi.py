"""CPU tests of the track establishment's ABI: include/xm_amd.h and the binding agree (sizes, offsets, defaults, constants), the symbols are
exported, the refusals that need no device are made before one is looked for, and the host splitter (xm_tracks_split_host, the
XM_TRACKS_SPLIT policy) equals the contract's restatement."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

import xm_tracks_numpy as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_FIELDS = ("struct_size", "min_views", "max_views", "conflict", "max_tracks", "thres_inconsistency", "flags", "reserved")
RES_FIELDS = ("struct_size", "rounds", "ntracks", "features_touched", "matches", "components", "components_conflicted", "rows_conflicted", "tracks_short",
              "tracks_long", "tracks_conflict", "tracks_few_registered", "tracks_beyond_max", "images_small", "images_large", "images_workspace",
              "max_touched", "edges_split", "unions_refused", "seconds_index", "seconds_kernels", "seconds_split", "seconds_download")
CODES = ("XM_TRACKS_DROP", "XM_TRACKS_GLOMAP", "XM_TRACKS_SPLIT", "XM_TRACK_UNTOUCHED", "XM_TRACK_SHORT", "XM_TRACK_LONG", "XM_TRACK_CONFLICT",
         "XM_TRACK_FEW_REGISTERED", "XM_TRACK_BEYOND_MAX")
PROTO = (" int (*f)(int64_t, const int64_t *, const double *, const uint8_t *, int64_t, const int32_t *, const int32_t *, const int64_t *, const int32_t *,"
         " const int32_t *, const xm_tracks_options_t *, int32_t *, int32_t *, int32_t *, double *, int64_t *, int32_t *, xm_tracks_result_t *) = xm_build_tracks;"
         " (void)f; int (*g)(int64_t *) = xm_tracks_limits; (void)g;"
         " int (*h)(int64_t, const int64_t *, int64_t, const int32_t *, const int32_t *, int32_t *, int64_t *, int64_t *) = xm_tracks_split_host; (void)h;")


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){ xm_tracks_options_t o = XM_TRACKS_OPTIONS_INIT;\n'
           'printf("%zu %zu %d", sizeof(xm_tracks_options_t), sizeof(xm_tracks_result_t), XM_ABI_REVISION);\n'
           + "".join(f' printf(" %d", {c});\n' for c in CODES)
           + 'printf(" %u %d %d %d %lld %.17g %u %u", o.struct_size, o.min_views, o.max_views, o.conflict, (long long)o.max_tracks, o.thres_inconsistency,'
             ' o.flags, o.reserved);\n'
           + "".join(f' printf(" %zu", offsetof(xm_tracks_options_t, {f}));\n' for f in OPT_FIELDS)
           + "".join(f' printf(" %zu", offsetof(xm_tracks_result_t, {f}));\n' for f in RES_FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
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
    assert ctypes.sizeof(xmamd.TracksOptions) == so == 40 and ctypes.sizeof(xmamd.TracksResult) == sr == 176
    codes = list(map(int, v[3:3 + len(CODES)]))
    assert codes == [xmamd.TRACKS_DROP, xmamd.TRACKS_GLOMAP, xmamd.TRACKS_SPLIT, xmamd.TRACK_UNTOUCHED, xmamd.TRACK_SHORT, xmamd.TRACK_LONG,
                     xmamd.TRACK_CONFLICT, xmamd.TRACK_FEW_REGISTERED, xmamd.TRACK_BEYOND_MAX] == [0, 1, 2, -1, -2, -3, -4, -5, -6]
    assert codes[3:] == [tn.UNTOUCHED, tn.SHORT, tn.LONG, tn.CONFLICT, tn.FEW_REGISTERED, tn.BEYOND_MAX]
    # the defaults are the pipeline's constants (track_establishment.h, 5_test_ceres.py:127), in the header's initialiser and in the binding
    at = 3 + len(CODES)
    assert [float(x) for x in v[at:at + 8]] == [40, 3, 1000000, 2, 10000000, 10.0, 0, 0]
    o = xmamd.TracksOptions()
    assert [getattr(o, f) for f in OPT_FIELDS] == [40, 3, 1000000, 2, 10000000, 10.0, 0, 0]
    assert tn.DEFAULTS == dict(min_views=3, max_views=1000000, max_tracks=10000000, thres_inconsistency=10.0)
    offs = [getattr(xmamd.TracksOptions, f).offset for f in OPT_FIELDS] + [getattr(xmamd.TracksResult, f).offset for f in RES_FIELDS]
    assert offs == list(map(int, v[at + 8:]))
    assert tuple(f for f, _ in xmamd.TracksResult._fields_) == RES_FIELDS


def test_exports_and_wrapper(xmamd):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_build_tracks", "xm_tracks_limits", "xm_tracks_split_host"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    sig = inspect.signature(xmamd.build_tracks).parameters
    assert list(sig)[:6] == ["foff_or_counts", "xy", "pi", "pj", "matches", "registered"] and sig["registered"].default is None
    assert {k: sig[k].default for k in list(sig)[6:]} == dict(tn.DEFAULTS, conflict="split")
    lim = xmamd.tracks_limits()                            # needs no device
    assert lim["threads"] == 256 and lim["lds_rows"] & (lim["lds_rows"] - 1) == 0 and lim["workspace_groups"] >= 1
    assert 2 <= lim["small_rows"] < lim["lds_rows"]
    xy = np.zeros((4, 2)); e = np.zeros(0, dtype=np.int32)
    for args, kw, word in ((([2, 2], xy[:, :1], e, e, []), {}, "features x 2"), (([2, 3], xy, e, e, []), {}, "neither the offsets"),
                           (([2, 2], xy, [0], [1, 0], []), {}, "one entry per pair"), (([2, 2], xy, [0], [1], []), {}, "npairs \\+ 1 offsets"),
                           (([2, 2], xy, [0], [1], ([0, 2], [0], [0])), {}, "npairs \\+ 1 offsets"),
                           (([2, 2], xy, e, e, []), dict(registered=[1]), "one entry per image"), (([2, 2], xy, e, e, []), dict(conflict="merge"), "one of")):
        with pytest.raises(xmamd.XmError, match=word):     # no device: the arguments are checked before anything else is looked at
            xmamd.build_tracks(*args, **kw)
    # counts and offsets are told apart; a list of (k, 2) arrays and (moff, f1, f2) are the same matches; no match needs no device
    t = xmamd.build_tracks([2, 2], xy, e, e, [])
    u = xmamd.build_tracks([0, 2, 4], xy, e, e, (np.zeros(1, dtype=np.int64), e, e))
    assert t.cam.size == u.cam.size == 0 and t.m == 0 and t.label.tolist() == u.label.tolist() == [-1] * 4 and t.foff.tolist() == u.foff.tolist() == [0, 2, 4]
    table = xmamd.TrackTable(np.array([1, 0], dtype=np.int32), np.array([1, 0], dtype=np.int32), None, None, 0, None, {}, np.array([0, 2, 4]))
    a, b = table.carry(np.arange(4) * 10, np.arange(8).reshape(4, 2))
    assert a.tolist() == [30, 0] and b.tolist() == [[6, 7], [0, 1]] and table.feature.tolist() == [3, 0]
    with pytest.raises(xmamd.XmError, match="another length"):
        table.carry(np.arange(5))


def test_library_refusals_need_no_device(xmamd):
    """struct sizes, options, sizes, offsets, pairs and null arrays are looked at before the device (XM_ERR_ARG = -2), and nothing is written"""
    L = xmamd.lib()
    foff = np.array([0, 2, 4], dtype=np.int64); xy = np.zeros((4, 2)); pi = np.array([0], dtype=np.int32); pj = np.array([1], dtype=np.int32)
    moff = np.array([0, 1], dtype=np.int64); f = np.zeros(1, dtype=np.int32); oi = np.full(4, 55, dtype=np.int32); oxy = np.full((4, 2), 5.5)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(o, r, n=2, npairs=1, foff_=foff, xy_=xy, pi_=pi, pj_=pj, moff_=moff, f1_=f, out_=oi, nout=True):
        no = ctypes.c_int64(-7)
        rc = L.xm_build_tracks(n, P(foff_), P(xy_), None, npairs, P(pi_), P(pj_), P(moff_), P(f1_), P(f), None if o is None else ctypes.byref(o), P(out_),
                               P(oi), P(oi), P(oxy), ctypes.byref(no) if nout else None, P(oi), None if r is None else ctypes.byref(r))
        assert no.value == -7 and (oi == 55).all() and (oxy == 5.5).all()
        return rc

    def fresh():
        r = xmamd.TracksResult(); r.struct_size = ctypes.sizeof(r)
        return xmamd.TracksOptions(), r
    for change, word in ((lambda o, r: setattr(o, "struct_size", 32), "struct_size"), (lambda o, r: setattr(r, "struct_size", 0), "struct_size"),
                         (lambda o, r: setattr(o, "min_views", 0), "min_views below 1"), (lambda o, r: setattr(o, "max_views", 2), "max_views below min_views"),
                         (lambda o, r: setattr(o, "max_tracks", -1), "negative max_tracks"),
                         (lambda o, r: setattr(o, "thres_inconsistency", -0.5), "thres_inconsistency"),
                         (lambda o, r: setattr(o, "thres_inconsistency", float("inf")), "thres_inconsistency"),
                         (lambda o, r: setattr(o, "thres_inconsistency", float("nan")), "thres_inconsistency"),
                         (lambda o, r: setattr(o, "conflict", 3), "unknown conflict policy"), (lambda o, r: setattr(o, "conflict", -1), "unknown conflict policy"),
                         (lambda o, r: setattr(o, "flags", 1), "unknown flag")):
        o, r = fresh(); change(o, r)
        assert call(o, r) == -2 and word in L.xm_last_error().decode()
    o, r = fresh()
    assert call(None, r) == -2 and call(o, None) == -2 and call(o, r, nout=False) == -2 and "null" in L.xm_last_error().decode()
    assert call(o, r, n=-1) == -2 and call(o, r, npairs=-1) == -2 and "negative size" in L.xm_last_error().decode()
    assert call(o, r, n=2 ** 31) == -2 and "2^31" in L.xm_last_error().decode()
    for kw in (dict(foff_=None), dict(xy_=None), dict(pi_=None), dict(pj_=None), dict(moff_=None), dict(f1_=None), dict(out_=None)):
        assert call(o, r, **kw) == -2 and "null" in L.xm_last_error().decode()
    for kw, word in ((dict(foff_=np.array([0, 3, 2], dtype=np.int64)), "foff decreases"), (dict(foff_=np.array([1, 2, 4], dtype=np.int64)), "foff does not start"),
                     (dict(foff_=np.array([0, 2, 2 ** 31], dtype=np.int64)), "features must stay below 2^31"),
                     (dict(moff_=np.array([1, 1], dtype=np.int64)), "moff does not start"), (dict(moff_=np.array([0, -1], dtype=np.int64)), "moff decreases"),
                     (dict(moff_=np.array([0, 2 ** 31], dtype=np.int64)), "matches must stay below 2^31"),
                     (dict(pj_=np.array([0], dtype=np.int32)), "names one image twice"), (dict(pi_=np.array([2], dtype=np.int32)), "image index out of range"),
                     (dict(pj_=np.array([-1], dtype=np.int32)), "image index out of range")):
        assert call(o, r, **kw) == -2 and word in L.xm_last_error().decode(), word
    assert L.xm_tracks_limits(None) == -2
    lab = np.zeros(4, dtype=np.int32)
    assert L.xm_tracks_split_host(2, P(foff), 1, P(np.array([4], dtype=np.int32)), P(f), P(lab), None, None) == -2 and "out of range" in L.xm_last_error().decode()
    assert L.xm_tracks_split_host(2, P(foff), 1, None, P(f), P(lab), None, None) == -2


def _split_both(xmamd, c):
    eu, ev = tn._global_edges(c)
    F = int(c["foff"][-1])
    label, distinct, refused = xmamd.split_host(c["foff"], F, eu, ev)
    new, d2, r2 = tn.split_numpy(c["foff"], eu, ev)
    want = np.full(F, -1, dtype=np.int32)
    for g, v in new.items():
        want[g] = v
    assert np.array_equal(label, want) and (distinct, refused) == (d2, r2)
    # any order of the edges, either orientation: the same sets
    q = np.random.default_rng(4).permutation(eu.size)
    turned, d3, r3 = xmamd.split_host(c["foff"], F, ev[q], eu[q])
    assert np.array_equal(turned, label) and (d3, r3) == (distinct, refused)
    return label, distinct, refused


def test_host_splitter_equals_the_contract(xmamd):
    P = tn.gpu_cases(dict(small_rows=256, lds_rows=4096))
    # a refused union: 0.1 stays alone
    label, distinct, refused = _split_both(xmamd, P["conflict_near"])
    assert label.tolist() == [0, 1, 0, 0, -1] and (distinct, refused) == (3, 1)
    # a chain of three conflicts
    label, distinct, refused = _split_both(xmamd, P["conflict_chain"])
    assert label.tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 1] and (distinct, refused) == (10, 3)
    # a duplicate edge, in both orientations
    c = P["conflict_chain"]
    eu, ev = tn._global_edges(c)
    again, d, r = xmamd.split_host(c["foff"], 9, np.concatenate([eu, ev[:4], eu[-1:]]), np.concatenate([ev, eu[:4], ev[-1:]]))
    assert np.array_equal(again, label) and (d, r) == (10, 3)
    # the two larger cases, every component (conflict-free ones included: nothing is refused inside them)
    _split_both(xmamd, P["sizes"][0] if isinstance(P["sizes"], tuple) else P["sizes"])
    c, _ = tn.load_case()
    label, distinct, refused = _split_both(xmamd, c)
    assert refused > 0 and np.sum(label >= 0) == 64427
    none, d, r = xmamd.split_host([3], 3, [], [])
    assert none.tolist() == [-1, -1, -1] and (d, r) == (0, 0)
