"""CPU tests of the device split's ABI (XM_TRACKS_SPLIT_DEVICE, xm_tracks_split_device / _limits / _stats of include/xm_amd.h): header and
binding agree, the struct sizes and the revision stay, the symbols are exported, and every refusal that needs no device is made before
one is looked for, with the outputs untouched."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("xm_tracks_split_device", "xm_tracks_split_limits", "xm_tracks_split_stats")
PROTO = (" int (*f)(int64_t, const int64_t *, int64_t, const int32_t *, const int32_t *, int32_t *, int64_t *, int64_t *) = xm_tracks_split_device; (void)f;"
         " int (*g)(int64_t *) = xm_tracks_split_limits; (void)g; int (*h)(int64_t *) = xm_tracks_split_stats; (void)h;")
P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_header_and_binding_agree(xmamd):
    src = ('#include "xm_amd.h"\n#include <stdio.h>\nint main(){ xm_tracks_options_t o = XM_TRACKS_OPTIONS_INIT;\n'
           'printf("%zu %zu %d %u %u %d\\n", sizeof(xm_tracks_options_t), sizeof(xm_tracks_result_t), XM_ABI_REVISION, XM_TRACKS_SPLIT_DEVICE, o.flags,'
           ' XM_TRACKS_SPLIT);' + PROTO + ' return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        so, sr, rev, flag, default, split = map(int, subprocess.check_output([os.path.join(d, "t")]).split())
    assert ctypes.sizeof(xmamd.TracksOptions) == so == 40 and ctypes.sizeof(xmamd.TracksResult) == sr == 176
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev
    assert flag == xmamd.TRACKS_SPLIT_DEVICE == 2 and default == 0 and xmamd.TracksOptions().flags == 0
    assert xmamd.TRACKS_POLICIES["split_device"] == xmamd.TRACKS_SPLIT == split


def test_exports(xmamd):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in SYMBOLS:
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names
    for f in ("split_device", "tracks_split_limits", "tracks_split_stats"):
        assert callable(getattr(xmamd, f))


def test_limits_and_stats_need_no_device(xmamd):
    L = xmamd.lib()
    assert L.xm_tracks_split_limits(None) == -2 and "null" in L.xm_last_error().decode()
    assert L.xm_tracks_split_stats(None) == -2 and "null" in L.xm_last_error().decode()
    lim = xmamd.tracks_split_limits()
    assert set(lim) == {"wave_endpoints", "wave_edges", "group_edges", "threads"}
    assert lim["threads"] == 256 and lim["group_edges"] >= 2048 and lim["group_edges"] & (lim["group_edges"] - 1) == 0
    assert lim["wave_edges"] <= lim["group_edges"] and lim["wave_endpoints"] >= 0
    if lim["wave_edges"]:                                          # the wavefront form is built
        assert 2 <= lim["wave_endpoints"] <= lim["wave_edges"] + 1
    st = xmamd.tracks_split_stats()
    assert tuple(st) == ("wave", "group", "host", "edges_device", "edges_host", "distinct", "refused")
    # a call that launches nothing leaves them at 0, all eight
    xmamd.build_tracks([2, 2], np.zeros((4, 2)), [], [], [], conflict="split_device")
    raw = np.full(8, 7, dtype=np.int64)
    assert L.xm_tracks_split_stats(P(raw)) == 0 and raw.tolist() == [0] * 8


def test_flag_refusals_need_no_device(xmamd):
    """the flag goes with XM_TRACKS_SPLIT only, any other bit is unknown: XM_ERR_ARG (-2) before a device is looked for, nothing written"""
    L = xmamd.lib()
    foff = np.array([0, 2, 4], dtype=np.int64); xy = np.zeros((4, 2)); pi = np.array([0], dtype=np.int32); pj = np.array([1], dtype=np.int32)
    moff = np.array([0, 1], dtype=np.int64); f = np.zeros(1, dtype=np.int32); oi = np.full(4, 55, dtype=np.int32); oxy = np.full((4, 2), 5.5)
    for conflict, flags, word in ((xmamd.TRACKS_DROP, 2, "XM_TRACKS_SPLIT only"), (xmamd.TRACKS_GLOMAP, 2, "XM_TRACKS_SPLIT only"),
                                  (xmamd.TRACKS_SPLIT, 3, "unknown flag"), (xmamd.TRACKS_SPLIT, 4, "unknown flag"), (xmamd.TRACKS_SPLIT, 1, "unknown flag"),
                                  (xmamd.TRACKS_DROP, 3, "unknown flag"), (3, 2, "unknown conflict policy")):
        o = xmamd.TracksOptions(conflict=conflict, flags=flags)
        r = xmamd.TracksResult(); r.struct_size = ctypes.sizeof(r); r.ntracks = -9
        no = ctypes.c_int64(-7)
        rc = L.xm_build_tracks(2, P(foff), P(xy), None, 1, P(pi), P(pj), P(moff), P(f), P(f), ctypes.byref(o), P(oi), P(oi), P(oi), P(oxy), ctypes.byref(no),
                               P(oi), ctypes.byref(r))
        assert rc == -2 and word in L.xm_last_error().decode(), (conflict, flags)
        assert no.value == -7 and (oi == 55).all() and (oxy == 5.5).all() and r.ntracks == -9
    with pytest.raises(xmamd.XmError, match="one of.*split_device"):
        xmamd.build_tracks([2, 2], xy, [], [], [], conflict="merge")


def test_split_device_refusals_need_no_device(xmamd):
    L = xmamd.lib()
    foff = np.array([0, 2, 4], dtype=np.int64); one = np.zeros(1, dtype=np.int32)
    d = ctypes.c_int64(-3); r = ctypes.c_int64(-4)

    def call(eu, ev, lab, n=2, ne=1, foff_=foff):
        rc = L.xm_tracks_split_device(n, P(foff_), ne, P(eu), P(ev), P(lab), ctypes.byref(d), ctypes.byref(r))
        assert (d.value, r.value) == (-3, -4) and (lab is None or (lab == 9).all())
        return rc
    lab = np.full(4, 9, dtype=np.int32)
    for eu, ev in ((np.array([4], dtype=np.int32), one), (one, np.array([4], dtype=np.int32)), (np.array([-1], dtype=np.int32), one),
                   (one, np.array([2 ** 31 - 1], dtype=np.int32))):
        assert call(eu, ev, lab) == -2 and "out of range" in L.xm_last_error().decode()
    assert call(None, one, lab) == -2 and call(one, None, lab) == -2 and "null" in L.xm_last_error().decode()
    assert call(one, one, None) == -2 and "null" in L.xm_last_error().decode()
    assert call(one, one, lab, foff_=None) == -2 and call(one, one, lab, n=-1) == -2 and call(one, one, lab, ne=-1) == -2
    assert call(one, one, lab, foff_=np.array([0, 3, 2], dtype=np.int64)) == -2 and "foff decreases" in L.xm_last_error().decode()
    with pytest.raises(xmamd.XmError, match="one entry per edge"):
        xmamd.split_device([2, 2], 4, [0], [1, 2])
    # no edge: nothing to launch, no device
    none, distinct, refused = xmamd.split_device([3], 3, [], [])
    assert none.tolist() == [-1, -1, -1] and (distinct, refused) == (0, 0)


def test_no_match_needs_no_device(xmamd):
    xy = np.zeros((4, 2)); e = np.zeros(0, dtype=np.int32)
    t = xmamd.build_tracks([2, 2], xy, e, e, [], conflict="split_device")
    u = xmamd.build_tracks([0, 2, 4], xy, e, e, (np.zeros(1, dtype=np.int64), e, e), conflict="split_device")
    assert t.cam.size == u.cam.size == 0 and t.m == u.m == 0 and t.label.tolist() == u.label.tolist() == [-1] * 4
    assert t.foff.tolist() == u.foff.tolist() == [0, 2, 4] and t.info["seconds_split"] == 0.0 and t.info["edges_split"] == 0
