"""CPU tests of the ABI of the global positioning with pairs (xm_ctx_global_positioning_pairs, xm_ctx_gp_probe_pairs, xm_gp_pair_limits;
include/xm_amd.h): sizes and offsets of the two new structs against a compiled C snippet and the ctypes mirrors, the constants, the
exports, and the structs of xm_ctx_global_positioning left as they were."""
import ctypes
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("xm_ctx_global_positioning_pairs", "xm_ctx_gp_probe_pairs", "xm_gp_pair_limits")
PAIRS_FIELDS = ("constraint", "flags", "npairs", "pi", "pj", "trel", "valid", "calibrated", "reweight_scale", "sigma", "pairs_used", "cams_heavy",
                "max_incidences", "weight_scale_pt")
PROBE_FIELDS = ("sigma_in", "cost", "gsmax", "cost1", "model", "step2", "x2", "Mp", "qp", "pfrozen", "pused", "dsigma", "sigma1")


def _c_numbers():
    items = ["sizeof(xm_gp_options_t)", "sizeof(xm_gp_result_t)", "sizeof(xm_gp_probe_t)", "sizeof(xm_gp_pairs_t)", "sizeof(xm_gp_pair_probe_t)"]
    items += [f"offsetof(xm_gp_pairs_t, {f})" for f in PAIRS_FIELDS] + [f"offsetof(xm_gp_pair_probe_t, {f})" for f in PROBE_FIELDS]
    items += ["(size_t)XM_GP_ONLY_POINTS", "(size_t)XM_GP_ONLY_CAMERAS", "(size_t)XM_GP_POINTS_AND_CAMERAS_BALANCED", "(size_t)XM_GP_POINTS_AND_CAMERAS",
              "(size_t)XM_GP_FIX_CENTRES"]
    src = '#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + "".join(f'printf("%zu\\n", {it});' for it in items) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        return list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_struct_sizes_and_offsets_match_ctypes(xmamd):
    v = _c_numbers()
    so, sr, sp, spairs, spp = v[:5]
    assert (so, sr, sp) == (80, 72, 288)                            # xm_gp_options_t, xm_gp_result_t, xm_gp_probe_t: unchanged
    assert (ctypes.sizeof(xmamd.GpOptions), ctypes.sizeof(xmamd.GpResult), ctypes.sizeof(xmamd.GpProbe)) == (so, sr, sp)
    assert (ctypes.sizeof(xmamd.GpPairs), ctypes.sizeof(xmamd.GpPairProbe)) == (spairs, spp)
    k = 5
    for f in PAIRS_FIELDS:
        assert getattr(xmamd.GpPairs, f).offset == v[k], f
        k += 1
    for f in PROBE_FIELDS:
        assert getattr(xmamd.GpPairProbe, f).offset == v[k], f
        k += 1
    assert v[k:k + 4] == [xmamd.GP_CONSTRAINT[c] for c in ("only_points", "only_cameras", "points_and_cameras_balanced", "points_and_cameras")]
    assert v[k + 4] == xmamd.GP_FIX_CENTRES
    assert xmamd.lib().xm_abi_revision() == 4                      # new entries only: the revision does not change


def test_entries_are_exported(xmamd):
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm
    out = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in SYMBOLS:
        assert hasattr(xmamd.lib(), s) and s in xmamd.EXPORTS and s in names, s


def test_pair_limits(xmamd):
    assert xmamd.gp_pair_limits() == dict(light_max=64, threads=256)
    assert xmamd.lib().xm_gp_pair_limits(None) == -2               # XM_ERR_ARG
