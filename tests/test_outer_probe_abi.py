"""CPU tests of the ABI of the test export xm_ctx_outer_probe (include/xm_amd.h): the prototype and the structs compile from the header, the
symbol is exported, the ABI revision stays where it was (an added export; xm_rtr_probe_t is untouched), and the binding's structs and argument
list agree with the header."""
import ctypes
import inspect
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("struct_size", "flags", "o", "slot", "lam", "t", "R", "s", "vR", "vs", "HvR", "Hvs", "D", "pR", "ps", "rR", "rs", "Rc", "sc", "partsB_in", "partsM_in",
          "partsB_in_count", "partsM_in_count", "scal_in", "os_in", "delta_bar", "gradtol", "max_outer", "stop_req", "product_kind", "nA", "nB", "nM", "w_native",
          "wpad", "polar", "grid", "nwave", "trace_written", "run", "ret_pad", "ls_pad", "out_pad", "f", "rr", "model", "pHp", "rHp", "HpHp", "f_cand", "rr_cand",
          "m_cand", "progress", "scal_out", "os_out", "trace", "rgR", "rgs", "ret_Rc", "ret_sc", "ret_W", "ret_Wpad", "ret_partsM", "ls_Rc", "ls_W", "HpR", "Hps",
          "cand_G", "cand_egs", "cand_S0", "cand_rgR", "cand_rgs", "out_R", "out_s", "out_Rc", "out_sc", "out_vR", "out_vs", "out_HvR", "out_Hvs", "out_rR",
          "out_rs", "out_pR", "out_ps", "out_W", "out_Wpad", "out_partsB", "out_partsM", "out_G", "out_egs", "out_S0", "out_rgR", "out_rgs")
TCG = ("rr", "vv", "vp", "pp", "delta", "gradnorm", "last_step", "model", "status", "iter", "seq", "phase")
OS = ("loss", "rr_point", "totalite", "shrink_count", "k", "stop_reason", "time_up", "slots")
FLAGS = ("XM_OUTER_PROBE_RETRACT", "XM_OUTER_PROBE_MODEL_REC", "XM_OUTER_PROBE_RETRACT_LS", "XM_OUTER_PROBE_STEP", "XM_OUTER_PROBE_POLAR", "XM_OUTER_PROBE_MGS",
         "XM_OUTER_PROBE_AUTO")
PROTO = " int (*f)(xm_ctx_t *, xm_outer_probe_t *) = xm_ctx_outer_probe; (void)f;"


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu %zu %d", sizeof(xm_outer_probe_t), sizeof(xm_outer_tcg_t), sizeof(xm_outer_scal_t), sizeof(xm_rtr_probe_t), XM_ABI_REVISION);\n'
           + "".join(f' printf(" %u", (unsigned){f});\n' for f in FLAGS)
           + "".join(f' printf(" %zu", offsetof(xm_outer_tcg_t, {f}));\n' for f in TCG)
           + "".join(f' printf(" %zu", offsetof(xm_outer_scal_t, {f}));\n' for f in OS)
           + "".join(f' printf(" %zu", offsetof(xm_outer_probe_t, {f}));\n' for f in FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declaration must match the signature above (the executable never calls it, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    size, tcg_size, os_size, rtr_size, rev, *rest = _c_values()
    cut = (len(FLAGS), len(FLAGS) + len(TCG), len(FLAGS) + len(TCG) + len(OS))
    flags, tcg_offs, os_offs, offs = rest[:cut[0]], rest[cut[0]:cut[1]], rest[cut[1]:cut[2]], rest[cut[2]:]
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # an added export: the revision stays
    assert rtr_size == ctypes.sizeof(xmamd.RtrProbe)                              # the existing probe's struct did not change
    assert flags == [xmamd.OUTER_PROBE_RETRACT, xmamd.OUTER_PROBE_MODEL_REC, xmamd.OUTER_PROBE_RETRACT_LS, xmamd.OUTER_PROBE_STEP, xmamd.OUTER_PROBE_POLAR,
                     xmamd.OUTER_PROBE_MGS, xmamd.OUTER_PROBE_AUTO] == [1, 2, 4, 8, 16, 32, 64]
    assert ctypes.sizeof(xmamd.OuterTcg) == tcg_size and [getattr(xmamd.OuterTcg, f).offset for f in TCG] == tcg_offs
    assert ctypes.sizeof(xmamd.OuterScal) == os_size and [getattr(xmamd.OuterScal, f).offset for f in OS] == os_offs
    assert ctypes.sizeof(xmamd.OuterProbe) == size
    assert [getattr(xmamd.OuterProbe, f).offset for f in FIELDS] == offs
    assert set(FIELDS) | {"pad", "pad2"} == {k for k, _ in xmamd.OuterProbe._fields_}
    assert set(TCG) == {k for k, _ in xmamd.OuterTcg._fields_} and set(OS) | {"pad"} == {k for k, _ in xmamd.OuterScal._fields_}


def test_probe_is_exported(xmamd):
    assert "xm_ctx_outer_probe" in xmamd.EXPORTS and hasattr(xmamd.lib(), "xm_ctx_outer_probe")
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert "xm_ctx_outer_probe" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_wrapper_arguments_and_the_progress_word(xmamd):
    sig = inspect.signature(xmamd.Context.outer_probe)
    assert list(sig.parameters) == ["self", "o", "lam", "R", "s", "v", "Hv", "retract", "model_recurrence", "retraction", "auto", "model", "partsM_fill", "ls", "step"]
    assert (xmamd.PH_TCG, xmamd.PH_CAND, xmamd.PH_STOP, xmamd.PH_INIT) == (0, 1, 2, 3)
    assert xmamd.pack_prog(7, 5, xmamd.PH_CAND) == (7 << 32) | (5 << 8) | 1 and xmamd.pack_prog(1, 1 << 24, 0) == 1 << 32
