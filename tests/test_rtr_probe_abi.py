"""CPU tests of the ABI of the test export xm_ctx_rtr_probe (include/xm_amd.h): the prototype and the structs compile from the header, the
symbol is exported, the ABI revision stays where it was (an added export), and the binding's structs and argument list agree with the header."""
import ctypes
import inspect
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("struct_size", "flags", "o", "k", "lam", "R", "s", "pR", "ps", "rR", "rs", "vR", "vs", "HvR", "Hvs", "partsB_in", "X", "partsB_in_count", "scal_in",
          "product_kind", "nA", "nB", "w_native", "wpad", "split_k", "sell_gather", "f", "rr", "pHp", "rHp", "HpHp", "rr_parts", "dual", "init_scal", "scal_out", "G", "egs", "S0", "rgR",
          "rgs", "HpR", "Hps", "init_rR", "init_rs", "init_pR", "init_ps", "init_vR", "init_vs", "init_HvR", "init_Hvs", "init_W", "init_Wpad", "out_vR",
          "out_vs", "out_HvR", "out_Hvs", "out_rR", "out_rs", "out_pR", "out_ps", "out_W", "out_Wpad", "partsB_out", "Lam", "dz", "SX")
SCAL = ("rr", "vv", "vp", "pp", "delta", "gradnorm", "last_step", "model", "status", "iter")
FLAGS = ("XM_RTR_PROBE_AUTO", "XM_RTR_PROBE_MODEL_REC", "XM_RTR_PROBE_TCG_INIT", "XM_RTR_PROBE_CG_STEP", "XM_RTR_PROBE_CERT")
PROTO = " int (*f)(xm_ctx_t *, xm_rtr_probe_t *) = xm_ctx_rtr_probe; (void)f;"


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %d", sizeof(xm_rtr_probe_t), sizeof(xm_rtr_scal_t), XM_ABI_REVISION);\n'
           + "".join(f' printf(" %u", (unsigned){f});\n' for f in FLAGS)
           + "".join(f' printf(" %zu", offsetof(xm_rtr_scal_t, {f}));\n' for f in SCAL)
           + "".join(f' printf(" %zu", offsetof(xm_rtr_probe_t, {f}));\n' for f in FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declaration must match the signature above (the executable never calls it, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    size, scal_size, rev, *rest = _c_values()
    flags, scal_offs, offs = rest[:len(FLAGS)], rest[len(FLAGS):len(FLAGS) + len(SCAL)], rest[len(FLAGS) + len(SCAL):]
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # an added export: the revision stays
    assert flags == [xmamd.RTR_PROBE_AUTO, xmamd.RTR_PROBE_MODEL_REC, xmamd.RTR_PROBE_TCG_INIT, xmamd.RTR_PROBE_CG_STEP, xmamd.RTR_PROBE_CERT] == [1, 2, 4, 8, 16]
    assert ctypes.sizeof(xmamd.RtrScal) == scal_size and [getattr(xmamd.RtrScal, f).offset for f in SCAL] == scal_offs
    assert ctypes.sizeof(xmamd.RtrProbe) == size
    assert [getattr(xmamd.RtrProbe, f).offset for f in FIELDS] == offs
    assert set(FIELDS) | {"pad", "pad2"} == {k for k, _ in xmamd.RtrProbe._fields_}


def test_probe_is_exported(xmamd):
    assert "xm_ctx_rtr_probe" in xmamd.EXPORTS and hasattr(xmamd.lib(), "xm_ctx_rtr_probe")
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert "xm_ctx_rtr_probe" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_wrapper_arguments(xmamd):
    sig = inspect.signature(xmamd.Context.rtr_probe)
    assert list(sig.parameters) == ["self", "o", "lam", "R", "s", "p", "r", "auto", "tcg_init", "delta", "cg_step", "model_recurrence", "cert", "X"]
    assert xmamd.RTR_SCAL_IN == ("rr", "vv", "vp", "pp", "delta", "gradnorm", "model", "iter")
