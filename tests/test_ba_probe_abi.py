"""CPU tests of the ABI of the test export xm_ctx_ba_probe (include/xm_amd.h): the prototype and the struct compile from the header, the
symbol is exported, the ABI revision stays where it was (an added export), and the binding's struct and argument list agree with the header."""
import ctypes
import inspect
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("struct_size", "flags", "loss", "loss_scale", "mu", "k", "X", "dc", "cost", "gmax", "cost1", "model", "step2", "x2", "n_used", "nagg",
          "ncoarse", "coarse_ok", "b", "g_l", "vinv", "ustar", "sinv", "cused", "lused", "SX", "Sdense", "MX", "Pm", "dropped", "Ac", "dP", "rot1", "t1", "p1")
PROTO = " int (*f)(xm_ctx_t *, const double *, const double *, const double *, xm_ba_probe_t *) = xm_ctx_ba_probe; (void)f;"


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %d %d", sizeof(xm_ba_probe_t), XM_ABI_REVISION, XM_BA_PROBE_DENSE_MAX_ROWS);\n'
           + "".join(f' printf(" %zu", offsetof(xm_ba_probe_t, {f}));\n' for f in FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declaration must match the signature above (the executable never calls it, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    size, rev, rows, *offs = _c_values()
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # an added export: the revision stays
    assert rows == xmamd.BA_PROBE_DENSE_MAX_ROWS == 4096
    assert ctypes.sizeof(xmamd.BaProbe) == size
    assert [getattr(xmamd.BaProbe, f).offset for f in FIELDS] == offs


def test_probe_is_exported(xmamd):
    assert "xm_ctx_ba_probe" in xmamd.EXPORTS and hasattr(xmamd.lib(), "xm_ctx_ba_probe")
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert "xm_ctx_ba_probe" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_wrapper_arguments(xmamd):
    sig = inspect.signature(xmamd.Context.ba_probe)
    assert list(sig.parameters) == ["self", "rot", "t", "P", "mu", "fix_rotations", "loss", "loss_scale", "preconditioner", "X", "dc", "dense"]
    import numpy as np
    ctx = xmamd.Context.__new__(xmamd.Context)   # no device: the names are checked before anything else is looked at
    ctx.n, ctx.n_landmarks = 1, 1
    for kw, word in ((dict(preconditioner="multigrid"), "multigrid"), (dict(loss="tukey"), "tukey")):
        try:
            ctx.ba_probe(np.eye(3), np.zeros((3, 1)), np.zeros((3, 1)), 1.0, **kw)
        except xmamd.XmError as e:
            assert word in str(e)
        else:
            raise AssertionError(f"{word} was accepted")
