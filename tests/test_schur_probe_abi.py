"""CPU tests of the ABI of the test export xm_ctx_schur_probe (include/xm_amd.h): the prototype and the struct compile from the header, the
symbol is exported, the ABI revision stays where it was (an added export, as for the four older probes), the binding's struct and argument
list agree with the header, and the refusals that need no device."""
import ctypes
import inspect
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("struct_size", "flags", "o", "k", "alpha", "W", "X", "nheavy", "lm_total", "nagg", "uses_cg", "two_level", "dup_pairs", "pcg_done", "pcg_iters",
          "pcg_cap", "pcg_relres", "pcg_tol", "deg", "perm", "Q1", "c", "q2", "q3inv", "dinv", "VTinv", "binv", "ainv", "h", "r", "xc", "xl", "Y", "VX",
          "pAp", "MX")
PROTO = " int (*f)(xm_ctx_t *, xm_schur_probe_t *) = xm_ctx_schur_probe; (void)f;"


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu %d %d", sizeof(xm_schur_probe_t), sizeof(xm_ba_probe_t), sizeof(xm_cert_probe_t), XM_ABI_REVISION,'
           ' XM_SCHUR_PROBE_DENSE_MAX_ROWS);\n'
           + "".join(f' printf(" %zu", offsetof(xm_schur_probe_t, {f}));\n' for f in FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declaration must match the signature above (the executable never calls it, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    size, ba_size, cert_size, rev, rows, *offs = _c_values()
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # an added export: the revision stays
    assert rows == xmamd.SCHUR_PROBE_DENSE_MAX_ROWS == 4096
    assert ctypes.sizeof(xmamd.SchurProbe) == size
    assert [getattr(xmamd.SchurProbe, f).offset for f in FIELDS] == offs
    assert ctypes.sizeof(xmamd.BaProbe) == ba_size and ctypes.sizeof(xmamd.CertProbe) == cert_size   # the older probes are untouched


def test_probe_is_exported(xmamd):
    assert "xm_ctx_schur_probe" in xmamd.EXPORTS and hasattr(xmamd.lib(), "xm_ctx_schur_probe")
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert "xm_ctx_schur_probe" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_wrapper_arguments_and_deviceless_refusals(xmamd):
    assert list(inspect.signature(xmamd.Context.schur_probe).parameters) == ["self", "W", "alpha", "X", "dense"]
    L = xmamd.lib()
    q = xmamd.SchurProbe()
    q.struct_size = ctypes.sizeof(xmamd.SchurProbe)
    assert L.xm_ctx_schur_probe(None, ctypes.byref(q)) == -2 and b"null argument" in L.xm_last_error()      # checked before any device is looked at
    assert L.xm_ctx_schur_probe(None, None) == -2
