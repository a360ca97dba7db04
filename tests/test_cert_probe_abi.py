"""CPU tests of the ABI of the test export xm_ctx_cert_probe and of the host export xm_tridiag_min (include/xm_amd.h): the prototypes and the
struct compile from the header, the symbols are exported, the ABI revision stays where it was (added exports; xm_rtr_probe_t and
xm_outer_probe_t are untouched), and the binding's struct and argument lists agree with the header."""
import ctypes
import inspect
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("struct_size", "flags", "o", "cap", "lam", "R", "s", "ret", "eig_exact", "iters", "m_use", "cycles", "mmax", "steps_dev", "steps_fused", "steps_unfused", "nseg",
          "product_kind", "len", "theta", "resid", "dual", "Lam", "dz", "alpha", "beta", "V", "c1", "c2", "y", "x")
PROTO = (" int (*f)(xm_ctx_t *, xm_cert_probe_t *) = xm_ctx_cert_probe; (void)f;"
         " int (*g)(const double *, const double *, int, double *, double *, double *) = xm_tridiag_min; (void)g;")
RTR_PROBE_SIZE, OUTER_PROBE_SIZE = 688, 944               # sizeof of the two older probe structs on the LP64 ABI the library is built for


def _c_values():
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu %d %u", sizeof(xm_cert_probe_t), sizeof(xm_rtr_probe_t), sizeof(xm_outer_probe_t), XM_ABI_REVISION, (unsigned)XM_CERT_PROBE_UNFUSED);\n'
           + "".join(f' printf(" %zu", offsetof(xm_cert_probe_t, {f}));\n' for f in FIELDS) + PROTO + ' printf("\\n"); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # -c first: the declarations must match the signatures above (the executable never calls them, so it is linked without the library)
        subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        open(os.path.join(d, "t2.c"), "w").write(src.replace(PROTO, ""))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t2.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_and_binding_agree(xmamd):
    size, rtr_size, outer_size, rev, unfused, *offs = _c_values()
    assert rev == 4 and xmamd.lib().xm_abi_revision() == rev                      # added exports: the revision stays
    assert rtr_size == ctypes.sizeof(xmamd.RtrProbe) == RTR_PROBE_SIZE            # the two older probes' structs did not change
    assert outer_size == ctypes.sizeof(xmamd.OuterProbe) == OUTER_PROBE_SIZE
    assert unfused == xmamd.CERT_PROBE_UNFUSED == 1
    assert ctypes.sizeof(xmamd.CertProbe) == size
    assert [getattr(xmamd.CertProbe, f).offset for f in FIELDS] == offs
    assert set(FIELDS) | {"pad2"} == {k for k, _ in xmamd.CertProbe._fields_}


def test_exports_are_there(xmamd):
    so = os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("xm_ctx_cert_probe", "xm_tridiag_min", "xm_ctx_rtr_probe", "xm_ctx_outer_probe"):
        assert sym in xmamd.EXPORTS and hasattr(xmamd.lib(), sym) and sym in names, sym


def test_wrapper_arguments(xmamd):
    assert list(inspect.signature(xmamd.Context.cert_probe).parameters) == ["self", "o", "lam", "R", "s", "unfused", "mmax", "want_V"]
    assert list(inspect.signature(xmamd.tridiag_min).parameters) == ["a", "b"]
