"""CPU tests of the ABI of the dense Q built from observations (xm_tuning_t.schur_dense_q, xm_ctx_dense_q, xm_create_matrix): the tuning
struct keeps its size, the new field takes the slot that was reserved, the revision stays 4 and the library exports the entry points."""
import ctypes
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("xm_ctx_dense_q", "xm_create_matrix", "xm_schur_dense_limits")


def _c_layout(compiler, std):
    """sizes and offsets as a compiler lays the header out (C and C++: the field lives in an anonymous union beside its old name)"""
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){xm_tuning_t t; t.schur_dense_q = 1; printf("%zu %zu %zu %zu %d %d\\n", sizeof(xm_tuning_t), offsetof(xm_tuning_t, hess_f32),'
           ' offsetof(xm_tuning_t, schur_dense_q), offsetof(xm_tuning_t, reserved), XM_ABI_REVISION, (int)t.reserved[0]); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "t.c" if compiler == "gcc" else "t.cpp")
        open(fn, "w").write(src)
        subprocess.check_call([compiler, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), fn, "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_header_compiles_and_the_field_sits_in_the_reserved_slot(xmamd):
    for compiler, std in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        size, off_f32, off_dq, off_res, rev, alias = _c_layout(compiler, std)
        assert size == 28 * 4                                  # revision 4: unchanged
        assert off_dq == off_res == off_f32 + 4 == 27 * 4      # where reserved[0] was (the old name stays as an alias of the same word)
        assert rev == 4 and alias == 1
    assert xmamd.lib().xm_abi_revision() == 4
    assert ctypes.sizeof(xmamd.Tuning) == 28 * 4 and xmamd.Tuning.schur_dense_q.offset == 27 * 4
    assert xmamd.Tuning().schur_dense_q == 0                   # the default leaves everything as it is


def test_entry_points_exported(xmamd):
    L = xmamd.lib()
    for s in NEW_EXPORTS:
        assert hasattr(L, s), s
    assert set(NEW_EXPORTS) <= set(xmamd.EXPORTS)
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "nm (binutils) is needed to read the dynamic symbol table"
    out = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in NEW_EXPORTS if s not in defined]
    for f in ("create_matrix", "create_matrix_arrays", "schur_dense_limits"):
        assert callable(getattr(xmamd, f))
    assert callable(xmamd.Context.dense_q)


def test_limits_are_the_documented_constants(xmamd):
    """host-only: no device is touched"""
    win, panel, cap = xmamd.schur_dense_limits()
    assert cap == 20000
    assert 12 * 8 * win <= 160 * 1024           # the assembly kernel's strip (12 doubles per window camera) fits the LDS of a gfx950 workgroup
    assert win >= 64 and panel >= 1
