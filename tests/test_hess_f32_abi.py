"""CPU tests of the ABI of the opt-in fp32 Hessian products (xm_tuning_t.hess_f32): the structs keep their sizes, the new fields take the
slots that were reserved for them, and the library exports the kernel-level entry points and their timing hooks."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("xm_dense_to_f32", "xm_qw_dense_f32", "xm_qw_dense_sym_f32")
NEW_BENCH = ("xm_qw_dense_f32_time", "xm_qw_dense_sym_f32_time")


def _c_layout():
    """sizes and offsets as a C compiler lays the header out"""
    src = ('#include "xm_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(xm_tuning_t), sizeof(xm_result_t),'
           ' offsetof(xm_tuning_t, hess_f32), offsetof(xm_tuning_t, reserved), offsetof(xm_result_t, hess_f32),'
           ' offsetof(xm_result_t, outer_on_device)); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        return tuple(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))


def test_struct_sizes_unchanged_and_fields_in_the_reserved_slots(xmamd):
    st, sr, off_t, off_res, off_r, off_dev = _c_layout()
    # revision 4 sizes: 26 settings + 2 reserved int32; the result ended with outer_on_device + reserved_ (int32 each)
    assert st == 28 * 4 and sr == off_dev + 8
    assert off_t == 26 * 4 and off_res == off_t + 4      # hess_f32 sits where reserved[0] was, reserved[1] stays reserved
    assert off_r == off_dev + 4                          # ... and where xm_result_t.reserved_ was
    assert xmamd.lib().xm_abi_revision() == 4
    # the Python mirrors agree with the header
    assert ctypes.sizeof(xmamd.Tuning) == st and ctypes.sizeof(xmamd.Result) == sr
    assert xmamd.Tuning.hess_f32.offset == off_t and xmamd.Result.hess_f32.offset == off_r
    assert "reserved_" not in dict(xmamd.Result._fields_)


def test_entry_points_exported(xmamd):
    L = xmamd.lib()
    for s in NEW_EXPORTS + NEW_BENCH:
        assert hasattr(L, s), s
    assert set(NEW_EXPORTS) <= set(xmamd.EXPORTS) and set(NEW_BENCH) <= set(xmamd.BENCH_EXPORTS)
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "nm (binutils) is needed to read the dynamic symbol table"
    out = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "xm-code_amd", "lib", "libxm_amd.so")], text=True)
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in NEW_EXPORTS + NEW_BENCH if s not in defined]


def test_solve_array_takes_hess_f32_keyword(xmamd):
    XM = xmamd.import_XM()
    doc = XM.solve_array.__doc__
    assert re.search(r"hess_f32: [^,)]*= 0\)", doc), doc
    # the file entry points keep the reference's five positional arguments
    for f in ("solve", "solve_rank3", "solve_rebuttle"):
        assert "hess_f32" not in getattr(XM, f).__doc__
