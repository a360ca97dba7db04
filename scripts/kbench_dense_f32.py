"""fp32 Hessian products (xm_tuning_t.hess_f32): what the fp32 copy of a dense Q buys per product and per solve.
   python scripts/kbench_dense_f32.py [--n 1778 3072] [--o 3 4] [--solves 3] [--out FILE]
1. per n and o: us per product, back-to-back launches with alternating direction (HIP events), of the f64 general kernel, the f64
   symmetric pair, the fp32 general kernel and the fp32 symmetric pair, with their error against numpy on a random symmetric matrix (the
   fp32 kernels against the ROUNDED matrix).  1778 cameras = the Venice-size headline (228 MB f64, 114 MB fp32); 3072 cameras = a matrix
   whose fp32 copy (340 MB) is beyond the 256 MiB Infinity Cache.
2. the Venice-size end-to-end solve (gen_dense(1778, seed 1778), max_rank 5, tol 1e-6, lam 0, the three summation groupings in turn):
   ms to the certified optimum, tCG and outer iterations, final rank, with and without hess_f32, each after one warm-up solve.
The first line stamps the sources (bench.py's source hash)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np

import xmamd
import xm_testlib as tl
from bench import source_sha256

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[1778, 3072])
ap.add_argument("--o", type=int, nargs="*", default=[3, 4])
ap.add_argument("--solves", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
out = open(a.out, "w") if a.out else sys.stdout


def emit(s):
    print(s, file=out, flush=True)
    if out is not sys.stdout:
        print(s, flush=True)


L = xmamd.lib()
xmamd.require_gpu()
emit(f"# scripts/kbench_dense_f32.py  sources_sha256 {source_sha256()[:16]}  {L.xm_version().decode()}  {time.strftime('%Y-%m-%dT%H:%M:%SZ', time.gmtime())}")
emit("## 1. us per product (alternating direction; algorithmic GB/s = bytes of the STORED matrix the kernel reads + W in / out, over the time)")
ms = C.c_double()
for n in a.n:
    m, ld = 3 * n, xmamd.dense_ld(n)
    reps = 200 if n < 2500 else 50
    rng = np.random.default_rng(n)
    A = rng.standard_normal((m, m)); Q = (A + A.T) * 0.5; del A
    dq = xmamd.dense_upload(Q)
    d32 = xmamd.dense_to_f32(dq, n)
    Qr = Q.astype(np.float32).astype(np.float64)
    for o in a.o:
        W = rng.standard_normal((m, o))
        dW = xmamd.DevArray(xmamd.to_rm(W, rows=ld)); dO = xmamd.DevArray(nbytes=m * xmamd.pitch_of(o) * 8)
        ref, ref32 = Q @ W, Qr @ W
        wb = 2 * 8 * m * o
        rows = [("f64 general", L.xm_qw_dense_time, L.xm_qw_dense, dq, 8 * m * m, ref),
                ("f64 symmetric", L.xm_qw_dense_sym_time, L.xm_qw_dense_sym, dq, 4 * m * (m + 6), ref),
                ("fp32 general", L.xm_qw_dense_f32_time, L.xm_qw_dense_f32, d32, 4 * m * m, ref32),
                ("fp32 symmetric", L.xm_qw_dense_sym_f32_time, L.xm_qw_dense_sym_f32, d32, 2 * m * (m + 6), ref32)]
        for name, tfn, fn, dmat, qb, r in rows:
            xmamd._chk(fn(dmat.ptr, n, o, dW.ptr, dO.ptr, 1.0, None)); xmamd._chk(L.xm_dev_sync())
            err = tl.rel_fro(xmamd.from_rm(dO.get(), m, o), r)
            xmamd._chk(tfn(dmat.ptr, n, o, dW.ptr, dO.ptr, reps, C.byref(ms)))
            emit(f"n={n:5d} ({8 * m * m / 1e6:6.0f} MB f64) o={o} {name:15s} {ms.value * 1e3:9.1f} us  {(qb + wb) / ms.value / 1e6:7.0f} GB/s"
                 f"  rel err {err:.1e}")
        dW.free(); dO.free()
    dq.free(); d32.free()

emit("## 2. Venice-size solve (gen_dense(1778, seed 1778), max_rank 5, tol 1e-6, lam 0): ms to the certified optimum, groupings 0, 1, 2, ...")
Q = tl.gen_dense(1778, seed=1778)["Q"]
for hf in (0, 1):
    ctx = xmamd.Context(Q=Q, tuning=dict(hess_f32=hf) if hf else None)
    ctx.solve(5, 1e-6, 0.0)                                  # warm-up
    for i in range(a.solves):
        R, s, info = ctx.solve(5, 1e-6, 0.0, grouping=i % 3)
        emit(f"hess_f32={hf} grouping={i % 3}  {info['seconds'] * 1e3:7.1f} ms  status {info['status']} rank {info['rank']}  tcg {info['tcg_iters']:5d}"
             f"  outer {info['outer_iters']:4d}  primal {info['primal']:.12g}  sym {info['sym_product']} hess_f32 {info['hess_f32']}"
             f"  qw_stream_bytes {info['qw_stream_bytes']}")
    ctx.close()
