#!/usr/bin/env python3
"""Condense the STAGE_ERR / STAGE_CONS lines of a run of the trust region's stage tests into profiles/r14_rtr_stage_errors.txt:

    python -m pytest tests/test_gpu_rtr_stages.py -m gpu -s -q > run.log
    python scripts/rtr_stage_table.py run.log > profiles/r14_rtr_stage_errors.txt

A second argument names the test file of the run (the outer iteration's other half: tests/test_gpu_outer_stages.py ->
profiles/r17_outer_stage_errors.txt; the certificate's eigen-solver: tests/test_gpu_cert_stages.py -> profiles/r18_cert_stage_errors.txt).  One line per case with its worst quantity (the run prints one per case and quantity), the worst case per quantity, and the largest value of every
consistency check."""
import collections
import re
import sys

cases, worst, cons, loose, n_err = collections.OrderedDict(), {}, collections.OrderedDict(), [], 0
tail = "passed"
for line in open(sys.argv[1]):
    if re.search(r"\d+ (passed|failed)", line):
        tail = line.strip().strip("= ")
    for m in re.finditer(r"STAGE_(ERR|CONS) (\S+) (.*?)(?=\.*STAGE_|$)", line.rstrip("\n")):
        kind, label, rest = m.group(1), m.group(2), m.group(3).rstrip(".FEsx ")
        r = re.match(r"(\S+): e_ref (\S+), e_gpu (\S+), ratio (\S+)$", rest)
        if kind == "ERR" and r:
            k, er, eg, v = r.group(1), r.group(2), r.group(3), float(r.group(4))
            n_err += 1
            c = cases.setdefault(label, [0, (-1.0,)])
            c[0] += 1
            if v > c[1][0]:
                c[1] = (v, k, er, eg)
            if v > worst.get(k, (-1.0,))[0]:
                worst[k] = (v, label, er, eg)
            continue
        r = re.match(r"(.*): (\S+e[+-]\d+)$", rest)
        if kind == "CONS" and r:
            c = cons.setdefault(r.group(1), [0, -1.0, ""])
            c[0] += 1
            if float(r.group(2)) > c[1]:
                c[1], c[2] = float(r.group(2)), label
        elif kind == "CONS":
            loose.append(f"{label} {rest}")
tests = sys.argv[2] if len(sys.argv) > 2 else "tests/test_gpu_rtr_stages.py"
what = "the certificate's eigen-solver" if "cert" in tests else "the trust region's kernels"
print(f"Stage errors of {what} on one MI355X (gfx950): python -m pytest {tests} -m gpu -s ({tail}),")
print("condensed by scripts/rtr_stage_table.py.  e_ref = error of the f64 run of tests/xm_rtr_exact.py against its longdouble run, e_gpu = error of the")
print("kernel's output against the same longdouble values, ratio = e_gpu / max(16 e_ref, 64 eps_f64) (the bound: <= 1).  Errors per camera block against")
print(f"the larger of the exact block's maximum and the magnitude of the terms it is formed from.  The run printed {n_err} STAGE_ERR lines.")
print("\nWorst ratio per quantity (case: e_ref, e_gpu):")
for k, (v, label, er, eg) in sorted(worst.items(), key=lambda x: -x[1][0]):
    print(f"  {k:16s} {v:.3f}  ({label}: {er}, {eg})")
print("\nWorst quantity per case (quantities compared; quantity: e_ref, e_gpu, ratio):")
for label, (cnt, (v, k, er, eg)) in cases.items():
    print(f"  {label:34s} {cnt:2d}  {k}: {er}, {eg}, {v:.3f}")
print("\nConsistency checks without a reference (STAGE_CONS; number of cases, largest value and its case):")
for k, (cnt, v, label) in cons.items():
    print(f"  {k}: {cnt}, {v:.3e} ({label})")
for t in loose:
    print(f"  {t}")
