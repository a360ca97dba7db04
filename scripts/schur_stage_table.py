#!/usr/bin/env python3
"""Condense the STAGE_ERR / STAGE_SYM / PCG_ITERS lines of a run of the matrix-free Q's stage tests into profiles/r19_schur_stage_errors.txt:

    python -m pytest tests/test_gpu_schur_stages.py -m gpu -s -q > run.log
    python scripts/schur_stage_table.py run.log [parent_hashes.txt head_hashes.txt] > profiles/r19_schur_stage_errors.txt

The two optional files hold lines "QW_SHA256 <label> <case> <form> o<k> <sha256 of ctx.qw's bytes>" from the parent commit's library and from
this one's; they are printed side by side."""
import collections
import re
import sys

worst, cases, sym, iters, n_err, tail = {}, collections.OrderedDict(), {}, collections.OrderedDict(), 0, ""
for line in open(sys.argv[1]):
    if re.search(r"\d+ (passed|failed)", line):
        tail = line.strip().strip("= ")
    for m in re.finditer(r"STAGE_ERR (\S+) (\S+) (o\d+) (\S+): e_ref (\d\S*) e_gpu (\d\S*) ratio \S+ bound (\d\S*) worst block (\d+)", line):
        case, form, o, k, er, eg, bd, blk = m.groups()
        v = float(eg) / float(bd)
        n_err += 1
        if v > worst.get(k, (-1.0,))[0]:
            worst[k] = (v, f"{case} {form} {o}", er, eg, blk)
        c = cases.setdefault(f"{case} {form}", [0, (-1.0,)])
        c[0] += 1
        if v > c[1][0]:
            c[1] = (v, f"{k} {o}", er, eg)
    for m in re.finditer(r"STAGE_SYM (\S+) (\S+) (\S+): (\d\S*) bound (\d\S*)", line):
        v = float(m.group(4)) / float(m.group(5))
        if v > sym.get(m.group(3), (-1.0,))[0]:
            sym[m.group(3)] = (v, f"{m.group(1)} {m.group(2)}", m.group(4))
    for m in re.finditer(r"PCG_ITERS (\S+) (\S+) (o\d+): gpu (\d+) numpy \((\d+), (\d+)\)", line):
        iters.setdefault(f"{m.group(1)} {m.group(2)}", []).append(f"{m.group(3)} {m.group(4)}/{m.group(5)}")
print(f"Stage errors of the matrix-free Q on one MI355X (gfx950): python -m pytest tests/test_gpu_schur_stages.py -m gpu -s ({tail}),")
print("condensed by scripts/schur_stage_table.py.  e_ref = error of the f64 numpy restatement (tests/xm_schur_stages.py) against the longdouble")
print("reference (tests/xm_schur_exact.py), e_gpu = error of the probe's output against the same longdouble values, ratio = e_gpu / max(16 e_ref,")
print("64 eps_f64) (the bound: <= 1).  Errors per landmark row, camera row, camera block or aggregate block against the larger of the exact")
print(f"block's maximum and the magnitude of the terms it is formed from.  The run printed {n_err} STAGE_ERR lines.")
print("\nWorst ratio per quantity (case form o: e_ref, e_gpu, worst block):")
for k, (v, label, er, eg, blk) in sorted(worst.items(), key=lambda x: -x[1][0]):
    print(f"  {k:8s} {v:.3f}  ({label}: {er}, {eg}, block {blk})")
print("\nWorst quantity per case and form (comparisons; quantity o: e_ref, e_gpu, ratio):")
for label, (cnt, (v, k, er, eg)) in cases.items():
    print(f"  {label:24s} {cnt:3d}  {k}: {er}, {eg}, {v:.3f}")
print("\nSymmetry on the identity columns, |A - A^T| / |A| over the bound (largest; case, value):")
for k, (v, label, val) in sym.items():
    print(f"  X^T ({'VT' if k == 'VX' else 'M^-1'} X)  {v:.3f}  ({label}: {val})")
print("\nInner iterations of the CG forms, o gpu/numpy restatement (printed, not asserted):")
for label, v in iters.items():
    print(f"  {label:24s} {'  '.join(v)}")
if len(sys.argv) > 3:
    rows = [collections.OrderedDict((tuple(l.split()[2:5]), l.split()[5]) for l in open(f) if l.startswith("QW_SHA256")) for f in sys.argv[2:4]]
    same = sum(rows[0][k] == rows[1].get(k) for k in rows[0])
    print(f"\nSHA-256 of the bytes of ctx.qw(W, alpha), parent commit | this commit ({same} of {len(rows[0])} rows equal):")
    for k, h in rows[0].items():
        print(f"  {' '.join(k):22s} {h} {rows[1].get(k)}{'' if h == rows[1].get(k) else '   DIFFERENT'}")
