#!/usr/bin/env python3
"""Step 3 of GLOMAP's pipeline as the reference's fork runs it (controllers/global_mapper.cc:76-111): rotations that do not bend to a wrong
pair, every stage on the device, on the SIMPLE2-derived view graph of viewgraph_tracks_lift_filter_clean_solve_simple2.py with its spoiled
pairs:

    A = xmamd.view_graph_filter(foff, xy, pi, pj, model, matches, ...)                                            pass A
    ctx = xmamd.Context(vg=(pi, pj, 1, Rrel^T)) over A.pairs(); ctx.solve; xmamd.recover_rotations               the chordal optimum, certified
    plan = xmamd.view_graph_rotations(cam_from_world, pi, pj, Rrel, registered=A.registered, valid_in=A.valid)   IRLS from it (Geman-McClure, 5 deg)
    B = xmamd.view_graph_filter(..., A.matches, valid_in=A.valid, registered_in=A.registered, rot=plan.rot, score=False)   pass B

Printed: the median rotation error against the recorded ground truth gtR.bin after the solve, after the new call, and after the route the
examples took so far (solve -> pass B -> second solve over the pairs pass B keeps); and pass B's pair statuses with either set of rotations.
The recorded case's relative rotations are exact but for the spoiled pairs, so the second solve runs on pairs without any noise; its status
is printed next to its error (XM_STATUS_LS_FAILED there means its rotations are not to be used).

    python examples/robust_rotations_simple2.py

Needs an MI355X."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np               # noqa: E402
import xmamd                     # noqa: E402
import xm_viewgraph_numpy as vn  # noqa: E402


def read_bin(fn):
    """int32 rows, int32 cols, float64 column-major"""
    with open(fn, "rb") as f:
        r, c = struct.unpack("<ii", f.read(8))
        return np.frombuffer(f.read(), dtype="<f8").reshape(c, r).T.copy()


G = os.path.join(ROOT, "tests", "golden", "simple2")
gt = read_bin(os.path.join(G, "gtR.bin"))
fi = np.load(os.path.join(G, "frame_index.npy"))
c = vn.simple2_case()
n = c["foff"].size - 1
args, kw = vn.call_args(c)
ms = lambda i: 1e3 * (i["seconds_index"] + i["seconds_kernels"] + i["seconds_download"])


def solve(registered, vi, vj, vR):
    """the view-graph solve over the given pairs of the registered images -> cam_from_world (n x 3 x 3, identity where unregistered)"""
    img = np.flatnonzero(registered)
    index = np.full(n, -1, dtype=np.int32); index[img] = np.arange(img.size, dtype=np.int32)
    ctx = xmamd.Context(vg=(index[vi], index[vj], np.ones(vi.size), np.ascontiguousarray(np.transpose(vR, (0, 2, 1)))), n=img.size)
    Rs, s, info = ctx.solve(5, 1e-8, 20.0)
    rot, _, _ = xmamd.recover_rotations(Rs, s)
    ctx.close()
    cam_from_world = np.tile(np.eye(3), (n, 1, 1))
    cam_from_world[img] = np.stack([rot[:, 3 * k:3 * k + 3].T for k in range(img.size)])
    return cam_from_world, info


def median_error(cam_from_world, registered):
    """median over the registered images of |C_0 C_k^T - G_f(0) G_f(k)^T|_F, f = frame_index (gtR.bin holds world-to-camera rotations per frame)"""
    img = np.flatnonzero(registered)
    f = fi[img]
    C0, G0 = cam_from_world[img[0]], gt[:, 3 * f[0]:3 * f[0] + 3]
    return float(np.median([np.linalg.norm(C0 @ cam_from_world[k].T - G0 @ gt[:, 3 * fk:3 * fk + 3].T) for k, fk in zip(img, f)]))


def pass_b(rot, A):
    return xmamd.view_graph_filter(c["foff"], c["xy"], c["pi"], c["pj"], c["model"], A.matches,
                                   **dict(kw, valid_in=A.valid, registered_in=A.registered, rot=rot, score=False))


def statuses(B):
    i = B.info
    return (f"{i['pairs_valid']} valid, {i['pairs_rotation']} rotation, {i['pairs_outside']} outside, {i['largest']} of {n} images registered "
            f"({ms(i):.2f} ms)")


A = xmamd.view_graph_filter(*args, **kw)
print(f"pass A: {A.info['pairs_valid']} of {c['pi'].size} pairs valid, {A.info['largest']} of {n} images registered ({ms(A.info):.2f} ms)")
vi, vj, vR = A.pairs()
chordal, info = solve(A.registered, vi, vj, vR)
print(f"view-graph solve over {vi.size} pairs: rank {info['rank']}, status {info['status']}")

plan = xmamd.view_graph_rotations(chordal, c["pi"], c["pj"], c["Rrel"], registered=A.registered, valid_in=A.valid)
i = plan.info
print(f"robust averaging: {i['pairs']} pairs of {i['registered']} images, fixed image {i['fixed_image']}, {i['cams_heavy']} cameras with a workgroup of "
      f"their own (most incidences {i['max_incidences']}); {i['irls_iterations']} IRLS iterations, {i['pcg_iterations']} PCG iterations "
      f"({i['pcg_capped']} capped), stop: {i['stop']}; steps {np.array2string(plan.step_trace, precision=6)}; {ms(i):.2f} ms "
      f"({1e3 * i['seconds_kernels']:.2f} ms of kernels)")
k = np.flatnonzero(plan.weight > 0)
sigma2 = np.radians(5.0) ** 2
print(f"weights: {int(np.sum(plan.weight[k] < 1.0))} of {k.size} pairs below 1, {int(np.sum(plan.weight[k] > 10.0))} above 10 (1 / sigma^2 = {1.0 / sigma2:.1f})")

B_chordal, B_robust = pass_b(chordal, A), pass_b(plan.rot, A)
print("pass B with the solve's rotations:  ", statuses(B_chordal))
print("pass B with the refined rotations:  ", statuses(B_robust))
print("pair statuses equal:", bool(np.array_equal(B_chordal.pair_status, B_robust.pair_status)), "| pairs that differ:",
      int(np.sum(B_chordal.pair_status != B_robust.pair_status)))

# the route so far: the pairs pass B keeps (with the solve's rotations), solved again
bi, bj, bR = B_chordal.pairs()
second, info2 = solve(B_chordal.registered, bi, bj, bR)
print(f"second view-graph solve over {bi.size} pairs: rank {info2['rank']}, status {info2['status']}"
      + (" (XM_STATUS_LS_FAILED: these pairs carry no noise and the cost is 0 to rounding)" if info2["status"] == -2 else ""))
both = (A.registered != 0) & (B_chordal.registered != 0) & (B_robust.registered != 0)
print(f"median rotation error against gtR.bin over the {int(both.sum())} images registered throughout: after the solve {median_error(chordal, both):.3e}, "
      f"after the robust averaging {median_error(plan.rot, both):.3e}, after solve -> pass B -> second solve {median_error(second, both):.3e}")
