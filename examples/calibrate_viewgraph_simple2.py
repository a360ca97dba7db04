#!/usr/bin/env python3
"""Step 1 of GLOMAP's pipeline (controllers/global_mapper.cc:37-46, ViewGraphCalibrator::Solve) in front of the view-graph steps on the GPU,
on the SIMPLE2-derived case with the focal lengths thrown away -- priors off by factors 0.7 to 1.4 in, rotations out:

    cal = xmamd.view_graph_calibrate(focal0, pp, has_prior, cam_of_image, pi, pj, model, F, valid_in=)       step 1
    A = xmamd.view_graph_filter(..., focal=cal.focal_per_image(), Kinv=cal.Kinv(), valid_in=cal.valid)       pass A
    ctx = xmamd.Context(vg=(pi, pj, 1, Rrel^T)) over A.pairs(); ctx.solve; xmamd.recover_rotations           rotation averaging
    B = xmamd.view_graph_filter(..., A.matches, valid_in=A.valid, registered_in=A.registered, rot=, score=False)   pass B

The same chain is run with the true focal lengths, and with the perturbed priors fed to pass A as they are (what a pipeline without step 1
would do).  Printed: the relative focal error after the calibration, the pairs pass A and pass B keep, and the median rotation error
against the recorded ground truth gtR.bin for each of the three.  The case (tests/xm_vgcalib_numpy.py: simple2_case) has one camera per
image and F built from the relative poses and the per-view intrinsics.

    python examples/calibrate_viewgraph_simple2.py [--seed 28]

Needs an MI355X."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                # noqa: E402
import xmamd                      # noqa: E402
import xm_vgcalib_numpy as vc     # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def read_bin(fn):
    """int32 rows, int32 cols, float64 column-major"""
    with open(fn, "rb") as f:
        r, c = struct.unpack("<ii", f.read(8))
        return np.frombuffer(f.read(), dtype="<f8").reshape(c, r).T.copy()


G = os.path.join(ROOT, "tests", "golden", "simple2")
gt = read_bin(os.path.join(G, "gtR.bin"))
fi = np.load(os.path.join(G, "frame_index.npy"))
g, c = vc.simple2_case(seed=arg("--seed", 28))
n = len(g["truth"])
matches = (c["moff"], c["f1"], c["f2"])
poses = dict(Rrel=c["Rrel"], trel=c["trel"], FH=c["FH"])


def chain(what, focal, Kinv, valid):
    """pass A, the view-graph solve over its pairs, pass B -> median rotation error against gtR.bin over the registered images"""
    A = xmamd.view_graph_filter(c["foff"], c["xy"], c["pi"], c["pj"], c["model"], matches, focal=focal, Kinv=Kinv, valid_in=valid, **poses)
    img = np.flatnonzero(A.registered)
    index = np.full(n, -1, dtype=np.int32); index[img] = np.arange(img.size, dtype=np.int32)
    vi, vj, vR = A.pairs()
    ctx = xmamd.Context(vg=(index[vi], index[vj], np.ones(vi.size), np.ascontiguousarray(np.transpose(vR, (0, 2, 1)))), n=img.size)
    Rs, s, info = ctx.solve(5, 1e-8, 20.0)
    rot, scale, _ = xmamd.recover_rotations(Rs, s)
    ctx.close()
    cam_from_world = np.tile(np.eye(3), (n, 1, 1))
    cam_from_world[img] = np.stack([rot[:, 3 * k:3 * k + 3].T for k in range(img.size)])
    B = xmamd.view_graph_filter(c["foff"], c["xy"], c["pi"], c["pj"], c["model"], A.matches, focal=focal, Kinv=Kinv, valid_in=A.valid,
                                registered_in=A.registered, rot=cam_from_world, score=False, **poses)
    f = fi[img]
    err = float(np.median([np.linalg.norm(rot[:, :3].T @ rot[:, 3 * k:3 * k + 3] - gt[:, 3 * f[0]:3 * f[0] + 3] @ gt[:, 3 * f[k]:3 * f[k] + 3].T)
                           for k in range(img.size)]))
    print(f"{what}: pass A keeps {A.info['pairs_valid']} pairs ({A.info['inliers']} inliers, {A.info['largest']} of {n} images), the solve ends at rank "
          f"{info['rank']}, pass B keeps {B.info['pairs_valid']} pairs; median rotation error against gtR.bin {err:.3e}")
    return A, B


cal = xmamd.view_graph_calibrate(g["focal0"], g["pp"], g["has_prior"], g["cam_of_image"], g["pi"], g["pj"], g["model"], g["F"], valid_in=g["valid_in"])
i = cal.info
print(f"calibration: {i['pairs']} pairs, {i['cams_free']} free cameras ({i['cams_heavy']} with a workgroup of their own); {i['iterations']} iterations, "
      f"{i['pcg_iterations']} PCG iterations, stop: {i['stop']}; cost {i['initial_cost']:.3e} -> {i['final_cost']:.3e}; {i['cams_rejected']} cameras rejected, "
      f"{i['pairs_invalidated']} pairs invalidated; {1e3 * (i['seconds_index'] + i['seconds_kernels'] + i['seconds_download']):.2f} ms "
      f"({1e3 * i['seconds_kernels']:.2f} ms of kernels)")
print(f"relative focal error: priors {np.max(np.abs(g['focal0'] - g['truth']) / g['truth']):.3e}, calibrated {np.max(np.abs(cal.focal - g['truth']) / g['truth']):.3e}")
At, Bt = chain("true focal lengths", g["truth"], c["Kinv"], g["valid_in"])
Ac, Bc = chain("calibrated", cal.focal_per_image(), cal.Kinv(), cal.valid)
Kp = np.zeros((n, 3, 3)); Kp[:, 0, 0] = Kp[:, 1, 1] = 1.0 / g["focal0"]; Kp[:, 2, 2] = 1.0
Kp[:, 0, 2] = -g["pp"][:, 0] / g["focal0"]; Kp[:, 1, 2] = -g["pp"][:, 1] / g["focal0"]
chain("priors as they are", g["focal0"], Kp, g["valid_in"])
print("pair statuses of the calibrated run equal those of the true focal lengths: pass A", bool(np.array_equal(Ac.pair_status, At.pair_status)),
      "pass B", bool(np.array_equal(Bc.pair_status, Bt.pair_status)))
