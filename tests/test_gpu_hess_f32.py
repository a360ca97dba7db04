"""GPU tests of the opt-in fp32 Hessian products (xm_tuning_t.hess_f32; run with -m gpu on an MI355X), through the C ABI of libxm_amd.so.

With the setting on, the Hessian products of the truncated CG read an fp32 copy of a dense Q (loaded as fp32, accumulated in f64); cost,
gradient, certificate and Lanczos stay on the f64 matrix.  The kernels must compute exactly the product with the ROUNDED matrix (to f64
round-off), the conversion must be numpy's astype(float32) bit for bit, a solve must reach the same certified optimum as the f64 solve,
contexts the setting does not cover must be refused cleanly, and with the setting off nothing may change."""
import json
import os

import numpy as np
import pytest

import xm_testlib as tl

pytestmark = pytest.mark.gpu
G = tl.GOLDEN


def _symmetric(n, seed):
    """random symmetric 3n x 3n matrix with entries that exercise the rounding: fp32 subnormals, values below the smallest subnormal,
    round-to-even ties and values far outside [-1, 1]"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((3 * n, 3 * n))
    A[0, 1:6] = [1e-40, -3e-39, 1e-46, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24]   # subnormal, subnormal, below half the least subnormal, ties
    A[2, 7] = 1.0e4
    return (A + A.T) * 0.5


@pytest.mark.parametrize("n", [37, 149, 1000, 1778])
def test_kernels_match_the_rounded_matrix(xmamd, n):
    """xm_dense_to_f32 is astype(float32) bit for bit (padding zero); xm_qw_dense_f32 (o = 1, 3, 4, 5, 8) and xm_qw_dense_sym_f32 (o = 3..5)
    equal Q.astype(float32).astype(float64) @ W to 1e-13 relative"""
    L = xmamd.lib()
    Q = _symmetric(n, seed=n)
    Q32 = Q.astype(np.float32)
    Qr = Q32.astype(np.float64)
    ld = xmamd.dense_ld(n)
    dq = xmamd.dense_upload(Q)
    d32 = xmamd.dense_to_f32(dq, n)
    dq.free()
    got = d32.get(np.float32).reshape(3 * n, ld)
    assert np.array_equal(got[:, :3 * n].view(np.uint32), Q32.view(np.uint32))      # (device rows = rows of Q: symmetric, row-major)
    assert not got[:, 3 * n:].any()
    rng = np.random.default_rng(n + 1)
    for o, sym in [(1, False), (3, False), (4, False), (5, False), (8, False), (3, True), (4, True), (5, True)]:
        W = rng.standard_normal((3 * n, o))
        dW = xmamd.DevArray(xmamd.to_rm(W, rows=ld))
        dO = xmamd.DevArray(nbytes=3 * n * xmamd.pitch_of(o) * 8)
        fn = L.xm_qw_dense_sym_f32 if sym else L.xm_qw_dense_f32
        assert fn(d32.ptr, n, o, dW.ptr, dO.ptr, -0.5, None) == 0, xmamd.lib().xm_last_error()
        assert L.xm_dev_sync() == 0
        out = xmamd.from_rm(dO.get(), 3 * n, o)
        dW.free(); dO.free()
        ref = -0.5 * (Qr @ W)
        err = tl.rel_fro(out, ref)
        assert err < 1e-13, (n, o, sym, err)
    d32.free()


def test_conversion_refuses_non_finite(xmamd):
    """an entry beyond the fp32 range (or NaN) is reported by xm_dense_to_f32 as XM_ERR_ARG"""
    for bad in (1e39, np.nan):
        Q = _symmetric(20, seed=1)
        Q[4, 9] = Q[9, 4] = bad
        dq = xmamd.dense_upload(Q)
        with pytest.raises(xmamd.XmError, match="not finite in fp32"):
            xmamd.dense_to_f32(dq, 20)
        dq.free()


def _cases():
    Q1 = tl.load_bin(os.path.join(G, "simple1", "Q.bin"))
    e1 = json.load(open(os.path.join(G, "simple1", "expected.json")))
    yield "simple1", Q1, (e1["max_rank"], e1["tol"], e1["lam"]), False
    yield "dense200", tl.gen_dense(200, seed=200)["Q"], (5, 1e-6, 0.0), False
    yield "dense1778", tl.gen_dense(1778, seed=1778)["Q"], (5, 1e-6, 0.0), True


@pytest.mark.parametrize("outer", ["host", "device"])
def test_solve_reaches_the_f64_optimum(xmamd, outer):
    """SIMPLE1, gen_dense(200) and the Venice-size gen_dense(1778) (symmetric pair) with hess_f32 = 1 against the same solve with the
    setting at zero: same rank, certified, costs to 1e-9, rotations to 1e-6, certified from scratch by numpy, result.hess_f32 == 1 --
    in the default host-driven outer loop and under XM_FLAG_DEVICE_OUTER"""
    flags = xmamd.FLAG_DEVICE_OUTER if outer == "device" else 0
    for name, Q, (mr, tol, lam), sym in _cases():
        R0, s0, i0 = xmamd.solve_dense(Q, mr, tol, lam, flags=flags)
        R1, s1, i1 = xmamd.solve_dense(Q, mr, tol, lam, tuning=dict(hess_f32=1), flags=flags)
        assert i0["hess_f32"] == 0 and i1["hess_f32"] == 1, name
        assert i1["status"] == i0["status"] == 1 and i1["rank"] == i0["rank"], name
        assert i1["sym_product"] == i0["sym_product"] == (1 if sym else 0), name
        if outer == "device":
            assert i1["outer_on_device"] >= 1, name
        assert i1["primal"] == pytest.approx(i0["primal"], rel=1e-9), name
        assert tl.rotation_parity(R1, s1, R0, s0) <= 1e-6, name
        # the fp32 copy's bytes are what the tCG products report
        m = Q.shape[0]
        assert i1["qw_stream_bytes"] == (2 if sym else 4) * m * m and i0["qw_stream_bytes"] == (4 if sym else 8) * m * m, name
        cn = tl.certificate_numpy(Q, R1, s1, lam)
        scale = max(1.0, abs(cn["primal"]))
        assert cn["min_eig"] > -1e-7 * scale and abs(cn["gap"]) <= 1e-6 * scale and cn["stationarity"] < 1e-5, (name, cn)
        assert cn["primal"] == pytest.approx(i1["primal"], rel=1e-10, abs=1e-12), name


def test_profile_sampling_still_works(xmamd):
    """XM_FLAG_PROFILE_QW times the fp32 Hessian launches like the f64 ones"""
    Q = tl.gen_dense(200, seed=200)["Q"]
    _, _, info = xmamd.solve_dense(Q, 5, 1e-6, 0.0, tuning=dict(hess_f32=1), flags=xmamd.FLAG_PROFILE_QW)
    assert info["status"] == 1 and info["hess_f32"] == 1
    assert info["qw_ms_count"] >= 1 and info["qw_ms_sum"] > 0.0


def test_refused_where_not_covered(xmamd):
    """hess_f32 = 1 with block-CSR, view-graph or matrix-free storage, or with two virtual ranks: XM_ERR_ARG with a message, no GPU fault;
    the device is still usable afterwards"""
    V = tl.gen_vg(60, deg=4, sigma=0.1, seed=60)
    t = dict(hess_f32=1)
    with pytest.raises(xmamd.XmError, match="hess_f32"):
        xmamd.Context(bsr=(V["rowptr"], V["colidx"], V["blocks"]), tuning=t)
    with pytest.raises(xmamd.XmError, match="hess_f32"):
        e = V["edges"]
        xmamd.Context(vg=(e[:, 0].astype(np.int32), e[:, 1].astype(np.int32), V["w"], V["M"]), tuning=t)
    S = tl.gen_scene(40, 400, 5, seed=12)
    with pytest.raises(xmamd.XmError, match="hess_f32"):
        xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), tuning=t)
    with pytest.raises(xmamd.XmError, match="hess_f32"):
        xmamd.Context(Q=V["Q"], n_gpus=2, gpu_map=1, tuning=t)
    Qbad = tl.gen_dense(30, seed=30)["Q"]
    Qbad[3, 5] = Qbad[5, 3] = 1e300
    with pytest.raises(xmamd.XmError, match="not finite in fp32"):
        xmamd.Context(Q=Qbad, tuning=t)
    with pytest.raises(xmamd.XmError, match="hess_f32"):
        xmamd.Context(Q=V["Q"], tuning=dict(hess_f32=2))
    R, s, info = xmamd.solve_dense(tl.gen_dense(60, seed=60)["Q"], 5, 1e-6, 0.0, tuning=t)
    assert info["status"] == 1 and info["hess_f32"] == 1


def test_off_is_unchanged(xmamd):
    """hess_f32 = 0 in an otherwise non-zero tuning: R, s and the iteration counts bit-identical to a context with an all-zero tuning"""
    for Q in (tl.gen_dense(200, seed=200)["Q"], tl.gen_dense(1400, seed=1400)["Q"]):
        R0, s0, i0 = xmamd.solve_dense(Q, 5, 1e-6, 0.0, tuning=None)
        R1, s1, i1 = xmamd.solve_dense(Q, 5, 1e-6, 0.0, tuning=dict(hess_f32=0, lanczos_mmax=400))
        assert np.array_equal(R0, R1) and np.array_equal(s0, s1)
        # (not qw_products: the host-driven loop counts the run-ahead launches that became no-ops, which depends on timing)
        for k in ("rank", "status", "primal", "tcg_iters", "outer_iters", "lanczos_iters", "hess_f32", "qw_stream_bytes"):
            assert i0[k] == i1[k], k
