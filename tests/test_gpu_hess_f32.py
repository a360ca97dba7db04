"""GPU tests of the opt-in fp32 Hessian products (xm_tuning_t.hess_f32; run with -m gpu on an MI355X), through the C ABI of libxm_amd.so.

With the setting on, the Hessian products of the truncated CG read an fp32 copy of a dense Q (loaded as fp32, accumulated in f64); cost,
gradient, certificate and Lanczos stay on the f64 matrix.  The kernels must compute exactly the product with the ROUNDED matrix (to f64
round-off), the conversion must be numpy's astype(float32) bit for bit, a solve must reach the same certified optimum as the f64 solve,
contexts the setting does not cover must be refused cleanly, and with the setting off nothing may change."""
import ctypes as C
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
    k = min(5, 3 * n - 1)
    A[0, 1:1 + k] = [1e-40, -3e-39, 1e-46, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24][:k]   # subnormal, subnormal, below half the least subnormal, ties
    if 3 * n > 7:
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


# ---------------------------------------------------------------------------------------------- kernel edges (index arithmetic of the fp32 loops)
ALPHA = -0.75                                  # neither 1 nor -1: a dropped or doubled alpha shows


def _nonsymmetric(n, seed):
    """random 3n x 3n matrix that is NOT symmetric (the general kernel must use rows of Q, not columns), with the rounding edge cases of
    _symmetric in its first row"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((3 * n, 3 * n))
    A[0, : min(5, 3 * n)] = [1e-40, -3e-39, 1e-46, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24][: min(5, 3 * n)]
    if 3 * n > 2:
        A[2, 1] = -1.0e4
    return A


def _to_f32(xmamd, Q):
    """device fp32 copy of Q, checked bit for bit against astype(float32) (padding zero)"""
    n = Q.shape[0] // 3
    dq = xmamd.dense_upload(Q)
    try:
        d32 = xmamd.dense_to_f32(dq, n)
    finally:
        dq.free()
    got = d32.get(np.float32).reshape(3 * n, xmamd.dense_ld(n))
    assert np.array_equal(got[:, :3 * n].view(np.uint32), Q.astype(np.float32).view(np.uint32)), n
    assert not got[:, 3 * n:].any(), n
    return d32


def _run(xmamd, fn, d32, n, W, alpha=None):
    """fn(d32, n, o, W, out, alpha, stream) for a functional entry (alpha given), or the timing hook with reps = 1 (alpha None): 3 warm-up
    launches with rev = 0, 1, 0 and one timed launch with rev = 1, alpha 1 -- the output is the reversed-direction product"""
    o = W.shape[1]
    dW = xmamd.DevArray(xmamd.to_rm(W, rows=xmamd.dense_ld(n)))
    dO = xmamd.DevArray(np.full(3 * n * xmamd.pitch_of(o), np.nan))
    try:
        if alpha is None:
            ms = C.c_double()
            xmamd._chk(fn(d32.ptr, n, o, dW.ptr, dO.ptr, 1, C.byref(ms)))
        else:
            xmamd._chk(fn(d32.ptr, n, o, dW.ptr, dO.ptr, alpha, None))
        xmamd._chk(xmamd.lib().xm_dev_sync())
        return xmamd.from_rm(dO.get(), 3 * n, o)
    finally:
        dW.free(); dO.free()


def _rows_match(got, ref, what):
    """error per row against the largest reference entry; the worst row and its camera on failure"""
    err = np.abs(got - ref).max(axis=1) / np.abs(ref).max()
    assert np.all(np.isfinite(got)), f"{what}: non-finite output in row {int(np.argmax(~np.isfinite(got).all(axis=1)))}"
    r = int(err.argmax())
    assert err[r] < 1e-13, f"{what}: worst row {r} (camera {r // 3}): {err[r]:.2e}"


# dense_ld(n) mod 512 = 128 128 256 384 0 128 384 128 128: the last 512-column tile of the two-sub-tile form (o <= 5) is a quarter, a half,
# three quarters or whole; the single-sub-tile form (o >= 6, 256-column tiles) ends on a half or a whole tile
@pytest.mark.parametrize("n,os_", [(n, (1, 3, 4, 5, 6, 7, 8, 9, 10)) for n in (1, 2, 43, 86, 149, 171, 600, 700, 1031)] + [(1778, (3, 6, 10))])
def test_general_fp32_product_every_o_and_last_tile(xmamd, n, os_):
    """xm_qw_dense_f32 on a NON-symmetric Q, every rank the products are built for (o = 1, 3..10), left-to-right (functional entry,
    alpha = -0.75) and right-to-left (the timing hook's last launch), against numpy's product with the rounded matrix, row by row; o = 2,
    which no product is built for, is refused by both entries"""
    L = xmamd.lib()
    Q = _nonsymmetric(n, seed=1000 + n)
    Qr = Q.astype(np.float32).astype(np.float64)
    d32 = _to_f32(xmamd, Q)
    rng = np.random.default_rng(n)
    try:
        W2 = rng.standard_normal((3 * n, 2))
        for fn, alpha in ((L.xm_qw_dense_f32, ALPHA), (L.xm_qw_dense_f32_time, None)):
            with pytest.raises(xmamd.XmError, match="error -2: rank o must be 1 or 3..10, got 2"):
                _run(xmamd, fn, d32, n, W2, alpha)
        for o in os_:
            W = rng.standard_normal((3 * n, o))
            ref = Qr @ W
            _rows_match(_run(xmamd, L.xm_qw_dense_f32, d32, n, W, ALPHA), ALPHA * ref, f"n={n} o={o} forward")
            _rows_match(_run(xmamd, L.xm_qw_dense_f32_time, d32, n, W), ref, f"n={n} o={o} reversed")
    finally:
        d32.free()


def _symmetric_sweep_both_ways(xmamd, Q, n, o, seed):
    L = xmamd.lib()
    Qr = Q.astype(np.float32).astype(np.float64)
    d32 = _to_f32(xmamd, Q)
    try:
        W = np.random.default_rng(seed).standard_normal((3 * n, o))
        ref = Qr @ W
        _rows_match(_run(xmamd, L.xm_qw_dense_sym_f32, d32, n, W, ALPHA), ALPHA * ref, f"n={n} o={o} top-down")
        _rows_match(_run(xmamd, L.xm_qw_dense_sym_f32_time, d32, n, W), ref, f"n={n} o={o} bottom-up")
    finally:
        d32.free()


@pytest.mark.parametrize("n,o", [(1, 3), (2, 3), (7, 3), (8, 4), (9, 5), (43, 3), (85, 3), (86, 4), (87, 5), (128, 3), (149, 4), (171, 5), (700, 3), (1031, 5)])
def test_symmetric_fp32_sweep_half_strips_and_folds(xmamd, n, o):
    """xm_qw_dense_sym_f32 at the shapes of the f64 sweep's test (half strips, a half strip inside a fold of several strips, odd camera
    counts), top-down (functional entry) and bottom-up (the timing hook's last launch), row by row against the rounded matrix"""
    _symmetric_sweep_both_ways(xmamd, _symmetric(n, seed=7 * n + o), n, o, seed=n + o)


@pytest.mark.parametrize("n,o,k,kf", [(700, 3, 16, 4), (700, 4, 8, 2), (1031, 3, 12, 5), (1031, 5, 7, 3), (343, 4, 5, 1), (2200, 3, 9, 2)])
def test_symmetric_fp32_sweep_with_a_forced_finer_cut(xmamd, n, o, k, kf):
    """the finer cut of the grid rows dispatched last (xm_bench_symv_k) on the fp32 sweep, in both directions"""
    L = xmamd.lib()
    try:
        xmamd._chk(L.xm_bench_symv_k(k, 1, kf))
        p = (C.c_int32 * 4)(); xmamd._chk(L.xm_symv_plan(n, p))
        assert p[0] == k and p[1] == kf
        _symmetric_sweep_both_ways(xmamd, _symmetric(n, seed=11 * n + o), n, o, seed=n * o)
    finally:
        xmamd._chk(L.xm_bench_symv_k(0, 1, 0))


def test_cache_policy_never_changes_an_fp32_product(xmamd):
    """the non-temporal copies of the fp32 loops run only beyond ~310 MB: force every policy (xm_bench_dense_policy) -- all cacheable, all
    non-temporal, a cacheable prefix that cuts the stream in the middle -- and compare bit for bit with the default, in both directions.
    n = 700, ld = 2176.  General kernel: a camera's three rows are 3 * 2176 * 4 = 26 112 bytes, the copy 18.3 MB; a 4 096 KB prefix holds
    4 194 304 / 26 112 = 160 cameras (nt_cam0 = 160: workgroups 0..39 cacheable, 40..174 non-temporal).  Sweep: m = 2100 rows, triangle
    4 m (m + 6) / 2 = 8.85 MB; the prefix holds rows r = m - sqrt(m^2 - 2 * 4 194 304 / 4) = 579, so nt0 = 96 of 350 steps (chunks of K = 4
    steps: the 24 first cacheable, the rest non-temporal)."""
    L = xmamd.lib()
    n = 700
    Qs = _symmetric(n, seed=70)
    Qg = _nonsymmetric(n, seed=71)
    dg, ds = _to_f32(xmamd, Qg), _to_f32(xmamd, Qs)
    rng = np.random.default_rng(72)
    Ws = [rng.standard_normal((3 * n, o)) for o in (3, 5, 8)]
    def products():
        out = []
        for W in Ws:
            out.append(_run(xmamd, L.xm_qw_dense_f32, dg, n, W, ALPHA)); out.append(_run(xmamd, L.xm_qw_dense_f32_time, dg, n, W))
            if W.shape[1] <= 5:
                out.append(_run(xmamd, L.xm_qw_dense_sym_f32, ds, n, W, ALPHA)); out.append(_run(xmamd, L.xm_qw_dense_sym_f32_time, ds, n, W))
        return out
    try:
        ref = products()
        for pol in (0, 1, -4096):
            xmamd._chk(L.xm_bench_dense_policy(pol))
            for i, (a, b) in enumerate(zip(ref, products())):
                assert np.array_equal(a, b), (pol, i)
    finally:
        xmamd._chk(L.xm_bench_dense_policy(-1))
        dg.free(); ds.free()
    _rows_match(ref[0], ALPHA * (Qg.astype(np.float32).astype(np.float64) @ Ws[0]), "general, default policy")
    _rows_match(ref[3], Qs.astype(np.float32).astype(np.float64) @ Ws[0], "sweep, default policy")


# ---------------------------------------------------------------------------------------------- conversion edges
FLT_MAX = float(np.finfo(np.float32).max)
HALF_ULP = 2.0 ** 103                          # half the fp32 spacing at FLT_MAX (2^104): FLT_MAX + 2^103 is a tie, rounded to even = inf


def test_conversion_at_the_fp32_range_edges(xmamd):
    """-0.0 (sign kept), +-FLT_MAX and the largest f64 below the tie FLT_MAX + half an ulp are accepted and equal astype(float32) bit for
    bit; the tie itself (rounds to inf), +-inf and NaN are refused with XM_ERR_ARG; the message counts the bad entries exactly"""
    n = 20
    below_tie = float(np.nextafter(FLT_MAX + HALF_ULP, 0.0))
    with np.errstate(over="ignore"):
        assert np.float32(below_tie) == np.float32(FLT_MAX) and np.isinf(np.float32(FLT_MAX + HALF_ULP))
    Q = _symmetric(n, seed=3)
    Q[1, 2] = -0.0
    Q[5, 6], Q[7, 8], Q[9, 10], Q[11, 12] = FLT_MAX, -FLT_MAX, below_tie, -below_tie
    d32 = _to_f32(xmamd, Q)                    # (bit-for-bit check inside)
    got = d32.get(np.float32).reshape(3 * n, xmamd.dense_ld(n))
    d32.free()
    assert got[1, 2].view(np.uint32) == 0x80000000 and got[9, 10] == got[5, 6] == np.float32(FLT_MAX)
    for bad in (FLT_MAX + HALF_ULP, -(FLT_MAX + HALF_ULP), np.inf, -np.inf, np.nan):
        Qb = Q.copy()
        Qb[30, 4] = bad
        dq = xmamd.dense_upload(Qb)
        with pytest.raises(xmamd.XmError, match=rf"error -2: 1 entries of Q are not finite in fp32"):
            xmamd.dense_to_f32(dq, n)
        dq.free()
    # several bad entries in different rows, one of them in the last row: the kernel counts per element with an atomic
    m = 3 * 150
    Qb = _symmetric(150, seed=4)
    spots = [(0, 0), (17, m - 1), (m - 1, 3), (m // 2, m // 2 + 1), (m - 1, m - 1)]
    for (r, c), v in zip(spots, (np.inf, np.nan, -1e39, FLT_MAX + HALF_ULP, -np.inf)):
        Qb[r, c] = v
    dq = xmamd.dense_upload(Qb)
    with pytest.raises(xmamd.XmError, match=rf"error -2: {len(spots)} entries of Q are not finite in fp32"):
        xmamd.dense_to_f32(dq, 150)
    dq.free()


# ---------------------------------------------------------------------------------------------- solver level
def test_gradient_and_stop_test_stay_f64(xmamd):
    """only the tCG's Hessian products read the fp32 copy; cost, gradient and stop test stay on the f64 Q.  A solver whose
    gradient came from the fp32 copy would stop at a stationary point of the ROUNDED matrix, whose f64 cost differs from the optimum only at
    second order -- so the test measures stationarity against the f64 Q (numpy certificate, |S sR| / |Q sR|): the fp32 solve must be as
    stationary as the f64 solve of the same case (10x, + 1e-9), and -- the power check -- the f64 solution measured against the rounded
    matrix must miss that bound by 10x more, which is what a solver stopping on an fp32 gradient would show.
    gen_dense(1000) takes the general kernel (3n < 4096), gen_dense(1778) the symmetric pair; host-driven and device-driven outer loop (the
    EPI_AUTO launch that picks the matrix by its role).  tol = 1e-10: measured on an MI355X, every tol from 1e-10 down to 1e-13 certifies
    both cases with bit-identical results -- the solve ends when |r|^2 of a tCG falls below 1e-15 (|grad| ~ 2e-8), before any of these
    tolerances is met.  (gen_dense(200) is too small for the power check: its f64 solution misses the rounded matrix's stationarity by only
    ~70x of its own.)"""
    for n, sym in ((1000, 0), (1778, 1)):
        Q = tl.gen_dense(n, seed=n)["Q"]
        Qr = Q.astype(np.float32).astype(np.float64)
        for outer in ("host", "device"):
            what = f"gen_dense({n}) {outer}"
            flags = xmamd.FLAG_DEVICE_OUTER if outer == "device" else 0
            R0, s0, i0 = xmamd.solve_dense(Q, 5, 1e-10, 0.0, flags=flags)
            R1, s1, i1 = xmamd.solve_dense(Q, 5, 1e-10, 0.0, tuning=dict(hess_f32=1), flags=flags)
            assert i0["status"] == i1["status"] == 1 and i0["hess_f32"] == 0 and i1["hess_f32"] == 1, what
            assert i0["sym_product"] == i1["sym_product"] == sym, what
            if outer == "device":
                assert i0["outer_on_device"] >= 1 and i1["outer_on_device"] >= 1, what
            st0 = tl.certificate_numpy(Q, R0, s0, 0.0)["stationarity"]
            st1 = tl.certificate_numpy(Q, R1, s1, 0.0)["stationarity"]
            power = tl.certificate_numpy(Qr, R0, s0, 0.0)["stationarity"]
            bound = 10.0 * st0 + 1e-9
            assert st1 <= bound, f"{what}: fp32-Hessian solve stationarity {st1:.2e} > {bound:.2e} (f64 solve {st0:.2e})"
            assert power >= 10.0 * bound, f"{what}: the test cannot tell an fp32 gradient: {power:.2e} < 10 x {bound:.2e}"


def _reweighting_problem(n, seed):
    """view graph with planted outliers (tl.vg_measurements), Q(w0 = 1) and filtered weights w1: the reference's XM^2 filter
    (np.percentile(error, 90)) applied to the residuals of the planted rotations, so that no solve is needed to make them"""
    edges, M, bad, Rs = tl.vg_measurements(n, deg=20, sigma=0.02, seed=seed, outlier_frac=0.03)
    res = np.sum((Rs[edges[:, 0]] - M @ Rs[edges[:, 1]]) ** 2, axis=(1, 2))
    w1 = (res <= np.percentile(res, 90)).astype(float)
    assert bad[w1 == 0].mean() > 0.25 and w1[bad].sum() == 0
    Q0 = tl.bsr_to_dense(n, *tl.vg_assemble(n, edges, M, np.ones(edges.shape[0])))
    Q1 = tl.bsr_to_dense(n, *tl.vg_assemble(n, edges, M, w1))
    return edges, M, w1, Q0, Q1


def _read_back(ctx, n):
    """the context's f64 Q, exactly: the plain product (never the fp32 copy) with unit columns, 10 at a time"""
    m = 3 * n
    out = np.zeros((m, m))
    for j in range(0, m, 10):
        k = min(10, m - j)
        E = np.zeros((m, k)); E[j + np.arange(k), np.arange(k)] = 1.0
        out[:, j:j + k] = ctx.qw(E)
    return out


@pytest.mark.parametrize("hess", [1, 0])
@pytest.mark.parametrize("n,sym", [(600, 0), (1400, 1)])
def test_fp32_copy_follows_a_reweighting(xmamd, n, sym, hess):
    """XM^2 re-weighting rewrites the resident f64 Q (set_edge_weights) and must refresh the fp32 copy: a context built from Q(w0) and
    re-weighted to w1 before its first solve (A) must solve bit for bit like a context built from A's own Q read back (C) -- R, s, tCG and
    outer iterations, rank, cost.  With a stale copy A's tCG would run on fp32(Q(w0)) and land elsewhere in the last bits, though on the
    same optimum.  hess_f32 = 0 is the control that two contexts on the same Q solve bit-identically; n = 600 takes the general kernel,
    n = 1400 (3n >= 4096) the symmetric pair; host-driven and device-driven outer loop."""
    edges, M, w1, Q0, Q1 = _reweighting_problem(n, seed=77 + n)
    lam = 20.0
    tun = dict(hess_f32=hess)
    for outer in ("host", "device"):
        what = f"n={n} hess_f32={hess} {outer}"
        flags = xmamd.FLAG_DEVICE_OUTER if outer == "device" else 0
        A = xmamd.Context(Q=Q0, tuning=tun)
        try:
            A.attach_edges(edges[:, 0], edges[:, 1], M)
            A.set_edge_weights(w1)
            Ra, sa, ia = A.solve(5, 1e-8, lam, flags=flags)
            Qa = _read_back(A, n)
        finally:
            A.close()
        assert np.abs(Qa - Q1).max() <= 1e-14 * np.abs(Q1).max(), what
        Cc = xmamd.Context(Q=Qa, tuning=tun)
        try:
            Rc, sc, ic = Cc.solve(5, 1e-8, lam, flags=flags)
        finally:
            Cc.close()
        assert ia["status"] == ic["status"] == 1 and ia["hess_f32"] == ic["hess_f32"] == hess, what
        assert ia["sym_product"] == ic["sym_product"] == sym, what
        for k in ("tcg_iters", "outer_iters", "rank", "primal"):
            assert ia[k] == ic[k], (what, k, ia[k], ic[k])
        assert np.array_equal(Ra, Rc) and np.array_equal(sa, sc), what


def test_device_resident_q_gets_its_copy(xmamd):
    """a borrowed device Q (Context(dq=...)) gets its fp32 copy made on the device as well: bit-identical to a context built from the host
    Q, host-driven and device-driven"""
    n = 200
    Q = tl.gen_dense(n, seed=n)["Q"]
    t = dict(hess_f32=1)
    for flags in (0, xmamd.FLAG_DEVICE_OUTER):
        Rh, sh, ih = xmamd.solve_dense(Q, 5, 1e-8, 0.0, tuning=t, flags=flags)
        dq = xmamd.dense_upload(Q)
        try:
            ctx = xmamd.Context(dq=dq, n=n, tuning=t)
            try:
                Rd, sd, idv = ctx.solve(5, 1e-8, 0.0, flags=flags)
            finally:
                ctx.close()
        finally:
            dq.free()
        assert ih["hess_f32"] == idv["hess_f32"] == 1 and ih["status"] == idv["status"] == 1, flags
        for k in ("tcg_iters", "outer_iters", "rank", "primal", "qw_stream_bytes"):
            assert ih[k] == idv[k], (flags, k)
        assert np.array_equal(Rh, Rd) and np.array_equal(sh, sd), flags
