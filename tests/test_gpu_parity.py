"""GPU parity tests (run with -m gpu on an MI355X): every call goes through the C ABI of libxm_amd.so and is checked
against the CPU oracle on the same seeded inputs, against the golden fixtures, and through size-independent invariants."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import xm_testlib as tl

pytestmark = pytest.mark.gpu
G = tl.GOLDEN


def _case(name):
    d = os.path.join(G, name)
    return tl.load_bin(os.path.join(d, "Q.bin")), json.load(open(os.path.join(d, "expected.json"))), d


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n,o", [(1, 3), (5, 3), (43, 3), (149, 3), (171, 4), (60, 5), (33, 7), (90, 10), (700, 3), (211, 1)])
def test_qw_dense_matches_oracle(xmamd, oracle, n, o):
    rng = np.random.default_rng(100 * n + o)
    Q = rng.standard_normal((3 * n, 3 * n))          # deliberately NOT symmetric: rows of C must be used like cublasDgemm
    W = rng.standard_normal((3 * n, o))
    ref = oracle.qw(Q, W, 2.0)
    got = xmamd.qw_dense(Q, W, 2.0)
    assert tl.rel_fro(got, ref) < 1e-13


@pytest.mark.parametrize("n,deg,o", [(1, 2, 3), (7, 3, 3), (200, 8, 3), (300, 20, 5), (150, 40, 10), (1000, 12, 4)])
def test_qw_bsr3_matches_dense(xmamd, oracle, n, deg, o):
    P = tl.gen_vg(n, deg=deg, sigma=0.3, seed=n + o)
    W = np.random.default_rng(n).standard_normal((3 * n, o))
    ref = oracle.qw(P["Q"], W, 1.0)
    got = xmamd.qw_bsr3(P["rowptr"], P["colidx"], P["blocks"], W, 1.0)
    assert tl.rel_fro(got, ref) < 1e-13


def _banded(n, half, seed):
    lo = np.maximum(np.arange(n) - half, 0); hi = np.minimum(np.arange(n) + half, n - 1)
    cnt = hi - lo + 1
    rowptr = np.zeros(n + 1, dtype=np.int64); rowptr[1:] = np.cumsum(cnt)
    colidx = (np.repeat(lo, cnt) + (np.arange(rowptr[-1]) - np.repeat(rowptr[:-1], cnt))).astype(np.int32)
    return rowptr, colidx, np.random.default_rng(seed).standard_normal((int(rowptr[-1]), 3, 3))


@pytest.mark.parametrize("o", [3, 4, 5, 6, 7, 10])
def test_qw_bsr3_banded(xmamd, o):
    """view graph with locality (camera i sees i-20 .. i+20): equal row lengths of 41 blocks = two full windows and a partial one
    (o <= 6: blocks and gathered records through LDS; o >= 7: blocks only -- the two compiled forms of the kernel)"""
    n = 1500
    rowptr, colidx, blocks = _banded(n, 20, o)
    W = np.random.default_rng(o).standard_normal((3 * n, o))
    ref = tl.bsr_to_dense(n, rowptr, colidx, blocks) @ W
    got = xmamd.qw_bsr3(rowptr, colidx, blocks, W, 1.0)
    assert tl.rel_fro(got, ref) < 1e-13


@pytest.mark.parametrize("o", [3, 5, 7])
def test_qw_bsr3_rows_ordered_by_window_count(xmamd, o):
    """inside a solve the block-CSR kernel takes the 16 rows of a workgroup in the order of their number of 16-block windows (one 16-byte
    row record instead of two row pointers; a wavefront's four rows then have similar lengths).  Same product bit for bit as in camera order:
    a row's sum does not depend on which lane group computes it.  Ragged rows incl. empty ones and a last workgroup that is not full"""
    import ctypes as C
    rng = np.random.default_rng(40 + o)
    n = 16 * 23 + 5
    cnt = rng.integers(0, 70, n); cnt[rng.integers(0, n, 25)] = 0
    rowptr = np.zeros(n + 1, dtype=np.int64); rowptr[1:] = np.cumsum(cnt)
    colidx = np.concatenate([np.sort(rng.choice(n, c, replace=False)) for c in cnt] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    blocks = rng.standard_normal((int(rowptr[-1]), 3, 3))
    W = rng.standard_normal((3 * n, o))
    ref = tl.bsr_to_dense(n, rowptr, colidx, blocks) @ W
    L = xmamd.lib()
    drp = xmamd.DevArray(rowptr); dci = xmamd.DevArray(colidx); dbl = xmamd.DevArray(blocks.reshape(-1))
    dW = xmamd.DevArray(xmamd.to_rm(W))
    outs = []
    for binned in (1, 0):
        dO = xmamd.DevArray(np.full(3 * n * xmamd.pitch_of(o), np.nan)); ms = C.c_double()
        xmamd._chk(L.xm_bench_bsr_binned(binned))
        xmamd._chk(L.xm_qw_bsr3_time(drp.ptr, dci.ptr, dbl.ptr, n, o, dW.ptr, dO.ptr, 1, C.byref(ms)))
        outs.append(xmamd.from_rm(dO.get(), 3 * n, o)); dO.free()
    xmamd._chk(L.xm_bench_bsr_binned(1))
    for b in (drp, dci, dbl, dW): b.free()
    assert np.array_equal(outs[0], outs[1])
    assert tl.rel_fro(outs[0], ref) < 1e-13


def test_qw_empty_rows_bsr(xmamd):
    # ragged: cameras without any stored block
    n = 9
    rowptr = np.array([0, 0, 2, 2, 2, 3, 3, 3, 3, 3], dtype=np.int64)
    colidx = np.array([0, 8, 4], dtype=np.int32)
    blocks = np.random.default_rng(3).standard_normal((3, 3, 3))
    W = np.random.default_rng(4).standard_normal((3 * n, 3))
    ref = tl.bsr_to_dense(n, rowptr, colidx, blocks) @ W
    assert np.allclose(xmamd.qw_bsr3(rowptr, colidx, blocks, W), ref, atol=1e-13)


@pytest.mark.parametrize("o", [3, 4, 6, 10])
def test_retraction_matches_oracle(xmamd, oracle, o):
    rng = np.random.default_rng(o)
    n = 77
    R = oracle.mgs_rows(rng.standard_normal((3 * n, o)))
    D = 0.3 * rng.standard_normal((3 * n, o)); s = rng.uniform(0.5, 2.0, n); s[0] = 1.0
    ds = rng.standard_normal(n)
    Rn, sn = xmamd.retract(R, s, D, ds, 0.7)
    assert np.allclose(Rn, oracle.mgs_rows(R + 0.7 * D), atol=1e-13)
    exp = s * np.exp(0.7 * ds / s); exp[0] = 1.0      # the anchor's scale never moves
    assert np.allclose(sn, exp, rtol=1e-14)
    assert tl.stiefel_defect(Rn) < 1e-13


@pytest.mark.parametrize("o", [3, 4, 5, 10])
def test_retraction_quad_per_camera_matches_oracle(xmamd, oracle, o):
    """the measured alternative of the MGS-QR retraction (a quad of lanes per camera, DPP reductions -- `north_star`'s cross-lane form;
    scripts/kbench_retract.py records why the thread-per-camera kernel stays the default): same result as the oracle's Gram-Schmidt"""
    rng = np.random.default_rng(o)
    n = 131                                                                  # not a multiple of 64: a partly filled workgroup
    R = oracle.mgs_rows(rng.standard_normal((3 * n, o)))
    D = 0.3 * rng.standard_normal((3 * n, o)); s = rng.uniform(0.5, 2.0, n); s[0] = 1.0
    ds = rng.standard_normal(n)
    dR = xmamd.DevArray(xmamd.to_rm(R)); dD = xmamd.DevArray(xmamd.to_rm(D)); dsv = xmamd.DevArray(s); dds = xmamd.DevArray(ds)
    dRo = xmamd.DevArray(nbytes=dR.nbytes); dso = xmamd.DevArray(nbytes=dsv.nbytes)
    xmamd._chk(xmamd.lib().xm_retract_variant(n, o, dR.ptr, dsv.ptr, dD.ptr, dds.ptr, 0.7, dRo.ptr, dso.ptr, 2, 1, None))
    Rn, sn = xmamd.from_rm(dRo.get(), 3 * n, o), dso.get()
    for b in (dR, dD, dsv, dds, dRo, dso):
        b.free()
    assert np.allclose(Rn, oracle.mgs_rows(R + 0.7 * D), atol=1e-13)
    exp = s * np.exp(0.7 * ds / s); exp[0] = 1.0
    assert np.allclose(sn, exp, rtol=1e-14) and tl.stiefel_defect(Rn) < 1e-13


# ---------------------------------------------------------------------------------------------- sliced-ELL product (xm_sell.hip)
@pytest.mark.parametrize("n,deg,o,slabs,lmax", [(1, 2, 3, 4, 64), (7, 3, 3, 8, 64), (200, 8, 3, 4, 64), (300, 20, 5, 2, 64), (1000, 12, 4, 8, 5),
                                                (150, 40, 3, 1, 64), (211, 9, 1, 4, 64), (4000, 30, 3, 4, 64)])
@pytest.mark.parametrize("gather", [0, 1])    # 0: a record of W per lane | 1: records fetched element-per-lane and transposed through LDS
def test_qw_sell_matches_dense(xmamd, oracle, n, deg, o, slabs, lmax, gather):
    """same product as test_qw_bsr3_matches_dense through the large-n layout (sorted virtual rows, two launches): every slab count, both
    gather modes, virtual rows / slices cut at lmax, odd and even slice widths (paired steps + unpaired last step)"""
    if o == 1 and gather >= 1:
        pytest.skip("o = 1 has one gather mode")
    P = tl.gen_vg(n, deg=deg, sigma=0.3, seed=n + o)
    W = np.random.default_rng(n).standard_normal((3 * n, o))
    ref = oracle.qw(P["Q"], W, 1.5)
    M = xmamd.SellMatrix(P["rowptr"], P["colidx"], P["blocks"], slabs=slabs, lmax=lmax)
    got = M.qw(W, 1.5, gather=gather)
    again = M.qw(W, 1.5, gather=gather)
    padded = M.qw(W, 1.5, gather=gather, padded=True) if o >= 3 else got   # input also at the 128-byte record pitch
    M.close()
    assert tl.rel_fro(got, ref) < 1e-13 and np.array_equal(got, again) and tl.rel_fro(padded, ref) < 1e-13


def test_stream_cache_policy_never_changes_a_result(xmamd):
    """the matrix streams pick their cache policy by size (default below the Infinity Cache, non-temporal beyond, a cacheable prefix in
    between); in the sliced-ELL and block-CSR kernels the two policies are two compiled copies of the loop under a uniform branch.  The test
    matrices are small, so the rule never reaches the non-temporal copies: force every policy (xm_bench_dense_policy) -- all cacheable, all
    non-temporal, a prefix that cuts the stream in the middle -- and compare bit for bit with the default.  Sliced ELL with full blocks and
    with the quaternion codec, block CSR, dense (general kernel with a resident prefix), and the f64 symmetric sweep in both directions (a
    prefix of whole steps from the top of the upper triangle)"""
    import ctypes as C
    L = xmamd.lib()
    P = tl.gen_vg(3000, deg=24, sigma=0.3, seed=31)
    W = np.random.default_rng(31).standard_normal((3 * 3000, 3))
    D = tl.gen_dense(300, seed=7)
    Wd = np.random.default_rng(8).standard_normal((900, 3))
    def products():
        out = []
        for codec in (0, 1):
            M = xmamd.SellMatrix(P["rowptr"], P["colidx"], P["blocks"], slabs=4, codec=codec)
            out.append(M.qw(W, 1.0, gather=1)); out.append(M.qw(W, 1.0, gather=0)); M.close()
        # block CSR through the timing hook: it knows the block count, as a solve does (the plain entry point does not and stays cacheable)
        drp = xmamd.DevArray(P["rowptr"]); dci = xmamd.DevArray(P["colidx"]); dbl = xmamd.DevArray(P["blocks"].reshape(-1))
        dW = xmamd.DevArray(xmamd.to_rm(W)); dO = xmamd.DevArray(np.full(3 * 3000 * 3, np.nan)); ms = C.c_double()
        xmamd._chk(L.xm_qw_bsr3_time(drp.ptr, dci.ptr, dbl.ptr, 3000, 3, dW.ptr, dO.ptr, 1, C.byref(ms)))
        out.append(xmamd.from_rm(dO.get(), 9000, 3))
        for b in (drp, dci, dbl, dW, dO): b.free()
        out.append(xmamd.qw_dense(D["Q"], Wd, 1.0))
        # the symmetric sweep: top-down (functional entry) and bottom-up (the timing hook's last launch: warm-ups rev 0 1 0, timed rev 1)
        out.append(xmamd.qw_dense(D["Q"], Wd, 1.0, dq=dD, sym=True))
        dW = xmamd.DevArray(xmamd.to_rm(Wd, rows=xmamd.dense_ld(300))); dO = xmamd.DevArray(np.full(900 * 3, np.nan))
        xmamd._chk(L.xm_qw_dense_sym_time(dD.ptr, 300, 3, dW.ptr, dO.ptr, 1, C.byref(ms)))
        out.append(xmamd.from_rm(dO.get(), 900, 3))
        dW.free(); dO.free()
        return out
    dD = xmamd.dense_upload(D["Q"])
    try:
        ref = products()
        # the sliced-ELL streams are ~9 MB / ~5 MB, the dense matrix 9 MB (general kernel: 24 KB per camera, prefixes of 42 / 125 of 300
        # cameras).  The f64 sweep streams the triangle 8 m (m + 6) / 2 = 3.26 MB (m = 900 rows); a prefix of P bytes holds its rows
        # r = m - sqrt(m^2 - 2 P / 8): 160 rows (1 024 KB) and 695 rows (3 000 KB), so the first non-temporal step is 26 and 115 of 150
        # (chunks of K = 4 steps: both policies run in one launch)
        for pol in (0, 1, -1024, -3000):
            xmamd._chk(L.xm_bench_dense_policy(pol))
            got = products()
            for i, (a, b) in enumerate(zip(ref, got)):
                assert np.array_equal(a, b), (pol, i)
    finally:
        xmamd._chk(L.xm_bench_dense_policy(-1))
        dD.free()
    assert tl.rel_fro(ref[0], tl.bsr_to_dense(3000, P["rowptr"], P["colidx"], P["blocks"]) @ W) < 1e-13
    Dw = D["Q"] @ Wd
    assert tl.rel_fro(ref[-3], Dw) < 1e-13 and tl.rel_fro(ref[-2], Dw) < 1e-13 and tl.rel_fro(ref[-1], Dw) < 1e-13


def test_qw_sell_skewed_degrees_and_unsorted_rows(xmamd):
    """hub cameras (rows of ~n/4 blocks among rows of ~20: cut into virtual rows of <= lmax blocks, partial results added per camera),
    cameras without blocks, rows handed over in arbitrary column order; the block-CSR kernel runs the same skewed matrix"""
    n = 6000
    P = tl.gen_skewed(n, 20, seed=7)
    rowptr, colidx, blocks = P["rowptr"], P["colidx"].copy(), P["blocks"].copy()
    assert np.diff(rowptr).max() > 50 * np.median(np.diff(rowptr))
    rng = np.random.default_rng(1)
    for r in rng.choice(n, size=300, replace=False):            # shuffle the column order inside some rows
        a, e = rowptr[r], rowptr[r + 1]
        perm = rng.permutation(e - a)
        colidx[a:e] = colidx[a:e][perm]; blocks[a:e] = blocks[a:e][perm]
    W = rng.standard_normal((3 * n, 3))
    ref = np.zeros((3 * n, 3))
    Wc = W.reshape(n, 3, 3)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    np.add.at(ref.reshape(n, 3, 3), rows, blocks @ Wc[colidx])
    for slabs, lmax in [(4, 64), (8, 16), (1, 1000)]:
        M = xmamd.SellMatrix(rowptr, colidx, blocks, slabs=slabs, lmax=lmax)
        assert tl.rel_fro(M.qw(W, gather=0), ref) < 1e-13
        assert tl.rel_fro(M.qw(W, gather=1), ref) < 1e-13
        M.close()
    assert tl.rel_fro(xmamd.qw_bsr3(rowptr, colidx, blocks, W), ref) < 1e-13


def test_qw_sell_wide_matrix_against_csr_arithmetic(xmamd):
    """70 000 cameras (too wide for a dense reference) in one slab and in four, full blocks and view-graph codec, every gather mode and the
    padded product input, against the product computed from the CSR arrays with numpy"""
    n = 70000
    P = tl.gen_vg(n, deg=4, sigma=0.2, seed=2, dense=False)
    rng = np.random.default_rng(4)
    W = rng.standard_normal((3 * n, 3))
    ref = np.zeros((3 * n, 3))
    rows = np.repeat(np.arange(n), np.diff(P["rowptr"]))
    np.add.at(ref.reshape(n, 3, 3), rows, P["blocks"] @ W.reshape(n, 3, 3)[P["colidx"]])
    for slabs in (1, 4):
        for codec in (0, 1):
            M = xmamd.SellMatrix(P["rowptr"], P["colidx"], P["blocks"], slabs=slabs, codec=codec)
            for gather in (0, 1):
                assert tl.rel_fro(M.qw(W, gather=gather), ref) < 1e-12, (slabs, codec, gather)
            assert tl.rel_fro(M.qw(W, gather=1, padded=True), ref) < 1e-12
            M.close()


def test_solve_through_sell_equals_csr_path(xmamd):
    """the whole solver (gradient / Hessian / certificate epilogues, Lanczos with o = 1) on the sliced-ELL product reaches the
    optimum of the block-CSR path: same rank, status, primal to 1e-12, rotations to 1e-8"""
    P = tl.gen_vg(700, deg=10, sigma=0.3, seed=11, dense=False)
    res = {}
    for key, tn in (("csr", dict(sell=-1)), ("sell", dict(sell=1)), ("sell_g0", dict(sell=1, sell_gather=1))):   # block-CSR kernel | sliced ELL | sliced ELL, a record per lane
        ctx = xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]), tuning=tn)          # xm_tuning_t fields, not the environment
        assert ctx.product_kind(3) == ("bsr3" if key == "csr" else "sell")
        res[key] = ctx.solve(5, 1e-9, 20.0)
        ctx.close()
    R0, s0, i0 = res["csr"]
    for key in ("sell", "sell_g0"):
        R1, s1, i1 = res[key]
        assert i0["rank"] == i1["rank"] and i0["status"] == i1["status"] == 1
        assert i1["primal"] == pytest.approx(i0["primal"], rel=1e-12)
        assert i1["min_eig"] == pytest.approx(i0["min_eig"], abs=1e-7)
        assert tl.rotation_parity(R1, s1, R0, s0) < 1e-8


@pytest.mark.parametrize("storage", ["bsr", "vg"])
def test_padded_product_input_of_the_tcg_changes_nothing(xmamd, storage):
    """xm_tuning_t.sell_wpad: inside the truncated CG the kernels that write the product input (tcg_init, cg_step) also write it at a
    record pitch of 128 bytes and the sliced-ELL gather reads that copy -- same numbers in the same order, so the whole solve (staircase
    3 -> 4 -> 5: records of 9 and of 15 doubles) is bit-identical with and without it"""
    P = tl.gen_vg(900, deg=12, sigma=0.6, seed=5, dense=False)
    out = {}
    for wpad in (1, -1):
        tn = dict(sell=1, sell_wpad=wpad)
        if storage == "vg":      # view-graph storage: quaternion codec
            e = P["edges"]
            ctx = xmamd.Context(vg=(e[:, 0].astype(np.int32), e[:, 1].astype(np.int32), np.ones(e.shape[0]), P["M"]), n=900, tuning=tn)
        else:
            ctx = xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]), tuning=tn)
        out[wpad] = ctx.solve(5, 1e-9, 30.0)
        ctx.close()
    (R1, s1, i1), (R0, s0, i0) = out[1], out[-1]
    assert i1["rank"] == i0["rank"] and i1["status"] == i0["status"] and i1["tcg_iters"] == i0["tcg_iters"] > 0
    assert i1["primal"] == i0["primal"] and np.array_equal(R1, R0) and np.array_equal(s1, s0)


# ---------------------------------------------------------------------------------------------- whole solves
def _check_against_golden(R, s, info, exp, d, tol_rot=1e-6):
    assert info["rank"] == exp["rank"] and info["status"] == exp["status"]
    assert info["primal"] == pytest.approx(exp["f_star"], rel=1e-9, abs=1e-12)
    assert tl.stiefel_defect(R) < 1e-12 and s[0] == 1.0
    rot, _ = tl.recover_rotations(R, s)
    assert tl.rel_fro(rot, np.load(os.path.join(d, "rot_anchor.npy"))) < tol_rot       # north_star: <= 1e-6
    sR = tl.scale_rows(R, s)
    idx = tl.gram_sample_index(sR.shape[0])
    X = (sR[idx[:, 0]] * sR[idx[:, 1]]).sum(axis=1)
    assert tl.rel_fro(X, np.load(os.path.join(d, "sR_gram_sample.npy"))) < tol_rot


@pytest.mark.parametrize("name", ["simple1", "simple2", "synth/dense49", "synth/vg60_cert"])
def test_solve_matches_golden_rank3(xmamd, name):
    Q, exp, d = _case(name)
    R, s, info = xmamd.solve_dense(Q, exp["max_rank"], exp["tol"], exp["lam"], trace=1000)
    _check_against_golden(R, s, info, exp, d)
    assert info["min_eig"] == pytest.approx(exp["cert"]["min_eig"], abs=1e-7)
    assert info["dual"] == pytest.approx(exp["cert"]["dual"], rel=1e-6)
    # early iterates agree with the oracle's trajectory (loss, gradnorm, inner count, exit reason)
    head = np.array(exp["trace_head"])
    got = info["trace"][: head.shape[0]]
    assert np.allclose(got[:, 0], head[:, 0], rtol=1e-9) and np.allclose(got[:, 1], head[:, 1], rtol=1e-7)
    assert np.array_equal(got[:, 2:5], head[:, 2:5])
    # iteration counts are within a few of the oracle's (trajectories agree until round-off decides the last steps)
    assert abs(info["outer_iters"] - exp["outer_iters"]) <= 2
    assert abs(info["tcg_iters"] - exp["tcg_iters"]) <= 0.05 * exp["tcg_iters"] + 10


@pytest.mark.parametrize("name", ["simple1", "simple2", "synth/dense49", "synth/vg60_cert", "synth/vg40_stair"])
def test_gpu_solution_certified_by_numpy(xmamd, name):
    """the GPU's own output on the golden inputs is certified from scratch with numpy/LAPACK (tl.certificate_numpy): dual
    feasibility lambda_min(S) >= -eps by eigvalsh, stationarity S sR = 0, zero duality gap -- independent of oracle and Lanczos"""
    Q, exp, d = _case(name)
    R, s, info = xmamd.solve_dense(Q, exp["max_rank"], exp["tol"], exp["lam"])
    assert info["status"] == 1
    cn = tl.certificate_numpy(Q, R, s, exp["lam"])
    scale = max(1.0, abs(cn["primal"]))
    assert cn["min_eig"] > -1e-7 * scale and abs(cn["gap"]) <= 1e-6 * scale and cn["stationarity"] < 1e-5
    assert cn["primal"] == pytest.approx(info["primal"], rel=1e-10, abs=1e-12)
    assert info["min_eig"] == pytest.approx(cn["min_eig"], abs=1e-7 * scale) and info["dual"] == pytest.approx(cn["dual"], rel=1e-6)
    # small problems (3n <= 384 rows) take the dense route: the tridiagonalisation runs to completion, min_eig is an eigenvalue of S
    # to round-off (the reference: cusolverDnDsyevd on S, Dense/eig.h:35-73); larger ones stop at a converged Ritz pair
    exact = 3 * exp["n"] <= 384
    assert info["cert_flags"] == (2 if exact else 0) and info["eig_residual"] <= 1e-6 * max(1.0, np.abs(cn["eigs"]).max())
    if exact:
        assert info["min_eig"] == pytest.approx(cn["min_eig"], abs=1e-11 * max(1.0, np.abs(cn["eigs"]).max()))
        assert info["eig_residual"] <= 1e-11 * max(1.0, np.abs(cn["eigs"]).max())


def test_unconverged_lanczos_never_certifies(xmamd):
    """A Ritz value is an upper bound of lambda_min: when Lanczos is cut short (here: 4 steps, one restart -- xm_tuning_t.lanczos_mmax /
    lanczos_restarts) the certificate must not be accepted on it and the result must say so (xm_result_t.cert_flags) -- the same instance
    certifies at rank 3 otherwise"""
    Q, exp, d = _case("synth/vg60_cert")
    R, s, out = xmamd.solve_dense(Q, 3, exp["tol"], exp["lam"], tuning=dict(lanczos_mmax=4, lanczos_restarts=1))
    assert out["cert_flags"] & xmamd.CERT_EIG_NOT_CONVERGED and out["status"] != 1 and out["eig_residual"] > 1e-6
    R, s, info = xmamd.solve_dense(Q, 3, exp["tol"], exp["lam"])
    assert info["status"] == 1 and not (info["cert_flags"] & xmamd.CERT_EIG_NOT_CONVERGED)


def test_lost_result_kernel_raises_instead_of_hanging(xmamd):
    """host spin loops: when the kernel that publishes an outer iteration's results never runs (injected: xm_tuning_t.debug_drop_finalize,
    what a failed launch or a device fault amounts to) the solve must return XM_ERR_HIP within the poll interval, not spin for ever"""
    import time
    Q, exp, d = _case("synth/dense49")
    t0 = time.time()
    with pytest.raises(xmamd.XmError) as ei:
        xmamd.solve_dense(Q, 3, 1e-9, 0.0, tuning=dict(debug_drop_finalize=4))
    assert "-3" in str(ei.value) and "did not reach host-mapped memory" in str(ei.value)
    assert time.time() - t0 < 60
    R, s, info = xmamd.solve_dense(Q, 3, 1e-9, 0.0)       # the process and the device are fine afterwards
    assert info["rank"] == 3


def test_staircase_matches_oracle(xmamd, oracle):
    """rank escalation 3 -> 6 with saddle escape along the certificate's eigenvector (XM_main.cu:223-277)"""
    Q, exp, d = _case("synth/vg40_stair")
    R, s, info = xmamd.solve_dense(Q, exp["max_rank"], exp["tol"], exp["lam"], trace=4000)
    assert info["rank"] == exp["rank"] and info["status"] == 1
    assert info["primal"] == pytest.approx(exp["f_star"], rel=1e-8)
    # the certified optimum X = sR sR^T is unique -> gauge-invariant comparison with the oracle
    Ro, so, io = oracle.solve(Q, exp["max_rank"], exp["tol"], exp["lam"], 1000.0)
    assert tl.rel_fro(tl.gram(R, s), tl.gram(Ro, so)) < 1e-6
    assert tl.rotation_parity(R, s, Ro, so) < 1e-6
    # rank-3-only run stops at the saddle, like the oracle
    R3, s3, i3 = xmamd.solve_dense(Q, 3, exp["tol"], exp["lam"])
    assert i3["status"] == 2 and i3["min_eig"] < -1e-3


def test_modes_rank3_and_rebuttle(xmamd, oracle):
    Q, exp, d = _case("synth/dense49")
    R, s, info = xmamd.solve_dense(Q, 7, 1e-3, 0.0, mode=xmamd.MODE_RANK3)
    Ro, so, io = oracle.solve(Q, 7, 1e-3, 0.0, 1000.0, mode=1)
    assert info["rank"] == 3 and tl.rel_fro(tl.gram(R, s), tl.gram(Ro, so)) < 1e-8
    s_ini = np.linspace(0.9, 1.1, 49); s_ini[0] = 1.0
    R2, s2, i2 = xmamd.solve_dense(Q, 5, 1e-12, 0.0, mode=xmamd.MODE_REBUTTLE, s_ini=s_ini)
    Ro2, so2, io2 = oracle.solve(Q, 5, 1e-12, 0.0, 1000.0, mode=2, s_ini=s_ini)
    assert i2["status"] == io2["status"] == 1
    assert tl.rotation_parity(R2, s2, Ro2, so2) < 1e-6


def test_host_stepped_equals_run_ahead(xmamd):
    """the enqueue-ahead tCG must give bit-identical results to the fully synchronised debug mode"""
    Q, exp, d = _case("simple2")
    a = xmamd.solve_dense(Q, 3, 1e-16, 0.0, trace=100, flags=xmamd.FLAG_HOST_OUTER)
    b = xmamd.solve_dense(Q, 3, 1e-16, 0.0, trace=100, flags=xmamd.FLAG_HOST_STEPPED)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2]["trace"], b[2]["trace"])
    # the default for dense products is the host-driven form: the same bits as with the flag
    d0 = xmamd.solve_dense(Q, 3, 1e-16, 0.0, trace=100)
    assert d0[2]["outer_on_device"] == 0 and np.array_equal(a[0], d0[0]) and np.array_equal(a[2]["trace"], d0[2]["trace"])
    # outer iteration on the device (XM_FLAG_DEVICE_OUTER, tests/test_gpu_device_outer.py): it walks the column tiles of the dense product in a
    # direction that alternates by launch pair instead of by tCG iteration: same optimum, last bits of the path differ
    c = xmamd.solve_dense(Q, 3, 1e-16, 0.0, trace=100, flags=xmamd.FLAG_DEVICE_OUTER)
    assert c[2]["outer_on_device"] == 1 and c[2]["primal"] == pytest.approx(a[2]["primal"], rel=1e-12) and tl.rotation_parity(c[0], c[1], a[0], a[1]) < 1e-7


def test_bsr_solve_equals_dense_solve(xmamd):
    P = tl.gen_vg(300, deg=10, sigma=0.1, seed=5)
    Rd, sd, idn = xmamd.solve_dense(P["Q"], 5, 1e-10, 10.0)
    ctx = xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]))
    Rb, sb, ib = ctx.solve(5, 1e-10, 10.0)
    ctx.close()
    assert idn["status"] == ib["status"] == 1 and idn["rank"] == ib["rank"]
    assert ib["primal"] == pytest.approx(idn["primal"], rel=1e-10)
    assert tl.rotation_parity(Rb, sb, Rd, sd) < 1e-7
    # planted rotations are recovered up to the noise level
    rot, _ = tl.recover_rotations(Rb, sb)
    Rs = P["R_star"]
    ref = np.concatenate([Rs[0] @ Rs[i].T for i in range(300)], axis=1)
    assert tl.rel_fro(rot, ref) < 0.2


def test_file_surface_XM_module(xmamd, tmp_path, monkeypatch):
    """the reference's own entry point: XM.solve(path, ...) reading Q.bin, writing R.bin / s.bin (1_test_solve.py:42)"""
    Q, exp, d = _case("simple1")
    tl.save_bin(tmp_path / "Q.bin", Q)
    monkeypatch.setenv("XM_QUIET", "1")
    XM = xmamd.import_XM()
    assert XM.solve(str(tmp_path) + "/", 3, 1e-16, 0.0, 1000) is None
    R = tl.load_bin(tmp_path / "R.bin"); s = tl.load_bin(tmp_path / "s.bin")
    assert R.shape == (447, 3) and s.shape == (149, 1) and s[0, 0] == 1.0
    raw = open(tmp_path / "s.bin", "rb").read()
    assert raw[:8] == np.array([149, 1], dtype="<i4").tobytes() and len(raw) == 8 + 8 * 149
    rot, _ = tl.recover_rotations(R, s)
    assert tl.rel_fro(rot, np.load(os.path.join(d, "rot_anchor.npy"))) < 1e-6
    assert XM.solve_rebuttle is not None
    tl.save_bin(tmp_path / "R_ini.bin", R); tl.save_bin(tmp_path / "s_ini.bin", s)
    assert XM.solve_rebuttle(str(tmp_path), 3, 1e-10, 0.0, 1000) == 1
    XM.solve_rank3(str(tmp_path), 3, 1e-3, 0.0, 1000)
    assert tl.load_bin(tmp_path / "R.bin").shape == (447, 3)
    with pytest.raises(RuntimeError):
        XM.solve(str(tmp_path / "missing"), 3, 1e-6, 0.0, 10)


def test_in_memory_XM_surface_and_bin_v2(xmamd, tmp_path, monkeypatch):
    """XM.solve_array / XM.solve_bsr return what the file surface writes (bit for bit), and Q.bin with the
    8-byte header fields of utils/io.py:24-26 (`byte = 8`, which the reference's own C++ loader cannot read) is accepted"""
    Q, exp, d = _case("simple2")
    monkeypatch.setenv("XM_QUIET", "1")
    XM = xmamd.import_XM()
    R, s, info = XM.solve_array(Q, 3, 1e-12, 0.0, 1000.0)
    assert R.shape == (3 * exp["n"], info["rank"]) and R.flags.f_contiguous and s.shape == (exp["n"],) and info["status"] == 1
    tl.save_bin(tmp_path / "Q.bin", Q)
    XM.solve(str(tmp_path), 3, 1e-12, 0.0, 1000.0)
    R1 = tl.load_bin(tmp_path / "R.bin"); s1 = tl.load_bin(tmp_path / "s.bin")
    assert np.array_equal(R, R1) and np.array_equal(s, s1[:, 0])
    with open(tmp_path / "Q.bin", "wb") as f:                     # the same Q with int64 header fields
        f.write(np.array(Q.shape, dtype="<i8").tobytes()); Q.T.tofile(f)
    os.remove(tmp_path / "R.bin")
    XM.solve(str(tmp_path), 3, 1e-12, 0.0, 1000.0)
    assert np.array_equal(tl.load_bin(tmp_path / "R.bin"), R1)
    tl.save_bin(tmp_path / "Q.bin", Q)
    with open(tmp_path / "Q.bin", "ab") as f:                     # trailing bytes after an int32-header file
        f.write(b"12345678")
    XM.solve(str(tmp_path), 3, 1e-12, 0.0, 1000.0)               # the reference's reader ignores trailing bytes; so does v1 here
    with open(tmp_path / "Q.bin", "wb") as f:
        f.write(np.array(Q.shape, dtype="<i4").tobytes()); f.write(b"\0" * 100)
    with pytest.raises(RuntimeError, match="short file"):
        XM.solve(str(tmp_path), 3, 1e-12, 0.0, 1000.0)
    # block-CSR in, warm-start mode with scales
    P = tl.gen_vg(60, deg=6, sigma=0.3, seed=60)
    Rb, sb, ib = XM.solve_bsr(P["rowptr"], P["colidx"], P["blocks"], 5, 1e-10, 2.0, 100.0)
    ctx = xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]))
    Rc, sc, ic = ctx.solve(5, 1e-10, 2.0)
    ctx.close()
    assert np.array_equal(Rb, Rc) and np.array_equal(sb, sc) and ib["rank"] == ic["rank"]
    Rw, sw, iw = XM.solve_array(P["Q"], 5, 1e-10, 2.0, 100.0, mode=2, s_ini=sb)
    assert iw["status"] == ib["status"] and abs(iw["primal"] - ib["primal"]) <= 1e-8 * abs(ib["primal"])


@pytest.mark.parametrize("n", [356, 1778])
def test_full_size_properties(xmamd, n):
    """BASELINE configs at full size (Dubrovnik-356 / Venice-1778 camera counts, dense SBA-like Q): too big for the
    oracle's O(n^3) certificate, so checked through size-independent properties: certificate closes (primal == dual,
    lambda_min >= 0), iterate on the manifold, planted rotations recovered, product linearity."""
    P = tl.gen_dense(n, seed=n)
    R, s, info = xmamd.solve_dense(P["Q"], 5, 1e-9, 0.0)
    # (rank-3 BM may stop at a saddle on the larger instance; the staircase then certifies at rank 4 or 5)
    assert info["status"] == 1 and 3 <= info["rank"] <= 5
    assert abs(info["gap"]) <= 1e-6 * max(1.0, abs(info["primal"])) and info["min_eig"] > -1e-6
    assert tl.stiefel_defect(R) < 1e-12
    # optimality as a fact independent of the library under test AND of the oracle: multipliers by lstsq, the spectrum of S by
    # LAPACK's eigvalsh on the GPU's own (R, s)  (the library's Lanczos value and dual must agree with it)
    cn = tl.certificate_numpy(P["Q"], R, s, 0.0)
    assert cn["min_eig"] > -1e-7 and abs(cn["gap"]) <= 1e-6 * max(1.0, cn["primal"]) and cn["stationarity"] < 1e-5
    assert cn["primal"] == pytest.approx(info["primal"], rel=1e-10) and cn["dual"] == pytest.approx(info["dual"], rel=1e-7)
    assert info["min_eig"] == pytest.approx(cn["min_eig"], abs=1e-7) and info["cert_flags"] == 0
    rot, sc = tl.recover_rotations(R, s)
    Rs = P["R_star"]
    ref = np.concatenate([Rs[0] @ Rs[i].T for i in range(n)], axis=1)
    if info["rank"] == 3:   # relaxation tight at rank 3: the planted rotations are the optimum up to the noise level
        assert tl.rel_fro(rot, ref) < 5e-2 and abs(sc - 1).max() < 0.15
    rng = np.random.default_rng(0)
    A = rng.standard_normal((3 * n, 3)); B = rng.standard_normal((3 * n, 3))
    dq = xmamd.dense_upload(P["Q"])
    lhs = xmamd.qw_dense(None, 2.0 * A - 0.5 * B, dq=dq)
    rhs = 2.0 * xmamd.qw_dense(None, A, dq=dq) - 0.5 * xmamd.qw_dense(None, B, dq=dq)
    assert tl.rel_fro(lhs, rhs) < 1e-13
    assert tl.rel_fro(xmamd.qw_dense(None, A, dq=dq), P["Q"] @ A) < 1e-13
    dq.free()


def test_dense_from_bsr3_equals_upload(xmamd):
    P = tl.gen_vg(200, deg=9, sigma=0.2, seed=9)
    W = np.random.default_rng(1).standard_normal((600, 4))
    dq = xmamd.dense_from_bsr3(P["rowptr"], P["colidx"], P["blocks"])
    got = xmamd.qw_dense(None, W, dq=dq)
    assert np.array_equal(got, xmamd.qw_dense(P["Q"], W))
    ctx = xmamd.Context(dq=dq, n=200)
    R, s, info = ctx.solve(4, 1e-8, 9.0)
    ctx.close(); dq.free()
    R2, s2, i2 = xmamd.solve_dense(P["Q"], 4, 1e-8, 9.0)
    assert np.array_equal(R, R2) and np.array_equal(s, s2)
    # XM_STORAGE_BSR3_DENSE: the context expands the block description itself (what bench.py uses at every N)
    ctx = xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]), densify=True)
    R3, s3, i3 = ctx.solve(4, 1e-8, 9.0)
    ctx.close()
    assert np.array_equal(R3, R2) and np.array_equal(s3, s2)


def test_rccl_path_single_rank(xmamd, tmp_path):
    """XM_FORCE_COMM=1 runs the multi-GPU code path on a 1-rank RCCL communicator (exercises dlopen(RCCL), ncclCommInitRank,
    the in-place ncclAllGather and the single-exchange tCG whose product input follows the recurrence W+ = beta W - A+
    instead of being rebuilt from p): same optimum as the plain single-GPU run; the trajectories agree to rounding."""
    import subprocess, sys, textwrap
    code = textwrap.dedent(f"""
        import sys, os, ctypes as C
        sys.path.insert(0, {os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'xm-code_amd')!r})
        sys.path.insert(0, {os.path.dirname(os.path.abspath(__file__))!r})
        import numpy as np, xmamd, xm_testlib as tl
        Q = tl.load_bin(os.path.join(tl.GOLDEN, 'simple2', 'Q.bin'))
        if os.environ.get('XM_FORCE_COMM') == '1':
            buf = (C.c_char * 128)()
            xmamd._chk(xmamd.lib().xm_comm_unique_id(buf))
            xmamd._chk(xmamd.lib().xm_comm_init(0, 1, 0, buf.raw, None))
        R, s, info = xmamd.solve_dense(Q, 3, 1e-16, 0.0, tuning=tl.env_tuning())
        np.savez(sys.argv[1], R=R, s=s, primal=info['primal'], tcg=info['tcg_iters'])
        xmamd.lib().xm_comm_finalize()
    """)
    outs = []
    for force in ("0", "1"):
        out = str(tmp_path / f"r{force}.npz")
        env = dict(os.environ, XM_FORCE_COMM=force)
        subprocess.check_call([sys.executable, "-c", code, out], env=env, timeout=600)
        outs.append(np.load(out))
    assert float(outs[0]["primal"]) == pytest.approx(float(outs[1]["primal"]), rel=1e-12)
    assert tl.rotation_parity(outs[0]["R"], outs[0]["s"], outs[1]["R"], outs[1]["s"]) < 1e-8
    assert abs(int(outs[0]["tcg"]) - int(outs[1]["tcg"])) <= 0.05 * int(outs[0]["tcg"])
    # the same through the split product (local strip on a second stream beside the RCCL all-gather): real RCCL stream
    # ordering between the two streams, one rank
    out = str(tmp_path / "r2.npz")
    subprocess.check_call([sys.executable, "-c", code, out], env=dict(os.environ, XM_FORCE_COMM="1", XMT_TUNING='{"overlap_min_mb": -1}'), timeout=600)
    o2 = np.load(out)
    assert float(o2["primal"]) == pytest.approx(float(outs[0]["primal"]), rel=1e-12)
    assert tl.rotation_parity(o2["R"], o2["s"], outs[0]["R"], outs[0]["s"]) < 1e-8


def test_dubrovnik356_full_solve_matches_oracle(xmamd, oracle):
    """BASELINE config 'Dubrovnik-356 on one MI355X': the complete staircase solve (trust region + certificate) against the
    CPU oracle on the same dense Q: optimum value, certificate and anchored rotations (<= 1e-6, north_star)."""
    P = tl.gen_dense(356, seed=356)
    R, s, info = xmamd.solve_dense(P["Q"], 5, 1e-9, 0.0, trace=2000)
    Ro, so, io = oracle.solve(P["Q"], 5, 1e-9, 0.0, 1000.0, trace=2000)
    assert info["rank"] == io["rank"] == 3 and info["status"] == io["status"] == 1
    assert info["primal"] == pytest.approx(io["trace"][-1, 0], rel=1e-10)
    assert info["min_eig"] == pytest.approx(io["cert"]["min_eig"], abs=1e-7)
    assert tl.rotation_parity(R, s, Ro, so) < 1e-6
    assert tl.rel_fro(tl.gram(R, s), tl.gram(Ro, so)) < 1e-6
    k = 8
    assert np.allclose(info["trace"][:k, 0], io["trace"][:k, 0], rtol=1e-9)
    assert np.array_equal(info["trace"][:k, 2:4], io["trace"][:k, 2:4])


def test_mid700_staircase_matches_recorded_oracle(xmamd):
    """700-camera dense instance whose rank-3 critical point is NOT optimal: both solvers escalate to rank 4 (saddle escape along the
    certificate's eigenvector) and certify there; value, certificate and gauge-invariant solution agree.  The oracle's side (two O(n^3)
    certificates, minutes of CPU) is recorded by scripts/record_oracle_large.py mid700 (tests/golden/synth/mid700_oracle.*), so the
    case runs in the driver's suite."""
    fj = os.path.join(G, "synth", "mid700_oracle.json")
    if not os.path.exists(fj):
        pytest.skip("recorded oracle run not present")
    c = json.load(open(fj))
    P = tl.gen_dense(c["n"], seed=c["seed"])
    R, s, info = xmamd.solve_dense(P["Q"], c["max_rank"], c["tol"], c["lam"])
    assert info["rank"] == c["rank"] == 4 and info["status"] == c["status"] == 1
    assert info["primal"] == pytest.approx(c["f"], rel=1e-9)
    rot, _ = tl.recover_rotations(R, s)
    assert tl.rel_fro(rot, np.load(os.path.join(G, "synth", "mid700_oracle_rot.npy"))) < 1e-6
    sR = tl.scale_rows(R, s)
    idx = tl.gram_sample_index(sR.shape[0])
    assert tl.rel_fro((sR[idx[:, 0]] * sR[idx[:, 1]]).sum(axis=1), np.load(os.path.join(G, "synth", "mid700_oracle_gram_sample.npy"))) < 1e-6


def test_lanczos_on_a_clustered_spectrum(xmamd):
    """certificate eigenvalue on a CLUSTERED spectrum: two noise-free view-graph clusters of 170 cameras joined by two weak edges.  At
    the planted optimum S = Q has the three-dimensional null space of a connected noise-free problem plus three more eigenvalues of
    order the coupling (2e-4): six eigenvalues within 1e-3 of each other at the bottom of a spectrum that reaches 20.  The Lanczos run
    (3n = 1020 rows: not the exhaustive small-problem route) must deliver lambda_min to 1e-9 |S| of numpy's eigvalsh on the same S and
    the solve must certify."""
    rng = np.random.default_rng(5)
    n1 = 170
    A, _ = tl.gen_vg_edges(n1, 8, 21); B, _ = tl.gen_vg_edges(n1, 8, 22)
    e = np.concatenate([A, B + n1, np.array([[3, n1 + 5], [100, n1 + 77]])])
    w = np.ones(e.shape[0]); w[-2:] = 1e-2
    n = 2 * n1
    Rs = tl.haar_so3(rng, n)
    M = Rs[e[:, 0]] @ np.transpose(Rs[e[:, 1]], (0, 2, 1))                      # noise-free: f* = 0, R* = Rs
    rp, ci, bl = tl.vg_from_edges(n, e[:, 0], e[:, 1], w, M)
    Q = tl.bsr_to_dense(n, rp, ci, bl)
    ev = np.linalg.eigvalsh(Q)
    assert ev[5] < 1e-3 and ev[6] > 1.0                                          # the cluster is really there
    R, s, info = xmamd.solve_dense(Q, 5, 1e-10, 5.0)
    assert info["rank"] == 3 and info["status"] == 1 and not (info["cert_flags"] & xmamd.CERT_EIG_NOT_CONVERGED)
    assert not (info["cert_flags"] & xmamd.CERT_EIG_EXACT)
    cert = tl.certificate_numpy(Q, R, s, 5.0)
    assert abs(info["min_eig"] - cert["min_eig"]) < 1e-9 * max(1.0, np.abs(ev).max())
    # the weak mode (stiffness 2e-4) limits the planted-rotation accuracy at this tolerance; the trust region ends by the reference's "rdotr
    # touched machine precision" rule (stop 5) or by "loss_qu > 0" (12), at a cost that depends on the path: 1.3e-13 ... 3.1e-9 over the three
    # summation groupings and the two outer-iteration forms (f* = 0; the certificate above is what decides)
    assert info["primal"] < 1e-8 and tl.rotation_parity(R, s, Rs.reshape(3 * n, 3), np.ones(n)) < 1e-5


@pytest.mark.parametrize("name", ["simple1", "simple2", "synth/dense49", "synth/vg40_stair"])
def test_recover_rotations_matches_reference_recover_XM(xmamd, oracle, name):
    """xm_recover_rotations against the golden output of the REFERENCE's own utils/recoversolution.py
    (rot_anchor.npy was produced by recover_XM on the oracle's solution; vg40_stair has rank 6 -> rank-3 projection)."""
    Q, exp, d = _case(name)
    Ro, so, io = oracle.solve(Q, exp["max_rank"], exp["tol"], exp["lam"], 1000.0)
    rot, sc, neg = xmamd.recover_rotations(Ro, so)
    gold = np.load(os.path.join(d, "rot_anchor.npy"))
    assert tl.rel_fro(rot, gold) < 1e-9
    rot2, sc2 = tl.recover_rotations(Ro, so)
    assert np.allclose(sc, sc2, rtol=1e-12)
    blocks = rot.T.reshape(-1, 3, 3)                    # block i transposed
    assert np.abs(blocks @ np.transpose(blocks, (0, 2, 1)) - np.eye(3)).max() < 1e-13
    assert np.allclose(np.abs(rot[:, :3]), np.eye(3), atol=1e-13)     # +-I (the reference flips the global sign on a negative-det majority)


def test_XM_solve_against_the_reference_held_ground_truth(xmamd, tmp_path, monkeypatch):
    """The one output-side artefact the REFERENCE itself holds for this path: assets/SIMPLE2/gtR.bin (ground-truth rotations read by
    utils/readgt_BAL.py:10-28 and compared at 2_test_creatematrix.py:173-217).  The HIP solve -- through the reference's own surface,
    XM.solve(path, 5, tol, 0, 1000) on the Q its create_matrix wrote, then xm_recover_rotations -- against gtR.bin DIRECTLY (no oracle in
    between), through the frame re-indexing of 2_test_creatematrix.py:86-91 (frame_index.npy): median <= 3e-3, max <= 6e-3 per camera,
    the agreement the SURVEY probe measured between the certified optimum and the ground truth (noise level of the scene)."""
    import shutil
    d = os.path.join(tl.GOLDEN, "simple2")
    shutil.copy(os.path.join(d, "Q.bin"), tmp_path / "Q.bin")
    monkeypatch.setenv("XM_QUIET", "1")
    XM = xmamd.import_XM()
    assert XM.solve(str(tmp_path), 5, 1e-9, 0.0, 1000.0) is None            # 2_test_creatematrix.py:149 (tighter tol: parity)
    R = tl.load_bin(tmp_path / "R.bin"); s = tl.load_bin(tmp_path / "s.bin").reshape(-1)
    assert R.shape == (279, 3)
    rot, sc, neg = xmamd.recover_rotations(R, s)
    gt = tl.load_bin(os.path.join(d, "gtR.bin"))
    fi = np.load(os.path.join(d, "frame_index.npy"))
    Gt = lambda i: gt[:, 3 * fi[i]:3 * fi[i] + 3]
    err = np.array([np.linalg.norm(rot[:, 3 * i:3 * i + 3] - Gt(0) @ Gt(i).T) for i in range(fi.size)])
    assert err.max() < 6e-3 and np.median(err) < 3e-3, (err.max(), np.median(err))
    assert np.all(np.abs(np.linalg.det(rot.T.reshape(-1, 3, 3)) - 1.0) < 1e-12)     # proper rotations, as the ground truth


def test_recover_rotations_on_degenerate_camera_blocks(xmamd):
    """utils/recoversolution.py:65-86 projects every block with numpy's SVD, which returns an orthogonal factor whatever the block;
    the device projection (scaled Newton) must not hand back a singular block unprojected: a camera with a ZERO block, one with a
    rank-1 and one with a rank-2 block come back orthogonal (the rank-2 case: the unique orthogonal polar factor with det +1), the
    regular cameras are untouched, nothing is NaN -- in both kernel forms"""
    rng = np.random.default_rng(5)
    n = 40
    Rs = tl.haar_so3(rng, n)
    s = rng.uniform(0.5, 2.0, n)
    R = np.concatenate([Rs[0].T @ Rs[i] for i in range(n)], axis=0)          # rows orthonormal, camera 0 = identity
    R[3 * 7:3 * 7 + 3] = 0.0                                                   # zero block
    u = rng.standard_normal(3); v = rng.standard_normal(3)
    R[3 * 11:3 * 11 + 3] = np.outer(u, v)                                      # rank 1
    B = Rs[13].copy(); B[2] = B[0] + B[1]                                      # rank 2
    R[3 * 13:3 * 13 + 3] = B
    ref, _ = tl.recover_rotations(np.delete(R.reshape(n, 3, 3), [7, 11, 13], axis=0).reshape(-1, 3), np.delete(s, [7, 11, 13]))
    for variant in (None, 0, 1):
        rot, sc, neg = xmamd.recover_rotations(R, s, variant=variant)[:3]
        assert np.all(np.isfinite(rot)) and np.all(np.isfinite(sc))
        blocks = rot.T.reshape(-1, 3, 3)
        assert np.abs(blocks @ np.transpose(blocks, (0, 2, 1)) - np.eye(3)).max() < 1e-12
        assert sc[7] == 0.0 and np.allclose(blocks[7], np.eye(3))
        keep = np.delete(rot.reshape(3, n, 3), [7, 11, 13], axis=1).reshape(3, -1)
        assert tl.rel_fro(keep, ref) < 1e-12
        # rank 2: X = B_0 B^T / (s_0 s_i) has a unique nearest rotation when its two non-zero singular values are distinct
        X = (R[:3] * s[0]) @ (R[39:42] * s[13]).T
        U, S, Vt = np.linalg.svd(X)
        want = U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt
        assert np.abs(rot[:, 39:42] - want).max() < 1e-9


def test_recover_projection_one_wavefront_per_camera_equals_thread_form(xmamd, oracle):
    """north_star's "one wavefront per camera for the 3x3 SVD with warp-shuffle reductions", built for the place the SVD really is (N1,
    utils/recoversolution.py:65-86): lane e < 9 owns one entry, cofactors through shuffles, sums through the DPP wave reduction.  Same
    rotations and scales as the thread-per-camera kernel (scripts/kbench_recover.py records the timing of both)"""
    Q, exp, d = _case("synth/vg40_stair")
    Ro, so, io = oracle.solve(Q, exp["max_rank"], exp["tol"], exp["lam"], 1000.0)
    a = xmamd.recover_rotations(Ro, so, variant=0)
    b = xmamd.recover_rotations(Ro, so, variant=1)
    assert tl.rel_fro(b[0], a[0]) < 1e-13 and np.allclose(a[1], b[1], rtol=1e-14) and a[2] == b[2]
    assert tl.rel_fro(b[0], np.load(os.path.join(d, "rot_anchor.npy"))) < 1e-9
    rng = np.random.default_rng(3)
    n = 1000
    R = np.concatenate([q for q in tl.haar_so3(rng, n)], axis=0) @ rng.standard_normal((3, 5)); s = rng.uniform(0.5, 2, n)   # rank-5 factor, odd camera count per workgroup
    a = xmamd.recover_rotations(R, s, variant=0); b = xmamd.recover_rotations(R, s, variant=1)
    assert tl.rel_fro(b[0], a[0]) < 1e-12 and np.allclose(a[1], b[1], rtol=1e-13) and a[2] == b[2]


@pytest.mark.parametrize("n,o", [(1, 3), (2, 3), (7, 3), (8, 4), (9, 5), (43, 3), (85, 3), (86, 4), (87, 5), (128, 3), (149, 4), (171, 5), (700, 3), (1031, 5)])
def test_qw_dense_symmetric_kernel_matches_oracle(xmamd, oracle, n, o):
    """half-traffic product (reads only the upper block triangle) on a symmetric Q == the full product"""
    rng = np.random.default_rng(7 * n + o)
    A = rng.standard_normal((3 * n, 3 * n)); Q = A + A.T
    W = rng.standard_normal((3 * n, o))
    ref = oracle.qw(Q, W, 2.0)
    got = xmamd.qw_dense(Q, W, 2.0, sym=True)
    assert tl.rel_fro(got, ref) < 1e-13
    assert tl.rel_fro(xmamd.qw_dense(Q, W, 2.0), ref) < 1e-13


@pytest.mark.parametrize("n,o,k,kf", [(700, 3, 16, 4), (700, 4, 8, 2), (1031, 3, 12, 5), (1031, 5, 7, 3), (343, 4, 5, 1), (2200, 3, 9, 2)])
def test_qw_dense_symmetric_kernel_with_a_forced_finer_cut(xmamd, n, o, k, kf):
    """the plan cuts the grid rows dispatched last into shorter chunks only for sweeps of several residency rounds (>= ~5 000 cameras); forced
    here at small sizes (xm_bench_symv_k) so that the reducer's per-column record counts -- a camera's three columns can lie in two strips
    that are cut differently -- meet numpy on every row, in both sweep directions"""
    rng = np.random.default_rng(11 * n + o)
    A = rng.standard_normal((3 * n, 3 * n)); Q = A + A.T; del A
    W = rng.standard_normal((3 * n, o))
    ref = 2.0 * (Q @ W)
    L = xmamd.lib()
    try:
        xmamd._chk(L.xm_bench_symv_k(k, 1, kf))
        p = (C.c_int32 * 4)(); xmamd._chk(L.xm_symv_plan(n, p))
        assert p[0] == k and p[1] == kf
        dq = xmamd.dense_upload(Q)
        got = xmamd.qw_dense(Q, W, 2.0, dq=dq, sym=True)
        err = np.abs(got - ref).max(axis=1) / np.abs(ref).max()
        assert err.max() < 1e-13, f"worst row {int(err.argmax())} (camera {int(err.argmax()) // 3}): {err.max():.2e}"
        # bottom-up sweep of every chunk (what odd tCG iterations do): xm_qw_dense_sym_time alternates, the functional entry sweeps top-down,
        # so time two launches and read the output of the second
        dW = xmamd.DevArray(xmamd.to_rm(W, rows=xmamd.dense_ld(n))); dO = xmamd.DevArray(nbytes=3 * n * xmamd.pitch_of(o) * 8)
        ms = C.c_double()
        xmamd._chk(L.xm_qw_dense_sym_time(dq.ptr, n, o, dW.ptr, dO.ptr, 1, C.byref(ms)))   # 3 warm-ups (rev 0 1 0) + 1 timed launch (rev 1)
        out = xmamd.from_rm(dO.get(), 3 * n, o)
        assert np.abs(out - 0.5 * ref).max() / np.abs(ref).max() < 1e-13
        for b in (dq, dW, dO):
            b.free()
    finally:
        xmamd._chk(L.xm_bench_symv_k(0, 1, 0))


@pytest.mark.parametrize("n,o,cut", [(1, 3, None), (2, 3, None), (7, 3, None), (42, 3, None), (43, 3, None), (85, 3, None), (86, 4, None),
                                     (87, 5, None), (128, 3, None), (171, 5, None), (343, 4, (5, 1, 1))])
def test_dense_products_of_small_integers_are_exact(xmamd, n, o, cut):
    """symmetric Q and W with integer entries in [-8, 8], alpha = 2: every product and partial sum is an integer far below 2^53 and Q is
    exact in fp32, so the general and the symmetric product, from the f64 matrix and from its fp32 copy, the sweeps top-down (functional
    entry) and bottom-up (the timing hook's last launch, alpha 1), equal numpy's 2 Q W exactly whatever their summation orders -- a wrong
    mask, a swapped column pair or a wrong partial-sum offset shows at zero tolerance.  Shapes: a half strip, a full strip, an odd camera
    count, two strips with a half second strip, an odd strip count whose middle strip has no fold partner; one forced finer cut"""
    rng = np.random.default_rng(13 * n + o)
    A = np.triu(rng.integers(-8, 9, (3 * n, 3 * n)).astype(np.float64))
    Q = A + np.triu(A, 1).T
    W = rng.integers(-8, 9, (3 * n, o)).astype(np.float64)
    ref = 2.0 * (Q @ W)
    L = xmamd.lib()
    ld = xmamd.dense_ld(n)
    dq = xmamd.dense_upload(Q); d32 = xmamd.dense_to_f32(dq, n)
    dW = xmamd.DevArray(xmamd.to_rm(W, rows=ld)); ms = C.c_double()
    def run(fn, mat, *tail):
        dO = xmamd.DevArray(np.full(3 * n * xmamd.pitch_of(o), np.nan))
        try:
            xmamd._chk(fn(mat.ptr, n, o, dW.ptr, dO.ptr, *tail)); xmamd._chk(L.xm_dev_sync())
            return xmamd.from_rm(dO.get(), 3 * n, o)
        finally:
            dO.free()
    try:
        if cut:
            xmamd._chk(L.xm_bench_symv_k(*cut))
        got = {"general f64": run(L.xm_qw_dense, dq, 2.0, None),
               "symmetric f64 top-down": run(L.xm_qw_dense_sym, dq, 2.0, None),
               "symmetric f64 bottom-up": 2.0 * run(L.xm_qw_dense_sym_time, dq, 1, C.byref(ms)),
               "general fp32": run(L.xm_qw_dense_f32, d32, 2.0, None),
               "symmetric fp32 top-down": run(L.xm_qw_dense_sym_f32, d32, 2.0, None),
               "symmetric fp32 bottom-up": 2.0 * run(L.xm_qw_dense_sym_f32_time, d32, 1, C.byref(ms))}
    finally:
        xmamd._chk(L.xm_bench_symv_k(0, 1, 0))
        for b in (dq, d32, dW):
            b.free()
    for what, out in got.items():
        bad = np.flatnonzero((out != ref).any(axis=1))
        assert np.array_equal(out, ref), f"{what}: {bad.size} rows differ, first {int(bad[0]) if bad.size else -1}"


def test_new_products_are_bit_reproducible(xmamd):
    """fixed summation orders everywhere: the half-traffic symmetric product (per-strip row sums through LDS, per-chunk column sums,
    list-ordered reducer) and the matrix-free chain (degree-sorted landmark groups, hub landmarks in the same launch) give the same
    bits on every call, and so does a whole matrix-free solve"""
    rng = np.random.default_rng(3)
    n = 700
    A = rng.standard_normal((3 * n, 3 * n)); Q = A + A.T
    dq = xmamd.dense_upload(Q)
    for o in (3, 4):
        W = rng.standard_normal((3 * n, o))
        a = xmamd.qw_dense(Q, W, 1.5, dq=dq, sym=True)
        for _ in range(3):
            assert np.array_equal(xmamd.qw_dense(Q, W, 1.5, dq=dq, sym=True), a)
    dq.free()
    S = tl.gen_scene(300, 6000, 5, seed=11)
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]))
    W = rng.standard_normal((900, 3))
    y = ctx.qw(W)
    assert np.array_equal(ctx.qw(W), y) and np.array_equal(ctx.qw(W), y)
    R1, s1, i1 = ctx.solve(5, 1e-8, 0.0)
    R2, s2, i2 = ctx.solve(5, 1e-8, 0.0)
    ctx.close()
    assert np.array_equal(R1, R2) and np.array_equal(s1, s2) and i1["tcg_iters"] == i2["tcg_iters"] and i1["primal"] == i2["primal"]


def test_symmetry_check_decides_the_dense_path(xmamd):
    """the half-traffic product reads the upper triangle only, so it is taken (3n >= 4096 rows on one GPU) for an EXACTLY symmetric Q alone: one
    entry of the lower triangle off by 1e-9, or a NaN, and the general kernel runs (asym_kernel: tiled transposed compare, sticky NaN)"""
    rng = np.random.default_rng(5)
    n = 2100
    A = rng.standard_normal((3 * n, 64))
    Q = A @ A.T / 64 + np.eye(3 * n)
    Q = 0.5 * (Q + Q.T)
    def picked(Qx):
        _, _, info = xmamd.solve_dense(Qx, 3, 1e-1, 0.0, max_time=0.0, mode=xmamd.MODE_RANK3)   # no iterations, no certificate: the decision is taken at upload
        return int(info["sym_product"])
    assert picked(Q) == 1
    Q2 = Q.copy(); Q2[4000, 17] += 1e-9
    assert picked(Q2) == 0
    Q3 = Q.copy(); Q3[6299, 6200] = np.nan
    assert picked(Q3) == 0


def test_symmetric_path_equals_general_path(xmamd):
    """the half-traffic symmetric product (forced at this size: xm_tuning_t.sym = 1) and the general kernel (sym = -1) must land on the
    same certified optimum (trajectories differ only by summation order)."""
    Q = tl.gen_dense(356, seed=356)["Q"]
    outs = [xmamd.solve_dense(Q, 5, 1e-9, 0.0, tuning=dict(sym=flag)) for flag in (1, -1)]
    assert outs[0][2]["sym_product"] == 1 and outs[1][2]["sym_product"] == 0
    assert outs[0][2]["rank"] == outs[1][2]["rank"] == 3
    assert outs[0][2]["primal"] == pytest.approx(outs[1][2]["primal"], rel=1e-11)
    assert tl.rotation_parity(outs[0][0], outs[0][1], outs[1][0], outs[1][1]) < 1e-7


def test_high_rank_staircase(xmamd, oracle):
    """noisy view graphs that need ranks up to 9 / run out at max_rank 10: exercises every rank instantiation (o = 3..10) of
    the kernels inside whole solves, status 1 (certified) and status 2 (max rank) exits (XM_main.cu:260-276)"""
    P = tl.gen_vg(80, deg=5, sigma=3.0, seed=5)
    R, s, info = xmamd.solve_dense(P["Q"], 10, 1e-9, 3.0)
    Ro, so, io = oracle.solve(P["Q"], 10, 1e-9, 3.0, 1000.0, trace=20000)
    assert info["rank"] == io["rank"] == 9 and info["status"] == io["status"] == 1
    assert info["primal"] == pytest.approx(io["trace"][-1, 0], rel=1e-8)
    assert tl.rel_fro(tl.gram(R, s), tl.gram(Ro, so)) < 1e-6          # certified optimum is unique
    assert tl.stiefel_defect(R) < 1e-12
    P = tl.gen_vg(100, deg=6, sigma=3.0, seed=6)
    R, s, info = xmamd.solve_dense(P["Q"], 10, 1e-9, 5.0)
    Ro, so, io = oracle.solve(P["Q"], 10, 1e-9, 5.0, 1000.0, trace=20000)
    assert info["rank"] == io["rank"] == 10 and info["status"] == io["status"] == 2
    assert R.shape == (300, 10) and info["min_eig"] < -1e-4
    assert info["primal"] == pytest.approx(io["trace"][-1, 0], rel=1e-3)


def _two_rank_worker_code():
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return textwrap.dedent(f"""
        import sys, os
        sys.path.insert(0, {os.path.join(root, 'xm-code_amd')!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
        import numpy as np, xmamd, xm_testlib as tl
        rank, world, name, out, case = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
        TN = tl.env_tuning()        # xm_tuning_t fields of this case (XMT_TUNING: a variable of the tests, not of the library)
        if world > 1:
            xmamd._chk(xmamd.lib().xm_comm_init_shm(rank, world, 0, name.encode(), 64 << 20))
        if case == "dense":
            P = tl.gen_vg(41, deg=3, sigma=1.5, seed=40)         # odd camera count (padding camera), needs rank escalation
            ctx = xmamd.Context(Q=P["Q"], tuning=TN); args = (6, 1e-9, 3.0)
        elif case == "densify":                                    # block description expanded per rank on the device
            P = tl.gen_vg(41, deg=3, sigma=1.5, seed=40)
            ctx = xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]), densify=True, tuning=TN); args = (6, 1e-9, 3.0)
        elif case == "overlap":                                    # enough columns per rank for whole tiles inside the own strip
            P = tl.gen_vg(400, deg=8, sigma=0.3, seed=9)
            ctx = xmamd.Context(Q=P["Q"], tuning=TN); args = (5, 1e-9, 10.0)
        elif case == "file":                                       # the reference's file surface: every rank reads ITS row strip of Q.bin
            d = os.path.join(os.path.dirname(out), "ds_w%d" % world)
            if rank == 0:
                os.makedirs(d, exist_ok=True)
                tl.save_bin(os.path.join(d, "Q.bin"), tl.gen_vg(41, deg=3, sigma=1.5, seed=40)["Q"])
                open(os.path.join(d, "ready"), "w").close()
            import time
            while not os.path.exists(os.path.join(d, "ready")):
                time.sleep(0.05)
            os.environ["XM_QUIET"] = "1"
            xmamd._chk(xmamd.lib().xm_solve(d.encode(), 6, 1e-9, 3.0, 1000.0))
            xmamd.lib().xm_comm_finalize()
            if rank == 0:
                R = tl.load_bin(os.path.join(d, "R.bin")); s = tl.load_bin(os.path.join(d, "s.bin")).reshape(-1)
                np.savez(out, R=R, s=s, primal=0.0, rank=R.shape[1], status=1, tcg=0, min_eig=0.0, trace=np.zeros((1, 6)))
            sys.exit(0)
        else:
            P = tl.gen_vg(301, deg=10, sigma=0.1, seed=5)      # "sell": the same through the sliced-ELL product (tuning sell = 1)
            ctx = xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]), tuning=TN); args = (5, 1e-10, 10.0)
        R, s, info = ctx.solve(*args, trace=4000)
        ctx.close()
        np.savez(out, R=R, s=s, primal=info["primal"], rank=info["rank"], status=info["status"], tcg=info["tcg_iters"],
                 min_eig=info["min_eig"], trace=info["trace"])
        xmamd.lib().xm_comm_finalize()
    """)


@pytest.mark.parametrize("case,world", [("dense", 2), ("bsr", 2), ("densify", 2), ("dense", 3), ("bsr", 3), ("dense-async", 2), ("bsr-async", 3),
                                        ("sell", 2), ("sell-async", 2), ("file", 2), ("overlap", 2), ("overlap-async", 3)])
def test_two_ranks_one_gpu(xmamd, tmp_path, case, world):
    """The whole row-partitioned solver with TWO or THREE ranks (processes) sharing the one GPU of the test box through the
    shared-memory test transport: camera partition 21+20 (+1 inert padding camera) resp. 14+14+13 (+1), replicated product input, gathered
    partial sums, staircase with rank escalation, Lanczos certificate.  Both ranks must return bit-identical results and
    agree with the single-rank run (same optimum; trajectories differ only by summation grouping).
    "-async": the transport is STREAM-ORDERED (XM_SHM_ASYNC=1: the exchange runs in a host function on the solver's stream, the
    calling thread never blocks, like an RCCL collective), so the enqueue-ahead logic of the tCG is exercised for real: a rank
    that enqueued a different number of collectives than its peer would leave a barrier unmatched and fail with XM_ERR_COMM.
    "sell": block-sparse storage through the sliced-ELL product.  "overlap": dense products outside the tCG split in two launches
    around the all-gather (local column strip first, on a second stream).  "file": the reference's file surface, each rank reading only
    its own row strip of Q.bin (xm_solve), rank 0 writing R.bin / s.bin."""
    import subprocess, sys, uuid
    code = _two_rank_worker_code()
    name = "/xm_test_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, XM_SHM_TIMEOUT="60")
    if case.endswith("-async"):
        env["XM_SHM_ASYNC"] = "1"; case = case[:-6]
    if case == "sell":
        env["XMT_TUNING"] = '{"sell": 1}'
    if case == "overlap":     # the local column strip of the dense product runs on a second stream beside the all-gather of W
        env["XMT_TUNING"] = '{"overlap_min_mb": -1}'
        env["XM_COMM_TRACE"] = str(tmp_path / "trace")
    procs, outs = [], []
    logs = []
    for r in range(world):
        out = str(tmp_path / f"w2_r{r}.npz"); outs.append(out)
        logs.append(open(tmp_path / f"w2_r{r}.log", "w+"))
        procs.append(subprocess.Popen([sys.executable, "-c", code, str(r), str(world), name, out, case], stdout=logs[-1], stderr=subprocess.STDOUT, env=env))
    rcs = [p.wait(timeout=600) for p in procs]
    if any(rcs) and os.environ.get("XM_COMM_TRACE"):
        a_, b_ = (open(os.environ["XM_COMM_TRACE"] + f".{r}").read().splitlines() for r in range(2))
        k = next((i for i, (x, y) in enumerate(zip(a_, b_)) if x != y), min(len(a_), len(b_)))
        print(f"first divergence at line {k} of {len(a_)}/{len(b_)}:\n rank0: {a_[max(0,k-4):k+4]}\n rank1: {b_[max(0,k-4):k+4]}")
    if any(rcs):
        for r, lg in enumerate(logs):
            lg.seek(0)
            print(f"---- rank {r} (rc {rcs[r]}) ----\n" + lg.read()[-1500:])
    assert rcs == [0] * world
    if case == "overlap":     # the split path really ran (a rank whose column strip holds no whole 256-column tile keeps the single launch)
        ran = ["overlap_split" in open(str(tmp_path / "trace") + f".{r_}").read() for r_ in range(world)]
        assert ran[0] and sum(ran) >= world - 1, ran
    single = str(tmp_path / "w1.npz")
    subprocess.check_call([sys.executable, "-c", code, "0", "1", name, single, case], timeout=600, env=env)
    a, c = np.load(outs[0]), np.load(single)
    if case == "file":   # R.bin / s.bin written by rank 0 of the partitioned run vs the single-process run of the same files
        assert a["R"].shape == c["R"].shape and tl.rel_fro(tl.gram(a["R"], a["s"]), tl.gram(c["R"], c["s"])) < 1e-6
        assert tl.rotation_parity(a["R"], a["s"], c["R"], c["s"]) < 1e-6
        return
    for o_ in outs[1:]:
        b = np.load(o_)
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["s"], b["s"]) and np.array_equal(a["trace"], b["trace"])
    assert int(a["rank"]) == int(c["rank"]) and int(a["status"]) == int(c["status"]) == 1
    assert float(a["primal"]) == pytest.approx(float(c["primal"]), rel=1e-9)
    assert tl.rel_fro(tl.gram(a["R"], a["s"]), tl.gram(c["R"], c["s"])) < 1e-6
    k = 5
    assert np.allclose(a["trace"][:k, :2], c["trace"][:k, :2], rtol=1e-9)


def test_rccl_two_ranks_on_one_gpu_or_documented_refusal(xmamd, tmp_path):
    """Real RCCL with MORE than one rank on the 1-GPU test box: two processes try to form a 2-rank communicator on device 0.
    If this RCCL build permits it, the partitioned solver runs over it and must reproduce the single-rank optimum.  If RCCL
    refuses (a communicator may hold each GPU only once: 'Duplicate GPU detected' / invalid usage), the refusal itself is asserted,
    so the record shows why the multi-rank RCCL path cannot be exercised on one GPU (the shared-memory transport, blocking and
    stream-ordered, covers the solver logic; RCCL's own multi-rank transport is left to the 8-GPU node)."""
    import subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    uid = (xmamd.C.c_char * 128)()
    xmamd._chk(xmamd.lib().xm_comm_unique_id(uid))
    idf = tmp_path / "uid.bin"
    idf.write_bytes(uid.raw)
    code = textwrap.dedent(f"""
        import sys, os, json
        sys.path.insert(0, {os.path.join(root, 'xm-code_amd')!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
        import numpy as np, xmamd, xm_testlib as tl
        rank = int(sys.argv[1]); uid = open(sys.argv[2], "rb").read()
        rc = xmamd.lib().xm_comm_init(rank, 2, 0, uid, None)
        if rc != 0:
            print(json.dumps(dict(ok=False, err=xmamd.lib().xm_last_error().decode()))); sys.exit(0)
        P = tl.gen_vg(41, deg=3, sigma=1.5, seed=40)
        ctx = xmamd.Context(Q=P["Q"]); R, s, info = ctx.solve(6, 1e-9, 3.0); ctx.close()
        xmamd.lib().xm_comm_finalize()
        print(json.dumps(dict(ok=True, primal=info["primal"], rank=info["rank"], status=info["status"])))
    """)
    env = dict(os.environ, NCCL_SOCKET_IFNAME="lo", HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_DEBUG="WARN", XM_WATCHDOG_S="120")
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(idf)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0].decode())
        except subprocess.TimeoutExpired:
            p.kill(); outs.append(p.communicate()[0].decode() + "\nTIMEOUT")
    res = []
    for o_ in outs:
        js = [l for l in o_.splitlines() if l.startswith("{")]
        res.append(json.loads(js[-1]) if js else dict(ok=False, err=o_[-600:]))
    print("RCCL 2 ranks on one GPU:", res)
    if all(r["ok"] for r in res):
        P = tl.gen_vg(41, deg=3, sigma=1.5, seed=40)
        R1, s1, i1 = xmamd.solve_dense(P["Q"], 6, 1e-9, 3.0)
        assert res[0]["primal"] == res[1]["primal"] == pytest.approx(i1["primal"], rel=1e-9) and res[0]["status"] == 1
    else:
        blob = " ".join(str(r.get("err", "")) for r in res) + " ".join(outs)
        # the one documented refusal of this RCCL build: a communicator may hold each GPU only once.  A time-out, a crash or any other
        # error is a failure of this test.
        assert all(not r["ok"] for r in res) and "TIMEOUT" not in blob and ("invalid usage" in blob or "Duplicate GPU" in blob), blob[-800:]


@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_problems(xmamd, oracle, n):
    """degenerate sizes: a single camera (no free scale, zero gradient at the start), two and three cameras"""
    Q = np.diag([2.0, 3.0, 4.0]) if n == 1 else tl.gen_vg(n, deg=2, sigma=0.3, seed=n)["Q"]
    R, s, info = xmamd.solve_dense(Q, 4, 1e-9, 1.0)
    Ro, so, io = oracle.solve(Q, 4, 1e-9, 1.0, 100.0, trace=100)
    assert info["rank"] == io["rank"] and info["status"] == io["status"] == 1
    assert info["primal"] == pytest.approx(io["trace"][-1, 0], rel=1e-9, abs=1e-12)
    assert np.allclose(tl.gram(R, s), tl.gram(Ro, so), atol=1e-7)
    assert R.shape == (3 * n, 3) and s[0] == 1.0


def test_loose_tolerance_and_small_max_rank(xmamd, oracle):
    Q, exp, d = _case("synth/dense49")
    R, s, info = xmamd.solve_dense(Q, 3, 1e6, 0.0)        # gradient norm already below tol: identity start is returned
    Ro, so, io = oracle.solve(Q, 3, 1e6, 0.0, 100.0)
    assert np.array_equal(R, Ro) and info["tcg_iters"] == io["tcg_iters"] == 0 and info["status"] == io["status"]
    R2, s2, i2 = xmamd.solve_dense(Q, 2, 1e-6, 0.0)       # max_rank < 3: the staircase loop never runs (XM_main.cu:223)
    assert i2["rank"] == 2 and i2["status"] == 0 and i2["tcg_iters"] == 0


@pytest.mark.parametrize("case", [0, 1, 2])
def test_medium_view_graph_vs_recorded_oracle(xmamd, case):
    """600- and 2000-camera view-graph problems in the hard regime (small scale regulariser: hundreds of outer iterations, the
    2000-camera one needs the staircase): rank, certificate and optimum recorded from the CPU oracle (hours of CPU), dense and
    BSR3 storage on the GPU"""
    c = json.load(open(os.path.join(G, "synth", "recorded_oracle_medium.json")))["cases"][case]
    P = tl.gen_vg(c["n"], deg=c["deg"], sigma=0.05, seed=c["n"])
    for ctx in (xmamd.Context(Q=P["Q"]), xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]))):
        R, s, i = ctx.solve(5, 1e-6, c["lam"])
        ctx.close()
        assert i["rank"] == c["rank"] and i["status"] == c["status"] == 1
        assert i["primal"] == pytest.approx(c["f"], rel=1e-9)
        assert abs(i["tcg_iters"] - c["tcg"]) <= 0.15 * c["tcg"]
        assert i["min_eig"] > -1e-6


def test_venice1778_vs_recorded_oracle(xmamd):
    """The headline workload itself (BASELINE config 'Venice-1778 on one MI355X', bench.py's default): the complete staircase
    3 -> 4 -> 5 against the CPU oracle's recorded run on the same Q (tests/golden/synth/venice1778_oracle.json + the oracle's
    anchored rotations): same final rank and certificate, same optimum, rotations <= 1e-6 (north_star)."""
    fj = os.path.join(G, "synth", "venice1778_oracle.json")
    if not os.path.exists(fj):
        pytest.skip("recorded oracle run not present")
    c = json.load(open(fj))
    P = tl.gen_dense(c["n"], seed=c["seed"])
    R, s, i = xmamd.solve_dense(P["Q"], c["max_rank"], c["tol"], c["lam"])
    assert i["rank"] == c["rank"] and i["status"] == c["status"] == 1
    assert i["primal"] == pytest.approx(c["f"], rel=1e-8)
    rot, _ = tl.recover_rotations(R, s)
    assert tl.rel_fro(rot, np.load(os.path.join(G, "synth", "venice1778_oracle_rot.npy"))) < 1e-6
    # the path through the two saddle points (ranks 3 and 4) is rounding-sensitive: 3061 iterations on the oracle, 3760-4924 on the
    # GPU depending on the summation grouping; only the order of magnitude is a property of the problem
    assert 0.5 * c["tcg"] <= i["tcg_iters"] <= 2.0 * c["tcg"]


def test_rome13682_vs_recorded_oracle(xmamd):
    """BASELINE config 'Final-13682' (bench.py's Rome-scale legs): the rank-3 trust region of the 13 682-camera view-graph Q on
    the CPU oracle (dense 13.5 GB on the host, recorded once: tests/golden/synth/rome13682_oracle.json + anchored rotations)
    against the GPU solve in BSR3 storage: same optimum, rotations <= 1e-6."""
    fj = os.path.join(G, "synth", "rome13682_oracle.json")
    if not os.path.exists(fj):
        pytest.skip("recorded oracle run not present")
    c = json.load(open(fj))
    P = tl.gen_vg(c["n"], deg=c["deg"], sigma=c["sigma"], seed=c["n"], dense=False)
    ctx = xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]))
    R, s, i = ctx.solve(5, c["tol"], c["lam"])
    ctx.close()
    assert i["rank"] == 3 and i["status"] == 1
    assert i["primal"] == pytest.approx(c["f"], rel=1e-9)
    rot, _ = tl.recover_rotations(R, s)
    assert tl.rel_fro(rot, np.load(os.path.join(G, "synth", "rome13682_oracle_rot.npy"))) < 1e-6
    assert abs(i["tcg_iters"] - c["tcg"]) <= 0.2 * c["tcg"]


def test_vg100k_vs_recorded_oracle(xmamd):
    """BASELINE config 'synthetic 100k-camera Erdos-Renyi view-graph Q': the rank-3 trust region on the CPU oracle multiplying
    from the same 3x3-block CSR (oracle.trustregion_bsr, 100 s on 8 cores; recorded in tests/golden/synth/vg100k_oracle.json with
    every 8th camera's anchored rotation) against the GPU solve: same optimum, rotations <= 1e-6."""
    fj = os.path.join(G, "synth", "vg100k_oracle.json")
    if not os.path.exists(fj):
        pytest.skip("recorded oracle run not present")
    c = json.load(open(fj))
    P = tl.gen_vg(c["n"], deg=c["deg"], sigma=c["sigma"], seed=c["n"], dense=False)
    ctx = xmamd.Context(bsr=(P["rowptr"], P["colidx"], P["blocks"]))
    R, s, i = ctx.solve(5, c["tol"], c["lam"])
    ctx.close()
    assert i["rank"] == 3 and i["status"] == 1
    assert i["primal"] == pytest.approx(c["f"], rel=1e-9)
    rot, _ = tl.recover_rotations(R, s)
    sub = rot.reshape(3, c["n"], 3)[:, ::8, :]
    assert tl.rel_fro(sub, np.load(os.path.join(G, "synth", "vg100k_oracle_rot_every8.npy"))) < 1e-6
    assert abs(i["tcg_iters"] - c["tcg"]) <= 0.2 * c["tcg"]


@pytest.mark.parametrize("transport", ["shm", "ipc"])
def test_bench_two_ranks_flow(xmamd, transport):
    """bench.py exactly as the driver launches it for N = 2 (torch.distributed.run, gloo control plane, per-rank on-device
    expansion of the Rome-scale Q, replicas leg), with both ranks on the one GPU of the test box and, in place of RCCL (which
    refuses two ranks on one device), (shm) the library's shared-memory test transport / (ipc) the direct peer exchange through
    hipIpcMemHandle mappings -- the transport xm_comm_init switches to on a real node: every leg must reach the certified optimum
    the single-GPU run reaches."""
    import socket, subprocess, sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, XM_BENCH_SINGLE_DEVICE="1", **({"XM_BENCH_SHM": "1"} if transport == "shm" else {"XM_BENCH_IPC": "1"}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--full"]
    if transport == "ipc":
        env["XM_BENCH_IPC_SPIN"] = "60"       # bound of the device-side waits in this run
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)   # a hard gate: no retry, no skip (see Context::tcg_blocks)
    err = "\n".join(l for l in out.stderr.splitlines() if "amdgpu.ids" not in l and "elastic" not in l)
    assert out.returncode == 0, out.stdout[-1500:] + err[-6000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1                                            # rank 0 prints ONE JSON line
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and d["steps"] == 1 and d["scaling"] == "strong" and d["value"] > 0
    assert d["solve"]["status"] == 1 and d["solve"]["primal"] == pytest.approx(0.2844696774, rel=1e-8)
    assert d["solve"]["exchange"] == (2 if transport == "ipc" else 1)          # fused peer exchange / all-gather between the launches
    assert ("IPC" in d["transport"]) == (transport == "ipc") and d["fallback"] is None
    assert ("IPC" in d["config"]["parallelism"]) == (transport == "ipc")
    for leg in ("rome_scale", "rome_scale_dense"):
        assert d[leg]["n_gpus"] == 2 and d[leg]["status"] == 1 and d[leg]["rank"] == 3
        assert d[leg]["primal"] == pytest.approx(2879.599460014564, rel=1e-10)
    assert d["replicas"]["scaling"] == "weak" and d["replicas"]["value"] > 0


def test_bench_plain_command_needs_no_launcher(xmamd):
    """`python bench.py --gpus 2` WITHOUT torch.distributed.run: the library's single-process multi-GPU mode (xm_problem_t.n_gpus,
    one host thread per rank, direct peer-write exchange); on this 1-GPU box the two ranks are virtual devices on device 0, which
    the JSON line says.  Exit code 0 and exactly one JSON line."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["XM_WATCHDOG_S"] = "60"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-rome", "--cpu-seconds", "0"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and d["solve"]["status"] == 1 and d["value"] > 0
    assert d["solve"]["exchange"] == (2 if xmamd.device_count() >= 2 or tl.virtual_ranks_wait_on_device(2) else 1)
    assert d["solve"]["primal"] == pytest.approx(0.2844696774, rel=1e-8)
    assert "ONE process" in d["config"]["parallelism"]
    assert d["transport"].startswith("direct peer writes") and d["fallback"] is None
    assert not {"rome_scale", "rome_scale_dense", "rccl_leg", "replicas"} & set(d)     # a plain run: the headline alone (legs: --full)
    if xmamd.device_count() < 2:
        assert "VIRTUAL devices" in d["config"]["devices"]


# ---------------------------------------------------------------------------------------------- XM^2 loop
@pytest.mark.parametrize("storage", ["dense", "bsr", "sell"])
def test_xm2_reweighting_on_resident_context(xmamd, monkeypatch, storage):
    """The reference's XM^2 outlier loop (3_test_colmap_glomap.py:299-351: residual per observation, np.percentile(error, 90) filter
    at :321, rebuild Q, solve again) on a RESIDENT context: residuals per edge from the device, the filtered weights go back as
    one vector, Q is rewritten on the device in its own storage (dense / block-CSR / sliced-ELL copy) and the second solve starts
    from the first one's point (XM_MODE_REBUTTLE + R_ini).  Checked against a cold solve of the filtered problem built from
    scratch: rotations within 1e-6, same optimum; the warm solve needs fewer tCG iterations than the cold one."""
    import time
    n, lam = 600, 20.0
    edges, M, bad, Rs = tl.vg_measurements(n, deg=20, sigma=0.02, seed=77, outlier_frac=0.03)
    ne = edges.shape[0]
    w0 = np.ones(ne)
    rowptr, colidx, blocks = tl.vg_assemble(n, edges, M, w0)
    Qd = tl.bsr_to_dense(n, rowptr, colidx, blocks)
    ctx = xmamd.Context(Q=Qd) if storage == "dense" else xmamd.Context(bsr=(rowptr, colidx, blocks), tuning=(dict(sell=1) if storage == "sell" else None))
    ctx.attach_edges(edges[:, 0], edges[:, 1], M)
    R1, s1, i1 = ctx.solve(5, 1e-8, lam)
    assert i1["status"] == 1
    res = ctx.edge_residuals()
    Y = tl.scale_rows(R1, s1).reshape(n, 3, -1)
    ref = np.sum((Y[edges[:, 0]] - M @ Y[edges[:, 1]]) ** 2, axis=(1, 2))
    assert np.allclose(res, ref, rtol=1e-11, atol=1e-13)
    assert np.sum(res) == pytest.approx(i1["primal"] - lam * np.sum((s1[1:] ** 2 - 1) ** 2), rel=1e-9)    # the residuals ARE the data term
    thr = np.percentile(res, 90)                                        # the reference's filter
    w1 = (res <= thr).astype(float)
    assert w1[bad].mean() < 0.05 and bad[w1 == 0].mean() > 0.25           # every planted outlier is among the 10 % removed
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    keep = w1 > 0     # (the reference re-checks connectivity after its filter, checklandmarks at 3_test_colmap_glomap.py:327; this instance stays connected)
    assert connected_components(coo_matrix((np.ones(keep.sum()), (edges[keep, 0], edges[keep, 1])), shape=(n, n)), directed=False)[0] == 1
    t0 = time.perf_counter(); ctx.set_edge_weights(w1); t_upd = time.perf_counter() - t0
    t0 = time.perf_counter()
    R2, s2, i2 = ctx.solve(5, 1e-8, lam, mode=xmamd.MODE_REBUTTLE, s_ini=s1, R_ini=R1)
    t_warm = time.perf_counter() - t0
    ctx.close()
    # cold reference: the filtered problem assembled from scratch on the host, fresh context, identity start
    rp2, ci2, bl2 = tl.vg_assemble(n, edges, M, w1)
    assert np.array_equal(rp2, rowptr) and np.array_equal(ci2, colidx)
    cold = xmamd.Context(Q=tl.bsr_to_dense(n, rp2, ci2, bl2)) if storage == "dense" else xmamd.Context(bsr=(rp2, ci2, bl2))
    t0 = time.perf_counter()
    Rc, sc, ic = cold.solve(5, 1e-8, lam)
    t_cold = time.perf_counter() - t0
    cold.close()
    assert i2["status"] == ic["status"] == 1 and i2["rank"] == ic["rank"]
    assert i2["primal"] == pytest.approx(ic["primal"], rel=1e-9)
    assert tl.rotation_parity(R2, s2, Rc, sc) < 1e-6
    assert i2["tcg_iters"] < ic["tcg_iters"]
    rot, _ = tl.recover_rotations(R2, s2)
    gt = np.concatenate([Rs[0] @ Rs[k].T for k in range(n)], axis=1)
    assert tl.rel_fro(rot, gt) < 0.02                                    # and the filtered solve recovers the planted rotations
    print(f"XM^2 [{storage}] n={n} ne={ne}: device re-weighting {t_upd*1e3:.2f} ms; second solve warm {t_warm*1e3:.1f} ms / {i2['tcg_iters']} tCG its "
          f"vs cold {t_cold*1e3:.1f} ms / {ic['tcg_iters']} tCG its")


def test_xm2_round_trip_through_XM_module(xmamd):
    """XM.solve_array(..., mode=2, s_ini, R_ini): the warm re-solve of an unchanged problem converges in far fewer tCG iterations
    than the cold one and returns the same optimum (the reference's solve_rebuttle surface, with R_ini honoured)"""
    XM = xmamd.import_XM()
    Q = tl.gen_vg(300, deg=8, sigma=0.1, seed=3)["Q"]
    R1, s1, i1 = XM.solve_array(Q, 5, 1e-8, 10.0, 1000.0)
    R2, s2, i2 = XM.solve_array(Q, 5, 1e-8, 10.0, 1000.0, mode=2, s_ini=s1, R_ini=R1)
    assert i1["status"] == i2["status"] == 1 and i2["primal"] == pytest.approx(i1["primal"], rel=1e-10)
    assert i2["tcg_iters"] < 0.25 * i1["tcg_iters"] and tl.rotation_parity(R2, s2, R1, s1) < 1e-7


# ---------------------------------------------------------------------------------------------- matrix-free Q
def _simple2_obs():
    Z = np.load(os.path.join(G, "simple2", "obs.npz"))
    return Z["cam"], Z["lm"], Z["p"], Z["w"]


@pytest.mark.parametrize("o", [1, 3, 4, 5, 8])
def test_matrix_free_product_equals_dense_Q(xmamd, o):
    """Q * W applied as the factor chain on the observation list of SIMPLE2 (the arguments the reference's own pipeline hands to
    create_matrix, tests/golden/make_simple2_obs.py) against the dense Q.bin create_matrix wrote from them"""
    Q = tl.load_bin(os.path.join(G, "simple2", "Q.bin"))
    W = np.random.default_rng(o).standard_normal((Q.shape[0], o))
    ctx = xmamd.Context(obs=_simple2_obs())
    got = ctx.qw(W, 2.0)
    ctx.close()
    assert tl.rel_fro(got, 2.0 * (Q @ W)) < 1e-11


def test_matrix_free_device_assembly_equals_host_assembly(xmamd):
    """round 4: the weight-dependent factors (Q1, c, Q2, 1/Q3, the reduced camera Laplacian row by row in LDS) are assembled on the device;
    the host assembly stays for observation lists that name a (camera, landmark) pair twice.  Same product from both (a scene with hub
    landmarks and zero weights), from a list WITH a duplicated pair (host path taken automatically), and against the numpy restatement."""
    S = tl.gen_scene(300, 4000, 6, seed=9)
    w = S["w"].copy(); w[::11] = 0.0
    W = np.random.default_rng(3).standard_normal((900, 3))
    ref = tl.schur_qw_numpy(S["cam"], S["lm"], S["p"], w, W)
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], w))
    dev = ctx.qw(W)
    ctx.close()
    assert tl.rel_fro(dev, ref) < 1e-10
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], w), tuning=dict(schur_host_assembly=1))     # the reference's route: host assembly
    host = ctx.qw(W)
    ctx.close()
    assert tl.rel_fro(dev, host) < 1e-11
    cam2 = np.concatenate([S["cam"], S["cam"][5:6]]); lm2 = np.concatenate([S["lm"], S["lm"][5:6]])        # observation 5 named twice
    p2 = np.concatenate([S["p"], S["p"][5:6] + 0.01]); w2 = np.concatenate([w, [0.7]])
    c2 = xmamd.Context(obs=(cam2, lm2, p2, w2))
    assert tl.rel_fro(c2.qw(W), tl.schur_qw_numpy(cam2, lm2, p2, w2, W)) < 1e-10
    c2.close()


def test_matrix_free_solve_matches_dense_solve(xmamd):
    """SIMPLE2 solved matrix-free (XM_STORAGE_SCHUR: Q never formed) against the solve of the dense Q the reference's create_matrix
    wrote: same optimum, certificate and rotations <= 1e-6 (north_star), and against the golden of the dense path"""
    Q, exp, d = _case("simple2")
    ctx = xmamd.Context(obs=_simple2_obs())
    R, s, info = ctx.solve(exp["max_rank"], exp["tol"], exp["lam"])
    ctx.close()
    Rd, sd, idn = xmamd.solve_dense(Q, exp["max_rank"], exp["tol"], exp["lam"])
    assert info["rank"] == idn["rank"] == exp["rank"] and info["status"] == idn["status"] == 1
    # the optimum value is 5e-2 against |Q| ~ 1e3: the factor chain and create_matrix's dense Q agree to 2e-13 |Q| (make_simple2_obs.py),
    # i.e. to ~1e-10 absolute in f -- the rotations are what must agree (measured 8e-11)
    assert info["primal"] == pytest.approx(idn["primal"], rel=1e-8)
    assert tl.rotation_parity(R, s, Rd, sd) < 1e-6
    rot, _ = tl.recover_rotations(R, s)
    assert tl.rel_fro(rot, np.load(os.path.join(d, "rot_anchor.npy"))) < 1e-6            # golden of the dense path (north_star: <= 1e-6)
    assert abs(info["tcg_iters"] - idn["tcg_iters"]) <= 5
    cn = tl.certificate_numpy(Q, R, s, exp["lam"])                       # certified from scratch against the DENSE matrix
    # tol = 1e-16 is never reached: the run ends by the tCG's residual test (stop reason 5) after a last step whose decrease (~|grad|^2 =
    # 7e-11) is below the 1e-10 to which the factor chain knows f -- whether that step is accepted (|grad| 3e-8, gap 3e-11: the dense run) or
    # rejected (|grad| 9e-6, gap 8e-6) is decided by the last bits of f; both are the same point to the 1e-6 asked of the rotations
    assert cn["min_eig"] > -1e-7 and abs(cn["gap"]) < 2e-5 and cn["stationarity"] < 1e-5


def test_matrix_free_recover_translations_and_landmarks(xmamd):
    """xm_ctx_recover_tp (recover_XM's t_est / p_est without Abar) on SIMPLE2: (1) on the reference's own anchored rotations and
    scales it reproduces the reference's t_est / p_est (golden tp.npz) to 1e-9; (2) the whole chain on the device — matrix-free
    solve, xm_recover_rotations, xm_ctx_recover_tp — agrees with the numpy restatement on the same rotations to 1e-9 and with the
    reference's result to the accuracy of the reference's own run (its script solves to tol 1e-1 only: 2_test_creatematrix.py:149,
    so its rotations sit 1e-3 from the optimum the tight solve reaches); (3) a dense-storage context refuses (no observations)."""
    T = np.load(os.path.join(G, "simple2", "tp.npz"))
    _, exp, _ = _case("simple2")
    ctx = xmamd.Context(obs=_simple2_obs())
    t, p = ctx.recover_tp(T["R_real"], T["s_real"])
    st, sp = np.abs(T["t_est"]).max(), np.abs(T["p_est"]).max()
    assert np.abs(t - T["t_est"]).max() < 1e-9 * st and np.abs(p - T["p_est"]).max() < 1e-9 * sp and np.all(t[:, 0] == 0.0)
    R, s, info = ctx.solve(exp["max_rank"], exp["tol"], exp["lam"])
    rot, sc, _ = xmamd.recover_rotations(R, s)
    t2, p2 = ctx.recover_tp(rot, sc)
    res = ctx.edge_residuals()                 # |s_i R_i p + t_i - P_l|^2 per observation: their weighted sum IS the objective (lam = 0)
    ctx.close()
    # (the objective is 5e-2 against |Q| ~ 1e3: the quadratic form carries ~1e-9 of cancellation, the residual sum does not)
    assert float(np.sum(_simple2_obs()[3].reshape(-1) * res)) == pytest.approx(info["primal"], rel=1e-7)
    obs = _simple2_obs()
    tn, pn = tl.schur_tp_numpy(obs[0], obs[1], obs[2], obs[3], rot, sc)
    assert np.abs(t2 - tn).max() < 1e-9 * st and np.abs(p2 - pn).max() < 1e-9 * sp
    assert tl.rel_fro(rot, T["R_real"]) < 5e-3 and np.abs(sc - T["s_real"]).max() < 5e-3
    assert np.abs(t2 - T["t_est"]).max() < 1e-2 * st and np.abs(p2 - T["p_est"]).max() < 1e-2 * sp
    Q = tl.load_bin(os.path.join(G, "simple2", "Q.bin"))
    cd = xmamd.Context(Q=Q)
    cd.n_landmarks = 1
    with pytest.raises(xmamd.XmError):
        cd.recover_tp(T["R_real"], T["s_real"])
    cd.close()


@pytest.mark.parametrize("n", [1, 5, 64, 65, 200, 777, 1500])
def test_spd_inverse_on_device(xmamd, n):
    """blocked Cholesky + triangular solves (xm_dense_la.hip, set-up of the matrix-free storage) against numpy: a graph-Laplacian-like
    SPD matrix (what the reduced camera Laplacian is), sizes around the 64-row block boundary"""
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, n + 3))
    A = B @ B.T + n * np.diag(rng.uniform(0.5, 2.0, n))
    X = xmamd.spd_inverse(A)
    assert tl.rel_fro(X, np.linalg.inv(A)) < 1e-11 and np.abs(X - X.T).max() <= 1e-12 * np.abs(X).max()
    assert np.abs(X @ A - np.eye(n)).max() < 1e-10
    with pytest.raises(xmamd.XmError):
        xmamd.spd_inverse(-np.eye(max(n, 2)))


def test_matrix_free_synthetic_scene(xmamd):
    """a synthetic scene (random cameras and landmarks, exact observations + noise): matrix-free product and solve against the
    dense Schur complement assembled in numpy (tl.schur_dense)"""
    rng = np.random.default_rng(7)
    N, M = 60, 500
    Rs = tl.haar_so3(rng, N); ts = rng.standard_normal((N, 3)) * 2; P = rng.standard_normal((M, 3)) * 3
    vis = rng.random((N, M)) < 0.25
    vis[:, :3] = True                                                    # a few landmarks seen by everybody keep the graph connected
    cam, lm = np.nonzero(vis)
    p = np.einsum("eba,eb->ea", Rs[cam], P[lm] - ts[cam]) + 0.01 * rng.standard_normal((cam.size, 3))     # camera-frame points
    w = rng.uniform(0.5, 1.5, cam.size)
    Q = tl.schur_dense(cam, lm, p, w)
    ctx = xmamd.Context(obs=(cam, lm, p, w))
    W = rng.standard_normal((3 * N, 3))
    assert tl.rel_fro(ctx.qw(W), Q @ W) < 1e-10
    R, s, info = ctx.solve(5, 1e-8, 0.0)
    ctx.close()
    Rd, sd, idn = xmamd.solve_dense(Q, 5, 1e-8, 0.0)
    assert info["status"] == idn["status"] == 1 and info["rank"] == idn["rank"]
    assert info["primal"] == pytest.approx(idn["primal"], rel=1e-8) and tl.rotation_parity(R, s, Rd, sd) < 1e-6
    rot, _ = tl.recover_rotations(R, s)                                  # and the planted cameras come back (noise level)
    gt = np.concatenate([Rs[0].T @ Rs[k] for k in range(N)], axis=1)
    assert min(tl.rel_fro(rot, gt), tl.rel_fro(rot, np.concatenate([Rs[0] @ Rs[k].T for k in range(N)], axis=1))) < 0.05


def test_matrix_free_symmetric_reduced_inverse(xmamd):
    """large scenes apply VT^-1 with the half-traffic symmetric kernel (upper triangle only, from xm_tuning_t.sym_min_rows rows on);
    forced here on a 300-camera scene: product (o = 3, 4 symmetric kernel; o = 5 general kernel) against the numpy restatement, and
    the solve against the general-kernel path"""
    S = tl.gen_scene(300, 6000, 5, seed=11)
    outs = []
    for rows in (1, 1000000000):
        ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]), tuning=dict(sym_min_rows=rows))
        errs = []
        for o in (3, 4, 5):
            W = np.random.default_rng(o).standard_normal((900, o))
            errs.append(tl.rel_fro(ctx.qw(W), tl.schur_qw_numpy(S["cam"], S["lm"], S["p"], S["w"], W)))
        R, s, info = ctx.solve(5, 1e-8, 0.0)
        ctx.close()
        outs.append(dict(errs=np.array(errs), R=R, s=s, primal=info["primal"], rank=info["rank"], status=info["status"]))
    assert outs[0]["errs"].max() < 1e-10 and outs[1]["errs"].max() < 1e-10
    assert outs[0]["status"] == outs[1]["status"] == 1 and outs[0]["rank"] == outs[1]["rank"]
    assert outs[0]["primal"] == pytest.approx(outs[1]["primal"], rel=1e-8)
    assert tl.rotation_parity(outs[0]["R"], outs[0]["s"], outs[1]["R"], outs[1]["s"]) < 1e-6


def test_matrix_free_venice_size_scene(xmamd):
    """a Venice-size synthetic scene (1778 cameras, 200 k landmarks, 1.2 M observations, three landmarks seen by every camera; the
    dense Q would be 228 MB and O(N^2 M) to build): the matrix-free product against the numpy / scipy.sparse restatement of the same
    chain, symmetry of the operator, and a certified solve that recovers the planted rotations"""
    S = tl.gen_scene(1778, 200000, 6, seed=2)
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]))
    rng = np.random.default_rng(0)
    W = rng.standard_normal((3 * S["n"], 3)); U = rng.standard_normal((3 * S["n"], 3))
    Y = ctx.qw(W)
    assert tl.rel_fro(Y, tl.schur_qw_numpy(S["cam"], S["lm"], S["p"], S["w"], W)) < 1e-9
    assert abs(np.sum(U * Y) - np.sum(ctx.qw(U) * W)) < 1e-9 * abs(np.sum(U * Y))
    R, s, info = ctx.solve(5, 1e-6, 0.0)
    ctx.close()
    assert info["status"] == 1 and info["min_eig"] > -1e-6 and tl.stiefel_defect(R) < 1e-12
    rot, _ = tl.recover_rotations(R, s)
    Rs = S["R_star"]
    gt = np.concatenate([Rs[0].T @ Rs[k] for k in range(S["n"])], axis=1)
    assert tl.rel_fro(rot, gt) < 0.02


def test_matrix_free_cg_form_equals_the_dense_inverse(xmamd):
    """SURVEY 8f N2 without the (N-1)^2 inverse: the reduced camera Laplacian is applied by preconditioned CG inside every product
    (xm_tuning_t.schur_solver = 2; Jacobi preconditioner, tolerance 1e-13, no N^2 array).  Products and whole solves against the
    dense-inverse form (schur_solver = 1) on the reference's own scene (SIMPLE2: the observation list its create_matrix takes) and on the
    Venice-size synthetic scene; both certify, optimum and rotations agree; the inner solves converge (no product at the iteration cap)."""
    d = os.path.join(tl.GOLDEN, "simple2")
    z = np.load(os.path.join(d, "obs.npz"))
    scenes = [("simple2", (z["cam"], z["lm"], z["p"], z["w"]), 1e-9, 0.0),
              ("venice", None, 1e-9, 0.0)]
    S = tl.gen_scene(1778, 200000, 6, seed=2)
    scenes[1] = ("venice", (S["cam"], S["lm"], S["p"], S["w"]), 1e-9, 0.0)   # (1e-9: two paths that stop at |grad| < 1e-6 end ~2e-8 apart, whatever the form)
    for name, obs, tol, lam in scenes:
        n = int(obs[0].max()) + 1
        out = {}
        for solver in (1, 2):
            # (inner solves of the Hessian products as tight as all others: this test is about the FORM; the default -- 1e-9 inside the tCG -- takes
            # another path to the same optimum and is compared at the solve's own tolerance in test_matrix_free_cg_batches_do_not_change_the_iteration)
            ctx = xmamd.Context(obs=obs, tuning=dict(schur_solver=solver, schur_pcg_hess_digits=13))
            assert ctx.schur_info()["cg"] == (solver == 2)
            prods = [ctx.qw(np.random.default_rng(o).standard_normal((3 * n, o))) for o in (1, 3, 4, 5)]
            R, s, info = ctx.solve(5, tol, lam)
            si = ctx.schur_info()
            ctx.close()
            out[solver] = (prods, R, s, info, si)
        for a, b in zip(out[1][0], out[2][0]):
            assert tl.rel_fro(b, a) < 1e-10, name
        i1, i2 = out[1][3], out[2][3]
        assert i1["status"] == i2["status"] == 1 and i1["rank"] == i2["rank"], name
        assert i2["primal"] == pytest.approx(i1["primal"], rel=1e-8)
        # (the optimum agrees to 1e-8 relative above; the rotations to 1e-7: on the synthetic scene the dense-inverse run ends by the reference's
        # "delta is too small" rule -- its O(N^3) inverse applies VT^-1 to ~1e-12 only, and the trust region notices -- 5e-10 in f above the point
        # the CG form reaches with stop reason 5)
        assert tl.rotation_parity(out[2][1], out[2][2], out[1][1], out[1][2]) < 1e-7
        si = out[2][4]
        assert si["capped"] == 0 and si["last_relres"] <= 1e-12 and si["products"] > 4
        assert si["inner_iters"] / si["products"] < 40, si            # well-connected co-visibility: 11-15 iterations per product (numpy emulation)
    if True:   # SIMPLE2 product against the Q the reference's create_matrix wrote
        Q = tl.load_bin(os.path.join(d, "Q.bin"))
        ctx = xmamd.Context(obs=scenes[0][1], tuning=dict(schur_solver=2))
        W = np.random.default_rng(7).standard_normal((Q.shape[0], 3))
        assert tl.rel_fro(ctx.qw(W), Q @ W) < 1e-9
        ctx.close()


def test_matrix_free_cg_batches_do_not_change_the_iteration(xmamd):
    """the inner CG of the matrix-free product is enqueued in batches and topped up after a look at the state word; a top-up batch used to
    repeat the direction update the closing launch of the previous batch had already applied (p = z + beta (z + beta p): no conjugate
    direction).  A context whose first batch is one iteration long (xm_tuning_t.schur_pcg_first: every product is topped up at
    least once) must need exactly the iterations of one that guesses generously, and produce the same bits; inside the tCG the Hessian
    products stop at 1e-9 (schur_pcg_hess_digits) and take fewer inner iterations than the gradient products for the same optimum"""
    S = tl.gen_scene(600, 60000, 6, seed=5)
    obs = (S["cam"], S["lm"], S["p"], S["w"])
    n = 600
    W = [np.random.default_rng(10 + o).standard_normal((3 * n, o)) for o in (3, 4, 1)]
    res = {}
    for first in (1, 60):
        ctx = xmamd.Context(obs=obs, tuning=dict(schur_solver=2, schur_pcg_first=first))
        Y = [ctx.qw(w) for w in W]
        si = ctx.schur_info()
        ctx.close()
        res[first] = (Y, si)
    (Ya, sa), (Yb, sb) = res[1], res[60]
    assert sa["capped"] == sb["capped"] == 0 and sa["products"] == sb["products"] == 3
    assert sa["inner_iters"] == sb["inner_iters"], (sa, sb)
    for a, b in zip(Ya, Yb):
        assert np.array_equal(a, b)
    lam = 1.5 * float(np.sum(S["w"] * np.sum(S["p"] ** 2, axis=1)) / (3 * n))
    out = {}
    for digits in (13, 0):
        ctx = xmamd.Context(obs=obs, tuning=dict(schur_solver=2, schur_pcg_hess_digits=digits))
        R, s, info = ctx.solve(5, 1e-8, lam)
        out[digits] = (R, s, info, ctx.schur_info())
        ctx.close()
    (R13, s13, i13, q13), (R9, s9, i9, q9) = out[13], out[0]
    assert i13["status"] == i9["status"] == 1 and i13["rank"] == i9["rank"]
    assert i9["primal"] == pytest.approx(i13["primal"], rel=1e-9)
    assert tl.rotation_parity(R9, s9, R13, s13) < 1e-7
    assert q9["capped"] == q13["capped"] == 0
    assert q9["inner_iters"] / q9["products"] < 0.85 * q13["inner_iters"] / q13["products"], (q9, q13)


def test_matrix_free_50k_cameras_without_any_n_squared_array(xmamd):
    """a 50 000-camera synthetic scene (1.5 M landmarks, ~9 M observations): beyond the dense inverse's limit (kSchurMaxCams = 40 000;
    8 N^2 = 20 GB and an O(N^3) factorisation) the matrix-free storage selects the CG form by itself.  Set-up in seconds (dominated by
    the host's list building), a certified solve, planted rotations recovered, operator symmetric"""
    import time
    N = 50000
    S = tl.gen_scene(N, 1500000, 6, seed=50)
    t0 = time.time()
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S["w"]))
    t_setup = time.time() - t0
    assert ctx.schur_info()["cg"] and ctx.product_kind(3) == "schur"
    rng = np.random.default_rng(0)
    W = rng.standard_normal((3 * N, 3)); U = rng.standard_normal((3 * N, 3))
    Y = ctx.qw(W)
    assert abs(np.sum(U * Y) - np.sum(ctx.qw(U) * W)) < 1e-9 * abs(np.sum(U * Y))
    lam = 1.5 * float(np.sum(S["w"] * np.sum(S["p"] ** 2, axis=1)) / (3 * N))     # at the data term's own scale (scripts/kbench_schur.py)
    R, s, info = ctx.solve(5, 1e-6, lam)
    si = ctx.schur_info()
    ctx.close()
    print(f"50k cameras: set-up {t_setup:.2f} s, solve {info['seconds']:.2f} s, tcg {info['tcg_iters']}, CG iterations per product {si['inner_iters'] / max(si['products'], 1):.1f}")
    assert t_setup < 20.0                                   # (host list building included; the device part is milliseconds)
    assert info["status"] == 1 and si["capped"] == 0
    rot, _ = tl.recover_rotations(R, s)
    Rs = S["R_star"]
    gt = np.concatenate([Rs[0].T @ Rs[k] for k in range(N)], axis=1)
    assert tl.rel_fro(rot, gt) < 0.02


def test_xm2_on_matrix_free_context(xmamd):
    """The reference's XM^2 loop on its OWN kind of Q (observations -> Schur complement), entirely on the resident matrix-free
    context: solve, per-observation residuals |p^T U_i + t_i - P_l|^2 from the device (checked against the numpy restatement and
    against sum_e w_e res_e == primal), np.percentile(error, 90) filter (3_test_colmap_glomap.py:321), weights handed back as one
    vector (Q1, V1, Q3 rebuilt, the reduced camera Laplacian re-inverted on the device), warm re-solve -- against a cold solve of
    the filtered observation list in a fresh context"""
    import time
    S = tl.gen_scene(400, 30000, 6, seed=11)
    cam, lm, p, w = S["cam"], S["lm"], S["p"].copy(), S["w"]
    rng = np.random.default_rng(5)
    bad = rng.random(cam.size) < 0.03
    p[bad] += rng.standard_normal((int(bad.sum()), 3))                    # planted outlier observations (100x the inlier noise)
    lam = cam.size / S["n"]                                               # the reference's choice, 3_test_colmap_glomap.py:287: without it
    ctx = xmamd.Context(obs=(cam, lm, p, w))                              # the outliers shrink every free scale to 0.64 against the anchor
    R1, s1, i1 = ctx.solve(5, 1e-8, lam)
    assert i1["status"] == 1
    res = ctx.edge_residuals()
    U = tl.scale_rows(R1, s1)
    assert np.allclose(res, tl.schur_residuals_numpy(cam, lm, p, w, U), rtol=1e-8, atol=1e-10 * res.max())
    assert np.sum(w * res) == pytest.approx(i1["primal"] - lam * np.sum((s1[1:] ** 2 - 1) ** 2), rel=1e-9)   # the residuals ARE the data term
    err = w * res
    keep = err <= np.percentile(err, 90)
    assert bad[~keep].mean() > 0.25 and keep[bad].mean() < 0.1             # the planted outliers are among the 10 % removed
    assert np.bincount(cam, weights=keep.astype(float)).min() > 100        # and every camera keeps most of its observations
    w1 = w * keep
    t0 = time.perf_counter(); ctx.set_edge_weights(w1); t_upd = time.perf_counter() - t0
    t0 = time.perf_counter()
    R2, s2, i2 = ctx.solve(5, 1e-8, lam, mode=xmamd.MODE_REBUTTLE, s_ini=s1, R_ini=R1)
    t_warm = time.perf_counter() - t0
    W = rng.standard_normal((3 * S["n"], 3))
    _, lmk = np.unique(lm[keep], return_inverse=True)                      # the filtered list, landmarks renumbered: same Q
    assert tl.rel_fro(ctx.qw(W), tl.schur_qw_numpy(cam[keep], lmk, p[keep], w[keep], W)) < 1e-9
    ctx.close()
    cold = xmamd.Context(obs=(cam[keep], lmk, p[keep], w[keep]))
    t0 = time.perf_counter(); Rc, sc, ic = cold.solve(5, 1e-8, lam); t_cold = time.perf_counter() - t0
    cold.close()
    assert i2["status"] == ic["status"] == 1 and i2["rank"] == ic["rank"]
    assert i2["primal"] == pytest.approx(ic["primal"], rel=1e-8) and tl.rotation_parity(R2, s2, Rc, sc) < 1e-6
    assert i2["tcg_iters"] < ic["tcg_iters"]
    rot, _ = tl.recover_rotations(R2, s2)
    Rs = S["R_star"]
    assert tl.rel_fro(rot, np.concatenate([Rs[0].T @ Rs[k] for k in range(S["n"])], axis=1)) < 0.02
    print(f"XM^2 [matrix-free] N={S['n']} obs={cam.size}: re-weighting incl. device re-inversion {t_upd*1e3:.1f} ms; second solve warm "
          f"{t_warm*1e3:.1f} ms / {i2['tcg_iters']} tCG its vs cold {t_cold*1e3:.1f} ms / {ic['tcg_iters']} tCG its")
