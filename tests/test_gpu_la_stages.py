"""The dense float64 linear algebra of xm_dense_la.hip stage by stage through the test export xm_la_probe: every host function on its own,
against the references, families and bounds of tests/xm_la_stages.py (derived there, not measured).  Integer-valued data must come back
bit for bit; real-valued data within the componentwise rounding-error bound of the operation; padding, sentinels and the info word must be
as the headers say."""
import numpy as np
import pytest

import xm_la_stages as la

pytestmark = pytest.mark.gpu
S = la.SENTINEL


@pytest.fixture(scope="module")
def gpu(xmamd):
    xmamd.require_gpu()
    return xmamd


# ---- one call each ---------------------------------------------------------------------------------------------------------------------
def dev_gemm(gpu, oa, ob, c0, ta, tb, lower_only, pad):
    """op(A) (m x k), op(B) (k x n), C0 (m x n) -> the whole C buffer; NaN in the padding of A and B, the sentinel in C's"""
    (m, k), n = oa.shape, ob.shape[1]
    A = la.pack(oa.T if ta else oa, (k if ta else m) + pad)
    B = la.pack(ob.T if tb else ob, (n if tb else k) + pad)
    C = la.pack(c0, m + pad, S)
    gpu.la_probe("gemm_sub", a=A, b=B, c=C, m=m, n=n, k=k, ta=ta, tb=tb, lower_only=lower_only, lda=A.shape[0], ldb=B.shape[0], ldc=C.shape[0])
    return C


def dev_cholesky(gpu, A, pad=0, info=0):
    """A with whatever it holds above the diagonal -> (buffer, info)"""
    n = A.shape[0]
    buf = la.pack(A, n + pad, S)
    return buf, gpu.la_probe("cholesky", a=buf, n=n, lda=n + pad, info=info)


def dev_substitute(gpu, L, rhs, pad=0, info=0):
    n = L.shape[0]
    Lb = la.pack(L); X = la.pack(rhs, n + pad, S)
    info = gpu.la_probe("substitute", a=Lb, c=X, n=n, lda=n, ldc=n + pad, nrhs=X.shape[1], info=info)
    assert la.same_bits(Lb, L)                                                   # the factor is an input
    return X, info


def dev_inverse(gpu, A):
    """-> (factor buffer, X buffer, ok); X goes up filled with the sentinel"""
    n = A.shape[0]
    F = la.pack(A); X = np.full((n, n), S, order="F")
    info = gpu.la_probe("inverse", a=F, c=X, n=n, lda=n, ldc=n, info=3)
    assert info in (0, 1)
    return F, X, info == 0


def dev_layout(gpu, X, pad=0):
    n = X.shape[0]
    Xb = la.pack(X); dst = np.full((n, n + pad), S)                              # row-major, n rows of ldd
    gpu.la_probe("layout", a=Xb, c=dst, n=n, lda=n, ldc=n + pad)
    assert la.same_bits(Xb, X)
    return dst


def dev_rank1(gpu, A, u, q):
    n = A.shape[0]
    buf = la.pack(A); ub = la.pack(u)
    gpu.la_probe("rank1_sub", a=buf, b=ub, n=n, lda=n, q=q)
    return buf


def upper_blocks_ok(buf, n, before=S):
    """above the diagonal: zeros inside the 64 x 64 diagonal blocks, the bits that went up elsewhere"""
    r, c = np.triu_indices(n, 1)
    inside = r // la.KB == c // la.KB
    kept = buf[r[~inside], c[~inside]]
    return bool(np.all(la.bits(buf[r[inside], c[inside]]) == 0)) and la.same_bits(kept, np.full(kept.shape, before))


# ---- GEMM_SUB ----------------------------------------------------------------------------------------------------------------------------
MS = (1, 63, 64, 65, 129)
KS = (1, 3, 15, 16, 17, 31, 32, 33, 80)


def gemm_cases(ta, tb):
    """27 launches per (ta, tb): every k with lower_only 0 and 1 on integer data, every k once more on real data; m and n walk through MS
    at different strides, the leading dimensions alternate between the rows and the rows + 5"""
    cases = []
    shift = 2 * ta + tb
    for lo in (0, 1):
        for i, k in enumerate(KS):
            m = MS[(i + shift + 2 * lo) % 5]
            n = m if lo else MS[(2 * i + shift + 1) % 5]
            cases.append((m, n, k, lo, 5 * ((i + lo) % 2), "int"))
    for i, k in enumerate(KS):
        lo = (i + shift) % 2
        m = MS[(3 * i + shift + 1) % 5]
        n = m if lo else MS[(i + 2 * shift + 3) % 5]
        cases.append((m, n, k, lo, 5 * ((i + 1) % 2), "real"))
    return cases


def test_gemm_cases_cover_the_shapes():
    seen = [c for ta in (0, 1) for tb in (0, 1) for c in gemm_cases(ta, tb)]
    assert len(seen) == 108
    for ta in (0, 1):
        for tb in (0, 1):
            cs = gemm_cases(ta, tb)
            for kind in ("int", "real"):
                assert {c[2] for c in cs if c[5] == kind} == set(KS)
            assert {c[0] for c in cs} == set(MS) and {c[1] for c in cs} == set(MS) and {c[3] for c in cs} == {0, 1} and {c[4] for c in cs} == {0, 5}
            assert {(c[2], c[3]) for c in cs if c[5] == "int"} == {(k, lo) for k in KS for lo in (0, 1)}


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_sub(gpu, ta, tb):
    for m, n, k, lo, pad, kind in gemm_cases(ta, tb):
        what = f"gemm_sub ta {ta} tb {tb} m {m} n {n} k {k} lower_only {lo} pad {pad} {kind}"
        oa, ob, c0 = (la.int_operands if kind == "int" else la.real_operands)(m, n, k, 7 * k + m)
        C = dev_gemm(gpu, oa, ob, c0, ta, tb, lo, pad)
        assert la.same_bits(C[m:], np.full((pad, n), S)), what                   # the padding of C keeps its bits
        t = np.arange(m) // la.KB
        dead = (t[:, None] < (np.arange(n) // la.KB)[None, :]) if lo else np.zeros((m, n), dtype=bool)
        live = ~dead
        assert not np.isnan(C[:m][live]).any(), what                             # no NaN of a padding row reaches a result
        if kind == "int":
            assert la.same_bits(C[:m][live], (c0 - oa @ ob)[live]), what
        else:
            ref = la.pack(c0)
            la.gemm_sub(m, n, k, la.pack(oa), 0, la.pack(ob), 0, ref, lo)
            assert la.check_gemm(what, C[:m], oa, ob, c0, lo, ref), what


@pytest.mark.parametrize("m", [129, 192])
def test_gemm_sub_lower_only_leaves_the_upper_tiles(gpu, m):
    """C goes up as the sentinel everywhere above the diagonal tiles: those tiles keep it, the diagonal tiles are written whole"""
    oa, ob, c0 = la.real_operands(m, m, 33, m)
    t = np.arange(m) // la.KB
    upper = t[:, None] < t[None, :]
    c0 = np.where(upper, S, c0)
    C = dev_gemm(gpu, oa, ob, c0, 0, 1, 1, 5)
    assert la.same_bits(C[:m][upper], np.full(int(upper.sum()), S)) and la.same_bits(C[m:], np.full((5, m), S))
    full = dev_gemm(gpu, oa, ob, np.where(upper, 0.0, c0), 0, 1, 0, 5)
    assert la.same_bits(C[:m][~upper], full[:m][~upper])                          # the other tiles: the bits of the full product
    diag = (t[:, None] == t[None, :]) & (np.arange(m)[:, None] < np.arange(m)[None, :])
    assert diag.any() and not np.isnan(C[:m][diag]).any()


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_sub_nan_stays_in_its_row_and_column(gpu, ta, tb):
    m, n, k = 129, 65, 33
    oa, ob, c0 = la.real_operands(m, n, k, 11)
    clean = dev_gemm(gpu, oa, ob, c0, ta, tb, 0, 5)
    for i, kk in ((64, 17), (63, 32), (128, 0)):
        bad = oa.copy(); bad[i, kk] = np.nan
        C = dev_gemm(gpu, bad, ob, c0, ta, tb, 0, 5)
        rows = np.arange(m) != i
        assert np.isnan(C[i]).all() and la.same_bits(C[:m][rows], clean[:m][rows])
    for j, kk in ((64, 16), (0, 32), (63, 15)):
        bad = ob.copy(); bad[kk, j] = np.nan
        C = dev_gemm(gpu, oa, bad, c0, ta, tb, 0, 5)
        cols = np.arange(n) != j
        assert np.isnan(C[:m, j]).all() and la.same_bits(C[:m][:, cols], clean[:m][:, cols])


# ---- CHOLESKY ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 191, 320])
def test_cholesky(gpu, n):
    A, L = la.chol_int(n)
    for pad in (0, 3):
        buf, info = dev_cholesky(gpu, la.nan_upper(A, S), pad, 0)
        assert info == 0 and la.same_bits(np.tril(buf[:n]), L)                   # bit for bit
        assert upper_blocks_ok(buf, n) and la.same_bits(buf[n:], np.full((pad, n), S))
        for family in sorted(la.REAL_SPD):
            Ar, Lref = la.ref_cholesky(family, n)
            buf, info = dev_cholesky(gpu, la.nan_upper(Ar, S), pad, 7)
            assert info == 7                                                     # never cleared, and not set on a definite matrix
            assert upper_blocks_ok(buf, n) and la.same_bits(buf[n:], np.full((pad, n), S))
            assert la.check_cholesky(f"cholesky {family} n {n} ld {n + pad}", buf[:n], Ar, Lref)


@pytest.mark.parametrize("r", [0, 63, 64, 100, 128])
def test_cholesky_sets_info_at_a_failing_pivot(gpu, r):
    n = 129
    for A in (la.negative_pivot(n, r), la.indefinite_block(n, r)):
        for preset in (0, 7):
            buf, info = dev_cholesky(gpu, la.nan_upper(A, S), 3, preset)
            assert info == 1 and upper_blocks_ok(buf, n) and la.same_bits(buf[n:], np.full((3, n), S))


@pytest.mark.parametrize("n", [2, 129, 320])
def test_cholesky_sets_info_on_the_singular_laplacian(gpu, n):
    buf, info = dev_cholesky(gpu, la.nan_upper(la.path_laplacian(n), S), 0, 0)
    assert info == 1
    assert la.same_bits(np.diag(buf), np.ones(n))                                # the pivots before it are 1 exactly; the failed one is replaced by 1
    assert la.same_bits(np.diag(buf, -1), -np.ones(n - 1))


@pytest.mark.parametrize("pos", [(70, 66), (100, 10), (128, 127), (128, 0), (128, 128)])
def test_cholesky_sets_info_on_a_nan(gpu, pos):
    n = 129
    A, _ = la.chol_int(n)
    A[pos] = np.nan
    _, info = dev_cholesky(gpu, la.nan_upper(A, S), 0, 0)
    assert info == 1


# ---- SUBSTITUTE --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257, 400])
def test_substitute(gpu, n):
    rng = np.random.default_rng(n)
    combos = [(nrhs, pad) for nrhs in (1, 2, 5) for pad in (0, 7)]
    for i, (nrhs, pad) in enumerate(combos):
        fam = sorted(la.EXACT_INVERSES)[i % 2]
        A, L, _ = la.EXACT_INVERSES[fam](n)
        x0 = rng.integers(-8, 9, (n, nrhs)).astype(np.float64)
        X, info = dev_substitute(gpu, la.nan_upper(L), A @ x0, pad, 7 * (i % 2))
        assert info == 7 * (i % 2)                                               # not set, not cleared
        assert la.same_bits(X[:n], x0), (fam, nrhs, pad)                         # x0 bit for bit; no NaN of L's upper triangle was read
        assert la.same_bits(X[n:], np.full((pad, nrhs), S))
        fam = sorted(la.REAL_SPD)[i % 2]
        _, Lref = la.ref_cholesky(fam, n)
        Lg = np.tril(Lref)
        rhs = rng.standard_normal((n, nrhs))
        X, info = dev_substitute(gpu, la.nan_upper(Lg), rhs, pad, 0)
        ref = la.pack(rhs)
        la.substitute(n, Lg, ref, nrhs, 0)
        assert info == 0 and la.same_bits(X[n:], np.full((pad, nrhs), S))
        assert la.check_substitute(f"substitute {fam} n {n} nrhs {nrhs} ldx {n + pad}", X[:n], Lg, rhs, ref), (fam, nrhs, pad)
        if i == 5:
            again, _ = dev_substitute(gpu, la.nan_upper(Lg), rhs, pad, 0)
            assert la.same_bits(again, X)                                        # two runs, the same bits


@pytest.mark.parametrize("r", [0, 70, 128])
def test_substitute_sets_info_on_a_zero_pivot(gpu, r):
    n = 129
    _, L, _ = la.ones_lower(n)
    L[r, r] = 0.0
    for preset in (0, 7):
        X, info = dev_substitute(gpu, la.nan_upper(L), np.ones((n, 2)), 7, preset)
        assert info == 1 and not np.isfinite(X[:n]).all() and la.same_bits(X[n:], np.full((7, 2), S))


# ---- INVERSE -----------------------------------------------------------------------------------------------------------------------------
INVERSE_N = [1, 64, 65, 255, 256, 257, 320, 513, 577]


@pytest.mark.parametrize("family", sorted(la.EXACT_INVERSES))
@pytest.mark.parametrize("n", INVERSE_N)
def test_inverse_exact(gpu, n, family):
    A, L, Ainv = la.EXACT_INVERSES[family](n)
    F, X, ok = dev_inverse(gpu, la.nan_upper(A, S))
    assert ok and la.same_bits(np.tril(F), L) and la.same_bits(np.tril(X), np.tril(Ainv))
    Fc, info = dev_cholesky(gpu, la.nan_upper(A, S), 0, 0)
    assert info == 0 and la.same_bits(F, Fc)                                     # the factor left in A is the CHOLESKY op's


@pytest.mark.parametrize("family", sorted(la.REAL_SPD))
@pytest.mark.parametrize("n", INVERSE_N)
def test_inverse_real(gpu, n, family):
    A, Fref, Xref = la.ref_inverse(family, n)
    F, X, ok = dev_inverse(gpu, la.nan_upper(A, S))
    Fc, info = dev_cholesky(gpu, la.nan_upper(A, S), 0, 0)
    assert ok and info == 0 and la.same_bits(F, Fc) and upper_blocks_ok(F, n)
    assert np.isfinite(np.tril(X)).all()
    assert la.check_inverse(f"inverse {family} n {n}", X, F, A, Xref)
    assert la.check_inverse_lower(f"inverse (lower triangle) {family} n {n}", X, F, Xref)
    F2, X2, ok2 = dev_inverse(gpu, la.nan_upper(A, S))
    assert ok2 and la.same_bits(F2, F) and la.same_bits(np.tril(X2), np.tril(X))  # two runs, the same bits


def refused_matrices():
    n = 513
    return {"pivot": la.negative_pivot(n, 300), "indefinite": la.indefinite_block(n, 300), "singular": la.path_laplacian(n)}


@pytest.mark.parametrize("which", ["pivot", "indefinite", "singular"])
def test_inverse_refuses(gpu, which):
    A = refused_matrices()[which]
    _, X, ok = dev_inverse(gpu, la.nan_upper(A, S))
    assert not ok and la.same_bits(X, np.full(X.shape, S))                       # X comes back as it went up


# ---- the public xm_spd_inverse -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257])
def test_public_inverse_reads_the_lower_triangle_only(gpu, n):
    A = la.laplacian(n) if n == 257 else la.random_spd(n)
    full = gpu.spd_inverse(A)
    assert la.same_bits(gpu.spd_inverse(la.nan_upper(A)), full)                  # "lower triangle read"
    _, X, ok = dev_inverse(gpu, la.nan_upper(A, S))
    assert ok and la.same_bits(dev_layout(gpu, X), full)                         # the two stages it is made of
    assert la.same_bits(full, full.T)


def test_public_inverse_refuses_and_works_again(gpu):
    good = la.random_spd(130)
    before = gpu.spd_inverse(good)
    for which, A in refused_matrices().items():
        with pytest.raises(gpu.XmError, match="error -2"):
            gpu.spd_inverse(A)
        assert la.same_bits(gpu.spd_inverse(good), before), which


# ---- LAYOUT ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_layout(gpu, n):
    X = la.nan_upper(np.random.default_rng(n).standard_normal((n, n)))           # the scratch triangle holds NaN
    for pad in (0, 9):
        dst = dev_layout(gpu, X, pad)
        assert not np.isnan(dst[:, :n]).any()
        assert la.same_bits(dst[:, :n], dst[:, :n].T) and la.same_bits(np.tril(dst[:, :n]), np.tril(X))
        assert la.same_bits(dst[:, n:], np.full((n, pad), S))


# ---- RANK1_SUB ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 300])
def test_rank1_sub(gpu, n):
    rng = np.random.default_rng(n)
    A = rng.integers(-8, 9, (n, n)).astype(np.float64); u = rng.integers(-8, 9, n).astype(np.float64)
    u[::4] = 0.0
    if n == 1:
        u[0] = 3.0
    assert la.same_bits(dev_rank1(gpu, A, u, 5.0), A - 5.0 * np.outer(u, u))
    A = rng.standard_normal((n, n)); u[u != 0.0] = rng.standard_normal(int((u != 0.0).sum()))
    ref = A.copy()
    la.rank1_sub(n, ref, u, 0.37)
    out = dev_rank1(gpu, A, u, 0.37)
    dead = ~np.outer(u != 0.0, u != 0.0)
    assert la.check_rank1(f"rank1_sub n {n}", out, A, u, 0.37, ref) and la.same_bits(out[dead], A[dead])
    # entries whose u_r or u_c is 0 keep their bits, even where A holds NaN and q is infinite
    u[0] = 0.0
    dead = ~np.outer(u != 0.0, u != 0.0)
    A[dead] = S
    out = dev_rank1(gpu, A, u, np.inf)
    assert la.same_bits(out[dead], A[dead]) and not np.isfinite(out[~dead]).any()
