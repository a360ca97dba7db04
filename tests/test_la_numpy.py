"""CPU tests of tests/xm_la_stages.py: the float64 restatement of the blocked algorithms of xm_dense_la.hip passes every checker on every
family, the exactness condition of the integer families holds (every accumulation stays below 2^53, every quotient and root is exact), and
the checkers have teeth: each planted fault of xm_la_stages.FAULTS fails the check that is meant to see it."""
import numpy as np
import pytest

import xm_la_stages as la

NAN = np.nan


def _gemm(m, n, k, ta, tb, lower_only, pad, ops, fault=None):
    """the restatement on padded buffers with NaN padding; returns (C buffer, C0 buffer, op(A), op(B), C0)"""
    oa, ob, c0 = ops
    A = la.pack(oa.T if ta else oa, (k if ta else m) + pad)
    B = la.pack(ob.T if tb else ob, (n if tb else k) + pad)
    C = la.pack(c0, m + pad, la.SENTINEL)
    C0 = C.copy()
    la.gemm_sub(m, n, k, A, ta, B, tb, C, lower_only, fault)
    return C, C0, oa, ob, c0


def _gemm_ok(what, m, n, k, ta, tb, lower_only, pad, ops, fault=None, exact=False):
    C, C0, oa, ob, c0 = _gemm(m, n, k, ta, tb, lower_only, pad, ops, fault)
    ok = la.same_bits(C[m:], C0[m:])                                             # the padding of C keeps its bits
    t = np.arange(m) // la.KB
    dead = (t[:, None] < (np.arange(n) // la.KB)[None, :]) if lower_only else np.zeros((m, n), dtype=bool)
    ok = ok and la.same_bits(C[:m][dead], c0[dead])                              # tiles above the diagonal keep theirs
    if exact:
        return ok and la.same_bits(np.where(dead, 0.0, C[:m]), np.where(dead, 0.0, c0 - oa @ ob))
    return ok and la.check_gemm(what, C[:m], oa, ob, c0, lower_only)


GEMM_SHAPES = [(65, 129, 17, 0, 0, 0, 5), (129, 63, 33, 1, 0, 0, 0), (64, 65, 80, 0, 1, 0, 5), (63, 64, 15, 1, 1, 0, 5), (129, 129, 31, 0, 1, 1, 5),
               (1, 1, 1, 1, 1, 0, 0), (65, 65, 16, 1, 0, 1, 0)]


@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_gemm_restatement(shape):
    m, n, k, ta, tb, lo, pad = shape
    with la.tracking() as t:
        assert _gemm_ok("", m, n, k, ta, tb, lo, pad, la.int_operands(m, n, k, 1), exact=True)
    assert t["mag"] < 2.0 ** 53                                                   # at most 8 + 64 k
    assert _gemm_ok(f"gemm {shape}", m, n, k, ta, tb, lo, pad, la.real_operands(m, n, k, 2))


@pytest.mark.parametrize("n", [1, 2, 65, 129, 257, 321])
def test_cholesky_restatement_exact(n):
    A, L = la.chol_int(n)
    buf = la.pack(la.nan_upper(A), n + 3)
    with la.tracking() as t:
        assert la.cholesky(n, buf, 0) == 0
    assert t["exact"] and t["mag"] < 2.0 ** 53
    assert la.same_bits(np.tril(buf[:n]), L) and np.isnan(buf[n:]).all()
    Li = L.astype(np.int64)
    assert np.array_equal(Li @ Li.T, A.astype(np.int64))
    # above the diagonal: zeros inside the diagonal blocks, the input's NaN elsewhere
    r, c = np.triu_indices(n, 1)
    inside = r // la.KB == c // la.KB
    assert np.all(buf[r[inside], c[inside]] == 0.0) and np.isnan(buf[r[~inside], c[~inside]]).all()


@pytest.mark.parametrize("family", sorted(la.EXACT_INVERSES))
@pytest.mark.parametrize("n", [1, 65, 257, 321, 577])
def test_exact_inverse_families(family, n):
    A, L, Ainv = la.EXACT_INVERSES[family](n)
    F = la.pack(A); X = np.zeros((n, n), order="F")
    with la.tracking() as t:
        assert la.inverse(n, F, X)
        x0 = np.random.default_rng(n).integers(-8, 9, (n, 3)).astype(np.float64)
        Bx = la.pack(A @ x0, n + 7)
        assert la.substitute(n, np.tril(L), Bx, 3, 0) == 0
    assert t["exact"] and t["mag"] < 2.0 ** 53
    assert la.same_bits(np.tril(F), L) and la.same_bits(np.tril(X), np.tril(Ainv)) and la.same_bits(Bx[:n], x0)
    Ai = A.astype(np.int64)
    assert np.array_equal(Ai @ Ainv.astype(np.int64), np.eye(n, dtype=np.int64))   # the stated inverse is the inverse, in integers
    dst = np.full((n, n + 9), la.SENTINEL)
    la.layout(n, la.nan_upper(X), dst)
    assert la.same_bits(dst[:, :n], Ainv) and la.same_bits(dst[:, n:], np.full((n, 9), la.SENTINEL))


@pytest.mark.parametrize("n", [2, 129, 320])
def test_singular_and_indefinite_are_refused(n):
    buf = la.pack(la.path_laplacian(n))
    with la.tracking() as t:
        assert la.cholesky(n, buf, 0) == 1                                      # the last pivot is exactly 0
    assert t["exact"]
    assert la.same_bits(np.diag(buf), np.ones(n))                               # every pivot but the last is 1; the last is replaced by 1
    for r in (0, 63, 64, 100, n - 1):
        if r < n:
            assert la.cholesky(n, la.pack(la.indefinite_block(n, r)), 0) == 1 and la.cholesky(n, la.pack(la.negative_pivot(n, r)), 0) == 1
            assert np.all(np.diag(la.indefinite_block(n, r)) > 0) and np.linalg.eigvalsh(la.indefinite_block(n, r)).min() < 0
    assert not la.inverse(n, la.pack(la.path_laplacian(n)), np.zeros((n, n), order="F"))


@pytest.mark.parametrize("family", sorted(la.REAL_SPD))
@pytest.mark.parametrize("n", [65, 300])
def test_real_families_pass_the_bounds(family, n):
    A, Lb = la.ref_cholesky(family, n)
    print(f"{family} n {n}: condition number {np.linalg.cond(A):.2e}")
    assert la.check_cholesky(f"cholesky {family} {n}", Lb, la.nan_upper(A))
    rhs = np.random.default_rng(n).standard_normal((n, 2))
    X = la.pack(rhs, n + 7)
    assert la.substitute(n, np.array(Lb), X, 2, 7) == 7 and np.isnan(X[n:]).all()
    assert la.check_substitute(f"substitute {family} {n}", X[:n], Lb, rhs)
    _, F, Xi = la.ref_inverse(family, n)
    assert la.same_bits(np.tril(F), np.tril(Lb))
    assert la.check_inverse(f"inverse {family} {n}", Xi, F, A) and la.check_inverse_lower(f"inverse (lower) {family} {n}", Xi, F)
    u = np.random.default_rng(n + 1).standard_normal(n); u[::3] = 0.0
    R = A.copy()
    la.rank1_sub(n, R, u, 0.37)
    assert la.check_rank1(f"rank1 {family} {n}", R, A, u, 0.37) and la.same_bits(R[::3], A[::3])


def test_laplacian_conditioning():
    """the family is as ill-conditioned as the issue it stands for: weights over ten decades"""
    for n in (300, 600):
        assert 1e6 < np.linalg.cond(la.laplacian(n)) < 1e10


# ---- the checkers have teeth -----------------------------------------------------------------------------------------------------------
def test_fault_k_tail_dropped():
    assert not _gemm_ok("fault", 65, 65, 17, 0, 0, 0, 0, la.int_operands(65, 65, 17, 3), "k tail dropped", exact=True)
    assert not _gemm_ok("fault", 65, 65, 17, 0, 0, 0, 0, la.real_operands(65, 65, 17, 3), "k tail dropped")


def test_fault_ta_ignored():
    assert not _gemm_ok("fault", 65, 63, 33, 1, 0, 0, 5, la.real_operands(65, 63, 33, 4), "ta ignored")
    assert not _gemm_ok("fault", 65, 63, 33, 1, 0, 0, 0, la.int_operands(65, 63, 33, 4), "ta ignored", exact=True)


def test_fault_upper_tile_written():
    assert not _gemm_ok("fault", 129, 129, 16, 0, 1, 1, 0, la.real_operands(129, 129, 16, 5), "upper tile written")


def test_fault_row_from_the_neighbouring_tile():
    assert not _gemm_ok("fault", 65, 64, 16, 0, 0, 0, 0, la.real_operands(65, 64, 16, 6), "row from the neighbouring tile")
    assert not _gemm_ok("fault", 65, 64, 16, 0, 0, 0, 0, la.int_operands(65, 64, 16, 6), "row from the neighbouring tile", exact=True)


def test_fault_padding_row_read():
    assert not _gemm_ok("fault", 64, 64, 17, 1, 0, 0, 5, la.real_operands(64, 64, 17, 7), "padding row read")


def test_fault_last_trailing_update_skipped():
    A, L = la.chol_int(129)
    buf = la.pack(A)
    la.cholesky(129, buf, 0, "last trailing update skipped")
    assert not la.same_bits(np.tril(buf), L)
    A = la.random_spd(129)
    buf = la.pack(A)
    la.cholesky(129, buf, 0, "last trailing update skipped")
    assert not la.check_cholesky("fault", buf, A)


def test_fault_info_cleared():
    A, _ = la.chol_int(65)
    assert la.cholesky(65, la.pack(A), 7) == 7 and la.cholesky(65, la.pack(A), 7, "info cleared") != 7
    _, L, _ = la.ones_lower(65)
    assert la.substitute(65, L, la.pack(np.ones(65)), 1, 7) == 7 and la.substitute(65, L, la.pack(np.ones(65)), 1, 7, "info cleared") != 7


def test_fault_backward_block_row_missing():
    A, Lb = la.ref_cholesky("random", 65)
    rhs = np.random.default_rng(0).standard_normal((65, 1))
    X = la.pack(rhs)
    la.substitute(65, np.array(Lb), X, 1, 0, "backward block row missing")
    assert not la.check_substitute("fault", X, Lb, rhs)
    A, L, _ = la.ones_lower(65)
    x0 = np.arange(1.0, 66.0)[:, None]
    X = la.pack(A @ x0)
    la.substitute(65, L, X, 1, 0, "backward block row missing")
    assert not la.same_bits(X, x0)


def test_fault_super_block_gemm_one_column_short():
    n = 321
    A = la.random_spd(n)
    F = la.pack(A); X = np.zeros((n, n), order="F")
    assert la.inverse(n, F, X, "super-block gemm one column short")
    assert not la.check_inverse("fault", X, F, A) and not la.check_inverse_lower("fault", X, F)
    A, L, Ainv = la.ramp_lower(n)
    F = la.pack(A); X = np.zeros((n, n), order="F")
    la.inverse(n, F, X, "super-block gemm one column short")
    assert not la.same_bits(np.tril(X), np.tril(Ainv))


def test_fault_layout_reads_the_scratch_triangle():
    X = la.nan_upper(np.arange(25.0).reshape(5, 5))
    dst = np.zeros((5, 5))
    la.layout(5, X, dst, "layout reads the scratch triangle")
    assert np.isnan(dst).any()
    la.layout(5, X, dst)
    assert not np.isnan(dst).any() and la.same_bits(dst, dst.T)


def test_fault_entry_off_by_2_40():
    n = 65
    oa, ob, c0 = la.real_operands(n, n, 33, 8)
    assert la.check_gemm("gemm", c0 - oa @ ob, oa, ob, c0) and not la.check_gemm("fault", la.off_by_2_40(c0 - oa @ ob), oa, ob, c0)
    for family in sorted(la.REAL_SPD):
        A, Lb = la.ref_cholesky(family, n)
        assert not la.check_cholesky("fault", la.off_by_2_40(np.tril(Lb)), A)
        rhs = np.random.default_rng(n).standard_normal((n, 1))
        X = la.pack(rhs)
        la.substitute(n, np.array(Lb), X, 1, 0)
        assert la.check_substitute("substitute", X, Lb, rhs) and not la.check_substitute("fault", la.off_by_2_40(X), Lb, rhs)
        _, F, Xi = la.ref_inverse(family, n)
        bad = la.off_by_2_40(np.array(Xi), np.tril(np.ones((n, n), dtype=bool)))
        assert not la.check_inverse("fault", bad, F, A) and not la.check_inverse_lower("fault", bad, F)
    u = np.random.default_rng(1).standard_normal(n)
    R = A.copy()
    la.rank1_sub(n, R, u, 2.5)
    assert la.check_rank1("rank1", R, A, u, 2.5) and not la.check_rank1("fault", la.off_by_2_40(R), A, u, 2.5)


def test_every_fault_has_a_test():
    names = {k for k in globals() if k.startswith("test_fault_")}
    assert len(names) == len(la.FAULTS) >= 10
