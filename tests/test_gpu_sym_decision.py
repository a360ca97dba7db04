"""asym_kernel decides whether the half-traffic symmetric product may run -- a kernel that never reads the lower triangle.  A wrong yes
is a silently wrong solve, so the decision is held here at the tile borders of the 64 x 64 sweep: one changed entry, its mirror image
left alone, at the first and last rows and columns, across the borders of the first and second tile, in partial last tiles (3n = 3, 63,
66, 129, 258) and in whole ones (192); changes of one ulp, of 5e-324 against a zero, and a NaN on either side or on the diagonal.  The
decision is read through xm_result_t.sym_product of a solve that takes no step and through Context.product_kind."""
import numpy as np
import pytest

import xm_xm2_exact as xx

pytestmark = pytest.mark.gpu

SIZES = (1, 21, 22, 43, 64, 86)


def decision(xmamd, Q, solve=False, **tuning):
    """(1 / 0, product_kind(3), product_kind(5)) of a context created from Q; solve=True: also through xm_result_t.sym_product of a solve
    that takes no step, as solve_dense reports it (the same flag of the context, and about a second per solve: read that way for the base
    matrix and for one change per size)"""
    tn = dict(sym_min_rows=1, **tuning)
    ctx = xmamd.Context(Q=Q, tuning=tn)
    try:
        k3, k5 = ctx.product_kind(3), ctx.product_kind(5)
    finally:
        ctx.close()
    if solve:
        _, _, info = xmamd.solve_dense(Q, 3, 1e-1, 0.0, max_time=0.0, mode=xmamd.MODE_RANK3, tuning=tn)
        assert int(info["sym_product"]) == int(k3 == "dense_sym")
    return int(k3 == "dense_sym"), k3, k5


@pytest.mark.parametrize("n", SIZES)
def test_exact_symmetry_is_required(xmamd, n):
    Q = xx.symmetric_base(n)
    m = 3 * n
    assert decision(xmamd, Q, solve=True) == (1, "dense_sym", "dense")        # automatic: ranks 3 and 4 only
    assert decision(xmamd, Q, sym=-1) == (0, "dense", "dense")
    for r, c in xx.sym_positions(m):
        case = (n, r, c)
        A = Q.copy(); A[r, c] = np.nextafter(A[r, c], np.inf)       # one ulp
        assert decision(xmamd, A, solve=(r, c) == (1, 0))[0] == 0, ("ulp",) + case
        Z = Q.copy(); Z[r, c] = Z[c, r] = 0.0
        assert decision(xmamd, Z)[0] == 1, ("zeros",) + case
        Z[r, c] = 5e-324                                            # the smallest double against a zero
        assert decision(xmamd, Z)[0] == 0, ("denormal",) + case
        Z[r, c] = 0.0; Z[c, r] = -0.0                               # equal values, the same product
        assert decision(xmamd, Z)[0] == 1, ("signed zero",) + case
        lo, hi = min(r, c), max(r, c)
        for pos, what in (((lo, hi), "NaN above"), ((hi, lo), "NaN below"), ((r, r), "NaN on the diagonal")):
            N = Q.copy(); N[pos] = np.nan
            assert decision(xmamd, N)[0] == 0, (what,) + case
        N = Q.copy(); N[lo, hi] = np.nan
        assert decision(xmamd, N, sym=1)[0] == 0 and decision(xmamd, A, sym=-1)[0] == 0


@pytest.mark.parametrize("n", SIZES)
def test_forced_symmetric_product_accepts_round_off_only(xmamd, n):
    """xm_tuning_t.sym = 1: |Q - Q^T| <= 1e-9 max|Q| is accepted, ranks up to 5"""
    Q = xx.symmetric_base(n)
    m = 3 * n
    mx = np.abs(Q).max()
    assert decision(xmamd, Q, solve=True, sym=1) == (1, "dense_sym", "dense_sym")
    for r, c in xx.sym_positions(m):
        for f, exp in ((0.5e-9, 1), (2e-9, 0)):
            A = Q.copy(); A[r, c] += f * mx
            assert abs(A[r, c] - A[c, r]) > 0
            assert decision(xmamd, A, sym=1, solve=(r, c, exp) == (1, 0, 0))[0] == exp, (n, r, c, f)
        assert decision(xmamd, A)[0] == 0
