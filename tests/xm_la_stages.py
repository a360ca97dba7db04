"""References, matrix families and checkers for the dense float64 linear algebra of xm-code_amd/csrc/xm_dense_la.hip (numpy only).

Three things live here:

* a float64 RESTATEMENT of the blocked algorithms in the order of the host functions (gemm_sub: 64 x 64 tiles, K in chunks of 16;
  cholesky: potrf / panel solve / lower-tile update per 64 columns; substitute: 64-row steps; inverse: super blocks of 256 rows; layout;
  rank1_sub).  It works on the buffers as the device sees them -- column-major 2-D arrays with `ld` rows, the rows past the matrix being
  padding -- and takes a `fault` name that plants one mistake (tests/test_la_numpy.py: the checkers must catch each).
* matrix families: integer-valued ones for which every intermediate of every summation order is an integer below 2^53 (the device must
  then return the integer result bit for bit), and real-valued ones (random, and a weighted reduced graph Laplacian with edge weights over
  ten decades).
* checkers.  Real-valued results are held to the standard componentwise rounding-error bounds (Higham, Accuracy and Stability of
  Numerical Algorithms, 2nd ed.), which hold for every order of summation and with or without fused multiply-add.  u = 2^-53,
  gamma_k = k u / (1 - k u):

      gemm_sub     |C^ - (C - A B)|   <= gamma_{k+1} (|C| + |A||B|)                 (3.5: an inner product of k + 1 terms)
      cholesky     |A - L^ L^^T|      <= gamma_{n+1} |L^||L^^T|                     (Theorem 10.3)
      substitute   |b - L L^T x^|     <= (2 gamma_n + gamma_n^2) |L||L^T||x^|       (Theorem 8.5 twice, L the given factor)
      inverse      |A X^ - I|         <= 4 gamma_{n+1} |L^||L^^T||X^|
      rank1_sub    |A^ - (A - q u u^T)| <= gamma_3 (|A| + |q u_r u_c|)              (two products and one subtraction)

  The inverse's constant.  Column j of X^ solves L^ L^^T x = e_j by the two substitutions, so by the third line
  e_j - L^ L^^T x^_j = r_j with |r_j| <= (2 gamma_n + gamma_n^2) |L^||L^^T||x^_j|, and by the second line L^ L^^T = A + dA with
  |dA| <= gamma_{n+1} |L^||L^^T|.  Hence A x^_j - e_j = -r_j - dA x^_j and
      |A x^_j - e_j| <= (2 gamma_n + gamma_n^2 + gamma_{n+1}) |L^||L^^T||x^_j| <= (3 + gamma_n) gamma_{n+1} |L^||L^^T||x^_j|,
  so c = 3 + gamma_n, and 4 is used.  This takes every column as ONE complete substitution.  spd_inverse_device computes the rows
  i >= j of column j only and takes the rest from the transposed entries, which belong to other columns' substitutions; the step above
  does not cover that exchange, so the lower triangle is ALSO held to a statement that needs no such step (check_inverse_lower): with
  J = {j, ..., n - 1}, the forward substitution leaves exact zeros above row j, so rows J of column j solve
  L^_JJ L^_JJ^T x_J = e_1 by two substitutions of order n - j, and for all columns at once
      |tril(I - L^ tril(L^^T tril(X^)))| <= (2 gamma_n + gamma_n^2) tril(|L^| tril(|L^^T| tril(|X^|))).
  An entry whose bound is 0 must be 0.  Left-hand sides are evaluated in longdouble (u_ld = 2^-64: its own error is 2^-11 of the bound);
  the right-hand sides, products of non-negative numbers, in float64 (relative error n u, immaterial).

Every check prints `what: e_gpu ... e_ref ... ratio ...`: the largest error of the result under test and of the float64 restatement, each
relative to the largest reference entry, and the largest error / bound of the result under test."""
import contextlib

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
KB = 64          # kLaB
KS = 256         # kLaS
KC = 16          # K chunk of la_gemm_sub_kernel
FAULTS = ("k tail dropped", "ta ignored", "upper tile written", "row from the neighbouring tile", "padding row read",
          "last trailing update skipped", "info cleared", "backward block row missing", "super-block gemm one column short",
          "layout reads the scratch triangle", "entry off by 2^-40")


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- buffers as the device sees them -------------------------------------------------------------------------------------------------
def pack(M, ld=None, fill=np.nan):
    """column-major buffer of ld rows holding M, the padding rows filled with `fill`"""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 1:
        M = M[:, None]
    buf = np.full((M.shape[0] if ld is None else ld, M.shape[1]), fill, order="F")
    buf[:M.shape[0]] = M
    return buf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


SENTINEL = float(np.frombuffer(np.uint64(0x7FF8_0000_0000_5A5A).tobytes(), dtype=np.float64)[0])   # a NaN with a payload of its own


# ---- exactness bookkeeping -----------------------------------------------------------------------------------------------------------
_track = None


@contextlib.contextmanager
def tracking():
    """inside, the restatement records the largest |c| + sum |a||b| of any accumulation and whether every quotient and root was exact:
    with integer inputs and that magnitude below 2^53, every partial sum of every order is an integer below 2^53, so exact in float64"""
    global _track
    _track = {"mag": 0.0, "exact": True}
    try:
        yield _track
    finally:
        _track = None


def _note(mag):
    if _track is not None and np.size(mag):
        with np.errstate(invalid="ignore"):
            _track["mag"] = max(_track["mag"], float(np.nanmax(mag)))


def _note_exact(ok):
    if _track is not None:
        _track["exact"] = _track["exact"] and bool(ok)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def gemm_sub(m, n, k, A, ta, Bm, tb, Cm, lower_only=0, fault=None):
    """Cm[:m, :n] -= op(A) op(B) in place, tile by tile.  A, Bm, Cm: 2-D views whose first m (k, ...) rows and columns are the operands"""
    if m <= 0 or n <= 0 or k <= 0:
        return
    ta_used = 0 if fault == "ta ignored" else ta

    def opa(rows, ks):
        if ta_used:
            return A[np.ix_(ks % A.shape[0], rows % A.shape[1])].T
        return A[np.ix_(rows % A.shape[0], ks % A.shape[1])]

    def opb(ks, cols):
        return Bm[np.ix_(cols, ks)].T if tb else Bm[np.ix_(ks, cols)]

    kend = k - k % KC if fault == "k tail dropped" else k
    kguard = k + 5 if fault == "padding row read" else kend     # the K guard of the loads
    with np.errstate(invalid="ignore", over="ignore"):
        for bi in range((m + KB - 1) // KB):
            for bj in range((n + KB - 1) // KB):
                if lower_only and bj > bi and fault != "upper tile written":
                    continue
                rows = np.arange(bi * KB, min(m, bi * KB + KB)); cols = np.arange(bj * KB, min(n, bj * KB + KB))
                arows = rows.copy()
                if fault == "row from the neighbouring tile" and bi > 0:
                    arows[0] -= 1
                acc = np.zeros((rows.size, cols.size)); mag = np.zeros((rows.size, cols.size))
                for k0 in range(0, kend, KC):
                    ks = np.arange(k0, min(k0 + KC, kguard))
                    a, b = opa(arows, ks), opb(ks, cols)
                    acc += a @ b
                    if _track is not None:
                        mag += np.abs(a) @ np.abs(b)
                c = Cm[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
                _note(np.abs(c) + mag)
                c -= acc


def potrf(Ab, info):
    """la_potrf_kernel: right-looking, unblocked, in place; zeros above the diagonal"""
    b = Ab.shape[0]
    L = Ab.copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(b):
            d = L[j, j]
            if not d > 0.0:
                info = 1
            r = np.sqrt(d if d > 0.0 else 1.0)
            _note_exact(r * r == (d if d > 0.0 else 1.0))
            L[j, j] = r
            if j + 1 < b:
                col = L[j + 1:, j] / r
                _note_exact(np.all(col * r == L[j + 1:, j]) and np.all(col == np.rint(col)))
                L[j + 1:, j] = col
                o = np.tril(np.outer(col, col))
                _note(np.tril(np.abs(L[j + 1:, j + 1:])) + np.abs(o))
                L[j + 1:, j + 1:] -= o
    Ab[:] = np.tril(L)
    return info


def trsm_right(P, L):
    """la_trsm_right_kernel: P <- P L^-T, forward along each row"""
    b = L.shape[0]
    X = np.zeros_like(P)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(b):
            _note(np.abs(P[:, c]) + np.abs(X[:, :c]) @ np.abs(L[c, :c]))
            t = P[:, c] - X[:, :c] @ L[c, :c]
            X[:, c] = t / L[c, c]
            _note_exact(np.all(X[:, c] * L[c, c] == t) and np.all(X[:, c] == np.rint(X[:, c])))
    P[:] = X


def trsm_left(L, T, trans):
    """la_trsm_left_kernel: T <- L^-1 T (trans 0) or L^-T T (trans 1), one column at a time in the device's order"""
    b = L.shape[0]
    X = np.zeros_like(T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in (range(b) if not trans else range(b - 1, -1, -1)):
            if not trans:
                row, prev = L[i, :i], X[:i]
            else:
                row, prev = L[i + 1:, i], X[i + 1:]
            _note(np.abs(T[i]) + np.abs(row) @ np.abs(prev))
            t = T[i] - row @ prev
            X[i] = t / L[i, i]
            _note_exact(np.all(X[i] * L[i, i] == t) and np.all(X[i] == np.rint(X[i])))
    T[:] = X


def cholesky(n, A, info=0, fault=None):
    """spd_cholesky_device on the buffer A (ld x n); returns info"""
    if fault == "info cleared":
        info = 0
    for k in range(0, n, KB):
        b = min(KB, n - k); m = n - k - b
        A11 = A[k:k + b, k:k + b]
        info = potrf(A11, info)
        if m > 0:
            A21 = A[k + b:n, k:k + b]
            trsm_right(A21, A11)
            if fault == "last trailing update skipped" and m <= KB:
                continue
            gemm_sub(m, m, b, A[k + b:, k:k + b], 0, A[k + b:, k:k + b], 1, A[k + b:, k + b:], 1)
    return info


def _solve_block(Lb, y, trans):
    """the diagonal block of la_trsv_step_kernel: the pivots in order, each applied to the rows it updates"""
    b = Lb.shape[0]
    y = y.copy(); x = np.zeros(b)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in (range(b) if not trans else range(b - 1, -1, -1)):
            x[j] = y[j] / Lb[j, j]
            _note_exact(x[j] * Lb[j, j] == y[j] and x[j] == np.rint(x[j]))
            if not trans:
                _note(np.abs(y[j + 1:]) + np.abs(Lb[j + 1:, j] * x[j]))
                y[j + 1:] -= Lb[j + 1:, j] * x[j]
            else:
                _note(np.abs(y[:j]) + np.abs(Lb[j, :j] * x[j]))
                y[:j] -= Lb[j, :j] * x[j]
    return x


def substitute(n, L, X, nrhs, info=0, fault=None):
    """spd_substitute_device: X (ldx x nrhs buffer) <- (L L^T)^-1 X; returns info"""
    if fault == "info cleared":
        info = 0
    Y = np.zeros_like(X)
    with np.errstate(invalid="ignore", over="ignore"):
        for trans, src, dst in ((0, X, Y), (1, Y, X)):
            starts = range(0, n, KB) if not trans else range(((n - 1) // KB) * KB, -1, -KB)
            for k0 in starts:
                if trans and k0 == 0 and fault == "backward block row missing":
                    continue
                b = min(KB, n - k0)
                for q in range(nrhs):
                    x = _solve_block(L[k0:k0 + b, k0:k0 + b], src[k0:k0 + b, q], trans)
                    dst[k0:k0 + b, q] = x
                    if not np.all(np.isfinite(x)):
                        info = 1
                    if not trans:
                        blk = L[k0 + b:n, k0:k0 + b]
                        _note(np.abs(src[k0 + b:n, q]) + np.abs(blk) @ np.abs(x))
                        src[k0 + b:n, q] -= blk @ x
                    else:
                        blk = L[k0:k0 + b, :k0]
                        _note(np.abs(src[:k0, q]) + np.abs(x) @ np.abs(blk))
                        src[:k0, q] -= x @ blk
    return info


def inverse(n, A, X, fault=None):
    """spd_inverse_device: A (n x n) -> factor, X (n x n) <- lower triangle of A^-1 and scratch; returns ok"""
    if cholesky(n, A, 0):
        return False
    X[:] = np.eye(n)
    for I in range(0, n, KS):
        Bs = min(KS, n - I)
        gemm_sub(Bs, I + Bs, I, A[I:, :], 0, X, 0, X[I:, :])
        for i in range(I, I + Bs, KB):
            b = min(KB, n - i); nc = i + b
            gemm_sub(b, nc, i - I, A[i:, I:], 0, X[I:, :], 0, X[i:, :])
            trsm_left(A[i:i + b, i:i + b], X[i:i + b, :nc], 0)
    for I in range(((n - 1) // KS) * KS, -1, -KS):
        Bs = min(KS, n - I); below = n - I - Bs
        # (the planted fault sits in the backward sweep: the forward one subtracts exact zeros in its last column, Y being lower triangular)
        gemm_sub(Bs, I + Bs - (fault == "super-block gemm one column short"), below, A[I + Bs:, I:], 1, X[I + Bs:, :], 0, X[I:, :])
        for i in range(I + ((Bs - 1) // KB) * KB, I - 1, -KB):
            b = min(KB, n - i); inside = I + Bs - i - b
            gemm_sub(b, i + b, inside, A[i + b:, i:], 1, X[i + b:, :], 0, X[i:, :])
            trsm_left(A[i:i + b, i:i + b], X[i:i + b, :i + b], 1)
    return True


def layout(n, X, dst, fault=None):
    """spd_inverse_layout: dst (row-major, n rows of ldd: an (n, ldd) C-ordered array) <- the symmetric matrix of X's lower triangle"""
    low = np.tril(X)
    dst[:, :n] = X if fault == "layout reads the scratch triangle" else low + np.tril(X, -1).T


def rank1_sub(n, A, u, q):
    with np.errstate(invalid="ignore", over="ignore"):
        live = np.outer(u != 0.0, u != 0.0)
        _note(np.where(live, np.abs(A) + np.abs(np.outer(u, u) * q), 0.0))
        A[live] -= (np.outer(u, u) * q)[live]


def off_by_2_40(R, mask=None):
    """the planted fault 'a result entry off by 2^-40 relative': the largest (unmasked) entry"""
    R = R.copy()
    a = np.abs(np.where(np.isfinite(R), R, 0.0))
    if mask is not None:
        a = np.where(mask, a, 0.0)
    i = np.unravel_index(np.argmax(a), R.shape)
    R[i] *= 1.0 + 2.0 ** -40
    return R


# ---- families ------------------------------------------------------------------------------------------------------------------------
def int_operands(m, n, k, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-8, 9, s).astype(np.float64) for s in ((m, k), (k, n), (m, n))]


def real_operands(m, n, k, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s) for s in ((m, k), (k, n), (m, n))]


def chol_int(n, seed=0):
    """A = L L^T, L lower with integer entries in [-3, 3] and diagonal in [1, 4]: (A, L) as float64"""
    rng = np.random.default_rng(1000 + n + seed)
    L = np.tril(rng.integers(-3, 4, (n, n)), -1) + np.diag(rng.integers(1, 5, n))
    return (L @ L.T).astype(np.float64), L.astype(np.float64)


def ones_lower(n):
    """L the all-ones lower triangle: A_ij = min(i, j) + 1, A^-1 = tridiag(-1, 2, -1) with the last diagonal entry 1"""
    L = np.tril(np.ones((n, n), dtype=np.int64))
    Ainv = 2 * np.eye(n, dtype=np.int64) - np.eye(n, k=1, dtype=np.int64) - np.eye(n, k=-1, dtype=np.int64)
    Ainv[-1, -1] = 1
    return (L @ L.T).astype(np.float64), L.astype(np.float64), Ainv.astype(np.float64)


def ramp_lower(n):
    """L_ij = i - j + 1 (unit lower, dense, the square of the all-ones triangle): L^-1 is the second difference (1, -2, 1), so A^-1 =
    L^-T L^-1 is pentadiagonal with entries of magnitude at most 6"""
    i = np.arange(n)
    L = np.tril(i[:, None] - i[None, :] + 1).astype(np.int64)
    Li = np.eye(n, dtype=np.int64) - 2 * np.eye(n, k=-1, dtype=np.int64) + np.eye(n, k=-2, dtype=np.int64)
    assert np.array_equal(L @ Li, np.eye(n, dtype=np.int64))
    return (L @ L.T).astype(np.float64), L.astype(np.float64), (Li.T @ Li).astype(np.float64)


EXACT_INVERSES = {"ones": ones_lower, "ramp": ramp_lower}


def path_laplacian(n):
    """the unreduced Laplacian of a path: integer, and its Cholesky pivots are 1, ..., 1, 0 exactly"""
    A = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    A[0, 0] = A[-1, -1] = 1.0
    return A


def indefinite_block(n, r):
    """the identity with [[1, 2], [2, 1]] at rows (r, r + 1) (the last two rows for r = n - 1): positive diagonal, indefinite"""
    A = np.eye(n)
    r = min(r, n - 2)
    A[r + 1, r] = A[r, r + 1] = 2.0
    return A


def negative_pivot(n, r):
    A = np.eye(n)
    A[r, r] = -1.0
    return A


def random_spd(n, seed=0):
    rng = np.random.default_rng(2000 + n + seed)
    M = rng.standard_normal((n, n))
    return M @ M.T / n + np.diag(rng.uniform(0.5, 2.0, n))


def laplacian(n, seed=0):
    """reduced weighted graph Laplacian (what the reduced camera Laplacian is): n + 1 nodes, a random spanning tree and about two more
    edges per node, edge weights 10^U(-5, 5), the row and column of node 0 removed"""
    rng = np.random.default_rng(3000 + n + seed)
    N = n + 1
    a = np.concatenate([np.arange(1, N), rng.integers(0, N, 2 * N)])
    b = np.concatenate([[rng.integers(0, i) for i in range(1, N)], rng.integers(0, N, 2 * N)]).astype(np.int64)
    keep = a != b
    a, b = a[keep], b[keep]
    w = 10.0 ** rng.uniform(-5.0, 5.0, a.size)
    Lp = np.zeros((N, N))
    np.add.at(Lp, (a, a), w); np.add.at(Lp, (b, b), w); np.add.at(Lp, (a, b), -w); np.add.at(Lp, (b, a), -w)
    return Lp[1:, 1:].copy()


REAL_SPD = {"random": random_spd, "laplacian": laplacian}


def nan_upper(A, fill=np.nan):
    A = np.array(A, dtype=np.float64)
    A[np.triu_indices(A.shape[0], 1)] = fill
    return A


# ---- checkers ------------------------------------------------------------------------------------------------------------------------
def ld_dot(a, b):
    # rows of a against columns of b, both contiguous: numpy's longdouble product has no blocking, and is eight times slower otherwise
    return np.dot(np.ascontiguousarray(a, dtype=LD), np.asfortranarray(b, dtype=LD))


def within(what, err, bound, scale, err_ref=None):
    """err <= bound entry by entry (an entry whose bound is 0 must be 0; a NaN fails)"""
    err = np.asarray(err, dtype=LD); bound = np.asarray(bound, dtype=LD)
    pos = bound > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.max(np.where(pos, err / np.where(pos, bound, 1), 0), initial=0.0))
    s = float(scale) if scale > 0 else 1.0
    e = float(np.max(err, initial=0.0)) / s
    er = float("nan") if err_ref is None else float(np.max(np.asarray(err_ref, dtype=LD), initial=0.0)) / s
    print(f"{what}: e_gpu {e:.3e} e_ref {er:.3e} ratio {ratio:.4f}")
    return bool(np.all(err <= bound))


def check_gemm(what, C_hat, opA, opB, C0, lower_only=0, C_ref64=None):
    """C_hat, opA (m x k), opB (k x n), C0 (m x n) without padding; lower_only: the tiles above the diagonal are left out"""
    k = opA.shape[1]
    ref = np.asarray(C0, dtype=LD) - ld_dot(opA, opB)
    bound = gamma(k + 1) * (np.abs(C0) + np.abs(opA) @ np.abs(opB))
    err = np.abs(np.asarray(C_hat, dtype=LD) - ref)
    err_ref = None if C_ref64 is None else np.abs(np.asarray(C_ref64, dtype=LD) - ref)
    if lower_only:
        t = np.arange(C0.shape[0]) // KB
        live = t[:, None] >= (np.arange(C0.shape[1]) // KB)[None, :]
        err = np.where(live, err, 0); err_ref = None if err_ref is None else np.where(live, err_ref, 0)
    return within(what, err, bound, np.max(np.abs(ref)), err_ref)


def check_cholesky(what, L_hat, A, L_ref64=None):
    """lower triangles only: A's upper triangle may hold anything"""
    n = A.shape[0]
    Al = np.tril(np.where(np.tril(np.ones((n, n), dtype=bool)), A, 0.0))

    def resid(L):
        L = np.tril(L)
        return np.tril(np.abs(np.asarray(Al, dtype=LD) - ld_dot(L, L.T)))

    Lh = np.tril(L_hat)
    bound = gamma(n + 1) * np.tril(np.abs(Lh) @ np.abs(Lh.T))
    return within(what, resid(L_hat), bound, np.max(np.abs(Al)), None if L_ref64 is None else resid(L_ref64))


def check_substitute(what, X_hat, L, Bm, X_ref64=None):
    n = L.shape[0]
    L = np.tril(L)

    def resid(X):
        return np.abs(np.asarray(Bm, dtype=LD) - ld_dot(L, ld_dot(L.T, X)))

    g = gamma(n)
    bound = (2 * g + g * g) * (np.abs(L) @ (np.abs(L.T) @ np.abs(X_hat)))
    return within(what, resid(X_hat), bound, np.max(np.abs(Bm)), None if X_ref64 is None else resid(X_ref64))


def sym_from_lower(X):
    return np.tril(X) + np.tril(X, -1).T


def check_inverse(what, X_hat, L_hat, A, X_ref64=None):
    """|A X - I| <= 4 gamma_{n+1} |L||L^T||X| for the symmetric matrix of X's lower triangle; A the full symmetric input"""
    n = A.shape[0]
    L = np.tril(L_hat)

    def resid(X):
        return np.abs(ld_dot(A, sym_from_lower(X)) - np.eye(n, dtype=LD))

    bound = 4 * gamma(n + 1) * (np.abs(L) @ (np.abs(L.T) @ np.abs(sym_from_lower(X_hat))))
    return within(what, resid(X_hat), bound, 1.0, None if X_ref64 is None else resid(X_ref64))


def check_inverse_lower(what, X_hat, L_hat, X_ref64=None):
    """the statement about the lower triangle alone, against the factor it was computed from (module docstring)"""
    n = L_hat.shape[0]
    L = np.tril(L_hat)

    def resid(X):
        return np.abs(np.tril(np.eye(n, dtype=LD) - ld_dot(L, np.tril(ld_dot(L.T, np.tril(X))))))

    g = gamma(n)
    bound = (2 * g + g * g) * np.tril(np.abs(L) @ np.tril(np.abs(L.T) @ np.tril(np.abs(X_hat))))
    return within(what, resid(X_hat), bound, 1.0, None if X_ref64 is None else resid(X_ref64))


def check_rank1(what, A_hat, A0, u, q, A_ref64=None):
    live = np.outer(u != 0.0, u != 0.0)
    uu = np.outer(np.asarray(u, dtype=LD), np.asarray(u, dtype=LD)) * LD(q)
    ref = np.asarray(A0, dtype=LD) - uu
    bound = gamma(3) * (np.abs(A0) + np.abs(np.asarray(uu, dtype=np.float64)))
    err = np.where(live, np.abs(np.asarray(A_hat, dtype=LD) - ref), 0)
    err_ref = None if A_ref64 is None else np.where(live, np.abs(np.asarray(A_ref64, dtype=LD) - ref), 0)
    return within(what, err, np.where(live, bound, 0), np.max(np.abs(np.where(live, ref, 0)), initial=0.0), err_ref)


# ---- results of the restatement, computed once per (family, n) and shared --------------------------------------------------------------
_cache = {}


def ref_cholesky(family, n):
    key = ("chol", family, n)
    if key not in _cache:
        A = REAL_SPD[family](n)
        buf = pack(nan_upper(A, 0.0))
        assert cholesky(n, buf, 0) == 0
        buf.setflags(write=False)
        _cache[key] = (A, buf)
    return _cache[key]


def ref_inverse(family, n):
    key = ("inv", family, n)
    if key not in _cache:
        A = REAL_SPD[family](n)
        F = pack(A); X = np.zeros((n, n), order="F")
        assert inverse(n, F, X)
        F.setflags(write=False); X.setflags(write=False)
        _cache[key] = (A, F, X)
    return _cache[key]
