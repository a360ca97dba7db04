"""CPU test of the host export xm_tridiag_min -- the certificate's own eigen-solve of the Lanczos tridiagonal matrix (tridiag_min and sturm_count
of xm_solver.hip: Sturm bisection, inverse iteration) -- against numpy's eigvalsh / eigh of the same matrix.

theta: |theta - eig_min| <= 8e-16 max(1, tmax).  The bisection stops at an interval of 4e-16 max(1, tmax) and returns its midpoint (2e-16 of
that unit); the rest is the margin for the Sturm count's own rounding, which moves the place where the count changes by a few eps tmax, and for
eigvalsh's.  y: |T y - theta y| against the residual of eigh's eigenvector on the same matrix with its own eigenvalue, e <= max(16 e_ref, 64 eps),
both over tmax (never under 1, the unit theta is resolved in); |y| = 1 and finite."""
import numpy as np
import pytest

import xm_ba_stages as st
import xm_rtr_exact as ex


def _wilkinson(k):
    return np.abs(np.arange(-k, k + 1)).astype(float), np.ones(2 * k)


def _close_pair():
    """two decoupled-looking halves whose smallest eigenvalues differ by 1e-13, joined by a weak link"""
    a = np.array([1.0, 3.0, 5.0, 1.0 + 1e-13, 3.5, 6.0])
    b = np.array([0.0, 0.5, 0.0, 0.0, 0.25])
    return a, b


def _matrices():
    rng = np.random.default_rng(11)
    M = {"m1": (np.array([-2.5]), np.zeros(0)), "m2": (np.array([1.0, -1.0]), np.array([0.5])), "m3": (np.array([2.0, 3.0, 4.0]), np.array([1.0, 1.0])),
         "wilkinson21": _wilkinson(10), "close-pair-1e-13": _close_pair(),
         "split": (rng.standard_normal(9), np.concatenate([rng.standard_normal(4), [0.0], rng.standard_normal(3)])),
         "zero-diagonal": (np.zeros(12), rng.uniform(0.5, 2.0, 11)),
         "random-1200": (rng.standard_normal(1200), rng.standard_normal(1199))}
    a, b = rng.standard_normal(40), rng.standard_normal(39)
    M["scaled-1e-150"] = (a * 1e-150, b * 1e-150)
    M["scaled-1e+150"] = (a * 1e150, b * 1e150)
    return M


MATRICES = _matrices()


@pytest.mark.parametrize("name", list(MATRICES))
def test_smallest_eigenpair_against_numpy(xmamd, name):
    a, b = MATRICES[name]
    m = a.size
    theta, y, tmax = xmamd.tridiag_min(a, b)
    T = np.diag(a) + np.diag(b, 1) + np.diag(b, -1)
    ev, evec = np.linalg.eigh(T)
    lo, hi, tmax_ref = ex.tridiag_bounds(a, np.append(b, 0.0))
    assert tmax == pytest.approx(float(tmax_ref), rel=4 * st.EPS, abs=0.0)
    unit = max(1.0, tmax)
    print(f"TRIDIAG {name}: m {m}, theta - eig_min {theta - ev[0]:.3e} (allowed {8e-16 * unit:.3e})")
    assert abs(theta - ev[0]) <= 8e-16 * unit
    assert np.isfinite(y).all() and abs(np.sqrt(y @ y) - 1.0) <= 4 * st.EPS
    r, r_ref = np.abs(T @ y - theta * y).max() / unit, np.abs(T @ evec[:, 0] - ev[0] * evec[:, 0]).max() / unit
    print(f"STAGE_ERR tridiag-{name} residual: e_ref {r_ref:.3e}, e_gpu {r:.3e}, ratio {r / st.bound(r_ref):.3f}")
    assert r <= st.bound(r_ref)
    if m == 1:
        assert theta == a[0] and y[0] == 1.0


def test_restatement_agrees_with_the_export(xmamd):
    """tests/xm_rtr_exact.tridiag_min (what the reference's whole run stops by) run in f64 gives the export's theta to the bisection's interval and
    its vector up to sign"""
    for name in ("m2", "m3", "wilkinson21", "split", "zero-diagonal"):
        a, b = MATRICES[name]
        theta, y, tmax = xmamd.tridiag_min(a, b)
        t2, y2, tmax2 = ex.tridiag_min(a, np.append(b, 0.0), np.float64)
        assert abs(theta - float(t2)) <= 4e-16 * max(1.0, tmax) and float(tmax2) == pytest.approx(tmax, rel=4 * st.EPS)
        assert min(np.abs(y - y2).max(), np.abs(y + y2).max()) <= 1e-6, name


def test_refusals(xmamd):
    L = xmamd.lib()
    a = np.ones(3)
    out = np.zeros(3)
    import ctypes as C
    th, tm = C.c_double(), C.c_double()
    assert L.xm_tridiag_min(a.ctypes.data_as(C.c_void_p), None, 3, C.byref(th), out.ctypes.data_as(C.c_void_p), C.byref(tm)) == -2
    assert L.xm_tridiag_min(a.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), 0, C.byref(th), out.ctypes.data_as(C.c_void_p), C.byref(tm)) == -2
