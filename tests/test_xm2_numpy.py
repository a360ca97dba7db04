"""The references of tests/xm_xm2_exact.py checked against each other and against the conditions the GPU tests rely on (no GPU)."""
from fractions import Fraction

import numpy as np
import pytest

import xm_testlib as tl
import xm_xm2_exact as xx

LD = np.longdouble


@pytest.mark.parametrize("name", xx.GRAPHS)
def test_rewrite_reference_against_the_assemblers_and_a_longdouble_sum(name):
    """the exact rewrite equals tl.vg_from_edges bit for bit (same products, diagonal sums in edge order) and tl.vg_assemble in every
    off-diagonal entry; its diagonals are within the summation bound of a longdouble sum; it is symmetric bit for bit; bsr_of, sorted or
    shuffled, holds the same matrix"""
    g = xx.graph(name)
    n, ei, ej = g["n"], g["ei"], g["ej"]
    for wname, w in xx.weight_sequences(g):
        Q = xx.rewrite_reference(g, w, extra=False)
        assert np.array_equal(Q, Q.T)
        assert np.array_equal(Q, tl.bsr_to_dense(n, *tl.vg_from_edges(n, ei, ej, w, g["M"]))), wname
        Qa = tl.bsr_to_dense(n, *tl.vg_assemble(n, np.stack([ei, ej], axis=1), g["M"], w))
        offd = np.kron(1 - np.eye(n), np.ones((3, 3))).astype(bool)
        assert np.array_equal(Q[offd], Qa[offd])
        d = xx.diag_sums(g, w)
        dl = np.zeros(n, dtype=LD); sa = np.zeros(n)
        np.add.at(dl, ei, w.astype(LD)); np.add.at(dl, ej, w.astype(LD)); np.add.at(sa, ei, np.abs(w)); np.add.at(sa, ej, np.abs(w))
        deg = np.bincount(np.r_[ei, ej], minlength=n)
        assert np.all(np.abs(d.astype(LD) - dl) <= deg * xx.EPS * sa) and np.all(np.abs(np.diag(Qa)[::3] - d) <= 2 * deg * xx.EPS * sa)
        for sh in (None, np.random.default_rng(3)):
            rp, ci, bl = xx.bsr_of(g, w, shuffle=sh)
            assert np.array_equal(tl.bsr_to_dense(n, rp, ci, bl), Q)
            assert rp[-1] == 2 * ei.size + n - len(g["nodiag"])
    assert np.array_equal(xx.weight_sequences(g)[0][1], xx.weight_sequences(g)[-1][1])      # w5 is w0 again
    # the packed identity columns: every row of Q W is one entry of Q, so the probe holds every stored entry once and nothing is summed
    W = xx.probe_columns(g)
    Q = xx.rewrite_reference(g, xx.weight_sequences(g)[4][1])
    assert np.all(W.sum(axis=1) == 1.0) and W.shape[1] % 3 == 0
    P = Q @ W
    assert np.array_equal(np.sort(np.abs(P[P != 0.0])), np.sort(np.abs(Q[Q != 0.0])))
    assert np.all(((Q != 0.0).astype(int) @ W) <= 1)
    if g["extra"] is not None:
        a, b, B = g["extra"]
        assert not ((ei == a) & (ej == b)).any() and not ((ei == b) & (ej == a)).any() and np.all(B != 0.0)


def test_graphs_sit_where_the_kernels_can_go_wrong():
    G = {k: xx.graph(k) for k in xx.GRAPHS}
    assert G["pair"]["ei"].size == 1 and G["path257"]["ei"].size == 256 and G["cycle257"]["ei"].size == 257
    assert [G[k]["n"] for k in ("path255", "path256", "path257")] == [255, 256, 257]
    deg = np.bincount(np.r_[G["star100"]["ei"], G["star100"]["ej"]], minlength=100)
    assert deg.max() == 99 and (G["star100"]["ei"] > G["star100"]["ej"]).any() and (G["star100"]["ei"] < G["star100"]["ej"]).any()
    assert 3 * G["er86"]["n"] == 258
    r = G["reversed"]
    assert (r["ei"] > r["ej"]).sum() == r["ei"].size // 2 and not np.all(np.diff(np.minimum(r["ei"], r["ej"])) >= 0)
    assert {tuple(sorted(p)) for p in zip(r["ei"], r["ej"])} == {tuple(p) for p in zip(G["er86"]["ei"], G["er86"]["ej"])}
    i = G["isolated"]
    assert not np.isin([9, 10, 11], np.r_[i["ei"], i["ej"]]).any() and i["nodiag"] == (10,)
    for g in G.values():
        M = g["M"]
        assert np.abs(M @ np.transpose(M, (0, 2, 1)) - np.eye(3)).max() < 1e-14 and np.all(np.linalg.det(M) > 0)
        for wname, w in xx.weight_sequences(g):
            assert np.all(np.isfinite(xx.rewrite_reference(g, w))), wname
    w4 = dict(xx.weight_sequences(G["er86"]))["w4"]
    assert w4.min() < 2.0 ** -899 and w4.max() >= 2.0 ** 900
    assert sum((w < 0).sum() for _, w in xx.weight_sequences(G["er86"])) == 1
    assert all((w >= 0).all() and w.max() < 2.0 ** 301 for _, w in xx.weight_sequences(G["er86"], codec=True))


@pytest.mark.parametrize("name", ["pair", "cycle257", "reversed"])
def test_residual_references(name):
    """the f64 restatement against longdouble: e_ref stays at round-off relative to |Y_i|^2 + |M Y_j|^2 at every point, also through the
    cancellation at the exact solution and at scales of 1e-150 and 1e150; a numpy einsum agrees"""
    g = xx.graph(name)
    for pname, M, rot, scale in xx.residual_points(g):
        ref, mag = xx.residual_reference(g, M, rot, scale)
        r64, _ = xx.residual_reference(g, M, rot, scale, dtype=np.float64)
        e_ref = xx.rel_err(r64, ref, mag)
        assert e_ref <= 16 * xx.EPS, (pname, e_ref)
        assert np.all(np.isfinite(r64)) and np.all(r64 >= 0)
        if pname == "exact":
            assert float(np.max(ref / mag)) < 1e-28              # noise-free: the residual is nothing but round-off
        Y = scale[:, None, None] * np.transpose(rot.reshape(3, g["n"], 3), (1, 2, 0))
        r2 = np.sum((Y[g["ei"]] - M @ Y[g["ej"]]) ** 2, axis=(1, 2))
        assert xx.rel_err(r2, ref, mag) <= 16 * xx.EPS


def test_half_turn_residual_is_exactly_eight():
    I = np.eye(3)
    assert np.sum((I - xx.HALF_TURN @ I) ** 2) == 8.0 and np.sum((I - I @ I) ** 2) == 0.0
    g = dict(n=2, ei=np.array([0]), ej=np.array([1]))
    r, _ = xx.residual_reference(g, xx.HALF_TURN[None], np.tile(I, 2), np.ones(2), dtype=np.float64)
    assert r[0] == 8.0


@pytest.mark.parametrize("name", xx.DESIGNS)
def test_filter_designs(name):
    """every design at every edge count and percentile: 8 w is exact; the four-pass select equals sorting at every order statistic the
    filter needs; no live error lies within the threshold's bound of the exact threshold without being bit-equal to it, so the removed
    set follows from the reference alone; at pct = 90 numpy's percentile removes the same set"""
    for ne in xx.NE:
        d = xx.design(name, ne)
        w = d["w"]
        assert np.array_equal((8.0 * w).astype(LD), 8 * w.astype(LD)) and np.all(np.isfinite(8.0 * w)) and np.all(w >= 0)
        err, live = xx.design_errors(d)
        nz = int((~live).sum())
        xs = np.sort(err[live])
        if name == "uniform":
            assert np.unique(err).size == ne
        if name == "exp":
            assert np.unique(np.frexp(err)[1]).size == ne
        if name == "low16":
            assert ne == 1 or np.unique(err.view(np.uint64) >> np.uint64(16)).size <= 2
        if name == "subnormal":
            assert err.max() < 2.0 ** -1022 and err.min() > 0
        if name == "livezero" and ne >= 11:
            assert nz > 0 and (err[live] == 0.0).any()
        assert d["pcts"]
        for pct in d["pcts"]:
            ref = xx.filter_reference(err, live, pct)
            for k in {ref["k0"], min(ref["k0"] + 1, xs.size - 1)}:
                assert xx.radix_select_numpy(err, k + nz) == xs[k]
            b = xx.thr_bound(ref)
            near = live & (np.abs(err.astype(LD) - ref["thr"]) <= b)
            assert np.all(err[near].astype(LD) == ref["thr"]), (ne, pct)
            if ref["integral"] or ref["x0"] == ref["x1"]:
                assert ref["thr"] == ref["x0"]
            if name == "subnormal":
                assert float(ref["thr"]) == ref["thr"]            # representable: below 2^-1022 the relative bound would be empty
            assert not ref["removed"][~live].any()
            if pct == 90.0:
                assert np.array_equal(ref["removed"], live & (err > np.percentile(err[live], 90.0)))
            if pct == 100.0:
                assert not ref["removed"].any()


def test_the_select_on_patterns_that_share_prefixes():
    rng = np.random.default_rng(0)
    x = np.r_[np.zeros(7), 1.375 * (1 + rng.permutation(300) * 2.0 ** -52), 1.375 * (1 + rng.permutation(300) * 2.0 ** -20), rng.uniform(0, 1e-300, 50),
              2.0 ** -1074 * np.arange(1, 40), np.full(9, 3.0)]
    s = np.sort(x)
    for k in range(x.size):
        assert xx.radix_select_numpy(x, k) == s[k]
    # what a weight of -0.0 did before it was taken for 0: its error -0.0 sorts behind every positive pattern
    y = np.r_[-0.0, 1.0, 2.0, 3.0]
    assert np.signbit(xx.radix_select_numpy(y, 3)) and xx.radix_select_numpy(y, 0) == 1.0


def test_exact_position_and_numpy():
    """the contract is the exact position (n - 1) pct / 100.  The f64 formula of the library, (double)(n - 1) * pct / 100.0, decides like
    exact rational arithmetic at every n <= 4000 for the percentiles below; numpy's (n - 1) * (pct / 100) lands one element lower at some
    (n, 70) -- an observation about the numpy at hand, printed, asserting nothing about the library"""
    for pct in (90.0, 95.0, 50.0, 10.0, 30.0, 99.0, 0.1, 99.9, 70.0, 35.0, 57.0):
        for n in range(1, 4001):
            h = Fraction(n - 1) * Fraction(pct) / 100
            hq = float(n - 1) * pct / 100.0
            assert int(np.floor(hq)) == h.numerator // h.denominator, (n, pct)
    # the fraction is what the plain formula loses: hq - floor(hq) carries the rounding of hq, n * eps of the gap between the neighbours
    # (n = 257, pct = 90: 0.4000000000000057 for 2/5).  The library's pair arithmetic keeps floor and fraction to two roundings.
    worst_plain = worst_pair = 0.0
    for pct in (90.0, 95.0, 50.0, 10.0, 30.0, 99.0, 0.1, 99.9, 70.0, 35.0, 57.0, 100.0, 0.0, 1e-300, 99.99999999999999):
        for n in list(range(1, 400)) + [1000, 4000, 10 ** 6 + 1, 2 ** 31, 2 ** 40 + 3]:
            h = Fraction(n - 1) * Fraction(pct) / 100
            k, fr = xx.position_f64(n, pct)
            assert k == h.numerator // h.denominator and 0.0 <= fr < 1.0
            exact = h - k
            assert abs(Fraction(fr) - exact) <= 2 * Fraction(xx.EPS) * exact, (n, pct)
            hq = float(n - 1) * pct / 100.0
            if exact:
                worst_plain = max(worst_plain, float(abs(Fraction(hq - np.floor(hq)) - exact) / exact))
                worst_pair = max(worst_pair, float(abs(Fraction(fr) - exact) / exact))
    assert worst_pair <= 2 * xx.EPS < 1e-6 < worst_plain
    assert float(256) * 90.0 / 100.0 - 230 == 0.4000000000000057 and xx.position_f64(257, 90.0) == (230, 0.4)
    x = np.arange(91.0)
    ref = xx.filter_reference(x, np.ones(91, dtype=bool), 70.0)
    assert ref["integral"] and ref["k0"] == 63 and ref["thr"] == 63.0 and ref["removed"].sum() == 27
    pos = 90 * (70.0 / 100)
    print(f"numpy {np.__version__}: position of pct 70 at n 91 = {pos!r}, np.percentile = {np.percentile(x, 70.0)!r}, removes {(x > np.percentile(x, 70.0)).sum()}")
    for pct in (90.0, 95.0, 50.0, 10.0, 30.0, 99.0):
        for n in range(1, 4001):
            h = Fraction(n - 1) * Fraction(pct) / 100
            assert int(np.floor((n - 1) * (pct / 100))) == h.numerator // h.denominator


def test_symmetry_cases():
    for n in (1, 21, 22, 43, 64, 86):
        Q = xx.symmetric_base(n)
        m = 3 * n
        pos = xx.sym_positions(m)
        assert all(r != c and r < m and c < m for r, c in pos)
        if m >= 129:
            assert {(63, 64), (64, 63), (65, 0), (127, 128)} <= set(pos)
            assert m - 1 == 64 * ((m - 1) // 64) or (m - 1, 64 * ((m - 1) // 64)) in pos      # m = 129: that position is the diagonal
        Q2 = Q.copy(); Q2[pos[0]] = np.nextafter(Q2[pos[0]], np.inf)
        assert not np.array_equal(Q2, Q2.T)
    assert [3 * n for n in (1, 21, 22, 43, 64)] == [3, 63, 66, 129, 192]
