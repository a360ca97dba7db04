"""Cases and references for the kernels that decide about or rewrite the resident Q (xm_kernels.hip: edge_locate / diag_locate,
edge_write / diag_write and SellMatrix::refill behind Context.set_edge_weights, edge_residual, xm2_error / radix_hist / xm2_filter behind
Context.xm2_filter).  No GPU in here: tests/test_xm2_numpy.py checks the references against each other, tests/test_gpu_xm2_stages.py
holds the kernels to them.

The rewrite reference is exact by construction (one product per off-diagonal entry, one f64 sum in edge order per diagonal), so it is
compared bit for bit.  The residual reference is numpy.longdouble with an f64 restatement whose own error is e_ref.  The filter
reference works on the exact position h = (nlive - 1) * pct / 100 as a fractions.Fraction."""
from fractions import Fraction
import math

import numpy as np

import xm_testlib as tl

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
HALF_TURN = np.diag([1.0, -1.0, -1.0])          # |I - HALF_TURN|_F^2 = 8 exactly, every term an integer


def bound(e_ref):
    """the rule of xm_rtr_stages.py"""
    return max(16.0 * float(e_ref), 64.0 * EPS)


# ------------------------------------------------------------------------------------------------ graphs
def _graph(name, n, ei, ej, seed, **kw):
    ei = np.asarray(ei, dtype=np.int32); ej = np.asarray(ej, dtype=np.int32)
    M = tl.haar_so3(np.random.default_rng(seed), max(ei.size, 1))[: ei.size]
    return dict(name=name, n=int(n), ei=ei, ej=ej, M=np.ascontiguousarray(M), nodiag=(), extra=None, **kw)


def graph(name):
    """ei, ej (edge e = (ei[e], ej[e]), any order), M (ne, 3, 3) Haar rotations; nodiag: cameras whose diagonal block the BSR form does
    not store; extra: (row camera, column camera, 3x3 block) written into the created Q at a position that is no edge (and its mirror)"""
    if name == "pair":
        return _graph(name, 2, [0], [1], 1)
    if name in ("path255", "path256", "path257"):          # 256-thread boundary of the per-camera kernels (and of the per-edge ones)
        n = int(name[4:])
        return _graph(name, n, np.arange(n - 1), np.arange(1, n), n)
    if name == "cycle257":                                  # 257 edges: one past the 256-thread block; the closing edge is listed as (j, i)
        return _graph(name, 257, np.r_[np.arange(256), 256], np.r_[np.arange(1, 257), 0], 257)
    if name == "star100":                                   # one hub of degree 99: a long incidence list, a long row search
        hub, oth = 37, np.array([k for k in range(100) if k != 37])
        flip = oth % 2 == 1
        return _graph(name, 100, np.where(flip, oth, hub), np.where(flip, hub, oth), 100)
    if name in ("er86", "reversed"):                        # 258 rows: around the 256-column tile
        e, _ = tl.gen_vg_edges(86, 6, seed=86)
        if name == "er86":
            return _graph(name, 86, e[:, 0], e[:, 1], 86)
        rng = np.random.default_rng(87)
        p = rng.permutation(e.shape[0])
        e = e[p]
        flip = rng.permutation(e.shape[0]) < e.shape[0] // 2
        return _graph(name, 86, np.where(flip, e[:, 1], e[:, 0]), np.where(flip, e[:, 0], e[:, 1]), 87)
    if name == "isolated":                                  # cameras 9, 10, 11 have no edge; 10 has no stored diagonal block in BSR
        e, _ = tl.gen_vg_edges(9, 4, seed=9)
        g = _graph(name, 12, e[:, 0], e[:, 1], 12)
        g["nodiag"] = (10,)
        g["extra"] = (9, 11, np.random.default_rng(13).standard_normal((3, 3)))
        return g
    raise KeyError(name)


GRAPHS = ("pair", "path255", "path256", "path257", "cycle257", "star100", "er86", "reversed", "isolated")


def weight_sequences(g, codec=False):
    """[(name, w)] applied in order on one context.  codec=True (the stored block passes through block_to_quat, which squares its
    entries in f64 and so holds weights between about 2^-500 and 2^500): w4 spans 2^-300 .. 2^300 and there is no negative entry."""
    ne = g["ei"].size
    rng = np.random.default_rng(1000 + ne)
    w0 = rng.uniform(0.25, 4.0, ne)
    w1 = np.where(rng.uniform(size=ne) < 0.3, 0.0, w0)
    if ne > 1:
        w1[0] = 0.0; w1[ne - 1] = w0[ne - 1]
    deg = np.bincount(np.r_[g["ei"], g["ej"]], minlength=g["n"])
    cam = int(np.argmax(deg))
    w2 = np.where((g["ei"] == cam) | (g["ej"] == cam), 0.0, w0)
    w3 = np.zeros(ne)
    top = 300 if codec else 900
    w4 = np.ldexp(rng.uniform(1.0, 2.0, ne), rng.permutation(np.round(np.linspace(-top, top, ne)).astype(np.int64)))
    seq = [("w0", w0), ("w1", w1), ("w2", w2), ("w3", w3), ("w4", w4)]
    if not codec:
        wn = w0.copy(); wn[ne // 2] = -wn[ne // 2]
        seq.append(("wneg", wn))
    seq.append(("w5", w0.copy()))
    return seq


# ------------------------------------------------------------------------------------------------ the rewrite, exact
def diag_sums(g, w):
    """f64 sum of the incident weights of every camera, added in edge order (diag_write_kernel, build_viewgraph_csr)"""
    d = np.zeros(g["n"])
    for e in range(g["ei"].size):
        d[g["ei"][e]] += w[e]; d[g["ej"][e]] += w[e]
    return d


def rewrite_reference(g, w, extra=True):
    """dense Q after set_edge_weights(w): off-diagonal entries (-w_e) * M_e[k] (row j: the transpose), diagonals d * I, the rest as created"""
    n = g["n"]
    Q = np.zeros((3 * n, 3 * n))
    if extra and g["extra"] is not None:
        a, b, B = g["extra"]
        Q[3 * a:3 * a + 3, 3 * b:3 * b + 3] = B; Q[3 * b:3 * b + 3, 3 * a:3 * a + 3] = B.T
    for e in range(g["ei"].size):
        i, j = int(g["ei"][e]), int(g["ej"][e])
        B = (-w[e]) * g["M"][e]
        Q[3 * i:3 * i + 3, 3 * j:3 * j + 3] = B; Q[3 * j:3 * j + 3, 3 * i:3 * i + 3] = B.T
    d = diag_sums(g, w)
    for c in range(n):
        Q[3 * c:3 * c + 3, 3 * c:3 * c + 3] = d[c] * np.eye(3)
    return Q


def bsr_of(g, w, shuffle=None, nodiag=True):
    """3x3-block CSR of rewrite_reference(g, w, extra=False): both blocks of every edge, a diagonal block per camera except g["nodiag"];
    shuffle: a Generator that permutes the blocks inside every row (the contract does not ask for sorted rows)"""
    n, ei, ej = g["n"], g["ei"].astype(np.int64), g["ej"].astype(np.int64)
    skip = set(g["nodiag"]) if nodiag else set()
    dc = np.array([c for c in range(n) if c not in skip], dtype=np.int64)
    d = diag_sums(g, w)
    off = (-np.asarray(w))[:, None, None] * g["M"]
    rows = np.r_[dc, ei, ej]; cols = np.r_[dc, ej, ei]
    blocks = np.concatenate([d[dc, None, None] * np.eye(3)[None], off, np.transpose(off, (0, 2, 1))], axis=0).reshape(-1, 3, 3)
    order = np.lexsort((cols, rows))
    rows, cols, blocks = rows[order], cols[order], blocks[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    rowptr = np.cumsum(rowptr)
    if shuffle is not None:
        for r in range(n):
            p = rowptr[r] + shuffle.permutation(int(rowptr[r + 1] - rowptr[r]))
            cols[rowptr[r]:rowptr[r + 1]] = cols[p]; blocks[rowptr[r]:rowptr[r + 1]] = blocks[p]
    return rowptr, cols.astype(np.int32), np.ascontiguousarray(blocks)


def probe_columns(g, colours=False):
    """W (3n x 3 ncolours): identity columns packed by a distance-2 colouring of the cameras -- two cameras share a colour only if no row
    of the pattern (edges, diagonals, g["extra"]) holds a block of both.  Every column of Q meets exactly one 1 and every row of Q W sums one
    entry of Q and zeros: Q W is exact, equals reference @ W bit for bit, and an entry written outside the pattern shows up in it."""
    n = g["n"]
    adj = [{c} for c in range(n)]
    pairs = list(zip(g["ei"].tolist(), g["ej"].tolist())) + ([g["extra"][:2]] if g["extra"] is not None else [])
    for i, j in pairs:
        adj[i].add(j); adj[j].add(i)
    used, colour = [], np.zeros(n, dtype=np.int64)
    for c in sorted(range(n), key=lambda c: -len(adj[c])):
        for k, u in enumerate(used):
            if not (adj[c] & u):
                colour[c] = k; u |= adj[c]
                break
        else:
            colour[c] = len(used); used.append(set(adj[c]))
    W = np.zeros((3 * n, 3 * len(used)))
    for c in range(n):
        W[3 * c + np.arange(3), 3 * colour[c] + np.arange(3)] = 1.0
    return (W, colour) if colours else W


def probe_decode(g, P, colour):
    """Q from P = Q W of probe_columns: every block of the pattern taken from its probe columns; raises if P holds anything else"""
    n = g["n"]
    Q = np.zeros((3 * n, 3 * n))
    blocks = [(c, c) for c in range(n)] + list(zip(g["ei"].tolist(), g["ej"].tolist())) + list(zip(g["ej"].tolist(), g["ei"].tolist()))
    if g["extra"] is not None:
        blocks += [g["extra"][:2], g["extra"][:2][::-1]]
    for i, j in blocks:
        Q[3 * i:3 * i + 3, 3 * j:3 * j + 3] = P[3 * i:3 * i + 3, 3 * colour[j]:3 * colour[j] + 3]
    W = np.zeros_like(P)
    for c in range(n):
        W[3 * c + np.arange(3), 3 * colour[c] + np.arange(3)] = 1.0
    if not np.array_equal(Q @ W, P):
        raise AssertionError("the product holds entries outside the pattern")
    return Q


# ------------------------------------------------------------------------------------------------ residuals
def residual_points(g):
    """[(name, M, rot (3 x 3n), scale (n))]: Haar rotations with scales in [0.5, 2]; the exact solution of noise-free measurements (the
    result is round-off through cancellation); scales of 1e-150 and of 1e150"""
    n, ei, ej = g["n"], g["ei"], g["ej"]
    rng = np.random.default_rng(5000 + n)
    Rs = tl.haar_so3(rng, n)
    rot_h = np.concatenate(list(tl.haar_so3(rng, n)), axis=1)
    s_h = rng.uniform(0.5, 2.0, n)
    M0 = Rs[ei] @ np.transpose(Rs[ej], (0, 2, 1))
    rot0 = np.concatenate([Rs[0] @ Rs[k].T for k in range(n)], axis=1)      # anchored: the camera's record is its transpose
    return [("haar", g["M"], rot_h, s_h), ("exact", M0, rot0, np.ones(n)), ("tiny", g["M"], rot_h, 1e-150 * s_h), ("huge", g["M"], rot_h, 1e150 * s_h)]


def residual_reference(g, M, rot, scale, dtype=LD):
    """(res, mag): res[e] = |Y_i - M_e Y_j|_F^2 with Y_i = s_i rot[:, 3i:3i+3]^T, mag[e] = |Y_i|_F^2 + |M_e Y_j|_F^2, in `dtype`"""
    n = g["n"]
    Y = (np.asarray(scale, dtype=dtype)[:, None, None] * np.transpose(np.asarray(rot, dtype=dtype).reshape(3, n, 3), (1, 2, 0)))
    Md = np.asarray(M, dtype=dtype)
    Yi, Yj = Y[g["ei"]], Y[g["ej"]]
    MY = np.zeros_like(Yi)
    for a in range(3):
        for k in range(3):
            MY[:, a, k] = Md[:, a, 0] * Yj[:, 0, k] + Md[:, a, 1] * Yj[:, 1, k] + Md[:, a, 2] * Yj[:, 2, k]
    D = Yi - MY
    return (D * D).sum(axis=(1, 2)), (Yi * Yi).sum(axis=(1, 2)) + (MY * MY).sum(axis=(1, 2))


def rel_err(x, ref, mag):
    """max over the edges of |x - ref| / mag (longdouble), as a float"""
    return float(np.max(np.abs(np.asarray(x, dtype=LD) - ref) / mag))


# ------------------------------------------------------------------------------------------------ the filter
def filter_reference(err, live, pct):
    """dict(k0, frac, x0, x1, thr (longdouble), integral, removed (bool per entry)) for the live errors err[live] at percentile pct:
    position h = (nlive - 1) * pct / 100 exactly, threshold x[floor h] + frac(h) (x[floor h + 1] - x[floor h]), removed = live & err > thr"""
    err = np.asarray(err, dtype=np.float64); live = np.asarray(live, dtype=bool)
    x = np.sort(err[live])
    nl = x.size
    h = Fraction(nl - 1) * Fraction(pct) / 100
    k0 = math.floor(h)
    fr = h - k0
    k1 = min(k0 + 1, nl - 1) if fr != 0 else k0             # an integral position asks for one order statistic
    x0, x1 = x[k0], x[k1]
    thr = LD(x0) + (LD(fr.numerator) / LD(fr.denominator)) * (LD(x1) - LD(x0))
    return dict(k0=k0, frac=fr, x0=float(x0), x1=float(x1), thr=thr, integral=(fr == 0), removed=live & (err.astype(LD) > thr))


def position_f64(nlive, pct):
    """(floor h, frac h) of h = (nlive - 1) * pct / 100 as the library computes them in f64: the product as an exact pair hi + lo (fma), the
    floor from hi / 100 corrected by the exact remainder, the fraction (remainder + lo) / 100 -- two roundings"""
    a = float(nlive - 1)
    hi = a * pct
    lo = float(Fraction(a) * Fraction(pct) - Fraction(hi))      # what fma(a, pct, -hi) returns: the difference is a double
    k = int(math.floor(hi / 100.0))
    r = (hi - 100.0 * k) + lo
    while r < 0.0:
        k -= 1; r += 100.0
    while r >= 100.0:
        k += 1; r -= 100.0
    return k, r / 100.0


def thr_bound(ref):
    """three roundings of magnitude at most max(x0, x1) in x0 + t (x1 - x0), doubled; nothing where the threshold is an order statistic"""
    return 0.0 if ref["x0"] == ref["x1"] else 4.0 * EPS * max(ref["x0"], ref["x1"])


def radix_select_numpy(x, k):
    """numpy statement of the device select (radix_hist_kernel + the host loop of radix_select): the k-th smallest (0-based) of the
    non-negative doubles x by four passes over 16 bits of the pattern, most significant first"""
    key = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    prefix = 0
    for p in range(4):
        shift = 48 - 16 * p
        sel = key if p == 0 else key[(key >> np.uint64(shift + 16)) == np.uint64(prefix)]
        hist = np.bincount(((sel >> np.uint64(shift)) & np.uint64(0xffff)).astype(np.int64), minlength=65536)
        c = np.cumsum(hist)
        b = int(np.searchsorted(c, k, side="right"))
        b = min(b, 65535)
        k -= int(c[b - 1]) if b > 0 else 0
        prefix = (prefix << 16) | b
    return float(np.array([prefix], dtype=np.uint64).view(np.float64)[0])


def complete_graph(ne):
    """(n, ei, ej): the first ne edges (i < j) of the complete graph on the fewest cameras that has them (at most 50 for ne <= 1000)"""
    n = 2
    while n * (n - 1) // 2 < ne:
        n += 1
    iu = np.triu_indices(n, 1)
    return n, iu[0][:ne].astype(np.int32), iu[1][:ne].astype(np.int32)


NE = (1, 2, 3, 11, 101, 256, 257, 1000)
PCTS = (0.0, 50.0, 90.0, 95.0, 100.0)


def design(name, ne):
    """dict(w (ne weights), half (bool: M_e is the half turn, res_e = 8; else M_e = I, res_e = 0), pcts, pre (weights already removed
    before the call: the filter runs with nz > 0)).  err_e = 8 w_e for half-turn edges, bit for bit."""
    rng = np.random.default_rng(7000 + ne)
    half = np.ones(ne, dtype=bool)
    pcts = list(PCTS)
    if ne in (11, 101):                                     # the integral positions, 70 among them (where numpy lands one lower at n = 91)
        pcts += [float(p) for p in (range(10, 100, 10) if ne == 11 else (1, 35, 57, 70, 99))]
    if name == "uniform":
        w = rng.permutation(ne) * 0.125 + rng.uniform(1.0, 1.0625, ne)          # distinct, spaced by about 1/8
    elif name == "exp":                                     # one value per binade from 2^-500 to 2^500: decided in the first pass
        w = np.ldexp(rng.uniform(1.0, 2.0, ne), rng.permutation(np.round(np.linspace(-500, 500, ne)).astype(np.int64)))
        if ne > 1001:
            raise ValueError("one value per binade")
    elif name == "low16":                                   # neighbours one ulp apart: decided in the last pass
        w = 1.375 * (1.0 + rng.permutation(ne) * 2.0 ** -52)
        pcts = [p for p in pcts if (Fraction(ne - 1) * Fraction(p) / 100).denominator == 1]
    elif name == "ties":
        w = np.array([0.75, 1.5, 3.0])[rng.integers(0, 3, ne)]
    elif name == "allequal":
        w = np.full(ne, 1.25)
    elif name == "subnormal":                               # err = 8 k 2^-1074
        w = (1 + rng.permutation(ne)) * 2.0 ** -1074
        # below 2^-1022 the rounding unit is the absolute 2^-1074 and a relative bound is empty: the positions kept are those whose exact
        # threshold x0 + frac * 8 * 2^-1074 is a double (frac a multiple of 1/8), where the bound asks for that double
        pcts = [p for p in pcts if ((Fraction(ne - 1) * Fraction(p) / 100) * 8).denominator == 1]
    elif name == "livezero":                                # live edges with error exactly 0 (M = I, positive weight) beside removed ones
        w = rng.permutation(ne) * 0.125 + rng.uniform(1.0, 1.0625, ne)
        half = rng.uniform(size=ne) < 0.6
        half[0] = True
        w = np.where(rng.uniform(size=ne) < 0.2, 0.0, w)
        w[0] = 2.0
    else:
        raise KeyError(name)
    return dict(w=np.ascontiguousarray(w, dtype=np.float64), half=half, pcts=pcts)


DESIGNS = ("uniform", "exp", "low16", "ties", "allequal", "subnormal", "livezero")


def design_errors(d):
    """(err, live) of a design: err_e = 8 w_e on half-turn edges, 0 elsewhere and for removed edges"""
    w = d["w"]
    return np.where(d["half"] & (w != 0.0), 8.0 * w, 0.0), w != 0.0


def design_M(d):
    return np.where(d["half"][:, None, None], HALF_TURN[None], np.eye(3)[None]).copy()


def symmetric_base(n, seed=None):
    """exactly symmetric random 3n x 3n matrix without a zero entry"""
    rng = np.random.default_rng(900 + n if seed is None else seed)
    A = rng.standard_normal((3 * n, 3 * n))
    Q = A + A.T
    assert np.array_equal(Q, Q.T) and np.all(Q != 0.0)
    return Q


def sym_positions(m):
    """the (row, column) positions of the symmetry cases that exist in an m x m matrix"""
    cand = [(1, 0), (m - 1, 0), (m - 1, m - 2), (0, m - 1), (63, 64), (64, 63), (65, 0), (m - 1, 64 * ((m - 1) // 64)), (127, 128)]
    out = []
    for r, c in cand:
        if 0 <= r < m and 0 <= c < m and r != c and (r, c) not in out:
            out.append((r, c))
    return out
