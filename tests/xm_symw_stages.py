"""Reference of the multi-rank symmetric window product (xm-code_amd/csrc/xm_symw.h, xm_symw.hip), stage by stage, for
tests/test_symw_plan.py (CPU) and tests/test_gpu_symw_stages.py (through the test export xm_symw_probe).

The model restates the three kernels in numpy in any of three arithmetics -- int64 (integer-valued data: every sum is exact in any order, the
kernels must give these bits), longdouble (the truth for real-valued data) and float64 (what plain double arithmetic loses on the same data:
e_ref) -- and returns next to every value the sum of |q| |w| over its addends, the scale its error is measured in:
    Prow[s, 6 j + r, k]   row-direction sum of local row 6 j + r over the columns of strip s, masks of row step t0 + j       (qw_symw_kernel)
    Pcol[i, c, k]         column-direction sums of work item i: its steps added in order, per column of its strip                   (qw_symw_kernel)
    csum                  per column, the items of its strip added up                                                          (symw_colsum_kernel)
    Y                     alpha * (row sums of the strips the step touches + every rank's column sums)                         (symw_reduce_kernel)
The masks come from the predicates of xm_symw.h, restated here (use_block, any_pair, full_pair); tests/test_symw_plan.py holds use_block
against the library's xm_symw_use and the work lists of xm_symw_plan against any_pair.

Bound for real-valued data: tests/xm_ba_stages.py's -- the error against longdouble, per entry over the entry's sum of |q| |w|, must stay
below max(16 e_ref, 64 eps) with e_ref the float64 model's error measured the same way.  Nothing here is measured from the kernels."""
import numpy as np

import xm_la_stages as la
from xm_ba_stages import bound

STRIP = 256
OS = (1, 3, 4, 5)
KS = (0, 1, 2, 3, 5)
ALPHAS = (1.0, -2.5)
# (ntot, worlds): the smallest shapes at which each thing can go wrong; test_gpu_symw_stages.py::test_case_list_reaches_every_path proves what they reach
CASES = ((2, (1,)),               # the diagonal block alone
         (4, (1, 2)),             # T = 2: the tie
         (6, (1, 3)),
         (84, (1, 2, 3, 6)),      # one strip (252 columns) with four padding columns inside it
         (86, (1,)),              # strip 1 holds two real columns, its second half lies outside ld = 384; step 42 straddles strips 0 and 1
         (128, (1, 2, 4)),        # 384 = ld: a last strip of exactly one half, no padding
         (130, (1, 5)),           # ld = 512: real and padding columns together in the second half of strip 1
         (140, (70,)),            # nstrips + world = 72 > 64: the reducer's second trip
         (256, (2, 4, 8)),        # three whole strips, even T
         (258, (1, 3)),           # odd T
         (344, (1, 2, 4)))        # Th = 86: whole strips inside the window (the unmasked path), the window wraps over the matrix end
LARGE = (256, 258, 344)           # K in KS here: items of 1 .. 5 steps
NT_NTOT = 344                     # both load policies here
SCAL_CASE = (130, 5)


def case_ids():
    return [(ntot, world) for ntot, worlds in CASES for world in worlds]


def dense_ld(ntot):
    return (3 * ntot + 127) // 128 * 128


# ---- the predicates of xm_symw.h ---------------------------------------------------------------------------------------------------------
def use_block(g, t, u):
    """block (t, u), t != u: used by row step t?"""
    d = (u - t) % g["T"]
    return (0 < d < g["Th"]) or bool(g["tie"] and d == g["Th"] and t < u)


def strip_steps(g, s):
    return (s * STRIP) // 6, min((s * STRIP + STRIP - 1) // 6, g["T"] - 1)


def any_pair(g, t, s):
    """may row step t use anything of strip s (the one predicate the planner, the sweep and the reducer share)?"""
    lo, hi = strip_steps(g, s)
    if lo > g["T"] - 1:
        return False
    dlo, dhi = (lo - t) % g["T"], (hi - t) % g["T"]
    return dlo > dhi or dlo <= g["Th"]


def full_pair(g, t, s):
    """is every column of strip s used by row step t in both directions (the sweep's unmasked path)?"""
    lo, hi = strip_steps(g, s)
    if lo > g["T"] - 1 or s * STRIP + STRIP > 6 * g["T"]:
        return False
    dlo, dhi = (lo - t) % g["T"], (hi - t) % g["T"]
    return dlo <= dhi and 0 < dlo and dhi < g["Th"]


def use_matrix(T):
    g = dict(T=T, Th=(T + 1) // 2, tie=1 if T % 2 == 0 else 0)
    return np.array([[use_block(g, t, u) for u in range(T)] for t in range(T)], dtype=bool)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def rank_pairs(Qr, W, g, use, dtype=np.float64):
    """the sweep of one rank, per (strip, local step) pair with any_pair: Qr the rank's strip (3 nloc x 3 ntot), use the T x T matrix of
    use_block (or of the library's xm_symw_use).  -> (row, col, row_scale, col_scale): dicts (s, j) -> 6 x o row-direction sums /
    ncol x o column-direction sums (ncol: the real columns of the strip) and the sums of |q| |w| behind them"""
    Qd, Wd = np.asarray(Qr).astype(dtype), np.asarray(W).astype(dtype)
    Qa, Wa = np.abs(Qd), np.abs(Wd)
    M = Wd.shape[0]
    row, col, rows, cols = {}, {}, {}, {}
    for s in range(g["nstrips"]):
        c0, c1 = s * STRIP, min(s * STRIP + STRIP, M)
        ucol = np.arange(c0, c1) // 6
        for j in range(g["nsteps"]):
            t = g["t0"] + j
            if not any_pair(g, t, s):
                continue
            mc = (use[t, ucol] & (ucol != t)).astype(dtype)
            mr = (use[t, ucol] | (ucol == t)).astype(dtype)
            B, Ba = Qd[6 * j:6 * j + 6, c0:c1], Qa[6 * j:6 * j + 6, c0:c1]
            row[(s, j)] = (B * mr) @ Wd[c0:c1]                     # row direction -> this rank's rows
            rows[(s, j)] = (Ba * mr) @ Wa[c0:c1]
            col[(s, j)] = (B * mc).T @ Wd[6 * t:6 * t + 6]         # column direction -> whoever owns those cameras
            cols[(s, j)] = (Ba * mc).T @ Wa[6 * t:6 * t + 6]
    return row, col, rows, cols


def rank_stages(pairs, g, items, o, M, dtype=np.float64):
    """the buffers of one rank from rank_pairs' output and the work list (xm_symw_plan's items): Prow (nstrips x 6 nsteps x o; NaN where
    the sweep writes nothing), Pcol (items x 256 x o; zero in the padding columns), csum (M x o) and the scales of the three"""
    row, col, rows, cols = pairs
    nan = np.nan if dtype != np.int64 else 0
    Prow = np.full((g["nstrips"], 6 * g["nsteps"], o), nan, dtype=dtype); Prow_s = np.zeros(Prow.shape, dtype=np.float64 if dtype == np.int64 else dtype)
    written = np.zeros((g["nstrips"], 6 * g["nsteps"]), dtype=bool)
    for s, jb, je in items:                                        # what the work list does not name stays unwritten (the reducer reads by any_pair)
        for j in range(jb, je):
            Prow[s, 6 * j:6 * j + 6] = row[(int(s), j)]; Prow_s[s, 6 * j:6 * j + 6] = rows[(int(s), j)]; written[s, 6 * j:6 * j + 6] = True
    Pcol = np.zeros((len(items), STRIP, o), dtype=dtype); Pcol_s = np.zeros(Pcol.shape, dtype=Prow_s.dtype)
    csum = np.zeros((M, o), dtype=dtype); csum_s = np.zeros((M, o), dtype=Prow_s.dtype)
    for i, (s, jb, je) in enumerate(items):
        for j in range(jb, je):                                    # the steps of an item in order, the items of a strip in order
            v = col[(int(s), j)]
            Pcol[i, :v.shape[0]] += v; Pcol_s[i, :v.shape[0]] += cols[(int(s), j)]
        c0, c1 = s * STRIP, min(s * STRIP + STRIP, M)
        csum[c0:c1] += Pcol[i, :c1 - c0]; csum_s[c0:c1] += Pcol_s[i, :c1 - c0]
    return dict(Prow=Prow, Prow_scale=Prow_s, written=written, Pcol=Pcol, Pcol_scale=Pcol_s, csum=csum, csum_scale=csum_s)


def rank_y(st, g, cs_all, cs_scale, cam0, nloc, alpha, dtype=np.float64):
    """symw_reduce_kernel with the plain epilogue for the cameras of one rank: per camera the row sums of the strips its step touches (strip
    order), then the ranks' vectors (rank order), times alpha.  cs_all: world x M x o as gathered; cs_scale: their scales.  -> (Y, scale)"""
    o = st["csum"].shape[1]
    acc = np.zeros((3 * nloc, o), dtype=dtype); sc = np.zeros((3 * nloc, o), dtype=st["Prow_scale"].dtype)
    for s in range(g["nstrips"]):
        for j in range(g["nsteps"]):
            if any_pair(g, g["t0"] + j, s):
                acc[6 * j:6 * j + 6] += st["Prow"][s, 6 * j:6 * j + 6]; sc[6 * j:6 * j + 6] += st["Prow_scale"][s, 6 * j:6 * j + 6]
    rows = slice(3 * cam0, 3 * (cam0 + nloc))
    for r2 in range(cs_all.shape[0]):
        acc += np.asarray(cs_all[r2][rows]).astype(dtype); sc += np.asarray(cs_scale[r2][rows]).astype(sc.dtype)
    return (acc * alpha if dtype == np.int64 else dtype(alpha) * acc), abs(alpha) * sc


def whole_model(Q, W, world, plans, use, alpha=1.0, dtype=np.float64):
    """every rank of the partition: sweep, column sums, the all-gather (a copy) and the per-camera sum.  plans: xm_symw_plan's output per rank.
    -> (Y of the whole matrix, scale of Y, per-rank stage dicts with Y and Y_scale added)"""
    M, o = W.shape
    ntot = M // 3
    nloc = ntot // world
    stages = []
    for r, p in enumerate(plans):
        g = {k: p[k] for k in ("T", "Th", "tie", "t0", "nsteps", "nstrips")}
        pairs = rank_pairs(Q[3 * r * nloc:3 * (r + 1) * nloc], W, g, use, dtype)
        st = rank_stages(pairs, g, p["items"], o, M, dtype)
        st["g"] = g
        stages.append(st)
    cs_all = np.stack([st["csum"] for st in stages]); cs_scale = np.stack([st["csum_scale"] for st in stages])
    for r, st in enumerate(stages):
        st["Y"], st["Y_scale"] = rank_y(st, st["g"], cs_all, cs_scale, r * nloc, nloc, alpha, dtype)
    return np.concatenate([st["Y"] for st in stages]), np.concatenate([st["Y_scale"] for st in stages]), stages


# ---- data --------------------------------------------------------------------------------------------------------------------------------
def int_operands(ntot, o, seed=0):
    """symmetric integer Q in [-8, 8], integer W in [-4, 4]: |sum| <= 32 * 3 ntot, far below 2^53 even times 2.5 -- exact in any order"""
    rng = np.random.default_rng(1000 * ntot + o + seed)
    M = 3 * ntot
    A = rng.integers(-8, 9, (M, M))
    Q = np.triu(A) + np.triu(A, 1).T
    return Q.astype(np.float64), rng.integers(-4, 5, (M, o)).astype(np.float64)


def real_operands(family, ntot, o, seed=0):
    rng = np.random.default_rng(2000 * ntot + o + seed)
    M = 3 * ntot
    if family == "random":
        A = rng.standard_normal((M, M))
        Q = A + A.T
    elif family == "laplacian":                                    # edge weights over ten decades (tests/xm_la_stages.py)
        Q = la.laplacian(M, seed)
        Q = np.triu(Q) + np.triu(Q, 1).T
    else:
        raise ValueError(family)
    assert np.array_equal(Q, Q.T)
    return Q, rng.standard_normal((M, o))


FAMILIES = ("random", "laplacian")


def noise_unused_mirror_blocks(Qr, g, use, seed=0):
    """a copy of a rank's strip with the block of every mirror pair that its row step does NOT use overwritten by finite noise (the
    diagonal block and the used blocks stay): a kernel that masks gives the same outputs, one that relies on symmetry does not"""
    rng = np.random.default_rng(seed)
    out = np.array(Qr, dtype=np.float64)
    for j in range(g["nsteps"]):
        t = g["t0"] + j
        for u in range(g["T"]):
            if u != t and not use[t, u]:
                out[6 * j:6 * j + 6, 6 * u:6 * u + 6] = rng.uniform(-1e3, 1e3, (6, 6))
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------------------------
def same_values(a, b):
    """equal entry by entry, a NaN only where the other has one (the sign of a zero is not compared: x * 0 of a masked entry carries x's)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def scaled_error(x, truth, scale, where=None):
    """max over the entries of |x - truth| / scale; an entry whose scale is 0 has no addend but zeros and must be 0 (else inf)"""
    x = np.asarray(x).astype(np.longdouble); truth = np.asarray(truth).astype(np.longdouble); scale = np.asarray(scale).astype(np.longdouble)
    if where is not None:
        x, truth, scale = x[where], truth[where], scale[where]
    if x.size == 0:
        return 0.0
    d = np.abs(x - truth)
    if not np.isfinite(d).all():
        return float("inf")
    zero = scale == 0
    if np.any(d[zero] != 0):
        return float("inf")
    return float(np.max(d[~zero] / scale[~zero])) if np.any(~zero) else 0.0


def check_stage(label, quantity, e_ref, e_gpu):
    b = bound(e_ref)
    print(f"STAGE_ERR {label} {quantity}: e_ref {e_ref:.3e}, e_gpu {e_gpu:.3e}, ratio {e_gpu / b:.3f}")
    return e_gpu <= b
