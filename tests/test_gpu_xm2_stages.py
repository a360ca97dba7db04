"""The kernels that rewrite the resident Q or decide what leaves it, stage by stage against the references of tests/xm_xm2_exact.py:
edge_locate / diag_locate, edge_write / diag_write and the sliced-ELL refill (Context.set_edge_weights), edge_residual
(Context.edge_residuals_recovered), xm2_error / radix_hist / xm2_filter (Context.xm2_filter).

Q is read back through the context's own product on identity columns (Context.qw), which is exact for a finite Q: the rewrite is compared
BIT FOR BIT with a reference that is exact by construction.  Where the stored block passes through the quaternion codec, and for the
residuals, the bound is max(16 e_ref, 64 eps) with e_ref the error of the f64 host statement against longdouble; every such comparison
prints `STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s; profiles/r34_xm2_stage_errors.txt holds one run).  No tolerance is
derived from the GPU's output.

The tuning fields count from one where the kernels count from zero: sell_gather 1 | 2 are the kernels' gather modes 0 | 1 (a record per
lane | LDS-transposed), sell_codec 2 is the quaternion codec."""
import numpy as np
import pytest

import xm_xm2_exact as xx

pytestmark = pytest.mark.gpu
LD = np.longdouble
ERR_ARG = r"error -2:"


def read_q(ctx, o):
    """Q through the context's product of rank o on identity columns, o at a time"""
    m = 3 * ctx.n
    Q = np.zeros((m, m))
    for c in range(0, m, o):
        k = min(o, m - c)
        W = np.zeros((m, o))
        W[np.arange(c, c + k), np.arange(k)] = 1.0
        Q[:, c:c + k] = ctx.qw(W)[:, :k]
    return Q


def read_probe(ctx, W, o):
    """Q W through the context's product of rank o, o columns of W at a time (xx.probe_columns: exact, every entry of Q once)"""
    P = np.zeros_like(W)
    for c in range(0, W.shape[1], o):
        k = min(o, W.shape[1] - c)
        B = np.zeros((W.shape[0], o))
        B[:, :k] = W[:, c:c + k]
        P[:, c:c + k] = ctx.qw(B)[:, :k]
    return P


def stage_err(case, what, e_ref, e_gpu):
    b = xx.bound(e_ref)
    print(f"STAGE_ERR {case} {what}: e_ref {e_ref:.3e}, e_gpu {e_gpu:.3e}, ratio {e_gpu / b:.3f}")
    return e_gpu <= b


SELL = {f"sell_g{g}_s{s}": dict(sell=1, sell_codec=1, sell_gather=g, sell_lmax=5, sell_slabs=s) for g in (1, 2) for s in (2, 8)}
FORMS = ("dense", "dense_sym", "bsr", "bsr_shuffled", "densify") + tuple(SELL)


def make_context(xmamd, g, form, w):
    """(context, reads = ((o, product kind), ...), extra: the created Q holds g["extra"])"""
    if form in ("dense", "dense_sym"):
        tn = dict(sym=-1) if form == "dense" else dict(sym=1, sym_min_rows=1)
        ctx = xmamd.Context(Q=xx.rewrite_reference(g, w), tuning=tn)
        reads = ((10, "dense"),) if form == "dense" else ((5, "dense_sym"), (3, "dense_sym"), (10, "dense"))
        extra = True
    else:
        bsr = xx.bsr_of(g, w, shuffle=np.random.default_rng(11) if form == "bsr_shuffled" else None)
        ctx = xmamd.Context(bsr=bsr, densify=(form == "densify"), tuning=SELL.get(form))
        reads = ((10, "dense"),) if form == "densify" else ((10, "bsr3"),) if form in ("bsr", "bsr_shuffled") else ((5, "sell"), (10, "bsr3"))
        extra = False
    ctx.attach_edges(g["ei"], g["ej"], g["M"])
    return ctx, reads, extra


# ------------------------------------------------------------------------------------------------ 1. the rewrite, bit for bit
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", xx.GRAPHS)
def test_rewrite_is_exact(xmamd, name, form):
    """every weight sequence in order on one context.  After each one the whole of Q is read on plain identity columns through the form's
    first product kind: equal to the exact rewrite in every entry, the lower triangle and the untouched entries included (a camera without a
    stored diagonal block stays empty, a block that is no edge survives), and Q == Q^T.  Through every product kind the form has, Q W for the
    packed identity columns of xx.probe_columns -- every stored entry once, a zero wherever nothing is stored -- equals the reference's bit
    for bit; the same call twice gives the same bytes, and w0 applied again at the end the bytes of the first time.  One sequence holds a
    negative weight: the rewrite is linear on these storages."""
    g = xx.graph(name)
    ones = np.ones(g["ei"].size)
    ctx, reads, extra = make_context(xmamd, g, form, ones)
    W = xx.probe_columns(g)
    try:
        first = {}
        for o, kind in reads:
            assert ctx.product_kind(o) == kind
            assert np.array_equal(read_probe(ctx, W, o), xx.rewrite_reference(g, ones, extra=extra) @ W), ("created", o)
        for wname, w in xx.weight_sequences(g):
            ref = xx.rewrite_reference(g, w, extra=extra)
            assert np.array_equal(ref, ref.T)
            ctx.set_edge_weights(w)
            for o, kind in reads:
                assert ctx.product_kind(o) == kind
                P = read_probe(ctx, W, o)
                bad = np.argwhere(P != ref @ W)
                assert bad.size == 0, (wname, o, bad[:5].tolist())
                if wname == "w0":
                    first[o] = P.tobytes()
                    ctx.set_edge_weights(w)
                    assert read_probe(ctx, W, o).tobytes() == first[o]
                if wname == "w5":
                    assert P.tobytes() == first[o]
            Q = read_q(ctx, reads[0][0])
            assert np.array_equal(Q, ref) and np.array_equal(Q, Q.T), wname
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the quaternion codec
def codec_context(xmamd, g, form, w):
    if form == "vg":
        return xmamd.Context(vg=(g["ei"], g["ej"], w, g["M"]), n=g["n"], tuning=dict(sell=1))
    ctx = xmamd.Context(bsr=xx.bsr_of(g, w, nodiag=False), tuning=dict(sell=1, sell_codec=2, sell_lmax=5))
    ctx.attach_edges(g["ei"], g["ej"], g["M"])
    return ctx


def check_codec_q(xmamd, g, w, Q, case):
    """diagonals bit-equal, zero weights exactly zero blocks, nothing outside the pattern; every other block within the bound of its own
    host round trip, relative to w_e"""
    n = g["n"]
    d = xx.diag_sums(g, w)
    rest = Q.copy()
    worst = (0.0, 0.0, 0.0)
    ok = True
    for c in range(n):
        assert np.array_equal(Q[3 * c:3 * c + 3, 3 * c:3 * c + 3], d[c] * np.eye(3)), (case, "diagonal", c)
        rest[3 * c:3 * c + 3, 3 * c:3 * c + 3] = 0.0
    for e in range(g["ei"].size):
        i, j = int(g["ei"][e]), int(g["ej"][e])
        Bij, Bji = Q[3 * i:3 * i + 3, 3 * j:3 * j + 3], Q[3 * j:3 * j + 3, 3 * i:3 * i + 3]
        rest[3 * i:3 * i + 3, 3 * j:3 * j + 3] = 0.0; rest[3 * j:3 * j + 3, 3 * i:3 * i + 3] = 0.0
        if w[e] == 0.0:
            assert not Bij.any() and not Bji.any(), (case, "removed edge", e)
            continue
        B = (-w[e]) * g["M"][e]
        _, r = xmamd.quat_roundtrip(B)
        _, rt = xmamd.quat_roundtrip(B.T)
        e_ref = float(max(np.abs(r.astype(LD) - B).max(), np.abs(rt.astype(LD) - B.T).max()) / LD(w[e]))
        e_gpu = float(max(np.abs(Bij.astype(LD) - B).max(), np.abs(Bji.astype(LD) - B.T).max()) / LD(w[e]))
        ok = ok and e_gpu <= xx.bound(e_ref)
        if e_gpu / xx.bound(e_ref) >= worst[2]:
            worst = (e_ref, e_gpu, e_gpu / xx.bound(e_ref))
    assert not rest.any(), (case, "entries outside the pattern")
    print(f"STAGE_ERR {case} codec_block: e_ref {worst[0]:.3e}, e_gpu {worst[1]:.3e}, ratio {worst[2]:.3f}")
    return ok


# the view-graph storage is given without the cameras that have no edge: its list describes a connected graph
CODEC_CASES = [(k, f) for k in xx.GRAPHS if k not in ("path255", "path256") for f in ("vg", "bsr_codec") if (k, f) != ("isolated", "vg")]


@pytest.mark.parametrize("name,form", CODEC_CASES)
def test_rewrite_through_the_quaternion_codec(xmamd, name, form):
    """XM_STORAGE_VIEWGRAPH and BSR3 with sell_codec = 2: the stored off-diagonal blocks pass through block_to_quat / quat_to_block, so
    bits are not promised for them.  Weights between 2^-300 and 2^300 (the codec squares the block's entries)."""
    g = xx.graph(name)
    seq = xx.weight_sequences(g, codec=True)
    ctx = codec_context(xmamd, g, form, seq[0][1])
    W, colour = xx.probe_columns(g, colours=True)
    read = lambda o: xx.probe_decode(g, read_probe(ctx, W, o), colour)      # every stored entry, and nothing else in the product
    try:
        assert ctx.product_kind(3) == ctx.product_kind(5) == "sell_quat"
        miss = [] if check_codec_q(xmamd, g, seq[0][1], read(3), f"{form}-{name}-created") else ["created"]
        for wname, w in seq:
            ctx.set_edge_weights(w)
            for o in ((3, 5) if wname in ("w0", "w4") else (3,)):
                if not check_codec_q(xmamd, g, w, read(o), f"{form}-{name}-{wname}-o{o}"):
                    miss.append((wname, o))
        assert not miss, miss
        # a negative or NaN weight is refused here, with Q and the weights as they were
        before = read_probe(ctx, W, 3)
        for v in (-1.0, np.nan, -np.inf):
            wb = seq[-1][1].copy(); wb[wb.size // 2] = v
            with pytest.raises(xmamd.XmError, match=ERR_ARG):
                ctx.set_edge_weights(wb)
            assert read_probe(ctx, W, 3).tobytes() == before.tobytes()
        wz = seq[-1][1].copy(); wz[0] = -0.0                      # -0.0 is 0: legal, an exactly zero block
        ctx.set_edge_weights(wz)
        assert check_codec_q(xmamd, g, wz, read(3), f"{form}-{name}-negzero")
        Q = read_q(ctx, 5)                                         # and once on plain identity columns
        assert check_codec_q(xmamd, g, wz, Q, f"{form}-{name}-negzero-identity") and np.array_equal(Q, read(5))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 3. residuals
@pytest.mark.parametrize("form", ["bsr", "dense", "vg"])
@pytest.mark.parametrize("name", ["pair", "cycle257", "reversed"])
def test_residuals_of_a_recovered_solution(xmamd, name, form):
    """|s_i R_i - M_e s_j R_j|_F^2 per edge (R_i: the transpose of the anchored block) against longdouble, relative to
    |Y_i|_F^2 + |M_e Y_j|_F^2: Haar rotations with scales in [0.5, 2], the exact solution of noise-free measurements (round-off through
    cancellation), scales of 1e-150 and of 1e150"""
    g = xx.graph(name)
    miss = []
    for pname, M, rot, scale in xx.residual_points(g):
        gp = dict(g, M=np.ascontiguousarray(M))
        w = np.ones(g["ei"].size)
        if form == "vg":
            ctx = xmamd.Context(vg=(g["ei"], g["ej"], w, M), n=g["n"], tuning=dict(sell=1))
        else:
            ctx = xmamd.Context(Q=xx.rewrite_reference(gp, w)) if form == "dense" else xmamd.Context(bsr=xx.bsr_of(gp, w))
            ctx.attach_edges(g["ei"], g["ej"], M)
        try:
            res = ctx.edge_residuals_recovered(rot, scale)
            again = ctx.edge_residuals_recovered(rot, scale)
        finally:
            ctx.close()
        ref, mag = xx.residual_reference(gp, M, rot, scale)
        r64, _ = xx.residual_reference(gp, M, rot, scale, dtype=np.float64)
        assert np.all(np.isfinite(res)) and np.all(res >= 0) and res.tobytes() == again.tobytes()
        if not stage_err(f"{form}-{name}-{pname}", "edge_residual", xx.rel_err(r64, ref, mag), xx.rel_err(res, ref, mag)):
            miss.append(pname)
    assert not miss, miss


# ------------------------------------------------------------------------------------------------ 4. the filter
def filter_graph(d, ne):
    n, ei, ej = xx.complete_graph(ne)
    return dict(n=n, ei=ei, ej=ej, M=xx.design_M(d), nodiag=(), extra=None)


def filter_context(xmamd, g, dense):
    w = np.ones(g["ei"].size)
    ctx = xmamd.Context(Q=xx.rewrite_reference(g, w)) if dense else xmamd.Context(bsr=xx.bsr_of(g, w))
    ctx.attach_edges(g["ei"], g["ej"], g["M"])
    return ctx


def identity_point(n):
    return np.tile(np.eye(3), n), np.ones(n)


def check_filter(xmamd, ctx, g, w, err, pct, case, read=True):
    """one xm2_filter call on the context's current weights w (errors err) against the exact-position reference -> the new weights"""
    live = w != 0.0
    ref = xx.filter_reference(err, live, pct)
    near = live & (np.abs(err.astype(LD) - ref["thr"]) <= xx.thr_bound(ref))
    assert np.all(err[near].astype(LD) == ref["thr"]), (case, pct, "the case does not decide the removed set")
    thr, removed, w_out = ctx.xm2_filter(*identity_point(g["n"]), pct)
    print(f"XM2_FILTER {case} pct {pct:g}: position {ref['k0']} + {ref['frac']}, threshold {thr!r} (exact {float(ref['thr'])!r}), removed {removed}")
    assert abs(LD(thr) - ref["thr"]) <= xx.thr_bound(ref), (case, pct)
    if ref["integral"] or ref["x0"] == ref["x1"]:
        assert thr == ref["x0"], (case, pct)
    assert np.array_equal(np.flatnonzero(live & (w_out == 0.0)), np.flatnonzero(ref["removed"])), (case, pct)
    assert removed == int(ref["removed"].sum())
    assert np.array_equal(w_out, np.where(ref["removed"] | ~live, 0.0, w)) and not np.signbit(w_out[w_out == 0.0]).any()
    assert np.all(w_out[live & (err == thr)] != 0.0)                       # an error equal to the threshold stays
    if pct == 90.0:
        assert np.array_equal(ref["removed"], live & (err > np.percentile(err[live], 90.0)))
    if read:
        assert np.array_equal(read_q(ctx, 10), xx.rewrite_reference(g, w_out)), (case, pct, "Q after the filter")
    return w_out


@pytest.mark.parametrize("name", xx.DESIGNS)
def test_filter_threshold_and_removed_set(xmamd, name):
    """rotations at the identity, scales 1, M_e the half turn diag(1, -1, -1) or I: res_e is exactly 8 or 0, so err_e = 8 w_e is set bit
    by bit through the weights.  Threshold within 4 eps max(x0, x1) of the exact-position one and bit-equal to the order statistic where
    the position is integral or the neighbours are equal; removed indices, count and new weights those of the reference; Q afterwards the
    exact rewrite for the new weights."""
    for ne in xx.NE:
        d = xx.design(name, ne)
        g = filter_graph(d, ne)
        err, _ = xx.design_errors(d)
        ctx = filter_context(xmamd, g, dense=ne in (1, 3, 101, 257))
        try:
            ctx.set_edge_weights(d["w"])
            res = ctx.edge_residuals_recovered(*identity_point(g["n"]))
            assert np.array_equal(res, np.where(d["half"], 8.0, 0.0))
            for pct in d["pcts"]:
                ctx.set_edge_weights(d["w"])
                check_filter(xmamd, ctx, g, d["w"], err, pct, f"{name}-ne{ne}")
        finally:
            ctx.close()


@pytest.mark.parametrize("name", ["uniform", "livezero", "ties"])
def test_second_filter_on_the_same_context(xmamd, name):
    """the removed edges keep their place with weight 0 (nz > 0): the order statistics of the next call are those of the survivors"""
    for ne in (11, 101, 257, 1000):
        d = xx.design(name, ne)
        g = filter_graph(d, ne)
        ctx = filter_context(xmamd, g, dense=ne in (101, 1000))
        try:
            w = d["w"]
            ctx.set_edge_weights(w)
            for pct in (90.0, 50.0, 70.0, 100.0, 0.0):
                w = check_filter(xmamd, ctx, g, w, np.where(d["half"] & (w != 0.0), 8.0 * w, 0.0), pct, f"second-{name}-ne{ne}")
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------------------ 5. zero, negative and NaN weights
@pytest.mark.parametrize("name", ["ties", "uniform"])
def test_a_weight_of_minus_zero_is_a_weight_of_zero(xmamd, name):
    """removed edges given as -0.0: error -0.0 sorted BEHIND every positive double in the select, the threshold came out as -0.0 and
    every live edge was removed.  Same threshold, count, weights (+0.0 for everything removed) and Q as with +0.0."""
    for ne in (11, 257, 1000):
        d = xx.design(name, ne)
        g = filter_graph(d, ne)
        gone = np.random.default_rng(ne).uniform(size=ne) < 0.1
        gone[1] = True; gone[0] = False
        err = np.where(gone, 0.0, 8.0 * d["w"])
        out = []
        for zero in (0.0, -0.0):
            w = np.where(gone, zero, d["w"])
            assert np.signbit(w[gone]).all() == bool(np.signbit(zero))
            ctx = filter_context(xmamd, g, dense=ne == 257)
            try:
                ctx.set_edge_weights(w)
                assert np.array_equal(read_q(ctx, 10), xx.rewrite_reference(g, np.where(gone, 0.0, d["w"])))
                for pct in (90.0, 50.0):
                    ctx.set_edge_weights(w)
                    wo = check_filter(xmamd, ctx, g, w, err, pct, f"negzero-{name}-ne{ne}")
                    out.append((pct, wo.tobytes()))
            finally:
                ctx.close()
        assert out[0] == out[2] and out[1] == out[3]


def test_filter_refusals_leave_q_alone(xmamd):
    """XM_ERR_ARG with Q unchanged: a percentile outside [0, 100] or NaN, every edge removed already, a negative or NaN weight, a dense or
    BSR3 context before set_edge_weights; the context goes on working"""
    d = xx.design("uniform", 101)
    g = filter_graph(d, 101)
    err, _ = xx.design_errors(d)
    pt = identity_point(g["n"])
    for dense in (True, False):
        ctx = filter_context(xmamd, g, dense)
        try:
            q0 = read_q(ctx, 10).tobytes()
            with pytest.raises(xmamd.XmError, match=ERR_ARG):      # the context was created from Q: it does not know its weights yet
                ctx.xm2_filter(*pt, 90.0)
            assert read_q(ctx, 10).tobytes() == q0
            ctx.set_edge_weights(d["w"])
            q1 = read_q(ctx, 10).tobytes()
            for pct in (-1e-300, -1.0, 100.0000001, np.nan, np.inf):
                with pytest.raises(xmamd.XmError, match=ERR_ARG):
                    ctx.xm2_filter(*pt, pct)
                assert read_q(ctx, 10).tobytes() == q1
            for v in (-1.0, np.nan, -2.0 ** -1074):
                wb = d["w"].copy(); wb[50] = v
                ctx.set_edge_weights(wb)                            # legal on these storages: the rewrite is linear
                qb = read_q(ctx, 10)
                if v == v:
                    assert np.array_equal(qb, xx.rewrite_reference(g, wb))
                with pytest.raises(xmamd.XmError, match=ERR_ARG):
                    ctx.xm2_filter(*pt, 90.0)
                if v == v:                                          # (a product with a NaN in Q is no read-back)
                    assert read_q(ctx, 10).tobytes() == qb.tobytes()
            ctx.set_edge_weights(np.zeros(101))
            qz = read_q(ctx, 10)
            assert not qz.any()
            with pytest.raises(xmamd.XmError, match=ERR_ARG):
                ctx.xm2_filter(*pt, 90.0)
            assert read_q(ctx, 10).tobytes() == qz.tobytes()
            ctx.set_edge_weights(d["w"])
            check_filter(xmamd, ctx, g, d["w"], err, 90.0, f"after-refusals-{'dense' if dense else 'bsr'}")
        finally:
            ctx.close()


def test_attach_edges_refusals(xmamd):
    """XM_ERR_ARG: a pair listed twice as (i, j) or as (j, i), i == j, an index out of range, an edge without its stored blocks, a camera
    with edges but without a stored diagonal block; the context stays usable"""
    g = xx.graph("er86")
    ne = g["ei"].size
    w = xx.weight_sequences(g)[0][1]
    ref = xx.rewrite_reference(g, w)

    def lists(ei, ej):
        return np.asarray(ei, dtype=np.int32), np.asarray(ej, dtype=np.int32), np.ascontiguousarray(np.broadcast_to(np.eye(3), (len(ei), 3, 3)))
    bad = [lists(np.r_[g["ei"], g["ei"][3]], np.r_[g["ej"], g["ej"][3]]), lists(np.r_[g["ei"], g["ej"][3]], np.r_[g["ej"], g["ei"][3]]),
           lists([0, 5], [1, 5]), lists([0, 1], [1, 86]), lists([0, -1], [1, 2])]
    for dense in (True, False):
        ctx = xmamd.Context(Q=xx.rewrite_reference(g, np.ones(ne))) if dense else xmamd.Context(bsr=xx.bsr_of(g, np.ones(ne)))
        try:
            for ei, ej, M in bad:
                with pytest.raises(xmamd.XmError, match=ERR_ARG):
                    ctx.attach_edges(ei, ej, M)
            if not dense:
                absent = next((i, j) for i in range(86) for j in range(i + 1, 86) if not (((g["ei"] == i) & (g["ej"] == j)) | ((g["ei"] == j) & (g["ej"] == i))).any())
                with pytest.raises(xmamd.XmError, match=ERR_ARG):
                    ctx.attach_edges(*lists([absent[0]], [absent[1]]))
            ctx.attach_edges(g["ei"], g["ej"], g["M"])
            ctx.set_edge_weights(w)
            assert np.array_equal(read_q(ctx, 10), ref)
        finally:
            ctx.close()
    # a camera that has edges needs its diagonal block; one that has none does not
    g2 = dict(g, nodiag=(int(g["ei"][0]),))
    ctx = xmamd.Context(bsr=xx.bsr_of(g2, np.ones(ne)))
    try:
        with pytest.raises(xmamd.XmError, match=ERR_ARG):
            ctx.attach_edges(g["ei"], g["ej"], g["M"])
        keep = (g["ei"] != g["ei"][0]) & (g["ej"] != g["ei"][0])
        gk = dict(g, ei=g["ei"][keep], ej=g["ej"][keep], M=np.ascontiguousarray(g["M"][keep]))
        ctx.attach_edges(gk["ei"], gk["ej"], gk["M"])
        wk = w[keep]
        ctx.set_edge_weights(wk)
        exp = xx.rewrite_reference(g2, np.ones(ne))
        new = xx.rewrite_reference(gk, wk)
        c = 3 * int(g["ei"][0])
        exp_rows = np.ones(3 * 86, dtype=bool); exp_rows[c:c + 3] = False
        sel = np.outer(exp_rows, exp_rows)
        exp[sel] = new[sel]                                         # that camera's row and column keep what they were created with
        exp[c:c + 3, c:c + 3] = 0.0                                 # and it has no diagonal block
        assert np.array_equal(read_q(ctx, 10), exp)
    finally:
        ctx.close()
