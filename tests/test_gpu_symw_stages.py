"""The multi-rank symmetric window product of xm_symw.hip kernel by kernel through the test export xm_symw_probe: qw_symw_kernel's row sums per
(strip, step) and column sums per item, symw_colsum_kernel's vector and symw_reduce_kernel's per-camera sum, every rank of every partition
of tests/xm_symw_stages.py's case list, against that module's model.  Integer-valued data must come back bit for bit (every sum is exact
in any order: a dropped, doubled or misplaced block cannot hide); real-valued data within max(16 e_ref, 64 eps) of the longdouble model,
per entry over the entry's sum of |q| |w|; what the sweep does not write keeps the sentinel and is never read."""
import numpy as np
import pytest

import xm_symw_stages as st

CASE_IDS = st.case_ids()


def plans_of(xmamd, ntot, world, K=0):
    nloc = ntot // world
    return [xmamd.symw_plan(ntot, nloc, r * nloc, K) for r in range(world)]


# ---- CPU: the case list reaches what it is meant to reach --------------------------------------------------------------------------------
def test_case_list_reaches_every_path(xmamd):
    """from xm_symw_plan and the predicates alone (no GPU): item lengths 1 .. 5 of both parities, the unmasked and the masked path in one
    case, half1 true and false, a diagonal block cut by a strip boundary, a last strip with padding columns, the reducer's second trip"""
    for T in sorted({ntot // 2 for ntot, _ in st.CASES}):          # the restated window predicate is the library's
        assert np.array_equal(st.use_matrix(T), np.array([[xmamd.lib().xm_symw_use(T, t, u) for u in range(T)] for t in range(T)], dtype=bool))
    lengths, mixed, half1, cut, padded, lanes, ties, odd_T, wraps = set(), [], set(), [], [], [], [], [], []
    for ntot, worlds in st.CASES:
        ld, M = st.dense_ld(ntot), 3 * ntot
        assert ld % 128 == 0 and M <= ld < M + 128
        for world in worlds:
            assert ntot % world == 0 and (ntot // world) % 2 == 0
            for K in (st.KS if ntot in st.LARGE else (0,)):
                full = masked = 0
                for p in plans_of(xmamd, ntot, world, K):
                    seen = set()
                    for s, jb, je in p["items"]:
                        lengths.add(int(je - jb))
                        assert je - jb <= p["K"]
                        for j in range(jb, je):
                            seen.add((int(s), j))
                            f = st.full_pair(p, p["t0"] + j, int(s))
                            full += f; masked += not f
                    assert seen == {(s, j) for s in range(p["nstrips"]) for j in range(p["nsteps"]) if st.any_pair(p, p["t0"] + j, s)}
                    for s in range(p["nstrips"]):
                        half1.add(s * 256 + 128 < ld)
                    lanes.append(p["nstrips"] + world)
                    if p["tie"]:
                        ties.append(ntot)
                    else:
                        odd_T.append(ntot)
                    # the window of a row step wraps over the matrix end
                    wraps += [ntot for j in range(p["nsteps"]) if p["t0"] + j + p["Th"] - 1 >= p["T"] > 1]
                if full and masked:
                    mixed.append((ntot, world, K))
        T = ntot // 2
        cut += [ntot for t in range(T) if (6 * t) // 256 != (6 * t + 5) // 256]
        if M % 256 and (M // 256) * 256 + 256 <= ld:
            padded.append(ntot)                                    # real and padding columns in a strip that lies whole inside ld
    assert {1, 2, 3, 4, 5} <= lengths
    assert any(c[0] == 344 for c in mixed)
    assert half1 == {True, False}
    assert 86 in cut and 84 not in cut
    assert {84, 130} <= set(padded)
    assert max(lanes) == 72 and min(lanes) < 64
    assert 4 in ties and 258 in odd_T and 344 in wraps
    # the table's own figures
    assert [st.dense_ld(n) for n in (84, 86, 128, 130, 256, 258, 344)] == [256, 384, 384, 512, 768, 896, 1152]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(xmamd):
    xmamd.require_gpu()
    return xmamd


_models = {}


def int_model(gpu, ntot, world, o, K):
    """(Q, W, Y, stages, plans) of the int64 model at alpha = 1, computed once, shared among the tests and left unchanged.  (Every value is an
    integer far below 2^50, so alpha = -2.5 times it is exact in float64 too.)"""
    key = (ntot, world, o, K)
    if key not in _models:
        Q, W = st.int_operands(ntot, o)
        plans = plans_of(gpu, ntot, world, K)
        y, _, stages = st.whole_model(Q, W, world, plans, st.use_matrix(ntot // 2), 1, np.int64)
        _models[key] = (Q, W, y, stages, plans)
    return _models[key]


def combos(ntot):
    """(o, K, alpha, nt) of a case: every o with every K of the case; both alphas at the automatic K and alternating elsewhere; both load
    policies where the case asks for them (alternating with K, and both at the automatic K)"""
    out = []
    for io, o in enumerate(st.OS):
        for ik, K in enumerate(st.KS if ntot in st.LARGE else (0,)):
            nts = ((0, 1) if K == 0 else ((io + ik) % 2,)) if ntot == st.NT_NTOT else (-1,)
            alphas = st.ALPHAS if K == 0 else (st.ALPHAS[(io + ik) % 2],)
            out += [(o, K, a, nt) for a in alphas for nt in nts]
    return out


def check_rank_int(what, got, want, p, alpha):
    """one rank's stages against the int64 model (want: the model at alpha = 1)"""
    w = want["written"]
    assert got["nitems"] == p["nitems"] and got["K"] == p["K"], what
    assert np.isfinite(got["Prow"][w]).all() and np.isnan(got["Prow"][~w]).all(), what          # written exactly where the plan says
    assert st.same_values(got["Prow"][w], want["Prow"][w]), what
    assert st.same_values(got["Pcol"], want["Pcol"]), what
    assert st.same_values(got["csum"], want["csum"]), what
    assert np.isfinite(got["Y"]).all() and st.same_values(got["Y"], alpha * want["Y"].astype(np.float64)), what


@pytest.mark.gpu
@pytest.mark.parametrize("ntot,world", CASE_IDS)
def test_integer_data_bit_for_bit(gpu, ntot, world):
    """Q symmetric with integer entries in [-8, 8], W integer in [-4, 4]: Prow, Pcol, csum and Y of every rank equal the int64 model, and
    Y over the ranks equals alpha * Q @ W (alpha = -2.5 is exact here)"""
    for o, K, alpha, nt in combos(ntot):
        what = f"ntot {ntot} world {world} o {o} K {K} alpha {alpha} nt {nt}"
        Q, W, y, stages, plans = int_model(gpu, ntot, world, o, K)
        Y, got = gpu.symw_product(Q, W, world, o, alpha=alpha, K=K, nt=nt)
        assert st.same_values(y, Q @ W) and st.same_values(Y, alpha * (Q @ W)), what
        for r in range(world):
            check_rank_int(f"{what} rank {r}", got[r], stages[r], plans[r], alpha)
            assert got[r]["nt"] == (nt if nt >= 0 else 0), what                                    # (a test-sized strip is far below the non-temporal threshold)
            assert got[r]["nfull"] == sum(st.full_pair(plans[r], plans[r]["t0"] + j, int(s)) for s, jb, je in plans[r]["items"] for j in range(jb, je)), what


@pytest.mark.gpu
@pytest.mark.parametrize("family", st.FAMILIES)
@pytest.mark.parametrize("ntot,world", CASE_IDS)
def test_real_data_within_the_stage_bound(gpu, ntot, world, family):
    """random symmetric Q and a graph Laplacian with weights over ten decades: per entry, the error against the longdouble model over the
    entry's sum of |q| |w| stays below max(16 e_ref, 64 eps), e_ref the float64 model's error measured the same way"""
    use = st.use_matrix(ntot // 2)
    bad = []
    for io, o in enumerate(st.OS):
        K = (0, 3, 5, 2)[io] if ntot in st.LARGE else 0
        alpha = st.ALPHAS[io % 2]
        Q, W = st.real_operands(family, ntot, o)
        plans = plans_of(gpu, ntot, world, K)
        _, _, truth = st.whole_model(Q, W, world, plans, use, alpha, np.longdouble)
        _, _, ref = st.whole_model(Q, W, world, plans, use, alpha, np.float64)
        _, got = gpu.symw_product(Q, W, world, o, alpha=alpha, K=K, nt=(io % 2 if ntot == st.NT_NTOT else -1))
        for q in ("Prow", "Pcol", "csum", "Y"):
            e_ref = e_gpu = 0.0
            for r in range(world):
                where = truth[r]["written"] if q == "Prow" else None
                e_ref = max(e_ref, st.scaled_error(ref[r][q], truth[r][q], truth[r][q + "_scale"], where))
                e_gpu = max(e_gpu, st.scaled_error(got[r][q], truth[r][q], truth[r][q + "_scale"], where))
            if not st.check_stage(f"{family}-n{ntot}-w{world}-o{o}-K{K}", q, e_ref, e_gpu):
                bad.append((o, q, e_ref, e_gpu))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("ntot,world", CASE_IDS)
def test_unwritten_records_keep_the_sentinel_and_are_never_read(gpu, ntot, world):
    """records of (strip, step) pairs with symw_any are finite, all others still hold the sentinel, and Y is finite all the same"""
    o = st.OS[(ntot // 2 + world) % 4]
    Q, W = st.real_operands("random", ntot, o, seed=1)
    _, got = gpu.symw_product(Q, W, world, o)
    nloc = ntot // world
    for r, g in enumerate(got):
        p = gpu.symw_plan(ntot, nloc, r * nloc)
        anyp = np.array([[st.any_pair(p, p["t0"] + j, s) for j in range(p["nsteps"]) for _ in range(6)] for s in range(p["nstrips"])])
        assert np.isfinite(g["Prow"][anyp]).all() and np.isnan(g["Prow"][~anyp]).all()
        assert np.isfinite(g["Pcol"]).all() and np.isfinite(g["csum"]).all() and np.isfinite(g["Y"]).all()
        M = 3 * ntot
        for i, (s, jb, je) in enumerate(p["items"]):                                                # padding columns sum to zero exactly
            assert not g["Pcol"][i, max(0, M - s * 256):].any()


@pytest.mark.gpu
@pytest.mark.parametrize("o", st.OS)
def test_a_stopped_status_word_writes_nothing(gpu, o):
    ntot, world = st.SCAL_CASE
    Q, W = st.int_operands(ntot, o)
    nloc = ntot // world
    for r in (0, 2, 4):
        Qr = Q[3 * r * nloc:3 * (r + 1) * nloc]
        none = gpu.symw_probe(Qr, W, ntot, nloc, r * nloc, world, o, scal_status=-1)
        run = gpu.symw_probe(Qr, W, ntot, nloc, r * nloc, world, o, scal_status=0)
        for k in ("Prow", "Pcol", "csum", "Y"):
            assert st.same_values(none[k], run[k]), k
        assert np.isfinite(run["Pcol"]).all() and np.isfinite(run["csum"]).all() and np.isfinite(run["Y"]).all()
        stop = gpu.symw_probe(Qr, W, ntot, nloc, r * nloc, world, o, scal_status=1)
        assert np.isnan(stop["Prow"]).all() and np.isnan(stop["Pcol"]).all() and np.isnan(stop["csum"]).all()
        assert np.isnan(stop["cs_all"][r]).all() and not stop["cs_all"][np.arange(world) != r].any()


@pytest.mark.gpu
@pytest.mark.parametrize("ntot,world,o", [(4, 2, 3), (84, 6, 5), (140, 70, 1), (140, 70, 4), (256, 8, 3), (344, 4, 4), (344, 2, 5)])
def test_the_gathered_vectors_are_really_used(gpu, ntot, world, o):
    """arbitrary vectors in the other ranks' slots: Y = alpha * (row sums + own column sums + those vectors) -- integer-valued ones bit for
    bit, real-valued ones by the stage bound (their |values| join the scale)"""
    Q, W, _, stages, plans = int_model(gpu, ntot, world, o, 0)
    nloc = ntot // world
    rng = np.random.default_rng(ntot + world + o)
    for r in sorted({0, world // 2, world - 1}):
        others = np.arange(world) != r
        Qr = Q[3 * r * nloc:3 * (r + 1) * nloc]
        cs = rng.integers(-10 ** 6, 10 ** 6, (world, 3 * ntot, o)).astype(np.float64)
        got = gpu.symw_probe(Qr, W, ntot, nloc, r * nloc, world, o, alpha=-2.5, cs_all=cs.copy())
        assert st.same_values(got["cs_all"][others], cs[others]) and st.same_values(got["cs_all"][r], stages[r]["csum"])
        model = cs.astype(np.int64); model[r] = stages[r]["csum"]
        y, _ = st.rank_y(stages[r], plans[r], model, np.zeros(model.shape), r * nloc, nloc, 1, np.int64)
        assert st.same_values(got["Y"], -2.5 * y.astype(np.float64)), (ntot, world, o, r)
        # real-valued vectors over six decades
        cs = rng.standard_normal((world, 3 * ntot, o)) * 10.0 ** rng.uniform(-3, 3, (world, 3 * ntot, o))
        got = gpu.symw_probe(Qr, W, ntot, nloc, r * nloc, world, o, alpha=-2.5, cs_all=cs.copy())
        full = cs.copy(); full[r] = stages[r]["csum"]
        scale = np.abs(full)
        stf = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.int64 else v) for k, v in stages[r].items()}
        stl = {k: (v.astype(np.longdouble) if isinstance(v, np.ndarray) and v.dtype != bool else v) for k, v in stf.items()}
        truth, tscale = st.rank_y(stl, plans[r], full, scale, r * nloc, nloc, -2.5, np.longdouble)
        ref, _ = st.rank_y(stf, plans[r], full, scale, r * nloc, nloc, -2.5, np.float64)
        assert st.check_stage(f"gathered-n{ntot}-w{world}-o{o}-r{r}", "Y", st.scaled_error(ref, truth, tscale), st.scaled_error(got["Y"], truth, tscale))


@pytest.mark.gpu
@pytest.mark.parametrize("ntot,world,o", [(86, 1, 3), (130, 5, 4), (258, 3, 5), (344, 2, 1), (344, 4, 3)])
def test_same_bits_whatever_the_run_the_load_policy_the_chunk_and_the_padding(gpu, ntot, world, o):
    """real-valued data: two calls and both load policies give the same bits, and so does every pad_value; integer data: K changes neither
    csum nor Y"""
    Q, W = st.real_operands("random", ntot, o, seed=2)
    Y0, a = gpu.symw_product(Q, W, world, o, alpha=-2.5, K=3, nt=0)
    for kw in (dict(nt=0), dict(nt=1), dict(nt=0, pad_value=1e30), dict(nt=1, pad_value=-7.0), dict(nt=-1, pad_value=0.0)):
        Y1, b = gpu.symw_product(Q, W, world, o, alpha=-2.5, K=3, **kw)
        assert st.same_values(Y0, Y1), kw
        for r in range(world):
            for k in ("Prow", "Pcol", "csum", "Y"):
                assert st.same_values(a[r][k], b[r][k]), (kw, r, k)
    Q, W = st.int_operands(ntot, o)
    Y0, a = gpu.symw_product(Q, W, world, o, K=0)
    for K in st.KS[1:]:
        Y1, b = gpu.symw_product(Q, W, world, o, K=K, pad_value=(1e30 if K & 1 else -7.0))
        assert st.same_values(Y0, Y1) and all(st.same_values(a[r]["csum"], b[r]["csum"]) and st.same_values(a[r]["Prow"], b[r]["Prow"]) for r in range(world)), K


@pytest.mark.gpu
@pytest.mark.parametrize("ntot,world", CASE_IDS)
def test_unused_mirror_blocks_may_hold_anything_finite(gpu, ntot, world):
    """the block of every mirror pair that a row step does not use, overwritten by noise in the rank's strip: every output is unchanged on
    integer data -- the kernel masks, it does not merely happen to meet a symmetric matrix"""
    o = st.OS[(ntot // 2 + world + 1) % 4]
    K = 3 if ntot in st.LARGE else 0
    Q, W, _, stages, plans = int_model(gpu, ntot, world, o, K)
    nloc = ntot // world
    use = st.use_matrix(ntot // 2)
    cs_all = np.stack([s_["csum"] for s_ in stages]).astype(np.float64)
    changed = 0
    for r in range(world):
        Qn = st.noise_unused_mirror_blocks(Q[3 * r * nloc:3 * (r + 1) * nloc], plans[r], use, seed=r)
        changed += not np.array_equal(Qn, Q[3 * r * nloc:3 * (r + 1) * nloc])
        got = gpu.symw_probe(Qn, W, ntot, nloc, r * nloc, world, o, K=K, cs_all=cs_all.copy())
        check_rank_int(f"noise ntot {ntot} world {world} o {o} rank {r}", got, stages[r], plans[r], 1.0)
    assert changed or ntot == 2                                                                     # (one step: no mirror pair)
