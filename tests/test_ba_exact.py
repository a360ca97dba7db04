"""CPU tests that tie the references of tests/test_gpu_ba_stages.py together before they judge a kernel: the f64 restatements
(xm_ba_numpy.py, xm_ba_loss_numpy.py, xm_ba_precond_numpy.py) agree with the longdouble module (xm_ba_exact.py) on every case of the GPU
test to e_ref <= 1e-8; the longdouble module is consistent in itself (symmetry, finite differences, M^-1 S_aa = I, P^T S P = A_c) and, where
mpmath is present, agrees with 50-digit arithmetic; and the bound max(16 e_ref, 64 eps) rejects the f64 result damaged the way a kernel bug
would damage it."""
import numpy as np
import pytest

import xm_ba_exact as ex
import xm_ba_stages as st

LD = ex.LD


def test_longdouble_is_extended():
    assert np.finfo(LD).eps < 2e-19 and np.finfo(LD).nmant >= 63


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("name", st.CASES)
def test_restatements_agree_with_longdouble(name, fix):
    """every case of the GPU test, none left out: e_ref <= 1e-8 for every compared quantity, flags and counts equal"""
    c = st.case(name, fix)
    S = c["S"]
    for mu in c["mus"]:
        kw = st.stage_args(c, mu)
        E = st.exact_stages(S, **kw)
        e_ref = st.reference_errors(S, E, c["keys"], **kw)
        print(f"{name} fix={fix} mu={mu:g}: " + ", ".join(f"{k} {v:.1e}" for k, v in e_ref.items()))
        assert max(e_ref.values()) <= st.MAX_E_REF, e_ref
        R = st.f64_stages(S, **kw)
        assert R["dropped"] == E["dropped"]
    if name == "degrees":
        assert list(c["extra"]["degrees"][:6]) == list(st.DEGREES) and c["extra"]["degrees"][6] > 1024
    if name == "one_centre":
        assert len(E["dropped"]) == 1
    if name == "clamp":
        d = E["_E"].V[:, np.arange(3), np.arange(3)]
        assert (d[E["lused"]] < 1e-6).any() and (d[E["lused"]].min(axis=1) > 1e-6).any()
    if name == "masks":
        assert not E["cused"][5] and not E["lused"][7] and E["cused"].sum() == S["n"] - 1
    if name == "loss_huber":
        assert [s for _, s in c["extra"]["edge"]] == [c["a"] * c["a"], np.nextafter(c["a"] * c["a"], np.inf)]


def test_aggregate_cases_cover_the_last_aggregates():
    got = set()
    for k in st.AGG_SIZES:
        order = st.plan_order(st.aggregate_scene(k)[0])
        assert len(order) == k
        got.add(k % 16)
    assert got == {0, 1, 2, 15}


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
def test_exact_module_is_consistent(fix):
    c = st.case("agg33", fix)
    S, (rot, t, P) = c["S"], c["point"]
    E = ex.Exact(S["cam"], S["lm"], S["p"], S["w"], S["n"], S["m"], rot, t, P, 1e-4, fix)
    cd, n, order = E.cd, E.n, c["order"]
    assert np.array_equal(E.S, E.S.T) or float(np.abs(E.S - E.S.T).max() / np.abs(E.S).max()) < 1e-18
    # M^-1 restricted to one aggregate times S_aa is the identity (blocks), and the merged member sits in the last coarse aggregate
    M = E.block_inverse(order)
    for k0 in range(0, len(order), ex.AGG_CAMS):
        idx = (cd * np.asarray(order[k0:k0 + ex.AGG_CAMS])[:, None] + np.arange(cd)[None, :]).reshape(-1)
        assert float(np.abs(M[np.ix_(idx, idx)] @ E.S[np.ix_(idx, idx)] - np.eye(idx.size)).max()) < 1e-13
    Pm, dropped = E.rigid_basis(order)
    assert Pm.shape[1] == (7 if cd == 6 else 4) * 2 and not dropped           # 33 members: three blocks, two coarse aggregates
    last = order[32]
    assert np.abs(Pm[cd * last:cd * last + cd, Pm.shape[1] // 2:]).max() > 0
    # P^T S P column by column against the module's A_c
    Ac = E.coarse_operator(Pm, dropped)
    SP = np.stack([E.S @ Pm[:, q] for q in range(Pm.shape[1])], axis=1)
    assert float(np.abs(Pm.T @ SP - Ac).max() / np.abs(Ac).max()) < 1e-17
    # the coarse space is what it says: moving the world rigidly (and scaling it) about the centroid leaves every residual unchanged to
    # first order, so J_c P + J_P (dX of the landmarks) = 0.  Checked for the first aggregate's columns on its own cameras' observations
    nc = Pm.shape[1] // 2
    mem = np.asarray(order[:16])
    C = -np.einsum("iba,ib->ia", E.Rcw, E.tcw)
    cen = C[mem].sum(axis=0) / LD(16)
    sel = np.isin(E.cam, mem)
    for q in range(nc):
        col = Pm[:, q].reshape(n, cd)
        scale = np.sqrt(np.sum(_unscaled_column(E, mem, cen, q) ** 2))
        X = E.P[E.lm[sel]]
        w, v, s = _motion(q, cd)
        dX = (np.cross(w, X - cen) + v + s * (X - cen)) / scale
        lin = np.einsum("kra,ka->kr", E.Jc[sel], col[E.cam[sel]]) + np.einsum("kra,ka->kr", E.JP[sel], dX)
        ref = np.abs(np.einsum("kra,ka->kr", E.JP[sel], dX)).max()
        assert float(np.abs(lin).max()) <= 1e-15 * float(ref), (q, float(np.abs(lin).max()), float(ref))
    # finite differences (longdouble, step 1e-9) of the residuals against J_c and J_P
    h = LD(1e-9)
    rng = np.random.default_rng(0)
    dcv, dPv = rng.standard_normal((n, cd)).astype(LD), rng.standard_normal((E.m, 3)).astype(LD)
    def res(sg):
        R1 = E.Rcw.copy()
        if cd == 6:
            R1 = ex.expmap(sg * h * dcv[:, :3]) @ E.Rcw
        return E.linearise(R1, E.tcw + sg * h * dcv[:, cd - 3:], E.P + sg * h * dPv)[0]
    fd = (res(1) - res(-1)) / (2 * h)
    lin = np.einsum("kra,ka->kr", E.Jc, dcv[E.cam]) + np.einsum("kra,ka->kr", E.JP, dPv[E.lm])
    assert float(np.abs(fd - lin).max() / np.abs(lin).max()) < 1e-8


def _motion(q, cd):
    """(w, v, s) of coarse column q"""
    e = np.zeros(7, dtype=LD)
    e[q + (3 if cd == 3 else 0)] = 1
    return e[:3], e[3:6], e[6]


def _unscaled_column(E, mem, cen, q):
    w, v, s = _motion(q, E.cd)
    C = -np.einsum("iba,ib->ia", E.Rcw, E.tcw)
    out = []
    for i in mem:
        R = E.Rcw[i]
        dth = -R @ w
        dt = R @ (np.cross(C[i] - cen, w) - np.cross(C[i], w)) - R @ v - s * (R @ (C[i] - cen))
        out.append(np.concatenate([dth, dt]) if E.cd == 6 else dt)
    return np.concatenate(out)


@pytest.mark.parametrize("loss", ["huber", "soft_l1", "cauchy", "arctan"])
def test_rho_prime_by_finite_differences(loss):
    a = 0.05
    s = np.array([1e-6, 0.3, 0.9, 1.1, 3.0, 1e3, 1e6], dtype=LD) * LD(a) * LD(a)
    h = s * LD(1e-9)
    fd = (ex.rho(loss, s + h, a)[0] - ex.rho(loss, s - h, a)[0]) / (2 * h)
    r0, r1 = ex.rho(loss, s, a)
    # truncation 1e-8 (relative; the step is 1e-9 s) plus the rounding of the two function values over the step
    assert np.all(np.abs(fd - r1) <= 1e-8 * r1 + 4 * np.finfo(LD).eps * r0 / h)
    at = ex.rho(loss, np.array([a * a], dtype=LD), a)          # Huber's kink: both branches meet at s = a^2
    up = ex.rho(loss, np.array([np.nextafter(a * a, np.inf)], dtype=LD), a)
    assert abs(float(up[0][0] / at[0][0]) - 1) < 1e-15 and abs(float(up[1][0] / at[1][0]) - 1) < 1e-15


def test_spot_check_at_50_digits():
    """where mpmath is present: the longdouble Rodrigues formula, rho and the Gauss-Jordan inverse against 50-digit arithmetic"""
    try:
        import mpmath as mp
    except ImportError:
        return
    mp.mp.dps = 50
    for nm in (1e-200, 9.9e-9, 1e-8, 1e-3, 1.0, np.pi - 1e-9, np.pi, 4.0):
        w = np.array([0.6, -0.48, 0.64]) * nm
        th = mp.sqrt(sum(mp.mpf(float(x)) ** 2 for x in w))
        K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        Em = mp.eye(3) + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * (K * K)
        El = ex.expmap(w[None, :])[0]
        assert max(abs(mp.mpf(float(El[i, j])) + mp.mpf(float(El[i, j] - LD(float(El[i, j])))) - Em[i, j]) for i in range(3) for j in range(3)) < 1e-18
    rng = np.random.default_rng(0)
    A = rng.standard_normal((12, 12)); A = A @ A.T + 1e-3 * np.eye(12)
    Am = mp.matrix(A.tolist()) ** -1
    Al = ex.gj_inverse(A)
    scale = max(abs(Am[i, j]) for i in range(12) for j in range(12))
    assert max(abs(mp.mpf(float(Al[i, j])) + mp.mpf(float(Al[i, j] - LD(float(Al[i, j])))) - Am[i, j]) for i in range(12) for j in range(12)) / scale < 1e-14
    a = 0.05
    for s in (1e-9, 2.4e-3, 2.6e-3, 7.0, 2500.0):
        want = {"huber": s if s <= a * a else 2 * a * mp.sqrt(s) - a * a, "soft_l1": 2 * a * a * (mp.sqrt(1 + mp.mpf(s) / (a * a)) - 1),
                "cauchy": a * a * mp.log(1 + mp.mpf(s) / (a * a)), "arctan": a * mp.atan2(s, a)}
        for loss, v in want.items():
            got = ex.rho(loss, np.array([s], dtype=LD), a)[0][0]
            assert abs(mp.mpf(float(got)) / mp.mpf(v) - 1) < 1e-13, (loss, s)


# ---- the bounds bite: the f64 restatement's result, damaged the way a kernel bug would damage it, must miss max(16 e_ref, 64 eps)
def _judge(c, mu, keys, damage):
    S = c["S"]
    kw = st.stage_args(c, mu)
    E = st.exact_stages(S, **kw)
    e_ref = st.reference_errors(S, E, keys, **kw)
    good = st.compare("undamaged", S, st.f64_stages(S, **kw), E, e_ref, keys, who="f64")
    bad = st.compare("damaged " + str(damage), S, st.f64_stages(S, damage=damage, **kw), E, e_ref, keys, who="f64")
    assert not good
    return {k for k, *_ in bad}


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
def test_bound_rejects_a_dropped_camera_pair(fix):
    c = st.case("agg33", fix)
    i, j = int(c["order"][3]), int(c["order"][4])                     # neighbours along the capture, both in the first aggregate
    assert {"MX_blocks", "MX_two_level"} <= _judge(c, 1e-4, ("MX_blocks", "MX_two_level"), dict(drop_pair=(i, j)))


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
def test_bound_rejects_swapped_coarse_columns(fix):
    c = st.case("agg33", fix)
    nc = 4 if fix else 7
    assert {"MX_two_level", "Ac"} <= _judge(c, 1e-4, ("MX_two_level", "Ac"), dict(swap_coarse=(nc - 1, nc)))


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
def test_bound_rejects_the_merged_member_left_out(fix):
    c = st.case("agg33", fix)                                         # 33 members: the last one is merged into the second coarse aggregate
    assert "MX_two_level" in _judge(c, 1e-4, ("MX_two_level",), dict(leave_out_merged=True))


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
def test_bound_rejects_mu_diag_where_the_clamp_applies(fix):
    c = st.case("clamp", fix)
    assert {"vinv", "S", "b"} <= _judge(c, 1.0, ("vinv", "S", "b"), dict(no_clamp=True))


@pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])
def test_bound_rejects_a_skipped_65th_observation(fix):
    c = st.case("degrees", fix)
    for l in (c["extra"]["roles"][4], c["extra"]["roles"][6]):        # the landmark of degree 65, and the one above 1024
        assert {"vinv", "b", "SX"} <= _judge(c, 1e-4, ("vinv", "b", "SX"), dict(skip_observation=(l, 64)))
