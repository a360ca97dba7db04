"""GPU tests of the kernels behind xm_ctx_global_positioning_pairs stage by stage (xm-code_amd/csrc/xm_gp.hip) through the test export
xm_ctx_gp_probe_pairs: one linearisation at a fixed point and two dampings, no LM loop, every array compared per natural block
(observation, pair, landmark, camera) with the longdouble evaluation of the restatement (xm_gp_pairs_numpy.stages, dtype = longdouble).

Bound (the project's, xm_ba_stages.py): e_gpu <= max(16 e_ref, 64 eps_f64) with e_ref the f64 restatement's own error against the
longdouble evaluation at the same point.  Nothing is derived from the GPU's output.  Every comparison prints a line
`GP_PAIR_STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s): the table of profiles/r39_gp_pairs_stage_errors.txt.

Which kernel an output pins: pused, cused -> gp_pair_used; Mp, qp, pfrozen, pcost, pgsmax -> gp_pair_setup, gp_pair_eval; ustar, sinv, b,
gmax -> gp_pair_cam and gp_cam<PAIRS>; SX -> gp_pairx and gp_camx<PAIRS>; dsigma, sigma1, pcost1, pmodel, pstep2, px2 -> gp_cand_pair;
M, q, cost, ds, cost1, model with `calibrated` or BALANCED -> the weighted instances of gp_eval and gp_cand_obs; the fixed-centre case
-> GpWork's launches without a camera pass."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import xm_ba_loss_numpy as rl
import xm_ba_numpy as ba
import xm_ba_stages as st
import xm_gp_pairs_numpy as gpp

pytestmark = pytest.mark.gpu

OBS_ARRAYS = ("M", "q", "vinv", "g_l", "dP", "ds", "p1", "s1", "step2", "x2")
CAM_ARRAYS = ("ustar", "sinv", "b", "SX", "t1")
PAIR_ARRAYS = ("Mp", "qp", "dsigma", "sigma1")
OBS_SCALARS = ("cost", "cost1", "model")
PAIR_SCALARS = ("pcost", "pgsmax", "pcost1", "pmodel", "pstep2", "px2")
MUS = (1e-4, 3.0)


def _point(S, pairs, seed, spread=0.05):
    rng = np.random.default_rng(seed)
    t = S["t"] + spread * rng.standard_normal(S["t"].shape)
    P = S["P"] + spread * rng.standard_normal(S["P"].shape)
    depth = np.linalg.norm(S["P"][:, S["lm"]] - S["t"][:, S["cam"]], axis=0)
    dist = np.linalg.norm(S["t"][:, pairs[1]] - S["t"][:, pairs[0]], axis=0)
    return t, P, (1.0 / depth) * rng.uniform(0.8, 1.25, depth.size), (1.0 / dist) * rng.uniform(0.8, 1.25, dist.size)


def ring_case():
    S = ba.ring_scene(n_cams=8, n_pts=40, seed=0, noise=2e-3)
    pi, pj = gpp.all_pairs(8)
    return S, (pi, pj, gpp.relative_translations(S, pi, pj, noise=1e-3, seed=1), None)


def edge_case(split):
    """split + 6 cameras.  Cameras 0, 1, 2 have split + 1, split and split - 1 incidences (camera 0: one pair named twice); the pairs
    alternate their direction; camera 3 has only invalid pairs and no used observation (it must come back bit-identical); camera 4 has valid
    pairs and no used observation; a few more invalid pairs; zero-weight observations"""
    n = split + 6
    S = ba.ring_scene(n_cams=n, n_pts=40, seed=2, noise=1e-3, frac=0.2)
    G = sp.coo_matrix((np.ones(S["cam"].size), (S["cam"], n + S["lm"])), shape=(n + S["m"], n + S["m"]))
    assert connected_components(G, directed=False)[0] == 1                    # a context needs a connected observation graph
    S = dict(S, p=S["p"].copy())
    S["p"][np.isin(S["cam"], (3, 4))] *= -1.0                                 # cameras 3 and 4: every observation behind them, none used
    w = np.ones(S["cam"].size)
    w[::7] = 0.0
    S["w0"], S["w"] = np.ones(S["cam"].size), w
    prs, valid = [], []
    for hub, last in ((0, split + 4), (1, split + 4), (2, split + 3)):        # partners 5 .. last: split, split, split - 1 of them
        for k in range(5, last + 1):
            prs.append((hub, k) if (hub + k) % 2 else (k, hub)); valid.append(1)
    prs.append((0, 5)); valid.append(1)                                       # named twice: camera 0 has split + 1 incidences
    prs += [(3, k) for k in range(5, 11)]; valid += [0] * 6
    prs += [(4, 20), (30, 4)]; valid += [1, 1]
    prs += [(0, n - 1), (n - 1, 1), (6, 7)]; valid += [0, 0, 0]
    pi, pj = np.array(prs, dtype=np.int32).T
    valid = np.array(valid, dtype=np.uint8)
    inc = np.bincount(np.concatenate([pi[valid != 0], pj[valid != 0]]), minlength=n)
    assert tuple(inc[:5]) == (split + 1, split, split - 1, 0, 2)
    return S, (np.ascontiguousarray(pi), np.ascontiguousarray(pj), gpp.relative_translations(S, pi, pj, noise=1e-3, seed=3), valid)


CASES = tuple("loss_" + k for k in rl.LOSSES) + ("edges", "bound", "balanced", "only_cameras", "fixed")


def case(name, split):
    kw = dict(constraint="points_and_cameras", calibrated=None, reweight_scale=1.0, fix_centres=False)
    loss, a = "huber", 0.1
    S, pairs = edge_case(split) if name == "edges" else ring_case()
    t, P, s, sg = _point(S, pairs, 11)
    if name.startswith("loss_"):
        loss = name[5:]
        a = 0.0 if loss == "trivial" else 0.02                              # residuals on both sides of the scale
    if name == "bound":                                                      # pair 0: c_j - c_i against tau (outward: frozen); pair 1: inward
        sg[[0, 1]] = gpp.S_MIN
        i, j = pairs[0][0], pairs[1][0]
        t[:, j] = t[:, i] - 3.0 * (S["t"][:, j] - S["t"][:, i])
    if name == "balanced":
        kw.update(constraint="points_and_cameras_balanced", calibrated=np.arange(S["n"]) % 3 != 1, reweight_scale=2.5)
    if name == "only_cameras":
        kw.update(constraint="only_cameras")
    if name == "fixed":
        kw.update(constraint="only_points", fix_centres=True, calibrated=np.arange(S["n"]) % 2 == 0)
    rng = np.random.default_rng(12)
    return dict(S=S, pairs=pairs, t=t, P=P, s=s, sg=sg, loss=loss, a=a, kw=kw, X=rng.standard_normal((3 * S["n"], 2)),
                dc=1e-2 * rng.standard_normal(3 * S["n"]))


def _blocks(k, v):
    v = np.asarray(v)
    if k in ("t1", "p1"):
        return v.T
    if k == "SX":
        return v.reshape(v.shape[0] // 3, -1)
    if k in ("step2", "x2"):
        return v.reshape(3, 1)
    return v.reshape(v.shape[0], -1)


@pytest.mark.parametrize("name", CASES)
def test_pair_stage_outputs_against_the_longdouble_evaluation(xmamd, name):
    split = xmamd.gp_pair_limits()["light_max"]
    c = case(name, split)
    S, pairs, kw = c["S"], c["pairs"], c["kw"]
    fix, has_obs, has_pairs = kw["fix_centres"], kw["constraint"] != "only_cameras", kw["constraint"] != "only_points"
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S.get("w0", S["w"])), n=S["n"])
    if "w0" in S:
        ctx.set_edge_weights(S["w"])
    bad = []
    for mu in MUS:
        got = ctx.gp_probe_pairs(S["rot"], c["t"], c["P"], mu, pairs=pairs, s=c["s"], sigma=c["sg"], loss=c["loss"], loss_scale=c["a"],
                                 X=None if fix else c["X"], dc=c["dc"], **kw)
        ev = {}
        for dt in (np.float64, gpp.LD):
            pr = gpp.Problem(S["cam"], S["lm"], S["p"], S["w"], S["rot"], S["n"], S["m"], pairs, kw["constraint"], kw["calibrated"],
                             kw["reweight_scale"], fix, 3, c["loss"], c["a"], dtype=dt)
            ev[dt] = gpp.stages(pr, c["t"], c["P"], c["s"], c["sg"], mu, X=c["X"], dc=c["dc"])
        F, E = ev[np.float64], ev[gpp.LD]
        # exact comparisons stay exact
        assert got["n_used"] == E["n_used"] and np.array_equal(got["oused"] != 0, pr.mask) and got["pairs_used"] == pr.M
        assert np.array_equal(got["cused"] != 0, E["cused"]) and np.array_equal(got["lused"] != 0, E["lused"])
        assert np.array_equal(got["frozen"], E["frozen"]) and np.array_equal(got["pfrozen"], E["pfrozen"]) and np.array_equal(got["pused"], E["pused"])
        assert got["weight_scale_pt"] == pr.weight_scale_pt
        arrays = (OBS_ARRAYS if has_obs else ("p1", "s1", "step2", "x2")) + (() if fix else CAM_ARRAYS) + (PAIR_ARRAYS if has_pairs else ())
        scalars = ("gmax",) + (OBS_SCALARS if has_obs else ()) + (PAIR_SCALARS if has_pairs else ())
        for k in arrays + scalars:
            if k in scalars:
                den = abs(E[k]) if E[k] != 0 else 1
                e_ref, e_gpu = abs(float(F[k]) - E[k]) / den, abs(gpp.LD(got[k]) - E[k]) / den
            else:
                e_ref, _ = st.err(_blocks(k, F[k]), _blocks(k, E[k]))
                e_gpu, _ = st.err(_blocks(k, got[k]), _blocks(k, E[k]))
            assert e_ref <= st.MAX_E_REF, (k, e_ref)
            lim = st.bound(e_ref)
            print(f"GP_PAIR_STAGE_ERR {name}-mu{mu:g} {k}: e_ref {float(e_ref):.3e}, e_gpu {float(e_gpu):.3e}, ratio {float(e_gpu) / lim:.3f}")
            if not e_gpu <= lim:
                bad.append((mu, k, float(e_ref), float(e_gpu)))
        if not has_pairs:
            assert got["pcost"] == 0 and not got["Mp"].any() and np.all(got["sigma1"] == -1)
        if not has_obs:
            assert got["cost"] == 0 and got["n_used"] == 0 and not got["M"].any() and np.all(got["s1"] == -1)
            assert got["p1"].tobytes() == np.asfortranarray(c["P"]).tobytes()
        if fix:
            assert got["t1"].tobytes() == np.asfortranarray(c["t"]).tobytes() and got["step2"][0] == 0 and got["x2"][0] == 0
        if name == "edges":
            assert got["cams_heavy"] == 1 and got["max_incidences"] == split + 1
            assert not E["cused"][3] and E["cused"][4] and not pr.mask[S["cam"] == 4].any()
            off = ~E["cused"]
            assert got["t1"][:, off].tobytes() == np.asfortranarray(c["t"])[:, off].tobytes()
            inv = pairs[3] == 0
            assert np.all(got["sigma1"][inv] == -1.0) and not got["dsigma"][inv].any() and not got["Mp"][inv].any() and not got["b"][off].any()
            assert not got["M"][~pr.mask].any() and np.all(got["s1"][~pr.mask] == -1.0)
        if name == "bound":
            assert got["pfrozen"][0] == 1 and got["pfrozen"][1] == 0
            assert got["dsigma"][0] == 0 and got["sigma1"][0] == gpp.S_MIN and got["sigma1"][1] > gpp.S_MIN
            assert np.all(got["Mp"][0][[1, 2, 4]] == 0)                     # M_m = w sigma^2 I
    ctx.close()
    assert not bad, bad
