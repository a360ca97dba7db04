"""GPU tests of the global positioning's kernels stage by stage (xm-code_amd/csrc/xm_gp.hip) through the test export xm_ctx_gp_probe: one
linearisation at a fixed point and a fixed mu, no LM loop, every array compared elementwise with the longdouble evaluation of the
restatement (xm_gp_numpy.stages with dtype = longdouble).

Bound (the bundle adjustment's, xm_ba_stages.py): e_gpu <= max(16 e_ref, 64 eps_f64) with e_ref the f64 restatement's own error against the
longdouble evaluation at the same point, per quantity and case; the error is max |x - x_exact| / max |x_exact| per natural block
(observation, landmark, camera).  Nothing is derived from the GPU's output.  Every comparison prints a line
`GP_STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s): the table of profiles/r27_gp_stage_errors.txt.

Which kernel an output pins: oused, cused, lused -> gp_setup, gp_lm_count, gp_used, gp_cam_count; cost, n_used, M, q, frozen -> gp_eval;
vinv, g_l -> gp_lm; ustar, sinv, b -> gp_cam; gmax -> all three; SX -> gp_lmx, gp_camx; dP -> gp_lmx (sign -1, with g_l); t1, p1 ->
gp_cand_vec; ds, s1, cost1, model, step2, x2 -> gp_cand_obs and ba_reduce."""
import numpy as np
import pytest

import xm_ba_loss_numpy as rl
import xm_ba_numpy as ba
import xm_ba_stages as st
import xm_gp_numpy as gp

pytestmark = pytest.mark.gpu

ARRAYS = ("M", "q", "vinv", "g_l", "ustar", "sinv", "b", "SX", "dP", "ds", "t1", "p1", "s1", "step2", "x2")
SCALARS = ("cost", "gmax", "cost1", "model")
MUS = (1e-4, 3.0)


def _observe(S, cams, lms):
    """depth-lifted camera-frame points of the (camera, landmark) pairs at the scene's geometry"""
    R = np.stack([S["rot"][:, 3 * i:3 * i + 3] for i in range(S["n"])])
    return np.einsum("kba,kb->ka", R[cams], (S["P"][:, lms] - S["t"][:, cams]).T)


def _point(S, seed, spread=0.05):
    rng = np.random.default_rng(seed)
    t = S["t"] + spread * rng.standard_normal(S["t"].shape)
    P = S["P"] + spread * rng.standard_normal(S["P"].shape)
    depth = np.linalg.norm(S["P"][:, S["lm"]] - S["t"][:, S["cam"]], axis=0)
    return t, P, (1.0 / depth) * rng.uniform(0.8, 1.25, depth.size)


def base_scene():
    return ba.ring_scene(n_cams=8, n_pts=40, seed=0, noise=2e-3)


def edge_scene(lim):
    """landmarks on each side of the light / heavy split and one at it, a camera list one longer than a wavefront pass, a pair named twice,
    zero weights, a landmark below min_views and a camera left without a used observation"""
    split, cpass = lim["light_max"], lim["cam_pass"]
    n = split + 6
    S = ba.ring_scene(n_cams=n, n_pts=cpass + 12, seed=2, noise=1e-3, frac=0.06)
    cam, lm = list(S["cam"]), list(S["lm"])
    keep = [k for k in range(len(cam)) if lm[k] >= 3 and cam[k] != 0]
    cam, lm = [cam[k] for k in keep], [lm[k] for k in keep]
    for l, d in zip((0, 1, 2), (split - 1, split, split + 1)):               # landmarks 0, 1, 2: 63, 64 and 65 observations
        cam += list(range(1, d + 1)); lm += [l] * d
    cam += [0] * (cpass + 1); lm += list(range(3, cpass + 4))                # camera 0: 65 observations
    cam += [5]; lm += [2]                                                    # (5, 2) named twice: landmark 2 has 66
    last = S["m"] - 1                                                       # the last landmark: two observations only (below min_views)
    sel = [k for k in range(len(cam)) if lm[k] != last]
    cam, lm = [cam[k] for k in sel] + [2, 3], [lm[k] for k in sel] + [last, last]
    cam, lm = np.array(cam, dtype=np.int32), np.array(lm, dtype=np.int32)
    p = _observe(S, cam, lm) * (1.0 + 1e-3 * np.random.default_rng(3).standard_normal((cam.size, 1)))
    p[:, :2] += 1e-3 * np.random.default_rng(4).standard_normal((cam.size, 2))
    p[cam == 4] *= -1.0                                                      # camera 4: every observation behind it (p_2 < 0): not used
    w = np.ones(cam.size)
    w[np.nonzero(lm == 9)[0][1:]] = 0.0                                      # landmark 9: one weighted observation left
    w[np.nonzero(lm == 2)[0][::9]] = 0.0                                     # and some of the heavy landmark's weights
    deg = np.bincount(lm, minlength=S["m"])
    assert tuple(deg[:3]) == (split - 1, split, split + 2) and np.bincount(cam)[0] == cpass + 1
    return dict(S, cam=cam, lm=lm, p=p, w=w, w0=np.ones(cam.size))


CASES = ("base", "edges", "bound") + tuple("loss_" + k for k in rl.LOSSES)


def case(name, lim):
    loss, a = "huber", 0.1
    if name == "edges":
        S = edge_scene(lim)
    else:
        S = base_scene()
    t, P, s = _point(S, 11)
    if name == "bound":
        P, s = gp.bound_point(S, t, P, s)
    if name.startswith("loss_"):
        loss = name[5:]
        a = 0.0 if loss == "trivial" else 0.02                              # residuals on both sides of the scale
    rng = np.random.default_rng(12)
    return dict(S=S, t=t, P=P, s=s, loss=loss, a=a, X=rng.standard_normal((3 * S["n"], 2)), dc=1e-2 * rng.standard_normal(3 * S["n"]))


def _ctx(xmamd, S):
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S.get("w0", S["w"])), n=S["n"])
    if "w0" in S:
        ctx.set_edge_weights(S["w"])
    return ctx


def _blocks(k, v):
    v = np.asarray(v)
    if k in ("t1", "p1"):
        return v.T
    if k in ("SX",):
        return v.reshape(v.shape[0] // 3, -1)
    if k in ("step2", "x2"):
        return v.reshape(3, 1)
    return v.reshape(v.shape[0], -1)


@pytest.mark.parametrize("name", CASES)
def test_stage_outputs_against_the_longdouble_evaluation(xmamd, name):
    c = case(name, xmamd.gp_limits())
    S = c["S"]
    ctx = _ctx(xmamd, S)
    bad = []
    for mu in MUS:
        got = ctx.gp_probe(S["rot"], c["t"], c["P"], mu, s=c["s"], loss=c["loss"], loss_scale=c["a"], X=c["X"], dc=c["dc"])
        ev = {}
        for dt in (np.float64, gp.LD):
            pr = gp.Problem(S["cam"], S["lm"], S["p"], S["w"], S["rot"], S["n"], S["m"], 3, c["loss"], c["a"], dtype=dt)
            ev[dt] = gp.stages(pr, c["t"], c["P"], c["s"], mu, X=c["X"], dc=c["dc"])
        F, E = ev[np.float64], ev[gp.LD]
        # exact comparisons stay exact
        assert got["n_used"] == E["n_used"] and np.array_equal(got["oused"] != 0, pr.mask)
        assert np.array_equal(got["cused"] != 0, E["cused"]) and np.array_equal(got["lused"] != 0, E["lused"])
        assert np.array_equal(got["frozen"], E["frozen"])
        for k in ARRAYS + SCALARS:
            if k in SCALARS:
                e_ref = abs(float(F[k]) - E[k]) / abs(E[k])
                e_gpu = abs(gp.LD(got[k]) - E[k]) / abs(E[k])
            else:
                e_ref, _ = st.err(_blocks(k, F[k]), _blocks(k, E[k]))
                e_gpu, _ = st.err(_blocks(k, got[k]), _blocks(k, E[k]))
            assert e_ref <= st.MAX_E_REF, (k, e_ref)
            lim = st.bound(e_ref)
            print(f"GP_STAGE_ERR {name}-mu{mu:g} {k}: e_ref {float(e_ref):.3e}, e_gpu {float(e_gpu):.3e}, ratio {float(e_gpu) / lim:.3f}")
            if not e_gpu <= lim:
                bad.append((mu, k, float(e_ref), float(e_gpu)))
        if name == "edges":
            assert not E["cused"][4] and not E["lused"][9] and not E["lused"][S["m"] - 1]
            off = ~E["cused"]
            assert got["t1"][:, off].tobytes() == np.asfortranarray(c["t"])[:, off].tobytes()
            assert got["p1"][:, ~E["lused"]].tobytes() == np.asfortranarray(c["P"])[:, ~E["lused"]].tobytes()
            assert np.all(got["s1"][~pr.mask] == -1.0) and not got["ds"][~pr.mask].any() and not got["M"][~pr.mask].any()
            assert not got["b"][off].any() and not got["dP"][~E["lused"]].any()
        if name == "bound":
            fr = got["frozen"] != 0
            at = pr.mask & (c["s"] <= gp.S_MIN)
            assert fr.any() and (at & ~fr).any()                            # at the bound: some frozen, some free
            assert not got["ds"][fr].any() and np.all(got["s1"][fr] == gp.S_MIN)
            assert np.all(got["M"][fr][:, [1, 2, 4]] == 0)                  # M_e = w s^2 I
    ctx.close()
    assert not bad, bad
