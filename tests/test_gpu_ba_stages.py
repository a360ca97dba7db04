"""GPU tests of the bundle adjustment's kernels stage by stage (xm-code_amd/csrc/xm_ba.hip) through the test export xm_ctx_ba_probe: one
linearisation at a fixed point and a fixed mu, no LM loop, every array compared elementwise with the longdouble reference xm_ba_exact.py.

Bound (xm_ba_stages.py): e_gpu <= max(16 e_ref, 64 eps_f64) with e_ref the f64 restatements' own error against the same reference at the
same point, evaluated here per quantity and case (the larger of two observation orders).  Nothing is derived from the GPU's output.  The
cases are those of test_ba_exact.py::test_restatements_agree_with_longdouble (which asserts e_ref <= 1e-8 for each); none is left out.
Every comparison prints a line `STAGE_ERR <case> <quantity>: e_ref, e_gpu, ratio` (pytest -s): the table of profiles/r12_ba_stage_errors.txt.

Which kernel an output pins: cost, n_used -> ba_eval, ba_reduce; g_l, vinv, lused -> ba_lm; b, ustar, sinv, cused -> ba_cam; gmax -> both;
SX -> ba_lmx, ba_camx; S -> ba_schur_dense; MX_jacobi -> ba_pcg_init; MX_blocks -> ba_tl_block, ba_tl_apply_block (and the sums of
ba_tl_apply_coarse); Pm, dropped -> ba_tl_basis; Ac -> ba_tl_coarse; MX_two_level -> those, spd_inverse_device and ba_tl_apply_coarse;
dP -> ba_lmx (sign -1, with g_l); rot1, t1, step2[0], x2[0] -> ba_cand_cam; p1, step2[1], x2[1] -> ba_cand_lm; cost1, model -> ba_cost.

What these tests found in the kernels as they were (fixed with them; DESIGN.md section 2.11 has the figures): on the degree case, whose last
landmark names each observation 16 times, sinv_i S_ii - I was 1.2e-2 and MX_jacobi off by 2.7e-3, because ba_cam_kernel left the cross terms
of a pair named more than once out of S_ii; Ac missed the bound on the base case at mu = 1e6 (2.2e-14, 31.6 e_ref) and on the degree case
(6.5e-14, up to 86 e_ref; MX_two_level 185 e_ref), because ba_tl_coarse_kernel subtracted thousands of small terms from P^T U* P one by one."""
import ctypes as C

import numpy as np
import pytest

import xm_ba_numpy as ba
import xm_ba_stages as st
import xm_testlib as tl

pytestmark = pytest.mark.gpu

FIX = pytest.mark.parametrize("fix", [False, True], ids=["free", "fixed"])


def _ctx(xmamd, S, **kw):
    ctx = xmamd.Context(obs=(S["cam"], S["lm"], S["p"], S.get("w0", S["w"])), n=S["n"], **kw)
    if "w0" in S:
        ctx.set_edge_weights(S["w"])
    return ctx


def _probe_all(ctx, c, mu, X=None):
    """the probe once per preconditioner; the outputs under the keys of xm_ba_stages"""
    rot, t, P = c["point"]
    X = c["X"] if X is None else X
    got = {}
    for kind in st.KINDS:
        g = ctx.ba_probe(rot, t, P, mu, fix_rotations=c["fix"], loss=c["loss"], loss_scale=c["a"], preconditioner=kind, X=X, dc=c["dc"],
                         dense=(kind == "jacobi"))
        got["MX_" + kind] = g["MX"]
        if kind == "jacobi":
            got.update(g)
            got["S"] = g["Sdense"]
        else:
            for k in ("b", "g_l", "vinv", "ustar", "sinv", "SX", "dP", "rot1", "t1", "p1"):       # the preconditioner changes nothing else
                assert g[k].tobytes() == got[k].tobytes(), (kind, k)
        if kind == "two_level":
            got.update(Pm=g["Pm"], Ac=g["Ac"], dropped=g["dropped"], coarse_ok=g["coarse_ok"], ncoarse=g["ncoarse"], nagg=g["nagg"])
    return got


def _judge(label, c, mu, got):
    S = c["S"]
    kw = st.stage_args(c, mu)
    E = st.exact_stages(S, **kw)
    e_ref = st.reference_errors(S, E, c["keys"], **kw)
    assert max(e_ref.values()) <= st.MAX_E_REF, e_ref
    bad = st.compare(label, S, got, E, e_ref, c["keys"])
    # exact comparisons stay exact
    assert got["n_used"] == E["n_used"]
    assert np.array_equal(got["cused"] != 0, E["cused"]) and np.array_equal(got["lused"] != 0, E["lused"])
    nmem = len(c["order"])
    nagg = (nmem + 15) // 16
    assert got["nagg"] == nagg and got["ncoarse"] == (nagg - 1 if nagg > 1 and nmem % 16 == 1 else nagg) and got["coarse_ok"] == 1
    assert sorted(np.nonzero(got["dropped"])[0].tolist()) == sorted(E["dropped"]) and set(np.unique(got["dropped"])) <= {0.0, 1.0}
    assert not bad, bad
    return E, e_ref


@FIX
@pytest.mark.parametrize("name", st.CASES)
def test_stage_outputs_against_the_longdouble_reference(xmamd, name, fix):
    c = st.case(name, fix)
    S, cd, n = c["S"], 3 if fix else 6, c["S"]["n"]
    rot, t, P = c["point"]
    ctx = _ctx(xmamd, S)
    for mu in c["mus"]:
        got = _probe_all(ctx, c, mu)
        E, e_ref = _judge(f"{name}-{'fixed' if fix else 'free'}-mu{mu:g}", c, mu, got)
        if name == "degrees":
            roles, deg = c["extra"]["roles"], c["extra"]["degrees"]
            assert list(deg[:6]) == list(st.DEGREES) and deg[6] > 1024
            for l, d in zip(roles, deg):                   # a failure above names the worst block; this names every degree
                print(f"STAGE_DEG degree {d} (landmark {l}): " + ", ".join(
                    f"{k} {st.err(np.asarray(got[k])[l][None], np.asarray(E[k])[l][None])[0]:.2e}" for k in ("vinv", "g_l", "dP")))
        if name == "masks":
            off = ~E["cused"]
            assert off[5] and not E["lused"][7]
            rows = np.repeat(off, cd)
            assert not c["X"][rows].any()                   # as the PCG's vectors: 0 where the right-hand side is 0
            for k in ("SX", "MX_jacobi", "MX_blocks", "MX_two_level"):
                assert not np.asarray(got[k])[rows].any(), k
            assert not got["b"].reshape(-1)[rows].any()
            assert got["rot1"][:, np.repeat(off, 3)].tobytes() == np.asfortranarray(rot)[:, np.repeat(off, 3)].tobytes()
            assert got["t1"][:, off].tobytes() == np.asfortranarray(t)[:, off].tobytes()
            assert got["p1"][:, ~E["lused"]].tobytes() == np.asfortranarray(P)[:, ~E["lused"]].tobytes()
            assert not got["dP"][~E["lused"]].any()
        if c["nid"]:
            # an unsymmetric preconditioner breaks PCG silently: on the identity columns X^T (M^-1 X) is M^-1 restricted to their rows
            rows = np.nonzero(c["X"][:, :c["nid"]])[0][np.argsort(np.nonzero(c["X"][:, :c["nid"]])[1])]
            for kind in st.KINDS:
                sub = np.asarray(got["MX_" + kind])[rows, :c["nid"]]
                asym = float((np.abs(sub - sub.T).max(axis=0) / np.abs(sub).max(axis=0)).max())
                print(f"STAGE_SYM {name} {kind}: asymmetry {asym:.3e} bound {2 * st.bound(e_ref['MX_' + kind]):.3e}")
                assert asym <= 2 * st.bound(e_ref["MX_" + kind])      # both entries of a pair within the bound of the exact, symmetric M^-1
        if name == "one_centre":
            assert len(E["dropped"]) == 1
        if name == "clamp":                                # from the reference: diagonals of J_P^T J_P on both sides of 1e-6
            d = E["_E"].V[:, np.arange(3), np.arange(3)][E["lused"]]
            assert (d < 1e-6).any() and (d.min(axis=1) > 1e-6).any()
        if name == "loss_huber":                           # the two observations built at the kink
            assert [s for _, s in c["extra"]["edge"]] == [c["a"] * c["a"], np.nextafter(c["a"] * c["a"], np.inf)]
        if name == "step" and not fix:
            R1 = np.stack([got["rot1"][:, 3 * i:3 * i + 3] for i in range(n)])
            assert float(np.abs(np.einsum("iab,icb->iac", R1, R1) - np.eye(3)).max()) <= 64 * st.EPS
    ctx.close()


@FIX
@pytest.mark.parametrize("name", ["base", "degrees", "agg33"])
def test_outputs_are_consistent_with_each_other(xmamd, name, fix):
    """without a reference (a layout slip that a shared misunderstanding would hide): Sdense X = SX; sinv_i S_ii = I; P^T (S P) through SX =
    Ac; cost = 1/2 sum of the reprojection errors; two calls give the same bytes.  Each side of an equation is within its bound of the exact
    value (the test above), so two sides differ by at most twice that bound."""
    c = st.case(name, fix)
    S, cd, n = c["S"], 3 if fix else 6, c["S"]["n"]
    nc = 4 if fix else 7
    rot, t, P = c["point"]
    mu = c["mus"][0]
    kw = st.stage_args(c, mu)
    E = st.exact_stages(S, **kw)
    e_ref = st.reference_errors(S, E, ("SX", "sinv", "Ac", "S"), **kw)
    ctx = _ctx(xmamd, S)
    got = _probe_all(ctx, c, mu)
    again = _probe_all(ctx, c, mu)
    for k, v in got.items():
        assert (v.tobytes() == again[k].tobytes()) if isinstance(v, np.ndarray) else (v == again[k] or (v != v and again[k] != again[k])), k
    L = got["S"]
    assert not np.triu(L, cd).any()                         # nothing above the block diagonal
    blockdiag = np.kron(np.eye(n), np.ones((cd, cd))) > 0
    full = L + np.where(blockdiag, 0.0, L).T
    assert np.where(blockdiag, L, 0.0)[np.triu_indices(cd * n, 1)].any()                   # the diagonal blocks are stored whole
    e, blk = st.err(st.shape_blocks("SX", full @ c["X"], n, S["m"], cd), st.shape_blocks("SX", got["SX"], n, S["m"], cd))
    print(f"STAGE_CONS {name} Sdense X vs SX: {e:.3e} (camera {blk})")
    assert e <= 2 * max(st.bound(e_ref["SX"]), st.bound(e_ref["S"]))
    for i in range(n):
        Sii, Bi = full[cd * i:cd * i + cd, cd * i:cd * i + cd], got["sinv"][i]
        # |(B + dB)(S + dS) - I| <= (e_B + e_S) |B| |S| cd entrywise, with each relative error within its bound
        tol = (st.bound(e_ref["sinv"]) + st.bound(e_ref["S"])) * cd * np.abs(Bi).max() * np.abs(Sii).max()
        assert np.abs(Bi @ Sii - np.eye(cd)).max() <= tol, i
    ncoarse = got["ncoarse"]
    Pfull = np.zeros((cd * n, nc * ncoarse))
    for a, (k0, k1) in enumerate(st.bp.coarse_ranges(len(c["order"]))):
        for i in c["order"][k0:k1]:
            Pfull[cd * i:cd * i + cd, nc * a:nc * a + nc] = got["Pm"][cd * i:cd * i + cd]
    g2 = ctx.ba_probe(rot, t, P, mu, fix_rotations=fix, X=Pfull)
    PSP = st.lower_blocks(Pfull.T @ g2["SX"], nc)
    for q in np.nonzero(got["dropped"])[0]:
        PSP[q, q] += 1.0
    e, blk = st.err(PSP.T, got["Ac"].T)
    print(f"STAGE_CONS {name} P^T (S P) vs Ac: {e:.3e} (column {blk})")
    assert e <= 2 * st.bound(e_ref["Ac"])
    sq = ctx.reprojection_errors(rot, t, P)
    assert (sq[sq >= 0] >= 0).all() and (sq >= 0).sum() == got["n_used"]
    assert abs(got["cost"] - 0.5 * sq[sq >= 0].sum()) <= 64 * st.EPS * got["cost"]
    ctx.close()


def _raw(xmamd, ctx, n, m, mu=1.0, flags=0, nan=False, struct_size=None, dense=False, loss=0, loss_scale=0.0):
    q = xmamd.BaProbe()
    q.struct_size = C.sizeof(q) if struct_size is None else struct_size
    q.mu, q.flags, q.loss, q.loss_scale = mu, flags, loss, loss_scale
    rot = np.asfortranarray(np.tile(np.eye(3), (1, n))); t = np.zeros((3, n), order="F"); P = np.zeros((3, max(m, 1)), order="F")
    P[2] = 10.0
    if nan:
        P[0, 0] = np.nan
    cd = 3 if flags & xmamd.BA_FIX_ROTATIONS else 6
    Sd = np.zeros((cd * n, cd * n), order="F") if dense else None
    if dense:
        q.Sdense = Sd.ctypes.data_as(C.c_void_p)
    return xmamd.lib().xm_ctx_ba_probe(ctx.h, rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p), C.byref(q))


def test_refusals_leave_contexts_usable_and_the_solver_state_untouched(xmamd):
    ERR_ARG = -2
    V = tl.gen_vg(40, deg=6, sigma=0.05, seed=80)
    e, _ = tl.gen_vg_edges(40, 6, 81)
    Mv = np.tile(np.eye(3).reshape(1, 9), (e.shape[0], 1))
    ctxs = [xmamd.Context(Q=V["Q"]), xmamd.Context(bsr=(V["rowptr"], V["colidx"], V["blocks"])),
            xmamd.Context(vg=(e[:, 0].astype(np.int32), e[:, 1].astype(np.int32), np.ones(e.shape[0]), Mv), n=40)]
    for c in ctxs:
        assert _raw(xmamd, c, c.n, 1) == ERR_ARG
        assert "XM_STORAGE_SCHUR" in xmamd.lib().xm_last_error().decode()
        _, _, info = c.solve(5, 1e-8, 0.0)
        assert info["status"] == 1
        c.close()
    S = ba.ring_scene(n_cams=12, n_pts=80, seed=82, noise=1e-3)
    two = _ctx(xmamd, S, n_gpus=2, gpu_map=1)
    assert _raw(xmamd, two, S["n"], S["m"]) == ERR_ARG
    _, _, i2 = two.solve(5, 1e-8, 0.0)
    two.close()
    a, b = _ctx(xmamd, S), _ctx(xmamd, S)
    a.solve(5, 1e-8, 0.0); b.solve(5, 1e-8, 0.0)
    both = xmamd.BA_PRECOND_TWO_LEVEL | xmamd.BA_PRECOND_BLOCKS
    for kw in (dict(struct_size=8), dict(nan=True), dict(mu=0.0), dict(mu=-1.0), dict(mu=float("inf")), dict(flags=both), dict(flags=xmamd.BA_DENSE_SCHUR),
               dict(loss=9), dict(loss=1, loss_scale=0.0), dict(loss_scale=1.0)):
        assert _raw(xmamd, a, S["n"], S["m"], **kw) == ERR_ARG, kw
    assert _raw(xmamd, a, S["n"], S["m"]) == 0 and _raw(xmamd, a, S["n"], S["m"], dense=True) == 0
    rot0, t0, P0 = ba.perturb(S["rot"], S["t"], S["P"], seed=83)
    a.ba_probe(rot0, t0, P0, 1e-4, preconditioner="two_level", X=np.eye(6 * S["n"])[:, :3], dc=np.zeros(6 * S["n"]), dense=True)
    Ra, sa, ia = a.solve(5, 1e-8, 0.0)                     # the probed context against one that was never probed: the same bits
    Rb, sb, ib = b.solve(5, 1e-8, 0.0)
    a.close(); b.close()
    assert Ra.tobytes() == Rb.tobytes() and sa.tobytes() == sb.tobytes() and ia["primal"] == ib["primal"] and ia["status"] == i2["status"] == 1
    # Sdense above its row limit: 6 n > XM_BA_PROBE_DENSE_MAX_ROWS
    big = ba.ring_scene(n_cams=xmamd.BA_PROBE_DENSE_MAX_ROWS // 6 + 1, n_pts=300, seed=84, frac=0.05)
    ctx = _ctx(xmamd, big)
    assert _raw(xmamd, ctx, big["n"], big["m"], dense=True) == ERR_ARG and "XM_BA_PROBE_DENSE_MAX_ROWS" in xmamd.lib().xm_last_error().decode()
    assert _raw(xmamd, ctx, big["n"], big["m"], dense=True, flags=xmamd.BA_FIX_ROTATIONS) == 0      # 3 n rows fit
    assert _raw(xmamd, ctx, big["n"], big["m"]) == 0
    ctx.close()
