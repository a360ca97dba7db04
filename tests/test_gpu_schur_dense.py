"""The dense Q (and Abar) of the reference's create_matrix built on the device from the observation list (xm_tuning_t.schur_dense_q,
xm_ctx_dense_q, xm_create_matrix; xm-code_amd/csrc/xm_schur_dense.hip).

Bounds: 1e-11 relative Frobenius against the golden Q.bin (the bound of test_matrix_free_product_equals_dense_Q: tl.schur_dense of obs.npz
itself sits 1.6e-13 from that file), 1e-10 against the numpy restatements (test_matrix_free_device_assembly_equals_host_assembly), 1e-9 for
the product of the window-edge scene (test_matrix_free_venice_size_scene) and for the recovered translations / landmarks
(test_matrix_free_recover_translations_and_landmarks), 1e-6 for rotations (north_star).

The numpy restatements divide by Q3, so for weights that empty a landmark the reference is taken on the SAME list without its
zero-weight observations and with the landmarks renumbered (the same matrix: such observations and landmarks contribute nothing)."""
import functools
import json
import os

import numpy as np
import pytest

import xm_testlib as tl

pytestmark = pytest.mark.gpu
G = tl.GOLDEN
DQ = dict(schur_dense_q=1)


@functools.lru_cache(maxsize=None)
def _simple2():
    d = os.path.join(G, "simple2")
    Z = np.load(os.path.join(d, "obs.npz"))
    Q = tl.load_bin(os.path.join(d, "Q.bin"))
    Q.setflags(write=False)
    return (Z["cam"], Z["lm"], Z["p"], Z["w"].reshape(-1)), Q, json.load(open(os.path.join(d, "expected.json"))), d


@functools.lru_cache(maxsize=None)
def _hub_scene():
    """300 cameras, 4000 landmarks + three hub landmarks of degree 300 (heavy: more than 64 observations), every 11th weight 0"""
    S = tl.gen_scene(300, 4000, 6, seed=9)
    w = S["w"].copy(); w[::11] = 0.0
    return S["cam"], S["lm"], S["p"], w


def _live(cam, lm, p, w):
    """the list without its zero-weight observations, landmarks renumbered compactly (every camera must keep an observation)"""
    k = w != 0.0
    assert np.unique(cam[k]).size == int(cam.max()) + 1
    _, l2 = np.unique(lm[k], return_inverse=True)
    return cam[k], l2, p[k], w[k]


@functools.lru_cache(maxsize=None)
def _hub_refs():
    """(tl.schur_dense, Abar = -Qtp_bar^-1 Vtp_bar^T) of the hub scene; Abar by the statements of tl.schur_dense"""
    cam, lm, p, w = _hub_scene()
    Q = tl.schur_dense(cam, lm, p, w)
    N, M, Q1, c, Q2, Q3 = tl.schur_parts(cam, lm, p, w)
    Vtp = np.zeros((3 * N, N + M))
    for i in range(N):
        Vtp[3 * i:3 * i + 3, i] = c[i]
    np.add.at(Vtp, (3 * cam[:, None] + np.arange(3)[None, :], N + lm[:, None]), -(w[:, None] * p))
    Qtp = np.zeros((N + M, N + M))
    Qtp[np.arange(N), np.arange(N)] = Q2
    Qtp[N + np.arange(M), N + np.arange(M)] = Q3
    np.add.at(Qtp, (cam, N + lm), -w); np.add.at(Qtp, (N + lm, cam), -w)
    A = -np.linalg.solve(Qtp[1:, 1:], Vtp[:, 1:].T)
    Q.setflags(write=False); A.setflags(write=False)
    return Q, A


def test_simple2_dense_q_equals_golden_and_is_symmetric_bit_for_bit(xmamd):
    obs, Qg, _, _ = _simple2()
    ctx = xmamd.Context(obs=obs, tuning=DQ)
    Q = ctx.dense_q()
    kinds = ctx.product_kind(3), ctx.product_kind(8)
    ctx.close()
    err = tl.rel_fro(Q, Qg)
    print(f"SIMPLE2 dense Q vs golden Q.bin: {err:.3e}")
    assert err < 1e-11
    assert np.array_equal(Q, Q.T)
    assert kinds == ("dense", "dense")            # 279 rows: below the size of the symmetric sweep, and not the factor chain
    c2 = xmamd.Context(obs=obs, tuning=DQ)
    Q2 = c2.dense_q()
    c2.close()
    assert np.array_equal(Q, Q2)                  # a second build gives the same bits
    plain = xmamd.Context(obs=obs)
    with pytest.raises(xmamd.XmError):
        plain.dense_q()                           # a context without the tuning field holds no dense Q
    assert plain.product_kind(3) == "schur"
    plain.close()


def test_heavy_landmarks_and_zero_weights(xmamd):
    cam, lm, p, w = _hub_scene()
    Qref, _ = _hub_refs()
    ctx = xmamd.Context(obs=(cam, lm, p, w), tuning=DQ)
    Q = ctx.dense_q()
    err = tl.rel_fro(Q, Qref)
    print(f"hub scene dense Q vs tl.schur_dense: {err:.3e}")
    assert err < 1e-10 and np.array_equal(Q, Q.T)
    for o in (1, 3, 4, 5, 8):
        W = np.random.default_rng(o).standard_normal((900, o))
        e = tl.rel_fro(ctx.qw(W), tl.schur_qw_numpy(cam, lm, p, w, W))
        print(f"  qw o = {o}: {e:.3e}")
        assert e < 1e-10
    # every observation of five non-hub landmarks gets weight 0: 1 / Q3 = 0 for them
    w2 = w.copy()
    for l in (3, 700, 1234, 2500, 3999):
        assert np.count_nonzero(lm == l) <= 64
        w2[lm == l] = 0.0
    ctx.set_edge_weights(w2)
    Q2 = ctx.dense_q()
    live = _live(cam, lm, p, w2)
    e2 = tl.rel_fro(Q2, tl.schur_dense(*live))
    print(f"hub scene, five landmarks emptied: {e2:.3e}")
    assert e2 < 1e-10 and np.array_equal(Q2, Q2.T)
    for o in (1, 3, 4, 5, 8):
        W = np.random.default_rng(10 + o).standard_normal((900, o))
        assert tl.rel_fro(ctx.qw(W), tl.schur_qw_numpy(*live, W)) < 1e-10
    ctx.close()


@pytest.mark.parametrize("N", [2, 21, 22, 43, 86])
def test_tile_edges(xmamd, N):
    """3N = 6, 63, 66, 129, 258: around the 64-row tiles of the GEMMs and of the finishing kernel (N = 86: the hub landmarks are heavy)"""
    S = tl.gen_scene(N, 200, 4, seed=1)
    obs = (S["cam"], S["lm"], S["p"], S["w"])
    ctx = xmamd.Context(obs=obs, tuning=DQ)
    Q = ctx.dense_q()
    ctx.close()
    err = tl.rel_fro(Q, tl.schur_dense(*obs))
    print(f"N = {N}: {err:.3e}")
    assert err < 1e-10 and np.array_equal(Q, Q.T)


def test_lds_column_window_edge(xmamd):
    """3N exceeds the assembly kernel's LDS column window (kSchurDenseQWinCams cameras) by 63 rows, less than one 64-row tile: the second
    window holds 21 cameras"""
    win, _, _ = xmamd.schur_dense_limits()
    N = win + 21
    assert 0 < 3 * N - 3 * win < 64
    S = tl.gen_scene(N, 3000, 6, seed=4)
    obs = (S["cam"], S["lm"], S["p"], S["w"])
    ctx = xmamd.Context(obs=obs, tuning=DQ)
    W = np.random.default_rng(0).standard_normal((3 * N, 3))
    Y = ctx.qw(W)
    Q = ctx.dense_q()
    ctx.close()
    err = tl.rel_fro(Y, tl.schur_qw_numpy(*obs, W))
    print(f"window edge N = {N}: {err:.3e}")
    assert err < 1e-9
    assert np.array_equal(Q, Q.T)


def test_solve_on_the_dense_q_matches_the_dense_solve(xmamd):
    obs, Qg, exp, d = _simple2()
    args = (exp["max_rank"], exp["tol"], exp["lam"])
    Rd, sd, idn = xmamd.solve_dense(Qg, *args)
    gold = np.load(os.path.join(d, "rot_anchor.npy"))

    def run(tuning):
        ctx = xmamd.Context(obs=obs, tuning=tuning)
        out = ctx.solve(*args)
        ctx.close()
        return out

    R, s, info = run(DQ)
    assert info["rank"] == idn["rank"] == exp["rank"] and info["status"] == idn["status"] == 1
    assert tl.rotation_parity(R, s, Rd, sd) < 1e-6
    rot, _, _ = xmamd.recover_rotations(R, s)
    assert tl.rel_fro(rot, gold) < 1e-6
    assert info["sym_product"] == 0 and info["qw_bytes"] >= 8 * 279 * 279       # the dense path is what the result reports
    Rs, ss, isym = run(dict(schur_dense_q=1, sym_min_rows=1))
    assert isym["sym_product"] == 1 and isym["rank"] == exp["rank"] and isym["status"] == 1
    assert tl.rotation_parity(Rs, ss, Rd, sd) < 1e-6
    cdo = xmamd.Context(obs=obs, tuning=DQ)                   # the outer iteration on the device, as for any dense context that asks for it
    Ro, so, ido = cdo.solve(*args, flags=xmamd.FLAG_DEVICE_OUTER)
    cdo.close()
    assert ido["outer_on_device"] >= 1 and ido["rank"] == exp["rank"] and ido["status"] == 1 and tl.rotation_parity(Ro, so, Rd, sd) < 1e-6
    Rf, sf, i32 = run(dict(schur_dense_q=1, hess_f32=1))
    assert i32["hess_f32"] == 1 and i32["rank"] == exp["rank"] and i32["status"] == 1
    rot32, _, _ = xmamd.recover_rotations(Rf, sf)
    assert tl.rel_fro(rot32, rot) < 1e-6
    with pytest.raises(xmamd.XmError, match="hess_f32"):
        xmamd.Context(obs=obs, tuning=dict(hess_f32=1))                          # without schur_dense_q it stays refused


def test_reweighting_rebuilds_q_on_the_device(xmamd):
    obs, _, _, d = _simple2()
    tp = np.load(os.path.join(d, "tp.npz"))
    ctx = xmamd.Context(obs=obs, tuning=DQ)
    mf = xmamd.Context(obs=obs)
    for c in (ctx, mf):   # edge_residuals reads the end point of the context's OWN solve: each against the numpy chain at that point
        R, s, _ = c.solve(5, 1e-6, 0.0)
        ref = tl.schur_residuals_numpy(*obs, tl.scale_rows(R, s))
        assert np.abs(c.edge_residuals() - ref).max() < 1e-9 * ref.max()
    thr, removed, w_new = ctx.xm2_filter(tp["R_real"], tp["s_real"], 90.0)
    thr0, removed0, w0 = mf.xm2_filter(tp["R_real"], tp["s_real"], 90.0)
    assert thr == thr0 and removed == removed0 and np.array_equal(w_new, w0)
    Q = ctx.dense_q()
    err = tl.rel_fro(Q, tl.schur_dense(*_live(obs[0], obs[1], obs[2], w_new)))
    print(f"SIMPLE2 after xm2_filter: {err:.3e}")
    assert err < 1e-10 and np.array_equal(Q, Q.T)
    fresh = xmamd.Context(obs=(obs[0], obs[1], obs[2], w_new), tuning=DQ)
    assert np.array_equal(Q, fresh.dense_q())
    fresh.close()
    # the lists behind the dense Q are the matrix-free context's: same arrays from the calls that read them
    a, b = ctx.clean_observations(), mf.clean_observations()
    assert np.array_equal(a.keep, b.keep) and np.array_equal(a.cam_index, b.cam_index) and np.array_equal(a.lm_index, b.lm_index)
    ta, pa = ctx.recover_tp(tp["R_real"], tp["s_real"])
    tb, pb = mf.recover_tp(tp["R_real"], tp["s_real"])
    assert np.array_equal(ta, tb) and np.array_equal(pa, pb)
    assert np.array_equal(ctx.edge_residuals_recovered(tp["R_real"], tp["s_real"]), mf.edge_residuals_recovered(tp["R_real"], tp["s_real"]))
    ctx.close(); mf.close()


def test_create_matrix_writes_the_reference_files(xmamd, tmp_path, monkeypatch):
    obs, Qg, exp, d = _simple2()
    cam, lm, p, w = obs
    edges = np.stack([cam.astype(np.int64) + 1, lm.astype(np.int64) + 1], axis=1)          # the reference's 1-based edges
    xmamd.create_matrix(w, edges, p, str(tmp_path))
    Q = tl.load_bin(tmp_path / "Q.bin"); A = tl.load_bin(tmp_path / "Abar.bin")
    N, M = int(cam.max()) + 1, int(lm.max()) + 1
    assert Q.shape == (3 * N, 3 * N) and A.shape == (N - 1 + M, 3 * N)
    err = tl.rel_fro(Q, Qg)
    print(f"create_matrix Q.bin vs golden: {err:.3e}")
    assert err < 1e-11 and np.array_equal(Q, Q.T)
    T = np.load(os.path.join(d, "tp.npz"))
    U = np.concatenate([(T["s_real"][i] * T["R_real"][:, 3 * i:3 * i + 3]).T for i in range(N)], axis=0)      # (s R)^T: 3N x 3
    X = A @ U
    t = np.concatenate([np.zeros((3, 1)), X[:N - 1].T], axis=1); P = X[N - 1:].T
    st, sp = np.abs(T["t_est"]).max(), np.abs(T["p_est"]).max()
    print(f"Abar (sR)^T vs tp.npz: t {np.abs(t - T['t_est']).max() / st:.3e}, p {np.abs(P - T['p_est']).max() / sp:.3e}")
    assert np.abs(t - T["t_est"]).max() < 1e-9 * st and np.abs(P - T["p_est"]).max() < 1e-9 * sp
    # abar=False skips the second file
    os.makedirs(tmp_path / "q_only")
    xmamd.create_matrix(w, edges, p, str(tmp_path / "q_only"), abar=False)
    assert os.path.exists(tmp_path / "q_only" / "Q.bin") and not os.path.exists(tmp_path / "q_only" / "Abar.bin")
    assert np.array_equal(tl.load_bin(tmp_path / "q_only" / "Q.bin"), Q)
    # the reference's file-based solve on the directory create_matrix filled
    monkeypatch.setenv("XM_QUIET", "1")
    XM = xmamd.import_XM()
    XM.solve(str(tmp_path), exp["max_rank"], exp["tol"], exp["lam"], 1000)
    assert tl.load_bin(tmp_path / "R.bin").shape == (3 * N, exp["rank"])


def test_abar_against_numpy_over_several_landmark_panels(xmamd):
    cam, lm, p, w = _hub_scene()
    Qref, Aref = _hub_refs()
    _, panel, _ = xmamd.schur_dense_limits()
    assert int(lm.max()) + 1 > panel                       # more than one panel of landmark rows
    Q, A = xmamd.create_matrix_arrays(cam, lm, p, w)
    ea, eq = tl.rel_fro(A, Aref), tl.rel_fro(Q, Qref)
    print(f"hub scene Abar vs numpy: {ea:.3e} (camera rows {tl.rel_fro(A[:299], Aref[:299]):.3e}), Q {eq:.3e}")
    assert ea < 1e-10 and tl.rel_fro(A[:299], Aref[:299]) < 1e-10 and eq < 1e-10


def test_refusals(xmamd):
    S = tl.gen_scene(40, 400, 5, seed=12)
    obs = (S["cam"], S["lm"], S["p"], S["w"])
    for solver in (2, 3):                                   # the CG forms hold no inverse of the reduced camera Laplacian
        with pytest.raises(xmamd.XmError, match="schur_dense_q"):
            xmamd.Context(obs=obs, tuning=dict(schur_dense_q=1, schur_solver=solver))
    with pytest.raises(xmamd.XmError, match="schur_dense_q"):
        xmamd.Context(obs=obs, n_gpus=2, gpu_map=1, tuning=DQ)
    name = b"/xm_test_schur_dense_%d" % os.getpid()
    xmamd._chk(xmamd.lib().xm_comm_init_shm(0, 1, 0, name, 1 << 20))       # a (single-rank) communicator is the process default
    try:
        with pytest.raises(xmamd.XmError, match="schur_dense_q"):
            xmamd.Context(obs=obs, tuning=DQ)
    finally:
        xmamd.lib().xm_comm_finalize()
    _, _, cap = xmamd.schur_dense_limits()
    assert cap == 20000
    with pytest.raises(xmamd.XmError, match="schur_dense_q"):
        xmamd.Context(obs=obs, n=cap + 1, tuning=DQ)
    dup = (np.concatenate([obs[0], obs[0][5:6]]), np.concatenate([obs[1], obs[1][5:6]]), np.concatenate([obs[2], obs[2][5:6] + 0.01]),
           np.concatenate([obs[3], [0.7]]))
    with pytest.raises(xmamd.XmError, match="twice"):
        xmamd.Context(obs=dup, tuning=DQ)
    with pytest.raises(xmamd.XmError, match="twice"):
        xmamd.create_matrix_arrays(*dup, abar=False)
    with pytest.raises(xmamd.XmError, match="schur_dense_q"):
        xmamd.Context(obs=obs, tuning=dict(schur_dense_q=2))
    # nothing is left behind: the plain matrix-free context on the same list (and on the list with the pair named twice) still works
    W = np.random.default_rng(1).standard_normal((120, 3))
    for o in (obs, dup):
        c = xmamd.Context(obs=o, tuning=dict(schur_dense_q=0))
        assert c.product_kind(3) == "schur"
        assert tl.rel_fro(c.qw(W), tl.schur_qw_numpy(*o, W)) < 1e-10
        c.close()
