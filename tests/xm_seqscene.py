"""Sequential-capture scenes for the matrix-free tests of the two-level preconditioner (xm_tuning_t.schur_solver = 3).

A camera trajectory where every landmark is seen by a few consecutive frames, as video and SLAM-style front ends produce: the reduced camera
Laplacian is then close to a path Laplacian, the case where the Jacobi-preconditioned CG needs O(N) iterations.  No hub landmarks
(xm_testlib.gen_scene adds landmarks seen by every camera, which make the co-visibility graph an expander)."""
import numpy as np

import xm_testlib as tl


def gen_sequential(N, per_cam=20, span=(2, 5), loops=0, seed=0, noise=0.01, heavy=0, heavy_views=80):
    """N cameras along a smooth trajectory; camera i starts `per_cam` landmarks, each seen by cameras i .. i+k-1 with k drawn from `span`
    (inclusive, clipped at the last camera).  `loops`: loop closures -- a pair of distant cameras (i, j) that see 4 common landmarks each
    with their successors.  `heavy`: landmarks seen by `heavy_views` consecutive cameras (more than 64: the heavy path of the set-up).
    Returns dict(cam, lm, p, w, R_star, n, m) like xm_testlib.gen_scene: p = R_i^T (P_l - t_i) + noise."""
    rng = np.random.default_rng(seed)
    s = np.arange(N, dtype=np.float64)
    ts = np.stack([0.5 * s, 3.0 * np.sin(0.05 * s), 2.0 * np.cos(0.03 * s)], axis=1)
    Rs = tl.haar_so3(rng, N)
    cams, lms, anchor = [], [], []
    m = 0
    for i in range(N):
        for _ in range(per_cam):
            k = int(rng.integers(span[0], span[1] + 1))
            seen = np.arange(i, min(N, i + k))
            if seen.size < 2:
                seen = np.arange(max(0, N - 2), N)
            cams.append(seen); lms.append(np.full(seen.size, m)); anchor.append(i)
            m += 1
    for _ in range(loops):
        i = int(rng.integers(0, N // 3)); j = int(rng.integers(2 * N // 3, N - 1))
        for _ in range(4):
            seen = np.array([i, i + 1, j, j + 1])
            cams.append(seen); lms.append(np.full(4, m)); anchor.append(i)
            m += 1
    for _ in range(heavy):
        i = int(rng.integers(0, max(1, N - heavy_views)))
        seen = np.arange(i, min(N, i + heavy_views))
        cams.append(seen); lms.append(np.full(seen.size, m)); anchor.append(i)
        m += 1
    cam = np.concatenate(cams).astype(np.int32)
    lm = np.concatenate(lms).astype(np.int32)
    anchor = np.asarray(anchor)
    P = ts[anchor] + rng.uniform(-3.0, 3.0, (m, 3))
    pts = np.einsum("eba,eb->ea", Rs[cam], P[lm] - ts[cam]) + noise * rng.standard_normal((cam.size, 3))
    w = rng.uniform(0.5, 1.5, cam.size)
    return dict(cam=cam, lm=lm, p=pts, w=w, R_star=Rs, n=N, m=m)


def renumber(S, seed=0):
    """the same scene with cameras 1..N-1 permuted (camera 0, the anchor, stays): (scene, pi) with new index pi[old]"""
    rng = np.random.default_rng(seed)
    N = S["n"]
    pi = np.concatenate([[0], 1 + rng.permutation(N - 1)]).astype(np.int32)
    R = np.empty_like(S["R_star"])
    R[pi] = S["R_star"]
    return dict(S, cam=pi[S["cam"]].astype(np.int32), R_star=R), pi


def permute_rows(X, pi):
    """camera rows (3 per camera) of X moved to the permuted numbering: out[3 pi[i] + a] = X[3 i + a]"""
    N = pi.size
    out = np.empty_like(X)
    out.reshape(N, 3, -1)[pi] = X.reshape(N, 3, -1)
    return out
