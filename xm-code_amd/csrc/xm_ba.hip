// xm_ba.hip — reprojection bundle adjustment on the lists of the matrix-free storage (design: xm_ba.h).  CD = 6 (rotation vector +
// translation per camera) or 3 (XM_BA_FIX_ROTATIONS: translation only); with XM_BA_REFINE_FOCAL one focal scale more, the last column
// of the camera block: CD = 7 or 4; with XM_BA_REFINE_RADIAL a radial coefficient behind it: CD = 8 or 5.
#include "xm_ba.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "xm_device.h"
#include "xm_lm_loop.h"
#include "xm_lm_shared.h"
#include "xm_schur.h"
#include "xm_stage.h"

namespace xm {

namespace {

// per-observation record, one plane of `stride` doubles per entry: J_c (2 x CD, row-major), J_P (2 x 3), r (2)
template <int CD> constexpr int ba_planes() { return 2 * CD + 8; }
template <int CD> constexpr int ba_jp() { return 2 * CD; }
template <int CD> constexpr int ba_res() { return 2 * CD + 6; }

// the camera block's columns: (dtheta, dt), (dt), (dtheta, dt, dg), (dt, dg), (dtheta, dt, dg, dk), (dt, dg, dk)
template <int CD> constexpr bool ba_has_rot() { return CD >= 6; }
template <int CD> constexpr bool ba_has_dist() { return CD == 8 || CD == 5; }
template <int CD> constexpr bool ba_has_focal() { return CD == 7 || CD == 4 || ba_has_dist<CD>(); }
template <int CD> constexpr bool ba_can_group() { return CD == 7 || CD == 4; }   // the focal groups' kernels: the focal-only blocks
template <int CD> constexpr int ba_toff() { return ba_has_rot<CD>() ? 3 : 0; }   // first translation column
template <int CD> constexpr int ba_fidx() { return ba_has_dist<CD>() ? CD - 2 : CD - 1; }   // the focal column (where there is one)
template <int CD> constexpr int ba_kidx() { return CD - 1; }                       // the distortion column (where there is one): the last

__device__ __forceinline__ bool obs_used(const double (&v)[6]) { return v[0] != 0.0 || v[1] != 0.0 || v[2] != 0.0; }   // J_P row 0 (never 0 when used)

// Y = Rcw P, X = Y + tcw: the camera-frame point of an observation.  The eval and cost bodies write the same expression out: called from
// them, this function changes the order of their vector instructions (profiles/r40_ba_one_kernel_per_stage.txt)
__device__ __forceinline__ void ba_point(const double *R, const double *T, const double *X3, double (&Y)[3], double (&X)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        Y[a] = R[3 * a] * X3[0] + R[3 * a + 1] * X3[1] + R[3 * a + 2] * X3[2];
        X[a] = Y[a] + T[a];
    }
}

// ---- residuals and Jacobians at (Rcw, tcw, P), written in both list orders (scaled by sqrt(rho') under a robust loss); partial sums of
// the cost 1/2 sum rho(|r|^2) and of the used observations
// (G, gfree: the focal scales of the parameter set and the mask of the free ones (null: all), read only where the camera block has a focal
// column and null elsewhere: r = g pi(X) - z, J_pose and J_P times g, d r / d g = pi(X) or 0.  scale: the loss scale a, not read under
// XM_BA_LOSS_TRIVIAL)
// The eval, cost and camera-candidate kernels each forward to a __forceinline__ body whose pointer parameters are __restrict__: with the
// body written into the kernel the __restrict__ of the kernel's own parameters alone gives other instruction streams and register counts
// (profiles/r40_ba_one_kernel_per_stage.txt), so the bodies stay functions.
template <int CD, int LOSS>
__device__ __forceinline__ void ba_eval_body(const SchurLists &S, const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                             const double *__restrict__ P, const double *__restrict__ G, const uint8_t *__restrict__ gfree,
                                             const double *__restrict__ Kd, const uint8_t *__restrict__ kfree,
                                             double *__restrict__ Jc, double *__restrict__ Jl, double *__restrict__ parts, double scale) {
    constexpr int NP = ba_planes<CD>(), JP = ba_jp<CD>(), RS = ba_res<CD>();
    __shared__ double sh[4];
    double cost = 0.0, used = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * 256) {
        const int64_t pc = S.pos_c[e], pl = S.dpos_l[e];
        const double w = S.cam_w[pc], q0 = S.obs_p[3 * e], q1 = S.obs_p[3 * e + 1], q2 = S.obs_p[3 * e + 2];
        double v[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) v[k] = 0.0;
        if (w > 0.0 && q2 > 0.0) {
            const double *R = Rcw + (size_t)9 * S.obs_cam[e], *T = tcw + (size_t)3 * S.obs_cam[e], *X3 = P + (size_t)3 * S.obs_lm[e];
            double Y[3], X[3];
            if constexpr (ba_has_dist<CD>() && ba_has_rot<CD>()) {
                // With k = 0 held this block is the focal form's and its records are to be that form's bytes.  Which two of the three
                // products of a row of R X3 the compiler fuses is its choice per instantiation: at CD = 7 it takes row 0 the other way
                // round than rows 1 and 2 (and than every row at CD = 4 / 5, which agree without help), and left alone it does not
                // here.  So the fused pairs of CD = 7 are written out (tests/test_gpu_ba_radial_stages.py, the k_zero case).
                Y[0] = fma(X3[2], R[2], fma(X3[1], R[1], X3[0] * R[0]));
                Y[1] = fma(X3[2], R[5], fma(X3[0], R[3], X3[1] * R[4]));
                Y[2] = fma(X3[2], R[8], fma(X3[0], R[6], X3[1] * R[7]));
#pragma unroll
                for (int a = 0; a < 3; ++a) X[a] = Y[a] + T[a];
            } else {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    Y[a] = R[3 * a] * X3[0] + R[3 * a + 1] * X3[1] + R[3 * a + 2] * X3[2];
                    X[a] = Y[a] + T[a];
                }
            }
            const double iz = 1.0 / X[2], u0 = X[0] / X[2], u1 = X[1] / X[2];
            const double d[2][3] = {{iz, 0.0, -u0 * iz}, {0.0, iz, -u1 * iz}};   // d pi / d X
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int k = 0; k < 3; ++k) v[JP + 3 * r + k] = d[r][0] * R[k] + d[r][1] * R[3 + k] + d[r][2] * R[6 + k];   // d pi / dX . Rcw
                if constexpr (ba_has_rot<CD>()) {   // X = Exp(th) Y + t: dX / dth = -[Y]x
                    v[CD * r + 0] = -d[r][1] * Y[2] + d[r][2] * Y[1];
                    v[CD * r + 1] = d[r][0] * Y[2] - d[r][2] * Y[0];
                    v[CD * r + 2] = -d[r][0] * Y[1] + d[r][1] * Y[0];
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) v[CD * r + ba_toff<CD>() + k] = d[r][k];
            }
            if constexpr (ba_has_dist<CD>()) {   // r = g s u - z, s = 1 + k |u|^2: d r / d u = g (s I + 2 k u u^T) in front of the pinhole rows
                const int64_t i = S.obs_cam[e];
                const double g = G[i], kd = Kd[i], rho2 = u0 * u0 + u1 * u1, s = 1.0 + kd * rho2;
                const double m00 = g * (s + 2.0 * kd * u0 * u0), m01 = g * (2.0 * kd * u0 * u1), m11 = g * (s + 2.0 * kd * u1 * u1);
#pragma unroll
                for (int k = 0; k < CD - 2; ++k) {   // the focal and distortion columns are still 0
                    const double a0 = v[k], a1 = v[CD + k];
                    v[k] = m00 * a0 + m01 * a1;
                    v[CD + k] = m01 * a0 + m11 * a1;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double a0 = v[JP + k], a1 = v[JP + 3 + k];
                    v[JP + k] = m00 * a0 + m01 * a1;
                    v[JP + 3 + k] = m01 * a0 + m11 * a1;
                }
                const bool fr = gfree == nullptr || gfree[i] != 0, kr = kfree == nullptr || kfree[i] != 0;
                v[ba_fidx<CD>()] = fr ? s * u0 : 0.0;
                v[CD + ba_fidx<CD>()] = fr ? s * u1 : 0.0;
                v[ba_kidx<CD>()] = kr ? g * rho2 * u0 : 0.0;
                v[CD + ba_kidx<CD>()] = kr ? g * rho2 * u1 : 0.0;
                v[RS] = g * s * u0 - q0 / q2;
                v[RS + 1] = g * s * u1 - q1 / q2;
            } else if constexpr (ba_has_focal<CD>()) {
                const int64_t i = S.obs_cam[e];
                const double g = G[i];
#pragma unroll
                for (int k = 0; k < RS; ++k) v[k] *= g;   // the focal column is still 0
                const bool fr = gfree == nullptr || gfree[i] != 0;
                v[ba_fidx<CD>()] = fr ? u0 : 0.0;
                v[CD + ba_fidx<CD>()] = fr ? u1 : 0.0;
                v[RS] = g * u0 - q0 / q2;
                v[RS + 1] = g * u1 - q1 / q2;
            } else {
                v[RS] = u0 - q0 / q2;
                v[RS + 1] = u1 - q1 / q2;
            }
            if constexpr (LOSS == XM_BA_LOSS_TRIVIAL) {
                cost += 0.5 * (v[RS] * v[RS] + v[RS + 1] * v[RS + 1]);
            } else {
                double rho1;
                cost += 0.5 * ba_rho<LOSS>(v[RS] * v[RS] + v[RS + 1] * v[RS + 1], scale, rho1);
                const double c = sqrt(rho1);
#pragma unroll
                for (int k = 0; k < NP; ++k) v[k] *= c;
            }
            used += 1.0;
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            Jc[(size_t)k * S.nobs + pc] = v[k];
            Jl[(size_t)k * S.lm_total + pl] = v[k];
        }
    }
    cost = block_sum256(cost, sh);
    used = block_sum256(used, sh);
    if (threadIdx.x == 0) { parts[blockIdx.x] = cost; parts[gridDim.x + blockIdx.x] = used; }
}
template <int CD, int LOSS>
__global__ __launch_bounds__(256) void ba_eval_kernel(SchurLists S, const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                      const double *__restrict__ P, const double *__restrict__ G,
                                                      const uint8_t *__restrict__ gfree, const double *__restrict__ Kd,
                                                      const uint8_t *__restrict__ kfree, double *__restrict__ Jc, double *__restrict__ Jl,
                                                      double *__restrict__ parts, double scale) {
    ba_eval_body<CD, LOSS>(S, Rcw, tcw, P, G, gfree, Kd, kfree, Jc, Jl, parts, scale);
}

// ---- landmark pass: V_l, g_l, (V_l + mu D_l)^-1 (6 entries of the symmetric inverse), used flag; per-workgroup max of |g_l|_inf
template <int CD>
__global__ __launch_bounds__(kBaHeavyThreads) void ba_lm_kernel(SchurLists S, const double *__restrict__ Jl, double mu, double *__restrict__ vinv,
                                                                double *__restrict__ gl, int32_t *__restrict__ lused, double *__restrict__ gpart) {
    constexpr int JP = ba_jp<CD>(), RS = ba_res<CD>();
    __shared__ double sh[kBaHeavyThreads / 64];
    const LmRange q = lm_range(S);
    double acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (int64_t e = q.e; e < q.e_end; e += q.step) {
        double j[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) j[k] = Jl[(size_t)(JP + k) * S.lm_total + e];
        const double r0 = Jl[(size_t)RS * S.lm_total + e], r1 = Jl[(size_t)(RS + 1) * S.lm_total + e];
        acc[0] += j[0] * j[0] + j[3] * j[3]; acc[1] += j[0] * j[1] + j[3] * j[4]; acc[2] += j[0] * j[2] + j[3] * j[5];
        acc[3] += j[1] * j[1] + j[4] * j[4]; acc[4] += j[1] * j[2] + j[4] * j[5]; acc[5] += j[2] * j[2] + j[5] * j[5];
        acc[6] += j[0] * r0 + j[3] * r1; acc[7] += j[1] * r0 + j[4] * r1; acc[8] += j[2] * r0 + j[5] * r1;
        acc[9] += obs_used(j) ? 1.0 : 0.0;
    }
    bool writer = q.active;
    if (q.heavy) writer = heavy_sum<10>(acc);
    double gabs = 0.0;
    if (writer) {
        const int64_t l = q.l;
        const double a00 = acc[0] + mu * clamp_diag(acc[0]), a11 = acc[3] + mu * clamp_diag(acc[3]), a22 = acc[5] + mu * clamp_diag(acc[5]);
        const double a01 = acc[1], a02 = acc[2], a12 = acc[4];
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double id = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
        double *vi = vinv + (size_t)6 * l;
        vi[0] = c00 * id; vi[1] = c01 * id; vi[2] = c02 * id; vi[3] = c11 * id; vi[4] = c12 * id; vi[5] = c22 * id;
        gl[3 * l] = acc[6]; gl[3 * l + 1] = acc[7]; gl[3 * l + 2] = acc[8];
        lused[l] = acc[9] > 0.0 ? 1 : 0;
        gabs = fmax(fabs(acc[6]), fmax(fabs(acc[7]), fabs(acc[8])));
    }
    if (q.heavy) {
        if (writer) gpart[blockIdx.x] = gabs;
        return;
    }
    const double m = block_max<kBaHeavyThreads>(gabs, sh);
    if (threadIdx.x == 0) gpart[blockIdx.x] = m;
}


// ---- camera pass (a wavefront per camera): U_i, g_i; S_ii = U*_i - sum_l (sum_e W_e) V*_l^-1 (sum_f W_f)^T over the observations e, f of
// (i, l) and its inverse; b_i = -g_i + sum W V*^-1 g_l
// (GR, focal groups: the focal diagonal of U*_i stays undamped -- the damping mu D_c of the shared parameter joins where the group sum is
// taken --, sinv is the inverse of the leading pose block with 1 in the focal slot (ba_group_setup_kernel puts 1 / F_c or 0 there), the
// focal gradient is left out of the maximum and goes with the undamped S_ii[f, f] to fstat (2 per camera))
template <int CD, bool GR>
__global__ __launch_bounds__(256) void ba_cam_kernel(SchurLists S, const double *__restrict__ Jc, const double *__restrict__ vinv,
                                                     const double *__restrict__ gl, double mu, double *__restrict__ ustar, double *__restrict__ sinv,
                                                     double *__restrict__ b, int32_t *__restrict__ cused, double *__restrict__ gpart,
                                                     double *__restrict__ fstat) {
    static_assert(!GR || ba_has_focal<CD>(), "focal groups need a focal column");
    constexpr int JP = ba_jp<CD>(), RS = ba_res<CD>(), NU = CD * (CD + 1) / 2, NA = 2 * NU + 2 * CD + 1;
    __shared__ double red[kQwWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cam = (int64_t)blockIdx.x * kQwWaves + wv;
    const bool on = cam < S.n;
    double acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    if (on)
        for (int64_t e = S.cam_ptr[cam] + lane; e < S.cam_ptr[cam + 1]; e += 64) {
            double jc[2 * CD], jp[6];
#pragma unroll
            for (int k = 0; k < 2 * CD; ++k) jc[k] = Jc[(size_t)k * S.nobs + e];
#pragma unroll
            for (int k = 0; k < 6; ++k) jp[k] = Jc[(size_t)(JP + k) * S.nobs + e];
            const double r0 = Jc[(size_t)RS * S.nobs + e], r1 = Jc[(size_t)(RS + 1) * S.nobs + e];
            const int64_t l = S.cam_lm[e];
            double V[3][3], W[CD][3], WV[CD][3];
            sym3(vinv + (size_t)6 * l, V);
            const double g0 = gl[3 * l], g1 = gl[3 * l + 1], g2 = gl[3 * l + 2];
#pragma unroll
            for (int k = 0; k < CD; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) W[k][c] = jc[k] * jp[c] + jc[CD + k] * jp[3 + c];
#pragma unroll
            for (int k = 0; k < CD; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) WV[k][c] = W[k][0] * V[0][c] + W[k][1] * V[1][c] + W[k][2] * V[2][c];
#pragma unroll
            for (int j = 0; j < CD; ++j)
#pragma unroll
                for (int k = 0; k <= j; ++k) {
                    acc[tri(k, j)] += jc[k] * jc[j] + jc[CD + k] * jc[CD + j];
                    acc[NU + tri(k, j)] += WV[k][0] * W[j][0] + WV[k][1] * W[j][1] + WV[k][2] * W[j][2];
                }
#pragma unroll
            for (int k = 0; k < CD; ++k) {
                acc[2 * NU + k] += jc[k] * r0 + jc[CD + k] * r1;
                acc[2 * NU + CD + k] += WV[k][0] * g0 + WV[k][1] * g1 + WV[k][2] * g2;
            }
            acc[NA - 1] += obs_used(jp) ? 1.0 : 0.0;
            // a (camera, landmark) pair named more than once: S_ii holds (sum_e W_e) V*^-1 (sum_f W_f)^T, so every other observation f of the
            // pair brings W_e V*^-1 W_f^T.  The list is sorted by landmark: they are this entry's neighbours (none in an ordinary scene)
            for (int dir = -1; dir <= 1; dir += 2)
                for (int64_t f = e + dir; f >= S.cam_ptr[cam] && f < S.cam_ptr[cam + 1] && S.cam_lm[f] == l; f += dir) {
                    double Wf[CD][3];
#pragma unroll
                    for (int k = 0; k < CD; ++k)
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            Wf[k][c] = Jc[(size_t)k * S.nobs + f] * Jc[(size_t)(JP + c) * S.nobs + f] +
                                       Jc[(size_t)(CD + k) * S.nobs + f] * Jc[(size_t)(JP + 3 + c) * S.nobs + f];
#pragma unroll
                    for (int j = 0; j < CD; ++j)
#pragma unroll
                        for (int k = 0; k <= j; ++k) acc[NU + tri(k, j)] += WV[k][0] * Wf[j][0] + WV[k][1] * Wf[j][1] + WV[k][2] * Wf[j][2];
                }
        }
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = wave_sum(acc[k]);
    double gabs = 0.0;
    if (on && lane == 0) {
        double Us[CD][CD], Sm[CD][CD];
#pragma unroll
        for (int j = 0; j < CD; ++j)
#pragma unroll
            for (int k = 0; k < CD; ++k) {
                const double u = acc[tri(k, j)];
                if constexpr (GR) Us[j][k] = (j == k && j != ba_fidx<CD>()) ? u + mu * clamp_diag(u) : u;
                else Us[j][k] = (j == k) ? u + mu * clamp_diag(u) : u;
                Sm[j][k] = Us[j][k] - acc[NU + tri(k, j)];
            }
        if constexpr (GR) {
            constexpr int F = ba_fidx<CD>();
            fstat[2 * cam] = Sm[F][F]; fstat[2 * cam + 1] = acc[2 * NU + F];
#pragma unroll
            for (int k = 0; k < CD; ++k) Sm[F][k] = Sm[k][F] = (k == F) ? 1.0 : 0.0;
        }
        double *us = ustar + (size_t)CD * CD * cam;
#pragma unroll
        for (int j = 0; j < CD; ++j)
#pragma unroll
            for (int k = 0; k < CD; ++k) us[CD * j + k] = Us[j][k];
        chol_inverse<CD>(Sm, sinv + (size_t)CD * CD * cam);
#pragma unroll
        for (int k = 0; k < CD; ++k) {
            b[(size_t)CD * cam + k] = -acc[2 * NU + k] + acc[2 * NU + CD + k];
            if (!(GR && k == ba_fidx<CD>())) gabs = fmax(gabs, fabs(acc[2 * NU + k]));
        }
        cused[cam] = acc[NA - 1] > 0.0 ? 1 : 0;
    }
    if (lane == 0) red[wv] = gabs;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = 0.0;
        for (int q = 0; q < kQwWaves; ++q) m = fmax(m, red[q]);
        gpart[blockIdx.x] = m;
    }
}

// landmark side of S x (and of the back-substitution): y_l = sgn V*_l^-1 (g_l + sum_{obs of l} J_P^T J_c x_i)   (g: optional)
template <int CD>
__global__ __launch_bounds__(kBaHeavyThreads) void ba_lmx_kernel(SchurLists S, const double *__restrict__ Jl, const double *__restrict__ vinv,
                                                                 const double *__restrict__ gl, double sgn, const int32_t *__restrict__ lused,
                                                                 const double *__restrict__ x, const BaState *__restrict__ st, double *__restrict__ y) {
    constexpr int JP = ba_jp<CD>();
    if (st != nullptr && st->done) return;
    const LmRange q = lm_range(S);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t e = q.e; e < q.e_end; e += q.step) {
        double jc[2 * CD], jp[6];
#pragma unroll
        for (int k = 0; k < 2 * CD; ++k) jc[k] = Jl[(size_t)k * S.lm_total + e];
#pragma unroll
        for (int k = 0; k < 6; ++k) jp[k] = Jl[(size_t)(JP + k) * S.lm_total + e];
        const double *xi = x + (size_t)CD * S.lm_cam[e];
        double u0 = 0.0, u1 = 0.0;
#pragma unroll
        for (int k = 0; k < CD; ++k) { u0 += jc[k] * xi[k]; u1 += jc[CD + k] * xi[k]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += jp[c] * u0 + jp[3 + c] * u1;
    }
    bool writer = q.active;
    if (q.heavy) writer = heavy_sum<3>(acc);
    if (!writer) return;
    const int64_t l = q.l;
    if (!lused[l]) { y[3 * l] = y[3 * l + 1] = y[3 * l + 2] = 0.0; return; }
    if (gl != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += gl[3 * l + c];
    }
    double V[3][3];
    sym3(vinv + (size_t)6 * l, V);
#pragma unroll
    for (int c = 0; c < 3; ++c) y[3 * l + c] = sgn * (V[c][0] * acc[0] + V[c][1] * acc[1] + V[c][2] * acc[2]);
}
// camera side: Ap_i = U*_i p_i - sum_{obs of i} J_c^T J_P y_l (a wavefront per camera); per-workgroup partials of <p, Ap>
template <int CD>
__global__ __launch_bounds__(256) void ba_camx_kernel(SchurLists S, const double *__restrict__ Jc, const double *__restrict__ y, BaPcg a) {
    constexpr int JP = ba_jp<CD>();
    __shared__ double red[kQwWaves];
    if (a.st->done) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cam = (int64_t)blockIdx.x * kQwWaves + wv;
    const bool on = cam < S.n;
    double acc[CD];
#pragma unroll
    for (int k = 0; k < CD; ++k) acc[k] = 0.0;
    if (on)
        for (int64_t e = S.cam_ptr[cam] + lane; e < S.cam_ptr[cam + 1]; e += 64) {
            double jc[2 * CD], jp[6];
#pragma unroll
            for (int k = 0; k < 2 * CD; ++k) jc[k] = Jc[(size_t)k * S.nobs + e];
#pragma unroll
            for (int k = 0; k < 6; ++k) jp[k] = Jc[(size_t)(JP + k) * S.nobs + e];
            const double *yl = y + (size_t)3 * S.cam_lm[e];
            const double v0 = jp[0] * yl[0] + jp[1] * yl[1] + jp[2] * yl[2], v1 = jp[3] * yl[0] + jp[4] * yl[1] + jp[5] * yl[2];
#pragma unroll
            for (int k = 0; k < CD; ++k) acc[k] += jc[k] * v0 + jc[CD + k] * v1;
        }
#pragma unroll
    for (int k = 0; k < CD; ++k) acc[k] = wave_sum(acc[k]);
    double pap = 0.0;
    if (on && lane == 0) {
        double up[CD];
        block_matvec<CD>(a.ustar + (size_t)CD * CD * cam, a.p + (size_t)CD * cam, up);
#pragma unroll
        for (int k = 0; k < CD; ++k) {
            const double v = up[k] - acc[k];
            a.Ap[CD * cam + k] = v;
            pap += a.p[CD * cam + k] * v;
        }
    }
    if (lane == 0) red[wv] = pap;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < kQwWaves; ++q) t += red[q];
        a.ppap[blockIdx.x] = t;
    }
}

// ---- dense reduced camera system (XM_BA_DENSE_SCHUR): the lower block triangle of
//   S_ij = delta_ij U*_i - sum_l (sum_{e in (i,l)} W_e) V*_l^-1 (sum_{f in (j,l)} W_f)^T,   j <= i,
// column-major with leading dimension ld = CD n, into a matrix the caller has zeroed.  A wavefront per block row i: it writes U*_i, then walks
// camera i's list in list order; for observation e of landmark l the lanes run over l's list (the packed group of a light landmark, the
// contiguous list of a heavy one, 64 at a time) and lane f subtracts (W_e V*_l^-1) W_f^T from block (i, camera of f).  Every pair (e, f) of a
// landmark is taken, so a (camera, landmark) pair named twice brings its cross terms.  Two lanes of one batch on the same block (such a pair
// again) write one after the other, in lane order, behind a workgroup fence each time: the additions to every entry come in a fixed order
// and no floating-point atomics are used.  Only this wavefront writes row i, so nothing else orders them.
template <int CD>
__global__ __launch_bounds__(256) void ba_schur_dense_kernel(SchurLists S, const double *__restrict__ Jc, const double *__restrict__ Jl,
                                                             const double *__restrict__ vinv, const double *__restrict__ ustar, double *__restrict__ Sd,
                                                             int64_t ld) {
    constexpr int JP = ba_jp<CD>();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kQwWaves + wv;
    if (i >= S.n) return;
    double *row = Sd + (size_t)CD * i;   // entry (CD i + a, c) at row[a + c ld]
    if (lane < CD * CD) row[lane / CD + ((size_t)CD * i + lane % CD) * ld] = ustar[(size_t)CD * CD * i + lane];
    __threadfence_block();
    for (int64_t e = S.cam_ptr[i]; e < S.cam_ptr[i + 1]; ++e) {
        double jc[2 * CD], jp[6];
#pragma unroll
        for (int k = 0; k < 2 * CD; ++k) jc[k] = Jc[(size_t)k * S.nobs + e];
#pragma unroll
        for (int k = 0; k < 6; ++k) jp[k] = Jc[(size_t)(JP + k) * S.nobs + e];
        if (!obs_used(jp)) continue;
        const int64_t l = S.cam_lm[e];
        double V[3][3], X[CD][3];
        sym3(vinv + (size_t)6 * l, V);
#pragma unroll
        for (int k = 0; k < CD; ++k) {
            double w[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) w[c] = jc[k] * jp[c] + jc[CD + k] * jp[3 + c];
#pragma unroll
            for (int c = 0; c < 3; ++c) X[k][c] = w[0] * V[0][c] + w[1] * V[1][c] + w[2] * V[2][c];
        }
        int64_t f0, cnt, stride;
        if (l < S.nheavy) { f0 = S.lm_ptr[l]; cnt = S.lm_ptr[l + 1] - f0; stride = 1; }
        else { const int64_t t = l - S.nheavy; f0 = S.gbase[t >> 6] + (t & 63); cnt = S.deg[l]; stride = 64; }
        for (int64_t k0 = 0; k0 < cnt; k0 += 64) {
            const int nb = (int)(cnt - k0 < 64 ? cnt - k0 : 64);
            int j = -1;
            double C[CD][CD];
            if (lane < nb) {
                const size_t f = (size_t)(f0 + (k0 + lane) * stride);
                double jc2[2 * CD], jp2[6];
#pragma unroll
                for (int k = 0; k < 2 * CD; ++k) jc2[k] = Jl[(size_t)k * S.lm_total + f];
#pragma unroll
                for (int k = 0; k < 6; ++k) jp2[k] = Jl[(size_t)(JP + k) * S.lm_total + f];
                const int jf = S.lm_cam[f];
                if (jf <= i && obs_used(jp2)) {
                    j = jf;
#pragma unroll
                    for (int b = 0; b < CD; ++b) {
                        double w[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) w[c] = jc2[b] * jp2[c] + jc2[CD + b] * jp2[3 + c];
#pragma unroll
                        for (int a = 0; a < CD; ++a) C[a][b] = X[a][0] * w[0] + X[a][1] * w[1] + X[a][2] * w[2];
                    }
                }
            }
            int rank = 0;   // earlier lanes of this batch on the same block
            for (int q = 0; q < nb; ++q) {
                const int jq = __builtin_amdgcn_readlane(j, q);
                rank += (q < lane && jq >= 0 && jq == j) ? 1 : 0;
            }
            const int rmax = (int)wave_max((double)rank);
            for (int r = 0; r <= rmax; ++r) {
                if (j >= 0 && rank == r) {
                    double *blk = row + (size_t)CD * j * ld;
#pragma unroll
                    for (int b = 0; b < CD; ++b)
#pragma unroll
                        for (int a = 0; a < CD; ++a) blk[a + (size_t)b * ld] -= C[a][b];
                }
                __threadfence_block();
            }
        }
    }
}
// per-workgroup partials of |b - S dc|^2 and |b|^2 (S dc from the matrix-free product)
template <int CD>
__global__ __launch_bounds__(256) void ba_dense_res_kernel(int64_t n, const double *__restrict__ b, const double *__restrict__ sx, double *__restrict__ parts) {
    __shared__ double sh[4];
    double rr = 0.0, bb = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n * CD; k += (int64_t)gridDim.x * 256) {
        const double d = b[k] - sx[k];
        rr += d * d; bb += b[k] * b[k];
    }
    rr = block_sum256(rr, sh);
    bb = block_sum256(bb, sh);
    if (threadIdx.x == 0) { parts[blockIdx.x] = rr; parts[gridDim.x + blockIdx.x] = bb; }
}

// ---- candidate point.  Cameras: Rcw <- Exp(dtheta) Rcw (Rodrigues), tcw += dt; cameras without a used observation are copied.
// With a focal column (G, gfree, Gn, st given): g += dg for a used camera whose focal is free, a copy elsewhere; g^2 joins |x|^2; a candidate
// focal that is not positive sets the state word's bad_focal (cleared before the launch; every writer stores the same 1).
// (GR, focal groups: dc is the expanded step; the focal entry is the group's -- ba_group_cand_kernel takes the step, the norms and the
// sign test once per group --, every member reads its group's candidate gnew[group_of[i]]; |x|^2 partials at parts[xoff + workgroup];
// G, gfree and st are not read.  Without GR: group_of, gnew and xoff are not read.)  Without a focal column G, gfree and Gn are null and
// st is not read.
template <int CD, bool GR>
__device__ __forceinline__ void ba_cand_cam_body(int64_t n, const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                 const double *__restrict__ G, const uint8_t *__restrict__ gfree, const double *__restrict__ dc,
                                                 const int32_t *__restrict__ cused, double *__restrict__ Rn, double *__restrict__ tn,
                                                 double *__restrict__ Gn, BaState *__restrict__ st, double *__restrict__ parts,
                                                 const int32_t *__restrict__ group_of, const double *__restrict__ gnew, int xoff,
                                                 const double *__restrict__ Kd, const uint8_t *__restrict__ kfree, double *__restrict__ Kn) {
    static_assert(!GR || ba_has_focal<CD>(), "focal groups need a focal column");
    __shared__ double sh[4];
    double s2 = 0.0, x2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double *R = Rcw + 9 * i, *T = tcw + 3 * i, *d = dc + CD * i;
        if (!cused[i]) {
#pragma unroll
            for (int k = 0; k < 9; ++k) Rn[9 * i + k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) tn[3 * i + k] = T[k];
            if constexpr (GR) Gn[i] = gnew[group_of[i]];
            else if constexpr (ba_has_focal<CD>()) Gn[i] = G[i];
            if constexpr (ba_has_dist<CD>()) Kn[i] = Kd[i];
            continue;
        }
        const double *dt = d + ba_toff<CD>();
#pragma unroll
        for (int k = 0; k < 3; ++k) { tn[3 * i + k] = T[k] + dt[k]; x2 += T[k] * T[k]; }
#pragma unroll
        for (int k = 0; k < (GR ? CD - 1 : CD); ++k) s2 += d[k] * d[k];
        if constexpr (GR) {
            Gn[i] = gnew[group_of[i]];
        } else if constexpr (ba_has_focal<CD>()) {
            const double g = G[i];
            if (gfree == nullptr || gfree[i] != 0) {
                const double gn = g + d[ba_fidx<CD>()];
                Gn[i] = gn;
                x2 += g * g;
                if (!(gn > 0.0)) st->bad_focal = 1;
            } else {
                Gn[i] = g;
            }
        }
        if constexpr (ba_has_dist<CD>()) {   // k += dk for a free coefficient (either sign is a value), a copy elsewhere; k^2 joins |x|^2
            const double kd = Kd[i];
            if (kfree == nullptr || kfree[i] != 0) {
                Kn[i] = kd + d[ba_kidx<CD>()];
                x2 += kd * kd;
            } else {
                Kn[i] = kd;
            }
        }
        if constexpr (ba_has_rot<CD>()) {
            x2 += 1.0;   // the unit quaternion of the rotation
            const double w0 = d[0], w1 = d[1], w2 = d[2], th2 = w0 * w0 + w1 * w1 + w2 * w2;
            double A, B;
            if (th2 < 1e-16) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; }
            else { const double th = sqrt(th2); A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
            const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
            double E[3][3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) E[a][c] = (a == c ? 1.0 : 0.0) + A * K[a][c] + B * (K[a][0] * K[0][c] + K[a][1] * K[1][c] + K[a][2] * K[2][c]);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) Rn[9 * i + 3 * a + c] = E[a][0] * R[c] + E[a][1] * R[3 + c] + E[a][2] * R[6 + c];
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) Rn[9 * i + k] = R[k];
        }
    }
    s2 = block_sum256(s2, sh);
    x2 = block_sum256(x2, sh);
    if constexpr (GR) {
        if (threadIdx.x == 0) { parts[blockIdx.x] = s2; parts[xoff + blockIdx.x] = x2; }
    } else {
        if (threadIdx.x == 0) { parts[blockIdx.x] = s2; parts[gridDim.x + blockIdx.x] = x2; }
    }
}
template <int CD, bool GR>
__global__ __launch_bounds__(256) void ba_cand_cam_kernel(int64_t n, const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                          const double *__restrict__ G, const uint8_t *__restrict__ gfree,
                                                          const double *__restrict__ dc, const int32_t *__restrict__ cused,
                                                          double *__restrict__ Rn, double *__restrict__ tn, double *__restrict__ Gn,
                                                          BaState *__restrict__ st, double *__restrict__ parts,
                                                          const int32_t *__restrict__ group_of, const double *__restrict__ gnew, int xoff,
                                                          const double *__restrict__ Kd, const uint8_t *__restrict__ kfree,
                                                          double *__restrict__ Kn) {
    ba_cand_cam_body<CD, GR>(n, Rcw, tcw, G, gfree, dc, cused, Rn, tn, Gn, st, parts, group_of, gnew, xoff, Kd, kfree, Kn);
}
// ---- focal groups (xm_ctx_bundle_adjust_focal_groups): one focal scale per group of cameras.  With E the 0/1 matrix that copies a group's
// focal unknown into the focal column of each member, J_shared = J_7 E, so S_shared = E^T S_7 E and b_shared = E^T b_7: the kernels above
// run as they are (CD = 7 / 4) on expanded vectors, and the kernels below expand before them and sum by group after them.  A vector of
// the shared space lives in a CD n array: the pose slots of every camera, the group's entry in the focal slot of its representative (its
// first member), 0 in the focal slots of the other members -- so the PCG's vector kernels run unchanged on it.  An empty group has no slot:
// it is held.  The sums over a group's members are taken in member order by one thread (up to 64 members) or lane-strided by one workgroup
// with the DPP tree of block_sum256 behind it (more): a fixed order, no atomics.
struct BaGroups {
    int32_t ng, nsmall, nsb;   // groups; those of at most 64 members (the first nsmall of list); the workgroups that take these, a thread each
    const int32_t *off, *mem;  // the members of group c: mem[off[c] .. off[c + 1]), ascending
    const int32_t *rep;        // its representative, -1: empty
    const int32_t *list;       // the groups in the order the workgroups take them: the small ones, then one workgroup for each other
    const uint8_t *free;       // 0 = held; null: all free
};
constexpr int kBaGroupThread = 64;   // a group of up to this many members: one thread
// the group of this thread (small groups; -1: none) or of this workgroup; K sums over its members, valid in `writer` (the thread itself, or
// every thread of the workgroup); sh: 4 doubles
template <int K, class Load>
__device__ __forceinline__ int group_reduce(const BaGroups &g, double (&acc)[K], double *sh, bool &big, Load &&load) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    big = (int)blockIdx.x >= g.nsb;
    if (!big) {
        const int q = blockIdx.x * 256 + threadIdx.x;
        if (q >= g.nsmall) return -1;
        const int c = g.list[q];
        for (int k = g.off[c]; k < g.off[c + 1]; ++k) load(g.mem[k], acc);
        return c;
    }
    const int c = g.list[g.nsmall + ((int)blockIdx.x - g.nsb)];
    for (int k = g.off[c] + threadIdx.x; k < g.off[c + 1]; k += 256) load(g.mem[k], acc);
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = block_sum256(acc[k], sh);
    return c;
}
// f(member) for every member of group c but its representative, by the threads that summed it
template <class F>
__device__ __forceinline__ void group_others(const BaGroups &g, int c, bool big, F &&f) {
    if (c < 0) return;
    const int first = g.off[c] + 1;   // the representative is the first member
    if (!big) { for (int k = first; k < g.off[c + 1]; ++k) f(g.mem[k]); }
    else { for (int k = first + threadIdx.x; k < g.off[c + 1]; k += 256) f(g.mem[k]); }
}
// per LM iteration, after the camera pass: D_c = clamp(sum U_ff,i), b_c = sum b_7,if into the representative's slot (0 in the others'),
// F_c = sum S_7,ii[f, f] (undamped) + mu D_c and 1 / F_c into the representative's focal slot of sinv (0 in the others'), moving_c = free and
// a member with a used observation; per-workgroup max of |sum g_if| for the gradient's maximum
template <int CD>
__global__ __launch_bounds__(256) void ba_group_setup_kernel(BaGroups g, const double *__restrict__ ustar, const double *__restrict__ fstat,
                                                             const int32_t *__restrict__ cused, double mu, double *__restrict__ b,
                                                             double *__restrict__ sinv, double *__restrict__ D, double *__restrict__ F,
                                                             int32_t *__restrict__ moving, double *__restrict__ gpart) {
    constexpr int FI = ba_fidx<CD>(), FF = CD * FI + FI;
    __shared__ double sh[4];
    __shared__ double shm[4];
    double acc[5];
    bool big;
    const int c = group_reduce<5>(g, acc, sh, big, [&](int i, double (&a)[5]) {
        a[0] += ustar[(size_t)CD * CD * i + FF]; a[1] += b[(size_t)CD * i + FI]; a[2] += fstat[2 * (size_t)i + 1]; a[3] += fstat[2 * (size_t)i];
        a[4] += cused[i] ? 1.0 : 0.0;
    });
    double gabs = 0.0;
    group_others(g, c, big, [&](int i) { b[(size_t)CD * i + FI] = 0.0; sinv[(size_t)CD * CD * i + FF] = 0.0; });
    if (c >= 0 && (!big || threadIdx.x == 0)) {
        const double d = clamp_diag(acc[0]);
        double f = acc[3] + mu * d;
        if (!(f > 0.0)) f = mu * d;
        D[c] = d; F[c] = f;
        moving[c] = ((g.free == nullptr || g.free[c] != 0) && acc[4] > 0.0) ? 1 : 0;
        const int r = g.rep[c];
        if (r >= 0) { b[(size_t)CD * r + FI] = acc[1]; sinv[(size_t)CD * CD * r + FF] = 1.0 / f; }
        gabs = fabs(acc[2]);
    }
    const double m = block_max<256>(gabs, shm);
    if (threadIdx.x == 0) gpart[blockIdx.x] = m;
}
// dst = E src: the pose slots copied, every member's focal slot from its group's representative (rep_of: per camera)
template <int CD>
__global__ __launch_bounds__(256) void ba_group_expand_kernel(int64_t n, const int32_t *__restrict__ rep_of, const double *__restrict__ src,
                                                              double *__restrict__ dst, const BaState *__restrict__ gate) {
    if (gate != nullptr && gate->done) return;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n * CD; j += (int64_t)gridDim.x * 256) {
        const int64_t i = j / CD;
        const int k = (int)(j - i * CD);
        dst[j] = (k == ba_fidx<CD>()) ? src[(size_t)CD * rep_of[i] + k] : src[j];
    }
}
// Ap <- E^T Ap + mu D x in the focal slots: the members' entries summed into the representative's, plus mu D_c x_c (x: the vector before
// the expansion); 0 in the other members' slots; per-workgroup partials of mu D_c x_c^2, the part of <x, A x> the camera kernel has not seen
template <int CD>
__global__ __launch_bounds__(256) void ba_group_sum_kernel(BaGroups g, const double *__restrict__ D, double mu, const double *__restrict__ x,
                                                           double *__restrict__ Ap, double *__restrict__ ppap, const BaState *__restrict__ gate) {
    constexpr int FI = ba_fidx<CD>();
    __shared__ double sh[4];
    if (gate != nullptr && gate->done) return;
    double acc[1];
    bool big;
    const int c = group_reduce<1>(g, acc, sh, big, [&](int i, double (&a)[1]) { a[0] += Ap[(size_t)CD * i + FI]; });
    group_others(g, c, big, [&](int i) { Ap[(size_t)CD * i + FI] = 0.0; });
    double pap = 0.0;
    if (c >= 0 && (!big || threadIdx.x == 0) && g.rep[c] >= 0) {
        const size_t at = (size_t)CD * g.rep[c] + FI;
        const double xc = x[at], dx = mu * D[c] * xc;
        Ap[at] = acc[0] + dx;
        pap = dx * xc;
    }
    pap = block_sum256(pap, sh);
    if (threadIdx.x == 0) ppap[blockIdx.x] = pap;
}
// the groups' candidate: g_c + dg_c for a moving group (dc: the step before the expansion), a copy elsewhere; dg_c^2 and g_c^2 once per
// moving group into the partials of |d|^2 and |x|^2 (at parts[workgroup] and parts[xoff + workgroup]); a candidate that is not positive
// sets bad_focal
template <int CD>
__global__ __launch_bounds__(256) void ba_group_cand_kernel(BaGroups g, const double *__restrict__ G, const double *__restrict__ dc,
                                                            const int32_t *__restrict__ moving, double *__restrict__ gnew,
                                                            BaState *__restrict__ st, double *__restrict__ parts, int xoff) {
    __shared__ double sh[4];
    double s2 = 0.0, x2 = 0.0;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < g.ng; c += gridDim.x * 256) {
        const int r = g.rep[c];
        if (r < 0) { gnew[c] = 1.0; continue; }   // empty: nobody reads it
        const double g0 = G[r];
        if (moving[c]) {
            const double d = dc[(size_t)CD * r + ba_fidx<CD>()], gn = g0 + d;
            gnew[c] = gn;
            s2 += d * d; x2 += g0 * g0;
            if (!(gn > 0.0)) st->bad_focal = 1;
        } else {
            gnew[c] = g0;
        }
    }
    s2 = block_sum256(s2, sh);
    x2 = block_sum256(x2, sh);
    if (threadIdx.x == 0) { parts[blockIdx.x] = s2; parts[xoff + blockIdx.x] = x2; }
}
// ---- the exact focal block of the preconditioner (at most XM_BA_FOCAL_GROUPS_EXACT groups): F = S_shared[focal, focal], column d from the
// product with the indicator of group d.  v <- e_slot
__global__ __launch_bounds__(256) void ba_group_unit_kernel(int64_t count, int64_t slot, double *__restrict__ v) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < count; j += (int64_t)gridDim.x * 256) v[j] = j == slot ? 1.0 : 0.0;
}
// column d of F (column-major G x G) from A p = S_shared e_d; an empty group (it has no slot): mu D_c on its diagonal, as the held groups have
template <int CD>
__global__ __launch_bounds__(256) void ba_group_col_kernel(BaGroups g, int d, const double *__restrict__ Ap, const double *__restrict__ D, double mu,
                                                           double *__restrict__ Fm) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= g.ng) return;
    const int r = g.rep[c];
    Fm[c + (size_t)g.ng * d] = (r >= 0 && g.rep[d] >= 0) ? Ap[(size_t)CD * r + ba_fidx<CD>()] : (c == d ? mu * D[c] : 0.0);
}
// F was inverted: the focal slots of the block-Jacobi inverse give way to it (z_f = 0 from the vector kernels)
template <int CD>
__global__ __launch_bounds__(256) void ba_group_exact_on_kernel(BaGroups g, double *__restrict__ sinv) {
    constexpr int FI = ba_fidx<CD>();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < g.ng && g.rep[c] >= 0) sinv[(size_t)CD * CD * g.rep[c] + CD * FI + FI] = 0.0;
}
// behind the PCG's start or update (one workgroup): z_focal = F^-1 r_focal (Finv: the full symmetric inverse), p = z at the start, and
// <r_focal, z_focal> into the partial behind the vector kernels' (slot a.grid - 1).  exact = 0 (the factorisation failed this iteration and
// the diagonal stands): that partial is 0
template <int CD>
__global__ __launch_bounds__(256) void ba_group_precond_kernel(BaGroups g, const double *__restrict__ Finv, BaPcg a, int it, int init, int exact) {
    constexpr int FI = ba_fidx<CD>();
    __shared__ double sh[4];
    if (!init && a.st->done) return;
    const int c = threadIdx.x;
    double rz = 0.0;
    if (exact && c < g.ng && g.rep[c] >= 0) {
        double z = 0.0;
        for (int d = 0; d < g.ng; ++d)
            if (g.rep[d] >= 0) z += Finv[(size_t)c * g.ng + d] * a.r[(size_t)CD * g.rep[d] + FI];
        const size_t at = (size_t)CD * g.rep[c] + FI;
        a.z[at] = z;
        if (init) a.p[at] = z;
        rz = a.r[at] * z;
    }
    rz = block_sum256(rz, sh);
    if (threadIdx.x == 0) a.prz[init ? 0 : (it & 1) ^ 1][a.grid - 1] = rz;
}

// ---- XM_BA_DENSE_SCHUR with focal groups: the CD n matrix of ba_schur_dense_kernel (the members' focal diagonal undamped) contracted by
// group in place, S_shared = E^T S_7 E + mu D in the layout of the vectors: the group's row and column in its representative's focal slot,
// the other members' focal slots a unit row and column.  Only the lower triangle is read and written (what the factorisation reads).
__device__ __forceinline__ double &dense_low(double *Sd, int64_t ld, int64_t a, int64_t b) { return a >= b ? Sd[a + b * ld] : Sd[b + a * ld]; }
// T[c nd + k] = sum_{i in c} S_7[f_i, k] over the members in order, every column k
template <int CD>
__global__ __launch_bounds__(256) void ba_group_dense_rows_kernel(BaGroups g, double *__restrict__ Sd, int64_t ld, int64_t nd, double *__restrict__ T) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < g.ng * nd; q += (int64_t)gridDim.x * 256) {
        const int c = (int)(q / nd);
        const int64_t k = q - c * nd;
        double s = 0.0;
        for (int m = g.off[c]; m < g.off[c + 1]; ++m) s += dense_low(Sd, ld, (int64_t)CD * g.mem[m] + ba_fidx<CD>(), k);
        T[q] = s;
    }
}
// U[c + G d] = sum_{j in d} T[c, f_j]
template <int CD>
__global__ __launch_bounds__(256) void ba_group_dense_cols_kernel(BaGroups g, int64_t nd, const double *__restrict__ T, double *__restrict__ U) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.ng * g.ng) return;
    const int c = q % g.ng, d = q / g.ng;
    double s = 0.0;
    for (int m = g.off[d]; m < g.off[d + 1]; ++m) s += T[(size_t)c * nd + (size_t)CD * g.mem[m] + ba_fidx<CD>()];
    U[q] = s;
}
// every focal row and column becomes a unit one ...
template <int CD>
__global__ __launch_bounds__(256) void ba_group_dense_clear_kernel(int64_t n, double *__restrict__ Sd, int64_t ld, int64_t nd) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n * nd; q += (int64_t)gridDim.x * 256) {
        const int64_t i = q / nd, k = q - i * nd, f = CD * i + ba_fidx<CD>();
        dense_low(Sd, ld, f, k) = k == f ? 1.0 : 0.0;
    }
}
// ... and the representatives' take the contracted entries: T against the pose columns, U (its lower triangle) + mu D among the groups
template <int CD>
__global__ __launch_bounds__(256) void ba_group_dense_write_kernel(BaGroups g, double *__restrict__ Sd, int64_t ld, int64_t nd, const double *__restrict__ T,
                                                                   const double *__restrict__ U, const double *__restrict__ D, double mu) {
    constexpr int FI = ba_fidx<CD>();
    const int64_t nt = g.ng * nd;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nt + (int64_t)g.ng * g.ng; q += (int64_t)gridDim.x * 256) {
        if (q < nt) {
            const int c = (int)(q / nd);
            const int64_t k = q - c * nd;
            if (g.rep[c] >= 0 && k % CD != FI) dense_low(Sd, ld, (int64_t)CD * g.rep[c] + FI, k) = T[q];
        } else {
            const int c = (int)((q - nt) % g.ng), d = (int)((q - nt) / g.ng);
            if (d <= c && g.rep[c] >= 0 && g.rep[d] >= 0)
                dense_low(Sd, ld, (int64_t)CD * g.rep[c] + FI, (int64_t)CD * g.rep[d] + FI) = U[c + (size_t)g.ng * d] + (c == d ? mu * D[c] : 0.0);
        }
    }
}
// (the landmarks' candidate: ba_cand_vec_kernel of xm_lm_shared.h)
// cost 1/2 sum rho(|r|^2) at the candidate (the eval kernel's expression) and the linear model's terms sum r.(J d) + |J d|^2 / 2 (J, r: the
// stored records of the current point, by-camera order)
// (Gn: the candidate's focal scales, read only where the camera block has a focal column and null elsewhere; scale: as in ba_eval_kernel)
template <int CD, int LOSS>
__device__ __forceinline__ void ba_cost_body(const SchurLists &S, const double *__restrict__ Rn, const double *__restrict__ tn,
                                             const double *__restrict__ Pn, const double *__restrict__ Gn, const double *__restrict__ Jc,
                                             const double *__restrict__ dc, const double *__restrict__ dP, double *__restrict__ parts,
                                             double scale, const double *__restrict__ Kn, BaState *__restrict__ st) {
    constexpr int JP = ba_jp<CD>(), RS = ba_res<CD>();
    __shared__ double sh[4];
    double cost = 0.0, model = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * 256) {
        const int64_t pc = S.pos_c[e];
        const double w = S.cam_w[pc], q0 = S.obs_p[3 * e], q1 = S.obs_p[3 * e + 1], q2 = S.obs_p[3 * e + 2];
        if (!(w > 0.0 && q2 > 0.0)) continue;
        const int64_t i = S.obs_cam[e], l = S.obs_lm[e];
        const double *R = Rn + 9 * i, *T = tn + 3 * i, *X3 = Pn + 3 * l;
        double X[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) X[a] = R[3 * a] * X3[0] + R[3 * a + 1] * X3[1] + R[3 * a + 2] * X3[2] + T[a];
        double e0, e1;
        if constexpr (ba_has_dist<CD>()) {   // past 1 + 3 k |u|^2 = 0 the radial map folds: an invalid candidate, as a focal that is not positive
            const double u0 = X[0] / X[2], u1 = X[1] / X[2], g = Gn[i], kd = Kn[i], rho2 = u0 * u0 + u1 * u1, s = 1.0 + kd * rho2;
            e0 = g * s * u0 - q0 / q2; e1 = g * s * u1 - q1 / q2;
            if (!(1.0 + 3.0 * kd * rho2 > 0.0)) st->bad_focal = 1;
        } else if constexpr (ba_has_focal<CD>()) { e0 = Gn[i] * (X[0] / X[2]) - q0 / q2; e1 = Gn[i] * (X[1] / X[2]) - q1 / q2; }
        else { e0 = X[0] / X[2] - q0 / q2; e1 = X[1] / X[2] - q1 / q2; }
        if constexpr (LOSS == XM_BA_LOSS_TRIVIAL) {
            cost += 0.5 * (e0 * e0 + e1 * e1);
        } else {
            double rho1;
            cost += 0.5 * ba_rho<LOSS>(e0 * e0 + e1 * e1, scale, rho1);
        }
        double jd0 = 0.0, jd1 = 0.0;
#pragma unroll
        for (int k = 0; k < CD; ++k) {
            jd0 += Jc[(size_t)k * S.nobs + pc] * dc[CD * i + k];
            jd1 += Jc[(size_t)(CD + k) * S.nobs + pc] * dc[CD * i + k];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            jd0 += Jc[(size_t)(JP + c) * S.nobs + pc] * dP[3 * l + c];
            jd1 += Jc[(size_t)(JP + 3 + c) * S.nobs + pc] * dP[3 * l + c];
        }
        const double r0 = Jc[(size_t)RS * S.nobs + pc], r1 = Jc[(size_t)(RS + 1) * S.nobs + pc];
        model += r0 * jd0 + r1 * jd1 + 0.5 * (jd0 * jd0 + jd1 * jd1);
    }
    cost = block_sum256(cost, sh);
    model = block_sum256(model, sh);
    if (threadIdx.x == 0) { parts[blockIdx.x] = cost; parts[gridDim.x + blockIdx.x] = model; }
}
template <int CD, int LOSS>
__global__ __launch_bounds__(256) void ba_cost_kernel(SchurLists S, const double *__restrict__ Rn, const double *__restrict__ tn,
                                                      const double *__restrict__ Pn, const double *__restrict__ Gn,
                                                      const double *__restrict__ Jc, const double *__restrict__ dc,
                                                      const double *__restrict__ dP, double *__restrict__ parts, double scale,
                                                      const double *__restrict__ Kn, BaState *__restrict__ st) {
    ba_cost_body<CD, LOSS>(S, Rn, tn, Pn, Gn, Jc, dc, dP, parts, scale, Kn, st);
}
// |r_e|^2 per observation in input order at (Rcw, tcw, P) (the eval kernel's projection, unrobustified); -1 where the observation is not used
// (FOCAL: at the focal scales G, |g_i pi(X) - z|^2; without it G is null and not read)
template <bool FOCAL>
__global__ __launch_bounds__(256) void ba_sqerr_kernel(SchurLists S, const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                       const double *__restrict__ P, const double *__restrict__ G, double *__restrict__ sqerr) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * 256) {
        const double w = S.cam_w[S.pos_c[e]], q0 = S.obs_p[3 * e], q1 = S.obs_p[3 * e + 1], q2 = S.obs_p[3 * e + 2];
        double sq = -1.0;
        if (w > 0.0 && q2 > 0.0) {
            double Y[3], X[3];
            ba_point(Rcw + (size_t)9 * S.obs_cam[e], tcw + (size_t)3 * S.obs_cam[e], P + (size_t)3 * S.obs_lm[e], Y, X);
            double r0, r1;
            if constexpr (FOCAL) { const double g = G[S.obs_cam[e]]; r0 = g * (X[0] / X[2]) - q0 / q2; r1 = g * (X[1] / X[2]) - q1 / q2; }
            else { r0 = X[0] / X[2] - q0 / q2; r1 = X[1] / X[2] - q1 / q2; }
            sq = r0 * r0 + r1 * r1;
        }
        sqerr[e] = sq;
    }
}

// the same at the focal scales G and the radial coefficients Kd: |g_i (1 + k_i |u|^2) u - z|^2, u = pi(X)
__global__ __launch_bounds__(256) void ba_sqerr_radial_kernel(SchurLists S, const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                              const double *__restrict__ P, const double *__restrict__ G,
                                                              const double *__restrict__ Kd, double *__restrict__ sqerr) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * 256) {
        const double w = S.cam_w[S.pos_c[e]], q0 = S.obs_p[3 * e], q1 = S.obs_p[3 * e + 1], q2 = S.obs_p[3 * e + 2];
        double sq = -1.0;
        if (w > 0.0 && q2 > 0.0) {
            double Y[3], X[3];
            ba_point(Rcw + (size_t)9 * S.obs_cam[e], tcw + (size_t)3 * S.obs_cam[e], P + (size_t)3 * S.obs_lm[e], Y, X);
            const double u0 = X[0] / X[2], u1 = X[1] / X[2], g = G[S.obs_cam[e]], s = 1.0 + Kd[S.obs_cam[e]] * (u0 * u0 + u1 * u1);
            const double r0 = g * s * u0 - q0 / q2, r1 = g * s * u1 - q1 / q2;
            sq = r0 * r0 + r1 * r1;
        }
        sqerr[e] = sq;
    }
}

// ---- opt-in preconditioners of the PCG (XM_BA_PRECOND_BLOCKS, XM_BA_PRECOND_TWO_LEVEL): M^-1 = blockdiag(S_aa)^-1 [+ P A_c^-1 P^T].
// Aggregates: runs of kBaAgg members of the host's breadth-first order (ba_aggregate_plan); members are the cameras with a used observation,
// the others keep z = 0 (their right-hand side and residual are 0).  A last aggregate of one member has a block of its own but shares the
// coarse columns of its predecessor: nagg blocks, ncoarse = nagg or nagg - 1 coarse aggregates.  The coarse space of an aggregate: the
// first-order effect on its members' (dtheta, dtcw) of the world motion X -> X + w x (X - c) + v + s (X - c) about the centroid c of their
// centres C_i = -Rcw_i^T tcw_i -- 7 columns (w, v, s), or the 4 columns (v, s) of the dtcw rows with fixed rotations -- scaled to unit norm.
constexpr int kBaAgg = XM_BA_AGG_CAMS;
template <int CD> constexpr int ba_nc() { return CD == 6 ? 7 : 4; }
struct BaTl {
    int32_t nagg, ncoarse, nmem, use_coarse;
    const int32_t *order;    // the members in plan order: block a = positions [a kBaAgg, min(nmem, (a + 1) kBaAgg))
    const int32_t *agg_of;   // camera -> block aggregate, -1: not a member
    const double *binv;      // nagg blocks S_aa^-1, (kBaAgg CD)^2 each, symmetric
    const double *Pm;        // per camera CD x NC (row-major), the scaled columns of its coarse aggregate
    const double *ainv;      // A_c^-1, (NC ncoarse)^2, symmetric
    double *gpart;           // P^T r by block aggregate: nagg x NC
};
__device__ __forceinline__ void coarse_range(const BaTl &t, int ca, int &k0, int &k1) {
    k0 = ca * kBaAgg;
    k1 = (ca == t.ncoarse - 1) ? t.nmem : k0 + kBaAgg;
}
// the CD x NC rows of camera (R, T) for the motion about c, unscaled
template <int CD>
__device__ __forceinline__ void tl_cam_basis(const double *R, const double *T, const double (&c)[3], double (&blk)[CD][ba_nc<CD>()]) {
    constexpr int NC = ba_nc<CD>();
    double C[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { C[a] = -(R[a] * T[0] + R[3 + a] * T[1] + R[6 + a] * T[2]); d[a] = C[a] - c[a]; }
#pragma unroll
    for (int r = 0; r < CD; ++r)
#pragma unroll
        for (int k = 0; k < NC; ++k) blk[r][k] = 0.0;
    constexpr int T0 = CD == 6 ? 3 : 0, V0 = CD == 6 ? 3 : 0;   // first dtcw row; first column of v
    if constexpr (CD == 6) {
        // dtheta = -R w;  dtcw = R ([d]x - [C]x) w
        const double K[3][3] = {{0.0, -(d[2] - C[2]), d[1] - C[1]}, {d[2] - C[2], 0.0, -(d[0] - C[0])}, {-(d[1] - C[1]), d[0] - C[0], 0.0}};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                blk[a][b] = -R[3 * a + b];
                blk[3 + a][b] = R[3 * a] * K[0][b] + R[3 * a + 1] * K[1][b] + R[3 * a + 2] * K[2][b];
            }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) blk[T0 + a][V0 + b] = -R[3 * a + b];
        blk[T0 + a][V0 + 3] = -(R[3 * a] * d[0] + R[3 * a + 1] * d[1] + R[3 * a + 2] * d[2]);
    }
}
// P at the current point, a thread per coarse aggregate (at most 17 members): centroid, column norms, scaled rows; drop[NC ca + k] = 1 for
// a column of norm 0 (all members at one centre: the scale column, and with one member the rotation about it)
template <int CD>
__global__ __launch_bounds__(256) void ba_tl_basis_kernel(BaTl t, const double *__restrict__ Rcw, const double *__restrict__ tcw, double *__restrict__ Pm,
                                                          double *__restrict__ drop) {
    constexpr int NC = ba_nc<CD>();
    const int ca = blockIdx.x * 256 + threadIdx.x;
    if (ca >= t.ncoarse) return;
    int k0, k1;
    coarse_range(t, ca, k0, k1);
    double c[3] = {0.0, 0.0, 0.0};
    for (int k = k0; k < k1; ++k) {
        const double *R = Rcw + (size_t)9 * t.order[k], *T = tcw + (size_t)3 * t.order[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] += -(R[a] * T[0] + R[3 + a] * T[1] + R[6 + a] * T[2]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] /= (double)(k1 - k0);
    double nrm[NC], blk[CD][NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) nrm[k] = 0.0;
    for (int k = k0; k < k1; ++k) {
        tl_cam_basis<CD>(Rcw + (size_t)9 * t.order[k], tcw + (size_t)3 * t.order[k], c, blk);
#pragma unroll
        for (int r = 0; r < CD; ++r)
#pragma unroll
            for (int q = 0; q < NC; ++q) nrm[q] += blk[r][q] * blk[r][q];
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const bool ok = nrm[q] > 0.0 && isfinite(nrm[q]);
        drop[(size_t)NC * ca + q] = ok ? 0.0 : 1.0;
        nrm[q] = ok ? 1.0 / sqrt(nrm[q]) : 0.0;
    }
    for (int k = k0; k < k1; ++k) {
        const int i = t.order[k];
        tl_cam_basis<CD>(Rcw + (size_t)9 * i, tcw + (size_t)3 * i, c, blk);
#pragma unroll
        for (int r = 0; r < CD; ++r)
#pragma unroll
            for (int q = 0; q < NC; ++q) Pm[((size_t)CD * i + r) * NC + q] = blk[r][q] * nrm[q];
    }
}

// the observations of landmark slot l in the by-landmark lists: f0 + k stride, k < cnt
__device__ __forceinline__ void lm_list(const SchurLists &S, int64_t l, int64_t &f0, int64_t &cnt, int64_t &stride) {
    if (l < S.nheavy) { f0 = S.lm_ptr[l]; cnt = S.lm_ptr[l + 1] - f0; stride = 1; }
    else { const int64_t q = l - S.nheavy; f0 = S.gbase[q >> 6] + (q & 63); cnt = S.deg[l]; stride = 64; }
}
__device__ __forceinline__ constexpr int ltri(int i, int j) { return i * (i + 1) / 2 + j; }   // packed lower triangle, j <= i

// S_aa^-1 of every aggregate, a workgroup each.  Assembly: thread (li, lj), lj <= li, holds block (member li, member lj) of
//   S_ij = delta_ij U*_i - sum_l (sum_{e in (i,l)} W_e) V*_l^-1 (sum_{f in (j,l)} W_f)^T
// in registers: it walks camera i's list and, for each used observation, the list of its landmark for the observations of camera j (the pair
// walk of ba_schur_dense_kernel restricted to one partner; the 16 threads of a row read the same records) -- one writer per entry, sums in
// list order.  The lower triangle goes to LDS packed (NB (NB + 1) / 2 doubles: 37 KB at NB = 96), is factored there (Cholesky, right-looking),
// the factor inverted in place (column by column from the last) and S_aa^-1 = L^-T L^-1 written to global memory as a full symmetric block.
// Rows of absent members (a last, shorter aggregate) are identity.  A pivot that is not positive: the inverse of the diagonal (as chol_inverse).
template <int CD>
__global__ __launch_bounds__(256) void ba_tl_block_kernel(SchurLists S, BaTl t, const double *__restrict__ Jc, const double *__restrict__ Jl,
                                                          const double *__restrict__ vinv, const double *__restrict__ ustar, double *__restrict__ binv) {
    constexpr int JP = ba_jp<CD>(), NB = kBaAgg * CD, NT = NB * (NB + 1) / 2;
    static_assert(kBaAgg == 16, "thread (li, lj) = (threadIdx.x / 16, threadIdx.x % 16)");
    __shared__ double A[NT];
    __shared__ double dg[NB], colv[NB];
    const int tid = threadIdx.x, li = tid >> 4, lj = tid & 15;
    const int k0 = blockIdx.x * kBaAgg, nm = min(kBaAgg, t.nmem - k0);
    if (lj <= li) {
        double acc[CD][CD];
#pragma unroll
        for (int a = 0; a < CD; ++a)
#pragma unroll
            for (int b = 0; b < CD; ++b) acc[a][b] = (li == lj && a == b && li >= nm) ? 1.0 : 0.0;
        if (li < nm) {
            const int i = t.order[k0 + li], j = t.order[k0 + lj];
            if (li == lj) {
#pragma unroll
                for (int a = 0; a < CD; ++a)
#pragma unroll
                    for (int b = 0; b < CD; ++b) acc[a][b] = ustar[(size_t)CD * CD * i + CD * a + b];
            }
            for (int64_t e = S.cam_ptr[i]; e < S.cam_ptr[i + 1]; ++e) {
                double jp[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) jp[k] = Jc[(size_t)(JP + k) * S.nobs + e];
                if (!obs_used(jp)) continue;
                const int64_t l = S.cam_lm[e];
                int64_t f0, cnt, stride;
                lm_list(S, l, f0, cnt, stride);
                bool have = false;
                double X[CD][3];
                for (int64_t k = 0; k < cnt; ++k) {
                    const size_t f = (size_t)(f0 + k * stride);
                    if (S.lm_cam[f] != j) continue;
                    double jc2[2 * CD], jp2[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) jp2[q] = Jl[(size_t)(JP + q) * S.lm_total + f];
                    if (!obs_used(jp2)) continue;
                    if (!have) {
                        double V[3][3];
                        sym3(vinv + (size_t)6 * l, V);
#pragma unroll
                        for (int a = 0; a < CD; ++a) {
                            const double j0 = Jc[(size_t)a * S.nobs + e], j1 = Jc[(size_t)(CD + a) * S.nobs + e];
                            double w[3];
#pragma unroll
                            for (int c = 0; c < 3; ++c) w[c] = j0 * jp[c] + j1 * jp[3 + c];
#pragma unroll
                            for (int c = 0; c < 3; ++c) X[a][c] = w[0] * V[0][c] + w[1] * V[1][c] + w[2] * V[2][c];
                        }
                        have = true;
                    }
#pragma unroll
                    for (int q = 0; q < 2 * CD; ++q) jc2[q] = Jl[(size_t)q * S.lm_total + f];
#pragma unroll
                    for (int b = 0; b < CD; ++b) {
                        double w[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) w[c] = jc2[b] * jp2[c] + jc2[CD + b] * jp2[3 + c];
#pragma unroll
                        for (int a = 0; a < CD; ++a) acc[a][b] -= X[a][0] * w[0] + X[a][1] * w[1] + X[a][2] * w[2];
                    }
                }
            }
        }
#pragma unroll
        for (int a = 0; a < CD; ++a)
#pragma unroll
            for (int b = 0; b < CD; ++b) {
                const int row = CD * li + a, col = CD * lj + b;
                if (col <= row) A[ltri(row, col)] = acc[a][b];
            }
    }
    __syncthreads();
    if (tid < NB) dg[tid] = A[ltri(tid, tid)];
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    bool ok = true;
    for (int j = 0; j < NB; ++j) {   // Cholesky; every thread sees the same pivots
        double d = A[ltri(j, j)];
        if (!(d > 0.0) || !isfinite(d)) { ok = false; break; }
        d = sqrt(d);
        __syncthreads();
        if (tid < NB - j - 1) A[ltri(j + 1 + tid, j)] /= d;
        if (tid == 255) A[ltri(j, j)] = d;
        __syncthreads();
        for (int i = j + 1 + ty; i < NB; i += 16) {
            const double lij = A[ltri(i, j)];
            for (int k = j + 1 + tx; k <= i; k += 16) A[ltri(i, k)] -= lij * A[ltri(k, j)];
        }
        __syncthreads();
    }
    double *out = binv + (size_t)NB * NB * blockIdx.x;
    if (!ok) {
        for (int q = tid; q < NB * NB; q += 256) out[q] = (q / NB == q % NB && dg[q / NB] > 0.0) ? 1.0 / dg[q / NB] : 0.0;
        return;
    }
    for (int j = NB - 1; j >= 0; --j) {   // L -> L^-1 in place: column j from the inverted trailing block
        const double ajj = 1.0 / A[ltri(j, j)];
        __syncthreads();
        if (tid < NB - j - 1) colv[tid] = A[ltri(j + 1 + tid, j)];
        if (tid == 255) A[ltri(j, j)] = ajj;
        __syncthreads();
        if (tid < NB - j - 1) {
            const int i = j + 1 + tid;
            double s = 0.0;
            for (int k = j + 1; k <= i; ++k) s += A[ltri(i, k)] * colv[k - j - 1];
            A[ltri(i, j)] = -ajj * s;
        }
    }
    __syncthreads();
    for (int i = ty; i < NB; i += 16)
        for (int j = tx; j <= i; j += 16) {
            double s = 0.0;
            for (int k = i; k < NB; ++k) s += A[ltri(k, i)] * A[ltri(k, j)];
            out[(size_t)NB * i + j] = s;
            out[(size_t)NB * j + i] = s;
        }
}

// A_c = P^T S P, the lower block triangle, column-major with leading dimension ld = NC ncoarse, into a matrix the caller has zeroed.  A
// wavefront per coarse aggregate a owns block row a: it writes sum_i P_i^T U*_i P_i (and 1 on the diagonal of a dropped column), then walks
// its members' lists in order; for observation e of landmark l the lanes run over l's list, 64 at a time: lane f forms T_f = J_P,f^T J_c,f
// P_cam(f) (3 x NC), the first lane of every coarse aggregate b <= a in the batch adds those of the later lanes of b in lane order and
// subtracts (P_i^T W_e V*_l^-1) T from block (a, b).  One writer per entry, a workgroup fence between batches: fixed order, no atomics.
// Every addition's rounding error (two-sum) is collected in a second matrix lo of the same shape and added once at the end: without it an
// entry lost about sqrt(additions) ulp of P^T U* P, which A_c's own entries can be far below (rigid motions are S's near-null vectors).
template <int CD>
__global__ __launch_bounds__(256) void ba_tl_coarse_kernel(SchurLists S, BaTl t, const double *__restrict__ Jc, const double *__restrict__ Jl,
                                                           const double *__restrict__ vinv, const double *__restrict__ ustar,
                                                           const double *__restrict__ drop, double *__restrict__ Ac, double *__restrict__ lo,
                                                           int64_t ld) {
    constexpr int JP = ba_jp<CD>(), NC = ba_nc<CD>();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ca = blockIdx.x * kQwWaves + wv;
    if (ca >= t.ncoarse) return;
    int k0, k1;
    coarse_range(t, ca, k0, k1);
    double *row = Ac + (size_t)NC * ca;   // entry (NC ca + r, c) at row[r + c ld]
    double *lrow = lo + (size_t)NC * ca;  // the rounding errors of the additions to that entry (zeroed by the caller), added at the end
    if (lane < NC * NC) {
        const int r = lane / NC, c = lane % NC;
        double s = 0.0;
        for (int k = k0; k < k1; ++k) {
            const int i = t.order[k];
            const double *Pi = t.Pm + (size_t)CD * NC * i, *U = ustar + (size_t)CD * CD * i;
            for (int x = 0; x < CD; ++x) {
                double u = 0.0;
                for (int y = 0; y < CD; ++y) u += U[CD * x + y] * Pi[NC * y + c];
                s += Pi[NC * x + r] * u;
            }
        }
        if (r == c && drop[(size_t)NC * ca + r] != 0.0) s += 1.0;
        row[r + ((size_t)NC * ca + c) * ld] = s;
    }
    __threadfence_block();
    for (int km = k0; km < k1; ++km) {
        const int i = t.order[km];
        const double *Pi = t.Pm + (size_t)CD * NC * i;
        for (int64_t e = S.cam_ptr[i]; e < S.cam_ptr[i + 1]; ++e) {
            double jc[2 * CD], jp[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) jp[k] = Jc[(size_t)(JP + k) * S.nobs + e];
            if (!obs_used(jp)) continue;
#pragma unroll
            for (int k = 0; k < 2 * CD; ++k) jc[k] = Jc[(size_t)k * S.nobs + e];
            const int64_t l = S.cam_lm[e];
            double V[3][3], X[NC][3];
            sym3(vinv + (size_t)6 * l, V);
#pragma unroll
            for (int r = 0; r < NC; ++r) {
                double u0 = 0.0, u1 = 0.0, w[3];
#pragma unroll
                for (int k = 0; k < CD; ++k) { u0 += jc[k] * Pi[NC * k + r]; u1 += jc[CD + k] * Pi[NC * k + r]; }
#pragma unroll
                for (int c = 0; c < 3; ++c) w[c] = u0 * jp[c] + u1 * jp[3 + c];
#pragma unroll
                for (int c = 0; c < 3; ++c) X[r][c] = w[0] * V[0][c] + w[1] * V[1][c] + w[2] * V[2][c];
            }
            int64_t f0, cnt, stride;
            lm_list(S, l, f0, cnt, stride);
            for (int64_t kb = 0; kb < cnt; kb += 64) {
                const int nb = (int)(cnt - kb < 64 ? cnt - kb : 64);
                int b = -1;
                double T[3][NC];
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int c = 0; c < NC; ++c) T[k][c] = 0.0;
                if (lane < nb) {
                    const size_t f = (size_t)(f0 + (kb + lane) * stride);
                    double jp2[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) jp2[k] = Jl[(size_t)(JP + k) * S.lm_total + f];
                    const int jf = S.lm_cam[f], af = t.agg_of[jf];
                    const int bf = af < t.ncoarse ? af : t.ncoarse - 1;
                    if (obs_used(jp2) && af >= 0 && bf <= ca) {
                        b = bf;
                        const double *Pj = t.Pm + (size_t)CD * NC * jf;
                        double jc2[2 * CD];
#pragma unroll
                        for (int k = 0; k < 2 * CD; ++k) jc2[k] = Jl[(size_t)k * S.lm_total + f];
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            double u0 = 0.0, u1 = 0.0;
#pragma unroll
                            for (int k = 0; k < CD; ++k) { u0 += jc2[k] * Pj[NC * k + c]; u1 += jc2[CD + k] * Pj[NC * k + c]; }
#pragma unroll
                            for (int k = 0; k < 3; ++k) T[k][c] = jp2[k] * u0 + jp2[3 + k] * u1;
                        }
                    }
                }
                int rank = 0;   // earlier lanes of this batch with the same coarse aggregate
                for (int q = 0; q < nb; ++q) {
                    const int bq = __builtin_amdgcn_readlane(b, q);
                    rank += (q < lane && bq >= 0 && bq == b) ? 1 : 0;
                }
                for (int q = 1; q < nb; ++q) {   // followers in lane order into the first lane of their aggregate
                    const int bq = __builtin_amdgcn_readlane(b, q), rq = __builtin_amdgcn_readlane(rank, q);
                    if (bq < 0 || rq == 0) continue;
                    const bool take = rank == 0 && b == bq;
#pragma unroll
                    for (int k = 0; k < 3; ++k)
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            const double v = __shfl(T[k][c], q);
                            if (take) T[k][c] += v;
                        }
                }
                if (b >= 0 && rank == 0) {
                    double *blk = row + (size_t)NC * b * ld, *lob = lrow + (size_t)NC * b * ld;
#pragma unroll
                    for (int c = 0; c < NC; ++c)
#pragma unroll
                        for (int r = 0; r < NC; ++r) {   // an entry takes thousands of small terms next to P^T U* P: the sum is compensated
                            const double u = -(X[r][0] * T[0][c] + X[r][1] * T[1][c] + X[r][2] * T[2][c]), h = blk[r + (size_t)c * ld];
                            const double s = h + u, v = s - h;
                            blk[r + (size_t)c * ld] = s;
                            lob[r + (size_t)c * ld] += (h - (s - v)) + (u - v);
                        }
                }
                __threadfence_block();
            }
        }
    }
    for (int q = lane; q < NC * NC * (ca + 1); q += 64) {
        const size_t at = (size_t)(q % NC) + (size_t)(q / NC) * ld;
        row[at] += lrow[at];
    }
}
// *flag <- 1 when an entry of the n x n matrix is not finite
__global__ __launch_bounds__(256) void ba_tl_finite_kernel(int64_t count, const double *__restrict__ A, int32_t *__restrict__ flag) {
    bool bad = false;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < count; k += (int64_t)gridDim.x * 256) bad = bad || !isfinite(A[k]);
    if (bad) *flag = 1;
}

// ---- the preconditioner inside the PCG: two launches in place of ba_pcg_upd_kernel (and, with init, of ba_pcg_init_kernel).
// A workgroup per block aggregate: alpha as the update kernel forms it; x += alpha p, r -= alpha Ap for its members (init: x = 0, r = b);
// z = S_aa^-1 r (the block is symmetric: thread k reads column k, coalesced) and the aggregate's part of P^T r.
template <int CD>
__global__ __launch_bounds__(256) void ba_tl_apply_block_kernel(BaPcg a, BaTl t, int it, int init) {
    constexpr int NB = kBaAgg * CD, NC = ba_nc<CD>();
    __shared__ double sh[4];
    __shared__ double rs[NB];
    if (!init && a.st->done) return;
    double alpha = 0.0;
    if (!init) {
        const double rz = sum_partials256(a.prz[it & 1], a.grid, sh), pap = sum_partials256(a.ppap, a.cgrid, sh);
        alpha = (pap > 0.0 && rz > 0.0) ? rz / pap : 0.0;
    }
    const int tid = threadIdx.x, k0 = blockIdx.x * kBaAgg, nm = min(kBaAgg, t.nmem - k0);
    size_t j = 0;
    const bool mine = tid < NB && tid / CD < nm;
    if (tid < NB) {
        double rn = 0.0;
        if (mine) {
            j = (size_t)CD * t.order[k0 + tid / CD] + tid % CD;
            if (init) { rn = a.b[j]; a.x[j] = 0.0; }
            else { a.x[j] += alpha * a.p[j]; rn = a.r[j] - alpha * a.Ap[j]; }
            a.r[j] = rn;
        }
        rs[tid] = rn;
    }
    __syncthreads();
    if (mine) {
        const double *Bk = t.binv + (size_t)NB * NB * blockIdx.x + tid;
        double z = 0.0;
        for (int k = 0; k < CD * nm; ++k) z += Bk[(size_t)NB * k] * rs[k];
        a.z[j] = z;
    }
    if (t.use_coarse && tid >= 128 && tid < 128 + NC) {
        const int q = tid - 128;
        double s = 0.0;
        for (int k = 0; k < CD * nm; ++k) s += t.Pm[((size_t)CD * t.order[k0 + k / CD] + k % CD) * NC + q] * rs[k];
        t.gpart[(size_t)NC * blockIdx.x + q] = s;
    }
    if (init && blockIdx.x == 0 && tid == 0) { a.st->done = 0; a.st->iters = 0; a.st->relres = 1.0; }
}
// A workgroup per coarse aggregate: y = its NC rows of A_c^-1 (P^T r) (the partials of a merged last block added to its predecessor's),
// z += P y for its members, and the partials of <r, z> and |r|^2 (init: also p = z and |b|^2)
template <int CD>
__global__ __launch_bounds__(256) void ba_tl_apply_coarse_kernel(BaPcg a, BaTl t, int it, int init) {
    constexpr int NC = ba_nc<CD>();
    __shared__ double sh[4];
    __shared__ double ys[NC];
    if (!init && a.st->done) return;
    const int tid = threadIdx.x, ca = blockIdx.x;
    int k0, k1;
    coarse_range(t, ca, k0, k1);
    if (t.use_coarse) {
        const int nct = NC * t.ncoarse;
        const bool merged = t.nagg != t.ncoarse;
        for (int q = 0; q < NC; ++q) {
            const double *row = t.ainv + (size_t)(NC * ca + q) * nct;
            double v = 0.0;
            for (int c = tid; c < nct; c += 256) {
                double g = t.gpart[c];
                if (merged && c >= nct - NC) g += t.gpart[c + NC];
                v += row[c] * g;
            }
            v = block_sum256(v, sh);
            if (tid == 0) ys[q] = v;
        }
        __syncthreads();
    }
    double rz = 0.0, rr = 0.0;
    if (tid < (k1 - k0) * CD) {
        const size_t j = (size_t)CD * t.order[k0 + tid / CD] + tid % CD;
        double z = a.z[j];
        if (t.use_coarse) {
#pragma unroll
            for (int q = 0; q < NC; ++q) z += t.Pm[j * NC + q] * ys[q];
            a.z[j] = z;
        }
        if (init) a.p[j] = z;
        const double r = a.r[j];
        rz = r * z; rr = r * r;
    }
    rz = block_sum256(rz, sh);
    rr = block_sum256(rr, sh);
    if (tid == 0) {
        if (init) { a.prz[0][ca] = rz; a.pbb[ca] = rr; a.prr[ca] = rr; }
        else { a.prz[(it & 1) ^ 1][ca] = rz; a.prr[ca] = rr; }
    }
}

constexpr const char *kStage = "bundle adjustment";

// the caller's parameters in the device layouts: Rcw = R_i^T (row-major), tcw = -R_i^T t_i, P by landmark slot
void to_device_layout(const SchurOp &SO, const double *rot, const double *t, const double *p, std::vector<double> &hR, std::vector<double> &hT,
                      std::vector<double> &hP) {
    const std::vector<int32_t> &slot_of = SO.slot_of();
    const int64_t n = SO.lists().n, m = SO.lists().m;
    hR.assign((size_t)9 * n, 0.0); hT.assign((size_t)3 * n, 0.0); hP.assign((size_t)3 * m, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) hR[(size_t)9 * i + 3 * a + c] = rot[(size_t)c + 3 * ((size_t)3 * i + a)];
        for (int a = 0; a < 3; ++a) {
            double s = 0.0;
            for (int c = 0; c < 3; ++c) s += hR[(size_t)9 * i + 3 * a + c] * t[(size_t)3 * i + c];
            hT[(size_t)3 * i + a] = -s;
        }
    }
    for (int64_t l = 0; l < m; ++l)
        for (int a = 0; a < 3; ++a) hP[(size_t)3 * slot_of[(size_t)l] + a] = p[(size_t)3 * l + a];
}
// and the cameras back: R_i = Rcw^T, t_i = -R_i tcw for the cameras whose cused is set, the others left as they are (rot or t null: not written)
void from_device_layout(int64_t n, const std::vector<double> &hR, const std::vector<double> &hT, const std::vector<int32_t> &cused, double *rot,
                        double *t) {
    for (int64_t i = 0; i < n; ++i) {
        if (!cused[(size_t)i]) continue;
        const double *Rc = &hR[(size_t)9 * i], *tc = &hT[(size_t)3 * i];
        for (int a = 0; a < 3; ++a) {
            if (rot)
                for (int c = 0; c < 3; ++c) rot[(size_t)a + 3 * ((size_t)3 * i + c)] = Rc[3 * c + a];
            if (t) t[(size_t)3 * i + a] = -(Rc[a] * tc[0] + Rc[3 + a] * tc[1] + Rc[6 + a] * tc[2]);
        }
    }
}

// One linearisation's device state and the launches on it: the workspace, the eval / landmark / camera passes, the preconditioner's
// set-up, the product S x, the dense assembly, the PCG's start and the candidate block.  run() (the LM loop) and probe() (the test export
// xm_ctx_ba_probe) both go through these members, so the probe launches what the loop launches: same kernels, grids and arguments.
template <int CD>
struct BaWork {
    static constexpr int NP = ba_planes<CD>(), NC = ba_nc<CD>(), NB = kBaAgg * CD;
    const SchurOp &SO;
    const BaSettings &cfg;
    hipStream_t st;
    const SchurLists S;
    const int64_t n, m, nobs;
    std::vector<double> hR, hT, hP;
    // ---- parameters on the device; three sets with non-monotonic steps (current, candidate, least cost so far), two otherwise
    DevBuf<double> R[3], T[3], P[3];
    DevBuf<double> G[3];        // with a focal column: the focal scales of each set
    DevBuf<uint8_t> gfree;      // the mask of the free focals (not allocated: all free)
    DevBuf<double> Kd[3];       // with a distortion column: the radial coefficients of each set
    DevBuf<uint8_t> kfree;      // the mask of the free coefficients (not allocated: all free)
    // ---- focal groups (cfg.ngroups > 0): G[] and gfree above are the groups' values copied to every member, so that the eval, candidate and
    // cost kernels read them as they read per-camera ones; the member lists (host counting sort, once per call) and the groups' arrays
    const bool grouped;
    const int64_t ng;
    std::vector<int32_t> h_rep;   // group -> representative, -1: empty
    BaGroups grp{};
    DevBuf<int32_t> grp_off, grp_mem, grp_rep, grp_list, grp_of, grp_repof, grp_moving;
    DevBuf<uint8_t> grp_free;
    DevBuf<double> grp_D, grp_F, grp_new, fstat, pe;   // pe: an expanded vector (the product's E p, the candidate's E dc)
    int ggrp = 0, ggf = 0;        // workgroups of the group sums; of the flat kernel over the groups
    // at most XM_BA_FOCAL_GROUPS_EXACT groups: the preconditioner's focal block is the exact F = S_shared[focal, focal] (G products per LM
    // iteration), inverted by spd_inverse_device; a failed factorisation leaves that iteration with diag F and is counted in
    // coarse_fallbacks
    bool f_small = false, f_exact = false;
    DevBuf<double> grp_Fm, grp_Fx, grp_Fcopy, grp_T, grp_U;   // F -> F^-1, the inverse's scratch, F as assembled; the dense contraction's sums
    DevBuf<int32_t> grp_flag;
    // ---- workspace (zero: the padding of the packed landmark lists stays 0 in every plane)
    DevBuf<double> Jc, Jl, vinv, gl, ustar, sinv, b, x, r, z, pv, Ap, y, dP, parts;
    DevBuf<int32_t> lused, cused, state_buf;
    BaState *dst = nullptr;
    Pinned<BaState> hs;
    int ge = 0, gfc = 0, gfl = 0, gcam = 0, glm = 0;
    size_t o_eval = 0, o_gmax = 0, o_pcg = 0, o_cand = 0, o_cost = 0;
    double *pp = nullptr;
    const dim3 b256{256}, blm{kBaHeavyThreads};
    int cur = 0, best = 0;   // the current point and the one of least cost so far (the same one without non-monotonic steps)
    BaPcg a;
    // opt-in preconditioners: the plan from the used observations (host, once), the blocks and the coarse operator (device, allocated here
    // and freed with the workspace).  atl: the PCG's arguments with the partial sums of <r, z>, |r|^2 and |b|^2 by coarse aggregate
    bool tlmode = false;
    BaTl tl{};
    BaPcg atl;
    DevBuf<int32_t> tl_order, tl_agg, tl_flag;
    DevBuf<double> tl_binv, tl_P, tl_drop, tl_gpart, tl_parts, tl_A, tl_X;
    int64_t nct = 0;
    bool basis_stale = true;   // P belongs to the current point: recomputed after every accepted step
    int coarse_fallbacks = 0;
    double *ac_copy = nullptr;   // probe only: A_c as assembled (device, nct x nct), copied before it is inverted in place
    // dense Schur: the CD n x CD n matrix, allocated here and freed with the workspace; the substitutions' scratch vector
    const int64_t nd;
    DevBuf<double> Sd, ysub;

    BaWork(const SchurOp &SO_, const BaSettings &cfg_, const double *rot, const double *t, const double *p, hipStream_t st_, bool dense)
        : SO(SO_), cfg(cfg_), st(st_), S(SO_.lists()), n(S.n), m(S.m), nobs(S.nobs), grouped(ba_can_group<CD>() && cfg_.ngroups > 0),
          ng(grouped ? cfg_.ngroups : 0), nd((int64_t)CD * S.n) {
        to_device_layout(SO, rot, t, p, hR, hT, hP);
        const bool nonmono = cfg.nonmonotonic;
        for (int k = 0; k < (nonmono ? 3 : 2); ++k) { R[k].alloc((size_t)9 * n, false); T[k].alloc((size_t)3 * n, false); P[k].alloc((size_t)3 * m, false); }
        XM_HIP_CHECK(hipMemcpyAsync(R[0].p, hR.data(), hR.size() * sizeof(double), hipMemcpyHostToDevice, st));
        XM_HIP_CHECK(hipMemcpyAsync(T[0].p, hT.data(), hT.size() * sizeof(double), hipMemcpyHostToDevice, st));
        XM_HIP_CHECK(hipMemcpyAsync(P[0].p, hP.data(), hP.size() * sizeof(double), hipMemcpyHostToDevice, st));
        if constexpr (ba_has_focal<CD>()) {
            for (int k = 0; k < (nonmono ? 3 : 2); ++k) G[k].alloc((size_t)n, false);
            if (grouped) {
                plan_groups();
            } else {
                XM_HIP_CHECK(hipMemcpyAsync(G[0].p, cfg.focal, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
                if (cfg.focal_free) {
                    gfree.alloc((size_t)n, false);
                    XM_HIP_CHECK(hipMemcpyAsync(gfree.p, cfg.focal_free, (size_t)n, hipMemcpyHostToDevice, st));
                }
            }
        }
        if constexpr (ba_has_dist<CD>()) {
            for (int k = 0; k < (nonmono ? 3 : 2); ++k) Kd[k].alloc((size_t)n, false);
            XM_HIP_CHECK(hipMemcpyAsync(Kd[0].p, cfg.dist, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
            if (cfg.dist_free) {
                kfree.alloc((size_t)n, false);
                XM_HIP_CHECK(hipMemcpyAsync(kfree.p, cfg.dist_free, (size_t)n, hipMemcpyHostToDevice, st));
            }
        }
        Jc.alloc((size_t)NP * nobs); Jl.alloc((size_t)NP * S.lm_total);
        vinv.alloc((size_t)6 * m); gl.alloc((size_t)3 * m); y.alloc((size_t)3 * m); dP.alloc((size_t)3 * m); lused.alloc((size_t)m);
        ustar.alloc((size_t)CD * CD * n); sinv.alloc((size_t)CD * CD * n); cused.alloc((size_t)n);
        for (DevBuf<double> *v : {&b, &x, &r, &z, &pv, &Ap}) v->alloc((size_t)CD * n);
        state_buf.alloc(sizeof(BaState) / sizeof(int32_t) + 2);
        dst = reinterpret_cast<BaState *>(state_buf.p);
        ge = flat_grid(nobs); gfc = flat_grid(n); gfl = flat_grid(m); gcam = qw_grid((int)n);
        glm = (int)(S.nheavy + (m - S.nheavy + kBaHeavyThreads - 1) / kBaHeavyThreads);
        // partials: eval (2 ge) | gmax (glm + gcam) | PCG (4 gfc + gcam) | candidate step / |x| (cameras then landmarks, 2 x (gfc + gfl)) | cost (2 ge)
        // (focal groups: ggrp more behind the cameras' gmax and <p, Ap> partials, ggf more behind each of the cameras' candidate sums)
        // (and one more partial behind each of the PCG's four sums: <r, z> of the exact focal block; the others stay 0)
        const int gx = grouped ? 1 : 0;
        o_eval = 0; o_gmax = o_eval + 2 * (size_t)ge; o_pcg = o_gmax + glm + gcam + ggrp; o_cand = o_pcg + 4 * ((size_t)gfc + gx) + gcam + ggrp;
        o_cost = o_cand + 2 * ((size_t)gfc + ggf + gfl);
        const size_t n_parts = o_cost + 2 * (size_t)ge;
        parts.alloc(n_parts);
        pp = parts.p;
        a.n = n; a.grid = gfc + gx; a.cgrid = gcam + ggrp; a.tol2 = cfg.eta * cfg.eta;
        a.b = b.p; a.sinv = sinv.p; a.ustar = ustar.p; a.x = x.p; a.r = r.p; a.z = z.p; a.p = pv.p; a.Ap = Ap.p;
        a.lay_partials(pp + o_pcg);
        a.st = dst;
        tlmode = cfg.precond != 0;
        atl = a;
        if (tlmode) plan_aggregates();
        if (dense) {
            if (nd > XM_BA_DENSE_MAX_ROWS) throw Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: the dense Schur system has more than XM_BA_DENSE_MAX_ROWS rows");
            const size_t elems = (size_t)nd * (size_t)nd;
            if (hipMalloc((void **)&Sd.p, elems * sizeof(double)) != hipSuccess) {
                (void)hipGetLastError();
                Sd.p = nullptr;
                throw Error(XM_ERR_NOMEM, "xm_ctx_bundle_adjust: no device memory for the dense Schur system (" + std::to_string(elems * 8 >> 20) + " MB)");
            }
            Sd.count = Sd.capacity = elems;
            ysub.alloc((size_t)nd);
            if (grouped) { grp_T.alloc((size_t)ng * nd, false); grp_U.alloc((size_t)ng * ng, false); }
        }
    }
    // the member lists by a counting sort (members ascending, the first one the representative), the groups' values and mask copied to the
    // members, the order in which the workgroups of the group sums take the groups
    void plan_groups() {
        std::vector<int32_t> off((size_t)ng + 1, 0), mem((size_t)n), repof((size_t)n), list;
        for (int64_t i = 0; i < n; ++i) off[(size_t)cfg.group_of[i] + 1]++;
        for (int64_t c = 0; c < ng; ++c) off[(size_t)c + 1] += off[(size_t)c];
        {
            std::vector<int32_t> at(off.begin(), off.end() - 1);
            for (int64_t i = 0; i < n; ++i) mem[(size_t)at[(size_t)cfg.group_of[i]]++] = (int32_t)i;
        }
        h_rep.assign((size_t)ng, -1);
        for (int64_t c = 0; c < ng; ++c)
            if (off[(size_t)c + 1] > off[(size_t)c]) h_rep[(size_t)c] = mem[(size_t)off[(size_t)c]];
        int64_t nsmall = 0;
        for (int pass = 0; pass < 2; ++pass) {
            for (int64_t c = 0; c < ng; ++c)
                if ((off[(size_t)c + 1] - off[(size_t)c] <= kBaGroupThread) == (pass == 0)) list.push_back((int32_t)c);
            if (pass == 0) nsmall = (int64_t)list.size();
        }
        std::vector<double> hG((size_t)n);
        std::vector<uint8_t> hfree((size_t)n, 1);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t c = cfg.group_of[i];
            repof[(size_t)i] = h_rep[(size_t)c];
            hG[(size_t)i] = cfg.focal[c];
            if (cfg.focal_free) hfree[(size_t)i] = cfg.focal_free[c];
        }
        auto up = [&](auto &buf, const auto &v) {
            buf.alloc(v.size(), false);
            XM_HIP_CHECK(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, st));
        };
        up(grp_off, off); up(grp_mem, mem); up(grp_rep, h_rep); up(grp_list, list); up(grp_repof, repof); up(G[0], hG);
        grp_of.alloc((size_t)n, false);
        XM_HIP_CHECK(hipMemcpyAsync(grp_of.p, cfg.group_of, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (cfg.focal_free) {
            up(gfree, hfree);
            grp_free.alloc((size_t)ng, false);
            XM_HIP_CHECK(hipMemcpyAsync(grp_free.p, cfg.focal_free, (size_t)ng, hipMemcpyHostToDevice, st));
        }
        wait_stream(st, cfg.watchdog_s, kStage, "the focal groups");   // the host vectors above end with this function
        grp_D.alloc((size_t)ng); grp_F.alloc((size_t)ng); grp_new.alloc((size_t)ng); grp_moving.alloc((size_t)ng);
        fstat.alloc((size_t)2 * n); pe.alloc((size_t)CD * n);
        const int nsb = (int)((nsmall + 255) / 256);
        grp.ng = (int32_t)ng; grp.nsmall = (int32_t)nsmall; grp.nsb = nsb;
        grp.off = grp_off.p; grp.mem = grp_mem.p; grp.rep = grp_rep.p; grp.list = grp_list.p; grp.free = grp_free.p;
        ggrp = nsb + (int)(ng - nsmall);
        ggf = flat_grid(ng);
        f_small = ng <= XM_BA_FOCAL_GROUPS_EXACT;
        if (ng <= XM_BA_FOCAL_GROUPS_EXACT) {
            grp_Fm.alloc((size_t)ng * ng); grp_Fx.alloc((size_t)ng * ng); grp_Fcopy.alloc((size_t)ng * ng); grp_flag.alloc(1);
        }
    }
    void plan_aggregates() {
        std::vector<int32_t> hc((size_t)nobs), hl((size_t)nobs), order;
        std::vector<int64_t> hpos((size_t)nobs);
        std::vector<double> hw((size_t)nobs), hp3((size_t)3 * nobs);
        XM_HIP_CHECK(hipMemcpyAsync(hc.data(), S.obs_cam, (size_t)nobs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(hl.data(), S.obs_lm, (size_t)nobs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(hpos.data(), S.pos_c, (size_t)nobs * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(hw.data(), S.cam_w, (size_t)nobs * sizeof(double), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(hp3.data(), S.obs_p, (size_t)3 * nobs * sizeof(double), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the observation lists");
        std::vector<uint8_t> used((size_t)nobs);
        for (int64_t e = 0; e < nobs; ++e) used[(size_t)e] = (hw[(size_t)hpos[(size_t)e]] > 0.0 && hp3[(size_t)3 * e + 2] > 0.0) ? 1 : 0;
        ba_aggregate_plan(n, nobs, hc.data(), hl.data(), used.data(), kBaAgg, order);
        const int64_t nmem = (int64_t)order.size();
        if (nmem == 0) { tlmode = false; return; }   // no used observation: nothing to precondition (b = 0, the PCG stops at once)
        const int64_t nagg = (nmem + kBaAgg - 1) / kBaAgg, ncoarse = (nagg > 1 && nmem - (nagg - 1) * kBaAgg < 2) ? nagg - 1 : nagg;
        nct = NC * ncoarse;
        std::vector<int32_t> agg((size_t)n, -1);
        for (int64_t k = 0; k < nmem; ++k) agg[(size_t)order[(size_t)k]] = (int32_t)(k / kBaAgg);
        auto try_alloc = [&](DevBuf<double> &buf, size_t elems, const char *what) {
            if (hipMalloc((void **)&buf.p, elems * sizeof(double)) != hipSuccess) {
                (void)hipGetLastError();
                buf.p = nullptr;
                throw Error(XM_ERR_NOMEM, std::string("xm_ctx_bundle_adjust: no device memory for ") + what + " (" + std::to_string(elems * 8 >> 20) + " MB)");
            }
            buf.count = buf.capacity = elems;
        };
        tl_order.alloc((size_t)nmem, false); tl_agg.alloc((size_t)n, false); tl_flag.alloc(1);
        XM_HIP_CHECK(hipMemcpyAsync(tl_order.p, order.data(), (size_t)nmem * sizeof(int32_t), hipMemcpyHostToDevice, st));
        XM_HIP_CHECK(hipMemcpyAsync(tl_agg.p, agg.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the aggregate plan");
        try_alloc(tl_binv, (size_t)nagg * NB * NB, "the preconditioner's blocks");
        tl_parts.alloc(4 * (size_t)ncoarse);
        if (cfg.precond == 2) {
            tl_P.alloc((size_t)n * CD * NC); tl_drop.alloc((size_t)nct); tl_gpart.alloc((size_t)(nagg + 1) * NC);
            try_alloc(tl_A, (size_t)nct * nct, "the coarse operator");
            try_alloc(tl_X, (size_t)nct * nct, "the coarse operator's inverse");
        }
        tl.nagg = (int32_t)nagg; tl.ncoarse = (int32_t)ncoarse; tl.nmem = (int32_t)nmem; tl.use_coarse = 0;
        tl.order = tl_order.p; tl.agg_of = tl_agg.p; tl.binv = tl_binv.p; tl.Pm = tl_P.p; tl.ainv = tl_A.p; tl.gpart = tl_gpart.p;
        atl.grid = (int)ncoarse;
        atl.prz[0] = tl_parts.p; atl.prz[1] = tl_parts.p + ncoarse; atl.prr = tl_parts.p + 2 * ncoarse; atl.pbb = tl_parts.p + 3 * ncoarse;
    }
    void reduce(BaReduce rd) { hipLaunchKernelGGL(ba_reduce_kernel, dim3(1), b256, 0, st, rd); }
    BaState read_state(const char *what) { return xm::read_state(dst, hs, st, cfg.watchdog_s, kStage, what); }
    // f(GR): `grouped` as a compile-time constant (the grouped kernels exist for a camera block with a focal column only)
    template <class F>
    void by_grouping(F &&f) {
        if constexpr (ba_can_group<CD>()) {
            if (grouped) return f(std::true_type{});
        }
        f(std::false_type{});
    }
    void eval() {
        with_loss(cfg.loss, [&](auto L) {   // G[] and gfree are not allocated (null) without a focal column, Kd[] and kfree without a distortion column
            hipLaunchKernelGGL((ba_eval_kernel<CD, L.value>), dim3(ge), b256, 0, st, S, (const double *)R[cur].p, (const double *)T[cur].p,
                               (const double *)P[cur].p, (const double *)G[cur].p, (const uint8_t *)gfree.p, (const double *)Kd[cur].p,
                               (const uint8_t *)kfree.p, Jc.p, Jl.p, pp + o_eval, cfg.loss_scale);
        });
        BaReduce rd{};
        rd.sum_p[0] = pp + o_eval; rd.sum_n[0] = ge; rd.sum_out[0] = &dst->cost;
        rd.sum_p[1] = pp + o_eval + ge; rd.sum_n[1] = ge; rd.sum_out[1] = &dst->used;
        reduce(rd);
    }
    void passes(double mu) {
        hipLaunchKernelGGL((ba_lm_kernel<CD>), dim3(glm), blm, 0, st, S, (const double *)Jl.p, mu, vinv.p, gl.p, lused.p, pp + o_gmax);
        by_grouping([&](auto GR) {   // fstat: allocated with the groups, null without
            hipLaunchKernelGGL((ba_cam_kernel<CD, GR.value>), dim3(gcam), b256, 0, st, S, (const double *)Jc.p, (const double *)vinv.p,
                               (const double *)gl.p, mu, ustar.p, sinv.p, b.p, cused.p, pp + o_gmax + glm, fstat.p);
        });
        if constexpr (ba_can_group<CD>()) {
            if (grouped) {   // the groups' pass: their gradient entries join the maximum
                hipLaunchKernelGGL((ba_group_setup_kernel<CD>), dim3(ggrp), b256, 0, st, grp, (const double *)ustar.p, (const double *)fstat.p,
                                   (const int32_t *)cused.p, mu, b.p, sinv.p, grp_D.p, grp_F.p, grp_moving.p, pp + o_gmax + glm + gcam);
                cur_mu = mu;
            }
        }
        BaReduce rd{};
        rd.max_p = pp + o_gmax; rd.max_n = glm + gcam + ggrp; rd.max_out = &dst->gmax;   // (ggrp = 0 without groups)
        reduce(rd);
        f_exact = false;
        if (grouped && f_small && !dense_mode) exact_focal_block();
    }
    double cur_mu = 0.0;   // focal groups: the damping of the last passes (mu D_c x_c joins in the group sum)
    bool dense_mode = false;   // the dense solver runs no PCG: no preconditioner to set up
    // F by G products with indicator vectors (through the PCG's direction and product vectors, which the PCG's start fills anew), its inverse
    void exact_focal_block() {
        if constexpr (ba_can_group<CD>()) {
            XM_HIP_CHECK(hipMemsetAsync(&dst->done, 0, sizeof(int32_t), st));   // the last solve's flag would skip the camera side of the product
            const int G = (int)ng;
            for (int d = 0; d < G; ++d) {
                if (h_rep[(size_t)d] >= 0) {
                    hipLaunchKernelGGL(ba_group_unit_kernel, dim3(flat_grid(nd)), b256, 0, st, nd, (int64_t)CD * h_rep[(size_t)d] + ba_fidx<CD>(), pv.p);
                    sx(a, nullptr);
                }
                hipLaunchKernelGGL((ba_group_col_kernel<CD>), dim3(ggf), b256, 0, st, grp, d, (const double *)Ap.p, (const double *)grp_D.p, cur_mu, grp_Fm.p);
            }
            XM_HIP_CHECK(hipMemcpyAsync(grp_Fcopy.p, grp_Fm.p, grp_Fm.count * sizeof(double), hipMemcpyDeviceToDevice, st));
            XM_HIP_CHECK(hipMemsetAsync(grp_flag.p, 0, sizeof(int32_t), st));
            check_launch("the exact focal block");
            bool ok = spd_inverse_device(G, grp_Fm.p, grp_Fx.p, st);
            if (ok) {
                spd_inverse_layout(G, grp_Fx.p, grp_Fm.p, G, st);
                hipLaunchKernelGGL(ba_tl_finite_kernel, dim3(1), b256, 0, st, (int64_t)G * G, (const double *)grp_Fm.p, grp_flag.p);
                int32_t bad = 0;
                XM_HIP_CHECK(hipMemcpyAsync(&bad, grp_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                wait_stream(st, cfg.watchdog_s, kStage, "the focal block's inverse");
                ok = bad == 0;
            }
            if (ok) {
                hipLaunchKernelGGL((ba_group_exact_on_kernel<CD>), dim3(ggf), b256, 0, st, grp, sinv.p);
                f_exact = true;
            } else {
                coarse_fallbacks++;
            }
        }
    }
    // behind the PCG's start (init) or the update of iteration it: the exact focal block's part of z
    void focal_precond(int it, int init) {
        if constexpr (ba_can_group<CD>())
            hipLaunchKernelGGL((ba_group_precond_kernel<CD>), dim3(1), b256, 0, st, grp, (const double *)grp_Fm.p, a, it, init, f_exact ? 1 : 0);
    }
    void pcg_update(int it) {
        hipLaunchKernelGGL((ba_pcg_upd_kernel<CD>), dim3(gfc), b256, 0, st, a, it);
        focal_precond(it, 0);
    }
    // pe = E src
    void expand(const double *src, const BaState *gate) {
        if constexpr (ba_can_group<CD>())
            hipLaunchKernelGGL((ba_group_expand_kernel<CD>), dim3(flat_grid(n * CD)), b256, 0, st, n, (const int32_t *)grp_repof.p, src, pe.p, gate);
    }
    // every LM iteration (S changes with mu): the block inverses; two-level: A_c = P^T S P and its inverse.  A_c that cannot be inverted (a
    // pivot that is not positive, an entry that is not finite): this iteration's PCG runs with the blocks alone
    void precond_setup() {
        if constexpr (ba_has_focal<CD>()) return;   // refused before the workspace is made: the ba_tl_* kernels are not instantiated for CD = 7 / 4
        else precond_setup_launches();
    }
    void precond_setup_launches() {
        hipLaunchKernelGGL((ba_tl_block_kernel<CD>), dim3((unsigned)tl.nagg), b256, 0, st, S, tl, (const double *)Jc.p, (const double *)Jl.p,
                           (const double *)vinv.p, (const double *)ustar.p, tl_binv.p);
        tl.use_coarse = 0;
        if (cfg.precond != 2) return;
        if (basis_stale) {
            hipLaunchKernelGGL((ba_tl_basis_kernel<CD>), dim3((unsigned)((tl.ncoarse + 255) / 256)), b256, 0, st, tl, (const double *)R[cur].p,
                               (const double *)T[cur].p, tl_P.p, tl_drop.p);
            basis_stale = false;
        }
        XM_HIP_CHECK(hipMemsetAsync(tl_A.p, 0, tl_A.count * sizeof(double), st));
        XM_HIP_CHECK(hipMemsetAsync(tl_X.p, 0, tl_X.count * sizeof(double), st));   // the assembly's error terms; the inverse is written over them
        XM_HIP_CHECK(hipMemsetAsync(tl_flag.p, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL((ba_tl_coarse_kernel<CD>), dim3((unsigned)((tl.ncoarse + kQwWaves - 1) / kQwWaves)), b256, 0, st, S, tl, (const double *)Jc.p,
                           (const double *)Jl.p, (const double *)vinv.p, (const double *)ustar.p, (const double *)tl_drop.p, tl_A.p, tl_X.p, nct);
        check_launch("the two-level preconditioner");
        if (ac_copy) XM_HIP_CHECK(hipMemcpyAsync(ac_copy, tl_A.p, tl_A.count * sizeof(double), hipMemcpyDeviceToDevice, st));
        bool ok = spd_inverse_device((int)nct, tl_A.p, tl_X.p, st);
        if (ok) {
            spd_inverse_layout((int)nct, tl_X.p, tl_A.p, nct, st);
            hipLaunchKernelGGL(ba_tl_finite_kernel, dim3((unsigned)std::min<int64_t>(1024, (nct * nct + 255) / 256)), b256, 0, st, nct * nct, (const double *)tl_A.p,
                               tl_flag.p);
            int32_t bad = 0;
            XM_HIP_CHECK(hipMemcpyAsync(&bad, tl_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            wait_stream(st, cfg.watchdog_s, kStage, "the coarse operator's inverse");
            ok = bad == 0;
        }
        if (ok) tl.use_coarse = 1;
        else coarse_fallbacks++;
    }
    // ar.Ap = S ar.p through the two lists (the PCG's product; gate: the state word whose done flag skips the landmark side, or null)
    void sx(const BaPcg &ar, const BaState *gate) {
        BaPcg ae = ar;   // focal groups: S_shared x = E^T S_7 (E x) + mu D x -- the two list passes read E x
        if (grouped) { expand(ar.p, gate); ae.p = pe.p; }
        hipLaunchKernelGGL((ba_lmx_kernel<CD>), dim3(glm), blm, 0, st, S, (const double *)Jl.p, (const double *)vinv.p, (const double *)nullptr, 1.0,
                           (const int32_t *)lused.p, (const double *)ae.p, gate, y.p);
        hipLaunchKernelGGL((ba_camx_kernel<CD>), dim3(gcam), b256, 0, st, S, (const double *)Jc.p, (const double *)y.p, ae);
        if constexpr (ba_can_group<CD>()) {
            if (grouped) {
                hipLaunchKernelGGL((ba_group_sum_kernel<CD>), dim3(ggrp), b256, 0, st, grp, (const double *)grp_D.p, cur_mu, (const double *)ar.p,
                                   ar.Ap, ar.ppap + gcam, gate);
            }
        }
    }
    // the dense lower block triangle of S into Sd (zeroed here), the failure flag cleared
    void dense_assemble() {
        XM_HIP_CHECK(hipMemsetAsync(Sd.p, 0, Sd.count * sizeof(double), st));
        XM_HIP_CHECK(hipMemsetAsync(&dst->fail, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL((ba_schur_dense_kernel<CD>), dim3(gcam), b256, 0, st, S, (const double *)Jc.p, (const double *)Jl.p, (const double *)vinv.p,
                           (const double *)ustar.p, Sd.p, nd);
        if constexpr (ba_can_group<CD>()) {
            if (grouped) {   // S_shared = E^T S_7 E + mu D in place
                hipLaunchKernelGGL((ba_group_dense_rows_kernel<CD>), dim3(flat_grid(ng * nd)), b256, 0, st, grp, Sd.p, nd, nd, grp_T.p);
                hipLaunchKernelGGL((ba_group_dense_cols_kernel<CD>), dim3((unsigned)((ng * ng + 255) / 256)), b256, 0, st, grp, nd, (const double *)grp_T.p,
                                   grp_U.p);
                hipLaunchKernelGGL((ba_group_dense_clear_kernel<CD>), dim3(flat_grid(n * nd)), b256, 0, st, n, Sd.p, nd, nd);
                hipLaunchKernelGGL((ba_group_dense_write_kernel<CD>), dim3(flat_grid(ng * nd + ng * ng)), b256, 0, st, grp, Sd.p, nd, nd,
                                   (const double *)grp_T.p, (const double *)grp_U.p, (const double *)grp_D.p, cur_mu);
            }
        }
    }
    // S dc = b exactly: assembly, Cholesky, substitutions (dc -> x); then |b - S dc|^2 and |b|^2 with S applied through the matrix-free
    // kernels of the PCG (the state word's done flag is never set on this path).  Nothing is read by the host here.
    void dense_solve() {
        dense_assemble();
        spd_cholesky_device((int)nd, Sd.p, nd, &dst->fail, st);
        XM_HIP_CHECK(hipMemcpyAsync(x.p, b.p, (size_t)nd * sizeof(double), hipMemcpyDeviceToDevice, st));
        spd_substitute_device((int)nd, Sd.p, nd, x.p, ysub.p, nd, 1, &dst->fail, st);
        BaPcg ar = a;
        ar.p = x.p;
        sx(ar, nullptr);
        hipLaunchKernelGGL((ba_dense_res_kernel<CD>), dim3(gfc), b256, 0, st, n, (const double *)b.p, (const double *)Ap.p, pp + o_pcg);
        BaReduce rd{};
        rd.sum_p[0] = pp + o_pcg; rd.sum_n[0] = gfc; rd.sum_out[0] = &dst->res2[0];
        rd.sum_p[1] = pp + o_pcg + gfc; rd.sum_n[1] = gfc; rd.sum_out[1] = &dst->res2[1];
        reduce(rd);
    }
    const BaPcg &pcg_args() const { return tlmode ? atl : a; }
    // the update of iteration it (or the start) with M^-1 = blocks [+ coarse]
    void precond(int it, int init) {
        if constexpr (!ba_has_focal<CD>()) {
            hipLaunchKernelGGL((ba_tl_apply_block_kernel<CD>), dim3((unsigned)tl.nagg), b256, 0, st, atl, tl, it, init);
            hipLaunchKernelGGL((ba_tl_apply_coarse_kernel<CD>), dim3((unsigned)tl.ncoarse), b256, 0, st, atl, tl, it, init);
        }
    }
    // the PCG's start: x = 0, r = b, z = M^-1 b, p = z and the first partial sums
    void pcg_start() {
        if (tlmode) precond(0, 1);
        else hipLaunchKernelGGL((ba_pcg_init_kernel<CD>), dim3(gfc), b256, 0, st, a);
        if (grouped && f_small) focal_precond(0, 1);
    }
    // back-substitution dP = -V*^-1 (g + W^T dc), candidate (parameter set nx), its cost and the model decrease; the scalars to the state word
    void candidate(int nx, const double *dc) {
        const double *dshared = dc;   // focal groups: the step before the expansion; every kernel below but the groups' reads E dc
        if (grouped) { expand(dc, nullptr); dc = pe.p; }
        const int gfg = gfc + ggf;
        hipLaunchKernelGGL((ba_lmx_kernel<CD>), dim3(glm), blm, 0, st, S, (const double *)Jl.p, (const double *)vinv.p, (const double *)gl.p, -1.0,
                           (const int32_t *)lused.p, dc, (const BaState *)nullptr, dP.p);
        if constexpr (ba_has_focal<CD>()) {
            XM_HIP_CHECK(hipMemsetAsync(&dst->bad_focal, 0, sizeof(int32_t), st));
            if constexpr (ba_can_group<CD>()) {
                if (grouped)
                    hipLaunchKernelGGL((ba_group_cand_kernel<CD>), dim3(ggf), b256, 0, st, grp, (const double *)G[cur].p, dshared,
                                       (const int32_t *)grp_moving.p, grp_new.p, dst, pp + o_cand + gfc, gfg);
            }
        }
        by_grouping([&](auto GR) {   // G[], gfree, Kd[], kfree and the groups' arrays: null where there are none
            hipLaunchKernelGGL((ba_cand_cam_kernel<CD, GR.value>), dim3(gfc), b256, 0, st, n, (const double *)R[cur].p, (const double *)T[cur].p,
                               (const double *)G[cur].p, (const uint8_t *)gfree.p, dc, (const int32_t *)cused.p, R[nx].p, T[nx].p, G[nx].p,
                               dst, pp + o_cand, (const int32_t *)grp_of.p, (const double *)grp_new.p, gfg, (const double *)Kd[cur].p,
                               (const uint8_t *)kfree.p, Kd[nx].p);
        });
        hipLaunchKernelGGL(ba_cand_vec_kernel<3>, dim3(gfl), b256, 0, st, m, (const double *)P[cur].p, (const double *)dP.p, (const int32_t *)lused.p,
                           P[nx].p, pp + o_cand + 2 * (size_t)gfg);
        with_loss(cfg.loss, [&](auto L) {
            hipLaunchKernelGGL((ba_cost_kernel<CD, L.value>), dim3(ge), b256, 0, st, S, (const double *)R[nx].p, (const double *)T[nx].p,
                               (const double *)P[nx].p, (const double *)G[nx].p, (const double *)Jc.p, dc, (const double *)dP.p, pp + o_cost,
                               cfg.loss_scale, (const double *)Kd[nx].p, dst);
        });
        reduce(candidate_sums(pp + o_cost, ge, pp + o_cand, gfg, gfl, dst));
    }
};

template <int CD>
void run(const SchurOp &SO, const BaSettings &cfg, double *rot, double *t, double *p, BaOutcome &out, hipStream_t st) {
    const auto t_start = std::chrono::steady_clock::now();
    BaWork<CD> W(SO, cfg, rot, t, p, st, cfg.dense_schur);
    const std::vector<int32_t> &slot_of = SO.slot_of();
    const int64_t n = W.n, m = W.m;
    std::vector<double> &hR = W.hR, &hT = W.hT, &hP = W.hP;
    int &cur = W.cur, &best = W.best;
    int pcg_last = 8;
    // the PCG's batch driver with this solver's product; two-level: the preconditioner's kernels start and update in place of the plain ones
    PcgHooks hooks;
    hooks.product = [&] { W.sx(W.pcg_args(), W.dst); };
    hooks.read = [&] { return W.read_state("the reduced camera PCG"); };
    hooks.start = [&] { W.pcg_start(); };
    if (W.tlmode) hooks.update = [&](int it) { W.precond(it, 0); };
    if (W.grouped && W.f_small) hooks.update = [&](int it) { W.pcg_update(it); };
    W.dense_mode = cfg.dense_schur;

    // the LM loop (xm_lm_loop.h) over this solver's launches and reads
    const LmRules rules{cfg.max_iters, cfg.function_tol, cfg.gradient_tol, cfg.parameter_tol, cfg.nonmonotonic, cfg.max_nonmonotonic};
    int nx = 0;   // the candidate's parameter set: neither the current one nor the least-cost one (without non-monotonic steps: cur ^ 1)
    LmHooks lm;
    lm.linearise = [&](double mu, bool point_changed) {
        if (point_changed) W.eval();
        W.passes(mu);
    };
    lm.read_point = [&](LmRead which) {
        const BaState s = W.read_state(which == kLmReadFinal ? "the final gradient" : "the cost and gradient");
        if (which == kLmReadFirst && !std::isfinite(s.cost))
            throw Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: the initial reprojection cost is not finite (a point on a camera's focal plane?)");
        return LmPoint{s.cost, s.gmax, s.used};
    };
    lm.solve = [&]() -> LmSolve {
        if (cfg.dense_schur) { W.dense_solve(); return {0, 0.0}; }
        if (W.tlmode) W.precond_setup();
        const PcgResult pr = pcg_solve_batched<CD>(W.pcg_args(), W.gfc, st, pcg_last, hooks);
        return {pr.iters, pr.relres};
    };
    lm.read_candidate = [&](double) {
        nx = 0;
        while (nx == cur || nx == best) ++nx;
        W.candidate(nx, W.x.p);
        const BaState s = W.read_state("the candidate's cost");
        LmCandidate c{s.cost_new, s.model, s.step2[0] + s.step2[1], s.x2[0] + s.x2[1]};
        if (cfg.dense_schur) {   // a failed factorisation: an invalid step
            c.solved = !s.fail;
            c.relres = c.solved ? (s.res2[1] > 0.0 ? std::sqrt(s.res2[0] / s.res2[1]) : 0.0) : -1.0;
        }
        if constexpr (ba_has_focal<CD>()) c.solved = c.solved && !s.bad_focal;   // a candidate focal that is not positive: an invalid step
        return c;
    };
    lm.accept = [&](bool new_best) {
        cur = nx;
        W.basis_stale = true;
        if (new_best) best = cur;
    };
    lm.to_best = [&] { cur = best; };
    lm.out_of_time = [&] { return secs_since(t_start) >= cfg.max_time; };
    const LmResult res = lm_loop(rules, lm);
    out.initial_cost = res.initial_cost; out.n_used = (int64_t)res.n_used;
    // ---- back to the caller's layouts; cameras / landmarks without a used observation are left as they came
    std::vector<int32_t> cu((size_t)n), lu((size_t)m);
    XM_HIP_CHECK(hipMemcpyAsync(hR.data(), W.R[cur].p, hR.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(hT.data(), W.T[cur].p, hT.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(hP.data(), W.P[cur].p, hP.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(cu.data(), W.cused.p, cu.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(lu.data(), W.lused.p, lu.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the refined parameters");
    from_device_layout(n, hR, hT, cu, rot, t);
    for (int64_t l = 0; l < m; ++l) {
        const int32_t sl = slot_of[(size_t)l];
        if (!lu[(size_t)sl]) continue;
        for (int a = 0; a < 3; ++a) p[(size_t)3 * l + a] = hP[(size_t)3 * sl + a];
    }
    if constexpr (ba_has_focal<CD>()) {   // held focals and those of cameras without a used observation were copied from set to set
        if (W.grouped) {   // a group's value: its representative's (every member holds it); an empty group keeps the caller's
            std::vector<double> hG((size_t)n);
            XM_HIP_CHECK(hipMemcpyAsync(hG.data(), W.G[cur].p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
            wait_stream(st, cfg.watchdog_s, kStage, "the refined focal scales");
            for (int64_t c = 0; c < W.ng; ++c)
                if (W.h_rep[(size_t)c] >= 0) cfg.focal[c] = hG[(size_t)W.h_rep[(size_t)c]];
        } else {
            XM_HIP_CHECK(hipMemcpyAsync(cfg.focal, W.G[cur].p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
            wait_stream(st, cfg.watchdog_s, kStage, "the refined focal scales");
        }
    }
    if constexpr (ba_has_dist<CD>()) {   // held coefficients and those of cameras without a used observation: copied from set to set
        XM_HIP_CHECK(hipMemcpyAsync(cfg.dist, W.Kd[cur].p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the refined radial coefficients");
    }
    out.status = res.status; out.iters = res.iters; out.accepted = res.accepted; out.pcg_iters = res.pcg_total;
    out.final_cost = res.final_cost; out.gradient_max = res.gmax; out.trace_len = lm_copy_trace(res, cfg.trace, cfg.trace_cap);
    out.coarse_fallbacks = W.coarse_fallbacks;
    out.seconds = secs_since(t_start);
}

// The test export xm_ctx_ba_probe: one eval + landmark pass + camera pass at (rot, t, p) with the damping mu, then whatever the caller
// asked for, every array brought back in the caller's index order.  Only BaWork's members launch kernels here.
template <int CD>
void probe(const SchurOp &SO, const BaSettings &cfg, const double *rot, const double *t, const double *p, BaProbe &q, hipStream_t st) {
    constexpr int NC = ba_nc<CD>();
    BaWork<CD> W(SO, cfg, rot, t, p, st, q.Sdense != nullptr);
    const std::vector<int32_t> &slot_of = SO.slot_of();
    const int64_t n = W.n, m = W.m, nd = W.nd;
    auto d2h = [&](void *dstp, const void *src, size_t bytes) { XM_HIP_CHECK(hipMemcpyAsync(dstp, src, bytes, hipMemcpyDeviceToHost, st)); };
    auto sync = [&](const char *what) { check_launch(what); wait_stream(st, cfg.watchdog_s, kStage, what); };
    // per-landmark arrays: device slot order -> input order
    std::vector<double> tmp;
    auto lm_out = [&](const double *dev, int w, double *outp) {
        if (!outp) return;
        tmp.resize((size_t)w * m);
        d2h(tmp.data(), dev, tmp.size() * sizeof(double));
        sync("a landmark array");
        for (int64_t l = 0; l < m; ++l)
            for (int k = 0; k < w; ++k) outp[(size_t)w * l + k] = tmp[(size_t)w * slot_of[(size_t)l] + k];
    };
    // focal groups: the caller's vectors have CP n + G entries (CP = CD - 1 columns per camera, then the groups' focal entries); the device's
    // have CD n (the group's entry in its representative's focal slot).  An empty group has no slot: 0 comes back for it
    constexpr int CP = CD - 1;
    const bool grouped = W.grouped;
    const int64_t ns = grouped ? CP * n + W.ng : nd;
    std::vector<double> hin, hout;
    auto to_dev = [&](const double *v, double *dev) {   // a caller's vector -> the device array
        if (!grouped) { XM_HIP_CHECK(hipMemcpyAsync(dev, v, (size_t)nd * sizeof(double), hipMemcpyHostToDevice, st)); return; }
        hin.assign((size_t)nd, 0.0);
        for (int64_t i = 0; i < n; ++i)
            for (int k = 0; k < CP; ++k) hin[(size_t)CD * i + k] = v[(size_t)CP * i + k];
        for (int64_t c = 0; c < W.ng; ++c)
            if (W.h_rep[(size_t)c] >= 0) hin[(size_t)CD * W.h_rep[(size_t)c] + CP] = v[(size_t)CP * n + c];
        XM_HIP_CHECK(hipMemcpyAsync(dev, hin.data(), (size_t)nd * sizeof(double), hipMemcpyHostToDevice, st));
        wait_stream(st, cfg.watchdog_s, kStage, "a probe vector");
    };
    auto from_dev = [&](double *v, const double *dev, const char *what) {   // and back (waits)
        if (!grouped) { d2h(v, dev, (size_t)nd * sizeof(double)); sync(what); return; }
        hout.resize((size_t)nd);
        d2h(hout.data(), dev, (size_t)nd * sizeof(double));
        sync(what);
        for (int64_t i = 0; i < n; ++i)
            for (int k = 0; k < CP; ++k) v[(size_t)CP * i + k] = hout[(size_t)CD * i + k];
        for (int64_t c = 0; c < W.ng; ++c) v[(size_t)CP * n + c] = W.h_rep[(size_t)c] >= 0 ? hout[(size_t)CD * W.h_rep[(size_t)c] + CP] : 0.0;
    };
    W.eval();
    W.passes(q.mu);
    const BaState s0 = W.read_state("the probe's passes");
    q.cost = s0.cost; q.n_used = (int64_t)s0.used; q.gmax = s0.gmax;
    if (q.b) from_dev(q.b, W.b.p, "the right-hand side");
    if (grouped && q.group_D) d2h(q.group_D, W.grp_D.p, (size_t)W.ng * sizeof(double));
    if (grouped && q.group_F) {   // the exact block (G x G, column-major, as assembled) where the rule builds it, else the diagonal (G)
        if (W.f_small) d2h(q.group_F, W.grp_Fcopy.p, (size_t)W.ng * W.ng * sizeof(double));
        else d2h(q.group_F, W.grp_F.p, (size_t)W.ng * sizeof(double));
        q.coarse_ok = W.f_exact ? 1 : 0;
    }
    if (q.ustar) d2h(q.ustar, W.ustar.p, (size_t)CD * nd * sizeof(double));
    if (q.sinv) d2h(q.sinv, W.sinv.p, (size_t)CD * nd * sizeof(double));
    if (q.cused) d2h(q.cused, W.cused.p, (size_t)n * sizeof(int32_t));
    sync("the camera arrays");
    lm_out(W.gl.p, 3, q.g_l);
    lm_out(W.vinv.p, 6, q.vinv);
    if (q.lused) {
        std::vector<int32_t> lu((size_t)m);
        d2h(lu.data(), W.lused.p, (size_t)m * sizeof(int32_t));
        sync("the landmark flags");
        for (int64_t l = 0; l < m; ++l) q.lused[l] = lu[(size_t)slot_of[(size_t)l]];
    }
    // S X: column j into the PCG's direction vector, the product pair, A p back (the state word's done flag is 0: nothing has set it)
    if (q.SX)
        for (int64_t j = 0; j < q.k; ++j) {
            to_dev(q.X + (size_t)ns * j, W.pv.p);
            W.sx(W.pcg_args(), W.dst);
            from_dev(q.SX + (size_t)ns * j, W.Ap.p, "the product S x");
        }
    if (q.Sdense && grouped) {   // the lower triangle of the (CP n + G)-row matrix, the rest 0
        W.dense_assemble();
        std::vector<double> hS((size_t)nd * nd);
        d2h(hS.data(), W.Sd.p, hS.size() * sizeof(double));
        sync("the dense Schur matrix");
        std::vector<int64_t> to((size_t)nd, -1);   // device index -> the caller's; -1: a pinned focal slot
        for (int64_t i = 0; i < n; ++i)
            for (int k = 0; k < CP; ++k) to[(size_t)CD * i + k] = CP * i + k;
        for (int64_t c = 0; c < W.ng; ++c)
            if (W.h_rep[(size_t)c] >= 0) to[(size_t)CD * W.h_rep[(size_t)c] + CP] = CP * n + c;
        std::fill(q.Sdense, q.Sdense + (size_t)ns * ns, 0.0);
        for (int64_t c = 0; c < W.ng; ++c)   // an empty group has no slot on the device: its row of the system is mu clamp(0) on the diagonal
            if (W.h_rep[(size_t)c] < 0) q.Sdense[(size_t)(CP * n + c) * (ns + 1)] = q.mu * 1e-6;
        for (int64_t bcol = 0; bcol < nd; ++bcol)
            for (int64_t arow = bcol; arow < nd; ++arow) {
                const int64_t sa = to[(size_t)arow], sb = to[(size_t)bcol];
                if (sa >= 0 && sb >= 0) q.Sdense[(size_t)std::max(sa, sb) + (size_t)std::min(sa, sb) * ns] = hS[(size_t)arow + (size_t)bcol * nd];
            }
    } else if (q.Sdense) {
        W.dense_assemble();
        d2h(q.Sdense, W.Sd.p, (size_t)nd * nd * sizeof(double));
        sync("the dense Schur matrix");
    }
    // the preconditioner's set-up as the loop runs it before the PCG, then M^-1 X through the PCG's start: b := X_j, z read back
    DevBuf<double> ac;
    if (W.tlmode) {
        if (cfg.precond == 2 && q.Ac) { ac.alloc((size_t)W.nct * W.nct); W.ac_copy = ac.p; }
        W.precond_setup();
        q.nagg = W.tl.nagg; q.ncoarse = cfg.precond == 2 ? W.tl.ncoarse : 0; q.coarse_ok = W.tl.use_coarse;
        if (cfg.precond == 2) {
            if (q.Pm) d2h(q.Pm, W.tl_P.p, (size_t)nd * NC * sizeof(double));
            if (q.dropped) d2h(q.dropped, W.tl_drop.p, (size_t)W.nct * sizeof(double));
            if (q.Ac) d2h(q.Ac, ac.p, (size_t)W.nct * W.nct * sizeof(double));
            sync("the coarse space");
        }
    }
    if (q.MX && q.k > 0) {
        DevBuf<double> keep;
        keep.alloc((size_t)nd, false);
        XM_HIP_CHECK(hipMemcpyAsync(keep.p, W.b.p, (size_t)nd * sizeof(double), hipMemcpyDeviceToDevice, st));
        for (int64_t j = 0; j < q.k; ++j) {
            to_dev(q.X + (size_t)ns * j, W.b.p);
            XM_HIP_CHECK(hipMemsetAsync(W.z.p, 0, (size_t)nd * sizeof(double), st));   // as the loop's first start finds it: cameras that are no members keep 0
            W.pcg_start();
            from_dev(q.MX + (size_t)ns * j, W.z.p, "the preconditioner");
        }
        XM_HIP_CHECK(hipMemcpyAsync(W.b.p, keep.p, (size_t)nd * sizeof(double), hipMemcpyDeviceToDevice, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the right-hand side");
    }
    if (q.dc) {
        to_dev(q.dc, W.x.p);
        W.candidate(1, W.x.p);
        const BaState s = W.read_state("the probe's candidate");
        q.cost1 = s.cost_new; q.model = s.model;
        q.step2[0] = s.step2[0]; q.step2[1] = s.step2[1]; q.x2[0] = s.x2[0]; q.x2[1] = s.x2[1];
        if constexpr (ba_has_focal<CD>()) {
            if (s.bad_focal) q.cost1 = std::nan("");   // the candidate the loop rejects as invalid
            if (q.focal1 && grouped) {
                std::vector<double> hG((size_t)n);
                d2h(hG.data(), W.G[1].p, (size_t)n * sizeof(double));
                sync("the candidate focal scales");
                for (int64_t c = 0; c < W.ng; ++c) q.focal1[c] = W.h_rep[(size_t)c] >= 0 ? hG[(size_t)W.h_rep[(size_t)c]] : cfg.focal[c];
            } else if (q.focal1) { d2h(q.focal1, W.G[1].p, (size_t)n * sizeof(double)); sync("the candidate focal scales"); }
        }
        if constexpr (ba_has_dist<CD>()) {
            if (q.dist1) { d2h(q.dist1, W.Kd[1].p, (size_t)n * sizeof(double)); sync("the candidate radial coefficients"); }
        }
        lm_out(W.dP.p, 3, q.dP);
        lm_out(W.P[1].p, 3, q.p1);
        if (q.rot1 || q.t1) {   // as the loop returns them: cameras without a used observation keep the caller's bits
            std::vector<double> hR((size_t)9 * n), hT((size_t)3 * n);
            std::vector<int32_t> cu((size_t)n);
            d2h(hR.data(), W.R[1].p, hR.size() * sizeof(double));
            d2h(hT.data(), W.T[1].p, hT.size() * sizeof(double));
            d2h(cu.data(), W.cused.p, cu.size() * sizeof(int32_t));
            sync("the candidate cameras");
            if (q.rot1) std::memcpy(q.rot1, rot, (size_t)9 * n * sizeof(double));
            if (q.t1) std::memcpy(q.t1, t, (size_t)3 * n * sizeof(double));
            from_device_layout(n, hR, hT, cu, q.rot1, q.t1);
        }
    }
}

// f(CD as a constant) for the camera block the settings ask for; who: the export's name up to the focal suffix, for the messages
template <class F>
void with_cd(const BaSettings &cfg, const std::string &who, F &&f) {
    if (cfg.refine_focal) {
        if (cfg.precond != 0 || !cfg.focal) throw Error(XM_ERR_ARG, who + "_focal: needs the focal scales and the default preconditioner");
        if (cfg.ngroups > 0 && !cfg.group_of) throw Error(XM_ERR_ARG, who + "_focal_groups: needs group_of");
        if (cfg.refine_dist) {
            if (!cfg.dist || cfg.ngroups > 0) throw Error(XM_ERR_ARG, who + "_radial: needs the radial coefficients and no focal groups");
            if (cfg.fix_rotations) f(std::integral_constant<int, 5>{});
            else f(std::integral_constant<int, 8>{});
        } else if (cfg.fix_rotations) f(std::integral_constant<int, 4>{});
        else f(std::integral_constant<int, 7>{});
    } else if (cfg.fix_rotations) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 6>{});
}

}  // namespace

void ba_aggregate_plan(int64_t n, int64_t nobs, const int32_t *cam, const int32_t *lm, const uint8_t *used, int B, std::vector<int32_t> &order) {
    if (n < 1 || nobs < 0 || (nobs > 0 && (!cam || !lm))) throw Error(XM_ERR_ARG, "aggregate plan: needs at least 1 camera and the observation arrays");
    if (B < 1 || B > 64) throw Error(XM_ERR_ARG, "aggregate plan: cameras per aggregate must be 1..64");
    int64_t M = 0;
    for (int64_t e = 0; e < nobs; ++e) {
        if (cam[e] < 0 || cam[e] >= n || lm[e] < 0) throw Error(XM_ERR_ARG, "aggregate plan: observation index out of range");
        M = std::max<int64_t>(M, (int64_t)lm[e] + 1);
    }
    // the bipartite graph of the used observations as two lists in input order (fixed visiting order)
    auto on = [&](int64_t e) { return used == nullptr || used[e] != 0; };
    std::vector<int64_t> cptr((size_t)n + 1, 0), lptr((size_t)M + 1, 0);
    for (int64_t e = 0; e < nobs; ++e)
        if (on(e)) { cptr[(size_t)cam[e] + 1]++; lptr[(size_t)lm[e] + 1]++; }
    for (int64_t i = 0; i < n; ++i) cptr[(size_t)i + 1] += cptr[(size_t)i];
    for (int64_t l = 0; l < M; ++l) lptr[(size_t)l + 1] += lptr[(size_t)l];
    const int64_t nused = cptr[(size_t)n];
    std::vector<int32_t> c_l((size_t)nused), l_c((size_t)nused);
    {
        std::vector<int64_t> nc(cptr.begin(), cptr.end() - 1), nl(lptr.begin(), lptr.end() - 1);
        for (int64_t e = 0; e < nobs; ++e)
            if (on(e)) { c_l[(size_t)nc[(size_t)cam[e]]++] = lm[e]; l_c[(size_t)nl[(size_t)lm[e]]++] = cam[e]; }
    }
    int64_t nmem = 0;
    for (int64_t i = 0; i < n; ++i) nmem += cptr[(size_t)i + 1] > cptr[(size_t)i] ? 1 : 0;
    if ((nmem + B - 1) / B > XM_BA_MAX_AGGREGATES)
        throw Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: " + std::to_string(nmem) + " cameras make more than XM_BA_MAX_AGGREGATES aggregates of " +
                                std::to_string(B) + " (use the default preconditioner)");
    // breadth-first order from `start` with the level (camera-to-camera hops) of every camera reached
    std::vector<char> cseen, lseen;
    std::vector<int32_t> level;
    auto bfs = [&](int32_t start, std::vector<int32_t> &out) {
        cseen.assign((size_t)n, 0); lseen.assign((size_t)M, 0); level.assign((size_t)n, -1);
        out.clear();
        out.push_back(start); cseen[(size_t)start] = 1; level[(size_t)start] = 0;
        for (size_t h = 0; h < out.size(); ++h) {
            const int32_t c = out[h];
            for (int64_t q = cptr[(size_t)c]; q < cptr[(size_t)c + 1]; ++q) {
                const int32_t l = c_l[(size_t)q];
                if (lseen[(size_t)l] || lptr[(size_t)l + 1] - lptr[(size_t)l] > 64) continue;   // heavy landmarks carry no locality
                lseen[(size_t)l] = 1;
                for (int64_t q2 = lptr[(size_t)l]; q2 < lptr[(size_t)l + 1]; ++q2) {
                    const int32_t c2 = l_c[(size_t)q2];
                    if (!cseen[(size_t)c2]) { cseen[(size_t)c2] = 1; level[(size_t)c2] = level[(size_t)c] + 1; out.push_back(c2); }
                }
            }
        }
    };
    order.clear();
    if (nmem == 0) return;
    int32_t start = 0;
    while (cptr[(size_t)start + 1] == cptr[(size_t)start]) ++start;   // camera 0, or the first member when camera 0 is none
    // From a camera in the middle of a trajectory the search advances on two fronts and every aggregate would hold two distant stretches.
    // So the search is repeated from the camera reached last; it replaces the first one unless the start lies in its last level (the start
    // is then an end of the trajectory itself and the order from it stands)
    std::vector<int32_t> first;
    bfs(start, first);
    const int32_t far = first.back();
    bfs(far, order);   // reaches the component of the first search: the same cameras, so cseen ends as that search left it
    if (level[(size_t)start] == level[(size_t)order.back()]) order.swap(first);
    for (int64_t i = 0; i < n; ++i)
        if (!cseen[(size_t)i] && cptr[(size_t)i + 1] > cptr[(size_t)i]) order.push_back((int32_t)i);
}

void bundle_adjust(const SchurOp &S, const BaSettings &cfg, double *rot, double *t, double *p, BaOutcome &out, hipStream_t st) {
    out = BaOutcome();
    with_cd(cfg, "xm_ctx_bundle_adjust", [&](auto CD) { run<CD.value>(S, cfg, rot, t, p, out, st); });
}

void ba_probe(const SchurOp &S, const BaSettings &cfg, const double *rot, const double *t, const double *p, BaProbe &q, hipStream_t st) {
    with_cd(cfg, "xm_ctx_ba_probe", [&](auto CD) { probe<CD.value>(S, cfg, rot, t, p, q, st); });
}

void reprojection_errors(const SchurOp &SO, const double *rot, const double *t, const double *p, const double *focal, const double *dist,
                         double *sqerr, double watchdog_s, hipStream_t st) {
    const SchurLists S = SO.lists();
    std::vector<double> hR, hT, hP;
    to_device_layout(SO, rot, t, p, hR, hT, hP);
    DevBuf<double> R, T, P, G, K, out;
    if (dist) {
        if (!focal) throw Error(XM_ERR_ARG, "xm_ctx_reprojection_errors_radial: needs the focal scales");
        K.alloc((size_t)S.n, false);
        XM_HIP_CHECK(hipMemcpyAsync(K.p, dist, (size_t)S.n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (focal) {
        G.alloc((size_t)S.n, false);
        XM_HIP_CHECK(hipMemcpyAsync(G.p, focal, (size_t)S.n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    R.alloc(hR.size(), false); T.alloc(hT.size(), false); P.alloc(hP.size(), false); out.alloc((size_t)std::max<int64_t>(S.nobs, 1), false);
    XM_HIP_CHECK(hipMemcpyAsync(R.p, hR.data(), hR.size() * sizeof(double), hipMemcpyHostToDevice, st));
    XM_HIP_CHECK(hipMemcpyAsync(T.p, hT.data(), hT.size() * sizeof(double), hipMemcpyHostToDevice, st));
    XM_HIP_CHECK(hipMemcpyAsync(P.p, hP.data(), hP.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (S.nobs > 0) {
        auto launch = [&](auto FOCAL) {
            hipLaunchKernelGGL(ba_sqerr_kernel<FOCAL.value>, dim3(flat_grid(S.nobs)), dim3(256), 0, st, S, (const double *)R.p, (const double *)T.p,
                               (const double *)P.p, (const double *)G.p, out.p);
        };
        if (dist)
            hipLaunchKernelGGL(ba_sqerr_radial_kernel, dim3(flat_grid(S.nobs)), dim3(256), 0, st, S, (const double *)R.p, (const double *)T.p,
                               (const double *)P.p, (const double *)G.p, (const double *)K.p, out.p);
        else if (focal) launch(std::true_type{});
        else launch(std::false_type{});
        check_launch("the reprojection errors");
        XM_HIP_CHECK(hipMemcpyAsync(sqerr, out.p, (size_t)S.nobs * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    wait_stream(st, watchdog_s, kStage, "the reprojection errors");
}

}  // namespace xm
