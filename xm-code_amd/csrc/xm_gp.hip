// xm_gp.hip — global positioning on the lists of the matrix-free storage (design: xm_gp.h).  3 x 3 camera blocks throughout.
#include "xm_gp.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "xm_device.h"
#include "xm_lm_loop.h"
#include "xm_lm_shared.h"
#include "xm_pair_lists.h"
#include "xm_schur.h"
#include "xm_stage.h"

namespace xm {

namespace {

constexpr const char *kStage = "global positioning";

// per-observation record, one plane of `stride` doubles per entry: a = w s^2, u = w s v / sqrt(h*) (3), q_e (3), k = g_s / sqrt(h*).
// M_e = a I - u u^T; the observation's part of the FULL gradient of its camera is w s r = q_e - k u.  An observation that is not used,
// and the padding of the packed landmark lists, is 0 in every plane and adds nothing to any sum.
constexpr int kGpPlanes = 8;
enum { GA = 0, GU = 1, GQ = 4, GK = 7 };
// per camera over its participating pairs: sum M_m (6, in tri() order), sum w sigma^2, the reduced gradient's part (3), the full gradient's (3)
constexpr int kGpPairSums = 13;

struct GpState {        // device-resident; the host reads it whole
    BaState b;          // the PCG's words and the scalars the bundle adjustment has too (step2 / x2: cameras, landmarks)
    double step2s, x2s; // |ds|^2 and |s|^2 over the used observations
    double gsmax;       // max |g_s| over the scales that are not frozen
    // the pairs' shares (0 without pair terms): cost and max |g_sigma| at the current point; the candidate's cost, model, |d sigma|^2, |sigma|^2
    double pcost, pgsmax, pcost_new, pmodel, pstep2, px2;
};

// what one observation contributes at (c_i, P_l, s_e): v = P - c, r = d - s v, w = rho'(|r|^2) (1 for the trivial loss), g_s = -w r.v, and
// whether its scale is frozen for this iteration (at the bound with the gradient pointing outward).  Returns rho(|r|^2).
struct GpLin {
    double v[3], r[3], w, gs, hs;
    bool frozen;
};
// AW: the loss is Ceres's ScaledLoss with the factor ae (rho and rho' times ae); without it ae is not read
template <int LOSS, bool AW = false>
__device__ __forceinline__ double gp_lin(const double *c, const double *P, const double *d, double s, double a, double mu, GpLin &o, double ae = 1.0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.v[k] = P[k] - c[k]; o.r[k] = d[k] - s * o.v[k]; }
    const double sq = o.r[0] * o.r[0] + o.r[1] * o.r[1] + o.r[2] * o.r[2];
    double rho = sq;
    o.w = 1.0;
    if constexpr (LOSS != XM_BA_LOSS_TRIVIAL) rho = ba_rho<LOSS>(sq, a, o.w);
    if constexpr (AW) { rho *= ae; o.w *= ae; }
    o.gs = -o.w * (o.r[0] * o.v[0] + o.r[1] * o.v[1] + o.r[2] * o.v[2]);
    o.frozen = s <= kGpMinScale && o.gs > 0.0;
    const double h = o.w * (o.v[0] * o.v[0] + o.v[1] * o.v[1] + o.v[2] * o.v[2]);
    o.hs = h + mu * clamp_diag(h);
    return rho;
}

// ---- once per call: the observed directions d_e = R_i p_e / |p_e| and, by landmark position, which observations pass the weight and depth tests
__global__ __launch_bounds__(256) void gp_setup_kernel(SchurLists S, const double *__restrict__ rot, double *__restrict__ dir, double *__restrict__ lflag) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * 256) {
        const double w = S.cam_w[S.pos_c[e]], p0 = S.obs_p[3 * e], p1 = S.obs_p[3 * e + 1], p2 = S.obs_p[3 * e + 2];
        const bool ok = w > 0.0 && p2 > 0.0;
        double d[3] = {0.0, 0.0, 0.0};
        if (ok) {
            const double *R = rot + (size_t)9 * S.obs_cam[e];   // column-major: R[a + 3 c]
            const double in = 1.0 / sqrt(p0 * p0 + p1 * p1 + p2 * p2), b0 = p0 * in, b1 = p1 * in, b2 = p2 * in;
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] = R[a] * b0 + R[3 + a] * b1 + R[6 + a] * b2;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) dir[3 * e + a] = d[a];
        lflag[S.dpos_l[e]] = ok ? 1.0 : 0.0;
    }
}
// out[l] = 1 when at least `need` flags of landmark slot l's list are set
__global__ __launch_bounds__(kBaHeavyThreads) void gp_lm_count_kernel(SchurLists S, const double *__restrict__ lflag, double need, int32_t *__restrict__ out) {
    const LmRange q = lm_range(S);
    double acc[1] = {0.0};
    for (int64_t e = q.e; e < q.e_end; e += q.step) acc[0] += lflag[e];
    bool writer = q.active;
    if (q.heavy) writer = heavy_sum<1>(acc);
    if (writer) out[q.l] = acc[0] >= need ? 1 : 0;
}
// used observations in input order and in both list orders (lflag is overwritten: the tests are evaluated again, not read from it)
__global__ __launch_bounds__(256) void gp_used_kernel(SchurLists S, const int32_t *__restrict__ lm_ok, int32_t *__restrict__ oused, double *__restrict__ cflag,
                                                      double *__restrict__ lflag) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * 256) {
        const int64_t pc = S.pos_c[e];
        const bool u = S.cam_w[pc] > 0.0 && S.obs_p[3 * e + 2] > 0.0 && lm_ok[S.obs_lm[e]] != 0;
        oused[e] = u ? 1 : 0;
        cflag[pc] = u ? 1.0 : 0.0;
        lflag[S.dpos_l[e]] = u ? 1.0 : 0.0;
    }
}
// cameras with a used observation (a wavefront per camera)
__global__ __launch_bounds__(256) void gp_cam_count_kernel(SchurLists S, const double *__restrict__ cflag, int32_t *__restrict__ cused) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cam = (int64_t)blockIdx.x * kQwWaves + wv;
    if (cam >= S.n) return;
    double acc = 0.0;
    for (int64_t e = S.cam_ptr[cam] + lane; e < S.cam_ptr[cam + 1]; e += 64) acc += cflag[e];
    acc = wave_sum(acc);
    if (lane == 0) cused[cam] = acc > 0.0 ? 1 : 0;
}

// ---- the records at (c, P, s) for the damping mu, written in both list orders; partial sums of the cost 1/2 sum rho(|r|^2) and of the
// used observations, per-workgroup max of |g_s|
template <int LOSS, bool AW>
__global__ __launch_bounds__(256) void gp_eval_kernel(SchurLists S, const int32_t *__restrict__ oused, const double *__restrict__ dir,
                                                      const double *__restrict__ C, const double *__restrict__ P, const double *__restrict__ sc, double a,
                                                      double mu, const double *__restrict__ cam_a, double *__restrict__ Jc, double *__restrict__ Jl,
                                                      int32_t *__restrict__ frozen, double *__restrict__ parts) {
    __shared__ double sh[4];
    __shared__ double shm[4];
    double cost = 0.0, used = 0.0, gsm = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * 256) {
        double v[kGpPlanes];
#pragma unroll
        for (int k = 0; k < kGpPlanes; ++k) v[k] = 0.0;
        int fz = 0;
        if (oused[e]) {
            GpLin o;
            const double s = sc[e];
            cost += 0.5 * gp_lin<LOSS, AW>(C + (size_t)3 * S.obs_cam[e], P + (size_t)3 * S.obs_lm[e], dir + (size_t)3 * e, s, a, mu, o,
                                           AW ? cam_a[S.obs_cam[e]] : 1.0);
            const double ws = o.w * s;
            v[GA] = ws * s;
            if (o.frozen) {
                fz = 1;
#pragma unroll
                for (int k = 0; k < 3; ++k) v[GQ + k] = ws * o.r[k];
            } else {
                const double ih = 1.0 / sqrt(o.hs);
                v[GK] = o.gs * ih;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    v[GU + k] = ws * ih * o.v[k];
                    v[GQ + k] = ws * o.r[k] + v[GU + k] * v[GK];
                }
                gsm = fmax(gsm, fabs(o.gs));
            }
            used += 1.0;
        }
        const int64_t pc = S.pos_c[e], pl = S.dpos_l[e];
#pragma unroll
        for (int k = 0; k < kGpPlanes; ++k) {
            Jc[(size_t)k * S.nobs + pc] = v[k];
            Jl[(size_t)k * S.lm_total + pl] = v[k];
        }
        frozen[e] = fz;
    }
    cost = block_sum256(cost, sh);
    used = block_sum256(used, sh);
    const double m = block_max<256>(gsm, shm);
    if (threadIdx.x == 0) { parts[blockIdx.x] = cost; parts[gridDim.x + blockIdx.x] = used; parts[2 * (size_t)gridDim.x + blockIdx.x] = m; }
}

// ---- landmark pass: V_l = sum M_e, g_l = -sum q_e, (V_l + mu clamp(sum a) I)^-1 (6 entries of the symmetric inverse); per-workgroup max of the
// FULL gradient's landmark part |sum -(q_e - k u)|_inf
__global__ __launch_bounds__(kBaHeavyThreads) void gp_lm_kernel(SchurLists S, const double *__restrict__ Jl, double mu, double *__restrict__ vinv,
                                                                double *__restrict__ gl, double *__restrict__ gpart) {
    __shared__ double sh[kBaHeavyThreads / 64];
    const LmRange q = lm_range(S);
    double acc[10], gf[3] = {0.0, 0.0, 0.0};   // V (6), g_l (3), sum a; the full gradient's part
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (int64_t e = q.e; e < q.e_end; e += q.step) {
        double v[kGpPlanes];
#pragma unroll
        for (int k = 0; k < kGpPlanes; ++k) v[k] = Jl[(size_t)k * S.lm_total + e];
        acc[0] += v[GA] - v[GU] * v[GU]; acc[1] -= v[GU] * v[GU + 1]; acc[2] -= v[GU] * v[GU + 2];
        acc[3] += v[GA] - v[GU + 1] * v[GU + 1]; acc[4] -= v[GU + 1] * v[GU + 2]; acc[5] += v[GA] - v[GU + 2] * v[GU + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[6 + k] -= v[GQ + k]; gf[k] -= v[GQ + k] - v[GK] * v[GU + k]; }
        acc[9] += v[GA];
    }
    bool writer = q.active;
    if (q.heavy) {   // two reductions of 10 and 3 values: one of 13 keeps 208 wavefront sums in flight in thread 0 and spills
        heavy_sum<3>(gf);
        writer = heavy_sum<10>(acc);
    }
    double gabs = 0.0;
    if (writer) {
        const int64_t l = q.l;
        const double dmp = mu * clamp_diag(acc[9]);
        const double a00 = acc[0] + dmp, a11 = acc[3] + dmp, a22 = acc[5] + dmp, a01 = acc[1], a02 = acc[2], a12 = acc[4];
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double id = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
        double *vi = vinv + (size_t)6 * l;
        vi[0] = c00 * id; vi[1] = c01 * id; vi[2] = c02 * id; vi[3] = c11 * id; vi[4] = c12 * id; vi[5] = c22 * id;
        gl[3 * l] = acc[6]; gl[3 * l + 1] = acc[7]; gl[3 * l + 2] = acc[8];
        gabs = fmax(fabs(gf[0]), fmax(fabs(gf[1]), fabs(gf[2])));
    }
    if (q.heavy) {
        if (writer) gpart[blockIdx.x] = gabs;
        return;
    }
    const double m = block_max<kBaHeavyThreads>(gabs, sh);
    if (threadIdx.x == 0) gpart[blockIdx.x] = m;
}

// M = a I - u u^T from a record's first four planes
__device__ __forceinline__ void gp_m(const double (&v)[kGpPlanes], double (&M)[3][3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[j][k] = (j == k ? v[GA] : 0.0) - v[GU + j] * v[GU + k];
}
__device__ __forceinline__ void gp_load(const double *J, size_t stride, int64_t e, double (&v)[kGpPlanes]) {
#pragma unroll
    for (int k = 0; k < kGpPlanes; ++k) v[k] = J[(size_t)k * stride + e];
}

// ---- camera pass (a wavefront per camera): U*_i; S_ii = U*_i - sum_l (sum_e M_e) V*_l^-1 (sum_f M_f) over the observations e, f of (i, l)
// and its inverse; b_i = -sum q_e - sum M_e V*_l^-1 g_l (W_e = -M_e); per-workgroup max of the FULL gradient's camera part
// PAIRS: the camera's sums over its pairs (gp_pair_cam_kernel: psum) join U_i, the damped diagonal, the gradient parts and so S_ii^-1, b_i and
// the gradient's max; obs_on = 0 (no observation terms): the observation list is not walked
template <bool PAIRS>
__global__ __launch_bounds__(256) void gp_cam_kernel(SchurLists S, const double *__restrict__ Jc, const double *__restrict__ vinv,
                                                     const double *__restrict__ gl, double mu, const double *__restrict__ psum, int obs_on,
                                                     double *__restrict__ ustar, double *__restrict__ sinv, double *__restrict__ b,
                                                     double *__restrict__ gpart) {
    constexpr int NU = 6, NA = 2 * NU + 10;   // U, the landmarks' term, sum q (3), sum M V^-1 g (3), the full gradient (3), sum a
    __shared__ double red[kQwWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cam = (int64_t)blockIdx.x * kQwWaves + wv;
    const bool on = cam < S.n;
    double acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    if (on && (!PAIRS || obs_on))
        for (int64_t e = S.cam_ptr[cam] + lane; e < S.cam_ptr[cam + 1]; e += 64) {
            double v[kGpPlanes], M[3][3], V[3][3], MV[3][3];
            gp_load(Jc, (size_t)S.nobs, e, v);
            gp_m(v, M);
            const int64_t l = S.cam_lm[e];
            sym3(vinv + (size_t)6 * l, V);
            const double g0 = gl[3 * l], g1 = gl[3 * l + 1], g2 = gl[3 * l + 2];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) MV[k][c] = M[k][0] * V[0][c] + M[k][1] * V[1][c] + M[k][2] * V[2][c];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int k = 0; k <= j; ++k) {
                    acc[tri(k, j)] += M[k][j];
                    acc[NU + tri(k, j)] += MV[k][0] * M[j][0] + MV[k][1] * M[j][1] + MV[k][2] * M[j][2];
                }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                acc[2 * NU + k] += v[GQ + k];
                acc[2 * NU + 3 + k] += MV[k][0] * g0 + MV[k][1] * g1 + MV[k][2] * g2;
                acc[2 * NU + 6 + k] += v[GQ + k] - v[GK] * v[GU + k];
            }
            acc[NA - 1] += v[GA];
            // a (camera, landmark) pair named more than once: every other observation f of the pair brings M_e V*^-1 M_f.  The list is sorted
            // by landmark: they are this entry's neighbours (none in an ordinary scene)
            for (int dir = -1; dir <= 1; dir += 2)
                for (int64_t f = e + dir; f >= S.cam_ptr[cam] && f < S.cam_ptr[cam + 1] && S.cam_lm[f] == l; f += dir) {
                    double vf[kGpPlanes], Mf[3][3];
                    gp_load(Jc, (size_t)S.nobs, f, vf);
                    gp_m(vf, Mf);
#pragma unroll
                    for (int j = 0; j < 3; ++j)
#pragma unroll
                        for (int k = 0; k <= j; ++k) acc[NU + tri(k, j)] += MV[k][0] * Mf[j][0] + MV[k][1] * Mf[j][1] + MV[k][2] * Mf[j][2];
                }
        }
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = wave_sum(acc[k]);
    double gabs = 0.0;
    if (on && lane == 0) {
        double Us[3][3], Sm[3][3];
        if constexpr (PAIRS) {
            const double *ps = psum + (size_t)kGpPairSums * cam;
#pragma unroll
            for (int k = 0; k < NU; ++k) acc[k] += ps[k];
            acc[NA - 1] += ps[6];
#pragma unroll
            for (int k = 0; k < 3; ++k) { acc[2 * NU + k] += ps[7 + k]; acc[2 * NU + 6 + k] += ps[10 + k]; }
        }
        const double dmp = mu * clamp_diag(acc[NA - 1]);
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                Us[j][k] = acc[tri(k, j)] + (j == k ? dmp : 0.0);
                Sm[j][k] = Us[j][k] - acc[NU + tri(k, j)];
            }
        double *us = ustar + (size_t)9 * cam;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) us[3 * j + k] = Us[j][k];
        chol_inverse<3>(Sm, sinv + (size_t)9 * cam);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b[(size_t)3 * cam + k] = -acc[2 * NU + k] - acc[2 * NU + 3 + k];
            gabs = fmax(gabs, fabs(acc[2 * NU + 6 + k]));
        }
    }
    if (lane == 0) red[wv] = gabs;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = 0.0;
        for (int q = 0; q < kQwWaves; ++q) m = fmax(m, red[q]);
        gpart[blockIdx.x] = m;
    }
}

// landmark side of S x (and of the back-substitution): y_l = sgn V*_l^-1 (g_l + sum_{obs of l} W_e^T x_i), W_e = -M_e   (g: optional)
__global__ __launch_bounds__(kBaHeavyThreads) void gp_lmx_kernel(SchurLists S, const double *__restrict__ Jl, const double *__restrict__ vinv,
                                                                 const double *__restrict__ gl, double sgn, const int32_t *__restrict__ lused,
                                                                 const double *__restrict__ x, const BaState *__restrict__ st, double *__restrict__ y) {
    if (st != nullptr && st->done) return;
    const LmRange q = lm_range(S);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t e = q.e; e < q.e_end; e += q.step) {
        const double a = Jl[(size_t)GA * S.lm_total + e], u0 = Jl[(size_t)GU * S.lm_total + e], u1 = Jl[(size_t)(GU + 1) * S.lm_total + e],
                     u2 = Jl[(size_t)(GU + 2) * S.lm_total + e];
        const double *xi = x + (size_t)3 * S.lm_cam[e];
        const double ux = u0 * xi[0] + u1 * xi[1] + u2 * xi[2];
        acc[0] -= a * xi[0] - u0 * ux; acc[1] -= a * xi[1] - u1 * ux; acc[2] -= a * xi[2] - u2 * ux;
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
// camera side: Ap_i = U*_i p_i - sum_{obs of i} W_e y_l = U*_i p_i + sum M_e y_l (a wavefront per camera); per-workgroup partials of <p, Ap>
// PAIRS: plus the pairs' off-diagonal part yp_i = -sum M_m p_other (gp_pairx_kernel), added before <p, Ap> is taken
template <bool PAIRS>
__global__ __launch_bounds__(256) void gp_camx_kernel(SchurLists S, const double *__restrict__ Jc, const double *__restrict__ y,
                                                      const double *__restrict__ yp, int obs_on, BaPcg a) {
    __shared__ double red[kQwWaves];
    if (a.st->done) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cam = (int64_t)blockIdx.x * kQwWaves + wv;
    const bool on = cam < S.n;
    double acc[3] = {0.0, 0.0, 0.0};
    if (on && (!PAIRS || obs_on))
        for (int64_t e = S.cam_ptr[cam] + lane; e < S.cam_ptr[cam + 1]; e += 64) {
            const double av = Jc[(size_t)GA * S.nobs + e], u0 = Jc[(size_t)GU * S.nobs + e], u1 = Jc[(size_t)(GU + 1) * S.nobs + e],
                         u2 = Jc[(size_t)(GU + 2) * S.nobs + e];
            const double *yl = y + (size_t)3 * S.cam_lm[e];
            const double uy = u0 * yl[0] + u1 * yl[1] + u2 * yl[2];
            acc[0] += av * yl[0] - u0 * uy; acc[1] += av * yl[1] - u1 * uy; acc[2] += av * yl[2] - u2 * uy;
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = wave_sum(acc[k]);
    double pap = 0.0;
    if (on && lane == 0) {
        double up[3];
        block_matvec<3>(a.ustar + (size_t)9 * cam, a.p + (size_t)3 * cam, up);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double v = up[k] + acc[k];
            if constexpr (PAIRS) v += yp[3 * cam + k];
            a.Ap[3 * cam + k] = v;
            pap += a.p[3 * cam + k] * v;
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

// ---- candidate point.  Centres and points: ba_cand_vec_kernel of xm_lm_shared.h.
// scales: ds_e = -(g_s - w s v.(dc - dP)) / h* (0 for a frozen one) from the linearisation at the current point (the eval kernel's
// expression), s <- max(s + ds, 1e-5); the cost 1/2 sum rho(|r|^2) at the candidate, the linear model's terms sum r.(J d) + |J d|^2 / 2 with
// J d = sqrt(w) (s (dc - dP) - v ds), and partials of |ds|^2 and |s|^2
template <int LOSS, bool AW>
__global__ __launch_bounds__(256) void gp_cand_obs_kernel(SchurLists S, const int32_t *__restrict__ oused, const double *__restrict__ dir,
                                                          const double *__restrict__ C, const double *__restrict__ P, const double *__restrict__ sc,
                                                          const double *__restrict__ dc, const double *__restrict__ dP, const double *__restrict__ Cn,
                                                          const double *__restrict__ Pn, double a, double mu, const double *__restrict__ cam_a,
                                                          double *__restrict__ sn, double *__restrict__ dsv, double *__restrict__ parts) {
    __shared__ double sh[4];
    double cost = 0.0, model = 0.0, s2 = 0.0, x2 = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * 256) {
        const double s = sc[e];
        double s1 = s, ds = 0.0;
        if (oused[e]) {
            const int64_t i = S.obs_cam[e], l = S.obs_lm[e];
            GpLin o;
            const double ae = AW ? cam_a[i] : 1.0;
            (void)gp_lin<LOSS, AW>(C + 3 * i, P + 3 * l, dir + (size_t)3 * e, s, a, mu, o, ae);
            double dd[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) dd[k] = dc[3 * i + k] - dP[3 * l + k];
            const double vd = o.v[0] * dd[0] + o.v[1] * dd[1] + o.v[2] * dd[2];
            if (!o.frozen) ds = -(o.gs - o.w * s * vd) / o.hs;
            s1 = fmax(s + ds, kGpMinScale);
            double rj = 0.0, jj = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double jd = s * dd[k] - o.v[k] * ds;
                rj += o.r[k] * jd; jj += jd * jd;
            }
            model += o.w * (rj + 0.5 * jj);
            GpLin o1;
            cost += 0.5 * gp_lin<LOSS, AW>(Cn + 3 * i, Pn + 3 * l, dir + (size_t)3 * e, s1, a, mu, o1, ae);
            s2 += ds * ds; x2 += s * s;
        }
        sn[e] = s1;
        dsv[e] = ds;
    }
    cost = block_sum256(cost, sh);
    model = block_sum256(model, sh);
    s2 = block_sum256(s2, sh);
    x2 = block_sum256(x2, sh);
    if (threadIdx.x == 0) {
        const size_t g = gridDim.x;
        parts[blockIdx.x] = cost; parts[g + blockIdx.x] = model; parts[2 * g + blockIdx.x] = s2; parts[3 * g + blockIdx.x] = x2;
    }
}

// ---- camera-to-camera terms (design: xm_gp.h).  The M participating pairs in input order; a pair is an observation of camera ci whose
// point is camera cj and whose direction is tau, so gp_lin, the record's eight planes (stride M) and the candidate's expressions are the
// observations'.
struct GpPairs {
    int64_t M;
    const int32_t *ci, *cj;
    const double *tau;   // 3 per pair
};
// once per call: tau_m = -R_j trel_m
__global__ __launch_bounds__(256) void gp_pair_setup_kernel(int64_t M, const int32_t *__restrict__ cj, const double *__restrict__ rot,
                                                            const double *__restrict__ trel, double *__restrict__ tau) {
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
        const double *R = rot + (size_t)9 * cj[m];   // column-major: R[a + 3 c]
        const double t0 = trel[3 * m], t1 = trel[3 * m + 1], t2 = trel[3 * m + 2];
#pragma unroll
        for (int a = 0; a < 3; ++a) tau[3 * m + a] = -(R[a] * t0 + R[3 + a] * t1 + R[6 + a] * t2);
    }
}
// cused |= the camera has a participating pair
__global__ __launch_bounds__(256) void gp_pair_used_kernel(int n, const int64_t *__restrict__ ptr, int32_t *__restrict__ cused) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        if (ptr[i + 1] > ptr[i]) cused[i] = 1;
}
// the records at (c, sigma) for the damping mu (a thread per pair); per-workgroup partials of the cost and of max |g_sigma|
template <int LOSS>
__global__ __launch_bounds__(256) void gp_pair_eval_kernel(GpPairs Q, const double *__restrict__ C, const double *__restrict__ sg, double a, double mu,
                                                           double *__restrict__ rec, int32_t *__restrict__ pfrozen, double *__restrict__ parts) {
    __shared__ double sh[4];
    __shared__ double shm[4];
    double cost = 0.0, gsm = 0.0;
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < Q.M; m += (int64_t)gridDim.x * 256) {
        double v[kGpPlanes];
#pragma unroll
        for (int k = 0; k < kGpPlanes; ++k) v[k] = 0.0;
        GpLin o;
        const double s = sg[m];
        cost += 0.5 * gp_lin<LOSS>(C + (size_t)3 * Q.ci[m], C + (size_t)3 * Q.cj[m], Q.tau + (size_t)3 * m, s, a, mu, o);
        const double ws = o.w * s;
        v[GA] = ws * s;
        if (o.frozen) {
#pragma unroll
            for (int k = 0; k < 3; ++k) v[GQ + k] = ws * o.r[k];
        } else {
            const double ih = 1.0 / sqrt(o.hs);
            v[GK] = o.gs * ih;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[GU + k] = ws * ih * o.v[k];
                v[GQ + k] = ws * o.r[k] + v[GU + k] * v[GK];
            }
            gsm = fmax(gsm, fabs(o.gs));
        }
#pragma unroll
        for (int k = 0; k < kGpPlanes; ++k) rec[(size_t)k * Q.M + m] = v[k];
        pfrozen[m] = o.frozen ? 1 : 0;
    }
    cost = block_sum256(cost, sh);
    const double mx = block_max<256>(gsm, shm);
    if (threadIdx.x == 0) { parts[blockIdx.x] = cost; parts[gridDim.x + blockIdx.x] = mx; }
}
// per camera over its incidence list, in list order: kGpPairSums values (side 0: the camera is the pair's ci and takes +q, side 1: its cj, -q)
__global__ __launch_bounds__(kPairListThreads) void gp_pair_cam_kernel(PairLists L, int64_t M, const double *__restrict__ rec, double *__restrict__ psum) {
    __shared__ double part[kPairListThreads / 64][10];
    __shared__ double part3[kPairListThreads / 64][3];
    const PairWalk k = pair_walk(L);
    double acc[10], gf[3] = {0.0, 0.0, 0.0};   // M (6), sum a, the reduced gradient's part (3); the full gradient's part
#pragma unroll
    for (int c = 0; c < 10; ++c) acc[c] = 0.0;
    for (int64_t e = k.e; e < k.e_end; e += k.step) {
        const int64_t m = L.pair[e];
        const double sg = L.side[e] == 0 ? 1.0 : -1.0;
        double v[kGpPlanes];
        gp_load(rec, (size_t)M, m, v);
        acc[0] += v[GA] - v[GU] * v[GU]; acc[1] -= v[GU] * v[GU + 1]; acc[2] += v[GA] - v[GU + 1] * v[GU + 1];
        acc[3] -= v[GU] * v[GU + 2]; acc[4] -= v[GU + 1] * v[GU + 2]; acc[5] += v[GA] - v[GU + 2] * v[GU + 2];
        acc[6] += v[GA];
#pragma unroll
        for (int c = 0; c < 3; ++c) { acc[7 + c] += sg * v[GQ + c]; gf[c] += sg * (v[GQ + c] - v[GK] * v[GU + c]); }
    }
    if (k.heavy) {   // two reductions, as gp_lm_kernel: fewer wavefront sums in flight
        pair_heavy_sum<3>(gf, part3);
        pair_heavy_sum<10>(acc, part);
    }
    if (k.u >= 0 && (!k.heavy || threadIdx.x == 0)) {
        double *ps = psum + (size_t)kGpPairSums * k.u;
#pragma unroll
        for (int c = 0; c < 10; ++c) ps[c] = acc[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) ps[10 + c] = gf[c];
    }
}
// the pairs' off-diagonal part of S x: yp_i = -sum M_m x_other over the camera's incidence list, gathering the other camera's x (the
// diagonal part sum M_m x_i is in U*_i)
__global__ __launch_bounds__(kPairListThreads) void gp_pairx_kernel(PairLists L, GpPairs Q, const double *__restrict__ rec, const double *__restrict__ x,
                                                                    const BaState *__restrict__ st, double *__restrict__ yp) {
    __shared__ double part[kPairListThreads / 64][3];
    if (st != nullptr && st->done) return;
    const PairWalk k = pair_walk(L);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t e = k.e; e < k.e_end; e += k.step) {
        const int64_t m = L.pair[e];
        const size_t o = 3 * (size_t)(L.side[e] == 0 ? Q.cj[m] : Q.ci[m]);
        const double av = rec[(size_t)GA * Q.M + m], u0 = rec[(size_t)GU * Q.M + m], u1 = rec[(size_t)(GU + 1) * Q.M + m],
                     u2 = rec[(size_t)(GU + 2) * Q.M + m];
        const double d0 = x[o], d1 = x[o + 1], d2 = x[o + 2];
        const double ud = u0 * d0 + u1 * d1 + u2 * d2;
        acc[0] -= av * d0 - u0 * ud; acc[1] -= av * d1 - u1 * ud; acc[2] -= av * d2 - u2 * ud;
    }
    if (k.heavy) pair_heavy_sum<3>(acc, part);
    if (k.u >= 0 && (!k.heavy || threadIdx.x == 0)) {
        const size_t o = 3 * (size_t)k.u;
        yp[o] = acc[0]; yp[o + 1] = acc[1]; yp[o + 2] = acc[2];
    }
}
// candidate: d sigma_m = -(g_sigma - w sigma v.(dc_i - dc_j)) / h* (0 for a frozen one), sigma <- max(sigma + d sigma, 1e-5); the pairs'
// cost at the candidate, model terms, |d sigma|^2 and |sigma|^2 (gp_cand_obs_kernel with camera j in the point's place)
template <int LOSS>
__global__ __launch_bounds__(256) void gp_cand_pair_kernel(GpPairs Q, const double *__restrict__ C, const double *__restrict__ sg,
                                                           const double *__restrict__ dc, const double *__restrict__ Cn, double a, double mu,
                                                           double *__restrict__ sgn, double *__restrict__ dsg, double *__restrict__ parts) {
    __shared__ double sh[4];
    double cost = 0.0, model = 0.0, s2 = 0.0, x2 = 0.0;
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < Q.M; m += (int64_t)gridDim.x * 256) {
        const double s = sg[m];
        const int64_t i = Q.ci[m], j = Q.cj[m];
        GpLin o;
        (void)gp_lin<LOSS>(C + 3 * i, C + 3 * j, Q.tau + (size_t)3 * m, s, a, mu, o);
        double dd[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) dd[k] = dc[3 * i + k] - dc[3 * j + k];
        const double vd = o.v[0] * dd[0] + o.v[1] * dd[1] + o.v[2] * dd[2];
        double ds = 0.0;
        if (!o.frozen) ds = -(o.gs - o.w * s * vd) / o.hs;
        const double s1 = fmax(s + ds, kGpMinScale);
        double rj = 0.0, jj = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double jd = s * dd[k] - o.v[k] * ds;
            rj += o.r[k] * jd; jj += jd * jd;
        }
        model += o.w * (rj + 0.5 * jj);
        GpLin o1;
        cost += 0.5 * gp_lin<LOSS>(Cn + 3 * i, Cn + 3 * j, Q.tau + (size_t)3 * m, s1, a, mu, o1);
        s2 += ds * ds; x2 += s * s;
        sgn[m] = s1;
        dsg[m] = ds;
    }
    cost = block_sum256(cost, sh);
    model = block_sum256(model, sh);
    s2 = block_sum256(s2, sh);
    x2 = block_sum256(x2, sh);
    if (threadIdx.x == 0) {
        const size_t g = gridDim.x;
        parts[blockIdx.x] = cost; parts[g + blockIdx.x] = model; parts[2 * g + blockIdx.x] = s2; parts[3 * g + blockIdx.x] = x2;
    }
}

// One call's device state and the launches on it.  run() (the LM loop) and probe() (the test export xm_ctx_gp_probe) both go through these
// members, so the probe launches what the loop launches: same kernels, grids and arguments.
struct GpWork {
    const SchurOp &SO;
    const GpSettings &cfg;
    hipStream_t st;
    const SchurLists S;
    const int64_t n, m, nobs;
    // parameters on the device, two sets (current, candidate): centres by camera, points by landmark slot, scales in input order
    DevBuf<double> C[2], P[2], Sc[2];
    DevBuf<double> rot, dir, cflag, lflag, Jc, Jl, vinv, gl, ustar, sinv, b, x, r, z, pv, Ap, y, dP, ds, parts;
    DevBuf<int32_t> oused, lm_ok, lused, cused, frozen, state_buf;
    GpState *dst = nullptr;
    Pinned<GpState> hs;
    int ge = 0, gfc = 0, gfl = 0, gcam = 0, glm = 0;
    size_t o_eval = 0, o_gmax = 0, o_pcg = 0, o_cand = 0, o_cost = 0;
    double *pp = nullptr;
    const dim3 b256{256}, blm{kBaHeavyThreads};
    int cur = 0;
    BaPcg a;
    // which terms (xm_gp.h): observation terms, pair terms, fixed centres, weighted observation terms.  Without pairs_in: observations only
    bool has_obs = true, has_pairs = false, fix = false, aw = false;
    std::vector<int32_t> plist;   // the participating pairs' input indices
    int64_t M = 0;
    PairListsDev lists;
    DevBuf<int32_t> ci, cj, pfrozen;
    DevBuf<double> trel, tau, prec, psum, yp, Sg[2], dsg, cam_a;
    GpPairs Q{};
    int gp = 1;
    size_t o_pe = 0, o_pc = 0;

    // the pair terms' host side: which pairs take part, the incidence lists, the weights a_e per camera; fills the outputs of pin
    void setup_pairs(GpPairsIn &pin, const double *sigma0) {
        has_obs = pin.constraint != XM_GP_ONLY_CAMERAS;
        has_pairs = pin.constraint != XM_GP_ONLY_POINTS;
        fix = pin.fix_centres;
        pin.pairs_used = pin.cams_heavy = pin.max_incidences = 0;
        pin.weight_scale_pt = 1.0;
        if (has_pairs) {
            std::vector<int32_t> ua, ub;
            std::vector<double> ht, hs;
            for (int64_t k = 0; k < pin.npairs; ++k) {
                if (pin.valid && !pin.valid[k]) continue;
                plist.push_back((int32_t)k); ua.push_back(pin.pi[k]); ub.push_back(pin.pj[k]);
                for (int c = 0; c < 3; ++c) ht.push_back(pin.trel[3 * k + c]);
                hs.push_back(sigma0 ? sigma0[k] : 1.0);
            }
            M = (int64_t)plist.size();
            if (M < 1) throw Error(XM_ERR_ARG, "xm_ctx_global_positioning_pairs: the constraint type has pair terms but no pair takes part");
            const PairListsHost h = build_pair_lists((int)n, ua, ub, kPairListLight, false);
            lists.upload_from(h, (int)n, st);
            upload(ci, ua.data(), (size_t)M, st); upload(cj, ub.data(), (size_t)M, st); upload(trel, ht.data(), ht.size(), st);
            upload(Sg[0], hs.data(), (size_t)M, st);
            wait_stream(st, cfg.watchdog_s, kStage, "the pair lists");   // the host vectors above end with this scope
            Sg[1].alloc((size_t)M); dsg.alloc((size_t)M); pfrozen.alloc((size_t)M); tau.alloc((size_t)3 * M);
            prec.alloc((size_t)kGpPlanes * M); psum.alloc((size_t)kGpPairSums * n); yp.alloc((size_t)3 * n);
            Q.M = M; Q.ci = ci.p; Q.cj = cj.p; Q.tau = tau.p;
            gp = flat_grid(M);
            pin.pairs_used = M; pin.cams_heavy = h.nheavy; pin.max_incidences = h.max_inc;
            if (pin.constraint == XM_GP_POINTS_AND_CAMERAS_BALANCED) pin.weight_scale_pt = pin.reweight_scale * (double)M / (double)m;
        }
        if (has_obs) {
            std::vector<double> ha((size_t)n, pin.weight_scale_pt);
            aw = pin.weight_scale_pt != 1.0;
            if (pin.calibrated)
                for (int64_t i = 0; i < n; ++i)
                    if (!pin.calibrated[i]) { ha[(size_t)i] = 0.5 * pin.weight_scale_pt; aw = true; }
            if (aw) {
                upload(cam_a, ha.data(), (size_t)n, st);
                wait_stream(st, cfg.watchdog_s, kStage, "the observation weights");
            }
        }
    }

    GpWork(const SchurOp &SO_, const GpSettings &cfg_, const double *rot_h, const double *t, const double *p, const double *s0, hipStream_t st_,
           GpPairsIn *pin = nullptr, const double *sigma0 = nullptr)
        : SO(SO_), cfg(cfg_), st(st_), S(SO_.lists()), n(S.n), m(S.m), nobs(S.nobs) {
        if (n < 1 || m < 1 || nobs < 1)   // no launch below has an empty grid
            throw Error(XM_ERR_ARG, "xm_ctx_global_positioning: the context holds no camera, landmark or observation");
        if (pin) setup_pairs(*pin, sigma0);
        const std::vector<int32_t> &slot_of = SO.slot_of();
        std::vector<double> hP((size_t)3 * m), hS((size_t)std::max<int64_t>(nobs, 1), 1.0);
        for (int64_t l = 0; l < m; ++l)
            for (int k = 0; k < 3; ++k) hP[(size_t)3 * slot_of[(size_t)l] + k] = p[(size_t)3 * l + k];
        if (s0) std::memcpy(hS.data(), s0, (size_t)nobs * sizeof(double));
        for (int k = 0; k < 2; ++k) { C[k].alloc((size_t)3 * n, false); P[k].alloc((size_t)3 * m, false); Sc[k].alloc(hS.size(), false); }
        rot.alloc((size_t)9 * n, false);
        XM_HIP_CHECK(hipMemcpyAsync(rot.p, rot_h, (size_t)9 * n * sizeof(double), hipMemcpyHostToDevice, st));
        XM_HIP_CHECK(hipMemcpyAsync(C[0].p, t, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, st));
        if (fix) XM_HIP_CHECK(hipMemcpyAsync(C[1].p, t, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, st));   // no launch writes a centre
        XM_HIP_CHECK(hipMemcpyAsync(P[0].p, hP.data(), hP.size() * sizeof(double), hipMemcpyHostToDevice, st));
        XM_HIP_CHECK(hipMemcpyAsync(Sc[0].p, hS.data(), hS.size() * sizeof(double), hipMemcpyHostToDevice, st));
        // workspace (zero: the padding of the packed landmark lists stays 0 in every plane and in the flags)
        dir.alloc(3 * hS.size()); cflag.alloc(hS.size()); lflag.alloc((size_t)S.lm_total); oused.alloc(hS.size()); frozen.alloc(hS.size()); ds.alloc(hS.size());
        Jc.alloc((size_t)kGpPlanes * hS.size()); Jl.alloc((size_t)kGpPlanes * S.lm_total);
        vinv.alloc((size_t)6 * m); gl.alloc((size_t)3 * m); y.alloc((size_t)3 * m); dP.alloc((size_t)3 * m); lused.alloc((size_t)m); lm_ok.alloc((size_t)m);
        ustar.alloc((size_t)9 * n); sinv.alloc((size_t)9 * n); cused.alloc((size_t)n);
        for (DevBuf<double> *v : {&b, &x, &r, &z, &pv, &Ap}) v->alloc((size_t)3 * n);
        state_buf.alloc(sizeof(GpState) / sizeof(int32_t) + 2);
        dst = reinterpret_cast<GpState *>(state_buf.p);
        ge = flat_grid(nobs); gfc = flat_grid(n); gfl = flat_grid(m); gcam = qw_grid((int)n);
        glm = (int)(S.nheavy + (m - S.nheavy + kBaHeavyThreads - 1) / kBaHeavyThreads);
        // partials: eval (3 ge) | gmax (glm + gcam) | PCG (4 gfc + gcam) | candidate step / |x| (cameras then landmarks, 2 x (gfc + gfl)) | cost (4 ge)
        o_eval = 0; o_gmax = o_eval + 3 * (size_t)ge; o_pcg = o_gmax + glm + gcam; o_cand = o_pcg + 4 * (size_t)gfc + gcam;
        o_cost = o_cand + 2 * ((size_t)gfc + gfl);
        // behind them, with pair terms: the pairs' eval (2 gp) | the pairs' candidate (4 gp)
        o_pe = o_cost + 4 * (size_t)ge; o_pc = o_pe + (has_pairs ? 2 * (size_t)gp : 0);
        parts.alloc(o_pc + (has_pairs ? 4 * (size_t)gp : 0));
        pp = parts.p;
        a.n = n; a.grid = gfc; a.cgrid = gcam; a.tol2 = cfg.eta * cfg.eta;
        a.b = b.p; a.sinv = sinv.p; a.ustar = ustar.p; a.x = x.p; a.r = r.p; a.z = z.p; a.p = pv.p; a.Ap = Ap.p;
        a.lay_partials(pp + o_pcg);
        a.st = &dst->b;
        // which observations, landmarks and cameras take part: fixed for the call (without observation terms every flag stays 0)
        if (has_obs) {
            hipLaunchKernelGGL(gp_setup_kernel, dim3(ge), b256, 0, st, S, (const double *)rot.p, dir.p, lflag.p);
            hipLaunchKernelGGL(gp_lm_count_kernel, dim3(glm), blm, 0, st, S, (const double *)lflag.p, (double)std::max(cfg.min_views, 1), lm_ok.p);
            hipLaunchKernelGGL(gp_used_kernel, dim3(ge), b256, 0, st, S, (const int32_t *)lm_ok.p, oused.p, cflag.p, lflag.p);
            hipLaunchKernelGGL(gp_lm_count_kernel, dim3(glm), blm, 0, st, S, (const double *)lflag.p, 1.0, lused.p);
            hipLaunchKernelGGL(gp_cam_count_kernel, dim3(gcam), b256, 0, st, S, (const double *)cflag.p, cused.p);
        }
        if (has_pairs) {
            hipLaunchKernelGGL(gp_pair_setup_kernel, dim3(gp), b256, 0, st, M, (const int32_t *)cj.p, (const double *)rot.p, (const double *)trel.p, tau.p);
            hipLaunchKernelGGL(gp_pair_used_kernel, dim3(gfc), b256, 0, st, (int)n, (const int64_t *)lists.ptr.p, cused.p);
        }
        check_launch("the used observations");
    }
    void reduce(BaReduce rd) { hipLaunchKernelGGL(ba_reduce_kernel, dim3(1), b256, 0, st, rd); }
    GpState read_state(const char *what) { return xm::read_state(dst, hs, st, cfg.watchdog_s, kStage, what); }
    // the records, the landmark pass and the camera pass at the current point for the damping mu; cost, used and |J^T r|_inf to the state word
    void linearise(double mu) {
        if (has_obs) {
            with_loss(cfg.loss, [&](auto L) {
                auto launch = [&](auto AW) {
                    hipLaunchKernelGGL((gp_eval_kernel<decltype(L)::value, decltype(AW)::value>), dim3(ge), b256, 0, st, S, (const int32_t *)oused.p, (const double *)dir.p,
                                       (const double *)C[cur].p, (const double *)P[cur].p, (const double *)Sc[cur].p, cfg.loss_scale, mu,
                                       (const double *)cam_a.p, Jc.p, Jl.p, frozen.p, pp + o_eval);
                };
                if (aw) launch(std::true_type{}); else launch(std::false_type{});
            });
            hipLaunchKernelGGL(gp_lm_kernel, dim3(glm), blm, 0, st, S, (const double *)Jl.p, mu, vinv.p, gl.p, pp + o_gmax);
        }
        if (has_pairs) {   // the pairs' records and the per-camera sums the camera pass reads
            with_loss(cfg.loss, [&](auto L) {
                hipLaunchKernelGGL((gp_pair_eval_kernel<L.value>), dim3(gp), b256, 0, st, Q, (const double *)C[cur].p, (const double *)Sg[cur].p,
                                   cfg.loss_scale, mu, prec.p, pfrozen.p, pp + o_pe);
            });
            hipLaunchKernelGGL(gp_pair_cam_kernel, dim3(lists.grid), dim3(kPairListThreads), 0, st, lists.L, M, (const double *)prec.p, psum.p);
            hipLaunchKernelGGL(gp_cam_kernel<true>, dim3(gcam), b256, 0, st, S, (const double *)Jc.p, (const double *)vinv.p, (const double *)gl.p, mu,
                               (const double *)psum.p, has_obs ? 1 : 0, ustar.p, sinv.p, b.p, pp + o_gmax + glm);
            BaReduce rp{};
            rp.sum_p[0] = pp + o_pe; rp.sum_n[0] = gp; rp.sum_out[0] = &dst->pcost;
            rp.max_p = pp + o_pe + gp; rp.max_n = gp; rp.max_out = &dst->pgsmax;
            reduce(rp);
        } else if (!fix) {
            hipLaunchKernelGGL(gp_cam_kernel<false>, dim3(gcam), b256, 0, st, S, (const double *)Jc.p, (const double *)vinv.p, (const double *)gl.p, mu,
                               (const double *)nullptr, 1, ustar.p, sinv.p, b.p, pp + o_gmax + glm);
        }
        BaReduce rd{};
        rd.sum_p[0] = pp + o_eval; rd.sum_n[0] = ge; rd.sum_out[0] = &dst->b.cost;
        rd.sum_p[1] = pp + o_eval + ge; rd.sum_n[1] = ge; rd.sum_out[1] = &dst->b.used;
        rd.max_p = pp + o_gmax; rd.max_n = glm + gcam; rd.max_out = &dst->b.gmax;
        reduce(rd);
        BaReduce rs{};
        rs.max_p = pp + o_eval + 2 * (size_t)ge; rs.max_n = ge; rs.max_out = &dst->gsmax;
        reduce(rs);
    }
    // ar.Ap = S ar.p through the two lists (gate: the state word whose done flag skips the landmark side, or null)
    void sx(const BaPcg &ar, const BaState *gate) {
        if (has_obs)
            hipLaunchKernelGGL(gp_lmx_kernel, dim3(glm), blm, 0, st, S, (const double *)Jl.p, (const double *)vinv.p, (const double *)nullptr, 1.0,
                               (const int32_t *)lused.p, (const double *)ar.p, gate, y.p);
        if (has_pairs) {
            hipLaunchKernelGGL(gp_pairx_kernel, dim3(lists.grid), dim3(kPairListThreads), 0, st, lists.L, Q, (const double *)prec.p, (const double *)ar.p,
                               gate, yp.p);
            hipLaunchKernelGGL(gp_camx_kernel<true>, dim3(gcam), b256, 0, st, S, (const double *)Jc.p, (const double *)y.p, (const double *)yp.p,
                               has_obs ? 1 : 0, ar);
        } else {
            hipLaunchKernelGGL(gp_camx_kernel<false>, dim3(gcam), b256, 0, st, S, (const double *)Jc.p, (const double *)y.p, (const double *)nullptr, 1, ar);
        }
    }
    // back-substitution, candidate (the other parameter set), its cost and the model decrease; the scalars to the state word
    void candidate(double mu, const double *dc) {
        const int nx = cur ^ 1;
        // fixed centres: dc is the zero vector, no centre is written (both sets hold the caller's) and the cameras' partials stay 0
        if (has_obs)
            hipLaunchKernelGGL(gp_lmx_kernel, dim3(glm), blm, 0, st, S, (const double *)Jl.p, (const double *)vinv.p, (const double *)gl.p, -1.0,
                               (const int32_t *)lused.p, dc, (const BaState *)nullptr, dP.p);
        if (!fix)
            hipLaunchKernelGGL(ba_cand_vec_kernel<3>, dim3(gfc), b256, 0, st, n, (const double *)C[cur].p, dc, (const int32_t *)cused.p, C[nx].p, pp + o_cand);
        if (has_obs) {
            hipLaunchKernelGGL(ba_cand_vec_kernel<3>, dim3(gfl), b256, 0, st, m, (const double *)P[cur].p, (const double *)dP.p, (const int32_t *)lused.p,
                               P[nx].p, pp + o_cand + 2 * (size_t)gfc);
            with_loss(cfg.loss, [&](auto L) {
                auto launch = [&](auto AW) {
                    hipLaunchKernelGGL((gp_cand_obs_kernel<decltype(L)::value, decltype(AW)::value>), dim3(ge), b256, 0, st, S, (const int32_t *)oused.p, (const double *)dir.p,
                                       (const double *)C[cur].p, (const double *)P[cur].p, (const double *)Sc[cur].p, dc, (const double *)dP.p,
                                       (const double *)C[nx].p, (const double *)P[nx].p, cfg.loss_scale, mu, (const double *)cam_a.p, Sc[nx].p, ds.p,
                                       pp + o_cost);
                };
                if (aw) launch(std::true_type{}); else launch(std::false_type{});
            });
        }
        if (has_pairs) {
            with_loss(cfg.loss, [&](auto L) {
                hipLaunchKernelGGL((gp_cand_pair_kernel<L.value>), dim3(gp), b256, 0, st, Q, (const double *)C[cur].p, (const double *)Sg[cur].p, dc,
                                   (const double *)C[nx].p, cfg.loss_scale, mu, Sg[nx].p, dsg.p, pp + o_pc);
            });
            BaReduce rp{};
            for (int k = 0; k < 4; ++k) { rp.sum_p[k] = pp + o_pc + (size_t)k * gp; rp.sum_n[k] = gp; }
            rp.sum_out[0] = &dst->pcost_new; rp.sum_out[1] = &dst->pmodel; rp.sum_out[2] = &dst->pstep2; rp.sum_out[3] = &dst->px2;
            reduce(rp);
        }
        reduce(candidate_sums(pp + o_cost, ge, pp + o_cand, gfc, gfl, &dst->b));
        BaReduce rs{};
        rs.sum_p[0] = pp + o_cost + 2 * (size_t)ge; rs.sum_n[0] = ge; rs.sum_out[0] = &dst->step2s;
        rs.sum_p[1] = pp + o_cost + 3 * (size_t)ge; rs.sum_n[1] = ge; rs.sum_out[1] = &dst->x2s;
        reduce(rs);
    }
    // per-landmark array: device slot order -> input order
    void lm_out(const double *dev, int w, double *outp, std::vector<double> &tmp) {
        const std::vector<int32_t> &slot_of = SO.slot_of();
        tmp.resize((size_t)w * m);
        XM_HIP_CHECK(hipMemcpyAsync(tmp.data(), dev, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "a landmark array");
        for (int64_t l = 0; l < m; ++l)
            for (int k = 0; k < w; ++k) outp[(size_t)w * l + k] = tmp[(size_t)w * slot_of[(size_t)l] + k];
    }
    // the caller's t, p and scales from parameter set k: what is not used keeps the caller's bits (scales: -1)
    void to_caller(int k, double *t, double *p, double *scales) {
        const std::vector<int32_t> &slot_of = SO.slot_of();
        std::vector<double> hC((size_t)3 * n), hP((size_t)3 * m), hS((size_t)nobs);
        std::vector<int32_t> cu((size_t)n), lu((size_t)m), ou((size_t)nobs);
        XM_HIP_CHECK(hipMemcpyAsync(hC.data(), C[k].p, hC.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(hP.data(), P[k].p, hP.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(cu.data(), cused.p, cu.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(lu.data(), lused.p, lu.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (scales && nobs > 0) {
            XM_HIP_CHECK(hipMemcpyAsync(hS.data(), Sc[k].p, hS.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(ou.data(), oused.p, ou.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        wait_stream(st, cfg.watchdog_s, kStage, "the positions");
        for (int64_t i = 0; i < n && !fix; ++i)
            if (cu[(size_t)i])
                for (int c = 0; c < 3; ++c) t[(size_t)3 * i + c] = hC[(size_t)3 * i + c];
        for (int64_t l = 0; l < m; ++l) {
            const int32_t sl = slot_of[(size_t)l];
            if (!lu[(size_t)sl]) continue;
            for (int c = 0; c < 3; ++c) p[(size_t)3 * l + c] = hP[(size_t)3 * sl + c];
        }
        if (scales)
            for (int64_t e = 0; e < nobs; ++e) scales[e] = ou[(size_t)e] ? hS[(size_t)e] : -1.0;
    }
};

// sigma of the participating pairs from parameter set k, by input index; -1 for a pair that takes no part
void pairs_to_caller(GpWork &W, int k, int64_t npairs, double *sigma) {
    std::vector<double> hs;
    download(hs, (const double *)W.Sg[k].p, (size_t)W.M, W.st);
    wait_stream(W.st, W.cfg.watchdog_s, kStage, "the pair scales");
    std::fill(sigma, sigma + npairs, -1.0);
    for (size_t q = 0; q < W.plist.size(); ++q) sigma[W.plist[q]] = hs[q];
}

void run(const SchurOp &SO, const GpSettings &cfg, GpPairsIn *pin, const double *rot, double *t, double *p, double *scales, GpOutcome &out,
         hipStream_t st) {
    const auto t_start = std::chrono::steady_clock::now();
    GpWork W(SO, cfg, rot, t, p, nullptr, st, pin);
    int pcg_last = 8;
    // the PCG's batch driver with this solver's product; the PCG's state word is the one GpState embeds
    PcgHooks hooks;
    hooks.product = [&] { W.sx(W.a, &W.dst->b); };
    hooks.read = [&] { return W.read_state("the reduced camera PCG").b; };

    // the LM loop (xm_lm_loop.h) over this solver's launches and reads; the records depend on mu and are written again in every iteration
    const LmRules rules{cfg.max_iters, cfg.function_tol, cfg.gradient_tol, cfg.parameter_tol};
    LmHooks lm;
    lm.linearise = [&](double mu, bool) { W.linearise(mu); };
    lm.read_point = [&](LmRead which) {
        const GpState s = W.read_state(which == kLmReadFinal ? "the final gradient" : "the cost and gradient");
        if (which == kLmReadFirst && !std::isfinite(s.b.cost)) throw Error(XM_ERR_ARG, "xm_ctx_global_positioning: the initial cost is not finite");
        if (W.has_pairs) return LmPoint{s.b.cost + s.pcost, std::max(std::max(s.b.gmax, s.gsmax), s.pgsmax), s.b.used};
        return LmPoint{s.b.cost, std::max(s.b.gmax, s.gsmax), s.b.used};
    };
    lm.solve = [&] {
        if (W.fix) return LmSolve{0, 0.0};   // dc = 0: the PCG's solution vector is never written
        const PcgResult pr = pcg_solve_batched<3>(W.a, W.gfc, st, pcg_last, hooks);
        return LmSolve{pr.iters, pr.relres};
    };
    lm.read_candidate = [&](double mu) {
        W.candidate(mu, W.x.p);
        const GpState s = W.read_state("the candidate's cost");
        if (W.has_pairs)
            return LmCandidate{s.b.cost_new + s.pcost_new, s.b.model + s.pmodel, s.b.step2[0] + s.b.step2[1] + s.step2s + s.pstep2,
                               s.b.x2[0] + s.b.x2[1] + s.x2s + s.px2};
        return LmCandidate{s.b.cost_new, s.b.model, s.b.step2[0] + s.b.step2[1] + s.step2s, s.b.x2[0] + s.b.x2[1] + s.x2s};
    };
    lm.accept = [&](bool) { W.cur ^= 1; };
    lm.out_of_time = [&] { return secs_since(t_start) >= cfg.max_time; };
    const LmResult res = lm_loop(rules, lm);
    W.to_caller(W.cur, t, p, scales);
    if (W.has_pairs && pin->sigma) pairs_to_caller(W, W.cur, pin->npairs, pin->sigma);
    out.initial_cost = res.initial_cost; out.n_used = (int64_t)res.n_used;
    out.status = res.status; out.iters = res.iters; out.accepted = res.accepted; out.pcg_iters = res.pcg_total;
    out.final_cost = res.final_cost; out.gradient_max = res.gmax; out.trace_len = lm_copy_trace(res, cfg.trace, cfg.trace_cap);
    out.seconds = secs_since(t_start);
}

}  // namespace

void global_positioning(const SchurOp &S, const GpSettings &cfg, const double *rot, double *t, double *p, double *scales, GpOutcome &out, hipStream_t st) {
    out = GpOutcome();
    run(S, cfg, nullptr, rot, t, p, scales, out, st);
}
void global_positioning_pairs(const SchurOp &S, const GpSettings &cfg, GpPairsIn &pairs, const double *rot, double *t, double *p, double *scales,
                              GpOutcome &out, hipStream_t st) {
    out = GpOutcome();
    run(S, cfg, &pairs, rot, t, p, scales, out, st);
    if (pairs.constraint == XM_GP_ONLY_POINTS && pairs.sigma) std::fill(pairs.sigma, pairs.sigma + pairs.npairs, -1.0);
}

// The test export xm_ctx_gp_probe: one linearisation at (t, p, s) with the damping mu, then whatever the caller asked for, every array
// brought back in the caller's index order.  Only GpWork's members launch kernels here.
namespace {
void probe(const SchurOp &SO, const GpSettings &cfg, GpPairsIn *pin, const double *rot, const double *t, const double *p, GpProbe &q, GpPairProbe *pq,
           hipStream_t st) {
    GpWork W(SO, cfg, rot, t, p, q.s, st, pin, pq ? pq->sigma_in : nullptr);
    const int64_t n = W.n, m = W.m, nobs = W.nobs, nd = 3 * n;
    auto d2h = [&](void *dstp, const void *src, size_t bytes) { XM_HIP_CHECK(hipMemcpyAsync(dstp, src, bytes, hipMemcpyDeviceToHost, st)); };
    auto sync = [&](const char *what) { check_launch(what); wait_stream(st, cfg.watchdog_s, kStage, what); };
    std::vector<double> tmp;
    W.linearise(q.mu);
    const GpState s0 = W.read_state("the probe's passes");
    q.cost = s0.b.cost; q.n_used = (int64_t)s0.b.used; q.gmax = std::max(s0.b.gmax, s0.gsmax);
    const int64_t np = pin ? pin->npairs : 0;
    if (W.has_pairs) {   // the pairs' records and flags, by input index
        q.gmax = std::max(q.gmax, s0.pgsmax);
        pq->cost = s0.pcost; pq->gsmax = s0.pgsmax;
        std::vector<double> rec;
        std::vector<int32_t> fz;
        download(rec, (const double *)W.prec.p, (size_t)kGpPlanes * W.M, st);
        download(fz, (const int32_t *)W.pfrozen.p, (size_t)W.M, st);
        sync("the pairs' records");
        if (pq->Mp) std::fill(pq->Mp, pq->Mp + 6 * np, 0.0);
        if (pq->qp) std::fill(pq->qp, pq->qp + 3 * np, 0.0);
        if (pq->pfrozen) std::fill(pq->pfrozen, pq->pfrozen + np, 0);
        if (pq->pused) std::fill(pq->pused, pq->pused + np, 0);
        for (int64_t k = 0; k < W.M; ++k) {
            const int64_t e = W.plist[(size_t)k];
            auto pl = [&](int c) { return rec[(size_t)c * W.M + (size_t)k]; };
            const double a = pl(GA), u[3] = {pl(GU), pl(GU + 1), pl(GU + 2)};
            if (pq->Mp) {
                double *Mm = pq->Mp + (size_t)6 * e;
                Mm[0] = a - u[0] * u[0]; Mm[1] = -u[0] * u[1]; Mm[2] = -u[0] * u[2]; Mm[3] = a - u[1] * u[1]; Mm[4] = -u[1] * u[2]; Mm[5] = a - u[2] * u[2];
            }
            if (pq->qp)
                for (int c = 0; c < 3; ++c) pq->qp[(size_t)3 * e + c] = pl(GQ + c);
            if (pq->pfrozen) pq->pfrozen[e] = fz[(size_t)k];
            if (pq->pused) pq->pused[e] = 1;
        }
    }
    if (q.M || q.q) {   // records by camera position -> input order; M_e = a I - u u^T
        std::vector<double> rec((size_t)kGpPlanes * nobs);
        std::vector<int64_t> pos((size_t)nobs);
        d2h(rec.data(), W.Jc.p, rec.size() * sizeof(double));
        d2h(pos.data(), W.S.pos_c, pos.size() * sizeof(int64_t));
        sync("the records");
        for (int64_t e = 0; e < nobs; ++e) {
            auto pl = [&](int k) { return rec[(size_t)k * nobs + (size_t)pos[(size_t)e]]; };
            const double a = pl(GA), u[3] = {pl(GU), pl(GU + 1), pl(GU + 2)};
            if (q.M) {
                double *M = q.M + (size_t)6 * e;
                M[0] = a - u[0] * u[0]; M[1] = -u[0] * u[1]; M[2] = -u[0] * u[2]; M[3] = a - u[1] * u[1]; M[4] = -u[1] * u[2]; M[5] = a - u[2] * u[2];
            }
            if (q.q)
                for (int k = 0; k < 3; ++k) q.q[(size_t)3 * e + k] = pl(GQ + k);
        }
    }
    if (q.frozen) d2h(q.frozen, W.frozen.p, (size_t)nobs * sizeof(int32_t));
    if (q.oused) d2h(q.oused, W.oused.p, (size_t)nobs * sizeof(int32_t));
    if (q.b) d2h(q.b, W.b.p, (size_t)nd * sizeof(double));
    if (q.ustar) d2h(q.ustar, W.ustar.p, (size_t)3 * nd * sizeof(double));
    if (q.sinv) d2h(q.sinv, W.sinv.p, (size_t)3 * nd * sizeof(double));
    if (q.cused) d2h(q.cused, W.cused.p, (size_t)n * sizeof(int32_t));
    sync("the camera arrays");
    if (q.g_l) W.lm_out(W.gl.p, 3, q.g_l, tmp);
    if (q.vinv) W.lm_out(W.vinv.p, 6, q.vinv, tmp);
    if (q.lused) {
        const std::vector<int32_t> &slot_of = SO.slot_of();
        std::vector<int32_t> lu((size_t)m);
        d2h(lu.data(), W.lused.p, (size_t)m * sizeof(int32_t));
        sync("the landmark flags");
        for (int64_t l = 0; l < m; ++l) q.lused[l] = lu[(size_t)slot_of[(size_t)l]];
    }
    // S X: column j into the PCG's direction vector, the product pair, A p back (the state word's done flag is 0: nothing has set it)
    if (q.SX && !W.fix)
        for (int64_t j = 0; j < q.k; ++j) {
            XM_HIP_CHECK(hipMemcpyAsync(W.pv.p, q.X + (size_t)nd * j, (size_t)nd * sizeof(double), hipMemcpyHostToDevice, st));
            W.sx(W.a, &W.dst->b);
            d2h(q.SX + (size_t)nd * j, W.Ap.p, (size_t)nd * sizeof(double));
            sync("the product S x");
        }
    if (q.dc) {
        if (!W.fix) XM_HIP_CHECK(hipMemcpyAsync(W.x.p, q.dc, (size_t)nd * sizeof(double), hipMemcpyHostToDevice, st));   // fixed centres: x stays 0
        W.candidate(q.mu, W.x.p);
        const GpState s = W.read_state("the probe's candidate");
        q.cost1 = s.b.cost_new; q.model = s.b.model;
        q.step2[0] = s.b.step2[0]; q.step2[1] = s.b.step2[1]; q.step2[2] = s.step2s;
        q.x2[0] = s.b.x2[0]; q.x2[1] = s.b.x2[1]; q.x2[2] = s.x2s;
        if (q.dP) W.lm_out(W.dP.p, 3, q.dP, tmp);
        if (q.ds) { d2h(q.ds, W.ds.p, (size_t)nobs * sizeof(double)); sync("the scale steps"); }
        if (q.t1 || q.p1 || q.s1) {   // as the loop returns them: what is not used keeps the caller's bits
            std::vector<double> t1(t, t + 3 * n), p1(p, p + 3 * m), s1((size_t)nobs);
            W.to_caller(1, t1.data(), p1.data(), s1.data());
            if (q.t1) std::memcpy(q.t1, t1.data(), t1.size() * sizeof(double));
            if (q.p1) std::memcpy(q.p1, p1.data(), p1.size() * sizeof(double));
            if (q.s1) std::memcpy(q.s1, s1.data(), s1.size() * sizeof(double));
        }
        if (W.has_pairs) {
            pq->cost1 = s.pcost_new; pq->model = s.pmodel; pq->step2 = s.pstep2; pq->x2 = s.px2;
            if (pq->sigma1) pairs_to_caller(W, 1, np, pq->sigma1);
            if (pq->dsigma) {
                std::vector<double> hd;
                download(hd, (const double *)W.dsg.p, (size_t)W.M, st);
                sync("the pair scale steps");
                std::fill(pq->dsigma, pq->dsigma + np, 0.0);
                for (int64_t k = 0; k < W.M; ++k) pq->dsigma[W.plist[(size_t)k]] = hd[(size_t)k];
            }
        }
    }
    if (pq && !W.has_pairs) {   // no pair terms: nothing takes part
        if (pq->Mp) std::fill(pq->Mp, pq->Mp + 6 * np, 0.0);
        if (pq->qp) std::fill(pq->qp, pq->qp + 3 * np, 0.0);
        if (pq->pfrozen) std::fill(pq->pfrozen, pq->pfrozen + np, 0);
        if (pq->pused) std::fill(pq->pused, pq->pused + np, 0);
        if (pq->dsigma) std::fill(pq->dsigma, pq->dsigma + np, 0.0);
        if (pq->sigma1) std::fill(pq->sigma1, pq->sigma1 + np, -1.0);
    }
}
}  // namespace

void gp_probe(const SchurOp &SO, const GpSettings &cfg, const double *rot, const double *t, const double *p, GpProbe &q, hipStream_t st) {
    probe(SO, cfg, nullptr, rot, t, p, q, nullptr, st);
}
void gp_probe_pairs(const SchurOp &SO, const GpSettings &cfg, GpPairsIn &pairs, const double *rot, const double *t, const double *p, GpProbe &q,
                    GpPairProbe &pq, hipStream_t st) {
    pq.cost = pq.gsmax = pq.cost1 = pq.model = pq.step2 = pq.x2 = 0.0;
    probe(SO, cfg, &pairs, rot, t, p, q, &pq, st);
}

void gp_limits(int64_t out[3]) {
    out[0] = kSchurHeavy; out[1] = 64; out[2] = kBaHeavyThreads;
}
void gp_pair_limits(int64_t out[2]) {
    out[0] = kPairListLight; out[1] = kPairListThreads;
}

}  // namespace xm
