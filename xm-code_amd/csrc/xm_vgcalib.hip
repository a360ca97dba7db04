// xm_vgcalib.hip — focal lengths from the view graph on the device (xm_vgcalib.h has the list of launches, include/xm_amd.h the rules).
#include "xm_vgcalib.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "xm_lm_loop.h"
#include "xm_lm_shared.h"
#include "xm_pair_lists.h"
#include "xm_stage.h"

// every product and every sum of the contract is rounded on its own
#pragma clang fp contract(off)

namespace xm {

namespace {

constexpr const char *kStage = "xm_view_graph_calibrate";
constexpr int kT = kVgcThreads;
static_assert(kVgcMaxPcgIters == kBaMaxPcgIters, "the limit reported is the one the PCG runs to");

// ---- rule 7: F = K2^-T [t]x R K1^-1 for the pairs that flip, the inverse of a pinhole K in closed form
__global__ __launch_bounds__(kT) void vgc_config_kernel(int nflip, const int32_t *__restrict__ flip, const int32_t *__restrict__ ca,
                                                        const int32_t *__restrict__ cb, const double *__restrict__ focal0, const double *__restrict__ pp,
                                                        const double *__restrict__ Rrel, const double *__restrict__ trel, double *__restrict__ F) {
    const int t = blockIdx.x * kT + threadIdx.x;
    if (t >= nflip) return;
    const int64_t k = flip[t];
    const int32_t c1 = ca[t], c2 = cb[t];
    const double *R = Rrel + 9 * k, *tr = trel + 3 * k;
    const double t0 = tr[0], t1 = tr[1], t2 = tr[2];
    double E[3][3], A[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        E[0][j] = t1 * R[6 + j] - t2 * R[3 + j];
        E[1][j] = t2 * R[j] - t0 * R[6 + j];
        E[2][j] = t0 * R[3 + j] - t1 * R[j];
    }
    const double a2 = 1.0 / focal0[c2], x2 = -pp[2 * c2] / focal0[c2], y2 = -pp[2 * c2 + 1] / focal0[c2];
    const double a1 = 1.0 / focal0[c1], x1 = -pp[2 * c1] / focal0[c1], y1 = -pp[2 * c1 + 1] / focal0[c1];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        A[0][j] = a2 * E[0][j];
        A[1][j] = a2 * E[1][j];
        A[2][j] = (x2 * E[0][j] + y2 * E[1][j]) + E[2][j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        F[9 * k + 3 * i] = A[i][0] * a1;
        F[9 * k + 3 * i + 1] = A[i][1] * a1;
        F[9 * k + 3 * i + 2] = (A[i][0] * x1 + A[i][1] * y1) + A[i][2];
    }
}

// ---- rule 1: the one-sided Jacobi SVD of G, columns P and Q of A and V rotated until they are orthogonal
template <int P, int Q>
__device__ __forceinline__ bool jacobi_rotate(double (&A)[3][3], double (&V)[3][3]) {
    const double alpha = (A[0][P] * A[0][P] + A[1][P] * A[1][P]) + A[2][P] * A[2][P];
    const double beta = (A[0][Q] * A[0][Q] + A[1][Q] * A[1][Q]) + A[2][Q] * A[2][Q];
    const double gamma = (A[0][P] * A[0][Q] + A[1][P] * A[1][Q]) + A[2][P] * A[2][Q];
    if (gamma == 0.0 || !(fabs(gamma) > 4.440892098500626e-16 * sqrt(alpha * beta))) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double ap = A[r][P], aq = A[r][Q], vp = V[r][P], vq = V[r][Q];
        A[r][P] = c * ap - s * aq; A[r][Q] = s * ap + c * aq;
        V[r][P] = c * vp - s * vq; V[r][Q] = s * vp + c * vq;
    }
    return true;
}
template <int P, int Q>
__device__ __forceinline__ void order_columns(double (&A)[3][3], double (&V)[3][3], double (&s)[3]) {   // the larger singular value first
    const bool sw = s[Q] > s[P];
    const double sp = s[P], sq = s[Q];
    s[P] = sw ? sq : sp; s[Q] = sw ? sp : sq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double ap = A[r][P], aq = A[r][Q], vp = V[r][P], vq = V[r][Q];
        A[r][P] = sw ? aq : ap; A[r][Q] = sw ? ap : aq;
        V[r][P] = sw ? vq : vp; V[r][Q] = sw ? vp : vq;
    }
}
__global__ __launch_bounds__(kT) void vgc_setup_kernel(int M, const int32_t *__restrict__ plist, const int32_t *__restrict__ ca,
                                                       const int32_t *__restrict__ cb, const double *__restrict__ pp, const double *__restrict__ F,
                                                       double *__restrict__ d) {
    const int m = blockIdx.x * kT + threadIdx.x;
    if (m >= M) return;
    const double *Fk = F + (size_t)9 * plist[m];
    const double px0 = pp[2 * ca[m]], py0 = pp[2 * ca[m] + 1], px1 = pp[2 * cb[m]], py1 = pp[2 * cb[m] + 1];
    double A[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // F K0
        A[i][0] = Fk[3 * i]; A[i][1] = Fk[3 * i + 1];
        A[i][2] = (Fk[3 * i] * px0 + Fk[3 * i + 1] * py0) + Fk[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {   // K1^T (F K0)
        A[2][j] = (px1 * A[0][j] + py1 * A[1][j]) + A[2][j];
        V[0][j] = j == 0 ? 1.0 : 0.0; V[1][j] = j == 1 ? 1.0 : 0.0; V[2][j] = j == 2 ? 1.0 : 0.0;
    }
    bool rotated = true;
    for (int sweep = 0; sweep < kVgcSweeps && rotated; ++sweep) {
        rotated = jacobi_rotate<0, 1>(A, V);
        rotated = jacobi_rotate<0, 2>(A, V) || rotated;
        rotated = jacobi_rotate<1, 2>(A, V) || rotated;
    }
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = sqrt((A[0][k] * A[0][k] + A[1][k] * A[1][k]) + A[2][k] * A[2][k]);
    order_columns<0, 1>(A, V, s);
    order_columns<1, 2>(A, V, s);
    order_columns<0, 1>(A, V, s);
    double u0[3], u1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u0[r] = s[0] > 0.0 ? A[r][0] / s[0] : 0.0;
        u1[r] = s[1] > 0.0 ? A[r][1] / s[1] : 0.0;
    }
    const double s00 = s[0] * s[0], s01 = s[0] * s[1], s11 = s[1] * s[1];
    const double ai[3] = {s00 * (V[0][0] * V[0][0] + V[1][0] * V[1][0]), s01 * (V[0][0] * V[0][1] + V[1][0] * V[1][1]),
                          s11 * (V[0][1] * V[0][1] + V[1][1] * V[1][1])};
    const double aj[3] = {u1[0] * u1[0] + u1[1] * u1[1], -(u0[0] * u1[0] + u0[1] * u1[1]), u0[0] * u0[0] + u0[1] * u0[1]};
    const double bi[3] = {s00 * V[2][0] * V[2][0], s01 * V[2][0] * V[2][1], s11 * V[2][1] * V[2][1]};
    const double bj[3] = {u1[2] * u1[2], -(u0[2] * u1[2]), u0[2] * u0[2]};
    const size_t Ms = (size_t)M;
    // fetzer_d(., u, v): d_01 is (u, v) = (1, 0), d_12 is (2, 1)
    d[0 * Ms + m] = ai[1] * aj[0] - ai[0] * aj[1];
    d[1 * Ms + m] = ai[1] * bj[0] - ai[0] * bj[1];
    d[2 * Ms + m] = bi[1] * aj[0] - bi[0] * aj[1];
    d[3 * Ms + m] = bi[1] * bj[0] - bi[0] * bj[1];
    d[4 * Ms + m] = ai[2] * aj[1] - ai[1] * aj[2];
    d[5 * Ms + m] = ai[2] * bj[1] - ai[1] * bj[2];
    d[6 * Ms + m] = bi[2] * aj[1] - bi[1] * aj[2];
    d[7 * Ms + m] = bi[2] * bj[1] - bi[1] * bj[2];
}

// ---- rule 2: the residual of pair m at (fi, fj); the intermediate values the Jacobian needs
struct VgcRes {
    double r0, r1, fi2, fj2, di, dj, n0, n1, K0, K1;
    bool di_set, dj_set;   // the denominator was replaced by 1e-6: it no longer depends on the focal
};
__device__ __forceinline__ VgcRes vgc_residual(const double *__restrict__ d, size_t M, int m, double fi, double fj) {
    VgcRes o;
    const double d0 = d[m], d1 = d[M + m], d2 = d[2 * M + m], d3 = d[3 * M + m];
    const double e0 = d[4 * M + m], e1 = d[5 * M + m], e2 = d[6 * M + m], e3 = d[7 * M + m];
    o.fi2 = fi * fi; o.fj2 = fj * fj;
    o.di = o.fj2 * d0 + d1;
    o.dj = o.fi2 * e0 + e2;
    o.di_set = o.di == 0.0; o.dj_set = o.dj == 0.0;
    if (o.di_set) o.di = 1e-6;
    if (o.dj_set) o.dj = 1e-6;
    o.n0 = o.fj2 * d2 + d3;
    o.n1 = o.fi2 * e1 + e3;
    o.K0 = -(o.n0 / o.di);
    o.K1 = -(o.n1 / o.dj);
    o.r0 = (o.fi2 - o.K0) / o.fi2;
    o.r1 = (o.fj2 - o.K1) / o.fj2;
    return o;
}

struct VgcPairs {   // the participating pairs on the device
    int M;
    const int32_t *ca, *cb;   // camera of image_id1 (fi) and of image_id2 (fj)
    const int32_t *ua, *ub;   // their unknowns, -1 for a constant camera
    const double *d;          // eight planes of M
};

// rules 2 and 3 at the focals f: raw residual (2 planes), corrector-scaled record (6 planes: r0, r1, dr0/dfi, dr0/dfj, dr1/dfi, dr1/dfj; a
// same-camera pair holds the sums of the two partials in planes 2 and 4 and zeros in 3 and 5), cost per workgroup
__global__ __launch_bounds__(kT) void vgc_eval_kernel(VgcPairs P, const double *__restrict__ f, double a, double *__restrict__ rraw,
                                                      double *__restrict__ rec, double *__restrict__ parts) {
    __shared__ double sh[4];
    const int m = blockIdx.x * kT + threadIdx.x;
    const size_t M = (size_t)P.M;
    double cost = 0.0;
    if (m < P.M) {
        const int32_t c0 = P.ca[m], c1 = P.cb[m];
        const double fi = f[c0], fj = f[c1];
        const VgcRes o = vgc_residual(P.d, M, m, fi, fj);
        const double d0 = P.d[m], d2 = P.d[2 * M + m], e0 = P.d[4 * M + m], e1 = P.d[5 * M + m];
        // r0 = 1 - K0 / fi^2, K0 = -n0 / di; r1 = 1 - K1 / fj^2, K1 = -n1 / dj
        const double dK0 = -((2.0 * fj * d2) * o.di - o.n0 * (o.di_set ? 0.0 : 2.0 * fj * d0)) / (o.di * o.di);
        const double dK1 = -((2.0 * fi * e1) * o.dj - o.n1 * (o.dj_set ? 0.0 : 2.0 * fi * e0)) / (o.dj * o.dj);
        double j00 = (2.0 * o.K0) / (o.fi2 * fi), j01 = -(dK0 / o.fi2), j10 = -(dK1 / o.fj2), j11 = (2.0 * o.K1) / (o.fj2 * fj);
        if (c0 == c1) { j00 = j00 + j01; j10 = j10 + j11; j01 = 0.0; j11 = 0.0; }
        double rho1;
        cost = 0.5 * ba_rho<XM_BA_LOSS_CAUCHY>(o.r0 * o.r0 + o.r1 * o.r1, a, rho1);
        const double w = sqrt(rho1);
        rraw[m] = o.r0; rraw[M + m] = o.r1;
        rec[m] = w * o.r0; rec[M + m] = w * o.r1;
        rec[2 * M + m] = w * j00; rec[3 * M + m] = w * j01; rec[4 * M + m] = w * j10; rec[5 * M + m] = w * j11;
    }
    cost = block_sum256(cost, sh);
    if (threadIdx.x == 0) parts[blockIdx.x] = cost;
}

// the candidate: cost at fnew and the model's r.Jd + |Jd|^2 / 2 at the step x from the records
__global__ __launch_bounds__(kT) void vgc_cand_kernel(VgcPairs P, const double *__restrict__ fnew, const double *__restrict__ x, double a,
                                                      const double *__restrict__ rec, double *__restrict__ parts) {
    __shared__ double sh[4];
    const int m = blockIdx.x * kT + threadIdx.x;
    const size_t M = (size_t)P.M;
    double cost = 0.0, model = 0.0;
    if (m < P.M) {
        const VgcRes o = vgc_residual(P.d, M, m, fnew[P.ca[m]], fnew[P.cb[m]]);
        double rho1;
        cost = 0.5 * ba_rho<XM_BA_LOSS_CAUCHY>(o.r0 * o.r0 + o.r1 * o.r1, a, rho1);
        const int32_t u0 = P.ua[m], u1 = P.ub[m];
        const double xa = u0 >= 0 ? x[u0] : 0.0, xb = u1 >= 0 ? x[u1] : 0.0;
        const double t0 = rec[2 * M + m] * xa + rec[3 * M + m] * xb, t1 = rec[4 * M + m] * xa + rec[5 * M + m] * xb;
        model = (rec[m] * t0 + rec[M + m] * t1) + 0.5 * (t0 * t0 + t1 * t1);
    }
    cost = block_sum256(cost, sh);
    model = block_sum256(model, sh);
    if (threadIdx.x == 0) { parts[blockIdx.x] = cost; parts[gridDim.x + blockIdx.x] = model; }
}

// the lists of the free cameras (xm_pair_lists.h): side 0 the camera is fi's, 1 fj's, 2 both (a same-camera pair)
// gradient g = J^T r and diagonal of J^T J per free camera; b = -g, sinv = 1 / (diag + mu clamp(diag)); |g|_inf per workgroup
__global__ __launch_bounds__(kT) void vgc_cam_kernel(PairLists L, int M_, const double *__restrict__ rec, double mu, double *__restrict__ grad,
                                                     double *__restrict__ diag, double *__restrict__ b, double *__restrict__ sinv,
                                                     double *__restrict__ gmaxp) {
    __shared__ double part[4][2];
    __shared__ double shm[4];
    const size_t M = (size_t)M_;
    const PairWalk w = pair_walk(L);
    double acc[2] = {0.0, 0.0};
    for (int64_t e = w.e; e < w.e_end; e += w.step) {
        const int m = L.pair[e];
        const bool second = L.side[e] == 1;
        const double c0 = rec[(second ? 3 : 2) * M + m], c1 = rec[(second ? 5 : 4) * M + m];
        acc[0] += c0 * rec[m] + c1 * rec[M + m];
        acc[1] += c0 * c0 + c1 * c1;
    }
    if (w.heavy) pair_heavy_sum<2>(acc, part);
    const bool writer = w.u >= 0 && (!w.heavy || threadIdx.x == 0);
    if (writer) {
        const double dd = acc[1] + mu * clamp_diag(acc[1]);
        grad[w.u] = acc[0]; diag[w.u] = acc[1]; b[w.u] = -acc[0]; sinv[w.u] = dd > 0.0 ? 1.0 / dd : 0.0;
    }
    const double gm = block_max<kT>(writer ? fabs(acc[0]) : 0.0, shm);
    if (threadIdx.x == 0) gmaxp[blockIdx.x] = gm;
}

// Ap = (J^T J + mu clamp(diag)) p in one pass over the incidence lists; <p, Ap> per workgroup.  gate: the PCG's state word (done: nothing to do)
__global__ __launch_bounds__(kT) void vgc_camx_kernel(PairLists L, VgcPairs P, const double *__restrict__ rec, const double *__restrict__ diag, double mu,
                                                      const double *__restrict__ p, const BaState *__restrict__ gate, double *__restrict__ Ap,
                                                      double *__restrict__ ppap) {
    __shared__ double part[4][1];
    __shared__ double sh[4];
    if (gate != nullptr && gate->done) return;
    const size_t M = (size_t)P.M;
    const PairWalk w = pair_walk(L);
    double acc[1] = {0.0};
    for (int64_t e = w.e; e < w.e_end; e += w.step) {
        const int m = L.pair[e];
        const bool second = L.side[e] == 1;
        const int32_t u0 = P.ua[m], u1 = P.ub[m];
        const double xa = u0 >= 0 ? p[u0] : 0.0, xb = u1 >= 0 ? p[u1] : 0.0;
        const double j00 = rec[2 * M + m], j01 = rec[3 * M + m], j10 = rec[4 * M + m], j11 = rec[5 * M + m];
        const double t0 = j00 * xa + j01 * xb, t1 = j10 * xa + j11 * xb;
        acc[0] += (second ? j01 : j00) * t0 + (second ? j11 : j10) * t1;
    }
    if (w.heavy) pair_heavy_sum<1>(acc, part);
    double pap = 0.0;
    if (w.u >= 0 && (!w.heavy || threadIdx.x == 0)) {
        const double v = acc[0] + (mu * clamp_diag(diag[w.u])) * p[w.u];
        Ap[w.u] = v;
        pap = p[w.u] * v;
    }
    pap = block_sum256(pap, sh);
    if (threadIdx.x == 0) ppap[blockIdx.x] = pap;
}

// candidate focals of the free cameras: f + x projected onto f >= lower_bound; |step|^2 and |f|^2 per workgroup
__global__ __launch_bounds__(kT) void vgc_step_kernel(int nfree, const int32_t *__restrict__ cam_of, const double *__restrict__ f, const double *__restrict__ x,
                                                      double lower, double *__restrict__ fnew, double *__restrict__ parts) {
    __shared__ double sh[4];
    double s2 = 0.0, x2 = 0.0;
    for (int64_t u = (int64_t)blockIdx.x * kT + threadIdx.x; u < nfree; u += (int64_t)gridDim.x * kT) {
        const int32_t c = cam_of[u];
        const double fo = f[c], fn = fmax(lower, fo + x[u]), st = fn - fo;
        fnew[c] = fn;
        s2 += st * st; x2 += fo * fo;
    }
    s2 = block_sum256(s2, sh);
    x2 = block_sum256(x2, sh);
    if (threadIdx.x == 0) { parts[blockIdx.x] = s2; parts[gridDim.x + blockIdx.x] = x2; }
}

// rule 6: per camera the ratio test, per participating pair the two-view error at the optimised focals (those of rejected cameras included)
__global__ __launch_bounds__(kT) void vgc_finish_kernel(int ncams, const int32_t *__restrict__ uslot, const uint8_t *__restrict__ touched,
                                                        const double *__restrict__ focal0, const double *__restrict__ f, double lo, double hi,
                                                        double *__restrict__ focal_out, double *__restrict__ focal_est, int32_t *__restrict__ cam_status,
                                                        int M_, const double *__restrict__ rraw, double thr2, int32_t *__restrict__ pair_bad) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t < ncams) {
        int32_t st = XM_VGC_CAM_UNUSED;
        double est = focal0[t], outv = focal0[t];
        if (uslot[t] >= 0) {
            est = f[t];
            const double ratio = est / focal0[t];
            const bool rejected = ratio > hi || ratio < lo;
            st = rejected ? XM_VGC_CAM_REJECTED : XM_VGC_CAM_REFINED;
            outv = rejected ? focal0[t] : est;
        } else if (touched[t]) {
            st = XM_VGC_CAM_CONSTANT;
        }
        focal_out[t] = outv; focal_est[t] = est; cam_status[t] = st;
    }
    if (t < M_) {
        const double r0 = rraw[t], r1 = rraw[(size_t)M_ + t];
        pair_bad[t] = (r0 * r0 + r1 * r1 > thr2) ? 1 : 0;
    }
}

// What the host prepares from the caller's arrays: the effective models (rule 7), the participating pairs, the unknowns, the lists
struct VgcPlan {
    int ncams = 0, npairs = 0, M = 0, nfree = 0;
    int64_t same = 0, constant = 0;
    std::vector<int32_t> model, flip, flip_ca, flip_cb, plist, ca, cb, ua, ub, uslot, cam_of;
    std::vector<uint8_t> touched;
    PairListsHost lists;

    VgcPlan(const VgcInput &in, bool update_config) {
        ncams = (int)in.ncams; npairs = (int)in.npairs;
        model.assign(in.model, in.model + npairs);
        auto valid = [&](int k) { return !in.valid_in || in.valid_in[k] != 0; };
        auto cam1 = [&](int k) { return in.cam_of_image[in.pi[k]]; };
        auto cam2 = [&](int k) { return in.cam_of_image[in.pj[k]]; };
        if (update_config) {   // view_graph_manipulation.cc:170-231
            std::vector<int64_t> total((size_t)ncams, 0), calibrated((size_t)ncams, 0);
            for (int k = 0; k < npairs; ++k) {
                if (!valid(k)) continue;
                const int32_t c1 = cam1(k), c2 = cam2(k);
                if (!in.has_prior[c1] || !in.has_prior[c2]) continue;
                if (model[(size_t)k] == XM_VG_MODEL_E) { total[(size_t)c1]++; total[(size_t)c2]++; calibrated[(size_t)c1]++; calibrated[(size_t)c2]++; }
                else if (model[(size_t)k] == XM_VG_MODEL_F) { total[(size_t)c1]++; total[(size_t)c2]++; }
            }
            auto cam_valid = [&](int32_t c) { return total[(size_t)c] > 0 && (double)calibrated[(size_t)c] * 1.0 / (double)total[(size_t)c] > 0.5; };
            for (int k = 0; k < npairs; ++k) {
                if (!valid(k) || model[(size_t)k] != XM_VG_MODEL_F) continue;
                const int32_t c1 = cam1(k), c2 = cam2(k);
                if (cam_valid(c1) && cam_valid(c2)) { flip.push_back(k); flip_ca.push_back(c1); flip_cb.push_back(c2); }
            }
            for (int32_t k : flip) model[(size_t)k] = XM_VG_MODEL_E;
        }
        touched.assign((size_t)ncams, 0);
        for (int k = 0; k < npairs; ++k) {
            if (!valid(k) || (model[(size_t)k] != XM_VG_MODEL_E && model[(size_t)k] != XM_VG_MODEL_F)) continue;
            plist.push_back(k); ca.push_back(cam1(k)); cb.push_back(cam2(k));
            touched[(size_t)ca.back()] = 1; touched[(size_t)cb.back()] = 1;
            if (ca.back() == cb.back()) same++;
        }
        M = (int)plist.size();
        uslot.assign((size_t)ncams, -1);
        for (int c = 0; c < ncams; ++c) {
            if (!touched[(size_t)c]) continue;
            if (in.has_prior[c]) { constant++; continue; }
            uslot[(size_t)c] = (int32_t)cam_of.size(); cam_of.push_back(c);
        }
        nfree = (int)cam_of.size();
        ua.resize((size_t)M); ub.resize((size_t)M);
        for (int m = 0; m < M; ++m) { ua[(size_t)m] = uslot[(size_t)ca[(size_t)m]]; ub[(size_t)m] = uslot[(size_t)cb[(size_t)m]]; }
        lists = build_pair_lists(nfree, ua, ub, kVgcLightIncidences, true);
    }
};

// One call's device state and the launches on it: the LM loop and the probe both go through these members
struct VgcWork {
    const VgcPlan &pl;
    const VgcSettings &cfg;
    hipStream_t st;
    DevBuf<double> F, pp, focal0, d, f[2], rraw, rec, grad, diag, b, sinv, x, r, z, pv, Ap, parts, fout, fest;
    DevBuf<int32_t> plist, ca, cb, ua, ub, uslot, cam_of, flip, flip_ca, flip_cb, cstat, pbad, state_buf;
    DevBuf<uint8_t> touched;
    PairListsDev lists;
    DevBuf<double> Rrel, trel;   // rule 7 only
    const double *rrel_p = nullptr, *trel_p = nullptr;
    BaState *dst = nullptr;
    Pinned<BaState> hs;
    int ge = 1, gfc = 1, cur = 0;
    size_t o_eval = 0, o_gmax = 0, o_pcg = 0, o_step = 0, o_cand = 0;
    VgcPairs P{};
    BaPcg a{};
    const dim3 blk{kT};

    VgcWork(const VgcPlan &pl_, const VgcSettings &cfg_, const VgcInput &in, const double *f_start, hipStream_t st_) : pl(pl_), cfg(cfg_), st(st_) {
        const size_t M = (size_t)pl.M, nf = (size_t)pl.nfree, nc = (size_t)pl.ncams;
        upload(F, in.F, (size_t)9 * pl.npairs, st);
        upload(pp, in.pp, 2 * nc, st);
        upload(focal0, in.focal0, nc, st);
        upload(f[0], f_start, nc, st);
        upload(f[1], f_start, nc, st);
        upload(plist, pl.plist.data(), M, st); upload(ca, pl.ca.data(), M, st); upload(cb, pl.cb.data(), M, st);
        upload(ua, pl.ua.data(), M, st); upload(ub, pl.ub.data(), M, st);
        upload(uslot, pl.uslot.data(), nc, st); upload(touched, pl.touched.data(), nc, st);
        upload(cam_of, pl.cam_of.data(), nf, st);
        lists.upload_from(pl.lists, pl.nfree, st);
        upload(flip, pl.flip.data(), pl.flip.size(), st); upload(flip_ca, pl.flip_ca.data(), pl.flip.size(), st);
        upload(flip_cb, pl.flip_cb.data(), pl.flip.size(), st);
        d.alloc(8 * M, false); rraw.alloc(2 * M, false); rec.alloc(6 * M, false);
        for (DevBuf<double> *v : {&grad, &diag, &b, &sinv, &x, &r, &z, &pv, &Ap}) fresh(*v, nf, 0, st);
        fout.alloc(nc, false); fest.alloc(nc, false); cstat.alloc(nc, false); pbad.alloc(M, false);
        fresh(state_buf, sizeof(BaState) / sizeof(int32_t) + 2, 0, st);
        dst = reinterpret_cast<BaState *>(state_buf.p);
        ge = (int)std::max<size_t>(1, (M + kT - 1) / kT);
        gfc = flat_grid_of((int64_t)nf);
        const int gcam = lists.grid;
        // partials: eval (ge) | gmax (gcam) | PCG (4 gfc + gcam) | step (2 gfc) | candidate (2 ge)
        o_eval = 0; o_gmax = (size_t)ge; o_pcg = o_gmax + gcam; o_step = o_pcg + 4 * (size_t)gfc + gcam; o_cand = o_step + 2 * (size_t)gfc;
        fresh(parts, o_cand + 2 * (size_t)ge, 0, st);
        P.M = pl.M; P.ca = ca.p; P.cb = cb.p; P.ua = ua.p; P.ub = ub.p; P.d = d.p;
        a.n = pl.nfree; a.grid = gfc; a.cgrid = gcam; a.tol2 = 1e-24;   // relative residual 1e-12
        a.b = b.p; a.sinv = sinv.p; a.ustar = nullptr; a.x = x.p; a.r = r.p; a.z = z.p; a.p = pv.p; a.Ap = Ap.p;
        a.lay_partials(parts.p + o_pcg);
        a.st = dst;
    }
    void config() {
        if (pl.flip.empty()) return;
        hipLaunchKernelGGL(vgc_config_kernel, dim3((unsigned)((pl.flip.size() + kT - 1) / kT)), blk, 0, st, (int)pl.flip.size(), (const int32_t *)flip.p,
                           (const int32_t *)flip_ca.p, (const int32_t *)flip_cb.p, (const double *)focal0.p, (const double *)pp.p, rrel_p, trel_p, F.p);
        check_launch("vgc_config_kernel");
    }
    void upload_motion(const VgcInput &in) {
        if (pl.flip.empty()) return;
        upload(Rrel, in.Rrel, (size_t)9 * pl.npairs, st); upload(trel, in.trel, (size_t)3 * pl.npairs, st);
        rrel_p = Rrel.p; trel_p = trel.p;
    }
    void setup() {
        if (pl.M == 0) return;
        hipLaunchKernelGGL(vgc_setup_kernel, dim3(ge), blk, 0, st, pl.M, (const int32_t *)plist.p, (const int32_t *)ca.p, (const int32_t *)cb.p,
                           (const double *)pp.p, (const double *)F.p, d.p);
        check_launch("vgc_setup_kernel");
    }
    void reduce(const BaReduce &rd) { hipLaunchKernelGGL(ba_reduce_kernel, dim3(1), dim3(256), 0, st, rd); }
    BaState read_state(const char *what) { return xm::read_state(dst, hs, st, cfg.watchdog_s, kStage, what); }
    // records, gradient and diagonal at the current focals for the damping mu; cost and |J^T r|_inf to the state word
    void linearise(double mu) {
        hipLaunchKernelGGL(vgc_eval_kernel, dim3(ge), blk, 0, st, P, (const double *)f[cur].p, cfg.loss_scale, rraw.p, rec.p, parts.p + o_eval);
        hipLaunchKernelGGL(vgc_cam_kernel, dim3(lists.grid), blk, 0, st, lists.L, pl.M, (const double *)rec.p, mu, grad.p, diag.p, b.p, sinv.p,
                           parts.p + o_gmax);
        BaReduce rd{};
        rd.sum_p[0] = parts.p + o_eval; rd.sum_n[0] = ge; rd.sum_out[0] = &dst->cost;
        rd.max_p = parts.p + o_gmax; rd.max_n = lists.grid; rd.max_out = &dst->gmax;
        reduce(rd);
    }
    void product(const double *p, const BaState *gate, double mu) {
        hipLaunchKernelGGL(vgc_camx_kernel, dim3(lists.grid), blk, 0, st, lists.L, P, (const double *)rec.p, (const double *)diag.p, mu, p, gate, Ap.p,
                           a.ppap);
    }
    void candidate() {
        const int nx = cur ^ 1;
        hipLaunchKernelGGL(vgc_step_kernel, dim3(gfc), blk, 0, st, pl.nfree, (const int32_t *)cam_of.p, (const double *)f[cur].p, (const double *)x.p,
                           cfg.lower_bound, f[nx].p, parts.p + o_step);
        hipLaunchKernelGGL(vgc_cand_kernel, dim3(ge), blk, 0, st, P, (const double *)f[nx].p, (const double *)x.p, cfg.loss_scale, (const double *)rec.p,
                           parts.p + o_cand);
        BaReduce rd{};
        rd.sum_p[0] = parts.p + o_cand; rd.sum_n[0] = ge; rd.sum_out[0] = &dst->cost_new;
        rd.sum_p[1] = parts.p + o_cand + ge; rd.sum_n[1] = ge; rd.sum_out[1] = &dst->model;
        rd.sum_p[2] = parts.p + o_step; rd.sum_n[2] = gfc; rd.sum_out[2] = &dst->step2[0];
        rd.sum_p[3] = parts.p + o_step + gfc; rd.sum_n[3] = gfc; rd.sum_out[3] = &dst->x2[0];
        reduce(rd);
    }
};

void run(const VgcInput &in, const VgcSettings &cfg, const VgcOutput &out, VgcOutcome &res, hipStream_t st) {
    const auto t_start = std::chrono::steady_clock::now();
    const VgcPlan pl(in, cfg.update_config);
    const int ncams = pl.ncams, npairs = pl.npairs, M = pl.M;
    res.pairs = M; res.pairs_same = pl.same; res.cams_free = pl.nfree; res.cams_constant = pl.constant; res.pairs_flipped = (int64_t)pl.flip.size();
    res.cams_heavy = pl.lists.nheavy; res.max_incidences = pl.lists.max_inc;
    // what holds whether or not anything is optimised
    auto write_inputs_through = [&](const double *F_now) {
        for (int c = 0; c < ncams; ++c) {
            out.focal_out[c] = in.focal0[c]; out.focal_est[c] = in.focal0[c]; out.refined[c] = 0;
            out.cam_status[c] = pl.touched[(size_t)c] ? XM_VGC_CAM_CONSTANT : XM_VGC_CAM_UNUSED;
        }
        for (int k = 0; k < npairs; ++k) {
            const bool valid = !in.valid_in || in.valid_in[k] != 0;
            out.pair_status[k] = valid ? XM_VGC_VALID : XM_VGC_INVALID_IN;
            out.residual[2 * (size_t)k] = 0.0; out.residual[2 * (size_t)k + 1] = 0.0;
            if (out.model_out) out.model_out[k] = pl.model[(size_t)k];
        }
        if (out.F_out && F_now != out.F_out) std::memcpy(out.F_out, F_now, (size_t)9 * npairs * sizeof(double));
        if (out.d_out) std::memset(out.d_out, 0, (size_t)8 * npairs * sizeof(double));
    };
    if (pl.nfree == 0 && pl.flip.empty()) {   // rule 5, and nothing for the device to do
        write_inputs_through(in.F);
        res.stop = XM_BA_NO_CONVERGENCE;
        res.seconds_index = secs_since(t_start);
        return;
    }
    VgcWork W(pl, cfg, in, in.focal0, st);
    W.upload_motion(in);
    wait_stream(st, cfg.watchdog_s, kStage, "the upload");
    res.seconds_index = secs_since(t_start);
    const auto t_kernels = std::chrono::steady_clock::now();
    W.config();
    std::vector<double> hF;
    if (pl.nfree == 0) {   // rule 5 behind rule 7: the pairs are rewritten, nothing is refined, no pair is invalidated
        download(hF, (const double *)W.F.p, (size_t)9 * npairs, st);
        wait_stream(st, cfg.watchdog_s, kStage, "the rewritten pairs");
        res.seconds_kernels = secs_since(t_kernels);
        write_inputs_through(hF.data());
        res.stop = XM_BA_NO_CONVERGENCE;
        return;
    }
    W.setup();

    int pcg_last = 8;
    double mu = 0.0;   // the damping of the current linearisation: the PCG's product reads it
    PcgHooks hooks;
    hooks.product = [&] { W.product(W.a.p, W.dst, mu); };
    hooks.read = [&] { return W.read_state("the PCG"); };

    // the LM loop (xm_lm_loop.h) over this solver's launches and reads; no time limit
    const LmRules rules{cfg.max_iters, cfg.function_tol, cfg.gradient_tol, cfg.parameter_tol};
    LmHooks lm;
    lm.linearise = [&](double m, bool) { mu = m; W.linearise(mu); };
    lm.read_point = [&](LmRead which) {   // the last accepted point is read for its residuals and cost
        const BaState s = W.read_state(which == kLmReadFinal ? "the final cost" : "the cost and gradient");
        if (which == kLmReadFirst && !std::isfinite(s.cost)) throw Error(XM_ERR_ARG, "xm_view_graph_calibrate: the initial cost is not finite");
        return LmPoint{s.cost, s.gmax, 0.0};
    };
    lm.solve = [&] { return LmSolve{pcg_solve_batched<1>(W.a, W.gfc, st, pcg_last, hooks).iters, 0.0}; };
    lm.read_candidate = [&](double) {
        W.candidate();
        const BaState s = W.read_state("the candidate's cost");
        return LmCandidate{s.cost_new, s.model, s.step2[0], s.x2[0]};
    };
    lm.accept = [&](bool) { W.cur ^= 1; };
    const LmResult lr = lm_loop(rules, lm);
    const int trace_n = (int)std::min<size_t>(lr.point_costs.size(), (size_t)std::max(cfg.max_iters + 1, 0));   // the cost at every point read
    if (out.cost_trace) std::copy_n(lr.point_costs.begin(), trace_n, out.cost_trace);
    res.initial_cost = lr.initial_cost;
    hipLaunchKernelGGL(vgc_finish_kernel, dim3((unsigned)((std::max(ncams, M) + kT - 1) / kT)), dim3(kT), 0, st, ncams, (const int32_t *)W.uslot.p,
                       (const uint8_t *)W.touched.p, (const double *)W.focal0.p, (const double *)W.f[W.cur].p, cfg.lower_ratio, cfg.higher_ratio, W.fout.p,
                       W.fest.p, W.cstat.p, M, (const double *)W.rraw.p, cfg.two_view_error * cfg.two_view_error, W.pbad.p);
    check_launch("vgc_finish_kernel");
    wait_stream(st, cfg.watchdog_s, kStage, "the results");
    res.seconds_kernels = secs_since(t_kernels);
    const auto t_down = std::chrono::steady_clock::now();
    std::vector<double> hfout, hfest, hr, hd;
    std::vector<int32_t> hcs, hbad;
    download(hfout, (const double *)W.fout.p, (size_t)ncams, st); download(hfest, (const double *)W.fest.p, (size_t)ncams, st);
    download(hcs, (const int32_t *)W.cstat.p, (size_t)ncams, st); download(hbad, (const int32_t *)W.pbad.p, (size_t)M, st);
    download(hr, (const double *)W.rraw.p, 2 * (size_t)M, st);
    if (out.d_out) download(hd, (const double *)W.d.p, 8 * (size_t)M, st);
    if (out.F_out) download(hF, (const double *)W.F.p, (size_t)9 * npairs, st);
    wait_stream(st, cfg.watchdog_s, kStage, "the download");
    write_inputs_through(out.F_out ? hF.data() : in.F);
    for (int c = 0; c < ncams; ++c) {
        out.focal_out[c] = hfout[(size_t)c]; out.focal_est[c] = hfest[(size_t)c]; out.cam_status[c] = hcs[(size_t)c];
        out.refined[c] = hcs[(size_t)c] == XM_VGC_CAM_REFINED ? 1 : 0;
        if (hcs[(size_t)c] == XM_VGC_CAM_REJECTED) res.cams_rejected++;
    }
    planes_to_pairs(pl.plist, npairs, hr, 2, out.residual);
    if (out.d_out) planes_to_pairs(pl.plist, npairs, hd, 8, out.d_out);
    for (int m = 0; m < M; ++m)
        if (hbad[(size_t)m]) { out.pair_status[pl.plist[(size_t)m]] = XM_VGC_TWO_VIEW_ERROR; res.pairs_invalidated++; }
    res.stop = lr.status; res.iters = lr.iters; res.accepted = lr.accepted; res.pcg_iters = lr.pcg_total; res.final_cost = lr.final_cost; res.trace_len = trace_n;
    res.seconds_download = secs_since(t_down);
}

void probe(const VgcInput &in, const VgcSettings &cfg, const VgcProbe &q, hipStream_t st) {
    const VgcPlan pl(in, false);
    const int ncams = pl.ncams, npairs = pl.npairs, M = pl.M;
    auto zero = [](double *p, size_t n) { if (p) std::memset(p, 0, n * sizeof(double)); };
    zero(q.d, 8 * (size_t)npairs); zero(q.residual, 2 * (size_t)npairs); zero(q.record, 6 * (size_t)npairs); zero(q.cost, 1);
    zero(q.gradient, (size_t)ncams); zero(q.diagonal, (size_t)ncams); zero(q.product, (size_t)ncams);
    if (M == 0) return;
    VgcWork W(pl, cfg, in, q.focal, st);
    if (q.d_in) {
        std::vector<double> hd(8 * (size_t)M);
        for (int m = 0; m < M; ++m)
            for (int c = 0; c < 8; ++c) hd[(size_t)c * M + m] = q.d_in[8 * (size_t)pl.plist[(size_t)m] + c];
        XM_HIP_CHECK(hipMemcpyAsync(W.d.p, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the given d");
    } else {
        W.setup();
    }
    W.linearise(q.mu);
    std::vector<double> hx((size_t)std::max(pl.nfree, 1), 0.0);
    if (q.x)
        for (int u = 0; u < pl.nfree; ++u) hx[(size_t)u] = q.x[pl.cam_of[(size_t)u]];
    XM_HIP_CHECK(hipMemcpyAsync(W.pv.p, hx.data(), (size_t)pl.nfree * sizeof(double), hipMemcpyHostToDevice, st));
    W.product(W.pv.p, nullptr, q.mu);
    const BaState s = W.read_state("the probe");
    std::vector<double> hd, hr, hrec, hg, hdg, hap;
    download(hd, (const double *)W.d.p, 8 * (size_t)M, st); download(hr, (const double *)W.rraw.p, 2 * (size_t)M, st);
    download(hrec, (const double *)W.rec.p, 6 * (size_t)M, st); download(hg, (const double *)W.grad.p, (size_t)pl.nfree, st);
    download(hdg, (const double *)W.diag.p, (size_t)pl.nfree, st); download(hap, (const double *)W.Ap.p, (size_t)pl.nfree, st);
    wait_stream(st, cfg.watchdog_s, kStage, "the probe's download");
    if (q.d) planes_to_pairs(pl.plist, npairs, hd, 8, q.d);
    if (q.residual) planes_to_pairs(pl.plist, npairs, hr, 2, q.residual);
    if (q.record) planes_to_pairs(pl.plist, npairs, hrec, 6, q.record);
    if (q.cost) *q.cost = s.cost;
    for (int u = 0; u < pl.nfree; ++u) {
        const int32_t c = pl.cam_of[(size_t)u];
        if (q.gradient) q.gradient[c] = hg[(size_t)u];
        if (q.diagonal) q.diagonal[c] = hdg[(size_t)u];
        if (q.product) q.product[c] = hap[(size_t)u];
    }
}

}  // namespace

void view_graph_calibrate_host(const VgcInput &in, const VgcSettings &cfg, const VgcOutput &out, VgcOutcome &res) {
    res = VgcOutcome();
    hipStream_t st = nullptr;   // the default stream, as xm_view_graph_filter
    try {
        run(in, cfg, out, res, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the device buffers are freed next: nothing may still be reading them
        throw;
    }
}

void view_graph_calibrate_probe_host(const VgcInput &in, const VgcSettings &cfg, const VgcProbe &q) {
    hipStream_t st = nullptr;
    try {
        probe(in, cfg, q, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);
        throw;
    }
}

}  // namespace xm
