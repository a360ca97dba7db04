// xm_rotavg.hip — robust rotation averaging over the view graph on the device (xm_rotavg.h has the list of launches, include/xm_amd.h the rules).
#include "xm_rotavg.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "xm_lm_shared.h"
#include "xm_pair_lists.h"
#include "xm_stage.h"

// every product and every sum of the contract is rounded on its own
#pragma clang fp contract(off)

namespace xm {

namespace {

constexpr const char *kStage = "xm_view_graph_rotations";
constexpr int kT = kRavThreads;
static_assert(kRavMaxPcgIters == kBaMaxPcgIters, "the limit reported is the one the PCG runs to");

// ---- rule 3: AngleAxisToRotation (rigid3d.cc:53-71), row-major; Eigen's AngleAxis::toRotationMatrix above the norm 1e-12
__host__ __device__ __forceinline__ void rav_exp(double a0, double a1, double a2, double (&R)[9]) {
    const double n = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
    if (n > 1e-12) {
        const double ux = a0 / n, uy = a1 / n, uz = a2 / n;
        const double s = sin(n), c = cos(n);
        const double sx = s * ux, sy = s * uy, sz = s * uz;
        const double k = 1.0 - c;
        const double cx = k * ux, cy = k * uy, cz = k * uz;
        double t = cx * uy;
        R[1] = t - sz; R[3] = t + sz;
        t = cx * uz;
        R[2] = t + sy; R[6] = t - sy;
        t = cy * uz;
        R[5] = t - sx; R[7] = t + sx;
        R[0] = cx * ux + c; R[4] = cy * uy + c; R[8] = cz * uz + c;
    } else {   // the first-order matrix of :59-69, not orthogonal
        R[0] = 1.0; R[3] = a2; R[6] = -a1;
        R[1] = -a2; R[4] = 1.0; R[7] = a0;
        R[2] = a1; R[5] = -a0; R[8] = 1.0;
    }
}
// ---- rule 4: RotationToAngleAxis, Eigen's matrix -> quaternion -> angle-axis
__host__ __device__ __forceinline__ void rav_log(const double (&R)[9], double &a0, double &a1, double &a2) {
    double x, y, z, w;
    double t = (R[0] + R[4]) + R[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        w = 0.5 * t;
        t = 0.5 / t;
        x = (R[7] - R[5]) * t; y = (R[2] - R[6]) * t; z = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i == 1 ? R[4] : R[0])) i = 2;
        if (i == 0) {
            t = sqrt(((R[0] - R[4]) - R[8]) + 1.0);
            x = 0.5 * t;
            t = 0.5 / t;
            w = (R[7] - R[5]) * t; y = (R[3] + R[1]) * t; z = (R[6] + R[2]) * t;
        } else if (i == 1) {
            t = sqrt(((R[4] - R[8]) - R[0]) + 1.0);
            y = 0.5 * t;
            t = 0.5 / t;
            w = (R[2] - R[6]) * t; z = (R[7] + R[5]) * t; x = (R[1] + R[3]) * t;
        } else {
            t = sqrt(((R[8] - R[0]) - R[4]) + 1.0);
            z = 0.5 * t;
            t = 0.5 / t;
            w = (R[3] - R[1]) * t; x = (R[2] + R[6]) * t; y = (R[5] + R[7]) * t;
        }
    }
    double nrm = sqrt((x * x + y * y) + z * z);
    if (nrm == 0.0) { a0 = 0.0; a1 = 0.0; a2 = 0.0; return; }
    const double angle = 2.0 * atan2(nrm, fabs(w));
    if (w < 0.0) nrm = -nrm;
    a0 = angle * (x / nrm); a1 = angle * (y / nrm); a2 = angle * (z / nrm);
}
// C = A B and C = A^T B, row-major, every entry (p0 + p1) + p2
__host__ __device__ __forceinline__ void mul33(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__host__ __device__ __forceinline__ void mul33t(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
}
__device__ __forceinline__ void load9(const double *__restrict__ p, double (&R)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = p[k];
}

// the state from the caller's matrices: slot u holds image img[u]
__global__ __launch_bounds__(kT) void rav_log_kernel(int nr, const int32_t *__restrict__ img, const double *__restrict__ rot0, double *__restrict__ est) {
    const int u = blockIdx.x * kT + threadIdx.x;
    if (u >= nr) return;
    double R[9], a0, a1, a2;
    load9(rot0 + (size_t)9 * img[u], R);
    rav_log(R, a0, a1, a2);
    est[3 * (size_t)u] = a0; est[3 * (size_t)u + 1] = a1; est[3 * (size_t)u + 2] = a2;
}
__global__ __launch_bounds__(kT) void rav_exp_kernel(int nr, const double *__restrict__ est, double *__restrict__ Rm) {
    const int u = blockIdx.x * kT + threadIdx.x;
    if (u >= nr) return;
    double R[9];
    rav_exp(est[3 * (size_t)u], est[3 * (size_t)u + 1], est[3 * (size_t)u + 2], R);
#pragma unroll
    for (int k = 0; k < 9; ++k) Rm[9 * (size_t)u + k] = R[k];
}

struct RavPairs {   // the participating pairs on the device
    int M;
    const int32_t *ca, *cb;   // slot of image_id1 and of image_id2
    const double *Rrel;       // nine per participating pair
};

// rules 5 and 7: r_e = -Log(R_2^T Rrel_e R_1) in three planes, w_e, and per workgroup whether a weight is not finite
template <int WT>
__global__ __launch_bounds__(kT) void rav_pair_kernel(RavPairs P, const double *__restrict__ Rm, double sigma2, double *__restrict__ res,
                                                      double *__restrict__ w, double *__restrict__ badp) {
    __shared__ double shm[4];
    const int m = blockIdx.x * kT + threadIdx.x;
    const size_t M = (size_t)P.M;
    double bad = 0.0;
    if (m < P.M) {
        double R1[9], R2[9], Rr[9], T[9], Q[9];
        load9(Rm + (size_t)9 * P.ca[m], R1);
        load9(Rm + (size_t)9 * P.cb[m], R2);
        load9(P.Rrel + (size_t)9 * m, Rr);
        mul33(Rr, R1, T);
        mul33t(R2, T, Q);
        double a0, a1, a2;
        rav_log(Q, a0, a1, a2);
        const double r0 = -a0, r1 = -a1, r2 = -a2;
        const double e2 = (r0 * r0 + r1 * r1) + r2 * r2;
        double wt;
        if constexpr (WT == XM_VGR_GEMAN_MCCLURE) {
            const double tmp = e2 + sigma2;
            wt = sigma2 / (tmp * tmp);
        } else {
            static_assert(WT == XM_VGR_HALF_NORM, "unknown weight type");
            wt = pow(e2, -0.75);
        }
        res[m] = r0; res[M + m] = r1; res[2 * M + m] = r2;
        w[m] = wt;
        bad = (fabs(wt) <= 1.7976931348623157e308) ? 0.0 : 1.0;
    }
    bad = block_max<kT>(bad, shm);
    if (threadIdx.x == 0) badp[blockIdx.x] = bad;
}

// The lists of the registered images as the two kernels below take them: side 0 the camera is image_id1 (the row holds -I there), 1
// image_id2 (+I).  PairLists's fields with the slot of the fixed camera next to the two counts: there the kernel's first scalar load brings
// it in, and both kernels assemble to what they were before the lists were shared.  As an argument of its own the slot gets a load and a
// wait of its own where it is used, after the walk
struct RavLists {
    int nr, nheavy, fixed;
    const int32_t *order;
    const int64_t *ptr;
    const int32_t *pair;
    const uint8_t *side;
    RavLists(const PairLists &L, int fixed_) : nr(L.n), nheavy(L.nheavy), fixed(fixed_), order(L.order), ptr(L.ptr), pair(L.pair), side(L.side) {}
    __device__ __forceinline__ PairLists lists() const { return {nr, nheavy, order, ptr, pair, side}; }
};
// rule 8: b_i = sum of +w r over the pairs where i is image_id2 and of -w r where it is image_id1, d_i = sum of w; at the fixed camera the
// gauge residual Log(R_fixed0^T R_fixed) (rule 6) with weight 1.  sinv holds 1 / d_i three times.
__global__ __launch_bounds__(kT) void rav_cam_kernel(RavLists R, int M_, const double *__restrict__ res, const double *__restrict__ w,
                                                     const double *__restrict__ Rm, const double *__restrict__ Rf0, double *__restrict__ b,
                                                     double *__restrict__ diag, double *__restrict__ sinv, double *__restrict__ gauge) {
    __shared__ double part[4][4];
    const size_t M = (size_t)M_;
    const PairLists L = R.lists();
    const PairWalk k = pair_walk(L);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t e = k.e; e < k.e_end; e += k.step) {
        const int m = L.pair[e];
        const double wt = w[m], sw = L.side[e] == 1 ? wt : -wt;
        acc[0] += sw * res[m]; acc[1] += sw * res[M + m]; acc[2] += sw * res[2 * M + m];
        acc[3] += wt;
    }
    if (k.heavy) pair_heavy_sum<4>(acc, part);
    if (k.u >= 0 && (!k.heavy || threadIdx.x == 0)) {
        if (k.u == R.fixed) {
            double A[9], B[9], Q[9], g0, g1, g2;
            load9(Rf0, A);
            load9(Rm + (size_t)9 * k.u, B);
            mul33t(A, B, Q);
            rav_log(Q, g0, g1, g2);
            gauge[0] = g0; gauge[1] = g1; gauge[2] = g2;
            acc[0] += g0; acc[1] += g1; acc[2] += g2; acc[3] += 1.0;
        }
        const size_t o = 3 * (size_t)k.u;
        const double si = acc[3] > 0.0 ? 1.0 / acc[3] : 0.0;
        b[o] = acc[0]; b[o + 1] = acc[1]; b[o + 2] = acc[2];
        diag[k.u] = acc[3];
        sinv[o] = si; sinv[o + 1] = si; sinv[o + 2] = si;
    }
}

// Ap_i = sum over i's pairs of w (p_i - p_other), + p_i at the fixed camera; <p, Ap> per workgroup.  gate: the PCG's state word
__global__ __launch_bounds__(kT) void rav_camx_kernel(RavLists R, RavPairs P, const double *__restrict__ w, const double *__restrict__ p,
                                                      const BaState *__restrict__ gate, double *__restrict__ Ap, double *__restrict__ ppap) {
    __shared__ double part[4][3];
    __shared__ double sh[4];
    if (gate != nullptr && gate->done) return;
    const PairLists L = R.lists();
    const PairWalk k = pair_walk(L);
    double acc[3] = {0.0, 0.0, 0.0};
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (k.u >= 0) { p0 = p[3 * (size_t)k.u]; p1 = p[3 * (size_t)k.u + 1]; p2 = p[3 * (size_t)k.u + 2]; }
    for (int64_t e = k.e; e < k.e_end; e += k.step) {
        const int m = L.pair[e];
        const size_t o = 3 * (size_t)(L.side[e] == 1 ? P.ca[m] : P.cb[m]);
        const double wt = w[m];
        acc[0] += wt * (p0 - p[o]); acc[1] += wt * (p1 - p[o + 1]); acc[2] += wt * (p2 - p[o + 2]);
    }
    if (k.heavy) pair_heavy_sum<3>(acc, part);
    double pap = 0.0;
    if (k.u >= 0 && (!k.heavy || threadIdx.x == 0)) {
        if (k.u == R.fixed) { acc[0] += p0; acc[1] += p1; acc[2] += p2; }
        const size_t o = 3 * (size_t)k.u;
        Ap[o] = acc[0]; Ap[o + 1] = acc[1]; Ap[o + 2] = acc[2];
        pap = (p0 * acc[0] + p1 * acc[1]) + p2 * acc[2];
    }
    pap = block_sum256(pap, sh);
    if (threadIdx.x == 0) ppap[blockIdx.x] = pap;
}

// rules 9 and 10: est_i <- Log(Exp(est_i) Exp(-x_i)) (Exp(est_i) is what Rm holds), the new nine doubles, |x_i| per workgroup
__global__ __launch_bounds__(kT) void rav_update_kernel(int nr, const double *__restrict__ x, double *__restrict__ est, double *__restrict__ Rm,
                                                        double *__restrict__ parts) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int64_t u = (int64_t)blockIdx.x * kT + threadIdx.x; u < nr; u += (int64_t)gridDim.x * kT) {
        const double x0 = x[3 * u], x1 = x[3 * u + 1], x2 = x[3 * u + 2];
        double R[9], E[9], Q[9], a0, a1, a2;
        load9(Rm + 9 * u, R);
        rav_exp(-x0, -x1, -x2, E);
        mul33(R, E, Q);
        rav_log(Q, a0, a1, a2);
        est[3 * u] = a0; est[3 * u + 1] = a1; est[3 * u + 2] = a2;
        rav_exp(a0, a1, a2, R);
#pragma unroll
        for (int k = 0; k < 9; ++k) Rm[9 * u + k] = R[k];
        s += sqrt((x0 * x0 + x1 * x1) + x2 * x2);
    }
    s = block_sum256(s, sh);
    if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

// What the host prepares from the caller's arrays: the slots, the participating pairs, the lists
struct RavPlan {
    int n = 0, npairs = 0, nr = 0, M = 0, fixed_slot = -1;
    std::vector<int32_t> img, slot, plist, ca, cb;
    PairListsHost lists;
    std::vector<double> rrel;

    RavPlan(const RavInput &in, int64_t fixed_image) {
        n = (int)in.n; npairs = (int)in.npairs;
        slot.assign((size_t)n, -1);
        for (int i = 0; i < n; ++i)
            if (!in.registered || in.registered[i]) { slot[(size_t)i] = (int32_t)img.size(); img.push_back(i); }
        nr = (int)img.size();
        if (fixed_image >= 0) fixed_slot = slot[(size_t)fixed_image];
        for (int k = 0; k < npairs; ++k) {
            if (!rav_takes_part(in, k)) continue;
            plist.push_back(k); ca.push_back(slot[(size_t)in.pi[k]]); cb.push_back(slot[(size_t)in.pj[k]]);
        }
        M = (int)plist.size();
        rrel.resize((size_t)9 * M);
        for (int m = 0; m < M; ++m) std::memcpy(&rrel[(size_t)9 * m], in.Rrel + (size_t)9 * plist[(size_t)m], 9 * sizeof(double));
        lists = build_pair_lists(nr, ca, cb, kRavLightIncidences, false);
    }
};

// One call's device state and the launches on it: the IRLS loop and the probe both go through these members
struct RavWork {
    const RavPlan &pl;
    const RavSettings &cfg;
    hipStream_t st;
    DevBuf<double> rot0, Rrel, est, Rm, Rf0, res, w[2], b, diag, sinv, x, r, z, pv, Ap, parts, gauge;
    DevBuf<int32_t> img, ca, cb, state_buf;
    PairListsDev lists;
    BaState *dst = nullptr;
    Pinned<BaState> hs;
    int ge = 1, gfc = 1, gup = 1, gr = 1;
    size_t o_bad = 0, o_pcg = 0, o_step = 0;
    double sigma2 = 0.0;
    RavPairs P{};
    BaPcg a{};
    const dim3 blk{kT};

    RavWork(const RavPlan &pl_, const RavSettings &cfg_, const RavInput &in, hipStream_t st_) : pl(pl_), cfg(cfg_), st(st_) {
        const size_t M = (size_t)pl.M, nr = (size_t)pl.nr;
        upload(rot0, in.rot0, (size_t)9 * pl.n, st);
        upload(Rrel, pl.rrel.data(), 9 * M, st);
        upload(img, pl.img.data(), nr, st); upload(ca, pl.ca.data(), M, st); upload(cb, pl.cb.data(), M, st);
        lists.upload_from(pl.lists, pl.nr, st);
        est.alloc(3 * nr, false); Rm.alloc(9 * nr, false); Rf0.alloc(9, false); res.alloc(3 * M, false);
        fresh(w[0], M, 0, st); fresh(w[1], M, 0, st); fresh(gauge, 3, 0, st);
        diag.alloc(nr, false);
        for (DevBuf<double> *v : {&b, &sinv, &x, &r, &z, &pv, &Ap}) fresh(*v, 3 * nr, 0, st);
        fresh(state_buf, sizeof(BaState) / sizeof(int32_t) + 2, 0, st);
        dst = reinterpret_cast<BaState *>(state_buf.p);
        ge = (int)std::max<size_t>(1, (M + kT - 1) / kT);
        gr = (int)std::max<size_t>(1, (nr + kT - 1) / kT);
        gfc = flat_grid_of((int64_t)(3 * nr));
        gup = flat_grid_of((int64_t)nr);
        const int gcam = lists.grid;
        // partials: flag (ge) | PCG (4 gfc + gcam) | step (gup)
        o_bad = 0; o_pcg = (size_t)ge; o_step = o_pcg + 4 * (size_t)gfc + gcam;
        fresh(parts, o_step + (size_t)gup, 0, st);
        const double sigma = cfg.sigma_deg * 3.141592653589793238462643383279502884 / 180.0;   // DegToRad (rigid3d.cc:37)
        sigma2 = sigma * sigma;
        P.M = pl.M; P.ca = ca.p; P.cb = cb.p; P.Rrel = Rrel.p;
        a.n = 3 * (int64_t)pl.nr; a.grid = gfc; a.cgrid = gcam; a.tol2 = 1e-24;   // relative residual 1e-12
        a.b = b.p; a.sinv = sinv.p; a.ustar = nullptr; a.x = x.p; a.r = r.p; a.z = z.p; a.p = pv.p; a.Ap = Ap.p;
        a.lay_partials(parts.p + o_pcg);
        a.st = dst;
    }
    // the state from rot0, its matrices, and the fixed camera's start Exp(fixed0)
    void start() {
        hipLaunchKernelGGL(rav_log_kernel, dim3(gr), blk, 0, st, pl.nr, (const int32_t *)img.p, (const double *)rot0.p, est.p);
        exponentiate();
        XM_HIP_CHECK(hipMemcpyAsync(Rf0.p, Rm.p + (size_t)9 * pl.fixed_slot, 9 * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    void exponentiate() {
        hipLaunchKernelGGL(rav_exp_kernel, dim3(gr), blk, 0, st, pl.nr, (const double *)est.p, Rm.p);
        check_launch("rav_exp_kernel");
    }
    // residuals at the current matrices and the weights they give, into w[which]
    void evaluate(int which) {
        if (cfg.weight_type == XM_VGR_GEMAN_MCCLURE)
            hipLaunchKernelGGL((rav_pair_kernel<XM_VGR_GEMAN_MCCLURE>), dim3(ge), blk, 0, st, P, (const double *)Rm.p, sigma2, res.p, w[which].p,
                               parts.p + o_bad);
        else
            hipLaunchKernelGGL((rav_pair_kernel<XM_VGR_HALF_NORM>), dim3(ge), blk, 0, st, P, (const double *)Rm.p, sigma2, res.p, w[which].p,
                               parts.p + o_bad);
        check_launch("rav_pair_kernel");
    }
    void normal_equations(int which) {
        hipLaunchKernelGGL(rav_cam_kernel, dim3(lists.grid), blk, 0, st, RavLists{lists.L, pl.fixed_slot}, pl.M, (const double *)res.p,
                           (const double *)w[which].p, (const double *)Rm.p, (const double *)Rf0.p, b.p, diag.p, sinv.p, gauge.p);
        check_launch("rav_cam_kernel");
    }
    void product(int which, const double *p, const BaState *gate) {
        hipLaunchKernelGGL(rav_camx_kernel, dim3(lists.grid), blk, 0, st, RavLists{lists.L, pl.fixed_slot}, P, (const double *)w[which].p, p, gate,
                           Ap.p, a.ppap);
    }
    void update(const double *xv) {
        hipLaunchKernelGGL(rav_update_kernel, dim3(gup), blk, 0, st, pl.nr, xv, est.p, Rm.p, parts.p + o_step);
        check_launch("rav_update_kernel");
    }
    // the step sum and the flag of the last evaluation into the state word
    void reduce() {
        BaReduce rd{};
        rd.sum_p[0] = parts.p + o_step; rd.sum_n[0] = gup; rd.sum_out[0] = &dst->step2[0];
        rd.max_p = parts.p + o_bad; rd.max_n = ge; rd.max_out = &dst->gmax;
        hipLaunchKernelGGL(ba_reduce_kernel, dim3(1), dim3(256), 0, st, rd);
    }
    BaState read_state(const char *what) { return xm::read_state(dst, hs, st, cfg.watchdog_s, kStage, what); }
};

// per image from the slots; what is not registered is 0
void slots_to_images(const RavPlan &pl, const std::vector<double> &h, int per, double *outp) {
    std::memset(outp, 0, (size_t)per * pl.n * sizeof(double));
    for (int u = 0; u < pl.nr; ++u) std::memcpy(outp + (size_t)per * pl.img[(size_t)u], &h[(size_t)per * u], (size_t)per * sizeof(double));
}

void run(const RavInput &in, const RavSettings &cfg, const RavOutput &out, RavOutcome &res, hipStream_t st) {
    const auto t_start = std::chrono::steady_clock::now();
    const RavPlan pl(in, cfg.fixed_image);
    const int n = pl.n, npairs = pl.npairs, M = pl.M, nr = pl.nr;
    res.pairs = M; res.registered = nr; res.fixed_image = cfg.fixed_image; res.cams_heavy = pl.lists.nheavy; res.max_incidences = pl.lists.max_inc;
    if (n > 0) std::memcpy(out.rot_out, in.rot0, (size_t)9 * n * sizeof(double));
    for (int i = 0; i < cfg.max_iters; ++i) out.step_trace[i] = 0.0;
    if (npairs > 0) { std::memset(out.residual, 0, (size_t)3 * npairs * sizeof(double)); std::memset(out.weight, 0, (size_t)npairs * sizeof(double)); }
    if (M == 0) {   // nothing to average: the start is returned, its angle-axis form by the same rule 4 on the host
        for (int i = 0; i < n; ++i) {
            double R[9], a0 = 0.0, a1 = 0.0, a2 = 0.0;
            std::memcpy(R, in.rot0 + (size_t)9 * i, sizeof(R));
            if (pl.slot[(size_t)i] >= 0) rav_log(R, a0, a1, a2);
            out.angle_axis_out[3 * (size_t)i] = a0; out.angle_axis_out[3 * (size_t)i + 1] = a1; out.angle_axis_out[3 * (size_t)i + 2] = a2;
        }
        res.stop = XM_VGR_STOP_NOTHING;
        res.seconds_index = secs_since(t_start);
        return;
    }
    RavWork W(pl, cfg, in, st);
    wait_stream(st, cfg.watchdog_s, kStage, "the upload");
    res.seconds_index = secs_since(t_start);
    const auto t_kernels = std::chrono::steady_clock::now();

    int pcg_last = 8, which = 0;   // which: the weights of the current iteration, read by the PCG's product
    PcgHooks hooks;
    hooks.product = [&] { W.product(which, W.a.p, W.dst); };
    hooks.read = [&] { return W.read_state("the PCG"); };

    W.start();
    W.evaluate(0);
    W.reduce();
    BaState s = W.read_state("the first residuals");
    int status = XM_VGR_STOP_ITERATIONS, iters = 0, used = -1;
    for (;;) {
        if (iters >= cfg.max_iters) { status = XM_VGR_STOP_ITERATIONS; break; }
        if (s.gmax > 0.0) { status = XM_VGR_STOP_NONFINITE; break; }   // rule 7: a weight of this iteration is not finite
        which = iters & 1;
        W.normal_equations(which);
        const PcgResult pr = pcg_solve_batched<1>(W.a, W.gfc, st, pcg_last, hooks);
        res.pcg_iters += pr.iters;
        if (pr.capped) res.pcg_capped++;
        W.update(W.x.p);
        W.evaluate(which ^ 1);
        W.reduce();
        s = W.read_state("the step");
        used = which;
        const double avg = s.step2[0] / (double)nr;
        out.step_trace[iters] = avg;
        iters++;
        if (avg < cfg.step_tol) { status = XM_VGR_STOP_STEP; break; }
    }
    res.seconds_kernels = secs_since(t_kernels);
    const auto t_down = std::chrono::steady_clock::now();
    std::vector<double> hR, hest, hres, hw;
    download(hR, (const double *)W.Rm.p, (size_t)9 * nr, st); download(hest, (const double *)W.est.p, (size_t)3 * nr, st);
    download(hres, (const double *)W.res.p, (size_t)3 * M, st);
    if (used >= 0) download(hw, (const double *)W.w[used].p, (size_t)M, st);
    wait_stream(st, cfg.watchdog_s, kStage, "the download");
    for (int u = 0; u < nr; ++u) std::memcpy(out.rot_out + (size_t)9 * pl.img[(size_t)u], &hR[(size_t)9 * u], 9 * sizeof(double));
    slots_to_images(pl, hest, 3, out.angle_axis_out);
    planes_to_pairs(pl.plist, npairs, hres, 3, out.residual);
    if (used >= 0) planes_to_pairs(pl.plist, npairs, hw, 1, out.weight);
    res.stop = status; res.iters = iters;
    res.seconds_download = secs_since(t_down);
}

void probe(const RavInput &in, const RavSettings &cfg, const RavProbe &q, hipStream_t st) {
    const RavPlan pl(in, cfg.fixed_image);
    const int n = pl.n, npairs = pl.npairs, M = pl.M, nr = pl.nr;
    auto zero = [](double *p, size_t k) { if (p) std::memset(p, 0, k * sizeof(double)); };
    zero(q.rot, 9 * (size_t)n); zero(q.residual, 3 * (size_t)npairs); zero(q.gauge, 3); zero(q.weight, (size_t)npairs); zero(q.rhs, 3 * (size_t)n);
    zero(q.diagonal, (size_t)n); zero(q.product, 3 * (size_t)n); zero(q.angle_axis_out, 3 * (size_t)n); zero(q.step, 1);
    if (M == 0) return;
    RavWork W(pl, cfg, in, st);
    W.start();
    std::vector<double> hest(3 * (size_t)nr), hx(3 * (size_t)nr), hwin;
    for (int u = 0; u < nr; ++u)
        for (int c = 0; c < 3; ++c) {
            hest[3 * (size_t)u + c] = q.angle_axis[3 * (size_t)pl.img[(size_t)u] + c];
            hx[3 * (size_t)u + c] = q.x[3 * (size_t)pl.img[(size_t)u] + c];
        }
    XM_HIP_CHECK(hipMemcpyAsync(W.est.p, hest.data(), hest.size() * sizeof(double), hipMemcpyHostToDevice, st));
    XM_HIP_CHECK(hipMemcpyAsync(W.pv.p, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice, st));
    W.exponentiate();
    W.evaluate(0);
    std::vector<double> hR, hres, hw, hg, hb, hd, hap, hnew;
    download(hR, (const double *)W.Rm.p, (size_t)9 * nr, st);
    download(hres, (const double *)W.res.p, (size_t)3 * M, st);
    download(hw, (const double *)W.w[0].p, (size_t)M, st);
    if (q.weight_in) {
        hwin.resize((size_t)M);
        for (int m = 0; m < M; ++m) hwin[(size_t)m] = q.weight_in[pl.plist[(size_t)m]];
        XM_HIP_CHECK(hipMemcpyAsync(W.w[0].p, hwin.data(), hwin.size() * sizeof(double), hipMemcpyHostToDevice, st));
    }
    W.normal_equations(0);
    W.product(0, W.pv.p, nullptr);
    W.update(W.pv.p);
    W.reduce();
    const BaState s = W.read_state("the probe");
    download(hg, (const double *)W.gauge.p, 3, st); download(hb, (const double *)W.b.p, (size_t)3 * nr, st);
    download(hd, (const double *)W.diag.p, (size_t)nr, st); download(hap, (const double *)W.Ap.p, (size_t)3 * nr, st);
    download(hnew, (const double *)W.est.p, (size_t)3 * nr, st);
    wait_stream(st, cfg.watchdog_s, kStage, "the probe's download");
    if (q.rot) slots_to_images(pl, hR, 9, q.rot);
    if (q.residual) planes_to_pairs(pl.plist, npairs, hres, 3, q.residual);
    if (q.weight) planes_to_pairs(pl.plist, npairs, hw, 1, q.weight);
    if (q.gauge) std::memcpy(q.gauge, hg.data(), 3 * sizeof(double));
    if (q.rhs) slots_to_images(pl, hb, 3, q.rhs);
    if (q.diagonal) slots_to_images(pl, hd, 1, q.diagonal);
    if (q.product) slots_to_images(pl, hap, 3, q.product);
    if (q.angle_axis_out) slots_to_images(pl, hnew, 3, q.angle_axis_out);
    if (q.step) *q.step = s.step2[0] / (double)nr;
}

}  // namespace

void view_graph_rotations_host(const RavInput &in, const RavSettings &cfg, const RavOutput &out, RavOutcome &res) {
    res = RavOutcome();
    hipStream_t st = nullptr;   // the default stream, as xm_view_graph_filter
    try {
        run(in, cfg, out, res, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the device buffers are freed next: nothing may still be reading them
        throw;
    }
}

void view_graph_rotations_probe_host(const RavInput &in, const RavSettings &cfg, const RavProbe &q) {
    hipStream_t st = nullptr;
    try {
        probe(in, cfg, q, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);
        throw;
    }
}

}  // namespace xm
