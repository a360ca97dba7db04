// xm_lm_shared.h — what the solvers of sparse normal equations share (xm_ba.hip: the reprojection bundle adjustment; xm_gp.hip: the global
// positioning; xm_vgcalib.hip: the focal lengths over the view graph; xm_rotavg.hip: the rotations over it): the state word, the
// fixed-order reductions over a heavy landmark's workgroup, the walk over a landmark's list, Ceres's losses, the small symmetric solves,
// the vector kernels of the PCG with the host's batch driver for them, the kernel that brings partial sums into the state word and the
// host's read of it, the candidate's vector kernel and the dispatch on the loss.  The device code is the one xm_ba.hip and xm_gp.hip
// had: moving it here changes no bit of its outputs.  (The LM loop above all this: xm_lm_loop.h.)
// Everything stays in the anonymous namespace it had there: internal linkage, so each translation unit that includes this file compiles
// its own copy of the kernels and of the __shared__ arrays inside heavy_sum (include it in .hip files only, never in a header).
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>
#include <type_traits>

#include "xm_device.h"
#include "xm_schur.h"
#include "xm_stage.h"

namespace xm {

namespace {

constexpr int kBaHeavyThreads = 1024;   // a landmark with more than 64 observations: a workgroup of its own (as schur_lm_*)
constexpr int kBaMaxPcgIters = 500;     // Ceres's max_linear_solver_iterations

struct BaState {              // device-resident; the host reads it whole
    int32_t done, iters;      // PCG: 1 = reached the tolerance; iterations performed
    double relres;            // PCG: |r| / |b| when it stopped
    double cost, used, gmax;  // at the current point: F, used observations, |J^T r|_inf
    double cost_new, model;   // candidate: F, sum r.Jd + |Jd|^2 / 2
    double step2[2], x2[2];   // |d|^2, |x|^2: cameras, landmarks
    double res2[2];           // dense Schur: |b - S dc|^2, |b|^2
    int32_t fail, bad_focal;  // dense Schur: 1 = the factorisation or a substitution failed (cleared before each factorisation); bundle
                              // adjustment with focal scales: 1 = a candidate focal is not positive (cleared before each candidate)
};

__device__ __forceinline__ double clamp_diag(double d) { return fmin(fmax(d, 1e-6), 1e32); }

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
template <int T>
__device__ __forceinline__ double block_max(double v, double *sh) {   // result valid in thread 0
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = 0.0;
    if (threadIdx.x == 0)
        for (int q = 0; q < T / 64; ++q) m = fmax(m, sh[q]);
    return m;
}
// sum of K values over a heavy landmark's workgroup: DPP tree per wavefront, the 16 wavefront sums in a fixed order; valid in thread 0
template <int K>
__device__ __forceinline__ bool heavy_sum(double (&acc)[K]) {
    __shared__ double part[kBaHeavyThreads / 64][K];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) part[wv][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        for (int q = 0; q < kBaHeavyThreads / 64; ++q) t += part[q][k];
        acc[k] = t;
    }
    return true;
}
// the observations of landmark slot l in the by-landmark lists (heavy: workgroup-strided, light: the packed 64-wide group)
struct LmRange {
    int64_t l, e, e_end, step;
    bool heavy, active;
};
__device__ __forceinline__ LmRange lm_range(const SchurLists &S) {
    LmRange r;
    r.heavy = (int64_t)blockIdx.x < S.nheavy;
    r.active = true;
    if (r.heavy) {
        r.l = blockIdx.x; r.e = S.lm_ptr[r.l] + threadIdx.x; r.e_end = S.lm_ptr[r.l + 1]; r.step = kBaHeavyThreads;
    } else {
        const int64_t t = ((int64_t)blockIdx.x - S.nheavy) * kBaHeavyThreads + threadIdx.x;
        r.l = S.nheavy + t; r.step = 64;
        r.active = r.l < S.m;
        r.e = r.active ? S.gbase[t >> 6] + (t & 63) : 0;
        r.e_end = r.active ? r.e + (int64_t)64 * S.deg[r.l] : 0;
    }
    return r;
}

// ---- robust losses: Ceres's definitions (loss_function.cc) of rho(s) and rho'(s) at s = |r|^2 for the scale a, rho' clamped below at the
// smallest normal double as Ceres does.  rho'' <= 0 everywhere for these four, so Ceres's Corrector reduces to scaling r and J by
// sqrt(rho'(s)): the eval kernels store the scaled records and every later pass reads them as they are.  (In the bundle adjustment rho' >=
// DBL_MIN keeps sqrt(rho') >= 2^-511 and with it the first row of a used observation's J_P non-zero: its obs_used does not depend on the loss.)
template <int LOSS>
__device__ __forceinline__ double ba_rho(double s, double a, double &rho1) {
    constexpr double kMinNormal = 2.2250738585072014e-308;
    if constexpr (LOSS == XM_BA_LOSS_HUBER) {
        const double b = a * a;
        if (s > b) {
            const double r = sqrt(s);
            rho1 = fmax(kMinNormal, a / r);
            return 2.0 * a * r - b;
        }
        rho1 = 1.0;
        return s;
    } else if constexpr (LOSS == XM_BA_LOSS_SOFT_L1) {
        const double b = a * a, sum = 1.0 + s * (1.0 / b), tmp = sqrt(sum);
        rho1 = fmax(kMinNormal, 1.0 / tmp);
        return 2.0 * b * (tmp - 1.0);
    } else if constexpr (LOSS == XM_BA_LOSS_CAUCHY) {
        const double b = a * a, sum = 1.0 + s * (1.0 / b);
        rho1 = fmax(kMinNormal, 1.0 / sum);
        return b * log(sum);
    } else {
        static_assert(LOSS == XM_BA_LOSS_ARCTAN, "unknown loss");
        const double sum = 1.0 + s * s * (1.0 / (a * a));
        rho1 = fmax(kMinNormal, 1.0 / sum);
        return a * atan2(s, a);
    }
}
// the host's choice of a kernel's loss: f(std::integral_constant<int, LOSS>), the loss a compile-time constant
template <class F>
void with_loss(int loss, F &&f) {
    switch (loss) {
    case XM_BA_LOSS_HUBER: f(std::integral_constant<int, XM_BA_LOSS_HUBER>{}); break;
    case XM_BA_LOSS_SOFT_L1: f(std::integral_constant<int, XM_BA_LOSS_SOFT_L1>{}); break;
    case XM_BA_LOSS_CAUCHY: f(std::integral_constant<int, XM_BA_LOSS_CAUCHY>{}); break;
    case XM_BA_LOSS_ARCTAN: f(std::integral_constant<int, XM_BA_LOSS_ARCTAN>{}); break;
    default: f(std::integral_constant<int, XM_BA_LOSS_TRIVIAL>{});
    }
}

__device__ __forceinline__ void sym3(const double *vi, double (&V)[3][3]) {
    V[0][0] = vi[0]; V[0][1] = V[1][0] = vi[1]; V[0][2] = V[2][0] = vi[2];
    V[1][1] = vi[3]; V[1][2] = V[2][1] = vi[4]; V[2][2] = vi[5];
}
__device__ __forceinline__ constexpr int tri(int a, int b) { return a <= b ? b * (b + 1) / 2 + a : a * (a + 1) / 2 + b; }

// A (CD x CD, symmetric positive definite) -> its inverse by Cholesky; not positive definite: the inverse of the diagonal
template <int CD>
__device__ void chol_inverse(const double (&A)[CD][CD], double *out) {
    double L[CD][CD], Li[CD][CD];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < CD; ++j) {
        double s = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 0.0)) { ok = false; s = 1.0; }
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < CD; ++i) {
            double t = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < CD; ++i)
#pragma unroll
            for (int j = 0; j < CD; ++j) out[CD * i + j] = (i == j && A[i][i] > 0.0) ? 1.0 / A[i][i] : 0.0;
        return;
    }
#pragma unroll
    for (int j = 0; j < CD; ++j) {
        Li[j][j] = 1.0 / L[j][j];
#pragma unroll
        for (int i = j + 1; i < CD; ++i) {
            double t = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) t += L[i][k] * Li[k][j];
            Li[i][j] = -t / L[i][i];
        }
    }
#pragma unroll
    for (int i = 0; i < CD; ++i)
#pragma unroll
        for (int j = 0; j < CD; ++j) {
            double t = 0.0;
#pragma unroll
            for (int k = (i > j ? i : j); k < CD; ++k) t += Li[k][i] * Li[k][j];
            out[CD * i + j] = t;
        }
}

// ---- PCG on S dc = b (vectors: CD per camera).  Same scheme as SchurOp::pcg_solve: per-workgroup partials, every workgroup of the flat
// kernels sums them in the same fixed order, the direction kernel decides convergence and publishes it through the state word
struct BaPcg {
    int64_t n;
    int grid, cgrid;
    double tol2;
    const double *b, *sinv, *ustar;
    double *x, *r, *z, *p, *Ap;
    double *prz[2], *prr, *pbb, *ppap;
    BaState *st;
    // the five partial sums behind one another in q: four of `grid` workgroups, then <p, Ap> of cgrid
    void lay_partials(double *q) { prz[0] = q; prz[1] = q + grid; prr = q + 2 * grid; pbb = q + 3 * grid; ppap = q + 4 * grid; }
};
template <int CD>
__device__ __forceinline__ void block_matvec(const double *M, const double *v, double (&out)[CD]) {
#pragma unroll
    for (int j = 0; j < CD; ++j) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < CD; ++k) t += M[CD * j + k] * v[k];
        out[j] = t;
    }
}
template <int CD>
__global__ __launch_bounds__(256) void ba_pcg_init_kernel(BaPcg a) {
    __shared__ double sh[4];
    double rz = 0.0, bb = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        double v[CD], z[CD];
#pragma unroll
        for (int k = 0; k < CD; ++k) v[k] = a.b[CD * i + k];
        block_matvec<CD>(a.sinv + (size_t)CD * CD * i, v, z);
#pragma unroll
        for (int k = 0; k < CD; ++k) {
            a.x[CD * i + k] = 0.0; a.r[CD * i + k] = v[k]; a.z[CD * i + k] = z[k]; a.p[CD * i + k] = z[k];
            rz += v[k] * z[k]; bb += v[k] * v[k];
        }
    }
    rz = block_sum256(rz, sh);
    bb = block_sum256(bb, sh);
    if (threadIdx.x == 0) { a.prz[0][blockIdx.x] = rz; a.pbb[blockIdx.x] = bb; a.prr[blockIdx.x] = bb; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.st->done = 0; a.st->iters = 0; a.st->relres = 1.0; }
}
// iteration it >= 1: convergence test of the last update, else beta = <r,z>_new / <r,z>_old and p = z + beta p
template <int CD>
__global__ __launch_bounds__(256) void ba_pcg_dir_kernel(BaPcg a, int it) {
    __shared__ double sh[4];
    __shared__ int was_done;
    if (threadIdx.x == 0) was_done = a.st->done;
    __syncthreads();
    if (was_done) return;
    const double rzn = sum_partials256(a.prz[it & 1], a.grid, sh), rzo = sum_partials256(a.prz[(it & 1) ^ 1], a.grid, sh);
    const double rr = sum_partials256(a.prr, a.grid, sh), bb = sum_partials256(a.pbb, a.grid, sh);
    const double q = bb > 0.0 ? rr / bb : 0.0;
    if (q <= a.tol2) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { a.st->done = 1; a.st->iters = it; a.st->relres = sqrt(q); }
        return;
    }
    const double beta = rzo > 0.0 ? rzn / rzo : 0.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < a.n * CD; j += (int64_t)gridDim.x * 256) a.p[j] = a.z[j] + beta * a.p[j];
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.st->iters = it; a.st->relres = sqrt(q); }
}
// alpha = <r,z> / <p,Ap>; x += alpha p, r -= alpha Ap, z = S_ii^-1 r; partials of the new <r,z> (other parity) and |r|^2
template <int CD>
__global__ __launch_bounds__(256) void ba_pcg_upd_kernel(BaPcg a, int it) {
    __shared__ double sh[4];
    if (a.st->done) return;
    const double rz = sum_partials256(a.prz[it & 1], a.grid, sh), pap = sum_partials256(a.ppap, a.cgrid, sh);
    const double alpha = (pap > 0.0 && rz > 0.0) ? rz / pap : 0.0;
    double rzn = 0.0, rr = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        double rn[CD], z[CD];
#pragma unroll
        for (int k = 0; k < CD; ++k) {
            const size_t j = (size_t)CD * i + k;
            a.x[j] += alpha * a.p[j];
            rn[k] = a.r[j] - alpha * a.Ap[j];
            a.r[j] = rn[k];
        }
        block_matvec<CD>(a.sinv + (size_t)CD * CD * i, rn, z);
#pragma unroll
        for (int k = 0; k < CD; ++k) {
            a.z[CD * i + k] = z[k];
            rzn += rn[k] * z[k]; rr += rn[k] * rn[k];
        }
    }
    rzn = block_sum256(rzn, sh);
    rr = block_sum256(rr, sh);
    if (threadIdx.x == 0) { a.prz[(it & 1) ^ 1][blockIdx.x] = rzn; a.prr[blockIdx.x] = rr; }
}

// ---- the host's side of one solve from zero: batches of iterations enqueued ahead of the host (as many as the last solve needed + 2,
// then steps of 8, at most kBaMaxPcgIters), one read of the state word per batch.  What differs between the solvers:
struct PcgHooks {
    std::function<void()> product;                     // a.Ap = S a.p, gated by the state word's done flag
    std::function<BaState()> read;                     // waits for the stream; the state word
    std::function<void()> start;                       // empty: ba_pcg_init_kernel
    std::function<void(int it)> update;                // empty: ba_pcg_upd_kernel
};
struct PcgResult {
    int iters;
    double relres;
    bool capped;
};
// grid: the workgroups of the vector kernels (a.grid, unless the partial sums of a are laid out otherwise).  last: the iterations of the
// last solve that reached the tolerance, kept by the caller from one solve to the next (8 before the first)
template <int CD>
PcgResult pcg_solve_batched(const BaPcg &a, int grid, hipStream_t st, int &last, const PcgHooks &h) {
    const dim3 g(grid), b256(256);
    if (h.start) h.start();
    else hipLaunchKernelGGL((ba_pcg_init_kernel<CD>), g, b256, 0, st, a);
    int it = 0, dir_applied = 0;
    auto enqueue = [&](int upto) {
        for (; it < upto; ++it) {
            if (it != dir_applied) hipLaunchKernelGGL((ba_pcg_dir_kernel<CD>), g, b256, 0, st, a, it);
            h.product();
            if (h.update) h.update(it);
            else hipLaunchKernelGGL((ba_pcg_upd_kernel<CD>), g, b256, 0, st, a, it);
        }
        hipLaunchKernelGGL((ba_pcg_dir_kernel<CD>), g, b256, 0, st, a, it);   // convergence test of the last update (or the next direction)
        dir_applied = it;
    };
    int target = std::min(kBaMaxPcgIters, std::max(4, last + 2));
    BaState s;
    for (;;) {
        enqueue(target);
        s = h.read();
        if (s.done || target >= kBaMaxPcgIters) break;
        target = std::min(kBaMaxPcgIters, target + 8);
    }
    if (s.done && s.iters > 0) last = s.iters;
    return {s.done ? s.iters : target, s.relres, !s.done};
}

// scalars of the state word from the partials, in a fixed order (one workgroup): up to 6 sums and one max
constexpr int kBaSums = 6;
struct BaReduce {
    const double *sum_p[kBaSums];
    int sum_n[kBaSums];
    double *sum_out[kBaSums];
    const double *max_p;
    int max_n;
    double *max_out;
};
__global__ __launch_bounds__(256) void ba_reduce_kernel(BaReduce r) {
    __shared__ double sh[4];
    __shared__ double shm[4];
    for (int k = 0; k < kBaSums; ++k) {
        if (r.sum_out[k] == nullptr) continue;
        const double v = sum_partials256(r.sum_p[k], r.sum_n[k], sh);
        if (threadIdx.x == 0) *r.sum_out[k] = v;
    }
    if (r.max_out != nullptr) {
        double m = 0.0;
        for (int i = threadIdx.x; i < r.max_n; i += 256) m = fmax(m, r.max_p[i]);
        m = block_max<256>(m, shm);
        if (threadIdx.x == 0) *r.max_out = m;
    }
}

// the candidate's six sums into the state word s: cost and model (ge partials each, at cost), then |d|^2 and |x|^2 of the cameras (gfc
// each, at cand) and of the landmarks (gfl each, behind them)
inline BaReduce candidate_sums(const double *cost, int ge, const double *cand, int gfc, int gfl, BaState *s) {
    BaReduce rd{};
    rd.sum_p[0] = cost; rd.sum_n[0] = ge; rd.sum_out[0] = &s->cost_new;
    rd.sum_p[1] = cost + ge; rd.sum_n[1] = ge; rd.sum_out[1] = &s->model;
    rd.sum_p[2] = cand; rd.sum_n[2] = gfc; rd.sum_out[2] = &s->step2[0];
    rd.sum_p[3] = cand + gfc; rd.sum_n[3] = gfc; rd.sum_out[3] = &s->x2[0];
    rd.sum_p[4] = cand + 2 * (size_t)gfc; rd.sum_n[4] = gfl; rd.sum_out[4] = &s->step2[1];
    rd.sum_p[5] = cand + 2 * (size_t)gfc + gfl; rd.sum_n[5] = gfl; rd.sum_out[5] = &s->x2[1];
    return rd;
}
// the host's read of a state word: waits for the stream
template <class State>
State read_state(const State *dev, Pinned<State> &hs, hipStream_t st, double watchdog_s, const char *stage, const char *what) {
    check_launch(what);
    XM_HIP_CHECK(hipMemcpyAsync(hs.h, dev, sizeof(State), hipMemcpyDeviceToHost, st));
    wait_stream(st, watchdog_s, stage, what);
    return *hs.h;
}

// ---- candidate point.  Centres or points (K = 3 per item): x + d where the item is used, a copy elsewhere; partials of |d|^2 and |x|^2
// over the used ones.  (A template, so that only the files that launch it compile it.)
template <int K>
__global__ __launch_bounds__(256) void ba_cand_vec_kernel(int64_t n, const double *__restrict__ x, const double *__restrict__ d,
                                                          const int32_t *__restrict__ used, double *__restrict__ xn, double *__restrict__ parts) {
    __shared__ double sh[4];
    double s2 = 0.0, x2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double v = x[K * i + k];
            if (used[i]) { xn[K * i + k] = v + d[K * i + k]; s2 += d[K * i + k] * d[K * i + k]; x2 += v * v; }
            else xn[K * i + k] = v;
        }
    }
    s2 = block_sum256(s2, sh);
    x2 = block_sum256(x2, sh);
    if (threadIdx.x == 0) { parts[blockIdx.x] = s2; parts[gridDim.x + blockIdx.x] = x2; }
}

}  // namespace

}  // namespace xm
