// xm_schur.hip — matrix-free Q*W from the observation list (design: xm_schur.h).  Replaces, for the reference's own Q
// (utils/creatematrix.py:51-339), the dense product Dense/matmul.h:42-87 by the factor chain; the fused epilogues are those of
// xm_device.h, so the solver above (trust region, certificate, Lanczos) is unchanged.
#include "xm_schur.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "xm_device.h"

namespace xm {

// ------------------------------------------------------------------------------------------------------------------
// device kernels
// ------------------------------------------------------------------------------------------------------------------
// kSchurHeavy (xm_schur.h): landmarks with more observations get a workgroup of their own

// h_l = -(1/Q3_l) sum_{obs of l} w (p . W_i)      a light landmark: one thread | a heavy one: a 1024-thread workgroup (a landmark
// seen by all 13 682 cameras: 14 strided steps instead of 13 682 serial ones; thread-strided order, DPP tree per wavefront, the 16
// wavefront sums added in a fixed order)
constexpr int kSchurHeavyThreads = 1024;
// a gathered record of N doubles at 8-byte alignment with 16-byte loads (5 instead of 9 instructions for the 72-byte row block of W).
// Measured neutral at Final-13682 size: the scattered gathers are bound by cache LINES (one per lane), not by instructions.
typedef double schur_d2 __attribute__((ext_vector_type(2), aligned(8)));
template <int N>
__device__ __forceinline__ void load_rec(const double *__restrict__ p, double (&v)[N]) {
#pragma unroll
    for (int i = 0; i + 1 < N; i += 2) {
        const schur_d2 t = *reinterpret_cast<const schur_d2 *>(p + i);
        v[i] = t.x; v[i + 1] = t.y;
    }
    if (N & 1) v[N - 1] = p[N - 1];
}
template <int O>
__device__ __forceinline__ bool heavy_block_sum(double (&acc)[O]) {   // result valid in thread 0 (returns true there)
    __shared__ double part[kSchurHeavyThreads / 64][O];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < O; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < O; ++k) part[wv][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int k = 0; k < O; ++k) {
        double t = 0.0;
        for (int q = 0; q < kSchurHeavyThreads / 64; ++q) t += part[q][k];
        acc[k] = t;
    }
    return true;
}
// Landmark lists on the device (SchurLm): landmarks are numbered by degree, descending ("slot").  The first nheavy slots keep contiguous
// lists [ptr[s], ptr[s+1]) (one workgroup each); the others are packed 64 to a group in slot order -- observation k of the group's lane
// j sits at gbase[group] + 64 k + j, so the thread-per-landmark kernels read cam / w / p as coalesced 64-wide rows (a contiguous list
// per thread made every load instruction touch 64 cache lines: 180 us for h at 800 k landmarks / 6.4 M observations, 5 x its traffic).
// p is stored as three planes of `total` doubles.
struct SchurLm {
    int64_t m, nheavy, total;
    const int64_t *ptr;      // nheavy + 1
    const int64_t *gbase;    // per group of 64 light slots
    const int32_t *deg;      // per slot
    const int32_t *cam;
    const double *w, *p;
};
// ONE launch for both kinds: workgroups [0, nheavy) take a heavy landmark each (1024 threads stride its list), the others 1024 light
// landmarks each -- the few heavy workgroups (14 serial steps for a landmark seen by all 13 682 cameras) run beside the light ones
// instead of after them (32 + 14 us of the chain at Final-13682 size)
template <int O>
__global__ __launch_bounds__(kSchurHeavyThreads) void schur_lm_h_kernel(SchurLm L, const double *__restrict__ q3inv,
                                                          const double *__restrict__ W, const TcgScal *__restrict__ scal, double *__restrict__ h) {
    constexpr int OP = pitch_of(O);
    if (scal != nullptr) {
        if (scal->status != 0) return;
    }
    const bool heavy = (int64_t)blockIdx.x < L.nheavy;   // workgroup-uniform
    int64_t l, e, e_end, step;
    if (heavy) {
        l = blockIdx.x; e = L.ptr[l] + threadIdx.x; e_end = L.ptr[l + 1]; step = kSchurHeavyThreads;
    } else {
        const int64_t t = ((int64_t)blockIdx.x - L.nheavy) * kSchurHeavyThreads + threadIdx.x;
        l = L.nheavy + t;
        if (l >= L.m) return;
        e = L.gbase[t >> 6] + (t & 63); e_end = e + (int64_t)64 * L.deg[l]; step = 64;
    }
    double acc[O];
#pragma unroll
    for (int k = 0; k < O; ++k) acc[k] = 0.0;
    for (; e < e_end; e += step) {
        double Wi[3 * OP];
        load_rec<3 * OP>(W + (size_t)L.cam[e] * 3 * OP, Wi);
        const double w = L.w[e], p0 = L.p[e], p1 = L.p[L.total + e], p2 = L.p[2 * L.total + e];
#pragma unroll
        for (int k = 0; k < O; ++k) acc[k] += w * (p0 * Wi[k] + p1 * Wi[OP + k] + p2 * Wi[2 * OP + k]);
    }
    const double qi = q3inv[l];
    if (heavy) {
        if (!heavy_block_sum<O>(acc)) return;
    }
#pragma unroll
    for (int k = 0; k < O; ++k) h[(size_t)l * OP + k] = -acc[k] * qi;
}

// r_{i-1} = c_i . W_i + sum_{obs of i} w h_l      one wavefront per camera (a camera has hundreds of observations; fixed lane-strided
// order + DPP tree: bit-reproducible)
template <int O>
__global__ __launch_bounds__(256) void schur_cam_r_kernel(int n, const int64_t *__restrict__ cam_ptr, const int32_t *__restrict__ cam_lm,
                                                           const double *__restrict__ cam_w, const double *__restrict__ c,
                                                           const double *__restrict__ W, const double *__restrict__ h,
                                                           const TcgScal *__restrict__ scal, double *__restrict__ r) {
    constexpr int OP = pitch_of(O);
    if (scal != nullptr) {
        if (scal->status != 0) return;
    }
    const int gl = threadIdx.x & 63, cam = blockIdx.x * kQwWaves + (threadIdx.x >> 6);
    double acc[O];
#pragma unroll
    for (int k = 0; k < O; ++k) acc[k] = 0.0;
    if (cam < n && cam >= 1)
        for (int64_t e = cam_ptr[cam] + gl; e < cam_ptr[cam + 1]; e += 64) {
            const double w = cam_w[e];
            double hl[O];
            load_rec<O>(h + (size_t)cam_lm[e] * OP, hl);
#pragma unroll
            for (int k = 0; k < O; ++k) acc[k] += w * hl[k];
        }
#pragma unroll
    for (int k = 0; k < O; ++k) acc[k] = wave_sum(acc[k]);
    if (cam < n && cam >= 1 && gl == 0) {
        const double *Wi = W + (size_t)cam * 3 * OP, *ci = c + (size_t)cam * 3;
#pragma unroll
        for (int k = 0; k < O; ++k) r[(size_t)(cam - 1) * OP + k] = acc[k] + ci[0] * Wi[k] + ci[1] * Wi[OP + k] + ci[2] * Wi[2 * OP + k];
    }
}

// x_l = h_l + (1/Q3_l) sum_{obs of l} w x_cam_i     (x_cam of the anchor camera 0 is 0: its translation is the gauge)
template <int O>
__global__ __launch_bounds__(kSchurHeavyThreads) void schur_lm_x_kernel(SchurLm L, const double *__restrict__ q3inv, const double *__restrict__ h,
                                                          const double *__restrict__ xc, const TcgScal *__restrict__ scal,
                                                          double *__restrict__ xl) {
    constexpr int OP = pitch_of(O);
    if (scal != nullptr) {
        if (scal->status != 0) return;
    }
    const bool heavy = (int64_t)blockIdx.x < L.nheavy;
    int64_t l, e, e_end, step;
    if (heavy) {
        l = blockIdx.x; e = L.ptr[l] + threadIdx.x; e_end = L.ptr[l + 1]; step = kSchurHeavyThreads;
    } else {
        const int64_t t = ((int64_t)blockIdx.x - L.nheavy) * kSchurHeavyThreads + threadIdx.x;
        l = L.nheavy + t;
        if (l >= L.m) return;
        e = L.gbase[t >> 6] + (t & 63); e_end = e + (int64_t)64 * L.deg[l]; step = 64;
    }
    double acc[O];
#pragma unroll
    for (int k = 0; k < O; ++k) acc[k] = 0.0;
    for (; e < e_end; e += step) {
        const int i = L.cam[e];
        if (i == 0) continue;
        const double w = L.w[e];
        double xi[O];
        load_rec<O>(xc + (size_t)(i - 1) * OP, xi);
#pragma unroll
        for (int k = 0; k < O; ++k) acc[k] += w * xi[k];
    }
    const double qi = q3inv[l];
    if (heavy) {
        if (!heavy_block_sum<O>(acc)) return;
    }
#pragma unroll
    for (int k = 0; k < O; ++k) xl[(size_t)l * OP + k] = h[(size_t)l * OP + k] + acc[k] * qi;
}

// Y_i = Q1_i W_i - c_i x_cam_i + sum_{obs of i} w p x_l, then the common tail of the Q*W kernels (xm_device.h)
template <int O, int EPI>
__global__ __launch_bounds__(256) void schur_cam_y_kernel(int64_t n, int64_t nobs, const int64_t *__restrict__ cam_ptr, const int32_t *__restrict__ cam_lm,
                                                           const double *__restrict__ cam_w, const double *__restrict__ cam_p,
                                                           const double *__restrict__ Q1, const double *__restrict__ c,
                                                           const double *__restrict__ W, const double *__restrict__ xc,
                                                           const double *__restrict__ xl, double alpha, CamArgs a) {
    constexpr int OP = pitch_of(O);
    if (EPI == EPI_HESS) {
        if (a.scal->status != 0) return;
    }
    __shared__ double red[kQwWaves][3];
    const int gl = threadIdx.x & 63, slot = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lcam = blockIdx.x * kQwWaves + slot;   // camera of THIS rank (epilogue arrays); cam: its global index (observation lists, W, Q1, c)
    const bool active = lcam < a.nloc;
    const int64_t cam = (int64_t)a.cam0 + lcam;
    EpiOps eops;
    epi_prefetch<O, EPI>(eops, active ? lcam : 0, gl, active, a);
    double acc[3][O];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < O; ++k) acc[r][k] = 0.0;
    if (active && cam < n) {   // (cam >= n: an inert padding camera of the row partition -- zero row)
        for (int64_t e = cam_ptr[cam] + gl; e < cam_ptr[cam + 1]; e += 64) {
            const double w = cam_w[e];
            double x[O];
            load_rec<O>(xl + (size_t)cam_lm[e] * OP, x);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double wp = w * cam_p[(size_t)r * (size_t)nobs + e];   // three planes: coalesced
#pragma unroll
                for (int k = 0; k < O; ++k) acc[r][k] += wp * x[k];
            }
        }
        if (gl == 0) {
            const double *Wi = W + (size_t)cam * 3 * OP, *q = Q1 + (size_t)cam * 9, *ci = c + (size_t)cam * 3;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < O; ++k) {
                    const double xk = (cam >= 1) ? xc[(size_t)(cam - 1) * OP + k] : 0.0;
                    acc[r][k] += q[3 * r] * Wi[k] + q[3 * r + 1] * Wi[OP + k] + q[3 * r + 2] * Wi[2 * OP + k] - ci[r] * xk;
                }
        }
    }
    qw_finish<O, EPI, 64, kQwWaves>(lcam, gl, slot, active, acc, alpha, a, eops, red);
}


// ------------------------------------------------------------------------------------------------------------------
// The reduced camera Laplacian WITHOUT its inverse ("a sparse Cholesky of the reduced Laplacian" -- here: no factorisation at
// all).  x_cam = VT^-1 r is solved per product by preconditioned CG on  VT = Q2_bar - V3_bar Q3^-1 V3_bar^T  applied matrix-free through the
// two observation lists (by landmark: y_l = (1/Q3_l) sum w x_cam; by camera: (VT x)_i = Q2_i x_i - sum w y_l -- the kernels of the chain
// itself), Jacobi preconditioner diag(VT), the o columns of the right-hand side advanced together with their own alpha / beta.  No
// (N-1)^2 array exists: memory and set-up are O(observations); the dense inverse costs 8 (N-1)^2 bytes (1.5 GB at 13 682 cameras, 80 GB
// at 100 k) and an O(N^3) factorisation.  Every scalar is a fixed-order sum of per-workgroup partial sums that each workgroup adds up
// itself (as cg_step_kernel does): no atomics, no grid barrier, bit-reproducible.  Launches per iteration: direction, landmark pass,
// camera pass (+ <p, VT p> partials), update (+ <r, z>, |r|^2 partials).
// ------------------------------------------------------------------------------------------------------------------
struct PcgState {             // device-resident; written by workgroup 0 of the kernel that decides
    int32_t done;             // 1: every column reached the tolerance (or the tCG launch this product belongs to is a no-op)
    int32_t iters;            // iterations performed
    double relres;            // max over the columns of |r| / |b| when it stopped
};
struct PcgArgs {
    int n1;                   // N - 1 unknowns per column
    int grid;                 // workgroups of the flat kernels == partial sums per column
    double tol2;              // (relative residual)^2 to reach
    const double *b;          // right-hand side r_ (pitch OP)
    union {
        const double *dinv;   // 1 / diag(VT), n1
        const double *z;      // two-level preconditioner (TL kernels): z = M^-1 r, pitch OP, written by pcg_block_kernel / pcg_coarse_kernel
    };
    const double *q2;         // Q2 per camera (index cam)
    double *x, *r, *p, *Ap;   // pitch OP, n1 records
    double *prz[2], *prr, *pbb;   // per-workgroup partial sums of <r,z> (by iteration parity), |r|^2, |b|^2: grid * O each (column-major: [k][workgroup])
    double *ppap;             // the same of <p, VT p> from the camera pass: cam_grid * O
    int cam_grid;
    PcgState *st;
};
template <int O>
__device__ __forceinline__ void pcg_sums(const double *parts, int grid, double (&out)[O], double *sh) {
#pragma unroll
    for (int k = 0; k < O; ++k) out[k] = sum_partials256(parts + (size_t)k * grid, grid, sh);
}
template <int O>
__device__ __forceinline__ void pcg_store_partials(const double (&acc)[O], double *parts, int grid, double *sh) {
#pragma unroll
    for (int k = 0; k < O; ++k) {
        const double t = block_sum256(acc[k], sh);
        if (threadIdx.x == 0) parts[(size_t)k * grid + blockIdx.x] = t;
    }
}
// x = 0, r = b, p = z = dinv .* r; partials of <r, z> (parity 0) and |b|^2.  TL (two-level preconditioner): x = 0, r = b and |b|^2 only --
// z, p = z and <r, z> come from pcg_block_kernel + pcg_coarse_kernel behind this launch
template <int O, bool TL = false>
__global__ __launch_bounds__(256) void pcg_init_kernel(PcgArgs a, const TcgScal *__restrict__ scal) {
    constexpr int OP = pitch_of(O);
    __shared__ double sh[4];
    if (scal != nullptr && scal->status != 0) {   // a launch enqueued past the end of the tCG: nothing to solve
        if (blockIdx.x == 0 && threadIdx.x == 0) { a.st->done = 1; a.st->iters = 0; a.st->relres = 0.0; }
        return;
    }
    double rz[O], bb[O];
#pragma unroll
    for (int k = 0; k < O; ++k) rz[k] = bb[k] = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n1; i += gridDim.x * 256) {
        if constexpr (TL) {
#pragma unroll
            for (int k = 0; k < O; ++k) {
                const double v = a.b[(size_t)i * OP + k];
                a.x[(size_t)i * OP + k] = 0.0; a.r[(size_t)i * OP + k] = v;
                bb[k] += v * v;
            }
        } else {
            const double di = a.dinv[i];
#pragma unroll
            for (int k = 0; k < O; ++k) {
                const double v = a.b[(size_t)i * OP + k], z = di * v;
                a.x[(size_t)i * OP + k] = 0.0; a.r[(size_t)i * OP + k] = v; a.p[(size_t)i * OP + k] = z;
                rz[k] += v * z; bb[k] += v * v;
            }
        }
    }
    if constexpr (!TL) pcg_store_partials<O>(rz, a.prz[0], a.grid, sh);
    pcg_store_partials<O>(bb, a.pbb, a.grid, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.st->done = 0; a.st->iters = 0; a.st->relres = 1.0; }
}
// iteration it >= 1: beta = <r,z>_new / <r,z>_old per column, p = z + beta p; decides whether the previous update reached the tolerance
template <int O, bool TL = false>
__global__ __launch_bounds__(256) void pcg_dir_kernel(PcgArgs a, int it) {
    constexpr int OP = pitch_of(O);
    __shared__ double sh[4];
    __shared__ int was_done;
    if (threadIdx.x == 0) was_done = a.st->done;   // ONE read per workgroup: workgroup 0 may set the flag while later workgroups start
    __syncthreads();
    if (was_done) return;
    double rzn[O], rzo[O], rr[O], bb[O];
    pcg_sums<O>(a.prz[it & 1], a.grid, rzn, sh);
    pcg_sums<O>(a.prz[(it & 1) ^ 1], a.grid, rzo, sh);
    pcg_sums<O>(a.prr, a.grid, rr, sh);
    pcg_sums<O>(a.pbb, a.grid, bb, sh);
    bool conv = true;
    double worst = 0.0;
#pragma unroll
    for (int k = 0; k < O; ++k) {
        const double q = (bb[k] > 0.0) ? rr[k] / bb[k] : 0.0;
        worst = fmax(worst, q);
        if (!(q <= a.tol2)) conv = false;
    }
    if (conv) {   // identical decision in every workgroup (identical sums); workgroup 0 publishes it for the launches behind this one.  The
                  // flag is written only AFTER every workgroup has read it above: all of them read st->done before this store can matter,
                  // because a workgroup that sees done == 1 here returns exactly as one that computes conv itself
        if (blockIdx.x == 0 && threadIdx.x == 0) { a.st->done = 1; a.st->iters = it; a.st->relres = sqrt(worst); }
        return;
    }
    double beta[O];
#pragma unroll
    for (int k = 0; k < O; ++k) beta[k] = (rzo[k] > 0.0) ? rzn[k] / rzo[k] : 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n1; i += gridDim.x * 256) {
        if constexpr (TL) {
#pragma unroll
            for (int k = 0; k < O; ++k) a.p[(size_t)i * OP + k] = a.z[(size_t)i * OP + k] + beta[k] * a.p[(size_t)i * OP + k];
        } else {
            const double di = a.dinv[i];
#pragma unroll
            for (int k = 0; k < O; ++k) a.p[(size_t)i * OP + k] = di * a.r[(size_t)i * OP + k] + beta[k] * a.p[(size_t)i * OP + k];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.st->iters = it; a.st->relres = sqrt(worst); }
}
// y_l = (1/Q3_l) sum_{obs of l} w p_cam   (the anchor camera 0 is not an unknown)
template <int O>
__global__ __launch_bounds__(kSchurHeavyThreads) void pcg_lm_kernel(SchurLm L, const double *__restrict__ q3inv, const double *__restrict__ pv,
                                                                  const PcgState *__restrict__ st, double *__restrict__ y) {
    constexpr int OP = pitch_of(O);
    if (st->done) return;
    const bool heavy = (int64_t)blockIdx.x < L.nheavy;
    int64_t l, e, e_end, step;
    if (heavy) {
        l = blockIdx.x; e = L.ptr[l] + threadIdx.x; e_end = L.ptr[l + 1]; step = kSchurHeavyThreads;
    } else {
        const int64_t t = ((int64_t)blockIdx.x - L.nheavy) * kSchurHeavyThreads + threadIdx.x;
        l = L.nheavy + t;
        if (l >= L.m) return;
        e = L.gbase[t >> 6] + (t & 63); e_end = e + (int64_t)64 * L.deg[l]; step = 64;
    }
    double acc[O];
#pragma unroll
    for (int k = 0; k < O; ++k) acc[k] = 0.0;
    for (; e < e_end; e += step) {
        const int i = L.cam[e];
        if (i == 0) continue;
        const double w = L.w[e];
        double xi[O];
        load_rec<O>(pv + (size_t)(i - 1) * OP, xi);
#pragma unroll
        for (int k = 0; k < O; ++k) acc[k] += w * xi[k];
    }
    const double qi = q3inv[l];
    if (heavy) {
        if (!heavy_block_sum<O>(acc)) return;
    }
#pragma unroll
    for (int k = 0; k < O; ++k) y[(size_t)l * OP + k] = acc[k] * qi;
}
// Ap_i = Q2_i p_i - sum_{obs of i} w y_l, one wavefront per camera 1..N-1; per-workgroup partials of <p, Ap>
template <int O>
__global__ __launch_bounds__(256) void pcg_cam_kernel(int n, const int64_t *__restrict__ cam_ptr, const int32_t *__restrict__ cam_lm,
                                                       const double *__restrict__ cam_w, const double *__restrict__ y, PcgArgs a) {
    constexpr int OP = pitch_of(O);
    __shared__ double red[kQwWaves][O];
    if (a.st->done) return;
    const int gl = threadIdx.x & 63, wv = threadIdx.x >> 6, cam = blockIdx.x * kQwWaves + wv;
    double acc[O];
#pragma unroll
    for (int k = 0; k < O; ++k) acc[k] = 0.0;
    const bool on = cam < n && cam >= 1;
    if (on)
        for (int64_t e = cam_ptr[cam] + gl; e < cam_ptr[cam + 1]; e += 64) {
            const double w = cam_w[e];
            double yl[O];
            load_rec<O>(y + (size_t)cam_lm[e] * OP, yl);
#pragma unroll
            for (int k = 0; k < O; ++k) acc[k] += w * yl[k];
        }
#pragma unroll
    for (int k = 0; k < O; ++k) acc[k] = wave_sum(acc[k]);
    if (gl == 0) {
#pragma unroll
        for (int k = 0; k < O; ++k) {
            double pap = 0.0;
            if (on) {
                const double pk = a.p[(size_t)(cam - 1) * OP + k];
                const double v = a.q2[cam] * pk - acc[k];
                a.Ap[(size_t)(cam - 1) * OP + k] = v;
                pap = pk * v;
            }
            red[wv][k] = pap;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < O; ++k) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < kQwWaves; ++q) t += red[q][k];
            a.ppap[(size_t)k * gridDim.x + blockIdx.x] = t;
        }
    }
}
// alpha = <r,z> / <p,Ap> per column; x += alpha p, r -= alpha Ap; partials of the new <r,z> (other parity) and |r|^2.  TL: |r|^2 only (the
// new <r,z> is pcg_coarse_kernel's)
template <int O, bool TL = false>
__global__ __launch_bounds__(256) void pcg_upd_kernel(PcgArgs a, int it) {
    constexpr int OP = pitch_of(O);
    __shared__ double sh[4];
    if (a.st->done) return;
    double rz[O], pap[O], alpha[O];
    pcg_sums<O>(a.prz[it & 1], a.grid, rz, sh);
    pcg_sums<O>(a.ppap, a.cam_grid, pap, sh);
#pragma unroll
    for (int k = 0; k < O; ++k) alpha[k] = (pap[k] > 0.0 && rz[k] > 0.0) ? rz[k] / pap[k] : 0.0;
    double rzn[O], rr[O];
#pragma unroll
    for (int k = 0; k < O; ++k) rzn[k] = rr[k] = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n1; i += gridDim.x * 256) {
        if constexpr (TL) {
#pragma unroll
            for (int k = 0; k < O; ++k) {
                const size_t j = (size_t)i * OP + k;
                a.x[j] += alpha[k] * a.p[j];
                const double rn = a.r[j] - alpha[k] * a.Ap[j];
                a.r[j] = rn;
                rr[k] += rn * rn;
            }
        } else {
            const double di = a.dinv[i];
#pragma unroll
            for (int k = 0; k < O; ++k) {
                const size_t j = (size_t)i * OP + k;
                a.x[j] += alpha[k] * a.p[j];
                const double rn = a.r[j] - alpha[k] * a.Ap[j];
                a.r[j] = rn;
                rzn[k] += rn * rn * di; rr[k] += rn * rn;
            }
        }
    }
    if constexpr (!TL) pcg_store_partials<O>(rzn, a.prz[(it & 1) ^ 1], a.grid, sh);
    pcg_store_partials<O>(rr, a.prr, a.grid, sh);
}
// 1 / diag(VT):  diag_i = Q2_i - sum_{obs of i} w^2 / Q3_l   (one wavefront per camera; set-up)
__global__ __launch_bounds__(256) void pcg_diag_kernel(int n, const int64_t *__restrict__ cam_ptr, const int32_t *__restrict__ cam_lm,
                                                        const double *__restrict__ cam_w, const double *__restrict__ q3inv,
                                                        const double *__restrict__ q2, double *__restrict__ dinv) {
    const int gl = threadIdx.x & 63, cam = blockIdx.x * kQwWaves + (threadIdx.x >> 6);
    double acc = 0.0;
    if (cam < n && cam >= 1)
        for (int64_t e = cam_ptr[cam] + gl; e < cam_ptr[cam + 1]; e += 64) { const double w = cam_w[e]; acc += w * w * q3inv[cam_lm[e]]; }
    acc = wave_sum(acc);
    if (cam < n && cam >= 1 && gl == 0) {
        const double d = q2[cam] - acc;
        dinv[cam - 1] = (d > 0.0) ? 1.0 / d : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Two-level additive Schwarz preconditioner of the CG form (xm_tuning_t.schur_solver = 3):
//      M^-1 r = blockdiag(VT_aa)^-1 r + P A_c^-1 P^T r
// a: aggregates of at most kSchurAggCams cameras (schur_aggregate_plan: runs of a breadth-first order, so that an aggregate is a stretch of
// the co-visibility graph), VT_aa: the exact principal block of VT, P: the 0/1 camera -> aggregate map, A_c = P^T VT P.  Both terms are SPD
// when VT is, so plain PCG stays valid.  Jacobi's diag(VT)^-1 VT is well conditioned only on expander-like graphs (random co-visibility);
// on a sequential capture VT is close to a path Laplacian and Jacobi needs O(N) iterations, the coarse term removes the smooth error
// the blocks cannot see.  Two launches per iteration behind pcg_upd_kernel<O, true>; every sum in a fixed order (no atomics).
// ------------------------------------------------------------------------------------------------------------------
struct PcgTwoLevel {
    int64_t nagg;
    const int32_t *perm;      // nagg * kSchurAggCams: reduced camera (camera - 1) at each row of each aggregate, -1 = padding
    const double *binv;       // nagg blocks of kSchurAggCams^2: VT_aa^-1, symmetric
    const double *ainv;       // nagg x nagg: A_c^-1, symmetric
    double *g;                // P^T r: nagg * O
    double *z;                // M^-1 r (= PcgArgs.z)
};
// z_a = VT_aa^-1 r_a and g_a = sum_{i in a} r_i: one wavefront per aggregate, a lane per row; the block inverse is read by columns (coalesced)
template <int O>
__global__ __launch_bounds__(256) void pcg_block_kernel(PcgArgs a, PcgTwoLevel t) {
    constexpr int OP = pitch_of(O), B = kSchurAggCams;
    __shared__ double rs[kQwWaves][B][O];
    if (a.st->done) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ag = (int64_t)blockIdx.x * kQwWaves + wv;
    if (ag >= t.nagg) return;   // wavefront-uniform; no workgroup barrier below
    const int i = t.perm[ag * B + lane];
    double ri[O];
#pragma unroll
    for (int k = 0; k < O; ++k) {
        ri[k] = (i >= 0) ? a.r[(size_t)i * OP + k] : 0.0;
        rs[wv][lane][k] = ri[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double z[O];
#pragma unroll
    for (int k = 0; k < O; ++k) z[k] = 0.0;
    const double *col = t.binv + (size_t)ag * B * B + lane;
    for (int m = 0; m < B; ++m) {
        const double bm = col[(size_t)m * B];
#pragma unroll
        for (int k = 0; k < O; ++k) z[k] += bm * rs[wv][m][k];
    }
    if (i >= 0) {
#pragma unroll
        for (int k = 0; k < O; ++k) t.z[(size_t)i * OP + k] = z[k];
    }
#pragma unroll
    for (int k = 0; k < O; ++k) ri[k] = wave_sum(ri[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < O; ++k) t.g[(size_t)ag * O + k] = ri[k];
    }
}
// z_i += (A_c^-1 g)_{a(i)} (one wavefront per aggregate, grid-strided over the aggregates; the row of A_c^-1 lane-strided + DPP tree), init:
// p = z as well; partials of <r, z> into parity `par` (grid: the flat kernels' -- pcg_dir_kernel sums them)
template <int O>
__global__ __launch_bounds__(256) void pcg_coarse_kernel(PcgArgs a, PcgTwoLevel t, int par, int init) {
    constexpr int OP = pitch_of(O), B = kSchurAggCams;
    __shared__ double sh[4];
    if (a.st->done) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double rz[O];
#pragma unroll
    for (int k = 0; k < O; ++k) rz[k] = 0.0;
    for (int64_t ag = (int64_t)blockIdx.x * kQwWaves + wv; ag < t.nagg; ag += (int64_t)gridDim.x * kQwWaves) {
        double c[O];
#pragma unroll
        for (int k = 0; k < O; ++k) c[k] = 0.0;
        const double *row = t.ainv + (size_t)ag * (size_t)t.nagg;
        for (int64_t b = lane; b < t.nagg; b += 64) {
            const double v = row[b];
#pragma unroll
            for (int k = 0; k < O; ++k) c[k] += v * t.g[(size_t)b * O + k];
        }
#pragma unroll
        for (int k = 0; k < O; ++k) c[k] = wave_sum(c[k]);
        const int i = t.perm[ag * B + lane];
        if (i >= 0) {
#pragma unroll
            for (int k = 0; k < O; ++k) {
                const size_t j = (size_t)i * OP + k;
                const double zz = t.z[j] + c[k];
                t.z[j] = zz;
                if (init) a.p[j] = zz;
                rz[k] += a.r[j] * zz;
            }
        }
    }
    pcg_store_partials<O>(rz, a.prz[par], a.grid, sh);
}

// set-up (every set_weights): U_g = the weights of group g's observations summed in list order (group: the observations of one landmark
// whose cameras fall in one aggregate)
__global__ __launch_bounds__(256) void tl_group_sum_kernel(int64_t ng, const int64_t *__restrict__ eptr, const int64_t *__restrict__ eobs,
                                                            const double *__restrict__ w, double *__restrict__ u) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= ng) return;
    double s = 0.0;
    for (int64_t e = eptr[g]; e < eptr[g + 1]; ++e) s += w[eobs[e]];
    u[g] = s;
}
// A_c entry (a, b), a >= b, one thread each: [a == b] sum_{i in a} Q2_i - sum over its group pairs (light landmarks in slot order) of
// (1/Q3_l) U_g1 U_g2; written to both triangles (column-major).  Heavy landmarks follow as rank-1 terms (rank1_sub_device).
__global__ __launch_bounds__(256) void tl_coarse_entries_kernel(int64_t nent, const int64_t *__restrict__ cptr, const int32_t *__restrict__ cab,
                                                                 const int32_t *__restrict__ cpair, const int32_t *__restrict__ gslot,
                                                                 const double *__restrict__ u, const double *__restrict__ q3inv,
                                                                 const int32_t *__restrict__ perm, const double *__restrict__ q2, int64_t nagg,
                                                                 double *__restrict__ A) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nent) return;
    const int64_t a = cab[2 * k], b = cab[2 * k + 1];
    double v = 0.0;
    if (a == b)
        for (int j = 0; j < kSchurAggCams; ++j) {
            const int i = perm[a * kSchurAggCams + j];
            if (i >= 0) v += q2[i + 1];
        }
    for (int64_t q = cptr[k]; q < cptr[k + 1]; ++q) {
        const int32_t g1 = cpair[2 * q], g2 = cpair[2 * q + 1];
        v -= q3inv[gslot[g1]] * u[g1] * u[g2];
    }
    A[(size_t)a + (size_t)b * nagg] = v;
    A[(size_t)b + (size_t)a * nagg] = v;
}
// VT_aa^-1 for one aggregate per workgroup (one wavefront, lane j owns column j of the block in LDS): diag(Q2), then per group in slot order
// -= (1/Q3_l) u u^T with u the group's weights by row (a row named twice sums: lane j's u_j, then every entry of the group into column j in
// list order), then Gauss-Jordan inversion in place without pivoting -- on an SPD matrix every pivot is the diagonal of a Schur complement,
// positive exactly when the block is positive definite (else *fail = 1) -- written out symmetrised.  Rows beyond the aggregate: identity.
__global__ __launch_bounds__(64) void tl_block_inverse_kernel(const int32_t *__restrict__ perm, const int64_t *__restrict__ gptr,
                                                               const int32_t *__restrict__ gslot, const int64_t *__restrict__ eptr,
                                                               const int32_t *__restrict__ eloc, const int64_t *__restrict__ eobs,
                                                               const double *__restrict__ w, const double *__restrict__ q3inv,
                                                               const double *__restrict__ q2, double *__restrict__ binv, int32_t *__restrict__ fail) {
    constexpr int B = kSchurAggCams;
    __shared__ double A[B * B];   // A[i * B + j]: row i, column j
    __shared__ double colk[B];
    const int j = threadIdx.x;
    const int64_t ag = blockIdx.x;
    const int cj = perm[ag * B + j];
    for (int i = 0; i < B; ++i) A[i * B + j] = (i == j) ? (cj >= 0 ? q2[cj + 1] : 1.0) : 0.0;
    for (int64_t g = gptr[ag]; g < gptr[ag + 1]; ++g) {   // wavefront-uniform
        const double q = q3inv[gslot[g]];
        if (q == 0.0) continue;
        double uj = 0.0;
        for (int64_t e = eptr[g]; e < eptr[g + 1]; ++e)
            if (eloc[e] == j) uj += w[eobs[e]];
        if (uj == 0.0) continue;
        const double qu = q * uj;
        for (int64_t e = eptr[g]; e < eptr[g + 1]; ++e) A[eloc[e] * B + j] -= w[eobs[e]] * qu;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    bool ok = true;
    for (int k = 0; k < B; ++k) {
        const double piv = A[k * B + k];
        colk[j] = A[j * B + k];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (!(piv > 0.0)) { ok = false; break; }   // (uniform)
        const double akj = ((j == k) ? 1.0 : A[k * B + j]) / piv;
        for (int i = 0; i < B; ++i) {
            if (i == k) A[i * B + j] = akj;
            else A[i * B + j] = ((j == k) ? 0.0 : A[i * B + j]) - colk[i] * akj;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (!ok) {
        if (j == 0) *fail = 1;
        return;
    }
    double *out = binv + (size_t)ag * B * B;
    for (int i = 0; i < B; ++i) out[i * B + j] = 0.5 * (A[i * B + j] + A[j * B + i]);
}

// ------------------------------------------------------------------------------------------------------------------
// device: everything that depends on the weights (round 4; the host version below stays as the fall-back for observation lists that name
// a (camera, landmark) pair twice).  utils/creatematrix.py:62-175 restated on the observation level.
// ------------------------------------------------------------------------------------------------------------------
// weights in input order -> the by-camera and by-landmark arrays
__global__ __launch_bounds__(256) void schur_scatter_w_kernel(int64_t nobs, const double *__restrict__ w, const int64_t *__restrict__ pos_c,
                                                               const int64_t *__restrict__ dpos_l, double *__restrict__ cam_w, double *__restrict__ lm_w) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nobs) return;
    const double x = w[e];
    cam_w[pos_c[e]] = x;
    lm_w[dpos_l[e]] = x;
}
// per camera: Q1 = sum w p p^T (creatematrix.py:26), c = V1 = sum w p (:27), Q2 = sum w (:68); one wavefront per camera, lane-strided
// list order + DPP tree (fixed order)
__global__ __launch_bounds__(256) void schur_cam_sums_kernel(int64_t n, int64_t nobs, const int64_t *__restrict__ cam_ptr, const double *__restrict__ cam_w,
                                                              const double *__restrict__ cam_p, double *__restrict__ Q1, double *__restrict__ c,
                                                              double *__restrict__ q2) {
    const int gl = threadIdx.x & 63;
    const int64_t cam = (int64_t)blockIdx.x * kQwWaves + (threadIdx.x >> 6);
    double a[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) a[k] = 0.0;
    if (cam < n)
        for (int64_t e = cam_ptr[cam] + gl; e < cam_ptr[cam + 1]; e += 64) {
            const double w = cam_w[e], p0 = cam_p[e], p1 = cam_p[nobs + e], p2 = cam_p[2 * nobs + e];
            const double pp[3] = {p0, p1, p2};
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                a[9 + x] += w * pp[x];
#pragma unroll
                for (int y = 0; y < 3; ++y) a[3 * x + y] += w * pp[x] * pp[y];
            }
            a[12] += w;
        }
#pragma unroll
    for (int k = 0; k < 13; ++k) a[k] = wave_sum(a[k]);
    if (cam < n && gl == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) Q1[cam * 9 + k] = a[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[cam * 3 + k] = a[9 + k];
        q2[cam] = a[12];
    }
}
// per landmark slot: 1 / Q3, Q3 = sum w over its observations (:69); a landmark without weight drops out (0)
__global__ __launch_bounds__(kSchurHeavyThreads) void schur_lm_q3_kernel(SchurLm L, double *__restrict__ q3inv) {
    const bool heavy = (int64_t)blockIdx.x < L.nheavy;
    int64_t l, e, e_end, step;
    if (heavy) {
        l = blockIdx.x; e = L.ptr[l] + threadIdx.x; e_end = L.ptr[l + 1]; step = kSchurHeavyThreads;
    } else {
        const int64_t t = ((int64_t)blockIdx.x - L.nheavy) * kSchurHeavyThreads + threadIdx.x;
        l = L.nheavy + t;
        if (l >= L.m) return;
        e = L.gbase[t >> 6] + (t & 63); e_end = e + (int64_t)64 * L.deg[l]; step = 64;
    }
    double acc[1] = {0.0};
    for (; e < e_end; e += step) acc[0] += L.w[e];
    if (heavy) {
        if (!heavy_block_sum<1>(acc)) return;
    }
    q3inv[l] = (acc[0] > 0.0) ? 1.0 / acc[0] : 0.0;
}
// the reduced camera Laplacian VT = Q2_bar - V3_bar Q3^-1 V3_bar^T (:150-166) row by row: ONE wavefront per camera a, the row (columns
// [col0, col0 + ncol)) in LDS; the camera's observations are walked in list order and for each the landmark's observation list is spread
// over the lanes (a landmark names a camera once: no two lanes meet on one entry; the additions into an entry happen in the camera's
// observation order -- the order of the host assembly this replaces).  Landmarks with more than kSchurHeavy observations are full rank-1
// terms and are applied afterwards (rank1_sub_device).
__global__ __launch_bounds__(64) void schur_vt_rows_kernel(int64_t mr, int64_t col0, int ncol, const int64_t *__restrict__ cam_ptr,
                                                            const int32_t *__restrict__ cam_lm, const double *__restrict__ cam_w, SchurLm L,
                                                            const double *__restrict__ q3inv, const double *__restrict__ q2, double *__restrict__ VT) {
    extern __shared__ double row[];
    const int lane = threadIdx.x;
    const int64_t a = (int64_t)blockIdx.x + 1;
    for (int j = lane; j < ncol; j += 64) row[j] = 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0 && a - 1 >= col0 && a - 1 < col0 + ncol) row[a - 1 - col0] = q2[a];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int64_t e = cam_ptr[a]; e < cam_ptr[a + 1]; ++e) {   // wave-uniform
        const int64_t sl = cam_lm[e];
        const double wa = cam_w[e];
        if (sl < L.nheavy || wa == 0.0) continue;
        const double qi = q3inv[sl];
        if (qi == 0.0) continue;
        const int64_t t = sl - L.nheavy;
        if (lane < L.deg[sl]) {
            const int64_t at = L.gbase[t >> 6] + (t & 63) + (int64_t)64 * lane;
            const int64_t b = L.cam[at];
            const int64_t j = b - 1 - col0;
            if (b != 0 && j >= 0 && j < ncol) row[j] -= wa * L.w[at] * qi;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    double *out = VT + (size_t)(a - 1) * (size_t)mr + (size_t)col0;   // row a-1 of the symmetric matrix = its column a-1 (column-major)
    for (int j = lane; j < ncol; j += 64) out[j] = row[j];
}

// ------------------------------------------------------------------------------------------------------------------
// host: factors from the observation list (utils/creatematrix.py:62-175, restated on the observation level)
// ------------------------------------------------------------------------------------------------------------------
SchurOp::SchurOp(int64_t n, int64_t n_landmarks, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *p, const double *w,
                 hipStream_t st, Comm *comm, const SchurSettings &cfg) {
    cfg_ = cfg;
    comm_ = (comm && comm->active()) ? comm : nullptr;
    world_ = comm_ ? comm_->world : 1;
    rank_ = comm_ ? comm_->rank : 0;
    if (n < 1 || n_landmarks < 1 || nobs < 1 || !cam || !lm || !p || !w) throw Error(XM_ERR_ARG, "matrix-free Q: bad observation list");
    // how VT^-1 is applied: the dense inverse (fast products, 8 (N-1)^2 bytes and an O(N^3) set-up) up to cfg.dense_max cameras, above that
    // preconditioned CG inside every product (no (N-1)^2 array at all); cfg.solver forces one of the two
    pcg_ = cfg.solver == 2 || cfg.solver == 3 || (cfg.solver == 0 && n > cfg.dense_max);
    tl_ = cfg.solver == 3;
    if (pcg_ && comm_) throw Error(XM_ERR_ARG, "matrix-free Q: the CG form of the reduced camera system runs on one GPU (row-partitioned contexts use the dense inverse)");
    if (!pcg_ && n > kSchurMaxCams) throw Error(XM_ERR_ARG, "matrix-free Q: more than " + std::to_string(kSchurMaxCams) + " cameras need the CG form (xm_tuning_t.schur_solver)");
    n_ = n; m_ = n_landmarks; nobs_ = nobs;
    const int64_t N = n, M = n_landmarks;
    // ---- structure (fixed for the life of the context): observation lists by camera and by landmark, input order inside each
    // (fixed summation order); pos_*[e] = where observation e of the input sits in them (weights are re-scattered by set_weights)
    hcam_.assign(cam, cam + nobs); hlm_.assign(lm, lm + nobs); hp_.assign(p, p + 3 * nobs);
    cp_.assign((size_t)N + 1, 0); lp_.assign((size_t)M + 1, 0);
    for (int64_t e = 0; e < nobs; ++e) {
        const int64_t i = cam[e], l = lm[e];
        if (i < 0 || i >= N || l < 0 || l >= M) throw Error(XM_ERR_ARG, "matrix-free Q: observation index out of range");
        cp_[(size_t)i + 1]++; lp_[(size_t)l + 1]++;
    }
    for (int64_t i = 0; i < N; ++i) cp_[(size_t)i + 1] += cp_[(size_t)i];
    for (int64_t l = 0; l < M; ++l) lp_[(size_t)l + 1] += lp_[(size_t)l];
    // device numbering of the landmarks ("slot"): by degree, descending, stable
    std::vector<int32_t> order((size_t)M);
    for (int64_t l = 0; l < M; ++l) order[(size_t)l] = (int32_t)l;
    auto deg_of = [&](int64_t l) { return lp_[(size_t)l + 1] - lp_[(size_t)l]; };
    // ... and, among equals, by the first camera that sees them (smallest index): the landmarks of neighbouring cameras get neighbouring
    // numbers, so that a camera's gathers of landmark records (schur_cam_*, pcg_cam_kernel: one 128-byte line per 24 .. 40-byte record when
    // the numbers are scattered) fall into few lines wherever the scene has locality (sequential capture; a scene whose landmarks are seen by
    // cameras drawn at random has none to find)
    std::vector<int32_t> first_cam((size_t)M, INT32_MAX);
    for (int64_t e = 0; e < nobs; ++e) first_cam[(size_t)lm[e]] = std::min(first_cam[(size_t)lm[e]], cam[e]);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        const int64_t dx = deg_of(x), dy = deg_of(y);
        return dx != dy ? dx > dy : first_cam[(size_t)x] < first_cam[(size_t)y];
    });
    slot_of_.assign((size_t)M, 0);
    std::vector<int32_t> ldeg((size_t)M);
    nheavy_ = 0;
    for (int64_t sl = 0; sl < M; ++sl) {
        slot_of_[(size_t)order[(size_t)sl]] = (int32_t)sl;
        ldeg[(size_t)sl] = (int32_t)deg_of(order[(size_t)sl]);
        if (ldeg[(size_t)sl] > kSchurHeavy) nheavy_ = sl + 1;
    }
    std::vector<int64_t> hptr((size_t)nheavy_ + 1, 0);
    for (int64_t sl = 0; sl < nheavy_; ++sl) hptr[(size_t)sl + 1] = hptr[(size_t)sl] + ldeg[(size_t)sl];
    int64_t total = hptr[(size_t)nheavy_];
    const int64_t ngroups = (M - nheavy_ + 63) / 64;
    std::vector<int64_t> gbase((size_t)std::max<int64_t>(ngroups, 1), 0);
    for (int64_t g = 0; g < ngroups; ++g) {
        gbase[(size_t)g] = total;
        total += (int64_t)64 * ldeg[(size_t)(nheavy_ + 64 * g)];   // the group's first slot has its longest list
    }
    ltotal_ = std::max<int64_t>(total, 1);
    std::vector<int32_t> c_lm((size_t)nobs), d_lcam((size_t)ltotal_, 0), o_lm((size_t)nobs);
    std::vector<double> c_p((size_t)nobs * 3), d_lp((size_t)ltotal_ * 3, 0.0);
    lcam_.assign((size_t)nobs, 0);
    pos_c_.assign((size_t)nobs, 0); pos_l_.assign((size_t)nobs, 0); dpos_l_.assign((size_t)nobs, 0); cam_obs_.assign((size_t)nobs, 0);
    {
        // position of every observation in its camera's list: ascending landmark number (ties: input order), so that the lanes of a wavefront
        // that walk a camera's list gather neighbouring landmark records
        std::vector<int64_t> apos((size_t)nobs);
        {
            std::vector<int64_t> nc0(cp_.begin(), cp_.end() - 1), byc((size_t)nobs);
            for (int64_t e = 0; e < nobs; ++e) byc[(size_t)nc0[(size_t)cam[e]]++] = e;
            for (int64_t i = 0; i < N; ++i)
                std::stable_sort(byc.begin() + cp_[(size_t)i], byc.begin() + cp_[(size_t)i + 1],
                                 [&](int64_t x, int64_t y) { return slot_of_[(size_t)lm[x]] < slot_of_[(size_t)lm[y]]; });
            for (int64_t q = 0; q < nobs; ++q) apos[(size_t)byc[(size_t)q]] = q;
        }
        std::vector<int64_t> nl(lp_.begin(), lp_.end() - 1);
        for (int64_t e = 0; e < nobs; ++e) {
            const int64_t a2 = apos[(size_t)e], b2 = nl[(size_t)lm[e]]++;
            const int64_t sl = slot_of_[(size_t)lm[e]], k = b2 - lp_[(size_t)lm[e]];
            const int64_t d2 = (sl < nheavy_) ? hptr[(size_t)sl] + k : gbase[(size_t)((sl - nheavy_) >> 6)] + 64 * k + ((sl - nheavy_) & 63);
            pos_c_[(size_t)e] = a2; pos_l_[(size_t)e] = b2; dpos_l_[(size_t)e] = d2;
            cam_obs_[(size_t)a2] = e;
            c_lm[(size_t)a2] = (int32_t)sl; o_lm[(size_t)e] = (int32_t)sl;
            for (int a = 0; a < 3; ++a) c_p[(size_t)a * (size_t)nobs + (size_t)a2] = p[3 * e + a];   // three planes
            lcam_[(size_t)b2] = cam[e];                           // host copy (by landmark, contiguous): assembly of VT
            d_lcam[(size_t)d2] = cam[e];
            for (int a = 0; a < 3; ++a) d_lp[(size_t)a * (size_t)ltotal_ + (size_t)d2] = p[3 * e + a];
        }
    }
    auto up = [&](auto &buf, const auto &v) {
        buf.alloc(std::max<size_t>(v.size(), 1), false);
        if (!v.empty()) XM_HIP_CHECK(hipMemcpy(buf.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
    };
    up(cam_ptr_, cp_); up(lm_ptr_, hptr); up(gbase_, gbase); up(ldeg_, ldeg); up(cam_lm_, c_lm); up(lm_cam_, d_lcam); up(cam_p_, c_p); up(lm_p_, d_lp);
    up(obs_cam_, hcam_); up(obs_lm_, o_lm); up(obs_p_, hp_);
    up(pos_c_dev_, pos_c_); up(dpos_l_dev_, dpos_l_);
    w_in_.alloc((size_t)nobs, false); q2_.alloc((size_t)N, false);
    {   // a (camera, landmark) pair named twice would put two lanes of the device assembly on one entry of VT: such a list keeps the host path
        std::vector<int64_t> seen((size_t)N, -1);
        dup_pairs_ = false;
        for (int64_t l = 0; l < M && !dup_pairs_; ++l)
            for (int64_t e2 = lp_[(size_t)l]; e2 < lp_[(size_t)l + 1]; ++e2) {
                const int64_t b = lcam_[(size_t)e2];
                if (seen[(size_t)b] == l) { dup_pairs_ = true; break; }
                seen[(size_t)b] = l;
            }
        has_dup_ = dup_pairs_;
        if (cfg_.host_assembly) dup_pairs_ = true;
    }
    hub_lm_.clear(); hub_obs_ptr_.assign(1, 0); hub_obs_.clear();   // heavy landmarks: their observations (input indices), for the rank-1 terms
    {
        std::vector<std::vector<int64_t>> by((size_t)nheavy_);
        for (int64_t e = 0; e < nobs; ++e) {
            const int64_t sl = slot_of_[(size_t)lm[e]];
            if (sl < nheavy_) by[(size_t)sl].push_back(e);
        }
        for (int64_t sl = 0; sl < nheavy_; ++sl) {
            hub_lm_.push_back(sl);
            hub_obs_.insert(hub_obs_.end(), by[(size_t)sl].begin(), by[(size_t)sl].end());
            hub_obs_ptr_.push_back((int64_t)hub_obs_.size());
        }
    }
    cam_w_.alloc((size_t)nobs, false); lm_w_.alloc((size_t)ltotal_, false);
    Q1_.alloc((size_t)N * 9, false); c_.alloc((size_t)N * 3, false); q3inv_.alloc((size_t)M, false);
    const int64_t mr = N - 1;
    nred_ = std::max<int64_t>(1, (mr + 2) / 3);
    ldv_ = dense_ld(nred_);
    // several ranks: the rows of VT^-1 are dealt out in equal ranges of pseudo-cameras (3 rows each); every rank keeps the whole inverse
    // (the set-up is replicated) but multiplies only its own rows, and the ranks all-gather x_cam
    nred_loc_ = (nred_ + world_ - 1) / world_;
    nred_pad_ = nred_loc_ * world_;
    if (pcg_) {
        dup_pairs_ = false;   // (the host assembly exists for VT; a pair named twice only makes the Jacobi diagonal approximate)
        if (cfg_.pcg_first > 0) pcg_last_iters_[0] = pcg_last_iters_[1] = std::max(1, cfg_.pcg_first - 2);
        if (cfg_.pcg_hess_digits > 0) pcg_tol_[1] = std::pow(10.0, -(double)std::min(13, std::max(6, cfg_.pcg_hess_digits)));
        pcg_dinv_.alloc((size_t)std::max<int64_t>(mr, 1));
        XM_HIP_CHECK(hipHostMalloc((void **)&pcg_host_, sizeof(PcgState), hipHostMallocDefault));
        pcg_state_.alloc(sizeof(PcgState) / sizeof(int32_t) + 2);
        if (tl_ && mr > 0) two_level_build(nobs, cam, lm);
    } else {
        vtinv_.alloc((size_t)3 * nred_pad_ * (size_t)ldv_);
    }
    set_weights(w, st);
}

SchurOp::~SchurOp() {
    if (pcg_host_) (void)hipHostFree(pcg_host_);
}

// Everything that depends on the weights (utils/creatematrix.py:62-175 restated on the observation level): Q1, c (= V1), Q3, the
// reduced camera Laplacian VT = Q2_bar - V3_bar Q3^{-1} V3_bar^T and its inverse.  Called by the constructor and by the XM^2 loop
// (observations filtered by weight 0).  A landmark whose observations all have weight 0 drops out (1/Q3 := 0); a camera without
// weight makes VT singular -> XM_ERR_ARG.
void SchurOp::set_weights(const double *w, hipStream_t st) {
    if (!w) throw Error(XM_ERR_ARG, "matrix-free Q: null weights");
    if (!dup_pairs_) { set_weights_device(w, st); return; }
    const int64_t N = n_, M = m_, nobs = nobs_;
    const bool trace = cfg_.trace;   // set-up phase times on stderr
    auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "schur set-up: %-28s %8.1f ms\n", what, std::chrono::duration<double>(now - tp).count() * 1e3);
        tp = now;
    };
    std::vector<double> Q1((size_t)N * 9, 0.0), c((size_t)N * 3, 0.0), Q2((size_t)N, 0.0), Q3((size_t)M, 0.0);
    std::vector<double> c_w((size_t)nobs), l_w((size_t)nobs), d_lw((size_t)ltotal_, 0.0);
    for (int64_t e = 0; e < nobs; ++e) {
        if (!(w[e] >= 0.0)) throw Error(XM_ERR_ARG, "matrix-free Q: negative or NaN weight");
        const int64_t i = hcam_[(size_t)e], l = hlm_[(size_t)e];
        const double *pe = &hp_[(size_t)e * 3];
        for (int a = 0; a < 3; ++a) {
            c[(size_t)i * 3 + a] += w[e] * pe[a];                                                 // V1 block (creatematrix.py:27)
            for (int b = 0; b < 3; ++b) Q1[(size_t)i * 9 + 3 * a + b] += w[e] * pe[a] * pe[b];    // Q1 block (:26)
        }
        Q2[(size_t)i] += w[e]; Q3[(size_t)l] += w[e];                                             // :68-69
        c_w[(size_t)pos_c_[(size_t)e]] = w[e]; l_w[(size_t)pos_l_[(size_t)e]] = w[e]; d_lw[(size_t)dpos_l_[(size_t)e]] = w[e];
    }
    lap("Q1, c, Q2, Q3 (host)");
    std::vector<double> q3inv((size_t)M), q3inv_slot((size_t)M);   // by landmark (host: VT) and by slot (device)
    for (int64_t l = 0; l < M; ++l) {
        q3inv[(size_t)l] = (Q3[(size_t)l] > 0.0) ? 1.0 / Q3[(size_t)l] : 0.0;
        q3inv_slot[(size_t)slot_of_[(size_t)l]] = q3inv[(size_t)l];
    }
    const int64_t mr = N - 1;
    std::vector<double> VT((size_t)std::max<int64_t>(mr, 1) * (size_t)std::max<int64_t>(mr, 1), 0.0);
    for (int64_t i = 1; i < N; ++i) VT[(size_t)(i - 1) + (size_t)(i - 1) * mr] = Q2[(size_t)i];
    // VT is assembled ROW BY ROW (camera a: its observations in list order, for each the cameras of that landmark): a row of N-1
    // doubles stays in the cache while its ~deg(a) * deg(l) updates land, rows are independent (threads own row ranges; the order of
    // the additions into an entry is the camera's observation order whatever the thread count), and the matrix is symmetric, so the
    // row-major image is the column-major one.  By landmark instead, the same 51 M updates at 13 682 cameras scatter over 1.5 GB: 1.7 s
    // against 0.1 s.  Landmarks with more than kSchurHeavy observations are full rank-1 terms and are applied on the device below.
    std::vector<int64_t> hubs;
    for (int64_t l = 0; l < M; ++l)
        if (q3inv[(size_t)l] != 0.0 && lp_[(size_t)l + 1] - lp_[(size_t)l] > kSchurHeavy && mr > 0) hubs.push_back(l);
    if (mr > 0) {
        auto rows = [&](int64_t a0, int64_t a1) {
            for (int64_t a = std::max<int64_t>(a0, 1); a < a1; ++a) {
                double *row = VT.data() + (size_t)(a - 1) * (size_t)mr;
                for (int64_t pc = cp_[(size_t)a]; pc < cp_[(size_t)a + 1]; ++pc) {
                    const int64_t e = cam_obs_[(size_t)pc], l = hlm_[(size_t)e];
                    const double qi = q3inv[(size_t)l], wa = w[e];
                    if (qi == 0.0 || wa == 0.0 || lp_[(size_t)l + 1] - lp_[(size_t)l] > kSchurHeavy) continue;
                    for (int64_t e2 = lp_[(size_t)l]; e2 < lp_[(size_t)l + 1]; ++e2) {
                        const int64_t b = lcam_[(size_t)e2];
                        if (b != 0) row[b - 1] -= wa * l_w[(size_t)e2] * qi;
                    }
                }
            }
        };
        const int nthr = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, (int64_t)std::thread::hardware_concurrency()), N / 256));
        if (nthr <= 1) rows(1, N);
        else {
            std::vector<std::thread> pool;
            for (int t = 0; t < nthr; ++t) pool.emplace_back(rows, N * t / nthr, N * (t + 1) / nthr);
            for (auto &th : pool) th.join();
        }
    }
    lap("VT rows (host threads)");
    auto put = [&](DevBuf<double> &buf, const std::vector<double> &v) {
        if (!v.empty()) XM_HIP_CHECK(hipMemcpy(buf.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    };
    put(cam_w_, c_w); put(lm_w_, d_lw); put(Q1_, Q1); put(c_, c); put(q2_, Q2); put(q3inv_, q3inv_slot);
    if (mr > 0) {   // invert on the device (blocked Cholesky, xm_dense_la.hip), then lay the inverse out like a dense Q
        DevBuf<double> tmp, inv;
        tmp.alloc((size_t)mr * mr, false); inv.alloc((size_t)mr * mr, false);
        XM_HIP_CHECK(hipMemcpy(tmp.p, VT.data(), (size_t)mr * mr * sizeof(double), hipMemcpyHostToDevice));
        std::vector<double>().swap(VT);
        lap("VT to the device");
        if (!hubs.empty()) {
            DevBuf<double> du;
            du.alloc((size_t)mr, false);
            std::vector<double> u((size_t)mr);
            for (int64_t l : hubs) {   // in landmark order (fixed): VT -= (1/Q3_l) u u^T, u = the weights of l's observations by camera
                std::fill(u.begin(), u.end(), 0.0);
                for (int64_t e1 = lp_[(size_t)l]; e1 < lp_[(size_t)l + 1]; ++e1)
                    if (lcam_[(size_t)e1] != 0) u[(size_t)lcam_[(size_t)e1] - 1] += l_w[(size_t)e1];
                XM_HIP_CHECK(hipMemcpyAsync(du.p, u.data(), (size_t)mr * sizeof(double), hipMemcpyHostToDevice, st));
                rank1_sub_device((int)mr, tmp.p, du.p, q3inv[(size_t)l], st);
                XM_HIP_CHECK(hipStreamSynchronize(st));   // u is reused
            }
        }
        XM_HIP_CHECK(hipStreamSynchronize(st));
        lap("hub rank-1 terms (device)");
        if (!spd_inverse_device((int)mr, tmp.p, inv.p, st, cfg_.trace))
            throw Error(XM_ERR_ARG, "matrix-free Q: the reduced camera Laplacian is not positive definite (observation graph not connected?)");
        lap("SPD inverse (device)");
        spd_inverse_layout((int)mr, inv.p, vtinv_.p, ldv_, st);
        XM_HIP_CHECK(hipStreamSynchronize(st));
        lap("layout of the inverse");
    }
}

// The same on the device: weights uploaded once, per-camera / per-landmark sums, the reduced camera Laplacian row by row in LDS (the host
// needed 0.2 + 0.3 s for them at 13 682 cameras and 0.18 s to ship the 1.5 GB matrix), hub landmarks as rank-1 terms, inverse, layout.
void SchurOp::set_weights_device(const double *w, hipStream_t st) {
    const int64_t N = n_, M = m_, nobs = nobs_;
    const bool trace = cfg_.trace;
    auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!trace) return;
        XM_HIP_CHECK(hipStreamSynchronize(st));
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "schur set-up: %-28s %8.1f ms\n", what, std::chrono::duration<double>(now - tp).count() * 1e3);
        tp = now;
    };
    for (int64_t e = 0; e < nobs; ++e)
        if (!(w[e] >= 0.0)) throw Error(XM_ERR_ARG, "matrix-free Q: negative or NaN weight");
    XM_HIP_CHECK(hipMemcpyAsync(w_in_.p, w, (size_t)nobs * sizeof(double), hipMemcpyHostToDevice, st));
    XM_HIP_CHECK(hipMemsetAsync(lm_w_.p, 0, (size_t)ltotal_ * sizeof(double), st));   // the padding entries of the packed landmark lists
    hipLaunchKernelGGL(schur_scatter_w_kernel, dim3((unsigned)((nobs + 255) / 256)), dim3(256), 0, st, nobs, w_in_.p, pos_c_dev_.p, dpos_l_dev_.p,
                       cam_w_.p, lm_w_.p);
    hipLaunchKernelGGL(schur_cam_sums_kernel, dim3((unsigned)((N + kQwWaves - 1) / kQwWaves)), dim3(256), 0, st, N, nobs, cam_ptr_.p, cam_w_.p, cam_p_.p,
                       Q1_.p, c_.p, q2_.p);
    const SchurLm L = lm_lists();
    const int64_t nlight = M - nheavy_;
    hipLaunchKernelGGL(schur_lm_q3_kernel, dim3((unsigned)(nheavy_ + (nlight + kSchurHeavyThreads - 1) / kSchurHeavyThreads)), dim3(kSchurHeavyThreads), 0, st, L,
                       q3inv_.p);
    check_launch("schur set-up (sums)");
    lap("weights, Q1, c, Q2, 1/Q3 (device)");
    const int64_t mr = N - 1;
    if (mr <= 0) { XM_HIP_CHECK(hipStreamSynchronize(st)); return; }
    if (pcg_) {   // no VT, no inverse: the Jacobi diagonal is all the CG form needs
        hipLaunchKernelGGL(pcg_diag_kernel, dim3((unsigned)((N + kQwWaves - 1) / kQwWaves)), dim3(256), 0, st, (int)N, cam_ptr_.p, cam_lm_.p, cam_w_.p,
                           q3inv_.p, q2_.p, pcg_dinv_.p);
        check_launch("schur set-up (Jacobi diagonal)");
        std::vector<double> hd((size_t)mr);
        XM_HIP_CHECK(hipMemcpyAsync(hd.data(), pcg_dinv_.p, (size_t)mr * sizeof(double), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipStreamSynchronize(st));
        for (double d : hd)
            if (!(d > 0.0) || !std::isfinite(d)) throw Error(XM_ERR_ARG, "matrix-free Q: a camera has no weight on the reduced camera Laplacian's diagonal (camera without observations?)");
        lap("Jacobi diagonal (device)");
        if (tl_) {
            two_level_set_weights(w, st);
            lap("two-level preconditioner (device)");
        }
        return;
    }
    DevBuf<double> tmp, inv;
    tmp.alloc((size_t)mr * mr, false); inv.alloc((size_t)mr * mr, false);
    constexpr int64_t kColsPerPass = 16384;   // 128 KB of LDS per wavefront (one workgroup per CU; gfx950 has 160 KB)
    {
        static const bool once = [] {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(schur_vt_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)(kColsPerPass * sizeof(double)));
            (void)hipGetLastError();
            return e == hipSuccess;
        }();
        (void)once;
    }
    for (int64_t col0 = 0; col0 < mr; col0 += kColsPerPass) {
        const int ncol = (int)std::min<int64_t>(kColsPerPass, mr - col0);
        hipLaunchKernelGGL(schur_vt_rows_kernel, dim3((unsigned)mr), dim3(64), (size_t)ncol * sizeof(double), st, mr, col0, ncol, cam_ptr_.p, cam_lm_.p,
                           cam_w_.p, L, q3inv_.p, q2_.p, tmp.p);
    }
    check_launch("schur set-up (VT rows)");
    lap("VT rows (device)");
    if (nheavy_ > 0) {   // hub landmarks in slot order (fixed): VT -= (1/Q3_l) u u^T, u = the weights of l's observations by camera
        std::vector<double> q3h((size_t)nheavy_);
        XM_HIP_CHECK(hipMemcpyAsync(q3h.data(), q3inv_.p, (size_t)nheavy_ * sizeof(double), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipStreamSynchronize(st));
        DevBuf<double> du;
        du.alloc((size_t)mr, false);
        std::vector<double> u((size_t)mr);
        for (int64_t h = 0; h < nheavy_; ++h) {
            if (q3h[(size_t)h] == 0.0) continue;
            std::fill(u.begin(), u.end(), 0.0);
            for (int64_t k = hub_obs_ptr_[(size_t)h]; k < hub_obs_ptr_[(size_t)h + 1]; ++k) {
                const int64_t e = hub_obs_[(size_t)k];
                if (hcam_[(size_t)e] != 0) u[(size_t)hcam_[(size_t)e] - 1] += w[e];
            }
            XM_HIP_CHECK(hipMemcpyAsync(du.p, u.data(), (size_t)mr * sizeof(double), hipMemcpyHostToDevice, st));
            rank1_sub_device((int)mr, tmp.p, du.p, q3h[(size_t)h], st);
            XM_HIP_CHECK(hipStreamSynchronize(st));   // u is reused
        }
    }
    lap("hub rank-1 terms (device)");
    if (!spd_inverse_device((int)mr, tmp.p, inv.p, st, cfg_.trace))
        throw Error(XM_ERR_ARG, "matrix-free Q: the reduced camera Laplacian is not positive definite (observation graph not connected?)");
    lap("SPD inverse (device)");
    spd_inverse_layout((int)mr, inv.p, vtinv_.p, ldv_, st);
    XM_HIP_CHECK(hipStreamSynchronize(st));
    lap("layout of the inverse");
}

// ------------------------------------------------------------------------------------------------------------------
// host: the two-level preconditioner's structure (once per context) and its weight-dependent parts (every set_weights)
// ------------------------------------------------------------------------------------------------------------------
void schur_aggregate_plan(int64_t n, int64_t nobs, const int32_t *cam, const int32_t *lm, int B, std::vector<int32_t> &order) {
    if (n < 2 || nobs < 1 || !cam || !lm) throw Error(XM_ERR_ARG, "aggregate plan: needs at least 2 cameras and 1 observation");
    if (B < 1 || B > kSchurAggCams) throw Error(XM_ERR_ARG, "aggregate plan: cameras per aggregate must be 1.." + std::to_string(kSchurAggCams));
    const int64_t nagg = (n - 1 + B - 1) / B;
    if (nagg > kSchurMaxAggregates)
        throw Error(XM_ERR_ARG, "two-level preconditioner: " + std::to_string(n - 1) + " cameras make " + std::to_string(nagg) + " aggregates of " +
                                std::to_string(B) + ", more than the coarse operator's limit of " + std::to_string(kSchurMaxAggregates) +
                                " (use xm_tuning_t.schur_solver = 2)");
    int64_t M = 0;
    for (int64_t e = 0; e < nobs; ++e) {
        if (cam[e] < 0 || cam[e] >= n || lm[e] < 0) throw Error(XM_ERR_ARG, "aggregate plan: observation index out of range");
        M = std::max<int64_t>(M, (int64_t)lm[e] + 1);
    }
    // the bipartite graph as two lists in input order (fixed visiting order)
    std::vector<int64_t> cptr((size_t)n + 1, 0), lptr((size_t)M + 1, 0);
    for (int64_t e = 0; e < nobs; ++e) { cptr[(size_t)cam[e] + 1]++; lptr[(size_t)lm[e] + 1]++; }
    for (int64_t i = 0; i < n; ++i) cptr[(size_t)i + 1] += cptr[(size_t)i];
    for (int64_t l = 0; l < M; ++l) lptr[(size_t)l + 1] += lptr[(size_t)l];
    std::vector<int32_t> c_l((size_t)nobs), l_c((size_t)nobs);
    {
        std::vector<int64_t> nc(cptr.begin(), cptr.end() - 1), nl(lptr.begin(), lptr.end() - 1);
        for (int64_t e = 0; e < nobs; ++e) { c_l[(size_t)nc[(size_t)cam[e]]++] = lm[e]; l_c[(size_t)nl[(size_t)lm[e]]++] = cam[e]; }
    }
    std::vector<char> cseen((size_t)n, 0), lseen((size_t)M, 0);
    std::vector<int32_t> queue;
    queue.reserve((size_t)n);
    queue.push_back(0); cseen[0] = 1;
    for (size_t h = 0; h < queue.size(); ++h) {
        const int32_t c = queue[h];
        for (int64_t q = cptr[(size_t)c]; q < cptr[(size_t)c + 1]; ++q) {
            const int32_t l = c_l[(size_t)q];
            if (lseen[(size_t)l] || lptr[(size_t)l + 1] - lptr[(size_t)l] > kSchurHeavy) continue;   // heavy landmarks carry no locality
            lseen[(size_t)l] = 1;
            for (int64_t q2 = lptr[(size_t)l]; q2 < lptr[(size_t)l + 1]; ++q2) {
                const int32_t c2 = l_c[(size_t)q2];
                if (!cseen[(size_t)c2]) { cseen[(size_t)c2] = 1; queue.push_back(c2); }
            }
        }
    }
    order.assign(queue.begin() + 1, queue.end());
    for (int64_t i = 1; i < n; ++i)
        if (!cseen[(size_t)i]) order.push_back((int32_t)i);
}

void SchurOp::two_level_build(int64_t nobs, const int32_t *cam, const int32_t *lm) {
    constexpr int B = kSchurAggCams;
    std::vector<int32_t> order;
    schur_aggregate_plan(n_, nobs, cam, lm, B, order);
    const int64_t nagg = (n_ - 1 + B - 1) / B;
    tl_nagg_ = nagg;
    std::vector<int32_t> perm((size_t)nagg * B, -1), loc((size_t)n_, -1);
    tl_agg_of_.assign((size_t)n_, -1);
    for (size_t k = 0; k < order.size(); ++k) {
        perm[k] = order[k] - 1;
        tl_agg_of_[(size_t)order[k]] = (int32_t)(k / B);
        loc[(size_t)order[k]] = (int32_t)(k % B);
    }
    // groups: the observations of cameras >= 1 by (aggregate, landmark slot, input order)
    std::vector<int64_t> aptr((size_t)nagg + 1, 0);
    for (int64_t e = 0; e < nobs; ++e)
        if (cam[e] != 0) aptr[(size_t)tl_agg_of_[(size_t)cam[e]] + 1]++;
    for (int64_t a = 0; a < nagg; ++a) aptr[(size_t)a + 1] += aptr[(size_t)a];
    std::vector<int64_t> obs((size_t)aptr[(size_t)nagg]);
    {
        std::vector<int64_t> na(aptr.begin(), aptr.end() - 1);
        for (int64_t e = 0; e < nobs; ++e)
            if (cam[e] != 0) obs[(size_t)na[(size_t)tl_agg_of_[(size_t)cam[e]]]++] = e;
    }
    for (int64_t a = 0; a < nagg; ++a)
        std::stable_sort(obs.begin() + aptr[(size_t)a], obs.begin() + aptr[(size_t)a + 1],
                         [&](int64_t x, int64_t y) { return slot_of_[(size_t)lm[x]] < slot_of_[(size_t)lm[y]]; });
    std::vector<int64_t> gptr((size_t)nagg + 1, 0), eptr(1, 0);
    std::vector<int32_t> gslot, gagg, eloc((size_t)obs.size());
    for (int64_t a = 0; a < nagg; ++a) {
        for (int64_t q = aptr[(size_t)a]; q < aptr[(size_t)a + 1]; ++q) {
            const int32_t sl = slot_of_[(size_t)lm[obs[(size_t)q]]];
            if (q == aptr[(size_t)a] || sl != gslot.back()) {
                if (q != aptr[(size_t)a]) eptr.push_back(q);
                gslot.push_back(sl); gagg.push_back((int32_t)a);
            }
            eloc[(size_t)q] = loc[(size_t)cam[obs[(size_t)q]]];
        }
        if (aptr[(size_t)a + 1] > aptr[(size_t)a]) eptr.push_back(aptr[(size_t)a + 1]);
        gptr[(size_t)a + 1] = (int64_t)gslot.size();
    }
    const int64_t ng = (int64_t)gslot.size();
    tl_ngroups_ = ng;
    // coarse entries (a, b), a >= b, with their group pairs: light landmarks in slot order (the groups of one landmark are in aggregate order);
    // every diagonal entry exists.  A heavy landmark (more than kSchurHeavy observations) would add up to n_c^2 pairs: a rank-1 term instead.
    std::vector<int64_t> sptr((size_t)m_ + 1, 0);
    for (int64_t g = 0; g < ng; ++g) sptr[(size_t)gslot[(size_t)g] + 1]++;
    for (int64_t sl = 0; sl < m_; ++sl) sptr[(size_t)sl + 1] += sptr[(size_t)sl];
    std::vector<int32_t> by_slot((size_t)ng);
    {
        std::vector<int64_t> ns(sptr.begin(), sptr.end() - 1);
        for (int64_t g = 0; g < ng; ++g) by_slot[(size_t)ns[(size_t)gslot[(size_t)g]]++] = (int32_t)g;
    }
    struct Pair { int64_t key; int32_t g1, g2; };
    std::vector<Pair> pairs;
    for (int64_t a = 0; a < nagg; ++a) pairs.push_back({a * nagg + a, -1, -1});
    for (int64_t sl = nheavy_; sl < m_; ++sl)
        for (int64_t x = sptr[(size_t)sl]; x < sptr[(size_t)sl + 1]; ++x)
            for (int64_t y = sptr[(size_t)sl]; y <= x; ++y) {
                const int32_t g1 = by_slot[(size_t)x], g2 = by_slot[(size_t)y];
                pairs.push_back({(int64_t)gagg[(size_t)g1] * nagg + gagg[(size_t)g2], g1, g2});
            }
    std::stable_sort(pairs.begin(), pairs.end(), [](const Pair &x, const Pair &y) { return x.key < y.key; });
    std::vector<int64_t> cptr(1, 0);
    std::vector<int32_t> cab, cpair;
    for (size_t q = 0; q < pairs.size(); ++q) {
        if (q == 0 || pairs[q].key != pairs[q - 1].key) {
            if (q != 0) cptr.push_back((int64_t)cpair.size() / 2);
            cab.push_back((int32_t)(pairs[q].key / nagg)); cab.push_back((int32_t)(pairs[q].key % nagg));
        }
        if (pairs[q].g1 >= 0) { cpair.push_back(pairs[q].g1); cpair.push_back(pairs[q].g2); }
    }
    cptr.push_back((int64_t)cpair.size() / 2);
    tl_nentries_ = (int64_t)cab.size() / 2;
    auto up = [&](auto &buf, const auto &v) {
        buf.alloc(std::max<size_t>(v.size(), 1), false);
        if (!v.empty()) XM_HIP_CHECK(hipMemcpy(buf.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
    };
    up(tl_perm_, perm); up(tl_gptr_, gptr); up(tl_gslot_, gslot); up(tl_eptr_, eptr); up(tl_eloc_, eloc); up(tl_eobs_, obs);
    up(tl_cptr_, cptr); up(tl_cab_, cab); up(tl_cpair_, cpair);
    tl_u_.alloc((size_t)std::max<int64_t>(ng, 1), false);
    tl_binv_.alloc((size_t)nagg * B * B, false);
    tl_ainv_.alloc((size_t)nagg * nagg, false);
    tl_fail_.alloc(1);
}

// the blocks VT_aa^-1 and A_c^-1 from the current weights (w_in_ / q2_ / q3inv_ already on the device: set_weights_device)
void SchurOp::two_level_set_weights(const double *w, hipStream_t st) {
    const int64_t nagg = tl_nagg_;
    hipLaunchKernelGGL(tl_group_sum_kernel, dim3((unsigned)std::max<int64_t>(1, (tl_ngroups_ + 255) / 256)), dim3(256), 0, st, tl_ngroups_, tl_eptr_.p, tl_eobs_.p,
                       w_in_.p, tl_u_.p);
    XM_HIP_CHECK(hipMemsetAsync(tl_fail_.p, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(tl_block_inverse_kernel, dim3((unsigned)nagg), dim3(kSchurAggCams), 0, st, tl_perm_.p, tl_gptr_.p, tl_gslot_.p, tl_eptr_.p,
                       tl_eloc_.p, tl_eobs_.p, w_in_.p, q3inv_.p, q2_.p, tl_binv_.p, tl_fail_.p);
    DevBuf<double> A, X;
    A.alloc((size_t)nagg * nagg, false); X.alloc((size_t)nagg * nagg, false);
    XM_HIP_CHECK(hipMemsetAsync(A.p, 0, (size_t)nagg * nagg * sizeof(double), st));
    hipLaunchKernelGGL(tl_coarse_entries_kernel, dim3((unsigned)((tl_nentries_ + 255) / 256)), dim3(256), 0, st, tl_nentries_, tl_cptr_.p, tl_cab_.p,
                       tl_cpair_.p, tl_gslot_.p, tl_u_.p, q3inv_.p, tl_perm_.p, q2_.p, nagg, A.p);
    check_launch("schur set-up (two-level preconditioner)");
    int32_t fail = 0;
    XM_HIP_CHECK(hipMemcpyAsync(&fail, tl_fail_.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipStreamSynchronize(st));
    if (fail) throw Error(XM_ERR_ARG, "matrix-free Q: the reduced camera Laplacian is not positive definite (observation graph not connected?): a block of the two-level preconditioner");
    if (nheavy_ > 0) {   // heavy landmarks in slot order (fixed): A_c -= (1/Q3_l) U U^T, U = the weights of l's observations by aggregate
        std::vector<double> q3h((size_t)nheavy_);
        XM_HIP_CHECK(hipMemcpyAsync(q3h.data(), q3inv_.p, (size_t)nheavy_ * sizeof(double), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipStreamSynchronize(st));
        DevBuf<double> du;
        du.alloc((size_t)nagg, false);
        std::vector<double> u((size_t)nagg);
        for (int64_t h = 0; h < nheavy_; ++h) {
            if (q3h[(size_t)h] == 0.0) continue;
            std::fill(u.begin(), u.end(), 0.0);
            for (int64_t k = hub_obs_ptr_[(size_t)h]; k < hub_obs_ptr_[(size_t)h + 1]; ++k) {
                const int64_t e = hub_obs_[(size_t)k];
                if (hcam_[(size_t)e] != 0) u[(size_t)tl_agg_of_[(size_t)hcam_[(size_t)e]]] += w[e];
            }
            XM_HIP_CHECK(hipMemcpyAsync(du.p, u.data(), (size_t)nagg * sizeof(double), hipMemcpyHostToDevice, st));
            rank1_sub_device((int)nagg, A.p, du.p, q3h[(size_t)h], st);
            XM_HIP_CHECK(hipStreamSynchronize(st));   // u is reused
        }
    }
    if (!spd_inverse_device((int)nagg, A.p, X.p, st))
        throw Error(XM_ERR_ARG, "matrix-free Q: the reduced camera Laplacian is not positive definite (observation graph not connected?): the coarse operator of the two-level preconditioner");
    spd_inverse_layout((int)nagg, X.p, tl_ainv_.p, nagg, st);
    XM_HIP_CHECK(hipStreamSynchronize(st));
}

// residual of every observation at the point whose scaled rows are U (camera records of 3 * pitch_of(o) doubles):
// |p^T U_i + t_i - P_l|^2 with the eliminated translations / landmarks [t; P] = -Qtp_bar^{-1} Vtp_bar^T U, i.e. the observation's share
// of <Q, U U^T> per unit weight (what the reference's XM^2 loop computes from recover_XM's p_est / t_est, 3_test_colmap_glomap.py:305-316)
template <int O>
__global__ __launch_bounds__(256) void schur_obs_residual_kernel(int64_t nobs, const int32_t *__restrict__ cam, const int32_t *__restrict__ lm,
                                                                  const double *__restrict__ p, const double *__restrict__ U,
                                                                  const double *__restrict__ xc, const double *__restrict__ xl,
                                                                  double *__restrict__ res) {
    constexpr int OP = pitch_of(O);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nobs) return;
    const int i = cam[e];
    const double *Ui = U + (size_t)i * 3 * OP, *x = xl + (size_t)lm[e] * OP;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < O; ++k) {
        const double xk = (i >= 1) ? xc[(size_t)(i - 1) * OP + k] : 0.0;
        const double d = p[3 * e] * Ui[k] + p[3 * e + 1] * Ui[OP + k] + p[3 * e + 2] * Ui[2 * OP + k] - xk + x[k];
        acc += d * d;
    }
    res[e] = acc;
}

const double *SchurOp::residuals_device(int o, const double *U, const CamArgs &a, hipStream_t st) {
    // the chain with the plain epilogue leaves x_cam / x_l of this U in the scratch buffers
    product(o, EPI_PLAIN, U, 1.0, a, st);
    if (res_.count < (size_t)nobs_) res_.alloc((size_t)nobs_, false);
    XM_DISPATCH_O(o, hipLaunchKernelGGL((schur_obs_residual_kernel<O_>), dim3((unsigned)((nobs_ + 255) / 256)), dim3(256), 0, st, nobs_, obs_cam_.p,
                                        obs_lm_.p, obs_p_.p, U, xc_.p, xl_.p, res_.p));
    check_launch("schur_obs_residual");
    return res_.p;
}
void SchurOp::residuals(int o, const double *U, double *res_host, const CamArgs &a, hipStream_t st) {
    const double *r = residuals_device(o, U, a, st);
    XM_HIP_CHECK(hipMemcpyAsync(res_host, r, (size_t)nobs_ * sizeof(double), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipStreamSynchronize(st));
}

// ybar_est = Abar @ sR_real^T of utils/recoversolution.py:77-86 without Abar (the dense (N-1+M) x 3N matrix of creatematrix.py:283-311):
// Abar = -Qtp_bar^-1 Vtp_bar^T, and the first four steps of the product chain at W = (sR_real)^T leave exactly Qtp_bar^-1 Vtp_bar^T W
// in x_cam (cameras 1..N-1) and x_l (landmarks).
void SchurOp::recover_tp(const double *rot, const double *scale, double *t, double *p, hipStream_t st) {
    if (!rot || !scale || !t || !p) throw Error(XM_ERR_ARG, "recover_tp: null argument");
    constexpr int OP = pitch_of(3);
    std::vector<double> hW((size_t)(n_ + kColPad) * 3 * OP, 0.0);
    for (int64_t i = 0; i < n_; ++i)
        for (int a = 0; a < 3; ++a)
            for (int k = 0; k < 3; ++k) hW[((size_t)i * 3 + a) * OP + k] = scale[i] * rot[(size_t)k + 3 * ((size_t)3 * i + a)];
    DevBuf<double> dW, dY;
    dW.alloc(hW.size(), false); dY.alloc((size_t)n_ * 3 * OP + 2);
    XM_HIP_CHECK(hipMemcpyAsync(dW.p, hW.data(), hW.size() * sizeof(double), hipMemcpyHostToDevice, st));
    CamArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nloc = (int)n_; a.out = dY.p;
    product(3, EPI_PLAIN, dW.p, 1.0, a, st);
    std::vector<double> hx((size_t)std::max<int64_t>(n_ - 1, 0) * OP), hl((size_t)m_ * OP);
    if (!hx.empty()) XM_HIP_CHECK(hipMemcpyAsync(hx.data(), xc_.p, hx.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(hl.data(), xl_.p, hl.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipStreamSynchronize(st));
    for (int k = 0; k < 3; ++k) t[k] = 0.0;                                   // the anchor
    for (int64_t i = 1; i < n_; ++i)
        for (int k = 0; k < 3; ++k) t[(size_t)3 * i + k] = -hx[(size_t)(i - 1) * OP + k];
    for (int64_t l = 0; l < m_; ++l)
        for (int k = 0; k < 3; ++k) p[(size_t)3 * l + k] = -hl[(size_t)slot_of_[(size_t)l] * OP + k];
}

void SchurOp::ensure(int o) {
    if (o <= o_alloc_) return;
    const size_t OP = (size_t)pitch_of(o);
    h_.alloc((size_t)m_ * OP); xl_.alloc((size_t)m_ * OP);
    r_.alloc((size_t)ldv_ * OP + 2);            // product input of the dense kernel: ldv rows, zero beyond N-1
    xc_.alloc((size_t)3 * nred_pad_ * OP + 2);
    if (pcg_) {
        const size_t v = (size_t)std::max<int64_t>(n_ - 1, 1) * OP + 2;
        pcg_r_.alloc(v); pcg_p_.alloc(v); pcg_ap_.alloc(v);
        pcg_grid_ = flat_grid(std::max<int64_t>(n_ - 1, 1));
        pcg_parts_.alloc(((size_t)4 * pcg_grid_ + (size_t)qw_grid((int)n_)) * (size_t)o + 16);
        if (tl_) { tl_z_.alloc(v); tl_g_.alloc((size_t)std::max<int64_t>(tl_nagg_, 1) * o + 2); }
    }
    // VT^-1 is symmetric: from xm_tuning_t.sym_min_rows rows on (default 4096, the measured threshold of the dense solver) the chain applies it
    // with the half-traffic kernel (upper triangle only; o = 3, 4)
    vt_sym_ = !pcg_ && 3 * nred_ >= cfg_.sym_min_rows;
    if (vt_sym_ && o >= 3) sym_work_.ensure((int)nred_, ldv_, std::min(o, 4));
    o_alloc_ = o;
}

int64_t SchurOp::bytes_per_product(int o) const {
    // observation arrays are streamed twice by camera (w, landmark index; w, p, landmark index) and twice by landmark, VT^{-1} once
    // CG form: every iteration streams both observation lists once more (w + index each way); counted with the iterations of the last product
    // (two-level preconditioner: + the block inverses and A_c^-1 once per iteration)
    const int64_t tl_iter = tl_ ? tl_nagg_ * kSchurAggCams * kSchurAggCams * 8 + tl_nagg_ * tl_nagg_ * 8 : 0;
    const int64_t inner = pcg_ ? (int64_t)std::max(1, pcg_last_iters_[1]) * (2 * nobs_ * (8 + 4) + tl_iter) : 8 * (n_ - 1) * (n_ - 1);
    return nobs_ * (8 + 4) + nobs_ * (8 + 24 + 4) + nobs_ * (8 + 24 + 4) + nobs_ * (8 + 4) + inner + 2LL * 8 * 3 * n_ * o;
}

template <int O>
static void schur_product_o(int epi, int64_t n, int64_t nobs, const SchurLm &L, const int64_t *cam_ptr, const int32_t *cam_lm, const double *cam_w, const double *cam_p,
                            const double *Q1,
                            const double *c, const double *q3inv, const double *vtinv, int64_t nred, int64_t ldv, double *h, double *r,
                            double *xc, double *xl, const double *W, double alpha, const CamArgs &a, SymvWork *sym_work, hipStream_t st,
                            Comm *comm, int64_t nred_loc, const std::function<void(const TcgScal *)> &solve_pcg) {
    const TcgScal *sc = (epi == EPI_HESS) ? a.scal : (const TcgScal *)nullptr;
    const int64_t nheavy = L.nheavy, nlight = L.m - L.nheavy;
    const dim3 b(256), gc(qw_grid((int)n)), gy(qw_grid(a.nloc));
    const dim3 glm((unsigned)(nheavy + (nlight + kSchurHeavyThreads - 1) / kSchurHeavyThreads)), blm(kSchurHeavyThreads);
    hipLaunchKernelGGL((schur_lm_h_kernel<O>), glm, blm, 0, st, L, q3inv, W, sc, h);
    hipLaunchKernelGGL((schur_cam_r_kernel<O>), gc, b, 0, st, (int)n, cam_ptr, cam_lm, cam_w, c, W, h, sc, r);
    if (n > 1 && solve_pcg) {
        solve_pcg(sc);   // x_cam by preconditioned CG on the matrix-free reduced camera Laplacian (SchurOp::pcg_solve)
    } else if (n > 1) {
        constexpr int OPc = pitch_of(O);
        CamArgs pa;
        std::memset(&pa, 0, sizeof(pa));
        pa.scal = a.scal;
        if (comm) {   // this rank's rows of VT^-1, then everybody's x_cam (equal chunks: the system is padded to world * nred_loc pseudo-cameras)
            const int64_t a0 = (int64_t)comm->rank * nred_loc;
            pa.nloc = (int)nred_loc; pa.out = xc + (size_t)3 * a0 * OPc;
            launch_qw_dense(O, EPI_PLAIN, vtinv + (size_t)3 * a0 * (size_t)ldv, ldv, r, 1.0, pa, st);
            comm->allgather(xc, (size_t)3 * nred_loc * OPc, st);
        } else {
            pa.nloc = (int)nred; pa.out = xc;
            if (sym_work && (O == 3 || O == 4)) launch_qw_sym(O, EPI_PLAIN, vtinv, ldv, r, 1.0, pa, *sym_work, st);
            else launch_qw_dense(O, EPI_PLAIN, vtinv, ldv, r, 1.0, pa, st);
        }
    }
    hipLaunchKernelGGL((schur_lm_x_kernel<O>), glm, blm, 0, st, L, q3inv, h, xc, sc, xl);
    switch (epi) {
        case EPI_PLAIN: hipLaunchKernelGGL((schur_cam_y_kernel<O, EPI_PLAIN>), gy, b, 0, st, n, nobs, cam_ptr, cam_lm, cam_w, cam_p, Q1, c, W, xc, xl, alpha, a); break;
        case EPI_GRAD: hipLaunchKernelGGL((schur_cam_y_kernel<O, EPI_GRAD>), gy, b, 0, st, n, nobs, cam_ptr, cam_lm, cam_w, cam_p, Q1, c, W, xc, xl, alpha, a); break;
        case EPI_HESS: hipLaunchKernelGGL((schur_cam_y_kernel<O, EPI_HESS>), gy, b, 0, st, n, nobs, cam_ptr, cam_lm, cam_w, cam_p, Q1, c, W, xc, xl, alpha, a); break;
        case EPI_CERT:
            if constexpr (O == 1) { hipLaunchKernelGGL((schur_cam_y_kernel<1, EPI_CERT>), gy, b, 0, st, n, nobs, cam_ptr, cam_lm, cam_w, cam_p, Q1, c, W, xc, xl, alpha, a); break; }
            throw Error(XM_ERR_ARG, "certificate operator needs o == 1");
        default: throw Error(XM_ERR_ARG, "bad epilogue");
    }
}

void SchurOp::product(int o, int epi, const double *W, double alpha, const CamArgs &a, hipStream_t st) {
    ensure(o);
    if (o != o_last_) {   // the row pitch of the scratch vectors changes with o: start from clean zero padding
        XM_HIP_CHECK(hipMemsetAsync(r_.p, 0, r_.count * sizeof(double), st));
        XM_HIP_CHECK(hipMemsetAsync(xc_.p, 0, xc_.count * sizeof(double), st));
        o_last_ = o;
    }
    const SchurLm L = lm_lists();
    std::function<void(const TcgScal *)> pcg;
    // inner tolerance by the kind of product: the truncated CG tolerates a Hessian applied to 1e-9 (its own stop rule is a RELATIVE residual of
    // 1e-1 .. 1e-6, its recurrences never look at the true residual), the gradient that decides convergence and the certificate do not
    const int kind = (epi == EPI_HESS) ? 1 : 0;
    if (pcg_) pcg = [&](const TcgScal *sc) {
        if (tl_) { XM_DISPATCH_O(o, (pcg_solve<O_, true>(L, sc, st, kind))); }
        else { XM_DISPATCH_O(o, (pcg_solve<O_, false>(L, sc, st, kind))); }
    };
    XM_DISPATCH_O(o, (schur_product_o<O_>(epi, n_, nobs_, L, cam_ptr_.p, cam_lm_.p, cam_w_.p, cam_p_.p, Q1_.p,
                                         c_.p, q3inv_.p, vtinv_.p, nred_, ldv_, h_.p, r_.p, xc_.p, xl_.p, W, alpha, a, (vt_sym_ && !comm_ && sym_work_) ? &sym_work_ : nullptr, st,
                                         comm_, nred_loc_, pcg)));
    check_launch("schur_product");
}

// x_cam = VT^-1 r by preconditioned CG (kernels above).  The iterations are enqueued in batches without looking at the device: as many as
// the previous product needed (+ 2), then the host reads the state word and tops up in steps of 8 -- one host round trip per product in
// the steady state, where consecutive right-hand sides of a truncated CG need the same number of iterations to within a few.
struct PcgGrids { dim3 b, gf, gc, glm, blm, gb; };   // flat kernels, camera pass, landmark pass, aggregate blocks
void SchurOp::pcg_setup(int o, int kind, const SchurLm &L, PcgArgs &a, PcgTwoLevel &t, PcgGrids &g) {
    a.n1 = (int)(n_ - 1); a.grid = pcg_grid_; a.tol2 = pcg_tol_[kind] * pcg_tol_[kind];
    a.b = r_.p; a.q2 = q2_.p;
    if (tl_) a.z = tl_z_.p; else a.dinv = pcg_dinv_.p;
    a.x = xc_.p; a.r = pcg_r_.p; a.p = pcg_p_.p; a.Ap = pcg_ap_.p;
    const size_t seg = (size_t)pcg_grid_ * o;
    a.prz[0] = pcg_parts_.p; a.prz[1] = pcg_parts_.p + seg; a.prr = pcg_parts_.p + 2 * seg; a.pbb = pcg_parts_.p + 3 * seg;
    a.ppap = pcg_parts_.p + 4 * seg; a.cam_grid = qw_grid((int)n_);
    a.st = reinterpret_cast<PcgState *>(pcg_state_.p);
    const int64_t nlight = L.m - L.nheavy;
    g.b = dim3(256); g.gf = dim3(pcg_grid_); g.gc = dim3(a.cam_grid);
    g.glm = dim3((unsigned)(L.nheavy + (nlight + kSchurHeavyThreads - 1) / kSchurHeavyThreads)); g.blm = dim3(kSchurHeavyThreads);
    t.nagg = tl_nagg_; t.perm = tl_perm_.p; t.binv = tl_binv_.p; t.ainv = tl_ainv_.p; t.g = tl_g_.p; t.z = tl_z_.p;
    g.gb = dim3((unsigned)std::max<int64_t>(1, (tl_nagg_ + kQwWaves - 1) / kQwWaves));
}
template <int O, bool TL>
void SchurOp::pcg_precond(const PcgArgs &a, const PcgTwoLevel &t, const PcgGrids &g, int par, int init, hipStream_t st) {   // z = M^-1 r, <r, z> into parity par (init: p = z)
    if constexpr (TL) {
        hipLaunchKernelGGL((pcg_block_kernel<O>), g.gb, g.b, 0, st, a, t);
        hipLaunchKernelGGL((pcg_coarse_kernel<O>), g.gf, g.b, 0, st, a, t, par, init);
    }
}
template <int O, bool TL>
void SchurOp::pcg_start(const PcgArgs &a, const PcgTwoLevel &t, const PcgGrids &g, const TcgScal *sc, hipStream_t st) {
    hipLaunchKernelGGL((pcg_init_kernel<O, TL>), g.gf, g.b, 0, st, a, sc);
    pcg_precond<O, TL>(a, t, g, 0, 1, st);
}
template <int O>
void SchurOp::pcg_operator(const SchurLm &L, const PcgArgs &a, const PcgGrids &g, hipStream_t st) {   // Ap = VT p through the two lists (y_l in xl_)
    hipLaunchKernelGGL((pcg_lm_kernel<O>), g.glm, g.blm, 0, st, L, q3inv_.p, (const double *)a.p, (const PcgState *)a.st, xl_.p);
    hipLaunchKernelGGL((pcg_cam_kernel<O>), g.gc, g.b, 0, st, (int)n_, cam_ptr_.p, cam_lm_.p, cam_w_.p, (const double *)xl_.p, a);
}
template <int O, bool TL>
void SchurOp::pcg_solve(const SchurLm &L, const TcgScal *sc, hipStream_t st, int kind) {
    PcgArgs a;
    PcgTwoLevel t;
    PcgGrids g;
    pcg_setup(O, kind, L, a, t, g);
    pcg_start<O, TL>(a, t, g, sc, st);
    int it = 0, dir_applied = 0;   // dir_applied: the iteration whose direction update is already in the queue (iteration 0 needs none)
    auto enqueue = [&](int upto) {
        for (; it < upto; ++it) {
            if (it != dir_applied) hipLaunchKernelGGL((pcg_dir_kernel<O, TL>), g.gf, g.b, 0, st, a, it);
            pcg_operator<O>(L, a, g, st);
            hipLaunchKernelGGL((pcg_upd_kernel<O, TL>), g.gf, g.b, 0, st, a, it);
            pcg_precond<O, TL>(a, t, g, (it & 1) ^ 1, 0, st);
        }
        // the convergence test of the last update (no-op once done).  When the test fails the same launch IS the direction update of iteration
        // `it`: a following batch must not repeat it (p = z + beta (z + beta p) is no conjugate direction -- ADVICE r5)
        hipLaunchKernelGGL((pcg_dir_kernel<O, TL>), g.gf, g.b, 0, st, a, it);
        dir_applied = it;
    };
    int target = std::min(pcg_max_iters_, std::max(4, pcg_last_iters_[kind] + 2));
    for (;;) {
        enqueue(target);
        check_launch("schur_pcg");
        XM_HIP_CHECK(hipMemcpyAsync(pcg_host_, a.st, sizeof(PcgState), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipStreamSynchronize(st));
        if (pcg_host_->done || target >= pcg_max_iters_) break;
        target = std::min(pcg_max_iters_, target + 8);
    }
    if (pcg_host_->done && pcg_host_->iters > 0) pcg_last_iters_[kind] = pcg_host_->iters;
    pcg_last_relres_ = pcg_host_->relres;
    pcg_products_++;
    pcg_iters_total_ += pcg_host_->done ? pcg_host_->iters : target;
    if (!pcg_host_->done) pcg_unconverged_++;
}

// ------------------------------------------------------------------------------------------------------------------
// The test export xm_ctx_schur_probe (include/xm_amd.h)
// ------------------------------------------------------------------------------------------------------------------
// <p, VT p> per column from the camera pass's partial sums, by the tree pcg_upd_kernel adds them with
template <int O>
__global__ __launch_bounds__(256) void pcg_probe_pap_kernel(PcgArgs a, double *__restrict__ out) {
    __shared__ double sh[4];
    double pap[O];
    pcg_sums<O>(a.ppap, a.cam_grid, pap, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < O; ++k) out[k] = pap[k];
    }
}
namespace {
template <class T>
std::vector<T> probe_fetch(const T *dev, size_t count, hipStream_t st) {
    std::vector<T> v(count);
    if (count) XM_HIP_CHECK(hipMemcpyAsync(v.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipStreamSynchronize(st));
    return v;
}
// records of `pitch` doubles (rows x o used) -> column-major rows x o; row_of: the record of output row i (null: i)
void probe_unpack(const std::vector<double> &rec, int64_t rows, int o, int pitch, const int32_t *row_of, double *out) {
    for (int64_t i = 0; i < rows; ++i) {
        const size_t s = (size_t)(row_of ? row_of[i] : i) * pitch;
        for (int k = 0; k < o; ++k) out[(size_t)i + (size_t)k * rows] = rec[s + k];
    }
}
std::vector<double> probe_pack(const double *in, int64_t rows, int o, int pitch, size_t count) {
    std::vector<double> rec(count, 0.0);
    for (int64_t i = 0; i < rows; ++i)
        for (int k = 0; k < o; ++k) rec[(size_t)i * pitch + k] = in[(size_t)i + (size_t)k * rows];
    return rec;
}
}  // namespace

template <int O>
void SchurOp::probe_chain(xm_schur_probe_t &q, hipStream_t st) {
    constexpr int OP = pitch_of(O);
    const int64_t n1 = n_ - 1;
    DevBuf<double> dW, dY;
    const std::vector<double> hW = probe_pack(q.W, 3 * n_, O, OP, (size_t)(n_ + kColPad) * 3 * OP);
    dW.alloc(hW.size(), false); dY.alloc((size_t)n_ * 3 * OP + 2);
    XM_HIP_CHECK(hipMemcpyAsync(dW.p, hW.data(), hW.size() * sizeof(double), hipMemcpyHostToDevice, st));
    CamArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nloc = (int)n_; a.out = dY.p;
    product(O, EPI_PLAIN, dW.p, q.alpha, a, st);
    if (q.h) probe_unpack(probe_fetch(h_.p, (size_t)m_ * OP, st), m_, O, OP, slot_of_.data(), q.h);
    if (q.xl) probe_unpack(probe_fetch(xl_.p, (size_t)m_ * OP, st), m_, O, OP, slot_of_.data(), q.xl);
    if (q.r) probe_unpack(probe_fetch(r_.p, (size_t)n1 * OP, st), n1, O, OP, nullptr, q.r);
    if (q.xc) probe_unpack(probe_fetch(xc_.p, (size_t)n1 * OP, st), n1, O, OP, nullptr, q.xc);
    if (q.Y) probe_unpack(probe_fetch(dY.p, (size_t)n_ * 3 * OP, st), 3 * n_, O, OP, nullptr, q.Y);
    XM_HIP_CHECK(hipStreamSynchronize(st));
    if (pcg_ && n1 > 0) { q.pcg_done = pcg_host_->done; q.pcg_iters = pcg_host_->iters; q.pcg_relres = pcg_host_->relres; }
}

template <int O, bool TL>
void SchurOp::probe_pcg(xm_schur_probe_t &q, const SchurLm &L, hipStream_t st) {
    constexpr int OP = pitch_of(O);
    const int64_t n1 = n_ - 1;
    ensure(O);
    PcgArgs a;
    PcgTwoLevel t;
    PcgGrids g;
    pcg_setup(O, 0, L, a, t, g);
    const std::vector<double> hX = probe_pack(q.X, n1, O, OP, (size_t)n1 * OP);
    // b := X (the rows beyond n1 of r_ stay as they are; product() clears the vector again: o_last_ below)
    XM_HIP_CHECK(hipMemcpyAsync(r_.p, hX.data(), hX.size() * sizeof(double), hipMemcpyHostToDevice, st));
    pcg_start<O, TL>(a, t, g, nullptr, st);
    check_launch("schur probe (M^-1 X)");
    if (q.MX) probe_unpack(probe_fetch(pcg_p_.p, (size_t)n1 * OP, st), n1, O, OP, nullptr, q.MX);
    // p := X; the state word says "not done" since the init launch
    XM_HIP_CHECK(hipMemcpyAsync(pcg_p_.p, hX.data(), hX.size() * sizeof(double), hipMemcpyHostToDevice, st));
    pcg_operator<O>(L, a, g, st);
    DevBuf<double> dpap;
    dpap.alloc(O);
    hipLaunchKernelGGL((pcg_probe_pap_kernel<O>), dim3(1), dim3(256), 0, st, a, dpap.p);
    check_launch("schur probe (VT X)");
    if (q.VX) probe_unpack(probe_fetch(pcg_ap_.p, (size_t)n1 * OP, st), n1, O, OP, nullptr, q.VX);
    if (q.pAp) {
        const std::vector<double> v = probe_fetch(dpap.p, O, st);
        std::copy(v.begin(), v.end(), q.pAp);
    }
    XM_HIP_CHECK(hipStreamSynchronize(st));
}

SchurLm SchurOp::lm_lists() const {
    SchurLm L;
    L.m = m_; L.nheavy = nheavy_; L.total = ltotal_; L.ptr = lm_ptr_.p; L.gbase = gbase_.p; L.deg = ldeg_.p; L.cam = lm_cam_.p; L.w = lm_w_.p; L.p = lm_p_.p;
    return L;
}

void SchurOp::probe(xm_schur_probe_t &q, hipStream_t st) {
    if (comm_) throw Error(XM_ERR_ARG, "xm_ctx_schur_probe: single-rank contexts only");
    const int64_t n1 = n_ - 1;
    const bool cg = pcg_ && n1 > 0, tl = tl_ && n1 > 0;
    if (!pcg_ && (q.dinv || q.VX || q.pAp || q.MX || q.k > 0)) throw Error(XM_ERR_ARG, "xm_ctx_schur_probe: dinv, X, VX, pAp and MX need the CG form (xm_tuning_t.schur_solver 2 or 3)");
    if (pcg_ && q.VTinv) throw Error(XM_ERR_ARG, "xm_ctx_schur_probe: the CG form keeps no VTinv");
    if (!tl_ && (q.perm || q.binv || q.ainv)) throw Error(XM_ERR_ARG, "xm_ctx_schur_probe: perm, binv and ainv need the two-level preconditioner (xm_tuning_t.schur_solver 3)");
    if (q.VTinv && n1 > XM_SCHUR_PROBE_DENSE_MAX_ROWS) throw Error(XM_ERR_ARG, "xm_ctx_schur_probe: VTinv with more than XM_SCHUR_PROBE_DENSE_MAX_ROWS rows");
    q.nheavy = nheavy_; q.lm_total = ltotal_; q.nagg = tl ? tl_nagg_ : 0;
    q.uses_cg = pcg_ ? 1 : 0; q.two_level = tl_ ? 1 : 0; q.dup_pairs = dup_pairs_ ? 1 : 0;
    q.pcg_done = 0; q.pcg_iters = 0; q.pcg_relres = 0.0; q.pcg_tol = pcg_ ? pcg_tol_[0] : 0.0; q.pcg_cap = pcg_ ? pcg_max_iters_ : 0;
    XM_HIP_CHECK(hipStreamSynchronize(st));
    auto by_landmark = [&](const auto &slot_vals, auto *out) {
        for (int64_t l = 0; l < m_; ++l) out[l] = slot_vals[(size_t)slot_of_[(size_t)l]];
    };
    auto copy_out = [&](const double *dev, size_t count, double *out) {
        const std::vector<double> v = probe_fetch(dev, count, st);
        std::copy(v.begin(), v.end(), out);
    };
    if (q.deg) by_landmark(probe_fetch(ldeg_.p, (size_t)m_, st), q.deg);
    if (q.q3inv) by_landmark(probe_fetch(q3inv_.p, (size_t)m_, st), q.q3inv);
    if (q.Q1) copy_out(Q1_.p, (size_t)n_ * 9, q.Q1);
    if (q.c) copy_out(c_.p, (size_t)n_ * 3, q.c);
    if (q.q2) copy_out(q2_.p, (size_t)n_, q.q2);
    if (q.dinv && cg) copy_out(pcg_dinv_.p, (size_t)n1, q.dinv);
    if (q.VTinv && n1 > 0) {   // row i of the padded row-major layout -> column-major n1 x n1
        std::vector<double> v((size_t)n1 * n1);
        XM_HIP_CHECK(hipMemcpy2DAsync(v.data(), (size_t)n1 * sizeof(double), vtinv_.p, (size_t)ldv_ * sizeof(double), (size_t)n1 * sizeof(double), (size_t)n1,
                                      hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipStreamSynchronize(st));
        for (int64_t i = 0; i < n1; ++i)
            for (int64_t j = 0; j < n1; ++j) q.VTinv[(size_t)i + (size_t)j * n1] = v[(size_t)i * n1 + j];
    }
    if (tl) {
        if (q.perm) {
            const std::vector<int32_t> v = probe_fetch(tl_perm_.p, (size_t)tl_nagg_ * kSchurAggCams, st);
            std::copy(v.begin(), v.end(), q.perm);
        }
        if (q.binv) copy_out(tl_binv_.p, (size_t)tl_nagg_ * kSchurAggCams * kSchurAggCams, q.binv);
        if (q.ainv) copy_out(tl_ainv_.p, (size_t)tl_nagg_ * tl_nagg_, q.ainv);
    }
    // the statistics of the CG form and its batch sizes are the products' own: put back behind the probe's launches
    const int64_t s_products = pcg_products_, s_iters = pcg_iters_total_, s_unconv = pcg_unconverged_;
    const int s_last[2] = {pcg_last_iters_[0], pcg_last_iters_[1]};
    const double s_relres = pcg_last_relres_;
    struct Leave {
        std::function<void()> f;
        ~Leave() { f(); }
    } leave{[&] {
        pcg_products_ = s_products; pcg_iters_total_ = s_iters; pcg_unconverged_ = s_unconv;
        pcg_last_iters_[0] = s_last[0]; pcg_last_iters_[1] = s_last[1]; pcg_last_relres_ = s_relres;
        o_last_ = 0;   // the next product starts from clean padding in r_ and xc_ (the CG pieces wrote X into r_)
    }};
    if (q.o > 0) { XM_DISPATCH_O(q.o, (probe_chain<O_>(q, st))); }
    if (q.k > 0 && cg) {
        const SchurLm L = lm_lists();
        if (tl_) { XM_DISPATCH_O(q.k, (probe_pcg<O_, true>(q, L, st))); }
        else { XM_DISPATCH_O(q.k, (probe_pcg<O_, false>(q, L, st))); }
    }
}

}  // namespace xm
