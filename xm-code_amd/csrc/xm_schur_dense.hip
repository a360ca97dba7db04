// xm_schur_dense.hip — the dense Q (and Abar) of utils/creatematrix.py:137-339 built on the device from the lists a SchurOp already holds.
//
// With D = diag(1/Q3) (0 for a landmark without weight), B the sparse 3N x M matrix with w p at (camera, landmark) and C the 3N x (N-1)
// matrix with c_i in column i-1 (the chain of xm_schur.h written as matrices):
//      G    = C - B D V3_bar^T                                   3N x (N-1)
//      Q    = blockdiag(Q1_i) - B D B^T - G VT^-1 G^T
//      Abar = [ -VT^-1 G^T ; D (B^T + V3_bar^T Abar_cam) ]      (N-1+M) x 3N
// The symmetric matrix lives in the context's own Q buffer from the start: read column-major (leading dimension ldq) its lower triangle is
// assembled, updated by the two lower_only GEMMs and finally mirrored, and a symmetric matrix is its own row-major image -- the layout of the
// dense kernels.  No floating-point atomics anywhere: every entry is owned by one lane (a landmark names a camera once) or one GEMM tile, so two
// builds give the same bits.
#include "xm_schur.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "xm_device.h"

namespace xm {

struct DenseQLists {
    int64_t n, nobs, nheavy, total;
    const int64_t *cam_ptr, *lm_ptr, *gbase;
    const int32_t *cam_lm, *lm_cam, *deg;
    const double *cam_w, *cam_p, *lm_w, *lm_p, *q3inv, *c;
};

// Light landmarks.  ONE wavefront per camera a and column window (blockIdx.y: the cameras [cb0, cb0 + ncam)), in the manner of
// schur_vt_rows_kernel: the strip of camera a -- three rows of B D B^T (9 doubles per window camera) and three rows of G (3 doubles) -- sits in
// LDS; the camera's observations are walked in list order and each landmark's observation list is spread over the lanes.  Of B D B^T only the
// blocks (b, a) with b >= a are kept: they are written as the COLUMNS 3a .. 3a+2 of the column-major lower triangle, contiguous along the strip.
// G is written transposed (Gt: (N-1) x 3N, column-major), three contiguous columns per camera.
__global__ __launch_bounds__(64) void schur_dense_rows_kernel(DenseQLists L, int wincams, double *__restrict__ S, int64_t lds,
                                                               double *__restrict__ Gt, int64_t mr) {
    extern __shared__ double strip[];
    const int lane = threadIdx.x;
    const int64_t a = blockIdx.x, cb0 = (int64_t)blockIdx.y * wincams;
    const int ncam = (int)min((int64_t)wincams, L.n - cb0);
    double *srow = strip, *grow = strip + (size_t)9 * ncam;   // srow[r][3 j + c], grow[r][j]
    for (int j = lane; j < 12 * ncam; j += 64) strip[j] = 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < 3 && a >= 1 && a >= cb0 && a < cb0 + ncam) grow[lane * ncam + (int)(a - cb0)] = L.c[a * 3 + lane];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const bool lower = cb0 + ncam > a;   // the window holds cameras b >= a (wave-uniform)
    // The camera's list is taken 64 observations at a time: lane k fetches what observation e0 + k contributes to every entry (u = w p / Q3_l,
    // where its landmark's list starts, how long it is) into LDS, then the wavefront walks the batch in list order reading those as
    // broadcasts -- the chain of dependent loads (observation -> landmark -> 1/Q3 -> list) is paid once per 64 observations, not once each.
    __shared__ double bu[3][64];
    __shared__ int64_t bbase[64];
    __shared__ int bdeg[64];
    const int64_t e_end = L.cam_ptr[a + 1];
    for (int64_t e0 = L.cam_ptr[a]; e0 < e_end; e0 += 64) {   // wave-uniform
        {
            const int64_t e = e0 + lane;
            int dg = 0;
            int64_t base = 0;
            double u0 = 0.0, u1 = 0.0, u2 = 0.0;
            if (e < e_end) {
                const int64_t sl = L.cam_lm[e];
                const double wa = L.cam_w[e];
                if (sl >= L.nheavy && wa != 0.0) {
                    const double qi = L.q3inv[sl];
                    if (qi != 0.0) {
                        const int64_t t = sl - L.nheavy;
                        dg = L.deg[sl];
                        base = L.gbase[t >> 6] + (t & 63);
                        u0 = wa * L.cam_p[e] * qi; u1 = wa * L.cam_p[L.nobs + e] * qi; u2 = wa * L.cam_p[2 * L.nobs + e] * qi;
                    }
                }
            }
            bu[0][lane] = u0; bu[1][lane] = u1; bu[2][lane] = u2; bbase[lane] = base; bdeg[lane] = dg;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nb = (int)min((int64_t)64, e_end - e0);
        for (int k = 0; k < nb; ++k) {
            const int dg = bdeg[k];
            if (dg == 0) continue;   // (wave-uniform: a heavy landmark, no weight, or a landmark without weight)
            if (lane < dg) {
                const double u[3] = {bu[0][k], bu[1][k], bu[2][k]};
                const int64_t at = bbase[k] + (int64_t)64 * lane;
                const int64_t b = L.lm_cam[at];
                const int64_t j = b - cb0;
                if (j >= 0 && j < ncam) {
                    const double wb = L.lm_w[at];
                    if (b != 0) {
#pragma unroll
                        for (int r = 0; r < 3; ++r) grow[r * ncam + j] -= u[r] * wb;
                    }
                    if (lower && b >= a) {
                        const double v[3] = {wb * L.lm_p[at], wb * L.lm_p[L.total + at], wb * L.lm_p[2 * L.total + at]};
#pragma unroll
                        for (int r = 0; r < 3; ++r)
#pragma unroll
                            for (int c = 0; c < 3; ++c) srow[r * 3 * ncam + 3 * j + c] -= u[r] * v[c];
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (lower)
        for (int r = 0; r < 3; ++r) {
            double *col = S + (size_t)(3 * a + r) * (size_t)lds;
            for (int j = lane; j < 3 * ncam; j += 64) {
                const int64_t row = 3 * cb0 + j;
                if (row >= 3 * a) col[row] = srow[r * 3 * ncam + j];
            }
        }
    for (int r = 0; r < 3; ++r) {
        double *col = Gt + (size_t)(3 * a + r) * (size_t)mr;
        for (int j = lane; j < ncam; j += 64) {
            const int64_t b = cb0 + j;
            if (b >= 1) col[b - 1] = grow[r * ncam + j];
        }
    }
}

// Heavy landmarks (more than kSchurHeavy observations: the first nheavy slots) are dense columns: slot h's column of the 3N x nheavy panel
// P = B sqrt(D) and of the (N-1) x nheavy panel U = V3_bar sqrt(D) (both zero-filled before).  One workgroup per landmark; a landmark names a
// camera once, so every entry has one writer.  Then B D B^T (heavy part) = P P^T and B D V3_bar^T (heavy part) = P U^T: two GEMMs.
__global__ __launch_bounds__(256) void schur_dense_heavy_kernel(DenseQLists L, double *__restrict__ P, double *__restrict__ U, int64_t mr) {
    const int64_t h = blockIdx.x;
    const double sq = sqrt(L.q3inv[h]);
    for (int64_t e = L.lm_ptr[h] + threadIdx.x; e < L.lm_ptr[h + 1]; e += 256) {
        const int64_t b = L.lm_cam[e];
        const double w = sq * L.lm_w[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) P[(size_t)h * 3 * L.n + 3 * b + c] = w * L.lm_p[c * L.total + e];
        if (b >= 1) U[(size_t)h * mr + b - 1] = w;
    }
}

__global__ __launch_bounds__(256) void schur_dense_negate_kernel(int64_t count, double *__restrict__ x) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < count) x[e] = -x[e];
}

// Finish: Q(i, j) = S(i, j) + [i / 3 == j / 3] Q1_{i/3}(i % 3, j % 3) for i >= j, stored at (i, j) AND (j, i) from the same register: the matrix
// is symmetric bit for bit (what the automatic choice of the half-traffic product asks for).  One workgroup per 64 x 64 tile on or below
// the diagonal; it reads its tile before it writes the tile and the mirror tile, and no other workgroup touches either: in place.
__global__ __launch_bounds__(256) void schur_dense_finish_kernel(int64_t n3, double *__restrict__ S, int64_t lds, const double *__restrict__ Q1) {
    if (blockIdx.y > blockIdx.x) return;
    __shared__ double T[64][65];   // T[i - i0][j - j0]
    const int64_t i0 = (int64_t)blockIdx.x * 64, j0 = (int64_t)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int k = ty; k < 64; k += 4) {
        const int64_t i = i0 + tx, j = j0 + k;
        double v = 0.0;
        if (i < n3 && j < n3 && i >= j) {
            v = S[(size_t)i + (size_t)j * lds];
            if (i / 3 == j / 3) v += Q1[(i / 3) * 9 + (i % 3) * 3 + (j % 3)];
        }
        T[tx][k] = v;
    }
    __syncthreads();
    const bool diag = blockIdx.x == blockIdx.y;
    for (int k = ty; k < 64; k += 4) {
        const int64_t i = i0 + tx, j = j0 + k;
        if (i < n3 && j < n3) S[(size_t)i + (size_t)j * lds] = (i >= j) ? T[tx][k] : T[k][tx];
    }
    if (diag) return;
    for (int k = ty; k < 64; k += 4) {
        const int64_t j = j0 + tx, i = i0 + k;
        if (i < n3 && j < n3) S[(size_t)j + (size_t)i * lds] = T[k][tx];
    }
}

// Landmark rows of Abar for the landmarks [l0, l0 + np): row l = (1/Q3_l) (sum_{obs of l} w p^T at the camera's columns + sum_{obs, camera >= 1}
// w Abar_cam[camera - 1, :]).  At: Abar_cam TRANSPOSED (3N x (N-1), column-major), so the threads of a workgroup (one per column j of the row)
// read it coalesced.  One workgroup per landmark, the observation list in list order: fixed summation order.  out: np rows of 3N doubles.
__global__ __launch_bounds__(256) void schur_abar_lm_kernel(DenseQLists L, int64_t l0, const int32_t *__restrict__ slot_of,
                                                            const double *__restrict__ At, double *__restrict__ out) {
    const int64_t sl = slot_of[l0 + blockIdx.x], n3 = 3 * L.n;
    const double qi = L.q3inv[sl];
    int64_t base, stride, count;
    if (sl < L.nheavy) { base = L.lm_ptr[sl]; stride = 1; count = L.lm_ptr[sl + 1] - base; }
    else { const int64_t t = sl - L.nheavy; base = L.gbase[t >> 6] + (t & 63); stride = 64; count = L.deg[sl]; }
    for (int64_t j = threadIdx.x; j < n3; j += 256) {
        const int64_t cj = j / 3;
        const int ax = (int)(j % 3);
        double acc = 0.0, own = 0.0;
        for (int64_t k = 0; k < count; ++k) {
            const int64_t at = base + k * stride, b = L.lm_cam[at];
            const double w = L.lm_w[at];
            if (b >= 1) acc += w * At[(size_t)j + (size_t)(b - 1) * (size_t)n3];
            if (b == cj) own = w * L.lm_p[ax * L.total + at];
        }
        out[(size_t)blockIdx.x * (size_t)n3 + j] = qi * (own + acc);
    }
}

void SchurOp::build_dense_q(double *Q, int64_t ldq, double *abar, hipStream_t st) {
    if (pcg_ || comm_) throw Error(XM_ERR_ARG, "dense Q from observations: needs the dense inverse of the reduced camera Laplacian on one GPU");
    if (dup_pairs_) throw Error(XM_ERR_ARG, "dense Q from observations: the device assembly assumes that a landmark names a camera once");
    const int64_t N = n_, mr = N - 1, n3 = 3 * N;
    const bool trace = cfg_.trace;
    auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!trace) return;
        XM_HIP_CHECK(hipStreamSynchronize(st));
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "schur dense Q: %-28s %8.1f ms\n", what, std::chrono::duration<double>(now - tp).count() * 1e3);
        tp = now;
    };
    DenseQLists L;
    L.n = N; L.nobs = nobs_; L.nheavy = nheavy_; L.total = ltotal_;
    L.cam_ptr = cam_ptr_.p; L.lm_ptr = lm_ptr_.p; L.gbase = gbase_.p; L.cam_lm = cam_lm_.p; L.lm_cam = lm_cam_.p; L.deg = ldeg_.p;
    L.cam_w = cam_w_.p; L.cam_p = cam_p_.p; L.lm_w = lm_w_.p; L.lm_p = lm_p_.p; L.q3inv = q3inv_.p; L.c = c_.p;
    const int64_t mr1 = std::max<int64_t>(mr, 1);
    DevBuf<double> Gt, At;   // G^T, later -G^T: (N-1) x 3N | Abar_cam^T = -G VT^-1: 3N x (N-1)
    Gt.alloc((size_t)mr1 * n3, false);
    {
        static const bool once = [] {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(schur_dense_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)(12 * kSchurDenseQWinCams * sizeof(double)));
            (void)hipGetLastError();
            return e == hipSuccess;
        }();
        (void)once;
    }
    const int win = (int)std::min<int64_t>(kSchurDenseQWinCams, N);
    const unsigned nwin = (unsigned)((N + win - 1) / win);
    hipLaunchKernelGGL(schur_dense_rows_kernel, dim3((unsigned)N, nwin), dim3(64), (size_t)12 * win * sizeof(double), st, L, win, Q, ldq, Gt.p, mr1);
    check_launch("dense Q (assembly)");
    lap("assembly (light landmarks)");
    if (nheavy_ > 0) {
        DevBuf<double> P, U;
        P.alloc((size_t)nheavy_ * n3, false); U.alloc((size_t)nheavy_ * mr1, false);
        XM_HIP_CHECK(hipMemsetAsync(P.p, 0, P.count * sizeof(double), st));
        XM_HIP_CHECK(hipMemsetAsync(U.p, 0, U.count * sizeof(double), st));
        hipLaunchKernelGGL(schur_dense_heavy_kernel, dim3((unsigned)nheavy_), dim3(256), 0, st, L, P.p, U.p, mr1);
        check_launch("dense Q (heavy panel)");
        gemm_sub_device((int)n3, (int)n3, (int)nheavy_, P.p, n3, 0, P.p, n3, 1, Q, ldq, 1, st);          // S -= P P^T (lower tiles)
        gemm_sub_device((int)mr, (int)n3, (int)nheavy_, U.p, mr1, 0, P.p, n3, 1, Gt.p, mr1, 0, st);      // G^T -= U P^T
        XM_HIP_CHECK(hipStreamSynchronize(st));   // P, U go out of scope
    }
    lap("heavy panel");
    if (mr > 0) {
        At.alloc((size_t)n3 * mr, false);
        XM_HIP_CHECK(hipMemsetAsync(At.p, 0, At.count * sizeof(double), st));
        // VT^-1 in the dense kernels' row-major layout is, being symmetric, a column-major matrix of leading dimension ldv_
        gemm_sub_device((int)n3, (int)mr, (int)mr, Gt.p, mr1, 1, vtinv_.p, ldv_, 0, At.p, n3, 0, st);    // Abar_cam^T = -G VT^-1
        lap("G VT^-1");
        hipLaunchKernelGGL(schur_dense_negate_kernel, dim3((unsigned)(((int64_t)Gt.count + 255) / 256)), dim3(256), 0, st, (int64_t)Gt.count, Gt.p);
        gemm_sub_device((int)n3, (int)n3, (int)mr, Gt.p, mr1, 1, At.p, n3, 1, Q, ldq, 1, st);            // S -= (-G) (-G VT^-1)^T (lower tiles)
        check_launch("dense Q (symmetric update)");
        lap("symmetric update");
    }
    {
        const unsigned nt = (unsigned)((n3 + 63) / 64);
        hipLaunchKernelGGL(schur_dense_finish_kernel, dim3(nt, nt), dim3(256), 0, st, n3, Q, ldq, Q1_.p);
        check_launch("dense Q (layout)");
    }
    XM_HIP_CHECK(hipStreamSynchronize(st));
    lap("Q1 blocks, mirror, layout");
    if (!abar) return;
    const int64_t rows = mr + m_;
    if (mr > 0) {   // camera rows: the transpose of At
        std::vector<double> h((size_t)n3 * mr);
        XM_HIP_CHECK(hipMemcpyAsync(h.data(), At.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipStreamSynchronize(st));
        for (int64_t j = 0; j < n3; ++j)
            for (int64_t b = 0; b < mr; ++b) abar[(size_t)b + (size_t)j * rows] = h[(size_t)j + (size_t)b * n3];
    }
    if (!slot_dev_.p) {
        slot_dev_.alloc(slot_of_.size(), false);
        XM_HIP_CHECK(hipMemcpy(slot_dev_.p, slot_of_.data(), slot_of_.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (mr <= 0) { At.alloc(1); }   // (one camera: no translation is an unknown; the kernel never reads At)
    const int64_t np_max = std::min<int64_t>(kSchurAbarPanel, m_);
    DevBuf<double> panel;
    panel.alloc((size_t)np_max * n3, false);
    std::vector<double> hp((size_t)np_max * n3);
    for (int64_t l0 = 0; l0 < m_; l0 += kSchurAbarPanel) {   // device memory does not depend on M: a panel at a time, copied out as it is finished
        const int64_t np = std::min<int64_t>(kSchurAbarPanel, m_ - l0);
        hipLaunchKernelGGL(schur_abar_lm_kernel, dim3((unsigned)np), dim3(256), 0, st, L, l0, slot_dev_.p, At.p, panel.p);
        check_launch("Abar (landmark panel)");
        XM_HIP_CHECK(hipMemcpyAsync(hp.data(), panel.p, (size_t)np * n3 * sizeof(double), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipStreamSynchronize(st));
        for (int64_t j = 0; j < n3; ++j)
            for (int64_t q = 0; q < np; ++q) abar[(size_t)(mr + l0 + q) + (size_t)j * rows] = hp[(size_t)q * n3 + j];
    }
    lap("Abar (landmark panels)");
}

}  // namespace xm
