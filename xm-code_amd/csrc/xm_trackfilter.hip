// xm_trackfilter.hip — track filtering on the device (xm_trackfilter.h has the design; definition in include/xm_amd.h at xm_ctx_filter_tracks).
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/xm_amd.h"
#include "xm_trackfilter.h"
#include "xm_stage.h"

// every product and every sum of the contract is rounded on its own
#pragma clang fp contract(off)

namespace xm {
namespace {

constexpr int kT = kTfThreads;
static_assert(kT == kStageThreads && kTfTile == kT, "a thread per ray of a tile; the helpers of xm_stage.h are written for this workgroup size");
constexpr const char *kStage = "track filter";
constexpr double kEps = 1e-12;   // GLOMAP's EPS (track_filter.cc:20, :70)

// what the per-observation kernel found (one byte per observation, in both orders)
enum { CODE_UNUSED = 0, CODE_SURVIVOR, CODE_DEPTH, CODE_REPROJECTION, CODE_ANGLE };
// bits of a landmark's flag byte
enum { LF_USED = 1, LF_REPROJECTION = 2, LF_ANGLE = 4, LF_TRIANGULATION = 8, LF_MIN_VIEWS = 16 };
// slots of the counters (per workgroup, then summed)
enum { N_USED = 0, N_KEPT, N_DEPTH, N_REPROJECTION, N_ANGLE, N_TRIANGULATION, N_MIN_VIEWS, N_TRACKS, N_TRACKS_KEPT, N_CH_REPROJECTION, N_CH_ANGLE,
       N_CH_TRIANGULATION, N_CH_MIN_VIEWS, N_COUNT, N_PITCH = 16 };
static_assert(N_COUNT <= N_PITCH, "the reduction walks N_PITCH counters per workgroup");

struct TfArgs {
    uint32_t flags;
    int32_t min_views;
    double thr_reprojection, cos_angle, cos_triangulation;
};
struct TfWork {   // device arrays of one call
    uint8_t *code_l, *code_e;       // lm_total / nobs
    double *rx, *ry, *rz;           // lm_total each
    int32_t *views;                 // per landmark slot
    uint8_t *status, *lflags;
};

__device__ inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// rot: 9 doubles per camera, column a of R_i (= row a of R_i^T) at 9 i + 3 a; t: 3 per camera; P: 3 per landmark SLOT
__global__ __launch_bounds__(kT) void tf_obs_kernel(SchurLists S, TfArgs a, const double *__restrict__ rot, const double *__restrict__ t,
                                                    const double *__restrict__ P, TfWork W) {
    const double nan = __longlong_as_double(-1ll);
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * kT) {
        const int64_t pl = S.dpos_l[e];
        const double w = S.cam_w[S.pos_c[e]], p0 = S.obs_p[3 * e], p1 = S.obs_p[3 * e + 1], p2 = S.obs_p[3 * e + 2];
        uint8_t c = CODE_UNUSED;
        double r0 = nan, r1 = nan, r2 = nan;
        if (w > 0.0 && p2 > 0.0) {
            const double *R = rot + (size_t)9 * S.obs_cam[e], *T = t + (size_t)3 * S.obs_cam[e], *X = P + (size_t)3 * S.obs_lm[e];
            const double d0 = X[0] - T[0], d1 = X[1] - T[1], d2 = X[2] - T[2];
            c = CODE_SURVIVOR;
            if (a.flags & (XM_TF_REPROJECTION | XM_TF_ANGLE)) {
                const double q0 = dot3(R[0], R[1], R[2], d0, d1, d2), q1 = dot3(R[3], R[4], R[5], d0, d1, d2), q2 = dot3(R[6], R[7], R[8], d0, d1, d2);
                if (q2 < kEps) {
                    c = CODE_DEPTH;
                } else {
                    if (a.flags & XM_TF_REPROJECTION) {
                        const double u = q0 / q2 - p0 / p2, v = q1 / q2 - p1 / p2;
                        if (!(sqrt(u * u + v * v) < a.thr_reprojection)) c = CODE_REPROJECTION;
                    }
                    if (c == CODE_SURVIVOR && (a.flags & XM_TF_ANGLE)) {
                        const double nq = sqrt(dot3(q0, q1, q2, q0, q1, q2)), np = sqrt(dot3(p0, p1, p2, p0, p1, p2));
                        if (!(dot3(q0 / nq, q1 / nq, q2 / nq, p0 / np, p1 / np, p2 / np) > a.cos_angle)) c = CODE_ANGLE;
                    }
                }
            }
            if (c == CODE_SURVIVOR) {
                const double nd = sqrt(dot3(d0, d1, d2, d0, d1, d2));
                r0 = d0 / nd; r1 = d1 / nd; r2 = d2 / nd;
            }
        }
        W.code_l[pl] = c; W.rx[pl] = r0; W.ry[pl] = r1; W.rz[pl] = r2;
        W.code_e[e] = c;
    }
}

// the landmark's survivors, status and "changed" bits from the counts of its codes and the outcome of the pair search
__device__ inline void tf_verdict(const TfArgs &a, int64_t s, int n_surv, int n_depth, int n_rep, int n_ang, bool found, const TfWork &W) {
    const bool used = n_surv + n_depth + n_rep + n_ang > 0;
    const bool rep_on = (a.flags & XM_TF_REPROJECTION) != 0, ang_on = (a.flags & XM_TF_ANGLE) != 0;
    // an observation behind the camera leaves the list in the first per-observation filter that runs (track_filter.cc:20, :70)
    const bool ch_rep = rep_on && (n_rep > 0 || n_depth > 0), ch_ang = ang_on && (n_ang > 0 || (!rep_on && n_depth > 0));
    const bool tri_fail = (a.flags & XM_TF_TRIANGULATION) && used && !found;
    int views = tri_fail ? 0 : n_surv;
    const bool mv_fail = a.min_views > 0 && views > 0 && views < a.min_views;
    if (mv_fail) views = 0;
    W.views[s] = views;
    W.status[s] = (uint8_t)(!used ? XM_TF_LM_UNUSED : tri_fail ? XM_TF_LM_TRIANGULATION : mv_fail ? XM_TF_LM_MIN_VIEWS : XM_TF_LM_KEPT);
    W.lflags[s] = (uint8_t)((used ? LF_USED : 0) | (ch_rep ? LF_REPROJECTION : 0) | (ch_ang ? LF_ANGLE : 0) | (tri_fail ? LF_TRIANGULATION : 0) |
                            (mv_fail ? LF_MIN_VIEWS : 0));
}

// light landmarks: a thread per landmark, its list at base + 64 k
__global__ __launch_bounds__(kT) void tf_light_kernel(SchurLists S, TfArgs a, TfWork W) {
    const int64_t tl = (int64_t)blockIdx.x * kT + threadIdx.x, s = S.nheavy + tl;
    if (s >= S.m) return;
    const int64_t base = S.gbase[tl >> 6] + (tl & 63);
    const int deg = S.deg[s];
    int n_surv = 0, n_depth = 0, n_rep = 0, n_ang = 0;
    for (int k = 0; k < deg; ++k) {
        const int c = W.code_l[base + (int64_t)64 * k];
        n_surv += c == CODE_SURVIVOR; n_depth += c == CODE_DEPTH; n_rep += c == CODE_REPROJECTION; n_ang += c == CODE_ANGLE;
    }
    bool found = false;
    if ((a.flags & XM_TF_TRIANGULATION) && n_surv >= 2) {
        for (int i = 0; i + 1 < deg && !found; ++i) {
            const int64_t pi = base + (int64_t)64 * i;
            const double xi = W.rx[pi], yi = W.ry[pi], zi = W.rz[pi];
            for (int j = i + 1; j < deg; ++j) {
                const int64_t pj = base + (int64_t)64 * j;
                if (dot3(xi, yi, zi, W.rx[pj], W.ry[pj], W.rz[pj]) < a.cos_triangulation) { found = true; break; }
            }
        }
    }
    tf_verdict(a, s, n_surv, n_depth, n_rep, n_ang, found, W);
}

__device__ inline int wave_sum_int(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// heavy landmarks: a workgroup per landmark, its list at [lm_ptr[s], lm_ptr[s + 1])
__global__ __launch_bounds__(kT) void tf_heavy_kernel(SchurLists S, TfArgs a, TfWork W) {
    __shared__ double A[3][kTfTile], B[3][kTfTile];
    __shared__ int cnt[kT / 64][4];
    __shared__ int found;
    const int64_t s = blockIdx.x, b0 = S.lm_ptr[s], len = S.lm_ptr[s + 1] - b0;
    const int tid = (int)threadIdx.x;
    const double nan = __longlong_as_double(-1ll);
    int n[4] = {0, 0, 0, 0};
    for (int64_t k = tid; k < len; k += kT) {
        const int c = W.code_l[b0 + k];
        n[0] += c == CODE_SURVIVOR; n[1] += c == CODE_DEPTH; n[2] += c == CODE_REPROJECTION; n[3] += c == CODE_ANGLE;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        n[k] = wave_sum_int(n[k]);
        if (lane_id() == 0) cnt[tid >> 6][k] = n[k];
    }
    if (tid == 0) found = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        n[k] = 0;
        for (int q = 0; q < kT / 64; ++q) n[k] += cnt[q][k];
    }
    // (n is the same in every thread, and found is only read behind a barrier that follows the last write to it: every branch below that
    // holds a barrier is taken by the whole workgroup)
    if ((a.flags & XM_TF_TRIANGULATION) && n[0] >= 2) {
        const int64_t nt = (len + kTfTile - 1) / kTfTile;
        for (int64_t ta = 0; ta < nt; ++ta) {
            __syncthreads();   // the pair of tiles before this one is done with A and B, and its writes to found have landed
            if (found) break;
            const int64_t ia = ta * kTfTile + tid;
            const double xi = ia < len ? W.rx[b0 + ia] : nan, yi = ia < len ? W.ry[b0 + ia] : nan, zi = ia < len ? W.rz[b0 + ia] : nan;
            A[0][tid] = xi; A[1][tid] = yi; A[2][tid] = zi;
            for (int64_t tb = ta; tb < nt; ++tb) {
                if (tb != ta) {
                    __syncthreads();   // as above, for B
                    if (found) break;
                    const int64_t ib = tb * kTfTile + tid;
                    B[0][tid] = ib < len ? W.rx[b0 + ib] : nan; B[1][tid] = ib < len ? W.ry[b0 + ib] : nan; B[2][tid] = ib < len ? W.rz[b0 + ib] : nan;
                }
                __syncthreads();       // the tile is staged, and every thread has read found: from here on it may be written
                const double(*Bt)[kTfTile] = tb == ta ? A : B;
                const int jn = (int)(len - tb * kTfTile < kTfTile ? len - tb * kTfTile : kTfTile);
                bool hit = false;
                if (xi == xi) {        // (a ray that is NaN pairs with nothing)
                    for (int j = tb == ta ? tid + 1 : 0; j < jn; ++j)
                        if (dot3(xi, yi, zi, Bt[0][j], Bt[1][j], Bt[2][j]) < a.cos_triangulation) { hit = true; break; }
                }
                if (hit) found = 1;
            }
        }
    }
    __syncthreads();
    if (tid == 0) tf_verdict(a, s, n[0], n[1], n[2], n[3], found != 0, W);
}

// keep and reason per observation (input order), the counters per workgroup
__global__ __launch_bounds__(kT) void tf_emit_kernel(SchurLists S, TfWork W, uint8_t *__restrict__ keep, uint8_t *__restrict__ reason, u64 *__restrict__ parts) {
    __shared__ int part[kT / 64][N_PITCH];
    int n[N_COUNT];
#pragma unroll
    for (int k = 0; k < N_COUNT; ++k) n[k] = 0;
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * kT) {
        const int c = W.code_e[e];
        int r = 0;
        if (c == CODE_SURVIVOR) {
            const int st = W.status[S.obs_lm[e]];
            r = st == XM_TF_LM_TRIANGULATION ? XM_TF_REASON_TRIANGULATION : st == XM_TF_LM_MIN_VIEWS ? XM_TF_REASON_MIN_VIEWS : 0;
        } else if (c != CODE_UNUSED) {
            r = c == CODE_DEPTH ? XM_TF_REASON_DEPTH : c == CODE_REPROJECTION ? XM_TF_REASON_REPROJECTION : XM_TF_REASON_ANGLE;
        }
        const bool k = c == CODE_SURVIVOR && r == 0;
        keep[e] = k ? 1 : 0; reason[e] = (uint8_t)r;
        n[N_USED] += c != CODE_UNUSED; n[N_KEPT] += k;
        n[N_DEPTH] += r == XM_TF_REASON_DEPTH; n[N_REPROJECTION] += r == XM_TF_REASON_REPROJECTION; n[N_ANGLE] += r == XM_TF_REASON_ANGLE;
        n[N_TRIANGULATION] += r == XM_TF_REASON_TRIANGULATION; n[N_MIN_VIEWS] += r == XM_TF_REASON_MIN_VIEWS;
    }
    for (int64_t s = (int64_t)blockIdx.x * kT + threadIdx.x; s < S.m; s += (int64_t)gridDim.x * kT) {
        const int f = W.lflags[s];
        n[N_TRACKS] += (f & LF_USED) != 0; n[N_TRACKS_KEPT] += W.views[s] > 0;
        n[N_CH_REPROJECTION] += (f & LF_REPROJECTION) != 0; n[N_CH_ANGLE] += (f & LF_ANGLE) != 0;
        n[N_CH_TRIANGULATION] += (f & LF_TRIANGULATION) != 0; n[N_CH_MIN_VIEWS] += (f & LF_MIN_VIEWS) != 0;
    }
    // (a thread walks at most 2^39 / (4096 * 256) entries of either list: the int counters cannot overflow before the u64 sums below)
#pragma unroll
    for (int k = 0; k < N_COUNT; ++k) {
        const int v = wave_sum_int(n[k]);
        if (lane_id() == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < N_PITCH) {
        u64 v = 0;
        if (threadIdx.x < N_COUNT)
            for (int q = 0; q < kT / 64; ++q) v += (u64)part[q][threadIdx.x];
        parts[(size_t)blockIdx.x * N_PITCH + threadIdx.x] = v;
    }
}
// out[k] = sum over the workgroups of parts[b][k], in a fixed order: 16 threads per counter take every 16th workgroup, then one adds the 16 sums
__global__ __launch_bounds__(kT) void tf_reduce_kernel(int nblocks, const u64 *__restrict__ parts, u64 *__restrict__ out) {
    __shared__ u64 sums[kT];
    const int k = (int)threadIdx.x % N_PITCH, g = (int)threadIdx.x / N_PITCH;
    u64 v = 0;
    for (int b = g; b < nblocks; b += kT / N_PITCH) v += parts[(size_t)b * N_PITCH + k];
    sums[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x < N_PITCH) {
        u64 total = 0;
        for (int q = 0; q < kT / N_PITCH; ++q) total += sums[q * N_PITCH + threadIdx.x];
        out[threadIdx.x] = total;
    }
}

struct Block { u64 cnt[N_PITCH]; };   // what the host reads besides the output arrays

}  // namespace

void filter_tracks(const SchurOp &SO, const TfSettings &cfg, const double *rot, const double *t, const double *p, uint8_t *keep, uint8_t *reason,
                   int32_t *lm_views, uint8_t *lm_status, TfOutcome &out, hipStream_t st) {
    const SchurLists S = SO.lists();
    const std::vector<int32_t> &slot_of = SO.slot_of();
    const int64_t n = S.n, m = S.m, nobs = S.nobs;
    out = TfOutcome();
    if (nobs >= ((int64_t)1 << 39)) throw Error(XM_ERR_ARG, "xm_ctx_filter_tracks: more than 2^39 observations");
    const auto t_kernels = std::chrono::steady_clock::now();
    // the landmarks by slot (the numbering of the device lists); rotations and centres are read as they come
    std::vector<double> hP((size_t)3 * m);
    for (int64_t l = 0; l < m; ++l)
        for (int c = 0; c < 3; ++c) hP[(size_t)3 * slot_of[(size_t)l] + c] = p[(size_t)3 * l + c];
    Pinned<Block> pin;
    DevBuf<double> dR, dT, dP, rays;
    DevBuf<uint8_t> code_l, code_e, status, lflags, dkeep, dreason;
    DevBuf<int32_t> views;
    DevBuf<u64> parts, cnt;
    upload(dR, rot, (size_t)9 * n, st); upload(dT, t, (size_t)3 * n, st); upload(dP, hP.data(), hP.size(), st);
    fresh(rays, (size_t)3 * S.lm_total, 0xff, st);   // NaN: the padding of the packed groups pairs with nothing
    fresh(code_l, (size_t)S.lm_total, 0, st);
    code_e.alloc((size_t)nobs, false); dkeep.alloc((size_t)nobs, false); dreason.alloc((size_t)nobs, false);
    views.alloc((size_t)m, false); status.alloc((size_t)m, false); lflags.alloc((size_t)m, false);
    const unsigned ge = grid_for(std::max(nobs, m), 4096);
    parts.alloc((size_t)ge * N_PITCH, false); cnt.alloc(N_PITCH, false);
    TfArgs a;
    a.flags = cfg.flags; a.min_views = cfg.min_views; a.thr_reprojection = cfg.max_reprojection_error; a.cos_angle = cfg.cos_angle;
    a.cos_triangulation = cfg.cos_triangulation;
    TfWork W;
    W.code_l = code_l.p; W.code_e = code_e.p; W.rx = rays.p; W.ry = rays.p + S.lm_total; W.rz = rays.p + 2 * S.lm_total;
    W.views = views.p; W.status = status.p; W.lflags = lflags.p;
    try {
        if (nobs > 0) {
            hipLaunchKernelGGL(tf_obs_kernel, dim3(grid_for(nobs, 4096)), dim3(kT), 0, st, S, a, (const double *)dR.p, (const double *)dT.p,
                               (const double *)dP.p, W);
            check_launch("tf_obs_kernel");
        }
        if (S.nheavy > 0) {
            hipLaunchKernelGGL(tf_heavy_kernel, dim3((unsigned)S.nheavy), dim3(kT), 0, st, S, a, W);
            check_launch("tf_heavy_kernel");
        }
        if (m > S.nheavy) {
            hipLaunchKernelGGL(tf_light_kernel, dim3(grid_of(m - S.nheavy)), dim3(kT), 0, st, S, a, W);
            check_launch("tf_light_kernel");
        }
        hipLaunchKernelGGL(tf_emit_kernel, dim3(ge), dim3(kT), 0, st, S, W, dkeep.p, dreason.p, parts.p);
        check_launch("tf_emit_kernel");
        hipLaunchKernelGGL(tf_reduce_kernel, dim3(1), dim3(kT), 0, st, (int)ge, (const u64 *)parts.p, cnt.p);
        check_launch("tf_reduce_kernel");
        XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt.p, N_PITCH * sizeof(u64), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the verdicts");
        out.seconds_kernels = secs_since(t_kernels);
        const auto t_down = std::chrono::steady_clock::now();
        std::vector<int32_t> hviews((size_t)m);
        std::vector<uint8_t> hstatus((size_t)m);
        if (nobs > 0) {
            XM_HIP_CHECK(hipMemcpyAsync(keep, dkeep.p, (size_t)nobs, hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(reason, dreason.p, (size_t)nobs, hipMemcpyDeviceToHost, st));
        }
        if (m > 0) {
            XM_HIP_CHECK(hipMemcpyAsync(hviews.data(), views.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(hstatus.data(), status.p, (size_t)m, hipMemcpyDeviceToHost, st));
        }
        wait_stream(st, cfg.watchdog_s, kStage, "the download");
        for (int64_t l = 0; l < m; ++l) {
            lm_views[l] = hviews[(size_t)slot_of[(size_t)l]];
            lm_status[l] = hstatus[(size_t)slot_of[(size_t)l]];
        }
        out.seconds_download = secs_since(t_down);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the buffers above are freed next: nothing may still be reading them
        throw;
    }
    const u64 *c = pin.h->cnt;
    out.obs_used = (int64_t)c[N_USED]; out.obs_kept = (int64_t)c[N_KEPT]; out.tracks_total = (int64_t)c[N_TRACKS]; out.tracks_kept = (int64_t)c[N_TRACKS_KEPT];
    out.dropped_depth = (int64_t)c[N_DEPTH]; out.dropped_reprojection = (int64_t)c[N_REPROJECTION]; out.dropped_angle = (int64_t)c[N_ANGLE];
    out.dropped_triangulation = (int64_t)c[N_TRIANGULATION]; out.dropped_min_views = (int64_t)c[N_MIN_VIEWS];
    out.changed_reprojection = (int64_t)c[N_CH_REPROJECTION]; out.changed_angle = (int64_t)c[N_CH_ANGLE];
    out.changed_triangulation = (int64_t)c[N_CH_TRIANGULATION]; out.changed_min_views = (int64_t)c[N_CH_MIN_VIEWS];
    if (out.obs_kept + out.dropped_depth + out.dropped_reprojection + out.dropped_angle + out.dropped_triangulation + out.dropped_min_views != out.obs_used)
        throw Error(XM_ERR_HIP, "track filter: the kept and the dropped observations do not add up to the used ones");
}

}  // namespace xm
