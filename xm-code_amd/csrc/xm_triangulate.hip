// xm_triangulate.hip — landmarks from 2-D tracks at given poses (xm_triangulate.h has the design; definition in include/xm_amd.h at
// xm_ctx_triangulate_tracks).
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/xm_amd.h"
#include "xm_triangulate.h"
#include "xm_stage.h"

// every product and every sum of the contract is rounded on its own
#pragma clang fp contract(off)

namespace xm {
namespace {

constexpr int kT = kTriThreads;
constexpr int kWaves = kT / 64;
static_assert(kT == kStageThreads && kTriTile == kT && kWaves == 4, "a thread per ray of a tile, four wavefronts per tile; the helpers of xm_stage.h are written for this workgroup size");
static_assert(kSchurHeavy == 64, "tri_light_kernel holds a light landmark's list in one wavefront, a ray per lane");
constexpr const char *kStage = "triangulation";
constexpr double kEps = 1e-12;   // the depth bound of xm_ctx_filter_tracks
constexpr int kLevels = 40;      // levels of the tree over a heavy landmark's tiles: 2^40 tiles

// bits of an observation's flag byte (input order)
enum { OF_CANDIDATE = 1, OF_WEIGHT = 2, OF_USED = 4 };
// slots of the counters (per workgroup, then summed)
enum { N_LM0 = 0, N_CANDIDATES = 6, N_KEPT, N_READMITTED, N_LOST, N_TESTED, N_SCORED, N_COUNT, N_PITCH = 16 };
static_assert(N_COUNT <= N_PITCH && XM_TRI_LM_ANGLE == 5, "the reduction walks N_PITCH counters per workgroup, six of them the landmark statuses");

struct TriArgs {
    int32_t max_hypotheses, refine_rounds, min_views;
    double cos_min, cos_create, thr;
};
struct TriWork {   // device arrays of one call
    double *bx, *by, *bz, *u, *v;       // lm_total each, by list position
    uint8_t *cand_l, *mem_l;            // lm_total
    uint8_t *flag_e;                    // nobs
    uint8_t *status;                    // per landmark slot, as everything below
    int32_t *views, *support, *hyp;
    int64_t *tested, *scored;
    double *X;                          // 3 per slot
};

__device__ inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
__device__ inline double nan_value() { return __longlong_as_double(-1ll); }

// the midpoint of the closest points of the rays c1 + s b1 and c2 + t b2; false when the pair is no hypothesis
__device__ inline bool two_view(const double *b1, const double *c1, const double *b2, const double *c2, double cos_min, double *X) {
    const double cs = dot3(b1[0], b1[1], b1[2], b2[0], b2[1], b2[2]);
    const double w0 = c2[0] - c1[0], w1 = c2[1] - c1[1], w2 = c2[2] - c1[2];
    const double d1 = dot3(b1[0], b1[1], b1[2], w0, w1, w2), d2 = dot3(b2[0], b2[1], b2[2], w0, w1, w2);
    const double den = 1.0 - cs * cs;
    const double s = (d1 - cs * d2) / den, t = (cs * d1 - d2) / den;
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = 0.5 * ((c1[k] + s * b1[k]) + (c2[k] + t * b2[k]));
    return cs < cos_min && den > 0.0 && s > 0.0 && t > 0.0;
}
__device__ inline bool supports(double X0, double X1, double X2, const double *c, const double *b, double cos_create) {
    const double d0 = X0 - c[0], d1 = X1 - c[1], d2 = X2 - c[2];
    return dot3(d0, d1, d2, b[0], b[1], b[2]) / sqrt(dot3(d0, d1, d2, d0, d1, d2)) > cos_create;
}
// one ray's terms of A = sum (I - b b^T) (00, 01, 02, 11, 12, 22) and r = sum (I - b b^T) c; none of them is -0.0
__device__ inline void ray_terms(const double *b, const double *c, double *v) {
    const double sc = dot3(b[0], b[1], b[2], c[0], c[1], c[2]);
    v[0] = 1.0 - b[0] * b[0]; v[1] = 0.0 - b[0] * b[1]; v[2] = 0.0 - b[0] * b[2];
    v[3] = 1.0 - b[1] * b[1]; v[4] = 0.0 - b[1] * b[2]; v[5] = 1.0 - b[2] * b[2];
    v[6] = (c[0] - b[0] * sc) + 0.0; v[7] = (c[1] - b[1] * sc) + 0.0; v[8] = (c[2] - b[2] * sc) + 0.0;
}
// X = A^-1 r by the adjugate; false when the determinant is not finite and positive
__device__ inline bool solve3(const double *S, double *X) {
    const double A00 = S[0], A01 = S[1], A02 = S[2], A11 = S[3], A12 = S[4], A22 = S[5], r0 = S[6], r1 = S[7], r2 = S[8];
    const double k00 = A11 * A22 - A12 * A12, k01 = A02 * A12 - A01 * A22, k02 = A01 * A12 - A02 * A11;
    const double k11 = A00 * A22 - A02 * A02, k12 = A01 * A02 - A00 * A12, k22 = A00 * A11 - A01 * A01;
    const double det = (A00 * k00 + A01 * k01) + A02 * k02;
    X[0] = ((k00 * r0 + k01 * r1) + k02 * r2) / det; X[1] = ((k01 * r0 + k11 * r1) + k12 * r2) / det; X[2] = ((k02 * r0 + k12 * r1) + k22 * r2) / det;
    return det > 0.0 && det < __longlong_as_double(0x7ff0000000000000ll);
}
// the completion test of one candidate: depth and reprojection error at X (the formulas of XM_TF_REPROJECTION)
__device__ inline bool is_member(const double *X, const double *T, const double *R, double u, double v, double thr) {
    const double d0 = X[0] - T[0], d1 = X[1] - T[1], d2 = X[2] - T[2];
    const double q0 = dot3(R[0], R[1], R[2], d0, d1, d2), q1 = dot3(R[3], R[4], R[5], d0, d1, d2), q2 = dot3(R[6], R[7], R[8], d0, d1, d2);
    if (!(q2 >= kEps)) return false;
    const double uu = q0 / q2 - u, vv = q1 / q2 - v;
    return sqrt(uu * uu + vv * vv) < thr;
}

// rot: 9 doubles per camera, column a of R_i at 9 i + 3 a; t: 3 per camera; candidate: nobs bytes or null (the used observations)
__global__ __launch_bounds__(kT) void tri_obs_kernel(SchurLists S, const double *__restrict__ rot, const uint8_t *__restrict__ candidate, TriWork W) {
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * kT) {
        const int64_t pl = S.dpos_l[e];
        const double w = S.cam_w[S.pos_c[e]], p0 = S.obs_p[3 * e], p1 = S.obs_p[3 * e + 1], p2 = S.obs_p[3 * e + 2];
        const bool cand = (candidate ? candidate[e] != 0 : w > 0.0) && p2 > 0.0;
        if (cand) {
            const double *R = rot + (size_t)9 * S.obs_cam[e];
            const double u = p0 / p2, v = p1 / p2;
            const double g0 = (R[0] * u + R[3] * v) + R[6], g1 = (R[1] * u + R[4] * v) + R[7], g2 = (R[2] * u + R[5] * v) + R[8];
            const double ng = sqrt(dot3(g0, g1, g2, g0, g1, g2));
            W.bx[pl] = g0 / ng; W.by[pl] = g1 / ng; W.bz[pl] = g2 / ng; W.u[pl] = u; W.v[pl] = v;
            W.cand_l[pl] = 1;
        }
        W.flag_e[e] = (uint8_t)((cand ? OF_CANDIDATE : 0) | (w > 0.0 ? OF_WEIGHT : 0) | (w > 0.0 && p2 > 0.0 ? OF_USED : 0));
    }
}

__device__ inline void tri_verdict(const TriWork &W, int64_t s, int status, int views, int support, int hyp, const double *X, int64_t tested, int64_t scored) {
    W.status[s] = (uint8_t)status; W.views[s] = views; W.support[s] = support; W.hyp[s] = hyp; W.tested[s] = tested; W.scored[s] = scored;
    if (status == XM_TRI_LM_ACCEPTED) { W.X[3 * s] = X[0]; W.X[3 * s + 1] = X[1]; W.X[3 * s + 2] = X[2]; }
}

// the value of a wavefront-uniform lane
__device__ inline double bcast(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
// the pairwise tree over the 64 lanes, adjacent pairs first; every lane gets the sum
__device__ inline double wave_tree(double v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// light landmarks: a wavefront per landmark, lane k holds the ray at gbase + 64 k + j
__global__ __launch_bounds__(kT) void tri_light_kernel(SchurLists S, TriArgs a, const double *__restrict__ rot, const double *__restrict__ t, TriWork W) {
    const int64_t tl = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), s = S.nheavy + tl;
    if (s >= S.m) return;   // (whole wavefronts leave; the kernel has no barrier)
    const int lane = lane_id(), L = S.deg[s];
    const int64_t pos = S.gbase[tl >> 6] + (tl & 63) + (int64_t)64 * lane;
    const double nan = nan_value();
    double b[3] = {nan, nan, nan}, c[3] = {0.0, 0.0, 0.0}, ou = 0.0, ov = 0.0, X[3] = {0.0, 0.0, 0.0};
    const double *R = rot;
    bool cand = false;
    if (lane < L) {
        cand = W.cand_l[pos] != 0;
        if (cand) {
            const int cam = S.lm_cam[pos];
            b[0] = W.bx[pos]; b[1] = W.by[pos]; b[2] = W.bz[pos]; ou = W.u[pos]; ov = W.v[pos];
            c[0] = t[(size_t)3 * cam]; c[1] = t[(size_t)3 * cam + 1]; c[2] = t[(size_t)3 * cam + 2];
            R = rot + (size_t)9 * cam;
        }
    }
    const int ncand = __popcll(__ballot(cand));
    if (ncand < 2) {
        if (lane == 0) tri_verdict(W, s, ncand == 0 ? XM_TRI_LM_UNUSED : XM_TRI_LM_NO_HYPOTHESIS, 0, 0, -1, X, 0, 0);
        return;
    }
    const int H = min(a.max_hypotheses, L * (L - 1) / 2);
    int best = -1, best_h = -1, scored = 0;
    u64 best_mask = 0;
    for (int h = 0, d = 1, pa = 0; h < H; ++h) {
        const int pb = pa + d >= L ? pa + d - L : pa + d;
        double b1[3], c1[3], b2[3], c2[3], Y[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { b1[k] = bcast(b[k], pa); c1[k] = bcast(c[k], pa); b2[k] = bcast(b[k], pb); c2[k] = bcast(c[k], pb); }
        if (two_view(b1, c1, b2, c2, a.cos_min, Y)) {   // (the same in every lane)
            const u64 mask = __ballot(supports(Y[0], Y[1], Y[2], c, b, a.cos_create));
            const int n = __popcll(mask);
            ++scored;
            if (n > best) { best = n; best_h = h; best_mask = mask; X[0] = Y[0]; X[1] = Y[1]; X[2] = Y[2]; }
        }
        if (++pa == L) { pa = 0; ++d; }
    }
    if (best < 2) {
        if (lane == 0) tri_verdict(W, s, XM_TRI_LM_NO_HYPOTHESIS, 0, best < 0 ? 0 : best, best_h, X, H, scored);
        return;
    }
    bool mem = (best_mask >> lane) & 1ull;
    int status = XM_TRI_LM_ACCEPTED;
    for (int round = 0; round < a.refine_rounds; ++round) {
        if (__popcll(__ballot(mem)) < 2) { status = XM_TRI_LM_MIN_VIEWS; break; }
        double v[9], sum[9];
        if (mem) ray_terms(b, c, v);
#pragma unroll
        for (int k = 0; k < 9; ++k) sum[k] = wave_tree(mem ? v[k] : 0.0);
        if (!solve3(sum, X)) { status = XM_TRI_LM_DEGENERATE; break; }
        mem = cand && is_member(X, c, R, ou, ov, a.thr);
    }
    const u64 members = __ballot(mem);
    int views = __popcll(members);
    if (status == XM_TRI_LM_ACCEPTED && views < max(a.min_views, 2)) status = XM_TRI_LM_MIN_VIEWS;
    if (status == XM_TRI_LM_ACCEPTED) {
        bool found = false;
        for (u64 left = members; left && !found; left &= left - 1) {
            const int i = __ffsll((long long)left) - 1;
            const double x = bcast(b[0], i), y = bcast(b[1], i), z = bcast(b[2], i);
            found = __ballot(mem && lane > i && dot3(x, y, z, b[0], b[1], b[2]) < a.cos_min) != 0;
        }
        if (!found) status = XM_TRI_LM_ANGLE;
    }
    if (status != XM_TRI_LM_ACCEPTED) views = 0;
    if (lane == 0) tri_verdict(W, s, status, views, best, best_h, X, H, scored);
    if (status == XM_TRI_LM_ACCEPTED && lane < L) W.mem_l[pos] = mem ? 1 : 0;
}

__device__ inline long long wave_sum_ll(long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// the workgroup's sum / maximum in every thread; lds: one entry per wavefront; begins and ends behind a barrier of its own
__device__ inline long long block_sum(long long v, long long *lds) {
    v = wave_sum_ll(v);
    __syncthreads();
    if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}
__device__ inline u64 block_max(u64 v, u64 *lds) {
    v = wave_max(v);
    __syncthreads();
    if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const u64 x = lds[0] > lds[1] ? lds[0] : lds[1], y = lds[2] > lds[3] ? lds[2] : lds[3];
    return x > y ? x : y;
}

// heavy landmarks: a workgroup per landmark, its list at [lm_ptr[s], lm_ptr[s + 1]).  Every branch that holds a barrier is taken by the
// whole workgroup: the values it depends on are the same in every thread.
__global__ __launch_bounds__(kT) void tri_heavy_kernel(SchurLists S, TriArgs a, const double *__restrict__ rot, const double *__restrict__ t, TriWork W) {
    __shared__ double hX[3][kTriTile], A[3][kTriTile], B[3][kTriTile];
    __shared__ int wcnt[kWaves][kTriTile];
    __shared__ double wsum[kWaves][9], stack[9][kLevels], tot[9];
    __shared__ long long red[kWaves];
    __shared__ u64 redk[kWaves];
    __shared__ int found;
    const int64_t s = blockIdx.x, b0 = S.lm_ptr[s], len = S.lm_ptr[s + 1] - b0;
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const double nan = nan_value();
    double X[3] = {0.0, 0.0, 0.0};
    auto load_ray = [&](int64_t k, double *b, double *c) {   // position k of the list (a non-candidate's ray is NaN in memory)
        const int cam = S.lm_cam[b0 + k];
        b[0] = W.bx[b0 + k]; b[1] = W.by[b0 + k]; b[2] = W.bz[b0 + k];
        c[0] = t[(size_t)3 * cam]; c[1] = t[(size_t)3 * cam + 1]; c[2] = t[(size_t)3 * cam + 2];
    };
    long long mine = 0;
    for (int64_t k = tid; k < len; k += kT) mine += W.cand_l[b0 + k] != 0;
    const long long ncand = block_sum(mine, red);
    if (ncand < 2) {
        if (tid == 0) tri_verdict(W, s, ncand == 0 ? XM_TRI_LM_UNUSED : XM_TRI_LM_NO_HYPOTHESIS, 0, 0, -1, X, 0, 0);
        return;
    }
    const int64_t npairs = len * (len - 1) / 2, H = npairs < a.max_hypotheses ? npairs : a.max_hypotheses;
    auto hypothesis = [&](int64_t h, double *Y) {   // entry h of the schedule: d = h / L + 1, a = h - (d - 1) L, b = (a + d) mod L
        const int64_t d = h / len + 1, pa = h - (d - 1) * len, pb = pa + d >= len ? pa + d - len : pa + d;
        double b1[3], c1[3], b2[3], c2[3];
        load_ray(pa, b1, c1); load_ray(pb, b2, c2);
        return two_view(b1, c1, b2, c2, a.cos_min, Y);
    };
    u64 best_key = 0;
    mine = 0;
    for (int64_t h0 = 0; h0 < H; h0 += kTriTile) {
        const int nh = (int)(H - h0 < kTriTile ? H - h0 : kTriTile);
        double Y[3] = {nan, nan, nan};
        bool valid = false;
        if (tid < nh) {
            valid = hypothesis(h0 + tid, Y);
            if (!valid) Y[0] = Y[1] = Y[2] = nan;   // (supports nothing)
        }
        mine += valid;
        __syncthreads();   // the batch before this one is done with hX and wcnt
        hX[0][tid] = Y[0]; hX[1][tid] = Y[1]; hX[2][tid] = Y[2];
        __syncthreads();
        int cnt[4] = {0, 0, 0, 0};
        for (int64_t k0 = 0; k0 < len; k0 += kTriTile) {
            double b[3] = {nan, nan, nan}, c[3] = {0.0, 0.0, 0.0};
            if (k0 + tid < len) load_ray(k0 + tid, b, c);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int jn = nh - 64 * q < 64 ? nh - 64 * q : 64;
                for (int j = 0; j < jn; ++j) {
                    const int hh = 64 * q + j;
                    const int n = __popcll(__ballot(supports(hX[0][hh], hX[1][hh], hX[2][hh], c, b, a.cos_create)));
                    if (lane == j) cnt[q] += n;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) wcnt[wave][64 * q + lane] = cnt[q];
        __syncthreads();
        const int total = (wcnt[0][tid] + wcnt[1][tid]) + (wcnt[2][tid] + wcnt[3][tid]);
        // the highest count wins, among equals the earliest schedule index (H < 2^31: max_hypotheses is an int32)
        const u64 key = valid ? ((u64)(total + 1) << 32) | (u64)(0x7fffffffll - (h0 + tid)) : 0ull;
        const u64 top = block_max(key, redk);
        best_key = top > best_key ? top : best_key;
    }
    const long long scored = block_sum(mine, red);
    const int best = (int)(best_key >> 32) - 1, best_h = best_key ? (int)(0x7fffffffll - (int64_t)(best_key & 0xffffffffull)) : -1;
    if (best < 2) {
        if (tid == 0) tri_verdict(W, s, XM_TRI_LM_NO_HYPOTHESIS, 0, best < 0 ? 0 : best, best_h, X, H, scored);
        return;
    }
    hypothesis(best_h, X);   // (the same operations as in its batch: the same point)
    mine = 0;
    for (int64_t k = tid; k < len; k += kT) {
        double b[3], c[3];
        load_ray(k, b, c);
        const bool mem = supports(X[0], X[1], X[2], c, b, a.cos_create);
        W.mem_l[b0 + k] = mem ? 1 : 0;
        mine += mem;
    }
    long long views = block_sum(mine, red);
    int status = XM_TRI_LM_ACCEPTED;
    const int64_t nt = (len + kTriTile - 1) / kTriTile;
    for (int round = 0; round < a.refine_rounds; ++round) {
        if (views < 2) { status = XM_TRI_LM_MIN_VIEWS; break; }
        for (int64_t j = 0; j < nt; ++j) {
            const int64_t k = j * kTriTile + tid;
            double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (k < len && W.mem_l[b0 + k]) {
                double b[3], c[3];
                load_ray(k, b, c);
                ray_terms(b, c, v);
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) v[i] = wave_tree(v[i]);
            __syncthreads();   // the tile before this one is done with wsum
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) wsum[wave][i] = v[i];
            }
            __syncthreads();
            if (tid < 9) {     // the tile's sum, then a binary counter over the tiles: level l holds the sum of 2^l whole tiles
                double carry = (wsum[0][tid] + wsum[1][tid]) + (wsum[2][tid] + wsum[3][tid]);
                int lvl = 0;
                for (; (j >> lvl) & 1; ++lvl) carry = stack[tid][lvl] + carry;
                stack[tid][lvl] = carry;
            }
        }
        if (tid < 9) {         // the levels that are set in nt, lowest first: what is missing to the power of two is +0.0
            double acc = 0.0;
            bool have = false;
            for (int lvl = 0; lvl < kLevels; ++lvl)
                if ((nt >> lvl) & 1) { acc = have ? stack[tid][lvl] + acc : stack[tid][lvl]; have = true; }
            tot[tid] = acc;
        }
        __syncthreads();
        double sum[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) sum[i] = tot[i];
        if (!solve3(sum, X)) { status = XM_TRI_LM_DEGENERATE; break; }
        mine = 0;
        for (int64_t k = tid; k < len; k += kT) {
            bool mem = false;
            if (W.cand_l[b0 + k]) {
                const int cam = S.lm_cam[b0 + k];
                mem = is_member(X, t + (size_t)3 * cam, rot + (size_t)9 * cam, W.u[b0 + k], W.v[b0 + k], a.thr);
            }
            W.mem_l[b0 + k] = mem ? 1 : 0;
            mine += mem;
        }
        views = block_sum(mine, red);   // (its barriers also stand between this round's reads of tot and the next one's writes)
    }
    if (status == XM_TRI_LM_ACCEPTED && views < (a.min_views > 2 ? a.min_views : 2)) status = XM_TRI_LM_MIN_VIEWS;
    if (status == XM_TRI_LM_ACCEPTED) {
        // some pair of members below the cosine: every pair of tiles (ta, tb >= ta) once, as in tf_heavy_kernel
        if (tid == 0) found = 0;
        auto member_ray = [&](int64_t k, double *r) {
            const bool in = k < len && W.mem_l[b0 + k];
            r[0] = in ? W.bx[b0 + k] : nan; r[1] = in ? W.by[b0 + k] : nan; r[2] = in ? W.bz[b0 + k] : nan;
        };
        for (int64_t ta = 0; ta < nt; ++ta) {
            __syncthreads();   // the pair of tiles before this one is done with A and B, and its writes to found have landed
            if (found) break;
            double r[3];
            member_ray(ta * kTriTile + tid, r);
            A[0][tid] = r[0]; A[1][tid] = r[1]; A[2][tid] = r[2];
            for (int64_t tb = ta; tb < nt; ++tb) {
                if (tb != ta) {
                    __syncthreads();   // as above, for B
                    if (found) break;
                    double q[3];
                    member_ray(tb * kTriTile + tid, q);
                    B[0][tid] = q[0]; B[1][tid] = q[1]; B[2][tid] = q[2];
                }
                __syncthreads();       // the tile is staged, and every thread has read found: from here on it may be written
                const double(*Bt)[kTriTile] = tb == ta ? A : B;
                const int jn = (int)(len - tb * kTriTile < kTriTile ? len - tb * kTriTile : kTriTile);
                bool hit = false;
                if (r[0] == r[0]) {    // (a ray that is NaN pairs with nothing)
                    for (int j = tb == ta ? tid + 1 : 0; j < jn; ++j)
                        if (dot3(r[0], r[1], r[2], Bt[0][j], Bt[1][j], Bt[2][j]) < a.cos_min) { hit = true; break; }
                }
                if (hit) found = 1;
            }
        }
        __syncthreads();
        if (!found) status = XM_TRI_LM_ANGLE;
    }
    if (tid == 0) tri_verdict(W, s, status, status == XM_TRI_LM_ACCEPTED ? (int)views : 0, best, best_h, X, H, scored);
}

__device__ inline u64 wave_sum_u64(u64 v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// keep and reason per observation (input order), the counters per workgroup
__global__ __launch_bounds__(kT) void tri_emit_kernel(SchurLists S, TriWork W, uint8_t *__restrict__ keep, uint8_t *__restrict__ reason, u64 *__restrict__ parts) {
    __shared__ u64 part[kWaves][N_PITCH];
    u64 n[N_COUNT];
#pragma unroll
    for (int k = 0; k < N_COUNT; ++k) n[k] = 0;
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < S.nobs; e += (int64_t)gridDim.x * kT) {
        const int f = W.flag_e[e];
        const bool cand = (f & OF_CANDIDATE) != 0, accepted = W.status[S.obs_lm[e]] == XM_TRI_LM_ACCEPTED;
        const bool k = cand && accepted && W.mem_l[S.dpos_l[e]] != 0;
        keep[e] = k ? 1 : 0;
        reason[e] = (uint8_t)(!cand ? XM_TRI_REASON_NOT_CANDIDATE : k ? 0 : accepted ? XM_TRI_REASON_NOT_MEMBER : XM_TRI_REASON_LANDMARK);
        n[N_CANDIDATES] += cand; n[N_KEPT] += k; n[N_READMITTED] += k && !(f & OF_WEIGHT); n[N_LOST] += (f & OF_USED) && !k;
    }
    for (int64_t s = (int64_t)blockIdx.x * kT + threadIdx.x; s < S.m; s += (int64_t)gridDim.x * kT) {
        const int st = W.status[s];
#pragma unroll
        for (int k = 0; k < 6; ++k) n[N_LM0 + k] += st == k;
        n[N_TESTED] += (u64)W.tested[s]; n[N_SCORED] += (u64)W.scored[s];
    }
#pragma unroll
    for (int k = 0; k < N_COUNT; ++k) {
        const u64 v = wave_sum_u64(n[k]);
        if (lane_id() == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < N_PITCH) {
        u64 v = 0;
        if (threadIdx.x < N_COUNT)
            for (int q = 0; q < kWaves; ++q) v += part[q][threadIdx.x];
        parts[(size_t)blockIdx.x * N_PITCH + threadIdx.x] = v;
    }
}
// out[k] = sum over the workgroups of parts[b][k], in a fixed order: 16 threads per counter take every 16th workgroup, then one adds the 16 sums
__global__ __launch_bounds__(kT) void tri_reduce_kernel(int nblocks, const u64 *__restrict__ parts, u64 *__restrict__ out) {
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

void triangulate_tracks(const SchurOp &SO, const TriSettings &cfg, const double *rot, const double *t, double *p, const uint8_t *candidate,
                        uint8_t *keep, uint8_t *reason, int32_t *lm_views, uint8_t *lm_status, int32_t *lm_support, int32_t *lm_hypothesis,
                        TriOutcome &out, hipStream_t st) {
    const SchurLists S = SO.lists();
    const std::vector<int32_t> &slot_of = SO.slot_of();
    const int64_t n = S.n, m = S.m, nobs = S.nobs;
    out = TriOutcome();
    if (nobs >= ((int64_t)1 << 31)) throw Error(XM_ERR_ARG, "xm_ctx_triangulate_tracks: more than 2^31 observations");
    const auto t_kernels = std::chrono::steady_clock::now();
    Pinned<Block> pin;
    DevBuf<double> dR, dT, planes, dX;
    DevBuf<uint8_t> dcand, cand_l, mem_l, flag_e, status, dkeep, dreason;
    DevBuf<int32_t> views, support, hyp;
    DevBuf<int64_t> tested, scored;
    DevBuf<u64> parts, cnt;
    upload(dR, rot, (size_t)9 * n, st); upload(dT, t, (size_t)3 * n, st);
    if (candidate) upload(dcand, candidate, (size_t)nobs, st);
    fresh(planes, (size_t)5 * S.lm_total, 0xff, st);   // NaN: a non-candidate and the padding of the packed groups support nothing
    fresh(cand_l, (size_t)S.lm_total, 0, st); fresh(mem_l, (size_t)S.lm_total, 0, st);
    flag_e.alloc((size_t)nobs, false); dkeep.alloc((size_t)nobs, false); dreason.alloc((size_t)nobs, false);
    status.alloc((size_t)m, false); views.alloc((size_t)m, false); support.alloc((size_t)m, false); hyp.alloc((size_t)m, false);
    tested.alloc((size_t)m, false); scored.alloc((size_t)m, false); dX.alloc((size_t)3 * m, false);
    const unsigned ge = grid_for(std::max(nobs, m), 4096);
    parts.alloc((size_t)ge * N_PITCH, false); cnt.alloc(N_PITCH, false);
    TriArgs a;
    a.max_hypotheses = cfg.max_hypotheses; a.refine_rounds = cfg.refine_rounds; a.min_views = cfg.min_views;
    a.cos_min = cfg.cos_min_angle; a.cos_create = cfg.cos_create; a.thr = cfg.complete_max_reproj_error;
    TriWork W;
    W.bx = planes.p; W.by = planes.p + S.lm_total; W.bz = planes.p + 2 * S.lm_total; W.u = planes.p + 3 * S.lm_total; W.v = planes.p + 4 * S.lm_total;
    W.cand_l = cand_l.p; W.mem_l = mem_l.p; W.flag_e = flag_e.p; W.status = status.p; W.views = views.p; W.support = support.p; W.hyp = hyp.p;
    W.tested = tested.p; W.scored = scored.p; W.X = dX.p;
    try {
        if (nobs > 0) {
            hipLaunchKernelGGL(tri_obs_kernel, dim3(grid_for(nobs, 4096)), dim3(kT), 0, st, S, (const double *)dR.p,
                               candidate ? (const uint8_t *)dcand.p : (const uint8_t *)nullptr, W);
            check_launch("tri_obs_kernel");
        }
        if (S.nheavy > 0) {
            hipLaunchKernelGGL(tri_heavy_kernel, dim3((unsigned)S.nheavy), dim3(kT), 0, st, S, a, (const double *)dR.p, (const double *)dT.p, W);
            check_launch("tri_heavy_kernel");
        }
        if (m > S.nheavy) {
            hipLaunchKernelGGL(tri_light_kernel, dim3((unsigned)((m - S.nheavy + kWaves - 1) / kWaves)), dim3(kT), 0, st, S, a, (const double *)dR.p,
                               (const double *)dT.p, W);
            check_launch("tri_light_kernel");
        }
        hipLaunchKernelGGL(tri_emit_kernel, dim3(ge), dim3(kT), 0, st, S, W, dkeep.p, dreason.p, parts.p);
        check_launch("tri_emit_kernel");
        hipLaunchKernelGGL(tri_reduce_kernel, dim3(1), dim3(kT), 0, st, (int)ge, (const u64 *)parts.p, cnt.p);
        check_launch("tri_reduce_kernel");
        XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt.p, N_PITCH * sizeof(u64), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the landmarks");
        out.seconds_kernels = secs_since(t_kernels);
        const auto t_down = std::chrono::steady_clock::now();
        std::vector<int32_t> hviews((size_t)m), hsupport((size_t)m), hhyp((size_t)m);
        std::vector<uint8_t> hstatus((size_t)m);
        std::vector<double> hX((size_t)3 * m);
        if (nobs > 0) {
            XM_HIP_CHECK(hipMemcpyAsync(keep, dkeep.p, (size_t)nobs, hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(reason, dreason.p, (size_t)nobs, hipMemcpyDeviceToHost, st));
        }
        if (m > 0) {
            XM_HIP_CHECK(hipMemcpyAsync(hviews.data(), views.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(hsupport.data(), support.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(hhyp.data(), hyp.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(hstatus.data(), status.p, (size_t)m, hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(hX.data(), dX.p, (size_t)3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        wait_stream(st, cfg.watchdog_s, kStage, "the download");
        for (int64_t l = 0; l < m; ++l) {
            const size_t sl = (size_t)slot_of[(size_t)l];
            lm_views[l] = hviews[sl]; lm_status[l] = hstatus[sl]; lm_support[l] = hsupport[sl]; lm_hypothesis[l] = hhyp[sl];
            if (hstatus[sl] == XM_TRI_LM_ACCEPTED)   // (a rejected or unused landmark's column stays as it came)
                for (int c = 0; c < 3; ++c) p[(size_t)3 * l + c] = hX[3 * sl + c];
        }
        out.seconds_download = secs_since(t_down);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the buffers above are freed next: nothing may still be reading them
        throw;
    }
    const u64 *c = pin.h->cnt;
    for (int k = 0; k < 6; ++k) out.lm[k] = (int64_t)c[N_LM0 + k];
    out.obs_candidates = (int64_t)c[N_CANDIDATES]; out.obs_kept = (int64_t)c[N_KEPT]; out.obs_readmitted = (int64_t)c[N_READMITTED];
    out.obs_lost = (int64_t)c[N_LOST]; out.pairs_tested = (int64_t)c[N_TESTED]; out.hypotheses_scored = (int64_t)c[N_SCORED];
    int64_t lms = 0;
    for (int k = 0; k < 6; ++k) lms += out.lm[k];
    if (lms != m || out.obs_kept > out.obs_candidates) throw Error(XM_ERR_HIP, "triangulation: the counters do not add up");
}

}  // namespace xm
