// xm_viewgraph.hip — two-view match verification and view-graph pruning on the device (xm_viewgraph.h; definition in include/xm_amd.h at
// xm_view_graph_filter).
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "xm_viewgraph.h"
#include "xm_stage.h"

// every product and every sum of the contract is rounded on its own
#pragma clang fp contract(off)

namespace xm {
namespace {

constexpr int kT = kVgThreads;
constexpr int kWaves = kT / 64;
static_assert(kT == kStageThreads && kVgGroupMatches % kT == 0 && kVgWaveMatches % 64 == 0, "the sweeps run whole tiles, the helpers of xm_stage.h this workgroup size");
constexpr const char *kStage = "view graph";

// what the scoring does with a pair (set on the host from the flag, valid_in and the model)
enum { MD_ZERO = 0, MD_ONES, MD_E, MD_F, MD_H };
// slots of the device counter block
enum { C_STATUS = 0, C_MODEL = 6, C_INLIERS = 10, C_MOUT, C_COUNT };
// slots of the result of vg_largest_kernel
enum { B_LABEL = 0, B_SIZE, B_COMPONENTS, B_COUNT };

__device__ inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// rule 0, for the features of the images that a scored E pair touches
__global__ __launch_bounds__(kT) void vg_bearing_kernel(int F, int n, const int64_t *foff, const uint8_t *needb, const double *xy, const double *Kinv,
                                                        double *bear) {
    for (int g = (int)blockIdx.x * kT + (int)threadIdx.x; g < F; g += (int)gridDim.x * kT) {
        const int img = owner_of(foff, n, g);
        if (!needb[img]) continue;
        const double *K = Kinv + 9 * (size_t)img;
        const double x = xy[2 * (size_t)g], y = xy[2 * (size_t)g + 1];
        const double h0 = (K[0] * x + K[1] * y) + K[2], h1 = (K[3] * x + K[4] * y) + K[5], h2 = (K[6] * x + K[7] * y) + K[8];
        const double nrm = sqrt((h0 * h0 + h1 * h1) + h2 * h2);
        bear[3 * (size_t)g] = h0 / nrm; bear[3 * (size_t)g + 1] = h1 / nrm; bear[3 * (size_t)g + 2] = h2 / nrm;
    }
}

struct ScoreArgs {
    const int64_t *foff, *moff;
    const int32_t *pi, *pj, *mode, *f1, *f2;
    const double *xy, *bear, *focal, *Rrel, *trel, *FH;
    double max_E, max_F, max_H;
    uint8_t *code;            // per match: the first sweep's code, then the inlier flag
    int32_t *pair_inliers;
    int32_t *firstbad;
    const int32_t *work;      // the pairs of this launch (wave and workgroup form); the workspace form: the pair of every chunk / every pair
    const int32_t *chunk;     // workspace form: the chunk's number within its pair
    const int32_t *wsoff;     // workspace form: the first chunk of every listed pair in wsc, one more entry than pairs
    int32_t *wsc;             // workspace form: two counts per chunk
    int32_t nwork;
};
// a pair's geometry, the same in every lane
struct Geo {
    int mode;
    int64_t a0, na, b0, nb;   // the two images' features
    double M[9];              // E, F or H, row-major
    double R[9], t[3], e21[3], e12[3];
    double sq;                // the squared threshold
    double ep1, ep2;          // F: the epipole's y and z
};
__device__ inline void load_geo(const ScoreArgs &a, int k, Geo &g) {
    g.mode = a.mode[k];
    const int i = a.pi[k], j = a.pj[k];   // (checked on the host)
    g.a0 = a.foff[i]; g.na = a.foff[i + 1] - g.a0; g.b0 = a.foff[j]; g.nb = a.foff[j + 1] - g.b0;
    g.sq = 0.0; g.ep1 = 0.0; g.ep2 = 0.0;
    if (g.mode == MD_E) {
        const double *R = a.Rrel + 9 * (size_t)k, *t = a.trel + 3 * (size_t)k;
        for (int x = 0; x < 9; ++x) g.R[x] = R[x];
        for (int x = 0; x < 3; ++x) g.t[x] = t[x];
        for (int c = 0; c < 3; ++c) {   // E = [t]x R
            g.M[c] = t[1] * R[6 + c] - t[2] * R[3 + c];
            g.M[3 + c] = t[2] * R[c] - t[0] * R[6 + c];
            g.M[6 + c] = t[0] * R[3 + c] - t[1] * R[c];
        }
        const double thr = (a.max_E * 0.5) * (1.0 / a.focal[i] + 1.0 / a.focal[j]);
        g.sq = thr * thr;
        for (int r = 0; r < 3; ++r) {
            g.e12[r] = t[r];
            g.e21[r] = -dot3(R[r], R[3 + r], R[6 + r], t[0], t[1], t[2]);
        }
        if (g.e12[2] < 0) for (int r = 0; r < 3; ++r) g.e12[r] = -g.e12[r];
        if (g.e21[2] < 0) for (int r = 0; r < 3; ++r) g.e21[r] = -g.e21[r];
    } else if (g.mode == MD_F || g.mode == MD_H) {
        const double *M = a.FH + 9 * (size_t)k;
        for (int x = 0; x < 9; ++x) g.M[x] = M[x];
        if (g.mode == MD_F) {
            g.sq = a.max_F * a.max_F;
            double e0 = M[1] * M[8] - M[2] * M[7], e1 = M[2] * M[6] - M[0] * M[8], e2 = M[0] * M[7] - M[1] * M[6];   // row 0 x row 2
            const double eps = XM_VG_EPS;
            const bool ok = e0 > eps || e0 < -eps || e1 > eps || e1 < -eps || e2 > eps || e2 < -eps;
            if (!ok) { e1 = M[5] * M[6] - M[3] * M[8]; e2 = M[3] * M[7] - M[4] * M[6]; }                            // row 1 x row 2
            g.ep1 = e1; g.ep2 = e2;
        } else {
            g.sq = a.max_H * a.max_H;
        }
    }
}
__device__ inline int score_E(const Geo &g, const double *x1, const double *x2) {
    const double *E = g.M, *R = g.R, *t = g.t;
    const double d1 = XM_VG_EPS + x1[2], d2 = XM_VG_EPS + x2[2];
    double Ex1[3], Etx2[3];
    for (int r = 0; r < 3; ++r) {
        Ex1[r] = dot3(E[3 * r], E[3 * r + 1], E[3 * r + 2], x1[0], x1[1], x1[2]) / d1;
        Etx2[r] = dot3(E[r], E[3 + r], E[6 + r], x2[0], x2[1], x2[2]) / d2;
    }
    const double C = dot3(Ex1[0], Ex1[1], Ex1[2], x2[0], x2[1], x2[2]);
    const double Cx = Ex1[0] * Ex1[0] + Ex1[1] * Ex1[1], Cy = Etx2[0] * Etx2[0] + Etx2[1] * Etx2[1];
    const double r2 = (C * C) / (Cx + Cy);
    if (!(r2 < g.sq)) return 0;
    double Rx1[3], Rtx2[3];
    for (int r = 0; r < 3; ++r) {
        Rx1[r] = dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], x1[0], x1[1], x1[2]);
        Rtx2[r] = dot3(R[r], R[3 + r], R[6 + r], x2[0], x2[1], x2[2]);
    }
    const double am = -dot3(Rx1[0], Rx1[1], Rx1[2], x2[0], x2[1], x2[2]);
    const double b1 = -dot3(Rx1[0], Rx1[1], Rx1[2], t[0], t[1], t[2]);
    const double b2 = dot3(x2[0], x2[1], x2[2], t[0], t[1], t[2]);
    const double l1 = b1 - am * b2, l2 = (-am) * b1 + b2;
    const double f = 1.0 - am * am;
    const double mn = XM_VG_MIN_DEPTH * f, mx = XM_VG_MAX_DEPTH * f;
    const bool cheir = l1 > mn && l2 > mn && l1 < mx && l2 < mx;
    const bool apart = dot3(x1[0], x1[1], x1[2], Rtx2[0], Rtx2[1], Rtx2[2]) < XM_VG_COS_PARALLEL;
    const bool off1 = dot3(x1[0], x1[1], x1[2], g.e21[0], g.e21[1], g.e21[2]) < XM_VG_COS_EPIPOLE;
    const bool off2 = dot3(x2[0], x2[1], x2[2], g.e12[0], g.e12[1], g.e12[2]) < XM_VG_COS_EPIPOLE;
    return cheir && apart && off1 && off2 ? 1 : 0;
}
__device__ inline int score_F(const Geo &g, double x1, double y1, double x2, double y2) {
    const double *F = g.M;
    const double a0 = (F[0] * x1 + F[1] * y1) + F[2], a1 = (F[3] * x1 + F[4] * y1) + F[5], a2 = (F[6] * x1 + F[7] * y1) + F[8];
    const double b0 = (F[0] * x2 + F[3] * y2) + F[6], b1 = (F[1] * x2 + F[4] * y2) + F[7];
    const double C = (a0 * x2 + a1 * y2) + a2;
    const double r2 = (C * C) / ((a0 * a0 + a1 * a1) + (b0 * b0 + b1 * b1));
    if (!(r2 < g.sq)) return 0;
    const double sig = b0 * (g.ep1 - g.ep2 * y1);   // b0 = (F_00*x2 + F_10*y2) + F_20
    return sig > 0 ? 1 : 2;
}
__device__ inline int score_H(const Geo &g, double x1, double y1, double x2, double y2) {
    const double *H = g.M;
    const double h0 = (H[0] * x1 + H[1] * y1) + H[2], h1 = (H[3] * x1 + H[4] * y1) + H[5], h2 = (H[6] * x1 + H[7] * y1) + H[8];
    const double d = XM_VG_EPS + h2;
    const double u = h0 / d - x2, v = h1 / d - y2;
    return u * u + v * v < g.sq ? 1 : 0;
}
// match e of the pair: 0, 1 (inlier; F: a positive pre-inlier) or 2 (F: a negative pre-inlier)
__device__ inline int score_one(const ScoreArgs &a, const Geo &g, int64_t e) {
    const int64_t x = a.f1[e], y = a.f2[e];
    if (x < 0 || x >= g.na || y < 0 || y >= g.nb) {
        atomicMin(a.firstbad, (int32_t)e);
        return 0;
    }
    if (g.mode == MD_ZERO) return 0;
    if (g.mode == MD_ONES) return 1;
    const size_t u = (size_t)(g.a0 + x), v = (size_t)(g.b0 + y);
    if (g.mode == MD_E) {
        const double x1[3] = {a.bear[3 * u], a.bear[3 * u + 1], a.bear[3 * u + 2]}, x2[3] = {a.bear[3 * v], a.bear[3 * v + 1], a.bear[3 * v + 2]};
        return score_E(g, x1, x2);
    }
    if (g.mode == MD_F) return score_F(g, a.xy[2 * u], a.xy[2 * u + 1], a.xy[2 * v], a.xy[2 * v + 1]);
    return score_H(g, a.xy[2 * u], a.xy[2 * u + 1], a.xy[2 * v], a.xy[2 * v + 1]);
}
// the first sweep over the matches m0 .. m1 - 1 by a team of TEAM threads (tid: the thread's number in it): the codes, and this
// wavefront's two counts (the same in all its lanes)
template <int TEAM>
__device__ inline void first_sweep(const ScoreArgs &a, const Geo &g, int64_t m0, int64_t m1, int tid, int &pos, int &neg) {
    pos = 0; neg = 0;
    for (int64_t base = m0; base < m1; base += TEAM) {
        const int64_t e = base + tid;
        const int c = e < m1 ? score_one(a, g, e) : 0;
        if (e < m1) a.code[e] = (uint8_t)c;
        pos += __popcll(__ballot(c == 1)); neg += __popcll(__ballot(c == 2));
    }
}
// the second sweep: only an F pair's codes change (rule 3's majority); returns the pair's inliers
template <int TEAM>
__device__ inline int second_sweep(const ScoreArgs &a, const Geo &g, int64_t m0, int64_t m1, int tid, int pos, int neg) {
    if (g.mode != MD_F) return pos;
    const int side = pos == neg ? 0 : (pos > neg ? 1 : 2);
    for (int64_t e = m0 + tid; e < m1; e += TEAM) {
        const int c = a.code[e];   // (written by this thread, or by an earlier launch)
        a.code[e] = (uint8_t)(c != 0 && c == side ? 1 : 0);
    }
    return side == 0 ? 0 : (side == 1 ? pos : neg);
}
// the four wavefronts' counts in wavefront order
__device__ inline void group_sum2(int &x, int &y, int *lds) {
    const int w = (int)threadIdx.x >> 6;
    if (lane_id() == 0) { lds[w] = x; lds[kWaves + w] = y; }
    __syncthreads();
    x = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    y = ((lds[kWaves] + lds[kWaves + 1]) + lds[kWaves + 2]) + lds[kWaves + 3];
    __syncthreads();
}
// GROUP = false: one wavefront per pair, four pairs per workgroup; GROUP = true: one workgroup per pair
template <bool GROUP>
__global__ __launch_bounds__(kT) void vg_score_kernel(ScoreArgs a) {
    __shared__ int lds[2 * kWaves];
    constexpr int TEAM = GROUP ? kT : 64;
    const int item = GROUP ? (int)blockIdx.x : (int)blockIdx.x * kWaves + ((int)threadIdx.x >> 6);
    if (item >= a.nwork) return;   // (a whole team)
    const int tid = GROUP ? (int)threadIdx.x : lane_id();
    const int k = a.work[item];
    const int64_t m0 = a.moff[k], m1 = a.moff[k + 1];
    if (m1 - m0 > (GROUP ? kVgGroupMatches : kVgWaveMatches)) return;   // (the host lists it for a larger form)
    Geo g;
    load_geo(a, k, g);
    int pos, neg;
    first_sweep<TEAM>(a, g, m0, m1, tid, pos, neg);
    if (GROUP) group_sum2(pos, neg, lds);
    const int cnt = second_sweep<TEAM>(a, g, m0, m1, tid, pos, neg);
    if (tid == 0) a.pair_inliers[k] = cnt;
}
// workspace form: one workgroup per chunk of kVgGroupMatches matches
__global__ __launch_bounds__(kT) void vg_score_chunk_kernel(ScoreArgs a) {
    __shared__ int lds[2 * kWaves];
    const int item = (int)blockIdx.x;
    if (item >= a.nwork) return;
    const int k = a.work[item];
    const int64_t m0 = a.moff[k] + (int64_t)a.chunk[item] * kVgGroupMatches;
    const int64_t m1 = m0 + kVgGroupMatches < a.moff[k + 1] ? m0 + kVgGroupMatches : a.moff[k + 1];
    Geo g;
    load_geo(a, k, g);
    int pos, neg;
    first_sweep<kT>(a, g, m0, m1, (int)threadIdx.x, pos, neg);
    group_sum2(pos, neg, lds);
    if (threadIdx.x == 0) { a.wsc[2 * item] = pos; a.wsc[2 * item + 1] = neg; }
}
// workspace form: one workgroup per pair adds its chunks' counts in chunk order and makes the second sweep
__global__ __launch_bounds__(kT) void vg_score_final_kernel(ScoreArgs a) {
    const int q = (int)blockIdx.x;
    if (q >= a.nwork) return;
    const int k = a.work[q];
    int pos = 0, neg = 0;
    for (int c = a.wsoff[q]; c < a.wsoff[q + 1]; ++c) { pos += a.wsc[2 * c]; neg += a.wsc[2 * c + 1]; }
    Geo g;
    g.mode = a.mode[k];
    const int cnt = second_sweep<kT>(a, g, a.moff[k], a.moff[k + 1], (int)threadIdx.x, pos, neg);
    if (threadIdx.x == 0) a.pair_inliers[k] = cnt;
}

struct DecideArgs {
    int32_t npairs, score, min_inlier_num;
    double min_inlier_ratio, cos_max;
    const int32_t *pi, *pj, *pair_inliers;
    const int64_t *moff;
    const uint8_t *valid_in, *reg_in;
    const double *rot, *Rrel;   // rot null: rule 6 is off
    int32_t *status, *linked;
};
// rules 5 and 6
__global__ __launch_bounds__(kT) void vg_decide_kernel(DecideArgs a) {
    const int k = (int)(blockIdx.x * kT + threadIdx.x);
    if (k >= a.npairs) return;
    const int i = a.pi[k], j = a.pj[k];
    int st = !a.valid_in || a.valid_in[k] ? XM_VG_VALID : XM_VG_INVALID_IN;
    if (a.score && st == XM_VG_VALID) {
        const int inl = a.pair_inliers[k];
        const int64_t m = a.moff[k + 1] - a.moff[k];
        if (inl < a.min_inlier_num) st = XM_VG_FEW_INLIERS;
        else if ((double)inl / (double)m < a.min_inlier_ratio) st = XM_VG_LOW_RATIO;
    }
    if (a.rot && st == XM_VG_VALID && (!a.reg_in || (a.reg_in[i] && a.reg_in[j]))) {
        const double *Ri = a.rot + 9 * (size_t)i, *Rj = a.rot + 9 * (size_t)j, *Q = a.Rrel + 9 * (size_t)k;
        double s = 0.0;
        for (int x = 0; x < 3; ++x)
            for (int y = 0; y < 3; ++y) {
                const double prod = dot3(Rj[3 * x], Rj[3 * x + 1], Rj[3 * x + 2], Ri[3 * y], Ri[3 * y + 1], Ri[3 * y + 2]) * Q[3 * x + y];
                s = x == 0 && y == 0 ? prod : s + prod;
            }
        double c = (s - 1.0) / 2.0;
        if (c > 1.0) c = 1.0;
        if (c < -1.0) c = -1.0;
        if (c < a.cos_max) st = XM_VG_ROTATION;
    }
    a.status[k] = st;
    if (st == XM_VG_VALID) { a.linked[i] = 1; a.linked[j] = 1; }   // (every writer stores the same value)
}

// components: labels p over the images; a pair that is still valid is an edge
struct VgEdge {
    const int32_t *pi, *pj, *status;
    __device__ bool operator()(int64_t k, int &u, int &v) const {
        if (status[k] != XM_VG_VALID) return false;
        u = pi[k]; v = pj[k];
        return true;
    }
};
__global__ __launch_bounds__(kT) void vg_size_kernel(int n, const int32_t *linked, const int32_t *p, int32_t *size) {
    const int i = (int)(blockIdx.x * kT + threadIdx.x);
    if (i < n && linked[i]) atomicAdd(size + p[i], 1);
}
// one workgroup: the largest component (ties: the smaller label) and the number of components
__global__ __launch_bounds__(kT) void vg_largest_kernel(int n, const int32_t *linked, const int32_t *p, const int32_t *size, int32_t *best) {
    __shared__ u64 key[kT];
    __shared__ int cnt[kT];
    const int tid = (int)threadIdx.x;
    u64 mine = 0ull;
    int comps = 0;
    for (int i = tid; i < n; i += kT) {
        if (!linked[i] || p[i] != i) continue;
        comps += 1;
        const u64 w = ((u64)(uint32_t)size[i] << 32) | (u64)(0xffffffffu - (uint32_t)i);
        mine = w > mine ? w : mine;
    }
    key[tid] = mine; cnt[tid] = comps;
    __syncthreads();
    for (int off = kT / 2; off > 0; off >>= 1) {
        if (tid < off) {
            key[tid] = key[tid + off] > key[tid] ? key[tid + off] : key[tid];
            cnt[tid] += cnt[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const u64 w = key[0];
        best[B_LABEL] = w ? (int32_t)(0xffffffffu - (uint32_t)(w & 0xffffffffull)) : -1;
        best[B_SIZE] = (int32_t)(w >> 32);
        best[B_COMPONENTS] = cnt[0];
    }
}
// rule 7's outputs and the kept inlier count of every pair
__global__ __launch_bounds__(kT) void vg_prune_kernel(int n, int npairs, const int32_t *pi, const int32_t *linked, const int32_t *p, const int32_t *best,
                                                      const int32_t *pair_inliers, int32_t *status, uint8_t *regout, int32_t *keepcnt) {
    const int x = (int)(blockIdx.x * kT + threadIdx.x);
    const int lab = best[B_LABEL];
    if (x < n) regout[x] = linked[x] && p[x] == lab ? 1 : 0;
    if (x < npairs) {
        int st = status[x];
        if (st == XM_VG_VALID && p[pi[x]] != lab) { st = XM_VG_OUTSIDE; status[x] = st; }   // (a valid pair's ends carry one label)
        keepcnt[x] = st == XM_VG_VALID ? pair_inliers[x] : 0;
    }
}
__global__ __launch_bounds__(kT) void vg_stats_kernel(int npairs, const int32_t *status, const int32_t *model, const int32_t *pair_inliers, u64 *cnt) {
    const int k = (int)(blockIdx.x * kT + threadIdx.x);
    const bool in = k < npairs;
    const int st = in ? status[k] : -1, md = in ? model[k] : -1;
    for (int s = 0; s < 6; ++s) wave_sum_to(cnt + C_STATUS + s, st == s, 1ull);
    for (int s = 0; s < 4; ++s) wave_sum_to(cnt + C_MODEL + s, md == s, 1ull);
    wave_sum_to(cnt + C_INLIERS, in, in ? (u64)(uint32_t)pair_inliers[k] : 0ull);
}

// the inliers of a kept pair at its offset, in input order
template <bool GROUP>
__global__ __launch_bounds__(kT) void vg_emit_kernel(int nwork, const int32_t *work, const int64_t *moff, const uint8_t *inl, const int32_t *keepcnt,
                                                     const int32_t *koff, const int32_t *f1, const int32_t *f2, int32_t *o1, int32_t *o2) {
    __shared__ int wtot[kWaves];
    constexpr int TEAM = GROUP ? kT : 64;
    const int item = GROUP ? (int)blockIdx.x : (int)blockIdx.x * kWaves + ((int)threadIdx.x >> 6);
    if (item >= nwork) return;   // (a whole team)
    const int tid = GROUP ? (int)threadIdx.x : lane_id();
    const int k = work[item];
    if (keepcnt[k] == 0) return;
    const int64_t m0 = moff[k], m1 = moff[k + 1];
    int64_t at = koff[k];
    for (int64_t base = m0; base < m1; base += TEAM) {
        const int64_t e = base + tid;
        const bool on = e < m1 && inl[e] != 0;
        const u64 mask = __ballot(on);
        int before = __popcll(mask & ((1ull << lane_id()) - 1ull)), tot = __popcll(mask);
        if (GROUP) {
            const int w = (int)threadIdx.x >> 6;
            if (lane_id() == 0) wtot[w] = tot;
            __syncthreads();
            tot = 0;
            for (int x = 0; x < kWaves; ++x) { if (x < w) before += wtot[x]; tot += wtot[x]; }
            __syncthreads();
        }
        if (on) { o1[at + before] = f1[e]; o2[at + before] = f2[e]; }
        at += tot;
    }
}

struct Block { int32_t changed[kBatch]; int32_t firstbad; int32_t best[B_COUNT]; u64 cnt[C_COUNT]; };   // what the host reads during a call

void run_device(int n, const int64_t *foff, const double *xy, const double *focal, const double *Kinv, const double *bearing, int npairs, const int32_t *pi,
                const int32_t *pj, const int32_t *model, const double *Rrel, const double *trel, const double *FH, const uint8_t *valid_in,
                const uint8_t *registered_in, const double *rot, const int64_t *moff, const int32_t *f1, const int32_t *f2, const VgSettings &cfg,
                uint8_t *inlier, int32_t *pair_inliers, int32_t *pair_status, uint8_t *registered_out, int64_t *moff_out, int32_t *f1_out, int32_t *f2_out,
                VgOutcome &out, std::chrono::steady_clock::time_point t_start, hipStream_t st) {
    const int F = (int)foff[n];
    const int64_t E = moff[npairs];
    // what the scoring does with every pair, the images whose bearings are needed, and the pairs by the form that runs them
    std::vector<int32_t> mode((size_t)npairs), lwave, lgroup, lws, cpair, cchunk, wsoff;
    std::vector<uint8_t> needb((size_t)n, 0);
    bool any_E = false, any_FH = false;
    for (int k = 0; k < npairs; ++k) {
        const bool valid = !valid_in || valid_in[k] != 0;
        int md = MD_ZERO;
        if (valid && !cfg.score) md = MD_ONES;
        else if (valid) md = model[k] == XM_VG_MODEL_E ? MD_E : model[k] == XM_VG_MODEL_F ? MD_F : model[k] == XM_VG_MODEL_H ? MD_H : MD_ZERO;
        mode[(size_t)k] = md;
        const int64_t m = moff[k + 1] - moff[k];
        out.max_matches = std::max(out.max_matches, m);
        if (m == 0) continue;
        if (md == MD_E) { any_E = true; needb[(size_t)pi[k]] = 1; needb[(size_t)pj[k]] = 1; }
        if (md == MD_F || md == MD_H) any_FH = true;
        if (m <= kVgWaveMatches) lwave.push_back(k);
        else if (m <= kVgGroupMatches) lgroup.push_back(k);
        else {
            wsoff.push_back((int32_t)cpair.size());
            lws.push_back(k);
            for (int64_t c = 0; c * kVgGroupMatches < m; ++c) { cpair.push_back(k); cchunk.push_back((int32_t)c); }
        }
    }
    wsoff.push_back((int32_t)cpair.size());
    out.pairs_wave = (int64_t)lwave.size(); out.pairs_group = (int64_t)lgroup.size(); out.pairs_workspace = (int64_t)lws.size();
    std::vector<int32_t> iota((size_t)n);
    for (int i = 0; i < n; ++i) iota[(size_t)i] = i;

    Pinned<Block> pin;
    DevBuf<int64_t> dfoff, dmoff;
    DevBuf<double> dxy, dfocal, dKinv, dbear, dRrel, dtrel, dFH, drot;
    DevBuf<uint8_t> dvalid, dreg, dneedb, dcode, dregout;
    DevBuf<int32_t> dpi, dpj, dmodel, dmode, df1, df2, dlwave, dlgroup, dlws, dcpair, dcchunk, dwsoff, dwsc, dinl, dstatus, linked, p, size, best, changed,
        firstbad, keepcnt, koff, sums, do1, do2;
    DevBuf<u64> cnt;
    upload(dfoff, foff, (size_t)n + 1, st);
    upload(dmoff, moff, (size_t)npairs + 1, st);
    upload(dxy, xy, (size_t)F * 2, st);
    if (any_E) {
        upload(dfocal, focal, (size_t)n, st);
        upload(dRrel, Rrel, (size_t)npairs * 9, st);
        upload(dtrel, trel, (size_t)npairs * 3, st);
        if (bearing) upload(dbear, bearing, (size_t)F * 3, st);
        else { upload(dKinv, Kinv, (size_t)n * 9, st); upload(dneedb, needb.data(), (size_t)n, st); dbear.alloc((size_t)F * 3, false); }
    }
    if (any_FH) upload(dFH, FH, (size_t)npairs * 9, st);
    if (rot) {
        upload(drot, rot, (size_t)n * 9, st);
        if (!any_E) upload(dRrel, Rrel, (size_t)npairs * 9, st);
    }
    if (valid_in) upload(dvalid, valid_in, (size_t)npairs, st);
    if (registered_in) upload(dreg, registered_in, (size_t)n, st);
    upload(dpi, pi, (size_t)npairs, st);
    upload(dpj, pj, (size_t)npairs, st);
    upload(dmodel, model, (size_t)npairs, st);
    upload(dmode, mode.data(), (size_t)npairs, st);
    upload(df1, f1, (size_t)E, st);
    upload(df2, f2, (size_t)E, st);
    upload(dlwave, lwave.data(), lwave.size(), st);
    upload(dlgroup, lgroup.data(), lgroup.size(), st);
    upload(dlws, lws.data(), lws.size(), st);
    upload(dcpair, cpair.data(), cpair.size(), st);
    upload(dcchunk, cchunk.data(), cchunk.size(), st);
    upload(dwsoff, wsoff.data(), wsoff.size(), st);
    upload(p, iota.data(), (size_t)n, st);
    dwsc.alloc(2 * cpair.size(), false);
    dcode.alloc((size_t)E, false);
    fresh(dinl, (size_t)npairs, 0, st);   // (a pair without matches runs in no scoring kernel)
    dstatus.alloc((size_t)npairs, false); keepcnt.alloc((size_t)npairs, false); koff.alloc((size_t)npairs, false);
    sums.alloc((size_t)(npairs / kScanTile + 1), false);
    fresh(linked, (size_t)n, 0, st); fresh(size, (size_t)n, 0, st); fresh(cnt, C_COUNT, 0, st);
    fresh(changed, (size_t)kMaxRounds + kBatch, 0, st);
    best.alloc(B_COUNT, false); dregout.alloc((size_t)n, false);
    do1.alloc((size_t)E, false); do2.alloc((size_t)E, false);
    firstbad.alloc(1, false);
    pin.h->firstbad = INT32_MAX;   // (above every match number)
    XM_HIP_CHECK(hipMemcpyAsync(firstbad.p, &pin.h->firstbad, sizeof(int32_t), hipMemcpyHostToDevice, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the upload");
    out.seconds_index = secs_since(t_start);
    const auto t_kernels = std::chrono::steady_clock::now();

    if (any_E && !bearing) {
        hipLaunchKernelGGL(vg_bearing_kernel, dim3(grid_for(F, 4096)), dim3(kT), 0, st, F, n, dfoff.p, dneedb.p, dxy.p, dKinv.p, dbear.p);
        check_launch("vg_bearing_kernel");
    }
    ScoreArgs a;
    a.foff = dfoff.p; a.moff = dmoff.p; a.pi = dpi.p; a.pj = dpj.p; a.mode = dmode.p; a.f1 = df1.p; a.f2 = df2.p; a.xy = dxy.p; a.bear = dbear.p;
    a.focal = dfocal.p; a.Rrel = dRrel.p; a.trel = dtrel.p; a.FH = dFH.p; a.max_E = cfg.max_E; a.max_F = cfg.max_F; a.max_H = cfg.max_H;
    a.code = dcode.p; a.pair_inliers = dinl.p; a.firstbad = firstbad.p; a.chunk = nullptr; a.wsoff = nullptr; a.wsc = nullptr;
    if (!lwave.empty()) {
        a.work = dlwave.p; a.nwork = (int32_t)lwave.size();
        hipLaunchKernelGGL(vg_score_kernel<false>, dim3((unsigned)((lwave.size() + kWaves - 1) / kWaves)), dim3(kT), 0, st, a);
        check_launch("vg_score_kernel (wavefront)");
    }
    if (!lgroup.empty()) {
        a.work = dlgroup.p; a.nwork = (int32_t)lgroup.size();
        hipLaunchKernelGGL(vg_score_kernel<true>, dim3((unsigned)lgroup.size()), dim3(kT), 0, st, a);
        check_launch("vg_score_kernel (workgroup)");
    }
    if (!lws.empty()) {
        a.work = dcpair.p; a.nwork = (int32_t)cpair.size(); a.chunk = dcchunk.p; a.wsc = dwsc.p;
        hipLaunchKernelGGL(vg_score_chunk_kernel, dim3((unsigned)cpair.size()), dim3(kT), 0, st, a);
        a.work = dlws.p; a.nwork = (int32_t)lws.size(); a.wsoff = dwsoff.p;
        hipLaunchKernelGGL(vg_score_final_kernel, dim3((unsigned)lws.size()), dim3(kT), 0, st, a);
        check_launch("vg_score_chunk_kernel");
    }
    DecideArgs d;
    d.npairs = npairs; d.score = cfg.score ? 1 : 0; d.min_inlier_num = cfg.min_inlier_num; d.min_inlier_ratio = cfg.min_inlier_ratio;
    d.cos_max = cfg.cos_max_rotation_error; d.pi = dpi.p; d.pj = dpj.p; d.pair_inliers = dinl.p; d.moff = dmoff.p;
    d.valid_in = valid_in ? dvalid.p : nullptr; d.reg_in = registered_in ? dreg.p : nullptr; d.rot = rot ? drot.p : nullptr; d.Rrel = dRrel.p;
    d.status = dstatus.p; d.linked = linked.p;
    const unsigned gp = grid_of(npairs), gn = grid_of(n);
    hipLaunchKernelGGL(vg_decide_kernel, dim3(gp), dim3(kT), 0, st, d);
    check_launch("vg_decide_kernel");
    XM_HIP_CHECK(hipMemcpyAsync(&pin.h->firstbad, firstbad.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));

    // the first wait is in label_components: firstbad, whose copy is enqueued above, is looked at behind it
    const VgEdge edge = {dpi.p, dpj.p, dstatus.p};
    out.rounds = label_components(npairs, n, edge, p.p, changed.p, pin.h->changed, kStage, cfg.watchdog_s, st);
    if ((int64_t)pin.h->firstbad < E) {
        const int64_t e = pin.h->firstbad;
        const int64_t k = (std::upper_bound(moff, moff + npairs + 1, e) - moff) - 1;
        throw Error(XM_ERR_ARG, "xm_view_graph_filter: feature index out of range at match " + std::to_string(e) + " (pair " + std::to_string(k) + ")");
    }

    hipLaunchKernelGGL(vg_size_kernel, dim3(gn), dim3(kT), 0, st, n, linked.p, p.p, size.p);
    hipLaunchKernelGGL(vg_largest_kernel, dim3(1), dim3(kT), 0, st, n, linked.p, p.p, size.p, best.p);
    hipLaunchKernelGGL(vg_prune_kernel, dim3(std::max(gp, gn)), dim3(kT), 0, st, n, npairs, dpi.p, linked.p, p.p, best.p, dinl.p, dstatus.p, dregout.p, keepcnt.p);
    check_launch("vg_prune_kernel");
    exclusive_scan(npairs, keepcnt.p, koff.p, sums, cnt.p + C_MOUT, st);
    if (!lwave.empty())
        hipLaunchKernelGGL(vg_emit_kernel<false>, dim3((unsigned)((lwave.size() + kWaves - 1) / kWaves)), dim3(kT), 0, st, (int)lwave.size(), dlwave.p, dmoff.p,
                           dcode.p, keepcnt.p, koff.p, df1.p, df2.p, do1.p, do2.p);
    if (!lgroup.empty())
        hipLaunchKernelGGL(vg_emit_kernel<true>, dim3((unsigned)lgroup.size()), dim3(kT), 0, st, (int)lgroup.size(), dlgroup.p, dmoff.p, dcode.p, keepcnt.p,
                           koff.p, df1.p, df2.p, do1.p, do2.p);
    if (!lws.empty())
        hipLaunchKernelGGL(vg_emit_kernel<true>, dim3((unsigned)lws.size()), dim3(kT), 0, st, (int)lws.size(), dlws.p, dmoff.p, dcode.p, keepcnt.p, koff.p,
                           df1.p, df2.p, do1.p, do2.p);
    hipLaunchKernelGGL(vg_stats_kernel, dim3(gp), dim3(kT), 0, st, npairs, dstatus.p, dmodel.p, dinl.p, cnt.p);
    check_launch("vg_emit_kernel");
    XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt.p, sizeof(u64) * C_COUNT, hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(pin.h->best, best.p, sizeof(int32_t) * B_COUNT, hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the kept matches");
    out.seconds_kernels = secs_since(t_kernels);
    const auto t_down = std::chrono::steady_clock::now();
    const u64 *c = pin.h->cnt;
    if (c[C_MOUT] > (u64)E) throw Error(XM_ERR_HIP, "view graph: more kept matches than matches");
    const size_t no = (size_t)c[C_MOUT];
    std::vector<int32_t> hkoff((size_t)npairs);
    XM_HIP_CHECK(hipMemcpyAsync(hkoff.data(), koff.p, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (E) XM_HIP_CHECK(hipMemcpyAsync(inlier, dcode.p, (size_t)E * sizeof(uint8_t), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(pair_inliers, dinl.p, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(pair_status, dstatus.p, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(registered_out, dregout.p, (size_t)n * sizeof(uint8_t), hipMemcpyDeviceToHost, st));
    if (no) {
        XM_HIP_CHECK(hipMemcpyAsync(f1_out, do1.p, no * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(f2_out, do2.p, no * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    wait_stream(st, cfg.watchdog_s, kStage, "the download");
    for (int k = 0; k < npairs; ++k) moff_out[k] = hkoff[(size_t)k];
    moff_out[npairs] = (int64_t)no;
    out.seconds_download = secs_since(t_down);
    out.matches_out = (int64_t)no; out.inliers = (int64_t)c[C_INLIERS];
    for (int s = 0; s < 6; ++s) out.pairs_by_status[s] = (int64_t)c[C_STATUS + s];
    for (int s = 0; s < 4; ++s) out.pairs_by_model[s] = (int64_t)c[C_MODEL + s];
    out.largest = pin.h->best[B_SIZE]; out.components = pin.h->best[B_COMPONENTS];
}

}  // namespace

void view_graph_filter_host(int64_t n, const int64_t *foff, const double *xy, const double *focal, const double *Kinv, const double *bearing,
                            int64_t npairs, const int32_t *pi, const int32_t *pj, const int32_t *model, const double *Rrel, const double *trel,
                            const double *FH, const uint8_t *valid_in, const uint8_t *registered_in, const double *rot, const int64_t *moff,
                            const int32_t *f1, const int32_t *f2, const VgSettings &cfg, uint8_t *inlier, int32_t *pair_inliers, int32_t *pair_status,
                            uint8_t *registered_out, int64_t *moff_out, int32_t *f1_out, int32_t *f2_out, VgOutcome &out) {
    const auto t_start = std::chrono::steady_clock::now();
    out = VgOutcome();
    out.matches = npairs > 0 ? moff[npairs] : 0;
    if (npairs == 0) {   // nothing to launch: no pair, nothing registered
        for (int64_t i = 0; i < n; ++i) registered_out[i] = 0;
        if (moff_out) moff_out[0] = 0;
        return;
    }
    hipStream_t st = nullptr;   // the default stream, as xm_pair_filter
    try {
        run_device((int)n, foff, xy, focal, Kinv, bearing, (int)npairs, pi, pj, model, Rrel, trel, FH, valid_in, registered_in, rot, moff, f1, f2, cfg, inlier,
                   pair_inliers, pair_status, registered_out, moff_out, f1_out, f2_out, out, t_start, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the device buffers are freed next: nothing may still be reading them
        throw;
    }
}

}  // namespace xm
