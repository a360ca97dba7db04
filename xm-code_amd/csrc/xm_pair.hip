// xm_pair.hip — the pairwise relative-rotation filter on the device (xm_pair.h; definition in include/xm_amd.h at xm_pair_filter).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "xm_pair.h"
#include "xm_device.h"
#include "xm_stage.h"

// every product and every sum below is rounded on its own: the residual that is sorted and the one compared with the threshold are the same bits
#pragma clang fp contract(off)
#include "xm_sortstat.h"   // after the pragma: its percentile is compiled without contraction too

namespace xm {
namespace {

constexpr int kT = kPairThreads;
static_assert(kT == kSortThreads, "the helpers of xm_sortstat.h are written for this workgroup size");
constexpr const char *kStage = "pair filter";
constexpr int kCap = kPairLdsJoint;

// slots of the device counter block
enum { C_OVER_SMALL = 0, C_OVER_LDS, C_MAX_JOINT, C_USED, C_TOO_FEW, C_DEGENERATE, C_FLAGGED, C_COUNT };

struct PairArgs {
    const int32_t *camptr, *slm, *srow;   // per camera: landmarks (increasing) and input rows of its observations
    const double *p;                      // nobs x 3, input order
    const int32_t *pi, *pj;
    const double *R;
    const int32_t *work;                  // LDS kernels: the pair of every workgroup; workspace kernel: the listed pairs
    int32_t nwork;
    int32_t min_joint;
    double trim, dist_q, err_q, mad;      // the percentiles as fractions (q / 100)
    int32_t *count;
    xm_pair_stat_t *stats;                // may be null
    int32_t *overflow;                    // LDS kernels: pairs with more common landmarks than the kernel holds are listed here ...
    int32_t over_slot;                    // ... and counted in this slot of cnt
    int32_t first;                        // the kernel that sees every pair: it records the largest joint set
    uint32_t *cnt;
    char *ws;                             // workspace kernel: ws_cap * 16 bytes per workgroup
    int32_t ws_cap;
};

__device__ inline bool finite_(double x) { return (__double_as_longlong(x) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }

// position of key in the increasing array a[0 .. len), -1 when absent
__device__ inline int find_lm(const int32_t *a, int len, int key) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < len && a[lo] == key) ? lo : -1;
}
// scipy.stats.trim_mean of the cnt smallest values of the sorted S: the mean of [lo, cnt - lo), lo = int(trim * cnt); a fixed tree
template <class P>
__device__ inline double trimmed_mean(P S, int cnt, double trim, double *dred) {
    const int lo = (int)(trim * (double)cnt), hi = cnt - lo;
    double v = 0.0;
    for (int q = lo + (int)threadIdx.x; q < hi; q += kT) v += S[q];
    const double sum = block_sum256(v, dred);
    __syncthreads();   // dred is free again
    return sum / (double)(hi - lo);
}
__device__ inline double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

struct Pt { double v[3]; };
__device__ inline Pt load_pt(const double *p, int row) {
    Pt r;
    const double *q = p + (size_t)row * 3;
    r.v[0] = q[0]; r.v[1] = q[1]; r.v[2] = q[2];
    return r;
}
__device__ inline double dist_to(const Pt &x, const double (&c)[3]) { return norm3(x.v[0] - c[0], x.v[1] - c[1], x.v[2] - c[2]); }
// R (src / scale2 * scale1)
__device__ inline Pt rotate_scaled(const Pt &s, const double (&R)[9], double scale1, double scale2) {
    const double x = s.v[0] / scale2 * scale1, y = s.v[1] / scale2 * scale1, z = s.v[2] / scale2 * scale1;
    Pt r;
#pragma unroll
    for (int a = 0; a < 3; ++a) r.v[a] = (R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z;
    return r;
}
__device__ inline double residual(const Pt &rs, const Pt &d, const double (&tr)[3], double scale1) {
    return norm3(rs.v[0] + tr[0] - d.v[0], rs.v[1] + tr[1] - d.v[1], rs.v[2] + tr[2] - d.v[2]) / scale1;
}

struct Scratch { double dred[4]; int ired[4]; int wtot[4]; };

__device__ inline void write_stat(const PairArgs &a, int pair, const xm_pair_stat_t &s, int slot) {
    if (threadIdx.x != 0) return;
    if (a.stats) a.stats[pair] = s;
    atomicAdd(a.cnt + slot, 1u);
}

// one pair by one workgroup.  S (doubles) and rows, cap entries each: rows[q] = the input rows of common landmark q in camera i (x) and in
// camera j (y); the sign bit of y says that step 4 dropped the point
constexpr int kDropped = (int)0x80000000u;
__device__ inline int row_i(const int2 &r) { return r.x; }
__device__ inline int row_j(const int2 &r) { return r.y & 0x7fffffff; }
__device__ inline bool kept(const int2 &r) { return r.y >= 0; }
template <bool WS, class PD, class PI>
__device__ inline void run_pair(const PairArgs &a, int pair, PD S, PI rows, int cap, Scratch &sc) {
    const int tid = (int)threadIdx.x;
    const int ci = a.pi[pair], cj = a.pj[pair];
    const int bi = a.camptr[ci], li = a.camptr[ci + 1] - bi, bj = a.camptr[cj], lj = a.camptr[cj + 1] - bj;
    const bool ishort = li <= lj;
    const int bs = ishort ? bi : bj, ls = ishort ? li : lj, bl = ishort ? bj : bi, ll = ishort ? lj : li;
    const int32_t *lms = a.slm + bs, *lml = a.slm + bl;

    // 1. how many common landmarks
    int c = 0;
    for (int t = tid; t < ls; t += kT) c += find_lm(lml, ll, lms[t]) >= 0 ? 1 : 0;
    const int k = block_sum_int(c, sc.ired);
    xm_pair_stat_t st;
    st.n_joint = k; st.n_kept = 0; st.n_flagged = 0; st.status = XM_PAIR_TOO_FEW;
    st.scale1 = st.scale2 = st.median = st.p95 = st.percentage = 0.0;
    st.translation[0] = st.translation[1] = st.translation[2] = 0.0;
    if (a.first && tid == 0) atomicMax(a.cnt + C_MAX_JOINT, (uint32_t)k);
    if (k < a.min_joint || k < 1) { write_stat(a, pair, st, C_TOO_FEW); return; }
    if (k > cap) {   // (the workspace is sized by the largest joint set: only the LDS instantiations come here)
        if (!WS && tid == 0) a.overflow[atomicAdd(a.cnt + a.over_slot, 1u)] = pair;
        return;
    }
    int KP = 2;
    while (KP < k) KP <<= 1;

    // the common landmarks in increasing order: their rows in camera i and in camera j
    int base = 0;
    for (int t0 = 0; t0 < ls; t0 += kT) {
        const int t = t0 + tid;
        const int f = t < ls ? find_lm(lml, ll, lms[t]) : -1;
        const bool hit = f >= 0;
        const u64 mask = __ballot(hit);
        const int before = __popcll(mask & ((1ull << lane_id()) - 1ull));
        if (lane_id() == 0) sc.wtot[tid >> 6] = __popcll(mask);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < (tid >> 6)) off += sc.wtot[w]; tot += sc.wtot[w]; }
        if (hit) {
            const int es = a.srow[bs + t], el = a.srow[bl + f];
            rows[off + before] = ishort ? make_int2(es, el) : make_int2(el, es);
        }
        base += tot;
        __syncthreads();
    }

    const double *p = a.p;
    const double trim = a.trim;
    // 2. trimmed means of the coordinates
    double sa[3], da[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        fill_sort(S, KP, k, [&](int q) { return p[(size_t)row_i(rows[q]) * 3 + x]; });
        sa[x] = trimmed_mean(S, k, trim, sc.dred);
        fill_sort(S, KP, k, [&](int q) { return p[(size_t)row_j(rows[q]) * 3 + x]; });
        da[x] = trimmed_mean(S, k, trim, sc.dred);
    }
    // 3., 4. distances to them, their percentiles, the kept points
    fill_sort(S, KP, k, [&](int q) { return dist_to(load_pt(p, row_i(rows[q])), sa); });
    const double thr_s = percentile(S, k, a.dist_q);
    __syncthreads();
    fill_sort(S, KP, k, [&](int q) { return dist_to(load_pt(p, row_j(rows[q])), da); });
    const double thr_d = percentile(S, k, a.dist_q);
    __syncthreads();
    int mine = 0;
    for (int q = tid; q < k; q += kT) {
        const bool kp = dist_to(load_pt(p, row_i(rows[q])), sa) < thr_s && dist_to(load_pt(p, row_j(rows[q])), da) < thr_d;
        if (!kp) rows[q].y |= kDropped;
        mine += kp ? 1 : 0;
    }
    const int nk = block_sum_int(mine, sc.ired);   // (its barriers publish the dropped bits)
    st.n_kept = nk;
    if (nk < 1) { st.status = XM_PAIR_DEGENERATE; write_stat(a, pair, st, C_DEGENERATE); return; }
    // 5. the means again over the kept points; 6. the two scales
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        fill_sort(S, KP, k, [&](int q) { return kept(rows[q]) ? p[(size_t)row_i(rows[q]) * 3 + x] : inf_(); });
        sa[x] = trimmed_mean(S, nk, trim, sc.dred);
        fill_sort(S, KP, k, [&](int q) { return kept(rows[q]) ? p[(size_t)row_j(rows[q]) * 3 + x] : inf_(); });
        da[x] = trimmed_mean(S, nk, trim, sc.dred);
    }
    fill_sort(S, KP, k, [&](int q) { return kept(rows[q]) ? dist_to(load_pt(p, row_j(rows[q])), da) : inf_(); });
    const double scale1 = trimmed_mean(S, nk, trim, sc.dred);
    fill_sort(S, KP, k, [&](int q) { return kept(rows[q]) ? dist_to(load_pt(p, row_i(rows[q])), sa) : inf_(); });
    const double scale2 = trimmed_mean(S, nk, trim, sc.dred);
    st.scale1 = scale1; st.scale2 = scale2;
    st.status = XM_PAIR_DEGENERATE;
    if (!finite_(scale1) || !finite_(scale2) || scale2 == 0.0) { write_stat(a, pair, st, C_DEGENERATE); return; }
    // 7., 8. the translation
    double R[9], tr[3];
#pragma unroll
    for (int x = 0; x < 9; ++x) R[x] = a.R[(size_t)pair * 9 + x];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        fill_sort(S, KP, k, [&](int q) { return p[(size_t)row_j(rows[q]) * 3 + x] - rotate_scaled(load_pt(p, row_i(rows[q])), R, scale1, scale2).v[x]; });
        tr[x] = trimmed_mean(S, k, trim, sc.dred);
        st.translation[x] = tr[x];
    }
    // 9., 10. residuals and their threshold
    int bad = 0;
    for (int q = tid; q < KP; q += kT) {
        double e = inf_();
        if (q < k) {
            e = residual(rotate_scaled(load_pt(p, row_i(rows[q])), R, scale1, scale2), load_pt(p, row_j(rows[q])), tr, scale1);
            if (!finite_(e)) { bad += 1; e = inf_(); }   // (a value that is not a number has no place in the order)
        }
        S[q] = e;
    }
    bad = block_sum_int(bad, sc.ired);
    sort_values(S, KP);
    const double med = (k & 1) ? S[k >> 1] : (S[(k >> 1) - 1] + S[k >> 1]) * 0.5;
    const double p95 = percentile(S, k, a.err_q);
    const double m3 = a.mad * med;
    const double thr = m3 > p95 ? m3 : p95;
    st.median = med; st.p95 = p95;
    if (bad || !finite_(tr[0]) || !finite_(tr[1]) || !finite_(tr[2]) || !finite_(thr)) { write_stat(a, pair, st, C_DEGENERATE); return; }
    int nfl = 0, nsmall = 0;
    for (int q = tid; q < k; q += kT) {
        const int ri = row_i(rows[q]), rj = row_j(rows[q]);
        const double e = residual(rotate_scaled(load_pt(p, ri), R, scale1, scale2), load_pt(p, rj), tr, scale1);
        nsmall += e < 0.05 ? 1 : 0;
        if (e - thr > 0.0) {
            nfl += 1;
            atomicAdd(a.count + ri, 1);
            atomicAdd(a.count + rj, 1);
        }
    }
    nfl = block_sum_int(nfl, sc.ired);
    nsmall = block_sum_int(nsmall, sc.ired);
    st.n_flagged = nfl;
    st.percentage = (double)nsmall / (double)k;
    st.status = XM_PAIR_USED;
    write_stat(a, pair, st, C_USED);
}

// CAP = kPairSmallJoint: 4 KB of LDS and registers for six workgroups per CU (eight would spill); CAP = kPairLdsJoint: 32 KB, four per CU
template <int CAP>
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(CAP <= 512 ? 6 : 4))) void pair_lds_kernel(PairArgs a) {
    __shared__ double S[CAP];
    __shared__ int2 rows[CAP];
    __shared__ Scratch sc;
    if ((int)blockIdx.x >= a.nwork) return;
    run_pair<false>(a, a.work[blockIdx.x], S, rows, CAP, sc);
}
__global__ __launch_bounds__(kT) void pair_ws_kernel(PairArgs a) {
    __shared__ Scratch sc;
    char *mine = a.ws + (size_t)blockIdx.x * (size_t)a.ws_cap * 16;
    double *S = (double *)mine;
    int2 *rows = (int2 *)(mine + (size_t)a.ws_cap * 8);
    for (int w = (int)blockIdx.x; w < a.nwork; w += (int)gridDim.x) {
        run_pair<true>(a, a.work[w], S, rows, a.ws_cap, sc);
        __syncthreads();
    }
}
__global__ __launch_bounds__(kT) void pair_outlier_kernel(int64_t nobs, const int32_t *count, int32_t min_flags, uint8_t *outlier, uint32_t *cnt) {
    uint32_t total = 0;   // per wavefront over a grid-stride walk: one atomic on the shared counter at the end
    for (int64_t base = (int64_t)blockIdx.x * kT; base < nobs; base += (int64_t)gridDim.x * kT) {
        const int64_t e = base + threadIdx.x;
        const bool out = e < nobs && count[e] >= min_flags;
        if (e < nobs) outlier[e] = out ? 1 : 0;
        total += (uint32_t)__popcll(__ballot(out));
    }
    if (lane_id() == 0 && total) atomicAdd(cnt + C_FLAGGED, total);
}

void run_device(int64_t n, int64_t nobs, const double *p, int64_t npairs, const int32_t *pi, const int32_t *pj, const double *R,
                const std::vector<int32_t> &camptr, const std::vector<int32_t> &slm, const std::vector<int32_t> &srow, const std::vector<int32_t> &order,
                const PairSettings &cfg, int32_t *count, uint8_t *outlier, xm_pair_stat_t *stats, PairOutcome &out,
                std::chrono::steady_clock::time_point t_start, hipStream_t st) {
    DevBuf<int32_t> dcamptr, dslm, dsrow, dpi, dpj, dorder, dcount, dover1, dover2;
    DevBuf<double> dp, dR;
    DevBuf<uint32_t> dcnt;
    DevBuf<uint8_t> doutlier;
    DevBuf<xm_pair_stat_t> dstats;
    DevBuf<char> ws;
    upload(dcamptr, camptr.data(), camptr.size(), st);
    upload(dslm, slm.data(), slm.size(), st);
    upload(dsrow, srow.data(), srow.size(), st);
    upload(dp, p, (size_t)nobs * 3, st);
    upload(dpi, pi, (size_t)npairs, st);
    upload(dpj, pj, (size_t)npairs, st);
    upload(dR, R, (size_t)npairs * 9, st);
    upload(dorder, order.data(), order.size(), st);
    dcount.alloc((size_t)nobs, false); doutlier.alloc((size_t)nobs, false); dover1.alloc((size_t)npairs, false); dcnt.alloc(C_COUNT, false);
    XM_HIP_CHECK(hipMemsetAsync(dcount.p, 0, (size_t)(nobs ? nobs : 1) * sizeof(int32_t), st));
    XM_HIP_CHECK(hipMemsetAsync(dcnt.p, 0, C_COUNT * sizeof(uint32_t), st));
    if (stats) dstats.alloc((size_t)npairs, false);
    wait_stream(st, cfg.watchdog_s, kStage, "the upload");
    out.seconds_index = secs_since(t_start);
    const auto t_kernels = std::chrono::steady_clock::now();

    PairArgs a;
    a.camptr = dcamptr.p; a.slm = dslm.p; a.srow = dsrow.p; a.p = dp.p; a.pi = dpi.p; a.pj = dpj.p; a.R = dR.p;
    a.work = dorder.p; a.nwork = (int32_t)npairs; a.min_joint = cfg.min_joint;
    a.trim = cfg.trim; a.dist_q = cfg.dist_pct / 100.0; a.err_q = cfg.err_pct / 100.0; a.mad = cfg.mad_factor;
    a.count = dcount.p; a.stats = stats ? dstats.p : nullptr; a.overflow = dover1.p; a.over_slot = C_OVER_SMALL; a.first = 1; a.cnt = dcnt.p; a.ws = nullptr; a.ws_cap = 0;
    uint32_t hcnt[C_COUNT] = {0};
    if (npairs > 0) {
        // every pair through the small kernel; those with more than kPairSmallJoint common landmarks through the large one; the rest through the workspace
        hipLaunchKernelGGL(pair_lds_kernel<kPairSmallJoint>, dim3((unsigned)npairs), dim3(kT), 0, st, a);
        check_launch("pair_lds_kernel (small)");
        XM_HIP_CHECK(hipMemcpyAsync(hcnt, dcnt.p, sizeof(hcnt), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the pairs");
        if (hcnt[C_OVER_SMALL] > 0) {
            dover2.alloc((size_t)hcnt[C_OVER_SMALL], false);
            a.work = dover1.p; a.nwork = (int32_t)hcnt[C_OVER_SMALL]; a.overflow = dover2.p; a.over_slot = C_OVER_LDS; a.first = 0;
            hipLaunchKernelGGL(pair_lds_kernel<kCap>, dim3((unsigned)a.nwork), dim3(kT), 0, st, a);
            check_launch("pair_lds_kernel (large)");
            XM_HIP_CHECK(hipMemcpyAsync(hcnt, dcnt.p, sizeof(hcnt), hipMemcpyDeviceToHost, st));
            wait_stream(st, cfg.watchdog_s, kStage, "the larger pairs");
        }
        const int64_t nover = hcnt[C_OVER_LDS];
        out.pairs_on_workspace_path = nover;
        if (nover > 0) {
            int64_t cap = 2 * (int64_t)kCap;
            while (cap < (int64_t)hcnt[C_MAX_JOINT]) cap <<= 1;
            const int groups = (int)std::min<int64_t>(nover, kPairWsGroups);
            ws.alloc((size_t)groups * (size_t)cap * 16, false);
            a.work = dover2.p; a.nwork = (int32_t)nover; a.first = 0; a.ws = ws.p; a.ws_cap = (int32_t)cap;
            hipLaunchKernelGGL(pair_ws_kernel, dim3((unsigned)groups), dim3(kT), 0, st, a);
            check_launch("pair_ws_kernel");
        }
    }
    if (nobs > 0) {
        hipLaunchKernelGGL(pair_outlier_kernel, dim3((unsigned)std::min<int64_t>((nobs + kT - 1) / kT, 2048)), dim3(kT), 0, st, nobs, dcount.p, cfg.min_flags, doutlier.p, dcnt.p);
        check_launch("pair_outlier_kernel");
    }
    XM_HIP_CHECK(hipMemcpyAsync(hcnt, dcnt.p, sizeof(hcnt), hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the flags");
    out.seconds_kernels = secs_since(t_kernels);
    const auto t_down = std::chrono::steady_clock::now();
    if (nobs > 0) {
        XM_HIP_CHECK(hipMemcpyAsync(count, dcount.p, (size_t)nobs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(outlier, doutlier.p, (size_t)nobs, hipMemcpyDeviceToHost, st));
    }
    if (stats && npairs > 0) XM_HIP_CHECK(hipMemcpyAsync(stats, dstats.p, (size_t)npairs * sizeof(xm_pair_stat_t), hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the download");
    out.seconds_download = secs_since(t_down);
    out.pairs_used = hcnt[C_USED]; out.pairs_skipped = hcnt[C_TOO_FEW]; out.pairs_degenerate = hcnt[C_DEGENERATE];
    out.nobs_flagged = hcnt[C_FLAGGED]; out.max_joint = hcnt[C_MAX_JOINT];
    if (out.pairs_used + out.pairs_skipped + out.pairs_degenerate != npairs)
        throw Error(XM_ERR_HIP, "pair filter: the pairs that reported do not add up to the pairs listed");
}

}  // namespace

void pair_filter_host(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *p, int64_t npairs, const int32_t *pi,
                      const int32_t *pj, const double *R, const PairSettings &cfg, int32_t *count, uint8_t *outlier, xm_pair_stat_t *stats,
                      PairOutcome &out) {
    const auto t_start = std::chrono::steady_clock::now();
    out = PairOutcome();
    for (int64_t e = 0; e < nobs; ++e) {
        if (cam[e] < 0 || cam[e] >= n) throw Error(XM_ERR_ARG, "xm_pair_filter: camera index out of range at observation " + std::to_string(e));
        if (lm[e] < 0 || lm[e] >= m) throw Error(XM_ERR_ARG, "xm_pair_filter: landmark index out of range at observation " + std::to_string(e));
    }
    for (int64_t k = 0; k < npairs; ++k) {
        if (pi[k] < 0 || pi[k] >= n || pj[k] < 0 || pj[k] >= n) throw Error(XM_ERR_ARG, "xm_pair_filter: camera index out of range at pair " + std::to_string(k));
        if (pi[k] == pj[k]) throw Error(XM_ERR_ARG, "xm_pair_filter: pair " + std::to_string(k) + " names one camera twice");
    }
    // the list by camera (a counting pass), every camera's observations by landmark (a sort of its (landmark, row) words)
    std::vector<int32_t> first((size_t)n + 1, 0);
    for (int64_t e = 0; e < nobs; ++e) first[(size_t)cam[e] + 1] += 1;
    for (int64_t c = 0; c < n; ++c) first[(size_t)c + 1] += first[(size_t)c];
    std::vector<u64> ent((size_t)nobs);
    {
        std::vector<int32_t> next(first.begin(), first.end() - 1);
        for (int64_t e = 0; e < nobs; ++e) ent[(size_t)next[(size_t)cam[e]]++] = ((u64)(uint32_t)lm[e] << 32) | (u64)(uint32_t)e;
    }
    std::vector<int32_t> camptr((size_t)n + 1, 0), slm, srow;
    slm.reserve((size_t)nobs); srow.reserve((size_t)nobs);
    for (int64_t c = 0; c < n; ++c) {
        const auto b = ent.begin() + first[(size_t)c], e = ent.begin() + first[(size_t)c + 1];
        std::sort(b, e);
        for (auto q = b; q != e; ++q) {
            if (q != b && (*q >> 32) == (*(q - 1) >> 32))
                throw Error(XM_ERR_ARG, "xm_pair_filter: the observation list names a (camera, landmark) pair twice (camera " + std::to_string(c) +
                                            ", landmark " + std::to_string(*q >> 32) + ")");
            const int32_t row = (int32_t)(*q & 0xFFFFFFFFull);
            if (cfg.skip_row0 && row == 0) continue;   // the reference's row 0 is "not visible"
            slm.push_back((int32_t)(*q >> 32));
            srow.push_back(row);
        }
        camptr[(size_t)c + 1] = (int32_t)slm.size();
    }
    // pairs to workgroups by descending bound on the joint size (the shorter of the two lists), ties in listed order: a counting sort
    auto bound = [&](int64_t k) { return std::min(camptr[(size_t)pi[k] + 1] - camptr[(size_t)pi[k]], camptr[(size_t)pj[k] + 1] - camptr[(size_t)pj[k]]); };
    int32_t longest = 0;
    for (int64_t c = 0; c < n; ++c) longest = std::max(longest, camptr[(size_t)c + 1] - camptr[(size_t)c]);
    std::vector<int64_t> slot((size_t)longest + 2, 0);
    for (int64_t k = 0; k < npairs; ++k) slot[(size_t)bound(k)] += 1;
    int64_t run = 0;
    for (int64_t b = longest; b >= 0; --b) { const int64_t here = slot[(size_t)b]; slot[(size_t)b] = run; run += here; }
    std::vector<int32_t> order((size_t)npairs);
    for (int64_t k = 0; k < npairs; ++k) order[(size_t)slot[(size_t)bound(k)]++] = (int32_t)k;

    hipStream_t st = nullptr;   // the default stream, as xm_clean_observations
    try {
        run_device(n, nobs, p, npairs, pi, pj, R, camptr, slm, srow, order, cfg, count, outlier, stats, out, t_start, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the device buffers are freed next: nothing may still be reading them
        throw;
    }
}

}  // namespace xm
