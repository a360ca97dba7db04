// xm_lift.hip — the depth lift on the device (xm_lift.h; definition in include/xm_amd.h at xm_lift_observations).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "xm_lift.h"
#include "xm_device.h"
#include "xm_stage.h"

// every product and every sum below is rounded on its own: the percentile is numpy's, and the point is the definition's three-term sum
#pragma clang fp contract(off)
#include "xm_sortstat.h"   // behind the pragma: its percentile is compiled without contraction too

namespace xm {
namespace {

constexpr int kT = kLiftThreads;
static_assert(kT == kStageThreads && kT == kSortThreads, "the helpers of xm_stage.h and xm_sortstat.h are written for this workgroup size");
constexpr const char *kStage = "lift";

// what a slot's code says when it is negative; a code >= 0 is the row's rank among its camera's survivors
enum { S_DUPLICATE = -1, S_BORDER = -2, S_DEPTH = -3, S_NO_MAP = -4 };
// per camera: four counts
enum { N_KEPT = 0, N_DUPLICATE, N_BORDER, N_DEPTH, N_COUNTS };

struct LiftArgs {
    const int32_t *cam, *lm;              // per input row
    const double *xy;                     // 2 per input row
    const int32_t *hw;                    // 2 per camera
    const float *const *depth;            // per camera; null: the camera has no map.  Host maps: only compared with null
    const float *const *conf;             // per camera or null altogether
    const float *sd, *sc;                 // host maps: the samples per input row (rows inside the border of a camera with a map); else null
    const double *Kinv;                   // 9 per camera
    const int32_t *camptr;                // n + 1: the camera's slots
    int32_t *srow;                        // per slot: in, the camera's rows in any order; out, in (landmark, row) order
    int32_t *code;                        // per slot
    float *dval, *wval;                   // per slot: the depth of a row inside the border, the weight of a survivor
    int32_t *camcnt;                      // N_COUNTS per camera
    double *thr;                          // per camera
    const int32_t *work;                  // the cameras of this launch; null: every camera, the workgroup's number
    int32_t nwork;
    int32_t margin;
    double q;                             // the percentile as a fraction
    char *ws;                             // workspace kernel: ws_cap * 12 bytes per workgroup
    int32_t ws_cap;
};

__device__ inline float inf32_() { return __int_as_float(0x7f800000); }
__device__ inline double nan_() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline bool inside(int u, int v, int h, int w, int mg) { return u >= mg && u < w - mg && v >= mg && v < h - mg; }

struct Scratch { int ired[4]; int wtot[4]; };

// one camera by one workgroup.  K: the (landmark << 32 | input row) words, S: the sampled depths -- as float32, which is what they are: widening
// keeps their order, and the percentile widens the two it reads; KP entries each are used
template <class PK, class PD>
__device__ inline void run_camera(const LiftArgs &a, int c, PK K, PD S, Scratch &sc) {
    const int tid = (int)threadIdx.x;
    const int b = a.camptr[c], k = a.camptr[c + 1] - b;
    if (k == 0) {
        if (tid == 0) {
            a.thr[c] = nan_();
#pragma unroll
            for (int x = 0; x < N_COUNTS; ++x) a.camcnt[(size_t)c * N_COUNTS + x] = 0;
        }
        return;
    }
    int KP = 2;
    while (KP < k) KP <<= 1;
    // 1. the rows by (landmark, input row): the first of every landmark is the one that stays
    for (int q = tid; q < KP; q += kT) {
        u64 key = ~0ull;
        if (q < k) {
            const int row = a.srow[b + q];
            key = ((u64)(uint32_t)a.lm[row] << 32) | (u64)(uint32_t)row;
        }
        K[q] = key;
    }
    __syncthreads();
    sort_values(K, KP);
    // 2., 3. the pixel, the border, the sample
    const float *D = a.depth[c];
    const float *C = a.conf ? a.conf[c] : nullptr;
    const int h = a.hw[2 * c], w = a.hw[2 * c + 1], mg = a.margin;
    int ndup = 0, nborder = 0, ncand = 0, nbad = 0;
    for (int q = tid; q < KP; q += kT) {
        float s = inf32_();
        if (q < k) {
            const u64 key = K[q];
            const int row = (int)(uint32_t)(key & 0xffffffffull);
            int cd = 0;
            if (q > 0 && (K[q - 1] >> 32) == (key >> 32)) { cd = S_DUPLICATE; ndup += 1; }
            else if (!D) cd = S_NO_MAP;
            else {
                const int u = (int)a.xy[2 * (size_t)row], v = (int)a.xy[2 * (size_t)row + 1];
                if (!inside(u, v, h, w, mg)) { cd = S_BORDER; nborder += 1; }
                else {
                    const float d = a.sd ? a.sd[row] : D[(size_t)v * (size_t)w + (size_t)u];
                    a.dval[b + q] = d;
                    ncand += 1;
                    if (d != d) nbad += 1; else s = d;   // (a value that is not a number has no place in the order)
                }
            }
            a.code[b + q] = cd;
            a.srow[b + q] = row;
        }
        S[q] = s;
    }
    ndup = block_sum_int(ndup, sc.ired);
    nborder = block_sum_int(nborder, sc.ired);
    ncand = block_sum_int(ncand, sc.ired);
    nbad = block_sum_int(nbad, sc.ired);
    if (ncand == 0) {
        if (tid == 0) {
            a.thr[c] = nan_();
            int32_t *cc = a.camcnt + (size_t)c * N_COUNTS;
            cc[N_KEPT] = 0; cc[N_DUPLICATE] = ndup; cc[N_BORDER] = nborder; cc[N_DEPTH] = 0;
        }
        return;
    }
    // 4. the threshold
    sort_values(S, KP);
    double thr = nbad ? nan_() : percentile(S, ncand, a.q);
    if (thr != thr) thr = nan_();
    __syncthreads();
    // 5., 7. every row's decision, the survivors' ranks in (landmark) order and their weights
    int base = 0;
    for (int t0 = 0; t0 < k; t0 += kT) {
        const int q = t0 + tid;
        const bool cand = q < k && a.code[b + q] == 0;
        bool kp = false;
        if (cand) {
            const float d = a.dval[b + q];
            kp = d > 0.0f && (double)d < thr;
        }
        const u64 mask = __ballot(kp);
        const int before = __popcll(mask & ((1ull << lane_id()) - 1ull));
        if (lane_id() == 0) sc.wtot[tid >> 6] = __popcll(mask);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) { if (x < (tid >> 6)) off += sc.wtot[x]; tot += sc.wtot[x]; }
        if (cand) {
            if (kp) {
                const int row = a.srow[b + q];
                float cv = 1.0f;
                if (a.sc) cv = a.sc[row];
                else if (C) {
                    const int u = (int)a.xy[2 * (size_t)row], v = (int)a.xy[2 * (size_t)row + 1];
                    cv = C[(size_t)v * (size_t)w + (size_t)u];
                }
                a.wval[b + q] = cv * cv;
                a.code[b + q] = off + before;
            } else a.code[b + q] = S_DEPTH;
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) {
        a.thr[c] = thr;
        int32_t *cc = a.camcnt + (size_t)c * N_COUNTS;
        cc[N_KEPT] = base; cc[N_DUPLICATE] = ndup; cc[N_BORDER] = nborder; cc[N_DEPTH] = ncand - base;
    }
}

// 12 bytes of LDS per row.  CAP = kLiftSmallRows: 3 KB; CAP = kLiftLdsRows: 48 KB, three workgroups per CU
template <int CAP>
__global__ __launch_bounds__(kT) void lift_cam_kernel(LiftArgs a) {
    __shared__ u64 K[CAP];
    __shared__ float S[CAP];
    __shared__ Scratch sc;
    if ((int)blockIdx.x >= a.nwork) return;
    const int c = a.work ? a.work[blockIdx.x] : (int)blockIdx.x;
    if (a.camptr[c + 1] - a.camptr[c] > CAP) return;   // (the host lists it for a larger size)
    run_camera(a, c, K, S, sc);
}
__global__ __launch_bounds__(kT) void lift_cam_ws_kernel(LiftArgs a) {
    __shared__ Scratch sc;
    char *mine = a.ws + (size_t)blockIdx.x * (size_t)a.ws_cap * 12;
    u64 *K = (u64 *)mine;
    float *S = (float *)(mine + (size_t)a.ws_cap * 8);
    for (int x = (int)blockIdx.x; x < a.nwork; x += (int)gridDim.x) {
        const int c = a.work[x];
        if (a.camptr[c + 1] - a.camptr[c] <= a.ws_cap) run_camera(a, c, K, S, sc);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kT) void lift_hist_kernel(int64_t nrows, const int32_t *cam, int32_t *cnt) {
    for (int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * kT) atomicAdd(cnt + cam[r], 1);
}
__global__ __launch_bounds__(kT) void lift_scatter_kernel(int64_t nrows, const int32_t *cam, int32_t *cursor, int32_t *srow) {
    for (int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * kT) srow[atomicAdd(cursor + cam[r], 1)] = (int32_t)r;
}
// out[i] = in[0] + in[stride] + ... + in[(i - 1) * stride] for i = 0 .. n: one workgroup
__global__ __launch_bounds__(kT) void lift_scan_kernel(const int32_t *in, int stride, int32_t *out, int n) {
    __shared__ int wt[4];
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += kT) {
        const int i = base + tid;
        const int v = i < n ? in[(size_t)i * (size_t)stride] : 0;
        int x = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) wt[wave] = x;
        __syncthreads();
        int pre = carry, tot = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) { if (s < wave) pre += wt[s]; tot += wt[s]; }
        if (i < n) out[i] = pre + x - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) out[n] = carry;
}
// 8., 9. one thread per slot: a survivor goes to (its camera's offset + its rank)
__global__ __launch_bounds__(kT) void lift_emit_kernel(int64_t nrows, LiftArgs a, const int32_t *off, int32_t *ocam, int32_t *olm, double *op, double *ow,
                                                       int32_t *orow) {
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < nrows; e += (int64_t)gridDim.x * kT) {
        const int cd = a.code[e];
        if (cd < 0) continue;
        const int row = a.srow[e], c = a.cam[row];
        const size_t o = (size_t)off[c] + (size_t)cd;
        const double u = (double)(int)a.xy[2 * (size_t)row], v = (double)(int)a.xy[2 * (size_t)row + 1];
        const double d = (double)a.dval[e];
        const double *Ki = a.Kinv + (size_t)c * 9;
        ocam[o] = c; olm[o] = a.lm[row]; orow[o] = row;
#pragma unroll
        for (int x = 0; x < 3; ++x) op[3 * o + x] = ((Ki[3 * x] * u + Ki[3 * x + 1] * v) + Ki[3 * x + 2]) * d;
        ow[o] = (double)a.wval[e];
    }
}

void run_device(int64_t n, int64_t nrows, const int32_t *cam, const int32_t *lm, const double *xy, const int32_t *hw, const float *const *depth,
                const float *const *conf, const double *Kinv, const std::vector<float> &sd, const std::vector<float> &sc, const LiftSettings &cfg,
                int32_t *out_cam, int32_t *out_lm, double *out_p, double *out_w, int32_t *out_row, double *threshold, LiftOutcome &out,
                std::chrono::steady_clock::time_point t_start, hipStream_t st) {
    DevBuf<int32_t> dcam, dlm, dhw, dcnt, dcamptr, dcursor, dsrow, dcode, dcamcnt, doff, dlarge, dwsl, docam, dolm, dorow;
    DevBuf<double> dxy, dK, dthr, dop, dow;
    DevBuf<float> dsd, dsc, ddval, dwval;
    DevBuf<const float *> ddepth, dconf;
    DevBuf<char> ws;
    upload(dcam, cam, (size_t)nrows, st);
    upload(dlm, lm, (size_t)nrows, st);
    upload(dxy, xy, (size_t)nrows * 2, st);
    upload(dhw, hw, (size_t)n * 2, st);
    upload(dK, Kinv, (size_t)n * 9, st);
    upload(ddepth, depth, (size_t)n, st);
    if (conf) upload(dconf, conf, (size_t)n, st);
    if (!cfg.maps_on_device) {
        upload(dsd, sd.data(), sd.size(), st);
        if (conf) upload(dsc, sc.data(), sc.size(), st);
    }
    dcnt.alloc((size_t)n, false); dcamptr.alloc((size_t)n + 1, false); dcursor.alloc((size_t)n, false);
    dsrow.alloc((size_t)nrows, false); dcode.alloc((size_t)nrows, false); ddval.alloc((size_t)nrows, false); dwval.alloc((size_t)nrows, false);
    dcamcnt.alloc((size_t)n * N_COUNTS, false); doff.alloc((size_t)n + 1, false); dthr.alloc((size_t)n, false);
    docam.alloc((size_t)nrows, false); dolm.alloc((size_t)nrows, false); dorow.alloc((size_t)nrows, false);
    dop.alloc((size_t)nrows * 3, false); dow.alloc((size_t)nrows, false);
    // binning: a counting sort of the rows by camera
    XM_HIP_CHECK(hipMemsetAsync(dcnt.p, 0, (size_t)n * sizeof(int32_t), st));
    hipLaunchKernelGGL(lift_hist_kernel, dim3(grid_for(nrows, 2048)), dim3(kT), 0, st, nrows, dcam.p, dcnt.p);
    check_launch("lift_hist_kernel");
    hipLaunchKernelGGL(lift_scan_kernel, dim3(1), dim3(kT), 0, st, dcnt.p, 1, dcamptr.p, (int)n);
    check_launch("lift_scan_kernel (rows)");
    XM_HIP_CHECK(hipMemcpyAsync(dcursor.p, dcamptr.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(lift_scatter_kernel, dim3(grid_for(nrows, 2048)), dim3(kT), 0, st, nrows, dcam.p, dcursor.p, dsrow.p);
    check_launch("lift_scatter_kernel");
    std::vector<int32_t> camptr((size_t)n + 1);
    XM_HIP_CHECK(hipMemcpyAsync(camptr.data(), dcamptr.p, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the binning");
    if (camptr[(size_t)n] != nrows) throw Error(XM_ERR_HIP, "lift: the cameras' rows do not add up to the rows listed");
    // which cameras need a larger size than the one all of them start in
    std::vector<int32_t> large, wsl;
    for (int64_t c = 0; c < n; ++c) {
        const int64_t k = camptr[(size_t)c + 1] - camptr[(size_t)c];
        out.max_rows = std::max(out.max_rows, k);
        if (k > kLiftLdsRows) wsl.push_back((int32_t)c);
        else if (k > kLiftSmallRows) large.push_back((int32_t)c);
        else if (k > 0) out.cams_small += 1;
    }
    if (out.max_rows > ((int64_t)1 << 30)) throw Error(XM_ERR_ARG, "xm_lift_observations: more than 2^30 rows of one camera");   // (the sort pads to a power of two)
    out.cams_large = (int64_t)large.size(); out.cams_workspace = (int64_t)wsl.size();
    if (!large.empty()) upload(dlarge, large.data(), large.size(), st);
    if (!wsl.empty()) upload(dwsl, wsl.data(), wsl.size(), st);
    wait_stream(st, cfg.watchdog_s, kStage, "the camera lists");
    out.seconds_index = secs_since(t_start);
    const auto t_kernels = std::chrono::steady_clock::now();

    LiftArgs a;
    a.cam = dcam.p; a.lm = dlm.p; a.xy = dxy.p; a.hw = dhw.p; a.depth = ddepth.p; a.conf = conf ? dconf.p : nullptr;
    a.sd = cfg.maps_on_device ? nullptr : dsd.p; a.sc = (cfg.maps_on_device || !conf) ? nullptr : dsc.p;
    a.Kinv = dK.p; a.camptr = dcamptr.p; a.srow = dsrow.p; a.code = dcode.p; a.dval = ddval.p; a.wval = dwval.p; a.camcnt = dcamcnt.p; a.thr = dthr.p;
    a.work = nullptr; a.nwork = (int32_t)n; a.margin = cfg.margin; a.q = cfg.depth_pct / 100.0; a.ws = nullptr; a.ws_cap = 0;
    hipLaunchKernelGGL(lift_cam_kernel<kLiftSmallRows>, dim3((unsigned)n), dim3(kT), 0, st, a);
    check_launch("lift_cam_kernel (small)");
    if (!large.empty()) {
        a.work = dlarge.p; a.nwork = (int32_t)large.size();
        hipLaunchKernelGGL(lift_cam_kernel<kLiftLdsRows>, dim3((unsigned)a.nwork), dim3(kT), 0, st, a);
        check_launch("lift_cam_kernel (large)");
    }
    if (!wsl.empty()) {
        int64_t cap = 2 * (int64_t)kLiftLdsRows;
        while (cap < out.max_rows) cap <<= 1;
        const int groups = (int)std::min<int64_t>((int64_t)wsl.size(), kLiftWsGroups);
        ws.alloc((size_t)groups * (size_t)cap * 12, false);
        a.work = dwsl.p; a.nwork = (int32_t)wsl.size(); a.ws = ws.p; a.ws_cap = (int32_t)cap;
        hipLaunchKernelGGL(lift_cam_ws_kernel, dim3((unsigned)groups), dim3(kT), 0, st, a);
        check_launch("lift_cam_ws_kernel");
    }
    hipLaunchKernelGGL(lift_scan_kernel, dim3(1), dim3(kT), 0, st, dcamcnt.p + N_KEPT, (int)N_COUNTS, doff.p, (int)n);
    check_launch("lift_scan_kernel (survivors)");
    hipLaunchKernelGGL(lift_emit_kernel, dim3(grid_for(nrows, 2048)), dim3(kT), 0, st, nrows, a, doff.p, docam.p, dolm.p, dop.p, dow.p, dorow.p);
    check_launch("lift_emit_kernel");
    std::vector<int32_t> camcnt((size_t)n * N_COUNTS);
    int32_t total = 0;
    XM_HIP_CHECK(hipMemcpyAsync(camcnt.data(), dcamcnt.p, camcnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(&total, doff.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the cameras");
    out.seconds_kernels = secs_since(t_kernels);
    const auto t_down = std::chrono::steady_clock::now();
    if (total < 0 || total > nrows) throw Error(XM_ERR_HIP, "lift: more survivors than rows");
    const size_t no = (size_t)total;
    if (no) {
        XM_HIP_CHECK(hipMemcpyAsync(out_cam, docam.p, no * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(out_lm, dolm.p, no * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(out_row, dorow.p, no * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(out_p, dop.p, no * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(out_w, dow.p, no * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (threshold) XM_HIP_CHECK(hipMemcpyAsync(threshold, dthr.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the download");
    out.seconds_download = secs_since(t_down);
    out.nout = total;
    int64_t accounted = total;
    for (int64_t c = 0; c < n; ++c) {
        const int32_t *cc = camcnt.data() + (size_t)c * N_COUNTS;
        const int64_t k = camptr[(size_t)c + 1] - camptr[(size_t)c];
        out.rows_duplicate += cc[N_DUPLICATE]; out.rows_border += cc[N_BORDER]; out.rows_depth += cc[N_DEPTH];
        if (!depth[c]) { out.cams_no_map += 1; out.rows_no_map += k - cc[N_DUPLICATE]; }
        else if (cc[N_KEPT] == 0) out.cams_empty += 1;
    }
    accounted += out.rows_duplicate + out.rows_border + out.rows_depth + out.rows_no_map;
    if (accounted != nrows) throw Error(XM_ERR_HIP, "lift: the rows that reported do not add up to the rows listed");
}

}  // namespace

void lift_observations_host(int64_t n, int64_t m, int64_t nrows, const int32_t *cam, const int32_t *lm, const double *xy, const int32_t *hw,
                            const float *const *depth, const float *const *conf, const double *Kinv, const LiftSettings &cfg, int32_t *out_cam,
                            int32_t *out_lm, double *out_p, double *out_w, int32_t *out_row, double *threshold, LiftOutcome &out) {
    const auto t_start = std::chrono::steady_clock::now();
    out = LiftOutcome();
    for (int64_t c = 0; c < n; ++c)
        if (depth[c] && (hw[2 * c] <= 0 || hw[2 * c + 1] <= 0))
            throw Error(XM_ERR_ARG, "xm_lift_observations: camera " + std::to_string(c) + " has a map of height or width <= 0");
    const double lim = 2147483648.0;
    for (int64_t r = 0; r < nrows; ++r) {
        if (cam[r] < 0 || cam[r] >= n) throw Error(XM_ERR_ARG, "xm_lift_observations: camera index out of range at row " + std::to_string(r));
        if (lm[r] < 0 || lm[r] >= m) throw Error(XM_ERR_ARG, "xm_lift_observations: landmark index out of range at row " + std::to_string(r));
        const double x = xy[2 * r], y = xy[2 * r + 1];
        if (!(std::fabs(x) < lim) || !(std::fabs(y) < lim))   // (not a number and infinite fail this too)
            throw Error(XM_ERR_ARG, "xm_lift_observations: a pixel position that is not finite or not below 2^31 at row " + std::to_string(r));
    }
    if (n == 0 || nrows == 0) {   // nothing to launch
        for (int64_t c = 0; c < n; ++c) {
            if (threshold) threshold[c] = std::numeric_limits<double>::quiet_NaN();
            if (depth[c]) out.cams_empty += 1; else out.cams_no_map += 1;
        }
        return;
    }
    // host maps: sampled here, so that only the samples travel; everything behind the sampling is the device code of the other transport
    std::vector<float> sd, sc;
    if (!cfg.maps_on_device) {
        sd.assign((size_t)nrows, 0.0f);
        if (conf) sc.assign((size_t)nrows, 1.0f);
        for (int64_t r = 0; r < nrows; ++r) {
            const int32_t c = cam[r];
            if (!depth[c]) continue;
            const int h = hw[2 * c], w = hw[2 * c + 1], mg = cfg.margin;
            const int u = (int)xy[2 * r], v = (int)xy[2 * r + 1];
            if (!(u >= mg && u < w - mg && v >= mg && v < h - mg)) continue;
            const size_t px = (size_t)v * (size_t)w + (size_t)u;
            sd[(size_t)r] = depth[c][px];
            if (conf && conf[c]) sc[(size_t)r] = conf[c][px];
        }
    }
    hipStream_t st = nullptr;   // the default stream, as xm_pair_filter
    try {
        run_device(n, nrows, cam, lm, xy, hw, depth, conf, Kinv, sd, sc, cfg, out_cam, out_lm, out_p, out_w, out_row, threshold, out, t_start, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the device buffers are freed next: nothing may still be reading them
        throw;
    }
}

}  // namespace xm
