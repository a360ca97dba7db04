// xm_tracks.hip — feature tracks from pairwise matches on the device (xm_tracks.h; definition in include/xm_amd.h at xm_build_tracks).
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "xm_tracks.h"
#include "xm_tracks_split.h"
#include "xm_stage.h"

// the distance test of XM_TRACKS_GLOMAP is sqrt(dx*dx + dy*dy) with every product and the sum rounded on its own
#pragma clang fp contract(off)
#include "xm_sortstat.h"

namespace xm {
namespace {

constexpr int kT = kTracksThreads;
static_assert(kT == kStageThreads && kT == kSortThreads, "the helpers of xm_stage.h and xm_sortstat.h are written for this workgroup size");
static_assert((kTracksSmallRows & (kTracksSmallRows - 1)) == 0 && (kTracksLdsRows & (kTracksLdsRows - 1)) == 0, "the sort pads to a power of two");
constexpr const char *kStage = "tracks";

// slots of the device counter block
enum { C_TOUCHED = 0, C_COMPONENTS, C_CONFLICTED, C_ROWS_CONFLICTED, C_NSPLIT, C_SHORT, C_LONG, C_CONFLICT, C_FEW, C_NTRACKS, C_NOUT, C_COUNT };
// a component's flag word
enum { F_CONFLICT = 1, F_FAR = 2 };

// one thread per match: the endpoints as global feature ids, smaller first; -1, -1 and the match's number in *firstbad when an index is out of range
__global__ __launch_bounds__(kT) void tracks_expand_kernel(int64_t E, int npairs, const int64_t *moff, const int32_t *pi, const int32_t *pj, const int64_t *foff,
                                                           const int32_t *f1, const int32_t *f2, int32_t *eu, int32_t *ev, int32_t *touched, int32_t *firstbad) {
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < E; e += (int64_t)gridDim.x * kT) {
        const int k = owner_of(moff, npairs, e);
        const int a = pi[k], b = pj[k];   // (checked on the host)
        const int64_t a0 = foff[a], b0 = foff[b];
        const int64_t x = f1[e], y = f2[e];
        if (x < 0 || x >= foff[a + 1] - a0 || y < 0 || y >= foff[b + 1] - b0) {
            eu[e] = -1; ev[e] = -1;
            atomicMin(firstbad, (int32_t)e);
            continue;
        }
        const int32_t u = (int32_t)(a0 + x), v = (int32_t)(b0 + y);
        eu[e] = u < v ? u : v; ev[e] = u < v ? v : u;
        touched[u] = 1; touched[v] = 1;   // (every writer stores the same value)
    }
}
__global__ __launch_bounds__(kT) void tracks_feat_kernel(int F, int n, const int64_t *foff, const int32_t *touched, int32_t *fimg, int32_t *p, int32_t *tcnt) {
    for (int base = (int)blockIdx.x * kT; base < F; base += (int)gridDim.x * kT) {
        const int g = base + (int)threadIdx.x;
        const bool in = g < F;
        const int img = in ? owner_of(foff, n, g) : 0;
        if (in) { fimg[g] = img; p[g] = g; }
        wave_add_one(tcnt, img, in && touched[g] != 0);
    }
}

// components: labels p over the features; a match whose indices are in range is an edge
struct TracksEdge {
    const int32_t *eu, *ev;
    __device__ bool operator()(int64_t e, int &u, int &v) const {
        u = eu[e]; v = ev[e];
        return u >= 0;
    }
};

struct ImgArgs {
    const int64_t *foff;
    const int32_t *touched, *p, *tcnt;
    const double *xy;
    const uint8_t *reg;        // null: every image is registered
    int32_t *cflag, *cdupreg;  // per label
    const int32_t *work;       // the images of this launch; null: every image, the workgroup's number
    int32_t nwork;
    int32_t glomap;
    double thres;
    u64 *ws;                   // workspace kernel: ws_cap words per workgroup
    int32_t ws_cap;
};
struct Scratch { int wtot[4]; };

// one image by one workgroup; K holds cap words, the image has at most cap touched features
template <class PK>
__device__ inline void run_image(const ImgArgs &a, int i, PK K, int cap, Scratch &sc) {
    const int tid = (int)threadIdx.x;
    const int t = a.tcnt[i];
    if (t < 2) return;   // (no two features: no conflict)
    const int64_t b = a.foff[i];
    const int nf = (int)(a.foff[i + 1] - b);
    // the touched features' words in feature order
    int base = 0;
    for (int c0 = 0; c0 < nf; c0 += kT) {
        const int q = c0 + tid;
        const bool on = q < nf && a.touched[b + q] != 0;
        const u64 mask = __ballot(on);
        const int before = __popcll(mask & ((1ull << lane_id()) - 1ull));
        if (lane_id() == 0) sc.wtot[tid >> 6] = __popcll(mask);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) { if (x < (tid >> 6)) off += sc.wtot[x]; tot += sc.wtot[x]; }
        if (on && off + before < cap) K[off + before] = ((u64)(uint32_t)a.p[b + q] << 32) | (u64)(uint32_t)(b + q);
        base += tot;
        __syncthreads();
    }
    int KP = 2;
    while (KP < t) KP <<= 1;
    for (int q = t + tid; q < KP; q += kT) K[q] = ~0ull;
    __syncthreads();
    sort_values(K, KP);
    const bool reg = !a.reg || a.reg[i] != 0;
    for (int q = 1 + tid; q < t; q += kT) {
        const u64 key = K[q];
        const uint32_t lab = (uint32_t)(key >> 32);
        if ((uint32_t)(K[q - 1] >> 32) != lab) continue;
        int bits = F_CONFLICT;
        if (a.glomap) {   // every earlier feature of the run against this one: all pairs of the run are looked at once
            const size_t g = (size_t)(key & 0xffffffffull);
            const double x = a.xy[2 * g], y = a.xy[2 * g + 1];
            for (int r = q - 1; r >= 0 && (uint32_t)(K[r] >> 32) == lab; --r) {
                const size_t h = (size_t)(K[r] & 0xffffffffull);
                const double dx = x - a.xy[2 * h], dy = y - a.xy[2 * h + 1];
                if (sqrt(dx * dx + dy * dy) > a.thres) bits = F_CONFLICT | F_FAR;
            }
        }
        atomicOr(a.cflag + lab, bits);
        if (reg) atomicAdd(a.cdupreg + lab, 1);
    }
}
// 8 bytes of LDS per touched feature.  CAP = kTracksSmallRows: 2 KB; CAP = kTracksLdsRows: 32 KB
template <int CAP>
__global__ __launch_bounds__(kT) void tracks_image_kernel(ImgArgs a) {
    __shared__ u64 K[CAP];
    __shared__ Scratch sc;
    if ((int)blockIdx.x >= a.nwork) return;
    const int i = a.work ? a.work[blockIdx.x] : (int)blockIdx.x;
    if (a.tcnt[i] > CAP) return;   // (the host lists it for a larger size)
    run_image(a, i, K, CAP, sc);
}
__global__ __launch_bounds__(kT) void tracks_image_ws_kernel(ImgArgs a) {
    __shared__ Scratch sc;
    u64 *K = a.ws + (size_t)blockIdx.x * (size_t)a.ws_cap;
    for (int x = (int)blockIdx.x; x < a.nwork; x += (int)gridDim.x) {
        const int i = a.work[x];
        if (a.tcnt[i] <= a.ws_cap) run_image(a, i, K, a.ws_cap, sc);
        __syncthreads();
    }
}

__device__ inline bool is_registered(const uint8_t *reg, int img) { return !reg || reg[img] != 0; }

// rows, and rows in registered images, per component (at its label)
__global__ __launch_bounds__(kT) void tracks_size_kernel(int F, const int32_t *touched, const int32_t *p, const int32_t *fimg, const uint8_t *reg,
                                                         int32_t *size, int32_t *regc) {
    const int g = (int)(blockIdx.x * kT + threadIdx.x);
    if (g >= F || !touched[g]) return;
    const int r = p[g];
    atomicAdd(size + r, 1);
    if (is_registered(reg, fimg[g])) atomicAdd(regc + r, 1);
}
__global__ __launch_bounds__(kT) void tracks_stats_kernel(int F, const int32_t *touched, const int32_t *p, const int32_t *size, const int32_t *cflag, u64 *cnt) {
    const int g = (int)(blockIdx.x * kT + threadIdx.x);
    const bool on = g < F && touched[g] != 0;
    const bool root = on && p[g] == g;
    const bool conf = root && cflag[g] != 0;
    wave_sum_to(cnt + C_TOUCHED, on, 1ull);
    wave_sum_to(cnt + C_COMPONENTS, root, 1ull);
    wave_sum_to(cnt + C_CONFLICTED, conf, 1ull);
    wave_sum_to(cnt + C_ROWS_CONFLICTED, conf, conf ? (u64)(uint32_t)size[g] : 0ull);
}
// the edges of flagged components, as (smaller id << 32 | larger id), in an arbitrary order (the host splitter sorts them)
__global__ __launch_bounds__(kT) void tracks_compact_kernel(int64_t E, const int32_t *eu, const int32_t *ev, const int32_t *p, const int32_t *cflag, u64 *cnt,
                                                            u64 *out) {
    for (int64_t base = (int64_t)blockIdx.x * kT; base < E; base += (int64_t)gridDim.x * kT) {
        const int64_t e = base + threadIdx.x;
        const int u = e < E ? eu[e] : -1;
        const bool on = u >= 0 && cflag[p[u]] != 0;
        const u64 mask = __ballot(on);
        if (!mask) continue;
        const int leader = __ffsll((long long)mask) - 1;
        u64 first = 0;
        if (lane_id() == leader) first = atomicAdd(cnt + C_NSPLIT, (u64)__popcll(mask));
        first = __shfl(first, leader);
        if (on) out[first + (u64)__popcll(mask & ((1ull << lane_id()) - 1ull))] = ((u64)(uint32_t)u << 32) | (u64)(uint32_t)ev[e];
    }
}
__global__ __launch_bounds__(kT) void tracks_relabel_kernel(int k, const int32_t *feat, const int32_t *lab, int32_t *p) {
    const int x = (int)(blockIdx.x * kT + threadIdx.x);
    if (x < k) p[feat[x]] = lab[x];
}

struct Rules { int32_t min_views, max_views, conflict; };
// per component (at its label): status 0 = kept, or the code of the first rule that drops it
__global__ __launch_bounds__(kT) void tracks_decide_kernel(int F, const int32_t *touched, const int32_t *p, const int32_t *size, const int32_t *regc,
                                                           const int32_t *cflag, const int32_t *cdupreg, Rules rl, int32_t *status, int32_t *keep, u64 *cnt) {
    const int g = (int)(blockIdx.x * kT + threadIdx.x);
    const bool root = g < F && touched[g] != 0 && p[g] == g;
    int code = 0;
    if (root) {
        const int cf = cflag[g];
        if (cf && (rl.conflict == XM_TRACKS_DROP || (rl.conflict == XM_TRACKS_GLOMAP && (cf & F_FAR)))) code = XM_TRACK_CONFLICT;
        else if (size[g] < rl.min_views) code = XM_TRACK_SHORT;
        else if (size[g] > rl.max_views) code = XM_TRACK_LONG;
        else if (regc[g] - (cf ? cdupreg[g] : 0) < rl.min_views) code = XM_TRACK_FEW_REGISTERED;
        status[g] = code;
    }
    if (g < F) keep[g] = root && code == 0 ? 1 : 0;
    wave_sum_to(cnt + C_CONFLICT, root && code == XM_TRACK_CONFLICT, 1ull);
    wave_sum_to(cnt + C_SHORT, root && code == XM_TRACK_SHORT, 1ull);
    wave_sum_to(cnt + C_LONG, root && code == XM_TRACK_LONG, 1ull);
    wave_sum_to(cnt + C_FEW, root && code == XM_TRACK_FEW_REGISTERED, 1ull);
}

// label[] and the row flag of every feature
__global__ __launch_bounds__(kT) void tracks_rows_kernel(int F, const int32_t *touched, const int32_t *p, const int32_t *fimg, const uint8_t *reg,
                                                         const int32_t *status, const int32_t *tnum, int32_t *label, int32_t *rowflag) {
    const int g = (int)(blockIdx.x * kT + threadIdx.x);
    if (g >= F) return;
    int lab = XM_TRACK_UNTOUCHED, row = 0;
    if (touched[g]) {
        const int r = p[g], st = status[r];
        lab = st < 0 ? st : tnum[r];
        row = st == 0 && is_registered(reg, fimg[g]) ? 1 : 0;
    }
    label[g] = lab; rowflag[g] = row;
}
__global__ __launch_bounds__(kT) void tracks_emit_kernel(int F, const int64_t *foff, const int32_t *fimg, const int32_t *label, const int32_t *rowflag,
                                                         const int32_t *rowoff, const double *xy, int32_t *ocam, int32_t *ofeat, int32_t *otrack, double *oxy) {
    const int g = (int)(blockIdx.x * kT + threadIdx.x);
    if (g >= F || !rowflag[g]) return;
    const size_t o = (size_t)rowoff[g];
    const int img = fimg[g];
    ocam[o] = img; ofeat[o] = (int32_t)(g - foff[img]); otrack[o] = label[g];
    oxy[2 * o] = xy[2 * (size_t)g]; oxy[2 * o + 1] = xy[2 * (size_t)g + 1];
}

struct Block { int32_t changed[kBatch]; int32_t firstbad; u64 cnt[C_COUNT]; };   // what the host reads during a call

void run_device(int64_t n64, const int64_t *foff, const double *xy, const uint8_t *registered, int64_t npairs, const int32_t *pi, const int32_t *pj,
                const int64_t *moff, const int32_t *f1, const int32_t *f2, const TracksSettings &cfg, int32_t *out_cam, int32_t *out_feat,
                int32_t *out_track, double *out_xy, int32_t *label, TracksOutcome &out, std::chrono::steady_clock::time_point t_start, hipStream_t st) {
    const int n = (int)n64, F = (int)foff[n64];
    const int64_t E = moff[npairs];
    Pinned<Block> pin;
    DevBuf<int64_t> dfoff, dmoff;
    DevBuf<double> dxy, doxy;
    DevBuf<uint8_t> dreg;
    DevBuf<int32_t> dpi, dpj, df1, df2, eu, ev, touched, fimg, p, tcnt, firstbad, changed, cflag, cdupreg, size, regc, status, keep, tnum, dlabel, rowflag,
        rowoff, sums, dlarge, dwsl, sfeat, slab, docam, dofeat, dotrack;
    DevBuf<u64> cnt, ws, sedges;
    upload(dfoff, foff, (size_t)n + 1, st);
    upload(dmoff, moff, (size_t)npairs + 1, st);
    upload(dxy, xy, (size_t)F * 2, st);
    if (registered) upload(dreg, registered, (size_t)n, st);
    upload(dpi, pi, (size_t)npairs, st);
    upload(dpj, pj, (size_t)npairs, st);
    upload(df1, f1, (size_t)E, st);
    upload(df2, f2, (size_t)E, st);
    const uint8_t *reg = registered ? dreg.p : nullptr;
    eu.alloc((size_t)E, false); ev.alloc((size_t)E, false);
    fresh(touched, (size_t)F, 0, st); fresh(tcnt, (size_t)n, 0, st); fresh(cnt, C_COUNT, 0, st);
    firstbad.alloc(1, false);
    pin.h->firstbad = INT32_MAX;   // (above every match number)
    XM_HIP_CHECK(hipMemcpyAsync(firstbad.p, &pin.h->firstbad, sizeof(int32_t), hipMemcpyHostToDevice, st));
    fresh(changed, (size_t)kMaxRounds + kBatch, 0, st);
    fresh(cflag, (size_t)F, 0, st); fresh(cdupreg, (size_t)F, 0, st); fresh(size, (size_t)F, 0, st); fresh(regc, (size_t)F, 0, st);
    fresh(status, (size_t)F, 0, st);
    fimg.alloc((size_t)F, false); p.alloc((size_t)F, false); keep.alloc((size_t)F, false); tnum.alloc((size_t)F, false);
    dlabel.alloc((size_t)F, false); rowflag.alloc((size_t)F, false); rowoff.alloc((size_t)F, false);
    sums.alloc((size_t)(F / kScanTile + 1), false);
    docam.alloc((size_t)F, false); dofeat.alloc((size_t)F, false); dotrack.alloc((size_t)F, false); doxy.alloc((size_t)F * 2, false);
    wait_stream(st, cfg.watchdog_s, kStage, "the upload");
    out.seconds_index = secs_since(t_start);
    const auto t_kernels = std::chrono::steady_clock::now();
    double seconds_aside = 0.0;   // the host split, which is timed on its own

    const unsigned gf = grid_of(F);
    hipLaunchKernelGGL(tracks_expand_kernel, dim3(grid_for(E, 4096)), dim3(kT), 0, st, E, (int)npairs, dmoff.p, dpi.p, dpj.p, dfoff.p, df1.p, df2.p, eu.p, ev.p,
                       touched.p, firstbad.p);
    hipLaunchKernelGGL(tracks_feat_kernel, dim3(grid_for(F, 4096)), dim3(kT), 0, st, F, n, dfoff.p, touched.p, fimg.p, p.p, tcnt.p);
    check_launch("tracks_expand");
    std::vector<int32_t> tc((size_t)n);
    XM_HIP_CHECK(hipMemcpyAsync(tc.data(), tcnt.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(&pin.h->firstbad, firstbad.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the matches");
    if ((int64_t)pin.h->firstbad < E) {
        const int64_t e = pin.h->firstbad;
        const int64_t k = (std::upper_bound(moff, moff + npairs + 1, e) - moff) - 1;
        throw Error(XM_ERR_ARG, "xm_build_tracks: feature index out of range at match " + std::to_string(e) + " (pair " + std::to_string(k) + ")");
    }

    const TracksEdge edge = {eu.p, ev.p};
    out.rounds = label_components(E, F, edge, p.p, changed.p, pin.h->changed, kStage, cfg.watchdog_s, st);

    // the images by the size of the kernel that looks for their conflicts
    std::vector<int32_t> large, wsl;
    for (int i = 0; i < n; ++i) {
        const int64_t k = tc[(size_t)i];
        out.max_touched = std::max(out.max_touched, k);
        if (k > kTracksLdsRows) wsl.push_back(i);
        else if (k > kTracksSmallRows) large.push_back(i);
        else if (k > 0) out.images_small += 1;
    }
    if (out.max_touched > ((int64_t)1 << 30)) throw Error(XM_ERR_ARG, "xm_build_tracks: more than 2^30 matched features of one image");
    out.images_large = (int64_t)large.size(); out.images_workspace = (int64_t)wsl.size();
    if (!large.empty()) upload(dlarge, large.data(), large.size(), st);
    if (!wsl.empty()) upload(dwsl, wsl.data(), wsl.size(), st);
    ImgArgs a;
    a.foff = dfoff.p; a.touched = touched.p; a.p = p.p; a.tcnt = tcnt.p; a.xy = dxy.p; a.reg = reg; a.cflag = cflag.p; a.cdupreg = cdupreg.p;
    a.work = nullptr; a.nwork = n; a.glomap = cfg.conflict == XM_TRACKS_GLOMAP ? 1 : 0; a.thres = cfg.thres_inconsistency; a.ws = nullptr; a.ws_cap = 0;
    hipLaunchKernelGGL(tracks_image_kernel<kTracksSmallRows>, dim3((unsigned)n), dim3(kT), 0, st, a);
    check_launch("tracks_image_kernel (small)");
    if (!large.empty()) {
        a.work = dlarge.p; a.nwork = (int32_t)large.size();
        hipLaunchKernelGGL(tracks_image_kernel<kTracksLdsRows>, dim3((unsigned)a.nwork), dim3(kT), 0, st, a);
        check_launch("tracks_image_kernel (large)");
    }
    if (!wsl.empty()) {
        int64_t cap = 2 * (int64_t)kTracksLdsRows;
        while (cap < out.max_touched) cap <<= 1;
        const int groups = (int)std::min<int64_t>((int64_t)wsl.size(), kTracksWsGroups);
        ws.alloc((size_t)groups * (size_t)cap, false);
        a.work = dwsl.p; a.nwork = (int32_t)wsl.size(); a.ws = ws.p; a.ws_cap = (int32_t)cap;
        hipLaunchKernelGGL(tracks_image_ws_kernel, dim3((unsigned)groups), dim3(kT), 0, st, a);
        check_launch("tracks_image_ws_kernel");
    }
    hipLaunchKernelGGL(tracks_size_kernel, dim3(gf), dim3(kT), 0, st, F, touched.p, p.p, fimg.p, reg, size.p, regc.p);
    hipLaunchKernelGGL(tracks_stats_kernel, dim3(gf), dim3(kT), 0, st, F, touched.p, p.p, size.p, cflag.p, cnt.p);
    check_launch("tracks_size_kernel");

    if (cfg.conflict == XM_TRACKS_SPLIT) {
        XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt.p, sizeof(u64) * C_COUNT, hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the conflicts");
        if (pin.h->cnt[C_CONFLICTED] > 0) {
            const auto t_split = std::chrono::steady_clock::now();
            sedges.alloc((size_t)E, false);
            hipLaunchKernelGGL(tracks_compact_kernel, dim3(grid_for(E, 4096)), dim3(kT), 0, st, E, eu.p, ev.p, p.p, cflag.p, cnt.p, sedges.p);
            check_launch("tracks_compact_kernel");
            XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt.p, sizeof(u64) * C_COUNT, hipMemcpyDeviceToHost, st));
            wait_stream(st, cfg.watchdog_s, kStage, "the conflicted edges");
            const u64 ns = pin.h->cnt[C_NSPLIT];
            if (ns > (u64)E) throw Error(XM_ERR_HIP, "tracks: more conflicted edges than matches");
            std::vector<uint64_t> edges((size_t)ns);
            static_assert(sizeof(uint64_t) == sizeof(u64), "the edge words are copied as they are");
            if (ns) XM_HIP_CHECK(hipMemcpyAsync(edges.data(), sedges.p, (size_t)ns * sizeof(u64), hipMemcpyDeviceToHost, st));
            wait_stream(st, cfg.watchdog_s, kStage, "the conflicted edges");
            TrackSplit sp;
            tracks_split(n64, foff, edges, sp);
            out.edges_split = sp.distinct; out.unions_refused = sp.refused;
            upload(sfeat, sp.feat.data(), sp.feat.size(), st);
            upload(slab, sp.label.data(), sp.label.size(), st);
            if (!sp.feat.empty())
                hipLaunchKernelGGL(tracks_relabel_kernel, dim3(grid_of((int64_t)sp.feat.size())), dim3(kT), 0, st, (int)sp.feat.size(), sfeat.p, slab.p, p.p);
            // every track is free of conflicts now: the flags go, and the sizes are counted again under the new labels
            XM_HIP_CHECK(hipMemsetAsync(cflag.p, 0, (size_t)F * sizeof(int32_t), st));
            XM_HIP_CHECK(hipMemsetAsync(cdupreg.p, 0, (size_t)F * sizeof(int32_t), st));
            XM_HIP_CHECK(hipMemsetAsync(size.p, 0, (size_t)F * sizeof(int32_t), st));
            XM_HIP_CHECK(hipMemsetAsync(regc.p, 0, (size_t)F * sizeof(int32_t), st));
            hipLaunchKernelGGL(tracks_size_kernel, dim3(gf), dim3(kT), 0, st, F, touched.p, p.p, fimg.p, reg, size.p, regc.p);
            check_launch("tracks_size_kernel (after the split)");
            wait_stream(st, cfg.watchdog_s, kStage, "the split labels");   // (the splitter's arrays are read by the copies above)
            seconds_aside = secs_since(t_split);
            out.seconds_split = seconds_aside;
        }
    }

    const Rules rl = {cfg.min_views, cfg.max_views, cfg.conflict};
    hipLaunchKernelGGL(tracks_decide_kernel, dim3(gf), dim3(kT), 0, st, F, touched.p, p.p, size.p, regc.p, cflag.p, cdupreg.p, rl, status.p, keep.p, cnt.p);
    check_launch("tracks_decide_kernel");
    auto number_and_emit = [&]() {
        exclusive_scan(F, keep.p, tnum.p, sums, cnt.p + C_NTRACKS, st);
        hipLaunchKernelGGL(tracks_rows_kernel, dim3(gf), dim3(kT), 0, st, F, touched.p, p.p, fimg.p, reg, status.p, tnum.p, dlabel.p, rowflag.p);
        exclusive_scan(F, rowflag.p, rowoff.p, sums, cnt.p + C_NOUT, st);
        hipLaunchKernelGGL(tracks_emit_kernel, dim3(gf), dim3(kT), 0, st, F, dfoff.p, fimg.p, dlabel.p, rowflag.p, rowoff.p, dxy.p, docam.p, dofeat.p,
                           dotrack.p, doxy.p);
        check_launch("tracks_emit_kernel");
        XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt.p, sizeof(u64) * C_COUNT, hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the rows");
    };
    number_and_emit();
    if ((int64_t)pin.h->cnt[C_NTRACKS] - 1 > cfg.max_tracks) {   // (max_tracks + 1 could overflow)
        // rule 6, the rare path: the max_tracks + 1 longest stay, ties to the larger label; chosen on the host from the components' sizes
        std::vector<int32_t> hsize((size_t)F), hkeep((size_t)F), hstatus((size_t)F);
        XM_HIP_CHECK(hipMemcpyAsync(hsize.data(), size.p, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(hkeep.data(), keep.p, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(hstatus.data(), status.p, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the sizes");
        std::vector<uint64_t> order;   // (size << 32 | label): the larger word is the track that stays
        for (int g = 0; g < F; ++g)
            if (hkeep[(size_t)g]) order.push_back(((uint64_t)(uint32_t)hsize[(size_t)g] << 32) | (uint64_t)(uint32_t)g);
        const size_t stay = (size_t)(cfg.max_tracks + 1);
        std::nth_element(order.begin(), order.begin() + (std::ptrdiff_t)(order.size() - stay), order.end());
        for (size_t x = 0; x + stay < order.size(); ++x) {
            const size_t g = (size_t)(order[x] & 0xffffffffull);
            hkeep[g] = 0; hstatus[g] = XM_TRACK_BEYOND_MAX;
            out.tracks_beyond_max += 1;
        }
        XM_HIP_CHECK(hipMemcpyAsync(keep.p, hkeep.data(), (size_t)F * sizeof(int32_t), hipMemcpyHostToDevice, st));
        XM_HIP_CHECK(hipMemcpyAsync(status.p, hstatus.data(), (size_t)F * sizeof(int32_t), hipMemcpyHostToDevice, st));
        number_and_emit();
    }
    const u64 *c = pin.h->cnt;
    out.seconds_kernels = secs_since(t_kernels) - seconds_aside;
    const auto t_down = std::chrono::steady_clock::now();
    if (c[C_NOUT] > (u64)F || c[C_NTRACKS] > (u64)F) throw Error(XM_ERR_HIP, "tracks: more rows than features");
    const size_t no = (size_t)c[C_NOUT];
    if (no) {
        XM_HIP_CHECK(hipMemcpyAsync(out_cam, docam.p, no * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(out_feat, dofeat.p, no * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(out_track, dotrack.p, no * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(out_xy, doxy.p, no * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (label) XM_HIP_CHECK(hipMemcpyAsync(label, dlabel.p, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the download");
    out.seconds_download = secs_since(t_down);
    out.nout = (int64_t)no; out.ntracks = (int64_t)c[C_NTRACKS];
    out.features_touched = (int64_t)c[C_TOUCHED]; out.components = (int64_t)c[C_COMPONENTS];
    out.components_conflicted = (int64_t)c[C_CONFLICTED]; out.rows_conflicted = (int64_t)c[C_ROWS_CONFLICTED];
    out.tracks_short = (int64_t)c[C_SHORT]; out.tracks_long = (int64_t)c[C_LONG]; out.tracks_conflict = (int64_t)c[C_CONFLICT];
    out.tracks_few_registered = (int64_t)c[C_FEW];
}

}  // namespace

void build_tracks_host(int64_t n, const int64_t *foff, const double *xy, const uint8_t *registered, int64_t npairs, const int32_t *pi, const int32_t *pj,
                       const int64_t *moff, const int32_t *f1, const int32_t *f2, const TracksSettings &cfg, int32_t *out_cam, int32_t *out_feat,
                       int32_t *out_track, double *out_xy, int32_t *label, TracksOutcome &out) {
    const auto t_start = std::chrono::steady_clock::now();
    out = TracksOutcome();
    const int64_t F = n > 0 ? foff[n] : 0, E = npairs > 0 ? moff[npairs] : 0;
    out.matches = E;
    if (n == 0 || E == 0) {   // nothing to launch
        if (label) for (int64_t g = 0; g < F; ++g) label[g] = XM_TRACK_UNTOUCHED;
        return;
    }
    if (F == 0) throw Error(XM_ERR_ARG, "xm_build_tracks: feature index out of range at match 0 (there is no feature)");
    hipStream_t st = nullptr;   // the default stream, as xm_pair_filter
    try {
        run_device(n, foff, xy, registered, npairs, pi, pj, moff, f1, f2, cfg, out_cam, out_feat, out_track, out_xy, label, out, t_start, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the device buffers are freed next: nothing may still be reading them
        throw;
    }
}

}  // namespace xm
