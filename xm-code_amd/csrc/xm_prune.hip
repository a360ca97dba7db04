// xm_prune.hip — pruning of weakly connected images on the device (xm_prune.h has the design; definition in include/xm_amd.h at
// xm_prune_weakly_connected).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/xm_amd.h"
#include "xm_prune.h"
#include "xm_stage.h"

namespace xm {
namespace {

constexpr int kT = kPruneThreads;
constexpr int kBins = kPruneTile / kT;   // bins of the tile that one thread looks at: [kBins t, kBins t + kBins)
static_assert(kT == kStageThreads, "the helpers of xm_stage.h are written for this workgroup size");
static_assert(kPruneTile % kT == 0 && kT % kPruneGroup == 0 && kPruneGroup <= 64, "tile, workgroup and lane groups must divide evenly");
constexpr const char *kStage = "image pruning";
constexpr int kSelLow = 1 << kPruneSelBits;

// slots of the device counter block
enum { C_PAIRS = 0, C_EDGES, C_WMAX, C_SCAN_E, C_BEST /* max of (size << 32 | ~root) */, C_STRONG, C_WEAK, C_COUNT };
// slots of the order statistics (int64) and of the thresholds (double)
enum { S_BUCKET = 0, S_KREM, S_MED, S_MAD, S_SPARE, S_COUNT };
enum { D_THR = 0, D_THR75, D_COUNT };

struct PruneArgs { int32_t min_cov, min_obs; };

__device__ inline bool obs_used(const PruneLists &L, int64_t e) { return !L.cam_w || L.cam_w[L.wpos ? L.wpos[e] : e] > 0.0; }

// per landmark slot: its used observations; whole wavefronts
__global__ __launch_bounds__(kT) void prune_lmused_kernel(PruneLists L, int32_t *lused) {
    for (int64_t base = (int64_t)blockIdx.x * kT; base < L.nobs; base += (int64_t)gridDim.x * kT) {
        const int64_t e = base + threadIdx.x;
        const bool in = e < L.nobs;
        wave_add_one(lused, in ? L.obs_lm[e] : 0, in && obs_used(L, e));
    }
}
// per camera: its used observations in landmarks with more than two (reconstruction_pruning.cc:14, :17)
__global__ __launch_bounds__(kT) void prune_obscount_kernel(PruneLists L, const int32_t *lused, int32_t *obs_count) {
    for (int64_t base = (int64_t)blockIdx.x * kT; base < L.nobs; base += (int64_t)gridDim.x * kT) {
        const int64_t e = base + threadIdx.x;
        const bool in = e < L.nobs;
        wave_add_one(obs_count, in ? L.obs_cam[e] : 0, in && obs_used(L, e) && lused[L.obs_lm[e]] > 2);
    }
}

// the list of landmark slot s: entry q at base + stride q, q < len
__device__ inline void lm_list(const PruneLists &L, int s, int64_t &base, int64_t &stride, int64_t &len) {
    if (s < L.nheavy) {
        base = L.lm_ptr[s]; len = L.lm_ptr[s + 1] - base; stride = 1;
    } else {
        const int64_t tl = s - L.nheavy;
        base = L.gbase[tl >> 6] + (tl & 63); len = L.deg[s]; stride = 64;
    }
}
// the landmark at position k of a camera's list if it takes part, or -1
__device__ inline int live_slot(const PruneLists &L, const int32_t *lused, int64_t k) {
    if (L.cam_w && !(L.cam_w[k] > 0.0)) return -1;
    const int s = L.cam_lm[k];
    return lused[s] > 2 ? s : -1;
}
__device__ inline void add_list(const PruneLists &L, int64_t base, int64_t stride, int64_t len, int first, int step, int64_t t0, int32_t *hist) {
    for (int64_t q = first; q < len; q += step) {
        const int64_t pos = base + stride * q;
        if (L.lm_w && !(L.lm_w[pos] > 0.0)) continue;
        const int64_t b = (int64_t)L.lm_cam[pos] - t0;
        if (b >= 0 && b < kPruneTile) atomicAdd(hist + b, 1);
    }
}

// WRITE = false: pairs and edges of camera blockIdx.x with a camera j > i, the largest edge weight.  WRITE = true: the edges, from off[i] on.
template <bool WRITE>
__global__ __launch_bounds__(kT) void prune_covis_kernel(PruneLists L, PruneArgs a, const int32_t *__restrict__ lused, const int32_t *__restrict__ obs_count,
                                                         int32_t *__restrict__ n_edge, const int32_t *__restrict__ off, int32_t *__restrict__ ei,
                                                         int32_t *__restrict__ ej, int32_t *__restrict__ ew, u64 *cnt) {
    __shared__ int32_t hist[kPruneTile];
    __shared__ int scan[kT];
    __shared__ int heavy[kT];
    const int tid = (int)threadIdx.x;
    const int64_t i = blockIdx.x, n = L.n, c0 = L.cam_ptr[i], c1 = L.cam_ptr[i + 1];
    const bool i_ok = obs_count[i] >= a.min_obs;
    int ncov = 0, nedge = 0, wmax = 0;
    int64_t wbase = WRITE ? (int64_t)off[i] : 0;
    for (int64_t t0 = (i + 1) / kPruneTile * kPruneTile; t0 < n; t0 += kPruneTile) {
        for (int b = tid; b < kPruneTile; b += kT) hist[b] = 0;
        __syncthreads();
        // landmarks of up to kPruneHeavy entries: a group of lanes each
        for (int64_t k = c0 + tid / kPruneGroup; k < c1; k += kT / kPruneGroup) {
            const int s = live_slot(L, lused, k);
            if (s < 0) continue;
            int64_t base, stride, len;
            lm_list(L, s, base, stride, len);
            if (len <= kPruneHeavy) add_list(L, base, stride, len, tid % kPruneGroup, kPruneGroup, t0, hist);
        }
        // the longer ones: found kT positions of the camera's list at a time, walked by the whole workgroup in the list's order
        for (int64_t kb = c0; kb < c1; kb += kT) {
            int mine = -1;
            if (kb + tid < c1) {
                const int s = live_slot(L, lused, kb + tid);
                if (s >= 0) {
                    int64_t base, stride, len;
                    lm_list(L, s, base, stride, len);
                    if (len > kPruneHeavy) mine = s;
                }
            }
            heavy[tid] = mine;
            __syncthreads();
            const int cntk = (int)(c1 - kb < kT ? c1 - kb : kT);
            for (int x = 0; x < cntk; ++x) {
                const int s = heavy[x];
                if (s < 0) continue;
                int64_t base, stride, len;
                lm_list(L, s, base, stride, len);
                add_list(L, base, stride, len, tid, kT, t0, hist);
            }
            __syncthreads();   // heavy[] is written again next
        }
        __syncthreads();
        int32_t v[kBins];
        int mine = 0;
#pragma unroll
        for (int r = 0; r < kBins; ++r) {
            const int64_t j = t0 + kBins * tid + r;
            const int32_t c = hist[kBins * tid + r];
            const bool pair = j > i && j < n && c >= a.min_cov;
            const bool edge = pair && i_ok && obs_count[j] >= a.min_obs;
            v[r] = edge ? c : -1;
            ncov += pair; mine += edge;
            if (edge && c > wmax) wmax = c;
        }
        nedge += mine;
        if (WRITE) {
            int total;
            int64_t at = wbase + block_scan_excl(mine, scan, &total);   // ends with a barrier
            wbase += total;
#pragma unroll
            for (int r = 0; r < kBins; ++r)
                if (v[r] >= 0) { ei[at] = (int32_t)i; ej[at] = (int32_t)(t0 + kBins * tid + r); ew[at] = v[r]; ++at; }
        } else {
            __syncthreads();   // the bins are read: the next tile may clear them
        }
    }
    if (!WRITE) {
        int total, total_cov;
        block_scan_excl(nedge, scan, &total);
        block_scan_excl(ncov, scan, &total_cov);
        const u64 wm = wave_max((u64)(uint32_t)wmax);
        if (lane_id() == 0 && wm) atomicMax(cnt + C_WMAX, wm);
        if (tid == 0) {
            n_edge[i] = total;
            if (total_cov) atomicAdd(cnt + C_PAIRS, (u64)total_cov);
            if (total) atomicAdd(cnt + C_EDGES, (u64)total);
        }
    }
}

// ---- the element k of the sorted values, exactly, in two levels: value >> kPruneSelBits, then the low bits inside the bucket found
__device__ inline int64_t sel_value(const int32_t *w, int64_t e, const int64_t *center) {
    const int64_t v = w[e];
    if (!center) return v;
    const int64_t d = v - *center;
    return d < 0 ? -d : d;
}
__global__ __launch_bounds__(kT) void prune_sel_hist_kernel(int64_t ne, const int32_t *w, const int64_t *center, const int64_t *bucket, int32_t *hist) {
    for (int64_t base = (int64_t)blockIdx.x * kT; base < ne; base += (int64_t)gridDim.x * kT) {
        const int64_t e = base + threadIdx.x;
        const bool in = e < ne;
        const int64_t v = in ? sel_value(w, e, center) : 0;
        const bool on = in && (!bucket || (v >> kPruneSelBits) == *bucket);
        wave_add_one(hist, (int)(bucket ? (v & (kSelLow - 1)) : (v >> kPruneSelBits)), on);
    }
}
// one workgroup: the bin that holds element k (k_dev when given) of the histogram; out = (hi << kPruneSelBits) + bin, krem = k - entries before the bin
__global__ __launch_bounds__(kT) void prune_sel_find_kernel(int nbins, const int32_t *hist, int64_t k_host, const int64_t *k_dev, const int64_t *hi,
                                                            int64_t *out, int64_t *krem) {
    __shared__ int scan[kT];
    const int chunk = (nbins + kT - 1) / kT, b0 = (int)threadIdx.x * chunk, b1 = b0 + chunk < nbins ? b0 + chunk : nbins;
    int sum = 0;
    for (int b = b0; b < b1; ++b) sum += hist[b];
    int total;
    const int64_t before = block_scan_excl(sum, scan, &total);
    const int64_t k = k_dev ? *k_dev : k_host;
    if (k >= before && k < before + sum) {
        int64_t c = before;
        for (int b = b0; b < b1; ++b) {
            if (k < c + hist[b]) {
                *out = (hi ? (*hi << kPruneSelBits) : 0) + b;
                *krem = k - c;
                break;
            }
            c += hist[b];
        }
    }
}
// threshold = max(median - mad, min_threshold) and 0.75 threshold, each computed once (reconstruction_pruning.cc:80, view_graph_manipulation.cc:115)
__global__ void prune_threshold_kernel(const int64_t *sel, double min_threshold, double *thr) {
    const double d = (double)(sel[S_MED] - sel[S_MAD]);
    const double t = d < min_threshold ? min_threshold : d;
    thr[D_THR] = t;
    thr[D_THR75] = 0.75 * t;
}

// ---- around the three labellings
struct PruneEdge {
    const int32_t *i, *j;
    const uint8_t *on;   // null: every edge
    __device__ bool operator()(int64_t e, int &u, int &v) const {
        if (on && !on[e]) return false;
        u = i[e]; v = j[e];
        return true;
    }
};
__global__ __launch_bounds__(kT) void prune_touch_kernel(int64_t ne, const int32_t *ei, const int32_t *ej, const uint8_t *on, int32_t *has) {
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (e >= ne || (on && !on[e])) return;
    has[ei[e]] = 1; has[ej[e]] = 1;
}
__global__ __launch_bounds__(kT) void prune_sizes_kernel(int n, const int32_t *has, const int32_t *p, int32_t *size) {
    const int v = (int)(blockIdx.x * kT + threadIdx.x);
    const bool in = v < n;
    wave_add_one(size, in ? p[v] : 0, in && has[v] != 0);
}
// the largest component; equal sizes: the one with the smallest image (the key holds ~root)
__global__ __launch_bounds__(kT) void prune_best_kernel(int n, const int32_t *has, const int32_t *p, const int32_t *size, u64 *cnt) {
    const int v = (int)(blockIdx.x * kT + threadIdx.x);
    const bool root = v < n && has[v] != 0 && p[v] == v;
    const u64 key = wave_max(root ? (((u64)(uint32_t)size[v] << 32) | (u64)(0xFFFFFFFFu - (uint32_t)v)) : 0ull);
    if (lane_id() == 0 && key) atomicMax(cnt + C_BEST, key);
}
__device__ inline int best_root(const u64 *cnt) { return (int)(0xFFFFFFFFu - (uint32_t)(cnt[C_BEST] & 0xFFFFFFFFull)); }
// valid: the edge lies in the largest component (view_graph.cc:36-40); strong: valid and weight > threshold (view_graph_manipulation.cc:85)
__global__ __launch_bounds__(kT) void prune_valid_kernel(int64_t ne, const int32_t *ei, const int32_t *ew, const int32_t *p, const u64 *cnt,
                                                         const double *thr, uint8_t *valid, uint8_t *strong) {
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (e >= ne) return;
    const bool ok = p[ei[e]] == best_root(cnt);
    valid[e] = ok ? 1 : 0;
    strong[e] = ok && (double)ew[e] > thr[D_THR] ? 1 : 0;
}
__global__ __launch_bounds__(kT) void prune_strong_count_kernel(int n, const int32_t *p, const int32_t *q, u64 *cnt) {
    const int v = (int)(blockIdx.x * kT + threadIdx.x);
    wave_count(cnt + C_STRONG, v < n && p[v] == best_root(cnt) && q[v] == v);
}
// the edges a merge round looks at: valid, not below 0.75 threshold, between two clusters (view_graph_manipulation.cc:108-126)
__global__ __launch_bounds__(kT) void prune_weak_flag_kernel(int64_t ne, const int32_t *ei, const int32_t *ej, const int32_t *ew, const uint8_t *valid,
                                                             const int32_t *q, const double *thr, int32_t *flag) {
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (e >= ne) return;
    flag[e] = valid[e] && !((double)ew[e] < thr[D_THR75]) && q[ei[e]] != q[ej[e]] ? 1 : 0;
}
__global__ __launch_bounds__(kT) void prune_weak_write_kernel(int64_t ne, const int32_t *ei, const int32_t *ej, const int32_t *flag, const int32_t *pos,
                                                              const int32_t *q, int32_t *wa, int32_t *wb) {
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (e >= ne || !flag[e]) return;
    wa[pos[e]] = q[ei[e]]; wb[pos[e]] = q[ej[e]];
}
__global__ __launch_bounds__(kT) void prune_remap_kernel(int n, const int32_t *cmap, int32_t *q) {
    const int v = (int)(blockIdx.x * kT + threadIdx.x);
    if (v < n) q[v] = cmap[q[v]];
}
// what is left for the final marking: valid edges inside one cluster (view_graph_manipulation.cc:151-160)
__global__ __launch_bounds__(kT) void prune_final_kernel(int64_t ne, const int32_t *ei, const int32_t *ej, const uint8_t *valid, const int32_t *q, uint8_t *fin) {
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (e < ne) fin[e] = valid[e] && q[ei[e]] == q[ej[e]] ? 1 : 0;
}

struct Block { int32_t changed[kBatch]; u64 cnt[C_COUNT]; int64_t sel[S_COUNT]; double thr[D_COUNT]; };   // what the host reads during a call

// element ne / 2 of the sorted values (of |value - *center| with a center) -> sel[dst]
void select_middle(int64_t ne, const int32_t *w, const int64_t *center, int64_t wmax, int64_t *sel, int dst, DevBuf<int32_t> &hist, hipStream_t st) {
    const int nb1 = (int)(wmax >> kPruneSelBits) + 1;
    const unsigned g = grid_for(ne, 4096);
    XM_HIP_CHECK(hipMemsetAsync(hist.p, 0, (size_t)(nb1 + kSelLow) * sizeof(int32_t), st));
    hipLaunchKernelGGL(prune_sel_hist_kernel, dim3(g), dim3(kT), 0, st, ne, w, center, (const int64_t *)nullptr, hist.p);
    hipLaunchKernelGGL(prune_sel_find_kernel, dim3(1), dim3(kT), 0, st, nb1, (const int32_t *)hist.p, ne / 2, (const int64_t *)nullptr,
                       (const int64_t *)nullptr, sel + S_BUCKET, sel + S_KREM);
    hipLaunchKernelGGL(prune_sel_hist_kernel, dim3(g), dim3(kT), 0, st, ne, w, center, (const int64_t *)(sel + S_BUCKET), hist.p + nb1);
    hipLaunchKernelGGL(prune_sel_find_kernel, dim3(1), dim3(kT), 0, st, kSelLow, (const int32_t *)(hist.p + nb1), (int64_t)0, (const int64_t *)(sel + S_KREM),
                       (const int64_t *)(sel + S_BUCKET), sel + dst, sel + S_SPARE);
    check_launch("prune_select");
}

// Merge rounds on the cluster labels (view_graph_manipulation.cc:95-149): a, b are the strong clusters of the two ends of every edge the rounds
// look at.  Every pair of clusters that at least two such edges join is united, all pairs of a round at once; the smaller label stays, so a
// cluster keeps the smallest image as its label.  Returns the number of bodies run; cmap[c] = merged cluster of c, *united = any union.
int merge_rounds(int n, const std::vector<int32_t> &a, const std::vector<int32_t> &b, std::vector<int32_t> &cmap, bool *united) {
    cmap.resize((size_t)n);
    for (int v = 0; v < n; ++v) cmap[(size_t)v] = v;
    auto find = [&](int32_t x) {
        while (cmap[(size_t)x] != x) { cmap[(size_t)x] = cmap[(size_t)cmap[(size_t)x]]; x = cmap[(size_t)x]; }
        return x;
    };
    *united = false;
    int rounds = 0;
    bool status = true;
    while (status) {
        status = false;
        if (rounds + 1 > 10) break;   // `iteration > 10` (:101)
        ++rounds;
        std::unordered_map<uint64_t, int> num_pairs;
        for (size_t e = 0; e < a.size(); ++e) {
            const int32_t r1 = find(a[e]), r2 = find(b[e]);
            if (r1 == r2) continue;
            ++num_pairs[((uint64_t)(uint32_t)std::min(r1, r2) << 32) | (uint32_t)std::max(r1, r2)];
        }
        std::vector<uint64_t> join;
        for (const auto &kv : num_pairs)
            if (kv.second >= 2) join.push_back(kv.first);
        for (uint64_t key : join) {   // the components of the cluster graph: the order of the unions cannot change them, nor the label (the minimum)
            const int32_t r1 = find((int32_t)(key >> 32)), r2 = find((int32_t)(key & 0xFFFFFFFFull));
            if (r1 != r2) cmap[(size_t)std::max(r1, r2)] = std::min(r1, r2);
            status = true;
        }
        if (status) *united = true;
    }
    for (int v = 0; v < n; ++v) cmap[(size_t)v] = find(v);
    return rounds;
}

}  // namespace

void prune_device(const PruneLists &L, const PruneSettings &cfg, int32_t *cluster_id, int32_t *obs_count, const PrunePairs *pairs, PruneOutcome &out,
                  hipStream_t st) {
    if (L.n < 0 || L.m < 0 || L.nobs < 0) throw Error(XM_ERR_ARG, "image pruning: negative size");
    if (L.n >= ((int64_t)1 << 31) || L.m >= ((int64_t)1 << 31) || L.nobs >= ((int64_t)1 << 31))
        throw Error(XM_ERR_ARG, "image pruning: cameras, landmarks and observations must each stay below 2^31");
    const int n = (int)L.n, m = (int)L.m;
    out = PruneOutcome();
    for (int v = 0; v < n; ++v) cluster_id[v] = -1;
    if (n == 0) return;
    const auto t_kernels = std::chrono::steady_clock::now();
    Pinned<Block> pin;
    DevBuf<u64> cnt;
    DevBuf<int64_t> sel;
    DevBuf<double> thr;
    DevBuf<int32_t> lused, dcount, n_edge, off, sums, ei, ej, ew, hist, changed, p, q, r, has, size, flag, pos, wa, wb, dcmap;
    DevBuf<uint8_t> valid, on;
    fresh(cnt, C_COUNT, 0, st); fresh(sel, S_COUNT, 0, st); fresh(thr, D_COUNT, 0, st);
    fresh(lused, (size_t)m, 0, st); fresh(dcount, (size_t)n, 0, st);
    n_edge.alloc((size_t)n, false); off.alloc((size_t)n, false);
    const PruneArgs a = {cfg.min_covisibility, cfg.min_num_observations};
    const unsigned go = grid_for(L.nobs, 4096), gc = grid_of(n);
    std::vector<int32_t> hlabel((size_t)n), hhas((size_t)n);
    try {
        if (L.nobs > 0) {
            hipLaunchKernelGGL(prune_lmused_kernel, dim3(go), dim3(kT), 0, st, L, lused.p);
            hipLaunchKernelGGL(prune_obscount_kernel, dim3(go), dim3(kT), 0, st, L, (const int32_t *)lused.p, dcount.p);
        }
        hipLaunchKernelGGL(prune_covis_kernel<false>, dim3((unsigned)n), dim3(kT), 0, st, L, a, (const int32_t *)lused.p, (const int32_t *)dcount.p, n_edge.p,
                           (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, cnt.p);
        check_launch("prune_covis_kernel (count)");
        XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt.p, C_COUNT * sizeof(u64), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(obs_count, dcount.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the covisibility counts");
        out.pairs_covisible = (int64_t)pin.h->cnt[C_PAIRS];
        const int64_t E = (int64_t)pin.h->cnt[C_EDGES], wmax = (int64_t)pin.h->cnt[C_WMAX];
        out.n_edges = E;
        if (E >= ((int64_t)1 << 31)) throw Error(XM_ERR_ARG, "image pruning: the visibility graph has 2^31 edges or more");
        if (E == 0) {   // the reference reads pair_count[0] of an empty vector here: no cluster, threshold 0
            out.seconds_kernels = secs_since(t_kernels);
            return;
        }
        sums.alloc((size_t)(std::max<int64_t>(n, E) / kScanTile + 1), false);
        exclusive_scan(n, n_edge.p, off.p, sums, cnt.p + C_SCAN_E, st);
        ei.alloc((size_t)E, false); ej.alloc((size_t)E, false); ew.alloc((size_t)E, false);
        hipLaunchKernelGGL(prune_covis_kernel<true>, dim3((unsigned)n), dim3(kT), 0, st, L, a, (const int32_t *)lused.p, (const int32_t *)dcount.p,
                           (int32_t *)nullptr, (const int32_t *)off.p, ei.p, ej.p, ew.p, cnt.p);
        check_launch("prune_covis_kernel (write)");
        // median, MAD, threshold
        hist.alloc((size_t)((wmax >> kPruneSelBits) + 1 + kSelLow), false);
        select_middle(E, ew.p, nullptr, wmax, sel.p, S_MED, hist, st);
        select_middle(E, ew.p, sel.p + S_MED, wmax, sel.p, S_MAD, hist, st);
        hipLaunchKernelGGL(prune_threshold_kernel, dim3(1), dim3(1), 0, st, (const int64_t *)sel.p, cfg.min_threshold, thr.p);
        check_launch("prune_threshold_kernel");
        // the largest component
        const unsigned ge = grid_of(E);
        fresh(changed, (size_t)3 * (kMaxRounds + kBatch), 0, st);
        p.alloc((size_t)n, false); q.alloc((size_t)n, false); r.alloc((size_t)n, false);
        fresh(has, (size_t)n, 0, st); fresh(size, (size_t)n, 0, st);
        valid.alloc((size_t)E, false); on.alloc((size_t)E, false);
        identity_labels(n, p.p, st);
        label_components(E, n, PruneEdge{ei.p, ej.p, nullptr}, p.p, changed.p, pin.h->changed, kStage, cfg.watchdog_s, st);
        hipLaunchKernelGGL(prune_touch_kernel, dim3(ge), dim3(kT), 0, st, E, (const int32_t *)ei.p, (const int32_t *)ej.p, (const uint8_t *)nullptr, has.p);
        hipLaunchKernelGGL(prune_sizes_kernel, dim3(gc), dim3(kT), 0, st, n, (const int32_t *)has.p, (const int32_t *)p.p, size.p);
        hipLaunchKernelGGL(prune_best_kernel, dim3(gc), dim3(kT), 0, st, n, (const int32_t *)has.p, (const int32_t *)p.p, (const int32_t *)size.p, cnt.p);
        hipLaunchKernelGGL(prune_valid_kernel, dim3(ge), dim3(kT), 0, st, E, (const int32_t *)ei.p, (const int32_t *)ew.p, (const int32_t *)p.p,
                           (const u64 *)cnt.p, (const double *)thr.p, valid.p, on.p);
        check_launch("prune_valid_kernel");
        // strong clusters
        identity_labels(n, q.p, st);
        label_components(E, n, PruneEdge{ei.p, ej.p, on.p}, q.p, changed.p + (kMaxRounds + kBatch), pin.h->changed, kStage, cfg.watchdog_s, st);
        hipLaunchKernelGGL(prune_strong_count_kernel, dim3(gc), dim3(kT), 0, st, n, (const int32_t *)p.p, (const int32_t *)q.p, cnt.p);
        // the edges of the merge rounds, in (i, j) order
        flag.alloc((size_t)E, false); pos.alloc((size_t)E, false);
        hipLaunchKernelGGL(prune_weak_flag_kernel, dim3(ge), dim3(kT), 0, st, E, (const int32_t *)ei.p, (const int32_t *)ej.p, (const int32_t *)ew.p,
                           (const uint8_t *)valid.p, (const int32_t *)q.p, (const double *)thr.p, flag.p);
        check_launch("prune_weak_flag_kernel");
        exclusive_scan((int)E, flag.p, pos.p, sums, cnt.p + C_WEAK, st);
        XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt.p, C_COUNT * sizeof(u64), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(pin.h->sel, sel.p, S_COUNT * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(pin.h->thr, thr.p, D_COUNT * sizeof(double), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the strong clusters");
        if ((int64_t)pin.h->cnt[C_SCAN_E] != E) throw Error(XM_ERR_HIP, "image pruning: the prefix sum disagrees with the counted edges");
        out.median = (double)pin.h->sel[S_MED]; out.mad = (double)pin.h->sel[S_MAD]; out.threshold = pin.h->thr[D_THR];
        out.component_images = (int64_t)(pin.h->cnt[C_BEST] >> 32);
        out.strong_clusters = (int64_t)pin.h->cnt[C_STRONG];
        const int64_t nweak = (int64_t)pin.h->cnt[C_WEAK];
        out.weak_edges = nweak;
        out.rounds = 1;   // a round without such an edge unites nothing: one body
        if (nweak > 0) {
            wa.alloc((size_t)nweak, false); wb.alloc((size_t)nweak, false);
            hipLaunchKernelGGL(prune_weak_write_kernel, dim3(ge), dim3(kT), 0, st, E, (const int32_t *)ei.p, (const int32_t *)ej.p, (const int32_t *)flag.p,
                               (const int32_t *)pos.p, (const int32_t *)q.p, wa.p, wb.p);
            check_launch("prune_weak_write_kernel");
            std::vector<int32_t> ha((size_t)nweak), hb((size_t)nweak), cmap;
            XM_HIP_CHECK(hipMemcpyAsync(ha.data(), wa.p, (size_t)nweak * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(hb.data(), wb.p, (size_t)nweak * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            wait_stream(st, cfg.watchdog_s, kStage, "the edges of the merge rounds");
            bool united = false;
            out.rounds = merge_rounds(n, ha, hb, cmap, &united);
            if (united) {
                upload(dcmap, cmap.data(), (size_t)n, st);
                hipLaunchKernelGGL(prune_remap_kernel, dim3(gc), dim3(kT), 0, st, n, (const int32_t *)dcmap.p, q.p);
                check_launch("prune_remap_kernel");
                wait_stream(st, cfg.watchdog_s, kStage, "the merged clusters");   // cmap is a local of this block
            }
        }
        // final marking
        hipLaunchKernelGGL(prune_final_kernel, dim3(ge), dim3(kT), 0, st, E, (const int32_t *)ei.p, (const int32_t *)ej.p, (const uint8_t *)valid.p,
                           (const int32_t *)q.p, on.p);
        XM_HIP_CHECK(hipMemsetAsync(has.p, 0, (size_t)n * sizeof(int32_t), st));
        identity_labels(n, r.p, st);
        check_launch("prune_final_kernel");
        label_components(E, n, PruneEdge{ei.p, ej.p, on.p}, r.p, changed.p + 2 * (kMaxRounds + kBatch), pin.h->changed, kStage, cfg.watchdog_s, st);
        hipLaunchKernelGGL(prune_touch_kernel, dim3(ge), dim3(kT), 0, st, E, (const int32_t *)ei.p, (const int32_t *)ej.p, (const uint8_t *)on.p, has.p);
        check_launch("prune_touch_kernel");
        XM_HIP_CHECK(hipMemcpyAsync(hlabel.data(), r.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipMemcpyAsync(hhas.data(), has.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        wait_stream(st, cfg.watchdog_s, kStage, "the final components");
        out.seconds_kernels = secs_since(t_kernels);
        const auto t_down = std::chrono::steady_clock::now();
        if (pairs && pairs->capacity >= E) {
            XM_HIP_CHECK(hipMemcpyAsync(pairs->i, ei.p, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(pairs->j, ej.p, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            XM_HIP_CHECK(hipMemcpyAsync(pairs->count, ew.p, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            wait_stream(st, cfg.watchdog_s, kStage, "the download");
        }
        out.seconds_download = secs_since(t_down);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the buffers above are freed next: nothing may still be reading them
        throw;
    }
    // components by size, descending; equal sizes: the smallest image first (view_graph.cc:72-87); ids while size >= min_num_images
    std::vector<int32_t> csize((size_t)n, 0);
    for (int v = 0; v < n; ++v)
        if (hhas[(size_t)v]) ++csize[(size_t)hlabel[(size_t)v]];
    std::vector<int32_t> roots;
    for (int v = 0; v < n; ++v)
        if (csize[(size_t)v] > 0) roots.push_back(v);
    std::stable_sort(roots.begin(), roots.end(), [&](int32_t x, int32_t y) { return csize[(size_t)x] > csize[(size_t)y]; });
    std::vector<int32_t> id_of((size_t)n, -1);
    for (size_t c = 0; c < roots.size(); ++c) {
        if (csize[(size_t)roots[c]] < cfg.min_num_images) break;
        id_of[(size_t)roots[c]] = (int32_t)c;
        ++out.n_clusters;
        out.images_clustered += csize[(size_t)roots[c]];
    }
    for (int v = 0; v < n; ++v)
        if (hhas[(size_t)v]) cluster_id[v] = id_of[(size_t)hlabel[(size_t)v]];
}

void prune_host(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *w, const PruneSettings &cfg, int32_t *cluster_id,
                int32_t *obs_count, const PrunePairs *pairs, PruneOutcome &out) {
    const std::string who("xm_prune_weakly_connected");
    if (n < 0 || m < 0 || nobs < 0) throw Error(XM_ERR_ARG, who + ": negative size");
    if (n >= ((int64_t)1 << 31) || m >= ((int64_t)1 << 31) || nobs >= ((int64_t)1 << 31))
        throw Error(XM_ERR_ARG, who + ": cameras, landmarks and observations must each stay below 2^31");
    // the used observations by camera and by landmark, each list in input order
    std::vector<int64_t> cp((size_t)n + 1, 0), lp((size_t)m + 1, 0);
    int64_t nu = 0;
    for (int64_t e = 0; e < nobs; ++e) {
        if (cam[e] < 0 || cam[e] >= n) throw Error(XM_ERR_ARG, who + ": camera index out of range at observation " + std::to_string(e));
        if (lm[e] < 0 || lm[e] >= m) throw Error(XM_ERR_ARG, who + ": landmark index out of range at observation " + std::to_string(e));
        if (w && !(w[e] > 0.0)) continue;
        ++cp[(size_t)cam[e] + 1]; ++lp[(size_t)lm[e] + 1]; ++nu;
    }
    for (int64_t i = 0; i < n; ++i) cp[(size_t)i + 1] += cp[(size_t)i];
    for (int64_t l = 0; l < m; ++l) lp[(size_t)l + 1] += lp[(size_t)l];
    std::vector<int32_t> c_lm((size_t)nu), l_cam((size_t)nu), o_cam((size_t)nu), o_lm((size_t)nu);
    {
        std::vector<int64_t> nc(cp.begin(), cp.end() - 1), nl(lp.begin(), lp.end() - 1);
        int64_t u = 0;
        for (int64_t e = 0; e < nobs; ++e) {
            if (w && !(w[e] > 0.0)) continue;
            c_lm[(size_t)nc[(size_t)cam[e]]++] = lm[e];
            l_cam[(size_t)nl[(size_t)lm[e]]++] = cam[e];
            o_cam[(size_t)u] = cam[e]; o_lm[(size_t)u] = lm[e]; ++u;
        }
    }
    hipStream_t st = nullptr;   // the default stream, as xm_clean_observations
    DevBuf<int64_t> dcp, dlp;
    DevBuf<int32_t> dc_lm, dl_cam, do_cam, do_lm;
    upload(dcp, cp.data(), cp.size(), st); upload(dlp, lp.data(), lp.size(), st);
    upload(dc_lm, c_lm.data(), c_lm.size(), st); upload(dl_cam, l_cam.data(), l_cam.size(), st);
    upload(do_cam, o_cam.data(), o_cam.size(), st); upload(do_lm, o_lm.data(), o_lm.size(), st);
    PruneLists L;
    L.n = n; L.m = m; L.nobs = nu; L.nheavy = m;   // every list is contiguous here
    L.cam_ptr = dcp.p; L.lm_ptr = dlp.p; L.cam_lm = dc_lm.p; L.lm_cam = dl_cam.p; L.obs_cam = do_cam.p; L.obs_lm = do_lm.p;
    try {
        prune_device(L, cfg, cluster_id, obs_count, pairs, out, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the buffers above are freed next, and the vectors they were filled from
        throw;
    }
    XM_HIP_CHECK(hipStreamSynchronize(st));   // the uploads read the vectors above
}

void prune(const SchurOp &S, const PruneSettings &cfg, int32_t *cluster_id, int32_t *obs_count, const PrunePairs *pairs, PruneOutcome &out, hipStream_t st) {
    const SchurLists l = S.lists();
    PruneLists L;
    L.n = l.n; L.m = l.m; L.nobs = l.nobs; L.nheavy = l.nheavy;
    L.cam_ptr = l.cam_ptr; L.lm_ptr = l.lm_ptr; L.gbase = l.gbase; L.wpos = l.pos_c;
    L.cam_lm = l.cam_lm; L.lm_cam = l.lm_cam; L.deg = l.deg; L.obs_cam = l.obs_cam; L.obs_lm = l.obs_lm;
    L.cam_w = l.cam_w; L.lm_w = l.lm_w;
    prune_device(L, cfg, cluster_id, obs_count, pairs, out, st);
}

}  // namespace xm
