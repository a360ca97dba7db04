// xm_stage.h — what the device queries (xm_clean.hip, xm_pair.hip, xm_lift.hip, xm_tracks.hip, xm_viewgraph.hip) and xm_ba.hip share, once:
// the wavefront helpers, the exclusive prefix sum, the component labelling, the watchdog-bounded host wait and the small host plumbing.
// The kernels that do not depend on the stage and the host functions are compiled once, in xm_stage.hip.
// Every device function here is integer code, so this header may stand on either side of a translation unit's
// `#pragma clang fp contract(off)` (unlike xm_sortstat.h, whose percentile() must stand behind it).
// All of it is for workgroups of kStageThreads threads; a user with a workgroup size of its own asserts that the two are equal.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <string>

#include "../../include/xm_amd.h"
#include "xm_common.h"

namespace xm {

typedef unsigned long long u64;

constexpr int kStageThreads = 256;   // threads per workgroup (four wavefronts)
constexpr int kScanTile = 1024;      // entries per workgroup of the prefix sums (256 threads x 4)
constexpr int kMaxRounds = 1024;     // more hooking rounds than this: XM_ERR_HIP ("did not converge")
constexpr int kBatch = 4;            // rounds enqueued between two looks at the changed words

// ---- device helpers
__device__ inline int lane_id() { return (int)(threadIdx.x & 63u); }
__device__ inline int ldi(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// dst[idx] += 1 for every active lane; the lanes that name the same entry as the first active lane share one atomic.  Called by whole
// wavefronts (inactive lanes pass active = false).
__device__ inline void wave_add_one(int32_t *dst, int idx, bool active) {
    const u64 mask = __ballot(active);
    if (!mask) return;
    const int leader = __ffsll((long long)mask) - 1;
    const int idx0 = __shfl(idx, leader);
    const u64 same = __ballot(active && idx == idx0);
    if (active && idx == idx0) {
        if (lane_id() == leader) atomicAdd(dst + idx0, (int32_t)__popcll(same));
    } else if (active) {
        atomicAdd(dst + idx, 1);
    }
}
// *dst += number of lanes with pred; whole wavefronts
__device__ inline void wave_count(u64 *dst, bool pred) {
    const u64 mask = __ballot(pred);
    if (mask && lane_id() == __ffsll((long long)mask) - 1) atomicAdd(dst, (u64)__popcll(mask));
}
// *dst += v over the lanes with pred; whole wavefronts
__device__ inline void wave_sum_to(u64 *dst, bool pred, u64 v) {
    v = pred ? v : 0ull;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane_id() == 0 && v) atomicAdd(dst, v);
}
__device__ inline u64 wave_max(u64 v) {
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}
// the largest k in [0, count) with off[k] <= x (off[0] <= x): at most 32 steps
__device__ inline int owner_of(const int64_t *off, int count, int64_t x) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}
// exclusive prefix sum of t over the workgroup and the workgroup's total; lds: kStageThreads ints; ends with a barrier
__device__ inline int block_scan_excl(int t, int *lds, int *total) {
    const int tid = (int)threadIdx.x;
    lds[tid] = t;
    __syncthreads();
    for (int off = 1; off < kStageThreads; off <<= 1) {
        const int v = tid >= off ? lds[tid - off] : 0;
        __syncthreads();
        lds[tid] += v;
        __syncthreads();
    }
    const int incl = lds[tid];
    *total = lds[kStageThreads - 1];
    __syncthreads();
    return incl - t;
}

// ---- host plumbing
double secs_since(std::chrono::steady_clock::time_point t);
// host wait on the stream, bounded by the watchdog; stage: the caller's name in front of the message
void wait_stream(hipStream_t st, double limit, const char *stage, const char *what);

template <class Block>
struct Pinned {   // what the host reads during a call: one pinned allocation
    Block *h = nullptr;
    Pinned() { XM_HIP_CHECK(hipHostMalloc((void **)&h, sizeof(Block), hipHostMallocDefault)); }
    ~Pinned() { if (h) (void)hipHostFree(h); }
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
};

template <class T>
void upload(DevBuf<T> &b, const T *src, size_t n, hipStream_t st) {
    b.alloc(n, false);
    if (n) XM_HIP_CHECK(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
}
template <class T>
void fresh(DevBuf<T> &b, size_t n, int byte, hipStream_t st) {   // n entries filled with `byte` on the stream
    b.alloc(n, false);
    XM_HIP_CHECK(hipMemsetAsync(b.p, byte, (n ? n : 1) * sizeof(T), st));
}
// workgroups of one thread per item (0 for no item), and of a grid-stride walk: at least one, at most cap
inline unsigned grid_of(int64_t items) { return (unsigned)((items + kStageThreads - 1) / kStageThreads); }
inline unsigned grid_for(int64_t items, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kStageThreads - 1) / kStageThreads, cap)); }

// ---- exclusive prefix sum of int32 flags in three launches: sums per tile of kScanTile, scan of the sums (one workgroup, a carry from
// one kScanTile of sums to the next), add.  out[i] = sum of flags[0 .. i); the total goes to *total (a device counter slot); sums holds
// n / kScanTile + 1 entries.  Nothing is launched for n <= 0.
void exclusive_scan(int n, const int32_t *flags, int32_t *out, DevBuf<int32_t> &sums, u64 *total, hipStream_t st);

// ---- components by hooking and pointer jumping (the FastSV family) on int32 labels p over nv vertices, p[v] <= v always: per edge the
// smaller grandparent label goes with atomicMin to the other end's parent and to the other end itself, then every vertex jumps to the root
// of its tree.  Labels only fall and only to vertices of the same component, so at the fixed point every vertex carries the smallest
// vertex of its component, whatever the order in which the atomics arrive; only the number of rounds depends on it.
void identity_labels(int nv, int32_t *p, hipStream_t st);   // p[v] = v (no check_launch of its own)
void jump_labels(int nv, int32_t *p, const int32_t *before, int32_t *changed, hipStream_t st);   // one launch of the jump kernel

// Edge: a plain struct passed by value with `__device__ bool operator()(int64_t e, int &u, int &v) const`: the two vertices of edge e, or
// false when e takes no part.
template <class Edge>
__global__ __launch_bounds__(kStageThreads) void stage_hook_kernel(int64_t ne, Edge edge, int32_t *p, const int32_t *before, int32_t *changed) {
    if (before && *before == 0) return;   // the round before this one changed nothing: the labels are final (rounds are enqueued ahead of the host)
    const int64_t e = (int64_t)blockIdx.x * kStageThreads + threadIdx.x;
    int u, v;
    if (e >= ne || !edge(e, u, v)) return;
    const int pu = ldi(p + u), pv = ldi(p + v);
    const int gu = ldi(p + pu), gv = ldi(p + pv);
    if (gu == gv) return;
    // the smaller grandparent goes to the other end's parent (hooking) and to the other end itself
    if (gv < gu) { atomicMin(p + pu, gv); atomicMin(p + u, gv); }
    else { atomicMin(p + pv, gu); atomicMin(p + v, gu); }
    *changed = 1;
}

// Labels the components of the ne edges over the nv vertices; p holds a label <= v for every vertex (identity_labels, or the caller's own).
// A round is two ordinary launches; kBatch rounds are enqueued, then one copy brings their words to the caller's pinned[kBatch] and one
// wait_stream follows.  changed: kMaxRounds + kBatch zeroed device words.  Allocates nothing.  Returns the number of rounds; launches
// nothing and returns 0 when there is no edge or no vertex.
// The first wait happens in here: an error that the caller enqueued a copy for in front of the call (xm_viewgraph.hip's firstbad) is
// looked at behind it, so a failure of the labelling itself (device error, watchdog, no convergence) is reported first.
template <class Edge>
int label_components(int64_t ne, int nv, Edge edge, int32_t *p, int32_t *changed, int32_t *pinned, const char *stage, double watchdog_s, hipStream_t st) {
    if (ne == 0 || nv == 0) return 0;
    const unsigned ge = grid_of(ne);
    int rounds = 0;
    bool converged = false;
    while (!converged) {
        if (rounds >= kMaxRounds)
            throw Error(XM_ERR_HIP, std::string(stage) + ": the component labels did not converge in " + std::to_string(kMaxRounds) + " rounds");
        for (int k = 0; k < kBatch; ++k) {
            int32_t *word = changed + rounds + k;
            const int32_t *prev = rounds + k > 0 ? word - 1 : nullptr;   // the round before this one's word
            hipLaunchKernelGGL(stage_hook_kernel<Edge>, dim3(ge), dim3(kStageThreads), 0, st, ne, edge, p, prev, word);
            jump_labels(nv, p, prev, word, st);
        }
        check_launch("label_components");
        XM_HIP_CHECK(hipMemcpyAsync(pinned, changed + rounds, kBatch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        wait_stream(st, watchdog_s, stage, "the component labels");
        for (int k = 0; k < kBatch && !converged; ++k) {
            ++rounds;
            converged = pinned[k] == 0;
        }
    }
    return rounds;
}

}  // namespace xm
