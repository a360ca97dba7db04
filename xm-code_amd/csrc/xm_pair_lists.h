// xm_pair_lists.h — what the solvers over the view graph's pairs share (xm_vgcalib.hip: the focal lengths; xm_rotavg.hip: the rotations):
// the incidence lists unknown -> (pair, side), built on the host by a stable counting sort and walked on the device by a workgroup per
// heavy unknown and a thread per light one, and the host's small steps around one call's stream.  The code is the one the two files had:
// moving it here changes no bit of their outputs.  The two limits stand in namespace xm, for xm_vgcalib.h and xm_rotavg.h to name their
// own from; everything else is in an anonymous namespace, as in xm_lm_shared.h: each translation unit compiles its own copy, so only .hip
// files (and the two headers, which only .hip files include) include this file.  It holds integer arithmetic and additions only, so
// whether a file includes it before or after a `#pragma clang fp contract` makes no difference to its code.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "xm_device.h"
#include "xm_stage.h"

namespace xm {

constexpr int kPairListThreads = 256;   // threads per workgroup of every kernel that walks the lists
constexpr int kPairListLight = 64;      // most incidences of an unknown that one thread walks; above: a workgroup of its own

namespace {

constexpr int kPairListFlatCap = 1024;   // most workgroups of a grid-stride launch
static_assert(kPairListThreads == 256, "block_sum256 and the four wavefront sums are for 256 threads");

// ---- device
struct PairLists {           // unknown -> (pair, side); what a side means is its solver's
    int n, nheavy;
    const int32_t *order;    // n unknowns: the heavy ones first, each group in index order
    const int64_t *ptr;      // n + 1, by unknown
    const int32_t *pair;
    const uint8_t *side;
};
// which unknown this thread works on and which of its incidences: a workgroup per heavy unknown, a thread per light one
struct PairWalk {
    int u;
    int64_t e, e_end, step;
    bool heavy;
};
__device__ __forceinline__ PairWalk pair_walk(const PairLists &L) {
    PairWalk w;
    w.heavy = (int)blockIdx.x < L.nheavy;
    const int64_t slot = w.heavy ? (int64_t)blockIdx.x : (int64_t)L.nheavy + ((int64_t)blockIdx.x - L.nheavy) * kPairListThreads + threadIdx.x;
    w.u = slot < L.n ? L.order[slot] : -1;
    w.e = 0; w.e_end = 0; w.step = 1;
    if (w.u >= 0) {
        w.e = L.ptr[w.u] + (w.heavy ? threadIdx.x : 0); w.e_end = L.ptr[w.u + 1]; w.step = w.heavy ? kPairListThreads : 1;
    }
    return w;
}
// sum of K values over a heavy unknown's workgroup: DPP tree per wavefront, the four wavefront sums in a fixed order; valid in thread 0
template <int K>
__device__ __forceinline__ void pair_heavy_sum(double (&acc)[K], double (*part)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) part[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
}

// ---- host: the lists
struct PairListsHost {
    int nheavy = 0;
    int64_t max_inc = 0;
    std::vector<int64_t> ptr;
    std::vector<int32_t> pair, order;
    std::vector<uint8_t> side;
};
// ua[m], ub[m]: the unknowns at the two ends of participating pair m, -1 for an end that is no unknown (it gets no incidence).  An
// unknown's incidences stay in input order; one with more than `light` of them is heavy.  same_once: a pair with one unknown at both
// ends is listed once, with side 2 (xm_vgcalib.hip); otherwise at both ends like any other, with sides 0 and 1 (xm_rotavg.hip)
inline PairListsHost build_pair_lists(int n, const std::vector<int32_t> &ua, const std::vector<int32_t> &ub, int light, bool same_once) {
    PairListsHost h;
    auto each_incidence = [&](auto &&f) {
        for (size_t m = 0; m < ua.size(); ++m) {
            const int32_t a = ua[m], b = ub[m];
            const bool sm = same_once && a == b;
            if (a >= 0) f(a, (int32_t)m, (uint8_t)(sm ? 2 : 0));
            if (b >= 0 && !sm) f(b, (int32_t)m, (uint8_t)1);
        }
    };
    h.ptr.assign((size_t)n + 1, 0);
    each_incidence([&](int32_t u, int32_t, uint8_t) { h.ptr[(size_t)u + 1]++; });
    for (int u = 0; u < n; ++u) {
        h.max_inc = std::max(h.max_inc, h.ptr[(size_t)u + 1]);
        h.ptr[(size_t)u + 1] += h.ptr[(size_t)u];
    }
    h.pair.resize((size_t)h.ptr[(size_t)n]); h.side.resize(h.pair.size());
    std::vector<int64_t> fill(h.ptr.begin(), h.ptr.end() - 1);
    each_incidence([&](int32_t u, int32_t m, uint8_t s) {
        const int64_t e = fill[(size_t)u]++;
        h.pair[(size_t)e] = m; h.side[(size_t)e] = s;
    });
    std::vector<int32_t> rest;
    for (int u = 0; u < n; ++u) {
        if (h.ptr[(size_t)u + 1] - h.ptr[(size_t)u] > light) h.order.push_back(u); else rest.push_back(u);
    }
    h.nheavy = (int)h.order.size();
    h.order.insert(h.order.end(), rest.begin(), rest.end());
    return h;
}
// the lists on the device, and the grid of a kernel that walks them
struct PairListsDev {
    DevBuf<int32_t> order, pair;
    DevBuf<uint8_t> side;
    DevBuf<int64_t> ptr;
    PairLists L{};
    int grid = 1;
    void upload_from(const PairListsHost &h, int n, hipStream_t st) {
        upload(order, h.order.data(), (size_t)n, st); upload(ptr, h.ptr.data(), (size_t)n + 1, st);
        upload(pair, h.pair.data(), h.pair.size(), st); upload(side, h.side.data(), h.side.size(), st);
        L.n = n; L.nheavy = h.nheavy; L.order = order.p; L.ptr = ptr.p; L.pair = pair.p; L.side = side.p;
        grid = std::max(1, h.nheavy + (n - h.nheavy + kPairListThreads - 1) / kPairListThreads);
    }
};

// ---- host: around one call's stream
inline int flat_grid_of(int64_t items) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((items + kPairListThreads - 1) / kPairListThreads, kPairListFlatCap));
}
// per pair in input order from the planes of the M participating pairs plist; what takes no part is 0
inline void planes_to_pairs(const std::vector<int32_t> &plist, int npairs, const std::vector<double> &h, int planes, double *outp) {
    const size_t M = plist.size();
    std::memset(outp, 0, (size_t)planes * npairs * sizeof(double));
    for (size_t m = 0; m < M; ++m)
        for (int c = 0; c < planes; ++c) outp[(size_t)planes * plist[m] + c] = h[(size_t)c * M + m];
}
template <class T>
void download(std::vector<T> &h, const T *dev, size_t n, hipStream_t st) {   // the caller waits for the stream
    h.resize(n);
    if (n) XM_HIP_CHECK(hipMemcpyAsync(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
}

}  // namespace

}  // namespace xm
