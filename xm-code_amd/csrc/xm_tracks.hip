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
static_assert((kSplitWaveEdges & (kSplitWaveEdges - 1)) == 0 && (kSplitGroupEdges & (kSplitGroupEdges - 1)) == 0 && kSplitWaveEdges <= kSplitGroupEdges,
              "the split's sorts pad to a power of two");
static_assert(kSplitWaveEnds == 64, "the wavefront form keeps one endpoint per lane and one image per bit of a 64-bit word");
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

// ---- XM_TRACKS_SPLIT_DEVICE: rule 4's split on the device.  A union never crosses components, so walking each component's distinct
// edges in ascending (smaller id, larger id) order gives exactly the sets of the host splitter's global sorted walk.
// slots of the split's counter block
enum { S_COMPONENTS = 0, S_EDGES, S_DISTINCT, S_REFUSED, S_BROKEN, S_COUNT };

// raw edges per flagged component, at its label
__global__ __launch_bounds__(kT) void split_count_kernel(int64_t E, const int32_t *eu, const int32_t *p, const int32_t *cflag, int32_t *ecnt) {
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < E; e += (int64_t)gridDim.x * kT) {
        const int u = eu[e];
        if (u < 0) continue;
        const int r = p[u];
        if (cflag[r] != 0) atomicAdd(ecnt + r, 1);
    }
}
__global__ __launch_bounds__(kT) void split_roots_kernel(int F, const int32_t *ecnt, int32_t *isroot) {
    const int g = (int)(blockIdx.x * kT + threadIdx.x);
    if (g < F) isroot[g] = ecnt[g] > 0 ? 1 : 0;
}
// the flagged roots in label order: (label, first word of its segment, raw edges, endpoints)
__global__ __launch_bounds__(kT) void split_list_kernel(int F, const int32_t *ecnt, const int32_t *segoff, const int32_t *rpos, const int32_t *size, int cap,
                                                        int4 *list) {
    const int g = (int)(blockIdx.x * kT + threadIdx.x);
    if (g >= F || ecnt[g] <= 0) return;
    const int k = rpos[g];
    if (k < cap) list[k] = make_int4(g, segoff[g], ecnt[g], size[g]);
}
// the edge words (smaller id << 32 | larger id) into their component's segment.  The slot counter gives an arbitrary order inside a
// segment; the teams sort it, so nothing depends on it
__global__ __launch_bounds__(kT) void split_scatter_kernel(int64_t E, const int32_t *eu, const int32_t *ev, const int32_t *p, const int32_t *cflag,
                                                           const int32_t *ecnt, const int32_t *segoff, int32_t *slot, u64 *out) {
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < E; e += (int64_t)gridDim.x * kT) {
        const int u = eu[e];
        if (u < 0) continue;
        const int r = p[u];
        if (cflag[r] == 0) continue;
        const int s = atomicAdd(slot + r, 1);
        if (s < ecnt[r]) out[(size_t)segoff[r] + (size_t)s] = ((u64)(uint32_t)u << 32) | (u64)(uint32_t)ev[e];
    }
}
__global__ __launch_bounds__(kT) void split_mark_kernel(int k, const int32_t *roots, int32_t *flag) {
    const int x = (int)(blockIdx.x * kT + threadIdx.x);
    if (x < k) flag[roots[x]] = 1;
}

struct SplitArgs {
    const int2 *work;       // per team: first word of its segment, raw edges
    int32_t nwork;
    const u64 *edges;
    const int64_t *foff;
    const int32_t *fimg;
    int32_t *p;
    u64 *cnt;               // S_* slots
};

// ascending bitonic sort as sort_values of xm_sortstat.h, for a team of T threads (one workgroup)
template <int T, class V>
__device__ inline void team_sort(V *S, int KP) {
    for (int size = 2; size <= KP; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = (int)threadIdx.x; t < (KP >> 1); t += T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const V x = S[i], y = S[j];
                if ((x > y) == up) { S[i] = y; S[j] = x; }
            }
            __syncthreads();
        }
}
// the first index in V[0 .. n) whose value is not below x
__device__ inline int first_not_below(const uint32_t *V, int n, uint32_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (V[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// A team of T threads (one workgroup) and one component of N <= CAP raw edges at edges[off ..): K[0 .. N) becomes the sorted edges as
// (local index of the smaller id << 32 | local index of the larger id), equal neighbours still in place; V[0 .. nv) the distinct
// endpoints, ascending (so the smaller local index is the smaller id).  Returns nv; *distinct (per thread) sums to the distinct edges
// over the team.  K: CAP words, V: 2 CAP words, wtot: T / 64 ints.  Ends with a barrier.
template <int T, int CAP>
__device__ inline int split_prepare(const SplitArgs &a, int off, int N, u64 *K, uint32_t *V, int *wtot, int *distinct) {
    const int tid = (int)threadIdx.x;
    int KP = 2;
    while (KP < N) KP <<= 1;
    for (int q = tid; q < KP; q += T) K[q] = q < N ? a.edges[(size_t)off + (size_t)q] : ~0ull;
    __syncthreads();
    team_sort<T>(K, KP);
    int d = 0;
    for (int q = tid; q < N; q += T) d += q == 0 || K[q] != K[q - 1] ? 1 : 0;
    *distinct = d;
    // both ends of every edge, sorted; ids stay below 2^31, so the padding sorts behind them
    for (int q = tid; q < 2 * KP; q += T) {
        const int e = q < KP ? q : q - KP;
        V[q] = e < N ? (q < KP ? (uint32_t)(K[e] >> 32) : (uint32_t)(K[e] & 0xffffffffull)) : ~0u;
    }
    __syncthreads();
    team_sort<T>(V, 2 * KP);
    // the distinct values to the front, in place: a value moves to an index that is not above its own, and every entry of a chunk is
    // read before the chunk's barrier.  V[c0 - 1] is still the value it was: an earlier chunk wrote there only if it kept everything
    int nv = 0;
    for (int c0 = 0; c0 < 2 * N; c0 += T) {
        const int q = c0 + tid;
        const uint32_t x = q < 2 * N ? V[q] : ~0u;
        const bool on = q < 2 * N && (q == 0 || V[q - 1] != x);
        const u64 mask = __ballot(on);
        const int before = __popcll(mask & ((1ull << lane_id()) - 1ull));
        if (lane_id() == 0) wtot[tid >> 6] = __popcll(mask);
        __syncthreads();
        int at = nv, tot = 0;
#pragma unroll
        for (int x2 = 0; x2 < T / 64; ++x2) { if (x2 < (tid >> 6)) at += wtot[x2]; tot += wtot[x2]; }
        if (on) V[at + before] = x;
        nv += tot;
        __syncthreads();
    }
    for (int q = tid; q < N; q += T) {
        const u64 w = K[q];
        K[q] = ((u64)(uint32_t)first_not_below(V, nv, (uint32_t)(w >> 32)) << 32) | (u64)(uint32_t)first_not_below(V, nv, (uint32_t)(w & 0xffffffffull));
    }
    __syncthreads();
    return nv;
}
// the local index of the first endpoint of endpoint g's image: one number per image of the component, below nv
__device__ inline int image_slot(const SplitArgs &a, const uint32_t *V, int nv, uint32_t g) { return first_not_below(V, nv, (uint32_t)a.foff[a.fimg[g]]); }

// One wavefront (a workgroup of 64) per component of at most kSplitWaveEnds endpoints and kSplitWaveEdges raw edges: lane i keeps
// endpoint i's set label (the smallest local index of its set) and the set's images as a bit mask in registers; an edge is two
// label reads, two mask reads and a compare.  8 KB of LDS
__global__ __launch_bounds__(kSplitWaveEnds) void split_wave_kernel(SplitArgs a) {
    constexpr int CAP = kSplitWaveEdges;
    __shared__ u64 K[CAP];
    __shared__ uint32_t V[2 * CAP];
    __shared__ int wtot[1];
    if ((int)blockIdx.x >= a.nwork) return;
    const int2 w = a.work[blockIdx.x];
    const int N = w.y;
    if (N < 1 || N > CAP) { if (threadIdx.x == 0) atomicAdd(a.cnt + S_BROKEN, 1ull); return; }   // (the host lists it for a larger size)
    int distinct;
    const int nv = split_prepare<kSplitWaveEnds, CAP>(a, w.x, N, K, V, wtot, &distinct);
    if (nv > kSplitWaveEnds) { if (threadIdx.x == 0) atomicAdd(a.cnt + S_BROKEN, 1ull); return; }
    const int lane = (int)threadIdx.x;
    const bool in = lane < nv;
    const uint32_t id = in ? V[lane] : 0u;
    int lab = in ? lane : -1;
    u64 images = in ? 1ull << image_slot(a, V, nv, id) : 0ull;
    int refused = 0;
    u64 prev = ~0ull;
    for (int q = 0; q < N; ++q) {
        const u64 e = K[q];   // (the same word in every lane)
        if (e == prev) continue;
        prev = e;
        const int x = __builtin_amdgcn_readfirstlane((int)(e >> 32)), y = __builtin_amdgcn_readfirstlane((int)(e & 0xffffffffull));
        const int lx = __shfl(lab, x), ly = __shfl(lab, y);
        if (lx == ly) continue;
        const u64 mx = __shfl(images, x), my = __shfl(images, y);
        if (mx & my) { refused += 1; continue; }
        const int lo = lx < ly ? lx : ly, hi = lx < ly ? ly : lx;
        if (lab == lo || lab == hi) images = mx | my;
        if (lab == hi) lab = lo;
    }
    const uint32_t first = (uint32_t)__shfl((int)id, in ? lab : 0);
    if (in) a.p[id] = (int32_t)first;
    wave_sum_to(a.cnt + S_DISTINCT, true, (u64)distinct);
    if (lane == 0 && refused) atomicAdd(a.cnt + S_REFUSED, (u64)refused);
}

// One workgroup per component of at most kSplitGroupEdges raw edges: set labels, image slots and the stamps in LDS.  Per edge that
// joins two sets: the members of the one stamp mark[image slot] with the edge's number, a barrier, the members of the other look
// theirs up (nothing is ever cleared), a barrier with the vote, the relabelling, a barrier.  112 KB of LDS
__global__ __launch_bounds__(kT) void split_group_kernel(SplitArgs a) {
    constexpr int CAP = kSplitGroupEdges;
    __shared__ u64 K[CAP];
    __shared__ uint32_t V[2 * CAP];
    __shared__ int32_t lab[CAP + 1], slot[CAP + 1], mark[CAP + 1];
    __shared__ int wtot[kT / 64];
    if ((int)blockIdx.x >= a.nwork) return;
    const int2 w = a.work[blockIdx.x];
    const int N = w.y;
    const int tid = (int)threadIdx.x;
    if (N < 1 || N > CAP) { if (tid == 0) atomicAdd(a.cnt + S_BROKEN, 1ull); return; }   // (the host splits it)
    int distinct;
    const int nv = split_prepare<kT, CAP>(a, w.x, N, K, V, wtot, &distinct);
    if (nv > CAP + 1) { if (tid == 0) atomicAdd(a.cnt + S_BROKEN, 1ull); return; }   // (a connected component has at most one endpoint more than edges)
    for (int i = tid; i < nv; i += kT) { lab[i] = i; slot[i] = image_slot(a, V, nv, V[i]); mark[i] = 0; }
    __syncthreads();
    int refused = 0;
    u64 prev = ~0ull;
    for (int q = 0; q < N; ++q) {
        const u64 e = K[q];   // (the same word in every thread: every branch below is taken by the whole workgroup)
        if (e == prev) continue;
        prev = e;
        const int lx = lab[(int)(e >> 32)], ly = lab[(int)(e & 0xffffffffull)];
        if (lx == ly) continue;
        const int stamp = q + 1;
        for (int i = tid; i < nv; i += kT)
            if (lab[i] == lx) mark[slot[i]] = stamp;
        __syncthreads();
        int hit = 0;
        for (int i = tid; i < nv; i += kT)
            if (lab[i] == ly && mark[slot[i]] == stamp) hit = 1;
        if (__syncthreads_or(hit)) { refused += 1; continue; }
        const int lo = lx < ly ? lx : ly, hi = lx < ly ? ly : lx;
        for (int i = tid; i < nv; i += kT)
            if (lab[i] == hi) lab[i] = lo;
        __syncthreads();
    }
    for (int i = tid; i < nv; i += kT) a.p[V[i]] = (int32_t)V[lab[i]];
    wave_sum_to(a.cnt + S_DISTINCT, true, (u64)distinct);
    if (tid == 0 && refused) atomicAdd(a.cnt + S_REFUSED, (u64)refused);
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

struct Block { int32_t changed[kBatch]; int32_t firstbad; u64 cnt[C_COUNT]; u64 scnt[S_COUNT]; };   // what the host reads during a call

thread_local int64_t t_split_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // xm_tracks_split_stats

// rule 4 on the host for the components whose label carries a flag: their edges come down, tracks_split walks them, the new labels go
// up.  Everything is enqueued when it returns; hs stays alive until the caller has waited for the stream (the uploads read it)
struct SplitHost {
    DevBuf<u64> sedges;
    DevBuf<int32_t> sfeat, slab;
    TrackSplit sp;
};
void split_on_host(int64_t n64, const int64_t *foff, int64_t E, const int32_t *eu, const int32_t *ev, int32_t *p, const int32_t *flag, u64 *cnt,
                   Pinned<Block> &pin, double watchdog_s, hipStream_t st, SplitHost &hs) {
    hs.sedges.alloc((size_t)E, false);
    hipLaunchKernelGGL(tracks_compact_kernel, dim3(grid_for(E, 4096)), dim3(kT), 0, st, E, eu, ev, p, flag, cnt, hs.sedges.p);
    check_launch("tracks_compact_kernel");
    XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt, sizeof(u64) * C_COUNT, hipMemcpyDeviceToHost, st));
    wait_stream(st, watchdog_s, kStage, "the conflicted edges");
    const u64 ns = pin.h->cnt[C_NSPLIT];
    if (ns > (u64)E) throw Error(XM_ERR_HIP, "tracks: more conflicted edges than matches");
    std::vector<uint64_t> edges((size_t)ns);
    static_assert(sizeof(uint64_t) == sizeof(u64), "the edge words are copied as they are");
    if (ns) XM_HIP_CHECK(hipMemcpyAsync(edges.data(), hs.sedges.p, (size_t)ns * sizeof(u64), hipMemcpyDeviceToHost, st));
    wait_stream(st, watchdog_s, kStage, "the conflicted edges");
    tracks_split(n64, foff, edges, hs.sp);
    upload(hs.sfeat, hs.sp.feat.data(), hs.sp.feat.size(), st);
    upload(hs.slab, hs.sp.label.data(), hs.sp.label.size(), st);
    if (!hs.sp.feat.empty())
        hipLaunchKernelGGL(tracks_relabel_kernel, dim3(grid_of((int64_t)hs.sp.feat.size())), dim3(kT), 0, st, (int)hs.sp.feat.size(), hs.sfeat.p, hs.slab.p, p);
}

// XM_TRACKS_SPLIT_DEVICE: rule 4 for the components whose label carries a flag in cflag (each has an edge), on the device; the
// components above the workgroup form's cap go through split_on_host.  size: endpoints per component, at its label; ncap: no more
// flagged components than this; sums: F / kScanTile + 1 entries.  Everything is enqueued when it returns, the copy of the counters
// into pin.h->scnt included: the caller waits for the stream, then calls split_collect.  ds stays alive until then
struct SplitDevice {
    DevBuf<int32_t> ecnt, isroot, segoff, rpos, slot, hroots, hflag;
    DevBuf<int4> list;
    DevBuf<int2> wwork, gwork;
    DevBuf<u64> scnt, segs;
    std::vector<int2> wlist, glist;   // what wwork and gwork are uploaded from
    std::vector<int32_t> hlist;
    SplitHost hs;
    int64_t wave = 0, group = 0, host = 0, edges_device = 0, edges_host = 0;
};
void split_on_device(int64_t n64, const int64_t *foff, const int64_t *dfoff, int F, int64_t E, const int32_t *eu, const int32_t *ev, int32_t *p,
                     const int32_t *cflag, const int32_t *size, const int32_t *fimg, int64_t ncap, DevBuf<int32_t> &sums, u64 *cnt, Pinned<Block> &pin,
                     double watchdog_s, hipStream_t st, SplitDevice &ds) {
    fresh(ds.ecnt, (size_t)F, 0, st); fresh(ds.slot, (size_t)F, 0, st); fresh(ds.scnt, S_COUNT, 0, st);
    ds.isroot.alloc((size_t)F, false); ds.segoff.alloc((size_t)F, false); ds.rpos.alloc((size_t)F, false);
    ds.list.alloc((size_t)ncap, false); ds.segs.alloc((size_t)E, false);
    const unsigned gf = grid_of(F), ge = grid_for(E, 4096);
    hipLaunchKernelGGL(split_count_kernel, dim3(ge), dim3(kT), 0, st, E, eu, p, cflag, ds.ecnt.p);
    exclusive_scan(F, ds.ecnt.p, ds.segoff.p, sums, ds.scnt.p + S_EDGES, st);
    hipLaunchKernelGGL(split_roots_kernel, dim3(gf), dim3(kT), 0, st, F, ds.ecnt.p, ds.isroot.p);
    exclusive_scan(F, ds.isroot.p, ds.rpos.p, sums, ds.scnt.p + S_COMPONENTS, st);
    hipLaunchKernelGGL(split_list_kernel, dim3(gf), dim3(kT), 0, st, F, ds.ecnt.p, ds.segoff.p, ds.rpos.p, size, (int)ncap, ds.list.p);
    hipLaunchKernelGGL(split_scatter_kernel, dim3(ge), dim3(kT), 0, st, E, eu, ev, p, cflag, ds.ecnt.p, ds.segoff.p, ds.slot.p, ds.segs.p);
    check_launch("split_scatter_kernel");
    std::vector<int4> list((size_t)ncap);
    XM_HIP_CHECK(hipMemcpyAsync(pin.h->scnt, ds.scnt.p, sizeof(u64) * S_COUNT, hipMemcpyDeviceToHost, st));
    if (ncap) XM_HIP_CHECK(hipMemcpyAsync(list.data(), ds.list.p, (size_t)ncap * sizeof(int4), hipMemcpyDeviceToHost, st));
    wait_stream(st, watchdog_s, kStage, "the conflicted components");
    const u64 nc = pin.h->scnt[S_COMPONENTS];
    if (nc > (u64)ncap || pin.h->scnt[S_EDGES] > (u64)E) throw Error(XM_ERR_HIP, "tracks: more conflicted components or edges than there can be");
    // the components by the form that splits them, in label order
    std::vector<int2> &wwork = ds.wlist, &gwork = ds.glist;
    std::vector<int32_t> &hroots = ds.hlist;
    for (size_t k = 0; k < (size_t)nc; ++k) {
        const int4 c = list[k];   // (label, first word, raw edges, endpoints)
        if (c.z <= kSplitWaveEdges && c.w <= kSplitWaveEnds) { wwork.push_back(make_int2(c.y, c.z)); ds.edges_device += c.z; }
        else if (c.z <= kSplitGroupEdges) { gwork.push_back(make_int2(c.y, c.z)); ds.edges_device += c.z; }
        else { hroots.push_back(c.x); ds.edges_host += c.z; }
    }
    ds.wave = (int64_t)wwork.size(); ds.group = (int64_t)gwork.size(); ds.host = (int64_t)hroots.size();
    SplitArgs a;
    a.edges = ds.segs.p; a.foff = dfoff; a.fimg = fimg; a.p = p; a.cnt = ds.scnt.p;
    if (!wwork.empty()) {
        upload(ds.wwork, wwork.data(), wwork.size(), st);
        a.work = ds.wwork.p; a.nwork = (int32_t)wwork.size();
        hipLaunchKernelGGL(split_wave_kernel, dim3((unsigned)a.nwork), dim3(kSplitWaveEnds), 0, st, a);
        check_launch("split_wave_kernel");
    }
    if (!gwork.empty()) {
        upload(ds.gwork, gwork.data(), gwork.size(), st);
        a.work = ds.gwork.p; a.nwork = (int32_t)gwork.size();
        hipLaunchKernelGGL(split_group_kernel, dim3((unsigned)a.nwork), dim3(kT), 0, st, a);
        check_launch("split_group_kernel");
    }
    if (!hroots.empty()) {
        upload(ds.hroots, hroots.data(), hroots.size(), st);
        fresh(ds.hflag, (size_t)F, 0, st);
        hipLaunchKernelGGL(split_mark_kernel, dim3(grid_of((int64_t)hroots.size())), dim3(kT), 0, st, (int)hroots.size(), ds.hroots.p, ds.hflag.p);
        check_launch("split_mark_kernel");
        split_on_host(n64, foff, E, eu, ev, p, ds.hflag.p, cnt, pin, watchdog_s, st, ds.hs);
    }
    XM_HIP_CHECK(hipMemcpyAsync(pin.h->scnt, ds.scnt.p, sizeof(u64) * S_COUNT, hipMemcpyDeviceToHost, st));
}
// behind the caller's wait: the counts of both paths, and the calling thread's statistics
void split_collect(Pinned<Block> &pin, const SplitDevice &ds, int64_t &distinct, int64_t &refused) {
    if (pin.h->scnt[S_BROKEN]) throw Error(XM_ERR_HIP, "tracks: a component did not fit the form it was listed for");
    distinct = (int64_t)pin.h->scnt[S_DISTINCT] + ds.hs.sp.distinct;
    refused = (int64_t)pin.h->scnt[S_REFUSED] + ds.hs.sp.refused;
    const int64_t s[8] = {ds.wave, ds.group, ds.host, ds.edges_device, ds.edges_host, distinct, refused, 0};
    std::memcpy(t_split_stats, s, sizeof(s));
}

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
        rowoff, sums, dlarge, dwsl, docam, dofeat, dotrack;
    DevBuf<u64> cnt, ws;
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
            SplitHost hs;
            SplitDevice ds;
            if (cfg.split_device)
                split_on_device(n64, foff, dfoff.p, F, E, eu.p, ev.p, p.p, cflag.p, size.p, fimg.p, (int64_t)pin.h->cnt[C_CONFLICTED], sums, cnt.p, pin,
                                cfg.watchdog_s, st, ds);
            else
                split_on_host(n64, foff, E, eu.p, ev.p, p.p, cflag.p, cnt.p, pin, cfg.watchdog_s, st, hs);
            // every track is free of conflicts now: the flags go, and the sizes are counted again under the new labels
            XM_HIP_CHECK(hipMemsetAsync(cflag.p, 0, (size_t)F * sizeof(int32_t), st));
            XM_HIP_CHECK(hipMemsetAsync(cdupreg.p, 0, (size_t)F * sizeof(int32_t), st));
            XM_HIP_CHECK(hipMemsetAsync(size.p, 0, (size_t)F * sizeof(int32_t), st));
            XM_HIP_CHECK(hipMemsetAsync(regc.p, 0, (size_t)F * sizeof(int32_t), st));
            hipLaunchKernelGGL(tracks_size_kernel, dim3(gf), dim3(kT), 0, st, F, touched.p, p.p, fimg.p, reg, size.p, regc.p);
            check_launch("tracks_size_kernel (after the split)");
            wait_stream(st, cfg.watchdog_s, kStage, "the split labels");   // (the splitter's arrays are read by the copies above)
            if (cfg.split_device) split_collect(pin, ds, out.edges_split, out.unions_refused);
            else { out.edges_split = hs.sp.distinct; out.unions_refused = hs.sp.refused; }
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

// one thread per edge: both ends are endpoints
__global__ __launch_bounds__(kT) void split_ends_kernel(int64_t E, const int32_t *eu, const int32_t *ev, int32_t *touched) {
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (e < E) { touched[eu[e]] = 1; touched[ev[e]] = 1; }   // (every writer stores the same value)
}

void run_split_device(int64_t n64, const int64_t *foff, int64_t E, const int32_t *eu, const int32_t *ev, int32_t *label, int64_t &distinct, int64_t &refused,
                      double watchdog_s, hipStream_t st) {
    const int F = (int)foff[n64];
    Pinned<Block> pin;
    DevBuf<int64_t> dfoff;
    DevBuf<int32_t> deu, dev, dfimg, p, touched, changed, cflag, size, regc, sums;
    DevBuf<u64> cnt;
    std::vector<int32_t> fimg((size_t)F), hp((size_t)F), ht((size_t)F);
    for (int64_t i = 0; i < n64; ++i)
        for (int64_t g = foff[i]; g < foff[i + 1]; ++g) fimg[(size_t)g] = (int32_t)i;
    upload(dfoff, foff, (size_t)n64 + 1, st);
    upload(deu, eu, (size_t)E, st);
    upload(dev, ev, (size_t)E, st);
    upload(dfimg, fimg.data(), (size_t)F, st);
    fresh(touched, (size_t)F, 0, st); fresh(changed, (size_t)kMaxRounds + kBatch, 0, st); fresh(cnt, C_COUNT, 0, st);
    fresh(cflag, (size_t)F, 1, st);   // (every byte 1: every component is one to split)
    fresh(size, (size_t)F, 0, st); fresh(regc, (size_t)F, 0, st);
    p.alloc((size_t)F, false); sums.alloc((size_t)(F / kScanTile + 1), false);
    identity_labels(F, p.p, st);
    hipLaunchKernelGGL(split_ends_kernel, dim3(grid_of(E)), dim3(kT), 0, st, E, deu.p, dev.p, touched.p);
    check_launch("split_ends_kernel");
    const TracksEdge edge = {deu.p, dev.p};
    label_components(E, F, edge, p.p, changed.p, pin.h->changed, kStage, watchdog_s, st);
    hipLaunchKernelGGL(tracks_size_kernel, dim3(grid_of(F)), dim3(kT), 0, st, F, touched.p, p.p, dfimg.p, (const uint8_t *)nullptr, size.p, regc.p);
    check_launch("tracks_size_kernel");
    SplitDevice ds;
    split_on_device(n64, foff, dfoff.p, F, E, deu.p, dev.p, p.p, cflag.p, size.p, dfimg.p, std::min<int64_t>(F, E), sums, cnt.p, pin, watchdog_s, st, ds);
    XM_HIP_CHECK(hipMemcpyAsync(hp.data(), p.p, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(ht.data(), touched.p, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    wait_stream(st, watchdog_s, kStage, "the split labels");
    split_collect(pin, ds, distinct, refused);
    for (int g = 0; g < F; ++g) label[g] = ht[(size_t)g] ? hp[(size_t)g] : -1;
}

}  // namespace

void tracks_split_stats_clear() { std::memset(t_split_stats, 0, sizeof(t_split_stats)); }
void tracks_split_stats_get(int64_t out[8]) { std::memcpy(out, t_split_stats, sizeof(t_split_stats)); }

void tracks_split_device_host(int64_t n, const int64_t *foff, int64_t nedges, const int32_t *eu, const int32_t *ev, int32_t *label, int64_t &distinct,
                              int64_t &refused, double watchdog_s) {
    hipStream_t st = nullptr;
    try {
        run_split_device(n, foff, nedges, eu, ev, label, distinct, refused, watchdog_s, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the device buffers are freed next: nothing may still be reading them
        throw;
    }
}

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
