// xm_clean.hip — observation cleaning on the device (xm_clean.h; definition in include/xm_amd.h at xm_clean_observations).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/xm_amd.h"
#include "xm_clean.h"
#include "xm_schur.h"
#include "xm_stage.h"

namespace xm {
namespace {

constexpr int kT = 256;   // threads per workgroup of every kernel here (four wavefronts)
static_assert(kT == kStageThreads, "the helpers of xm_stage.h are written for this workgroup size");
constexpr const char *kStage = "observation cleaning";

// slots of the device counter block
enum { C_LIVE = 0, C_OBS_NEW, C_CAMS_WEAK, C_CAMS_EMPTIED, C_CAMS_OFF, C_N_NEW, C_LMS_WEAK, C_LMS_OFF, C_M_NEW, C_COMPONENTS,
       C_FIRST_KEY,   // max over the cameras of (d1 << 32 | ~c): the lowest camera with the largest degree
       C_MAX_SIZE,    // nodes of the largest component
       C_BEST_OBS,    // earliest observation of the largest components
       C_N1, C_SCAN_B, C_SCAN_C, C_COUNT };

__device__ inline u64 ldu(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline bool is_live(int64_t e, const uint8_t *live, const double *w, const int64_t *wpos) {
    if (live) return live[e] != 0;
    if (w) return w[wpos[e]] > 0.0;
    return true;
}

// stage 1: observations per camera
__global__ __launch_bounds__(kT) void clean_deg1_kernel(int64_t nobs, const int32_t *cam, const uint8_t *live, const double *w, const int64_t *wpos,
                                                        uint8_t *live_out, int32_t *d1, u64 *cnt) {
    u64 total = 0;   // per wavefront; one atomic on the shared counter at the end (an atomic per wavefront and 64 observations was a third of a call)
    for (int64_t base = (int64_t)blockIdx.x * kT; base < nobs; base += (int64_t)gridDim.x * kT) {
        const int64_t e = base + threadIdx.x;
        const bool in = e < nobs;
        const bool on = in && is_live(e, live, w, wpos);
        if (in) live_out[e] = on ? 1 : 0;
        wave_add_one(d1, in ? cam[e] : 0, on);
        total += (u64)__popcll(__ballot(on));
    }
    if (lane_id() == 0 && total) atomicAdd(cnt + C_LIVE, total);
}
__global__ __launch_bounds__(kT) void clean_stage1_kernel(int n, const int32_t *d1, int32_t min_cam, int32_t *cs1, u64 *cnt) {
    const int c = (int)(blockIdx.x * kT + threadIdx.x);
    const bool in = c < n;
    const int d = in ? d1[c] : 0;
    const bool ok = in && d > min_cam;
    if (in) cs1[c] = ok ? 1 : 0;
    const u64 key = wave_max(in ? (((u64)(uint32_t)d << 32) | (u64)(0xFFFFFFFFu - (uint32_t)c)) : 0ull);
    if (lane_id() == 0 && key) atomicMax(cnt + C_FIRST_KEY, key);
    wave_count(cnt + C_CAMS_WEAK, in && !ok);
}
// stage 2: observations per landmark among the surviving cameras
__global__ __launch_bounds__(kT) void clean_deg2_kernel(int64_t nobs, const int32_t *cam, const int32_t *lm, const uint8_t *live, const int32_t *cs1,
                                                        int32_t *d2) {
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    const bool in = e < nobs;
    const bool on = in && live[e] && cs1[cam[e]];
    wave_add_one(d2, in ? lm[e] : 0, on);
}
__global__ __launch_bounds__(kT) void clean_stage2_kernel(int m, const int32_t *d2, int32_t min_lm, int32_t *ls2, u64 *cnt) {
    const int l = (int)(blockIdx.x * kT + threadIdx.x);
    const bool in = l < m;
    const bool ok = in && d2[l] > min_lm;
    if (in) ls2[l] = ok ? 1 : 0;
    wave_count(cnt + C_LMS_WEAK, in && !ok);
}
// stage 3: the remaining observations (act) and how many each camera keeps
__global__ __launch_bounds__(kT) void clean_deg3_kernel(int64_t nobs, const int32_t *cam, const int32_t *lm, const uint8_t *live, const int32_t *cs1,
                                                        const int32_t *ls2, uint8_t *act, int32_t *d3) {
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    const bool in = e < nobs;
    const bool on = in && live[e] && cs1[cam[e]] && ls2[lm[e]];
    if (in) act[e] = on ? 1 : 0;
    wave_add_one(d3, in ? cam[e] : 0, on);
}

// components: labels p over the vertices 0 .. n-1 (cameras), n .. n+m-1 (landmarks); an observation that remains is an edge
struct CleanEdge {
    int n;
    const int32_t *cam, *lm;
    const uint8_t *act;
    __device__ bool operator()(int64_t e, int &u, int &v) const {
        if (!act[e]) return false;
        u = cam[e]; v = n + lm[e];
        return true;
    }
};

// nodes per component (at its root, a camera) and its earliest observation
__global__ __launch_bounds__(kT) void clean_sizes_kernel(int n, int m, const int32_t *d3, const int32_t *ls2, const int32_t *p, int32_t *size) {
    const int v = (int)(blockIdx.x * kT + threadIdx.x);
    const bool in = v < n + m;
    const bool node = in && (v < n ? d3[v] > 0 : ls2[v - n] != 0);
    const int r = in ? p[v] : 0;
    wave_add_one(size, r, node && r < n);
}
__global__ __launch_bounds__(kT) void clean_firstobs_kernel(int64_t nobs, const int32_t *cam, const uint8_t *act, const int32_t *p, u64 *firstobs) {
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    const bool on = e < nobs && act[e];
    const int r = on ? p[cam[e]] : 0;
    const u64 mask = __ballot(on);
    if (!mask) return;
    const int leader = __ffsll((long long)mask) - 1;
    const int r0 = __shfl(r, leader);
    // the lanes of the first active lane's component: that lane holds their earliest observation
    if (on && (r != r0 || lane_id() == leader) && ldu(firstobs + r) > (u64)e) atomicMin(firstobs + r, (u64)e);
}
__global__ __launch_bounds__(kT) void clean_select1_kernel(int n, const int32_t *d3, const int32_t *p, const int32_t *size, u64 *cnt) {
    const int c = (int)(blockIdx.x * kT + threadIdx.x);
    const bool root = c < n && d3[c] > 0 && p[c] == c;
    wave_count(cnt + C_COMPONENTS, root);
    const u64 best = wave_max(root ? (u64)(uint32_t)size[c] : 0ull);
    if (lane_id() == 0 && best) atomicMax(cnt + C_MAX_SIZE, best);
}
__global__ __launch_bounds__(kT) void clean_select2_kernel(int n, const int32_t *d3, const int32_t *p, const int32_t *size, const u64 *firstobs, u64 *cnt) {
    const int c = (int)(blockIdx.x * kT + threadIdx.x);
    if (c >= n || d3[c] <= 0 || p[c] != c) return;
    if ((u64)(uint32_t)size[c] == cnt[C_MAX_SIZE]) atomicMin(cnt + C_BEST_OBS, firstobs[c]);
}
// the component of root r is the one that stays
__device__ inline bool chosen(int r, const int32_t *size, const u64 *firstobs, const u64 *cnt) {
    return cnt[C_MAX_SIZE] > 0 && (u64)(uint32_t)size[r] == cnt[C_MAX_SIZE] && firstobs[r] == cnt[C_BEST_OBS];
}
__global__ __launch_bounds__(kT) void clean_keep_obs_kernel(int64_t nobs, const int32_t *cam, const uint8_t *act, const int32_t *p, const int32_t *size,
                                                            const u64 *firstobs, u64 *cnt, uint8_t *keep) {
    u64 total = 0;   // as in clean_deg1_kernel
    for (int64_t base = (int64_t)blockIdx.x * kT; base < nobs; base += (int64_t)gridDim.x * kT) {
        const int64_t e = base + threadIdx.x;
        const bool in = e < nobs;
        const bool k = in && act[e] && chosen(p[cam[e]], size, firstobs, cnt);
        if (in) keep[e] = k ? 1 : 0;
        total += (u64)__popcll(__ballot(k));
    }
    if (lane_id() == 0 && total) atomicAdd(cnt + C_OBS_NEW, total);
}
__global__ __launch_bounds__(kT) void clean_keep_cam_kernel(int n, const int32_t *cs1, const int32_t *d3, const int32_t *p, const int32_t *size,
                                                            const u64 *firstobs, u64 *cnt, int32_t *ckeep) {
    const int c = (int)(blockIdx.x * kT + threadIdx.x);
    const bool in = c < n;
    const bool node = in && d3[c] > 0;
    const bool k = node && chosen(p[c], size, firstobs, cnt);
    if (in) ckeep[c] = k ? 1 : 0;
    wave_count(cnt + C_CAMS_EMPTIED, in && cs1[c] && !node);
    wave_count(cnt + C_CAMS_OFF, node && !k);
    wave_count(cnt + C_N_NEW, k);
}
// one thread per landmark in the CALLER's numbering (slot: where it sits in the kernels' numbering, null = the same)
__global__ __launch_bounds__(kT) void clean_keep_lm_kernel(int m, int n, const int32_t *slot, const int32_t *ls2, const int32_t *p, const int32_t *size,
                                                           const u64 *firstobs, u64 *cnt, int32_t *lkeep) {
    const int l = (int)(blockIdx.x * kT + threadIdx.x);
    const bool in = l < m;
    const int s = in ? (slot ? slot[l] : l) : 0;
    const bool node = in && ls2[s] != 0;
    const int r = node ? p[n + s] : 0;
    const bool k = node && r < n && chosen(r, size, firstobs, cnt);
    if (in) lkeep[l] = k ? 1 : 0;
    wave_count(cnt + C_LMS_OFF, node && !k);
    wave_count(cnt + C_M_NEW, k);
}

// stage-1 index after the exchange of `first` with the camera of index 0, and the final keep flag of every stage-1 POSITION
__global__ __launch_bounds__(kT) void clean_swap_kernel(int n, const int32_t *cs1, const int32_t *idx1, const int32_t *ckeep, const u64 *cnt, int swap,
                                                        int32_t *idx1s, int32_t *posflag) {
    const int c = (int)(blockIdx.x * kT + threadIdx.x);
    if (c >= n) return;
    if (!cs1[c]) { idx1s[c] = -1; return; }
    int k = idx1[c];
    if (swap) {
        const int first = (int)(0xFFFFFFFFu - (uint32_t)(cnt[C_FIRST_KEY] & 0xFFFFFFFFull));
        if (cs1[first]) {   // a first camera below the threshold means that no camera is left: nothing to exchange
            if (c == first) k = 0;
            else if (k == 0) k = idx1[first];
        }
    }
    idx1s[c] = k;
    posflag[k] = ckeep[c];
}
__global__ __launch_bounds__(kT) void clean_cam_index_kernel(int n, const int32_t *ckeep, const int32_t *idx1s, const int32_t *before, int32_t *cam_index) {
    const int c = (int)(blockIdx.x * kT + threadIdx.x);
    if (c < n) cam_index[c] = ckeep[c] ? before[idx1s[c]] : -1;
}
__global__ __launch_bounds__(kT) void clean_lm_index_kernel(int m, const int32_t *lkeep, const int32_t *before, int32_t *lm_index) {
    const int l = (int)(blockIdx.x * kT + threadIdx.x);
    if (l < m) lm_index[l] = lkeep[l] ? before[l] : -1;
}

struct Block { int32_t changed[kBatch]; u64 cnt[C_COUNT]; };   // what the host reads during a call

}  // namespace

void clean_observations_device(const CleanList &L, const CleanSettings &cfg, uint8_t *keep, int32_t *cam_index, int32_t *lm_index, CleanOutcome &out,
                               hipStream_t st) {
    const int64_t nobs = L.nobs;
    if (L.n < 0 || L.m < 0 || nobs < 0) throw Error(XM_ERR_ARG, "observation cleaning: negative size");
    if (L.n + L.m >= ((int64_t)1 << 31)) throw Error(XM_ERR_ARG, "observation cleaning: cameras + landmarks must stay below 2^31");
    if (nobs >= ((int64_t)1 << 39)) throw Error(XM_ERR_ARG, "observation cleaning: more than 2^39 observations");
    const int n = (int)L.n, m = (int)L.m, nv = n + m;
    out = CleanOutcome();
    Pinned<Block> pin;
    DevBuf<u64> cnt, firstobs;
    DevBuf<uint8_t> live, act, dkeep;
    DevBuf<int32_t> d1, d2, d3, cs1, ls2, p, size, ckeep, lkeep, idx1, idx1s, posflag, before, lmbefore, dcam_index, dlm_index, sums, changed, slot;
    fresh(cnt, C_COUNT, 0, st);
    XM_HIP_CHECK(hipMemsetAsync(cnt.p + C_BEST_OBS, 0xff, sizeof(u64), st));
    live.alloc((size_t)nobs, false); act.alloc((size_t)nobs, false); dkeep.alloc((size_t)nobs, false);
    fresh(d1, (size_t)n, 0, st); fresh(d3, (size_t)n, 0, st); fresh(size, (size_t)n, 0, st); fresh(firstobs, (size_t)n, 0xff, st);
    fresh(d2, (size_t)m, 0, st);
    cs1.alloc((size_t)n, false); ckeep.alloc((size_t)n, false); idx1.alloc((size_t)n, false); idx1s.alloc((size_t)n, false);
    fresh(posflag, (size_t)n, 0, st); before.alloc((size_t)n, false); dcam_index.alloc((size_t)n, false);
    ls2.alloc((size_t)m, false); lkeep.alloc((size_t)m, false); lmbefore.alloc((size_t)m, false); dlm_index.alloc((size_t)m, false);
    p.alloc((size_t)nv, false);
    sums.alloc((size_t)(std::max(n, m) / kScanTile + 1), false);
    fresh(changed, (size_t)kMaxRounds + kBatch, 0, st);
    if (L.lm_slot && m > 0) {
        slot.alloc((size_t)m, false);
        XM_HIP_CHECK(hipMemcpyAsync(slot.p, L.lm_slot, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    const unsigned ge = grid_of(nobs), gc = grid_of(n), gl = grid_of(m), gv = grid_of(nv);
    const unsigned gs = std::min(ge, 4096u);   // the two kernels that count observations walk the list with a grid stride

    // degrees and thresholds
    if (ge) hipLaunchKernelGGL(clean_deg1_kernel, dim3(gs), dim3(kT), 0, st, nobs, L.cam, L.live, L.w, L.wpos, live.p, d1.p, cnt.p);
    if (gc) hipLaunchKernelGGL(clean_stage1_kernel, dim3(gc), dim3(kT), 0, st, n, d1.p, cfg.min_cam_obs, cs1.p, cnt.p);
    if (ge) hipLaunchKernelGGL(clean_deg2_kernel, dim3(ge), dim3(kT), 0, st, nobs, L.cam, L.lm, live.p, cs1.p, d2.p);
    if (gl) hipLaunchKernelGGL(clean_stage2_kernel, dim3(gl), dim3(kT), 0, st, m, d2.p, cfg.min_lm_obs, ls2.p, cnt.p);
    if (ge) hipLaunchKernelGGL(clean_deg3_kernel, dim3(ge), dim3(kT), 0, st, nobs, L.cam, L.lm, live.p, cs1.p, ls2.p, act.p, d3.p);
    identity_labels(nv, p.p, st);
    check_launch("clean_degrees");

    const CleanEdge edge = {n, L.cam, L.lm, act.p};
    out.rounds = label_components(nobs, nv, edge, p.p, changed.p, pin.h->changed, kStage, cfg.watchdog_s, st);

    // the largest component, the flags and the index maps
    if (gv) hipLaunchKernelGGL(clean_sizes_kernel, dim3(gv), dim3(kT), 0, st, n, m, d3.p, ls2.p, p.p, size.p);
    if (ge && gc) hipLaunchKernelGGL(clean_firstobs_kernel, dim3(ge), dim3(kT), 0, st, nobs, L.cam, act.p, p.p, firstobs.p);
    if (gc) hipLaunchKernelGGL(clean_select1_kernel, dim3(gc), dim3(kT), 0, st, n, d3.p, p.p, size.p, cnt.p);
    if (gc) hipLaunchKernelGGL(clean_select2_kernel, dim3(gc), dim3(kT), 0, st, n, d3.p, p.p, size.p, firstobs.p, cnt.p);
    if (ge) hipLaunchKernelGGL(clean_keep_obs_kernel, dim3(gs), dim3(kT), 0, st, nobs, L.cam, act.p, p.p, size.p, firstobs.p, cnt.p, dkeep.p);
    if (gc) hipLaunchKernelGGL(clean_keep_cam_kernel, dim3(gc), dim3(kT), 0, st, n, cs1.p, d3.p, p.p, size.p, firstobs.p, cnt.p, ckeep.p);
    if (gl) hipLaunchKernelGGL(clean_keep_lm_kernel, dim3(gl), dim3(kT), 0, st, m, n, slot.p, ls2.p, p.p, size.p, firstobs.p, cnt.p, lkeep.p);
    check_launch("clean_select");
    exclusive_scan(n, cs1.p, idx1.p, sums, cnt.p + C_N1, st);
    if (gc) hipLaunchKernelGGL(clean_swap_kernel, dim3(gc), dim3(kT), 0, st, n, cs1.p, idx1.p, ckeep.p, cnt.p, cfg.swap_first ? 1 : 0, idx1s.p, posflag.p);
    exclusive_scan(n, posflag.p, before.p, sums, cnt.p + C_SCAN_B, st);
    if (gc) hipLaunchKernelGGL(clean_cam_index_kernel, dim3(gc), dim3(kT), 0, st, n, ckeep.p, idx1s.p, before.p, dcam_index.p);
    exclusive_scan(m, lkeep.p, lmbefore.p, sums, cnt.p + C_SCAN_C, st);
    if (gl) hipLaunchKernelGGL(clean_lm_index_kernel, dim3(gl), dim3(kT), 0, st, m, lkeep.p, lmbefore.p, dlm_index.p);
    check_launch("clean_index");

    if (nobs) XM_HIP_CHECK(hipMemcpyAsync(keep, dkeep.p, (size_t)nobs, hipMemcpyDeviceToHost, st));
    if (n) XM_HIP_CHECK(hipMemcpyAsync(cam_index, dcam_index.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (m) XM_HIP_CHECK(hipMemcpyAsync(lm_index, dlm_index.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XM_HIP_CHECK(hipMemcpyAsync(pin.h->cnt, cnt.p, C_COUNT * sizeof(u64), hipMemcpyDeviceToHost, st));
    wait_stream(st, cfg.watchdog_s, kStage, "the kept observations");
    const u64 *c = pin.h->cnt;
    out.nobs_live = (int64_t)c[C_LIVE]; out.nobs_new = (int64_t)c[C_OBS_NEW]; out.n_new = (int64_t)c[C_N_NEW]; out.m_new = (int64_t)c[C_M_NEW];
    out.components = (int64_t)c[C_COMPONENTS]; out.cams_weak = (int64_t)c[C_CAMS_WEAK]; out.lms_weak = (int64_t)c[C_LMS_WEAK];
    out.cams_emptied = (int64_t)c[C_CAMS_EMPTIED]; out.cams_off_component = (int64_t)c[C_CAMS_OFF]; out.lms_off_component = (int64_t)c[C_LMS_OFF];
    out.first_camera = n > 0 ? (int32_t)(0xFFFFFFFFu - (uint32_t)(c[C_FIRST_KEY] & 0xFFFFFFFFull)) : -1;
    if ((int64_t)c[C_SCAN_B] != out.n_new || (int64_t)c[C_SCAN_C] != out.m_new)
        throw Error(XM_ERR_HIP, "observation cleaning: the prefix sums disagree with the counted survivors");
}

void clean_observations_host(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *w, const CleanSettings &cfg,
                             uint8_t *keep, int32_t *cam_index, int32_t *lm_index, CleanOutcome &out) {
    if (n < 0 || m < 0 || nobs < 0) throw Error(XM_ERR_ARG, "xm_clean_observations: negative size");
    if (n + m >= ((int64_t)1 << 31)) throw Error(XM_ERR_ARG, "xm_clean_observations: cameras + landmarks must stay below 2^31");
    std::vector<uint8_t> hlive;
    if (w) hlive.resize((size_t)nobs);
    for (int64_t e = 0; e < nobs; ++e) {
        if (cam[e] < 0 || cam[e] >= n) throw Error(XM_ERR_ARG, "xm_clean_observations: camera index out of range at observation " + std::to_string(e));
        if (lm[e] < 0 || lm[e] >= m) throw Error(XM_ERR_ARG, "xm_clean_observations: landmark index out of range at observation " + std::to_string(e));
        if (w) hlive[(size_t)e] = w[e] > 0.0 ? 1 : 0;
    }
    hipStream_t st = nullptr;   // the default stream: creating one of its own would cost more than a call on a small list
    DevBuf<int32_t> dcam, dlm;
    DevBuf<uint8_t> dlive;
    dcam.alloc((size_t)nobs, false); dlm.alloc((size_t)nobs, false);
    if (nobs) {
        XM_HIP_CHECK(hipMemcpyAsync(dcam.p, cam, (size_t)nobs * sizeof(int32_t), hipMemcpyHostToDevice, st));
        XM_HIP_CHECK(hipMemcpyAsync(dlm.p, lm, (size_t)nobs * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    if (w) {
        dlive.alloc((size_t)nobs, false);
        if (nobs) XM_HIP_CHECK(hipMemcpyAsync(dlive.p, hlive.data(), (size_t)nobs, hipMemcpyHostToDevice, st));
    }
    CleanList L;
    L.n = n; L.m = m; L.nobs = nobs; L.cam = dcam.p; L.lm = dlm.p; L.live = w ? dlive.p : nullptr;
    try {
        clean_observations_device(L, cfg, keep, cam_index, lm_index, out, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);   // the buffers above are freed next: nothing may still be reading them
        throw;
    }
}

void clean_observations(const SchurOp &S, const CleanSettings &cfg, uint8_t *keep, int32_t *cam_index, int32_t *lm_index, CleanOutcome &out, hipStream_t st) {
    const SchurLists l = S.lists();
    CleanList L;
    L.n = l.n; L.m = l.m; L.nobs = l.nobs; L.cam = l.obs_cam; L.lm = l.obs_lm; L.w = l.cam_w; L.wpos = l.pos_c; L.lm_slot = S.slot_of().data();
    try {
        clean_observations_device(L, cfg, keep, cam_index, lm_index, out, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);
        throw;
    }
}

}  // namespace xm
