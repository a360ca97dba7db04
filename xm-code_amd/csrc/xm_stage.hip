// xm_stage.hip — the kernels and host functions of xm_stage.h that do not depend on the stage, compiled once.
#include <thread>

#include "xm_stage.h"

namespace xm {
namespace {

constexpr int kT = kStageThreads;

__global__ __launch_bounds__(kT) void stage_labels_kernel(int nv, int32_t *p) {
    const int v = (int)(blockIdx.x * kT + threadIdx.x);
    if (v < nv) p[v] = v;
}
__global__ __launch_bounds__(kT) void stage_jump_kernel(int nv, int32_t *p, const int32_t *before, int32_t *changed) {
    if (before && *before == 0) return;
    const int v = (int)(blockIdx.x * kT + threadIdx.x);
    if (v >= nv) return;
    const int p0 = ldi(p + v);
    int r = p0, x = ldi(p + r);
    while (x != r) { r = x; x = ldi(p + r); }   // labels fall strictly along the way: at most v steps
    if (r != p0) { p[v] = r; *changed = 1; }
}

__global__ __launch_bounds__(kT) void stage_scan_sums_kernel(int n, const int32_t *flags, int32_t *sums) {
    __shared__ int lds[kT];
    const int base = (int)blockIdx.x * kScanTile + (int)threadIdx.x * 4;
    int t = 0;
    for (int j = 0; j < 4; ++j)
        if (base + j < n) t += flags[base + j];
    int total;
    block_scan_excl(t, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(kT) void stage_scan_top_kernel(int nb, int32_t *sums, u64 *total_out) {
    __shared__ int lds[kT];
    int carry = 0;
    for (int base = 0; base < nb; base += kScanTile) {
        const int i0 = base + (int)threadIdx.x * 4;
        int v[4], t = 0;
        for (int j = 0; j < 4; ++j) { v[j] = i0 + j < nb ? sums[i0 + j] : 0; t += v[j]; }
        int total;
        int ex = carry + block_scan_excl(t, lds, &total);
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < nb) sums[i0 + j] = ex;
            ex += v[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = (u64)(uint32_t)carry;
}
__global__ __launch_bounds__(kT) void stage_scan_add_kernel(int n, const int32_t *flags, const int32_t *sums, int32_t *out) {
    __shared__ int lds[kT];
    const int base = (int)blockIdx.x * kScanTile + (int)threadIdx.x * 4;
    int v[4], t = 0;
    for (int j = 0; j < 4; ++j) { v[j] = base + j < n ? flags[base + j] : 0; t += v[j]; }
    int total;
    int ex = sums[blockIdx.x] + block_scan_excl(t, lds, &total);
    for (int j = 0; j < 4; ++j) {
        if (base + j < n) out[base + j] = ex;
        ex += v[j];
    }
}

}  // namespace

double secs_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }

void wait_stream(hipStream_t st, double limit, const char *stage, const char *what) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) return;
        if (q != hipErrorNotReady) {
            (void)hipGetLastError();
            throw Error(XM_ERR_HIP, std::string(stage) + ": device error while waiting for " + what + ": " + hipGetErrorString(q));
        }
        if (secs_since(t0) > limit)
            throw Error(XM_ERR_HIP, std::string(stage) + ": watchdog: no progress for " + std::to_string((int)limit) + " s while waiting for " + what);
        std::this_thread::yield();
    }
}

void exclusive_scan(int n, const int32_t *flags, int32_t *out, DevBuf<int32_t> &sums, u64 *total, hipStream_t st) {
    if (n <= 0) return;
    const int nb = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(stage_scan_sums_kernel, dim3((unsigned)nb), dim3(kT), 0, st, n, flags, sums.p);
    hipLaunchKernelGGL(stage_scan_top_kernel, dim3(1), dim3(kT), 0, st, nb, sums.p, total);
    hipLaunchKernelGGL(stage_scan_add_kernel, dim3((unsigned)nb), dim3(kT), 0, st, n, flags, sums.p, out);
    check_launch("exclusive_scan");
}

void identity_labels(int nv, int32_t *p, hipStream_t st) {
    if (nv > 0) hipLaunchKernelGGL(stage_labels_kernel, dim3(grid_of(nv)), dim3(kT), 0, st, nv, p);
}
void jump_labels(int nv, int32_t *p, const int32_t *before, int32_t *changed, hipStream_t st) {
    hipLaunchKernelGGL(stage_jump_kernel, dim3(grid_of(nv)), dim3(kT), 0, st, nv, p, before, changed);
}

}  // namespace xm
