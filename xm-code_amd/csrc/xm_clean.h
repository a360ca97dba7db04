// xm_clean.h — the reference's observation cleaning (utils/checkconnection.py:checklandmarks) on the device: which observations, cameras
// and landmarks of a list survive the degree thresholds and lie in the largest connected component, and how the survivors are renumbered
// (include/xm_amd.h: xm_clean_observations has the definition).  A pure query: nothing it is given changes.
//
// Kernels on input-order arrays cam[e], lm[e], live[e]; integer arithmetic only.  Degrees by integer atomics (the sums do not depend on
// the order of arrival).  Components by hooking and pointer jumping in the FastSV family on int32 labels over the n + m vertices (cameras
// first): per observation the smaller grandparent label is written with atomicMin to the other end's parent and to the other end itself,
// then every vertex jumps to the root of its tree.  Labels only fall and only to vertices of the same component, so the fixed point is
// unique -- every vertex carries the smallest vertex of its component, which is a camera -- and all outputs are the same bits on every
// call; only the number of rounds depends on the order in which the atomics arrive.  A round is two ordinary launches; the host enqueues
// kBatch rounds and reads their "changed" words in one copy.  The labelling (stage_labels_kernel, stage_hook_kernel<CleanEdge>,
// stage_jump_kernel, label_components) and the prefix sums (stage_scan_*_kernel, exclusive_scan) are xm_stage.h's.
#pragma once

#include <cstdint>

#include "xm_solver.h"

namespace xm {

struct CleanSettings {
    int32_t min_cam_obs = 10, min_lm_obs = 1;
    bool swap_first = true;
    double watchdog_s = 600.0;          // host waits give up after this long
};
struct CleanOutcome {
    int32_t rounds = 0, first_camera = -1;
    int64_t nobs_live = 0, n_new = 0, m_new = 0, nobs_new = 0, components = 0;
    int64_t cams_weak = 0, lms_weak = 0, cams_emptied = 0, cams_off_component = 0, lms_off_component = 0;
};

// Device arrays of one list.  lm[e] numbers the landmarks as the kernels see them (0 .. m-1); lm_slot (HOST, may be null = identity) says
// where the caller's landmark l sits in that numbering, so that lm_index comes out in the caller's order.  The live flags come either as
// live[e] or, when live is null, as w[wpos[e]] > 0 (both null: every observation is live).
struct CleanList {
    int64_t n = 0, m = 0, nobs = 0;
    const int32_t *cam = nullptr, *lm = nullptr;
    const uint8_t *live = nullptr;
    const double *w = nullptr;
    const int64_t *wpos = nullptr;
    const int32_t *lm_slot = nullptr;
};
// keep (nobs), cam_index (n), lm_index (m): host arrays.  The indices of L must be in range (the callers check).
void clean_observations_device(const CleanList &L, const CleanSettings &cfg, uint8_t *keep, int32_t *cam_index, int32_t *lm_index, CleanOutcome &out,
                               hipStream_t st);
// host arrays (w may be null): checks the indices (XM_ERR_ARG), uploads and runs the above on the default stream
void clean_observations_host(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *w, const CleanSettings &cfg,
                             uint8_t *keep, int32_t *cam_index, int32_t *lm_index, CleanOutcome &out);
// the list and the current weights of a matrix-free context
void clean_observations(const SchurOp &S, const CleanSettings &cfg, uint8_t *keep, int32_t *cam_index, int32_t *lm_index, CleanOutcome &out, hipStream_t st);

}  // namespace xm
