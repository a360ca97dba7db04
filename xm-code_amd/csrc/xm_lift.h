// xm_lift.h — the reference's depth lift (5_test_ceres.py:191-204 and :244-296; 4_test_unidepth.py:217-262) on the device: from the front
// end's match table and every camera's depth and confidence map to the observation list (cam, lm, p, w) that xm_pair_filter,
// xm_clean_observations and an XM_STORAGE_SCHUR context take (include/xm_amd.h: xm_lift_observations has the definition).
//
// Launches, all on the default stream and all deterministic in what they write:
//   lift_hist_kernel     rows per camera (integer atomics: the sums do not depend on their order)
//   lift_scan_kernel     exclusive prefix sum (one workgroup): the camera's first slot
//   lift_scatter_kernel  row numbers into the camera's slots (the order inside a camera is arbitrary: the next kernel sorts it)
//   lift_cam_kernel      one workgroup of kLiftThreads per camera: sorts the camera's (landmark, input row) words, marks every row but the
//                        first of a landmark as duplicate, samples the maps at the rows inside the border, sorts the sampled depths (as
//                        float32, padded with +inf), forms the percentile in f64 (xm_sortstat.h, as xm_pair.hip), decides every row and
//                        writes, per slot, either the reason it was dropped or its rank among the camera's survivors
//   lift_scan_kernel     exclusive prefix sum of the cameras' survivor counts
//   lift_emit_kernel     one thread per slot: writes cam, lm, p, w, row at (camera's offset + rank)
// lift_cam_kernel exists at three sizes like xm_pair.hip's (12 bytes per row: the word and the float32 depth): every camera with at most
// kLiftSmallRows rows runs in the instantiation with 3 KB of LDS, cameras with at most kLiftLdsRows rows in the one with 48 KB (the
// reference's scenes have a few thousand matches per image), larger ones on a global-memory workspace (kLiftWsGroups
// workgroups, each with its own slice).  The host reads the per-camera row counts after the first scan and lists the cameras of the two
// larger sizes in increasing camera order.
#pragma once

#include <cstdint>

#include "../../include/xm_amd.h"
#include "xm_solver.h"

namespace xm {

constexpr int kLiftThreads = 256;       // threads per workgroup (four wavefronts)
constexpr int kLiftSmallRows = 256;     // most rows of a camera in the small instantiation
constexpr int kLiftLdsRows = 4096;      // most rows of a camera that are sorted in LDS
constexpr int kLiftWsGroups = 64;       // workgroups of the workspace path (each handles the listed cameras with its stride)

struct LiftSettings {
    int32_t margin = 10;
    double depth_pct = 95.0;
    bool maps_on_device = false;
    double watchdog_s = 600.0;          // host waits give up after this long
};
struct LiftOutcome {
    int64_t nout = 0, rows_duplicate = 0, rows_border = 0, rows_depth = 0, rows_no_map = 0;
    int64_t cams_no_map = 0, cams_empty = 0, cams_small = 0, cams_large = 0, cams_workspace = 0, max_rows = 0;
    double seconds_index = 0.0, seconds_kernels = 0.0, seconds_download = 0.0;
};

// host arrays except, with maps_on_device, the maps behind depth[i] / conf[i].  Checks every row (XM_ERR_ARG), uploads and runs on the
// default stream.  conf may be null; threshold may be null.
void lift_observations_host(int64_t n, int64_t m, int64_t nrows, const int32_t *cam, const int32_t *lm, const double *xy, const int32_t *hw,
                            const float *const *depth, const float *const *conf, const double *Kinv, const LiftSettings &cfg, int32_t *out_cam,
                            int32_t *out_lm, double *out_p, double *out_w, int32_t *out_row, double *threshold, LiftOutcome &out);

}  // namespace xm
