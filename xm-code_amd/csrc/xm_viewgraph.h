// xm_viewgraph.h — two-view match verification and view-graph pruning on the device (include/xm_amd.h: xm_view_graph_filter has the
// definition): the block in front of track establishment in the reference's fork of GLOMAP (global_mapper.cc:56-111:
// image_pair_inliers.cc, relpose_filter.cc, view_graph.cc:9-46).
//
// Launches, all on the default stream and all deterministic in what they write:
//   vg_bearing_kernel      one thread per feature of an image that a scored E pair touches: rule 0
//   vg_score_kernel<TEAM>  one team per pair, TEAM = a wavefront (pairs up to kVgWaveMatches matches, four pairs per workgroup) or a
//                          workgroup (up to kVgGroupMatches): the pair's geometry (E, thresholds, epipoles) in registers, its matches
//                          streamed through the team; the range check of the feature indices (an index out of range is reported and never
//                          used as an address); a first sweep writes a code per match (0, inlier / positive pre-inlier, negative
//                          pre-inlier) and counts both by ballots and a fixed LDS sum; the second sweep applies the F majority
//   vg_score_chunk_kernel  pairs above kVgGroupMatches: one workgroup per chunk of kVgGroupMatches matches does the first sweep; the two
//   vg_score_final_kernel  counts of every chunk go to a workspace; one workgroup per pair adds them in chunk order and does the second sweep
//   vg_decide_kernel       one thread per pair: rules 5 and 6, the pair's status, the `linked` mark of its two images
//   stage_hook_kernel<VgEdge> /  xm_stage.h's FastSV hooking and pointer jumping on int32 image labels over the valid pairs (atomicMin;
//   stage_jump_kernel      a component's final label is its smallest image); kBatch rounds are enqueued ahead of the host
//   vg_size_kernel         images per component (integer atomicAdd)
//   vg_largest_kernel      one workgroup: arg-max of (size, smallest label) and the number of components, by a fixed LDS reduction
//   vg_prune_kernel        registered_out; OUTSIDE; the kept inlier count of every pair
//   stage_scan_*_kernel    xm_stage.h's exclusive prefix sum of the kept counts (three launches): moff_out
//   vg_emit_kernel<TEAM>   one team per kept pair: its inliers in input order through a ballot prefix
//   vg_stats_kernel        the counters per status and per model, inliers
#pragma once

#include <cstdint>

#include "../../include/xm_amd.h"
#include "xm_solver.h"

namespace xm {

constexpr int kVgThreads = 256;          // threads per workgroup (four wavefronts)
constexpr int kVgWaveMatches = 256;      // most matches of a pair that one wavefront runs
constexpr int kVgGroupMatches = 8192;    // most matches of a pair that one workgroup runs; the chunk of the workspace form

struct VgSettings {
    bool score = true;
    double max_E = 1.0, max_F = 4.0, max_H = 4.0;
    int32_t min_inlier_num = 30;
    double min_inlier_ratio = 0.25, cos_max_rotation_error = XM_VG_COS_10DEG;
    double watchdog_s = 600.0;           // host waits give up after this long
};
struct VgOutcome {
    int32_t rounds = 0;
    int64_t matches = 0, inliers = 0, matches_out = 0;
    int64_t pairs_by_status[6] = {0, 0, 0, 0, 0, 0};
    int64_t pairs_by_model[4] = {0, 0, 0, 0};
    int64_t largest = 0, components = 0, pairs_wave = 0, pairs_group = 0, pairs_workspace = 0, max_matches = 0;
    double seconds_index = 0.0, seconds_kernels = 0.0, seconds_download = 0.0;
};

// host arrays; the caller (xm_capi.hip) has checked everything but the feature indices, which are checked on the device (XM_ERR_ARG,
// nothing written).  Runs on the default stream.  Kinv, bearing, FH, valid_in, registered_in and rot may be null.
void view_graph_filter_host(int64_t n, const int64_t *foff, const double *xy, const double *focal, const double *Kinv, const double *bearing,
                            int64_t npairs, const int32_t *pi, const int32_t *pj, const int32_t *model, const double *Rrel, const double *trel,
                            const double *FH, const uint8_t *valid_in, const uint8_t *registered_in, const double *rot, const int64_t *moff,
                            const int32_t *f1, const int32_t *f2, const VgSettings &cfg, uint8_t *inlier, int32_t *pair_inliers, int32_t *pair_status,
                            uint8_t *registered_out, int64_t *moff_out, int32_t *f1_out, int32_t *f2_out, VgOutcome &out);

}  // namespace xm
