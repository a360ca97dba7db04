// xm_pair.h — the reference's pairwise relative-rotation filter (5_test_ceres.py:316-431, "YOUR OWN FILTER HERE") on the device: per camera
// pair with a relative rotation, which common landmarks disagree with it (include/xm_amd.h: xm_pair_filter has the definition).
//
// The list is indexed by camera on the HOST inside the call (a counting pass over the cameras and a sort of every camera's landmarks: it also finds a pair named twice); the
// device gets camptr (n + 1), the landmarks and the input rows of every camera in increasing landmark order, and the points.  One workgroup
// of kPairThreads per pair: it counts the common landmarks (binary search from the shorter list into the longer), compacts them in landmark
// order with a prefix sum, and runs the definition's steps on them.  Every order statistic and every trimmed mean comes from a bitonic sort
// of the workgroup's values (padded with +inf to a power of two); the sums run over the sorted range in a fixed tree (strided partial sums,
// the DPP wave sum of xm_device.h, four wave totals), so two calls give the same bits whatever the input order of the list.  Floating-point
// contraction is off in the whole translation unit: the residual that was sorted and the residual that is compared with the threshold are
// the same bits.  The same code runs at three sizes: every pair goes to an instantiation that holds kPairSmallJoint points in LDS (4 KB per
// workgroup: six workgroups per CU); it lists the pairs with more common landmarks for the instantiation with kPairLdsJoint points (32 KB:
// four per CU), which lists what it cannot hold for the one on a global-memory workspace (kPairWsGroups workgroups, each with its own slice).
// The host reads the length of a list before it launches the next size.
#pragma once

#include <cstdint>

#include "../../include/xm_amd.h"
#include "xm_solver.h"

namespace xm {

constexpr int kPairThreads = 256;       // threads per workgroup (four wavefronts)
constexpr int kPairSmallJoint = 256;     // largest joint set of the small instantiation
constexpr int kPairLdsJoint = 2048;     // largest joint set that is sorted in LDS
constexpr int kPairWsGroups = 64;       // workgroups of the workspace path (each handles the listed pairs with its stride)

struct PairSettings {
    int32_t min_joint = 20, min_flags = 1;
    bool skip_row0 = false;
    double trim = 0.05, dist_pct = 90.0, err_pct = 95.0, mad_factor = 3.0;
    double watchdog_s = 600.0;          // host waits give up after this long
};
struct PairOutcome {
    int64_t pairs_used = 0, pairs_skipped = 0, pairs_degenerate = 0, nobs_flagged = 0, max_joint = 0, pairs_on_workspace_path = 0;
    double seconds_index = 0.0, seconds_kernels = 0.0, seconds_download = 0.0;
};

// host arrays; count (nobs), outlier (nobs), stats (npairs, may be null).  Checks every index (XM_ERR_ARG), builds the index, uploads and
// runs on the default stream.
void pair_filter_host(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *p, int64_t npairs, const int32_t *pi,
                      const int32_t *pj, const double *R, const PairSettings &cfg, int32_t *count, uint8_t *outlier, xm_pair_stat_t *stats,
                      PairOutcome &out);

}  // namespace xm
