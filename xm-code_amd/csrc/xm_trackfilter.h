// xm_trackfilter.h — GLOMAP's TrackFilter (deps/glomap/glomap/processors/track_filter.cc:7-126) against a refined geometry, as a query on
// the device over the observation lists of a matrix-free context (include/xm_amd.h: xm_ctx_filter_tracks has the definition).  A pure
// query: nothing it is given changes, and two calls give the same bits.
//
// Four launches and one reduction over SchurLists (xm_schur.h), no atomics anywhere:
//   tf_obs_kernel      a thread per observation in input order (the order obs_p, obs_cam and obs_lm are read in, coalesced): the
//                      camera-frame point q = R^T (P - t), the depth, reprojection and angle tests and the ray (P - t) / |P - t|.  It
//                      writes one code byte and the ray (three planes of lm_total doubles) at the observation's position of the by-landmark
//                      lists (dpos_l) and the code byte again in input order.  The ray of an observation that does not survive is NaN, and
//                      so is the padding of the packed groups (the planes are filled with 0xff bytes first): a dot product with it compares
//                      false, so the pair loops below need no survivor test.
//   tf_light_kernel    a thread per landmark with at most kSchurHeavy observations (lane j of a packed group reads gbase + 64 k + j: every
//                      load of the wavefront is one run of consecutive addresses).  It counts the codes of its list, then walks the pairs
//                      (i, j > i) and stops at the first one whose dot product is below the threshold.  Slots are numbered by descending
//                      degree, so the 64 lists of a wavefront have nearly the same length.  The alternative for a wavefront that idles on
//                      its longest member -- a sub-group of lanes per landmark with cross-lane rotation -- is NOT built and NOT measured:
//                      the scenes measured (profiles/r25_kbench_trackfilter.txt) spend their time in tf_obs_kernel and the copies.
//   tf_heavy_kernel    a workgroup per landmark with a contiguous list of any length: tiles of kTfTile rays are staged in LDS from global
//                      memory and every pair of tiles (a, b >= a) is visited once; thread i of the workgroup owns ray i of tile a and reads
//                      the rays of tile b at one address per step (an LDS broadcast, no bank conflict).  An LDS flag raised by any thread
//                      that found a pair is looked at before each pair of tiles, so a well-conditioned track ends after its first one.
//                      A pair's dot product (x x' + y y') + z z' is symmetric in its arguments, so the visiting order cannot change the
//                      verdict, a boolean OR over the pairs.
//                      Tile size: kTfTile = 256 rays = 6 KiB per tile, 12 KiB per workgroup for the two tiles; the 160 KiB of a CU hold 13
//                      such workgroups, so the wave slots (8 workgroups of 4 wavefronts, MI355X_MICROARCH.md "Max waves per CU 32") and
//                      not the LDS bound the occupancy.  A larger tile would halve the barriers per pair of rays but is not measured.
//   tf_emit_kernel     a thread per observation in input order: keep and the final reason from the code byte, the landmark's verdict and
//                      min_views; and, in the same grid-stride walk, the per-landmark counters.  Every workgroup leaves its partial counts;
//   tf_reduce_kernel   one workgroup adds them in a fixed order.
// Both landmark kernels end in tf_verdict(): the survivors, the status and the "changed" bits of one landmark.
#pragma once

#include <cstdint>

#include "xm_schur.h"

namespace xm {

constexpr int kTfThreads = 256;   // threads per workgroup of every kernel here
constexpr int kTfTile = 256;      // rays per LDS tile of tf_heavy_kernel (one per thread)

struct TfSettings {
    uint32_t flags = 0;              // XM_TF_REPROJECTION | XM_TF_ANGLE | XM_TF_TRIANGULATION
    double max_reprojection_error = 0.0;
    double cos_angle = 0.0, cos_triangulation = 0.0;   // computed once on the host (xm_capi.hip)
    int32_t min_views = 0;
    double watchdog_s = 600.0;
};
struct TfOutcome {
    int64_t tracks_total = 0, tracks_kept = 0, obs_used = 0, obs_kept = 0;
    int64_t dropped_depth = 0, dropped_reprojection = 0, dropped_angle = 0, dropped_triangulation = 0, dropped_min_views = 0;
    int64_t changed_reprojection = 0, changed_angle = 0, changed_triangulation = 0, changed_min_views = 0;
    double seconds_kernels = 0.0, seconds_download = 0.0;
};

// rot 3 x 3n, t 3 x n, p 3 x m column-major (the layouts of bundle_adjust, host); keep, reason (nobs), lm_views, lm_status (m): host arrays
void filter_tracks(const SchurOp &S, const TfSettings &cfg, const double *rot, const double *t, const double *p, uint8_t *keep, uint8_t *reason,
                   int32_t *lm_views, uint8_t *lm_status, TfOutcome &out, hipStream_t st);

}  // namespace xm
