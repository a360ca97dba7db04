// xm_triangulate.h — landmarks from 2-D tracks at given poses: the capability behind step 7 of the reference's fork of GLOMAP
// (deps/glomap/glomap/controllers/global_mapper.cc:322-375, controllers/track_retriangulation.cc), as a query on the device over the
// observation lists of a matrix-free context (include/xm_amd.h: xm_ctx_triangulate_tracks has the contract).  NOTHING HERE WAS COMPARED WITH
// THE REFERENCE'S COMPILED CODE: the fork calls COLMAP's incremental mapper, whose sources are not part of it; the contract is the
// project's own (tests/xm_triangulate_numpy.py).  A pure query: nothing it is given changes, two calls give the same bits, no atomics.
//
// Five launches over SchurLists (xm_schur.h):
//   tri_obs_kernel     a thread per observation in input order: the world ray b = R z / |R z|, the observed point (u, v) = (p_0, p_1) / p_2
//                      and the candidate flag, written at the observation's position of the by-landmark lists (dpos_l).  The ray of a
//                      non-candidate is NaN and so is the padding of the packed groups (the planes are filled with 0xff bytes first): every
//                      comparison with it is false, so the loops below need no mask test.  The candidate bytes are the only new upload.
//   tri_light_kernel   a WAVEFRONT per landmark with at most kSchurHeavy (= 64) observations, a ray per lane.  The two rays of a
//                      hypothesis are broadcast with v_readlane (the pair index is wavefront-uniform), every lane scores its own ray, the
//                      count is the population count of a ballot, and the nine refinement sums are xor butterflies (offsets 1, 2, .. 32:
//                      the contract's pairwise tree).  Chosen over a thread per landmark (tf_light_kernel's form, with coalesced loads of
//                      the packed groups) because that form runs max_hypotheses x L score evaluations and the tree sums serially per
//                      lane with the list either re-read from memory for every hypothesis or held in 6 x 64 registers; the wavefront form
//                      holds one ray per lane and pays for it with loads of stride 64 (lane k reads gbase + 64 k + j; the other 63
//                      landmarks of the group, handled by neighbouring wavefronts, use the rest of each line).  Slots are numbered by
//                      descending degree, so neighbouring wavefronts have nearly equal work.  The thread-per-landmark form is NOT built
//                      and NOT measured; this form is measured at the two sizes of profiles/r39_kbench_triangulate.txt.
//   tri_heavy_kernel   a workgroup per longer landmark, of any length.  Hypotheses are made kTriTile at a time, one per thread (the pair
//                      of a schedule index is a closed form), and their points staged in LDS; then the list is walked once per batch in
//                      tiles of kTriTile rays, a ray per thread held in registers, against all staged points (LDS broadcast reads): a
//                      hypothesis's count is the sum of the ballots' population counts, kept by lane (h mod 64) of each wavefront and
//                      added over the wavefronts in a fixed order through LDS.  The refinement sums are the butterfly per wavefront, a
//                      fixed tree over the four wavefronts of a tile and a binary-counter tree over the tiles (40 levels of LDS: no limit
//                      on the length).  Membership lives in a byte per list position in global memory (each thread re-reads only what it
//                      wrote).  The closing pair search stages tiles of kTriTile member rays in LDS, as tf_heavy_kernel does.
//   tri_emit_kernel    a thread per observation in input order: keep and reason; and, in the same grid-stride walk, the landmark counters.
//   tri_reduce_kernel  one workgroup adds the workgroups' partial counts in a fixed order.
#pragma once

#include <cstdint>

#include "xm_schur.h"

namespace xm {

constexpr int kTriThreads = 256;   // threads per workgroup of every kernel here
constexpr int kTriTile = 256;      // rays per tile and hypotheses per batch of tri_heavy_kernel (one per thread)

struct TriSettings {
    int32_t max_hypotheses = 64, refine_rounds = 2, min_views = 2;
    double cos_min_angle = 0.0, cos_create = 0.0;   // computed once on the host (xm_capi.hip)
    double complete_max_reproj_error = 1e-2;
    double watchdog_s = 600.0;
};
struct TriOutcome {
    int64_t lm[6] = {0, 0, 0, 0, 0, 0};   // landmarks per XM_TRI_LM_* status
    int64_t obs_candidates = 0, obs_kept = 0, obs_readmitted = 0, obs_lost = 0, pairs_tested = 0, hypotheses_scored = 0;
    double seconds_kernels = 0.0, seconds_download = 0.0;
};

// rot 3 x 3n, t 3 x n, p 3 x m column-major (the layouts of bundle_adjust, host; p in-out); candidate: nobs bytes or null; keep, reason
// (nobs), lm_views, lm_status, lm_support, lm_hypothesis (m): host arrays
void triangulate_tracks(const SchurOp &S, const TriSettings &cfg, const double *rot, const double *t, double *p, const uint8_t *candidate,
                        uint8_t *keep, uint8_t *reason, int32_t *lm_views, uint8_t *lm_status, int32_t *lm_support, int32_t *lm_hypothesis,
                        TriOutcome &out, hipStream_t st);

}  // namespace xm
