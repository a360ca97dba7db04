// xm_prune.h — GLOMAP's PruneWeaklyConnectedImages (deps/glomap/glomap/processors/reconstruction_pruning.cc:6-84 with
// ViewGraphManipulater::EstablishStrongClusters, processors/view_graph_manipulation.cc:68-168, and ViewGraph::KeepLargestConnectedComponents /
// MarkConnectedComponents, scene/view_graph.cc:9-90) as a query on the device over observation lists (include/xm_amd.h:
// xm_prune_weakly_connected has the definition).  A pure query: nothing it is given changes, and two calls give the same bits.
//
// Launches, in order (integer arithmetic only; the threshold is the one double, computed once by one thread):
//   prune_lmused_kernel    a thread per observation in input order: used observations per landmark (integer atomics);
//   prune_obscount_kernel  the same walk: obs_count per camera over the landmarks with more than two;
//   prune_covis_kernel<0>  a workgroup per camera i.  A histogram over the cameras j lives in LDS, kPruneTile int32 bins at a time; only the
//                          tiles that hold a j > i are visited, so a camera makes (n - i) / kPruneTile passes, rounded up.  In a pass the
//                          workgroup walks camera i's list: a group of kPruneGroup lanes takes one landmark of up to kPruneHeavy entries
//                          and adds 1 to bin j for every used observation of it (ds_add, an integer sum: one value in any order); the
//                          longer landmarks are then walked by the whole workgroup, one after the other.  A landmark that camera i names
//                          a times is walked a times, which is the a_l(i) a_l(j) of the contract.  Thread t then looks at the bins
//                          [8 t, 8 t + 8): pairs with count >= min_covisibility, edges among them, the largest edge weight;
//   exclusive_scan         over the edges per camera: where camera i's edges start;
//   prune_covis_kernel<1>  the same passes again; the eight bins of a thread are ranked by a prefix sum over the workgroup, so the
//                          edges come out in (i, j) order and no atomic decides a position.  The work is the sum of L^2 over the
//                          landmarks: the reference's, met from both ends, twice (count, then write);
//   select_kth x 2         median and MAD, exact: a histogram of the values' high bits (value >> 12) and a one-workgroup prefix walk that
//                          finds the bucket of the element E / 2, then the same over the low 12 bits inside that bucket; the MAD's values
//                          are |weight - median| with the median read from the device.  Then one thread computes the threshold;
//   label_components x 3   (xm_stage.h) the largest component, the strong clusters and the final marking, each with a few small kernels
//                          around it (sizes per root, the best root by an atomicMax of (size, ~root), the flags of the edges that stay).
// The merge rounds (view_graph_manipulation.cc:95-149) run on the HOST in this version: the valid edges at or above 0.75 threshold that
// join two different strong clusters are compacted on the device (flags, exclusive_scan, a write by rank), their cluster pairs are
// downloaded, a union-find over the cluster labels runs the rounds, and the map cluster -> merged cluster goes back up.  The final ranking
// of the components by (size, smallest image) is a sort of at most n / 2 entries on the host.
//
// LDS: the histogram tile is kPruneTile = 2048 int32 bins = 8 KiB, the scan and the list of long landmarks 1 KiB each: 10 KiB per
// workgroup.  The 160 KiB of a CU hold 16 such workgroups, twice what the wave slots take (8 workgroups of 4 wavefronts, "Max waves per
// CU 32"); the compiler's resource report gives 7 wavefronts per SIMD for both instantiations (34 and 44 VGPR, no scratch).  A tile of 4096
// bins would still fit 8 workgroups and cut the passes at 13 682 cameras (7 -> 4 for camera 0); 2048 keeps the boundary scenes of the
// tests (n = tile +- 1, 2 tile + 1) small.  Not measured.
#pragma once

#include <cstdint>

#include "xm_schur.h"

namespace xm {

constexpr int kPruneThreads = 256;   // threads per workgroup of every kernel here
constexpr int kPruneTile = 2048;     // camera bins of the LDS histogram
constexpr int kPruneGroup = 16;      // lanes that walk one landmark of up to kPruneHeavy entries
constexpr int kPruneHeavy = 64;      // longer landmark lists are walked by the whole workgroup
constexpr int kPruneSelBits = 12;    // low bits of the second level of the order statistics

struct PruneSettings {
    int32_t min_covisibility = 5, min_num_images = 2, min_num_observations = 0;
    double min_threshold = 20.0;
    double watchdog_s = 600.0;
};
struct PruneOutcome {
    int64_t pairs_covisible = 0, n_edges = 0, component_images = 0, strong_clusters = 0, weak_edges = 0, n_clusters = 0, images_clustered = 0;
    int32_t rounds = 0;
    double median = 0.0, mad = 0.0, threshold = 0.0;
    double seconds_kernels = 0.0, seconds_download = 0.0;
};
struct PrunePairs {   // optional host arrays for the visibility graph
    int64_t capacity = 0;
    int32_t *i = nullptr, *j = nullptr, *count = nullptr;
};

// Device lists of one problem.  By camera: the observations of camera i at [cam_ptr[i], cam_ptr[i+1]) with the landmark slot of each.  By
// landmark slot: the first nheavy slots have contiguous lists [lm_ptr[s], lm_ptr[s+1]); the others are packed 64 to a group (entry k of the
// group's lane j at gbase[group] + 64 k + j, deg[s] of them) -- the layout of SchurLists.  Input order: camera and slot of observation e.
// The weights decide which observations are used (> 0); all three null: every observation is used.
struct PruneLists {
    int64_t n = 0, m = 0, nobs = 0, nheavy = 0;
    const int64_t *cam_ptr = nullptr, *lm_ptr = nullptr, *gbase = nullptr, *wpos = nullptr;
    const int32_t *cam_lm = nullptr, *lm_cam = nullptr, *deg = nullptr, *obs_cam = nullptr, *obs_lm = nullptr;
    const double *cam_w = nullptr, *lm_w = nullptr;   // by position of the two lists; observation e's weight is cam_w[wpos[e]]
};

// cluster_id, obs_count (n): host arrays
void prune_device(const PruneLists &L, const PruneSettings &cfg, int32_t *cluster_id, int32_t *obs_count, const PrunePairs *pairs, PruneOutcome &out,
                  hipStream_t st);
// host arrays (w may be null): checks the indices (XM_ERR_ARG), builds the lists of the used observations, uploads and runs the above
void prune_host(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *w, const PruneSettings &cfg, int32_t *cluster_id,
                int32_t *obs_count, const PrunePairs *pairs, PruneOutcome &out);
// the lists and the current weights of a matrix-free context, read where they lie
void prune(const SchurOp &S, const PruneSettings &cfg, int32_t *cluster_id, int32_t *obs_count, const PrunePairs *pairs, PruneOutcome &out, hipStream_t st);

}  // namespace xm
