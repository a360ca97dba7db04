// xm_tracks.h — feature tracks from pairwise matches on the device (include/xm_amd.h: xm_build_tracks has the definition): the track
// establishment of the reference's fork of GLOMAP (track_establishment.cc:19-227, union_find.h) as connected components of the match graph
// plus an explicit policy for the components that hold two features of one image.
//
// Launches, all on the default stream and all deterministic in what they write:
//   tracks_expand_kernel   one thread per match: the pair by binary search in moff, the two global feature ids (smaller first), the range
//                          check of the feature indices (an index out of range is reported and never used as an address), touched marks
//   tracks_feat_kernel     one thread per feature: its image by binary search in foff, label = itself, touched features per image
//   stage_hook_kernel<TracksEdge> /  xm_stage.h's FastSV hooking and pointer jumping on int32 labels (atomicMin; a component's final
//   stage_jump_kernel      label is its smallest member); kBatch rounds are enqueued ahead of the host, which reads their "changed" words
//   tracks_image_kernel    one workgroup of kTracksThreads per image: compacts (ballots) and sorts (xm_sortstat.h) the (label << 32 |
//                          feature) words of its touched features; equal neighbouring labels are the image's conflicts: they set the
//                          component's flag (atomicOr), count its duplicates in registered images (atomicAdd) and, under
//                          XM_TRACKS_GLOMAP, run the distance test over the run.  Three sizes as xm_lift.hip: kTracksSmallRows words in
//                          2 KB of LDS for every image, kTracksLdsRows in 32 KB for the images the host lists, a global workspace above
//   tracks_size_kernel     rows and rows in registered images per component (integer atomicAdd)
//   tracks_stats_kernel    components, conflicted components and their rows
//   tracks_compact_kernel  XM_TRACKS_SPLIT: the edges of flagged components for the host splitter (xm_tracks_split.h).  Their order in
//                          the list is arbitrary; the splitter sorts them first, so nothing depends on it
//   tracks_relabel_kernel  the splitter's labels back into the label array
//   split_count_kernel /   XM_TRACKS_SPLIT_DEVICE: raw edges per flagged component at its label (integer atomicAdd), two prefix sums (segment
//   split_roots_kernel /   offsets; the flagged roots in label order), the list (label, segment, raw edges, endpoints) the host sorts into
//   split_list_kernel /    the three forms, and the edge words into their segments (an integer slot counter per component: the order inside
//   split_scatter_kernel   a segment is arbitrary, the teams sort it)
//   split_wave_kernel      one wavefront (a workgroup of 64) per component of at most kSplitWaveEnds endpoints and kSplitWaveEdges raw edges:
//                          sorts the segment and both ends of every edge in LDS, drops equal neighbours, turns ids into local indices by
//                          binary search, then walks the edges with endpoint i in lane i: its set label (the smallest local index of its
//                          set, so no find) and its set's images as one bit each in registers; an edge is four lane reads and an AND
//   split_group_kernel     one workgroup per component of at most kSplitGroupEdges raw edges: the same preparation; labels, image slots
//                          and stamps in LDS; per joining edge the members of one set stamp mark[image slot] with the edge's number and
//                          the members of the other look theirs up (no clearing), three barriers, one of them carrying the vote
//   split_mark_kernel      flags the components above the cap for tracks_compact_kernel: they go through the host splitter as before
//   tracks_decide_kernel   per component: kept, or the first rule that drops it
//   stage_scan_*_kernel    xm_stage.h's exclusive prefix sums (three launches): track numbers over the labels, row offsets
//   tracks_rows_kernel     label[] and the row flag of every feature
//   tracks_emit_kernel     one thread per feature: a row at its offset
#pragma once

#include <cstdint>

#include "../../include/xm_amd.h"
#include "xm_solver.h"

namespace xm {

constexpr int kTracksThreads = 256;      // threads per workgroup (four wavefronts)
constexpr int kTracksSmallRows = 256;    // most touched features of an image in the small instantiation
constexpr int kTracksLdsRows = 4096;     // most touched features of an image that are sorted in LDS
constexpr int kTracksWsGroups = 64;      // workgroups of the workspace path
// XM_TRACKS_SPLIT_DEVICE, per conflicted component.  The wavefront form keeps an endpoint per lane and its set's images as one bit each
// of a 64-bit word, so 64 endpoints are its limit; its 512 raw edges take 8 KB of LDS (edge words and both ends of each), twenty
// wavefronts to a CU.  The workgroup form keeps 28 bytes of LDS per raw edge (edge word, both ends, and label, image slot and stamp of
// up to one endpoint more than edges): 4 096 raw edges are 112 KB of the CU's 160 KB, and the next power of two would not fit
constexpr int kSplitWaveEnds = 64;       // most endpoints of a component in the wavefront form (= its threads)
constexpr int kSplitWaveEdges = 512;     // most raw (listed) edges of a component in the wavefront form
constexpr int kSplitGroupEdges = 4096;   // most raw edges of a component in the workgroup form; above: the host splitter

struct TracksSettings {
    int32_t min_views = 3, max_views = 1000000, conflict = XM_TRACKS_SPLIT;
    int64_t max_tracks = 10000000;
    double thres_inconsistency = 10.0;
    double watchdog_s = 600.0;           // host waits give up after this long
    bool split_device = false;           // XM_TRACKS_SPLIT_DEVICE
};
struct TracksOutcome {
    int32_t rounds = 0;
    int64_t nout = 0, ntracks = 0, features_touched = 0, matches = 0, components = 0, components_conflicted = 0, rows_conflicted = 0;
    int64_t tracks_short = 0, tracks_long = 0, tracks_conflict = 0, tracks_few_registered = 0, tracks_beyond_max = 0;
    int64_t images_small = 0, images_large = 0, images_workspace = 0, max_touched = 0, edges_split = 0, unions_refused = 0;
    double seconds_index = 0.0, seconds_kernels = 0.0, seconds_split = 0.0, seconds_download = 0.0;
};

// host arrays.  Checks the offsets and the pairs on the host and the feature indices on the device (XM_ERR_ARG, nothing written), runs on
// the default stream.  registered and label may be null.
void build_tracks_host(int64_t n, const int64_t *foff, const double *xy, const uint8_t *registered, int64_t npairs, const int32_t *pi, const int32_t *pj,
                       const int64_t *moff, const int32_t *f1, const int32_t *f2, const TracksSettings &cfg, int32_t *out_cam, int32_t *out_feat,
                       int32_t *out_track, double *out_xy, int32_t *label, TracksOutcome &out);


// xm_tracks_split_device: label[F] = the smallest member of the set of every endpoint, -1 elsewhere.  eu[e] < ev[e], both checked, nedges > 0.
void tracks_split_device_host(int64_t n, const int64_t *foff, int64_t nedges, const int32_t *eu, const int32_t *ev, int32_t *label, int64_t &distinct,
                              int64_t &refused, double watchdog_s);
// xm_tracks_split_stats: what the calling thread's most recent device split did (SplitDevice's counts, then distinct, refused, 0)
void tracks_split_stats_clear();
void tracks_split_stats_get(int64_t out[8]);

}  // namespace xm
