// xm_vgcalib.h — focal lengths from the view graph on the device (include/xm_amd.h: xm_view_graph_calibrate has the definition): step 1 of
// the reference's fork of GLOMAP (global_mapper.cc:37-46, estimators/view_graph_calibration.cc, estimators/cost_function.h:44-222) and,
// with XM_VGC_UPDATE_CONFIG, step 0 in front of it (processors/view_graph_manipulation.cc:170-231, math/two_view_geometry.cc:41-55).
//
// Host: the checks (xm_capi.hip), the participating pairs in input order, the unknown of every camera (-1: constant), the incidence lists
// camera -> (pair, side) of xm_pair_lists.h over the free cameras, a same-camera pair listed once.
//
// Launches, all on the default stream and all deterministic in what they write (no floating-point atomic, no atomic at all):
//   vgc_config_kernel     XM_VGC_UPDATE_CONFIG: one thread per pair that flips from F to E: F = K2^-T [t]x R K1^-1 (rule 7)
//   vgc_setup_kernel      one thread per participating pair: G = K1^T F K0 in registers, a one-sided Jacobi SVD in f64 (at most
//                         kVgcSweeps sweeps), d_01 and d_12 stored as eight planes (rule 1)
//   vgc_eval_kernel       one thread per pair: residual, Jacobian, rho, the corrector-scaled record in six planes; the cost per workgroup
//                         by the DPP tree and a fixed LDS order (rules 2 and 3)
//   vgc_cam_kernel        gradient and diagonal of J^T J per free camera over its incidence list in list order: a workgroup per heavy
//                         camera (DPP tree per wavefront, the wavefront sums in a fixed order), a thread per light camera; b = -g, the
//                         inverse of the damped diagonal, |g|_inf per workgroup
//   vgc_camx_kernel       Ap = (J^T J + mu clamp(diag)) p in one pass over the incidence lists, gathering p of the opposite camera; <p, Ap>
//                         per workgroup
//   ba_pcg_*_kernel<1>    xm_lm_shared.h's PCG vector kernels, one scalar per camera
//   vgc_step_kernel       candidate focals: f + d projected onto f >= lower_bound; |step|^2 and |f|^2 per workgroup
//   vgc_cand_kernel       one thread per pair: the candidate's cost and the model's r.Jd + |Jd|^2 / 2 from the records
//   ba_reduce_kernel      xm_lm_shared.h: partial sums into the state word
//   vgc_finish_kernel     rule 6: one thread per camera and per pair
#pragma once

#include <cstdint>

#include "../../include/xm_amd.h"
#include "xm_pair_lists.h"
#include "xm_solver.h"

namespace xm {

constexpr int kVgcThreads = kPairListThreads;          // threads per workgroup
constexpr int kVgcLightIncidences = kPairListLight;    // most incidences of a camera that one thread walks
constexpr int kVgcMaxPcgIters = 500;         // most PCG iterations of one solve (xm_lm_shared.h: kBaMaxPcgIters)
constexpr int kVgcSweeps = 30;              // most sweeps of the one-sided Jacobi SVD (a 3 x 3 matrix converges in 5 to 8)

struct VgcSettings {
    bool update_config = false;
    double loss_scale = 1e-2, lower_ratio = 0.1, higher_ratio = 10.0, two_view_error = 2.0, function_tol = 1e-5, lower_bound = 1e-3;
    int32_t max_iters = 100;
    double gradient_tol = 1e-10, parameter_tol = 1e-8;   // Ceres's defaults: the reference sets neither
    double watchdog_s = 600.0;
};
struct VgcOutcome {
    int64_t pairs = 0, pairs_same = 0, cams_free = 0, cams_constant = 0, cams_rejected = 0, pairs_invalidated = 0, pairs_flipped = 0;
    int64_t cams_heavy = 0, max_incidences = 0, pcg_iters = 0;
    int32_t iters = 0, accepted = 0, stop = 0, trace_len = 0;
    double initial_cost = 0.0, final_cost = 0.0;
    double seconds_index = 0.0, seconds_kernels = 0.0, seconds_download = 0.0;
};
struct VgcInput {   // host arrays, checked by the caller (xm_capi.hip)
    int64_t ncams = 0, n = 0, npairs = 0;
    const double *focal0 = nullptr, *pp = nullptr;
    const uint8_t *has_prior = nullptr;
    const int32_t *cam_of_image = nullptr, *pi = nullptr, *pj = nullptr, *model = nullptr;
    const double *F = nullptr;
    const uint8_t *valid_in = nullptr;
    const double *Rrel = nullptr, *trel = nullptr;
};
struct VgcOutput {   // host arrays; d_out, model_out, F_out and cost_trace may be null
    double *focal_out = nullptr, *focal_est = nullptr;
    uint8_t *refined = nullptr;
    int32_t *cam_status = nullptr, *pair_status = nullptr;
    double *residual = nullptr, *d_out = nullptr;
    int32_t *model_out = nullptr;
    double *F_out = nullptr, *cost_trace = nullptr;
};
struct VgcProbe {   // the test export: host arrays, every output may be null
    const double *focal = nullptr, *x = nullptr, *d_in = nullptr;
    double mu = 0.0;
    double *d = nullptr, *residual = nullptr, *record = nullptr, *cost = nullptr, *gradient = nullptr, *diagonal = nullptr, *product = nullptr;
};

void view_graph_calibrate_host(const VgcInput &in, const VgcSettings &cfg, const VgcOutput &out, VgcOutcome &res);
void view_graph_calibrate_probe_host(const VgcInput &in, const VgcSettings &cfg, const VgcProbe &q);

}  // namespace xm
