// xm_rotavg.h — robust rotation averaging over the view graph on the device (include/xm_amd.h: xm_view_graph_rotations has the definition):
// the IRLS stage of step 3 of the reference's fork of GLOMAP (controllers/global_mapper.cc:76-111, estimators/global_rotation_averaging.cc
// :334-499 with skip_initialization = true and max_num_l1_iterations = 0, math/rigid3d.cc:41-71), from rotations the caller supplies.
//
// Host: the checks (xm_capi.hip, the union-find over the participating pairs among them), the slot of every registered image in image
// order, the participating pairs in input order, the incidence lists camera -> (pair, side) of xm_pair_lists.h over the registered images,
// every pair listed at both of its ends.
//
// Launches, all on the default stream and all deterministic in what they write (no atomic at all):
//   rav_log_kernel        one thread per registered image: rot0 -> angle-axis (rule 4), the state
//   rav_exp_kernel        one thread per registered image: angle-axis -> nine doubles (rule 3); the pair kernel reads matrices
//   rav_pair_kernel       one thread per participating pair: R_2^T (Rrel R_1) and its logarithm in registers; r_e, w_e of the weight type,
//                         a flag per workgroup for a weight that is not finite (rules 5 and 7)
//   rav_cam_kernel        right-hand side and weighted degree per camera over its incidence list in list order: a workgroup per heavy
//                         camera (DPP tree per wavefront, the wavefront sums in a fixed order), a thread per light camera; the gauge
//                         residual and its unit weight at the fixed camera; the inverse diagonal (rules 6 and 8)
//   rav_camx_kernel       Ap = ((L_w + e_f e_f^T) (x) I_3) p in one pass over the incidence lists, gathering p of the opposite camera;
//                         <p, Ap> per workgroup
//   ba_pcg_*_kernel<1>    xm_lm_shared.h's PCG vector kernels on the 3 * registered scalars
//   rav_update_kernel     one thread per registered image: est <- Log(Exp(est) Exp(-x)), the new nine doubles, |x_i| per workgroup
//                         (rules 9 and 10)
//   ba_reduce_kernel      xm_lm_shared.h: the step sum and the flag into the state word
#pragma once

#include <cstdint>

#include "../../include/xm_amd.h"
#include "xm_pair_lists.h"
#include "xm_solver.h"

namespace xm {

constexpr int kRavThreads = kPairListThreads;          // threads per workgroup
constexpr int kRavLightIncidences = kPairListLight;    // most incidences of a camera that one thread walks
constexpr int kRavMaxPcgIters = 500;        // most PCG iterations of one solve (xm_lm_shared.h: kBaMaxPcgIters)

struct RavSettings {
    int32_t weight_type = XM_VGR_GEMAN_MCCLURE, max_iters = 100;
    int64_t fixed_image = -1;               // resolved by the caller: a registered image
    double step_tol = 1e-3, sigma_deg = 5.0;
    double watchdog_s = 600.0;
};
struct RavOutcome {
    int32_t stop = XM_VGR_STOP_NOTHING, iters = 0;
    int64_t pcg_iters = 0, pcg_capped = 0, pairs = 0, registered = 0, fixed_image = -1, cams_heavy = 0, max_incidences = 0;
    double seconds_index = 0.0, seconds_kernels = 0.0, seconds_download = 0.0;
};
struct RavInput {   // host arrays, checked by the caller (xm_capi.hip)
    int64_t n = 0, npairs = 0;
    const uint8_t *registered = nullptr;
    const double *rot0 = nullptr;
    const int32_t *pi = nullptr, *pj = nullptr;
    const double *Rrel = nullptr;
    const uint8_t *valid_in = nullptr;
};
struct RavOutput {   // host arrays
    double *rot_out = nullptr, *angle_axis_out = nullptr, *residual = nullptr, *weight = nullptr, *step_trace = nullptr;
};
struct RavProbe {   // the test export: host arrays, every output may be null
    const double *angle_axis = nullptr, *x = nullptr, *weight_in = nullptr;
    double *rot = nullptr, *residual = nullptr, *gauge = nullptr, *weight = nullptr, *rhs = nullptr, *diagonal = nullptr, *product = nullptr,
           *angle_axis_out = nullptr, *step = nullptr;
};

// true when pair k takes part (rule 1)
inline bool rav_takes_part(const RavInput &in, int64_t k) {
    if (in.valid_in && !in.valid_in[k]) return false;
    return !in.registered || (in.registered[in.pi[k]] && in.registered[in.pj[k]]);
}

void view_graph_rotations_host(const RavInput &in, const RavSettings &cfg, const RavOutput &out, RavOutcome &res);
void view_graph_rotations_probe_host(const RavInput &in, const RavSettings &cfg, const RavProbe &q);

}  // namespace xm
