// xm_gp.h — global positioning on the matrix-free storage: camera centres and points from rotations and bearings, without an initial value.
//
// GLOMAP's estimators/global_positioning.cc in its default ONLY_POINTS form (step 5 of controllers/global_mapper.cc:188-231).  NOT COMPARED
// WITH THE REFERENCE'S COMPILED CODE (it needs Ceres, COLMAP, Eigen and glog): parity rests on the line-cited restatement
// tests/xm_gp_numpy.py.  One residual per used observation e = (camera i, landmark l),
//      r_e = d_e - s_e (P_l - c_i),   d_e = R_i p_e / |p_e|,   F = 1/2 sum rho(|r_e|^2),
// over the camera centres c, the points P and one scale s_e >= 1e-5 per observation; the rotations are read only and the gauge is free.
// Used: current weight > 0, p_e2 > 0 (the bundle adjustment's rule) and a landmark with at least min_views such observations.
//
// The Levenberg-Marquardt loop, the damping D = diag(J^T J) clamped to [1e-6, 1e32], the acceptance rule, the radius updates, the stops and
// the trace record are those of xm_ba.hip.  The elimination has three levels (Ceres's ordering of .cc:310-331): scales, landmarks, cameras.
// With w = rho', v = P_l - c_i, h = w |v|^2, h* = h + mu clamp(h), g_s = -w r.v, eliminating s_e in closed form leaves
//      M_e = w s^2 I - u u^T,  u = w s v / sqrt(h*);     q_e = w s r + u g_s / sqrt(h*)
// and the reduced system is the bundle adjustment's with 3 x 3 camera blocks: U_i = sum M_e, V_l = sum M_e, W_e = -M_e, gradient parts +q_e
// (camera) and -q_e (landmark); the damping of c and P is mu clamp(sum w s^2), the diagonal of the FULL J^T J.
//
// Per LM iteration (host loop, xm_gp.hip):
//   eval        the record (w s^2, u, q_e, g_s / sqrt(h*): 8 doubles) of every observation in both list orders; it depends on mu, so it is
//               written every iteration; cost, used observations, max |g_s|
//   landmarks   V*_l^-1, g_l; thread per light landmark, workgroup per heavy one
//   cameras     U*_i, S_ii^-1, b_i; wavefront per camera
//   PCG         S dc = b from zero with the inverted 3 x 3 camera blocks, to eta or 500 iterations, batches that run ahead of the host and
//               are polled through a state word; the vector kernels are the bundle adjustment's (xm_lm_shared.h)
//   back-subst  dP_l = -V*_l^-1 (g_l + sum W^T dc), then ds_e = -(g_s - w s v.dc + w s v.dP) / h*
//   candidate   c + dc, P + dP, max(s + ds, 1e-5); its cost and the model decrease; ONE read of the scalars by the host
// The bound (DEPARTURE from Ceres, which projects the step and runs a line search): a scale with s_e <= 1e-5 and g_s > 0 is frozen for the
// iteration: its column of J is zero (M_e = w s^2 I, q_e = w s r, ds_e = 0).
// Every sum over observations is a fixed-order sum (lane-strided lists + DPP trees, per-workgroup partials added in a fixed order), no
// atomics: two calls give the same bits.  f64 throughout.
#pragma once

#include <cstdint>

#include "xm_solver.h"

namespace xm {

class SchurOp;

constexpr double kGpMinScale = 1e-5;   // global_positioning.cc:297

struct GpSettings {
    int max_iters = 100;          // optimization_base.h:23
    double max_time = 300.0, eta = 0.1, function_tol = 1e-5, gradient_tol = 1e-10, parameter_tol = 1e-8;   // function_tol: optimization_base.h:25
    int min_views = 3;            // global_positioning.h:33
    int loss = XM_BA_LOSS_HUBER;  // global_positioning.h:44-45
    double loss_scale = 0.1;
    int trace_cap = 0;
    double *trace = nullptr;      // trace_cap x 6 row-major: cost, candidate cost, mu, accepted, PCG iterations, PCG relative residual
    double watchdog_s = 600.0;
};
struct GpOutcome {
    int status = 0, iters = 0, accepted = 0, trace_len = 0;
    int64_t pcg_iters = 0, n_used = 0;
    double initial_cost = 0, final_cost = 0, gradient_max = 0, seconds = 0;
};

// One linearisation for the test export xm_ctx_gp_probe (include/xm_amd.h): inputs and host output arrays, each written only when its
// pointer is not null.  Per-observation and per-landmark arrays come back by input index.
struct GpProbe {
    double mu = 0.0;
    int64_t k = 0;
    const double *s = nullptr, *X = nullptr, *dc = nullptr;   // nobs (null: all 1); 3n x k column-major; 3n
    double cost = 0, gmax = 0, cost1 = 0, model = 0, step2[3] = {0, 0, 0}, x2[3] = {0, 0, 0};
    int64_t n_used = 0;
    double *M = nullptr, *q = nullptr;       // nobs x 6 (upper triangle, row-major), nobs x 3
    int32_t *frozen = nullptr, *oused = nullptr;   // nobs
    double *vinv = nullptr, *g_l = nullptr, *ustar = nullptr, *sinv = nullptr, *b = nullptr;
    int32_t *cused = nullptr, *lused = nullptr;
    double *SX = nullptr, *dP = nullptr, *ds = nullptr, *t1 = nullptr, *p1 = nullptr, *s1 = nullptr;
};

// Camera-to-camera terms and the fixed-centre pass (xm_ctx_global_positioning_pairs, include/xm_amd.h): the view graph's relative translations
// in the same residual, r_m = tau_m - sigma_m (c_j - c_i) with tau_m = -R_j trel_m and one scale sigma_m >= 1e-5 per participating pair
// (global_positioning.cc:149-183).  A pair is an observation whose "point" is the other camera: the record, the closed-form elimination of
// sigma, the freezing rule and the candidate are the observations' (gp_lin), with camera i in the camera's role and camera j in the
// point's.  Pairs touch no landmark: sum M_m, sum w sigma^2 and the gradient parts are summed per camera over the incidence lists of
// xm_pair_lists.h (thread per light camera, workgroup per heavy one) and enter U*_i, S_ii, b_i and the damping inside the camera pass;
// the product adds -sum M_m p_other to the camera side (sum M_m p_i is in U*_i p_i) before <p, Ap> is taken.  Fixed centres: no camera pass and no PCG, dc = 0.
struct GpPairsIn {
    int constraint = XM_GP_ONLY_POINTS;
    bool fix_centres = false;
    int64_t npairs = 0;
    const int32_t *pi = nullptr, *pj = nullptr;   // image_id1, image_id2
    const double *trel = nullptr;                 // 3 npairs: translation of cam2_from_cam1
    const uint8_t *valid = nullptr, *calibrated = nullptr;   // npairs (null: all valid); n (null: all calibrated)
    double reweight_scale = 1.0;
    double *sigma = nullptr;                      // out (may be null): npairs, -1 for a pair that takes no part
    int64_t pairs_used = 0, cams_heavy = 0, max_incidences = 0;   // out
    double weight_scale_pt = 1.0;                 // out
};
// the pairs' side of one linearisation for xm_ctx_gp_probe_pairs: per pair in input order, 0 (sigma1: -1) where it takes no part
struct GpPairProbe {
    const double *sigma_in = nullptr;             // npairs (null: all 1)
    double cost = 0, gsmax = 0, cost1 = 0, model = 0, step2 = 0, x2 = 0;
    double *Mp = nullptr, *qp = nullptr;          // npairs x 6, npairs x 3
    int32_t *pfrozen = nullptr, *pused = nullptr;
    double *dsigma = nullptr, *sigma1 = nullptr;
};

// rot: 3 x 3n column-major (R_i, camera-to-world, read only), t: 3 x n (centres), p: 3 x m (host, the start, updated in place); scales (may be
// null): nobs in input order, -1 for an observation that is not used.  The SchurOp is only read.
void global_positioning(const SchurOp &S, const GpSettings &cfg, const double *rot, double *t, double *p, double *scales, GpOutcome &out, hipStream_t st);
// the same with camera-to-camera terms, per-camera weights of the observation terms or fixed centres; with XM_GP_ONLY_POINTS, no flag and
// calibrated null it launches what global_positioning launches
void global_positioning_pairs(const SchurOp &S, const GpSettings &cfg, GpPairsIn &pairs, const double *rot, double *t, double *p, double *scales,
                              GpOutcome &out, hipStream_t st);
// cfg: min_views, loss, loss_scale and watchdog_s are read.  The launches are those of global_positioning (one workspace class serves both).
void gp_probe(const SchurOp &S, const GpSettings &cfg, const double *rot, const double *t, const double *p, GpProbe &q, hipStream_t st);
// q is filled as by gp_probe from the observation terms (its gmax: over everything the loop's gradient test sees); the pairs' shares go to pq
void gp_probe_pairs(const SchurOp &S, const GpSettings &cfg, GpPairsIn &pairs, const double *rot, const double *t, const double *p, GpProbe &q,
                    GpPairProbe &pq, hipStream_t st);
// out[0]: a landmark with more observations than this has a workgroup of its own; out[1]: observations a wavefront takes from a camera's
// list in one pass; out[2]: threads of a heavy landmark's workgroup (host-only; the tests size their edge cases from them)
void gp_limits(int64_t out[3]);
// out[0]: a camera with more incidences (participating pair ends) than this has a workgroup of its own; out[1]: threads of that workgroup
void gp_pair_limits(int64_t out[2]);

}  // namespace xm
