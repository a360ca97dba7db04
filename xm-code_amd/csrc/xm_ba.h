// xm_ba.h — reprojection bundle adjustment of a recovered XM solution on the matrix-free storage.
//
// The reference refines the XM solution with Ceres (5_test_ceres.py:610-616, utils/ceresforXM.py): SIMPLE_PINHOLE with f = 1, c = 0,
// one residual per observation r_e = pi(Rcw_i P_l + tcw_i) - (p_e0 / p_e2, p_e1 / p_e2), trivial loss, Levenberg-Marquardt with
// ITERATIVE_SCHUR + SCHUR_JACOBI.  Here the same problem runs on the device over the observation lists the SchurOp already holds
// (SchurLists): nothing of the observation structure is copied, only the per-observation Jacobians are stored (in both list orders).
//
// Per LM iteration (host loop, xm_ba.hip):
//   eval        r_e, J_e = [J_c | J_P] at the current point (after an accepted step only)
//   landmarks   V_l = sum J_P^T J_P, g_l = sum J_P^T r, (V_l + mu D_l)^-1                 thread per light landmark, workgroup per heavy one
//   cameras     U_i, g_i, S_ii = U*_i - sum_l (sum_e W_e) V*^-1 (sum_f W_f)^T (e, f: the observations of (i, l), one unless a pair is named
//               twice), its Cholesky inverse, b_i = -g_i + sum W V*^-1 g_l                                             wavefront per camera
//   PCG         S dc = b from zero, S applied as U* x - sum W V*^-1 W^T x through the two lists, block-Jacobi preconditioner, batches that
//               run ahead of the host and are polled through a state word (as SchurOp::pcg_solve)
//   or dense    (XM_BA_DENSE_SCHUR) S assembled as a dense lower block triangle (wavefront per block row), Cholesky factor and two
//               triangular substitutions (xm_dense_la.hip); a pivot that is not positive or a non-finite solution makes the step invalid
//               (flag in the state word, read with the candidate's scalars); |b - S dc| / |b| through the matrix-free product for the trace
//   back-subst  dP_l = -V*_l^-1 (g_l + sum W^T dc)
//   candidate   Rcw <- Exp(dtheta) Rcw, tcw += dt, P += dP; its cost and the model decrease; ONE read of the scalars by the host
//   precond     (XM_BA_PRECOND_BLOCKS / XM_BA_PRECOND_TWO_LEVEL, opt-in) M^-1 = blockdiag(S_aa)^-1 [+ P A_c^-1 P^T] in place of the inverted camera
//               blocks: aggregates of XM_BA_AGG_CAMS cameras along a breadth-first order (host, once per call); per LM iteration a workgroup
//               per aggregate assembles S_aa in LDS and inverts it there, a wavefront per aggregate assembles its rows of A_c = P^T S P
//               (a compensated sum: thousands of small terms meet P^T U* P in every entry)
//               (P: the 7 rigid-plus-scale motions of each aggregate, 4 with fixed rotations; recomputed after every accepted step), and
//               A_c is inverted by spd_inverse_device; per PCG iteration two launches (update + block GEMVs + P^T r; coarse GEMV +
//               combination + <r, z>) replace the update kernel
// Every sum over observations is a fixed-order sum (lane-strided lists + DPP trees, per-workgroup partials added in a fixed order): two
// calls give the same bits.  f64 throughout.
//
// Robust losses (Huber, SoftL1, Cauchy, Arctan; Ceres's definitions): the eval kernel stores sqrt(rho') r and sqrt(rho') J (Ceres's
// Corrector when rho'' <= 0) and the cost 1/2 sum rho(|r|^2), so every later pass is the same.  Non-monotonic steps (the reference's
// use_nonmonotonic_steps): Ceres's TrustRegionStepEvaluator on the host, the least-cost point is returned.
// Deliberate deviation from Ceres: no Jacobi column scaling of J (with block-Jacobi PCG and the damping mu diag(J^T J) it changes only the
// clamp of D and the norm of the PCG's stop test).  The rotation is the left-multiplied rotation vector (Ceres's quaternion Plus turns by
// 2|delta|: only the meaning of gradient_tol differs).  |x| in the parameter tolerance counts 1 per free rotation (a unit quaternion) plus
// |tcw|^2 and |P|^2.
//
// Focal scales (XM_BA_REFINE_FOCAL, xm_ctx_bundle_adjust_focal; the model: include/xm_amd.h): one g_i > 0 per camera, r_e = g_i pi(X) - z_e,
// the last column of the camera block (CD = 7, or 4 with fixed rotations): d r / d g = pi(X), the pose and point Jacobians times g_i.  The
// eval, candidate and cost kernels read the focal scales of their parameter set (three sets beside R / T / P); every pass between them reads
// the stored records and is the CD-generic code of the 6 / 3 forms.  A held focal (focal_free[i] = 0) has a zero column: its diagonal entry
// is mu 1e-6 by the clamp, its right-hand side 0, its step exactly 0; the candidate kernel copies it.  A candidate focal <= 0 sets
// bad_focal in the state word and the host rejects the step as it rejects a failed factorisation.  |x|^2 adds g_i^2 per used camera with
// a free focal.  The aggregate preconditioners are not instantiated for CD = 7 / 4 (refused at the entry point).
//
// Radial distortion (XM_BA_REFINE_RADIAL, xm_ctx_bundle_adjust_radial; the model: include/xm_amd.h): one coefficient k_i per camera beside
// the focal scale, r_e = g_i s u - z_e with u = pi(X), s = 1 + k_i |u|^2 (COLMAP's SIMPLE_RADIAL, BAL's model with k2 = 0).  The last column
// of the camera block (CD = 8, or 5 with fixed rotations), the focal column before it: d r / d g = s u, d r / d k = g |u|^2 u, and
// d r / d u = g (s I + 2 k u u^T) in front of the pinhole pose and point rows.  As with the focal scales only the eval, candidate and cost
// kernels read the coefficients; every pass between them is the CD-generic code.  focal_free and dist_free are independent masks; a held
// column is zero (diagonal mu 1e-6, right-hand side 0, step exactly 0).  A candidate with 1 + 3 k |u|^2 <= 0 at a used observation (the
// radial map folds there) sets bad_focal from the cost kernel, which computes the candidate's projection anyway; the caller's start is not
// checked.  |x|^2 adds k_i^2 per used camera with a free coefficient.  No focal groups and no aggregate preconditioners at CD = 8 / 5.
//
// Focal groups (xm_ctx_bundle_adjust_focal_groups): one focal scale per group of cameras, GLOMAP's Camera shared among images.  With E the
// 0/1 matrix that copies a group's unknown into the focal column of each member, J_shared = J_7 E and, as the landmark elimination commutes
// with E, S_shared = E^T S_7 E, b_shared = E^T b_7: the CD = 7 / 4 kernels run unchanged on expanded vectors.  New around them: an expand
// before the product (and before the back-substitution), a fixed-order sum by group after it, a set-up pass per LM iteration (D_c, b_c, the
// preconditioner's F_c, which groups move) and the group's candidate.  The camera pass leaves the members' focal diagonal undamped
// (summing mu clamp(U_ff,i) is not mu clamp(sum U_ff,i) once a member's clamp is active); mu D_c x_c joins in the group sum.  The PCG runs
// on CD n vectors whose focal slots are 0 but for each group's representative, with M = blockdiag(inverted pose blocks, F): the exact G x G
// focal block for G <= XM_BA_FOCAL_GROUPS_EXACT, its diagonal rule above.  XM_BA_DENSE_SCHUR: the CD n matrix contracted by group in place.
#pragma once

#include <cstdint>
#include <vector>

#include "xm_solver.h"

namespace xm {

class SchurOp;

struct BaSettings {
    int max_iters = 1000;
    double max_time = 300.0, eta = 0.1, function_tol = 1e-6, gradient_tol = 1e-10, parameter_tol = 1e-8;
    bool fix_rotations = false;   // XM_BA_FIX_ROTATIONS: camera blocks are the translation only (3 x 3)
    int loss = XM_BA_LOSS_TRIVIAL;
    double loss_scale = 0.0;      // Ceres's a (normalised image units); robust losses only
    bool nonmonotonic = false;    // XM_BA_NONMONOTONIC
    int max_nonmonotonic = 5;     // Ceres's max_consecutive_nonmonotonic_steps
    bool dense_schur = false;     // XM_BA_DENSE_SCHUR: the reduced camera system assembled densely and solved by Cholesky (eta unused)
    bool refine_focal = false;    // XM_BA_REFINE_FOCAL: a focal scale per camera, the last column of the camera block (CD = 7 / 4)
    double *focal = nullptr;      // n focal scales > 0 (host; bundle_adjust updates them in place, ba_probe only reads them)
    const uint8_t *focal_free = nullptr;   // n, 0 = held; null: all free
    bool refine_dist = false;     // XM_BA_REFINE_RADIAL (with refine_focal, no groups): a radial coefficient per camera, the last column (CD = 8 / 5)
    double *dist = nullptr;       // n radial coefficients, either sign (host; bundle_adjust updates them in place, ba_probe only reads them)
    const uint8_t *dist_free = nullptr;    // n, 0 = held; null: all free
    int64_t ngroups = 0;          // > 0 (xm_ctx_bundle_adjust_focal_groups): one focal scale per group of cameras; focal and focal_free have
    const int32_t *group_of = nullptr;     // ngroups entries then, group_of (n, host) names every camera's group
    int precond = 0;              // PCG preconditioner: 0 the inverted camera blocks | 1 XM_BA_PRECOND_BLOCKS | 2 XM_BA_PRECOND_TWO_LEVEL
    int trace_cap = 0;
    double *trace = nullptr;      // trace_cap x 6 row-major: cost, candidate cost, mu, accepted, PCG iterations, PCG relative residual
                                  // (dense Schur: 0 and |b - S dc| / |b| with S applied matrix-free, -1 after a failed factorisation)
    double watchdog_s = 600.0;    // host waits give up after this long
};
struct BaOutcome {
    int status = 0, iters = 0, accepted = 0, trace_len = 0;
    int coarse_fallbacks = 0;     // two-level preconditioner: LM iterations whose coarse operator could not be inverted (blocks alone)
    int64_t pcg_iters = 0, n_used = 0;
    double initial_cost = 0, final_cost = 0, gradient_max = 0, seconds = 0;
};

// Aggregates of the PCG's opt-in preconditioners (host; xm_ba_aggregate_plan): the cameras with a used observation (used == nullptr: every
// observation counts) in the order of a breadth-first search over the camera-landmark graph of the used observations from camera 0
// (landmarks with more than 64 of them are not expanded) -- repeated from the camera reached last, and that order kept unless camera 0 lies in
// its last level (camera 0 in the middle of a trajectory would give every aggregate two distant stretches) --, the members it never reaches
// appended in index order; aggregate = position / B.
// More than XM_BA_MAX_AGGREGATES aggregates: XM_ERR_ARG.
void ba_aggregate_plan(int64_t n, int64_t nobs, const int32_t *cam, const int32_t *lm, const uint8_t *used, int B, std::vector<int32_t> &order);

// One linearisation for the test export xm_ctx_ba_probe (include/xm_amd.h): inputs and host output arrays, each written only when its pointer
// is not null.  Per-landmark arrays come back by input index.
struct BaProbe {
    double mu = 0.0;
    int64_t k = 0;
    const double *X = nullptr, *dc = nullptr;   // CD n x k column-major; CD n
    double cost = 0, gmax = 0, cost1 = 0, model = 0, step2[2] = {0, 0}, x2[2] = {0, 0};
    int64_t n_used = 0;
    int32_t nagg = 0, ncoarse = 0, coarse_ok = 0;
    double *b = nullptr, *g_l = nullptr, *vinv = nullptr, *ustar = nullptr, *sinv = nullptr;
    int32_t *cused = nullptr, *lused = nullptr;
    double *SX = nullptr, *Sdense = nullptr, *MX = nullptr, *Pm = nullptr, *dropped = nullptr, *Ac = nullptr;
    double *dP = nullptr, *rot1 = nullptr, *t1 = nullptr, *p1 = nullptr;
    double *focal1 = nullptr;   // refine_focal: the candidate's focal scales (n); cost1 is NaN when one of them is not positive
    double *dist1 = nullptr;    // refine_dist: the candidate's radial coefficients (n); cost1 is NaN too when the radial map folds at a used observation
    // focal groups: b, X, SX, MX and dc are vectors of CP n + G entries (CP = CD - 1 columns per camera, then the G focal entries); focal1
    // has G entries; ustar and sinv are the blocks the device holds (the focal diagonal of U* undamped; the inverted pose block with the
    // preconditioner's 1 / F_c in the representative's focal slot)
    double *group_D = nullptr, *group_F = nullptr;   // D_c = clamp(sum U_ff,i) (G); F: G x G column-major for G <= XM_BA_FOCAL_GROUPS_EXACT, else G
};

// rot: 3 x 3n column-major (R_i, camera-to-world), t: 3 x n, p: 3 x m (host, updated in place).  The SchurOp is only read.
void bundle_adjust(const SchurOp &S, const BaSettings &cfg, double *rot, double *t, double *p, BaOutcome &out, hipStream_t st);
// cfg: fix_rotations, loss, loss_scale, precond and watchdog_s are read.  The launches are those of bundle_adjust (one workspace class serves both).
void ba_probe(const SchurOp &S, const BaSettings &cfg, const double *rot, const double *t, const double *p, BaProbe &q, hipStream_t st);
// sqerr[e] = |r_e|^2 (unrobustified) of observation e in input order at (rot, t, p), -1 where it is not used (weight <= 0 or p_e2 <= 0);
// focal: n focal scales, or null for g = 1 (the kernel without them); dist: n radial coefficients beside the focal scales, or null for k = 0
void reprojection_errors(const SchurOp &S, const double *rot, const double *t, const double *p, const double *focal, const double *dist,
                         double *sqerr, double watchdog_s, hipStream_t st);

}  // namespace xm
