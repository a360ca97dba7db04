// xm_schur.h — matrix-free Q for the XM solve (the reference's own "TODO: implement sparse Q matrix
// construction", utils/creatematrix.py:54-56).
//
// The reference forms the dense 3N x 3N Schur complement Q = Q1 - Vtp_bar Qtp_bar^{-1} Vtp_bar^T on the host
// (creatematrix.py:137-339: Q1, V1, V2, V3, the bipartite Laplacian Qtp, two solves with the reduced camera Laplacian
// VT = Q2_bar - V3_bar Q3^{-1} V3_bar^T) and the solver multiplies with it (72 N^2 bytes per product).  Here the factors stay
// factors: the context is created from the observation list itself (the arguments of create_matrix: camera, landmark,
// camera-frame point, weight) and a product Y = alpha * Q * W is the chain
//      h_l   = -(1/Q3_l) sum_{obs of l} w (p . W_i)                       per landmark      (V2^T W, landmarks eliminated)
//      r_i   =  c_i . W_i + sum_{obs of i} w h_l                          per camera i >= 1 (right-hand side of the camera system)
//      x_cam =  VT^{-1} r                                                 dense (N-1)^2, the existing dense Q*W kernel
//      x_l   =  h_l + (1/Q3_l) sum_{obs of l} w x_cam_i                   per landmark
//      Y_i   =  Q1_i W_i - c_i x_cam_i + sum_{obs of i} w p x_l           per camera, + the fused epilogue of the Q*W kernels
// i.e. O(observations) + (N-1)^2 bytes per product instead of 9 N^2: at N = 13682 cameras / 4.5 M observations 0.4 GB + 1.5 GB
// against 13.5 GB.  Single GPU in this version.  VT is assembled on the host from the co-visibility lists (O(sum of squared
// landmark degrees)) and inverted on the device at context creation (xm_dense_la.hip: blocked Cholesky + two blocked triangular
// solves, O(N^3): 2 s at N = 14 000).
#pragma once

#include <cstdint>
#include <vector>

#include "xm_solver.h"

namespace xm {

constexpr int64_t kSchurMaxCams = 40000;   // (N-1)^2 inverse + workspace = 3 x 8 N^2 bytes during set-up: 38 GB at the limit
// Dense Q built on the device from the observation list (xm_tuning_t.schur_dense_q, xm_create_matrix; xm_schur_dense.hip).  At the cap the
// padded 3N x 3N matrix is 28.8 GB, the two 3N x (N-1) work arrays (G^T and the camera rows of Abar) 9.6 GB each and VT^-1 3.2 GB: 51 GB
// while Q is built, 32 GB afterwards (+ 14.4 GB for an fp32 copy)
constexpr int64_t kSchurDenseQMaxCams = 20000;
constexpr int kSchurDenseQWinCams = 512;   // column window of the assembly kernel in cameras: 12 doubles of LDS per camera (a 3 x 3 block of B D B^T
                                           // and a 3-vector of G for each of the strip's three rows) = 48 KB per wavefront, three wavefronts on a CU's
                                           // 160 KB.  Every window walks the camera's list again; measured at 8000 cameras / 5.4 M observations:
                                           // 1024 cameras (one wavefront per CU) 113 ms, 512 cameras 66 ms
constexpr int kSchurAbarPanel = 2048;      // landmark rows of Abar are produced and copied out this many at a time (a panel of 3N doubles per landmark)
constexpr int kSchurHeavy = 64;            // landmarks with more observations get a workgroup of their own (a thread per landmark serialises
                                           // them: 963 us per product with three landmarks seen by all 1778 cameras, 122 us once split)
constexpr int kSchurAggCams = 64;          // two-level preconditioner of the CG form: cameras per aggregate (one wavefront, a lane per camera)
constexpr int64_t kSchurMaxAggregates = 4096;   // ... and its coarse operator: the n_c x n_c inverse is at most 134 MB

// Aggregates of the two-level preconditioner (host; xm_schur_aggregate_plan): the cameras 1..n-1 in the order of a breadth-first search over
// the bipartite camera-landmark graph from camera 0 (landmarks with more than kSchurHeavy observations are not expanded: they carry no
// locality), cameras it never reaches appended in index order, cut into runs of B.  order[k] = the camera at position k (aggregate k / B).
// More than kSchurMaxAggregates runs: XM_ERR_ARG.
void schur_aggregate_plan(int64_t n, int64_t nobs, const int32_t *cam, const int32_t *lm, int B, std::vector<int32_t> &order);

// A (device, column-major n x n, lower triangle read) -> Cholesky factor; X <- the LOWER triangle of A^-1 (above the diagonal: scratch).
// false: not positive definite
bool spd_inverse_device(int n, double *A, double *X, hipStream_t st, bool trace = false);   // trace: phase times on stderr
// A (device, column-major n x n, leading dimension ld, lower triangle read) -> its Cholesky factor, the launches of spd_inverse_device; *info
// (device) <- 1 when a pivot is not positive (never cleared).  No host synchronisation.
void spd_cholesky_device(int n, double *A, int64_t ld, int *info, hipStream_t st);
// X (device, n x nrhs, leading dimension ldx) <- A^-1 X from that factor by two blocked substitutions; Y: scratch of X's shape; *info <- 1
// when a solution entry is not finite.  No host synchronisation.
void spd_substitute_device(int n, const double *L, int64_t ld, double *X, double *Y, int64_t ldx, int nrhs, int *info, hipStream_t st);
// dst (row-major n x n, leading dimension ldd) <- the full symmetric inverse from X's lower triangle
void spd_inverse_layout(int n, const double *X, double *dst, int64_t ldd, hipStream_t st);
// A (device, column-major n x n) -= q * u u^T  (u: device, n doubles)
void rank1_sub_device(int n, double *A, const double *u, double q, hipStream_t st);
// C[m x n] -= opA(A)[m x k] * opB(B)[k x n] on the f64 matrix cores (la_gemm_sub_kernel; ta / tb: 1 = transposed; lower_only: the tiles on and
// below the diagonal).  Column-major, enqueued on st only.
void gemm_sub_device(int m, int n, int k, const double *A, int64_t lda, int ta, const double *B, int64_t ldb, int tb, double *C, int64_t ldc,
                     int lower_only, hipStream_t st);

struct SchurSettings {          // from xm_tuning_t (Settings::resolve)
    bool host_assembly = false; // assemble the reduced camera Laplacian on the host (the reference's route, utils/creatematrix.py:137-260; tests)
    int64_t sym_min_rows = 4096; // VT^-1 is applied with the half-traffic symmetric kernel from this many rows on
    bool trace = false;         // set-up phase times on stderr (scripts/kbench_schur.py)
    int solver = 0;             // reduced camera system inside the product: 0 by size (dense inverse up to dense_max cameras, CG above) | 1 dense inverse | 2 preconditioned CG
                                // (Jacobi) | 3 CG with the two-level preconditioner (aggregate blocks + coarse operator; xm_schur.hip)
    int64_t dense_max = 20000;  // (the dense inverse costs 8 (N-1)^2 bytes -- 3.2 GB here -- and an O(N^3) set-up; the CG form nothing but the observation lists)
    int pcg_first = 0;          // CG form: iterations of the first batch of a context's first product (0 = 26; tests force top-up batches with a small one)
    int pcg_hess_digits = 0;    // CG form: relative residual 10^-digits of the inner solve inside HESSIAN products (0 = 9; gradient, cost and certificate products: 13)
};
struct SchurLm;                 // xm_schur.hip
struct PcgArgs;
struct PcgTwoLevel;
struct PcgGrids;

// The device lists of a SchurOp, read-only, for the kernels of other files (the bundle adjustment, xm_ba.h).  By camera: the observations of
// camera i at [cam_ptr[i], cam_ptr[i+1]) with the landmark SLOT of each and its current weight.  By landmark slot: the first nheavy slots
// have contiguous lists [lm_ptr[s], lm_ptr[s+1]); the others are packed 64 to a group (observation k of the group's lane j at
// gbase[group] + 64 k + j, deg[s] of them); positions index arrays of lm_total entries, padding has weight 0.  Input order: camera, slot
// and point (nobs x 3 row-major) of observation e, and where it sits in the two lists (pos_c, dpos_l).
struct SchurLists {
    int64_t n, m, nobs, nheavy, lm_total;
    const int64_t *cam_ptr, *lm_ptr, *gbase, *pos_c, *dpos_l;
    const int32_t *cam_lm, *lm_cam, *deg, *obs_cam, *obs_lm;
    const double *cam_w, *lm_w, *obs_p;
};

class SchurOp {
public:
    // cam / lm: 0-based indices of the nobs observations, p: nobs x 3 (row-major), w: nobs
    // comm (not owned; may be null): the communicator of a row-partitioned context -- every rank holds all the observations and repeats
    // the landmark kernels, multiplies its own rows of VT^-1 only and all-gathers x_cam; the last kernel runs for the rank's cameras
    // (CamArgs.nloc / cam0)
    SchurOp(int64_t n, int64_t n_landmarks, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *p, const double *w,
            hipStream_t st, Comm *comm = nullptr, const SchurSettings &cfg = SchurSettings());
    // Y = alpha * Q * W for all n cameras (W: camera records of 3 * pitch_of(o) doubles), same CamArgs / epilogue contract and
    // per-workgroup partial sums (grid qw_grid(n)) as launch_qw_dense
    void product(int o, int epi, const double *W, double alpha, const CamArgs &a, hipStream_t st);
    // XM^2 loop on the reference's own Q: per-observation residuals at U = s.*R (input order of the observations) and new weights
    void residuals(int o, const double *U, double *res_host, const CamArgs &a, hipStream_t st);
    const double *residuals_device(int o, const double *U, const CamArgs &a, hipStream_t st);   // the same, left on the device
    void set_weights(const double *w, hipStream_t st);
    // translations t (3 x n column-major, camera 0 at the origin) and landmarks p (3 x m column-major) of a rank-3 solution given as
    // anchored rotations rot (3 x 3n column-major) and scales (n): the eliminated variables of the chain at U = (s.*R)^T, negated
    void recover_tp(const double *rot, const double *scale, double *t, double *p, hipStream_t st);
    int64_t n_landmarks() const { return m_; }
    int64_t nobs() const { return nobs_; }
    int64_t bytes_per_product(int o) const;
    // CG form of the reduced camera system: statistics since construction (products, inner iterations, products that hit the iteration cap)
    // and the relative residual of the last one
    bool uses_pcg() const { return pcg_; }
    void pcg_stats(int64_t out[3], double *relres) const { out[0] = pcg_products_; out[1] = pcg_iters_total_; out[2] = pcg_unconverged_; if (relres) *relres = pcg_last_relres_; }
    bool two_level() const { return tl_; }
    int64_t aggregates() const { return tl_nagg_; }
    SchurLists lists() const {
        return SchurLists{n_, m_, nobs_, nheavy_, ltotal_, cam_ptr_.p, lm_ptr_.p, gbase_.p, pos_c_dev_.p, dpos_l_dev_.p,
                          cam_lm_.p, lm_cam_.p, ldeg_.p, obs_cam_.p, obs_lm_.p, cam_w_.p, lm_w_.p, obs_p_.p};
    }
    const std::vector<int32_t> &slot_of() const { return slot_of_; }   // landmark -> slot
    // The dense Q of the CURRENT weights (xm_schur_dense.hip): Q (device, zero-filled padding, 3n rows of ldq doubles) <- the symmetric 3N x 3N
    // matrix in the dense kernels' layout, bit-for-bit symmetric.  abar (host, may be null): the (n-1+m) x 3n column-major matrix of
    // utils/creatematrix.py:283-311.  Needs the dense inverse of VT (not the CG form) and a list without a (camera, landmark) pair named twice.
    void build_dense_q(double *Q, int64_t ldq, double *abar, hipStream_t st);
    bool names_a_pair_twice() const { return has_dup_; }
    // The test export xm_ctx_schur_probe (include/xm_amd.h): the layout, the set-up factors as the last set_weights left them, the stages of one
    // product() of q.W and the pieces of the inner CG for q.X, the latter through the members pcg_solve() calls.  Leaves the statistics of the CG
    // form and the scratch vectors' clean padding as a product expects them.
    void probe(xm_schur_probe_t &q, hipStream_t st);

private:
    int64_t n_ = 0, m_ = 0, nobs_ = 0, nred_ = 0, ldv_ = 0;   // nred = cameras of the padded (N-1) system / 3
    Comm *comm_ = nullptr;
    int world_ = 1, rank_ = 0;
    int64_t nred_loc_ = 0, nred_pad_ = 0;                     // pseudo-cameras per rank, padded total
    DevBuf<int64_t> cam_ptr_, lm_ptr_;
    DevBuf<int32_t> cam_lm_, lm_cam_;         // by camera: landmark of each observation; by landmark: camera
    // landmarks are numbered by degree (descending) on the device; the first nheavy_ (more than kSchurHeavy observations) keep contiguous
    // lists (lm_ptr_), the others are packed 64 to a group (gbase_, ldeg_): xm_schur.hip, SchurLm
    DevBuf<int64_t> gbase_;
    DevBuf<int32_t> ldeg_;
    int64_t nheavy_ = 0, ltotal_ = 1;
    std::vector<int32_t> slot_of_;            // landmark -> device number
    std::vector<int64_t> dpos_l_;             // observation -> position in the device's by-landmark arrays
    DevBuf<double> cam_w_, cam_p_, lm_w_, lm_p_;
    DevBuf<double> Q1_, c_, q3inv_;
    DevBuf<double> vtinv_;                     // (N-1)^2 inverse in the dense kernel's padded row-major layout
    DevBuf<double> h_, r_, xc_, xl_, res_;
    SymvWork sym_work_;                        // plan and partial sums of the half-traffic product with VT^-1 (large N only)
    bool vt_sym_ = false;
    DevBuf<int32_t> obs_cam_, obs_lm_;        // the observations in input order (residual kernel)
    DevBuf<double> obs_p_;
    std::vector<int32_t> hcam_, hlm_, lcam_;  // host copies of the structure for set_weights
    std::vector<double> hp_;
    std::vector<int64_t> cp_, lp_, pos_c_, pos_l_;
    std::vector<int64_t> cam_obs_;            // observation (input index) at each position of the by-camera lists
    int o_alloc_ = 0, o_last_ = 0;
    void ensure(int o);
    // weight-dependent factors assembled on the device (set_weights_device); the host version serves lists with duplicate (camera, landmark) pairs
    DevBuf<int64_t> pos_c_dev_, dpos_l_dev_;
    DevBuf<double> w_in_, q2_;
    bool dup_pairs_ = false, has_dup_ = false;   // has_dup_: what the list says; dup_pairs_: the host path is taken (also forced by host_assembly)
    DevBuf<int32_t> slot_dev_;                   // landmark -> slot on the device (build_dense_q with abar)
    SchurSettings cfg_;
    std::vector<int64_t> hub_lm_, hub_obs_ptr_, hub_obs_;
    void set_weights_device(const double *w, hipStream_t st);
    // preconditioned CG on the matrix-free reduced camera Laplacian (cfg.solver; xm_schur.hip)
    bool pcg_ = false;
    DevBuf<double> pcg_dinv_, pcg_r_, pcg_p_, pcg_ap_, pcg_parts_;
    DevBuf<int32_t> pcg_state_;
    struct PcgState *pcg_host_ = nullptr;   // pinned copy of the device state word
    int pcg_grid_ = 1, pcg_last_iters_[2] = {24, 24}, pcg_max_iters_ = 1000;   // [0] products at the tight tolerance, [1] Hessian products
    double pcg_tol_[2] = {1e-13, 1e-9}, pcg_last_relres_ = 0.0;
    int64_t pcg_products_ = 0, pcg_iters_total_ = 0, pcg_unconverged_ = 0;
    template <int O, bool TL> void pcg_solve(const SchurLm &L, const struct TcgScal *sc, hipStream_t st, int kind);
    // the pieces of pcg_solve (the probe calls the same): arguments and grids at o columns; x = 0, r = b and z = p = M^-1 b; VT p (+ <p, VT p>
    // partial sums); z = M^-1 r with <r, z> into parity par (Jacobi: nothing to launch, the flat kernels apply the diagonal themselves)
    void pcg_setup(int o, int kind, const SchurLm &L, PcgArgs &a, PcgTwoLevel &t, PcgGrids &g);
    template <int O, bool TL> void pcg_start(const PcgArgs &a, const PcgTwoLevel &t, const PcgGrids &g, const struct TcgScal *sc, hipStream_t st);
    template <int O> void pcg_operator(const SchurLm &L, const PcgArgs &a, const PcgGrids &g, hipStream_t st);
    template <int O, bool TL> void pcg_precond(const PcgArgs &a, const PcgTwoLevel &t, const PcgGrids &g, int par, int init, hipStream_t st);
    template <int O> void probe_chain(xm_schur_probe_t &q, hipStream_t st);
    template <int O, bool TL> void probe_pcg(xm_schur_probe_t &q, const SchurLm &L, hipStream_t st);
    SchurLm lm_lists() const;
    // two-level preconditioner M^-1 r = blockdiag(VT_aa)^-1 r + P A_c^-1 P^T r (cfg.solver == 3).  Structure (fixed): the aggregates and, per
    // aggregate, its "groups" -- the observations of one landmark whose cameras fall in the aggregate, by landmark slot -- and the coarse
    // entries with their lists of group pairs (light landmarks; heavy ones are rank-1 terms).  Weight-dependent: the block inverses and A_c^-1.
    bool tl_ = false;
    int64_t tl_nagg_ = 0, tl_ngroups_ = 0, tl_nentries_ = 0;
    DevBuf<int32_t> tl_perm_;                 // position (aggregate * kSchurAggCams + row) -> reduced camera (camera - 1), -1 = padding
    DevBuf<int64_t> tl_gptr_, tl_eptr_, tl_eobs_, tl_cptr_;
    DevBuf<int32_t> tl_gslot_, tl_eloc_, tl_cab_, tl_cpair_;
    DevBuf<double> tl_u_, tl_binv_, tl_ainv_, tl_g_, tl_z_;
    DevBuf<int32_t> tl_fail_;
    std::vector<int32_t> tl_agg_of_;          // camera -> aggregate (-1: camera 0)
    void two_level_build(int64_t nobs, const int32_t *cam, const int32_t *lm);
    void two_level_set_weights(const double *w, hipStream_t st);
public:
    ~SchurOp();
    SchurOp(const SchurOp &) = delete;
    SchurOp &operator=(const SchurOp &) = delete;
};

}  // namespace xm
