/*
 * xm_amd.h — C ABI of the MI355X-native XM solver (libxm_amd.so).
 *
 * Drop-in boundary for the Burer-Monteiro / Riemannian-staircase SDP solve of
 * ComputationalRobotics/XM-code.  The reference exposes this path as three pybind11 functions
 * (XM/src/XM_main.cu:403-408):
 *      XM.solve(dataset_path, max_rank, tol, lam, max_time)           -> None   (XM_main.cu:180)
 *      XM.solve_rank3(dataset_path, max_rank, tol, lam, max_time)     -> None   (XM_main.cu:312)
 *      XM.solve_rebuttle(dataset_path, max_rank, tol, lam, max_time)  -> int    (XM_main.cu:35)
 * Section 1 below are exactly those entry points (same argument meaning, same Q.bin/R.bin/s.bin
 * files); the pybind11 module `XM` shipped in xm-code_amd/csrc/xm_pybind.cpp is a ~30-line shim
 * over them (INTEGRATION.md shows the stub).  Sections 2-4 are additive: an in-memory context API
 * (what bench.py times: Q already resident in HBM), kernel-level entry points on device pointers
 * (what the parity tests call), and the multi-GPU row-partition hooks.
 *
 * Conventions: plain pointers and sizes only, no exceptions cross the ABI, 0 == success,
 * negative == error (xm_last_error() gives the message).  All matrices float64.
 * Host-side matrices use the reference's layouts (column-major; R is 3n x r, camera i = rows
 * 3i..3i+2, XM_main.cu:231-237).  Device-side vectors use the solver's internal row-major
 * "camera-major" layout: element (row r, column k) of a 3n x o matrix at r*o + k.
 */
#ifndef XM_AMD_H
#define XM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ error codes */
#define XM_OK              0
#define XM_ERR_IO         -1   /* missing / short Q.bin etc. (reference: prints "cannot open file" and goes on, XM_main.cu:21-24) */
#define XM_ERR_ARG        -2
#define XM_ERR_HIP        -3   /* HIP runtime / no device / kernel failure */
#define XM_ERR_COMM       -4   /* RCCL failure */
#define XM_ERR_NOMEM      -5

/* status codes of the staircase (solve_rebuttle's return value, XM_main.cu:35-178) */
#define XM_STATUS_NONE          0
#define XM_STATUS_CERTIFIED     1
#define XM_STATUS_MAX_RANK      2
#define XM_STATUS_LS_FAILED    -2

const char *xm_last_error(void);
const char *xm_version(void);
/* ABI revision of the structs below.  Since revision 3 xm_problem_t, xm_options_t and xm_result_t START with `struct_size`, which the
 * caller sets to sizeof(its own struct).  The library copies min(struct_size, its own sizeof) bytes, treats what the caller did not
 * pass as zero and never writes past the caller's size, so a caller compiled against a shorter (older) header keeps working;
 * struct_size == 0 is rejected with XM_ERR_ARG (revisions 1-2 had no size field and are NOT binary compatible).  Revision 4 (this
 * one): xm_tuning_t re-laid (the fields that selected removed experiment kernels are gone, test / matrix-free switches added) -- a
 * caller that passes a NON-NULL xm_problem_t.tuning must be compiled against this header; timing hooks moved to xm_bench.h. */
#define XM_ABI_REVISION 4
int xm_abi_revision(void);

/* ================================================================== 1. file-based surface == the reference's pybind functions */
/* replaces XM_main.cu:180  solve(): reads <path>/Q.bin, writes <path>/R.bin and <path>/s.bin
 * (.bin = int32 rows, int32 cols, float64 column-major, XM_main.cu:18-33; Q.bin may instead carry the two 8-byte header
 * fields of utils/io.py:24-26, recognised by the file size) */
int xm_solve(const char *dataset_path, unsigned int max_rank, double tol, double lam, double max_time);
/* replaces XM_main.cu:312  solve_rank3() */
int xm_solve_rank3(const char *dataset_path, unsigned int max_rank, double tol, double lam, double max_time);
/* replaces XM_main.cu:35   solve_rebuttle(): also reads R_ini.bin / s_ini.bin; *status receives 1 / 2 / -2 / 0 */
int xm_solve_rebuttle(const char *dataset_path, unsigned int max_rank, double tol, double lam, double max_time,
                      int *status);

/* ================================================================== 2. in-memory context API */
typedef struct xm_ctx xm_ctx_t;

#define XM_STORAGE_DENSE 0     /* dense symmetric 3n x 3n, column-major (the reference format, XM_main.cu:18-33,191) */
#define XM_STORAGE_BSR3  1     /* 3x3-block CSR over view-graph edges, both triangles stored */
#define XM_STORAGE_BSR3_DENSE 2 /* described as BSR3 on the host (same fields), expanded to the dense layout on the device:
                                  each rank builds only its own camera rows (a >= 10k-camera Q never exists on the host) */
#define XM_STORAGE_VIEWGRAPH 4 /* the north_star workload described by its EDGE LIST: Q = sum_e w_e G_e over view-graph edges e = (i, j), Q_ii += w_e I,
                                  Q_jj += w_e I, Q_ij = -w_e M_e, Q_ji = Q_ij^T with M_e the measured relative rotation (what xm_ctx_attach_edges takes).
                                  Stored as 3x3-block CSR; with >= 2.2 M blocks per GPU (xm_tuning_t.sell) the products stream the compressed sliced-ELL copy
                                  (quaternion per off-diagonal block, one double per diagonal block: 36 B per stored block instead of 76,
                                  xm-code_amd/csrc/xm_sell.h).  The edges are attached for the XM^2 calls at creation. */
#define XM_STORAGE_SCHUR 3     /* MATRIX-FREE: Q is never formed.  The problem is the observation list the reference's
                                  utils/creatematrix.py:create_matrix(weight, edges, landmarks) takes (creatematrix.py:51); the product applies
                                  Q = Q1 - Vtp_bar Qtp_bar^{-1} Vtp_bar^T as a factor chain (xm-code_amd/csrc/xm_schur.h).  Single GPU. */

/* Context-creation settings that select kernels / layouts (all 0 = the defaults = automatic choice).  They are the ONLY way to select
 * a kernel or a layout: the library reads no environment variable for that (the variables it does read are listed in INTEGRATION.md:
 * XM_QUIET, XM_GPUS, XM_GPU_MAP, XM_RETRACTION, XM_WATCHDOG_S for callers of the file surface, which has no tuning argument, and
 * XM_COMM_PEER, XM_COMM_TRACE, XM_FORCE_COMM, XM_SHM_TIMEOUT, XM_SHM_ASYNC for the process-level communicator set-up of section 4). */
typedef struct {
    int32_t sym;               /* half-traffic symmetric dense product: 0 auto (3n >= sym_min_rows, exactly symmetric Q), 1 force (1e-9 asymmetry accepted), -1 off */
    int32_t sym_min_rows;      /* 0 = measured: 4096 on one GPU (also where the matrix-free storage starts applying its inverse with the symmetric kernel), 6144 for the multi-rank window */
    int32_t sell;              /* sliced-ELL copy of a block-sparse Q: 0 auto (by size, xm_solver.hip), 1 force, -1 off */
    int32_t sell_slabs;        /* 0 = 4 (1, 2, 4, 8) */
    int32_t sell_lmax;         /* 0 = 64 */
    int32_t sell_gather;       /* how the records of W are fetched: 0 = default (2), 1 = one record per lane, 2 = records fetched element-per-lane and
                                  transposed through LDS; anything else: XM_ERR_ARG */
    int32_t sell_codec;        /* 0 auto (view-graph storage: quaternion codec; BSR3: full blocks), 1 full blocks, 2 quaternion codec (XM_ERR_ARG if Q is not a view-graph matrix) */
    int32_t overlap;           /* split dense products outside the tCG around the all-gather of W: 0 auto (>= overlap_min_mb per rank), -1 off */
    int32_t overlap_min_mb;    /* 0 = 64; -1 = no minimum (tests) */
    int32_t cert_dense_rows;   /* certificate: complete tridiagonalisation for 3n <= this; 0 = 384 */
    int32_t lanczos_mmax;      /* 0 = 400 */
    int32_t lanczos_restarts;  /* 0 = 12 */
    int32_t watchdog_s;        /* host spin loops give up after this many seconds without progress; 0 = XM_WATCHDOG_S, else 600 */
    int32_t balance;           /* row partition of block-sparse storage: 0 = by stored blocks, 1 = equal camera ranges */
    int32_t exchange;          /* multi-GPU tCG exchange: 0 auto (direct peer writes fused into the tCG kernel when the ranks share this process or IPC
                                  is set up and the transport passes its self-test, else RCCL), 1 an all-gather between the launches (whatever the
                                  transport), 2 direct peer writes, 3 RCCL even where peer writes would work (single-process mode) */
    int32_t split_k;           /* dense product of a SMALL row strip with its columns split over several workgroups per camera group: 0 auto
                                  (multi-GPU runs whose strip has fewer than ~1.5 workgroups per CU), -1 off, 2..8 forced (also on one GPU) */
    int32_t sell_wpad;         /* sliced-ELL product inside the truncated CG (single GPU, rank 3..5): the kernels that write the product input also write
                                  a copy at a record pitch of 128 bytes, which the gather reads (one cache line per record instead of 1.4 / 1.9):
                                  0 auto (when the column pattern has no locality: random view graphs yes, banded ones no) | 1 always | -1 never */
    int32_t exchange_fence;    /* 1: the direct peer exchange publishes with plain stores + a system-scope release fence instead of write-through stores */
    int32_t schur_host_assembly; /* XM_STORAGE_SCHUR: 1 = assemble the reduced camera Laplacian on the host (the reference's route, utils/creatematrix.py:137-260) */
    int32_t schur_trace;       /* XM_STORAGE_SCHUR: 1 = set-up phase times on stderr */
    int32_t schur_solver;      /* XM_STORAGE_SCHUR: how the reduced camera Laplacian is applied inside the product: 0 auto (dense inverse up to
                                  schur_dense_max cameras, preconditioned CG above), 1 dense inverse, 2 preconditioned CG (Jacobi;
                                  xm-code_amd/csrc/xm_schur.h), 3 CG with the two-level preconditioner: exact blocks of VT on aggregates of
                                  64 cameras in breadth-first order plus the coarse operator P^T VT P (sequential captures, where Jacobi needs
                                  O(N) iterations); single GPU, at most 4096 aggregates (262 144 cameras).  Auto never picks 3. */
    int32_t schur_dense_max;   /* 0 = 20000 */
    int32_t debug_drop_finalize; /* tests: the k-th outer iteration loses its result kernel (the host must come back with XM_ERR_HIP) */
    int32_t debug_peer_mute;   /* tests: rank 1 never publishes its tCG epoch (a dead peer: the bounded waits must expire) */
    int32_t schur_pcg_first;   /* XM_STORAGE_SCHUR, CG form: iterations enqueued in the first batch of the first product (0 = 26; tests force top-up batches) */
    int32_t schur_pcg_hess_digits; /* ... relative residual 10^-d of the inner solve inside Hessian products: 0 = 9, 6 .. 13 (13 = as tight as the
                                  gradient / cost / certificate products always are) */
    int32_t hess_f32;          /* 1: the Hessian products of the truncated CG read an fp32 copy of Q (rounded to nearest, made on the device at
                                  creation; loaded as fp32, accumulated in f64).  Gradient, cost, certificate, escalation line search and Lanczos stay
                                  on the f64 Q, so the stop test and the certificate are unchanged; only the tCG steps see the rounded operator.
                                  Dense storage on one rank only (or XM_STORAGE_SCHUR with schur_dense_q = 1): any other storage, n_gpus > 1, a
                                  communicator, or an entry of Q that is not finite in fp32 gives XM_ERR_ARG.  0 (default): off */
    union {                    /* (anonymous: the slot keeps its old name reserved[0] as an alias, so callers that zero it by name still compile) */
    int32_t schur_dense_q;     /* XM_STORAGE_SCHUR: 1 = the context also builds the dense 3n x 3n Q of utils/creatematrix.py on the device from its
                                  observation lists (xm-code_amd/csrc/xm_schur_dense.hip) and EVERY product (xm_ctx_qw, the solve, the certificate)
                                  goes through the dense dispatch: the general kernel, the half-traffic symmetric sweep by the usual rule (the
                                  matrix is symmetric bit for bit), XM_FLAG_DEVICE_OUTER, and hess_f32 = 1, which is accepted together with it.
                                  The lists stay: residuals, xm_ctx_recover_tp, the XM^2 calls, cleaning and bundle adjustment work unchanged, and
                                  xm_ctx_set_edge_weights / xm_ctx_xm2_filter / xm_ctx_xm2_round rebuild Q (and the fp32 copy) on the device.
                                  XM_ERR_ARG: the CG forms (schur_solver 2 or 3), n_gpus > 1, a communicator, more than 20000 cameras (28.8 GB of Q),
                                  or a list that names a (camera, landmark) pair twice.  0 (default): off, nothing changes.  */
    int32_t reserved[1];
    };
} xm_tuning_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(xm_problem_t) of the CALLER (XM_ABI_REVISION) */
    int64_t n;                 /* cameras */
    int32_t storage;           /* XM_STORAGE_* */
    int32_t q_on_device;       /* dense only: q is a DEVICE pointer already in the solver's padded row-major layout
                                  (xm_dense_ld(n) doubles per row); the context borrows it (no copy) */
    const double *q;           /* dense: host column-major (ldq >= 3n) unless q_on_device */
    int64_t ldq;
    int64_t nb;                /* BSR3: stored blocks */
    const int64_t *rowptr;     /* n+1 */
    const int32_t *colidx;     /* nb */
    const double *blocks;      /* nb x 9, each block ROW-major (b[3*a+c] = Q[3i+a, 3j+c]) */
    /* XM_STORAGE_SCHUR: nobs observations (camera obs_cam[e], landmark obs_lm[e], both 0-based; obs_p: nobs x 3 row-major point in the
     * camera frame, already normalised with the intrinsics; obs_w: weights) -- i.e. edges - 1, landmarks, weight of create_matrix */
    int64_t nobs, n_landmarks;
    const int32_t *obs_cam, *obs_lm;
    const double *obs_p, *obs_w;
    int64_t q_row0;            /* dense host q only: q holds the rows [q_row0, q_row0 + ldq) of Q (all 3n columns, column-major,
                                  leading dimension ldq); 0 with ldq >= 3n = the whole matrix.  Lets a rank of a multi-GPU run hand
                                  over just its own row strip (xm_solve reads only that strip of Q.bin) */
    /* XM_STORAGE_VIEWGRAPH: ne edges (edge_i[e], edge_j[e]), 0-based, i != j, no unordered pair twice; edge_w: ne weights;
     * edge_M: ne x 9 row-major rotations */
    int64_t ne;
    const int32_t *edge_i, *edge_j;
    const double *edge_w, *edge_M;
    /* SINGLE-PROCESS MULTI-GPU (SURVEY.md 8b "Threading"): n_gpus > 1 row-partitions the cameras over n_gpus devices driven by one host
     * thread each inside THIS process; every xm_ctx_* call fans out to them and returns the (identical) result of rank 0.  The
     * reference's callers (1_test_solve.py:42, 3_test_colmap_glomap.py:285) stay single-process scripts.  0 / 1 = one GPU.  The file
     * surface (xm_solve...) takes the count from the environment variable XM_GPUS. */
    int32_t n_gpus;
    int32_t gpu_map;           /* 0: rank g on device g;  1: every rank on device 0 with its own stream ("virtual devices": exercises the
                                  whole multi-GPU path, peer writes included, on a 1-GPU box) */
    const xm_tuning_t *tuning; /* NULL = all defaults */
} xm_problem_t;

#define XM_MODE_SOLVE    0     /* XM_main.cu:180 */
#define XM_MODE_RANK3    1     /* XM_main.cu:312 */
#define XM_MODE_REBUTTLE 2     /* XM_main.cu:35 (s_ini honoured, R_ini overwritten by the identity stack like the reference) */

#define XM_FLAG_VERBOSE        1u   /* reference-style progress lines on stdout (trustregion.h:504, checkeig.h:317-337) */
#define XM_FLAG_FIX_STALE_SR   2u   /* recompute sR after the escalation line search (reference does not, trustregion.h:394-422) */
#define XM_FLAG_PROFILE_QW     4u   /* time every 64th tCG Q*W launch with HIP events (result.qw_*) */
#define XM_FLAG_HOST_STEPPED   8u   /* debugging: synchronise after every tCG iteration instead of run-ahead polling */
#define XM_FLAG_MODEL_RECURRENCE 32u /* the model decrease of a truncated CG from its own recurrences (m -= step <r,r> - step^2 <p,Hp> / 2) instead of from the
                                     * accumulated vectors v, Hv as the reference forms it (trustregion.h:605-610, 667-668): the tCG neither reads nor writes
                                     * Hv (2 x 24 n o bytes per iteration -- it shows from ~50 k cameras on, where cg_step is bound by its bytes).  Equal in
                                     * exact arithmetic; the last bits of the model value, hence possibly the path, differ: default OFF */
#define XM_FLAG_HOST_OUTER    64u   /* keep the outer iteration of the trust region on the HOST (the form of rounds 1-5: the host notices the end of a truncated
                                     * CG, enqueues retraction / candidate gradient / result kernel and confirms a speculatively started next tCG).  Default on
                                     * one GPU with block-CSR products -- and with dense products when XM_FLAG_DEVICE_OUTER asks for it -- (not: sliced ELL,
                                     * matrix-free, several ranks, XM_FLAG_HOST_STEPPED; with XM_FLAG_VERBOSE a stage's progress lines appear when its trust region has ended)
                                     * is the DEVICE-driven form: everything trustregion.h:527-708 does between two truncated CGs (retraction, candidate's cost /
                                     * gradient, accept / reject, radius, stop tests, start of the next tCG) is decided on the device, the host enqueues one
                                     * repeating pair of launches ahead and watches a progress word.  Same decisions from the same numbers: bit-identical
                                     * paths in block-CSR storage; the dense products alternate their sweep direction by launch pair instead of by tCG
                                     * iteration, so dense paths differ in the last bits */
#define XM_FLAG_DEVICE_OUTER 128u   /* the device-driven outer iteration also for DENSE products (one GPU), where the host-driven form is the default because
                                     * it measures 1.5-2 % faster there (the role-switching product kernels are 0.3-0.8 us dearer per launch and the host-driven
                                     * loop's round trips are hidden behind the speculative start of the next tCG: 41.7 against 42.4 us per tCG iteration on
                                     * the Venice-1778-size problem); in block-CSR storage the device-driven form is the faster one (34.7 against 35.5 us at
                                     * 13 682 cameras) and the default.  XM_FLAG_HOST_OUTER wins over this flag */
#define XM_FLAG_TCG_THREE_LAUNCH 256u /* keep the truncated CG's iteration at three launches (product sweep, per-camera sums, step) where the default is two:
                                     * on one GPU with the host-driven outer iteration and the f64 symmetric dense pair at ranks 3 and 4, the sweep of
                                     * iteration i carries the step of iteration i - 1 in its own launch and forms its product input itself.  Same bits
                                     * either way (xm_ctx_tcg_two_launch says which form a solve ran) */
#define XM_FLAG_TCG_RECOMPUTE 512u  /* recompute the truncated CG behind a rejected step.  The default, on one GPU with the host-driven outer iteration
                                     * and every storage but the matrix-free one (not: several ranks, XM_FLAG_HOST_STEPPED, XM_FLAG_HOST_OUTER, the
                                     * device-driven outer iteration), replays it: a rejection keeps the point, so the next truncated CG differs only
                                     * in its radius and repeats the rejected one's iterations bit for bit up to the one at which the smaller radius
                                     * trips.  The steps keep their direction and Hessian product (64 iterations, xm_ctx_set_tcg_history) and one launch
                                     * rebuilds the step from them, without a product.  Same bits either way (xm_ctx_tcg_replay counts the replays) */
#define XM_FLAG_WARM_R        16u   /* XM_MODE_REBUTTLE: start the rank-3 stage from opt.R_ini instead of the identity stack.  The reference
                                       reads R_ini.bin and then overwrites it with the identity (XM_main.cu:41,95-103); this flag honours it,
                                       which is what makes the second solve of the XM^2 loop cheap */

#define XM_RETRACT_QR    0     /* the reference's retraction: modified Gram-Schmidt of the 3 rows (Dense/batchedQR.h:9-69, trustregion.h:341-351) */
#define XM_RETRACT_POLAR 1     /* polar retraction R_i <- (M M^T)^{-1/2} M, M = R_i + xi_i (the orthogonal factor of the 3 x o block, via the 3x3 Gram
                                  matrix; BASELINE.json north_star names it, the reference uses it only in utils/recoversolution.py:65-86).  Same
                                  fixed points and certified optimum, different trajectory. */

typedef struct {
    uint32_t struct_size;      /* sizeof(xm_options_t) of the CALLER */
    uint32_t max_rank;
    double tol, lam, max_time;
    int32_t mode;
    uint32_t flags;
    const double *s_ini;       /* n values, XM_MODE_REBUTTLE only (may be NULL -> ones) */
    int32_t trace_cap;         /* optional per-outer-iteration trace: records of 6 doubles */
    double *trace;             /*   loss, gradnorm, inner_iters, endreason, trstatus, delta (same as the oracle) */
    const double *R_ini;       /* XM_FLAG_WARM_R only: 3n x 3 column-major starting point (rows are re-orthonormalised) */
    int32_t retraction;        /* XM_RETRACT_* */
    int32_t sum_grouping;      /* order in which the per-workgroup partial sums of the tCG / outer iteration are added: 0 ascending (default),
                                  1 descending, 2 even-then-odd.  Every grouping is fixed and bit-reproducible; they differ in the last bits, which
                                  is enough to change the iteration count at the saddle points of a staircase -- bench.py
                                  rotates through them so that the headline is not one draw of that lottery */
} xm_options_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(xm_result_t) of the CALLER */
    double *R;                 /* caller-allocated 3n x max(max_rank,3)+1, column-major, leading dim 3n */
    double *s;                 /* caller-allocated n (s[0] == 1) */
    int32_t rank;              /* columns of R that are valid (what R.bin would hold) */
    int32_t status;            /* XM_STATUS_* */
    double primal, dual, min_eig, gap;
    int64_t tcg_iters;         /* sum over outer iterations of (i+1) — the reference's "Total iteration".  A truncated CG that is replayed from the
                                  history of a rejected step (XM_FLAG_TCG_RECOMPUTE) counts the i+1 iterations it stands for, although none of them ran */
    int64_t outer_iters;
    int64_t qw_products;       /* launches of the Q*W kernel (any epilogue): a replayed truncated CG launches none, so this is smaller than with
                                  XM_FLAG_TCG_RECOMPUTE while tcg_iters is the same */
    int64_t lanczos_iters;
    double seconds;            /* wall clock of the whole solve (Q already resident) */
    double tr_seconds;         /* time inside the trust-region loops */
    double cert_seconds;       /* time inside the certificates */
    double qw_ms_sum;          /* XM_FLAG_PROFILE_QW: summed duration of the sampled Q*W launches (HIP events) */
    int64_t qw_ms_count;       /*   number of sampled launches */
    int64_t qw_bytes;          /* algorithmic bytes of ONE tCG Q*W launch at the final rank */
    int32_t trace_len;
    int32_t last_stop_reason;
    int32_t sym_product;       /* 1 when the half-traffic symmetric product was used (dense, single GPU, Q exactly symmetric) */
    int32_t cert_flags;        /* XM_CERT_* bits of the LAST certificate */
    double eig_residual;       /* Ritz residual |S x - theta x| of the last certificate's Lanczos run (reference: exact syevd, checkeig.h:303-318) */
    int32_t n_gpus;            /* ranks that took part in the solve */
    int32_t exchange;          /* multi-GPU tCG exchange used: 1 RCCL all-gather, 2 direct peer writes (0 single GPU) */
    int64_t qw_stream_bytes;   /* bytes of Q one tCG product actually streams (== the matrix part of qw_bytes unless a compressed or
                                  symmetric path is used) */
    int32_t outer_on_device;   /* trust regions (rank levels) of this solve whose outer iteration was driven by the device (0: all by the host --
                                  XM_FLAG_HOST_OUTER, dense products without XM_FLAG_DEVICE_OUTER, or a configuration the device-driven form does not
                                  cover); appended in round 6 */
    int32_t hess_f32;          /* 1 when the tCG Hessian products of the final rank read the fp32 copy of Q (xm_tuning_t.hess_f32); qw_bytes and
                                  qw_stream_bytes then count the fp32 bytes */
} xm_result_t;
#define XM_CERT_EIG_NOT_CONVERGED 1   /* Lanczos hit its iteration cap: min_eig is only an upper bound, the certificate was NOT accepted on it */
#define XM_CERT_EIG_EXACT 2           /* small problem (3n <= cert_dense_rows, default 384): the Krylov space of S was EXHAUSTED (3n steps, or an
                                       * invariant subspace was hit: beta below round-off under full re-orthogonalisation) and min_eig is the
                                       * smallest eigenvalue of the complete tridiagonal matrix -- the dense path of the reference
                                       * (Dense/eig.h:35-73 dsyevd, checkeig.h:303-318) with the reduction done matrix-free.  Set AFTER the run. */

#define XM_CERT_INEXACT_OPERATOR 4     /* matrix-free storage, CG form: an inner solve of the reduced camera system stopped at its iteration cap without
                                       * reaching the tolerance while the multipliers or the Lanczos products were formed -- S was applied inexactly and
                                       * the certificate was NOT accepted (xm_ctx_schur_info counts such products over the context's life) */

int xm_ctx_create(const xm_problem_t *prob, xm_ctx_t **out);          /* uploads / lays out Q on device 0 (or the rank's device) */
int xm_ctx_solve(xm_ctx_t *ctx, const xm_options_t *opt, xm_result_t *res);
void xm_ctx_destroy(xm_ctx_t *ctx);
/* out = alpha * Q * W through the storage the context holds (dense, BSR3 / sliced ELL, matrix-free; after a re-weighting: the
 * updated Q).  W, out: HOST, column-major 3n x o, o in 1, 3..10.  Diagnostic / test entry (single-rank contexts). */
int xm_ctx_qw(xm_ctx_t *ctx, int o, const double *W, double *out, double alpha);
int64_t xm_dense_ld(int64_t n);                                       /* padded leading dimension (doubles) of the device layout */

/* ---- XM^2 re-weighting on a resident context (reference loop 3_test_colmap_glomap.py:299-351: residual per
 * observation, 90-percentile filter at :321, rebuild Q, solve again).  For a view-graph Q = sum_e w_e G_e (Q_ii += w_e I,
 * Q_jj += w_e I, Q_ij = -w_e M_e, Q_ji = Q_ij^T) the rebuild is linear in the weights and happens on the device, in the
 * storage the context was created with (dense or BSR3, incl. its sliced-ELL copy): Q is never uploaded again.
 *   attach:    edges e = (ei[e], ej[e]), ei != ej, M: ne x 9 row-major; the stored pattern must hold both blocks of every edge and
 *              every diagonal block.  Does not change Q.
 *   residuals: res[e] = |Y_i - M_e Y_j|_F^2 with Y = s.*R of the LAST solve (the edge's share of <Q, Y Y^T> per unit weight)
 *   weights:   rewrites every edge block and every diagonal block from w: each off-diagonal entry is the one product (-w[e]) * M_e[k], each
 *              diagonal block (the f64 sum of the incident weights in edge order) * I.  w[e] = 0 removes an observation, and -0.0 IS 0
 *              everywhere: the same Q (up to the sign of a zero), the same filter.  On dense and BSR3 storage the rewrite is linear,
 *              so a negative weight is legal there; on a context whose sliced-ELL copy uses the quaternion codec (XM_STORAGE_VIEWGRAPH, or
 *              sell_codec = 2) the weight is read back as a norm, so a negative or NaN weight is XM_ERR_ARG, with Q and the context's
 *              weights unchanged.
 * XM_STORAGE_SCHUR contexts need no attach: their observations ARE the edges -- residuals: one per observation in input order,
 * |p^T U_i + t_i - P_l|^2 with the eliminated translations / landmarks of the last solution (what the reference computes from
 * recover_XM's p_est / t_est, 3_test_colmap_glomap.py:305-316); weights: one per observation (Q1, V1, Q3 and the reduced camera
 * Laplacian are rebuilt; the latter is re-inverted on the device). */
int xm_ctx_attach_edges(xm_ctx_t *ctx, int64_t ne, const int32_t *ei, const int32_t *ej, const double *M);
int xm_ctx_edge_residuals(xm_ctx_t *ctx, double *res);
int xm_ctx_set_edge_weights(xm_ctx_t *ctx, const double *w);
/* ---- the same loop with the REFERENCE's residual definition and sequencing (3_test_colmap_glomap.py:299-351).
 *   residuals_recovered: res[e] = squared distance of edge / observation e for the RECOVERED solution -- rot: 3 x 3n column-major anchored
 *              rotations and scale: n, as xm_recover_rotations returns them (the reference's R_real / s_real, :295-316).  Matrix-free
 *              contexts: |s_i R_i p + t_i - P_l|^2 with t, P eliminated (== the reference's landmarks_transformed vs p_est); view-graph
 *              contexts: |s_i R_i - M_e s_j R_j|_F^2 with R_i the camera's 3 x 3 record of the solution, the TRANSPOSE of its anchored
 *              block rot[:, 3i .. 3i+2].  Host array, input order.  Single-GPU contexts.
 *   xm2_filter: error = w .* res on the device over the LIVE edges (w != 0; an edge with w = +0.0 or -0.0 has been removed, has error +0.0
 *              and takes no part).  threshold = the value at the EXACT position h = (nlive - 1) * pct / 100 of the sorted live errors:
 *              x[floor h] + (h - floor h) (x[floor h + 1] - x[floor h]), the two order statistics found by a device radix select (:321);
 *              with h integral, or two equal neighbours, it is that order statistic bit for bit.  This is np.percentile's "linear" rule
 *              with the position computed exactly; numpy computes it as (nlive - 1) * (pct / 100) and so lands one element lower
 *              at some (nlive, pct), e.g. nlive = 91, pct = 70: 62.99999999999999 for 63 (pct = 70, 35 and 57 do this, the reference's
 *              90 and 95, 50, 10, 30, 99, 0.1, 99.9 do not).  Every live edge with error > threshold gets weight +0.0 (an error equal to
 *              the threshold stays), and Q is rebuilt (:323-338, without the reference's re-indexing of emptied landmarks / cameras:
 *              that is xm_ctx_clean_observations below, which answers for the filtered list without an upload).  The select is defined
 *              for non-negative errors: XM_ERR_ARG, with Q and the weights unchanged, for a negative or NaN current weight, pct outside
 *              [0, 100] or NaN, no live edge left, or a dense / BSR3 context before xm_ctx_set_edge_weights.
 *   xm2_round: filter at `percentile` (0 -> 90), then the reference's second pass (:339-351): solve_rank3 at lam = 0, statistics of its
 *              scales; |mean(s[1:]) - 1| > 2 std(s[1:]) or more than 10 scales < 0.1  ->  lam = kept edges / n, else lam = 0; final solve
 *              with opt->max_rank / tol / max_time / flags (XM_FLAG_WARM_R in opt->flags: start it from the rank-3 result instead of the
 *              reference's cold start).  R (3n x r column-major), s (n): the solution the round starts from (what the first solve
 *              returned).  res: the final solve's result. */
typedef struct {
    uint32_t struct_size;
    double percentile;         /* in: 0 = the reference's 90 */
    double threshold;          /* out */
    int64_t removed;           /* out: edges newly removed by this round */
    double s_avg, s_std;       /* out: mean / standard deviation of the rank-3 scales s[1:] (:343-344) */
    int64_t n_small;           /* out: scales < 0.1 */
    int32_t regularised;       /* out: 1 = the final solve ran with lam = kept / n */
    int32_t rank3_status;
    double lam_used;
    int64_t rank3_tcg_iters;
} xm_xm2_info_t;
int xm_ctx_edge_residuals_recovered(xm_ctx_t *ctx, const double *rot, const double *scale, double *res);
int xm_ctx_xm2_filter(xm_ctx_t *ctx, const double *rot, const double *scale, double percentile, double *threshold, int64_t *removed,
                      double *w_out /* optional: the new weights */);
int xm_ctx_xm2_round(xm_ctx_t *ctx, const double *R, const double *s, int r, const xm_options_t *opt, xm_xm2_info_t *info,
                     xm_result_t *res);
/* ---- Cleaning an observation list: the reference's utils/checkconnection.py:checklandmarks (run before the first create_matrix and again
 * between the XM^2 filter and the second solve, 5_test_ceres.py:482 / :578; 2_test_creatematrix.py:85-144 is the same sequence with the
 * thresholds 0 and 1) as a query on the device.  A list whose graph is not connected cannot become an XM_STORAGE_SCHUR context ("not
 * positive definite"); this call says which observations to drop and how the survivors are renumbered.
 * Input: n cameras, m landmarks, nobs observations (cam[e], lm[e]), 0-based, in input order; a weight per observation.  An observation is
 * LIVE when its weight is > 0 (w == NULL: all are live; the reference deletes filtered rows, so weight 0 means deleted there).  One pass,
 * not a fixed point; every count counts observations, a (camera, landmark) pair named twice counts twice (np.bincount):
 *   1. d1[c] = live observations of camera c.  Camera c survives when d1[c] > min_cam_obs.  first = the lowest c with the largest d1.
 *   2. among the live observations of surviving cameras d2[l] = observations of landmark l; l survives when d2[l] > min_lm_obs.
 *   3. a camera with no observation left is dropped (one that step 2 pushed to <= min_cam_obs but > 0 stays).
 *   4. of the connected components of the bipartite graph of the remaining observations (nodes: the cameras and landmarks that still have
 *      one) the one with the most nodes, cameras plus landmarks, stays; among several of that size the one that holds the earliest
 *      remaining observation in input order (max(nx.connected_components(G), key=len) for the reference's insertion order).
 * Output (host arrays): keep[nobs] (1 = the observation stays); lm_index[m] = rank of l among the kept landmarks in original order, -1 when
 * dropped; cam_index[n] = the reference's indices_all: the stage-1 index is the rank among the stage-1 survivors in original order; then
 * `first` takes index 0 and the camera that had index 0 takes first's index (not with XM_CLEAN_NO_SWAP: the reference calls the exchange
 * optional); the final index is the number of kept cameras with a smaller stage-1 index, -1 when dropped.  Nothing survives: XM_OK, every
 * index -1, keep all 0, zero counts.  min_cam_obs / min_lm_obs are literal (0 is a value, not "default"): checklandmarks is 10 and 1.
 * On the device: degrees by integer atomics, components by hooking (atomicMin on the parent's label) and pointer jumping over int32 labels
 * of the n + m vertices, a round being two launches and the host reading one word per few rounds; the labels' fixed point is unique, so
 * every output is the same on every call -- only `rounds` depends on the order in which the atomics arrive.  More than 1024 rounds:
 * XM_ERR_HIP.  n + m >= 2^31 or an index out of range: XM_ERR_ARG.
 * xm_clean_observations needs no context (creating one on a disconnected list fails): host arrays, uploaded inside the call.
 * xm_ctx_clean_observations: the list and the CURRENT weights of an XM_STORAGE_SCHUR context, so after xm_ctx_xm2_filter /
 * xm_ctx_set_edge_weights it answers for the filtered list with no upload of observations; nothing in the context changes (a solve after
 * it gives the bits of one without it).  XM_ERR_ARG (context unchanged and usable): another storage, several ranks or a communicator, a
 * struct_size that is not sizeof, negative thresholds, unknown flags, null outputs. */
#define XM_CLEAN_NO_SWAP 1u
typedef struct {
    uint32_t struct_size;
    int32_t min_cam_obs, min_lm_obs;
    uint32_t flags;            /* XM_CLEAN_NO_SWAP */
} xm_clean_options_t;
typedef struct {
    uint32_t struct_size;
    int32_t rounds;            /* hooking rounds until no label changed (the round that found nothing to change included) */
    int64_t nobs_live, n_new, m_new, nobs_new;
    int64_t components;        /* of the graph after stage 3 */
    int64_t cams_weak;         /* cameras that fail stage 1 (unobserved ones included) */
    int64_t lms_weak;          /* landmarks that fail stage 2 (unobserved ones included) */
    int64_t cams_emptied;      /* stage-1 survivors that stage 2 left without an observation */
    int64_t cams_off_component, lms_off_component;   /* nodes of the stage-3 graph outside the component that stays */
    int32_t first_camera;      /* `first` of stage 1 (-1: n = 0) */
    int32_t reserved;
} xm_clean_result_t;
int xm_clean_observations(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *w /* NULL: all live */,
                          const xm_clean_options_t *opt, uint8_t *keep, int32_t *cam_index, int32_t *lm_index, xm_clean_result_t *res);
int xm_ctx_clean_observations(xm_ctx_t *ctx, const xm_clean_options_t *opt, uint8_t *keep, int32_t *cam_index, int32_t *lm_index,
                              xm_clean_result_t *res);
/* ---- Flagging observations that disagree with pairwise relative rotations: the block the reference's last pipeline script marks "YOUR OWN
 * FILTER HERE" (5_test_ceres.py:316-431), which runs in front of checklandmarks and create_matrix, as a query on the device.
 * Input: n cameras, m landmarks, nobs observations in input order: cam[e], lm[e] 0-based, p[e] = 3 doubles, the camera-frame point; npairs
 * pairs (pi[k], pj[k], R_k), R_k a 3x3 rotation, row-major (9 doubles per pair).
 * Per pair (i, j, R), with src the points of camera i and dst those of camera j on their common landmarks, in increasing landmark order
 * (k of them):
 *   1. fewer than min_joint (20) common landmarks (or none at all): the pair is skipped.
 *   2. src_avg, dst_avg = the trimmed mean of every coordinate, `trim` = 0.05 cut from each end: scipy.stats.trim_mean, lo = int(trim * k),
 *      the mean of the sorted values [lo, k - lo).
 *   3. src_dis, dst_dis = the distances to those means.
 *   4. keep = src_dis < P(src_dis, dist_pct = 90) & dst_dis < P(dst_dis, dist_pct).  P is numpy's default percentile: position
 *      (k - 1) * (q / 100) in the sorted values, a + (b - a) t between the two neighbours, b - (b - a)(1 - t) for t >= 1/2 (numpy's _lerp).
 *      With t = 0 the threshold is an order statistic itself, bit for bit: the decision is a rank.
 *   5. src_avg, dst_avg again over the kept points.
 *   6. scale1 = the trimmed mean of |dst_n - dst_avg| over the kept points, scale2 likewise for src.
 *   7. src <- src / scale2 * scale1, all k points.
 *   8. translation = the trimmed mean, per coordinate, of dst - R src.
 *   9. err = |R src + translation - dst| / scale1.
 *  10. thr = max(mad_factor * median(err), P(err, err_pct = 95)); a point with err - thr > 0 is flagged at BOTH of its observations.
 * Output (host arrays): count[e] = the number of pairs that flagged observation e (a pair listed twice counts twice; (j, i, R^T) next to
 * (i, j, R) is a pair of its own); outlier[e] = count[e] >= min_flags (the reference: error_sum > 0, min_flags = 1).  stats (npairs entries
 * or NULL): what the pair found.  The option fields are literal (0 is a value): XM_PAIR_OPTIONS_INIT holds the reference's constants.
 * Where this differs from the reference, on purpose:
 *   (a) the reference stores ROW NUMBERS as the values of its sparse visibility matrix and tests them for truth, so observation row 0 never
 *       takes part in any pair.  Here it takes part; XM_PAIR_SKIP_ROW0 reproduces the reference.
 *   (b) a (camera, landmark) pair named twice is summed into a wrong row number by the reference's coo_matrix -> csr; here it is XM_ERR_ARG.
 *   (c) the reference computes error_angle and percentage and uses neither; percentage (the share of points with err < 0.05) is kept as a
 *       diagnostic of the pair.
 *   (d) the front end's translation of a pair is never read by the reference, so it is not an input.
 *   (e) the reference visits the pairs i < j of its pose table; here every listed pair is visited, in any order.
 * A pair with scale2 == 0, no kept point or a value that is not finite (scale1, scale2, translation, any err) flags nothing and has status
 * XM_PAIR_DEGENERATE.  XM_ERR_ARG: a pair with pi == pj, an index out of range, nobs >= 2^31, a struct_size that is not sizeof, a negative
 * option, a percentile above 100, trim >= 0.5, unknown flags, null arrays.
 * On the device: the list is indexed by camera on the host inside the call; one workgroup per pair intersects the two sorted lists, and
 * every order statistic comes from a sort in LDS, every sum from a fixed tree over the sorted range, all in f64: two calls give the same
 * bits in every output, and count does not depend on the order of the input list.  Joint sets above xm_pair_filter_limits()[0] points take
 * the same code through a global-memory workspace.  Needs no context (it runs before the list is clean enough to create one). */
#define XM_PAIR_SKIP_ROW0   1u
#define XM_PAIR_USED        0
#define XM_PAIR_TOO_FEW     1
#define XM_PAIR_DEGENERATE  2
typedef struct {
    uint32_t struct_size;
    int32_t min_joint;         /* 20 */
    int32_t min_flags;         /* 1 */
    uint32_t flags;            /* XM_PAIR_SKIP_ROW0 */
    double trim;               /* 0.05 */
    double dist_pct;           /* 90 */
    double err_pct;            /* 95 */
    double mad_factor;         /* 3 */
} xm_pair_options_t;
#define XM_PAIR_OPTIONS_INIT { (uint32_t)sizeof(xm_pair_options_t), 20, 1, 0u, 0.05, 90.0, 95.0, 3.0 }
typedef struct {
    int32_t n_joint;           /* common landmarks */
    int32_t n_kept;            /* points that pass step 4 */
    int32_t n_flagged;         /* points flagged (each at two observations) */
    int32_t status;            /* XM_PAIR_USED / XM_PAIR_TOO_FEW / XM_PAIR_DEGENERATE */
    double scale1, scale2;
    double translation[3];
    double median, p95;        /* of err (p95: at err_pct) */
    double percentage;         /* share of the points with err < 0.05 */
} xm_pair_stat_t;
typedef struct {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t pairs_used, pairs_skipped /* too few */, pairs_degenerate;
    int64_t nobs_flagged;      /* observations with outlier[e] = 1 */
    int64_t max_joint;         /* largest number of common landmarks over the listed pairs */
    int64_t pairs_on_workspace_path;
    double seconds_index;      /* host: index + upload */
    double seconds_kernels;
    double seconds_download;
} xm_pair_result_t;
int xm_pair_filter(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *p, int64_t npairs, const int32_t *pi,
                   const int32_t *pj, const double *R /* 9 per pair */, const xm_pair_options_t *opt, int32_t *count, uint8_t *outlier,
                   xm_pair_stat_t *stats /* npairs or NULL */, xm_pair_result_t *res);
/* out[0]: largest joint set that is sorted in LDS; out[1]: threads per workgroup; out[2]: workgroups of the workspace path; out[3]: largest
 * joint set of the small LDS instantiation (every pair starts there) */
int xm_pair_filter_limits(int64_t out[4]);
/* ---- The depth lift: from the front end's match table and every camera's depth and confidence map to the observation list, on the device
 * (5_test_ceres.py:191-204, the de-duplication, and :244-296, the loop over the cameras; 4_test_unidepth.py:217-262 is the same loop with
 * margin = 5).  It runs in front of xm_pair_filter, xm_clean_observations and xm_ctx_create (XM_STORAGE_SCHUR), which take its output as it
 * is.  The maps are what a depth network leaves on the GPU: with XM_LIFT_MAPS_ON_DEVICE depth[i] and conf[i] are device pointers and no
 * map travels (the reference copies every H x W map to the host to read a few thousand pixels of each).
 * Input: n cameras, m tracks, nrows rows of the match table in input order: cam[r], lm[r] 0-based, xy[r] = 2 doubles, the pixel position
 * (x, y).  Per camera i: hw[2i], hw[2i + 1] = height and width of its maps; depth[i], conf[i]: f32, row-major, pitch = width.  depth[i] ==
 * NULL: the camera has no map and yields nothing (the reference's `continue` at :253).  conf == NULL, or conf[i] == NULL: every weight (of
 * that camera) is 1.  Kinv + 9i: the INVERSE intrinsics of camera i, row-major; nothing is inverted here (the reference inverts K at :284).
 * Without XM_LIFT_MAPS_ON_DEVICE the maps are host memory: the call samples them on the host and uploads the samples only; everything
 * behind the sampling is the same device code, so the two transports give the same bits.
 *   1. Of the rows with the same (cam, lm) the earliest in input order stays (:194-198: a stable lexsort, then np.unique(...,
 *      return_index), which names the first row of every group).
 *   2. u = (int)x, v = (int)y, truncated toward zero (:261-262, astype(int)).  A row passes when margin <= u < w - margin and
 *      margin <= v < h - margin (:265).
 *   3. d = the f32 depth at (v, u), over all rows of the camera that passed 2., non-positive values included (:272).
 *   4. threshold = P(d, depth_pct = 95) (:273): numpy's default percentile IN F64 ON THE WIDENED SAMPLES -- position (k - 1) * (q / 100)
 *      in the sorted values, a + (b - a) t between the two neighbours, b - (b - a)(1 - t) for t >= 1/2 (numpy's _lerp), every product and
 *      sum rounded on its own: the rule of xm_pair_filter's step 4.
 *   5. A row survives when d > 0 && d < threshold (:275); so the largest depth of a camera never survives.
 *   6. One NaN among a camera's d leaves the camera with nothing (numpy's percentile is NaN then); threshold[i] is NaN.
 *   7. w = the f32 product c * c of the confidence at (v, u), widened to double (:281, :289: w ** 2 on a float32 array).
 *   8. p = (Kinv (u, v, 1)^T) * (double)d, the sum of every row of Kinv as (K0 u + K1 v) + K2 (:282-285).
 *   9. Output order: camera ascending, then track ascending (the order in which the reference walks its CSR rows).
 * Output (host arrays of capacity nrows; *nout entries are written): out_cam, out_lm, out_p (3 doubles), out_w, and out_row = the input
 * row every output came from (what carries the reference's rgbs, or anything else, along).  threshold (n entries or NULL): the camera's
 * percentile, NaN for a camera the reference skips (no map, no row, no row inside the border) and for 6.  The option fields are literal
 * (0 is a value); XM_LIFT_OPTIONS_INIT holds the constants of 5_test_ceres.py.
 * Where this differs from the reference, on purpose: the script hands np.percentile the float32 array, and numpy then interpolates in
 * float32 (with numpy 2.x the position as well), which depends on the numpy version.  The f64 rule above is the contract.  The two can
 * differ only where the interpolated threshold rounds onto its lower neighbour in float32: 19 samples 1.0f and one nextafter(1.0f) give
 * threshold == 1.0f in float32 and > 1 in f64, which decides the 19 rows.
 * XM_ERR_ARG: an index out of range, a pixel position that is not finite or |x|, |y| >= 2^31, nrows (n, m) >= 2^31, more than 2^30 rows of
 * one camera, a negative size or margin, a percentile outside [0, 100], h or w <= 0 with a non-null map, a struct_size that is not
 * sizeof, unknown flags, null arrays (cam, lm, xy and the outputs with nrows > 0; hw, depth, Kinv with n > 0; opt, nout, res).
 * On the device: the rows are binned by camera (a counting sort), one workgroup per camera sorts its (track, row) words and its sampled
 * depths in LDS, an exclusive scan of the cameras' survivor counts gives their offsets and one more kernel writes the list.  No atomic
 * decides an order or a value: two calls give the same bits in every output.  Cameras above xm_lift_limits()[0] rows take the same code
 * through a global-memory workspace.  Needs no context. */
#define XM_LIFT_MAPS_ON_DEVICE 1u
typedef struct {
    uint32_t struct_size;
    int32_t margin;            /* 10 */
    uint32_t flags;            /* XM_LIFT_MAPS_ON_DEVICE */
    uint32_t reserved;
    double depth_pct;          /* 95 */
} xm_lift_options_t;
#define XM_LIFT_OPTIONS_INIT { (uint32_t)sizeof(xm_lift_options_t), 10, 0u, 0u, 95.0 }
typedef struct {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t rows_duplicate;    /* rows dropped by 1. */
    int64_t rows_border;       /* ... by 2. */
    int64_t rows_depth;        /* ... by 5. or 6. */
    int64_t rows_no_map;       /* rows (after 1.) of cameras without a map; the four and *nout add up to nrows */
    int64_t cams_no_map;       /* cameras with depth[i] == NULL */
    int64_t cams_empty;        /* cameras with a map that yielded nothing */
    int64_t cams_small, cams_large, cams_workspace;   /* cameras with at least one row, by the size of the kernel that handled them */
    int64_t max_rows;          /* most rows of one camera */
    double seconds_index;      /* host: checks, sampling of host maps, upload, binning */
    double seconds_kernels;
    double seconds_download;
} xm_lift_result_t;
int xm_lift_observations(int64_t n, int64_t m, int64_t nrows, const int32_t *cam, const int32_t *lm, const double *xy, const int32_t *hw,
                         const float *const *depth, const float *const *conf /* or NULL */, const double *Kinv /* 9 per camera */,
                         const xm_lift_options_t *opt, int32_t *out_cam, int32_t *out_lm, double *out_p, double *out_w, int32_t *out_row,
                         int64_t *nout, double *threshold /* n or NULL */, xm_lift_result_t *res);
/* out[0]: most rows of a camera that are sorted in LDS; out[1]: threads per workgroup; out[2]: workgroups of the workspace path; out[3]:
 * most rows of a camera in the small LDS instantiation (every camera with that many rows or fewer runs there) */
int xm_lift_limits(int64_t out[4]);
/* ---- Feature tracks from pairwise matches, on the device: the stage that produces the match table the depth lift reads.  It stands for the
 * track establishment of the reference's fork of GLOMAP (deps/glomap/glomap/controllers/track_establishment.cc: BlindConcatenation :19-63,
 * TrackCollection :65-151, FindTracksForProblem :153-227, called from global_mapper.cc:113-156) with its modified union-find
 * (deps/glomap/glomap/math/union_find.h, which refuses to merge two sets that share an image).  NOTHING HERE WAS COMPARED WITH THE
 * REFERENCE'S COMPILED CODE (it needs COLMAP, Eigen and glog): parity rests on a line-cited sequential restatement
 * (tests/xm_tracks_numpy.py) and on the argument of rule 3.  Needs no context; host arrays in, host arrays out.
 * Input: n images; foff[n + 1], foff[0] = 0, non-decreasing: image i owns the global features foff[i] .. foff[i + 1] - 1, F = foff[n];
 * xy: 2 doubles per feature; registered[n] (NULL: every image is registered); npairs pairs pi[k], pj[k] in any order and either
 * orientation; moff[npairs + 1], moff[0] = 0, non-decreasing; f1[e], f2[e]: the feature index IN image pi[k] / pj[k] of every inlier match
 * of every valid pair (the caller applies is_valid and the inlier mask, :28-36).
 *   1. A feature takes part only if it is an endpoint of some match (union_find.h:18-25 creates a point in Find): it is "touched".  A match
 *      listed twice, in both orientations, or in a pair listed twice changes nothing.
 *   2. The connected components of the match graph over the touched features are computed.  A component's label is its smallest global
 *      feature index.
 *   3. A component is conflicted when it holds two features of one image.  A conflict-free component is a track as it is: no Union inside
 *      it is ever refused, whatever the order of the pairs, so the fork, upstream GLOMAP and plain connected components agree on it, and
 *      the check at :120-136 never fires for it.
 *   4. Conflicted components have no order-independent statement in the reference (its result depends on the hash order of the pairs);
 *      they follow `conflict`:
 *      XM_TRACKS_DROP    the component yields nothing.
 *      XM_TRACKS_GLOMAP  upstream GLOMAP, and :120-136 on the merged set: the component is discarded whole if any two of its features in
 *                        one image have sqrt(dx*dx + dy*dy) > thres_inconsistency (every product and sum rounded on its own, strictly
 *                        greater); otherwise it is kept with ALL its rows -- two rows of one image then carry one track, and
 *                        xm_lift_observations' rule 1 keeps the earlier, the smaller feature index.
 *      XM_TRACKS_SPLIT   the fork's refusal in an order that does not depend on the input: the distinct edges of the component, sorted as
 *                        (smaller id, larger id) ascending, are visited one by one; the two roots are united when their image sets are
 *                        disjoint, the larger root under the smaller.  The resulting sets are the tracks: none sees an image twice and
 *                        every label is still the set's smallest member.  ON PURPOSE this departs from the fork: the fork puts the refused
 *                        endpoint into the other endpoint's track all the same (:102-105), which :125-136 then discards or keeps with two
 *                        rows of one image.  That step is not reproduced.  The split is sequential; it runs on the host over the edges of
 *                        the conflicted components only (xm_tracks_split_host) and is timed on its own.  It is sequential only inside a
 *                        component, and a union never crosses components: with XM_TRACKS_SPLIT_DEVICE in flags every conflicted
 *                        component is split by a team of its own on the device, walking the component's distinct edges in the same
 *                        ascending order, which gives the same sets and so the same bits (see the flag).
 *   5. A track is dropped when its observation count (all images, :161, :163) is below min_views or above max_views, or when the number of
 *      distinct REGISTERED images in it (:186-197) is below min_views.
 *   6. If more than max_tracks + 1 tracks remain, the max_tracks + 1 longest stay (:219 breaks on `>`).  Ties go to the larger label; the
 *      reference's tie order is its union-find root, which is arbitrary.
 *   7. min_num_tracks_per_view >= 0 is the reference's sequential per-view greedy (:203-218).  The pipeline never sets it (-1 compared with
 *      an unsigned counter: no limit), it is not offered and there is no such field.
 *   8. Kept tracks are numbered 0 .. ntracks - 1 in ascending label (the reference's idx is hash order).
 * Output (the four row arrays have capacity F; *nout rows are written): one row per touched feature of a registered image in a kept
 * track, image ascending, then feature ascending: out_cam, out_feat (the index in the image), out_track, out_xy (the input's bits).
 * label[F] or NULL: the track of every feature, or a negative XM_TRACK_* code.  A feature of an unregistered image in a kept track carries
 * the track's number and has no row.  XM_TRACK_CONFLICT also stands for a GLOMAP discard.
 * XM_ERR_ARG, nothing written: pi[k] == pj[k], an image or feature index out of range (feature indices are checked on the device and
 * never used as an address when out of range), foff or moff not starting at 0 or decreasing, F, n, npairs or the number of matches
 * >= 2^31, thres_inconsistency negative or not finite, min_views < 1, max_views < min_views, max_tracks < 0, an unknown policy, unknown
 * flags, a struct_size that is not sizeof, null arrays where counts are positive.  n == 0 or no match: success with *nout = 0.
 * On the device: one kernel expands moff into global endpoint ids, checks them and marks the touched features; hooking and pointer
 * jumping on int32 labels (atomicMin), rounds enqueued four at a time, at most 1024 (XM_ERR_HIP beyond); one workgroup per image sorts
 * the (label, feature) words of its touched features -- equal neighbours are the conflicts; integer atomics count rows and registered
 * images per component; two prefix sums number the tracks and the rows; one kernel writes the rows.  No floating-point atomic, no atomic
 * decides an order or a value: two calls, and any permutation of pairs, matches and orientations, give the same bits. */
#define XM_TRACKS_DROP   0
#define XM_TRACKS_GLOMAP 1
#define XM_TRACKS_SPLIT  2
/* xm_tracks_options_t.flags.  XM_TRACKS_SPLIT_DEVICE: rule 4's split runs on the device; valid with conflict == XM_TRACKS_SPLIT only
 * (XM_ERR_ARG with another policy).  Opt-in: nothing chooses it automatically, and every output equals the host split's bit for bit.  The
 * edge words of the conflicted components are counted per component (integer atomicAdd), placed into one segment per component (two
 * prefix sums and an integer slot counter whose order nothing depends on) and handed to one team per component: a wavefront for at most
 * 64 endpoints and 512 listed edges, a workgroup of 256 for at most 4 096 listed edges (xm_tracks_split_limits).  The team sorts the
 * segment in LDS, drops equal neighbours, lists the distinct endpoints and walks the edges in order; every endpoint carries the smallest
 * local index of its set, so no find is needed.  A component above the workgroup's cap goes to the host splitter as before; one call may
 * use both.  No floating-point atomic, no atomic decides an order or a value, no workgroup waits on another, and the walk is bounded by
 * the cap.  Bit 0 is left undefined ON PURPOSE: flags = 1 has always been refused as an unknown flag, callers rely on that refusal, and
 * a later meaning for it would turn their error into a silent change. */
#define XM_TRACKS_SPLIT_DEVICE 2u
#define XM_TRACK_UNTOUCHED      (-1)   /* label[]: the feature is in no match */
#define XM_TRACK_SHORT          (-2)   /* fewer than min_views observations */
#define XM_TRACK_LONG           (-3)   /* more than max_views observations */
#define XM_TRACK_CONFLICT       (-4)   /* discarded by the conflict policy */
#define XM_TRACK_FEW_REGISTERED (-5)   /* fewer than min_views distinct registered images */
#define XM_TRACK_BEYOND_MAX     (-6)   /* not among the max_tracks + 1 longest */
typedef struct {
    uint32_t struct_size;
    int32_t min_views;             /* 3 */
    int32_t max_views;             /* 1000000 (5_test_ceres.py:127) */
    int32_t conflict;              /* XM_TRACKS_SPLIT */
    int64_t max_tracks;            /* 10000000 */
    double thres_inconsistency;    /* 10.0 px; XM_TRACKS_GLOMAP only */
    uint32_t flags;                /* 0, or XM_TRACKS_SPLIT_DEVICE */
    uint32_t reserved;
} xm_tracks_options_t;
#define XM_TRACKS_OPTIONS_INIT { (uint32_t)sizeof(xm_tracks_options_t), 3, 1000000, XM_TRACKS_SPLIT, 10000000, 10.0, 0u, 0u }
typedef struct {
    uint32_t struct_size;
    int32_t rounds;                /* hooking rounds until the labels stood still */
    int64_t ntracks;               /* kept tracks */
    int64_t features_touched;
    int64_t matches;               /* matches listed (duplicates included) */
    int64_t components, components_conflicted;
    int64_t rows_conflicted;       /* touched features in conflicted components */
    int64_t tracks_short, tracks_long, tracks_conflict, tracks_few_registered, tracks_beyond_max;   /* by the first rule that dropped them */
    int64_t images_small, images_large, images_workspace;   /* images with a touched feature, by the size of the kernel that sorted them */
    int64_t max_touched;           /* most touched features of one image */
    int64_t edges_split;           /* XM_TRACKS_SPLIT: DISTINCT edges of the conflicted components, whether the host or the device split them */
    int64_t unions_refused;        /* ... of which the split refused */
    double seconds_index;          /* host: checks and upload */
    double seconds_kernels;        /* without seconds_split */
    double seconds_split;          /* XM_TRACKS_SPLIT: download of the conflicted edges, the host split, upload of the new labels; with
                                      XM_TRACKS_SPLIT_DEVICE: from the first launch of the split until the labels are final, the host's
                                      part for components above the cap included */
    double seconds_download;
} xm_tracks_result_t;
int xm_build_tracks(int64_t n, const int64_t *foff, const double *xy, const uint8_t *registered /* n or NULL */, int64_t npairs, const int32_t *pi,
                    const int32_t *pj, const int64_t *moff, const int32_t *f1, const int32_t *f2, const xm_tracks_options_t *opt, int32_t *out_cam,
                    int32_t *out_feat, int32_t *out_track, double *out_xy, int64_t *nout, int32_t *label /* F or NULL */, xm_tracks_result_t *res);
/* out[0]: most touched features of an image that are sorted in LDS; out[1]: threads per workgroup; out[2]: workgroups of the workspace
 * path; out[3]: most touched features of an image in the small LDS instantiation */
int xm_tracks_limits(int64_t out[4]);
/* Test export: rule 4's XM_TRACKS_SPLIT on the host, as xm_build_tracks runs it.  nedges edges eu[e], ev[e] (global feature indices, any
 * order, duplicates allowed); label[F]: the smallest member of the set of every feature that is an endpoint, -1 for the others.  distinct,
 * refused (or NULL): the distinct edges and the unions refused.  Needs no device. */
int xm_tracks_split_host(int64_t n, const int64_t *foff, int64_t nedges, const int32_t *eu, const int32_t *ev, int32_t *label, int64_t *distinct,
                         int64_t *refused);
/* Test export: the same on the device, with the split code xm_build_tracks runs under XM_TRACKS_SPLIT_DEVICE.  Arguments, checks and
 * outputs as xm_tracks_split_host.  The components of the given edges are labelled on the device and every one is treated as one to
 * split (nothing is ever refused inside a conflict-free one).  An index out of range: XM_ERR_ARG, nothing written.  No edge needs no device. */
int xm_tracks_split_device(int64_t n, const int64_t *foff, int64_t nedges, const int32_t *eu, const int32_t *ev, int32_t *label, int64_t *distinct,
                           int64_t *refused);
/* The forms of the device split; needs no device.  out[0]: most endpoints of a component in the wavefront form; out[1]: most raw (listed)
 * edges of a component in the wavefront form; out[2]: most raw edges of a component in the workgroup form (above: the host splitter);
 * out[3]: threads per workgroup.  A form that is not built reports 0. */
int xm_tracks_split_limits(int64_t out[4]);
/* What the calling thread's most recent xm_build_tracks or xm_tracks_split_device did (thread-local as xm_last_error, zeroed when either
 * call starts; needs no device).  out[0], out[1], out[2]: components split in the wavefront form, in the workgroup form, on the host;
 * out[3], out[4]: raw edges given to the device forms, to the host; out[5]: distinct edges; out[6]: unions refused; out[7]: 0.  All 0
 * without XM_TRACKS_SPLIT_DEVICE. */
int xm_tracks_split_stats(int64_t out[8]);
/* ---- Two-view match verification and view-graph pruning, on the device: the stage that produces what xm_build_tracks reads (the inlier
 * matches of the valid pairs, and `registered`) and the pair list xm_pair_filter reads.  It stands for the block in front of track
 * establishment in the reference's fork of GLOMAP, deps/glomap/glomap/controllers/global_mapper.cc:56-111: ImagePairsInlierCount
 * (processors/image_pair_inliers.cc), FilterInlierNum / FilterInlierRatio / FilterRotations (processors/relpose_filter.cc),
 * KeepLargestConnectedComponents (scene/view_graph.cc:9-46).  NOTHING HERE WAS COMPARED WITH THE REFERENCE'S COMPILED CODE (it needs
 * COLMAP, Eigen and glog): parity rests on a line-cited sequential restatement in plain Python loops (tests/xm_viewgraph_numpy.py,
 * restatement (a)) which the vectorised contract (run_numpy, restatement (b)) equals exactly.  Needs no context; host arrays in, host
 * arrays out.  A pipeline calls it twice: pass A (XM_VG_SCORE, rot = NULL) scores, applies the number and ratio rules and prunes; pass B
 * (no flag, rot given, fed with pass A's compacted matches, its pair validity and its registered_out) applies the rotation rule after a
 * view-graph solve and prunes again.  Pass B's f1_out / f2_out / moff_out and registered_out go into xm_build_tracks as they are.
 * Input: n images; foff[n + 1] and xy (2 doubles per feature, pixels) as xm_build_tracks; focal[n]; Kinv: 9 per image, row-major (nothing
 * is inverted here); bearing: 3 doubles per feature or NULL -- if given it replaces rule 0 (cameras with distortion); npairs pairs pi, pj;
 * model[npairs]: XM_VG_MODEL_*, the caller maps COLMAP's configuration (image_pair_inliers.cc:7-18: CALIBRATED -> E, UNCALIBRATED -> F,
 * PLANAR / PANORAMIC / PLANAR_OR_PANORAMIC -> H, anything else -> NONE); Rrel: 9 per pair, row-major, the rotation of cam2_from_cam1;
 * trel: 3 per pair, used as given (GLOMAP keeps it at unit length); FH: 9 per pair, row-major, F of an F pair and H of an H pair (NULL only
 * if no pair is F or H); valid_in[npairs] or NULL (all valid); registered_in[n] or NULL (all registered); rot: 9 per image, row-major,
 * cam_from_world, or NULL (rule 6 is off); moff[npairs + 1], f1, f2 as xm_build_tracks.
 * Every product and every sum is rounded on its own (no fused multiply-add); a sum of three runs left to right, dot(a, b) =
 * (a0*b0 + a1*b1) + a2*b2; division and square root are IEEE.  A NaN makes every comparison false.
 *   0. Bearing (image_undistorter.cc:33-36; only without `bearing`, only E pairs read it): h_r = (K_r0*x + K_r1*y) + K_r2 over the rows of
 *      Kinv, b = h / sqrt((h0*h0 + h1*h1) + h2*h2), component by component.
 *   1. With XM_VG_SCORE a pair that is invalid at input gets no inliers and is not scored (image_pair_inliers.cc:205-212); a NONE pair
 *      gets none (:17).  Without the flag every listed match of a valid pair is an inlier, and a pair invalid at input has none.
 *   2. E pairs (:20-92).  E = [t]x R (two_view_geometry.cc:41-45): E_0c = t1*R_2c - t2*R_1c, E_1c = t2*R_0c - t0*R_2c, E_2c = t0*R_1c -
 *      t1*R_0c.  thr = (max_epipolar_error_E*0.5)*(1/focal_i + 1/focal_j), sq = thr*thr.  Sampson error (:71-83): Ex1_r = dot(E_r, x1) /
 *      (XM_VG_EPS + x1_2), Etx2_r = dot(E column r, x2) / (XM_VG_EPS + x2_2), C = dot(Ex1, x2), r2 = (C*C) / ((Ex1_0*Ex1_0 + Ex1_1*Ex1_1) +
 *      (Etx2_0*Etx2_0 + Etx2_1*Etx2_1)).  CheckCheirality (:5-29): Rx1_r = dot(R_r, x1), a = -dot(Rx1, x2), b1 = -dot(Rx1, t), b2 =
 *      dot(x2, t), l1 = b1 - a*b2, l2 = (-a)*b1 + b2, f = 1 - a*a; it holds when l1 and l2 are > XM_VG_MIN_DEPTH*f and < XM_VG_MAX_DEPTH*f.
 *      e12 = t, e21_r = -dot(R column r, t), each negated when its z is negative (:26-31).  A match is an inlier when r2 < sq, the
 *      cheirality holds, dot(x1, R^T x2) < XM_VG_COS_PARALLEL with (R^T x2)_r = dot(R column r, x2), dot(x1, e21) < XM_VG_COS_EPIPOLE and
 *      dot(x2, e12) < XM_VG_COS_EPIPOLE.  The reference rotates by the pose's quaternion; here the rotation is the matrix Rrel.
 *   3. F pairs (:94-164), on the pixels.  The epipole is F.row(0) x F.row(2) with cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 -
 *      a1*b0); if no component is > XM_VG_EPS or < -XM_VG_EPS it is F.row(1) x F.row(2).  Fx1_r = (F_r0*x1 + F_r1*y1) + F_r2, Ftx2_r =
 *      (F_0r*x2 + F_1r*y2) + F_2r, C = (Fx1_0*x2 + Fx1_1*y2) + Fx1_2, r2 = (C*C) / ((Fx1_0^2 + Fx1_1^2) + (Ftx2_0^2 + Ftx2_1^2)) (:57-69);
 *      pre-inliers have r2 < maxF*maxF.  Signum (:32-39): ((F_00*x2 + F_10*y2) + F_20) * (ep_1 - ep_2*y1), positive when > 0.  Equal
 *      positive and negative counts over the pre-inliers (zero included): no inliers.  Otherwise the pre-inliers of the majority side.
 *   4. H pairs (:166-198): Hx_r = (H_r0*x1 + H_r1*y1) + H_r2, d = XM_VG_EPS + Hx_2, u = Hx_0/d - x2, v = Hx_1/d - y2, u*u + v*v < maxH*maxH.
 *   5. With XM_VG_SCORE (relpose_filter.cc:35-65): a valid pair with inliers < min_inlier_num becomes invalid (XM_VG_FEW_INLIERS); then a
 *      valid pair with inliers / (double)matches < min_inlier_ratio becomes invalid (XM_VG_LOW_RATIO).  No matches: NaN, false, as there.
 *   6. With rot (relpose_filter.cc:7-33, rigid3d.cc:7-15), for valid pairs with both images in registered_in: M_ab = dot(rot_j row a,
 *      rot_i row b); s = the sum of M_ab*Rrel_ab in row-major order, starting from the first product; c = (s - 1)/2, set to 1 when > 1 and
 *      to -1 when < -1; the pair becomes invalid (XM_VG_ROTATION) when c < cos_max_rotation_error.  ON PURPOSE the test is on the cosine and
 *      from matrices: the reference takes acos of a quaternion product and compares degrees; the two differ only within the rounding of acos
 *      at the boundary.
 *   7. Largest component (view_graph.cc:9-46): the connected components of the images over the valid pairs; an image without a valid pair
 *      forms none.  The largest wins, ties go to the component with the smallest image index (the reference's tie is hash order).
 *      registered_out is membership in it; every valid pair with an unregistered end becomes invalid (XM_VG_OUTSIDE).  With no valid pair
 *      the call succeeds with nothing registered and largest = 0 (the reference gives up there).
 *   8. Output: inlier[e] (rules 1-4); pair_inliers[k]; pair_status[k], the first rule that dropped the pair; registered_out[n]; moff_out
 *      [npairs + 1], f1_out, f2_out (capacity: the input's matches): the inliers of the pairs still valid, in input order.
 * XM_ERR_ARG, nothing written, everything but the feature indices checked on the host before any device call: an image or feature index
 * out of range (feature indices are checked on the device and never used as an address when out of range), pi[k] == pj[k], foff or moff
 * not starting at 0 or decreasing, n, npairs, features or matches >= 2^31, an unknown model or flag, an F or H pair with FH == NULL, an E
 * pair that is scored with neither Kinv nor bearing (or without focal), a negative or non-finite threshold, a negative min_inlier_num, a
 * struct_size that is not sizeof, a null array where its count is positive.
 * On the device: one kernel computes the bearings of the images E pairs touch; the scoring holds a pair's geometry in registers and
 * streams its matches through a wavefront (pairs up to xm_view_graph_limits()[2] matches), a workgroup (up to [0]) or, above, workgroups
 * over chunks of [0] matches whose counts meet in a workspace -- the F majority is known before the second sweep in every form; one
 * kernel applies rules 5 and 6; hooking and pointer jumping on int32 image labels, rounds enqueued four at a time, at most 1024
 * (XM_ERR_HIP beyond); integer atomics count the component sizes, one reduction takes the arg-max; a three-launch exclusive scan gives
 * moff_out and one kernel writes the kept inliers through ballot prefixes.  No floating-point atomic, no atomic decides an order or a
 * value: two calls give the same bits, and a permutation of the pairs permutes the per-pair outputs. */
#define XM_VG_SCORE 1u                 /* flags: score the matches and apply rule 5 (pass A) */
#define XM_VG_MODEL_NONE 0
#define XM_VG_MODEL_E    1
#define XM_VG_MODEL_F    2
#define XM_VG_MODEL_H    3
#define XM_VG_VALID       0            /* pair_status[] */
#define XM_VG_INVALID_IN  1
#define XM_VG_FEW_INLIERS 2
#define XM_VG_LOW_RATIO   3
#define XM_VG_ROTATION    4
#define XM_VG_OUTSIDE     5
/* the constants the reference hard-codes, as 17-digit literals */
#define XM_VG_EPS          9.9999999999999998e-13   /* glomap/types.h: EPS = 1e-12 */
#define XM_VG_MIN_DEPTH    1.0000000000000000e-02   /* image_pair_inliers.cc:65 */
#define XM_VG_MAX_DEPTH    1.0000000000000000e+02
#define XM_VG_COS_EPIPOLE  9.9863053475457386e-01   /* cos(3 deg) + 1e-6 (:54, :57) */
#define XM_VG_COS_PARALLEL 1.0000009999999999e+00   /* 1 + 1e-6 (:55-56) */
#define XM_VG_COS_10DEG    9.8480775301220802e-01   /* the default of cos_max_rotation_error: max_rotation_error = 10 degrees */
typedef struct {
    uint32_t struct_size;
    uint32_t flags;                    /* XM_VG_SCORE */
    double max_epipolar_error_E;       /* 1 (glomap/types.h:18-33) */
    double max_epipolar_error_F;       /* 4 */
    double max_epipolar_error_H;       /* 4 */
    int32_t min_inlier_num;            /* 30 */
    int32_t reserved;
    double min_inlier_ratio;           /* 0.25 */
    double cos_max_rotation_error;     /* XM_VG_COS_10DEG */
} xm_vg_options_t;
#define XM_VG_OPTIONS_INIT { (uint32_t)sizeof(xm_vg_options_t), XM_VG_SCORE, 1.0, 4.0, 4.0, 30, 0, 0.25, XM_VG_COS_10DEG }
typedef struct {
    uint32_t struct_size;
    int32_t rounds;                    /* hooking rounds until the labels stood still */
    int64_t matches;                   /* matches listed */
    int64_t inliers;                   /* ... that are inliers (rules 1-4) */
    int64_t matches_out;               /* ... that are written to f1_out / f2_out */
    int64_t pairs_valid, pairs_invalid_in, pairs_few_inliers, pairs_low_ratio, pairs_rotation, pairs_outside;   /* by pair_status */
    int64_t pairs_none, pairs_E, pairs_F, pairs_H;   /* listed pairs by model */
    int64_t largest;                   /* images in the largest component */
    int64_t components;
    int64_t pairs_wave, pairs_group, pairs_workspace;   /* pairs with a match, by the form of the kernels that ran them */
    int64_t max_matches;               /* most matches of one pair */
    double seconds_index;              /* host: checks and upload */
    double seconds_kernels;
    double seconds_download;
} xm_vg_result_t;
int xm_view_graph_filter(int64_t n, const int64_t *foff, const double *xy, const double *focal, const double *Kinv,
                         const double *bearing /* 3 per feature or NULL */, int64_t npairs, const int32_t *pi, const int32_t *pj,
                         const int32_t *model, const double *Rrel, const double *trel, const double *FH, const uint8_t *valid_in /* or NULL */,
                         const uint8_t *registered_in /* or NULL */, const double *rot /* 9 per image or NULL */, const int64_t *moff,
                         const int32_t *f1, const int32_t *f2, const xm_vg_options_t *opt, uint8_t *inlier, int32_t *pair_inliers,
                         int32_t *pair_status, uint8_t *registered_out, int64_t *moff_out, int32_t *f1_out, int32_t *f2_out, xm_vg_result_t *res);
/* out[0]: most matches of a pair that one workgroup runs (and the chunk of the workspace form above it); out[1]: threads per workgroup;
 * out[2]: most matches of a pair that one wavefront runs; out[3]: most hooking rounds */
int xm_view_graph_limits(int64_t out[4]);
/* Focal lengths from the view graph on the device: step 1 of the reference's fork of GLOMAP (controllers/global_mapper.cc:37-46:
 * ViewGraphCalibrator::Solve, estimators/view_graph_calibration.cc, estimators/cost_function.h:44-222), a robust least-squares fit of one
 * focal length per camera to the pairs' fundamental matrices (Fetzer's cost, Cauchy loss), the rejection of wild estimates and the
 * invalidation of the pairs that still disagree; with XM_VGC_UPDATE_CONFIG also step 0 in front of it
 * (processors/view_graph_manipulation.cc:170-231).  Context-free like xm_view_graph_filter: host arrays in, host arrays out.  Its
 * focal_out[cam_of_image[.]] and pair_status == XM_VGC_VALID are what xm_view_graph_filter takes as focal and valid_in.
 *
 * Cameras: focal0[ncams] the prior (Camera::Focal()), pp[2 ncams] the principal point, has_prior[ncams]: a camera with a prior is held
 * constant (view_graph_calibration.cc:113-117).  Images: cam_of_image[n].  Pairs: pi, pj (image indices, image_id1 and image_id2),
 * model[npairs] (XM_VG_MODEL_*), F[9 npairs] row-major (image_pair.F for E and F pairs alike), valid_in[npairs] or NULL, and with
 * XM_VGC_UPDATE_CONFIG Rrel[9 npairs], trel[3 npairs] (cam2_from_cam1).  Only valid pairs of model E or F take part (:72-79).
 *
 * Rules:
 *   1. Set-up, once per participating pair (cost_function.h:47-122): G = K1^T F K0 with K = [[1,0,px],[0,1,py],[0,0,1]], K0 of image_id1's
 *      camera and K1 of image_id2's, every entry as (a*b + c*d) + e; the SVD of G with singular values descending (here a one-sided Jacobi
 *      SVD in f64, at most xm_view_graph_calibrate_limits()[2] sweeps); ai, aj, bi, bj as there; d_01 = fetzer_d(., 1, 0) and d_12 =
 *      fetzer_d(., 2, 1), eight doubles per pair (d_02 is computed by the reference and never read; it is not stored).  A joint sign flip of
 *      (u_0, v_0) or of (u_1, v_1) flips all of d_01 and all of d_12 and leaves every residual unchanged: d is defined up to that sign.
 *   2. Residual at (fi, fj), fi the focal of image_id1's camera (:132-152, :189-212): fi2 = fi*fi, fj2 = fj*fj, di = fj2*d_01[0] + d_01[1],
 *      dj = fi2*d_12[0] + d_12[2], each replaced by 1e-6 when exactly 0; n0 = fj2*d_01[2] + d_01[3], n1 = fi2*d_12[1] + d_12[3], K0 =
 *      -(n0/di), K1 = -(n1/dj), r = ((fi2 - K0)/fi2, (fj2 - K1)/fj2).  Every product and sum is rounded on its own (no fused multiply-add),
 *      so with the same d and focals the residuals and the flags of rule 6 equal the numpy contract's bit for bit.  When both images have
 *      one camera, fi = fj is one unknown (:89-94, :160-222).  The Jacobian is analytic where Ceres differentiates automatically (a
 *      departure in rounding only); for a same-camera pair it is the sum of the two partials.
 *   3. Loss: Ceres's CauchyLoss with scale thres_loss_function and Ceres's corrector, as xm_ctx_bundle_adjust applies XM_BA_LOSS_CAUCHY.
 *   4. Minimiser: the Levenberg-Marquardt rules of xm_ctx_bundle_adjust (initial radius 1e4, step acceptance above 1e-3, Ceres's radius
 *      update, the damping mu * clamp(diag(J^T J), 1e-6, 1e32)), function_tolerance as given, gradient tolerance 1e-10 and parameter
 *      tolerance 1e-8 (Ceres's defaults).  Unknowns: one scalar per camera that takes part and has no prior.
 *   5. Early return (:32-35): with no free camera the call succeeds and refines nothing and invalidates nothing.
 *   6. Results (:123-186): a free camera that takes part is rejected when f_est/focal0 > thres_higher_ratio or < thres_lower_ratio:
 *      focal_out = focal0, refined = 0, XM_VGC_CAM_REJECTED; otherwise focal_out = f_est, refined = 1.  Cameras in no participating pair
 *      are untouched.  residual[2 npairs] is evaluated without the loss at the OPTIMISED focals, those of rejected cameras included
 *      (problem_->Evaluate reads focals_, not the cameras); a participating pair becomes XM_VGC_TWO_VIEW_ERROR when r0*r0 + r1*r1 >
 *      thres_two_view_error * thres_two_view_error.
 *   7. With XM_VGC_UPDATE_CONFIG, before rule 1: per camera, over the valid pairs whose two cameras both have a prior, total counts E and F
 *      pairs and calibrated the E pairs; a camera is "valid" when calibrated/total > 0.5; a valid F pair whose two cameras are both valid
 *      becomes E (model_out) and its F is rewritten (F_out) as K2^-T [t]x R K1^-1 (math/two_view_geometry.cc:41-55): E row 0 = t1*R2. -
 *      t2*R1., row 1 = t2*R0. - t0*R2., row 2 = t0*R1. - t1*R0.; with a = 1/f, x = -px/f, y = -py/f of each camera (the inverse of a pinhole K
 *      in closed form, f = focal0), A = K2^-T E: rows a2*E0., a2*E1., (x2*E0. + y2*E1.) + E2.; F columns A.0*a1, A.1*a1, (A.0*x1 + A.1*y1) +
 *      A.2.  Every operation rounded on its own: exact against the contract.
 *
 * Departures from the reference, all listed in DESIGN.md 2.21: a camera has ONE focal length (the reference writes the estimate into both
 * of FocalLengthIdxs(); a camera with fx != fy is represented by its mean); the normal equations are solved matrix-free by
 * Jacobi-preconditioned CG on the device (relative residual 1e-12 or xm_view_graph_calibrate_limits()[3] iterations) where Ceres
 * factorises them; the bound f >= lower_bound is kept by projecting the candidate, without Ceres's line search; the Jacobian is analytic;
 * the SVD is a one-sided Jacobi SVD.  Nothing here is compared with the reference's compiled code (it needs Ceres, COLMAP, Eigen and
 * glog): tests/xm_vgcalib_numpy.py restates the C++ line by line and the device is tested against that.
 *
 * XM_ERR_ARG, nothing written, everything checked on the host before any device call: an index out of range, pi == pj, an unknown model
 * or flag, a non-finite F entry of a participating pair, a non-positive or non-finite focal0 or option, thres_lower_ratio >
 * thres_higher_ratio, XM_VGC_UPDATE_CONFIG without Rrel / trel, a wrong struct_size, a null array where its count is positive, counts >= 2^31.
 * No floating-point atomic and no atomic at all: two calls give the same bytes. */
#define XM_VGC_UPDATE_CONFIG 1u         /* flags: rule 7 */
#define XM_VGC_VALID          0         /* pair_status[]: valid at input and not invalidated (whether or not it took part) */
#define XM_VGC_INVALID_IN     1
#define XM_VGC_TWO_VIEW_ERROR 2
#define XM_VGC_CAM_UNUSED   0           /* cam_status[]: in no participating pair */
#define XM_VGC_CAM_CONSTANT 1           /* takes part and has a prior (or nothing was optimised: rule 5) */
#define XM_VGC_CAM_REFINED  2
#define XM_VGC_CAM_REJECTED 3
typedef struct {
    uint32_t struct_size;
    uint32_t flags;                    /* XM_VGC_UPDATE_CONFIG */
    double thres_loss_function;        /* 1e-2 (view_graph_calibration.h:21-23) */
    double thres_lower_ratio;          /* 0.1 */
    double thres_higher_ratio;         /* 10 */
    double thres_two_view_error;       /* 2 */
    int32_t max_num_iterations;        /* 100 (optimization_base.h:21-26) */
    int32_t reserved;
    double function_tolerance;         /* 1e-5 */
    double lower_bound;                /* 1e-3 (view_graph_calibration.cc:113) */
} xm_vgc_options_t;
#define XM_VGC_OPTIONS_INIT { (uint32_t)sizeof(xm_vgc_options_t), 0u, 1e-2, 0.1, 10.0, 2.0, 100, 0, 1e-5, 1e-3 }
typedef struct {
    uint32_t struct_size;
    int32_t stop_reason;               /* XM_BA_* (XM_BA_NO_CONVERGENCE when nothing was optimised) */
    int64_t pairs;                     /* participating pairs */
    int64_t pairs_same_camera;
    int64_t cams_free, cams_constant, cams_rejected;
    int64_t pairs_invalidated;
    int64_t pairs_flipped;             /* rule 7 */
    int64_t cams_heavy;                /* free cameras above xm_view_graph_calibrate_limits()[0] incidences */
    int64_t max_incidences;
    int64_t pcg_iterations;            /* in total */
    int32_t iterations, accepted;      /* Levenberg-Marquardt */
    int32_t trace_len, reserved;       /* entries written to cost_trace: the cost at the start and after every accepted step */
    double initial_cost, final_cost;
    double seconds_index;              /* host: lists and upload */
    double seconds_kernels;
    double seconds_download;
} xm_vgc_result_t;
int xm_view_graph_calibrate(int64_t ncams, const double *focal0, const double *pp, const uint8_t *has_prior, int64_t n,
                            const int32_t *cam_of_image, int64_t npairs, const int32_t *pi, const int32_t *pj, const int32_t *model,
                            const double *F, const uint8_t *valid_in /* or NULL */, const double *Rrel /* or NULL */,
                            const double *trel /* or NULL */, const xm_vgc_options_t *opt, double *focal_out, double *focal_est,
                            uint8_t *refined, int32_t *cam_status, int32_t *pair_status, double *residual, double *d_out /* 8 per pair or NULL */,
                            int32_t *model_out /* or NULL */, double *F_out /* or NULL */,
                            double *cost_trace /* max_num_iterations + 1 or NULL */, xm_vgc_result_t *res);
/* Test export (like xm_ctx_gp_probe): set-up, evaluation, the camera kernel and one product (J^T J + mu clamp(diag)) x, with the kernels,
 * grids and arguments of the call, at the caller's focal[ncams] and x[ncams] (entries of cameras that are not free are ignored).  d_in
 * (8 per pair, or NULL) replaces the set-up's result.  Every output whose pointer is not null is filled: d (8 per pair: d_01, d_12),
 * residual (2 per pair, without the loss), record (6 per pair, corrector-scaled: r0, r1, dr0/dfi, dr0/dfj, dr1/dfi, dr1/dfj; a
 * same-camera pair holds the summed partials in entries 2 and 4), cost (one double), gradient, diagonal and product per camera.  Pairs
 * that take no part and cameras that are not free hold 0. */
typedef struct {
    uint32_t struct_size;
    uint32_t reserved;
    const double *focal, *x, *d_in;
    double mu;
    double *d, *residual, *record, *cost, *gradient, *diagonal, *product;
} xm_vgc_probe_t;
int xm_view_graph_calibrate_probe(int64_t ncams, const double *focal0, const double *pp, const uint8_t *has_prior, int64_t n,
                                  const int32_t *cam_of_image, int64_t npairs, const int32_t *pi, const int32_t *pj, const int32_t *model,
                                  const double *F, const uint8_t *valid_in, const xm_vgc_options_t *opt, xm_vgc_probe_t *probe);
/* out[0]: most incidences of a camera that one thread walks (a camera above it gets a workgroup); out[1]: threads per workgroup;
 * out[2]: most sweeps of the Jacobi SVD; out[3]: most PCG iterations of one solve */
int xm_view_graph_calibrate_limits(int64_t out[4]);
/* Robust rotation averaging over the view graph on the device: the IRLS stage of step 3 of the reference's fork of GLOMAP
 * (controllers/global_mapper.cc:76-111: RotationEstimator::EstimateRotations, estimators/global_rotation_averaging.cc, math/rigid3d.cc
 * :41-71) with the reference's own options skip_initialization = true and max_num_l1_iterations = 0: iteratively re-weighted least squares
 * on the tangent space from rotations the caller supplies (those of a view-graph solve), so that a pair with a wrong relative rotation
 * ends with a vanishing weight before xm_view_graph_filter's rotation test.  Context-free like xm_view_graph_filter and in its
 * conventions, so nothing is transposed between the calls: registered[n] or NULL (all), rot0[9n] cam_from_world row-major (the start),
 * pi, pj (image_id1, image_id2), Rrel[9 npairs] cam2_from_cam1 row-major, valid_in[npairs] or NULL.
 *
 * Rules (lines of global_rotation_averaging.cc unless a file is named):
 *   1. Participation: a pair takes part when it is valid and both ends are registered (:163-164).  The fixed camera is fixed_image; with
 *      -1 the smallest registered index (a departure: :150-156 takes the first entry in hash order).
 *   2. State: one angle-axis vector per registered image (rotation_estimated_), Log of rot0 by rule 4, kept as angle-axis across the
 *      iterations as the reference does (:143-144, :425-430).
 *   3. AngleAxisToRotation (rigid3d.cc:53-71): n = sqrt((a0*a0 + a1*a1) + a2*a2).  Above n = 1e-12, Eigen's AngleAxis(n, a/n)
 *      .toRotationMatrix(): u = a/n, s = sin n, c = cos n, su = s*u, cu = (1 - c)*u; R01 = cu0*u1 - su2, R10 = cu0*u1 + su2, R02 = cu0*u2 +
 *      su1, R20 = cu0*u2 - su1, R12 = cu1*u2 - su0, R21 = cu1*u2 + su0, Rkk = cuk*uk + c.  At or below 1e-12 the first-order matrix of
 *      :59-69, [[1, -a2, a1], [a2, 1, -a0], [-a1, a0, 1]], which is not orthogonal, on purpose.
 *   4. RotationToAngleAxis (rigid3d.cc:47-51) is Eigen's AngleAxis(Matrix3d), which the reference does not contain; in full: matrix ->
 *      quaternion by the four-branch rule: t = (R00 + R11) + R22; when t > 0: t' = sqrt(t + 1), w = t'/2, f = 0.5/t', vec = ((R21 - R12) f,
 *      (R02 - R20) f, (R10 - R01) f); otherwise i the index of the largest diagonal entry (i = 1 when R11 > R00, then i = 2 when R22 > Rii),
 *      j = (i+1)%3, k = (j+1)%3: t' = sqrt(((Rii - Rjj) - Rkk) + 1), vec_i = t'/2, f = 0.5/t', w = (Rkj - Rjk) f, vec_j = (Rji + Rij) f,
 *      vec_k = (Rki + Rik) f.  Then nrm = |vec|, angle = 2 atan2(nrm, |w|), the axis is vec/nrm with nrm negated when w < 0, the result
 *      angle * axis, and the zero vector when nrm == 0.
 *   5. Residual (:453-469): r_e = -Log(R_2^T (Rrel_e R_1)), R_1 of image_id1; every entry of a 3x3 product as (p0 + p1) + p2.
 *   6. Gauge residual (:478-482): Log(Exp(fixed0)^T R_fixed), fixed0 the fixed camera's state at the start.
 *   7. Weights (:362-393): e2 = (r0*r0 + r1*r1) + r2*r2; XM_VGR_GEMAN_MCCLURE: w = s2/((e2 + s2)*(e2 + s2)) with s2 the square of sigma in
 *      radians (sigma * pi / 180, rigid3d.cc:37); XM_VGR_HALF_NORM: w = pow(e2, -0.75).  The three gauge rows have weight 1.  A weight that
 *      is not finite ends the call with XM_VGR_STOP_NONFINITE and the rotations, residuals and weights of the last completed iteration
 *      (weights 0 when there is none); a departure: the reference tests for NaN only and an infinite weight would poison its system.
 *   8. Linear system (:396-402): without gravity A^T W A = (L_w + e_f e_f^T) (x) I_3, L_w the weighted Laplacian of the participating
 *      pairs; the right-hand side at camera i is the sum of +w r over the pairs where i is image_id2, of -w r where it is image_id1 (a
 *      camera's pairs in input order), plus the gauge residual at the fixed camera.  It is solved matrix-free as ONE system of
 *      3 * registered unknowns by conjugate gradients preconditioned with the diagonal (weighted degree, + 1 at the fixed camera), from
 *      zero to a relative residual of 1e-12 or xm_view_graph_rotations_limits()[2] iterations; a capped solve is counted and its iterate
 *      used.  A departure: the reference factorises with CHOLMOD.
 *   9. Update (:418-435): est_i <- Log(Exp(est_i) Exp(-x_i)) for every registered image, the fixed one included.
 *  10. Stop (:485-499, :407-411): the sum of |x_i| over the registered images divided by their number goes to step_trace[iteration]; the
 *      loop ends when it is < irls_step_convergence_threshold (XM_VGR_STOP_STEP) or after max_num_irls_iterations (XM_VGR_STOP_ITERATIONS).
 *  11. XM_ERR_ARG, nothing written, everything checked on the host before any device call: an index out of range, pi == pj, an unknown
 *      weight type, a non-finite or non-positive option, a non-finite entry of rot0 of a registered image or of Rrel of a participating
 *      pair, a wrong struct_size, a null array where its count is positive, counts >= 2^31, fixed_image out of range or unregistered,
 *      registered images that the participating pairs do not connect (a host union-find; the reference assumes
 *      KeepLargestConnectedComponents ran, and a second component would make the system singular).  With no participating pair the call
 *      succeeds, copies rot0, reports zero iterations and XM_VGR_STOP_NOTHING, and needs no device.
 * Outputs: rot_out[9n] (Exp of the state; unregistered images keep rot0), angle_axis_out[3n] (0 when unregistered), residual[3 npairs] at
 * the final rotations, weight[npairs] of the last iteration's solve (0 for a pair that takes no part), step_trace[max_num_irls_iterations]
 * (0 behind the last iteration).
 * Not built: the maximum-spanning-tree start, the L1 / ADMM stage, gravity, use_weight (a TODO in the reference too).
 * Nothing here is compared with the reference's compiled code (it needs Eigen, SuiteSparse, COLMAP and glog): tests/xm_rotavg_numpy.py
 * restates the C++ line by line and the device is tested against that.  All f64; sums run in a fixed order and there is no atomic at all:
 * two calls give the same bytes. */
#define XM_VGR_GEMAN_MCCLURE 0          /* weight_type (RotationEstimatorOptions::GEMAN_MCCLURE, the default) */
#define XM_VGR_HALF_NORM     1
#define XM_VGR_STOP_NOTHING    0        /* stop_reason: no participating pair */
#define XM_VGR_STOP_STEP       1
#define XM_VGR_STOP_ITERATIONS 2
#define XM_VGR_STOP_NONFINITE  3
typedef struct {
    uint32_t struct_size;
    int32_t weight_type;                     /* XM_VGR_GEMAN_MCCLURE (global_rotation_averaging.h) */
    int32_t max_num_irls_iterations;         /* 100 */
    int32_t fixed_image;                     /* -1: the smallest registered index */
    double irls_step_convergence_threshold;  /* 1e-3 */
    double irls_loss_parameter_sigma;        /* 5.0, degrees */
} xm_vgr_options_t;
#define XM_VGR_OPTIONS_INIT { (uint32_t)sizeof(xm_vgr_options_t), XM_VGR_GEMAN_MCCLURE, 100, -1, 1e-3, 5.0 }
typedef struct {
    uint32_t struct_size;
    int32_t stop_reason;               /* XM_VGR_STOP_* */
    int32_t irls_iterations;
    int32_t reserved;
    int64_t pcg_iterations;            /* in total */
    int64_t pcg_capped;                /* solves that hit xm_view_graph_rotations_limits()[2] */
    int64_t pairs;                     /* participating pairs */
    int64_t registered;
    int64_t fixed_image;               /* -1 when nothing is registered */
    int64_t cams_heavy;                /* cameras above xm_view_graph_rotations_limits()[0] incidences */
    int64_t max_incidences;
    double seconds_index;              /* host: lists and upload */
    double seconds_kernels;
    double seconds_download;
} xm_vgr_result_t;
int xm_view_graph_rotations(int64_t n, const uint8_t *registered /* or NULL */, const double *rot0, int64_t npairs, const int32_t *pi,
                            const int32_t *pj, const double *Rrel, const uint8_t *valid_in /* or NULL */, const xm_vgr_options_t *opt,
                            double *rot_out, double *angle_axis_out, double *residual, double *weight, double *step_trace,
                            xm_vgr_result_t *res);
/* Test export (like xm_view_graph_calibrate_probe): with the kernels, grids and arguments of the call, at the caller's angle_axis[3n] (the
 * state) and x[3n] (a step; entries of unregistered images are ignored): the camera matrices rot (9 per image), residual (3 per pair), the
 * gauge residual (3; fixed0 comes from rot0), weight (per pair, of opt's type from those residuals), then with weight_in (per pair, or
 * NULL: the computed weights) rhs (3 per image), diagonal (per image), product (A^T W A x, 3 per image), and angle_axis_out (rule 9 with x)
 * and step (rule 10, one double).  Every output whose pointer is not null is filled; pairs and cameras that take no part hold 0. */
typedef struct {
    uint32_t struct_size;
    uint32_t reserved;
    const double *angle_axis, *x, *weight_in;
    double *rot, *residual, *gauge, *weight, *rhs, *diagonal, *product, *angle_axis_out, *step;
} xm_vgr_probe_t;
int xm_view_graph_rotations_probe(int64_t n, const uint8_t *registered, const double *rot0, int64_t npairs, const int32_t *pi,
                                  const int32_t *pj, const double *Rrel, const uint8_t *valid_in, const xm_vgr_options_t *opt,
                                  xm_vgr_probe_t *probe);
/* out[0]: most incidences of a camera that one thread walks (a camera above it gets a workgroup); out[1]: threads per workgroup;
 * out[2]: most PCG iterations of one solve; out[3]: 0 (spare) */
int xm_view_graph_rotations_limits(int64_t out[4]);
/* Translations and landmarks of a solution: the last step of utils/recoversolution.py:recover_XM (lines 77-86,
 * ybar_est = Abar @ sR_real.T; t_est = [0 | first N-1 columns], p_est = the rest) for an XM_STORAGE_SCHUR context.  The reference
 * needs the dense (N-1+M) x 3N matrix Abar.bin that create_matrix writes (creatematrix.py:283-311; 80 GB at Final-13682 with 800 k
 * landmarks); here Abar = -Qtp_bar^-1 Vtp_bar^T is applied through the factor chain of the matrix-free product, O(observations +
 * N^2).  rot: 3 x 3n column-major and scale: n as returned by xm_recover_rotations; t: 3 x n column-major (t[:, 0] = 0, the
 * anchor), p: 3 x n_landmarks column-major.  Uses the context's CURRENT observation weights. */
int xm_ctx_recover_tp(xm_ctx_t *ctx, const double *rot, const double *scale, double *t, double *p);
/* xm_tuning_t.schur_dense_q contexts: the context's CURRENT dense Q (after a re-weighting: the rebuilt one) to a host array, column-major,
 * ldq >= 3n.  XM_ERR_ARG for a context that did not build one. */
int xm_ctx_dense_q(xm_ctx_t *ctx, double *q, int64_t ldq);
/* The reference's create_matrix (utils/creatematrix.py:51-339) in one call from host arrays, on the device, without solver state: cam / lm
 * 0-based indices of the nobs observations, p nobs x 3 row-major camera-frame points, w weights (the arguments of an XM_STORAGE_SCHUR
 * problem).  Q: 3n x 3n column-major, ldq >= 3n, symmetric bit for bit.  Abar (NULL: not wanted): (n-1+m) x 3n column-major, the matrix
 * recover_XM multiplies with (camera rows -VT^-1 G^T, then one row per landmark, produced on the device 2048 landmarks at a time).  The limits
 * of xm_tuning_t.schur_dense_q apply (20000 cameras, no (camera, landmark) pair named twice). */
int xm_create_matrix(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *p, const double *w, double *Q,
                     int64_t ldq, double *Abar /* NULL: not wanted; (n-1+m) x 3n column-major */);
/* constants of the device build: out[0] = cameras per LDS column window of the assembly kernel, out[1] = landmarks per panel of Abar,
 * out[2] = the camera cap (host-only; tests derive their window-edge and multi-panel cases from them) */
int xm_schur_dense_limits(int64_t out[3]);
/* XM_STORAGE_SCHUR: how the reduced camera Laplacian VT = Q2_bar - V3_bar Q3^-1 V3_bar^T (utils/creatematrix.py:150-166) is applied inside a
 * product -- *uses_cg = 0: through its dense inverse (set-up O(N^3), 8 (N-1)^2 bytes; up to xm_tuning_t.schur_dense_max cameras), 1: by
 * preconditioned CG on the matrix-free VT (no N^2 array) -- and, for the CG form, stats = {products so far, inner CG iterations
 * so far, products that stopped at the iteration cap instead of at the tolerance 1e-13} and the relative residual of the last product. */
int xm_ctx_schur_info(xm_ctx_t *ctx, int *uses_cg, int64_t stats[3], double *last_relres);
/* *count = trust regions (rank levels) of the context's LAST xm_ctx_solve whose truncated CG ran in the two-launch form (XM_FLAG_TCG_THREE_LAUNCH,
 * or a configuration that form does not cover: 0).  Single-GPU contexts; XM_ERR_ARG otherwise.  (A getter, not a field: xm_result_t keeps its size.) */
int xm_ctx_tcg_two_launch(xm_ctx_t *ctx, int *count);
/* out[0] = truncated CGs of the context's LAST xm_ctx_solve that were replayed from the history of a rejected step instead of recomputed, out[1] = the
 * iterations they stand for (counted in tcg_iters, not executed).  Both 0 with XM_FLAG_TCG_RECOMPUTE or where the replay does not apply.
 * Single-GPU contexts; XM_ERR_ARG otherwise.  (A getter, not a field: xm_result_t keeps its size.) */
int xm_ctx_tcg_replay(xm_ctx_t *ctx, int64_t out[2]);
/* Iterations of a truncated CG whose direction and Hessian product are kept for that replay, from the context's next xm_ctx_solve on: 0 = the
 * default (64), 1 .. 256; anything else XM_ERR_ARG.  A rejected truncated CG that needs more iterations than this at the smaller radius is
 * recomputed, so the setting changes time and memory (2 x iterations x (3n x pitch + n) doubles), never a result.  Tests force small values.
 * (A setter, not a field: xm_tuning_t keeps its size.)  Single-GPU contexts; XM_ERR_ARG otherwise. */
int xm_ctx_set_tcg_history(xm_ctx_t *ctx, int32_t iterations);
/* ... and the preconditioner of the CG form: *kind = -1 no CG form (dense inverse, or not a matrix-free context), 0 Jacobi (schur_solver 2 or
 * auto), 1 two-level (schur_solver 3; *aggregates = their number n_c, *block = cameras per aggregate).  aggregates / block may be NULL. */
int xm_ctx_schur_precond_info(xm_ctx_t *ctx, int *kind, int64_t *aggregates, int *block);

/* ---- reprojection bundle adjustment of a recovered solution (the reference's Ceres refinement, 5_test_ceres.py:610-616,
 * utils/ceresforXM.py), on the device over the observation lists of an XM_STORAGE_SCHUR context.
 *   parameters  camera i: Rcw_i = R_i^T, tcw_i = -R_i^T t_i (rot: 3 x 3n column-major, t: 3 x n, as xm_recover_rotations /
 *               xm_ctx_recover_tp return them); landmark l: world point P_l (p: 3 x n_landmarks).  Host arrays, updated in place.
 *   residual    r_e = pi(Rcw_i P_l + tcw_i) - (p_e0 / p_e2, p_e1 / p_e2), pi(X) = (X0 / X2, X1 / X2) (SIMPLE_PINHOLE, f = 1, c = 0),
 *               cost F = 1/2 sum |r_e|^2 (unweighted) over the USED observations: current weight > 0 (XM^2-filtered ones drop out)
 *               and p_e2 > 0.  Cameras and landmarks without a used observation come back bit-identical.
 *   update      Rcw <- Exp(dtheta) Rcw (rotation vector, left), tcw += dt, P += dP; the gauge is free (no anchor, no scale).
 *   step        Levenberg-Marquardt with Ceres's rules: (J^T J + mu D) d = -J^T r, D = diag(J^T J) clamped to [1e-6, 1e32], mu = 1 / radius,
 *               radius 1e4 at the start; accepted when rho = (F - F_new) / model decrease > 1e-3 (radius /= max(1/3, 1 - (2 rho - 1)^3));
 *               rejected: radius /= nu, nu *= 2.  Landmarks eliminated, the reduced camera system solved by PCG from zero with the
 *               inverted diagonal camera blocks as preconditioner (ITERATIVE_SCHUR + SCHUR_JACOBI) to relative residual eta or 500
 *               iterations.  Deviation from Ceres: no Jacobi scaling (with block-Jacobi PCG and mu diag(J^T J) damping it changes
 *               only the clamp of D and the norm of the PCG's stop test).
 *   loss        loss (XM_BA_LOSS_*) with scale a = loss_scale in the normalised image units of r (pixels / focal length); Ceres's
 *               definitions (loss_function.cc) at s = |r_e|^2:  Huber  rho = s (s <= a^2), 2 a sqrt(s) - a^2;  SoftL1  2 b (sqrt(1 + s / b)
 *               - 1);  Cauchy  b log(1 + s / b);  Arctan  a atan2(s, a)  (b = a^2); rho' clamped below at the smallest normal double.  The
 *               cost is F = 1/2 sum rho(s_e) (initial_cost, final_cost and the trace report it); r_e and J_e are scaled by sqrt(rho'(s_e)),
 *               which is Ceres's Corrector for these losses (rho'' <= 0).  Which observations are used does not depend on the loss.
 *   steps       XM_BA_NONMONOTONIC: Ceres's non-monotonic steps (use_nonmonotonic_steps = true, the reference's configuration): step
 *               quality rho = max((F - F_new) / dm, (F_ref - F_new) / (dm_ref + dm)) with the reference cost F_ref reset after
 *               max_nonmonotonic (0 = 5) accepted steps without a new minimum (Conn, Gould & Toint, Algorithm 10.1.2); the call returns
 *               the point of least cost, and final_cost and gradient_max are those of that point.  Without the flag every accepted
 *               step decreases F.
 *   stops       |dF| / F <= function_tol on an accepted step; |J^T r|_inf <= gradient_tol (tangent coordinates); |d| <= parameter_tol
 *               (|x| + parameter_tol) with |x|^2 = sum over used cameras of (1 for a free rotation + |tcw|^2) + sum |P|^2; max_iters; max_time
 *               (seconds); radius < 1e-32.
 * Options: struct_size = sizeof(xm_ba_options_t), or XM_BA_OPTIONS_SIZE_V1 (64: the fields through trace, as the first version of this
 * struct had them; it means the trivial loss and monotonic steps); max_iters, max_time, function_tol, gradient_tol, parameter_tol: 0 = the
 * defaults (1000, 300, 1e-6, 1e-10, 1e-8); eta is required and lies in (0, 1) (Ceres's is 0.1).  trace: trace_cap x 6 doubles, one record
 * per LM iteration: cost, candidate cost, mu, accepted (0 / 1), PCG iterations, PCG relative residual.
 * XM_BA_DENSE_SCHUR (Ceres's linear_solver_type = DENSE_SCHUR): every LM iteration solves the reduced camera system (U* - sum W V*^-1 W^T)
 * dc = b exactly over all CD n rows instead of by PCG: S is assembled densely on the device (the lower block triangle, fixed-order sums, no
 * atomics), factored by Cholesky and solved by two triangular substitutions; everything else in the iteration is unchanged, and eta is
 * validated but not read.  A camera without a used observation has the block mu 1e-6 I and right-hand side 0 (its step is 0).  A pivot
 * that is not positive or a non-finite solution makes the step invalid (radius /= nu, nu *= 2, as a step without model decrease).
 * pcg_iters = 0; trace column 4 = 0 and column 5 = |b - S dc| / |b| with S applied matrix-free (a check of assembly and solve; -1 after a
 * failed factorisation).  The CD n x CD n matrix is allocated inside the call and freed before it returns: CD n > XM_BA_DENSE_MAX_ROWS is
 * XM_ERR_ARG, a failed allocation XM_ERR_NOMEM (both leave the context unchanged and usable).
 * XM_BA_PRECOND_TWO_LEVEL / XM_BA_PRECOND_BLOCKS (opt-in; for sequential captures, whose reduced camera system is close to a path graph and
 * takes block-Jacobi PCG to its 500-iteration cap): the PCG's preconditioner becomes M^-1 = blockdiag(S_aa)^-1 + P A_c^-1 P^T (TWO_LEVEL) or
 * its first term alone (BLOCKS, Ceres's CLUSTER_JACOBI in spirit); S, the stop rule, the start from zero and everything outside the PCG
 * are unchanged.  Aggregates a: the cameras with a used observation in breadth-first order over the camera-landmark graph
 * (xm_ba_aggregate_plan), cut into runs of XM_BA_AGG_CAMS; S_aa (16 CD square) is assembled and inverted on the device every LM iteration.
 * P: per aggregate the seven rigid-plus-scale motions X -> X + w x (X - c) + v + s (X - c) of its cameras about the centroid c of their
 * centres, in the tangent coordinates above (with XM_BA_FIX_ROTATIONS the four columns v, s of the translation rows), columns of unit
 * norm, recomputed after every accepted step; a column of norm 0 (all centres coincide) is dropped; a last aggregate of one camera shares
 * its predecessor's columns.  A_c = P^T S P is assembled (fixed-order sums, no atomics) and inverted every LM iteration; when it cannot be
 * (a pivot that is not positive, a non-finite entry) that iteration runs with the blocks alone and coarse_fallbacks counts it.  Both flags
 * together, either with XM_BA_DENSE_SCHUR, or more than XM_BA_MAX_AGGREGATES aggregates: XM_ERR_ARG.  The workspace is allocated inside
 * the call and freed before it returns (a failed allocation: XM_ERR_NOMEM).  Two calls give the same bits.
 * XM_ERR_ARG (context unchanged and usable): not XM_STORAGE_SCHUR, several ranks or a communicator, a struct_size other than those two,
 * null arrays, non-finite input, eta outside (0, 1), negative settings, unknown flags, an unknown loss, a robust loss whose loss_scale is
 * not finite and > 0, loss_scale != 0 with the trivial loss, max_nonmonotonic < 0.  The call reads the context and changes nothing in it
 * (Q, weights, solver workspace).
 * xm_ctx_reprojection_errors: sqerr[e] = |r_e|^2 (unrobustified) of every observation e in input order at (rot, t, p) (the layouts, context
 * and refusals of xm_ctx_bundle_adjust), -1 for an observation the adjustment does not use (current weight <= 0 or p_e2 <= 0); computed on
 * the device with the context's current weights, nothing in the context changes.  For choosing the loss scale before an adjustment and for
 * finding the outliers after it (xm_ctx_set_edge_weights can then drop them before the next solve).
 *
 * Focal refinement (XM_BA_REFINE_FOCAL, xm_ctx_bundle_adjust_focal): GLOMAP's bundle adjustment optimises the intrinsics by default
 * (estimators/bundle_adjustment.h:16) and holds only the principal point constant (bundle_adjustment.cc:163-175).  Here:
 *   model       one focal scale g_i > 0 per camera, g_i = f_i / f_prior_i, f_prior_i the focal with which the observations were normalised
 *               (focal: n, host, in-out).  r_e = g_i pi(Rcw_i P_l + tcw_i) - (p_e0 / p_e2, p_e1 / p_e2): with g = 1 the residual above; GLOMAP's
 *               pixel residual divided by f_prior, principal point constant.  Update g_i += dg_i.
 *   tangent     camera block (dtheta, dt, dg), CD = 7; (dt, dg), CD = 4, with XM_BA_FIX_ROTATIONS: the focal is the last column, the
 *               leading ones are those of the forms above.  d r / d g = pi(X); the pose and point Jacobians are those above times g_i;
 *               a robust loss's corrector scales the whole record as before.
 *   mask        focal_free (n, uint8; NULL = all free): a camera with focal_free = 0 has a zero focal column, so its diagonal entry is
 *               mu 1e-6 by the clamp of D and its right-hand side 0: its step is exactly 0 and its g_i comes back bit-identical.  The
 *               same holds for cameras without a used observation.
 *   g <= 0      a candidate with g_i + dg_i <= 0 for a used camera with a free focal is an invalid step: rejected exactly as a step
 *               without model decrease (radius /= nu, nu *= 2).  A returned focal is always > 0.
 *   stops       |x|^2 adds g_i^2 per used camera with a free focal, |d|^2 adds dg_i^2, gradient_tol sees the focal gradient.
 * Everything else is that of xm_ctx_bundle_adjust word for word: the LM rules, D = diag(J^T J) clamped, the PCG and its stop, non-monotonic
 * steps, losses, which observations are used, XM_BA_DENSE_SCHUR (XM_BA_DENSE_MAX_ROWS applies to 7 n / 4 n), determinism (two calls give
 * the same bytes).  xm_ctx_bundle_adjust_focal requires XM_BA_REFINE_FOCAL in opt->flags; xm_ctx_bundle_adjust refuses the flag as unknown.
 * The aggregate preconditioners are not available with a focal column (their coarse space, LDS block size and compensated assembly are
 * tuned to CD = 6 / 3): XM_BA_REFINE_FOCAL with XM_BA_PRECOND_TWO_LEVEL or XM_BA_PRECOND_BLOCKS is XM_ERR_ARG.  Also XM_ERR_ARG (context
 * unchanged and usable): focal NULL, a focal that is not finite or not positive, the flag missing, and every refusal above.
 * Departures from the reference: of the distortion parameters only one radial coefficient (xm_ctx_bundle_adjust_radial below: no second
 * coefficient, no tangential terms, none shared by focal group); fx = fy; no aggregate preconditioners with a focal column.
 * xm_ctx_reprojection_errors_focal: sqerr[e] = |g_i pi(X) - z_e|^2, -1 where the observation is unused.
 *
 * Radial distortion (XM_BA_REFINE_RADIAL, xm_ctx_bundle_adjust_radial): GLOMAP builds colmap::CreateCameraCostFunction<ReprojErrorCostFunctor>
 * over the camera's whole parameter vector (estimators/bundle_adjustment.cc:72-84) and with optimize_intrinsics holds only the principal
 * point (:163-175), so a radial coefficient moves with the focal.  Here:
 *   model       one radial coefficient k_i per camera beside the focal scale g_i (dist: n, host, in-out; dimensionless, either sign).  With
 *               u = pi(Rcw_i P_l + tcw_i), rho^2 = u0^2 + u1^2, s = 1 + k_i rho^2:  r_e = g_i s u - (p_e0 / p_e2, p_e1 / p_e2).  COLMAP's
 *               SIMPLE_RADIAL and BAL's model with k2 = 0, in pixels divided by the focal prior, principal point removed and held.  With
 *               k = 0 the residual of xm_ctx_bundle_adjust_focal.  Update g_i += dg_i, k_i += dk_i.
 *   tangent     camera block (dtheta, dt, dg, dk), CD = 8; (dt, dg, dk), CD = 5, with XM_BA_FIX_ROTATIONS: the leading columns and the focal
 *               column where they are at CD = 7 / 4, the distortion column last.  d r / d g = s u, d r / d k = g rho^2 u,
 *               d r / d u = g (s I + 2 k u u^T) in front of the pose and point Jacobians of the pinhole form; a robust loss's corrector scales
 *               the whole record as before.
 *   masks       focal_free and dist_free (n, uint8; NULL = all free), independent.  A held column is zero: diagonal mu 1e-6 by the clamp of D,
 *               right-hand side 0, a step of exactly 0, the value comes back bit-identical; the same for cameras without a used observation.
 *               An observation with rho = 0 contributes a zero distortion column, by the formula.
 *   invalid     a candidate with g_i <= 0 for a moving focal, or with 1 + 3 k_i rho^2 <= 0 at some used observation (there rho -> rho (1 +
 *               k rho^2) folds and stops being invertible), is rejected exactly as a step without model decrease (radius /= nu, nu *= 2).
 *               The caller's start is not checked.
 *   stops       |x|^2 adds g_i^2 and k_i^2 per used camera with the respective column free, |d|^2 adds dg_i^2 and dk_i^2, gradient_tol sees
 *               both gradients.
 * Everything else is xm_ctx_bundle_adjust_focal word for word: the LM rules, the block-Jacobi PCG with the inverted 8 x 8 / 5 x 5 blocks,
 * XM_BA_DENSE_SCHUR (XM_BA_DENSE_MAX_ROWS applies to 8 n / 5 n), losses, non-monotonic steps, which observations are used, determinism (no
 * atomics, fixed-order sums: two calls give the same bytes).  XM_BA_REFINE_RADIAL is valid only together with XM_BA_REFINE_FOCAL and only
 * in xm_ctx_bundle_adjust_radial and xm_ctx_ba_probe_radial; every other entry point refuses it as unknown.  XM_ERR_ARG (context unchanged
 * and usable): dist NULL or not finite, the flag without XM_BA_REFINE_FOCAL, either aggregate preconditioner flag, and every refusal of
 * the focal form.  Not built: a second radial coefficient (BAL's k2, COLMAP's RADIAL), distortion shared by focal group, aggregate
 * preconditioners, tangential terms, fx != fy.
 * xm_ctx_reprojection_errors_radial: sqerr[e] = |g_i s u - z_e|^2, -1 where the observation is unused.
 *
 * Focal groups (xm_ctx_bundle_adjust_focal_groups): GLOMAP shares a Camera among images -- every residual block takes
 * cameras[image.camera_id].params (estimators/bundle_adjustment.cc:72-84), so the focal belongs to the camera, not to the image.  Here:
 *   model       G groups; group_of (n, int32, in [0, G)) names every camera's group; focal (G, host, in-out, > 0), focal_free (G, uint8, or
 *               NULL = all free).  r_e = g_{group_of[i]} pi(Rcw_i P_l + tcw_i) - z_e.
 *   tangent     CP = CD - 1 columns per camera (6, or 3 with XM_BA_FIX_ROTATIONS), then the G focal entries: CP n + G in all (the order of
 *               the probe's vectors).  With E the 0/1 matrix that copies a group's unknown into the focal column of each member,
 *               J_shared = J_7 E; the reduced camera system is E^T S_7 E, its right-hand side E^T b_7.
 *   damping     Ceres's rule on the shared parameter: D_c = clamp(sum_{i in c} (J_7^T J_7)_ff,i, 1e-6, 1e32), mu D_c on the group's diagonal
 *               (not the sum of the members' clamped terms).
 *   held        a group with focal_free[c] = 0, and a group none of whose members has a used observation (an empty group among them): zero
 *               columns, right-hand side 0, diagonal mu 1e-6, a step of exactly 0; its focal comes back bit-identical.
 *   g <= 0      a candidate g_c + dg_c <= 0 of a moving group is an invalid step, as above.
 *   stops       |x|^2 adds g_c^2 and |d|^2 adds dg_c^2 once per moving group, not per member.
 *   PCG         preconditioner blockdiag(the cameras' pose blocks of S, F).  G <= XM_BA_FOCAL_GROUPS_EXACT: F = S_shared[focal, focal], the
 *               exact G x G block, from G products with indicator vectors once per LM iteration, inverted on the device; a factorisation
 *               that fails leaves that iteration with the rule for larger G and is counted in xm_ba_result_t.coarse_fallbacks.  Larger G:
 *               F = diag(sum_{i in c} S_7,ii[f, f] + mu D_c).  Both are SPD: principal blocks of an SPD matrix, or positive scalars.
 *   dense       XM_BA_DENSE_SCHUR solves the (CP n + G)-row system exactly: the CD n matrix is assembled as before and its focal rows and
 *               columns are contracted by group in a fixed order; XM_BA_DENSE_MAX_ROWS applies to CD n.
 * Everything else is xm_ctx_bundle_adjust_focal word for word: the LM rules, losses, non-monotonic steps, stops, which observations are
 * used, determinism (the sums over a group's members are taken in a fixed order without atomics: two calls give the same bytes).
 * XM_ERR_ARG with the context unchanged: XM_BA_REFINE_FOCAL missing, G < 1 or G > n, a group_of entry out of range, a focal that is not
 * positive or not finite, an aggregate preconditioner flag, and every refusal of the per-image form.  xm_ctx_reprojection_errors_focal takes per-image scales: pass focal[group_of[i]]. */
#define XM_BA_FIX_ROTATIONS 1u          /* the reference's only_landmarks = True: rotations constant (bit-identical), t and P free */
#define XM_BA_NONMONOTONIC  2u          /* Ceres's non-monotonic steps (see above) */
#define XM_BA_DENSE_SCHUR   16u         /* Ceres's DENSE_SCHUR (see below) instead of ITERATIVE_SCHUR; 4 and 8 are not flags */
#define XM_BA_PRECOND_TWO_LEVEL 32u     /* PCG preconditioner: aggregate blocks + rigid-motion coarse operator (see below) */
#define XM_BA_PRECOND_BLOCKS    64u     /* PCG preconditioner: the aggregate blocks alone (the ablation of the above) */
#define XM_BA_REFINE_FOCAL      128u    /* a focal scale per camera joins the camera block (xm_ctx_bundle_adjust_focal only; see above) */
#define XM_BA_REFINE_RADIAL     256u    /* a radial coefficient per camera behind the focal scale (xm_ctx_bundle_adjust_radial only; see above) */
#define XM_BA_AGG_CAMS          16      /* cameras per aggregate */
#define XM_BA_FOCAL_GROUPS_EXACT 16     /* focal groups: up to this many, the preconditioner's focal block is the exact G x G one */
#define XM_BA_MAX_AGGREGATES    4096    /* at most this many aggregates (65 536 cameras): A_c has up to 28 672 rows */
#define XM_BA_DENSE_MAX_ROWS 32768      /* XM_BA_DENSE_SCHUR: largest CD n (CD = 6, or 3 with XM_BA_FIX_ROTATIONS): an 8.6 GB matrix */
#define XM_BA_LOSS_TRIVIAL  0
#define XM_BA_LOSS_HUBER    1
#define XM_BA_LOSS_SOFT_L1  2
#define XM_BA_LOSS_CAUCHY   3
#define XM_BA_LOSS_ARCTAN   4
#define XM_BA_OPTIONS_SIZE_V1 64u       /* struct_size of callers built before loss, max_nonmonotonic and loss_scale */
#define XM_BA_NO_CONVERGENCE       0
#define XM_BA_CONVERGED_FUNCTION   1
#define XM_BA_CONVERGED_GRADIENT   2
#define XM_BA_CONVERGED_PARAMETER  3
#define XM_BA_MAX_ITERATIONS       4
#define XM_BA_TIME_LIMIT           5
#define XM_BA_NO_PROGRESS          6    /* the trust-region radius fell below 1e-32 */
typedef struct {
    uint32_t struct_size;
    int32_t max_iters;
    double max_time, eta, function_tol, gradient_tol, parameter_tol;
    uint32_t flags;            /* XM_BA_* */
    int32_t trace_cap;
    double *trace;
    int32_t loss;              /* XM_BA_LOSS_* */
    int32_t max_nonmonotonic;  /* Ceres's max_consecutive_nonmonotonic_steps; 0 = 5 */
    double loss_scale;         /* Ceres's a; 0 with the trivial loss */
} xm_ba_options_t;
typedef struct {
    uint32_t struct_size;
    int32_t status;            /* XM_BA_* */
    int32_t iters, accepted;   /* LM iterations, accepted steps */
    int64_t pcg_iters, n_used; /* PCG iterations over all steps; observations in the cost */
    double initial_cost, final_cost, gradient_max, seconds;
    int32_t trace_len;
    int32_t coarse_fallbacks;  /* XM_BA_PRECOND_TWO_LEVEL: LM iterations that ran with the blocks alone (in what was tail padding) */
} xm_ba_result_t;
int xm_ctx_bundle_adjust(xm_ctx_t *ctx, const xm_ba_options_t *opt, double *rot, double *t, double *p, xm_ba_result_t *res);
int xm_ctx_reprojection_errors(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, double *sqerr);
int xm_ctx_bundle_adjust_focal(xm_ctx_t *ctx, const xm_ba_options_t *opt, double *rot, double *t, double *p, double *focal /* n, in-out */,
                               const uint8_t *focal_free /* n or NULL */, xm_ba_result_t *res);
int xm_ctx_reprojection_errors_focal(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, const double *focal, double *sqerr);
int xm_ctx_bundle_adjust_focal_groups(xm_ctx_t *ctx, const xm_ba_options_t *opt, double *rot, double *t, double *p, int64_t ngroups,
                                      const int32_t *group_of /* n */, double *focal /* ngroups, in-out */,
                                      const uint8_t *focal_free /* ngroups or NULL */, xm_ba_result_t *res);
int xm_ctx_bundle_adjust_radial(xm_ctx_t *ctx, const xm_ba_options_t *opt, double *rot, double *t, double *p, double *focal /* n, in-out */,
                                const uint8_t *focal_free /* n or NULL */, double *dist /* n, in-out */, const uint8_t *dist_free /* n or NULL */,
                                xm_ba_result_t *res);
int xm_ctx_reprojection_errors_radial(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, const double *focal, const double *dist,
                                      double *sqerr);
/* ---- Filtering tracks against a refined geometry: the TrackFilter of the reference's fork of GLOMAP
 * (deps/glomap/glomap/processors/track_filter.cc: FilterTracksByReprojection :7-51, FilterTracksByAngle :53-89,
 * FilterTrackTriangulationAngle :91-126), which GLOMAP alternates with its bundle adjustment (controllers/global_mapper.cc:243-317), as a
 * query on the device over the observation lists of an XM_STORAGE_SCHUR context.  NOTHING HERE WAS COMPARED WITH THE REFERENCE'S COMPILED
 * CODE (it needs COLMAP, Eigen and glog): parity rests on a line-cited sequential restatement (tests/xm_trackfilter_numpy.py).
 * Input: rot (3 x 3n), t (3 x n), p (3 x n_landmarks), column-major, the layouts of xm_ctx_bundle_adjust: R_i is camera-to-world, t_i the
 * camera centre, P_l the world point.  An observation e = (i, l) with the camera-frame point p_e is USED when its current weight is > 0
 * and p_e2 > 0 (the bundle adjustment's rule).  Every product and sum below is rounded on its own, in the order written:
 *   d = P_l - t_i;  q_a = (R_i[0][a] d_0 + R_i[1][a] d_1) + R_i[2][a] d_2 (q = R_i^T d);  x . y = (x_0 y_0 + x_1 y_1) + x_2 y_2;
 *   |x| = sqrt(x . x); division and square root are IEEE.
 *   depth          with XM_TF_REPROJECTION or XM_TF_ANGLE: q_2 < 1e-12 (GLOMAP's EPS, :20, :70) drops the observation.
 *   reprojection   XM_TF_REPROJECTION (:27-30, :39, the normalised-image branch): u = q_0 / q_2 - p_e0 / p_e2, v = q_1 / q_2 - p_e1 / p_e2; kept
 *                  iff sqrt(u u + v v) < max_reprojection_error (1e-2 is glomap/types.h:21).  DEPARTURE: the observed point is the bundle
 *                  adjustment's p_e / p_e2, without the reference's + EPS in the denominator.
 *   angle          XM_TF_ANGLE (:60-79), on what the reprojection filter left: kept iff (q / |q|) . (p_e / |p_e|) > cos(max_angle_error)
 *                  (degrees; 1.0 is types.h:20).  DEPARTURE: every camera counts as calibrated (no has_prior_focal_length, no doubled
 *                  threshold).
 *   triangulation  XM_TF_TRIANGULATION (:97-121), over the SURVIVORS of a landmark: rays r_e = d / |d|; the landmark is kept iff some pair
 *                  of survivors has r_e . r_f < cos(min_triangulation_angle) (degrees; 1.0 is types.h:22), otherwise all its observations
 *                  are dropped; fewer than two survivors: no such pair.
 *   min_views      > 0: a landmark that is left with fewer observations than that (and at least one) loses them all; applied last
 *                  (the reference's bundle adjustment skips tracks below 3, bundle_adjustment.cc:65).
 * The two cosines are computed once on the host, cos(angle * (pi / 180)), and come back in the result: the comparisons above are against
 * those doubles.  A comparison with a NaN is false (the observation or pair does not pass).
 * Output (host arrays): keep[nobs] (1 = used and it stays), reason[nobs] (one XM_TF_REASON_* bit for a used observation that is dropped: the
 * first rule above that drops it; 0 where kept or unused), lm_views[n_landmarks] (observations left after all filters), lm_status
 * [n_landmarks] (XM_TF_LM_*: KEPT = no rule dropped the landmark as a whole, also when no observation of it is left).  Result: observations
 * used, kept and dropped per reason; tracks_total = landmarks with a used observation before the call, tracks_kept = landmarks with
 * lm_views > 0; tracks_changed_* = GLOMAP's return value `counter` of each filter applied in the order above: the landmarks whose list the
 * reprojection filter changed (:43-46; observations behind the camera included), then the angle filter (:81-84; those included when it
 * runs first), the landmarks without a qualifying pair (:118-120, which counts a track that an earlier filter of the same call emptied
 * too), and the landmarks that min_views dropped.  seconds_kernels: upload of (rot, t, p) and kernels; seconds_download: the four arrays.
 * On the device (xm_trackfilter.h): a thread per observation, a thread per landmark of up to xm_track_filter_limits()[0] observations, a
 * workgroup with LDS tiles of [1] rays per longer one (no limit on the length), a thread per observation again, one fixed-order
 * reduction; no atomics.  The call reads the context and changes nothing in it; two calls give the same bits, and every output equals the
 * restatement in numpy exactly.  XM_ERR_ARG (context unchanged and usable): not XM_STORAGE_SCHUR, several ranks or a communicator, a
 * struct_size that is not sizeof, null arrays, non-finite input, unknown flags, min_views < 0, and for a filter that is switched on a
 * threshold that is not finite and positive (angles: at most 180). */
#define XM_TF_REPROJECTION  1u
#define XM_TF_ANGLE         2u
#define XM_TF_TRIANGULATION 4u
#define XM_TF_REASON_DEPTH          1
#define XM_TF_REASON_REPROJECTION   2
#define XM_TF_REASON_ANGLE          4
#define XM_TF_REASON_TRIANGULATION  8
#define XM_TF_REASON_MIN_VIEWS      16
#define XM_TF_LM_KEPT           0
#define XM_TF_LM_UNUSED         1       /* no used observation before the call */
#define XM_TF_LM_TRIANGULATION  2
#define XM_TF_LM_MIN_VIEWS      3
typedef struct {
    uint32_t struct_size;
    uint32_t flags;                    /* XM_TF_REPROJECTION | XM_TF_ANGLE | XM_TF_TRIANGULATION */
    double max_reprojection_error;     /* normalised image units; GLOMAP: 1e-2 */
    double max_angle_error;            /* degrees; GLOMAP: 1.0 */
    double min_triangulation_angle;    /* degrees; GLOMAP: 1.0 */
    int32_t min_views;                 /* 0 = off */
    int32_t reserved;
} xm_tf_options_t;
typedef struct {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t tracks_total, tracks_kept, obs_used, obs_kept;
    int64_t dropped_depth, dropped_reprojection, dropped_angle, dropped_triangulation, dropped_min_views;
    int64_t tracks_changed_reprojection, tracks_changed_angle, tracks_changed_triangulation, tracks_changed_min_views;
    double cos_angle, cos_triangulation;   /* the thresholds the kernels compared against (0 for a filter that is off) */
    double seconds_kernels, seconds_download;
} xm_tf_result_t;
int xm_ctx_filter_tracks(xm_ctx_t *ctx, const xm_tf_options_t *opt, const double *rot, const double *t, const double *p, uint8_t *keep,
                         uint8_t *reason, int32_t *lm_views, uint8_t *lm_status, xm_tf_result_t *res);
/* out[0] = observations of the longest landmark that one thread walks (longer ones get a workgroup), out[1] = rays per LDS tile of the
 * workgroup form, out[2] = threads per workgroup (host-only; tests derive their boundary cases from them) */
int xm_track_filter_limits(int64_t out[3]);
/* ---- Landmarks from 2-D tracks at given poses: the capability behind step 7 of the reference's fork of GLOMAP, retriangulation
 * (deps/glomap/glomap/controllers/global_mapper.cc:322-375, controllers/track_retriangulation.cc), as a query on the device over the
 * observation lists of an XM_STORAGE_SCHUR context.  NOTHING HERE WAS COMPARED WITH THE REFERENCE'S COMPILED CODE: the fork only calls
 * COLMAP's IncrementalMapper::TriangulateImage and CompleteAndMergeTracks, and COLMAP's sources are not part of it.  Parity rests on
 * the project's own contract, restated in tests/xm_triangulate_numpy.py and modelled on the structure of COLMAP's triangulator as GLOMAP
 * configures it: create from two-view samples under an angular error, refine linearly, complete under a reprojection error, require a
 * minimum triangulation angle.  DESIGN.md 2.23 lists the departures.
 * Input: rot (3 x 3n), t (3 x n), p (3 x n_landmarks, in-out), column-major, the layouts of xm_ctx_bundle_adjust: R_i is camera-to-world,
 * t_i the camera centre.  Observation e = (i, l) has the camera-frame point p_e.  The CANDIDATES of a landmark: with candidate == NULL
 * the observations the bundle adjustment uses (current weight > 0 and p_e2 > 0); otherwise those with candidate[e] != 0 and p_e2 > 0,
 * whatever their weight (this is how dropped observations come back).  A landmark's LIST is all its observations in input order
 * (the order of the context's by-landmark list), positions 0 .. L-1; a position that holds no candidate takes part in nothing but keeps
 * its place in the schedule and in the sums.  Every product and sum below is rounded on its own, in the order written:
 *   x . y = (x_0 y_0 + x_1 y_1) + x_2 y_2;  |x| = sqrt(x . x); division and square root are IEEE; a comparison with a NaN is false.
 *   A sum over a list is the pairwise tree over the positions padded with +0.0 to a power of two, adjacent pairs first:
 *   ((x_0 + x_1) + (x_2 + x_3)) + ...; the term of a position that is masked out is +0.0.
 *   1 rays        u = p_e0 / p_e2, v = p_e1 / p_e2;  g_r = (R_i[r][0] u + R_i[r][1] v) + R_i[r][2];  b_e = g / |g|;  c_e = t_i.
 *   2 hypotheses  unordered pairs of positions in the schedule d = 1 .. L / 2 (integer), a = 0 .. L-1, pair (a, (a + d) mod L); for
 *                 2 d = L only a < L / 2.  That is every pair once; entry h is d = h / L + 1, a = h - (d - 1) L.  The first H =
 *                 min(max_hypotheses, L (L-1) / 2) entries are tried (counted in pairs_tested for a landmark with two candidates or
 *                 more).  For the pair (1, 2) = (a, (a + d) mod L):  cs = b_1 . b_2;  w = c_2 - c_1;  d_1 = b_1 . w;  d_2 = b_2 . w;
 *                 den = 1 - cs cs;  s = (d_1 - cs d_2) / den;  t = (cs d_1 - d_2) / den;  X_k = 0.5 ((c_1k + s b_1k) + (c_2k + t b_2k)),
 *                 the midpoint of the two closest points.  The pair is a hypothesis iff both positions hold candidates,
 *                 cs < cos(min_angle), den > 0, s > 0 and t > 0 (counted in hypotheses_scored).
 *   3 score       the number of candidates with (dx . b_e) / |dx| > cos(create_max_angle_error), dx = X - c_e.  The highest count wins,
 *                 among equals the earliest entry of the schedule.  lm_support is that count and lm_hypothesis that entry (0 and -1
 *                 when there is no hypothesis).  No hypothesis, or a count below two: XM_TRI_LM_NO_HYPOTHESIS.  The supporters of the
 *                 winner are the first members.
 *   4 refinement and completion, refine_rounds times.  Fewer than two members: XM_TRI_LM_MIN_VIEWS.  Per member, with sc = b . c:
 *                 A_00 += 1 - b_0 b_0, A_01 += 0 - b_0 b_1, A_02 += 0 - b_0 b_2, A_11 += 1 - b_1 b_1, A_12 += 0 - b_1 b_2,
 *                 A_22 += 1 - b_2 b_2, r_k += (c_k - b_k sc) + 0 (nine tree sums; no term is -0.0, so the padding cannot show).
 *                 k_00 = A_11 A_22 - A_12 A_12, k_01 = A_02 A_12 - A_01 A_22, k_02 = A_01 A_12 - A_02 A_11, k_11 = A_00 A_22 - A_02 A_02,
 *                 k_12 = A_01 A_02 - A_00 A_12, k_22 = A_00 A_11 - A_01 A_01;  det = (A_00 k_00 + A_01 k_01) + A_02 k_02;
 *                 det not finite and > 0: XM_TRI_LM_DEGENERATE.  X_0 = ((k_00 r_0 + k_01 r_1) + k_02 r_2) / det, X_1 = ((k_01 r_0 +
 *                 k_11 r_1) + k_12 r_2) / det, X_2 = ((k_02 r_0 + k_12 r_1) + k_22 r_2) / det.  The members afterwards: the candidates
 *                 with d = X - t_i, q = R_i^T d as in xm_ctx_filter_tracks, q_2 >= 1e-12 and sqrt(uu uu + vv vv) <
 *                 complete_max_reproj_error for uu = q_0 / q_2 - u, vv = q_1 / q_2 - v (the formulas of XM_TF_REPROJECTION).
 *   5 acceptance  fewer than max(min_views, 2) members: XM_TRI_LM_MIN_VIEWS; no pair of members with b_e . b_f < cos(min_angle):
 *                 XM_TRI_LM_ANGLE.  Accepted: p[:, l] = X, keep = the members, lm_views = their number.  Rejected, or without a
 *                 candidate (XM_TRI_LM_UNUSED): the landmark's column of p comes back bit for bit, keep = 0, lm_views = 0.
 * The two cosines are computed once on the host, cos(angle * (pi / 180)), and come back in the result.
 * Output (host arrays): p, keep[nobs], reason[nobs] (XM_TRI_REASON_*; 0 where kept), lm_views, lm_status (XM_TRI_LM_*), lm_support,
 * lm_hypothesis [n_landmarks].  Result: landmarks per status; observations that are candidates, kept, re-admitted (kept with current
 * weight <= 0) and lost (used by the bundle adjustment before, not kept); pairs tested and hypotheses scored; seconds_kernels: upload of
 * (rot, t, candidate) and kernels; seconds_download: the arrays.
 * On the device (xm_triangulate.h): a thread per observation, a wavefront per landmark of up to xm_triangulate_limits()[0] observations,
 * a workgroup with tiles of [1] rays per longer one (no limit on the length), a thread per observation again, one fixed-order
 * reduction; no atomics.  The call reads the context and changes nothing in it; two calls give the same bits, and every output equals the
 * restatement in numpy exactly.  XM_ERR_ARG (context unchanged and usable): the refusals of xm_ctx_filter_tracks (not
 * XM_STORAGE_SCHUR, several ranks or a communicator, a struct_size that is not sizeof, null arrays, non-finite input), max_hypotheses < 1, refine_rounds < 1, min_views < 0, an angle outside
 * (0, 180], a complete_max_reproj_error that is not finite and positive, 2^31 observations or more. */
#define XM_TRI_LM_ACCEPTED       0
#define XM_TRI_LM_UNUSED         1       /* no candidate */
#define XM_TRI_LM_NO_HYPOTHESIS  2
#define XM_TRI_LM_DEGENERATE     3
#define XM_TRI_LM_MIN_VIEWS      4
#define XM_TRI_LM_ANGLE          5
#define XM_TRI_REASON_NOT_CANDIDATE  1
#define XM_TRI_REASON_NOT_MEMBER     2   /* a candidate of an accepted landmark that the completion left out */
#define XM_TRI_REASON_LANDMARK       4   /* a candidate of a landmark that was not accepted */
typedef struct {
    uint32_t struct_size;
    int32_t max_hypotheses;            /* entries of the pair schedule tried per landmark; 64 */
    double min_angle;                  /* degrees; GLOMAP: 1.0 (track_retriangulation.h:13) */
    double create_max_angle_error;     /* degrees; COLMAP's default, 2.0 */
    double complete_max_reproj_error;  /* normalised image units; 1e-2, the project's max_reprojection_error */
    int32_t min_views;                 /* members an accepted landmark needs (at least 2 are always needed); 2 */
    int32_t refine_rounds;             /* 2 */
} xm_tri_options_t;
#define XM_TRI_OPTIONS_INIT { (uint32_t)sizeof(xm_tri_options_t), 64, 1.0, 2.0, 1e-2, 2, 2 }
typedef struct {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t lm_accepted, lm_unused, lm_no_hypothesis, lm_degenerate, lm_min_views, lm_angle;
    int64_t obs_candidates, obs_kept, obs_readmitted, obs_lost;
    int64_t pairs_tested, hypotheses_scored;
    double cos_min_angle, cos_create;      /* the thresholds the kernels compared against */
    double seconds_kernels, seconds_download;
} xm_tri_result_t;
int xm_ctx_triangulate_tracks(xm_ctx_t *ctx, const xm_tri_options_t *opt, const double *rot, const double *t, double *p,
                              const uint8_t *candidate /* nobs or NULL */, uint8_t *keep, uint8_t *reason, int32_t *lm_views,
                              uint8_t *lm_status, int32_t *lm_support, int32_t *lm_hypothesis, xm_tri_result_t *res);
/* out[0] = observations of the longest landmark that one wavefront holds (longer ones get a workgroup), out[1] = rays per tile and
 * hypotheses per batch of the workgroup form, out[2] = threads per workgroup (host-only; tests derive their boundary cases from them) */
int xm_triangulate_limits(int64_t out[3]);
/* ---- Pruning weakly connected images by covisibility clusters: step 8 of the reference's fork of GLOMAP, PruneWeaklyConnectedImages
 * (deps/glomap/glomap/processors/reconstruction_pruning.cc:6-84) with ViewGraphManipulater::EstablishStrongClusters
 * (processors/view_graph_manipulation.cc:68-168) and ViewGraph::KeepLargestConnectedComponents / MarkConnectedComponents
 * (scene/view_graph.cc:9-90), as a query on the device over an observation list.  NOTHING HERE WAS COMPARED WITH THE REFERENCE'S COMPILED
 * CODE (it needs COLMAP, Eigen and glog): parity rests on a line-cited sequential restatement (tests/xm_prune_numpy.py).
 * Input: n cameras (the reference's images), m landmarks (its tracks), nobs observations (cam[e], lm[e]), 0-based.  An observation is
 * USED when its weight is > 0 (w == NULL: all; the rule of xm_clean_observations).  L_l = used observations of landmark l; landmarks with
 * L_l <= 2 are skipped (:14).  A (camera, landmark) pair named twice counts twice, as in the reference's loops.  a_l(i) = used
 * observations of camera i in the landmark l that is not skipped.
 *   1 observation count  obs_count[i] = sum over l of a_l(i) (:17).
 *   2 covisibility       for i < j: covis(i, j) = sum over l of a_l(i) a_l(j) (:16-31, with its image_id1 == image_id2 skip).
 *   3 visibility graph   pairs_covisible = pairs with covis >= min_covisibility (5, :41; the reference's `counter`); the EDGES are those of
 *                        them with obs_count >= min_num_observations at both ends (:46-48); an edge's weight is its covis.
 *   4 threshold          median = element E / 2 (integer division) of the sorted edge weights, mad = element E / 2 of the sorted
 *                        |weight - median| (:61-70), threshold = max(median - mad, min_threshold) (20.0, :80): integers held exactly in a
 *                        double.  DEPARTURE: E = 0 is undefined behaviour in the reference (pair_count[0] of an empty vector); here every
 *                        cluster_id = -1, n_clusters = 0, threshold = 0, rounds = 0 and XM_OK.
 *   5 largest component  of the edges (view_graph.cc:9-46); edges outside it become invalid.  DEPARTURE: of several largest ones the
 *                        component with the smallest image index stays (the reference: the first in hash order).
 *   6 strong clusters    union over the valid edges with weight > threshold (view_graph_manipulation.cc:79-90); an image without such an
 *                        edge is a cluster of its own.  strong_clusters counts the clusters among the images of the largest component.
 *   7 merge rounds       (:95-149) in a round every valid edge that is not `weight < 0.75 threshold` (the product computed once, in double)
 *                        and whose ends lie in different clusters counts once for its unordered pair of clusters; all cluster pairs with
 *                        count >= 2 are united at once: the new clusters are the components of that cluster graph, so the order of the
 *                        unions cannot matter.  Rounds repeat while a round united anything; the body runs at most 10 times
 *                        (`iteration > 10` breaks in front of the 11th).  rounds = bodies run; weak_edges = the edges the first round
 *                        looked at.
 *   8 final marking      (:151-161, view_graph.cc:66-90) valid edges whose ends differ in cluster become invalid; the components of what
 *                        is left are sorted by size, descending; DEPARTURE: equal sizes go by smallest image index first (the reference
 *                        sorts (size, index into a hash-ordered vector)).  Components get cluster_id 0, 1, ... while their size is
 *                        >= min_num_images (2); every other image, every image without a valid edge included, gets -1.
 * Output (host arrays): cluster_id[n], obs_count[n]; pairs (optional): the visibility graph in (i, j) order, i < j, into host arrays of
 * `capacity` entries each; with a capacity below n_edges nothing is written, and n_edges says what is needed.  seconds_kernels: from the
 * call to the final labels on the host; seconds_download: the pairs.
 * On the device (xm_prune.h): a workgroup per camera with an LDS histogram of xm_prune_limits()[0] camera bins at a time (integer LDS
 * atomics: a sum has one value in any order), a prefix sum for the positions of the edges, a two-level histogram select for the two order
 * statistics, and three component labellings.  No floating-point atomic, and no atomic decides an order or a position.  The merge rounds
 * run on the host over the downloaded edges that step 7 looks at; the final ranking of the components too.  The call changes nothing it is
 * given; two calls give the same bits, and every output equals the restatement in numpy exactly.
 * Limits: n, m, nobs and n_edges below 2^31 each and every covis below 2^31 (XM_ERR_ARG where the call can see it).
 * xm_prune_weakly_connected: host arrays, uploaded inside the call.  xm_ctx_prune_weakly_connected: the lists an XM_STORAGE_SCHUR
 * context holds on the device at its CURRENT weights, with no upload of the list.  XM_ERR_ARG (context unchanged and usable): another
 * storage, several ranks or a communicator, a struct_size that is not sizeof, null outputs, a negative option, a min_threshold that is
 * not finite, a pairs struct with capacity < 0 or with a null array at capacity > 0, an index out of range. */
typedef struct {
    uint32_t struct_size;
    int32_t min_covisibility;      /* GLOMAP: 5 */
    int32_t min_num_images;        /* GLOMAP: 2 */
    int32_t min_num_observations;  /* GLOMAP: 0 */
    double min_threshold;          /* GLOMAP: 20.0 */
} xm_prune_options_t;
#define XM_PRUNE_OPTIONS_INIT {(uint32_t)sizeof(xm_prune_options_t), 5, 2, 0, 20.0}
typedef struct {
    int64_t capacity;
    int32_t *i, *j, *count;
} xm_prune_pairs_t;
typedef struct {
    uint32_t struct_size;
    int32_t rounds;                /* bodies of the merge loop that ran (0: empty graph) */
    int64_t pairs_covisible, n_edges;
    double median, mad, threshold;
    int64_t component_images;      /* images of the largest component */
    int64_t strong_clusters;       /* clusters of step 6 among them */
    int64_t weak_edges;            /* edges the first merge round looked at */
    int64_t n_clusters, images_clustered;
    double seconds_kernels, seconds_download;
} xm_prune_result_t;
int xm_prune_weakly_connected(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *w /* NULL: all used */,
                              const xm_prune_options_t *opt, int32_t *cluster_id, int32_t *obs_count, const xm_prune_pairs_t *pairs /* may be NULL */,
                              xm_prune_result_t *res);
int xm_ctx_prune_weakly_connected(xm_ctx_t *ctx, const xm_prune_options_t *opt, int32_t *cluster_id, int32_t *obs_count,
                                  const xm_prune_pairs_t *pairs /* may be NULL */, xm_prune_result_t *res);
/* out[0] = camera bins per LDS tile of the covisibility histogram, out[1] = threads per workgroup, out[2] = entries of the longest landmark
 * list that a group of out[3] lanes walks (longer ones: the whole workgroup), out[4] = low bits of the order statistics' second level
 * (host-only; tests derive their boundary cases from them) */
int xm_prune_limits(int64_t out[5]);

/* ================================================================== 3. kernel-level entry points (device pointers) */
/* device memory helpers so that callers need no other GPU runtime */
int xm_dev_count(int *count);
int xm_dev_alloc(void **ptr, size_t bytes);
int xm_dev_free(void *ptr);
int xm_dev_h2d(void *dst, const void *src, size_t bytes);
int xm_dev_d2h(void *dst, const void *src, size_t bytes);
int xm_dev_sync(void);

/* lay a host column-major symmetric Q out as the device row-major padded matrix (allocates *dq) */
int xm_dense_upload(const double *q_host, int64_t ldq, int64_t n, double **dq);
/* build the same device layout from a 3x3-block CSR description on the host (zero elsewhere) without ever forming
 * the dense matrix on the host — used to store a >= 10k-camera view-graph Q densely (13.5 GB at n = 13682) */
int xm_dense_from_bsr3(const int64_t *rowptr, const int32_t *colidx, const double *blocks, int64_t n, double **dq);
/* out = alpha * Q * W.  dq from xm_dense_upload; dW, dOut: device, row-major 3n x o (o in 1,3..10).
 * Replaces cublasDgemm via DnMatDnMat (Dense/matmul.h:42-87). stream: hipStream_t or NULL. */
int xm_qw_dense(const double *dq, int64_t n, int o, const double *dW, double *dOut, double alpha, void *stream);
/* the same product reading only the upper block triangle of a SYMMETRIC Q (o in 1, 3..5; allocates its scratch per call) */
int xm_qw_dense_sym(const double *dq, int64_t n, int o, const double *dW, double *dOut, double alpha, void *stream);
/* fp32 copy of a device matrix in the padded layout above (*dq32 allocated here, free with xm_dev_free): 3n rows of xm_dense_ld(n) floats,
 * the SAME leading dimension in elements (row pitch 4 * xm_dense_ld(n) bytes), each element rounded to nearest (subnormals kept).
 * XM_ERR_ARG when an element is not finite in fp32 (the copy is made either way). */
int xm_dense_to_f32(const double *dq, int64_t n, float **dq32);
/* out = alpha * Q32 * W with Q32 from xm_dense_to_f32: Q loaded as fp32 and accumulated in f64 (o in 1, 3..10); dW, dOut as for xm_qw_dense */
int xm_qw_dense_f32(const float *dq32, int64_t n, int o, const double *dW, double *dOut, double alpha, void *stream);
/* the half-traffic symmetric pair on the fp32 copy (o in 3..5; allocates its scratch per call) */
int xm_qw_dense_sym_f32(const float *dq32, int64_t n, int o, const double *dW, double *dOut, double alpha, void *stream);
/* same product from 3x3-block CSR (device arrays; blocks row-major 9 doubles) */
int xm_qw_bsr3(const int64_t *d_rowptr, const int32_t *d_colidx, const double *d_blocks, int64_t n, int o,
               const double *dW, double *dOut, double alpha, void *stream);

/* A (host, column-major n x n, symmetric positive definite; lower triangle read) is overwritten by its inverse, computed on the device
 * (blocked Cholesky + triangular solves, xm-code_amd/csrc/xm_dense_la.hip): the set-up step of XM_STORAGE_SCHUR, which the reference
 * does on the host with scipy.linalg.solve (utils/creatematrix.py:260). */
int xm_spd_inverse(int64_t n, double *A);
/* B (host, column-major n x k) is overwritten by A^-1 B for A (host, column-major n x n, symmetric positive definite; only the lower
 * triangle is read), by the Cholesky factorisation and the two triangular substitutions of the dense Schur solver of xm_ctx_bundle_adjust
 * (xm_dense_la.hip).  XM_ERR_ARG: n outside [1, 46000], k < 1, null arrays, a pivot that is not positive or a non-finite solution. */
int xm_spd_solve(int64_t n, int64_t k, const double *A, double *B);
/* Test export (the xm_ctx_*_probe pattern, without a context): ONE host function of xm-code_amd/csrc/xm_dense_la.hip on host arrays.  The
 * arrays named for the operation are uploaded whole (padding between the rows and the leading dimension included), the function runs on
 * the null stream, the device is synchronised, and the in/out arrays come back whole -- what was not to be touched can be looked at.
 * Column-major unless stated.  info goes up with the caller's value and comes back (the kernels set it and never clear it).
 *
 *   op                       calls                    arrays
 *   XM_LA_GEMM_SUB           gemm_sub_device          C (ldc x n; in/out) -= op(A) op(B): op(A) m x k, op(B) k x n; A: lda x k (ta = 0) or lda x m
 *                                                     (ta = 1); B: ldb x n (tb = 0) or ldb x k (tb = 1); lower_only: the 64 x 64 tiles on and below
 *                                                     the diagonal only, the diagonal tiles whole
 *   XM_LA_CHOLESKY           spd_cholesky_device      A (lda x n; in/out): lower triangle read -> the factor L; zeros above the diagonal inside the
 *                                                     64 x 64 diagonal blocks, the other upper blocks untouched; info
 *   XM_LA_SUBSTITUTE         spd_substitute_device    A = L (lda x n; in), C = X (ldc x nrhs; in/out) <- (L L^T)^-1 X; info
 *   XM_LA_INVERSE            spd_inverse_device       A (n x n, lda = n; in/out) -> the factor; C = X (n x n, ldc = n; in/out) <- the LOWER
 *                                                     triangle of A^-1, scratch above the diagonal; info <- 0 when it returned true, 1 when it
 *                                                     refused (X then comes back as it went up)
 *   XM_LA_LAYOUT             spd_inverse_layout       A = X (n x n, lda = n; in), C = dst (ROW-major, n rows of ldc; in/out)
 *   XM_LA_RANK1_SUB          rank1_sub_device         A (n x n, lda = n; in/out) -= q u u^T, B = u (n; in)
 *
 * Fields an operation does not name are ignored.  XM_ERR_ARG, nothing written: a struct_size that is not sizeof, an unknown op, a null
 * array the operation names, m, n, k or nrhs outside [1, XM_LA_PROBE_MAX_N], ta, tb or lower_only outside {0, 1}, a leading dimension below
 * the rows it spans or above 2 XM_LA_PROBE_MAX_N, lda or ldc other than n where the table says so. */
#define XM_LA_PROBE_MAX_N 4096
#define XM_LA_GEMM_SUB 0
#define XM_LA_CHOLESKY 1
#define XM_LA_SUBSTITUTE 2
#define XM_LA_INVERSE 3
#define XM_LA_LAYOUT 4
#define XM_LA_RANK1_SUB 5
typedef struct {
    uint32_t struct_size;
    int32_t op;
    int32_t m, n, k, nrhs;
    int32_t ta, tb, lower_only;
    int32_t info;              /* in/out */
    int64_t lda, ldb, ldc;
    double q;
    double *A, *B, *C;
} xm_la_probe_t;
int xm_la_probe(xm_la_probe_t *probe);

/* Work decomposition of the half-traffic symmetric dense product (xm_qw_dense_sym, vertical sweep) for n cameras, host-only (CPU
 * test of the index arithmetic, tests/test_symv_layout.py): plan = { K steps (of two cameras) per chunk, Kf for the strip groups
 * dispatched last, first such group, chunks }. */
int xm_symv_plan(int64_t n, int32_t plan[4]);

/* Multi-rank symmetric dense product (xm-code_amd/csrc/xm_symw.h), host-only views for the CPU test tests/test_symw_plan.py: the work list of one
 * rank -- geom = {T, Th, tie, t0, nsteps, nstrips, K, number of items}, items: (strip, first step, end step) triples (NULL: sizes only) -- and the
 * predicate "row step t uses block (t, u)" of a matrix of T steps. */
int xm_symw_plan(int64_t ntot, int nloc, int cam0, int K, int32_t geom[8], int32_t *items);
int xm_symw_use(int T, int t, int u);
/* Test export (the xm_la_probe pattern: no context, host arrays that go up and come back whole): ONE rank's share of the multi-rank symmetric
 * product, kernel by kernel -- qw_symw_kernel + symw_colsum_kernel (SymwProduct::sweep), then symw_reduce_kernel with the plain epilogue
 * (SymwProduct::reduce) -- with every stage returned (tests/test_gpu_symw_stages.py).  The rank is cam0 / nloc of world ranks with
 * world * nloc == ntot, as a context sets them up; cameras in the padded numbering (ntot, nloc, cam0 even).
 *   in   o            1, 3, 4 or 5
 *        K            <= 0: the automatic chunk length, else the chunk length of the plan (xm_symw_plan); comes back as used
 *        nt           -1: the load policy the solver would choose, 0 / 1: the cached / non-temporal instantiation; comes back as used (0 / 1)
 *        scal_status  -1: no status word (null), 0: a status word that says "running", 1: one that says "stopped" -- the sweep and the
 *                     column sums then write nothing
 *        Q            this rank's strip, 3 nloc x 3 ntot, row-major, compact.  The probe lays it out at the leading dimension of the solver
 *                     (the next multiple of 128) and fills the padding columns with pad_value
 *        pad_value    FINITE.  The kernels mask a padding column by a product with zero (x * 0), never by a select, so whatever pads
 *                     a dense Q on the device must be finite: a NaN or an infinity there would reach every row of the strip
 *        W            3 ntot x o, row-major, compact
 *        cs_all       world x 3 ntot x o (in/out): the other ranks' column-sum vectors as the all-gather would deliver them; the slot of
 *                     this rank is overwritten by the device result
 *   out  (each filled when its pointer is not null; Prow, Pcol and this rank's slot of cs_all hold a quiet-NaN sentinel before the
 *        sweep, so a record that was never written shows)
 *        Prow         nstrips x 6 nsteps x o: the row-direction partial sums per (strip, local row)
 *        Pcol         max(items, 1) x 256 x o: the column sums per work item
 *        csum         3 ntot x o: this rank's column sums (the slot of cs_all)
 *        Y            3 nloc x o, compact: alpha * (row sums + every rank's column sums)
 *        nitems, nfull  work items of the plan; (item, step) pairs that take the unmasked path (symw_full)
 * XM_ERR_ARG, nothing written, before any device call: a struct_size that is not sizeof, o outside {1, 3, 4, 5}, ntot, nloc or cam0 odd or
 * out of order (cam0 + nloc > ntot, cam0 no multiple of nloc, world * nloc != ntot), ntot above XM_SYMW_PROBE_MAX_NTOT, nt outside
 * {-1, 0, 1}, scal_status outside {-1, 0, 1}, alpha or pad_value not finite, a null Q, W or cs_all. */
#define XM_SYMW_PROBE_MAX_NTOT 4096
typedef struct {
    uint32_t struct_size;
    int32_t ntot, nloc, cam0, world;
    int32_t o;
    int32_t K;                 /* in/out */
    int32_t nt;                /* in/out */
    int32_t scal_status;
    int32_t nitems, nfull;     /* out */
    double alpha, pad_value;
    const double *Q, *W;
    double *cs_all;            /* in/out */
    double *Prow, *Pcol, *csum, *Y;
} xm_symw_probe_t;
int xm_symw_probe(xm_symw_probe_t *probe);
/* Aggregates of the two-level preconditioner (xm_tuning_t.schur_solver = 3) for an observation list, host-only (CPU test): the cameras
 * 1..n-1 in breadth-first order over the camera-landmark graph from camera 0 (landmarks seen more than 64 times are not expanded), unreached
 * cameras appended, cut into runs of B (1..64; the solver uses 64).  agg_of_camera[n]: aggregate of every camera, -1 for camera 0.  More
 * than 4096 aggregates: XM_ERR_ARG. */
int xm_schur_aggregate_plan(int64_t n, int64_t nobs, const int32_t *cam, const int32_t *lm, int B, int32_t *agg_of_camera);
/* Aggregates of xm_ctx_bundle_adjust's opt-in preconditioners, host-only (CPU test): the cameras with a used observation (used[e] != 0; NULL =
 * every observation) in breadth-first order over the graph of the used observations from camera 0 (landmarks with more than 64 of them are
 * not expanded) -- or, when camera 0 is not an end of the capture, from the camera that search reaches last: the search is repeated from
 * there and kept unless camera 0 lies in its last level, so that the order runs along a trajectory on one front, not outwards from its
 * middle on two -- the members never reached appended in index order, cut into runs of B (1..64; the solver uses XM_BA_AGG_CAMS).  agg_of_camera[n]: the
 * aggregate of every camera, -1 for one without a used observation.  More than XM_BA_MAX_AGGREGATES aggregates: XM_ERR_ARG. */
int xm_ba_aggregate_plan(int64_t n, int64_t nobs, const int32_t *cam, const int32_t *lm, const uint8_t *used, int B, int32_t *agg_of_camera);
/* The Levenberg-Marquardt loop that xm_ctx_bundle_adjust, xm_ctx_global_positioning and xm_view_graph_calibrate share, run over a script
 * in place of a device, host-only (CPU test, tests/test_lm_loop.py); no time limit.  points (2 npoints): cost and |J^T r|_inf of every
 * point the loop reads, one consumed per read; steps (5 nsteps): cost_new, model (sum r.Jd + |Jd|^2 / 2: negative for a decrease), |d|^2,
 * |x|^2 and solved (0: the linear solve failed) of every candidate, one consumed per iteration.  mu and accepted (nsteps each): the
 * damping and the verdict of every iteration.  info[7]: status (XM_BA_*), iterations, accepted steps, points consumed, steps consumed,
 * which accepted step's point is the current one at the end and which one is returned (0: the start; they differ only with non-monotonic
 * steps).  radius: the trust-region radius at the end.  A script that runs out, or a null array: XM_ERR_ARG. */
int xm_lm_replay(int max_iters, double function_tol, double gradient_tol, double parameter_tol, int nonmonotonic, int max_nonmonotonic,
                 int64_t npoints, const double *points, int64_t nsteps, const double *steps, double *mu, uint8_t *accepted, int32_t info[7],
                 double *radius);
/* One linearisation of xm_ctx_bundle_adjust, a test export (tests/test_gpu_ba_stages.py): at the point (rot, t, p) (the layouts, context and
 * refusals of xm_ctx_bundle_adjust) and the damping mu > 0 it runs one eval + landmark pass + camera pass with the kernels, grids and
 * arguments of the LM loop (one workspace class serves both) and fills the scalars and every array whose pointer is not null; arrays per
 * landmark come by input index, CD = 3 with XM_BA_FIX_ROTATIONS, else 6; NC = 4 or 7.  flags: XM_BA_FIX_ROTATIONS, XM_BA_PRECOND_BLOCKS,
 * XM_BA_PRECOND_TWO_LEVEL (the others: XM_ERR_ARG); loss, loss_scale as in xm_ba_options_t.
 *   cost, n_used, gmax                       the state word after the passes
 *   b (CD n), g_l (3 m), vinv (6 m: the entries 00 01 02 11 12 22 of (V + mu D)^-1), ustar, sinv (CD CD n, row-major blocks), cused (n), lused (m)
 *   X (CD n x k, column-major, input) -> SX = S X by the matrix-free product, MX = M^-1 X for the selected preconditioner through the PCG's
 *                                            start (b := X_j, the init launch or launches, z read back)
 *   Sdense (CD n square, column-major)       the assembled lower block triangle before factorisation, the rest 0; CD n >
 *                                            XM_BA_PROBE_DENSE_MAX_ROWS: XM_ERR_ARG
 *   XM_BA_PRECOND_TWO_LEVEL: Pm (CD n x NC, row-major: every camera's rows of its coarse aggregate's scaled columns), dropped (NC ncoarse,
 *                                            1 = a column of norm 0), Ac (NC ncoarse square, column-major, the lower block triangle as assembled,
 *                                            before inversion; the caller sizes both for ncoarse <= ceil(n / XM_BA_AGG_CAMS)), coarse_ok (A_c was
 *                                            inverted); nagg, ncoarse (0 without the coarse space)
 *   dc (CD n, input) -> dP (3 m) = -V*^-1 (g_l + W^T dc), the candidate rot1, t1, p1 in the caller's layouts (members without a used
 *                                            observation: the input bits), cost1, model = sum r.(J d) + |J d|^2 / 2, step2, x2 (cameras, landmarks)
 * The context is only read.  Allocates and frees its workspace per call. */
#define XM_BA_PROBE_DENSE_MAX_ROWS 4096  /* a 134 MB matrix copied to the host */
typedef struct {
    uint32_t struct_size;
    uint32_t flags;
    int32_t loss, pad;
    double loss_scale, mu;
    int64_t k;
    const double *X, *dc;
    double cost, gmax, cost1, model, step2[2], x2[2];
    int64_t n_used;
    int32_t nagg, ncoarse, coarse_ok, pad2;
    double *b, *g_l, *vinv, *ustar, *sinv;
    int32_t *cused, *lused;
    double *SX, *Sdense, *MX, *Pm, *dropped, *Ac;
    double *dP, *rot1, *t1, *p1;
} xm_ba_probe_t;
int xm_ctx_ba_probe(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, xm_ba_probe_t *probe);
/* The same with focal scales (xm_ctx_bundle_adjust_focal; tests/test_gpu_ba_focal_stages.py): probe->flags must hold XM_BA_REFINE_FOCAL and
 * may hold XM_BA_FIX_ROTATIONS (a preconditioner flag: XM_ERR_ARG); the arrays are sized by CD = 7, or 4 with fixed rotations.  focal (n, > 0),
 * focal_free (n or NULL) as there.  focal1 (n or NULL): the candidate's focal scales when probe->dc is given; a candidate focal that is
 * not positive is reported as cost1 = NaN (the loop rejects that step as invalid). */
int xm_ctx_ba_probe_focal(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, const double *focal, const uint8_t *focal_free,
                          xm_ba_probe_t *probe, double *focal1);
/* The same with a radial coefficient behind the focal scale (xm_ctx_bundle_adjust_radial; tests/test_gpu_ba_radial_stages.py): probe->flags
 * must hold XM_BA_REFINE_FOCAL | XM_BA_REFINE_RADIAL and may hold XM_BA_FIX_ROTATIONS; the arrays are sized by CD = 8, or 5 with fixed
 * rotations.  dist (n, finite), dist_free (n or NULL) as there.  dist1 (n or NULL): the candidate's coefficients when probe->dc is given; a
 * candidate at which the radial map folds at a used observation is reported as cost1 = NaN, as a focal that is not positive is. */
int xm_ctx_ba_probe_radial(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, const double *focal, const uint8_t *focal_free,
                           const double *dist, const uint8_t *dist_free, xm_ba_probe_t *probe, double *focal1, double *dist1);
/* The same with focal groups (xm_ctx_bundle_adjust_focal_groups; tests/test_gpu_ba_groups_stages.py): ngroups, group_of, focal (ngroups),
 * focal_free (ngroups or NULL) as there.  b, the columns of X, SX and MX, and dc have CP n + G entries: CP = CD - 1 per camera, then the G
 * focal entries (0 comes back for an empty group).  ustar and sinv (CD CD n) are the blocks the device holds: U* with the focal diagonal
 * undamped; the inverse of the pose block of S_ii with the preconditioner's 1 / F_c in the focal slot of the group's first member and 0 in
 * the other members'.  The aggregate arrays have no meaning here and the struct keeps its size, so two of their pointers serve the groups:
 * dropped (G or NULL) receives D_c; Ac (or NULL) receives F: the exact block as assembled, G x G column-major, for G <=
 * XM_BA_FOCAL_GROUPS_EXACT (coarse_ok = 1 when it was inverted and the preconditioner uses it), else the G diagonal entries; Pm is ignored.
 * focal1 (G or NULL): the groups' candidate scales.  gmax sees the groups' gradient entries sum_i g_if.  Sdense (CP n + G square,
 * column-major): the lower triangle of the contracted matrix, the rest 0; CD n > XM_BA_PROBE_DENSE_MAX_ROWS: XM_ERR_ARG. */
int xm_ctx_ba_probe_focal_groups(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, int64_t ngroups, const int32_t *group_of,
                                 const double *focal, const uint8_t *focal_free, xm_ba_probe_t *probe, double *focal1);

/* ---- Global positioning: camera centres and points from rotations and 2-D tracks, without an initial value.  Step 5 of GLOMAP's pipeline
 * (controllers/global_mapper.cc:188-231), estimators/global_positioning.cc in its default ONLY_POINTS form, on the device over the observation
 * lists of an XM_STORAGE_SCHUR context.  NOTHING HERE WAS COMPARED WITH THE REFERENCE'S COMPILED CODE (it needs Ceres, COLMAP, Eigen and glog):
 * parity rests on a line-cited restatement (tests/xm_gp_numpy.py).
 *   input       rot (3 x 3n column-major, R_i camera-to-world, READ ONLY), t (3 x n, camera centres), p (3 x n_landmarks, world points): the
 *               layouts of xm_ctx_bundle_adjust.  t and p are host arrays; the call starts from them and updates them in place (xmamd.py's
 *               gp_random_start gives the reference's 100 U(-1, 1)^3, .cc:141, :235).  Of an observation's camera-frame point p_e only the
 *               bearing p_e / |p_e| is read.
 *   used        an observation e = (i, l) is used when its current weight is > 0, p_e2 > 0 (the bundle adjustment's rule) and landmark l has
 *               at least min_views observations that pass these two tests (0 = 3, global_positioning.h:33, .cc:119, :231).  Cameras,
 *               landmarks and scales that are not used come back bit-identical (scales: -1).
 *   residual    r_e = d_e - s_e (P_l - c_i) with d_e = R_i p_e / |p_e| (.cc:265-267, cost_function.h:26-29) and one scale s_e per used
 *               observation: 1 at the start (.cc:273), bounded below by 1e-5 (.cc:297).  No camera is held fixed (.cc:337-338).
 *   cost        F = 1/2 sum rho(|r_e|^2); loss, loss_scale as in xm_ba_options_t (the reference: XM_BA_LOSS_HUBER with 0.1,
 *               global_positioning.h:44-45); definitions, the clamp of rho' and the Corrector convention are those of xm_ctx_bundle_adjust.
 *   step        the Levenberg-Marquardt rules of xm_ctx_bundle_adjust word for word (radius, D = diag(J^T J) clamped to [1e-6, 1e32],
 *               acceptance at rho > 1e-3, radius updates, stops, trace record) over x = (c, P, s); |x|^2 of the parameter test is
 *               sum |c|^2 + sum |P|^2 + sum s^2 over what is used.  Elimination in Ceres's order (.cc:310-331): the scales in closed form
 *               (with w = rho', v = P_l - c_i, h* = w |v|^2 + mu clamp(w |v|^2), g_s = -w r.v:  M_e = w s^2 I - (w s)^2 v v^T / h*,
 *               q_e = w s (r + v g_s / h*)), then the landmarks (V_l = sum M_e, W_e = -M_e), then the cameras (U_i = sum M_e) by PCG from
 *               zero with the inverted 3 x 3 blocks of S to relative residual eta or 500 iterations; the damping of c and P is
 *               mu clamp(sum w s^2), the diagonal of the full J^T J.  ds_e = -(g_s - w s v.dc + w s v.dP) / h*.
 *   bound       DEPARTURE from Ceres (which projects the step and runs a line search): a scale with s_e <= 1e-5 whose gradient points
 *               outward (g_s > 0) is frozen for that iteration (its column of J is zero: M_e = w s^2 I, q_e = w s r, ds_e = 0), and the
 *               candidate is s <- max(s + ds, 1e-5).
 *   departures  the start is the caller's (the reference draws it from std::mt19937 in hash-map order); no NormalizeReconstruction; no Jacobi column
 *               scaling (as xm_ctx_bundle_adjust).  This entry is the ONLY_POINTS form with every camera calibrated; the other constraint
 *               types, the has_prior_focal_length down-weighting and the fixed-centre pass: xm_ctx_global_positioning_pairs below.
 * Options: struct_size = sizeof(xm_gp_options_t); max_iters, max_time, function_tol, gradient_tol, parameter_tol, min_views: 0 = the defaults
 * (100 and 1e-5: optimization_base.h:23, :25; 300 s, 1e-10, 1e-8, 3); eta is required and lies in (0, 1).  trace as in xm_ba_options_t.  scales
 * (may be NULL): nobs doubles in input order, -1 for an observation that is not used.
 * XM_ERR_ARG (context unchanged and usable): not XM_STORAGE_SCHUR, several ranks or GPUs, a wrong struct_size, null arrays, non-finite
 * input, eta outside (0, 1), negative settings, an unknown loss, a robust loss whose loss_scale is not finite and > 0, loss_scale != 0 with
 * the trivial loss, a non-finite initial cost.  The call reads the context and changes nothing in it (Q, weights, solver workspace).  The
 * workspace is allocated inside the call and freed before it returns.  Every sum over observations has a fixed order and no atomics are
 * used: two calls give the same bits. */
typedef struct {
    uint32_t struct_size;
    int32_t max_iters;
    double max_time, eta, function_tol, gradient_tol, parameter_tol;
    int32_t min_views;
    int32_t trace_cap;
    double *trace;
    int32_t loss;              /* XM_BA_LOSS_* */
    int32_t pad;
    double loss_scale;
} xm_gp_options_t;
typedef struct {
    uint32_t struct_size;
    int32_t status;            /* XM_BA_* */
    int32_t iters, accepted;
    int64_t pcg_iters, n_used;
    double initial_cost, final_cost, gradient_max, seconds;
    int32_t trace_len, pad;
} xm_gp_result_t;
int xm_ctx_global_positioning(xm_ctx_t *ctx, const xm_gp_options_t *opt, const double *rot, double *t, double *p, double *scales_or_null,
                              xm_gp_result_t *res);
/* One linearisation of xm_ctx_global_positioning, a test export (tests/test_gpu_gp_stages.py): at the point (t, p, s) (s: nobs scales in
 * input order, read where the observation is used; NULL = all 1) and the damping mu > 0 it writes the records and runs the landmark and
 * camera passes with the kernels, grids and arguments of the LM loop (one workspace class serves both) and fills the scalars and every
 * array whose pointer is not null; arrays per observation and per landmark come by input index.
 *   cost, n_used, gmax                       the state word after the passes (gmax: |J^T r|_inf over c, P and the scales that are not frozen)
 *   M (6 nobs: the entries 00 01 02 11 12 22 of M_e), q (3 nobs), frozen, oused (nobs)
 *   vinv (6 m: (V + mu D)^-1), g_l (3 m), ustar, sinv (9 n, row-major blocks), b (3 n), cused (n), lused (m)
 *   X (3n x k, column-major, input) -> SX = S X by the matrix-free product
 *   dc (3n, input) -> dP (3 m), ds (nobs), the candidate t1, p1, s1 in the caller's layouts (what is not used: the input bits, s1: -1), cost1,
 *                                            model = sum r.(J d) + |J d|^2 / 2, step2, x2 (cameras, landmarks, scales)
 * min_views, loss, loss_scale as in xm_gp_options_t.  The context is only read.  Allocates and frees its workspace per call. */
typedef struct {
    uint32_t struct_size;
    int32_t min_views;
    int32_t loss, pad;
    double loss_scale, mu;
    int64_t k;
    const double *s, *X, *dc;
    double cost, gmax, cost1, model, step2[3], x2[3];
    int64_t n_used;
    double *M, *q;
    int32_t *frozen, *oused;
    double *vinv, *g_l, *ustar, *sinv, *b;
    int32_t *cused, *lused;
    double *SX, *dP, *ds, *t1, *p1, *s1;
} xm_gp_probe_t;
int xm_ctx_gp_probe(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, xm_gp_probe_t *probe);
/* constants of the kernels, host-only (the tests size their edge cases from them): out[0] = a landmark with more observations than this
 * has a workgroup of its own, out[1] = observations a wavefront takes from a camera's list in one pass, out[2] = threads of that workgroup */
int xm_gp_limits(int64_t out[3]);

/* ---- Global positioning with camera-to-camera constraints, per-camera weights and a fixed-centre point pass: the other three constraint
 * types of estimators/global_positioning.cc (ONLY_CAMERAS, POINTS_AND_CAMERAS, POINTS_AND_CAMERAS_BALANCED, .cc:53-60) and the second pass
 * of controllers/global_mapper.cc:205-217 (optimize_positions = false).  Everything xm_ctx_global_positioning states holds word for word
 * (input layouts, used observations, loss, LM rules, bound, PCG, stops, trace, refusals, fixed-order sums, f64); what is added:
 *   pairs       pi, pj (image_id1, image_id2), trel (3 npairs: the translation of cam2_from_cam1, used as given), valid (npairs bytes, NULL =
 *               all valid): the conventions of xm_view_graph_filter and xm_view_graph_rotations.  A pair takes part when it is valid
 *               (.cc:152).  pi == pj or an index outside [0, n) is XM_ERR_ARG, for every pair named.
 *   residual    r_m = tau_m - sigma_m (c_j - c_i) with tau_m = -R_j trel_m (.cc:165-175; R_j = rot of image_id2, camera-to-world; position1 =
 *               c_i, position2 = c_j) and one scale sigma_m per participating pair: 1 at the start, bounded below by 1e-5 (.cc:163, :177) by
 *               the active-set rule of the observation scales.  Loss: the plain loss of the options (.cc:172), never weighted.
 *   weights     of the observation terms (.cc:201-228, :283-295): rho and rho' are multiplied by a_e (Ceres's ScaledLoss).
 *               weight_scale_pt = reweight_scale * (participating pairs) / (landmarks of the context) for BALANCED with at least one
 *               participating pair, else 1.  The divisor is ALL landmarks of the context, as the reference divides by tracks.size()
 *               (.cc:193), not the used ones.  a_e = weight_scale_pt for a calibrated camera (1 unless BALANCED) and 0.5 weight_scale_pt for
 *               one with calibrated[i] == 0, in every type that has observation terms.  calibrated: n bytes, NULL = all calibrated.
 *   terms       XM_GP_ONLY_POINTS: observations; XM_GP_ONLY_CAMERAS: pairs -- no observation is used, p comes back bit-identical and every
 *               scale -1; the two mixed types: both.  A type with pair terms and no participating pair is XM_ERR_ARG (.cc:32-36).
 *   used        a camera is used when it has a used observation (where observation terms exist) or a participating pair (where pair terms
 *               exist), .cc:108-127.  Everything else comes back with the caller's bits.
 *   elimination pair scales in closed form like observation scales: with v = c_j - c_i, w = rho', h* = w |v|^2 + mu clamp(w |v|^2),
 *               g_sigma = -w r.v:  M_m = w sigma^2 I - (w sigma)^2 v v^T / h*,  q_m = w sigma (r + v g_sigma / h*).  M_m enters the reduced
 *               camera system directly: S_ii += M_m, S_jj += M_m, S_ij = S_ji = -M_m; q_m enters the gradient of i with the camera's sign
 *               and of j with the point's.  Camera damping mu clamp(sum_obs a w s^2 + sum_pairs w sigma^2): one clamp of the whole diagonal.
 *               d sigma_m = -(g_sigma - w sigma v.dc_i + w sigma v.dc_j) / h*.  |x|^2 and |step|^2 add sigma^2 and d sigma^2; the gradient
 *               test sees g_sigma of the pairs that are not frozen.  The PCG's 3 x 3 blocks of S_ii include the pair terms.
 *   fixed       XM_GP_FIX_CENTRES (with XM_GP_ONLY_POINTS only, anything else is XM_ERR_ARG): the centres are constants, t is read only and
 *               comes back bit-identical; no camera pass and no PCG, dP_l = -V*_l^-1 g_l; |x|^2 and |step|^2 count points and scales only;
 *               the gradient test sees points and scales.
 * With XM_GP_ONLY_POINTS, no flag and calibrated NULL the call launches what xm_ctx_global_positioning launches and returns its bytes.
 * xm_gp_pairs_t: struct_size = sizeof; reweight_scale 0 = 1.0 (negative or non-finite: XM_ERR_ARG); sigma (out, may be NULL): npairs doubles,
 * -1 for a pair that takes no part.  Outputs: pairs_used, cams_heavy (cameras whose incidence list a workgroup walks), max_incidences,
 * weight_scale_pt.  NOTHING HERE WAS COMPARED WITH THE REFERENCE'S COMPILED CODE: parity rests on tests/xm_gp_pairs_numpy.py. */
#define XM_GP_ONLY_POINTS                  0
#define XM_GP_ONLY_CAMERAS                 1
#define XM_GP_POINTS_AND_CAMERAS_BALANCED  2
#define XM_GP_POINTS_AND_CAMERAS           3
#define XM_GP_FIX_CENTRES                  1u
typedef struct {
    uint32_t struct_size;
    int32_t constraint;        /* XM_GP_ONLY_POINTS ... */
    uint32_t flags;            /* XM_GP_FIX_CENTRES */
    int32_t pad;
    int64_t npairs;
    const int32_t *pi, *pj;
    const double *trel;
    const uint8_t *valid, *calibrated;
    double reweight_scale;
    double *sigma;
    int64_t pairs_used, cams_heavy, max_incidences;
    double weight_scale_pt;
} xm_gp_pairs_t;
int xm_ctx_global_positioning_pairs(xm_ctx_t *ctx, const xm_gp_options_t *opt, xm_gp_pairs_t *pairs, const double *rot, double *t, double *p,
                                    double *scales_or_null, xm_gp_result_t *res);
/* One linearisation of xm_ctx_global_positioning_pairs, a test export (tests/test_gpu_gp_pairs_stages.py): xm_ctx_gp_probe with the terms
 * that `pairs` selects, through the workspace class and the launches of the LM loop.  probe is filled as by xm_ctx_gp_probe: cost, cost1,
 * model, step2 and x2 from the observation terms alone, gmax over everything the loop's gradient test sees, ustar / sinv / b / SX with the
 * pair terms in them; with XM_GP_FIX_CENTRES dc is taken as 0 and k must be 0.  pair_probe: sigma_in (npairs, read where the pair takes
 * part, NULL = all 1) -> the pairs' cost, gsmax (max |g_sigma| over the pairs that are not frozen), cost1, model, step2, x2, and per pair in
 * input order Mp (6 npairs: 00 01 02 11 12 22), qp (3 npairs), pfrozen, pused, dsigma and sigma1 (-1 where the pair takes no part). */
typedef struct {
    uint32_t struct_size;
    int32_t pad;
    const double *sigma_in;
    double cost, gsmax, cost1, model, step2, x2;
    double *Mp, *qp;
    int32_t *pfrozen, *pused;
    double *dsigma, *sigma1;
} xm_gp_pair_probe_t;
int xm_ctx_gp_probe_pairs(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, xm_gp_probe_t *probe, xm_gp_pairs_t *pairs,
                          xm_gp_pair_probe_t *pair_probe);
/* out[0] = a camera with more incidences (ends of participating pairs) than this has a workgroup of its own, out[1] = threads of it */
int xm_gp_pair_limits(int64_t out[2]);
/* The trust region's kernels stage by stage, a test export (tests/test_gpu_rtr_stages.py): at the point (R: 3n x o column-major, s: n; s[0] is
 * forced to 1 as in a solve) and with lam, the stages below run through the context's own setup for rank o, its product dispatch and the
 * launchers, grids and arguments of a solve -- the kernels are those the storage and xm_tuning_t select (product_kind: XM_PRODUCT_*; split_k: slices of
 * the column-split dense product in effect at this rank, 1 = not split; sell_gather: gather mode of the sliced-ELL kernels, 0 a record per lane | 1 LDS-transposed, -1 without that layout).  Every
 * array whose pointer is not null is filled; matrices are 3n x o column-major, vectors n.  Single-rank contexts only (XM_ERR_ARG otherwise, and
 * for o outside 3..10 (a point needs three orthonormal rows), non-finite input, a wrong struct_size, XM_RTR_PROBE_AUTO where the device-driven outer iteration does not apply).
 *   grad (always)      scale_rows, the EPI_GRAD product, outer_finalize -> f, rr = <rg,rg>, G = 2 Q sR, egs, S0 (9 n, row-major blocks), rgR, rgs
 *   hess (pR, ps given; rR, rs optional = 0)   W = s.*pR + ps.*R (anchor's ps taken as 0, written by the tCG's own start kernel), the EPI_HESS
 *                      product -> HpR, Hps and pHp = <p,Hp>, rHp = <r,Hp>, HpHp = <Hp,Hp>: the per-workgroup partial sums (nA each) added by
 *                      the summation tree cg_step_kernel uses.  hess_f32 contexts: the fp32 launch
 *   XM_RTR_PROBE_AUTO  both stages through the role-switching EPI_AUTO instantiation (TcgScal.phase = PH_CAND / PH_TCG)
 *   XM_RTR_PROBE_TCG_INIT  tcg_init_kernel from the grad stage's rg and rr with scal_in.delta -> init_* (init_W / init_Wpad: the product input
 *                      at its native pitch / at the 16-double record pitch (16 n); w_native / wpad say which of the two this context's tCG keeps)
 *   XM_RTR_PROBE_CG_STEP (needs hess)  one cg_step_kernel launch from scal_in (rr, vv, vp, pp, delta, gradnorm, model, iter; status 0), p, r,
 *                      v = (vR, vs), Hv = (HvR, Hvs; none with XM_RTR_PROBE_MODEL_REC = XM_FLAG_MODEL_RECURRENCE), Hp and the three sums as
 *                      the hess stage left them on the device, and for scal_in.iter > 0 partsB_in (partsB_in_count == nB partial sums of
 *                      |r|^2, as partsB_out of the launch before) -> scal_out, out_* (arrays a branch does not write come back with their
 *                      input bits), partsB_out (up to 1024 doubles, nB used) and rr_parts, their sum by the same tree
 *   XM_RTR_PROBE_CERT  cert_prepare_kernel at the point -> Lam (9 n), dz (n), dual[2] = the two sums (y0 + y3 + y5 of the anchor; lam sum(1 - xii^2));
 *                      with X (3n x k column-major): SX = S X, column by column through the EPI_CERT product
 * Solver state: the next solve on the context gives the bits it would have given without the call (the workspace is re-created by every
 * solve); the resident end point of an earlier solve is gone (as after xm_ctx_qw).  Allocates only the grow-only workspace of a solve at rank o. */
#define XM_RTR_PROBE_AUTO      1u
#define XM_RTR_PROBE_MODEL_REC 2u
#define XM_RTR_PROBE_TCG_INIT  4u
#define XM_RTR_PROBE_CG_STEP   8u
#define XM_RTR_PROBE_CERT      16u
typedef struct {
    double rr, vv, vp, pp, delta, gradnorm, last_step, model;
    int32_t status, iter;
} xm_rtr_scal_t;
typedef struct {
    uint32_t struct_size;
    uint32_t flags;
    int32_t o, k;
    double lam;
    const double *R, *s, *pR, *ps, *rR, *rs, *vR, *vs, *HvR, *Hvs, *partsB_in, *X;
    int32_t partsB_in_count, pad;
    xm_rtr_scal_t scal_in;
    int32_t product_kind, nA, nB, w_native, wpad, split_k, sell_gather, pad2;
    double f, rr, pHp, rHp, HpHp, rr_parts, dual[2];
    xm_rtr_scal_t init_scal, scal_out;
    double *G, *egs, *S0, *rgR, *rgs, *HpR, *Hps;
    double *init_rR, *init_rs, *init_pR, *init_ps, *init_vR, *init_vs, *init_HvR, *init_Hvs, *init_W, *init_Wpad;
    double *out_vR, *out_vs, *out_HvR, *out_Hvs, *out_rR, *out_rs, *out_pR, *out_ps, *out_W, *out_Wpad, *partsB_out;
    double *Lam, *dz, *SX;
} xm_rtr_probe_t;
int xm_ctx_rtr_probe(xm_ctx_t *ctx, xm_rtr_probe_t *probe);
/* The other half of an outer iteration stage by stage, a test export (tests/test_gpu_outer_stages.py): the retraction with the model decrease
 * it delivers, and one step launch of the device-driven outer iteration.  As xm_ctx_rtr_probe: the context's own setup for rank o, its product
 * dispatch, the launchers, grids and arguments of a solve (the step launch's arguments come from the function a solve takes them from);
 * matrices 3n x o column-major, vectors n; every array whose pointer is not null is filled; single-rank contexts only (XM_ERR_ARG otherwise, and
 * for o outside 3..10, non-finite input, a wrong struct_size, XM_OUTER_PROBE_STEP where the device-driven outer iteration does not apply).
 * The gradient stage runs first at (R, s) as in xm_ctx_rtr_probe (through the EPI_AUTO launch with XM_OUTER_PROBE_AUTO and with
 * XM_OUTER_PROBE_STEP) -> f, rr, rgR, rgs.  The retraction is the context's (that of its last solve), or XM_OUTER_PROBE_POLAR / _MGS; polar says which.
 *   XM_OUTER_PROBE_RETRACT     launch_retract_model of the step v = (vR, vs; vs[0] taken as 0) with Hv = (HvR, Hvs) and the gradient stage's rg,
 *                      then outer_finalize_kernel -> ret_Rc, ret_sc, ret_W (native pitch) and ret_Wpad (16 n; w_native / wpad say which the
 *                      context keeps), ret_partsM (up to 1024, nM used), model = the sum the result kernel hands to the host.
 *                      With XM_OUTER_PROBE_MODEL_REC the launch runs without Hv: ret_partsM keeps what the caller put there, model = scal_in.model
 *   XM_OUTER_PROBE_RETRACT_LS  launch_retract(D, no ds, t, no sout): the line search's form -> ls_Rc, ls_W
 *   XM_OUTER_PROBE_STEP        one outer_step_kernel launch from scal_in (all fields), os_in, delta_bar, gradtol, max_outer, stop_req and the tCG
 *                      vectors p, r, v, Hv (none with _MODEL_REC); slot: the launch pair's index (its parity picks the parity copies and the sweep direction).
 *                      scal_in.phase 0 (PH_TCG): the EPI_AUTO Hessian product of p first -> HpR, Hps, pHp, rHp, HpHp; scal_in.iter > 0 needs
 *                      partsB_in (nB).  1 (PH_CAND): the candidate (Rc, sc) and partsM_in (one partial per wavefront of 64 cameras) are given;
 *                      the EPI_AUTO product in its gradient role at the candidate first -> cand_G .. cand_rgs, f_cand, rr_cand (the two sums by
 *                      the result kernel's tree) and m_cand (the partials regrouped four by four and summed by the same tree; scal_in.model with
 *                      _MODEL_REC).  3 (PH_INIT), 2 (PH_STOP): the launch alone.
 *                      -> scal_out, os_out, progress (run: the run number in it), trace (record os_in.k + 1; trace_written says whether the launch
 *                      wrote it), grid, nwave, and out_*: every array the launch may write (those a role leaves alone come back with their
 *                      input bits; the candidate's buffers start as a copy of the point unless given)
 * Pad columns (even ranks: the pitch is o + 1): before a retraction the pad column of every copy it writes holds ones; ret_pad / ls_pad / out_pad
 * (scal_in.phase 0 only) count the entries that are not zero afterwards in Rc, W and the padded copy (-1: the context keeps no such copy).
 * Solver state: as after xm_ctx_rtr_probe. */
#define XM_OUTER_PROBE_RETRACT    1u
#define XM_OUTER_PROBE_MODEL_REC  2u
#define XM_OUTER_PROBE_RETRACT_LS 4u
#define XM_OUTER_PROBE_STEP       8u
#define XM_OUTER_PROBE_POLAR      16u
#define XM_OUTER_PROBE_MGS        32u
#define XM_OUTER_PROBE_AUTO       64u
typedef struct {
    double rr, vv, vp, pp, delta, gradnorm, last_step, model;
    int32_t status, iter, seq, phase;
} xm_outer_tcg_t;
typedef struct {
    double loss, rr_point;
    int64_t totalite;
    int32_t shrink_count, k, stop_reason, time_up, slots, pad;
} xm_outer_scal_t;
typedef struct {
    uint32_t struct_size;
    uint32_t flags;
    int32_t o, slot;
    double lam, t;
    const double *R, *s, *vR, *vs, *HvR, *Hvs, *D, *pR, *ps, *rR, *rs, *Rc, *sc, *partsB_in, *partsM_in;
    int32_t partsB_in_count, partsM_in_count;
    xm_outer_tcg_t scal_in;
    xm_outer_scal_t os_in;
    double delta_bar, gradtol;
    int32_t max_outer, stop_req;
    int32_t product_kind, nA, nB, nM, w_native, wpad, polar, grid, nwave, trace_written;
    uint32_t run, pad;
    int32_t ret_pad[3], ls_pad[2], out_pad[2], pad2;
    double f, rr, model, pHp, rHp, HpHp, f_cand, rr_cand, m_cand;
    uint64_t progress;
    xm_outer_tcg_t scal_out;
    xm_outer_scal_t os_out;
    double trace[6];
    double *rgR, *rgs, *ret_Rc, *ret_sc, *ret_W, *ret_Wpad, *ret_partsM, *ls_Rc, *ls_W, *HpR, *Hps;
    double *cand_G, *cand_egs, *cand_S0, *cand_rgR, *cand_rgs;
    double *out_R, *out_s, *out_Rc, *out_sc, *out_vR, *out_vs, *out_HvR, *out_Hvs, *out_rR, *out_rs, *out_pR, *out_ps, *out_W, *out_Wpad;
    double *out_partsB, *out_partsM, *out_G, *out_egs, *out_S0, *out_rgR, *out_rgs;
} xm_outer_probe_t;
int xm_ctx_outer_probe(xm_ctx_t *ctx, xm_outer_probe_t *probe);
/* The certificate's Lanczos eigen-solver, a test export (tests/test_gpu_cert_stages.py): at the point (R: 3n x o column-major, s: n; s[0] taken
 * as 1) and with lam, the context's setup for rank o, the certificate's right-hand side and cert_prepare_kernel as in a solve (the code a solve
 * runs), then Context::lanczos_min itself with cert_dense_rows, lanczos_mmax and lanczos_restarts of the context's xm_tuning_t.  Single-rank
 * contexts only (XM_ERR_ARG otherwise, and for o outside 3..10, non-finite input, a wrong struct_size).
 *   -> ret (lanczos_min's return value: 0 converged, 1 not), eig_exact (XM_CERT_EIG_EXACT would be set), theta, resid (the Ritz residual
 *      |beta_{m-1} y_{m-1}|), iters (steps of all restart cycles), m_use (size of the tridiagonal matrix theta and y come from), cycles (restart
 *      cycles run), mmax (steps a cycle can take: min(3n, max(2, lanczos_mmax))), steps_dev (steps the LAST cycle ran on the device: the host
 *      looks every eight steps, so m_use <= steps_dev), steps_fused / steps_unfused (steps of all cycles through the two forms of a step),
 *      len (length of the replicated vectors, >= 3n) and nseg (segments a dot product over len is cut into), product_kind (XM_PRODUCT_*),
 *      Lam (9 n), dz (n), dual[2] as xm_ctx_rtr_probe
 *   and, from what the last cycle left on the device, into arrays of the caller sized for cap steps (a null pointer skips one; XM_ERR_ARG, with
 *   the scalars above filled, if mmax > cap and any array is given):
 *      alpha, beta (mmax each; steps_dev filled), V (3n x (mmax + 1) column-major, columns 0..steps_dev filled, the padding rows dropped),
 *      c1, c2 (mmax each: the Gram-Schmidt coefficients of the two passes of step steps_dev - 1, steps_dev filled), y (mmax; m_use filled:
 *      the tridiagonal matrix's eigenvector as the Ritz vector's kernel read it), x (3n: the normalised Ritz vector in global camera order)
 *   XM_CERT_PROBE_UNFUSED  every step takes the form a solve uses beyond 1024 Lanczos columns (no solve sets this)
 * Solver state: as after xm_ctx_rtr_probe. */
#define XM_CERT_PROBE_UNFUSED 1u
typedef struct {
    uint32_t struct_size;
    uint32_t flags;
    int32_t o, cap;
    double lam;
    const double *R, *s;
    int32_t ret, eig_exact, iters, m_use, cycles, mmax, steps_dev, steps_fused, steps_unfused, nseg, product_kind, pad2;
    int64_t len;
    double theta, resid, dual[2];
    double *Lam, *dz, *alpha, *beta, *V, *c1, *c2, *y, *x;
} xm_cert_probe_t;
int xm_ctx_cert_probe(xm_ctx_t *ctx, xm_cert_probe_t *probe);
/* The matrix-free Q (XM_STORAGE_SCHUR) stage by stage, a test export (tests/test_gpu_schur_stages.py): the layout of the packed landmark
 * lists, the set-up factors as the last set_weights left them, what one product leaves behind in every stage of the factor chain, and the
 * pieces of the inner CG.  Single-GPU, single-rank XM_STORAGE_SCHUR contexts only (XM_ERR_ARG otherwise, and for a wrong struct_size, flags
 * != 0, non-finite input, o or k outside 0, 1, 3..10 -- the ranks the kernels are instantiated for --, an array the context's form does not
 * have: dinv, VX, pAp, MX without the CG form, VTinv with it, perm, binv, ainv without the two-level preconditioner).  Every array whose
 * pointer is not null is filled; arrays per landmark come by INPUT landmark index (the device numbers landmarks by degree), matrices are
 * column-major, n1 = n - 1 (the reduced cameras 1..n-1), m landmarks.
 *   layout   nheavy (landmarks with more than 64 observations: a workgroup each), lm_total (entries of the packed by-landmark arrays, padding
 *            included), deg (m: observations per landmark as the device holds them), uses_cg, two_level, nagg (aggregates of 64 cameras),
 *            dup_pairs (1: set_weights takes the host assembly -- a (camera, landmark) pair named twice, or xm_tuning_t.schur_host_assembly)
 *   set-up   Q1 (9 n, row-major 3 x 3 blocks: sum w p p^T), c (3 n: sum w p), q2 (n: sum w), q3inv (m: 1 / sum w, 0 for a landmark without
 *            weight); CG form: dinv (n1: 1 / diag VT); dense form: VTinv (n1 x n1, from the padded layout the product reads; n1 >
 *            XM_SCHUR_PROBE_DENSE_MAX_ROWS: XM_ERR_ARG); two-level: perm (64 nagg: reduced camera at each row of each aggregate, -1 = padding),
 *            binv (64 x 64 x nagg: VT_aa^-1, padding rows the identity), ainv (nagg x nagg: (P^T VT P)^-1)
 *   chain    W (3n x o, input; o = 0: none) -> one SchurOp::product with the plain epilogue and alpha, then the scratch vectors it wrote:
 *            h (m x o), r (n1 x o), xc (n1 x o), xl (m x o), and Y (3n x o) = alpha Q W.  CG form: pcg_done, pcg_iters, pcg_relres (the state
 *            word the product's inner solve ended with), pcg_tol and pcg_cap (the relative residual it asks for, the iteration cap)
 *   CG form  X (n1 x k, input; k = 0: none) -> MX = M^-1 X through the PCG's start (b := X; the init launch, then for the two-level form the block
 *            and coarse launches; p read back), VX = VT X through the operator's two launches with p := X, pAp (k) = <p, VT p>: the camera
 *            pass's per-workgroup partial sums added by the tree pcg_upd_kernel uses.  All through the functions the product's solve calls.
 * The context is only read: the factors are untouched, the statistics of xm_ctx_schur_info are restored, and a later product or solve gives the
 * bits it would have given without the call.  Allocates the grow-only scratch of a product at o and k columns. */
#define XM_SCHUR_PROBE_DENSE_MAX_ROWS 4096  /* a 134 MB matrix copied to the host */
typedef struct {
    uint32_t struct_size;
    uint32_t flags;
    int32_t o, k;
    double alpha;
    const double *W, *X;
    int64_t nheavy, lm_total, nagg;
    int32_t uses_cg, two_level, dup_pairs, pcg_done, pcg_iters, pcg_cap;
    double pcg_relres, pcg_tol;
    int32_t *deg, *perm;
    double *Q1, *c, *q2, *q3inv, *dinv, *VTinv, *binv, *ainv;
    double *h, *r, *xc, *xl, *Y;
    double *VX, *pAp, *MX;
} xm_schur_probe_t;
int xm_ctx_schur_probe(xm_ctx_t *ctx, xm_schur_probe_t *probe);
/* Smallest eigenpair of the symmetric tridiagonal matrix with diagonal a[0..m) and off-diagonal b[0..m-1), by the certificate's own host code
 * (Sturm bisection to an interval of 4e-16 max(1, tmax), inverse iteration): *theta, y[0..m) (unit norm), *tmax = the Gershgorin bound of |T|.
 * Host only, a test export (tests/test_tridiag_min.py). */
int xm_tridiag_min(const double *a, const double *b, int m, double *theta, double *y, double *tmax);
/* Large block-sparse Q: "sliced ELL over per-XCD column slabs" (xm-code_amd/csrc/xm_sell.h).  Same product as xm_qw_bsr3
 * (the reference has no sparse product: Dense/matmul.h:42-87 on a dense Q); the matrix is described on the HOST as 3x3-block CSR
 * (rows n, global columns in [0, ncols)) and re-laid on the device.  slabs in {1,2,4,8}; lmax = longest virtual row (hub
 * cameras are cut); gather_mode 0 (a record of W per lane) | 1 (LDS-transposed, the solver's default) selects how the rows of W are fetched.  xm_sell_layout is host-only (CPU tests): with
 * NULL arrays it fills sizes = {slices, steps, partial results, virtual rows, entries of the partial-result array}. */
int xm_sell_layout(const int64_t *rowptr, const int32_t *colidx, int64_t n, int64_t ncols, int slabs, int lmax, int64_t sizes[5],
                   int64_t *slice_off, int32_t *slab_start, uint8_t *kind, int64_t *src, int32_t *pslot, int64_t *pptr, int32_t *ridx);
int xm_sell_create(const int64_t *rowptr, const int32_t *colidx, const double *blocks, int64_t n, int64_t ncols, int slabs, int lmax,
                   void **handle);
/* the same with a block codec (xm-code_amd/csrc/xm_sell.h): codec 0 = 9 doubles per block, 1 = view-graph codec (off-diagonal blocks
 * -w * rotation stored as 4 doubles, diagonal blocks d * I as one double per camera; XM_ERR_ARG when the matrix is not of that form).
 * row0 = global camera index of row 0 (which column is "the diagonal"). */
int xm_sell_create2(const int64_t *rowptr, const int32_t *colidx, const double *blocks, int64_t n, int64_t ncols, int slabs, int lmax,
                    int codec, int64_t row0, void **handle);
/* host-only: distinct 128-byte lines of W the 64 lanes of a step touch, summed over every 4th step -- records of 72 bytes (o = 3), of 120 bytes
 * (o = 4, 5) at their native pitch, and at the 128-byte pitch: the figures behind the automatic choice of xm_tuning_t.sell_wpad */
int xm_sell_locality(const int64_t *rowptr, const int32_t *colidx, int64_t n, int64_t ncols, int slabs, int lmax, int64_t lines[3]);
/* host-only: block (row-major 3x3, -w * rotation) -> stored quaternion -> the block the product kernel rebuilds (CPU test of the codec) */
int xm_sell_quat_roundtrip(const double block[9], double quat[4], double rebuilt[9]);
void xm_sell_destroy(void *handle);
int xm_qw_sell(void *handle, int o, const double *dW, double *dOut, double alpha, int gather_mode, void *stream);
/* the same products with the input ALSO given at a record pitch of 16 doubles (dWpad16[cam * 16 + e] = dW[cam * 3 * pitch + e]; o = 3..5, layout 1;
 * NULL = not given): the gather reads one 128-byte line per camera.  Inside the solver the kernels that write the product input of the truncated
 * CG write that copy as well (xm_tuning_t.sell_wpad). */
int xm_qw_sell_padded(void *handle, int o, const double *dW, const double *dWpad16, double *dOut, double alpha, int gather_mode, void *stream);
/* per-camera kernels (device, row-major 3n x o; s: n):
 * Rout = MGS_rows(R + t*D) (Dense/batchedQR.h:42-67), sout = s*exp(t*ds/s) (trustregion.h:19-24), s[0] stays 1 */
int xm_retract(int64_t n, int o, const double *dR, const double *ds, const double *dD, const double *dds, double t,
               double *dRout, double *dsout, void *stream);
/* the same with the polar retraction (XM_RETRACT_POLAR): Rout_i = (M M^T)^{-1/2} M, M = R_i + t D_i */
int xm_retract_polar(int64_t n, int o, const double *dR, const double *ds, const double *dD, const double *dds, double t,
                     double *dRout, double *dsout, void *stream);
/* Solution recovery, the step right after the solve (replaces the rotation/scale part of
 * utils/recoversolution.py:recover_XM, lines 12-86): R (3n x r column-major) and s (n) as written to R.bin / s.bin ->
 * rot: 3 x 3n column-major, block i = the anchored orthogonal 3x3 of camera i (block 0 = identity), scale: n.
 * n_negative_det (optional) = cameras whose block had negative determinant before the majority sign flip. */
int xm_recover_rotations(int64_t n, int r, const double *R, const double *s, double *rot, double *scale, int *n_negative_det);

/* ================================================================== 4. multi-GPU row partition (one process per GPU) */
/* 128-byte unique id of the RCCL communicator: rank 0 calls xm_comm_unique_id and broadcasts the bytes
 * (bench.py does that with torch.distributed); every rank then calls xm_comm_init before xm_ctx_create. */
int xm_comm_unique_id(unsigned char id[128]);
int xm_comm_init(int rank, int world, int device, const unsigned char id[128], const char *rccl_path /* NULL = default search */);
/* Which transport joins the ranks of a context -- *kind: 0 none (one GPU), 1 RCCL all-gathers, 2 shared-memory TEST transport, 3 direct peer
 * writes between the host threads of this process (xm_problem_t.n_gpus), 4 direct peer writes between processes (IPC-mapped buffers) -- and,
 * in note (NUL-terminated, truncated to note_cap), why a faster transport was given up for it (empty: first choice).  The multi-GPU modes try
 * direct peer writes first (self-tested on the machine at context creation), then RCCL, and fail with XM_ERR_COMM naming both reasons. */
int xm_ctx_transport(xm_ctx_t *ctx, int *kind, char *note, size_t note_cap);
/* *on = 1 when the truncated CG of the last solved rank kept its product input at the 128-byte record pitch as well (xm_tuning_t.sell_wpad) */
int xm_ctx_sell_wpad(xm_ctx_t *ctx, int *on);
/* which product kernel serves the tCG of this context at rank o (3..10): XM_PRODUCT_* below */
#define XM_PRODUCT_DENSE       0   /* qw_dense_kernel */
#define XM_PRODUCT_DENSE_SYM   1   /* half-traffic symmetric dense product (one GPU: qw_symv_kernel; several: the cyclic half window) */
#define XM_PRODUCT_BSR3        2   /* qw_bsr3_kernel (3x3-block CSR, one launch) */
#define XM_PRODUCT_SELL        3   /* sliced ELL, 9 doubles per block (two launches) */
#define XM_PRODUCT_SELL_QUAT   4   /* sliced ELL, view-graph codec */
#define XM_PRODUCT_SCHUR       5   /* matrix-free factor chain */
int xm_ctx_product_kind(xm_ctx_t *ctx, int o, int *kind);

/* One process per GPU WITHOUT a collective library on the data path: every rank exports its exchange buffers as hipIpcMemHandle_t
 * through the POSIX shared-memory segment `name` (same string on every rank of the node, unique per job), maps the peers' and uses
 * the direct peer-write exchange of the single-process mode (fused into the tCG kernel).  xm_comm_init tries the same transport on
 * its own (segment name derived from the unique id) and keeps RCCL when any rank cannot map a peer, the transport's self-test
 * fails, the ranks span several nodes, or XM_COMM_PEER=0; this entry point has no fallback: XM_ERR_COMM instead.
 * spin_seconds <= 0: default bound (20 s) of the device-side waits.  Two ranks may share one GPU (tests). */
int xm_comm_init_ipc(int rank, int world, int device, const char *name, double spin_seconds);
/* TEST transport: the same collectives through a POSIX shared-memory segment, so several ranks can share one GPU on a
 * 1-GPU box (tests/test_gpu_parity.py::test_two_ranks_one_gpu); `bytes` = capacity of the exchange area */
int xm_comm_init_shm(int rank, int world, int device, const char *name, size_t bytes);
int xm_comm_finalize(void);
/* contiguous camera range [*c0, *c1) owned by `rank` for DENSE storage: equal ranges of ceil(n / world) cameras (the last rank is
 * padded with inert cameras inside the solver) */
int xm_partition(int64_t n, int world, int rank, int64_t *c0, int64_t *c1);
/* the same for block-sparse storage (XM_STORAGE_BSR3 / _VIEWGRAPH): ranges balanced by STORED BLOCKS (rowptr: n + 1 offsets), which
 * is what a context uses unless xm_tuning_t.balance == 1.  Host only. */
int xm_partition_blocks(int64_t n, const int64_t *rowptr, int world, int rank, int64_t *c0, int64_t *c1);

#ifdef __cplusplus
}
#endif
#endif /* XM_AMD_H */
