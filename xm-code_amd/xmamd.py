"""ctypes binding of the C ABI in include/xm_amd.h (libxm_amd.so) — the host-side mirror used by the tests,
bench.py and __graft_entry__.  The product path is the HIP library; this file only marshals numpy arrays.

There is NO CPU fallback: every compute entry point raises XmError when the library or a GPU is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XMAMD_LIB") or os.path.join(_HERE, "lib", "libxm_amd.so")   # XMAMD_LIB: a development aid of this binding (A/B builds)
MODULE_DIR = os.path.join(_HERE, "build")      # holds XM.cpython-*.so (the reference's module name)

STORAGE_DENSE, STORAGE_BSR3 = 0, 1
STORAGE_BSR3_DENSE = 2   # BSR3 on the host, expanded to the dense layout on the device (each rank: its own rows)
STORAGE_SCHUR = 3        # matrix-free: the observation list of the reference's create_matrix (cam, lm, p, w)
STORAGE_VIEWGRAPH = 4    # the view-graph edge list (ei, ej, w, M): block CSR + quaternion-compressed sliced ELL on the device
RETRACT_QR, RETRACT_POLAR = 0, 1
MODE_SOLVE, MODE_RANK3, MODE_REBUTTLE = 0, 1, 2
FLAG_VERBOSE, FLAG_FIX_STALE_SR, FLAG_PROFILE_QW, FLAG_HOST_STEPPED = 1, 2, 4, 8
CERT_EIG_NOT_CONVERGED = 1
CERT_EIG_EXACT = 2           # small problem: the certificate's tridiagonalisation ran to completion (dense route)
FLAG_WARM_R = 16
FLAG_HOST_OUTER = 64           # outer iteration of the trust region on the host instead of the device (xm_amd.h)
FLAG_DEVICE_OUTER = 128        # ... on the device also with dense products, where the host-driven form is the (faster) default (xm_amd.h)
FLAG_MODEL_RECURRENCE = 32     # model decrease of a tCG from its recurrences instead of from accumulated H v (xm_amd.h)
FLAG_TCG_THREE_LAUNCH = 256    # three launches per tCG iteration where the default is two (symmetric dense pair, one GPU; xm_amd.h): same bits
FLAG_TCG_RECOMPUTE = 512       # recompute the truncated CG behind a rejected step where the default replays it from the rejected one's history (xm_amd.h): same bits

EXPORTS = [
    "xm_last_error", "xm_version", "xm_abi_revision", "xm_solve", "xm_solve_rank3", "xm_solve_rebuttle", "xm_ctx_create", "xm_ctx_solve",
    "xm_ctx_destroy", "xm_dense_ld", "xm_dev_count", "xm_dev_alloc", "xm_dev_free", "xm_dev_h2d", "xm_dev_d2h",
    "xm_dev_sync", "xm_dense_upload", "xm_dense_from_bsr3", "xm_qw_dense", "xm_qw_dense_sym", "xm_qw_bsr3", "xm_retract", "xm_retract_polar", "xm_recover_rotations",
    "xm_comm_unique_id", "xm_comm_init", "xm_comm_init_shm", "xm_comm_init_ipc", "xm_comm_finalize", "xm_partition", "xm_partition_blocks",
    "xm_symv_plan", "xm_sell_layout", "xm_sell_locality", "xm_sell_create", "xm_sell_create2", "xm_sell_quat_roundtrip", "xm_sell_destroy", "xm_qw_sell", "xm_qw_sell_padded",
    "xm_ctx_attach_edges", "xm_ctx_edge_residuals", "xm_ctx_edge_residuals_recovered", "xm_ctx_xm2_filter", "xm_ctx_xm2_round", "xm_ctx_set_edge_weights", "xm_ctx_recover_tp", "xm_ctx_schur_info", "xm_ctx_tcg_two_launch", "xm_ctx_tcg_replay", "xm_ctx_set_tcg_history", "xm_ctx_qw", "xm_spd_inverse", "xm_ctx_transport", "xm_ctx_sell_wpad", "xm_ctx_product_kind", "xm_symw_plan", "xm_symw_use", "xm_symw_probe",
    "xm_ctx_schur_precond_info", "xm_schur_aggregate_plan",
    "xm_dense_to_f32", "xm_qw_dense_f32", "xm_qw_dense_sym_f32",
    "xm_ctx_bundle_adjust", "xm_ctx_reprojection_errors", "xm_spd_solve", "xm_la_probe", "xm_ba_aggregate_plan", "xm_ctx_ba_probe", "xm_lm_replay",
    "xm_ctx_bundle_adjust_focal", "xm_ctx_reprojection_errors_focal", "xm_ctx_ba_probe_focal",
    "xm_ctx_bundle_adjust_focal_groups", "xm_ctx_ba_probe_focal_groups",
    "xm_ctx_bundle_adjust_radial", "xm_ctx_reprojection_errors_radial", "xm_ctx_ba_probe_radial",
    "xm_clean_observations", "xm_ctx_clean_observations", "xm_ctx_rtr_probe", "xm_ctx_outer_probe", "xm_ctx_cert_probe", "xm_tridiag_min", "xm_ctx_schur_probe",
    "xm_ctx_dense_q", "xm_create_matrix", "xm_schur_dense_limits",
    "xm_pair_filter", "xm_pair_filter_limits",
    "xm_lift_observations", "xm_lift_limits",
    "xm_build_tracks", "xm_tracks_limits", "xm_tracks_split_host", "xm_tracks_split_device", "xm_tracks_split_limits", "xm_tracks_split_stats",
    "xm_view_graph_filter", "xm_view_graph_limits",
    "xm_view_graph_calibrate", "xm_view_graph_calibrate_probe", "xm_view_graph_calibrate_limits",
    "xm_view_graph_rotations", "xm_view_graph_rotations_probe", "xm_view_graph_rotations_limits",
    "xm_ctx_filter_tracks", "xm_track_filter_limits",
    "xm_ctx_triangulate_tracks", "xm_triangulate_limits",
    "xm_prune_weakly_connected", "xm_ctx_prune_weakly_connected", "xm_prune_limits",
    "xm_ctx_global_positioning", "xm_ctx_gp_probe", "xm_gp_limits",
    "xm_ctx_global_positioning_pairs", "xm_ctx_gp_probe_pairs", "xm_gp_pair_limits",
]
# include/xm_bench.h: timing hooks of the micro-benchmarks (same library, not part of the product ABI)
BENCH_EXPORTS = ["xm_bench_last_error", "xm_qw_dense_time", "xm_qw_dense_sym_time", "xm_qw_dense_f32_time", "xm_qw_dense_sym_f32_time", "xm_bench_symv_k", "xm_bench_dense_policy", "xm_qw_dense_sym_trace", "xm_qw_dense_strip_time", "xm_qw_dense_strip_ks", "xm_qw_bsr3_time", "xm_bench_bsr_binned", "xm_qw_sell_time",
                 "xm_retract_variant", "xm_recover_rotations_variant", "xm_peer_allgather_bench", "xm_qw_symw_time", "xm_bench_grid_barrier"]
PRODUCT_KINDS = {0: "dense", 1: "dense_sym", 2: "bsr3", 3: "sell", 4: "sell_quat", 5: "schur"}


class XmError(RuntimeError):
    pass


class Tuning(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("sym", "sym_min_rows", "sell", "sell_slabs", "sell_lmax", "sell_gather", "sell_codec", "overlap",
                                         "overlap_min_mb", "cert_dense_rows", "lanczos_mmax", "lanczos_restarts", "watchdog_s", "balance",
                                         "exchange", "split_k", "sell_wpad", "exchange_fence", "schur_host_assembly", "schur_trace",
                                         "schur_solver", "schur_dense_max", "debug_drop_finalize", "debug_peer_mute", "schur_pcg_first",
                                         "schur_pcg_hess_digits", "hess_f32", "schur_dense_q")]


class Problem(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int64), ("storage", C.c_int32), ("q_on_device", C.c_int32), ("q", C.c_void_p),
                ("ldq", C.c_int64), ("nb", C.c_int64), ("rowptr", C.c_void_p), ("colidx", C.c_void_p),
                ("blocks", C.c_void_p), ("nobs", C.c_int64), ("n_landmarks", C.c_int64), ("obs_cam", C.c_void_p), ("obs_lm", C.c_void_p),
                ("obs_p", C.c_void_p), ("obs_w", C.c_void_p), ("q_row0", C.c_int64),
                ("ne", C.c_int64), ("edge_i", C.c_void_p), ("edge_j", C.c_void_p), ("edge_w", C.c_void_p), ("edge_M", C.c_void_p),
                ("n_gpus", C.c_int32), ("gpu_map", C.c_int32), ("tuning", C.POINTER(Tuning))]


class Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_rank", C.c_uint32), ("tol", C.c_double), ("lam", C.c_double), ("max_time", C.c_double),
                ("mode", C.c_int32), ("flags", C.c_uint32), ("s_ini", C.c_void_p), ("trace_cap", C.c_int32),
                ("trace", C.c_void_p), ("R_ini", C.c_void_p), ("retraction", C.c_int32), ("sum_grouping", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("R", C.c_void_p), ("s", C.c_void_p), ("rank", C.c_int32), ("status", C.c_int32),
                ("primal", C.c_double), ("dual", C.c_double), ("min_eig", C.c_double), ("gap", C.c_double),
                ("tcg_iters", C.c_int64), ("outer_iters", C.c_int64), ("qw_products", C.c_int64),
                ("lanczos_iters", C.c_int64), ("seconds", C.c_double), ("tr_seconds", C.c_double),
                ("cert_seconds", C.c_double), ("qw_ms_sum", C.c_double), ("qw_ms_count", C.c_int64),
                ("qw_bytes", C.c_int64), ("trace_len", C.c_int32), ("last_stop_reason", C.c_int32),
                ("sym_product", C.c_int32), ("cert_flags", C.c_int32), ("eig_residual", C.c_double),
                ("n_gpus", C.c_int32), ("exchange", C.c_int32), ("qw_stream_bytes", C.c_int64),
                ("outer_on_device", C.c_int32), ("hess_f32", C.c_int32)]


class Xm2Info(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("percentile", C.c_double), ("threshold", C.c_double), ("removed", C.c_int64),
                ("s_avg", C.c_double), ("s_std", C.c_double), ("n_small", C.c_int64), ("regularised", C.c_int32), ("rank3_status", C.c_int32),
                ("lam_used", C.c_double), ("rank3_tcg_iters", C.c_int64)]


class BaOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_iters", C.c_int32), ("max_time", C.c_double), ("eta", C.c_double),
                ("function_tol", C.c_double), ("gradient_tol", C.c_double), ("parameter_tol", C.c_double), ("flags", C.c_uint32),
                ("trace_cap", C.c_int32), ("trace", C.c_void_p), ("loss", C.c_int32), ("max_nonmonotonic", C.c_int32), ("loss_scale", C.c_double)]


class BaResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_int32), ("iters", C.c_int32), ("accepted", C.c_int32),
                ("pcg_iters", C.c_int64), ("n_used", C.c_int64), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("gradient_max", C.c_double), ("seconds", C.c_double), ("trace_len", C.c_int32), ("coarse_fallbacks", C.c_int32)]


class BaProbe(C.Structure):   # xm_ba_probe_t, the test export xm_ctx_ba_probe
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("loss", C.c_int32), ("pad", C.c_int32), ("loss_scale", C.c_double),
                ("mu", C.c_double), ("k", C.c_int64), ("X", C.c_void_p), ("dc", C.c_void_p), ("cost", C.c_double), ("gmax", C.c_double),
                ("cost1", C.c_double), ("model", C.c_double), ("step2", C.c_double * 2), ("x2", C.c_double * 2), ("n_used", C.c_int64),
                ("nagg", C.c_int32), ("ncoarse", C.c_int32), ("coarse_ok", C.c_int32), ("pad2", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("b", "g_l", "vinv", "ustar", "sinv", "cused", "lused", "SX", "Sdense", "MX", "Pm", "dropped", "Ac",
                                          "dP", "rot1", "t1", "p1")]


class GpOptions(C.Structure):   # xm_gp_options_t
    _fields_ = [("struct_size", C.c_uint32), ("max_iters", C.c_int32), ("max_time", C.c_double), ("eta", C.c_double),
                ("function_tol", C.c_double), ("gradient_tol", C.c_double), ("parameter_tol", C.c_double), ("min_views", C.c_int32),
                ("trace_cap", C.c_int32), ("trace", C.c_void_p), ("loss", C.c_int32), ("pad", C.c_int32), ("loss_scale", C.c_double)]


class GpResult(C.Structure):   # xm_gp_result_t
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_int32), ("iters", C.c_int32), ("accepted", C.c_int32),
                ("pcg_iters", C.c_int64), ("n_used", C.c_int64), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("gradient_max", C.c_double), ("seconds", C.c_double), ("trace_len", C.c_int32), ("pad", C.c_int32)]


GP_PROBE_OUT = ("M", "q", "frozen", "oused", "vinv", "g_l", "ustar", "sinv", "b", "cused", "lused", "SX", "dP", "ds", "t1", "p1", "s1")


class GpProbe(C.Structure):   # xm_gp_probe_t, the test export xm_ctx_gp_probe
    _fields_ = [("struct_size", C.c_uint32), ("min_views", C.c_int32), ("loss", C.c_int32), ("pad", C.c_int32), ("loss_scale", C.c_double),
                ("mu", C.c_double), ("k", C.c_int64), ("s", C.c_void_p), ("X", C.c_void_p), ("dc", C.c_void_p), ("cost", C.c_double),
                ("gmax", C.c_double), ("cost1", C.c_double), ("model", C.c_double), ("step2", C.c_double * 3), ("x2", C.c_double * 3),
                ("n_used", C.c_int64)] + [(k, C.c_void_p) for k in GP_PROBE_OUT]


GP_CONSTRAINT = {"only_points": 0, "only_cameras": 1, "points_and_cameras_balanced": 2, "points_and_cameras": 3}   # XM_GP_*
GP_FIX_CENTRES = 1
GP_PAIR_PROBE_OUT = ("Mp", "qp", "pfrozen", "pused", "dsigma", "sigma1")


class GpPairs(C.Structure):   # xm_gp_pairs_t
    _fields_ = [("struct_size", C.c_uint32), ("constraint", C.c_int32), ("flags", C.c_uint32), ("pad", C.c_int32), ("npairs", C.c_int64),
                ("pi", C.c_void_p), ("pj", C.c_void_p), ("trel", C.c_void_p), ("valid", C.c_void_p), ("calibrated", C.c_void_p),
                ("reweight_scale", C.c_double), ("sigma", C.c_void_p), ("pairs_used", C.c_int64), ("cams_heavy", C.c_int64),
                ("max_incidences", C.c_int64), ("weight_scale_pt", C.c_double)]


class GpPairProbe(C.Structure):   # xm_gp_pair_probe_t, the test export xm_ctx_gp_probe_pairs
    _fields_ = [("struct_size", C.c_uint32), ("pad", C.c_int32), ("sigma_in", C.c_void_p)] + \
               [(k, C.c_double) for k in ("cost", "gsmax", "cost1", "model", "step2", "x2")] + [(k, C.c_void_p) for k in GP_PAIR_PROBE_OUT]


class RtrScal(C.Structure):    # xm_rtr_scal_t: the truncated CG's scalar block as the test export xm_ctx_rtr_probe passes it
    _fields_ = [(k, C.c_double) for k in ("rr", "vv", "vp", "pp", "delta", "gradnorm", "last_step", "model")] + [("status", C.c_int32), ("iter", C.c_int32)]


RTR_IN = ("R", "s", "pR", "ps", "rR", "rs", "vR", "vs", "HvR", "Hvs", "partsB_in", "X")
RTR_OUT = ("G", "egs", "S0", "rgR", "rgs", "HpR", "Hps", "init_rR", "init_rs", "init_pR", "init_ps", "init_vR", "init_vs", "init_HvR", "init_Hvs", "init_W",
           "init_Wpad", "out_vR", "out_vs", "out_HvR", "out_Hvs", "out_rR", "out_rs", "out_pR", "out_ps", "out_W", "out_Wpad", "partsB_out", "Lam", "dz", "SX")


class RtrProbe(C.Structure):   # xm_rtr_probe_t, the test export xm_ctx_rtr_probe
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("o", C.c_int32), ("k", C.c_int32), ("lam", C.c_double)] + \
               [(k, C.c_void_p) for k in RTR_IN] + [("partsB_in_count", C.c_int32), ("pad", C.c_int32), ("scal_in", RtrScal)] + \
               [(k, C.c_int32) for k in ("product_kind", "nA", "nB", "w_native", "wpad", "split_k", "sell_gather", "pad2")] + \
               [(k, C.c_double) for k in ("f", "rr", "pHp", "rHp", "HpHp", "rr_parts")] + [("dual", C.c_double * 2), ("init_scal", RtrScal), ("scal_out", RtrScal)] + \
               [(k, C.c_void_p) for k in RTR_OUT]


RTR_PROBE_AUTO, RTR_PROBE_MODEL_REC, RTR_PROBE_TCG_INIT, RTR_PROBE_CG_STEP, RTR_PROBE_CERT = 1, 2, 4, 8, 16
RTR_SCAL_IN = ("rr", "vv", "vp", "pp", "delta", "gradnorm", "model", "iter")


class OuterTcg(C.Structure):   # xm_outer_tcg_t: the truncated CG's scalar block with the fields the device-driven outer iteration adds
    _fields_ = [(k, C.c_double) for k in ("rr", "vv", "vp", "pp", "delta", "gradnorm", "last_step", "model")] + \
               [(k, C.c_int32) for k in ("status", "iter", "seq", "phase")]


class OuterScal(C.Structure):  # xm_outer_scal_t: the trust-region state of the device-driven outer iteration
    _fields_ = [("loss", C.c_double), ("rr_point", C.c_double), ("totalite", C.c_int64)] + \
               [(k, C.c_int32) for k in ("shrink_count", "k", "stop_reason", "time_up", "slots", "pad")]


OUTER_IN = ("R", "s", "vR", "vs", "HvR", "Hvs", "D", "pR", "ps", "rR", "rs", "Rc", "sc", "partsB_in", "partsM_in")
OUTER_MATS = ("rgR", "ret_Rc", "ret_W", "ls_Rc", "ls_W", "HpR", "cand_G", "cand_rgR", "out_R", "out_Rc", "out_vR", "out_HvR", "out_rR", "out_pR", "out_W",
              "out_G", "out_rgR")
OUTER_OUT = ("rgR", "rgs", "ret_Rc", "ret_sc", "ret_W", "ret_Wpad", "ret_partsM", "ls_Rc", "ls_W", "HpR", "Hps", "cand_G", "cand_egs", "cand_S0", "cand_rgR",
             "cand_rgs", "out_R", "out_s", "out_Rc", "out_sc", "out_vR", "out_vs", "out_HvR", "out_Hvs", "out_rR", "out_rs", "out_pR", "out_ps", "out_W",
             "out_Wpad", "out_partsB", "out_partsM", "out_G", "out_egs", "out_S0", "out_rgR", "out_rgs")


class OuterProbe(C.Structure):   # xm_outer_probe_t, the test export xm_ctx_outer_probe
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("o", C.c_int32), ("slot", C.c_int32), ("lam", C.c_double), ("t", C.c_double)] + \
               [(k, C.c_void_p) for k in OUTER_IN] + [("partsB_in_count", C.c_int32), ("partsM_in_count", C.c_int32), ("scal_in", OuterTcg), ("os_in", OuterScal),
                                                      ("delta_bar", C.c_double), ("gradtol", C.c_double), ("max_outer", C.c_int32), ("stop_req", C.c_int32)] + \
               [(k, C.c_int32) for k in ("product_kind", "nA", "nB", "nM", "w_native", "wpad", "polar", "grid", "nwave", "trace_written")] + \
               [("run", C.c_uint32), ("pad", C.c_uint32), ("ret_pad", C.c_int32 * 3), ("ls_pad", C.c_int32 * 2), ("out_pad", C.c_int32 * 2), ("pad2", C.c_int32)] + \
               [(k, C.c_double) for k in ("f", "rr", "model", "pHp", "rHp", "HpHp", "f_cand", "rr_cand", "m_cand")] + \
               [("progress", C.c_uint64), ("scal_out", OuterTcg), ("os_out", OuterScal), ("trace", C.c_double * 6)] + [(k, C.c_void_p) for k in OUTER_OUT]


OUTER_PROBE_RETRACT, OUTER_PROBE_MODEL_REC, OUTER_PROBE_RETRACT_LS, OUTER_PROBE_STEP, OUTER_PROBE_POLAR, OUTER_PROBE_MGS, OUTER_PROBE_AUTO = 1, 2, 4, 8, 16, 32, 64
PH_TCG, PH_CAND, PH_STOP, PH_INIT = 0, 1, 2, 3


CERT_OUT = ("Lam", "dz", "alpha", "beta", "V", "c1", "c2", "y", "x")
CERT_INTS = ("ret", "eig_exact", "iters", "m_use", "cycles", "mmax", "steps_dev", "steps_fused", "steps_unfused", "nseg", "product_kind")


class CertProbe(C.Structure):   # xm_cert_probe_t, the test export xm_ctx_cert_probe
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("o", C.c_int32), ("cap", C.c_int32), ("lam", C.c_double), ("R", C.c_void_p), ("s", C.c_void_p)] + \
               [(k, C.c_int32) for k in CERT_INTS + ("pad2",)] + [("len", C.c_int64), ("theta", C.c_double), ("resid", C.c_double), ("dual", C.c_double * 2)] + \
               [(k, C.c_void_p) for k in CERT_OUT]


CERT_PROBE_UNFUSED = 1

SCHUR_PROBE_INTS = ("uses_cg", "two_level", "dup_pairs", "pcg_done", "pcg_iters", "pcg_cap")
SCHUR_PROBE_OUT = ("deg", "perm", "Q1", "c", "q2", "q3inv", "dinv", "VTinv", "binv", "ainv", "h", "r", "xc", "xl", "Y", "VX", "pAp", "MX")


class SchurProbe(C.Structure):   # xm_schur_probe_t, the test export xm_ctx_schur_probe
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("o", C.c_int32), ("k", C.c_int32), ("alpha", C.c_double), ("W", C.c_void_p),
                ("X", C.c_void_p), ("nheavy", C.c_int64), ("lm_total", C.c_int64), ("nagg", C.c_int64)] + \
               [(k, C.c_int32) for k in SCHUR_PROBE_INTS] + [("pcg_relres", C.c_double), ("pcg_tol", C.c_double)] + \
               [(k, C.c_void_p) for k in SCHUR_PROBE_OUT]


SCHUR_PROBE_DENSE_MAX_ROWS = 4096
SCHUR_AGG_CAMS = 64


def tridiag_min(a, b):
    """smallest eigenpair of the symmetric tridiagonal matrix (diagonal a[0..m), off-diagonal b[0..m-1)) by the certificate's host code
    (xm_tridiag_min; no GPU): theta, y, tmax"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.ndim != 1 or a.size < 1 or b.shape != (a.size - 1,):
        raise ValueError("tridiag_min: a is the diagonal (m >= 1), b the m - 1 off-diagonal entries")
    theta, tmax, y = C.c_double(), C.c_double(), np.zeros(a.size)
    bp = b.ctypes.data_as(C.c_void_p) if b.size else None
    _chk(lib().xm_tridiag_min(a.ctypes.data_as(C.c_void_p), bp, int(a.size), C.byref(theta), y.ctypes.data_as(C.c_void_p), C.byref(tmax)))
    return theta.value, y, tmax.value


def pack_prog(run, slots, phase):
    """the progress word of the device-driven outer iteration: [run : 32 | launch pairs done : 24 | phase : 8]"""
    return (int(run) << 32) | ((int(slots) & 0xffffff) << 8) | (int(phase) & 0xff)


class CleanOptions(C.Structure):   # xm_clean_options_t
    _fields_ = [("struct_size", C.c_uint32), ("min_cam_obs", C.c_int32), ("min_lm_obs", C.c_int32), ("flags", C.c_uint32)]


class CleanResult(C.Structure):    # xm_clean_result_t
    _fields_ = [("struct_size", C.c_uint32), ("rounds", C.c_int32)] + \
               [(k, C.c_int64) for k in ("nobs_live", "n_new", "m_new", "nobs_new", "components", "cams_weak", "lms_weak", "cams_emptied",
                                         "cams_off_component", "lms_off_component")] + [("first_camera", C.c_int32), ("reserved", C.c_int32)]


class TfOptions(C.Structure):      # xm_tf_options_t
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("max_reprojection_error", C.c_double), ("max_angle_error", C.c_double),
                ("min_triangulation_angle", C.c_double), ("min_views", C.c_int32), ("reserved", C.c_int32)]


TF_COUNTS = ("tracks_total", "tracks_kept", "obs_used", "obs_kept", "dropped_depth", "dropped_reprojection", "dropped_angle", "dropped_triangulation",
             "dropped_min_views", "tracks_changed_reprojection", "tracks_changed_angle", "tracks_changed_triangulation", "tracks_changed_min_views")


class TfResult(C.Structure):       # xm_tf_result_t
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(k, C.c_int64) for k in TF_COUNTS] + \
               [(k, C.c_double) for k in ("cos_angle", "cos_triangulation", "seconds_kernels", "seconds_download")]


class TriOptions(C.Structure):     # xm_tri_options_t; the defaults are XM_TRI_OPTIONS_INIT
    _fields_ = [("struct_size", C.c_uint32), ("max_hypotheses", C.c_int32), ("min_angle", C.c_double), ("create_max_angle_error", C.c_double),
                ("complete_max_reproj_error", C.c_double), ("min_views", C.c_int32), ("refine_rounds", C.c_int32)]


TRI_COUNTS = ("lm_accepted", "lm_unused", "lm_no_hypothesis", "lm_degenerate", "lm_min_views", "lm_angle", "obs_candidates", "obs_kept",
              "obs_readmitted", "obs_lost", "pairs_tested", "hypotheses_scored")


class TriResult(C.Structure):      # xm_tri_result_t
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(k, C.c_int64) for k in TRI_COUNTS] + \
               [(k, C.c_double) for k in ("cos_min_angle", "cos_create", "seconds_kernels", "seconds_download")]


class PruneOptions(C.Structure):   # xm_prune_options_t; the defaults are GLOMAP's (XM_PRUNE_OPTIONS_INIT)
    _fields_ = [("struct_size", C.c_uint32), ("min_covisibility", C.c_int32), ("min_num_images", C.c_int32), ("min_num_observations", C.c_int32),
                ("min_threshold", C.c_double)]


class PrunePairs(C.Structure):     # xm_prune_pairs_t
    _fields_ = [("capacity", C.c_int64), ("i", C.c_void_p), ("j", C.c_void_p), ("count", C.c_void_p)]


class PruneResult(C.Structure):    # xm_prune_result_t
    _fields_ = [("struct_size", C.c_uint32), ("rounds", C.c_int32), ("pairs_covisible", C.c_int64), ("n_edges", C.c_int64), ("median", C.c_double),
                ("mad", C.c_double), ("threshold", C.c_double), ("component_images", C.c_int64), ("strong_clusters", C.c_int64),
                ("weak_edges", C.c_int64), ("n_clusters", C.c_int64), ("images_clustered", C.c_int64), ("seconds_kernels", C.c_double),
                ("seconds_download", C.c_double)]


class PairOptions(C.Structure):    # xm_pair_options_t; the defaults are the reference's constants (XM_PAIR_OPTIONS_INIT)
    _fields_ = [("struct_size", C.c_uint32), ("min_joint", C.c_int32), ("min_flags", C.c_int32), ("flags", C.c_uint32), ("trim", C.c_double),
                ("dist_pct", C.c_double), ("err_pct", C.c_double), ("mad_factor", C.c_double)]

    def __init__(self, min_joint=20, min_flags=1, flags=0, trim=0.05, dist_pct=90.0, err_pct=95.0, mad_factor=3.0):
        super().__init__(C.sizeof(PairOptions), min_joint, min_flags, flags, trim, dist_pct, err_pct, mad_factor)


class PairStat(C.Structure):       # xm_pair_stat_t
    _fields_ = [(k, C.c_int32) for k in ("n_joint", "n_kept", "n_flagged", "status")] + [("scale1", C.c_double), ("scale2", C.c_double),
               ("translation", C.c_double * 3), ("median", C.c_double), ("p95", C.c_double), ("percentage", C.c_double)]


class PairResult(C.Structure):     # xm_pair_result_t
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + \
               [(k, C.c_int64) for k in ("pairs_used", "pairs_skipped", "pairs_degenerate", "nobs_flagged", "max_joint", "pairs_on_workspace_path")] + \
               [(k, C.c_double) for k in ("seconds_index", "seconds_kernels", "seconds_download")]


class LiftOptions(C.Structure):    # xm_lift_options_t; the defaults are the constants of 5_test_ceres.py (XM_LIFT_OPTIONS_INIT)
    _fields_ = [("struct_size", C.c_uint32), ("margin", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("depth_pct", C.c_double)]

    def __init__(self, margin=10, flags=0, depth_pct=95.0):
        super().__init__(C.sizeof(LiftOptions), margin, flags, 0, depth_pct)


class LiftResult(C.Structure):     # xm_lift_result_t
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + \
               [(k, C.c_int64) for k in ("rows_duplicate", "rows_border", "rows_depth", "rows_no_map", "cams_no_map", "cams_empty", "cams_small",
                                         "cams_large", "cams_workspace", "max_rows")] + \
               [(k, C.c_double) for k in ("seconds_index", "seconds_kernels", "seconds_download")]


class TracksOptions(C.Structure):  # xm_tracks_options_t; the defaults are the pipeline's constants (XM_TRACKS_OPTIONS_INIT)
    _fields_ = [("struct_size", C.c_uint32), ("min_views", C.c_int32), ("max_views", C.c_int32), ("conflict", C.c_int32), ("max_tracks", C.c_int64),
                ("thres_inconsistency", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, min_views=3, max_views=1000000, conflict=2, max_tracks=10000000, thres_inconsistency=10.0, flags=0):
        super().__init__(C.sizeof(TracksOptions), min_views, max_views, conflict, max_tracks, thres_inconsistency, flags, 0)


class TracksResult(C.Structure):   # xm_tracks_result_t
    _fields_ = [("struct_size", C.c_uint32), ("rounds", C.c_int32)] + \
               [(k, C.c_int64) for k in ("ntracks", "features_touched", "matches", "components", "components_conflicted", "rows_conflicted",
                                         "tracks_short", "tracks_long", "tracks_conflict", "tracks_few_registered", "tracks_beyond_max",
                                         "images_small", "images_large", "images_workspace", "max_touched", "edges_split", "unions_refused")] + \
               [(k, C.c_double) for k in ("seconds_index", "seconds_kernels", "seconds_split", "seconds_download")]


class VgOptions(C.Structure):      # xm_vg_options_t; the defaults are those of glomap/types.h:18-33 (XM_VG_OPTIONS_INIT)
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("max_epipolar_error_E", C.c_double), ("max_epipolar_error_F", C.c_double),
                ("max_epipolar_error_H", C.c_double), ("min_inlier_num", C.c_int32), ("reserved", C.c_int32), ("min_inlier_ratio", C.c_double),
                ("cos_max_rotation_error", C.c_double)]

    def __init__(self, flags=1, max_epipolar_error_E=1.0, max_epipolar_error_F=4.0, max_epipolar_error_H=4.0, min_inlier_num=30, min_inlier_ratio=0.25,
                 cos_max_rotation_error=9.8480775301220802e-01):
        super().__init__(C.sizeof(VgOptions), flags, max_epipolar_error_E, max_epipolar_error_F, max_epipolar_error_H, min_inlier_num, 0, min_inlier_ratio,
                         cos_max_rotation_error)


class VgResult(C.Structure):       # xm_vg_result_t
    _fields_ = [("struct_size", C.c_uint32), ("rounds", C.c_int32)] + \
               [(k, C.c_int64) for k in ("matches", "inliers", "matches_out", "pairs_valid", "pairs_invalid_in", "pairs_few_inliers", "pairs_low_ratio",
                                         "pairs_rotation", "pairs_outside", "pairs_none", "pairs_E", "pairs_F", "pairs_H", "largest", "components",
                                         "pairs_wave", "pairs_group", "pairs_workspace", "max_matches")] + \
               [(k, C.c_double) for k in ("seconds_index", "seconds_kernels", "seconds_download")]


class VgcOptions(C.Structure):     # xm_vgc_options_t; the defaults are those of view_graph_calibration.h:21-23 and optimization_base.h:21-26
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("thres_loss_function", C.c_double), ("thres_lower_ratio", C.c_double),
                ("thres_higher_ratio", C.c_double), ("thres_two_view_error", C.c_double), ("max_num_iterations", C.c_int32), ("reserved", C.c_int32),
                ("function_tolerance", C.c_double), ("lower_bound", C.c_double)]

    def __init__(self, flags=0, thres_loss_function=1e-2, thres_lower_ratio=0.1, thres_higher_ratio=10.0, thres_two_view_error=2.0,
                 max_num_iterations=100, function_tolerance=1e-5, lower_bound=1e-3):
        super().__init__(C.sizeof(VgcOptions), flags, thres_loss_function, thres_lower_ratio, thres_higher_ratio, thres_two_view_error,
                         max_num_iterations, 0, function_tolerance, lower_bound)


class VgcResult(C.Structure):      # xm_vgc_result_t
    _fields_ = [("struct_size", C.c_uint32), ("stop_reason", C.c_int32)] + \
               [(k, C.c_int64) for k in ("pairs", "pairs_same_camera", "cams_free", "cams_constant", "cams_rejected", "pairs_invalidated", "pairs_flipped",
                                         "cams_heavy", "max_incidences", "pcg_iterations")] + \
               [(k, C.c_int32) for k in ("iterations", "accepted", "trace_len", "reserved")] + \
               [(k, C.c_double) for k in ("initial_cost", "final_cost", "seconds_index", "seconds_kernels", "seconds_download")]


class VgcProbe(C.Structure):       # xm_vgc_probe_t, the test export xm_view_graph_calibrate_probe
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("focal", C.c_void_p), ("x", C.c_void_p), ("d_in", C.c_void_p), ("mu", C.c_double)] + \
               [(k, C.c_void_p) for k in ("d", "residual", "record", "cost", "gradient", "diagonal", "product")]


class VgrOptions(C.Structure):     # xm_vgr_options_t; the defaults are those of global_rotation_averaging.h
    _fields_ = [("struct_size", C.c_uint32), ("weight_type", C.c_int32), ("max_num_irls_iterations", C.c_int32), ("fixed_image", C.c_int32),
                ("irls_step_convergence_threshold", C.c_double), ("irls_loss_parameter_sigma", C.c_double)]

    def __init__(self, weight_type=0, max_num_irls_iterations=100, fixed_image=-1, irls_step_convergence_threshold=1e-3,
                 irls_loss_parameter_sigma=5.0):
        super().__init__(C.sizeof(VgrOptions), weight_type, max_num_irls_iterations, fixed_image, irls_step_convergence_threshold,
                         irls_loss_parameter_sigma)


class VgrResult(C.Structure):      # xm_vgr_result_t
    _fields_ = [("struct_size", C.c_uint32), ("stop_reason", C.c_int32), ("irls_iterations", C.c_int32), ("reserved", C.c_int32)] + \
               [(k, C.c_int64) for k in ("pcg_iterations", "pcg_capped", "pairs", "registered", "fixed_image", "cams_heavy", "max_incidences")] + \
               [(k, C.c_double) for k in ("seconds_index", "seconds_kernels", "seconds_download")]


class VgrProbe(C.Structure):       # xm_vgr_probe_t, the test export xm_view_graph_rotations_probe
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + \
               [(k, C.c_void_p) for k in ("angle_axis", "x", "weight_in", "rot", "residual", "gauge", "weight", "rhs", "diagonal", "product",
                                          "angle_axis_out", "step")]


class LaProbe(C.Structure):        # xm_la_probe_t, the test export xm_la_probe
    _fields_ = [("struct_size", C.c_uint32)] + [(k, C.c_int32) for k in ("op", "m", "n", "k", "nrhs", "ta", "tb", "lower_only", "info")] + \
               [(k, C.c_int64) for k in ("lda", "ldb", "ldc")] + [("q", C.c_double)] + [(k, C.c_void_p) for k in ("A", "B", "C")]


class SymwProbe(C.Structure):      # xm_symw_probe_t, the test export xm_symw_probe
    _fields_ = [("struct_size", C.c_uint32)] + [(k, C.c_int32) for k in ("ntot", "nloc", "cam0", "world", "o", "K", "nt", "scal_status", "nitems", "nfull")] + \
               [(k, C.c_double) for k in ("alpha", "pad_value")] + [(k, C.c_void_p) for k in ("Q", "W", "cs_all", "Prow", "Pcol", "csum", "Y")]


LA_PROBE_MAX_N = 4096
SYMW_PROBE_MAX_NTOT = 4096
LA_OPS = {"gemm_sub": 0, "cholesky": 1, "substitute": 2, "inverse": 3, "layout": 4, "rank1_sub": 5}
VGC_UPDATE_CONFIG = 1
VGC_VALID, VGC_INVALID_IN, VGC_TWO_VIEW_ERROR = 0, 1, 2
VGC_CAM_UNUSED, VGC_CAM_CONSTANT, VGC_CAM_REFINED, VGC_CAM_REJECTED = 0, 1, 2, 3
VGR_GEMAN_MCCLURE, VGR_HALF_NORM = 0, 1
VGR_WEIGHT_TYPES = {"geman_mcclure": VGR_GEMAN_MCCLURE, "half_norm": VGR_HALF_NORM}
VGR_STOP_NOTHING, VGR_STOP_STEP, VGR_STOP_ITERATIONS, VGR_STOP_NONFINITE = 0, 1, 2, 3
VGR_STOP = {0: "nothing", 1: "step_tolerance", 2: "max_iterations", 3: "nonfinite_weight"}
VG_SCORE = 1
VG_MODEL_NONE, VG_MODEL_E, VG_MODEL_F, VG_MODEL_H = 0, 1, 2, 3
VG_MODELS = {"none": VG_MODEL_NONE, "E": VG_MODEL_E, "F": VG_MODEL_F, "H": VG_MODEL_H}
VG_VALID, VG_INVALID_IN, VG_FEW_INLIERS, VG_LOW_RATIO, VG_ROTATION, VG_OUTSIDE = 0, 1, 2, 3, 4, 5
TRACKS_DROP, TRACKS_GLOMAP, TRACKS_SPLIT = 0, 1, 2
TRACKS_SPLIT_DEVICE = 2            # xm_tracks_options_t.flags: rule 4's split on the device (with TRACKS_SPLIT only)
TRACKS_POLICIES = {"drop": TRACKS_DROP, "glomap": TRACKS_GLOMAP, "split": TRACKS_SPLIT, "split_device": TRACKS_SPLIT}
TRACK_UNTOUCHED, TRACK_SHORT, TRACK_LONG, TRACK_CONFLICT, TRACK_FEW_REGISTERED, TRACK_BEYOND_MAX = -1, -2, -3, -4, -5, -6
LIFT_MAPS_ON_DEVICE = 1
PAIR_STAT_DTYPE = np.dtype([("n_joint", "<i4"), ("n_kept", "<i4"), ("n_flagged", "<i4"), ("status", "<i4"), ("scale1", "<f8"), ("scale2", "<f8"),
                            ("translation", "<f8", (3,)), ("median", "<f8"), ("p95", "<f8"), ("percentage", "<f8")])
PAIR_SKIP_ROW0 = 1
PAIR_USED, PAIR_TOO_FEW, PAIR_DEGENERATE = 0, 1, 2
CLEAN_NO_SWAP = 1
TF_REPROJECTION, TF_ANGLE, TF_TRIANGULATION = 1, 2, 4                     # xm_tf_options_t.flags
TF_REASON_DEPTH, TF_REASON_REPROJECTION, TF_REASON_ANGLE, TF_REASON_TRIANGULATION, TF_REASON_MIN_VIEWS = 1, 2, 4, 8, 16   # reason[e]
TF_LM_KEPT, TF_LM_UNUSED, TF_LM_TRIANGULATION, TF_LM_MIN_VIEWS = 0, 1, 2, 3   # lm_status[l]
TRI_LM_ACCEPTED, TRI_LM_UNUSED, TRI_LM_NO_HYPOTHESIS, TRI_LM_DEGENERATE, TRI_LM_MIN_VIEWS, TRI_LM_ANGLE = 0, 1, 2, 3, 4, 5   # lm_status[l]
TRI_REASON_NOT_CANDIDATE, TRI_REASON_NOT_MEMBER, TRI_REASON_LANDMARK = 1, 2, 4   # reason[e]
BA_PROBE_DENSE_MAX_ROWS = 4096
BA_FIX_ROTATIONS = 1
BA_NONMONOTONIC = 2
BA_DENSE_SCHUR = 16            # Ceres's DENSE_SCHUR for the reduced camera system (include/xm_amd.h)
BA_DENSE_MAX_ROWS = 32768      # ... up to this many rows (6 per camera, 3 with fixed rotations)
BA_LINEAR_SOLVERS = {"iterative_schur": 0, "dense_schur": BA_DENSE_SCHUR}
BA_PRECOND_TWO_LEVEL = 32      # PCG preconditioner: aggregate blocks + rigid-motion coarse operator (include/xm_amd.h)
BA_PRECOND_BLOCKS = 64         # ... the aggregate blocks alone
BA_AGG_CAMS = 16               # cameras per aggregate
BA_MAX_AGGREGATES = 4096
BA_FOCAL_GROUPS_EXACT = 16     # focal groups: up to this many, the preconditioner's focal block is the exact G x G one
BA_REFINE_FOCAL = 128          # a focal scale per camera in the camera block (xm_ctx_bundle_adjust_focal; the default preconditioner only)
BA_REFINE_RADIAL = 256         # a radial coefficient per camera behind the focal scale (xm_ctx_bundle_adjust_radial; with BA_REFINE_FOCAL only)
BA_PRECONDITIONERS = {"jacobi": 0, "blocks": BA_PRECOND_BLOCKS, "two_level": BA_PRECOND_TWO_LEVEL}
BA_LOSS = {"trivial": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}
BA_OPTIONS_SIZE_V1 = 64        # struct_size of callers built before loss, max_nonmonotonic and loss_scale (include/xm_amd.h)
BA_STATUS = {0: "no_convergence", 1: "function_tolerance", 2: "gradient_tolerance", 3: "parameter_tolerance", 4: "max_iterations",
             5: "time_limit", 6: "no_progress"}
BA_CONVERGED = (1, 2, 3)


_lib = None


def lib():
    """Load libxm_amd.so (built by `make -C xm-code_amd` / __graft_entry__.build()).  Fails loudly when absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise XmError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.xm_last_error.restype = C.c_char_p
        L.xm_version.restype = C.c_char_p
        L.xm_dense_ld.restype = C.c_int64
        L.xm_dense_ld.argtypes = [C.c_int64]
        for name in ("xm_solve", "xm_solve_rank3"):
            getattr(L, name).argtypes = [C.c_char_p, C.c_uint, C.c_double, C.c_double, C.c_double]
        L.xm_solve_rebuttle.argtypes = [C.c_char_p, C.c_uint, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int)]
        L.xm_ctx_create.argtypes = [C.POINTER(Problem), C.POINTER(C.c_void_p)]
        L.xm_ctx_solve.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(Result)]
        L.xm_ctx_destroy.argtypes = [C.c_void_p]
        L.xm_ctx_destroy.restype = None
        L.xm_spd_inverse.argtypes = [C.c_int64, C.c_void_p]
        L.xm_spd_solve.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        L.xm_la_probe.argtypes = [C.POINTER(LaProbe)]
        L.xm_ctx_qw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double]
        L.xm_ctx_attach_edges.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xm_ctx_edge_residuals.argtypes = [C.c_void_p, C.c_void_p]
        L.xm_ctx_set_edge_weights.argtypes = [C.c_void_p, C.c_void_p]
        L.xm_ctx_edge_residuals_recovered.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xm_ctx_xm2_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_void_p]
        L.xm_ctx_xm2_round.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Options), C.POINTER(Xm2Info), C.POINTER(Result)]
        L.xm_ctx_recover_tp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xm_ctx_bundle_adjust.argtypes = [C.c_void_p, C.POINTER(BaOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BaResult)]
        L.xm_ctx_ba_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BaProbe)]
        L.xm_ctx_bundle_adjust_focal.argtypes = [C.c_void_p, C.POINTER(BaOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.POINTER(BaResult)]
        L.xm_ctx_reprojection_errors_focal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xm_ctx_bundle_adjust_radial.argtypes = [C.c_void_p, C.POINTER(BaOptions)] + [C.c_void_p] * 7 + [C.POINTER(BaResult)]
        L.xm_ctx_reprojection_errors_radial.argtypes = [C.c_void_p] * 7
        L.xm_ctx_ba_probe_radial.argtypes = [C.c_void_p] * 8 + [C.POINTER(BaProbe), C.c_void_p, C.c_void_p]
        L.xm_ctx_ba_probe_focal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BaProbe), C.c_void_p]
        L.xm_ctx_bundle_adjust_focal_groups.argtypes = [C.c_void_p, C.POINTER(BaOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.POINTER(BaResult)]
        L.xm_ctx_ba_probe_focal_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.POINTER(BaProbe), C.c_void_p]
        L.xm_ctx_rtr_probe.argtypes = [C.c_void_p, C.POINTER(RtrProbe)]
        L.xm_ctx_outer_probe.argtypes = [C.c_void_p, C.POINTER(OuterProbe)]
        L.xm_ctx_cert_probe.argtypes = [C.c_void_p, C.POINTER(CertProbe)]
        L.xm_ctx_schur_probe.argtypes = [C.c_void_p, C.POINTER(SchurProbe)]
        L.xm_tridiag_min.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_double)]
        L.xm_clean_observations.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CleanOptions), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.POINTER(CleanResult)]
        L.xm_ctx_clean_observations.argtypes = [C.c_void_p, C.POINTER(CleanOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CleanResult)]
        L.xm_pair_filter.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(PairOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PairResult)]
        L.xm_pair_filter_limits.argtypes = [C.c_void_p]
        L.xm_lift_observations.argtypes = [C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 7 + [C.POINTER(LiftOptions)] + [C.c_void_p] * 5 + \
                                          [C.POINTER(C.c_int64), C.c_void_p, C.POINTER(LiftResult)]
        L.xm_lift_limits.argtypes = [C.c_void_p]
        L.xm_build_tracks.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.POINTER(TracksOptions)] + \
                                     [C.c_void_p] * 4 + [C.POINTER(C.c_int64), C.c_void_p, C.POINTER(TracksResult)]
        L.xm_tracks_limits.argtypes = [C.c_void_p]
        L.xm_view_graph_filter.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_int64] + [C.c_void_p] * 12 + [C.POINTER(VgOptions)] + [C.c_void_p] * 7 + \
                                          [C.POINTER(VgResult)]
        L.xm_view_graph_limits.argtypes = [C.c_void_p]
        L.xm_view_graph_calibrate.argtypes = [C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + \
                                             [C.POINTER(VgcOptions)] + [C.c_void_p] * 10 + [C.POINTER(VgcResult)]
        L.xm_view_graph_calibrate_probe.argtypes = [C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + \
                                                   [C.POINTER(VgcOptions), C.POINTER(VgcProbe)]
        L.xm_view_graph_calibrate_limits.argtypes = [C.c_void_p]
        L.xm_view_graph_rotations.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.POINTER(VgrOptions)] + \
                                             [C.c_void_p] * 5 + [C.POINTER(VgrResult)]
        L.xm_view_graph_rotations_probe.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + \
                                                   [C.POINTER(VgrOptions), C.POINTER(VgrProbe)]
        L.xm_view_graph_rotations_limits.argtypes = [C.c_void_p]
        L.xm_tracks_split_host.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.xm_tracks_split_device.argtypes = L.xm_tracks_split_host.argtypes
        L.xm_tracks_split_limits.argtypes = [C.c_void_p]
        L.xm_tracks_split_stats.argtypes = [C.c_void_p]
        L.xm_ctx_filter_tracks.argtypes = [C.c_void_p, C.POINTER(TfOptions)] + [C.c_void_p] * 7 + [C.POINTER(TfResult)]
        L.xm_track_filter_limits.argtypes = [C.c_void_p]
        L.xm_ctx_triangulate_tracks.argtypes = [C.c_void_p, C.POINTER(TriOptions)] + [C.c_void_p] * 10 + [C.POINTER(TriResult)]
        L.xm_triangulate_limits.argtypes = [C.c_void_p]
        L.xm_ctx_global_positioning.argtypes = [C.c_void_p, C.POINTER(GpOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GpResult)]
        L.xm_ctx_gp_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GpProbe)]
        L.xm_gp_limits.argtypes = [C.c_void_p]
        L.xm_ctx_global_positioning_pairs.argtypes = [C.c_void_p, C.POINTER(GpOptions), C.POINTER(GpPairs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.POINTER(GpResult)]
        L.xm_ctx_gp_probe_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GpProbe), C.POINTER(GpPairs), C.POINTER(GpPairProbe)]
        L.xm_gp_pair_limits.argtypes = [C.c_void_p]
        L.xm_prune_weakly_connected.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PruneOptions), C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.POINTER(PruneResult)]
        L.xm_ctx_prune_weakly_connected.argtypes = [C.c_void_p, C.POINTER(PruneOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PruneResult)]
        L.xm_prune_limits.argtypes = [C.c_void_p]
        L.xm_ctx_reprojection_errors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xm_ctx_transport.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        L.xm_ctx_dense_q.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.xm_create_matrix.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.xm_schur_dense_limits.argtypes = [C.c_void_p]
        L.xm_ctx_tcg_two_launch.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.xm_ctx_tcg_replay.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.xm_ctx_set_tcg_history.argtypes = [C.c_void_p, C.c_int32]
        L.xm_ctx_schur_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_double)]
        L.xm_ctx_schur_precond_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.xm_schur_aggregate_plan.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.xm_ba_aggregate_plan.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.xm_lm_replay.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        L.xm_ctx_sell_wpad.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.xm_ctx_product_kind.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.xm_bench_last_error.restype = C.c_char_p
        L.xm_symw_plan.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.xm_symw_use.argtypes = [C.c_int, C.c_int, C.c_int]
        L.xm_symw_probe.argtypes = [C.POINTER(SymwProbe)]
        L.xm_qw_symw_time.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int64)]
        L.xm_bench_grid_barrier.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.xm_dev_count.argtypes = [C.POINTER(C.c_int)]
        L.xm_dev_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.xm_dev_free.argtypes = [C.c_void_p]
        L.xm_dev_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.xm_dev_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.xm_dense_upload.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]
        L.xm_dense_from_bsr3.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        L.xm_qw_dense.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
        L.xm_qw_dense_sym.argtypes = L.xm_qw_dense.argtypes
        L.xm_dense_to_f32.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        L.xm_qw_dense_f32.argtypes = L.xm_qw_dense.argtypes
        L.xm_qw_dense_sym_f32.argtypes = L.xm_qw_dense.argtypes
        L.xm_qw_dense_f32_time.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.xm_qw_dense_sym_f32_time.argtypes = L.xm_qw_dense_f32_time.argtypes
        L.xm_qw_dense_sym_time.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.xm_bench_symv_k.argtypes = [C.c_int, C.c_int, C.c_int]
        L.xm_qw_dense_sym_trace.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int)]
        L.xm_qw_bsr3.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_double, C.c_void_p]
        L.xm_retract.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.xm_retract_polar.argtypes = L.xm_retract.argtypes
        L.xm_retract_variant.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.xm_qw_dense_time.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_double)]
        L.xm_qw_dense_strip_time.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.xm_qw_dense_strip_ks.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double),
                                           C.POINTER(C.c_int)]
        L.xm_peer_allgather_bench.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_double)]
        L.xm_qw_bsr3_time.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                      C.POINTER(C.c_double)]
        L.xm_recover_rotations.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.xm_recover_rotations_variant.argtypes = L.xm_recover_rotations.argtypes + [C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.xm_comm_unique_id.argtypes = [C.c_char_p]
        L.xm_comm_init.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
        L.xm_comm_init_shm.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
        L.xm_comm_init_ipc.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_double]
        L.xm_partition.argtypes = [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.xm_partition_blocks.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.xm_sell_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p] + [C.c_void_p] * 7
        L.xm_sell_locality.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        L.xm_sell_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.xm_sell_create2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_void_p)]
        L.xm_sell_quat_roundtrip.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.xm_sell_destroy.argtypes = [C.c_void_p]
        L.xm_sell_destroy.restype = None
        L.xm_qw_sell.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p]
        L.xm_qw_sell_padded.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p]
        L.xm_qw_sell_time.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        msg = lib().xm_last_error().decode() or lib().xm_bench_last_error().decode()   # the timing hooks keep their own message (xm_bench.h)
        raise XmError(f"xm_amd error {rc}: {msg}")


def device_count():
    c = C.c_int(0)
    lib().xm_dev_count(C.byref(c))
    return c.value


def require_gpu():
    if device_count() < 1:
        raise XmError("no HIP device visible: the XM solver has no CPU fallback")


def pitch_of(o):
    return o | 1


def dense_ld(n):
    return int(lib().xm_dense_ld(n))


# ------------------------------------------------------------------------------------------------ device buffers
class DevArray:
    """A float64 / int device buffer owned through the C ABI (no torch needed)."""

    def __init__(self, host=None, nbytes=None):
        self.ptr = C.c_void_p()
        self.nbytes = int(host.nbytes if host is not None else nbytes)
        _chk(lib().xm_dev_alloc(C.byref(self.ptr), self.nbytes))
        if host is not None:
            host = np.ascontiguousarray(host)
            _chk(lib().xm_dev_h2d(self.ptr, host.ctypes.data_as(C.c_void_p), self.nbytes))

    def get(self, dtype=np.float64, shape=None):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _chk(lib().xm_dev_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes))
        return out if shape is None else out.reshape(shape)

    def free(self):
        if self.ptr:
            lib().xm_dev_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def to_rm(M, o=None, rows=None):
    """host (m x o) matrix -> the device layout: row-major, pitch OP = o|1, `rows` rows (zero padded)."""
    M = np.asarray(M, dtype=np.float64)
    m, o = M.shape
    out = np.zeros((rows or m, pitch_of(o)))
    out[:m, :o] = M
    return out


def from_rm(buf, m, o):
    return np.asarray(buf).reshape(-1, pitch_of(o))[:m, :o].copy()


# ------------------------------------------------------------------------------------------------ kernel-level calls
def dense_upload(Q):
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64))
    n = Q.shape[0] // 3
    p = C.c_void_p()
    _chk(lib().xm_dense_upload(Q.ctypes.data_as(C.c_void_p), Q.shape[0], n, C.byref(p)))
    d = DevArray.__new__(DevArray)
    d.ptr, d.nbytes = p, 3 * n * dense_ld(n) * 8
    return d


def dense_from_bsr3(rowptr, colidx, blocks):
    """device-side densification of a 3x3-block CSR matrix into the solver's padded row-major layout"""
    require_gpu()
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64); colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    blocks = np.ascontiguousarray(blocks, dtype=np.float64)
    n = rowptr.size - 1
    p = C.c_void_p()
    _chk(lib().xm_dense_from_bsr3(rowptr.ctypes.data_as(C.c_void_p), colidx.ctypes.data_as(C.c_void_p),
                                  blocks.ctypes.data_as(C.c_void_p), n, C.byref(p)))
    d = DevArray.__new__(DevArray)
    d.ptr, d.nbytes = p, 3 * n * dense_ld(n) * 8
    return d


def pad16(W):
    """W (3n x o, o <= 5) at a record pitch of 16 doubles: camera c's 3 x pitch_of(o) row-major block at [16 c, 16 c + 3 pitch_of(o))"""
    W = np.asarray(W, dtype=np.float64)
    n, o = W.shape[0] // 3, W.shape[1]
    rec = 3 * pitch_of(o)
    out = np.zeros((n, 16))
    out[:, :rec] = to_rm(W).reshape(-1)[: n * rec].reshape(n, rec)
    return out.reshape(-1)


def qw_dense(Q, W, alpha=1.0, dq=None, sym=False):
    """alpha * Q @ W on the GPU through xm_qw_dense (Q: 3n x 3n, W: 3n x o); sym=True: the half-traffic symmetric kernel."""
    require_gpu()
    W = np.asarray(W, dtype=np.float64)
    n, o = W.shape[0] // 3, W.shape[1]
    own = dq is None
    dq = dq or dense_upload(Q)
    dW = DevArray(to_rm(W, rows=dense_ld(n)))
    dO = DevArray(nbytes=3 * n * pitch_of(o) * 8)
    _chk((lib().xm_qw_dense_sym if sym else lib().xm_qw_dense)(dq.ptr, n, o, dW.ptr, dO.ptr, alpha, None))
    _chk(lib().xm_dev_sync())
    out = from_rm(dO.get(), 3 * n, o)
    for b in (dW, dO) + ((dq,) if own else ()):
        b.free()
    return out


def dense_to_f32(dq, n):
    """fp32 copy of a device matrix in the padded layout (xm_dense_to_f32): 3n rows of dense_ld(n) floats; .get(np.float32) reads it back"""
    p = C.c_void_p()
    rc = lib().xm_dense_to_f32(dq.ptr, n, C.byref(p))
    d = DevArray.__new__(DevArray)
    d.ptr, d.nbytes = p, 3 * n * dense_ld(n) * 4
    if rc != 0:
        d.free()
        _chk(rc)
    return d


def qw_dense_f32(Q, W, alpha=1.0, sym=False):
    """alpha * fp32(Q) @ W on the GPU, Q read from its fp32 copy and accumulated in f64 (xm_qw_dense_f32; sym=True: xm_qw_dense_sym_f32)"""
    require_gpu()
    W = np.asarray(W, dtype=np.float64)
    n, o = W.shape[0] // 3, W.shape[1]
    dq = dense_upload(Q)
    try:
        d32 = dense_to_f32(dq, n)
    finally:
        dq.free()
    dW = DevArray(to_rm(W, rows=dense_ld(n)))
    dO = DevArray(nbytes=3 * n * pitch_of(o) * 8)
    _chk((lib().xm_qw_dense_sym_f32 if sym else lib().xm_qw_dense_f32)(d32.ptr, n, o, dW.ptr, dO.ptr, alpha, None))
    _chk(lib().xm_dev_sync())
    out = from_rm(dO.get(), 3 * n, o)
    for b in (d32, dW, dO):
        b.free()
    return out


def qw_dense_strip(Qs, n, W, alpha=1.0, ks=0, reps=0):
    """alpha * Qs @ W for a ROW STRIP Qs (3 nloc x 3n, the rows one rank of a row partition owns) through the column-split kernel
    (ks workgroups per camera group; 0 = policy).  Returns (product, ks used, average ms when reps > 0)."""
    require_gpu()
    Qs = np.asarray(Qs, dtype=np.float64); W = np.asarray(W, dtype=np.float64)
    nloc, o, ld = Qs.shape[0] // 3, W.shape[1], dense_ld(n)
    Qp = np.zeros((3 * nloc, ld)); Qp[:, :3 * n] = Qs
    dq = DevArray(Qp); dW = DevArray(to_rm(W, rows=ld)); dO = DevArray(nbytes=3 * nloc * pitch_of(o) * 8)
    ms = C.c_double(); used = C.c_int()
    _chk(lib().xm_qw_dense_strip_ks(dq.ptr, nloc, n, o, dW.ptr, dO.ptr, alpha, ks, reps, C.byref(ms), C.byref(used)))
    out = from_rm(dO.get(), 3 * nloc, o)
    for b in (dq, dW, dO):
        b.free()
    return out, used.value, ms.value


def qw_bsr3(rowptr, colidx, blocks, W, alpha=1.0):
    require_gpu()
    W = np.asarray(W, dtype=np.float64)
    n, o = W.shape[0] // 3, W.shape[1]
    drp = DevArray(np.asarray(rowptr, dtype=np.int64)); dci = DevArray(np.asarray(colidx, dtype=np.int32))
    dbl = DevArray(np.asarray(blocks, dtype=np.float64).reshape(-1))
    dW = DevArray(to_rm(W)); dO = DevArray(nbytes=3 * n * pitch_of(o) * 8)
    _chk(lib().xm_qw_bsr3(drp.ptr, dci.ptr, dbl.ptr, n, o, dW.ptr, dO.ptr, alpha, None))
    _chk(lib().xm_dev_sync())
    out = from_rm(dO.get(), 3 * n, o)
    for b in (drp, dci, dbl, dW, dO):
        b.free()
    return out


def spd_inverse(A):
    """inverse of a symmetric positive definite matrix on the GPU (xm_spd_inverse)"""
    require_gpu()
    A = np.asfortranarray(np.array(A, dtype=np.float64))
    _chk(lib().xm_spd_inverse(A.shape[0], A.ctypes.data_as(C.c_void_p)))
    return np.ascontiguousarray(A)


def spd_solve(A, B):
    """A^-1 B on the GPU for a symmetric positive definite A (only its lower triangle is read; xm_spd_solve): B of shape (n,) or (n, k)"""
    require_gpu()
    A = np.asfortranarray(np.array(A, dtype=np.float64))
    B = np.array(B, dtype=np.float64)
    vec = B.ndim == 1
    X = np.asfortranarray(B.reshape(B.shape[0], -1))
    assert A.ndim == 2 and A.shape[0] == A.shape[1] == X.shape[0]
    _chk(lib().xm_spd_solve(A.shape[0], X.shape[1], A.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p)))
    return X[:, 0].copy() if vec else np.ascontiguousarray(X)


def la_probe(op, a=None, b=None, c=None, m=0, n=0, k=0, nrhs=0, ta=0, tb=0, lower_only=0, info=0, lda=0, ldb=0, ldc=0, q=0.0):
    """one host function of xm_dense_la.hip on host arrays (the test export xm_la_probe, include/xm_amd.h): op is a key of LA_OPS; a, b, c (the
    struct's A, B, C) are contiguous float64 arrays holding the buffers exactly as the device sees them (leading dimensions and padding included), the
    in/out ones are overwritten in place.  Returns info."""
    if op not in LA_OPS:
        raise XmError(f"la_probe: unknown op {op!r}")
    for x in (a, b, c):
        if x is not None and not (isinstance(x, np.ndarray) and x.dtype == np.float64 and (x.flags.c_contiguous or x.flags.f_contiguous) and x.flags.writeable):
            raise XmError("la_probe: the arrays are contiguous writable float64 numpy arrays")
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    p = LaProbe(struct_size=C.sizeof(LaProbe), op=LA_OPS[op], m=m, n=n, k=k, nrhs=nrhs, ta=ta, tb=tb, lower_only=lower_only, info=info, lda=lda,
                ldb=ldb, ldc=ldc, q=q, A=ptr(a), B=ptr(b), C=ptr(c))
    _chk(lib().xm_la_probe(C.byref(p)))
    return int(p.info)


def quat_roundtrip(block):
    """host-only: (stored quaternion, block rebuilt by the product kernel) of a 3x3 block -w * rotation"""
    b = np.ascontiguousarray(block, dtype=np.float64).reshape(9)
    q = np.zeros(4); r = np.zeros(9)
    _chk(lib().xm_sell_quat_roundtrip(b.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p)))
    return q, r.reshape(3, 3)


def sell_layout(rowptr, colidx, ncols=None, slabs=4, lmax=64):
    """host-side description of the sliced-ELL layout (xm_sell.h) -- no GPU involved; used by the CPU tests"""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64); colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    n = rowptr.size - 1
    ncols = n if ncols is None else ncols
    sizes = np.zeros(5, dtype=np.int64)
    args = (rowptr.ctypes.data_as(C.c_void_p), colidx.ctypes.data_as(C.c_void_p), n, ncols, slabs, lmax)
    _chk(lib().xm_sell_layout(*args, sizes.ctypes.data_as(C.c_void_p), *([None] * 7)))
    nsl, nst, npart, nvr, nstore = (int(x) for x in sizes)
    out = dict(nslices=nsl, nsteps=nst, nparts=npart, nvrows=nvr, nstore=nstore, slabs=slabs, ridx=np.zeros(max(npart, 1), dtype=np.int32),
               slice_off=np.zeros(nsl + 1, dtype=np.int64), slab_start=np.zeros(slabs + 1, dtype=np.int32),
               kind=np.zeros(max(nst, 1), dtype=np.uint8), src=np.zeros(max(nst, 1) * 64, dtype=np.int64),
               pslot=np.zeros(max(nsl, 1) * 64, dtype=np.int32), pptr=np.zeros(n + 1, dtype=np.int64))
    _chk(lib().xm_sell_layout(*args, sizes.ctypes.data_as(C.c_void_p),
                              *(out[k].ctypes.data_as(C.c_void_p) for k in ("slice_off", "slab_start", "kind", "src", "pslot", "pptr", "ridx"))))
    return out


def sell_locality(rowptr, colidx, ncols=None, slabs=4, lmax=64):
    """(lines at the native pitch of 72-byte records, of 120-byte records, at the 128-byte pitch) -- host only (xm_sell_locality)"""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64); colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    n = rowptr.size - 1
    out = np.zeros(3, dtype=np.int64)
    _chk(lib().xm_sell_locality(rowptr.ctypes.data_as(C.c_void_p), colidx.ctypes.data_as(C.c_void_p), n, n if ncols is None else ncols, slabs, lmax,
                                out.ctypes.data_as(C.c_void_p)))
    return tuple(int(x) for x in out)


def schur_aggregate_plan(cam, lm, n=None, B=64):
    """aggregate of every camera in the two-level preconditioner of the matrix-free CG form (xm_tuning_t.schur_solver = 3), -1 for the
    anchor camera 0 -- host only"""
    cam = np.ascontiguousarray(cam, dtype=np.int32); lm = np.ascontiguousarray(lm, dtype=np.int32)
    n = int(cam.max()) + 1 if n is None else int(n)
    out = np.zeros(n, dtype=np.int32)
    _chk(lib().xm_schur_aggregate_plan(n, cam.size, cam.ctypes.data_as(C.c_void_p), lm.ctypes.data_as(C.c_void_p), int(B),
                                       out.ctypes.data_as(C.c_void_p)))
    return out


def _focal_args(n, focal, focal_free, preconditioner="jacobi"):
    """the focal scales (ones when None) and the mask of the free ones (None = all) of a call with focal scales, refused here, before
    the device, as the C entry points refuse them: a preconditioner other than "jacobi", a wrong length, a focal that is not finite and > 0"""
    if preconditioner != "jacobi":
        raise XmError(f"refine_focal: the preconditioner {preconditioner!r} has no focal column (only 'jacobi')")
    focal = np.ones(n) if focal is None else np.array(focal, dtype=np.float64).reshape(-1)
    if focal.shape != (n,):
        raise XmError(f"focal: {focal.size} values for {n} cameras")
    if not (np.isfinite(focal).all() and (focal > 0.0).all()):
        raise XmError("focal: every focal scale must be finite and > 0")
    if focal_free is not None:
        focal_free = np.ascontiguousarray(np.asarray(focal_free).reshape(-1) != 0, dtype=np.uint8)
        if focal_free.shape != (n,):
            raise XmError(f"focal_free: {focal_free.size} values for {n} cameras")
    return focal, focal_free


def _focal_group_args(n, focal_group, focal, focal_free, preconditioner="jacobi", linear_solver="iterative_schur"):
    """the arguments of a call with focal groups, refused here as the C entry points refuse them: group_of (n, int32, in [0, G)), focal
    (G; None: ones, with G = max(group_of) + 1), focal_free (G or None); G < 1 or G > n, an entry out of range"""
    group_of = np.asarray(focal_group).reshape(-1)
    if group_of.shape != (n,) or not np.issubdtype(group_of.dtype, np.integer):
        raise XmError(f"focal_group: one integer per camera ({n}) is needed")
    G = (int(group_of.max()) + 1 if n else 0) if focal is None else np.asarray(focal).size
    if G < 1 or G > n:
        raise XmError(f"focal_group: {G} groups for {n} cameras (must lie in [1, n])")
    if group_of.min() < 0 or group_of.max() >= G:
        raise XmError(f"focal_group: an entry lies outside [0, {G})")
    focal, focal_free = _focal_args(G, focal, focal_free, preconditioner)
    return np.ascontiguousarray(group_of, dtype=np.int32), focal, focal_free


def _dist_args(n, dist, dist_free):
    """the radial coefficients (zeros when None) and the mask of the free ones (None = all) of a call with a distortion column, refused
    here, before the device, as the C entry points refuse them: a wrong length, a coefficient that is not finite"""
    dist = np.zeros(n) if dist is None else np.array(dist, dtype=np.float64).reshape(-1)
    if dist.shape != (n,):
        raise XmError(f"distortion: {dist.size} values for {n} cameras")
    if not np.isfinite(dist).all():
        raise XmError("distortion: every radial coefficient must be finite")
    if dist_free is not None:
        dist_free = np.ascontiguousarray(np.asarray(dist_free).reshape(-1) != 0, dtype=np.uint8)
        if dist_free.shape != (n,):
            raise XmError(f"distortion_free: {dist_free.size} values for {n} cameras")
    return dist, dist_free


def undistort_observations(p, cam, focal, distortion):
    """the observations (3 x nobs or nobs x 3 as given) of the cameras cam (nobs) as a pinhole camera at g = 1, k = 0 sees them, from the
    refined focal scales and radial coefficients of bundle_adjust(refine_distortion=True): z = (p0, p1) / p2 = g s u with s = 1 + k rho^2,
    rho = |u|, so rho solves rho (1 + k rho^2) = |z| / g on the monotone branch (Newton from |z| / g, at most 50 iterations, stopped when
    the iterate no longer changes) and the result is (p0 / (g s), p1 / (g s), p2).  With k = 0 the bytes of rescale_observations.
    -> (p, no_root): no_root (nobs, bool) flags the observations that have no root on that branch (beyond the fold of a negative k);
    they are left as given.  A Context built from the result carries the refined calibration: filter_tracks, refine_filtered,
    global_positioning, triangulate_tracks and a second solve then use it.  Host numpy."""
    p = np.array(p, dtype=np.float64)
    cam = np.asarray(cam).reshape(-1)
    g = np.asarray(focal, dtype=np.float64).reshape(-1)[cam]
    k = np.asarray(distortion, dtype=np.float64).reshape(-1)[cam]
    if not (np.isfinite(g).all() and (g > 0.0).all()):
        raise XmError("undistort_observations: every focal scale must be finite and > 0")
    if not np.isfinite(k).all():
        raise XmError("undistort_observations: every radial coefficient must be finite")
    if p.ndim == 2 and p.shape[0] == 3 and p.shape[1] == cam.size:
        rows = p
    elif p.ndim == 2 and p.shape == (cam.size, 3):
        rows = p.T
    else:
        raise XmError("undistort_observations: p must be 3 x nobs or nobs x 3")
    with np.errstate(all="ignore"):
        c = np.hypot(rows[0] / rows[2], rows[1] / rows[2]) / g          # |z| / g
        # k < 0: rho (1 + k rho^2) rises up to the fold rho_f = 1 / sqrt(-3 k), where it is 2 rho_f / 3: beyond that no root
        fold = np.where(k < 0.0, 1.0 / np.sqrt(-3.0 * np.where(k < 0.0, k, -1.0)), np.inf)
        no_root = (~np.isfinite(c) & (k != 0.0)) | ((k < 0.0) & ~(c < 2.0 * fold / 3.0))   # k = 0: nothing to solve, whatever c is
        rho = np.where(no_root, 0.0, c)
        live = ~no_root & (k != 0.0)
        for _ in range(50):
            f = rho * (1.0 + k * rho * rho) - c
            nxt = np.where(live, rho - f / (1.0 + 3.0 * k * rho * rho), rho)
            same = nxt == rho
            rho = nxt
            if same.all():
                break
        s = 1.0 + k * rho * rho
        no_root |= (k != 0.0) & (~np.isfinite(rho) | ~(1.0 + 3.0 * k * rho * rho > 0.0) | ~(rho >= 0.0))
    gs = np.where(no_root, 1.0, np.where(k != 0.0, g * s, g))
    rows[0] /= gs; rows[1] /= gs
    return p, no_root


def rescale_observations(p, cam, focal):
    """the observations (3 x nobs or nobs x 3 as given, p_e = (p0, p1, p2)) of the cameras cam (nobs) as the refined focal scales normalise
    them: (p0 / g, p1 / g, p2) with g = focal[cam].  A Context built from them carries the refined calibration at g = 1: everything
    that has no focal argument (filter_tracks, refine_filtered, global_positioning, a second solve) then uses it."""
    p = np.array(p, dtype=np.float64)
    cam = np.asarray(cam).reshape(-1)
    g = np.asarray(focal, dtype=np.float64).reshape(-1)[cam]
    if not (np.isfinite(g).all() and (g > 0.0).all()):
        raise XmError("rescale_observations: every focal scale must be finite and > 0")
    if p.ndim == 2 and p.shape[0] == 3 and p.shape[1] == cam.size:
        p[0] /= g; p[1] /= g
    elif p.ndim == 2 and p.shape == (cam.size, 3):
        p[:, 0] /= g; p[:, 1] /= g
    else:
        raise XmError("rescale_observations: p must be 3 x nobs or nobs x 3")
    return p


def ba_aggregate_plan(cam, lm, n=None, used=None, B=BA_AGG_CAMS):
    """aggregate of every camera in the opt-in preconditioners of Context.bundle_adjust ("blocks", "two_level"), -1 for a camera without
    a used observation (used: one flag per observation, None = all) -- host only"""
    cam = np.ascontiguousarray(cam, dtype=np.int32); lm = np.ascontiguousarray(lm, dtype=np.int32)
    n = int(cam.max()) + 1 if n is None else int(n)
    u = None if used is None else np.ascontiguousarray(np.asarray(used) != 0, dtype=np.uint8)
    if cam.size != lm.size or (u is not None and u.size != cam.size):
        raise XmError("ba_aggregate_plan: cam, lm and used must have one entry per observation")
    out = np.zeros(n, dtype=np.int32)
    _chk(lib().xm_ba_aggregate_plan(n, cam.size, cam.ctypes.data_as(C.c_void_p), lm.ctypes.data_as(C.c_void_p),
                                    None if u is None else u.ctypes.data_as(C.c_void_p), int(B), out.ctypes.data_as(C.c_void_p)))
    return out


def lm_replay(points, steps, max_iters=50, function_tol=1e-6, gradient_tol=1e-10, parameter_tol=1e-8, nonmonotonic=False, max_nonmonotonic=5):
    """the solvers' Levenberg-Marquardt loop over a script: points (k, 2) = (cost, gmax) per point read, steps (k, 5) = (cost_new, model,
    step2, x2, solved) per candidate -- host only.  Returns a dict: mu and accepted per iteration, status (BA_STATUS name), iters,
    n_accepted, points_read, steps_read, current, returned (accepted step whose point is current / returned, 0 = the start), radius"""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    stp = np.ascontiguousarray(steps, dtype=np.float64).reshape(-1, 5)
    npts, nstp = len(pts), len(stp)
    pts = pts if npts else np.zeros((1, 2)); stp = stp if nstp else np.zeros((1, 5))   # an empty script still passes an address
    mu = np.zeros(len(stp)); acc = np.zeros(len(stp), dtype=np.uint8)
    info = np.zeros(7, dtype=np.int32); radius = C.c_double(0.0)
    _chk(lib().xm_lm_replay(int(max_iters), float(function_tol), float(gradient_tol), float(parameter_tol), int(bool(nonmonotonic)), int(max_nonmonotonic),
                            npts, pts.ctypes.data_as(C.c_void_p), nstp, stp.ctypes.data_as(C.c_void_p), mu.ctypes.data_as(C.c_void_p),
                            acc.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p), C.cast(C.byref(radius), C.c_void_p)))
    k = int(info[1])
    return dict(mu=mu[:k].copy(), accepted=acc[:k].astype(bool), status=BA_STATUS[int(info[0])], iters=k, n_accepted=int(info[2]),
                points_read=int(info[3]), steps_read=int(info[4]), current=int(info[5]), returned=int(info[6]), radius=radius.value)


class CleanPlan:
    """what clean_observations / Context.clean_observations found: keep (bool per observation), cam_index (n) and lm_index (m) -- the new
    number of every camera (the reference's indices_all) and landmark, -1 when dropped -- and info, the fields of xm_clean_result_t"""

    def __init__(self, keep, cam_index, lm_index, info):
        self.keep, self.cam_index, self.lm_index, self.info = keep, cam_index, lm_index, info

    def apply(self, cam, lm, *per_observation):
        """the compacted, re-indexed list on the host: (cam, lm, *arrays) of the kept observations in input order -- the reference's
        edges - 1, landmarks, weights, rgbs, ready for Context(obs=...)"""
        cam = np.asarray(cam); lm = np.asarray(lm)
        if cam.shape != self.keep.shape or lm.shape != self.keep.shape:
            raise XmError("CleanPlan.apply: cam and lm must have one entry per observation of the cleaned list")
        k = self.keep
        out = [self.cam_index[cam[k]], self.lm_index[lm[k]]]
        for a in per_observation:
            a = np.asarray(a)
            if a.shape[:1] != k.shape:
                raise XmError("CleanPlan.apply: a per-observation array has another length than the cleaned list")
            out.append(a[k])
        return tuple(out)


def _clean_options(min_cam_obs, min_lm_obs, swap_first):
    if int(min_cam_obs) < 0 or int(min_lm_obs) < 0:
        raise XmError("clean_observations: negative threshold")
    opt = CleanOptions(); res = CleanResult()
    opt.struct_size, res.struct_size = C.sizeof(CleanOptions), C.sizeof(CleanResult)
    opt.min_cam_obs, opt.min_lm_obs, opt.flags = int(min_cam_obs), int(min_lm_obs), 0 if swap_first else CLEAN_NO_SWAP
    return opt, res


def _clean_plan(keep, ci, li, res):
    return CleanPlan(keep.astype(bool), ci, li, {k: getattr(res, k) for k, _ in CleanResult._fields_ if k not in ("struct_size", "reserved")})


def clean_observations(cam, lm, w=None, n=None, m=None, min_cam_obs=10, min_lm_obs=1, swap_first=True):
    """the reference's checklandmarks on the device for a host list (xm_clean_observations; include/xm_amd.h has the definition): cam, lm
    0-based per observation, w: weights (an observation with w <= 0 counts as deleted; None: all live), n / m: cameras / landmarks (None:
    largest index + 1).  Thresholds are literal: (10, 1) is checklandmarks, (0, 1) the sequence of 2_test_creatematrix.py.  -> CleanPlan"""
    cam = np.ascontiguousarray(cam, dtype=np.int32).reshape(-1); lm = np.ascontiguousarray(lm, dtype=np.int32).reshape(-1)
    if cam.size != lm.size:
        raise XmError("clean_observations: cam and lm must have one entry per observation")
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if w.size != cam.size:
            raise XmError("clean_observations: w must have one entry per observation")
    n = (int(cam.max()) + 1 if cam.size else 0) if n is None else int(n)
    m = (int(lm.max()) + 1 if lm.size else 0) if m is None else int(m)
    opt, res = _clean_options(min_cam_obs, min_lm_obs, swap_first)
    require_gpu()
    keep = np.zeros(cam.size, dtype=np.uint8); ci = np.full(max(n, 0), -1, dtype=np.int32); li = np.full(max(m, 0), -1, dtype=np.int32)
    _chk(lib().xm_clean_observations(n, m, cam.size, cam.ctypes.data_as(C.c_void_p), lm.ctypes.data_as(C.c_void_p),
                                     None if w is None else w.ctypes.data_as(C.c_void_p), C.byref(opt), keep.ctypes.data_as(C.c_void_p),
                                     ci.ctypes.data_as(C.c_void_p), li.ctypes.data_as(C.c_void_p), C.byref(res)))
    return _clean_plan(keep, ci, li, res)


class TrackFilterPlan:
    """what Context.filter_tracks found: keep (bool per observation: used and it stays), reason (uint8 per observation: one TF_REASON_* bit
    where a used observation is dropped, 0 where kept or unused), lm_views (int32 per landmark: observations left), lm_status (uint8 per
    landmark: TF_LM_*) and info, the fields of xm_tf_result_t"""

    def __init__(self, keep, reason, lm_views, lm_status, info):
        self.keep, self.reason, self.lm_views, self.lm_status, self.info = keep, reason, lm_views, lm_status, info

    @property
    def dropped(self):
        """bool per observation: used before the call and dropped by it"""
        return self.reason != 0

    def weights(self, w):
        """w (one weight per observation) with zeros where the call dropped the observation: the argument of Context.set_edge_weights"""
        w = np.array(w, dtype=np.float64).reshape(-1)
        if w.shape != self.reason.shape:
            raise XmError("TrackFilterPlan.weights: w must have one entry per observation of the filtered list")
        w[self.reason != 0] = 0.0
        return w

    def apply(self, *per_observation):
        """the rows of the kept observations, in input order, of every array given (cam, lm, p, w, ...)"""
        k = self.keep
        out = []
        for a in per_observation:
            a = np.asarray(a)
            if a.shape[:1] != k.shape:
                raise XmError("TrackFilterPlan.apply: a per-observation array has another length than the filtered list")
            out.append(a[k])
        return tuple(out)


def gp_limits():
    """-> dict(light_max: observations of the longest landmark that one thread walks in Context.global_positioning (longer ones get a
    workgroup), cam_pass: observations a wavefront takes from a camera's list in one pass, threads: of a heavy landmark's workgroup)"""
    out = np.zeros(3, dtype=np.int64)
    _chk(lib().xm_gp_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(light_max=int(out[0]), cam_pass=int(out[1]), threads=int(out[2]))


def gp_pair_limits():
    """-> dict(light_max: incidences (ends of participating pairs) of a camera that one thread walks in Context.global_positioning with
    pairs (a camera with more gets a workgroup), threads: of that workgroup)"""
    out = np.zeros(2, dtype=np.int64)
    _chk(lib().xm_gp_pair_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(light_max=int(out[0]), threads=int(out[1]))


def _gp_pairs_struct(n, pairs, constraint, calibrated, reweight_scale, fix_centres, want_sigma=True):
    """xm_gp_pairs_t from the Python arguments -> (struct, arrays kept alive, sigma or None)"""
    if constraint not in GP_CONSTRAINT:
        raise XmError(f"unknown constraint {constraint!r} (one of {', '.join(GP_CONSTRAINT)})")
    g = GpPairs()
    g.struct_size = C.sizeof(GpPairs)
    g.constraint, g.flags, g.reweight_scale = GP_CONSTRAINT[constraint], (GP_FIX_CENTRES if fix_centres else 0), float(reweight_scale)
    keep, sigma = [], None
    if pairs is not None:
        pi = np.ascontiguousarray(pairs[0], dtype=np.int32); pj = np.ascontiguousarray(pairs[1], dtype=np.int32)
        trel = np.ascontiguousarray(np.asarray(pairs[2], dtype=np.float64).reshape(pi.size, 3))
        assert pj.shape == pi.shape
        keep += [pi, pj, trel]
        g.npairs, g.pi, g.pj, g.trel = pi.size, pi.ctypes.data_as(C.c_void_p), pj.ctypes.data_as(C.c_void_p), trel.ctypes.data_as(C.c_void_p)
        if len(pairs) > 3 and pairs[3] is not None:
            valid = np.ascontiguousarray(np.asarray(pairs[3]).reshape(pi.size) != 0, dtype=np.uint8)
            keep.append(valid); g.valid = valid.ctypes.data_as(C.c_void_p)
        if want_sigma:
            sigma = np.zeros(max(pi.size, 1)); g.sigma = sigma.ctypes.data_as(C.c_void_p)
            sigma = sigma[: pi.size]
    if calibrated is not None:
        cal = np.ascontiguousarray(np.asarray(calibrated).reshape(n) != 0, dtype=np.uint8)
        keep.append(cal); g.calibrated = cal.ctypes.data_as(C.c_void_p)
    return g, keep, sigma


def gp_random_start(n, m, seed=1):
    """the start of GLOMAP's global positioning: 100 U(-1, 1)^3 for every camera centre (3 x n) and point (3 x m)
    (global_positioning.cc:141, :235), cameras first, from numpy's default Generator.  DEPARTURE: the reference draws from std::mt19937 in
    hash-map order, which has no order-independent restatement."""
    rng = np.random.default_rng(seed)
    return 100.0 * rng.uniform(-1.0, 1.0, (3, int(n))), 100.0 * rng.uniform(-1.0, 1.0, (3, int(m)))


def track_filter_limits():
    """-> dict(light_max: observations of the longest landmark that one thread walks (longer ones get a workgroup), tile: rays per LDS tile
    of the workgroup form, threads: per workgroup)"""
    out = np.zeros(3, dtype=np.int64)
    _chk(lib().xm_track_filter_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(light_max=int(out[0]), tile=int(out[1]), threads=int(out[2]))


class TriangulationPlan:
    """what Context.triangulate_tracks found: P (3 x m: the triangulated point of every accepted landmark, the column that was given for
    every other), keep (bool per observation: a member of an accepted landmark), reason (uint8 per observation: TRI_REASON_*, 0 where
    kept), views (int32 per landmark: members), status (uint8 per landmark: TRI_LM_*), support and hypothesis (int32 per landmark: the
    winning count and its entry of the pair schedule, -1 when there was none) and info, the fields of xm_tri_result_t"""

    def __init__(self, P, keep, reason, views, status, support, hypothesis, info):
        self.P, self.keep, self.reason, self.views, self.status = P, keep, reason, views, status
        self.support, self.hypothesis, self.info = support, hypothesis, info

    def weights(self, w):
        """w (one weight per observation) where kept and 0 elsewhere: the argument of Context.set_edge_weights (give it the weights the
        candidates had before they were dropped, so that a re-admitted observation gets its weight back)"""
        w = np.array(w, dtype=np.float64).reshape(-1)
        if w.shape != self.keep.shape:
            raise XmError("TriangulationPlan.weights: w must have one entry per observation of the list")
        w[~self.keep] = 0.0
        return w

    def apply(self, *per_observation):
        """the rows of the kept observations, in input order, of every array given (cam, lm, p, w, ...)"""
        k = self.keep
        out = []
        for a in per_observation:
            a = np.asarray(a)
            if a.shape[:1] != k.shape:
                raise XmError("TriangulationPlan.apply: a per-observation array has another length than the list")
            out.append(a[k])
        return tuple(out)


def triangulate_limits():
    """-> dict(light_max: observations of the longest landmark that one wavefront holds in Context.triangulate_tracks (longer ones get a
    workgroup), tile: rays per tile and hypotheses per batch of the workgroup form, threads: per workgroup)"""
    out = np.zeros(3, dtype=np.int64)
    _chk(lib().xm_triangulate_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(light_max=int(out[0]), tile=int(out[1]), threads=int(out[2]))


class PrunePlan:
    """what prune_weakly_connected / Context.prune_weakly_connected found: cluster_id (int32 per camera: 0 is the largest cluster, -1 a
    pruned image), obs_count (int32 per camera), info (the fields of xm_prune_result_t) and pairs -- the visibility graph as (i, j, count),
    three int32 arrays in (i, j) order, or None when it was not asked for"""

    def __init__(self, cluster_id, obs_count, info, pairs=None, cam=None):
        self.cluster_id, self.obs_count, self.info, self.pairs = cluster_id, obs_count, info, pairs
        self._cam = cam   # camera of every observation of the list the call was made on

    def keep(self, cluster=0):
        """bool per observation of the pruned list: its camera lies in `cluster`"""
        if self._cam is None:
            raise XmError("PrunePlan: the observations' cameras are not known here")
        return self.cluster_id[self._cam] == int(cluster)

    def weights(self, w, cluster=0):
        """w (one weight per observation) with zeros for the observations of cameras outside `cluster`: the w of the
        clean_observations call that drops and renumbers those cameras for the next context"""
        w = np.array(w, dtype=np.float64).reshape(-1)
        k = self.keep(cluster)
        if w.shape != k.shape:
            raise XmError("PrunePlan.weights: w must have one entry per observation of the pruned list")
        w[~k] = 0.0
        return w

    def apply(self, *per_observation, cluster=0):
        """the rows of the observations whose camera lies in `cluster`, in input order, of every array given (cam, lm, p, w, ...)"""
        k = self.keep(cluster)
        out = []
        for a in per_observation:
            a = np.asarray(a)
            if a.shape[:1] != k.shape:
                raise XmError("PrunePlan.apply: a per-observation array has another length than the pruned list")
            out.append(a[k])
        return tuple(out)


def prune_limits():
    """-> dict(tile: camera bins per LDS tile of the covisibility histogram, threads: per workgroup, group_max: entries of the longest
    landmark list that a group of `group` lanes walks (longer ones: the whole workgroup), select_bits: low bits of the second level of the
    order statistics)"""
    out = np.zeros(5, dtype=np.int64)
    _chk(lib().xm_prune_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(tile=int(out[0]), threads=int(out[1]), group_max=int(out[2]), group=int(out[3]), select_bits=int(out[4]))


def _prune_options(min_covisibility, min_num_images, min_num_observations, min_threshold):
    if int(min_covisibility) < 0 or int(min_num_images) < 0 or int(min_num_observations) < 0:
        raise XmError("prune_weakly_connected: negative option")
    if not np.isfinite(min_threshold):
        raise XmError("prune_weakly_connected: min_threshold is not finite")
    opt = PruneOptions(); res = PruneResult()
    opt.struct_size, res.struct_size = C.sizeof(PruneOptions), C.sizeof(PruneResult)
    opt.min_covisibility, opt.min_num_images, opt.min_num_observations = int(min_covisibility), int(min_num_images), int(min_num_observations)
    opt.min_threshold = float(min_threshold)
    return opt, res


def _prune_call(call, n, pairs, cam):
    """call(cluster_id, obs_count, pairs struct or None, result) -> rc; with pairs a second call sized by the first one's n_edges"""
    cid = np.full(max(n, 0), -1, dtype=np.int32); cnt = np.zeros(max(n, 0), dtype=np.int32)
    res = PruneResult(); res.struct_size = C.sizeof(PruneResult)
    got = None
    if pairs:
        cap = 0 if pairs is True else int(pairs)          # True: ask for the size first; a number: the capacity to try
        pi, pj, pc = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        pp = PrunePairs(cap, pi.ctypes.data_as(C.c_void_p), pj.ctypes.data_as(C.c_void_p), pc.ctypes.data_as(C.c_void_p))
        _chk(call(cid, cnt, C.byref(pp), res))
        if res.n_edges > cap and pairs is True:
            cap = int(res.n_edges)
            pi, pj, pc = (np.zeros(cap, dtype=np.int32) for _ in range(3))
            pp = PrunePairs(cap, pi.ctypes.data_as(C.c_void_p), pj.ctypes.data_as(C.c_void_p), pc.ctypes.data_as(C.c_void_p))
            _chk(call(cid, cnt, C.byref(pp), res))
        if res.n_edges <= cap:
            e = int(res.n_edges)
            got = (pi[:e], pj[:e], pc[:e])
    else:
        _chk(call(cid, cnt, None, res))
    info = {k: getattr(res, k) for k, _ in PruneResult._fields_ if k != "struct_size"}
    return PrunePlan(cid, cnt, info, got, cam)


def prune_weakly_connected(cam, lm, n=None, m=None, w=None, min_covisibility=5, min_num_images=2, min_num_observations=0, min_threshold=20.0,
                           pairs=False):
    """GLOMAP's PruneWeaklyConnectedImages (reconstruction_pruning.cc:6-84) on the device for a host list (xm_prune_weakly_connected;
    include/xm_amd.h has the definition): cam, lm 0-based per observation, w: weights (an observation with w <= 0 is not used; None: all),
    n / m: cameras / landmarks (None: largest index + 1).  pairs: True also returns the visibility graph (a second call sized by the
    first), a number tries that capacity only (too small: plan.pairs is None and plan.info["n_edges"] says what is needed).  -> PrunePlan"""
    cam = np.ascontiguousarray(cam, dtype=np.int32).reshape(-1); lm = np.ascontiguousarray(lm, dtype=np.int32).reshape(-1)
    if cam.size != lm.size:
        raise XmError("prune_weakly_connected: cam and lm must have one entry per observation")
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if w.size != cam.size:
            raise XmError("prune_weakly_connected: w must have one entry per observation")
    n = (int(cam.max()) + 1 if cam.size else 0) if n is None else int(n)
    m = (int(lm.max()) + 1 if lm.size else 0) if m is None else int(m)
    opt, _ = _prune_options(min_covisibility, min_num_images, min_num_observations, min_threshold)
    require_gpu()

    def call(cid, cnt, pp, res):
        return lib().xm_prune_weakly_connected(n, m, cam.size, cam.ctypes.data_as(C.c_void_p), lm.ctypes.data_as(C.c_void_p),
                                               None if w is None else w.ctypes.data_as(C.c_void_p), C.byref(opt), cid.ctypes.data_as(C.c_void_p),
                                               cnt.ctypes.data_as(C.c_void_p), pp, C.byref(res))
    return _prune_call(call, n, pairs, cam)


class PairFilterPlan:
    """what pair_filter found: count (int32 per observation: the pairs that flagged it), outlier (bool per observation), stats (a structured
    array with one xm_pair_stat_t per pair) and info, the fields of xm_pair_result_t"""

    def __init__(self, count, outlier, stats, info):
        self.count, self.outlier, self.stats, self.info = count, outlier, stats, info

    def apply(self, *per_observation):
        """the rows of the observations that are no outliers, in input order, of every array given (cam, lm, p, w, ...): what the reference
        hands to checklandmarks (5_test_ceres.py:423-426)"""
        k = ~self.outlier
        out = []
        for a in per_observation:
            a = np.asarray(a)
            if a.shape[:1] != k.shape:
                raise XmError("PairFilterPlan.apply: a per-observation array has another length than the filtered list")
            out.append(a[k])
        return tuple(out)


def pair_filter_limits():
    """-> dict(lds_joint: the largest joint set of a pair that is sorted in LDS (larger ones take the workspace path), threads: per workgroup,
    workspace_groups: workgroups of the workspace path, small_joint: the largest joint set of the small LDS instantiation)"""
    out = np.zeros(4, dtype=np.int64)
    _chk(lib().xm_pair_filter_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(lds_joint=int(out[0]), threads=int(out[1]), workspace_groups=int(out[2]), small_joint=int(out[3]))


def pair_filter(cam, lm, p, pairs_i, pairs_j, R, n=None, m=None, min_joint=20, trim=0.05, dist_pct=90, err_pct=95, mad_factor=3.0, min_flags=1,
                skip_row0=False):
    """the reference's pairwise relative-rotation filter (5_test_ceres.py:316-431) on the device (xm_pair_filter; include/xm_amd.h has the
    definition): cam, lm 0-based per observation, p nobs x 3 camera-frame points; pairs_i, pairs_j the cameras of every pair and R (npairs x
    3 x 3) its relative rotation, dst ~ R src for src in camera pairs_i and dst in camera pairs_j.  The options are literal; the defaults are
    the reference's constants.  skip_row0: the reference's quirk that observation row 0 never takes part.  -> PairFilterPlan"""
    cam = np.ascontiguousarray(cam, dtype=np.int32).reshape(-1); lm = np.ascontiguousarray(lm, dtype=np.int32).reshape(-1)
    p = np.ascontiguousarray(p, dtype=np.float64)
    if cam.size != lm.size or p.shape != (cam.size, 3):
        raise XmError("pair_filter: cam, lm and p (nobs x 3) must have one entry per observation")
    pi = np.ascontiguousarray(pairs_i, dtype=np.int32).reshape(-1); pj = np.ascontiguousarray(pairs_j, dtype=np.int32).reshape(-1)
    R = np.ascontiguousarray(R, dtype=np.float64)
    if pi.size != pj.size or R.size != 9 * pi.size or (pi.size and R.shape[-2:] != (3, 3)):
        raise XmError("pair_filter: pairs_i, pairs_j and R (npairs x 3 x 3) must have one entry per pair")
    if int(min_joint) < 0 or int(min_flags) < 0 or not trim >= 0 or not dist_pct >= 0 or not err_pct >= 0 or not mad_factor >= 0:
        raise XmError("pair_filter: negative option")
    if not trim < 0.5:
        raise XmError("pair_filter: trim must stay below 0.5")
    if dist_pct > 100 or err_pct > 100:
        raise XmError("pair_filter: a percentile above 100")
    n = (int(cam.max()) + 1 if cam.size else 0) if n is None else int(n)
    m = (int(lm.max()) + 1 if lm.size else 0) if m is None else int(m)
    opt = PairOptions(int(min_joint), int(min_flags), PAIR_SKIP_ROW0 if skip_row0 else 0, float(trim), float(dist_pct), float(err_pct), float(mad_factor))
    res = PairResult(); res.struct_size = C.sizeof(PairResult)
    require_gpu()
    count = np.zeros(cam.size, dtype=np.int32); outlier = np.zeros(cam.size, dtype=np.uint8); stats = np.zeros(pi.size, dtype=PAIR_STAT_DTYPE)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_pair_filter(n, m, cam.size, P(cam), P(lm), P(p), pi.size, P(pi), P(pj), P(R), C.byref(opt), P(count), P(outlier), P(stats),
                              C.byref(res)))
    return PairFilterPlan(count, outlier.astype(bool), stats, {k: getattr(res, k) for k, _ in PairResult._fields_ if k not in ("struct_size", "reserved")})


class LiftPlan:
    """what lift_observations returns: the observation list cam, lm (int32), p (nout x 3), w in camera-then-track order, row (the input
    row of every output), threshold (per camera, NaN where the camera was skipped) and info, the fields of xm_lift_result_t"""

    def __init__(self, cam, lm, p, w, row, threshold, info, nrows):
        self.cam, self.lm, self.p, self.w, self.row, self.threshold, self.info, self.nrows = cam, lm, p, w, row, threshold, info, nrows

    def carry(self, *per_row_arrays):
        """the rows of every array given (colours, ...) that belong to the outputs, in output order"""
        out = []
        for a in per_row_arrays:
            a = np.asarray(a)
            if a.shape[:1] != (self.nrows,):
                raise XmError("LiftPlan.carry: a per-row array has another length than the match table")
            out.append(a[self.row])
        return tuple(out)


def lift_limits():
    """-> dict(lds_rows: most rows of a camera that are sorted in LDS (larger cameras take the workspace path), threads: per workgroup,
    workspace_groups: workgroups of the workspace path, small_rows: most rows of a camera in the small LDS instantiation)"""
    out = np.zeros(4, dtype=np.int64)
    _chk(lib().xm_lift_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(lds_rows=int(out[0]), threads=int(out[1]), workspace_groups=int(out[2]), small_rows=int(out[3]))


def _lift_map(x, what, i):
    """one entry of depth / conf -> (pointer, on_device, (h, w), the object that keeps the memory alive)"""
    if x is None:
        return 0, None, None, None
    if isinstance(x, tuple) and len(x) == 3 and isinstance(x[0], DevArray):
        d, h, w = x
        if int(h) * int(w) * 4 > d.nbytes:
            raise XmError(f"lift_observations: {what}[{i}]: the device buffer is smaller than h x w float32")
        return int(d.ptr.value or 0), True, (int(h), int(w)), d
    if isinstance(x, np.ndarray):
        if x.ndim != 2 or x.dtype != np.float32:
            raise XmError(f"lift_observations: {what}[{i}] must be a 2-D float32 array")
        x = np.ascontiguousarray(x)
        return x.ctypes.data, False, (int(x.shape[0]), int(x.shape[1])), x
    if hasattr(x, "data_ptr") and hasattr(x, "shape") and hasattr(x, "is_cuda"):
        if len(x.shape) != 2 or "float32" not in str(getattr(x, "dtype", "float32")):
            raise XmError(f"lift_observations: {what}[{i}] must be a 2-D float32 tensor")
        if hasattr(x, "is_contiguous") and not x.is_contiguous():
            x = x.contiguous()
        return int(x.data_ptr()), bool(x.is_cuda), (int(x.shape[0]), int(x.shape[1])), x
    raise XmError(f"lift_observations: {what}[{i}] is none of None, a float32 array, (DevArray, h, w) or a tensor")


def lift_observations(cam, lm, xy, depth, conf, K, n=None, m=None, margin=10, depth_pct=95.0):
    """the reference's depth lift (5_test_ceres.py:191-204, :244-296) on the device (xm_lift_observations; include/xm_amd.h has the
    definition): cam, lm 0-based per row of the match table, xy nrows x 2 pixel positions; depth, conf: one entry per camera -- None, a 2-D
    float32 array (host), (DevArray, h, w), or an object with data_ptr(), shape and is_cuda (a torch tensor); conf may be None altogether
    (every weight 1); K: n x 3 x 3 intrinsics, inverted here.  Host and device maps cannot be mixed.  -> LiftPlan"""
    cam = np.ascontiguousarray(cam, dtype=np.int32).reshape(-1); lm = np.ascontiguousarray(lm, dtype=np.int32).reshape(-1)
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if cam.size != lm.size or xy.shape != (cam.size, 2):
        raise XmError("lift_observations: cam, lm and xy (nrows x 2) must have one entry per row")
    depth = list(depth)
    n = len(depth) if n is None else int(n)
    m = (int(lm.max()) + 1 if lm.size else 0) if m is None else int(m)
    if len(depth) != n or (conf is not None and len(conf) != n):
        raise XmError("lift_observations: depth and conf must have one entry per camera")
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (n, 3, 3):
        raise XmError("lift_observations: K must be n x 3 x 3")
    if int(margin) < 0:
        raise XmError("lift_observations: negative margin")
    if not (depth_pct >= 0 and depth_pct <= 100):
        raise XmError("lift_observations: a percentile outside [0, 100]")
    Kinv = np.ascontiguousarray(np.linalg.inv(K)) if n else np.zeros((0, 3, 3))
    hw = np.zeros((n, 2), dtype=np.int32); dptr = np.zeros(n, dtype=np.uint64); cptr = np.zeros(n, dtype=np.uint64)
    where = set(); alive = []
    for i in range(n):
        pd, on_d, shp, keep = _lift_map(depth[i], "depth", i)
        pc, on_c, shc, keepc = _lift_map(None if conf is None else conf[i], "conf", i)
        if pd == 0:
            continue                                   # (no depth map: the camera's confidence map is not looked at)
        if pc and shc != shp:
            raise XmError(f"lift_observations: depth[{i}] and conf[{i}] differ in shape")
        where.add(on_d)
        if pc:
            where.add(on_c)
        hw[i] = shp; dptr[i] = pd; cptr[i] = pc; alive += [keep, keepc]
    if len(where) > 1:
        raise XmError("lift_observations: host and device maps are mixed in one call")
    opt = LiftOptions(int(margin), LIFT_MAPS_ON_DEVICE if where == {True} else 0, float(depth_pct))
    res = LiftResult(); res.struct_size = C.sizeof(LiftResult)
    require_gpu()
    nr = cam.size
    ocam = np.zeros(nr, dtype=np.int32); olm = np.zeros(nr, dtype=np.int32); orow = np.zeros(nr, dtype=np.int32)
    op = np.zeros((nr, 3)); ow = np.zeros(nr); thr = np.full(n, np.nan); nout = C.c_int64(0)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_lift_observations(n, m, nr, P(cam), P(lm), P(xy), P(hw), P(dptr), None if conf is None else P(cptr), P(Kinv), C.byref(opt), P(ocam),
                                    P(olm), P(op), P(ow), P(orow), C.byref(nout), P(thr), C.byref(res)))
    del alive
    k = nout.value
    info = {f: getattr(res, f) for f, _ in LiftResult._fields_ if f not in ("struct_size", "reserved")}
    return LiftPlan(ocam[:k].copy(), olm[:k].copy(), op[:k].copy(), ow[:k].copy(), orow[:k].copy(), thr, info, nr)


class TrackTable:
    """what build_tracks returns: one row per touched feature of a registered image in a kept track, image ascending, then feature
    ascending: cam, feat (the index in the image), track (int32), xy (rows x 2, the input's bits); m, the number of tracks; label (per
    global feature: its track or a negative TRACK_* code); info, the fields of xm_tracks_result_t; foff, the feature offsets.
    lift_observations(t.cam, t.track, t.xy, depth, conf, K, n=n, m=t.m) takes it as it is"""

    def __init__(self, cam, feat, track, xy, m, label, info, foff):
        self.cam, self.feat, self.track, self.xy, self.m, self.label, self.info, self.foff = cam, feat, track, xy, m, label, info, foff

    @property
    def feature(self):
        """the global feature index of every row"""
        return self.foff[self.cam] + self.feat

    def carry(self, *per_feature_arrays):
        """the rows of every array given (colours, descriptors, ...; one entry per global feature) that belong to the table's rows"""
        out = []
        g = self.feature
        for a in per_feature_arrays:
            a = np.asarray(a)
            if a.shape[:1] != (int(self.foff[-1]),):
                raise XmError("TrackTable.carry: a per-feature array has another length than the feature list")
            out.append(a[g])
        return tuple(out)


def tracks_limits():
    """-> dict(lds_rows: most touched features of an image that are sorted in LDS (larger images take the workspace path), threads: per
    workgroup, workspace_groups: workgroups of the workspace path, small_rows: most touched features of an image in the small LDS instantiation)"""
    out = np.zeros(4, dtype=np.int64)
    _chk(lib().xm_tracks_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(lds_rows=int(out[0]), threads=int(out[1]), workspace_groups=int(out[2]), small_rows=int(out[3]))


def _tracks_foff(foff_or_counts, nfeat):
    """feature offsets from either the offsets themselves (n + 1 entries, the last one the number of features) or the counts per image"""
    a = np.ascontiguousarray(foff_or_counts, dtype=np.int64).reshape(-1)
    if a.size and a[0] == 0 and a[-1] == nfeat and np.all(np.diff(a) >= 0):   # (an array that reads both ways, as [0, 0, 5] does, is the offsets)
        return a
    if int(a.sum()) != nfeat:
        raise XmError("build_tracks: foff_or_counts is neither the offsets (n + 1 entries ending in the number of features) nor the counts per image")
    return np.concatenate([[0], np.cumsum(a)]).astype(np.int64)


def _tracks_matches(matches, npairs):
    if isinstance(matches, tuple) and len(matches) == 3:
        moff, f1, f2 = (np.ascontiguousarray(matches[0], dtype=np.int64).reshape(-1), np.ascontiguousarray(matches[1], dtype=np.int32).reshape(-1),
                        np.ascontiguousarray(matches[2], dtype=np.int32).reshape(-1))
    else:
        per = [np.asarray(x, dtype=np.int32).reshape(-1, 2) for x in matches]
        moff = np.concatenate([[0], np.cumsum([x.shape[0] for x in per])]).astype(np.int64)
        cat = np.concatenate(per, axis=0) if per else np.zeros((0, 2), dtype=np.int32)
        f1, f2 = np.ascontiguousarray(cat[:, 0]), np.ascontiguousarray(cat[:, 1])
    if moff.size != npairs + 1 or f1.size != f2.size or (moff.size and int(moff[-1]) != f1.size):
        raise XmError("build_tracks: matches must be (moff, f1, f2) with npairs + 1 offsets ending in the number of matches, or one (k, 2) array per pair")
    return moff, f1, f2


def build_tracks(foff_or_counts, xy, pi, pj, matches, registered=None, min_views=3, max_views=1000000, max_tracks=10000000,
                 thres_inconsistency=10.0, conflict="split"):
    """feature tracks from pairwise matches on the device (xm_build_tracks; include/xm_amd.h has the definition and where it departs from
    the reference's fork of GLOMAP): foff_or_counts: the feature offsets (n + 1) or the feature counts (n) of the images; xy: features x 2;
    pi, pj: the images of every pair, 0-based; matches: (moff, f1, f2) or one (k, 2) array of feature indices per pair; registered: per
    image or None; conflict: "drop", "glomap", "split" or "split_device" (the split policy with XM_TRACKS_SPLIT_DEVICE: the conflicted components
    are split on the device, with the same bits).  -> TrackTable"""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise XmError("build_tracks: xy must be features x 2")
    foff = _tracks_foff(foff_or_counts, xy.shape[0])
    n = foff.size - 1
    pi = np.ascontiguousarray(pi, dtype=np.int32).reshape(-1); pj = np.ascontiguousarray(pj, dtype=np.int32).reshape(-1)
    if pi.size != pj.size:
        raise XmError("build_tracks: pi and pj must have one entry per pair")
    moff, f1, f2 = _tracks_matches(matches, pi.size)
    reg = None
    if registered is not None:
        reg = np.ascontiguousarray(np.asarray(registered) != 0, dtype=np.uint8).reshape(-1)
        if reg.size != n:
            raise XmError("build_tracks: registered must have one entry per image")
    if isinstance(conflict, str) and conflict not in TRACKS_POLICIES:
        raise XmError(f"build_tracks: conflict must be one of {sorted(TRACKS_POLICIES)} (or an XM_TRACKS_* number)")
    opt = TracksOptions(int(min_views), int(max_views), int(TRACKS_POLICIES.get(conflict, conflict)), int(max_tracks), float(thres_inconsistency),
                        TRACKS_SPLIT_DEVICE if conflict == "split_device" else 0)
    res = TracksResult(); res.struct_size = C.sizeof(TracksResult)
    F = xy.shape[0]
    ocam = np.zeros(F, dtype=np.int32); ofeat = np.zeros(F, dtype=np.int32); otrack = np.zeros(F, dtype=np.int32); oxy = np.zeros((F, 2))
    label = np.full(F, TRACK_UNTOUCHED, dtype=np.int32); nout = C.c_int64(0)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_build_tracks(n, P(foff), P(xy), P(reg), pi.size, P(pi), P(pj), P(moff), P(f1), P(f2), C.byref(opt), P(ocam), P(ofeat), P(otrack),
                               P(oxy), C.byref(nout), P(label), C.byref(res)))
    k = nout.value
    info = {f: getattr(res, f) for f, _ in TracksResult._fields_ if f != "struct_size"}
    return TrackTable(ocam[:k].copy(), ofeat[:k].copy(), otrack[:k].copy(), oxy[:k].copy(), int(res.ntracks), label, info, foff)


def split_host(foff_or_counts, nfeat, eu, ev):
    """the test export xm_tracks_split_host: rule 4's XM_TRACKS_SPLIT over the edges (eu, ev) of global feature indices, on the host.
    -> (label per feature: the smallest member of its set, -1 for a feature in no edge; distinct edges; unions refused)"""
    foff = _tracks_foff(foff_or_counts, int(nfeat))
    eu = np.ascontiguousarray(eu, dtype=np.int32).reshape(-1); ev = np.ascontiguousarray(ev, dtype=np.int32).reshape(-1)
    if eu.size != ev.size:
        raise XmError("split_host: eu and ev must have one entry per edge")
    label = np.full(int(nfeat), -1, dtype=np.int32); d = C.c_int64(0); r = C.c_int64(0)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_tracks_split_host(foff.size - 1, P(foff), eu.size, P(eu), P(ev), P(label), C.byref(d), C.byref(r)))
    return label, d.value, r.value


def split_device(foff_or_counts, nfeat, eu, ev):
    """the test export xm_tracks_split_device: as split_host, on the device with the split code of build_tracks(conflict="split_device");
    every component of the edges is treated as one to split.  -> (label, distinct edges, unions refused)"""
    foff = _tracks_foff(foff_or_counts, int(nfeat))
    eu = np.ascontiguousarray(eu, dtype=np.int32).reshape(-1); ev = np.ascontiguousarray(ev, dtype=np.int32).reshape(-1)
    if eu.size != ev.size:
        raise XmError("split_device: eu and ev must have one entry per edge")
    label = np.full(int(nfeat), -1, dtype=np.int32); d = C.c_int64(0); r = C.c_int64(0)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_tracks_split_device(foff.size - 1, P(foff), eu.size, P(eu), P(ev), P(label), C.byref(d), C.byref(r)))
    return label, d.value, r.value


def tracks_split_limits():
    """-> dict(wave_endpoints, wave_edges: most endpoints and most raw (listed) edges of a conflicted component that one wavefront splits;
    group_edges: most raw edges of one that a workgroup splits (above: the host splitter); threads: per workgroup).  Needs no device"""
    out = np.zeros(4, dtype=np.int64)
    _chk(lib().xm_tracks_split_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(wave_endpoints=int(out[0]), wave_edges=int(out[1]), group_edges=int(out[2]), threads=int(out[3]))


def tracks_split_stats():
    """what this thread's most recent build_tracks or split_device did -> dict(wave, group, host: components split in the wavefront form, in the
    workgroup form, on the host; edges_device, edges_host: raw edges given to either; distinct, refused).  All 0 unless the device split ran"""
    out = np.zeros(8, dtype=np.int64)
    _chk(lib().xm_tracks_split_stats(out.ctypes.data_as(C.c_void_p)))
    return dict(zip(("wave", "group", "host", "edges_device", "edges_host", "distinct", "refused"), (int(x) for x in out[:7])))


class ViewGraphPlan:
    """what view_graph_filter returns: inlier (uint8 per listed match), pair_inliers (int32 per pair), pair_status (int32 per pair: VG_VALID,
    VG_INVALID_IN, VG_FEW_INLIERS, VG_LOW_RATIO, VG_ROTATION or VG_OUTSIDE, the first rule that dropped the pair), valid (pair_status ==
    VG_VALID), registered (uint8 per image: membership in the largest component), matches (moff, f1, f2: the inliers of the pairs still
    valid, in input order, an entry of moff per listed pair), info (the fields of xm_vg_result_t).  matches and registered go into
    build_tracks, and into a second view_graph_filter call with valid_in=plan.valid, as they are"""

    def __init__(self, inlier, pair_inliers, pair_status, registered, matches, info, pi, pj, Rrel):
        self.inlier, self.pair_inliers, self.pair_status, self.registered, self.matches, self.info = inlier, pair_inliers, pair_status, registered, matches, info
        self.valid = (pair_status == VG_VALID).astype(np.uint8)
        self._pi, self._pj, self._Rrel = pi, pj, Rrel

    def pairs(self):
        """-> pi, pj, Rrel (k x 3 x 3) of the valid pairs: what pair_filter takes"""
        k = np.flatnonzero(self.valid)
        return self._pi[k], self._pj[k], (None if self._Rrel is None else self._Rrel.reshape(-1, 3, 3)[k])


def view_graph_limits():
    """-> dict(group_matches: most matches of a pair that one workgroup runs (larger pairs run in chunks of this size over a workspace),
    threads: per workgroup, wave_matches: most matches of a pair that one wavefront runs, max_rounds: most hooking rounds)"""
    out = np.zeros(4, dtype=np.int64)
    _chk(lib().xm_view_graph_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(group_matches=int(out[0]), threads=int(out[1]), wave_matches=int(out[2]), max_rounds=int(out[3]))


def _vg_array(x, dtype, shape, what):
    if x is None:
        return None
    a = np.ascontiguousarray(x, dtype=dtype)
    if a.size != int(np.prod(shape)):
        raise XmError(f"view_graph_filter: {what} must be {' x '.join(str(v) for v in shape)}")
    return a.reshape(shape)


def view_graph_filter(foff_or_counts, xy, pi, pj, model, matches, focal=None, Kinv=None, bearing=None, Rrel=None, trel=None, FH=None, valid_in=None,
                      registered_in=None, rot=None, score=True, max_epipolar_error_E=1.0, max_epipolar_error_F=4.0, max_epipolar_error_H=4.0,
                      min_inlier_num=30, min_inlier_ratio=0.25, max_rotation_error_deg=10.0, cos_max_rotation_error=None):
    """two-view match verification and view-graph pruning on the device (xm_view_graph_filter; include/xm_amd.h has the definition and the
    lines of the reference's fork of GLOMAP it stands for): foff_or_counts, xy, pi, pj, matches as build_tracks; model: per pair, VG_MODEL_* or
    "none" / "E" / "F" / "H"; focal (n), Kinv (n x 3 x 3) or bearing (features x 3); Rrel (pairs x 3 x 3, cam2_from_cam1), trel (pairs x 3),
    FH (pairs x 3 x 3); valid_in per pair, registered_in per image, rot (n x 3 x 3, cam_from_world) or None.  score=True is pass A (rules
    1-5 and 7), score=False with rot is pass B (rules 6 and 7).  max_rotation_error_deg becomes the cosine the library compares with;
    cos_max_rotation_error, if given, is passed as it is.  -> ViewGraphPlan"""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise XmError("view_graph_filter: xy must be features x 2")
    foff = _tracks_foff(foff_or_counts, xy.shape[0])
    n, F = foff.size - 1, xy.shape[0]
    pi = np.ascontiguousarray(pi, dtype=np.int32).reshape(-1); pj = np.ascontiguousarray(pj, dtype=np.int32).reshape(-1)
    if pi.size != pj.size:
        raise XmError("view_graph_filter: pi and pj must have one entry per pair")
    npairs = pi.size
    try:
        model = np.ascontiguousarray([VG_MODELS.get(v, v) if isinstance(v, str) else v for v in np.asarray(model).reshape(-1).tolist()], dtype=np.int32)
    except (TypeError, ValueError):
        raise XmError(f"view_graph_filter: model must hold VG_MODEL_* numbers or the names {sorted(VG_MODELS)}") from None
    if model.size != npairs:
        raise XmError("view_graph_filter: model must have one entry per pair")
    moff, f1, f2 = _tracks_matches(matches, npairs)
    focal = _vg_array(focal, np.float64, (n,), "focal"); Kinv = _vg_array(Kinv, np.float64, (n, 3, 3), "Kinv")
    bearing = _vg_array(bearing, np.float64, (F, 3), "bearing"); Rrel = _vg_array(Rrel, np.float64, (npairs, 3, 3), "Rrel")
    trel = _vg_array(trel, np.float64, (npairs, 3), "trel"); FH = _vg_array(FH, np.float64, (npairs, 3, 3), "FH")
    rot = _vg_array(rot, np.float64, (n, 3, 3), "rot")
    valid_in = None if valid_in is None else _vg_array(np.asarray(valid_in) != 0, np.uint8, (npairs,), "valid_in")
    registered_in = None if registered_in is None else _vg_array(np.asarray(registered_in) != 0, np.uint8, (n,), "registered_in")
    cosmax = float(np.cos(np.radians(float(max_rotation_error_deg)))) if cos_max_rotation_error is None else float(cos_max_rotation_error)
    opt = VgOptions(VG_SCORE if score else 0, float(max_epipolar_error_E), float(max_epipolar_error_F), float(max_epipolar_error_H), int(min_inlier_num),
                    float(min_inlier_ratio), cosmax)
    res = VgResult(); res.struct_size = C.sizeof(VgResult)
    E = f1.size
    inlier = np.zeros(E, dtype=np.uint8); pinl = np.zeros(npairs, dtype=np.int32); pst = np.zeros(npairs, dtype=np.int32)
    regout = np.zeros(n, dtype=np.uint8); mo = np.zeros(npairs + 1, dtype=np.int64); o1 = np.zeros(E, dtype=np.int32); o2 = np.zeros(E, dtype=np.int32)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_view_graph_filter(n, P(foff), P(xy), P(focal), P(Kinv), P(bearing), npairs, P(pi), P(pj), P(model), P(Rrel), P(trel), P(FH), P(valid_in),
                                    P(registered_in), P(rot), P(moff), P(f1), P(f2), C.byref(opt), P(inlier), P(pinl), P(pst), P(regout), P(mo), P(o1), P(o2),
                                    C.byref(res)))
    k = int(mo[-1])
    info = {f: getattr(res, f) for f, _ in VgResult._fields_ if f != "struct_size"}
    return ViewGraphPlan(inlier, pinl, pst, regout, (mo, o1[:k].copy(), o2[:k].copy()), info, pi, pj, Rrel)


class CalibrationPlan:
    """what view_graph_calibrate returns: per camera focal (focal_out), focal_est (the raw estimate), refined (uint8), cam_status
    (VGC_CAM_*); per pair pair_status (VGC_VALID, VGC_INVALID_IN or VGC_TWO_VIEW_ERROR), valid (pair_status == VGC_VALID: the valid_in of
    view_graph_filter), residual (pairs x 2, without the loss, at the optimised focals), d (pairs x 8) when asked for, model and F (as given,
    or as rule 7 left them with update_config), cost_trace, info (the fields of xm_vgc_result_t)"""

    def __init__(self, focal, focal_est, refined, cam_status, pair_status, residual, d, model, F, cost_trace, info, pp, cam_of_image):
        self.focal, self.focal_est, self.refined, self.cam_status, self.pair_status = focal, focal_est, refined, cam_status, pair_status
        self.residual, self.d, self.model, self.F, self.cost_trace, self.info = residual, d, model, F, cost_trace, info
        self.valid = (pair_status == VGC_VALID).astype(np.uint8)
        self._pp, self._cam = pp, cam_of_image

    def focal_per_image(self):
        """-> focal_out[cam_of_image]: the focal of view_graph_filter"""
        return self.focal[self._cam]

    def Kinv(self):
        """-> images x 3 x 3: the inverse of [[f, 0, px], [0, f, py], [0, 0, 1]] per image, the Kinv of view_graph_filter"""
        f = self.focal[self._cam]
        K = np.zeros((self._cam.size, 3, 3))
        K[:, 0, 0] = 1.0 / f; K[:, 1, 1] = 1.0 / f; K[:, 2, 2] = 1.0
        K[:, 0, 2] = -self._pp[self._cam, 0] / f; K[:, 1, 2] = -self._pp[self._cam, 1] / f
        return K


def view_graph_calibrate_limits():
    """-> dict(light_incidences: most incidences of a camera that one thread walks (a camera above it gets a workgroup), threads: per
    workgroup, svd_sweeps: most sweeps of the Jacobi SVD, pcg_iterations: most PCG iterations of one solve)"""
    out = np.zeros(4, dtype=np.int64)
    _chk(lib().xm_view_graph_calibrate_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(light_incidences=int(out[0]), threads=int(out[1]), svd_sweeps=int(out[2]), pcg_iterations=int(out[3]))


def _vgc_inputs(what, focal0, pp, has_prior, cam_of_image, pi, pj, model, F, valid_in):
    focal0 = np.ascontiguousarray(focal0, dtype=np.float64).reshape(-1)
    ncams = focal0.size
    pp = np.ascontiguousarray(pp, dtype=np.float64)
    if pp.size != 2 * ncams:
        raise XmError(f"{what}: pp must be cameras x 2")
    pp = pp.reshape(ncams, 2)
    has_prior = np.ascontiguousarray(np.asarray(has_prior) != 0, dtype=np.uint8).reshape(-1)
    if has_prior.size != ncams:
        raise XmError(f"{what}: has_prior must have one entry per camera")
    cam = np.ascontiguousarray(cam_of_image, dtype=np.int32).reshape(-1)
    pi = np.ascontiguousarray(pi, dtype=np.int32).reshape(-1); pj = np.ascontiguousarray(pj, dtype=np.int32).reshape(-1)
    if pi.size != pj.size:
        raise XmError(f"{what}: pi and pj must have one entry per pair")
    npairs = pi.size
    try:
        model = np.ascontiguousarray([VG_MODELS.get(v, v) if isinstance(v, str) else v for v in np.asarray(model).reshape(-1).tolist()], dtype=np.int32)
    except (TypeError, ValueError):
        raise XmError(f"{what}: model must hold VG_MODEL_* numbers or the names {sorted(VG_MODELS)}") from None
    if model.size != npairs:
        raise XmError(f"{what}: model must have one entry per pair")
    F = np.ascontiguousarray(F, dtype=np.float64)
    if F.size != 9 * npairs:
        raise XmError(f"{what}: F must be pairs x 3 x 3")
    F = F.reshape(npairs, 3, 3)
    if valid_in is not None:
        valid_in = np.ascontiguousarray(np.asarray(valid_in) != 0, dtype=np.uint8).reshape(-1)
        if valid_in.size != npairs:
            raise XmError(f"{what}: valid_in must have one entry per pair")
    return focal0, pp, has_prior, cam, pi, pj, model, F, valid_in


def view_graph_calibrate(focal0, pp, has_prior, cam_of_image, pi, pj, model, F, valid_in=None, Rrel=None, trel=None, update_config=False,
                         thres_loss_function=1e-2, thres_lower_ratio=0.1, thres_higher_ratio=10.0, thres_two_view_error=2.0, max_num_iterations=100,
                         function_tolerance=1e-5, lower_bound=1e-3, want_d=False):
    """focal lengths from the view graph on the device (xm_view_graph_calibrate; include/xm_amd.h has the rules and the lines of the reference's
    fork of GLOMAP they stand for): focal0, has_prior per camera, pp cameras x 2; cam_of_image per image; pi, pj, model ("E" / "F" / ... or
    VG_MODEL_*), F (pairs x 3 x 3) per pair; valid_in per pair or None; Rrel (pairs x 3 x 3), trel (pairs x 3) with update_config.
    -> CalibrationPlan"""
    w = "view_graph_calibrate"
    focal0, pp, has_prior, cam, pi, pj, model, F, valid_in = _vgc_inputs(w, focal0, pp, has_prior, cam_of_image, pi, pj, model, F, valid_in)
    ncams, n, npairs = focal0.size, cam.size, pi.size
    Rrel = None if Rrel is None else np.ascontiguousarray(Rrel, dtype=np.float64)
    trel = None if trel is None else np.ascontiguousarray(trel, dtype=np.float64)
    if (Rrel is not None and Rrel.size != 9 * npairs) or (trel is not None and trel.size != 3 * npairs):
        raise XmError(f"{w}: Rrel must be pairs x 3 x 3 and trel pairs x 3")
    opt = VgcOptions(VGC_UPDATE_CONFIG if update_config else 0, float(thres_loss_function), float(thres_lower_ratio), float(thres_higher_ratio),
                     float(thres_two_view_error), int(max_num_iterations), float(function_tolerance), float(lower_bound))
    res = VgcResult(); res.struct_size = C.sizeof(VgcResult)
    fo = np.zeros(ncams); fe = np.zeros(ncams); refined = np.zeros(ncams, dtype=np.uint8); cst = np.zeros(ncams, dtype=np.int32)
    pst = np.zeros(npairs, dtype=np.int32); resid = np.zeros((npairs, 2)); d = np.zeros((npairs, 8)) if want_d else None
    mo = np.zeros(npairs, dtype=np.int32); Fo = np.zeros((npairs, 3, 3)); trace = np.zeros(max(int(max_num_iterations), 0) + 1)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_view_graph_calibrate(ncams, P(focal0), P(pp), P(has_prior), n, P(cam), npairs, P(pi), P(pj), P(model), P(F), P(valid_in), P(Rrel), P(trel),
                                       C.byref(opt), P(fo), P(fe), P(refined), P(cst), P(pst), P(resid), P(d), P(mo), P(Fo), P(trace), C.byref(res)))
    info = {f: getattr(res, f) for f, _ in VgcResult._fields_ if f not in ("struct_size", "reserved")}
    info["stop"] = BA_STATUS.get(res.stop_reason, str(res.stop_reason))
    return CalibrationPlan(fo, fe, refined, cst, pst, resid, d, mo, Fo, trace[:res.trace_len].copy(), info, pp, cam)


def view_graph_calibrate_probe(focal0, pp, has_prior, cam_of_image, pi, pj, model, F, focal, x=None, mu=0.0, d_in=None, valid_in=None,
                               thres_loss_function=1e-2):
    """the test export xm_view_graph_calibrate_probe: set-up (or d_in, pairs x 8), evaluation, the camera kernel and one product at the focals
    `focal` (per camera) and the vector x (per camera) -> dict(d, residual, record, cost, gradient, diagonal, product)"""
    w = "view_graph_calibrate_probe"
    focal0, pp, has_prior, cam, pi, pj, model, F, valid_in = _vgc_inputs(w, focal0, pp, has_prior, cam_of_image, pi, pj, model, F, valid_in)
    ncams, n, npairs = focal0.size, cam.size, pi.size
    focal = np.ascontiguousarray(focal, dtype=np.float64).reshape(-1)
    x = np.zeros(ncams) if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    if focal.size != ncams or x.size != ncams:
        raise XmError(f"{w}: focal and x must have one entry per camera")
    if d_in is not None:
        d_in = np.ascontiguousarray(d_in, dtype=np.float64)
        if d_in.size != 8 * npairs:
            raise XmError(f"{w}: d_in must be pairs x 8")
    opt = VgcOptions(0, float(thres_loss_function))
    out = dict(d=np.zeros((npairs, 8)), residual=np.zeros((npairs, 2)), record=np.zeros((npairs, 6)), cost=np.zeros(1), gradient=np.zeros(ncams),
               diagonal=np.zeros(ncams), product=np.zeros(ncams))
    P = lambda a: None if a is None else a.ctypes.data
    q = VgcProbe(C.sizeof(VgcProbe), 0, P(focal), P(x), P(d_in), float(mu), *[P(out[k]) for k in ("d", "residual", "record", "cost", "gradient", "diagonal", "product")])
    V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_view_graph_calibrate_probe(ncams, V(focal0), V(pp), V(has_prior), n, V(cam), npairs, V(pi), V(pj), V(model), V(F), V(valid_in),
                                             C.byref(opt), C.byref(q)))
    out["cost"] = float(out["cost"][0])
    return out


class RotationPlan:
    """what view_graph_rotations returns: rot (n x 3 x 3, cam_from_world: the rot of view_graph_filter's pass B as it is; unregistered images
    keep rot0), angle_axis (n x 3), residual (pairs x 3, at the final rotations), weight (per pair, of the last iteration's solve; 0 for a
    pair that takes no part), step_trace (the average step of every iteration), info (the fields of xm_vgr_result_t and stop, its name)"""

    def __init__(self, rot, angle_axis, residual, weight, step_trace, info):
        self.rot, self.angle_axis, self.residual, self.weight, self.step_trace, self.info = rot, angle_axis, residual, weight, step_trace, info


def view_graph_rotations_limits():
    """-> dict(light_incidences: most incidences of a camera that one thread walks (a camera above it gets a workgroup), threads: per
    workgroup, pcg_iterations: most PCG iterations of one solve).  Needs no device"""
    out = np.zeros(4, dtype=np.int64)
    _chk(lib().xm_view_graph_rotations_limits(out.ctypes.data_as(C.c_void_p)))
    return dict(light_incidences=int(out[0]), threads=int(out[1]), pcg_iterations=int(out[2]))


def _vgr_inputs(what, rot0, pi, pj, Rrel, registered, valid_in, weight_type):
    rot0 = np.ascontiguousarray(rot0, dtype=np.float64)
    if rot0.size % 9:
        raise XmError(f"{what}: rot0 must be images x 3 x 3")
    rot0 = rot0.reshape(-1, 3, 3)
    n = rot0.shape[0]
    pi = np.ascontiguousarray(pi, dtype=np.int32).reshape(-1); pj = np.ascontiguousarray(pj, dtype=np.int32).reshape(-1)
    if pi.size != pj.size:
        raise XmError(f"{what}: pi and pj must have one entry per pair")
    npairs = pi.size
    Rrel = np.ascontiguousarray(Rrel, dtype=np.float64)
    if Rrel.size != 9 * npairs:
        raise XmError(f"{what}: Rrel must be pairs x 3 x 3")
    Rrel = Rrel.reshape(npairs, 3, 3)
    if registered is not None:
        registered = np.ascontiguousarray(np.asarray(registered) != 0, dtype=np.uint8).reshape(-1)
        if registered.size != n:
            raise XmError(f"{what}: registered must have one entry per image")
    if valid_in is not None:
        valid_in = np.ascontiguousarray(np.asarray(valid_in) != 0, dtype=np.uint8).reshape(-1)
        if valid_in.size != npairs:
            raise XmError(f"{what}: valid_in must have one entry per pair")
    if isinstance(weight_type, str):
        if weight_type not in VGR_WEIGHT_TYPES:
            raise XmError(f"{what}: weight_type must be a VGR_* number or one of {sorted(VGR_WEIGHT_TYPES)}")
        weight_type = VGR_WEIGHT_TYPES[weight_type]
    return rot0, pi, pj, Rrel, registered, valid_in, int(weight_type)


def view_graph_rotations(rot0, pi, pj, Rrel, registered=None, valid_in=None, weight_type=VGR_GEMAN_MCCLURE, max_num_irls_iterations=100,
                         irls_step_convergence_threshold=1e-3, irls_loss_parameter_sigma=5.0, fixed_image=-1):
    """robust rotation averaging over the view graph on the device (xm_view_graph_rotations; include/xm_amd.h has the rules and the lines of
    the reference's fork of GLOMAP they stand for): rot0 (n x 3 x 3, cam_from_world, the start: the rotations of a view-graph solve), pi, pj,
    Rrel (pairs x 3 x 3, cam2_from_cam1) as view_graph_filter takes them; registered per image and valid_in per pair or None; weight_type
    VGR_GEMAN_MCCLURE / VGR_HALF_NORM or "geman_mcclure" / "half_norm"; sigma in degrees.  -> RotationPlan"""
    w = "view_graph_rotations"
    rot0, pi, pj, Rrel, registered, valid_in, wt = _vgr_inputs(w, rot0, pi, pj, Rrel, registered, valid_in, weight_type)
    n, npairs = rot0.shape[0], pi.size
    opt = VgrOptions(wt, int(max_num_irls_iterations), int(fixed_image), float(irls_step_convergence_threshold), float(irls_loss_parameter_sigma))
    res = VgrResult(); res.struct_size = C.sizeof(VgrResult)
    rot = np.zeros((n, 3, 3)); aa = np.zeros((n, 3)); resid = np.zeros((npairs, 3)); weight = np.zeros(npairs)
    trace = np.zeros(max(int(max_num_irls_iterations), 1))
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_view_graph_rotations(n, P(registered), P(rot0), npairs, P(pi), P(pj), P(Rrel), P(valid_in), C.byref(opt), P(rot), P(aa), P(resid),
                                       P(weight), P(trace), C.byref(res)))
    info = {f: getattr(res, f) for f, _ in VgrResult._fields_ if f not in ("struct_size", "reserved")}
    info["stop"] = VGR_STOP.get(res.stop_reason, str(res.stop_reason))
    return RotationPlan(rot, aa, resid, weight, trace[:res.irls_iterations].copy(), info)


def view_graph_rotations_probe(rot0, pi, pj, Rrel, angle_axis, x=None, weight_in=None, registered=None, valid_in=None,
                               weight_type=VGR_GEMAN_MCCLURE, irls_loss_parameter_sigma=5.0, fixed_image=-1):
    """the test export xm_view_graph_rotations_probe: the camera matrices, residuals, gauge residual and weights at the state angle_axis (n x 3),
    then with weight_in (per pair, or None: the computed weights) the right-hand side, the diagonal and the product with x (n x 3), and the
    update by x with its average step -> dict(rot, residual, gauge, weight, rhs, diagonal, product, angle_axis_out, step)"""
    w = "view_graph_rotations_probe"
    rot0, pi, pj, Rrel, registered, valid_in, wt = _vgr_inputs(w, rot0, pi, pj, Rrel, registered, valid_in, weight_type)
    n, npairs = rot0.shape[0], pi.size
    angle_axis = np.ascontiguousarray(angle_axis, dtype=np.float64)
    x = np.zeros((n, 3)) if x is None else np.ascontiguousarray(x, dtype=np.float64)
    if angle_axis.size != 3 * n or x.size != 3 * n:
        raise XmError(f"{w}: angle_axis and x must be images x 3")
    if weight_in is not None:
        weight_in = np.ascontiguousarray(weight_in, dtype=np.float64).reshape(-1)
        if weight_in.size != npairs:
            raise XmError(f"{w}: weight_in must have one entry per pair")
    opt = VgrOptions(wt, 100, int(fixed_image), 1e-3, float(irls_loss_parameter_sigma))
    out = dict(rot=np.zeros((n, 3, 3)), residual=np.zeros((npairs, 3)), gauge=np.zeros(3), weight=np.zeros(npairs), rhs=np.zeros((n, 3)),
               diagonal=np.zeros(n), product=np.zeros((n, 3)), angle_axis_out=np.zeros((n, 3)), step=np.zeros(1))
    P = lambda a: None if a is None else a.ctypes.data
    q = VgrProbe(C.sizeof(VgrProbe), 0, P(angle_axis), P(x), P(weight_in),
                 *[P(out[k]) for k in ("rot", "residual", "gauge", "weight", "rhs", "diagonal", "product", "angle_axis_out", "step")])
    V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _chk(lib().xm_view_graph_rotations_probe(n, V(registered), V(rot0), npairs, V(pi), V(pj), V(Rrel), V(valid_in), C.byref(opt), C.byref(q)))
    out["step"] = float(out["step"][0])
    return out


def symw_plan(ntot, nloc, cam0, K=0):
    """work list of one rank of the multi-rank symmetric window product (xm_symw.h) -- host only"""
    geom = np.zeros(8, dtype=np.int32)
    _chk(lib().xm_symw_plan(ntot, nloc, cam0, K, geom.ctypes.data_as(C.c_void_p), None))
    items = np.zeros((max(int(geom[7]), 1), 3), dtype=np.int32)
    _chk(lib().xm_symw_plan(ntot, nloc, cam0, K, geom.ctypes.data_as(C.c_void_p), items.ctypes.data_as(C.c_void_p)))
    keys = ("T", "Th", "tie", "t0", "nsteps", "nstrips", "K", "nitems")
    out = {k: int(v) for k, v in zip(keys, geom)}
    out["items"] = items[: out["nitems"]]
    return out


def symw_probe(Q, W, ntot, nloc, cam0, world, o, alpha=1.0, K=0, nt=-1, scal_status=-1, pad_value=0.0, cs_all=None):
    """one rank's share of the multi-rank symmetric product, kernel by kernel (the test export xm_symw_probe, include/xm_amd.h): Q is the rank's
    strip (3 nloc x 3 ntot), W 3 ntot x o, cs_all (world x 3 ntot x o, float64, contiguous; zeros when None) the ranks' column sums as the
    all-gather would deliver them -- the slot of this rank is overwritten in place.  Returns Prow (nstrips, 6 nsteps, o), Pcol (items, 256, o),
    csum (3 ntot, o), Y (3 nloc, o), cs_all and K, nt, nitems, nfull as used."""
    Q = np.ascontiguousarray(Q, dtype=np.float64); W = np.ascontiguousarray(W, dtype=np.float64).reshape(-1, max(int(o), 1))
    if Q.shape != (3 * nloc, 3 * ntot) or W.shape[0] != 3 * ntot:
        raise XmError("symw_probe: Q is 3 nloc x 3 ntot and W 3 ntot x o")
    if cs_all is None:
        cs_all = np.zeros((max(world, 1), 3 * ntot, o))
    if not (isinstance(cs_all, np.ndarray) and cs_all.dtype == np.float64 and cs_all.flags.c_contiguous and cs_all.flags.writeable
            and cs_all.shape == (world, 3 * ntot, o)):
        raise XmError("symw_probe: cs_all is a contiguous writable float64 array of world x 3 ntot x o")
    try:
        g = symw_plan(ntot, nloc, cam0, K)
    except XmError:
        g = dict(nstrips=1, nsteps=1, nitems=1)       # (the export refuses what the plan refuses)
    out = dict(Prow=np.zeros((g["nstrips"], 6 * g["nsteps"], o)), Pcol=np.zeros((max(g["nitems"], 1), 256, o)), csum=np.zeros((3 * ntot, o)),
               Y=np.zeros((3 * nloc, o)))
    V = lambda a: a.ctypes.data_as(C.c_void_p)
    p = SymwProbe(struct_size=C.sizeof(SymwProbe), ntot=ntot, nloc=nloc, cam0=cam0, world=world, o=o, K=K, nt=nt, scal_status=scal_status,
                  alpha=alpha, pad_value=pad_value, Q=V(Q), W=V(W), cs_all=V(cs_all), **{k: V(v) for k, v in out.items()})
    _chk(lib().xm_symw_probe(C.byref(p)))
    out.update(cs_all=cs_all, K=int(p.K), nt=int(p.nt), nitems=int(p.nitems), nfull=int(p.nfull))
    out["Pcol"] = out["Pcol"][:out["nitems"]]
    return out


def symw_product(Q, W, world, o, alpha=1.0, K=0, nt=-1, scal_status=-1, pad_value=0.0):
    """alpha * Q W of a whole symmetric Q (3 ntot x 3 ntot) by the multi-rank window product on `world` equal row strips, one xm_symw_probe call
    per rank for the column sums and one more per rank with all of them (the all-gather is a copy here).  Returns (Y, stages): Y 3 ntot x o and
    the per-rank results of the second round of calls."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    ntot = Q.shape[0] // 3
    if Q.shape != (3 * ntot, 3 * ntot) or world < 1 or ntot % world:
        raise XmError("symw_product: Q is 3 ntot x 3 ntot and world divides ntot")
    nloc = ntot // world
    cs_all = np.zeros((world, 3 * ntot, o))
    kw = dict(alpha=alpha, K=K, nt=nt, scal_status=scal_status, pad_value=pad_value)
    for r in range(world):
        symw_probe(Q[3 * r * nloc:3 * (r + 1) * nloc], W, ntot, nloc, r * nloc, world, o, cs_all=cs_all, **kw)
    stages = [symw_probe(Q[3 * r * nloc:3 * (r + 1) * nloc], W, ntot, nloc, r * nloc, world, o, cs_all=cs_all.copy(), **kw) for r in range(world)]
    return np.concatenate([s["Y"] for s in stages], axis=0), stages


class SellMatrix:
    """3x3-block sparse Q in the sliced-ELL device layout (xm_sell_create); product through xm_qw_sell"""

    def __init__(self, rowptr, colidx, blocks, ncols=None, slabs=4, lmax=0, codec=0, row0=0):
        """codec 1 = view-graph codec (quaternion per off-diagonal block, scalar per diagonal block)"""
        require_gpu()
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64); colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        blocks = np.ascontiguousarray(blocks, dtype=np.float64)
        self.n = rowptr.size - 1
        self.h = C.c_void_p()
        _chk(lib().xm_sell_create2(rowptr.ctypes.data_as(C.c_void_p), colidx.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p),
                                   self.n, self.n if ncols is None else ncols, slabs, lmax, codec, row0, C.byref(self.h)))

    def qw(self, W, alpha=1.0, gather=1, padded=False):
        """gather: 0 a record of W per lane | 1 LDS-transposed (the solver's default).  padded=True: the input is also handed over at a
        record pitch of 16 doubles (xm_qw_sell_padded; o = 3..5)"""
        W = np.asarray(W, dtype=np.float64)
        o = W.shape[1]
        dW = DevArray(to_rm(W)); dO = DevArray(nbytes=3 * self.n * pitch_of(o) * 8)
        dP = DevArray(pad16(W)) if padded else None
        _chk(lib().xm_qw_sell_padded(self.h, o, dW.ptr, dP.ptr if padded else None, dO.ptr, alpha, gather, None))
        _chk(lib().xm_dev_sync())
        out = from_rm(dO.get(), 3 * self.n, o)
        dW.free(); dO.free()
        if padded:
            dP.free()
        return out

    def close(self):
        if self.h:
            lib().xm_sell_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def retract(R, s, D, ds, t, polar=False):
    """(MGS_rows(R + t D), s*exp(t ds/s)) through xm_retract; polar=True: the polar retraction (xm_retract_polar)."""
    require_gpu()
    R = np.asarray(R, dtype=np.float64)
    n, o = R.shape[0] // 3, R.shape[1]
    dR = DevArray(to_rm(R)); dD = DevArray(to_rm(D)); dsv = DevArray(np.asarray(s, dtype=np.float64))
    dds = DevArray(np.asarray(ds, dtype=np.float64))
    dRo = DevArray(nbytes=dR.nbytes); dso = DevArray(nbytes=dsv.nbytes)
    _chk((lib().xm_retract_polar if polar else lib().xm_retract)(n, o, dR.ptr, dsv.ptr, dD.ptr, dds.ptr, t, dRo.ptr, dso.ptr, None))
    _chk(lib().xm_dev_sync())
    out = from_rm(dRo.get(), 3 * n, o), dso.get()
    for b in (dR, dD, dsv, dds, dRo, dso):
        b.free()
    return out


def recover_rotations(R, s, variant=None, reps=0):
    """anchored O(3) rotations (3 x 3n) and scales of a solution (R: 3n x r, s: n) through xm_recover_rotations.  variant (xm_bench.h): 0 the
    default kernel, 1 one wavefront per camera; with reps > 0 a fourth value is returned: average ms of the projection launch"""
    require_gpu()
    R = np.asfortranarray(np.asarray(R, dtype=np.float64)); s = np.ascontiguousarray(np.asarray(s, dtype=np.float64).reshape(-1))
    n, r = s.size, R.shape[1]
    rot = np.zeros((3, 3 * n), order="F"); sc = np.zeros(n); neg = C.c_int(0)
    args = (n, r, R.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), rot.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.byref(neg))
    if variant is None:
        _chk(lib().xm_recover_rotations(*args))
        return np.ascontiguousarray(rot), sc, neg.value
    ms = C.c_double(0.0)
    _chk(lib().xm_recover_rotations_variant(*args, int(variant), int(reps), C.byref(ms)))
    return (np.ascontiguousarray(rot), sc, neg.value) + ((ms.value,) if reps > 0 else ())


def schur_dense_limits():
    """(cameras per LDS column window of the assembly kernel, landmarks per panel of Abar, camera cap) of the device build of the dense Q"""
    out = (C.c_int64 * 3)()
    _chk(lib().xm_schur_dense_limits(out))
    return int(out[0]), int(out[1]), int(out[2])


def create_matrix_arrays(cam, lm, p, w, n=None, m=None, abar=True):
    """dense Q (3n x 3n) and, with abar=True, Abar ((n-1+m) x 3n) of the reference's create_matrix from 0-based observation arrays, built on
    the device (xm_create_matrix).  Returns (Q, Abar or None)."""
    require_gpu()
    cam = np.ascontiguousarray(cam, dtype=np.int32).reshape(-1); lm = np.ascontiguousarray(lm, dtype=np.int32).reshape(-1)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3); w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    assert cam.size == lm.size == w.size == p.shape[0]
    n = int(cam.max()) + 1 if n is None else int(n)
    m = int(lm.max()) + 1 if m is None else int(m)
    Q = np.zeros((3 * n, 3 * n), order="F")
    A = np.zeros((n - 1 + m, 3 * n), order="F") if abar else None
    _chk(lib().xm_create_matrix(n, m, cam.size, cam.ctypes.data_as(C.c_void_p), lm.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p),
                                w.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p), 3 * n, A.ctypes.data_as(C.c_void_p) if abar else None))
    return Q, A


def _write_bin(fn, M):
    """the reference's .bin matrix (utils/io.py): int32 rows, int32 cols, float64 column-major"""
    M = np.asfortranarray(M, dtype=np.float64)
    with open(fn, "wb") as f:
        np.array(M.shape, dtype=np.int32).tofile(f)
        f.write(M.tobytes(order="F"))


def create_matrix(weight, edges, landmarks, output_path, abar=True):
    """drop-in for the reference's utils/creatematrix.py:create_matrix on the device: weight (nobs), edges (nobs x 2, 1-based camera and
    landmark), landmarks (nobs x 3 camera-frame points); writes Q.bin and (abar=True) Abar.bin into output_path in the reference's format and
    returns (Q, Abar or None)."""
    edges = np.asarray(edges)
    Q, A = create_matrix_arrays(edges[:, 0].astype(np.int64) - 1, edges[:, 1].astype(np.int64) - 1, landmarks, weight, abar=abar)
    os.makedirs(output_path, exist_ok=True)
    _write_bin(os.path.join(output_path, "Q.bin"), Q)
    if abar:
        _write_bin(os.path.join(output_path, "Abar.bin"), A)
    return Q, A


# ------------------------------------------------------------------------------------------------ context API
class Context:
    """Q resident in HBM; solve() == the reference's staircase (XM_main.cu:180 / :312 / :35)."""

    def __init__(self, Q=None, bsr=None, dq=None, n=None, densify=False, obs=None, vg=None, n_gpus=1, gpu_map=0, tuning=None):
        """vg = (ei, ej, w, M): view-graph edge list (STORAGE_VIEWGRAPH).  n_gpus > 1: single-process row partition over that many GPUs
        (gpu_map=1: all ranks on device 0).  tuning: dict of xm_tuning_t fields."""
        require_gpu()
        self._keep = []
        p = Problem()
        p.struct_size = C.sizeof(Problem)
        p.n_gpus, p.gpu_map = int(n_gpus), int(gpu_map)
        if tuning:
            tn = Tuning()
            for k, v in tuning.items():
                setattr(tn, k, int(v))
            p.tuning = C.pointer(tn)
            self._keep.append(tn)
        if vg is not None:
            ei, ej, w, M = vg
            ei = np.ascontiguousarray(ei, dtype=np.int32); ej = np.ascontiguousarray(ej, dtype=np.int32)
            w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1); M = np.ascontiguousarray(M, dtype=np.float64).reshape(-1, 9)
            assert ei.size == ej.size == w.size == M.shape[0]
            self.n = int(max(ei.max(), ej.max())) + 1 if n is None else int(n)
            p.n, p.storage, p.ne = self.n, STORAGE_VIEWGRAPH, ei.size
            p.edge_i, p.edge_j, p.edge_w, p.edge_M = (a.ctypes.data_as(C.c_void_p) for a in (ei, ej, w, M))
            self._keep += [ei, ej, w, M]
            self.ne = ei.size
        elif obs is not None:                     # matrix-free: (cam, lm, p, w) = (edges[:, 0] - 1, edges[:, 1] - 1, landmarks, weight)
            cam, lm, pts, w = obs
            cam = np.ascontiguousarray(cam, dtype=np.int32); lm = np.ascontiguousarray(lm, dtype=np.int32)
            pts = np.ascontiguousarray(pts, dtype=np.float64); w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
            self.n = int(cam.max()) + 1 if n is None else int(n)
            p.n, p.storage, p.nobs, p.n_landmarks = self.n, STORAGE_SCHUR, cam.size, int(lm.max()) + 1
            self.n_landmarks = int(lm.max()) + 1
            p.obs_cam, p.obs_lm, p.obs_p, p.obs_w = (a.ctypes.data_as(C.c_void_p) for a in (cam, lm, pts, w))
            self._keep += [cam, lm, pts, w]
            self.ne = cam.size                      # residuals / weights of the XM^2 loop are per observation
            self._w = w.copy()                      # the current weights, as far as this object set them (refine_filtered)
            self._cam = cam.copy()                  # the camera of every observation (prune_weakly_connected's plan)
        elif dq is not None:                      # dense Q already on the device in the solver's layout (borrowed)
            self.n = int(n)
            p.n, p.storage, p.q_on_device, p.q, p.ldq = self.n, STORAGE_DENSE, 1, dq.ptr, dense_ld(self.n)
            self._dq = dq
        elif Q is not None:
            Q = np.asfortranarray(np.asarray(Q, dtype=np.float64))
            self.n = Q.shape[0] // 3
            p.n, p.storage, p.q, p.ldq = self.n, STORAGE_DENSE, Q.ctypes.data_as(C.c_void_p), Q.shape[0]
            self._keep.append(Q)
        else:
            rowptr, colidx, blocks = bsr
            rowptr = np.ascontiguousarray(rowptr, dtype=np.int64); colidx = np.ascontiguousarray(colidx, dtype=np.int32)
            blocks = np.ascontiguousarray(blocks, dtype=np.float64)
            self.n = rowptr.size - 1
            p.n, p.storage, p.nb = self.n, (STORAGE_BSR3_DENSE if densify else STORAGE_BSR3), colidx.size
            p.rowptr, p.colidx, p.blocks = (a.ctypes.data_as(C.c_void_p) for a in (rowptr, colidx, blocks))
            self._keep += [rowptr, colidx, blocks]
        self.h = C.c_void_p()
        _chk(lib().xm_ctx_create(C.byref(p), C.byref(self.h)))
        self._keep = []   # Q has been copied to the device

    TRANSPORTS = {0: "none (one GPU)", 1: "RCCL all-gather", 2: "shared-memory test transport", 3: "direct peer writes (threads of one process)",
                  4: "direct peer writes (one process per GPU, IPC-mapped buffers)"}

    def transport(self):
        """(kind, name, note): the transport that joins the ranks of this context and why a faster one was given up (xm_ctx_transport)"""
        k = C.c_int(0); buf = C.create_string_buffer(512)
        _chk(lib().xm_ctx_transport(self.h, C.byref(k), buf, 512))
        return k.value, self.TRANSPORTS.get(k.value, "?"), buf.value.decode()

    def product_kind(self, o=3):
        """name of the kernel family that serves a tCG product of rank o (xm_ctx_product_kind)"""
        k = C.c_int(0)
        _chk(lib().xm_ctx_product_kind(self.h, int(o), C.byref(k)))
        return PRODUCT_KINDS.get(k.value, "?")

    def schur_info(self):
        """matrix-free contexts: dict(cg=bool, products, inner_iters, capped, last_relres, precond, aggregates) (xm_ctx_schur_info,
        xm_ctx_schur_precond_info); precond: "jacobi" / "two-level" for the CG form, None otherwise"""
        u = C.c_int(0); st = (C.c_int64 * 3)(); rr = C.c_double(0.0)
        _chk(lib().xm_ctx_schur_info(self.h, C.byref(u), st, C.byref(rr)))
        kind = C.c_int(-1); na = C.c_int64(0); blk = C.c_int(0)
        _chk(lib().xm_ctx_schur_precond_info(self.h, C.byref(kind), C.byref(na), C.byref(blk)))
        return dict(cg=bool(u.value), products=int(st[0]), inner_iters=int(st[1]), capped=int(st[2]), last_relres=rr.value,
                    precond={0: "jacobi", 1: "two-level"}.get(kind.value), aggregates=int(na.value))

    def dense_q(self):
        """the context's current dense Q (3n x 3n) built on the device from its observation lists (tuning schur_dense_q=1; xm_ctx_dense_q)"""
        Q = np.zeros((3 * self.n, 3 * self.n), order="F")
        _chk(lib().xm_ctx_dense_q(self.h, Q.ctypes.data_as(C.c_void_p), 3 * self.n))
        return Q

    def sell_wpad(self):
        """True when the tCG of the last solved rank read its product input at the 128-byte record pitch (xm_ctx_sell_wpad)"""
        on = C.c_int(0)
        _chk(lib().xm_ctx_sell_wpad(self.h, C.byref(on)))
        return bool(on.value)

    def qw(self, W, alpha=1.0):
        """alpha * Q @ W through the context's storage (xm_ctx_qw)"""
        W = np.asfortranarray(np.asarray(W, dtype=np.float64))
        out = np.zeros_like(W, order="F")
        _chk(lib().xm_ctx_qw(self.h, W.shape[1], W.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), alpha))
        return np.ascontiguousarray(out)

    # ---- XM^2 re-weighting on the resident Q (reference loop 3_test_colmap_glomap.py:299-351)
    def attach_edges(self, ei, ej, M):
        ei = np.ascontiguousarray(ei, dtype=np.int32); ej = np.ascontiguousarray(ej, dtype=np.int32)
        M = np.ascontiguousarray(M, dtype=np.float64)
        self.ne = ei.size
        _chk(lib().xm_ctx_attach_edges(self.h, self.ne, ei.ctypes.data_as(C.c_void_p), ej.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p)))

    def edge_residuals(self):
        res = np.zeros(self.ne)
        _chk(lib().xm_ctx_edge_residuals(self.h, res.ctypes.data_as(C.c_void_p)))
        return res

    def recover_tp(self, rot, scale):
        """translations (3 x n, camera 1 at the origin) and landmarks (3 x m) of a solution given as anchored rotations (3 x 3n) and
        scales (n) — recover_XM's t_est / p_est without Abar (matrix-free contexts only)"""
        rot = np.asfortranarray(np.asarray(rot, dtype=np.float64)); scale = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(-1))
        assert rot.shape == (3, 3 * self.n) and scale.size == self.n
        t = np.zeros((3, self.n), order="F"); p = np.zeros((3, self.n_landmarks), order="F")
        _chk(lib().xm_ctx_recover_tp(self.h, rot.ctypes.data_as(C.c_void_p), scale.ctypes.data_as(C.c_void_p),
                                     t.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)))
        return np.ascontiguousarray(t), np.ascontiguousarray(p)

    def bundle_adjust(self, rot, t, P, fix_rotations=False, max_iters=1000, max_time=300.0, eta=0.1, function_tol=1e-6,
                      gradient_tol=1e-10, parameter_tol=1e-8, trace=0, loss="trivial", loss_scale=0.0, nonmonotonic=False, max_nonmonotonic=0,
                      linear_solver="iterative_schur", preconditioner="jacobi", refine_focal=False, focal=None, focal_free=None,
                      focal_group=None, refine_distortion=False, distortion=None, distortion_free=None):
        """reprojection bundle adjustment of a recovered solution (the reference's Ceres refinement, xm_ctx_bundle_adjust): rot 3 x 3n
        (R_i), t 3 x n, P 3 x m as recover_rotations / recover_tp return them -> refined (rot, t, P, info); matrix-free contexts only.
        loss: a BA_LOSS name with its scale loss_scale (Ceres's a, in normalised image units: pixels / focal length); nonmonotonic=True:
        Ceres's non-monotonic steps (the reference's configuration), reference cost reset after max_nonmonotonic (0 = 5) steps without a
        new minimum, the least-cost point returned.  linear_solver: "iterative_schur" (block-Jacobi PCG to eta, Ceres's ITERATIVE_SCHUR) or
        "dense_schur" (the reduced camera system assembled densely and solved by Cholesky, Ceres's DENSE_SCHUR; up to BA_DENSE_MAX_ROWS rows).
        preconditioner (of the PCG): "jacobi" (the inverted camera blocks, Ceres's SCHUR_JACOBI), "blocks" (inverted blocks of BA_AGG_CAMS
        cameras along a breadth-first order) or "two_level" (those blocks plus a coarse operator on the rigid-plus-scale motions of every
        aggregate: for sequential captures, where the default runs into its iteration cap); info["coarse_fallbacks"]: LM iterations
        whose coarse operator could not be inverted and that ran with the blocks alone.
        info: status (BA_STATUS), iters, accepted, pcg_iters, n_used, initial_cost, final_cost, gradient_max, seconds, and with trace > 0
        "trace": one row per LM iteration (cost, candidate cost, mu, accepted, PCG iterations, PCG relative residual); costs are
        1/2 sum rho(|r|^2).
        refine_focal=True (xm_ctx_bundle_adjust_focal): one focal scale g_i > 0 per camera joins its block, r = g_i pi(X) - z; focal (n;
        None = ones) is the start, focal_free (n; None = all) holds the cameras with 0 at their value; info["focal"] is the refined
        array.  preconditioner must be "jacobi".
        focal_group (n integers in [0, G); xm_ctx_bundle_adjust_focal_groups): the cameras of a group share ONE focal scale, as the images
        of one physical camera do; focal and focal_free then have G entries (focal None: ones, G = max(focal_group) + 1) and
        info["focal"] has shape (G,); pass info["focal"][focal_group] where per-image scales are taken (reprojection_errors,
        rescale_observations).  With at most BA_FOCAL_GROUPS_EXACT groups the PCG's preconditioner holds the exact focal block
        (info["coarse_fallbacks"]: LM iterations in which it could not be factored).  None: the per-image call, unchanged.
        refine_distortion=True (xm_ctx_bundle_adjust_radial; implies refine_focal=True): one radial coefficient k_i per camera joins the
        block behind the focal scale, r = g_i (1 + k_i |u|^2) u - z with u = pi(X) (COLMAP's SIMPLE_RADIAL); distortion (n; None = zeros) is
        the start, distortion_free (n; None = all) holds the cameras with 0; info["distortion"] is the refined array (n,).  A candidate
        at which the radial map folds at a used observation (1 + 3 k |u|^2 <= 0) is rejected like one with a focal <= 0.  Not with
        focal_group.  undistort_observations carries the result to everything that has no distortion argument."""
        group_of = None
        dist = dist_free = None
        if refine_distortion:   # refused before the device
            if focal_group is not None:
                raise XmError("refine_distortion: a radial coefficient shared by focal group is not built (no focal_group)")
            refine_focal = True
            dist, dist_free = _dist_args(self.n, distortion, distortion_free)
        elif distortion is not None or distortion_free is not None:
            raise XmError("distortion / distortion_free are given but refine_distortion is not set")
        if focal_group is not None:
            if not refine_focal:
                raise XmError("focal_group is given but refine_focal is not set")
            group_of, focal, focal_free = _focal_group_args(self.n, focal_group, focal, focal_free, preconditioner, linear_solver)
        elif refine_focal:   # refused before the device
            focal, focal_free = _focal_args(self.n, focal, focal_free, preconditioner)
        elif focal is not None or focal_free is not None:
            raise XmError("focal / focal_free are given but refine_focal is not set")
        rot = np.array(rot, dtype=np.float64, order="F"); t = np.array(t, dtype=np.float64, order="F"); P = np.array(P, dtype=np.float64, order="F")
        assert rot.shape == (3, 3 * self.n) and t.shape == (3, self.n) and P.shape == (3, self.n_landmarks)
        if loss not in BA_LOSS:
            raise XmError(f"unknown loss {loss!r} (one of {', '.join(BA_LOSS)})")
        if linear_solver not in BA_LINEAR_SOLVERS:
            raise XmError(f"unknown linear solver {linear_solver!r} (one of {', '.join(BA_LINEAR_SOLVERS)})")
        if preconditioner not in BA_PRECONDITIONERS:
            raise XmError(f"unknown preconditioner {preconditioner!r} (one of {', '.join(BA_PRECONDITIONERS)})")
        opt = BaOptions(); res = BaResult()
        opt.struct_size, res.struct_size = C.sizeof(BaOptions), C.sizeof(BaResult)
        opt.max_iters, opt.max_time, opt.eta = int(max_iters), float(max_time), float(eta)
        opt.function_tol, opt.gradient_tol, opt.parameter_tol = float(function_tol), float(gradient_tol), float(parameter_tol)
        opt.flags = (BA_FIX_ROTATIONS if fix_rotations else 0) | (BA_NONMONOTONIC if nonmonotonic else 0) | BA_LINEAR_SOLVERS[linear_solver]
        opt.flags |= BA_PRECONDITIONERS[preconditioner]
        opt.loss, opt.loss_scale, opt.max_nonmonotonic = BA_LOSS[loss], float(loss_scale), int(max_nonmonotonic)
        tr = None
        if trace:
            tr = np.zeros((int(trace), 6)); opt.trace_cap = int(trace); opt.trace = tr.ctypes.data_as(C.c_void_p)
        if group_of is not None:
            opt.flags |= BA_REFINE_FOCAL
            _chk(lib().xm_ctx_bundle_adjust_focal_groups(self.h, C.byref(opt), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                                         P.ctypes.data_as(C.c_void_p), focal.size, group_of.ctypes.data_as(C.c_void_p),
                                                         focal.ctypes.data_as(C.c_void_p),
                                                         None if focal_free is None else focal_free.ctypes.data_as(C.c_void_p), C.byref(res)))
        elif refine_distortion:
            opt.flags |= BA_REFINE_FOCAL | BA_REFINE_RADIAL
            V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
            _chk(lib().xm_ctx_bundle_adjust_radial(self.h, C.byref(opt), V(rot), V(t), V(P), V(focal), V(focal_free), V(dist), V(dist_free), C.byref(res)))
        elif refine_focal:
            opt.flags |= BA_REFINE_FOCAL
            _chk(lib().xm_ctx_bundle_adjust_focal(self.h, C.byref(opt), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                                  P.ctypes.data_as(C.c_void_p), focal.ctypes.data_as(C.c_void_p),
                                                  None if focal_free is None else focal_free.ctypes.data_as(C.c_void_p), C.byref(res)))
        else:
            _chk(lib().xm_ctx_bundle_adjust(self.h, C.byref(opt), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                            P.ctypes.data_as(C.c_void_p), C.byref(res)))
        info = {k: getattr(res, k) for k, _ in BaResult._fields_ if k != "struct_size"}
        if refine_focal:
            info["focal"] = focal
        if refine_distortion:
            info["distortion"] = dist
        info["status_name"] = BA_STATUS.get(res.status, "?")
        if tr is not None:
            info["trace"] = tr[: res.trace_len].copy()
        return rot, t, P, info

    def global_positioning(self, rot, t=None, P=None, seed=1, min_views=3, loss="huber", loss_scale=0.1, max_iters=100, max_time=300.0, eta=0.1,
                           function_tol=1e-5, gradient_tol=1e-10, parameter_tol=1e-8, trace=0, pairs=None, constraint="only_points",
                           calibrated=None, reweight_scale=1.0, fix_centres=False, points=True):
        """GLOMAP's global positioning (estimators/global_positioning.cc, ONLY_POINTS; xm_ctx_global_positioning, include/xm_amd.h has the
        contract): camera centres t (3 x n) and points P (3 x m) from the rotations rot (3 x 3n, R_i camera to world, read only) and the
        bearings p_e / |p_e| of this context's observations at their CURRENT weights; matrix-free contexts only.  t or P None: both start
        from gp_random_start(n, m, seed).  -> (t, P, info) with info: status (BA_STATUS), iters, accepted, pcg_iters, n_used, initial_cost,
        final_cost, gradient_max, seconds, scales (one per observation in input order, -1 = not used) and with trace > 0 "trace" (the rows
        of bundle_adjust).  The result has a free gauge (origin and scale); bundle_adjust can start from it.
        pairs = (pi, pj, trel[, valid]), constraint ("only_points", "only_cameras", "points_and_cameras_balanced", "points_and_cameras"),
        calibrated (n flags), reweight_scale, fix_centres: xm_ctx_global_positioning_pairs (with the defaults of all five the old entry
        point is called).  constraint="only_cameras" with points=True then makes the second call of global_mapper.cc:205-217, "only_points"
        with the centres fixed, so that P is placed against the centres just found; info is the first call's, with "points" the second's.
        info gains sigma (one per pair, -1 = takes no part), pairs_used, weight_scale_pt, cams_heavy, max_incidences."""
        n, m = self.n, self.n_landmarks
        rot = np.asfortranarray(np.asarray(rot, dtype=np.float64))
        if t is None or P is None:
            t, P = gp_random_start(n, m, seed)
        t = np.array(t, dtype=np.float64, order="F"); P = np.array(P, dtype=np.float64, order="F")
        assert rot.shape == (3, 3 * n) and t.shape == (3, n) and P.shape == (3, m)
        if loss not in BA_LOSS:
            raise XmError(f"unknown loss {loss!r} (one of {', '.join(BA_LOSS)})")
        opt = GpOptions(); res = GpResult()
        opt.struct_size, res.struct_size = C.sizeof(GpOptions), C.sizeof(GpResult)
        opt.max_iters, opt.max_time, opt.eta, opt.min_views = int(max_iters), float(max_time), float(eta), int(min_views)
        opt.function_tol, opt.gradient_tol, opt.parameter_tol = float(function_tol), float(gradient_tol), float(parameter_tol)
        opt.loss, opt.loss_scale = BA_LOSS[loss], float(loss_scale)
        tr = None
        if trace:
            tr = np.zeros((int(trace), 6)); opt.trace_cap = int(trace); opt.trace = tr.ctypes.data_as(C.c_void_p)
        scales = np.zeros(max(self.ne, 1))
        plain = pairs is None and constraint == "only_points" and calibrated is None and reweight_scale == 1.0 and not fix_centres
        if plain:
            _chk(lib().xm_ctx_global_positioning(self.h, C.byref(opt), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                                 P.ctypes.data_as(C.c_void_p), scales.ctypes.data_as(C.c_void_p), C.byref(res)))
        else:
            g, keep, sigma = _gp_pairs_struct(n, pairs, constraint, calibrated, reweight_scale, fix_centres)
            _chk(lib().xm_ctx_global_positioning_pairs(self.h, C.byref(opt), C.byref(g), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                                       P.ctypes.data_as(C.c_void_p), scales.ctypes.data_as(C.c_void_p), C.byref(res)))
        info = {k: getattr(res, k) for k, _ in GpResult._fields_ if k not in ("struct_size", "pad")}
        info["status_name"] = BA_STATUS.get(res.status, "?")
        info["scales"] = scales[: self.ne]
        if tr is not None:
            info["trace"] = tr[: res.trace_len].copy()
        if not plain:
            info.update(sigma=sigma, pairs_used=g.pairs_used, weight_scale_pt=g.weight_scale_pt, cams_heavy=g.cams_heavy, max_incidences=g.max_incidences)
            if constraint == "only_cameras" and points:
                _, P, info["points"] = self.global_positioning(rot, t, P, min_views=min_views, loss=loss, loss_scale=loss_scale, max_iters=max_iters,
                                                               max_time=max_time, eta=eta, function_tol=function_tol, gradient_tol=gradient_tol,
                                                               parameter_tol=parameter_tol, calibrated=calibrated, fix_centres=True)
                info["scales"] = info["points"]["scales"]
        return t, P, info

    def gp_probe_pairs(self, rot, t, P, mu, pairs=None, constraint="only_points", calibrated=None, reweight_scale=1.0, fix_centres=False, s=None,
                       sigma=None, min_views=3, loss="huber", loss_scale=0.1, X=None, dc=None):
        """gp_probe with the terms of global_positioning(pairs=..., constraint=..., ...) (the test export xm_ctx_gp_probe_pairs;
        include/xm_amd.h): gp_probe's dict -- cost, cost1, model, step2, x2 from the observation terms alone -- plus, per pair in input
        order, Mp (npairs x 6), qp (npairs x 3), pfrozen, pused, and with dc: dsigma, sigma1 (-1 = takes no part); the pairs' scalars
        pcost, pgsmax, and with dc pcost1, pmodel, pstep2, px2; pairs_used, cams_heavy, max_incidences, weight_scale_pt.  sigma: npairs
        scales read where the pair takes part (None: all 1)."""
        n = self.n
        g, keep, _ = _gp_pairs_struct(n, pairs, constraint, calibrated, reweight_scale, fix_centres, want_sigma=False)
        npairs = int(g.npairs)
        pq = GpPairProbe()
        pq.struct_size = C.sizeof(GpPairProbe)
        if sigma is not None:
            sigma = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(npairs))
            pq.sigma_in = sigma.ctypes.data_as(C.c_void_p)
        k1 = max(npairs, 1)
        pout = dict(Mp=np.zeros((k1, 6)), qp=np.zeros((k1, 3)), pfrozen=np.zeros(k1, dtype=np.int32), pused=np.zeros(k1, dtype=np.int32))
        if dc is not None or fix_centres:
            pout.update(dsigma=np.zeros(k1), sigma1=np.zeros(k1))
        for k, v in pout.items():
            setattr(pq, k, v.ctypes.data_as(C.c_void_p))
        if fix_centres and dc is None:
            dc = np.zeros(3 * n)
        out = self.gp_probe(rot, t, P, mu, s=s, min_views=min_views, loss=loss, loss_scale=loss_scale, X=X, dc=dc, _pairs=(g, pq))
        out.update({k: v[:npairs] for k, v in pout.items()})
        out.update(pcost=pq.cost, pgsmax=pq.gsmax, pairs_used=g.pairs_used, cams_heavy=g.cams_heavy, max_incidences=g.max_incidences,
                   weight_scale_pt=g.weight_scale_pt)
        if dc is not None:
            out.update(pcost1=pq.cost1, pmodel=pq.model, pstep2=pq.step2, px2=pq.x2)
        return out

    def gp_probe(self, rot, t, P, mu, s=None, min_views=3, loss="huber", loss_scale=0.1, X=None, dc=None, _pairs=None):
        """one linearisation of global_positioning at (t, P, s) with the damping mu (the test export xm_ctx_gp_probe; include/xm_amd.h): a
        dict of cost, n_used, gmax, M (nobs x 6), q (nobs x 3), frozen, oused (nobs), vinv (m x 6), g_l (m x 3), ustar, sinv (n x 3 x 3), b
        (n x 3), cused, lused; with X (3n x k): SX; with dc (3n): dP (m x 3), ds (nobs), t1, p1, s1, cost1, model, step2, x2.  Arrays per
        observation and per landmark by input index."""
        n, m, nobs = self.n, self.n_landmarks, self.ne
        rot = np.asfortranarray(np.asarray(rot, dtype=np.float64)); t = np.asfortranarray(np.asarray(t, dtype=np.float64))
        P = np.asfortranarray(np.asarray(P, dtype=np.float64))
        assert rot.shape == (3, 3 * n) and t.shape == (3, n) and P.shape == (3, m)
        if loss not in BA_LOSS:
            raise XmError(f"unknown loss {loss!r} (one of {', '.join(BA_LOSS)})")
        q = GpProbe()
        q.struct_size = C.sizeof(GpProbe)
        q.min_views, q.loss, q.loss_scale, q.mu = int(min_views), BA_LOSS[loss], float(loss_scale), float(mu)
        i32 = lambda k: np.zeros(k, dtype=np.int32)
        out = dict(M=np.zeros((nobs, 6)), q=np.zeros((nobs, 3)), frozen=i32(nobs), oused=i32(nobs), vinv=np.zeros((m, 6)), g_l=np.zeros((m, 3)),
                   ustar=np.zeros((n, 3, 3)), sinv=np.zeros((n, 3, 3)), b=np.zeros((n, 3)), cused=i32(n), lused=i32(m))
        if s is not None:
            s = np.ascontiguousarray(np.asarray(s, dtype=np.float64).reshape(nobs))
            q.s = s.ctypes.data_as(C.c_void_p)
        if X is not None:
            X = np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(3 * n, -1))
            q.k, q.X = X.shape[1], X.ctypes.data_as(C.c_void_p)
            out["SX"] = np.zeros(X.shape, order="F")
        if dc is not None:
            dc = np.ascontiguousarray(np.asarray(dc, dtype=np.float64).reshape(3 * n))
            q.dc = dc.ctypes.data_as(C.c_void_p)
            out.update(dP=np.zeros((m, 3)), ds=np.zeros(nobs), t1=np.zeros((3, n), order="F"), p1=np.zeros((3, m), order="F"), s1=np.zeros(nobs))
        for k, v in out.items():
            setattr(q, k, v.ctypes.data_as(C.c_void_p))
        if _pairs is not None:   # gp_probe_pairs: the same arrays through xm_ctx_gp_probe_pairs
            _chk(lib().xm_ctx_gp_probe_pairs(self.h, rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p),
                                             C.byref(q), C.byref(_pairs[0]), C.byref(_pairs[1])))
        else:
            _chk(lib().xm_ctx_gp_probe(self.h, rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p), C.byref(q)))
        out.update(cost=q.cost, n_used=q.n_used, gmax=q.gmax)
        if dc is not None:
            out.update(cost1=q.cost1, model=q.model, step2=np.array(q.step2[:]), x2=np.array(q.x2[:]))
        return out

    def ba_probe(self, rot, t, P, mu, fix_rotations=False, loss="trivial", loss_scale=0.0, preconditioner="jacobi", X=None, dc=None, dense=False):
        """one linearisation of bundle_adjust at (rot, t, P) with the damping mu (the test export xm_ctx_ba_probe; include/xm_amd.h): a dict
        of cost, n_used, gmax, b (n x CD), g_l (m x 3), vinv (m x 6), ustar, sinv (n x CD x CD), cused, lused; with X (CD n x k): SX and MX
        (M^-1 X for the preconditioner); dense=True: Sdense (the lower block triangle); preconditioner "two_level": Pm (CD n x NC), dropped,
        Ac (lower block triangle), coarse_ok, nagg, ncoarse; with dc (CD n): dP (m x 3), rot1, t1, p1, cost1, model, step2, x2.  Landmark
        arrays by input index."""
        return self._ba_probe(rot, t, P, mu, fix_rotations, loss, loss_scale, preconditioner, X, dc, dense, False, None, None)

    def ba_probe_focal(self, rot, t, P, mu, focal=None, focal_free=None, fix_rotations=False, loss="trivial", loss_scale=0.0, X=None, dc=None,
                       dense=False, preconditioner="jacobi", focal_group=None):
        """ba_probe for bundle_adjust(refine_focal=True) (the test export xm_ctx_ba_probe_focal): focal, focal_free as there; the same dict
        with CD = 7, or 4 with fixed rotations, the focal the last entry of a camera's block; with dc also focal1 (n), the candidate's focal
        scales, and cost1 is NaN when one of them is not positive.  preconditioner: only "jacobi" (the others are refused here).
        focal_group (xm_ctx_ba_probe_focal_groups): focal, focal_free per group (G); b (CP n + G), X, SX, MX (CP n + G rows) and dc
        (CP n + G) are vectors of the shared space -- CP = CD - 1 entries per camera, then the G focal entries --, focal1 has G entries,
        and the dict also holds D (G: D_c) and F (the preconditioner's focal block: G x G for G <= BA_FOCAL_GROUPS_EXACT, with coarse_ok =
        1 when it was inverted, else its G diagonal entries); dense=True: Sdense is the lower triangle of the (CP n + G)-row matrix."""
        if focal_group is not None:
            group_of, focal, focal_free = _focal_group_args(self.n, focal_group, focal, focal_free, preconditioner)
            return self._ba_probe(rot, t, P, mu, fix_rotations, loss, loss_scale, preconditioner, X, dc, dense, True, focal, focal_free, group_of)
        focal, focal_free = _focal_args(self.n, focal, focal_free, preconditioner)
        return self._ba_probe(rot, t, P, mu, fix_rotations, loss, loss_scale, preconditioner, X, dc, dense, True, focal, focal_free)

    def ba_probe_radial(self, rot, t, P, mu, focal=None, focal_free=None, distortion=None, distortion_free=None, fix_rotations=False,
                        loss="trivial", loss_scale=0.0, X=None, dc=None, dense=False, preconditioner="jacobi"):
        """ba_probe for bundle_adjust(refine_distortion=True) (the test export xm_ctx_ba_probe_radial): focal, focal_free, distortion,
        distortion_free as there; the same dict with CD = 8, or 5 with fixed rotations, the focal and then the radial coefficient the last
        entries of a camera's block; with dc also focal1 and dist1 (n), the candidate's values, and cost1 is NaN when a focal is not
        positive or the radial map folds at a used observation.  preconditioner: only "jacobi"."""
        focal, focal_free = _focal_args(self.n, focal, focal_free, preconditioner)
        dist, dist_free = _dist_args(self.n, distortion, distortion_free)
        return self._ba_probe(rot, t, P, mu, fix_rotations, loss, loss_scale, preconditioner, X, dc, dense, True, focal, focal_free,
                              dist=dist, dist_free=dist_free)

    def _ba_probe(self, rot, t, P, mu, fix_rotations, loss, loss_scale, preconditioner, X, dc, dense, refine_focal, focal, focal_free,
                  group_of=None, dist=None, dist_free=None):
        rot = np.asfortranarray(np.asarray(rot, dtype=np.float64)); t = np.asfortranarray(np.asarray(t, dtype=np.float64))
        P = np.asfortranarray(np.asarray(P, dtype=np.float64))
        n, m = self.n, self.n_landmarks
        assert rot.shape == (3, 3 * n) and t.shape == (3, n) and P.shape == (3, m)
        if loss not in BA_LOSS:
            raise XmError(f"unknown loss {loss!r} (one of {', '.join(BA_LOSS)})")
        if preconditioner not in BA_PRECONDITIONERS:
            raise XmError(f"unknown preconditioner {preconditioner!r} (one of {', '.join(BA_PRECONDITIONERS)})")
        cd, nc = (3, 4) if fix_rotations else (6, 7)
        cd += 1 if refine_focal else 0
        cd += 1 if dist is not None else 0
        nd = cd * n
        nvec = nd if group_of is None else (cd - 1) * n + focal.size   # entries of b, of a column of X and of dc
        q = BaProbe()
        q.struct_size = C.sizeof(BaProbe)
        q.flags = (BA_FIX_ROTATIONS if fix_rotations else 0) | BA_PRECONDITIONERS[preconditioner] | (BA_REFINE_FOCAL if refine_focal else 0)
        q.flags |= BA_REFINE_RADIAL if dist is not None else 0
        q.loss, q.loss_scale, q.mu = BA_LOSS[loss], float(loss_scale), float(mu)
        out = dict(b=np.zeros((n, cd) if group_of is None else nvec), g_l=np.zeros((m, 3)), vinv=np.zeros((m, 6)), ustar=np.zeros((n, cd, cd)), sinv=np.zeros((n, cd, cd)),
                   cused=np.zeros(n, dtype=np.int32), lused=np.zeros(m, dtype=np.int32))
        if X is not None:
            X = np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(nvec, -1))
            q.k, q.X = X.shape[1], X.ctypes.data_as(C.c_void_p)
            out["SX"] = np.zeros(X.shape, order="F"); out["MX"] = np.zeros(X.shape, order="F")
        if dense:
            if nd > BA_PROBE_DENSE_MAX_ROWS:
                raise XmError("ba_probe: Sdense with more than BA_PROBE_DENSE_MAX_ROWS rows")
            out["Sdense"] = np.zeros((nvec, nvec), order="F")
        ncmax = nc * ((n + BA_AGG_CAMS - 1) // BA_AGG_CAMS)
        if preconditioner == "two_level":
            out["Pm"] = np.zeros((nd, nc)); out["dropped"] = np.zeros(ncmax); out["Ac"] = np.zeros(ncmax * ncmax)
        if dc is not None:
            dc = np.ascontiguousarray(np.asarray(dc, dtype=np.float64).reshape(nvec))
            q.dc = dc.ctypes.data_as(C.c_void_p)
            out.update(dP=np.zeros((m, 3)), rot1=np.zeros((3, 3 * n), order="F"), t1=np.zeros((3, n), order="F"), p1=np.zeros((3, m), order="F"))
        for k, v in out.items():
            setattr(q, k, v.ctypes.data_as(C.c_void_p))
        if group_of is not None:   # the aggregates' pointers serve the groups (include/xm_amd.h): dropped <- D_c, Ac <- F_c
            G = focal.size
            out["D"] = np.zeros(G); out["F"] = np.zeros((G, G), order="F") if G <= BA_FOCAL_GROUPS_EXACT else np.zeros(G)
            q.dropped, q.Ac = out["D"].ctypes.data_as(C.c_void_p), out["F"].ctypes.data_as(C.c_void_p)
            focal1 = np.zeros(focal.size) if dc is not None else None
            _chk(lib().xm_ctx_ba_probe_focal_groups(self.h, rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p),
                                                    focal.size, group_of.ctypes.data_as(C.c_void_p), focal.ctypes.data_as(C.c_void_p),
                                                    None if focal_free is None else focal_free.ctypes.data_as(C.c_void_p), C.byref(q),
                                                    None if focal1 is None else focal1.ctypes.data_as(C.c_void_p)))
            if focal1 is not None:
                out["focal1"] = focal1
        elif dist is not None:
            focal1 = np.zeros(n) if dc is not None else None
            dist1 = np.zeros(n) if dc is not None else None
            V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
            _chk(lib().xm_ctx_ba_probe_radial(self.h, V(rot), V(t), V(P), V(focal), V(focal_free), V(dist), V(dist_free), C.byref(q), V(focal1), V(dist1)))
            if dc is not None:
                out["focal1"] = focal1; out["dist1"] = dist1
        elif refine_focal:
            focal1 = np.zeros(n) if dc is not None else None
            _chk(lib().xm_ctx_ba_probe_focal(self.h, rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p),
                                             focal.ctypes.data_as(C.c_void_p), None if focal_free is None else focal_free.ctypes.data_as(C.c_void_p),
                                             C.byref(q), None if focal1 is None else focal1.ctypes.data_as(C.c_void_p)))
            if focal1 is not None:
                out["focal1"] = focal1
        else:
            _chk(lib().xm_ctx_ba_probe(self.h, rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p), C.byref(q)))
        out.update(cost=q.cost, n_used=q.n_used, gmax=q.gmax, nagg=q.nagg, ncoarse=q.ncoarse, coarse_ok=q.coarse_ok)
        if preconditioner == "two_level":
            k = nc * q.ncoarse
            out["dropped"] = out["dropped"][:k].copy()
            out["Ac"] = out["Ac"][:k * k].reshape(k, k).T.copy()   # column-major with leading dimension NC ncoarse
        if dc is not None:
            out.update(cost1=q.cost1, model=q.model, step2=np.array(q.step2[:]), x2=np.array(q.x2[:]))
        return out

    def rtr_probe(self, o, lam, R, s, p=None, r=None, auto=False, tcg_init=False, delta=1.0, cg_step=None, model_recurrence=False, cert=False, X=None):
        """the trust region's kernels stage by stage at the point (R: 3n x o, s: n) (the test export xm_ctx_rtr_probe; include/xm_amd.h): a dict of
        f, rr, G, egs, S0 (n x 3 x 3), rgR, rgs, product_kind, nA, nB, wpad, w_native; with p = (pR, ps) [and r = (rR, rs)]: HpR, Hps, pHp, rHp,
        HpHp; split_k, sell_gather: the column split and the sliced-ELL gather mode in effect; auto=True: both through the role-switching launch; tcg_init=True (radius delta): init_* and init_scal; cg_step = dict(rr, vv, vp,
        pp, delta, gradnorm, model, iter, v=(vR, vs), Hv=(HvR, Hvs), partsB=array for iter > 0): one cg_step launch -> scal_out, out_*,
        partsB_out, rr_parts (model_recurrence=True: no Hv); cert=True: Lam (n x 3 x 3), dz, dual (2), and SX for X (3n x k)."""
        n, o = self.n, int(o)
        f64 = lambda a, shape: np.asfortranarray(np.asarray(a, dtype=np.float64).reshape(shape))
        q = RtrProbe()
        q.struct_size = C.sizeof(RtrProbe)
        q.o, q.lam = o, float(lam)
        q.flags = (RTR_PROBE_AUTO if auto else 0) | (RTR_PROBE_MODEL_REC if model_recurrence else 0) | (RTR_PROBE_TCG_INIT if tcg_init else 0) | \
                  (RTR_PROBE_CG_STEP if cg_step is not None else 0) | (RTR_PROBE_CERT if cert else 0)
        q.scal_in.delta = float(delta)
        ins = dict(R=f64(R, (3 * n, o)), s=f64(s, (n,)))
        mat = lambda: np.zeros((3 * n, o), order="F")
        out = dict(G=mat(), egs=np.zeros(n), S0=np.zeros((n, 3, 3)), rgR=mat(), rgs=np.zeros(n))
        if p is not None:
            ins.update(pR=f64(p[0], (3 * n, o)), ps=f64(p[1], (n,)))
            out.update(HpR=mat(), Hps=np.zeros(n))
        if r is not None:
            ins.update(rR=f64(r[0], (3 * n, o)), rs=f64(r[1], (n,)))
        if tcg_init:
            out.update({"init_" + k: (np.zeros(n) if k.endswith("s") else mat()) for k in ("rR", "rs", "pR", "ps", "vR", "vs", "HvR", "Hvs")})
            out.update(init_W=mat(), init_Wpad=np.zeros((n, 16)))
        if cg_step is not None:
            for k in RTR_SCAL_IN:
                setattr(q.scal_in, k, (int if k == "iter" else float)(cg_step[k]))
            ins.update(vR=f64(cg_step["v"][0], (3 * n, o)), vs=f64(cg_step["v"][1], (n,)))
            if not model_recurrence:
                ins.update(HvR=f64(cg_step["Hv"][0], (3 * n, o)), Hvs=f64(cg_step["Hv"][1], (n,)))
            if cg_step.get("partsB") is not None:
                ins["partsB_in"] = f64(cg_step["partsB"], (-1,))
                q.partsB_in_count = ins["partsB_in"].size
            out.update({"out_" + k: (np.zeros(n) if k.endswith("s") else mat()) for k in ("vR", "vs", "HvR", "Hvs", "rR", "rs", "pR", "ps")})
            out.update(out_W=mat(), out_Wpad=np.zeros((n, 16)), partsB_out=np.zeros(1024))
        if cert:
            out.update(Lam=np.zeros((n, 3, 3)), dz=np.zeros(n))
            if X is not None:
                ins["X"] = f64(X, (3 * n, -1))
                q.k = ins["X"].shape[1]
                out["SX"] = np.zeros(ins["X"].shape, order="F")
        for k, v in list(ins.items()) + list(out.items()):
            setattr(q, k, v.ctypes.data_as(C.c_void_p))
        _chk(lib().xm_ctx_rtr_probe(self.h, C.byref(q)))
        scal = lambda sc: {k: getattr(sc, k) for k, _ in RtrScal._fields_}
        out.update(f=q.f, rr=q.rr, product_kind=PRODUCT_KINDS.get(q.product_kind, "?"), nA=q.nA, nB=q.nB, wpad=bool(q.wpad), w_native=bool(q.w_native),
                   split_k=q.split_k, sell_gather=q.sell_gather)
        if p is not None:
            out.update(pHp=q.pHp, rHp=q.rHp, HpHp=q.HpHp)
        if tcg_init:
            out["init_scal"] = scal(q.init_scal)
        if cg_step is not None:
            out.update(scal_out=scal(q.scal_out), rr_parts=q.rr_parts, partsB_out=out["partsB_out"][:q.nB].copy())
        if cert:
            out["dual"] = np.array(q.dual[:])
        return {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in out.items()}

    def schur_probe(self, W=None, alpha=1.0, X=None, dense=False):
        """the matrix-free Q stage by stage (the test export xm_ctx_schur_probe; include/xm_amd.h): a dict of the layout (nheavy, lm_total, nagg,
        uses_cg, two_level, dup_pairs, deg), the set-up factors (Q1 n x 3 x 3, c n x 3, q2, q3inv; CG form: dinv; dense=True: VTinv; two-level:
        perm nagg x 64, binv nagg x 64 x 64, ainv); with W (3n x o): h, r, xc, xl, Y of one product alpha Q W and, for the CG form, pcg_done,
        pcg_iters, pcg_relres, pcg_tol, pcg_cap; with X (n - 1 x k, CG form): MX, VX, pAp.  Landmark arrays by input index."""
        n, m = self.n, self.n_landmarks
        n1 = n - 1
        info = self.schur_info()
        q = SchurProbe()
        q.struct_size = C.sizeof(SchurProbe)
        out = dict(deg=np.zeros(m, dtype=np.int32), Q1=np.zeros((n, 3, 3)), c=np.zeros((n, 3)), q2=np.zeros(n), q3inv=np.zeros(m))
        if info["cg"]:
            out["dinv"] = np.zeros(n1)
        elif dense:
            if n1 > SCHUR_PROBE_DENSE_MAX_ROWS:
                raise XmError("schur_probe: VTinv with more than SCHUR_PROBE_DENSE_MAX_ROWS rows")
            out["VTinv"] = np.zeros((n1, n1), order="F")
        if info["precond"] == "two-level" and n1 > 0:
            na = info["aggregates"]
            out.update(perm=np.zeros((na, SCHUR_AGG_CAMS), dtype=np.int32), binv=np.zeros((na, SCHUR_AGG_CAMS, SCHUR_AGG_CAMS)), ainv=np.zeros((na, na), order="F"))
        if W is not None:
            W = np.asfortranarray(np.asarray(W, dtype=np.float64).reshape(3 * n, -1))
            o = W.shape[1]
            q.o, q.W, q.alpha = o, W.ctypes.data_as(C.c_void_p), float(alpha)
            out.update(h=np.zeros((m, o), order="F"), r=np.zeros((n1, o), order="F"), xc=np.zeros((n1, o), order="F"), xl=np.zeros((m, o), order="F"),
                       Y=np.zeros((3 * n, o), order="F"))
        if X is not None:
            X = np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(n1, -1))
            k = X.shape[1]
            q.k, q.X = k, X.ctypes.data_as(C.c_void_p)
            out.update(MX=np.zeros((n1, k), order="F"), VX=np.zeros((n1, k), order="F"), pAp=np.zeros(k))
        for key, v in out.items():
            setattr(q, key, v.ctypes.data_as(C.c_void_p))
        _chk(lib().xm_ctx_schur_probe(self.h, C.byref(q)))
        out.update(nheavy=q.nheavy, lm_total=q.lm_total, nagg=q.nagg, pcg_relres=q.pcg_relres, pcg_tol=q.pcg_tol)
        out.update({key: getattr(q, key) for key in SCHUR_PROBE_INTS})
        return out

    def cert_probe(self, o, lam, R, s, unfused=False, mmax=None, want_V=True):
        """the certificate's Lanczos eigen-solver at the point (R: 3n x o, s: n) (the test export xm_ctx_cert_probe; include/xm_amd.h): a dict of
        ret, eig_exact, theta, resid, iters, m_use, cycles, mmax, steps_dev, steps_fused, steps_unfused, nseg, len, product_kind, Lam (n x 3 x 3), dz,
        dual (2), alpha, beta, c1, c2 (steps_dev each), y (m_use), x (3n) and V (3n x (steps_dev + 1)) from the last restart cycle.  mmax: the
        context's lanczos_mmax (None: its default, 400), which sizes the arrays; unfused=True: XM_CERT_PROBE_UNFUSED."""
        n, o = self.n, int(o)
        cap = min(3 * n, max(2, int(mmax) if mmax else 400))
        q = CertProbe()
        q.struct_size = C.sizeof(CertProbe)
        q.o, q.cap, q.lam, q.flags = o, cap, float(lam), (CERT_PROBE_UNFUSED if unfused else 0)
        ins = dict(R=np.asfortranarray(np.asarray(R, dtype=np.float64).reshape(3 * n, o)), s=np.ascontiguousarray(np.asarray(s, dtype=np.float64).reshape(n)))
        out = dict(Lam=np.zeros((n, 3, 3)), dz=np.zeros(n), alpha=np.zeros(cap), beta=np.zeros(cap), c1=np.zeros(cap), c2=np.zeros(cap), y=np.zeros(cap),
                   x=np.zeros(3 * n))
        if want_V:
            out["V"] = np.zeros((3 * n, cap + 1), order="F")
        for k, v in list(ins.items()) + list(out.items()):
            setattr(q, k, v.ctypes.data_as(C.c_void_p))
        _chk(lib().xm_ctx_cert_probe(self.h, C.byref(q)))
        k = q.steps_dev
        out.update(alpha=out["alpha"][:k].copy(), beta=out["beta"][:k].copy(), c1=out["c1"][:k].copy(), c2=out["c2"][:k].copy(), y=out["y"][:q.m_use].copy())
        if want_V:
            out["V"] = np.ascontiguousarray(out["V"][:, :k + 1])
        out.update({f: getattr(q, f) for f in CERT_INTS if f != "product_kind"})
        out.update(product_kind=PRODUCT_KINDS.get(q.product_kind, "?"), len=q.len, theta=q.theta, resid=q.resid, dual=np.array(q.dual[:]))
        return out

    def outer_probe(self, o, lam, R, s, v=None, Hv=None, retract=False, model_recurrence=False, retraction=None, auto=False, model=0.0, partsM_fill=None,
                    ls=None, step=None):
        """the other half of an outer iteration stage by stage at the point (R: 3n x o, s: n) (the test export xm_ctx_outer_probe; include/xm_amd.h): a
        dict of f, rr, rgR, rgs, product_kind, nA, nB, nM, nwave, grid, wpad, w_native, polar.  retract=True with v = (vR, vs), Hv = (HvR, Hvs):
        ret_Rc, ret_sc, ret_W, ret_Wpad, ret_partsM (nM), model, ret_pad; model_recurrence=True: no Hv, ret_partsM keeps partsM_fill and model is
        the given one.  retraction: None the context's | "polar" | "mgs".  auto=True: the gradient through the role-switching launch.
        ls = (D, t): ls_Rc, ls_W, ls_pad.  step = dict(scal=dict of xm_outer_tcg_t fields, os=dict of xm_outer_scal_t fields, delta_bar, gradtol,
        max_outer, stop_req, slot, p=(pR, ps), r=(rR, rs), cand=(Rc, sc), partsB, partsM) with v, Hv: one outer_step_kernel launch -> scal_out,
        os_out, progress, run, trace (None unless written), out_* and, by role, HpR, Hps, pHp, rHp, HpHp / cand_*, f_cand, rr_cand, m_cand."""
        n, o = self.n, int(o)
        f64 = lambda a, shape: np.asfortranarray(np.asarray(a, dtype=np.float64).reshape(shape))
        q = OuterProbe()
        q.struct_size = C.sizeof(OuterProbe)
        q.o, q.lam = o, float(lam)
        q.flags = (OUTER_PROBE_RETRACT if retract else 0) | (OUTER_PROBE_MODEL_REC if model_recurrence else 0) | (OUTER_PROBE_RETRACT_LS if ls is not None else 0) | \
                  (OUTER_PROBE_STEP if step is not None else 0) | (OUTER_PROBE_AUTO if auto else 0) | \
                  {None: 0, "polar": OUTER_PROBE_POLAR, "mgs": OUTER_PROBE_MGS}[retraction]
        q.scal_in.model = float(model)
        ins = dict(R=f64(R, (3 * n, o)), s=f64(s, (n,)))
        mat = lambda: np.zeros((3 * n, o), order="F")
        nwave = (n + 63) // 64
        shapes = dict(ret_Wpad=(n, 16), out_Wpad=(n, 16), ret_partsM=(1024,), out_partsB=(1024,), out_partsM=(max(1024, nwave),), cand_S0=(n, 3, 3), out_S0=(n, 3, 3))
        new = lambda k: mat() if k in OUTER_MATS else np.zeros(shapes.get(k, (n,)))
        out = {k: new(k) for k in ("rgR", "rgs")}
        if v is not None:
            ins.update(vR=f64(v[0], (3 * n, o)), vs=f64(v[1], (n,)))
        if Hv is not None and not model_recurrence:
            ins.update(HvR=f64(Hv[0], (3 * n, o)), Hvs=f64(Hv[1], (n,)))
        if retract:
            out.update({k: new(k) for k in OUTER_OUT if k.startswith("ret_")})
            if partsM_fill is not None:
                out["ret_partsM"][:] = partsM_fill
        if ls is not None:
            ins["D"] = f64(ls[0], (3 * n, o))
            q.t = float(ls[1])
            out.update(ls_Rc=mat(), ls_W=mat())
        if step is not None:
            for k, val in step["scal"].items():
                setattr(q.scal_in, k, float(val) if k in RTR_SCAL_IN[:7] + ("last_step",) else int(val))
            for k, val in step.get("os", {}).items():
                setattr(q.os_in, k, float(val) if k in ("loss", "rr_point") else int(val))
            q.delta_bar, q.gradtol = float(step.get("delta_bar", 1e30)), float(step.get("gradtol", 0.0))
            q.max_outer, q.stop_req, q.slot = int(step.get("max_outer", 0)), int(step.get("stop_req", 0)), int(step.get("slot", 0))
            ins.update(pR=f64(step["p"][0], (3 * n, o)), ps=f64(step["p"][1], (n,)), rR=f64(step["r"][0], (3 * n, o)), rs=f64(step["r"][1], (n,)))
            if step.get("cand") is not None:
                ins.update(Rc=f64(step["cand"][0], (3 * n, o)), sc=f64(step["cand"][1], (n,)))
            for k in ("partsB", "partsM"):
                if step.get(k) is not None:
                    ins[k + "_in"] = f64(step[k], (-1,))
                    setattr(q, k + "_in_count", ins[k + "_in"].size)
            phase = int(step["scal"].get("phase", PH_TCG))
            out.update({k: new(k) for k in OUTER_OUT if k.startswith("out_")})
            if phase == PH_TCG:
                out.update(HpR=mat(), Hps=np.zeros(n))
            if phase == PH_CAND:
                out.update({k: new(k) for k in OUTER_OUT if k.startswith("cand_")})
        for k, val in list(ins.items()) + list(out.items()):
            setattr(q, k, val.ctypes.data_as(C.c_void_p))
        _chk(lib().xm_ctx_outer_probe(self.h, C.byref(q)))
        fields = lambda sc: {k: getattr(sc, k) for k, _ in sc._fields_ if k != "pad"}
        out.update(f=q.f, rr=q.rr, product_kind=PRODUCT_KINDS.get(q.product_kind, "?"), nA=q.nA, nB=q.nB, nM=q.nM, nwave=q.nwave, grid=q.grid, wpad=bool(q.wpad),
                   w_native=bool(q.w_native), polar=bool(q.polar))
        if retract:
            out.update(model=q.model, ret_partsM=out["ret_partsM"][:q.nM].copy(), ret_pad=tuple(q.ret_pad))
        if ls is not None:
            out["ls_pad"] = tuple(q.ls_pad)
        if step is not None:
            out.update(scal_out=fields(q.scal_out), os_out=fields(q.os_out), progress=int(q.progress), run=int(q.run), out_pad=tuple(q.out_pad),
                       trace=np.array(q.trace[:]) if q.trace_written else None, out_partsB=out["out_partsB"][:q.nB].copy(),
                       out_partsM=out["out_partsM"][:q.nwave].copy())
            if phase == PH_TCG:
                out.update(pHp=q.pHp, rHp=q.rHp, HpHp=q.HpHp)
            if phase == PH_CAND:
                out.update(f_cand=q.f_cand, rr_cand=q.rr_cand, m_cand=q.m_cand)
        return {k: (np.ascontiguousarray(val) if isinstance(val, np.ndarray) else val) for k, val in out.items()}

    def reprojection_errors(self, rot, t, P, focal=None, distortion=None):
        """|r_e|^2 (unrobustified) of every observation in input order at (rot, t, P) -- the layouts of bundle_adjust -- with the
        context's current weights, -1 where the adjustment does not use the observation (weight <= 0 or p_e2 <= 0): an (nobs,) array.
        focal (n): the residual with focal scales, g_i pi(X) - z (xm_ctx_reprojection_errors_focal); distortion (n; focal None = ones):
        the residual g_i (1 + k_i |u|^2) u - z of bundle_adjust(refine_distortion=True) (xm_ctx_reprojection_errors_radial)"""
        if focal is not None or distortion is not None:
            focal, _ = _focal_args(self.n, focal, None)
        if distortion is not None:
            distortion, _ = _dist_args(self.n, distortion, None)
        rot = np.asfortranarray(np.asarray(rot, dtype=np.float64)); t = np.asfortranarray(np.asarray(t, dtype=np.float64))
        P = np.asfortranarray(np.asarray(P, dtype=np.float64))
        assert rot.shape == (3, 3 * self.n) and t.shape == (3, self.n) and P.shape == (3, self.n_landmarks)
        out = np.zeros(self.ne)
        if distortion is not None:
            V = lambda a: a.ctypes.data_as(C.c_void_p)
            _chk(lib().xm_ctx_reprojection_errors_radial(self.h, V(rot), V(t), V(P), V(focal), V(distortion), V(out)))
            return out
        if focal is not None:
            _chk(lib().xm_ctx_reprojection_errors_focal(self.h, rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                                        P.ctypes.data_as(C.c_void_p), focal.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
            return out
        _chk(lib().xm_ctx_reprojection_errors(self.h, rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p),
                                              out.ctypes.data_as(C.c_void_p)))
        return out

    def filter_tracks(self, rot, t, P, reprojection=1e-2, angle=None, triangulation=None, min_views=0):
        """GLOMAP's TrackFilter (track_filter.cc:7-126) at the geometry (rot, t, P) -- the layouts of bundle_adjust -- over this context's
        observations at their CURRENT weights, on the device (xm_ctx_filter_tracks; include/xm_amd.h has the contract); matrix-free
        contexts only, nothing in the context changes.  reprojection: largest reprojection error in normalised image units (GLOMAP:
        1e-2), angle: largest angle between the observed and the predicted ray in degrees (GLOMAP: 1.0), triangulation: smallest
        triangulation angle of a landmark in degrees (GLOMAP: 1.0); None switches a filter off.  min_views > 0: a landmark left with
        fewer observations loses them all.  -> TrackFilterPlan; ctx.set_edge_weights(plan.weights(w)) takes what it dropped out of the
        next solve or bundle_adjust."""
        flags = (TF_REPROJECTION if reprojection is not None else 0) | (TF_ANGLE if angle is not None else 0) | \
                (TF_TRIANGULATION if triangulation is not None else 0)
        for name, v in (("reprojection", reprojection), ("angle", angle), ("triangulation", triangulation)):
            if v is not None and not (np.isfinite(v) and float(v) > 0.0):
                raise XmError(f"filter_tracks: {name} must be finite and positive (None switches the filter off)")
        if int(min_views) < 0:
            raise XmError("filter_tracks: min_views is negative")
        rot = np.asfortranarray(np.asarray(rot, dtype=np.float64)); t = np.asfortranarray(np.asarray(t, dtype=np.float64))
        P = np.asfortranarray(np.asarray(P, dtype=np.float64))
        m = getattr(self, "n_landmarks", 0)   # (a context of another storage has no landmarks: sized for nothing, the library refuses it)
        assert rot.shape == (3, 3 * self.n) and t.shape == (3, self.n) and P.shape == (3, m)
        opt = TfOptions(); res = TfResult()
        opt.struct_size, res.struct_size = C.sizeof(TfOptions), C.sizeof(TfResult)
        opt.flags, opt.min_views = flags, int(min_views)
        opt.max_reprojection_error = float(reprojection or 0.0); opt.max_angle_error = float(angle or 0.0)
        opt.min_triangulation_angle = float(triangulation or 0.0)
        nobs = getattr(self, "ne", 0)
        keep = np.zeros(nobs, dtype=np.uint8); reason = np.zeros(nobs, dtype=np.uint8)
        views = np.zeros(m, dtype=np.int32); status = np.zeros(m, dtype=np.uint8)
        _chk(lib().xm_ctx_filter_tracks(self.h, C.byref(opt), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p),
                                        keep.ctypes.data_as(C.c_void_p), reason.ctypes.data_as(C.c_void_p), views.ctypes.data_as(C.c_void_p),
                                        status.ctypes.data_as(C.c_void_p), C.byref(res)))
        info = {k: getattr(res, k) for k, _ in TfResult._fields_ if k not in ("struct_size", "reserved")}
        return TrackFilterPlan(keep.astype(bool), reason, views, status, info)

    def triangulate_tracks(self, rot, t, P=None, candidates=None, max_hypotheses=64, min_angle=1.0, create_angle=2.0, complete_reprojection=1e-2,
                           min_views=2, refine_rounds=2):
        """every landmark of this context from the rays of its observations at the poses (rot, t) -- the layouts of bundle_adjust -- on the
        device (xm_ctx_triangulate_tracks; include/xm_amd.h has the contract): a search over two-view midpoints in a fixed pair schedule
        (at most max_hypotheses per landmark, scored by the candidates within create_angle degrees), refine_rounds of a linear multi-view
        solve with completion under complete_reprojection (normalised image units), and acceptance with min_views members and a pair of
        them at least min_angle degrees apart.  candidates: None -- the observations of CURRENT weight > 0; a bool mask, or weights whose
        positive entries are the candidates, whatever the context's weights are: this is how dropped observations come back.  P: the
        columns that rejected landmarks keep (None: zeros).  Matrix-free contexts only, nothing in the context changes.
        -> TriangulationPlan; ctx.set_edge_weights(plan.weights(w)) makes the next bundle_adjust use exactly what it kept."""
        rot = np.asfortranarray(np.asarray(rot, dtype=np.float64)); t = np.asfortranarray(np.asarray(t, dtype=np.float64))
        m = getattr(self, "n_landmarks", 0)   # (a context of another storage has no landmarks: sized for nothing, the library refuses it)
        nobs = getattr(self, "ne", 0)
        P = np.zeros((3, m), order="F") if P is None else np.array(P, dtype=np.float64, order="F", copy=True)
        assert rot.shape == (3, 3 * self.n) and t.shape == (3, self.n) and P.shape == (3, m)
        for name, v in (("min_angle", min_angle), ("create_angle", create_angle), ("complete_reprojection", complete_reprojection)):
            if not (np.isfinite(v) and float(v) > 0.0):
                raise XmError(f"triangulate_tracks: {name} must be finite and positive")
        if int(max_hypotheses) < 1 or int(refine_rounds) < 1 or int(min_views) < 0:
            raise XmError("triangulate_tracks: max_hypotheses and refine_rounds must be at least 1, min_views not negative")
        cand = None
        if candidates is not None:
            c = np.asarray(candidates).reshape(-1)
            if c.size != nobs:
                raise XmError("triangulate_tracks: candidates must have one entry per observation")
            cand = np.ascontiguousarray(c if c.dtype == bool else c > 0, dtype=np.uint8)
        opt = TriOptions(); res = TriResult()
        opt.struct_size, res.struct_size = C.sizeof(TriOptions), C.sizeof(TriResult)
        opt.max_hypotheses, opt.min_views, opt.refine_rounds = int(max_hypotheses), int(min_views), int(refine_rounds)
        opt.min_angle, opt.create_max_angle_error, opt.complete_max_reproj_error = float(min_angle), float(create_angle), float(complete_reprojection)
        keep = np.zeros(nobs, dtype=np.uint8); reason = np.zeros(nobs, dtype=np.uint8)
        views = np.zeros(m, dtype=np.int32); status = np.zeros(m, dtype=np.uint8)
        support = np.zeros(m, dtype=np.int32); hyp = np.zeros(m, dtype=np.int32)
        _chk(lib().xm_ctx_triangulate_tracks(self.h, C.byref(opt), rot.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                             P.ctypes.data_as(C.c_void_p), None if cand is None else cand.ctypes.data_as(C.c_void_p),
                                             keep.ctypes.data_as(C.c_void_p), reason.ctypes.data_as(C.c_void_p), views.ctypes.data_as(C.c_void_p),
                                             status.ctypes.data_as(C.c_void_p), support.ctypes.data_as(C.c_void_p), hyp.ctypes.data_as(C.c_void_p),
                                             C.byref(res)))
        info = {k: getattr(res, k) for k, _ in TriResult._fields_ if k not in ("struct_size", "reserved")}
        return TriangulationPlan(P, keep.astype(bool), reason, views, status, support, hyp, info)

    def retriangulate(self, rot, t, P, rounds=1, weights=None, restore_weights=False, reprojection=1e-2, triangulation=1.0, min_views=0,
                      **bundle_adjust_kwargs):
        """GLOMAP's retriangulation step (controllers/global_mapper.cc:322-375) on this context:
          for ite < rounds (:327): triangulate_tracks at the current poses with candidates = weights > 0 (:328-336, where the fork calls
            COLMAP's triangulator: RetriangulateTracks), the context's weights become plan.weights(weights), bundle_adjust (:339-344),
            filter_tracks(reprojection) (:347-354; the fork filters at its fixed threshold here, with no scaling), bundle_adjust (:355-356);
          then the reprojection filter (:364-369) and the triangulation-angle filter (:370-374; None: not run).
        weights: the ENTRY weights, what every observation weighs when it is used (default: the context's current weights); an
        observation that an earlier filter set to 0 comes back when it is positive here and the triangulation at the current poses
        takes it as a member.  THIS METHOD CHANGES THE CONTEXT'S WEIGHTS; restore_weights=True puts back the ones it had when the
        method was called.  min_views goes to every filter call, bundle_adjust_kwargs to every bundle_adjust.
        A round that would leave a camera without a weighted observation raises XmError naming the cameras (set_edge_weights refuses
        such a list); the context then has the weights it had at entry.
        Departures from the reference: those of triangulate_tracks, no NormalizeReconstruction (:358) and no
        UndistortImages (:346).
        -> (rot, t, P, info): info["rounds"] one record per round (triangulation: the plan's counters; ba_first / ba_second: status and
        costs; filter: dropped, tracks_changed, tracks_total), info["final"] the records of the closing filters, info["keep"] the
        observations it ends with, info["weights"] the weights it ends with (before a restore)."""
        if int(rounds) < 0:
            raise XmError("retriangulate: rounds is negative")
        w_ctx = getattr(self, "_w", None)
        w_in = w_ctx if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w_in is None or w_ctx is None:
            raise XmError("retriangulate: the context's current weights are not known here (xm2_round filters inside the library): "
                          "call set_edge_weights first")
        if w_in.size != self.ne:
            raise XmError("retriangulate: weights must have one entry per observation")
        w_entry = w_ctx.copy()
        state = {"w": w_ctx.copy(), "changed": False}

        def give(w, what):
            cam = getattr(self, "_cam", None)
            if cam is not None:
                empty = np.nonzero(np.bincount(np.asarray(cam)[w > 0], minlength=self.n) == 0)[0]
                if empty.size:
                    if state["changed"]:
                        self.set_edge_weights(w_entry)
                    raise XmError(f"retriangulate: {what} would leave no weighted observation for cameras {empty.tolist()}")
            try:
                self.set_edge_weights(w)
            except XmError:
                if state["changed"]:
                    self.set_edge_weights(w_entry)
                raise
            state["w"] = w; state["changed"] = True

        def run_filter(rep, tri):
            plan = self.filter_tracks(rot, t, P, reprojection=rep, angle=None, triangulation=tri, min_views=min_views)
            dropped = int(np.count_nonzero(plan.reason))
            if dropped:
                give(plan.weights(state["w"]), "a filter")
            changed = plan.info["tracks_changed_reprojection"] if rep is not None else plan.info["tracks_changed_triangulation"]
            return dict(reprojection=rep, triangulation=tri, dropped=dropped, tracks_changed=int(changed),
                        tracks_total=int(plan.info["tracks_total"]), info=plan.info)

        def ba_record(i):
            return {k: i[k] for k in ("status", "status_name", "iters", "initial_cost", "final_cost", "n_used")}
        records = []
        for ite in range(int(rounds)):                                                   # :327
            plan = self.triangulate_tracks(rot, t, P, candidates=w_in > 0)               # :328-336
            P = plan.P
            give(plan.weights(w_in), "the triangulation")
            rot, t, P, i1 = self.bundle_adjust(rot, t, P, **bundle_adjust_kwargs)        # :339-344
            f = run_filter(reprojection, None)                                           # :347-354
            rot, t, P, i2 = self.bundle_adjust(rot, t, P, **bundle_adjust_kwargs)        # :355-356
            records.append(dict(ite=ite, triangulation=plan.info, ba_first=ba_record(i1), filter=f, ba_second=ba_record(i2)))
        final = [run_filter(reprojection, None)]                                         # :364-369
        if triangulation is not None:
            final.append(run_filter(None, triangulation))                                # :370-374
        info = dict(rounds=records, final=final, keep=state["w"] > 0, weights=state["w"])
        if restore_weights and state["changed"]:
            self.set_edge_weights(w_entry)
        return rot, t, P, info

    def prune_weakly_connected(self, min_covisibility=5, min_num_images=2, min_num_observations=0, min_threshold=20.0, pairs=False):
        """GLOMAP's PruneWeaklyConnectedImages (reconstruction_pruning.cc:6-84) over this context's observations at their CURRENT weights,
        on the device and with no upload of the list (xm_ctx_prune_weakly_connected; include/xm_amd.h has the contract); matrix-free
        contexts only, nothing in the context changes.  pairs: as in xmamd.prune_weakly_connected.  -> PrunePlan;
        clean_observations(cam, lm, w=plan.weights(w)) gives the list of the next context without the images outside cluster 0 (this
        context cannot take those weights: set_edge_weights refuses a camera without a weighted observation)."""
        opt, _ = _prune_options(min_covisibility, min_num_images, min_num_observations, min_threshold)

        def call(cid, cnt, pp, res):
            return lib().xm_ctx_prune_weakly_connected(self.h, C.byref(opt), cid.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), pp,
                                                       C.byref(res))
        return _prune_call(call, self.n, pairs, getattr(self, "_cam", None))

    def refine_filtered(self, rot, t, P, rounds=3, reprojection=1e-2, triangulation=1.0, min_views=0, restore_weights=False, weights=None,
                        prune=False, **bundle_adjust_kwargs):
        """GLOMAP's alternation of bundle adjustment and track filtering (controllers/global_mapper.cc:243-317) on this context:
          for ite < rounds (:243): bundle_adjust with fix_rotations=True (:250-253), then the full one (:260-265); then (:282-297)
            while ite < rounds: filter_tracks(reprojection = max(3 - ite, 1) * reprojection) (:285-291); the landmarks it changed add up in
            filtered_num; more than 1e-3 * tracks_total of them: back to the adjustment (:293-294), else ite += 1 (:296) and filter again
            with the tighter threshold; the while ending without that: stop (:298-301);
          then the reprojection filter at 1 x reprojection (:307-312) and the triangulation-angle filter (:313-317; None: not run).
        After every filter that dropped something the context's weights become plan.weights(w) (set_edge_weights): THIS METHOD CHANGES
        THE CONTEXT'S WEIGHTS, so that the next adjustment (and a later solve) leaves the dropped observations out; restore_weights=True
        puts the entry weights back before it returns.  weights: the context's current weights (default: those it was created with or
        was last given through set_edge_weights / xm2_filter).  min_views goes to every filter call.  bundle_adjust_kwargs go to every
        bundle_adjust (not fix_rotations).
        Departures from the reference: no NormalizeReconstruction (:273) and no UndistortImages (:279, :305) -- the thresholds are in
        normalised image units and in angles, both free of the scale; the 0.1 % is counted against the landmarks with a used observation
        at that filter call (tracks_total), not against every track ever made (:293); and the departures of filter_tracks itself.
        -> (rot, t, P, info): info["rounds"] one record per adjustment round (ba_fixed / ba_full: status and costs; filters: one record per
        filter call with scaling, threshold, dropped, tracks_changed, tracks_total), info["final"] the records of the two closing
        filters, info["keep"] the kept observations of the last filter call, info["weights"] the weights it ends with (before a
        restore), info["stopped_early"] whether the 0.1 % rule ended the loop.
        prune=True runs prune_weakly_connected (GLOMAP's defaults) behind the closing filters: info["prune"] is its PrunePlan, and
        info["weights"] has zeros for the observations of every camera with cluster_id != 0.  The CONTEXT keeps the weights of the closing
        filters: set_edge_weights refuses a camera without a weighted observation, which is what every pruned camera becomes, so the
        pruned list goes into the next context through clean_observations(cam, lm, w=info["weights"]), which drops and renumbers them.
        The default, False, runs nothing more than before."""
        if "fix_rotations" in bundle_adjust_kwargs:
            raise XmError("refine_filtered: fix_rotations is set by the loop itself (a fixed-rotation adjustment, then the full one)")
        if int(rounds) < 0:
            raise XmError("refine_filtered: rounds is negative")
        w0 = getattr(self, "_w", None) if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w0 is None:
            raise XmError("refine_filtered: the context's current weights are not known here (xm2_round filters inside the library): pass weights=")
        if w0.size != self.ne:
            raise XmError("refine_filtered: weights must have one entry per observation")
        state = {"w": w0.copy(), "changed": False, "keep": None}

        def run_filter(rep, tri, scaling):
            plan = self.filter_tracks(rot, t, P, reprojection=rep, angle=None, triangulation=tri, min_views=min_views)
            dropped = int(np.count_nonzero(plan.reason))
            if dropped:
                state["w"] = plan.weights(state["w"]); state["changed"] = True
                self.set_edge_weights(state["w"])
            state["keep"] = plan.keep
            changed = plan.info["tracks_changed_reprojection"] if rep is not None else plan.info["tracks_changed_triangulation"]
            return dict(scaling=scaling, reprojection=rep, triangulation=tri, dropped=dropped, tracks_changed=int(changed),
                        tracks_total=int(plan.info["tracks_total"]), info=plan.info)

        def ba_record(i):
            return {k: i[k] for k in ("status", "status_name", "iters", "initial_cost", "final_cost", "n_used")}
        records, stopped = [], False
        ite = 0
        while ite < int(rounds):                                                        # :243
            rot, t, P, i1 = self.bundle_adjust(rot, t, P, fix_rotations=True, **bundle_adjust_kwargs)    # :250-253
            rot, t, P, i2 = self.bundle_adjust(rot, t, P, fix_rotations=False, **bundle_adjust_kwargs)   # :260-265
            rec = dict(ite=ite, ba_fixed=ba_record(i1), ba_full=ba_record(i2), filters=[])
            records.append(rec)
            status, filtered_num = True, 0                                              # :282-283
            while status and ite < int(rounds):                                         # :284
                scaling = max(3 - ite, 1)                                               # :285
                f = run_filter(scaling * reprojection, None, scaling)                   # :286-291
                rec["filters"].append(f)
                filtered_num += f["tracks_changed"]
                if filtered_num > 1e-3 * f["tracks_total"]:                             # :293
                    status = False                                                      # :294
                else:
                    ite += 1                                                            # :296
            if status:                                                                  # :298-301
                stopped = True
                break
            ite += 1                                                                    # :243, the for's increment
        final = [run_filter(reprojection, None, 1)]                                     # :307-312
        if triangulation is not None:
            final.append(run_filter(None, triangulation, 1))                            # :313-317
        plan = None
        if prune:                                                                       # global_mapper.cc step 8: PruneWeaklyConnectedImages
            plan = self.prune_weakly_connected()
            state["w"] = plan.weights(state["w"])            # (not given to the context: it cannot hold a camera without a weight)
        info = dict(rounds=records, final=final, keep=state["keep"], weights=state["w"], stopped_early=stopped)
        if plan is not None:
            info["prune"] = plan
        if restore_weights and state["changed"]:
            self.set_edge_weights(w0)
        return rot, t, P, info

    def clean_observations(self, min_cam_obs=10, min_lm_obs=1, swap_first=True):
        """the reference's checklandmarks for this context's list at its CURRENT weights (after xm2_filter / set_edge_weights: the filtered
        list; xm_ctx_clean_observations), matrix-free contexts only; nothing in the context changes.  -> CleanPlan; plan.apply(cam, lm, p, w)
        gives the arguments of the next Context(obs=...)"""
        opt, res = _clean_options(min_cam_obs, min_lm_obs, swap_first)
        # (a context of another storage has no observations: sized for nothing, the library refuses it)
        keep = np.zeros(getattr(self, "ne", 0), dtype=np.uint8); ci = np.full(self.n, -1, dtype=np.int32)
        li = np.full(getattr(self, "n_landmarks", 0), -1, dtype=np.int32)
        _chk(lib().xm_ctx_clean_observations(self.h, C.byref(opt), keep.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                             li.ctypes.data_as(C.c_void_p), C.byref(res)))
        return _clean_plan(keep, ci, li, res)

    def edge_residuals_recovered(self, rot, scale):
        """squared distance per edge / observation of a RECOVERED solution (rot 3 x 3n, scale n): the reference's XM^2 residual"""
        rot = np.asfortranarray(np.asarray(rot, dtype=np.float64)); scale = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(-1))
        res = np.zeros(self.ne)
        _chk(lib().xm_ctx_edge_residuals_recovered(self.h, rot.ctypes.data_as(C.c_void_p), scale.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)))
        return res

    def xm2_filter(self, rot, scale, percentile=90.0):
        """the reference's percentile filter on the device -> (threshold, newly removed, new weights); Q is rebuilt.  The threshold sits at the
        exact position (nlive - 1) * percentile / 100 of the live errors; a weight of -0.0 is a removed edge like 0, removed edges come back
        as +0.0; a negative or NaN current weight is refused (xm_ctx_xm2_filter)"""
        rot = np.asfortranarray(np.asarray(rot, dtype=np.float64)); scale = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(-1))
        thr = C.c_double(); rm = C.c_int64(); w = np.zeros(self.ne)
        _chk(lib().xm_ctx_xm2_filter(self.h, rot.ctypes.data_as(C.c_void_p), scale.ctypes.data_as(C.c_void_p), percentile, C.byref(thr), C.byref(rm),
                                     w.ctypes.data_as(C.c_void_p)))
        self._w = w.copy()
        return thr.value, rm.value, w

    def xm2_round(self, R, s, max_rank, tol, max_time=1000.0, percentile=90.0, flags=0):
        """one round of the reference's XM^2 loop starting from the solution (R, s): filter, solve_rank3 at lam 0, lam decision, final solve"""
        n = self.n
        R = np.asfortranarray(np.asarray(R, dtype=np.float64)); s = np.ascontiguousarray(np.asarray(s, dtype=np.float64).reshape(-1))
        rmax = max(int(max_rank), 3)
        Ro = np.zeros((3 * n, rmax + 1), order="F"); so = np.zeros(n)
        opt = Options(); res = Result(); inf = Xm2Info()
        opt.struct_size, res.struct_size, inf.struct_size = C.sizeof(Options), C.sizeof(Result), C.sizeof(Xm2Info)
        opt.max_rank, opt.tol, opt.max_time, opt.flags = int(max_rank), tol, max_time, flags
        inf.percentile = percentile
        res.R = Ro.ctypes.data_as(C.c_void_p); res.s = so.ctypes.data_as(C.c_void_p)
        _chk(lib().xm_ctx_xm2_round(self.h, R.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), R.shape[1], C.byref(opt), C.byref(inf), C.byref(res)))
        self._w = None   # the round filtered inside the library: the weights are no longer known here
        info = {k: getattr(res, k) for k, _ in Result._fields_ if k not in ("R", "s", "struct_size")}
        x2 = {k: getattr(inf, k) for k, _ in Xm2Info._fields_ if k != "struct_size"}
        return np.ascontiguousarray(Ro[:, : res.rank]), so, info, x2

    def set_edge_weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert w.size == self.ne
        _chk(lib().xm_ctx_set_edge_weights(self.h, w.ctypes.data_as(C.c_void_p)))
        self._w = w.reshape(-1).copy()

    def solve(self, max_rank, tol, lam, max_time=1000.0, mode=MODE_SOLVE, flags=0, s_ini=None, trace=0, R_ini=None, retraction=RETRACT_QR,
              grouping=0):
        n = self.n
        rmax = max(int(max_rank), 3)
        R = np.zeros((3 * n, rmax + 1), order="F"); s = np.zeros(n)
        opt = Options(); res = Result()
        opt.struct_size, res.struct_size = C.sizeof(Options), C.sizeof(Result)
        opt.retraction, opt.sum_grouping = int(retraction), int(grouping)
        opt.max_rank, opt.tol, opt.lam, opt.max_time, opt.mode, opt.flags = int(max_rank), tol, lam, max_time, mode, flags
        si = None
        if s_ini is not None:
            si = np.ascontiguousarray(s_ini, dtype=np.float64).reshape(-1)
            opt.s_ini = si.ctypes.data_as(C.c_void_p)
        ri = None
        if R_ini is not None:
            ri = np.asfortranarray(np.asarray(R_ini, dtype=np.float64)[:, :3])
            opt.R_ini = ri.ctypes.data_as(C.c_void_p); opt.flags |= FLAG_WARM_R
        tr = None
        if trace:
            tr = np.zeros((trace, 6)); opt.trace_cap = trace; opt.trace = tr.ctypes.data_as(C.c_void_p)
        res.R = R.ctypes.data_as(C.c_void_p); res.s = s.ctypes.data_as(C.c_void_p)
        _chk(lib().xm_ctx_solve(self.h, C.byref(opt), C.byref(res)))
        info = {k: getattr(res, k) for k, _ in Result._fields_ if k not in ("R", "s", "struct_size")}
        # trust regions of this solve whose tCG iteration was two launches (0: all three -- FLAG_TCG_THREE_LAUNCH or a form it does not cover)
        cnt = C.c_int(0)
        info["tcg_two_launch"] = cnt.value if lib().xm_ctx_tcg_two_launch(self.h, C.byref(cnt)) == 0 else 0
        # truncated CGs behind a rejected step that were replayed from the rejected one's history, and the iterations they stand for (in tcg_iters)
        rp = (C.c_int64 * 2)(0, 0)
        ok = lib().xm_ctx_tcg_replay(self.h, rp) == 0
        info["tcg_replays"], info["tcg_replayed_iters"] = (int(rp[0]), int(rp[1])) if ok else (0, 0)
        if tr is not None:
            info["trace"] = tr[: res.trace_len].copy()
        return np.ascontiguousarray(R[:, : res.rank]), s, info

    def set_tcg_history(self, iterations):
        """iterations of a truncated CG kept for the replay of a rejected step, from the next solve on (0 = default 64, 1 .. 256; xm_ctx_set_tcg_history)"""
        _chk(lib().xm_ctx_set_tcg_history(self.h, int(iterations)))

    def close(self):
        if self.h:
            lib().xm_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_dense(Q, max_rank, tol, lam, tuning=None, **kw):
    ctx = Context(Q=Q, tuning=tuning)
    try:
        return ctx.solve(max_rank, tol, lam, **kw)
    finally:
        ctx.close()


def import_XM():
    """import the reference-named extension module `XM` (xm-code_amd/build/XM*.so)"""
    import importlib
    import sys
    if MODULE_DIR not in sys.path:
        sys.path.insert(0, MODULE_DIR)
    return importlib.import_module("XM")
