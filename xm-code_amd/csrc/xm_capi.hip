// xm_capi.hip — extern "C" boundary (include/xm_amd.h).  No exceptions cross it.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <mutex>
#include <vector>

#include "xm_ba.h"
#include "xm_gp.h"
#include "xm_lm_loop.h"
#include "xm_clean.h"
#include "xm_trackfilter.h"
#include "xm_triangulate.h"
#include "xm_prune.h"
#include "xm_lift.h"
#include "xm_tracks.h"
#include "xm_tracks_split.h"
#include "xm_viewgraph.h"
#include "xm_vgcalib.h"
#include "xm_rotavg.h"
#include "xm_pair.h"
#include "xm_schur.h"
#include "xm_sell.h"
#include "xm_symw.h"
#include "xm_solver.h"
#include "xm_stage.h"

struct xm_ctx {
    std::unique_ptr<xm::Context> impl;   // one GPU (or one rank of a multi-process run)
    std::unique_ptr<xm::Team> team;      // n_gpus > 1: single-process multi-GPU
};

namespace {
thread_local std::string g_err;
int fail(const xm::Error &e) { g_err = e.what(); return e.code; }
int fail(const std::exception &e) { g_err = e.what(); return XM_ERR_HIP; }

#define XM_TRY try {
#define XM_CATCH                                                       \
    }                                                                  \
    catch (const xm::Error &e) { return fail(e); }                     \
    catch (const std::bad_alloc &) { g_err = "out of host memory"; return XM_ERR_NOMEM; } \
    catch (const std::exception &e) { return fail(e); }

// Revision-3 structs start with the caller's sizeof: copy what the caller has, zero the rest (include/xm_amd.h, XM_ABI_REVISION)
template <class T>
T take_struct(const T *p, const char *what) {
    T out;
    std::memset(&out, 0, sizeof(T));
    if (!p) throw xm::Error(XM_ERR_ARG, std::string(what) + ": null");
    const uint32_t sz = p->struct_size;
    if (sz < 16 || sz > 4096) throw xm::Error(XM_ERR_ARG, std::string(what) + ": struct_size is not set (ABI revision 3: the first field of the struct is sizeof(struct))");
    std::memcpy(&out, p, std::min<size_t>(sz, sizeof(T)));
    out.struct_size = (uint32_t)sizeof(T);
    return out;
}
void give_result(xm_result_t *dst, const xm_result_t &src, uint32_t caller_size) {
    xm_result_t tmp = src;
    tmp.struct_size = caller_size;
    std::memcpy(dst, &tmp, std::min<size_t>(caller_size, sizeof(xm_result_t)));
}

void require_device() {
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt < 1)
        throw xm::Error(XM_ERR_HIP, "no HIP device available: the XM solver has no CPU fallback (it needs an MI355X / gfx950 GPU)");
}

// .bin matrix: int32 rows, int32 cols, float64 column-major (XM_main.cu:18-33, utils/io.py:17-54).  The reference's Python I/O
// also knows a variant with two 8-byte header fields (utils/io.py:24-26 `byte = 8`) that its C++ loader cannot read; it is
// accepted here (told apart by the file size), which lifts the int32 limit on rows*cols for large Q.
void read_bin(const std::string &fn, std::vector<double> &d, int64_t &rows, int64_t &cols) {
    std::ifstream f(fn, std::ios::binary | std::ios::ate);
    if (!f) throw xm::Error(XM_ERR_IO, "cannot open file " + fn);
    const int64_t size = (int64_t)f.tellg();
    f.seekg(0);
    unsigned char raw[16] = {0};
    f.read(reinterpret_cast<char *>(raw), std::min<int64_t>(16, size));
    int32_t h4[2];
    int64_t h8[2];
    std::memcpy(h4, raw, 8);
    std::memcpy(h8, raw, 16);
    int64_t skip;
    const bool v1 = size >= 8 && h4[0] >= 0 && h4[1] >= 0 && 8 + 8 * (int64_t)h4[0] * (int64_t)h4[1] == size;
    const bool v2 = !v1 && size >= 16 && h8[0] >= 0 && h8[1] >= 0 && h8[0] < (1LL << 31) && h8[1] < (1LL << 31) &&
                    16 + 8 * h8[0] * h8[1] == size;
    if (v2) { rows = h8[0]; cols = h8[1]; skip = 16; }
    else {
        if (size < 8 || h4[0] < 0 || h4[1] < 0) throw xm::Error(XM_ERR_IO, "bad header in " + fn);
        rows = h4[0]; cols = h4[1]; skip = 8;
        if (8 + 8 * rows * cols > size) throw xm::Error(XM_ERR_IO, "short file " + fn);
    }
    f.clear();
    f.seekg(skip);
    d.resize((size_t)rows * (size_t)cols);
    f.read(reinterpret_cast<char *>(d.data()), (std::streamsize)(d.size() * sizeof(double)));
    if ((size_t)f.gcount() != d.size() * sizeof(double)) throw xm::Error(XM_ERR_IO, "short file " + fn);
}
// header of a .bin matrix without reading the data: rows, cols and the byte offset of element (0, 0)
void peek_bin(const std::string &fn, int64_t &rows, int64_t &cols, int64_t &skip) {
    std::ifstream f(fn, std::ios::binary | std::ios::ate);
    if (!f) throw xm::Error(XM_ERR_IO, "cannot open file " + fn);
    const int64_t size = (int64_t)f.tellg();
    f.seekg(0);
    unsigned char raw[16] = {0};
    f.read(reinterpret_cast<char *>(raw), std::min<int64_t>(16, size));
    int32_t h4[2];
    int64_t h8[2];
    std::memcpy(h4, raw, 8);
    std::memcpy(h8, raw, 16);
    const bool v1 = size >= 8 && h4[0] >= 0 && h4[1] >= 0 && 8 + 8 * (int64_t)h4[0] * (int64_t)h4[1] == size;
    const bool v2 = !v1 && size >= 16 && h8[0] >= 0 && h8[1] >= 0 && h8[0] < (1LL << 31) && h8[1] < (1LL << 31) && 16 + 8 * h8[0] * h8[1] == size;
    if (v2) { rows = h8[0]; cols = h8[1]; skip = 16; }
    else {
        if (size < 8 || h4[0] < 0 || h4[1] < 0) throw xm::Error(XM_ERR_IO, "bad header in " + fn);
        rows = h4[0]; cols = h4[1]; skip = 8;
        if (8 + 8 * rows * cols > size) throw xm::Error(XM_ERR_IO, "short file " + fn);
    }
}
// rows [r0, r0 + nr) of a column-major .bin matrix, all columns -> dst (column-major, leading dimension nr): one contiguous
// piece per column, so a rank of a multi-GPU run reads 1/world of Q.bin instead of all of it
void read_bin_rows(const std::string &fn, int64_t r0, int64_t nr, std::vector<double> &dst, int64_t rows, int64_t cols, int64_t skip) {
    std::ifstream f(fn, std::ios::binary);
    if (!f) throw xm::Error(XM_ERR_IO, "cannot open file " + fn);
    dst.resize((size_t)std::max<int64_t>(nr, 0) * (size_t)cols);
    for (int64_t c = 0; c < cols && nr > 0; ++c) {
        f.seekg(skip + 8 * (c * rows + r0));
        f.read(reinterpret_cast<char *>(dst.data() + (size_t)c * nr), (std::streamsize)(nr * 8));
        if (f.gcount() != (std::streamsize)(nr * 8)) throw xm::Error(XM_ERR_IO, "short file " + fn);
    }
}
void write_bin(const std::string &fn, const double *d, int32_t rows, int32_t cols) {
    std::ofstream f(fn, std::ios::binary);
    if (!f) throw xm::Error(XM_ERR_IO, "cannot write " + fn);
    f.write(reinterpret_cast<const char *>(&rows), 4);
    f.write(reinterpret_cast<const char *>(&cols), 4);
    f.write(reinterpret_cast<const char *>(d), (std::streamsize)((size_t)rows * (size_t)cols * sizeof(double)));
}

int solve_path(const char *dataset_path, unsigned max_rank, double tol, double lam, double max_time, int mode, int *status) {
    if (!dataset_path) throw xm::Error(XM_ERR_ARG, "dataset_path is NULL");
    require_device();
    const std::string base(dataset_path);
    std::vector<double> Q, sini;
    int64_t rows = 0, cols = 0, skip = 0;
    const std::shared_ptr<xm::Comm> cmp = xm::default_comm();
    const xm::Comm &cm = *cmp;
    const bool strip = cm.world > 1;                    // row-partitioned run: this rank needs only the rows of its cameras
    if (strip) peek_bin(base + "/Q.bin", rows, cols, skip);
    else read_bin(base + "/Q.bin", Q, rows, cols);      // XM_main.cu:185
    if (rows != cols || rows % 3 != 0 || rows < 3) throw xm::Error(XM_ERR_IO, "Q.bin must be 3n x 3n");
    const bool verbose = std::getenv("XM_QUIET") == nullptr;
    if (verbose) printf("rows: %lld, cols: %lld\n", (long long)rows, (long long)cols);
    const int64_t n = rows / 3;
    if (mode == XM_MODE_REBUTTLE) {
        int64_t r2, c2;
        read_bin(base + "/s_ini.bin", sini, r2, c2);      // XM_main.cu:42,62
        if ((int64_t)sini.size() < n) throw xm::Error(XM_ERR_IO, "s_ini.bin too short");
        std::vector<double> rini;
        read_bin(base + "/R_ini.bin", rini, r2, c2);      // read like the reference (XM_main.cu:41,61); its content is then
                                                          // overwritten by the identity stack at rank 3 (XM_main.cu:95-103)
    }
    xm_problem_t prob;
    std::memset(&prob, 0, sizeof(prob));
    prob.struct_size = sizeof(prob);
    prob.n = n; prob.storage = XM_STORAGE_DENSE; prob.q = Q.data(); prob.ldq = rows;
    // XM_GPUS=N: the reference's own single-process call on N GPUs of this node (XM_GPU_MAP=1: N virtual ranks on device 0)
    const int n_gpus = (int)std::max(1L, std::min(8L, std::getenv("XM_GPUS") ? std::atol(std::getenv("XM_GPUS")) : 1L));
    const int gpu_map = std::getenv("XM_GPU_MAP") ? std::atoi(std::getenv("XM_GPU_MAP")) : 0;
    if (strip) {
        const int64_t per = xm::equal_range_len(n, cm.world);                    // same partition as xm_partition / Context
        const int64_t c0 = std::min<int64_t>(n, (int64_t)cm.rank * per), c1 = std::min<int64_t>(n, (int64_t)(cm.rank + 1) * per);
        read_bin_rows(base + "/Q.bin", 3 * c0, 3 * (c1 - c0), Q, rows, cols, skip);
        prob.q = Q.data(); prob.ldq = 3 * (c1 - c0); prob.q_row0 = 3 * c0;
        if (c1 == c0) { Q.assign(1, 0.0); prob.q = Q.data(); prob.ldq = 0; prob.q_row0 = 3 * c0; }
    }
    std::unique_ptr<xm::Context> ctx;
    std::unique_ptr<xm::Team> team;
    if (!strip && n_gpus > 1) team.reset(new xm::Team(prob, n_gpus, gpu_map));
    else ctx.reset(new xm::Context(prob));
    std::vector<double>().swap(Q);
    const unsigned rmax = std::max(3u, max_rank);
    std::vector<double> R((size_t)rows * (rmax + 1), 0.0), s((size_t)n, 1.0);
    xm_options_t opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.struct_size = sizeof(opt);
    opt.max_rank = max_rank; opt.tol = tol; opt.lam = lam; opt.max_time = max_time; opt.mode = mode;
    opt.flags = verbose ? XM_FLAG_VERBOSE : 0;
    opt.s_ini = sini.empty() ? nullptr : sini.data();
    if (const char *e = std::getenv("XM_RETRACTION")) opt.retraction = (*e == 'p' || *e == 'P' || *e == '1') ? XM_RETRACT_POLAR : XM_RETRACT_QR;
    xm_result_t res;
    std::memset(&res, 0, sizeof(res));
    res.R = R.data(); res.s = s.data();
    if (team) team->solve(opt, res); else ctx->solve(opt, res);
    if (cm.rank == 0) {
        write_bin(base + "/R.bin", R.data(), (int32_t)rows, res.rank);   // XM_main.cu:284-294
        if (verbose) printf("saved R\n");
        write_bin(base + "/s.bin", s.data(), (int32_t)n, 1);             // XM_main.cu:298-305
    }
    if (status) *status = res.status;
    return XM_OK;
}
// what xm_ctx_global_positioning and xm_ctx_gp_probe refuse alike
void gp_check(const char *who, xm_ctx_t *ctx, int loss, double loss_scale, int min_views, const double *rot, const double *t, const double *p) {
    const std::string w(who);
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, w + ": single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1) throw xm::Error(XM_ERR_ARG, w + ": single-rank contexts only");
    if (loss < XM_BA_LOSS_TRIVIAL || loss > XM_BA_LOSS_ARCTAN) throw xm::Error(XM_ERR_ARG, w + ": unknown loss");
    if (loss == XM_BA_LOSS_TRIVIAL && loss_scale != 0.0) throw xm::Error(XM_ERR_ARG, w + ": loss_scale is given but the loss is trivial");
    if (loss != XM_BA_LOSS_TRIVIAL && !(std::isfinite(loss_scale) && loss_scale > 0.0))
        throw xm::Error(XM_ERR_ARG, w + ": a robust loss needs a finite loss_scale > 0");
    if (min_views < 0) throw xm::Error(XM_ERR_ARG, w + ": min_views is negative");
    const int64_t n = ctx->impl->cameras(), m = ctx->impl->n_landmarks();
    for (int64_t k = 0; k < 9 * n; ++k)
        if (!std::isfinite(rot[k])) throw xm::Error(XM_ERR_ARG, w + ": rotations are not finite");
    for (int64_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(t[k])) throw xm::Error(XM_ERR_ARG, w + ": centres are not finite");
    for (int64_t k = 0; k < 3 * m; ++k)
        if (!std::isfinite(p[k])) throw xm::Error(XM_ERR_ARG, w + ": points are not finite");
}
// xm_gp_options_t -> the solver's settings, with the refusals the two positioning entries share
xm::GpSettings gp_settings(const char *who, xm_ctx_t *ctx, const xm_gp_options_t *opt, const xm_gp_result_t *res, const double *rot, const double *t,
                           const double *p) {
    const std::string w(who);
    if (!ctx || !opt || !res || !rot || !t || !p) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_gp_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_gp_options_t.struct_size is not sizeof(xm_gp_options_t)");
    if (res->struct_size != sizeof(xm_gp_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_gp_result_t.struct_size is not sizeof(xm_gp_result_t)");
    const xm_gp_options_t &o = *opt;
    auto bad = [](double v) { return !(v >= 0.0) || !std::isfinite(v); };
    if (!(o.eta > 0.0 && o.eta < 1.0)) throw xm::Error(XM_ERR_ARG, w + ": eta must lie in (0, 1)");
    if (o.max_iters < 0 || bad(o.max_time) || bad(o.function_tol) || bad(o.gradient_tol) || bad(o.parameter_tol))
        throw xm::Error(XM_ERR_ARG, w + ": negative or non-finite setting");
    if (o.trace_cap < 0 || (o.trace_cap > 0 && !o.trace)) throw xm::Error(XM_ERR_ARG, w + ": trace_cap > 0 needs a trace array");
    gp_check(who, ctx, o.loss, o.loss_scale, o.min_views, rot, t, p);
    xm::GpSettings c;
    if (o.max_iters > 0) c.max_iters = o.max_iters;
    if (o.max_time > 0.0) c.max_time = o.max_time;
    if (o.function_tol > 0.0) c.function_tol = o.function_tol;
    if (o.gradient_tol > 0.0) c.gradient_tol = o.gradient_tol;
    if (o.parameter_tol > 0.0) c.parameter_tol = o.parameter_tol;
    if (o.min_views > 0) c.min_views = o.min_views;
    c.eta = o.eta;
    c.loss = o.loss; c.loss_scale = o.loss_scale;
    c.trace_cap = o.trace_cap; c.trace = o.trace;
    return c;
}
void gp_result_out(const xm::GpOutcome &r, xm_gp_result_t *res) {
    xm_gp_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_gp_result_t);
    out.status = r.status; out.iters = r.iters; out.accepted = r.accepted; out.pcg_iters = r.pcg_iters; out.n_used = r.n_used;
    out.initial_cost = r.initial_cost; out.final_cost = r.final_cost; out.gradient_max = r.gradient_max; out.seconds = r.seconds;
    out.trace_len = r.trace_len;
    *res = out;
}
// xm_gp_pairs_t -> the solver's view of it, with the refusals of the contract (the context is known to be a single one: gp_check came first)
xm::GpPairsIn gp_pairs_in(const char *who, xm_ctx_t *ctx, const xm_gp_pairs_t *pr) {
    const std::string w(who);
    if (pr->struct_size != sizeof(xm_gp_pairs_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_gp_pairs_t.struct_size is not sizeof(xm_gp_pairs_t)");
    if (pr->constraint < XM_GP_ONLY_POINTS || pr->constraint > XM_GP_POINTS_AND_CAMERAS) throw xm::Error(XM_ERR_ARG, w + ": unknown constraint type");
    if (pr->flags & ~XM_GP_FIX_CENTRES) throw xm::Error(XM_ERR_ARG, w + ": unknown flag");
    const bool fix = (pr->flags & XM_GP_FIX_CENTRES) != 0;
    if (fix && pr->constraint != XM_GP_ONLY_POINTS) throw xm::Error(XM_ERR_ARG, w + ": XM_GP_FIX_CENTRES goes with XM_GP_ONLY_POINTS only");
    if (pr->npairs < 0 || pr->npairs > INT32_MAX) throw xm::Error(XM_ERR_ARG, w + ": npairs is negative or too large");
    if (pr->npairs > 0 && (!pr->pi || !pr->pj || !pr->trel)) throw xm::Error(XM_ERR_ARG, w + ": npairs > 0 needs pi, pj and trel");
    if (!(pr->reweight_scale >= 0.0) || !std::isfinite(pr->reweight_scale)) throw xm::Error(XM_ERR_ARG, w + ": reweight_scale is negative or not finite");
    const int64_t n = ctx->impl->cameras();
    int64_t part = 0;
    for (int64_t k = 0; k < pr->npairs; ++k) {
        const int64_t i = pr->pi[k], j = pr->pj[k];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j) throw xm::Error(XM_ERR_ARG, w + ": a pair names a camera outside [0, n) or one camera twice");
        if (pr->valid && !pr->valid[k]) continue;
        ++part;
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(pr->trel[3 * k + c])) throw xm::Error(XM_ERR_ARG, w + ": trel of a participating pair is not finite");
    }
    if (pr->constraint != XM_GP_ONLY_POINTS && part == 0)
        throw xm::Error(XM_ERR_ARG, w + ": the constraint type has pair terms but no pair takes part");
    xm::GpPairsIn in;
    in.constraint = pr->constraint; in.fix_centres = fix; in.npairs = pr->npairs;
    in.pi = pr->pi; in.pj = pr->pj; in.trel = pr->trel; in.valid = pr->valid; in.calibrated = pr->calibrated;
    in.reweight_scale = pr->reweight_scale > 0.0 ? pr->reweight_scale : 1.0;
    in.sigma = pr->sigma;
    return in;
}
void gp_pairs_out(const xm::GpPairsIn &in, xm_gp_pairs_t *pr) {
    pr->pairs_used = in.pairs_used; pr->cams_heavy = in.cams_heavy; pr->max_incidences = in.max_incidences; pr->weight_scale_pt = in.weight_scale_pt;
}
}  // namespace

extern "C" {

const char *xm_last_error(void) { return g_err.c_str(); }
const char *xm_version(void) { return "xm-amd 0.5 (gfx950)"; }
int xm_abi_revision(void) { return XM_ABI_REVISION; }

int xm_solve(const char *p, unsigned int max_rank, double tol, double lam, double max_time) {
    XM_TRY return solve_path(p, max_rank, tol, lam, max_time, XM_MODE_SOLVE, nullptr); XM_CATCH
}
int xm_solve_rank3(const char *p, unsigned int max_rank, double tol, double lam, double max_time) {
    XM_TRY return solve_path(p, max_rank, tol, lam, max_time, XM_MODE_RANK3, nullptr); XM_CATCH
}
int xm_solve_rebuttle(const char *p, unsigned int max_rank, double tol, double lam, double max_time, int *status) {
    XM_TRY return solve_path(p, max_rank, tol, lam, max_time, XM_MODE_REBUTTLE, status); XM_CATCH
}

int xm_ctx_create(const xm_problem_t *prob, xm_ctx_t **out) {
    XM_TRY
    if (!prob || !out) throw xm::Error(XM_ERR_ARG, "null argument");
    require_device();
    const xm_problem_t pr = take_struct(prob, "xm_problem_t");
    auto *c = new xm_ctx;
    try {
        if (pr.n_gpus > 1) {
            if (xm::default_comm()->world > 1) throw xm::Error(XM_ERR_ARG, "n_gpus > 1 inside a multi-process run (xm_comm_init): use one or the other");
            c->team.reset(new xm::Team(pr, pr.n_gpus, pr.gpu_map));
        } else {
            c->impl.reset(new xm::Context(pr));
        }
    } catch (...) { delete c; throw; }
    *out = c;
    return XM_OK;
    XM_CATCH
}
int xm_ctx_solve(xm_ctx_t *ctx, const xm_options_t *opt, xm_result_t *res) {
    XM_TRY
    if (!ctx || !opt || !res) throw xm::Error(XM_ERR_ARG, "null argument");
    const xm_options_t op = take_struct(opt, "xm_options_t");
    xm_result_t rs = take_struct(res, "xm_result_t");
    const uint32_t caller = res->struct_size;
    if (ctx->team) ctx->team->solve(op, rs); else ctx->impl->solve(op, rs);
    give_result(res, rs, caller);
    return XM_OK;
    XM_CATCH
}
void xm_ctx_destroy(xm_ctx_t *ctx) { delete ctx; }
int xm_ctx_qw(xm_ctx_t *ctx, int o, const double *W, double *out, double alpha) {
    XM_TRY
    if (!ctx) throw xm::Error(XM_ERR_ARG, "null argument");
    if (!ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_qw: single-GPU contexts only");
    ctx->impl->apply(o, W, out, alpha);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_attach_edges(xm_ctx_t *ctx, int64_t ne, const int32_t *ei, const int32_t *ej, const double *M) {
    XM_TRY
    if (!ctx) throw xm::Error(XM_ERR_ARG, "null argument");
    if (ctx->team) ctx->team->attach_edges(ne, ei, ej, M); else ctx->impl->attach_edges(ne, ei, ej, M);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_edge_residuals(xm_ctx_t *ctx, double *res) {
    XM_TRY
    if (!ctx) throw xm::Error(XM_ERR_ARG, "null argument");
    if (ctx->team) ctx->team->edge_residuals(res); else ctx->impl->edge_residuals(res);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_recover_tp(xm_ctx_t *ctx, const double *rot, const double *scale, double *t, double *p) {
    XM_TRY
    if (!ctx) throw xm::Error(XM_ERR_ARG, "null argument");
    if (!ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_recover_tp: single-GPU contexts only");
    ctx->impl->recover_tp(rot, scale, t, p);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_dense_q(xm_ctx_t *ctx, double *q, int64_t ldq) {
    XM_TRY
    if (!ctx || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_dense_q: single-GPU contexts only");
    ctx->impl->dense_q(q, ldq);
    return XM_OK;
    XM_CATCH
}
int xm_create_matrix(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *p, const double *w, double *Q,
                     int64_t ldq, double *Abar) {
    XM_TRY
    if (!Q || ldq < 3 * n) throw xm::Error(XM_ERR_ARG, "xm_create_matrix: null Q or ldq < 3n");
    if (n > xm::kSchurDenseQMaxCams) throw xm::Error(XM_ERR_ARG, "xm_create_matrix: more than " + std::to_string(xm::kSchurDenseQMaxCams) + " cameras");
    require_device();
    hipStream_t st = nullptr;
    XM_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    double *dq = nullptr;
    try {
        xm::SchurSettings sc;
        sc.solver = 1;
        xm::SchurOp op(n, m, nobs, cam, lm, p, w, st, nullptr, sc);
        if (op.names_a_pair_twice()) throw xm::Error(XM_ERR_ARG, "xm_create_matrix: the observation list names a (camera, landmark) pair twice");
        const int64_t ld = xm_dense_ld(n);
        XM_HIP_CHECK(hipMalloc((void **)&dq, (size_t)3 * n * (size_t)ld * sizeof(double)));
        XM_HIP_CHECK(hipMemsetAsync(dq, 0, (size_t)3 * n * (size_t)ld * sizeof(double), st));
        op.build_dense_q(dq, ld, Abar, st);
        XM_HIP_CHECK(hipMemcpy2DAsync(Q, (size_t)ldq * sizeof(double), dq, (size_t)ld * sizeof(double), (size_t)3 * n * sizeof(double), (size_t)3 * n,
                                      hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipStreamSynchronize(st));
    } catch (...) {
        if (dq) (void)hipFree(dq);
        (void)hipStreamDestroy(st);
        throw;
    }
    (void)hipFree(dq);
    (void)hipStreamDestroy(st);
    return XM_OK;
    XM_CATCH
}
int xm_schur_dense_limits(int64_t out[3]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_schur_dense_limits: null output");
    out[0] = xm::kSchurDenseQWinCams; out[1] = xm::kSchurAbarPanel; out[2] = xm::kSchurDenseQMaxCams;
    return XM_OK;
    XM_CATCH
}
int xm_ctx_tcg_two_launch(xm_ctx_t *ctx, int *count) {
    XM_TRY
    if (!ctx || !ctx->impl || !count) throw xm::Error(XM_ERR_ARG, "xm_ctx_tcg_two_launch: single-GPU context and a non-null output needed");
    *count = ctx->impl->tcg_two_launch_count();
    return XM_OK;
    XM_CATCH
}
int xm_ctx_tcg_replay(xm_ctx_t *ctx, int64_t out[2]) {
    XM_TRY
    if (!ctx || !ctx->impl || !out) throw xm::Error(XM_ERR_ARG, "xm_ctx_tcg_replay: single-GPU context and a non-null output needed");
    ctx->impl->tcg_replay_counts(out);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_set_tcg_history(xm_ctx_t *ctx, int32_t iterations) {
    XM_TRY
    if (!ctx || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_set_tcg_history: single-GPU context needed");
    ctx->impl->set_tcg_history(iterations);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_schur_info(xm_ctx_t *ctx, int *uses_cg, int64_t stats[3], double *last_relres) {
    XM_TRY
    if (!ctx || !ctx->impl || !uses_cg) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_info: single-GPU context and a non-null output needed");
    int64_t st[3] = {0, 0, 0};
    double rr = 0.0;
    *uses_cg = ctx->impl->schur_info(st, &rr) ? 1 : 0;
    if (stats) { stats[0] = st[0]; stats[1] = st[1]; stats[2] = st[2]; }
    if (last_relres) *last_relres = rr;
    return XM_OK;
    XM_CATCH
}
int xm_ctx_schur_precond_info(xm_ctx_t *ctx, int *kind, int64_t *aggregates, int *block) {
    XM_TRY
    if (!ctx || !ctx->impl || !kind) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_precond_info: single-GPU context and a non-null output needed");
    int64_t na = 0;
    int b = 0;
    *kind = ctx->impl->schur_precond(&na, &b);
    if (aggregates) *aggregates = na;
    if (block) *block = b;
    return XM_OK;
    XM_CATCH
}
// xm_ctx_bundle_adjust (with_focal = false: XM_BA_REFINE_FOCAL is an unknown flag) and xm_ctx_bundle_adjust_focal (it is required)
// (groups: xm_ctx_bundle_adjust_focal_groups -- focal and focal_free have ngroups entries, group_of names every camera's group)
static void check_focal_groups(const std::string &w, int64_t n, int64_t ngroups, const int32_t *group_of) {
    if (!group_of) throw xm::Error(XM_ERR_ARG, w + ": group_of is null");
    if (ngroups < 1 || ngroups > n) throw xm::Error(XM_ERR_ARG, w + ": ngroups must lie in [1, n]");
    for (int64_t i = 0; i < n; ++i)
        if (group_of[i] < 0 || group_of[i] >= ngroups) throw xm::Error(XM_ERR_ARG, w + ": group_of[" + std::to_string(i) + "] is out of range");
}
static void ba_entry(xm_ctx_t *ctx, const xm_ba_options_t *opt, double *rot, double *t, double *p, bool with_focal, double *focal,
                     const uint8_t *focal_free, xm_ba_result_t *res, bool groups = false, int64_t ngroups = 0, const int32_t *group_of = nullptr,
                     bool with_dist = false, double *dist = nullptr, const uint8_t *dist_free = nullptr) {
    if (!ctx || !opt || !res || !rot || !t || !p || (with_focal && !focal) || (with_dist && !dist))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: null argument");
    static_assert(offsetof(xm_ba_options_t, loss) == XM_BA_OPTIONS_SIZE_V1, "the first version of xm_ba_options_t ends at trace");
    if (opt->struct_size != sizeof(xm_ba_options_t) && opt->struct_size != XM_BA_OPTIONS_SIZE_V1)
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: xm_ba_options_t.struct_size is neither sizeof(xm_ba_options_t) nor XM_BA_OPTIONS_SIZE_V1");
    if (res->struct_size != sizeof(xm_ba_result_t)) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: xm_ba_result_t.struct_size is not sizeof(xm_ba_result_t)");
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: single-rank contexts only");
    xm_ba_options_t o;   // a caller of the first version: the fields it does not have are 0 (trivial loss, monotonic steps)
    std::memset(&o, 0, sizeof(o));
    std::memcpy(&o, opt, opt->struct_size);
    auto bad = [](double v) { return !(v >= 0.0) || !std::isfinite(v); };
    if (!(o.eta > 0.0 && o.eta < 1.0)) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: eta must lie in (0, 1)");
    if (o.max_iters < 0 || bad(o.max_time) || bad(o.function_tol) || bad(o.gradient_tol) || bad(o.parameter_tol))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: negative or non-finite setting");
    if (o.flags & ~(XM_BA_FIX_ROTATIONS | XM_BA_NONMONOTONIC | XM_BA_DENSE_SCHUR | XM_BA_PRECOND_TWO_LEVEL | XM_BA_PRECOND_BLOCKS |
                    (with_focal ? XM_BA_REFINE_FOCAL : 0u) | (with_dist ? XM_BA_REFINE_RADIAL : 0u)))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: unknown flag");
    if (with_focal && !(o.flags & XM_BA_REFINE_FOCAL)) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust_focal: XM_BA_REFINE_FOCAL is not set");
    if (with_dist && !(o.flags & XM_BA_REFINE_RADIAL)) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust_radial: XM_BA_REFINE_RADIAL is not set");
    if (with_focal && (o.flags & (XM_BA_PRECOND_TWO_LEVEL | XM_BA_PRECOND_BLOCKS)))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust_focal: the aggregate preconditioners have no focal column (use the default preconditioner)");
    if ((o.flags & XM_BA_PRECOND_TWO_LEVEL) && (o.flags & XM_BA_PRECOND_BLOCKS))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: XM_BA_PRECOND_TWO_LEVEL and XM_BA_PRECOND_BLOCKS exclude each other");
    if ((o.flags & XM_BA_DENSE_SCHUR) && (o.flags & (XM_BA_PRECOND_TWO_LEVEL | XM_BA_PRECOND_BLOCKS)))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: a PCG preconditioner is given but XM_BA_DENSE_SCHUR does not run the PCG");
    if (o.loss < XM_BA_LOSS_TRIVIAL || o.loss > XM_BA_LOSS_ARCTAN) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: unknown loss");
    if (o.loss == XM_BA_LOSS_TRIVIAL && o.loss_scale != 0.0)
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: loss_scale is given but the loss is trivial");
    if (o.loss != XM_BA_LOSS_TRIVIAL && !(std::isfinite(o.loss_scale) && o.loss_scale > 0.0))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: a robust loss needs a finite loss_scale > 0");
    if (o.max_nonmonotonic < 0) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: max_nonmonotonic is negative");
    if (o.trace_cap < 0 || (o.trace_cap > 0 && !o.trace)) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: trace_cap > 0 needs a trace array");
    const int64_t n = ctx->impl->cameras(), m = ctx->impl->n_landmarks();
    if (groups) {
        check_focal_groups("xm_ctx_bundle_adjust_focal_groups", n, ngroups, group_of);
    }
    if ((o.flags & XM_BA_DENSE_SCHUR) && (((o.flags & XM_BA_FIX_ROTATIONS) ? 3 : 6) + (with_focal ? 1 : 0) + (with_dist ? 1 : 0)) * n > XM_BA_DENSE_MAX_ROWS)
        throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: XM_BA_DENSE_SCHUR with more than XM_BA_DENSE_MAX_ROWS rows in the reduced camera system");
    for (int64_t k = 0; k < 9 * n; ++k)
        if (!std::isfinite(rot[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: rotations are not finite");
    for (int64_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(t[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: translations are not finite");
    for (int64_t k = 0; k < 3 * m; ++k)
        if (!std::isfinite(p[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: landmarks are not finite");
    if (with_focal)
        for (int64_t k = 0; k < (groups ? ngroups : n); ++k)
            if (!std::isfinite(focal[k]) || !(focal[k] > 0.0)) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust_focal: a focal scale is not finite and > 0");
    if (with_dist)
        for (int64_t k = 0; k < n; ++k)
            if (!std::isfinite(dist[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_bundle_adjust_radial: a radial coefficient is not finite");
    xm::BaSettings c;
    c.refine_focal = with_focal; c.focal = focal; c.focal_free = focal_free;
    c.refine_dist = with_dist; c.dist = dist; c.dist_free = dist_free;
    if (groups) { c.ngroups = ngroups; c.group_of = group_of; }
    if (o.max_iters > 0) c.max_iters = o.max_iters;
    if (o.max_time > 0.0) c.max_time = o.max_time;
    if (o.function_tol > 0.0) c.function_tol = o.function_tol;
    if (o.gradient_tol > 0.0) c.gradient_tol = o.gradient_tol;
    if (o.parameter_tol > 0.0) c.parameter_tol = o.parameter_tol;
    c.eta = o.eta;
    c.fix_rotations = (o.flags & XM_BA_FIX_ROTATIONS) != 0;
    c.loss = o.loss; c.loss_scale = o.loss_scale;
    c.nonmonotonic = (o.flags & XM_BA_NONMONOTONIC) != 0;
    c.dense_schur = (o.flags & XM_BA_DENSE_SCHUR) != 0;
    c.precond = (o.flags & XM_BA_PRECOND_TWO_LEVEL) ? 2 : (o.flags & XM_BA_PRECOND_BLOCKS) ? 1 : 0;
    if (o.max_nonmonotonic > 0) c.max_nonmonotonic = o.max_nonmonotonic;
    c.trace_cap = o.trace_cap; c.trace = o.trace;
    xm::BaOutcome r;
    ctx->impl->bundle_adjust(c, rot, t, p, r);
    xm_ba_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_ba_result_t);
    out.status = r.status; out.iters = r.iters; out.accepted = r.accepted; out.pcg_iters = r.pcg_iters; out.n_used = r.n_used;
    out.initial_cost = r.initial_cost; out.final_cost = r.final_cost; out.gradient_max = r.gradient_max; out.seconds = r.seconds;
    out.trace_len = r.trace_len; out.coarse_fallbacks = r.coarse_fallbacks;
    *res = out;
}
int xm_ctx_bundle_adjust(xm_ctx_t *ctx, const xm_ba_options_t *opt, double *rot, double *t, double *p, xm_ba_result_t *res) {
    XM_TRY
    ba_entry(ctx, opt, rot, t, p, false, nullptr, nullptr, res);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_bundle_adjust_focal(xm_ctx_t *ctx, const xm_ba_options_t *opt, double *rot, double *t, double *p, double *focal, const uint8_t *focal_free,
                               xm_ba_result_t *res) {
    XM_TRY
    ba_entry(ctx, opt, rot, t, p, true, focal, focal_free, res);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_bundle_adjust_focal_groups(xm_ctx_t *ctx, const xm_ba_options_t *opt, double *rot, double *t, double *p, int64_t ngroups,
                                      const int32_t *group_of, double *focal, const uint8_t *focal_free, xm_ba_result_t *res) {
    XM_TRY
    ba_entry(ctx, opt, rot, t, p, true, focal, focal_free, res, true, ngroups, group_of);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_bundle_adjust_radial(xm_ctx_t *ctx, const xm_ba_options_t *opt, double *rot, double *t, double *p, double *focal, const uint8_t *focal_free,
                                double *dist, const uint8_t *dist_free, xm_ba_result_t *res) {
    XM_TRY
    ba_entry(ctx, opt, rot, t, p, true, focal, focal_free, res, false, 0, nullptr, true, dist, dist_free);
    return XM_OK;
    XM_CATCH
}
static void sqerr_entry(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, bool with_focal, const double *focal, double *sqerr,
                        bool with_dist = false, const double *dist = nullptr) {
    if (!ctx || !rot || !t || !p || !sqerr || (with_focal && !focal) || (with_dist && !dist)) throw xm::Error(XM_ERR_ARG, "xm_ctx_reprojection_errors: null argument");
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_reprojection_errors: single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1) throw xm::Error(XM_ERR_ARG, "xm_ctx_reprojection_errors: single-rank contexts only");
    const int64_t n = ctx->impl->cameras(), m = ctx->impl->n_landmarks();
    for (int64_t k = 0; k < 9 * n; ++k)
        if (!std::isfinite(rot[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_reprojection_errors: rotations are not finite");
    for (int64_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(t[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_reprojection_errors: translations are not finite");
    for (int64_t k = 0; k < 3 * m; ++k)
        if (!std::isfinite(p[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_reprojection_errors: landmarks are not finite");
    if (with_focal)
        for (int64_t k = 0; k < n; ++k)
            if (!std::isfinite(focal[k]) || !(focal[k] > 0.0)) throw xm::Error(XM_ERR_ARG, "xm_ctx_reprojection_errors_focal: a focal scale is not finite and > 0");
    if (with_dist)
        for (int64_t k = 0; k < n; ++k)
            if (!std::isfinite(dist[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_reprojection_errors_radial: a radial coefficient is not finite");
    ctx->impl->reprojection_errors(rot, t, p, sqerr, with_focal ? focal : nullptr, with_dist ? dist : nullptr);
}
int xm_ctx_reprojection_errors_radial(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, const double *focal, const double *dist,
                                      double *sqerr) {
    XM_TRY
    sqerr_entry(ctx, rot, t, p, true, focal, sqerr, true, dist);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_reprojection_errors(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, double *sqerr) {
    XM_TRY
    sqerr_entry(ctx, rot, t, p, false, nullptr, sqerr);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_reprojection_errors_focal(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, const double *focal, double *sqerr) {
    XM_TRY
    sqerr_entry(ctx, rot, t, p, true, focal, sqerr);
    return XM_OK;
    XM_CATCH
}
static void probe_entry(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, bool with_focal, const double *focal,
                        const uint8_t *focal_free, xm_ba_probe_t *pr, double *focal1, bool groups = false, int64_t ngroups = 0,
                        const int32_t *group_of = nullptr, bool with_dist = false, const double *dist = nullptr, const uint8_t *dist_free = nullptr,
                        double *dist1 = nullptr) {
    if (!ctx || !rot || !t || !p || !pr || (with_focal && !focal) || (with_dist && !dist)) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: null argument");
    if (pr->struct_size != sizeof(xm_ba_probe_t)) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: xm_ba_probe_t.struct_size is not sizeof(xm_ba_probe_t)");
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: single-rank contexts only");
    if (!(pr->mu > 0.0) || !std::isfinite(pr->mu)) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: mu must be finite and > 0");
    if (pr->flags & ~(XM_BA_FIX_ROTATIONS | XM_BA_PRECOND_TWO_LEVEL | XM_BA_PRECOND_BLOCKS | (with_focal ? XM_BA_REFINE_FOCAL : 0u) |
                      (with_dist ? XM_BA_REFINE_RADIAL : 0u)))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: unknown flag");
    if (with_dist && !(pr->flags & XM_BA_REFINE_RADIAL)) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe_radial: XM_BA_REFINE_RADIAL is not set");
    if (with_focal && !(pr->flags & XM_BA_REFINE_FOCAL)) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe_focal: XM_BA_REFINE_FOCAL is not set");
    if (with_focal && (pr->flags & (XM_BA_PRECOND_TWO_LEVEL | XM_BA_PRECOND_BLOCKS)))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe_focal: the aggregate preconditioners have no focal column");
    if ((pr->flags & XM_BA_PRECOND_TWO_LEVEL) && (pr->flags & XM_BA_PRECOND_BLOCKS))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: XM_BA_PRECOND_TWO_LEVEL and XM_BA_PRECOND_BLOCKS exclude each other");
    if (pr->loss < XM_BA_LOSS_TRIVIAL || pr->loss > XM_BA_LOSS_ARCTAN) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: unknown loss");
    if (pr->loss == XM_BA_LOSS_TRIVIAL && pr->loss_scale != 0.0) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: loss_scale is given but the loss is trivial");
    if (pr->loss != XM_BA_LOSS_TRIVIAL && !(std::isfinite(pr->loss_scale) && pr->loss_scale > 0.0))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: a robust loss needs a finite loss_scale > 0");
    if (pr->k < 0 || (pr->k > 0 && !pr->X)) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: k > 0 needs X");
    const int64_t n = ctx->impl->cameras(), m = ctx->impl->n_landmarks(), cd = ((pr->flags & XM_BA_FIX_ROTATIONS) ? 3 : 6) + (with_focal ? 1 : 0) + (with_dist ? 1 : 0);
    if (pr->Sdense && cd * n > XM_BA_PROBE_DENSE_MAX_ROWS) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: Sdense with more than XM_BA_PROBE_DENSE_MAX_ROWS rows");
    if (groups) {
        check_focal_groups("xm_ctx_ba_probe_focal_groups", n, ngroups, group_of);
    }
    const int64_t nvec = groups ? (cd - 1) * n + ngroups : cd * n;   // entries of b, a column of X, dc
    for (int64_t k = 0; k < 9 * n; ++k)
        if (!std::isfinite(rot[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: rotations are not finite");
    for (int64_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(t[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: translations are not finite");
    for (int64_t k = 0; k < 3 * m; ++k)
        if (!std::isfinite(p[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: landmarks are not finite");
    for (int64_t k = 0; k < nvec * pr->k; ++k)
        if (!std::isfinite(pr->X[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: X is not finite");
    if (pr->dc)
        for (int64_t k = 0; k < nvec; ++k)
            if (!std::isfinite(pr->dc[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe: dc is not finite");
    if (with_focal)
        for (int64_t k = 0; k < (groups ? ngroups : n); ++k)
            if (!std::isfinite(focal[k]) || !(focal[k] > 0.0)) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe_focal: a focal scale is not finite and > 0");
    if (with_dist)
        for (int64_t k = 0; k < n; ++k)
            if (!std::isfinite(dist[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_ba_probe_radial: a radial coefficient is not finite");
    xm::BaSettings c;
    c.refine_focal = with_focal; c.focal = const_cast<double *>(focal); c.focal_free = focal_free;   // the probe only reads them
    c.refine_dist = with_dist; c.dist = const_cast<double *>(dist); c.dist_free = dist_free;
    if (groups) { c.ngroups = ngroups; c.group_of = group_of; }
    c.fix_rotations = (pr->flags & XM_BA_FIX_ROTATIONS) != 0;
    c.loss = pr->loss; c.loss_scale = pr->loss_scale;
    c.precond = (pr->flags & XM_BA_PRECOND_TWO_LEVEL) ? 2 : (pr->flags & XM_BA_PRECOND_BLOCKS) ? 1 : 0;
    xm::BaProbe q;
    q.mu = pr->mu; q.k = pr->k; q.X = pr->X; q.dc = pr->dc;
    q.b = pr->b; q.g_l = pr->g_l; q.vinv = pr->vinv; q.ustar = pr->ustar; q.sinv = pr->sinv; q.cused = pr->cused; q.lused = pr->lused;
    q.SX = pr->SX; q.Sdense = pr->Sdense; q.MX = pr->MX; q.Pm = pr->Pm; q.dropped = pr->dropped; q.Ac = pr->Ac;
    q.dP = pr->dP; q.rot1 = pr->rot1; q.t1 = pr->t1; q.p1 = pr->p1; q.focal1 = with_focal ? focal1 : nullptr;
    q.dist1 = with_dist ? dist1 : nullptr;
    if (groups) { q.group_D = pr->dropped; q.group_F = pr->Ac; q.Pm = q.dropped = q.Ac = nullptr; }   // no aggregates here: their pointers serve the groups
    ctx->impl->ba_probe(c, rot, t, p, q);
    pr->cost = q.cost; pr->gmax = q.gmax; pr->cost1 = q.cost1; pr->model = q.model; pr->n_used = q.n_used;
    pr->step2[0] = q.step2[0]; pr->step2[1] = q.step2[1]; pr->x2[0] = q.x2[0]; pr->x2[1] = q.x2[1];
    pr->nagg = q.nagg; pr->ncoarse = q.ncoarse; pr->coarse_ok = q.coarse_ok;   // (focal groups: coarse_ok = the exact focal block was inverted)
}
int xm_ctx_ba_probe(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, xm_ba_probe_t *pr) {
    XM_TRY
    probe_entry(ctx, rot, t, p, false, nullptr, nullptr, pr, nullptr);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_ba_probe_focal(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, const double *focal, const uint8_t *focal_free,
                          xm_ba_probe_t *pr, double *focal1) {
    XM_TRY
    probe_entry(ctx, rot, t, p, true, focal, focal_free, pr, focal1);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_ba_probe_radial(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, const double *focal, const uint8_t *focal_free,
                           const double *dist, const uint8_t *dist_free, xm_ba_probe_t *pr, double *focal1, double *dist1) {
    XM_TRY
    probe_entry(ctx, rot, t, p, true, focal, focal_free, pr, focal1, false, 0, nullptr, true, dist, dist_free, dist1);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_ba_probe_focal_groups(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, int64_t ngroups, const int32_t *group_of,
                                 const double *focal, const uint8_t *focal_free, xm_ba_probe_t *pr, double *focal1) {
    XM_TRY
    probe_entry(ctx, rot, t, p, true, focal, focal_free, pr, focal1, true, ngroups, group_of);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_global_positioning(xm_ctx_t *ctx, const xm_gp_options_t *opt, const double *rot, double *t, double *p, double *scales, xm_gp_result_t *res) {
    XM_TRY
    const xm::GpSettings c = gp_settings("xm_ctx_global_positioning", ctx, opt, res, rot, t, p);
    xm::GpOutcome r;
    ctx->impl->global_positioning(c, rot, t, p, scales, r);
    gp_result_out(r, res);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_global_positioning_pairs(xm_ctx_t *ctx, const xm_gp_options_t *opt, xm_gp_pairs_t *pairs, const double *rot, double *t, double *p,
                                    double *scales, xm_gp_result_t *res) {
    XM_TRY
    if (!pairs) throw xm::Error(XM_ERR_ARG, "xm_ctx_global_positioning_pairs: null argument");
    const xm::GpSettings c = gp_settings("xm_ctx_global_positioning_pairs", ctx, opt, res, rot, t, p);
    xm::GpPairsIn in = gp_pairs_in("xm_ctx_global_positioning_pairs", ctx, pairs);
    xm::GpOutcome r;
    ctx->impl->global_positioning_pairs(c, in, rot, t, p, scales, r);
    gp_result_out(r, res);
    gp_pairs_out(in, pairs);
    return XM_OK;
    XM_CATCH
}
static void gp_probe_entry(const char *who, xm_ctx_t *ctx, const double *rot, const double *t, const double *p, xm_gp_probe_t *pr, xm_gp_pairs_t *pairs,
                           xm_gp_pair_probe_t *pp) {
    const std::string w(who);
    if (!ctx || !rot || !t || !p || !pr) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (pr->struct_size != sizeof(xm_gp_probe_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_gp_probe_t.struct_size is not sizeof(xm_gp_probe_t)");
    if (!(pr->mu > 0.0) || !std::isfinite(pr->mu)) throw xm::Error(XM_ERR_ARG, w + ": mu must be finite and > 0");
    if (pr->k < 0 || (pr->k > 0 && !pr->X)) throw xm::Error(XM_ERR_ARG, w + ": k > 0 needs X");
    gp_check(who, ctx, pr->loss, pr->loss_scale, pr->min_views, rot, t, p);
    const int64_t n = ctx->impl->cameras(), nobs = ctx->impl->n_observations();
    if (pr->s)
        for (int64_t k = 0; k < nobs; ++k)
            if (!std::isfinite(pr->s[k])) throw xm::Error(XM_ERR_ARG, w + ": s is not finite");
    for (int64_t k = 0; k < 3 * n * pr->k; ++k)
        if (!std::isfinite(pr->X[k])) throw xm::Error(XM_ERR_ARG, w + ": X is not finite");
    if (pr->dc)
        for (int64_t k = 0; k < 3 * n; ++k)
            if (!std::isfinite(pr->dc[k])) throw xm::Error(XM_ERR_ARG, w + ": dc is not finite");
    xm::GpSettings c;
    if (pr->min_views > 0) c.min_views = pr->min_views;
    c.loss = pr->loss; c.loss_scale = pr->loss_scale;
    xm::GpProbe q;
    q.mu = pr->mu; q.k = pr->k; q.s = pr->s; q.X = pr->X; q.dc = pr->dc;
    q.M = pr->M; q.q = pr->q; q.frozen = pr->frozen; q.oused = pr->oused;
    q.vinv = pr->vinv; q.g_l = pr->g_l; q.ustar = pr->ustar; q.sinv = pr->sinv; q.b = pr->b; q.cused = pr->cused; q.lused = pr->lused;
    q.SX = pr->SX; q.dP = pr->dP; q.ds = pr->ds; q.t1 = pr->t1; q.p1 = pr->p1; q.s1 = pr->s1;
    if (pairs) {
        if (!pp) throw xm::Error(XM_ERR_ARG, w + ": null argument");
        if (pp->struct_size != sizeof(xm_gp_pair_probe_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_gp_pair_probe_t.struct_size is not sizeof(xm_gp_pair_probe_t)");
        xm::GpPairsIn in = gp_pairs_in(who, ctx, pairs);
        if (in.fix_centres && pr->k > 0) throw xm::Error(XM_ERR_ARG, w + ": fixed centres have no reduced camera system (k must be 0)");
        if (pp->sigma_in)
            for (int64_t k = 0; k < in.npairs; ++k)
                if (!std::isfinite(pp->sigma_in[k])) throw xm::Error(XM_ERR_ARG, w + ": sigma_in is not finite");
        xm::GpPairProbe pq;
        pq.sigma_in = pp->sigma_in; pq.Mp = pp->Mp; pq.qp = pp->qp; pq.pfrozen = pp->pfrozen; pq.pused = pp->pused; pq.dsigma = pp->dsigma;
        pq.sigma1 = pp->sigma1;
        ctx->impl->gp_probe_pairs(c, in, rot, t, p, q, pq);
        pp->cost = pq.cost; pp->gsmax = pq.gsmax; pp->cost1 = pq.cost1; pp->model = pq.model; pp->step2 = pq.step2; pp->x2 = pq.x2;
        gp_pairs_out(in, pairs);
    } else {
        ctx->impl->gp_probe(c, rot, t, p, q);
    }
    pr->cost = q.cost; pr->gmax = q.gmax; pr->cost1 = q.cost1; pr->model = q.model; pr->n_used = q.n_used;
    for (int k = 0; k < 3; ++k) { pr->step2[k] = q.step2[k]; pr->x2[k] = q.x2[k]; }
}
int xm_ctx_gp_probe(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, xm_gp_probe_t *pr) {
    XM_TRY
    gp_probe_entry("xm_ctx_gp_probe", ctx, rot, t, p, pr, nullptr, nullptr);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_gp_probe_pairs(xm_ctx_t *ctx, const double *rot, const double *t, const double *p, xm_gp_probe_t *pr, xm_gp_pairs_t *pairs,
                          xm_gp_pair_probe_t *pp) {
    XM_TRY
    if (!pairs) throw xm::Error(XM_ERR_ARG, "xm_ctx_gp_probe_pairs: null argument");
    gp_probe_entry("xm_ctx_gp_probe_pairs", ctx, rot, t, p, pr, pairs, pp);
    return XM_OK;
    XM_CATCH
}
int xm_gp_limits(int64_t out[3]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_gp_limits: null output");
    xm::gp_limits(out);
    return XM_OK;
    XM_CATCH
}
int xm_gp_pair_limits(int64_t out[2]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_gp_pair_limits: null output");
    xm::gp_pair_limits(out);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_schur_probe(xm_ctx_t *ctx, xm_schur_probe_t *pr) {
    XM_TRY
    if (!ctx || !pr) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: null argument");
    if (pr->struct_size != sizeof(xm_schur_probe_t)) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: xm_schur_probe_t.struct_size is not sizeof(xm_schur_probe_t)");
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1 || ctx->impl->comm_kind() != 0) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: single-rank contexts only");
    if (pr->flags != 0) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: unknown flag");
    auto cols = [](int v) { return v == 0 || v == 1 || (v >= 3 && v <= 10); };
    if (!cols(pr->o) || !cols(pr->k)) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: o and k must be 0, 1 or 3..10");
    if ((pr->o > 0) != (pr->W != nullptr)) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: o > 0 and W go together");
    if ((pr->k > 0) != (pr->X != nullptr)) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: k > 0 and X go together");
    if (pr->o == 0 && (pr->h || pr->r || pr->xc || pr->xl || pr->Y)) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: the chain stages need W");
    if (pr->k == 0 && (pr->VX || pr->pAp || pr->MX)) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: VX, pAp and MX need X");
    const int64_t n = ctx->impl->cameras();
    if (pr->o > 0 && !std::isfinite(pr->alpha)) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: alpha is not finite");
    for (int64_t k = 0; k < 3 * n * pr->o; ++k)
        if (!std::isfinite(pr->W[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: W is not finite");
    for (int64_t k = 0; k < (n - 1) * pr->k; ++k)
        if (!std::isfinite(pr->X[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_schur_probe: X is not finite");
    ctx->impl->schur_probe(*pr);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_rtr_probe(xm_ctx_t *ctx, xm_rtr_probe_t *pr) {
    XM_TRY
    if (!ctx || !pr) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: null argument");
    if (pr->struct_size != sizeof(xm_rtr_probe_t)) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: xm_rtr_probe_t.struct_size is not sizeof(xm_rtr_probe_t)");
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1 || ctx->impl->comm_kind() != 0) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: single-rank contexts only");
    if (pr->o < 3 || pr->o > 10) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: rank o must be in 3..10");
    if (pr->flags & ~(XM_RTR_PROBE_AUTO | XM_RTR_PROBE_MODEL_REC | XM_RTR_PROBE_TCG_INIT | XM_RTR_PROBE_CG_STEP | XM_RTR_PROBE_CERT))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: unknown flag");
    if (!pr->R || !pr->s) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: the point (R, s) is missing");
    if ((pr->pR == nullptr) != (pr->ps == nullptr)) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: pR and ps go together");
    if (pr->k < 0 || (pr->k > 0 && !pr->X)) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: k > 0 needs X");
    const int64_t n = ctx->impl->cameras(), mat = 3 * n * pr->o;
    auto finite = [](const double *x, int64_t len, const char *what) {
        if (!x) return;
        for (int64_t k = 0; k < len; ++k)
            if (!std::isfinite(x[k])) throw xm::Error(XM_ERR_ARG, std::string("xm_ctx_rtr_probe: ") + what + " is not finite");
    };
    if (!std::isfinite(pr->lam)) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: lam is not finite");
    finite(pr->R, mat, "R"); finite(pr->s, n, "s"); finite(pr->pR, mat, "pR"); finite(pr->ps, n, "ps"); finite(pr->rR, mat, "rR"); finite(pr->rs, n, "rs");
    finite(pr->X, 3 * n * pr->k, "X");
    if (pr->flags & XM_RTR_PROBE_CG_STEP) {
        finite(pr->vR, mat, "vR"); finite(pr->vs, n, "vs");
        if (!(pr->flags & XM_RTR_PROBE_MODEL_REC)) { finite(pr->HvR, mat, "HvR"); finite(pr->Hvs, n, "Hvs"); }
        if (pr->scal_in.iter > 0) finite(pr->partsB_in, pr->partsB_in_count, "partsB_in");
        const xm_rtr_scal_t &sc = pr->scal_in;
        const double v[7] = {sc.rr, sc.vv, sc.vp, sc.pp, sc.delta, sc.gradnorm, sc.model};
        finite(v, 7, "scal_in");
        if (sc.iter < 0 || sc.iter >= 1000) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: scal_in.iter must be in 0..999");
    }
    if ((pr->flags & XM_RTR_PROBE_TCG_INIT) && !std::isfinite(pr->scal_in.delta)) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: scal_in.delta is not finite");
    for (int64_t i = 0; i < n; ++i)
        if (!(pr->s[i] > 0.0)) throw xm::Error(XM_ERR_ARG, "xm_ctx_rtr_probe: scales must be positive");
    ctx->impl->rtr_probe(*pr);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_outer_probe(xm_ctx_t *ctx, xm_outer_probe_t *pr) {
    XM_TRY
    if (!ctx || !pr) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: null argument");
    if (pr->struct_size != sizeof(xm_outer_probe_t)) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: xm_outer_probe_t.struct_size is not sizeof(xm_outer_probe_t)");
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1 || ctx->impl->comm_kind() != 0) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: single-rank contexts only");
    if (pr->o < 3 || pr->o > 10) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: rank o must be in 3..10");
    const uint32_t known = XM_OUTER_PROBE_RETRACT | XM_OUTER_PROBE_MODEL_REC | XM_OUTER_PROBE_RETRACT_LS | XM_OUTER_PROBE_STEP | XM_OUTER_PROBE_POLAR |
                           XM_OUTER_PROBE_MGS | XM_OUTER_PROBE_AUTO;
    if (pr->flags & ~known) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: unknown flag");
    if ((pr->flags & XM_OUTER_PROBE_POLAR) && (pr->flags & XM_OUTER_PROBE_MGS)) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: one retraction at a time");
    if (!pr->R || !pr->s) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: the point (R, s) is missing");
    const bool ret = pr->flags & XM_OUTER_PROBE_RETRACT, ls = pr->flags & XM_OUTER_PROBE_RETRACT_LS, step = pr->flags & XM_OUTER_PROBE_STEP;
    const bool rec = pr->flags & XM_OUTER_PROBE_MODEL_REC;
    if ((ret || step) && !(pr->vR && pr->vs && (rec || (pr->HvR && pr->Hvs))))
        throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: the retraction and the step launch need v (and Hv unless XM_OUTER_PROBE_MODEL_REC)");
    if (ls && !pr->D) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: XM_OUTER_PROBE_RETRACT_LS needs D");
    if (step && !(pr->pR && pr->ps && pr->rR && pr->rs)) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: XM_OUTER_PROBE_STEP needs p and r");
    if ((pr->Rc == nullptr) != (pr->sc == nullptr)) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: Rc and sc go together");
    const int64_t n = ctx->impl->cameras(), mat = 3 * n * pr->o;
    auto finite = [](const double *x, int64_t len, const char *what) {
        if (!x) return;
        for (int64_t k = 0; k < len; ++k)
            if (!std::isfinite(x[k])) throw xm::Error(XM_ERR_ARG, std::string("xm_ctx_outer_probe: ") + what + " is not finite");
    };
    const double sv[2] = {pr->lam, pr->t};
    finite(sv, 2, "lam or t");
    finite(pr->R, mat, "R"); finite(pr->s, n, "s"); finite(pr->vR, mat, "vR"); finite(pr->vs, n, "vs"); finite(pr->HvR, mat, "HvR"); finite(pr->Hvs, n, "Hvs");
    finite(pr->D, mat, "D"); finite(pr->pR, mat, "pR"); finite(pr->ps, n, "ps"); finite(pr->rR, mat, "rR"); finite(pr->rs, n, "rs");
    finite(pr->Rc, mat, "Rc"); finite(pr->sc, n, "sc");
    if (pr->partsB_in_count < 0 || pr->partsM_in_count < 0) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: a negative count");
    finite(pr->partsB_in, pr->partsB_in_count, "partsB_in"); finite(pr->partsM_in, pr->partsM_in_count, "partsM_in");
    if (ret || step) {
        const xm_outer_tcg_t &sc = pr->scal_in;
        const double v[8] = {sc.rr, sc.vv, sc.vp, sc.pp, sc.delta, sc.gradnorm, sc.last_step, sc.model};
        finite(v, 8, "scal_in");
    }
    if (step) {
        const xm_outer_tcg_t &sc = pr->scal_in;
        if (sc.iter < 0 || sc.iter >= 1000) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: scal_in.iter must be in 0..999");
        if (sc.phase < 0 || sc.phase > 3) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: scal_in.phase must be 0 (tCG), 1 (candidate), 2 (stop) or 3 (init)");
        if (pr->slot < 0) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: slot must not be negative");
        const double w[4] = {pr->os_in.loss, pr->os_in.rr_point, pr->delta_bar, pr->gradtol};
        finite(w, 4, "os_in, delta_bar or gradtol");
        if (pr->os_in.k < 0 || pr->os_in.k >= 1000 || pr->max_outer < 0) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: os_in.k must be in 0..999 and max_outer >= 0");
    }
    for (const double *sp : {pr->s, pr->sc})
        for (int64_t i = 0; sp && i < n; ++i)
            if (!(sp[i] > 0.0)) throw xm::Error(XM_ERR_ARG, "xm_ctx_outer_probe: scales must be positive");
    ctx->impl->outer_probe(*pr);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_cert_probe(xm_ctx_t *ctx, xm_cert_probe_t *pr) {
    XM_TRY
    if (!ctx || !pr) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: null argument");
    if (pr->struct_size != sizeof(xm_cert_probe_t)) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: xm_cert_probe_t.struct_size is not sizeof(xm_cert_probe_t)");
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1 || ctx->impl->comm_kind() != 0) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: single-rank contexts only");
    if (pr->o < 3 || pr->o > 10) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: rank o must be in 3..10");
    if (pr->flags & ~XM_CERT_PROBE_UNFUSED) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: unknown flag");
    if (!pr->R || !pr->s) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: the point (R, s) is missing");
    const int64_t n = ctx->impl->cameras();
    if (!std::isfinite(pr->lam)) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: lam is not finite");
    for (int64_t k = 0; k < 3 * n * pr->o; ++k)
        if (!std::isfinite(pr->R[k])) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: R is not finite");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(pr->s[i]) || !(pr->s[i] > 0.0)) throw xm::Error(XM_ERR_ARG, "xm_ctx_cert_probe: scales must be finite and positive");
    ctx->impl->cert_probe(*pr);
    return XM_OK;
    XM_CATCH
}
int xm_tridiag_min(const double *a, const double *b, int m, double *theta, double *y, double *tmax) {
    XM_TRY
    if (!a || !theta || !y || !tmax || m < 1 || (m > 1 && !b)) throw xm::Error(XM_ERR_ARG, "xm_tridiag_min: null argument or m < 1");
    xm::tridiag_min_export(a, b, m, theta, y, tmax);
    return XM_OK;
    XM_CATCH
}
namespace {
void clean_settings(const char *who, const xm_clean_options_t *opt, const uint8_t *keep, const int32_t *cam_index, const int32_t *lm_index,
                    const xm_clean_result_t *res, xm::CleanSettings &c) {
    const std::string w(who);
    if (!opt || !keep || !cam_index || !lm_index || !res) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_clean_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_clean_options_t.struct_size is not sizeof(xm_clean_options_t)");
    if (res->struct_size != sizeof(xm_clean_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_clean_result_t.struct_size is not sizeof(xm_clean_result_t)");
    if (opt->min_cam_obs < 0 || opt->min_lm_obs < 0) throw xm::Error(XM_ERR_ARG, w + ": negative threshold");
    if (opt->flags & ~XM_CLEAN_NO_SWAP) throw xm::Error(XM_ERR_ARG, w + ": unknown flag");
    c.min_cam_obs = opt->min_cam_obs; c.min_lm_obs = opt->min_lm_obs; c.swap_first = !(opt->flags & XM_CLEAN_NO_SWAP);
}
void give_clean(xm_clean_result_t *res, const xm::CleanOutcome &r) {
    xm_clean_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_clean_result_t);
    out.rounds = r.rounds; out.nobs_live = r.nobs_live; out.n_new = r.n_new; out.m_new = r.m_new; out.nobs_new = r.nobs_new;
    out.components = r.components; out.cams_weak = r.cams_weak; out.lms_weak = r.lms_weak; out.cams_emptied = r.cams_emptied;
    out.cams_off_component = r.cams_off_component; out.lms_off_component = r.lms_off_component; out.first_camera = r.first_camera;
    *res = out;
}
}  // namespace
int xm_clean_observations(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *w, const xm_clean_options_t *opt,
                          uint8_t *keep, int32_t *cam_index, int32_t *lm_index, xm_clean_result_t *res) {
    XM_TRY
    xm::CleanSettings c;
    clean_settings("xm_clean_observations", opt, keep, cam_index, lm_index, res, c);
    if (n < 0 || m < 0 || nobs < 0) throw xm::Error(XM_ERR_ARG, "xm_clean_observations: negative size");
    if (n + m >= ((int64_t)1 << 31)) throw xm::Error(XM_ERR_ARG, "xm_clean_observations: cameras + landmarks must stay below 2^31");
    if (nobs > 0 && (!cam || !lm)) throw xm::Error(XM_ERR_ARG, "xm_clean_observations: null observation arrays");
    require_device();
    if (const char *e = std::getenv("XM_WATCHDOG_S")) { const double v = std::atof(e); if (v > 0) c.watchdog_s = v; }
    xm::CleanOutcome r;
    xm::clean_observations_host(n, m, nobs, cam, lm, w, c, keep, cam_index, lm_index, r);
    give_clean(res, r);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_clean_observations(xm_ctx_t *ctx, const xm_clean_options_t *opt, uint8_t *keep, int32_t *cam_index, int32_t *lm_index, xm_clean_result_t *res) {
    XM_TRY
    if (!ctx) throw xm::Error(XM_ERR_ARG, "xm_ctx_clean_observations: null argument");
    xm::CleanSettings c;
    clean_settings("xm_ctx_clean_observations", opt, keep, cam_index, lm_index, res, c);
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_clean_observations: single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1) throw xm::Error(XM_ERR_ARG, "xm_ctx_clean_observations: single-rank contexts only");
    xm::CleanOutcome r;
    ctx->impl->clean_observations(c, keep, cam_index, lm_index, r);
    give_clean(res, r);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_filter_tracks(xm_ctx_t *ctx, const xm_tf_options_t *opt, const double *rot, const double *t, const double *p, uint8_t *keep, uint8_t *reason,
                         int32_t *lm_views, uint8_t *lm_status, xm_tf_result_t *res) {
    XM_TRY
    const std::string w("xm_ctx_filter_tracks");
    if (!ctx || !opt || !rot || !t || !p || !keep || !reason || !lm_views || !lm_status || !res) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_tf_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_tf_options_t.struct_size is not sizeof(xm_tf_options_t)");
    if (res->struct_size != sizeof(xm_tf_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_tf_result_t.struct_size is not sizeof(xm_tf_result_t)");
    if (opt->flags & ~(XM_TF_REPROJECTION | XM_TF_ANGLE | XM_TF_TRIANGULATION)) throw xm::Error(XM_ERR_ARG, w + ": unknown flag");
    if (opt->min_views < 0) throw xm::Error(XM_ERR_ARG, w + ": min_views is negative");
    // the threshold of a filter that is switched on must be usable (one that is off is not read)
    if ((opt->flags & XM_TF_REPROJECTION) && !(std::isfinite(opt->max_reprojection_error) && opt->max_reprojection_error > 0.0))
        throw xm::Error(XM_ERR_ARG, w + ": max_reprojection_error must be finite and positive");
    if ((opt->flags & XM_TF_ANGLE) && !(opt->max_angle_error > 0.0 && opt->max_angle_error <= 180.0))
        throw xm::Error(XM_ERR_ARG, w + ": max_angle_error must be positive and at most 180 degrees");
    if ((opt->flags & XM_TF_TRIANGULATION) && !(opt->min_triangulation_angle > 0.0 && opt->min_triangulation_angle <= 180.0))
        throw xm::Error(XM_ERR_ARG, w + ": min_triangulation_angle must be positive and at most 180 degrees");
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, w + ": single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1) throw xm::Error(XM_ERR_ARG, w + ": single-rank contexts only");
    const int64_t n = ctx->impl->cameras(), m = ctx->impl->n_landmarks();
    for (int64_t k = 0; k < 9 * n; ++k)
        if (!std::isfinite(rot[k])) throw xm::Error(XM_ERR_ARG, w + ": rotations are not finite");
    for (int64_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(t[k])) throw xm::Error(XM_ERR_ARG, w + ": translations are not finite");
    for (int64_t k = 0; k < 3 * m; ++k)
        if (!std::isfinite(p[k])) throw xm::Error(XM_ERR_ARG, w + ": landmarks are not finite");
    xm::TfSettings c;
    c.flags = opt->flags; c.min_views = opt->min_views; c.max_reprojection_error = opt->max_reprojection_error;
    // the cosines of the two angles, once, on the host (track_filter.cc:60, :97: cos(DegToRad(angle))); the kernels compare against these doubles
    constexpr double kPi = 3.14159265358979323846;
    c.cos_angle = (opt->flags & XM_TF_ANGLE) ? std::cos(opt->max_angle_error * (kPi / 180.0)) : 0.0;
    c.cos_triangulation = (opt->flags & XM_TF_TRIANGULATION) ? std::cos(opt->min_triangulation_angle * (kPi / 180.0)) : 0.0;
    xm::TfOutcome r;
    ctx->impl->filter_tracks(c, rot, t, p, keep, reason, lm_views, lm_status, r);
    xm_tf_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_tf_result_t);
    out.tracks_total = r.tracks_total; out.tracks_kept = r.tracks_kept; out.obs_used = r.obs_used; out.obs_kept = r.obs_kept;
    out.dropped_depth = r.dropped_depth; out.dropped_reprojection = r.dropped_reprojection; out.dropped_angle = r.dropped_angle;
    out.dropped_triangulation = r.dropped_triangulation; out.dropped_min_views = r.dropped_min_views;
    out.tracks_changed_reprojection = r.changed_reprojection; out.tracks_changed_angle = r.changed_angle;
    out.tracks_changed_triangulation = r.changed_triangulation; out.tracks_changed_min_views = r.changed_min_views;
    out.cos_angle = c.cos_angle; out.cos_triangulation = c.cos_triangulation;
    out.seconds_kernels = r.seconds_kernels; out.seconds_download = r.seconds_download;
    *res = out;
    return XM_OK;
    XM_CATCH
}
int xm_track_filter_limits(int64_t out[3]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_track_filter_limits: null argument");
    out[0] = xm::kSchurHeavy; out[1] = xm::kTfTile; out[2] = xm::kTfThreads;
    return XM_OK;
    XM_CATCH
}
int xm_ctx_triangulate_tracks(xm_ctx_t *ctx, const xm_tri_options_t *opt, const double *rot, const double *t, double *p, const uint8_t *candidate,
                              uint8_t *keep, uint8_t *reason, int32_t *lm_views, uint8_t *lm_status, int32_t *lm_support, int32_t *lm_hypothesis,
                              xm_tri_result_t *res) {
    XM_TRY
    const std::string w("xm_ctx_triangulate_tracks");
    if (!ctx || !opt || !rot || !t || !p || !keep || !reason || !lm_views || !lm_status || !lm_support || !lm_hypothesis || !res)
        throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_tri_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_tri_options_t.struct_size is not sizeof(xm_tri_options_t)");
    if (res->struct_size != sizeof(xm_tri_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_tri_result_t.struct_size is not sizeof(xm_tri_result_t)");
    if (opt->max_hypotheses < 1) throw xm::Error(XM_ERR_ARG, w + ": max_hypotheses must be at least 1");
    if (opt->refine_rounds < 1) throw xm::Error(XM_ERR_ARG, w + ": refine_rounds must be at least 1");
    if (opt->min_views < 0) throw xm::Error(XM_ERR_ARG, w + ": min_views is negative");
    if (!(opt->min_angle > 0.0 && opt->min_angle <= 180.0)) throw xm::Error(XM_ERR_ARG, w + ": min_angle must be positive and at most 180 degrees");
    if (!(opt->create_max_angle_error > 0.0 && opt->create_max_angle_error <= 180.0))
        throw xm::Error(XM_ERR_ARG, w + ": create_max_angle_error must be positive and at most 180 degrees");
    if (!(std::isfinite(opt->complete_max_reproj_error) && opt->complete_max_reproj_error > 0.0))
        throw xm::Error(XM_ERR_ARG, w + ": complete_max_reproj_error must be finite and positive");
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, w + ": single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1) throw xm::Error(XM_ERR_ARG, w + ": single-rank contexts only");
    const int64_t n = ctx->impl->cameras(), m = ctx->impl->n_landmarks();
    for (int64_t k = 0; k < 9 * n; ++k)
        if (!std::isfinite(rot[k])) throw xm::Error(XM_ERR_ARG, w + ": rotations are not finite");
    for (int64_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(t[k])) throw xm::Error(XM_ERR_ARG, w + ": translations are not finite");
    for (int64_t k = 0; k < 3 * m; ++k)
        if (!std::isfinite(p[k])) throw xm::Error(XM_ERR_ARG, w + ": landmarks are not finite");
    xm::TriSettings c;
    c.max_hypotheses = opt->max_hypotheses; c.refine_rounds = opt->refine_rounds; c.min_views = opt->min_views;
    c.complete_max_reproj_error = opt->complete_max_reproj_error;
    // the cosines of the two angles, once, on the host; the kernels compare against these doubles
    constexpr double kPi = 3.14159265358979323846;
    c.cos_min_angle = std::cos(opt->min_angle * (kPi / 180.0));
    c.cos_create = std::cos(opt->create_max_angle_error * (kPi / 180.0));
    xm::TriOutcome r;
    ctx->impl->triangulate_tracks(c, rot, t, p, candidate, keep, reason, lm_views, lm_status, lm_support, lm_hypothesis, r);
    xm_tri_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_tri_result_t);
    out.lm_accepted = r.lm[XM_TRI_LM_ACCEPTED]; out.lm_unused = r.lm[XM_TRI_LM_UNUSED]; out.lm_no_hypothesis = r.lm[XM_TRI_LM_NO_HYPOTHESIS];
    out.lm_degenerate = r.lm[XM_TRI_LM_DEGENERATE]; out.lm_min_views = r.lm[XM_TRI_LM_MIN_VIEWS]; out.lm_angle = r.lm[XM_TRI_LM_ANGLE];
    out.obs_candidates = r.obs_candidates; out.obs_kept = r.obs_kept; out.obs_readmitted = r.obs_readmitted; out.obs_lost = r.obs_lost;
    out.pairs_tested = r.pairs_tested; out.hypotheses_scored = r.hypotheses_scored;
    out.cos_min_angle = c.cos_min_angle; out.cos_create = c.cos_create;
    out.seconds_kernels = r.seconds_kernels; out.seconds_download = r.seconds_download;
    *res = out;
    return XM_OK;
    XM_CATCH
}
int xm_triangulate_limits(int64_t out[3]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_triangulate_limits: null argument");
    out[0] = xm::kSchurHeavy; out[1] = xm::kTriTile; out[2] = xm::kTriThreads;
    return XM_OK;
    XM_CATCH
}
namespace {
void prune_settings(const char *who, const xm_prune_options_t *opt, const int32_t *cluster_id, const int32_t *obs_count, const xm_prune_pairs_t *pairs,
                    const xm_prune_result_t *res, xm::PruneSettings &c, xm::PrunePairs &pp) {
    const std::string w(who);
    if (!opt || !cluster_id || !obs_count || !res) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_prune_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_prune_options_t.struct_size is not sizeof(xm_prune_options_t)");
    if (res->struct_size != sizeof(xm_prune_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_prune_result_t.struct_size is not sizeof(xm_prune_result_t)");
    if (opt->min_covisibility < 0 || opt->min_num_images < 0 || opt->min_num_observations < 0) throw xm::Error(XM_ERR_ARG, w + ": negative option");
    if (!std::isfinite(opt->min_threshold)) throw xm::Error(XM_ERR_ARG, w + ": min_threshold is not finite");
    if (pairs) {
        if (pairs->capacity < 0) throw xm::Error(XM_ERR_ARG, w + ": xm_prune_pairs_t.capacity is negative");
        if (pairs->capacity > 0 && (!pairs->i || !pairs->j || !pairs->count)) throw xm::Error(XM_ERR_ARG, w + ": null array in xm_prune_pairs_t");
        pp.capacity = pairs->capacity; pp.i = pairs->i; pp.j = pairs->j; pp.count = pairs->count;
    }
    c.min_covisibility = opt->min_covisibility; c.min_num_images = opt->min_num_images; c.min_num_observations = opt->min_num_observations;
    c.min_threshold = opt->min_threshold;
}
void give_prune(xm_prune_result_t *res, const xm::PruneOutcome &r) {
    xm_prune_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_prune_result_t);
    out.rounds = r.rounds; out.pairs_covisible = r.pairs_covisible; out.n_edges = r.n_edges; out.median = r.median; out.mad = r.mad;
    out.threshold = r.threshold; out.component_images = r.component_images; out.strong_clusters = r.strong_clusters; out.weak_edges = r.weak_edges;
    out.n_clusters = r.n_clusters; out.images_clustered = r.images_clustered; out.seconds_kernels = r.seconds_kernels;
    out.seconds_download = r.seconds_download;
    *res = out;
}
}  // namespace
int xm_prune_weakly_connected(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *w, const xm_prune_options_t *opt,
                              int32_t *cluster_id, int32_t *obs_count, const xm_prune_pairs_t *pairs, xm_prune_result_t *res) {
    XM_TRY
    xm::PruneSettings c;
    xm::PrunePairs pp;
    prune_settings("xm_prune_weakly_connected", opt, cluster_id, obs_count, pairs, res, c, pp);
    if (n < 0 || m < 0 || nobs < 0) throw xm::Error(XM_ERR_ARG, "xm_prune_weakly_connected: negative size");
    if (n >= ((int64_t)1 << 31) || m >= ((int64_t)1 << 31) || nobs >= ((int64_t)1 << 31))
        throw xm::Error(XM_ERR_ARG, "xm_prune_weakly_connected: cameras, landmarks and observations must each stay below 2^31");
    if (nobs > 0 && (!cam || !lm)) throw xm::Error(XM_ERR_ARG, "xm_prune_weakly_connected: null observation arrays");
    require_device();
    if (const char *e = std::getenv("XM_WATCHDOG_S")) { const double v = std::atof(e); if (v > 0) c.watchdog_s = v; }
    xm::PruneOutcome r;
    xm::prune_host(n, m, nobs, cam, lm, w, c, cluster_id, obs_count, pairs ? &pp : nullptr, r);
    give_prune(res, r);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_prune_weakly_connected(xm_ctx_t *ctx, const xm_prune_options_t *opt, int32_t *cluster_id, int32_t *obs_count, const xm_prune_pairs_t *pairs,
                                  xm_prune_result_t *res) {
    XM_TRY
    if (!ctx) throw xm::Error(XM_ERR_ARG, "xm_ctx_prune_weakly_connected: null argument");
    xm::PruneSettings c;
    xm::PrunePairs pp;
    prune_settings("xm_ctx_prune_weakly_connected", opt, cluster_id, obs_count, pairs, res, c, pp);
    if (ctx->team || !ctx->impl) throw xm::Error(XM_ERR_ARG, "xm_ctx_prune_weakly_connected: single-GPU contexts only (not n_gpus > 1)");
    if (ctx->impl->world() > 1) throw xm::Error(XM_ERR_ARG, "xm_ctx_prune_weakly_connected: single-rank contexts only");
    xm::PruneOutcome r;
    ctx->impl->prune_weakly_connected(c, cluster_id, obs_count, pairs ? &pp : nullptr, r);
    give_prune(res, r);
    return XM_OK;
    XM_CATCH
}
int xm_prune_limits(int64_t out[5]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_prune_limits: null argument");
    out[0] = xm::kPruneTile; out[1] = xm::kPruneThreads; out[2] = xm::kPruneHeavy; out[3] = xm::kPruneGroup; out[4] = xm::kPruneSelBits;
    return XM_OK;
    XM_CATCH
}
int xm_pair_filter(int64_t n, int64_t m, int64_t nobs, const int32_t *cam, const int32_t *lm, const double *p, int64_t npairs, const int32_t *pi,
                   const int32_t *pj, const double *R, const xm_pair_options_t *opt, int32_t *count, uint8_t *outlier, xm_pair_stat_t *stats,
                   xm_pair_result_t *res) {
    XM_TRY
    const std::string w("xm_pair_filter");
    if (!opt || !res) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_pair_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_pair_options_t.struct_size is not sizeof(xm_pair_options_t)");
    if (res->struct_size != sizeof(xm_pair_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_pair_result_t.struct_size is not sizeof(xm_pair_result_t)");
    if (opt->min_joint < 0 || opt->min_flags < 0 || !(opt->trim >= 0.0) || !(opt->dist_pct >= 0.0) || !(opt->err_pct >= 0.0) || !(opt->mad_factor >= 0.0))
        throw xm::Error(XM_ERR_ARG, w + ": negative option");
    if (!(opt->trim < 0.5)) throw xm::Error(XM_ERR_ARG, w + ": trim must stay below 0.5");
    if (!(opt->dist_pct <= 100.0) || !(opt->err_pct <= 100.0)) throw xm::Error(XM_ERR_ARG, w + ": a percentile above 100");
    if (opt->flags & ~XM_PAIR_SKIP_ROW0) throw xm::Error(XM_ERR_ARG, w + ": unknown flag");
    if (n < 0 || m < 0 || nobs < 0 || npairs < 0) throw xm::Error(XM_ERR_ARG, w + ": negative size");
    if (n >= ((int64_t)1 << 31) || m >= ((int64_t)1 << 31) || nobs >= ((int64_t)1 << 31) || npairs >= ((int64_t)1 << 31))
        throw xm::Error(XM_ERR_ARG, w + ": cameras, landmarks, observations and pairs must each stay below 2^31");
    if (nobs > 0 && (!cam || !lm || !p || !count || !outlier)) throw xm::Error(XM_ERR_ARG, w + ": null observation or output arrays");
    if (npairs > 0 && (!pi || !pj || !R)) throw xm::Error(XM_ERR_ARG, w + ": null pair arrays");
    xm::PairSettings c;
    c.min_joint = opt->min_joint; c.min_flags = opt->min_flags; c.skip_row0 = (opt->flags & XM_PAIR_SKIP_ROW0) != 0;
    c.trim = opt->trim; c.dist_pct = opt->dist_pct; c.err_pct = opt->err_pct; c.mad_factor = opt->mad_factor;
    require_device();
    if (const char *e = std::getenv("XM_WATCHDOG_S")) { const double v = std::atof(e); if (v > 0) c.watchdog_s = v; }
    xm::PairOutcome r;
    xm::pair_filter_host(n, m, nobs, cam, lm, p, npairs, pi, pj, R, c, count, outlier, stats, r);
    xm_pair_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_pair_result_t);
    out.pairs_used = r.pairs_used; out.pairs_skipped = r.pairs_skipped; out.pairs_degenerate = r.pairs_degenerate; out.nobs_flagged = r.nobs_flagged;
    out.max_joint = r.max_joint; out.pairs_on_workspace_path = r.pairs_on_workspace_path;
    out.seconds_index = r.seconds_index; out.seconds_kernels = r.seconds_kernels; out.seconds_download = r.seconds_download;
    *res = out;
    return XM_OK;
    XM_CATCH
}
int xm_lift_observations(int64_t n, int64_t m, int64_t nrows, const int32_t *cam, const int32_t *lm, const double *xy, const int32_t *hw,
                         const float *const *depth, const float *const *conf, const double *Kinv, const xm_lift_options_t *opt, int32_t *out_cam,
                         int32_t *out_lm, double *out_p, double *out_w, int32_t *out_row, int64_t *nout, double *threshold, xm_lift_result_t *res) {
    XM_TRY
    const std::string w("xm_lift_observations");
    if (!opt || !res || !nout) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_lift_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_lift_options_t.struct_size is not sizeof(xm_lift_options_t)");
    if (res->struct_size != sizeof(xm_lift_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_lift_result_t.struct_size is not sizeof(xm_lift_result_t)");
    if (opt->margin < 0) throw xm::Error(XM_ERR_ARG, w + ": negative margin");
    if (!(opt->depth_pct >= 0.0) || !(opt->depth_pct <= 100.0)) throw xm::Error(XM_ERR_ARG, w + ": a percentile outside [0, 100]");
    if (opt->flags & ~XM_LIFT_MAPS_ON_DEVICE) throw xm::Error(XM_ERR_ARG, w + ": unknown flag");
    if (n < 0 || m < 0 || nrows < 0) throw xm::Error(XM_ERR_ARG, w + ": negative size");
    if (n >= ((int64_t)1 << 31) || m >= ((int64_t)1 << 31) || nrows >= ((int64_t)1 << 31))
        throw xm::Error(XM_ERR_ARG, w + ": cameras, tracks and rows must each stay below 2^31");
    if (nrows > 0 && (!cam || !lm || !xy || !out_cam || !out_lm || !out_p || !out_w || !out_row)) throw xm::Error(XM_ERR_ARG, w + ": null row or output arrays");
    if (n > 0 && (!hw || !depth || !Kinv)) throw xm::Error(XM_ERR_ARG, w + ": null camera arrays");
    xm::LiftSettings c;
    c.margin = opt->margin; c.depth_pct = opt->depth_pct; c.maps_on_device = (opt->flags & XM_LIFT_MAPS_ON_DEVICE) != 0;
    require_device();
    if (const char *e = std::getenv("XM_WATCHDOG_S")) { const double v = std::atof(e); if (v > 0) c.watchdog_s = v; }
    xm::LiftOutcome r;
    xm::lift_observations_host(n, m, nrows, cam, lm, xy, hw, depth, conf, Kinv, c, out_cam, out_lm, out_p, out_w, out_row, threshold, r);
    xm_lift_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_lift_result_t);
    out.rows_duplicate = r.rows_duplicate; out.rows_border = r.rows_border; out.rows_depth = r.rows_depth; out.rows_no_map = r.rows_no_map;
    out.cams_no_map = r.cams_no_map; out.cams_empty = r.cams_empty; out.cams_small = r.cams_small; out.cams_large = r.cams_large;
    out.cams_workspace = r.cams_workspace; out.max_rows = r.max_rows;
    out.seconds_index = r.seconds_index; out.seconds_kernels = r.seconds_kernels; out.seconds_download = r.seconds_download;
    *nout = r.nout;
    *res = out;
    return XM_OK;
    XM_CATCH
}
int xm_lift_limits(int64_t out[4]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_lift_limits: null output");
    out[0] = xm::kLiftLdsRows; out[1] = xm::kLiftThreads; out[2] = xm::kLiftWsGroups; out[3] = xm::kLiftSmallRows;
    return XM_OK;
    XM_CATCH
}
int xm_build_tracks(int64_t n, const int64_t *foff, const double *xy, const uint8_t *registered, int64_t npairs, const int32_t *pi, const int32_t *pj,
                    const int64_t *moff, const int32_t *f1, const int32_t *f2, const xm_tracks_options_t *opt, int32_t *out_cam, int32_t *out_feat,
                    int32_t *out_track, double *out_xy, int64_t *nout, int32_t *label, xm_tracks_result_t *res) {
    XM_TRY
    xm::tracks_split_stats_clear();
    const std::string w("xm_build_tracks");
    const int64_t lim = (int64_t)1 << 31;
    if (!opt || !res || !nout) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_tracks_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_tracks_options_t.struct_size is not sizeof(xm_tracks_options_t)");
    if (res->struct_size != sizeof(xm_tracks_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_tracks_result_t.struct_size is not sizeof(xm_tracks_result_t)");
    if (opt->min_views < 1) throw xm::Error(XM_ERR_ARG, w + ": min_views below 1");
    if (opt->max_views < opt->min_views) throw xm::Error(XM_ERR_ARG, w + ": max_views below min_views");
    if (opt->max_tracks < 0) throw xm::Error(XM_ERR_ARG, w + ": negative max_tracks");
    if (!(opt->thres_inconsistency >= 0.0) || !(opt->thres_inconsistency <= 1.7976931348623157e308))
        throw xm::Error(XM_ERR_ARG, w + ": thres_inconsistency is negative or not finite");
    if (opt->conflict != XM_TRACKS_DROP && opt->conflict != XM_TRACKS_GLOMAP && opt->conflict != XM_TRACKS_SPLIT)
        throw xm::Error(XM_ERR_ARG, w + ": unknown conflict policy");
    if (opt->flags & ~XM_TRACKS_SPLIT_DEVICE) throw xm::Error(XM_ERR_ARG, w + ": unknown flag");
    if (opt->flags && opt->conflict != XM_TRACKS_SPLIT) throw xm::Error(XM_ERR_ARG, w + ": XM_TRACKS_SPLIT_DEVICE goes with XM_TRACKS_SPLIT only");
    if (n < 0 || npairs < 0) throw xm::Error(XM_ERR_ARG, w + ": negative size");
    if (n >= lim || npairs >= lim) throw xm::Error(XM_ERR_ARG, w + ": images and pairs must each stay below 2^31");
    if (n > 0 && !foff) throw xm::Error(XM_ERR_ARG, w + ": null feature offsets");
    if (npairs > 0 && (!pi || !pj || !moff)) throw xm::Error(XM_ERR_ARG, w + ": null pair arrays");
    if (n > 0 && foff[0] != 0) throw xm::Error(XM_ERR_ARG, w + ": foff does not start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (foff[i + 1] < foff[i]) throw xm::Error(XM_ERR_ARG, w + ": foff decreases at image " + std::to_string(i));
    const int64_t F = n > 0 ? foff[n] : 0;
    if (F >= lim) throw xm::Error(XM_ERR_ARG, w + ": features must stay below 2^31");
    if (npairs > 0 && moff[0] != 0) throw xm::Error(XM_ERR_ARG, w + ": moff does not start at 0");
    for (int64_t k = 0; k < npairs; ++k) {
        if (moff[k + 1] < moff[k]) throw xm::Error(XM_ERR_ARG, w + ": moff decreases at pair " + std::to_string(k));
        if (pi[k] < 0 || pi[k] >= n || pj[k] < 0 || pj[k] >= n) throw xm::Error(XM_ERR_ARG, w + ": image index out of range at pair " + std::to_string(k));
        if (pi[k] == pj[k]) throw xm::Error(XM_ERR_ARG, w + ": pair " + std::to_string(k) + " names one image twice");
    }
    const int64_t E = npairs > 0 ? moff[npairs] : 0;
    if (E >= lim) throw xm::Error(XM_ERR_ARG, w + ": matches must stay below 2^31");
    if (E > 0 && (!f1 || !f2)) throw xm::Error(XM_ERR_ARG, w + ": null match arrays");
    if (F > 0 && (!xy || !out_cam || !out_feat || !out_track || !out_xy)) throw xm::Error(XM_ERR_ARG, w + ": null feature or output arrays");
    xm::TracksSettings c;
    c.min_views = opt->min_views; c.max_views = opt->max_views; c.conflict = opt->conflict; c.max_tracks = opt->max_tracks;
    c.thres_inconsistency = opt->thres_inconsistency; c.split_device = (opt->flags & XM_TRACKS_SPLIT_DEVICE) != 0;
    if (n > 0 && E > 0) require_device();
    if (const char *e = std::getenv("XM_WATCHDOG_S")) { const double v = std::atof(e); if (v > 0) c.watchdog_s = v; }
    xm::TracksOutcome r;
    xm::build_tracks_host(n, foff, xy, registered, npairs, pi, pj, moff, f1, f2, c, out_cam, out_feat, out_track, out_xy, label, r);
    xm_tracks_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_tracks_result_t);
    out.rounds = r.rounds; out.ntracks = r.ntracks; out.features_touched = r.features_touched; out.matches = r.matches;
    out.components = r.components; out.components_conflicted = r.components_conflicted; out.rows_conflicted = r.rows_conflicted;
    out.tracks_short = r.tracks_short; out.tracks_long = r.tracks_long; out.tracks_conflict = r.tracks_conflict;
    out.tracks_few_registered = r.tracks_few_registered; out.tracks_beyond_max = r.tracks_beyond_max;
    out.images_small = r.images_small; out.images_large = r.images_large; out.images_workspace = r.images_workspace; out.max_touched = r.max_touched;
    out.edges_split = r.edges_split; out.unions_refused = r.unions_refused;
    out.seconds_index = r.seconds_index; out.seconds_kernels = r.seconds_kernels; out.seconds_split = r.seconds_split; out.seconds_download = r.seconds_download;
    *nout = r.nout;
    *res = out;
    return XM_OK;
    XM_CATCH
}
int xm_tracks_limits(int64_t out[4]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_tracks_limits: null output");
    out[0] = xm::kTracksLdsRows; out[1] = xm::kTracksThreads; out[2] = xm::kTracksWsGroups; out[3] = xm::kTracksSmallRows;
    return XM_OK;
    XM_CATCH
}
int xm_tracks_split_host(int64_t n, const int64_t *foff, int64_t nedges, const int32_t *eu, const int32_t *ev, int32_t *label, int64_t *distinct,
                         int64_t *refused) {
    XM_TRY
    const std::string w("xm_tracks_split_host");
    if (n < 0 || nedges < 0) throw xm::Error(XM_ERR_ARG, w + ": negative size");
    if (n > 0 && !foff) throw xm::Error(XM_ERR_ARG, w + ": null feature offsets");
    if (n > 0 && foff[0] != 0) throw xm::Error(XM_ERR_ARG, w + ": foff does not start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (foff[i + 1] < foff[i]) throw xm::Error(XM_ERR_ARG, w + ": foff decreases at image " + std::to_string(i));
    const int64_t F = n > 0 ? foff[n] : 0;
    if (F >= ((int64_t)1 << 31)) throw xm::Error(XM_ERR_ARG, w + ": features must stay below 2^31");
    if (nedges > 0 && (!eu || !ev)) throw xm::Error(XM_ERR_ARG, w + ": null edge arrays");
    if (F > 0 && !label) throw xm::Error(XM_ERR_ARG, w + ": null label array");
    std::vector<uint64_t> edges((size_t)nedges);
    for (int64_t e = 0; e < nedges; ++e) {
        if (eu[e] < 0 || eu[e] >= F || ev[e] < 0 || ev[e] >= F) throw xm::Error(XM_ERR_ARG, w + ": feature index out of range at edge " + std::to_string(e));
        const uint32_t a = (uint32_t)std::min(eu[e], ev[e]), b = (uint32_t)std::max(eu[e], ev[e]);
        edges[(size_t)e] = ((uint64_t)a << 32) | (uint64_t)b;
    }
    xm::TrackSplit sp;
    xm::tracks_split(n, foff, edges, sp);
    for (int64_t g = 0; g < F; ++g) label[g] = -1;
    for (size_t v = 0; v < sp.feat.size(); ++v) label[sp.feat[v]] = sp.label[v];
    if (distinct) *distinct = sp.distinct;
    if (refused) *refused = sp.refused;
    return XM_OK;
    XM_CATCH
}
int xm_tracks_split_device(int64_t n, const int64_t *foff, int64_t nedges, const int32_t *eu, const int32_t *ev, int32_t *label, int64_t *distinct,
                           int64_t *refused) {
    XM_TRY
    xm::tracks_split_stats_clear();
    const std::string w("xm_tracks_split_device");
    if (n < 0 || nedges < 0) throw xm::Error(XM_ERR_ARG, w + ": negative size");
    if (n >= ((int64_t)1 << 31) || nedges >= ((int64_t)1 << 31)) throw xm::Error(XM_ERR_ARG, w + ": images and edges must each stay below 2^31");
    if (n > 0 && !foff) throw xm::Error(XM_ERR_ARG, w + ": null feature offsets");
    if (n > 0 && foff[0] != 0) throw xm::Error(XM_ERR_ARG, w + ": foff does not start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (foff[i + 1] < foff[i]) throw xm::Error(XM_ERR_ARG, w + ": foff decreases at image " + std::to_string(i));
    const int64_t F = n > 0 ? foff[n] : 0;
    if (F >= ((int64_t)1 << 31)) throw xm::Error(XM_ERR_ARG, w + ": features must stay below 2^31");
    if (nedges > 0 && (!eu || !ev)) throw xm::Error(XM_ERR_ARG, w + ": null edge arrays");
    if (F > 0 && !label) throw xm::Error(XM_ERR_ARG, w + ": null label array");
    std::vector<int32_t> lo((size_t)nedges), hi((size_t)nedges);
    for (int64_t e = 0; e < nedges; ++e) {
        if (eu[e] < 0 || eu[e] >= F || ev[e] < 0 || ev[e] >= F) throw xm::Error(XM_ERR_ARG, w + ": feature index out of range at edge " + std::to_string(e));
        lo[(size_t)e] = std::min(eu[e], ev[e]); hi[(size_t)e] = std::max(eu[e], ev[e]);
    }
    int64_t d = 0, r = 0;
    if (nedges > 0) {
        require_device();
        double watchdog_s = xm::TracksSettings().watchdog_s;
        if (const char *e = std::getenv("XM_WATCHDOG_S")) { const double v = std::atof(e); if (v > 0) watchdog_s = v; }
        std::vector<int32_t> out((size_t)F);
        xm::tracks_split_device_host(n, foff, nedges, lo.data(), hi.data(), out.data(), d, r, watchdog_s);
        std::memcpy(label, out.data(), (size_t)F * sizeof(int32_t));
    } else {
        for (int64_t g = 0; g < F; ++g) label[g] = -1;
    }
    if (distinct) *distinct = d;
    if (refused) *refused = r;
    return XM_OK;
    XM_CATCH
}
int xm_tracks_split_limits(int64_t out[4]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_tracks_split_limits: null output");
    out[0] = xm::kSplitWaveEnds; out[1] = xm::kSplitWaveEdges; out[2] = xm::kSplitGroupEdges; out[3] = xm::kTracksThreads;
    return XM_OK;
    XM_CATCH
}
int xm_tracks_split_stats(int64_t out[8]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_tracks_split_stats: null output");
    xm::tracks_split_stats_get(out);
    return XM_OK;
    XM_CATCH
}
int xm_view_graph_filter(int64_t n, const int64_t *foff, const double *xy, const double *focal, const double *Kinv, const double *bearing, int64_t npairs,
                         const int32_t *pi, const int32_t *pj, const int32_t *model, const double *Rrel, const double *trel, const double *FH,
                         const uint8_t *valid_in, const uint8_t *registered_in, const double *rot, const int64_t *moff, const int32_t *f1, const int32_t *f2,
                         const xm_vg_options_t *opt, uint8_t *inlier, int32_t *pair_inliers, int32_t *pair_status, uint8_t *registered_out, int64_t *moff_out,
                         int32_t *f1_out, int32_t *f2_out, xm_vg_result_t *res) {
    XM_TRY
    const std::string w("xm_view_graph_filter");
    const int64_t lim = (int64_t)1 << 31;
    const double dmax = 1.7976931348623157e308;
    if (!opt || !res) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_vg_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_vg_options_t.struct_size is not sizeof(xm_vg_options_t)");
    if (res->struct_size != sizeof(xm_vg_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_vg_result_t.struct_size is not sizeof(xm_vg_result_t)");
    if (opt->flags & ~XM_VG_SCORE) throw xm::Error(XM_ERR_ARG, w + ": unknown flag");
    const double thr[5] = {opt->max_epipolar_error_E, opt->max_epipolar_error_F, opt->max_epipolar_error_H, opt->min_inlier_ratio, opt->cos_max_rotation_error};
    const char *thr_name[5] = {"max_epipolar_error_E", "max_epipolar_error_F", "max_epipolar_error_H", "min_inlier_ratio", "cos_max_rotation_error"};
    for (int x = 0; x < 5; ++x) {
        const double lo = x == 4 ? -dmax : 0.0;   // (a cosine may be negative)
        if (!(thr[x] >= lo) || !(thr[x] <= dmax)) throw xm::Error(XM_ERR_ARG, w + ": " + thr_name[x] + " is negative or not finite");
    }
    if (opt->min_inlier_num < 0) throw xm::Error(XM_ERR_ARG, w + ": negative min_inlier_num");
    if (n < 0 || npairs < 0) throw xm::Error(XM_ERR_ARG, w + ": negative size");
    if (n >= lim || npairs >= lim) throw xm::Error(XM_ERR_ARG, w + ": images and pairs must each stay below 2^31");
    if (n > 0 && (!foff || !registered_out)) throw xm::Error(XM_ERR_ARG, w + ": null feature offsets or registered_out");
    if (npairs > 0 && (!pi || !pj || !model || !moff || !pair_inliers || !pair_status || !moff_out)) throw xm::Error(XM_ERR_ARG, w + ": null pair arrays");
    if (n > 0 && foff[0] != 0) throw xm::Error(XM_ERR_ARG, w + ": foff does not start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (foff[i + 1] < foff[i]) throw xm::Error(XM_ERR_ARG, w + ": foff decreases at image " + std::to_string(i));
    const int64_t F = n > 0 ? foff[n] : 0;
    if (F >= lim) throw xm::Error(XM_ERR_ARG, w + ": features must stay below 2^31");
    if (npairs > 0 && moff[0] != 0) throw xm::Error(XM_ERR_ARG, w + ": moff does not start at 0");
    const bool score = (opt->flags & XM_VG_SCORE) != 0;
    bool any_E = false;
    for (int64_t k = 0; k < npairs; ++k) {
        if (moff[k + 1] < moff[k]) throw xm::Error(XM_ERR_ARG, w + ": moff decreases at pair " + std::to_string(k));
        if (pi[k] < 0 || pi[k] >= n || pj[k] < 0 || pj[k] >= n) throw xm::Error(XM_ERR_ARG, w + ": image index out of range at pair " + std::to_string(k));
        if (pi[k] == pj[k]) throw xm::Error(XM_ERR_ARG, w + ": pair " + std::to_string(k) + " names one image twice");
        if (model[k] < XM_VG_MODEL_NONE || model[k] > XM_VG_MODEL_H) throw xm::Error(XM_ERR_ARG, w + ": unknown model at pair " + std::to_string(k));
        if ((model[k] == XM_VG_MODEL_F || model[k] == XM_VG_MODEL_H) && !FH)
            throw xm::Error(XM_ERR_ARG, w + ": pair " + std::to_string(k) + " is an F or H pair and FH is null");
        if (model[k] == XM_VG_MODEL_E && score && (!valid_in || valid_in[k])) any_E = true;
    }
    if (any_E && ((!Kinv && !bearing) || !focal || !Rrel || !trel))
        throw xm::Error(XM_ERR_ARG, w + ": an E pair is scored and Kinv and bearing are both null, or focal, Rrel or trel is null");
    if (rot && npairs > 0 && !Rrel) throw xm::Error(XM_ERR_ARG, w + ": rot is given and Rrel is null");
    const int64_t E = npairs > 0 ? moff[npairs] : 0;
    if (E >= lim) throw xm::Error(XM_ERR_ARG, w + ": matches must stay below 2^31");
    if (E > 0 && (!f1 || !f2 || !inlier || !f1_out || !f2_out)) throw xm::Error(XM_ERR_ARG, w + ": null match arrays");
    if (F > 0 && !xy) throw xm::Error(XM_ERR_ARG, w + ": null feature positions");
    xm::VgSettings c;
    c.score = score; c.max_E = opt->max_epipolar_error_E; c.max_F = opt->max_epipolar_error_F; c.max_H = opt->max_epipolar_error_H;
    c.min_inlier_num = opt->min_inlier_num; c.min_inlier_ratio = opt->min_inlier_ratio; c.cos_max_rotation_error = opt->cos_max_rotation_error;
    if (npairs > 0) require_device();
    if (const char *e = std::getenv("XM_WATCHDOG_S")) { const double v = std::atof(e); if (v > 0) c.watchdog_s = v; }
    xm::VgOutcome r;
    xm::view_graph_filter_host(n, foff, xy, focal, Kinv, bearing, npairs, pi, pj, model, Rrel, trel, FH, valid_in, registered_in, rot, moff, f1, f2, c, inlier,
                               pair_inliers, pair_status, registered_out, moff_out, f1_out, f2_out, r);
    xm_vg_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_vg_result_t);
    out.rounds = r.rounds; out.matches = r.matches; out.inliers = r.inliers; out.matches_out = r.matches_out;
    out.pairs_valid = r.pairs_by_status[XM_VG_VALID]; out.pairs_invalid_in = r.pairs_by_status[XM_VG_INVALID_IN];
    out.pairs_few_inliers = r.pairs_by_status[XM_VG_FEW_INLIERS]; out.pairs_low_ratio = r.pairs_by_status[XM_VG_LOW_RATIO];
    out.pairs_rotation = r.pairs_by_status[XM_VG_ROTATION]; out.pairs_outside = r.pairs_by_status[XM_VG_OUTSIDE];
    out.pairs_none = r.pairs_by_model[XM_VG_MODEL_NONE]; out.pairs_E = r.pairs_by_model[XM_VG_MODEL_E]; out.pairs_F = r.pairs_by_model[XM_VG_MODEL_F];
    out.pairs_H = r.pairs_by_model[XM_VG_MODEL_H];
    out.largest = r.largest; out.components = r.components; out.pairs_wave = r.pairs_wave; out.pairs_group = r.pairs_group;
    out.pairs_workspace = r.pairs_workspace; out.max_matches = r.max_matches;
    out.seconds_index = r.seconds_index; out.seconds_kernels = r.seconds_kernels; out.seconds_download = r.seconds_download;
    *res = out;
    return XM_OK;
    XM_CATCH
}
int xm_view_graph_limits(int64_t out[4]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_view_graph_limits: null output");
    out[0] = xm::kVgGroupMatches; out[1] = xm::kVgThreads; out[2] = xm::kVgWaveMatches; out[3] = xm::kMaxRounds;
    return XM_OK;
    XM_CATCH
}
namespace {
// the checks xm_view_graph_calibrate and its probe share: everything on the host, before any device call
void vgc_check(const std::string &w, const xm::VgcInput &in, const xm_vgc_options_t *opt, xm::VgcSettings &c) {
    const int64_t lim = (int64_t)1 << 31;
    const double dmax = 1.7976931348623157e308;
    if (!opt) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_vgc_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_vgc_options_t.struct_size is not sizeof(xm_vgc_options_t)");
    if (opt->flags & ~XM_VGC_UPDATE_CONFIG) throw xm::Error(XM_ERR_ARG, w + ": unknown flag");
    const double v[6] = {opt->thres_loss_function, opt->thres_lower_ratio, opt->thres_higher_ratio, opt->thres_two_view_error, opt->function_tolerance,
                         opt->lower_bound};
    const char *name[6] = {"thres_loss_function", "thres_lower_ratio", "thres_higher_ratio", "thres_two_view_error", "function_tolerance", "lower_bound"};
    for (int x = 0; x < 6; ++x)
        if (!(v[x] > 0.0) || !(v[x] <= dmax)) throw xm::Error(XM_ERR_ARG, w + ": " + name[x] + " is not positive or not finite");
    if (opt->max_num_iterations <= 0) throw xm::Error(XM_ERR_ARG, w + ": max_num_iterations is not positive");
    if (opt->thres_lower_ratio > opt->thres_higher_ratio) throw xm::Error(XM_ERR_ARG, w + ": thres_lower_ratio is above thres_higher_ratio");
    if (in.ncams < 0 || in.n < 0 || in.npairs < 0) throw xm::Error(XM_ERR_ARG, w + ": negative size");
    if (in.ncams >= lim || in.n >= lim || in.npairs >= lim) throw xm::Error(XM_ERR_ARG, w + ": cameras, images and pairs must each stay below 2^31");
    if (in.ncams > 0 && (!in.focal0 || !in.pp || !in.has_prior)) throw xm::Error(XM_ERR_ARG, w + ": null camera arrays");
    if (in.n > 0 && !in.cam_of_image) throw xm::Error(XM_ERR_ARG, w + ": null cam_of_image");
    if (in.npairs > 0 && (!in.pi || !in.pj || !in.model || !in.F)) throw xm::Error(XM_ERR_ARG, w + ": null pair arrays");
    const bool update = (opt->flags & XM_VGC_UPDATE_CONFIG) != 0;
    if (update && in.npairs > 0 && (!in.Rrel || !in.trel)) throw xm::Error(XM_ERR_ARG, w + ": XM_VGC_UPDATE_CONFIG without Rrel or trel");
    for (int64_t c = 0; c < in.ncams; ++c) {
        if (!(in.focal0[c] > 0.0) || !(in.focal0[c] <= dmax)) throw xm::Error(XM_ERR_ARG, w + ": focal0 of camera " + std::to_string(c) + " is not positive or not finite");
        if (!(std::fabs(in.pp[2 * c]) <= dmax) || !(std::fabs(in.pp[2 * c + 1]) <= dmax))
            throw xm::Error(XM_ERR_ARG, w + ": the principal point of camera " + std::to_string(c) + " is not finite");
    }
    for (int64_t i = 0; i < in.n; ++i)
        if (in.cam_of_image[i] < 0 || in.cam_of_image[i] >= in.ncams) throw xm::Error(XM_ERR_ARG, w + ": camera index out of range at image " + std::to_string(i));
    for (int64_t k = 0; k < in.npairs; ++k) {
        if (in.pi[k] < 0 || in.pi[k] >= in.n || in.pj[k] < 0 || in.pj[k] >= in.n) throw xm::Error(XM_ERR_ARG, w + ": image index out of range at pair " + std::to_string(k));
        if (in.pi[k] == in.pj[k]) throw xm::Error(XM_ERR_ARG, w + ": pair " + std::to_string(k) + " names one image twice");
        if (in.model[k] < XM_VG_MODEL_NONE || in.model[k] > XM_VG_MODEL_H) throw xm::Error(XM_ERR_ARG, w + ": unknown model at pair " + std::to_string(k));
        if ((in.valid_in && !in.valid_in[k]) || (in.model[k] != XM_VG_MODEL_E && in.model[k] != XM_VG_MODEL_F)) continue;
        for (int e = 0; e < 9; ++e)
            if (!(std::fabs(in.F[9 * k + e]) <= dmax)) throw xm::Error(XM_ERR_ARG, w + ": F of pair " + std::to_string(k) + " is not finite");
        if (update)
            for (int e = 0; e < 12; ++e) {
                const double x = e < 9 ? in.Rrel[9 * k + e] : in.trel[3 * k + e - 9];
                if (!(std::fabs(x) <= dmax)) throw xm::Error(XM_ERR_ARG, w + ": Rrel or trel of pair " + std::to_string(k) + " is not finite");
            }
    }
    c.update_config = update;
    c.loss_scale = opt->thres_loss_function; c.lower_ratio = opt->thres_lower_ratio; c.higher_ratio = opt->thres_higher_ratio;
    c.two_view_error = opt->thres_two_view_error; c.max_iters = opt->max_num_iterations; c.function_tol = opt->function_tolerance;
    c.lower_bound = opt->lower_bound;
    if (const char *e = std::getenv("XM_WATCHDOG_S")) { const double s = std::atof(e); if (s > 0) c.watchdog_s = s; }
}
}  // namespace
int xm_view_graph_calibrate(int64_t ncams, const double *focal0, const double *pp, const uint8_t *has_prior, int64_t n, const int32_t *cam_of_image,
                            int64_t npairs, const int32_t *pi, const int32_t *pj, const int32_t *model, const double *F, const uint8_t *valid_in,
                            const double *Rrel, const double *trel, const xm_vgc_options_t *opt, double *focal_out, double *focal_est, uint8_t *refined,
                            int32_t *cam_status, int32_t *pair_status, double *residual, double *d_out, int32_t *model_out, double *F_out,
                            double *cost_trace, xm_vgc_result_t *res) {
    XM_TRY
    const std::string w("xm_view_graph_calibrate");
    if (!res) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (res->struct_size != sizeof(xm_vgc_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_vgc_result_t.struct_size is not sizeof(xm_vgc_result_t)");
    xm::VgcInput in;
    in.ncams = ncams; in.n = n; in.npairs = npairs; in.focal0 = focal0; in.pp = pp; in.has_prior = has_prior; in.cam_of_image = cam_of_image;
    in.pi = pi; in.pj = pj; in.model = model; in.F = F; in.valid_in = valid_in; in.Rrel = Rrel; in.trel = trel;
    xm::VgcSettings c;
    vgc_check(w, in, opt, c);
    if (ncams > 0 && (!focal_out || !focal_est || !refined || !cam_status)) throw xm::Error(XM_ERR_ARG, w + ": null camera outputs");
    if (npairs > 0 && (!pair_status || !residual)) throw xm::Error(XM_ERR_ARG, w + ": null pair outputs");
    xm::VgcOutput o;
    o.focal_out = focal_out; o.focal_est = focal_est; o.refined = refined; o.cam_status = cam_status; o.pair_status = pair_status;
    o.residual = residual; o.d_out = d_out; o.model_out = model_out; o.F_out = F_out; o.cost_trace = cost_trace;
    if (npairs > 0) require_device();
    xm::VgcOutcome r;
    xm::view_graph_calibrate_host(in, c, o, r);
    xm_vgc_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_vgc_result_t);
    out.stop_reason = r.stop; out.pairs = r.pairs; out.pairs_same_camera = r.pairs_same; out.cams_free = r.cams_free; out.cams_constant = r.cams_constant;
    out.cams_rejected = r.cams_rejected; out.pairs_invalidated = r.pairs_invalidated; out.pairs_flipped = r.pairs_flipped; out.cams_heavy = r.cams_heavy;
    out.max_incidences = r.max_incidences; out.pcg_iterations = r.pcg_iters; out.iterations = r.iters; out.accepted = r.accepted;
    out.trace_len = r.trace_len; out.initial_cost = r.initial_cost; out.final_cost = r.final_cost;
    out.seconds_index = r.seconds_index; out.seconds_kernels = r.seconds_kernels; out.seconds_download = r.seconds_download;
    *res = out;
    return XM_OK;
    XM_CATCH
}
int xm_view_graph_calibrate_probe(int64_t ncams, const double *focal0, const double *pp, const uint8_t *has_prior, int64_t n, const int32_t *cam_of_image,
                                  int64_t npairs, const int32_t *pi, const int32_t *pj, const int32_t *model, const double *F, const uint8_t *valid_in,
                                  const xm_vgc_options_t *opt, xm_vgc_probe_t *probe) {
    XM_TRY
    const std::string w("xm_view_graph_calibrate_probe");
    if (!probe) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (probe->struct_size != sizeof(xm_vgc_probe_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_vgc_probe_t.struct_size is not sizeof(xm_vgc_probe_t)");
    xm::VgcInput in;
    in.ncams = ncams; in.n = n; in.npairs = npairs; in.focal0 = focal0; in.pp = pp; in.has_prior = has_prior; in.cam_of_image = cam_of_image;
    in.pi = pi; in.pj = pj; in.model = model; in.F = F; in.valid_in = valid_in;
    xm::VgcSettings c;
    vgc_check(w, in, opt, c);
    if (opt->flags) throw xm::Error(XM_ERR_ARG, w + ": the probe takes no flag");
    if (ncams > 0 && !probe->focal) throw xm::Error(XM_ERR_ARG, w + ": null focal");
    if (!(probe->mu >= 0.0) || !(probe->mu <= 1.7976931348623157e308)) throw xm::Error(XM_ERR_ARG, w + ": mu is negative or not finite");
    for (int64_t i = 0; i < ncams; ++i)
        if (!(probe->focal[i] > 0.0) || !(probe->focal[i] <= 1.7976931348623157e308)) throw xm::Error(XM_ERR_ARG, w + ": a focal is not positive or not finite");
    xm::VgcProbe q;
    q.focal = probe->focal; q.x = probe->x; q.d_in = probe->d_in; q.mu = probe->mu; q.d = probe->d; q.residual = probe->residual; q.record = probe->record;
    q.cost = probe->cost; q.gradient = probe->gradient; q.diagonal = probe->diagonal; q.product = probe->product;
    if (npairs > 0) require_device();
    xm::view_graph_calibrate_probe_host(in, c, q);
    return XM_OK;
    XM_CATCH
}
int xm_view_graph_calibrate_limits(int64_t out[4]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_view_graph_calibrate_limits: null output");
    out[0] = xm::kVgcLightIncidences; out[1] = xm::kVgcThreads; out[2] = xm::kVgcSweeps; out[3] = xm::kVgcMaxPcgIters;
    return XM_OK;
    XM_CATCH
}
namespace {
// the checks xm_view_graph_rotations and its probe share (rule 11): everything on the host, before any device call.  Returns the number of
// participating pairs.
int64_t vgr_check(const std::string &w, const xm::RavInput &in, const xm_vgr_options_t *opt, xm::RavSettings &c) {
    const int64_t lim = (int64_t)1 << 31;
    const double dmax = 1.7976931348623157e308;
    if (!opt) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (opt->struct_size != sizeof(xm_vgr_options_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_vgr_options_t.struct_size is not sizeof(xm_vgr_options_t)");
    if (opt->weight_type != XM_VGR_GEMAN_MCCLURE && opt->weight_type != XM_VGR_HALF_NORM) throw xm::Error(XM_ERR_ARG, w + ": unknown weight type");
    if (opt->max_num_irls_iterations <= 0) throw xm::Error(XM_ERR_ARG, w + ": max_num_irls_iterations is not positive");
    const double v[2] = {opt->irls_step_convergence_threshold, opt->irls_loss_parameter_sigma};
    const char *name[2] = {"irls_step_convergence_threshold", "irls_loss_parameter_sigma"};
    for (int x = 0; x < 2; ++x)
        if (!(v[x] > 0.0) || !(v[x] <= dmax)) throw xm::Error(XM_ERR_ARG, w + ": " + name[x] + " is not positive or not finite");
    if (in.n < 0 || in.npairs < 0) throw xm::Error(XM_ERR_ARG, w + ": negative size");
    if (in.n >= lim || in.npairs >= lim) throw xm::Error(XM_ERR_ARG, w + ": images and pairs must each stay below 2^31");
    if (in.n > 0 && !in.rot0) throw xm::Error(XM_ERR_ARG, w + ": null rot0");
    if (in.npairs > 0 && (!in.pi || !in.pj || !in.Rrel)) throw xm::Error(XM_ERR_ARG, w + ": null pair arrays");
    if (opt->fixed_image < -1 || opt->fixed_image >= in.n) throw xm::Error(XM_ERR_ARG, w + ": fixed_image out of range");
    int64_t fixed = opt->fixed_image, nreg = 0;
    for (int64_t i = 0; i < in.n; ++i) {
        if (in.registered && !in.registered[i]) continue;
        nreg++;
        if (fixed < 0) fixed = i;
        for (int e = 0; e < 9; ++e)
            if (!(std::fabs(in.rot0[9 * i + e]) <= dmax)) throw xm::Error(XM_ERR_ARG, w + ": rot0 of image " + std::to_string(i) + " is not finite");
    }
    if (opt->fixed_image >= 0 && in.registered && !in.registered[opt->fixed_image]) throw xm::Error(XM_ERR_ARG, w + ": fixed_image is not registered");
    for (int64_t k = 0; k < in.npairs; ++k) {
        if (in.pi[k] < 0 || in.pi[k] >= in.n || in.pj[k] < 0 || in.pj[k] >= in.n) throw xm::Error(XM_ERR_ARG, w + ": image index out of range at pair " + std::to_string(k));
        if (in.pi[k] == in.pj[k]) throw xm::Error(XM_ERR_ARG, w + ": pair " + std::to_string(k) + " names one image twice");
    }
    // the registered images must be one component over the participating pairs
    std::vector<int32_t> parent((size_t)in.n);
    for (int64_t i = 0; i < in.n; ++i) parent[(size_t)i] = (int32_t)i;
    auto find = [&](int32_t a) {
        while (parent[(size_t)a] != a) { parent[(size_t)a] = parent[(size_t)parent[(size_t)a]]; a = parent[(size_t)a]; }
        return a;
    };
    int64_t M = 0, joins = 0;
    for (int64_t k = 0; k < in.npairs; ++k) {
        if (!xm::rav_takes_part(in, k)) continue;
        M++;
        for (int e = 0; e < 9; ++e)
            if (!(std::fabs(in.Rrel[9 * k + e]) <= dmax)) throw xm::Error(XM_ERR_ARG, w + ": Rrel of pair " + std::to_string(k) + " is not finite");
        const int32_t a = find(in.pi[k]), b = find(in.pj[k]);
        if (a != b) { parent[(size_t)std::max(a, b)] = std::min(a, b); joins++; }
    }
    if (M > 0 && joins != nreg - 1) throw xm::Error(XM_ERR_ARG, w + ": the participating pairs do not connect the registered images");
    c.weight_type = opt->weight_type; c.max_iters = opt->max_num_irls_iterations; c.fixed_image = fixed;
    c.step_tol = opt->irls_step_convergence_threshold; c.sigma_deg = opt->irls_loss_parameter_sigma;
    if (const char *e = std::getenv("XM_WATCHDOG_S")) { const double s = std::atof(e); if (s > 0) c.watchdog_s = s; }
    return M;
}
}  // namespace
int xm_view_graph_rotations(int64_t n, const uint8_t *registered, const double *rot0, int64_t npairs, const int32_t *pi, const int32_t *pj,
                            const double *Rrel, const uint8_t *valid_in, const xm_vgr_options_t *opt, double *rot_out, double *angle_axis_out,
                            double *residual, double *weight, double *step_trace, xm_vgr_result_t *res) {
    XM_TRY
    const std::string w("xm_view_graph_rotations");
    if (!res) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (res->struct_size != sizeof(xm_vgr_result_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_vgr_result_t.struct_size is not sizeof(xm_vgr_result_t)");
    xm::RavInput in;
    in.n = n; in.npairs = npairs; in.registered = registered; in.rot0 = rot0; in.pi = pi; in.pj = pj; in.Rrel = Rrel; in.valid_in = valid_in;
    xm::RavSettings c;
    const int64_t M = vgr_check(w, in, opt, c);
    if (n > 0 && (!rot_out || !angle_axis_out)) throw xm::Error(XM_ERR_ARG, w + ": null image outputs");
    if (npairs > 0 && (!residual || !weight)) throw xm::Error(XM_ERR_ARG, w + ": null pair outputs");
    if (!step_trace) throw xm::Error(XM_ERR_ARG, w + ": null step_trace");
    xm::RavOutput o;
    o.rot_out = rot_out; o.angle_axis_out = angle_axis_out; o.residual = residual; o.weight = weight; o.step_trace = step_trace;
    if (M > 0) require_device();
    xm::RavOutcome r;
    xm::view_graph_rotations_host(in, c, o, r);
    xm_vgr_result_t out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(xm_vgr_result_t);
    out.stop_reason = r.stop; out.irls_iterations = r.iters; out.pcg_iterations = r.pcg_iters; out.pcg_capped = r.pcg_capped; out.pairs = r.pairs;
    out.registered = r.registered; out.fixed_image = r.fixed_image; out.cams_heavy = r.cams_heavy; out.max_incidences = r.max_incidences;
    out.seconds_index = r.seconds_index; out.seconds_kernels = r.seconds_kernels; out.seconds_download = r.seconds_download;
    *res = out;
    return XM_OK;
    XM_CATCH
}
int xm_view_graph_rotations_probe(int64_t n, const uint8_t *registered, const double *rot0, int64_t npairs, const int32_t *pi, const int32_t *pj,
                                  const double *Rrel, const uint8_t *valid_in, const xm_vgr_options_t *opt, xm_vgr_probe_t *probe) {
    XM_TRY
    const std::string w("xm_view_graph_rotations_probe");
    const double dmax = 1.7976931348623157e308;
    if (!probe) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (probe->struct_size != sizeof(xm_vgr_probe_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_vgr_probe_t.struct_size is not sizeof(xm_vgr_probe_t)");
    xm::RavInput in;
    in.n = n; in.npairs = npairs; in.registered = registered; in.rot0 = rot0; in.pi = pi; in.pj = pj; in.Rrel = Rrel; in.valid_in = valid_in;
    xm::RavSettings c;
    const int64_t M = vgr_check(w, in, opt, c);
    if (n > 0 && (!probe->angle_axis || !probe->x)) throw xm::Error(XM_ERR_ARG, w + ": null angle_axis or x");
    for (int64_t i = 0; i < n; ++i) {
        if (registered && !registered[i]) continue;
        for (int e = 0; e < 3; ++e)
            if (!(std::fabs(probe->angle_axis[3 * i + e]) <= dmax) || !(std::fabs(probe->x[3 * i + e]) <= dmax))
                throw xm::Error(XM_ERR_ARG, w + ": angle_axis or x of image " + std::to_string(i) + " is not finite");
    }
    xm::RavProbe q;
    q.angle_axis = probe->angle_axis; q.x = probe->x; q.weight_in = probe->weight_in; q.rot = probe->rot; q.residual = probe->residual;
    q.gauge = probe->gauge; q.weight = probe->weight; q.rhs = probe->rhs; q.diagonal = probe->diagonal; q.product = probe->product;
    q.angle_axis_out = probe->angle_axis_out; q.step = probe->step;
    if (M > 0) require_device();
    xm::view_graph_rotations_probe_host(in, c, q);
    return XM_OK;
    XM_CATCH
}
int xm_view_graph_rotations_limits(int64_t out[4]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_view_graph_rotations_limits: null output");
    out[0] = xm::kRavLightIncidences; out[1] = xm::kRavThreads; out[2] = xm::kRavMaxPcgIters; out[3] = 0;
    return XM_OK;
    XM_CATCH
}
int xm_pair_filter_limits(int64_t out[4]) {
    XM_TRY
    if (!out) throw xm::Error(XM_ERR_ARG, "xm_pair_filter_limits: null output");
    out[0] = xm::kPairLdsJoint; out[1] = xm::kPairThreads; out[2] = xm::kPairWsGroups; out[3] = xm::kPairSmallJoint;
    return XM_OK;
    XM_CATCH
}
int xm_ctx_set_edge_weights(xm_ctx_t *ctx, const double *w) {
    XM_TRY
    if (!ctx) throw xm::Error(XM_ERR_ARG, "null argument");
    if (ctx->team) ctx->team->set_edge_weights(w); else ctx->impl->set_edge_weights(w);
    return XM_OK;
    XM_CATCH
}
int64_t xm_dense_ld(int64_t n) { return xm::dense_ld(n); }

int xm_dev_count(int *count) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    if (count) *count = c;
    return XM_OK;
}
int xm_dev_alloc(void **ptr, size_t bytes) {
    XM_TRY require_device(); const size_t padded = (bytes ? bytes : 8) + 128;   /* slack: the sector-window gather reads whole 64-byte sectors around a record */
    XM_HIP_CHECK(hipMalloc(ptr, padded)); XM_HIP_CHECK(hipMemset(*ptr, 0, padded)); XM_HIP_CHECK(hipDeviceSynchronize()); return XM_OK; XM_CATCH
}
int xm_dev_free(void *ptr) { XM_TRY XM_HIP_CHECK(hipFree(ptr)); return XM_OK; XM_CATCH }
int xm_dev_h2d(void *dst, const void *src, size_t bytes) { XM_TRY XM_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return XM_OK; XM_CATCH }
int xm_dev_d2h(void *dst, const void *src, size_t bytes) { XM_TRY XM_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return XM_OK; XM_CATCH }
int xm_dev_sync(void) { XM_TRY XM_HIP_CHECK(hipDeviceSynchronize()); return XM_OK; XM_CATCH }

int xm_dense_upload(const double *q_host, int64_t ldq, int64_t n, double **dq) {
    XM_TRY
    require_device();
    if (!q_host || !dq || ldq < 3 * n) throw xm::Error(XM_ERR_ARG, "bad argument");
    const int64_t ld = xm::dense_ld(n), m = 3 * n;
    double *tmp = nullptr, *out = nullptr;
    XM_HIP_CHECK(hipMalloc((void **)&tmp, (size_t)m * m * sizeof(double)));
    XM_HIP_CHECK(hipMalloc((void **)&out, (size_t)m * ld * sizeof(double)));
    XM_HIP_CHECK(hipMemcpy2D(tmp, (size_t)m * sizeof(double), q_host, (size_t)ldq * sizeof(double), (size_t)m * sizeof(double), (size_t)m,
                             hipMemcpyHostToDevice));
    xm::launch_transpose_pad(tmp, m, m, m, out, ld, nullptr);
    XM_HIP_CHECK(hipDeviceSynchronize());
    XM_HIP_CHECK(hipFree(tmp));
    *dq = out;
    return XM_OK;
    XM_CATCH
}

int xm_dense_from_bsr3(const int64_t *rowptr, const int32_t *colidx, const double *blocks, int64_t n, double **dq) {
    XM_TRY
    require_device();
    if (!rowptr || !colidx || !blocks || !dq || n < 1) throw xm::Error(XM_ERR_ARG, "bad argument");
    const int64_t ld = xm::dense_ld(n), nb = rowptr[n];
    xm::DevBuf<int64_t> rp; xm::DevBuf<int32_t> ci; xm::DevBuf<double> bl;
    rp.alloc((size_t)n + 1, false); ci.alloc((size_t)nb, false); bl.alloc((size_t)nb * 9, false);
    XM_HIP_CHECK(hipMemcpy(rp.p, rowptr, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    XM_HIP_CHECK(hipMemcpy(ci.p, colidx, (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice));
    XM_HIP_CHECK(hipMemcpy(bl.p, blocks, (size_t)nb * 9 * sizeof(double), hipMemcpyHostToDevice));
    double *out = nullptr;
    XM_HIP_CHECK(hipMalloc((void **)&out, (size_t)3 * n * ld * sizeof(double)));
    XM_HIP_CHECK(hipMemset(out, 0, (size_t)3 * n * ld * sizeof(double)));
    xm::launch_dense_from_bsr(rp.p, ci.p, bl.p, n, 0, out, ld, nullptr);
    XM_HIP_CHECK(hipDeviceSynchronize());
    *dq = out;
    return XM_OK;
    XM_CATCH
}

xm::CamArgs plain_args(int64_t n, double *out) {
    xm::CamArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nloc = (int)n;
    a.out = out;
    return a;
}
int xm_qw_dense(const double *dq, int64_t n, int o, const double *dW, double *dOut, double alpha, void *stream) {
    XM_TRY
    xm::launch_qw_dense(o, xm::EPI_PLAIN, dq, xm::dense_ld(n), dW, alpha, plain_args(n, dOut), (hipStream_t)stream);
    return XM_OK;
    XM_CATCH
}
int xm_qw_dense_sym(const double *dq, int64_t n, int o, const double *dW, double *dOut, double alpha, void *stream) {
    XM_TRY
    const int64_t ld = xm::dense_ld(n);
    xm::SymvWork work;
    work.ensure((int)n, ld, o);
    xm::launch_qw_sym(o, xm::EPI_PLAIN, dq, ld, dW, alpha, plain_args(n, dOut), work, (hipStream_t)stream);
    XM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return XM_OK;
    XM_CATCH
}
int xm_dense_to_f32(const double *dq, int64_t n, float **dq32) {
    XM_TRY
    require_device();
    if (!dq || !dq32 || n < 1) throw xm::Error(XM_ERR_ARG, "bad argument");
    const int64_t ld = xm::dense_ld(n), rows = 3 * n;
    float *out = nullptr;
    XM_HIP_CHECK(hipMalloc((void **)&out, (size_t)rows * ld * sizeof(float)));
    xm::DevBuf<unsigned int> bad;
    bad.alloc(1);
    unsigned int h = 0;
    try {
        xm::launch_dense_to_f32(dq, out, rows, ld, bad.p, nullptr);
        XM_HIP_CHECK(hipMemcpy(&h, bad.p, sizeof(h), hipMemcpyDeviceToHost));
    } catch (...) { (void)hipFree(out); throw; }
    *dq32 = out;
    if (h) throw xm::Error(XM_ERR_ARG, std::to_string(h) + " entries of Q are not finite in fp32");
    return XM_OK;
    XM_CATCH
}
int xm_qw_dense_f32(const float *dq32, int64_t n, int o, const double *dW, double *dOut, double alpha, void *stream) {
    XM_TRY
    xm::launch_qw_dense_f32(o, xm::EPI_PLAIN, dq32, nullptr, xm::dense_ld(n), dW, alpha, plain_args(n, dOut), (hipStream_t)stream);
    return XM_OK;
    XM_CATCH
}
int xm_qw_dense_sym_f32(const float *dq32, int64_t n, int o, const double *dW, double *dOut, double alpha, void *stream) {
    XM_TRY
    const int64_t ld = xm::dense_ld(n);
    if (o < 3 || o > 5) throw xm::Error(XM_ERR_ARG, "fp32 symmetric product: o in 3..5");
    xm::SymvWork work;
    work.ensure((int)n, ld, o);
    xm::launch_qw_sym_f32(o, xm::EPI_PLAIN, dq32, nullptr, ld, dW, alpha, plain_args(n, dOut), work, (hipStream_t)stream);
    XM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return XM_OK;
    XM_CATCH
}
int xm_qw_bsr3(const int64_t *rp, const int32_t *ci, const double *bl, int64_t n, int o, const double *dW, double *dOut, double alpha,
               void *stream) {
    XM_TRY
    xm::launch_qw_bsr3(o, xm::EPI_PLAIN, rp, ci, bl, dW, alpha, plain_args(n, dOut), (hipStream_t)stream);
    return XM_OK;
    XM_CATCH
}
int xm_retract(int64_t n, int o, const double *dR, const double *ds, const double *dD, const double *dds, double t, double *dRout,
               double *dsout, void *stream) {
    XM_TRY
    xm::launch_retract(o, (int)n, 0, dR, ds, dD, dds, t, dRout, dsout, nullptr, (hipStream_t)stream);
    return XM_OK;
    XM_CATCH
}
int xm_retract_polar(int64_t n, int o, const double *dR, const double *ds, const double *dD, const double *dds, double t, double *dRout,
                     double *dsout, void *stream) {
    XM_TRY
    xm::launch_retract(o, (int)n, 0, dR, ds, dD, dds, t, dRout, dsout, nullptr, (hipStream_t)stream, 1);
    return XM_OK;
    XM_CATCH
}



// inverse of a symmetric positive definite matrix on the device (xm_dense_la.hip; set-up step of the matrix-free storage)
int xm_spd_inverse(int64_t n, double *A) {
    XM_TRY
    require_device();
    if (n < 1 || n > 46000 || !A) throw xm::Error(XM_ERR_ARG, "bad argument");
    xm::DevBuf<double> a, x;
    a.alloc((size_t)n * n, false); x.alloc((size_t)n * n, false);
    XM_HIP_CHECK(hipMemcpy(a.p, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
    if (!xm::spd_inverse_device((int)n, a.p, x.p, nullptr)) throw xm::Error(XM_ERR_ARG, "matrix is not positive definite");
    xm::spd_inverse_layout((int)n, x.p, a.p, n, nullptr);   // full symmetric matrix from the computed lower triangle (a is free now)
    XM_HIP_CHECK(hipDeviceSynchronize());
    XM_HIP_CHECK(hipMemcpy(A, a.p, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost));
    return XM_OK;
    XM_CATCH
}

// A^-1 B by the factorisation and substitutions of the dense Schur solver (xm_dense_la.hip)
int xm_spd_solve(int64_t n, int64_t k, const double *A, double *B) {
    XM_TRY
    require_device();
    if (n < 1 || n > 46000 || k < 1 || k > (int64_t)1 << 20 || !A || !B) throw xm::Error(XM_ERR_ARG, "bad argument");
    xm::DevBuf<double> a, x, y;
    xm::DevBuf<int> info;
    a.alloc((size_t)n * n, false); x.alloc((size_t)n * k, false); y.alloc((size_t)n * k, false); info.alloc(1);
    XM_HIP_CHECK(hipMemcpy(a.p, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
    XM_HIP_CHECK(hipMemcpy(x.p, B, (size_t)n * k * sizeof(double), hipMemcpyHostToDevice));
    xm::spd_cholesky_device((int)n, a.p, n, info.p, nullptr);
    xm::spd_substitute_device((int)n, a.p, n, x.p, y.p, n, (int)k, info.p, nullptr);
    xm::check_launch("spd_solve");
    XM_HIP_CHECK(hipDeviceSynchronize());
    int h = 0;
    XM_HIP_CHECK(hipMemcpy(&h, info.p, sizeof(int), hipMemcpyDeviceToHost));
    if (h) throw xm::Error(XM_ERR_ARG, "matrix is not positive definite");
    XM_HIP_CHECK(hipMemcpy(B, x.p, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost));
    return XM_OK;
    XM_CATCH
}

// Test export: one host function of xm_dense_la.hip on host arrays (include/xm_amd.h); everything is checked before the first device call
int xm_la_probe(xm_la_probe_t *probe) {
    XM_TRY
    const std::string w("xm_la_probe");
    if (!probe) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (probe->struct_size != sizeof(xm_la_probe_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_la_probe_t.struct_size is not sizeof(xm_la_probe_t)");
    const xm_la_probe_t p = *probe;
    const int64_t cap = XM_LA_PROBE_MAX_N;
    auto dim = [&](int64_t v, const char *what) { if (v < 1 || v > cap) throw xm::Error(XM_ERR_ARG, w + ": " + what + " outside [1, XM_LA_PROBE_MAX_N]"); };
    auto ld = [&](int64_t v, int64_t rows, const char *what) { if (v < rows || v > 2 * cap) throw xm::Error(XM_ERR_ARG, w + ": " + what + " below the rows or above 2 XM_LA_PROBE_MAX_N"); };
    auto same = [&](int64_t v, const char *what) { if (v != p.n) throw xm::Error(XM_ERR_ARG, w + ": " + what + " must be n for this operation"); };
    auto arr = [&](const double *a, const char *what) { if (!a) throw xm::Error(XM_ERR_ARG, w + ": null " + what); };
    size_t na = 0, nb = 0, nc = 0;   // doubles of A, B, C that travel
    bool a_back = false, c_back = false;
    dim(p.n, "n");
    switch (p.op) {
    case XM_LA_GEMM_SUB:
        dim(p.m, "m"); dim(p.k, "k");
        if ((p.ta | p.tb | p.lower_only) & ~1) throw xm::Error(XM_ERR_ARG, w + ": ta, tb and lower_only are 0 or 1");
        ld(p.lda, p.ta ? p.k : p.m, "lda"); ld(p.ldb, p.tb ? p.n : p.k, "ldb"); ld(p.ldc, p.m, "ldc");
        arr(p.A, "A"); arr(p.B, "B"); arr(p.C, "C");
        na = (size_t)p.lda * (p.ta ? p.m : p.k); nb = (size_t)p.ldb * (p.tb ? p.k : p.n); nc = (size_t)p.ldc * p.n; c_back = true;
        break;
    case XM_LA_CHOLESKY:
        ld(p.lda, p.n, "lda"); arr(p.A, "A");
        na = (size_t)p.lda * p.n; a_back = true;
        break;
    case XM_LA_SUBSTITUTE:
        dim(p.nrhs, "nrhs"); ld(p.lda, p.n, "lda"); ld(p.ldc, p.n, "ldc"); arr(p.A, "A"); arr(p.C, "C");
        na = (size_t)p.lda * p.n; nc = (size_t)p.ldc * p.nrhs; c_back = true;
        break;
    case XM_LA_INVERSE:
        same(p.lda, "lda"); same(p.ldc, "ldc"); arr(p.A, "A"); arr(p.C, "C");
        na = nc = (size_t)p.n * p.n; a_back = c_back = true;
        break;
    case XM_LA_LAYOUT:
        same(p.lda, "lda"); ld(p.ldc, p.n, "ldc"); arr(p.A, "A"); arr(p.C, "C");
        na = (size_t)p.n * p.n; nc = (size_t)p.ldc * p.n; c_back = true;
        break;
    case XM_LA_RANK1_SUB:
        same(p.lda, "lda"); arr(p.A, "A"); arr(p.B, "B");
        na = (size_t)p.n * p.n; nb = (size_t)p.n; a_back = true;
        break;
    default:
        throw xm::Error(XM_ERR_ARG, w + ": unknown op");
    }
    require_device();
    xm::DevBuf<double> a, b, c, y;
    xm::DevBuf<int> info;
    info.alloc(1);
    if (na) { a.alloc(na, false); XM_HIP_CHECK(hipMemcpy(a.p, p.A, na * sizeof(double), hipMemcpyHostToDevice)); }
    if (nb) { b.alloc(nb, false); XM_HIP_CHECK(hipMemcpy(b.p, p.B, nb * sizeof(double), hipMemcpyHostToDevice)); }
    if (nc) { c.alloc(nc, false); XM_HIP_CHECK(hipMemcpy(c.p, p.C, nc * sizeof(double), hipMemcpyHostToDevice)); }
    XM_HIP_CHECK(hipMemcpy(info.p, &p.info, sizeof(int), hipMemcpyHostToDevice));
    int h = p.info;
    bool info_back = false;
    switch (p.op) {
    case XM_LA_GEMM_SUB: xm::gemm_sub_device(p.m, p.n, p.k, a.p, p.lda, p.ta, b.p, p.ldb, p.tb, c.p, p.ldc, p.lower_only, nullptr); break;
    case XM_LA_CHOLESKY: xm::spd_cholesky_device(p.n, a.p, p.lda, info.p, nullptr); xm::check_launch("la_probe(cholesky)"); info_back = true; break;
    case XM_LA_SUBSTITUTE:
        y.alloc(nc);
        xm::spd_substitute_device(p.n, a.p, p.lda, c.p, y.p, p.ldc, p.nrhs, info.p, nullptr);
        xm::check_launch("la_probe(substitute)");
        info_back = true;
        break;
    case XM_LA_INVERSE: h = xm::spd_inverse_device(p.n, a.p, c.p, nullptr) ? 0 : 1; break;
    case XM_LA_LAYOUT: xm::spd_inverse_layout(p.n, a.p, c.p, p.ldc, nullptr); break;
    case XM_LA_RANK1_SUB: xm::rank1_sub_device(p.n, a.p, b.p, p.q, nullptr); break;
    }
    XM_HIP_CHECK(hipDeviceSynchronize());
    if (info_back) XM_HIP_CHECK(hipMemcpy(&h, info.p, sizeof(int), hipMemcpyDeviceToHost));
    if (a_back) XM_HIP_CHECK(hipMemcpy(p.A, a.p, na * sizeof(double), hipMemcpyDeviceToHost));
    if (c_back) XM_HIP_CHECK(hipMemcpy(p.C, c.p, nc * sizeof(double), hipMemcpyDeviceToHost));
    probe->info = h;
    return XM_OK;
    XM_CATCH
}

int xm_symv_plan(int64_t n, int32_t plan[4]) {
    XM_TRY
    if (n < 1 || !plan) throw xm::Error(XM_ERR_ARG, "bad argument");
    int out[4];
    xm::symv_plan_get((int)n, xm::dense_ld(n), out);   // host only: no device needed
    for (int i = 0; i < 4; ++i) plan[i] = out[i];
    return XM_OK;
    XM_CATCH
}

// ---- sliced-ELL product for large block-sparse Q (xm_sell.h) -------------------------------------------------------------
int xm_sell_layout(const int64_t *rowptr, const int32_t *colidx, int64_t n, int64_t ncols, int slabs, int lmax, int64_t sizes[5],
                   int64_t *slice_off, int32_t *slab_start, uint8_t *kind, int64_t *src, int32_t *pslot, int64_t *pptr, int32_t *ridx) {
    XM_TRY
    xm::SellHost h;
    xm::sell_build_host(rowptr, colidx, n, ncols, slabs, lmax, h);   // host only: no device needed
    if (sizes) { sizes[0] = h.nslices; sizes[1] = h.nsteps; sizes[2] = h.nparts; sizes[3] = h.nvrows; sizes[4] = h.nstore; }
    if (slice_off) std::copy(h.slice_off.begin(), h.slice_off.end(), slice_off);
    if (slab_start) std::copy(h.slab_start.begin(), h.slab_start.end(), slab_start);
    if (kind) std::copy(h.kind.begin(), h.kind.end(), kind);
    if (src) std::copy(h.src.begin(), h.src.end(), src);
    if (pslot) std::copy(h.pslot.begin(), h.pslot.end(), pslot);
    if (pptr) std::copy(h.pptr.begin(), h.pptr.end(), pptr);
    if (ridx) std::copy(h.ridx.begin(), h.ridx.begin() + h.nparts, ridx);
    return XM_OK;
    XM_CATCH
}
// host-only: the column-locality figures behind the automatic choice of xm_tuning_t.sell_wpad (SellHost::lines_*):
// lines[0..2] = distinct 128-byte lines of W per sampled step at the native pitch of 72-byte records, of 120-byte records, at the 128-byte pitch
int xm_sell_locality(const int64_t *rowptr, const int32_t *colidx, int64_t n, int64_t ncols, int slabs, int lmax, int64_t lines[3]) {
    XM_TRY
    if (!lines) throw xm::Error(XM_ERR_ARG, "null output");
    xm::SellHost h;
    xm::sell_build_host(rowptr, colidx, n, ncols, slabs, lmax, h);
    lines[0] = h.lines_native72; lines[1] = h.lines_native120; lines[2] = h.lines_padded;
    return XM_OK;
    XM_CATCH
}
// which transport joins the ranks of this context: 0 none (one GPU) | 1 RCCL | 2 shared-memory test transport | 3 direct peer writes between the
// host threads of this process | 4 direct peer writes between processes (IPC); note = why a faster transport was given up (empty: it was not)
int xm_ctx_transport(xm_ctx_t *ctx, int *kind, char *note, size_t note_cap) {
    XM_TRY
    if (!ctx || (!ctx->impl && !ctx->team)) throw xm::Error(XM_ERR_ARG, "null context");
    const int k = ctx->team ? ctx->team->comm_kind() : ctx->impl->comm_kind();
    const std::string &n = ctx->team ? ctx->team->fallback_note() : ctx->impl->fallback_note();
    if (kind) *kind = k;
    if (note && note_cap > 0) { std::strncpy(note, n.c_str(), note_cap - 1); note[note_cap - 1] = 0; }
    return XM_OK;
    XM_CATCH
}

int xm_ctx_product_kind(xm_ctx_t *ctx, int o, int *kind) {
    XM_TRY
    if (!ctx || (!ctx->impl && !ctx->team) || !kind) throw xm::Error(XM_ERR_ARG, "null argument");
    *kind = ctx->team ? ctx->team->product_kind(o) : ctx->impl->product_kind(o);
    return XM_OK;
    XM_CATCH
}

// 1 when the tCG of the last solved rank kept its product input at the 128-byte record pitch as well (xm_tuning_t.sell_wpad); 0 otherwise / several GPUs
int xm_ctx_sell_wpad(xm_ctx_t *ctx, int *on) {
    XM_TRY
    if (!ctx || (!ctx->impl && !ctx->team) || !on) throw xm::Error(XM_ERR_ARG, "null argument");
    *on = (ctx->impl && ctx->impl->sell_wpad_on()) ? 1 : 0;
    return XM_OK;
    XM_CATCH
}

int xm_sell_create2(const int64_t *rowptr, const int32_t *colidx, const double *blocks, int64_t n, int64_t ncols, int slabs, int lmax,
                    int codec, int64_t row0, void **handle) {
    XM_TRY
    require_device();
    if (!rowptr || !handle || n < 1 || row0 < 0) throw xm::Error(XM_ERR_ARG, "bad argument");
    *handle = new xm::SellMatrix(rowptr, colidx, blocks, n, ncols, slabs, lmax > 0 ? lmax : 64, nullptr, codec, row0);
    return XM_OK;
    XM_CATCH
}
int xm_sell_create(const int64_t *rowptr, const int32_t *colidx, const double *blocks, int64_t n, int64_t ncols, int slabs, int lmax,
                   void **handle) {
    return xm_sell_create2(rowptr, colidx, blocks, n, ncols, slabs, lmax, 0, 0, handle);
}
int xm_sell_quat_roundtrip(const double block[9], double quat[4], double rebuilt[9]) {
    XM_TRY
    if (!block || !quat || !rebuilt) throw xm::Error(XM_ERR_ARG, "null argument");
    xm::sell_quat_roundtrip(block, quat, rebuilt);
    return XM_OK;
    XM_CATCH
}
void xm_sell_destroy(void *handle) { delete static_cast<xm::SellMatrix *>(handle); }
int xm_qw_sell_padded(void *handle, int o, const double *dW, const double *dWpad16, double *dOut, double alpha, int gather_mode, void *stream) {
    XM_TRY
    if (!handle) throw xm::Error(XM_ERR_ARG, "null handle");
    if (gather_mode != 0 && gather_mode != 1) throw xm::Error(XM_ERR_ARG, "gather_mode must be 0 or 1");
    xm::SellMatrix &m = *static_cast<xm::SellMatrix *>(handle);
    xm::launch_qw_sell(o, xm::EPI_PLAIN, m, dW, alpha, plain_args(m.nloc(), dOut), gather_mode, (hipStream_t)stream, dWpad16);
    return XM_OK;
    XM_CATCH
}
int xm_qw_sell(void *handle, int o, const double *dW, double *dOut, double alpha, int gather_mode, void *stream) {
    return xm_qw_sell_padded(handle, o, dW, nullptr, dOut, alpha, gather_mode, stream);
}

// symmetric r x r eigen-decomposition (cyclic Jacobi), ascending; V columns = eigenvectors (col-major)
static void jacobi_eig(int r, std::vector<double> &A, std::vector<double> &V, std::vector<double> &w) {
    V.assign((size_t)r * r, 0.0);
    for (int i = 0; i < r; ++i) V[i + (size_t)i * r] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < r; ++p) for (int q = p + 1; q < r; ++q) off += A[p + (size_t)q * r] * A[p + (size_t)q * r];
        if (off < 1e-300) break;
        for (int p = 0; p < r; ++p)
            for (int q = p + 1; q < r; ++q) {
                const double apq = A[p + (size_t)q * r];
                if (apq == 0.0) continue;
                const double theta = (A[q + (size_t)q * r] - A[p + (size_t)p * r]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < r; ++k) {
                    const double akp = A[k + (size_t)p * r], akq = A[k + (size_t)q * r];
                    A[k + (size_t)p * r] = c * akp - sn * akq; A[k + (size_t)q * r] = sn * akp + c * akq;
                }
                for (int k = 0; k < r; ++k) {
                    const double apk = A[p + (size_t)k * r], aqk = A[q + (size_t)k * r];
                    A[p + (size_t)k * r] = c * apk - sn * aqk; A[q + (size_t)k * r] = sn * apk + c * aqk;
                }
                for (int k = 0; k < r; ++k) {
                    const double vkp = V[k + (size_t)p * r], vkq = V[k + (size_t)q * r];
                    V[k + (size_t)p * r] = c * vkp - sn * vkq; V[k + (size_t)q * r] = sn * vkp + c * vkq;
                }
            }
    }
    w.resize((size_t)r);
    for (int i = 0; i < r; ++i) w[(size_t)i] = A[i + (size_t)i * r];
}

}  // extern "C"
// variant: kernel form of the per-camera projection (launch_recover_project); reps > 0 and ms_avg: that launch timed with HIP events
void xm::recover_rotations(int64_t n, int r, const double *R, const double *s, double *rot, double *scale, int *n_negative_det, int variant,
                           int reps, double *ms_avg) {
    require_device();
    if (n < 1 || r < 3 || r > 16 || !R || !s || !rot || !scale || variant < 0 || variant > 1) throw xm::Error(XM_ERR_ARG, "bad argument");
    const int64_t m = 3 * n;
    xm::DevBuf<double> dR, ds, dV, drot, dscale, dparts;
    xm::DevBuf<int> dneg;
    dR.alloc((size_t)m * r, false); ds.alloc((size_t)n, false); dV.alloc((size_t)r * 3); drot.alloc((size_t)9 * n, false);
    dscale.alloc((size_t)n, false); dneg.alloc(1);
    XM_HIP_CHECK(hipMemcpy(dR.p, R, (size_t)m * r * sizeof(double), hipMemcpyHostToDevice));
    XM_HIP_CHECK(hipMemcpy(ds.p, s, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double> V((size_t)r * 3, 0.0);
    if (r == 3) {
        V[0] = V[4] = V[8] = 1.0;
    } else {
        // top-3 eigenvectors of the r x r Gram matrix sR^T sR == top-3 right singular vectors of sR; sR*V spans the same
        // rank-3 factor as the reference's eigh of the 3n x 3n matrix sR sR^T (recoversolution.py:12-24) up to a 3x3 orthogonal
        // gauge, which the anchoring removes.
        const int grid = xm::flat_grid(m);
        dparts.alloc((size_t)grid * r * r);
        xm::launch_recover_gram(n, r, dR.p, ds.p, dparts.p, grid, nullptr);
        std::vector<double> parts((size_t)grid * r * r), G((size_t)r * r, 0.0), Ev, w;
        XM_HIP_CHECK(hipMemcpy(parts.data(), dparts.p, parts.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int b = 0; b < grid; ++b) for (int e = 0; e < r * r; ++e) G[(size_t)e] += parts[(size_t)b * r * r + e];
        jacobi_eig(r, G, Ev, w);
        std::vector<int> idx((size_t)r);
        for (int i = 0; i < r; ++i) idx[(size_t)i] = i;
        std::sort(idx.begin(), idx.end(), [&](int a, int b) { return w[(size_t)a] > w[(size_t)b]; });
        for (int c = 0; c < 3; ++c) for (int k = 0; k < r; ++k) V[k + (size_t)c * r] = Ev[k + (size_t)idx[(size_t)c] * r];
    }
    XM_HIP_CHECK(hipMemcpy(dV.p, V.data(), V.size() * sizeof(double), hipMemcpyHostToDevice));
    xm::launch_recover_project(n, r, dR.p, ds.p, dV.p, drot.p, dscale.p, dneg.p, nullptr, variant);
    if (reps > 0 && ms_avg) {
        hipEvent_t e0, e1;
        XM_HIP_CHECK(hipEventCreate(&e0)); XM_HIP_CHECK(hipEventCreate(&e1));
        XM_HIP_CHECK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < reps; ++i) {
            XM_HIP_CHECK(hipMemsetAsync(dneg.p, 0, sizeof(int), nullptr));
            xm::launch_recover_project(n, r, dR.p, ds.p, dV.p, drot.p, dscale.p, dneg.p, nullptr, variant);
        }
        XM_HIP_CHECK(hipEventRecord(e1, nullptr));
        XM_HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        XM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        *ms_avg = (double)ms / reps;
    }
    int neg = 0;
    XM_HIP_CHECK(hipMemcpy(&neg, dneg.p, sizeof(int), hipMemcpyDeviceToHost));
    if (2 * (int64_t)neg > n) xm::launch_negate(drot.p, 9 * n, nullptr);   // recoversolution.py:60-62 (polar(-M) = -polar(M))
    XM_HIP_CHECK(hipMemcpy(rot, drot.p, (size_t)9 * n * sizeof(double), hipMemcpyDeviceToHost));
    XM_HIP_CHECK(hipMemcpy(scale, dscale.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (n_negative_det) *n_negative_det = neg;
}
extern "C" {
int xm_recover_rotations(int64_t n, int r, const double *R, const double *s, double *rot, double *scale, int *n_negative_det) {
    XM_TRY
    xm::recover_rotations(n, r, R, s, rot, scale, n_negative_det, 0, 0, nullptr);
    return XM_OK;
    XM_CATCH
}

int xm_ctx_edge_residuals_recovered(xm_ctx_t *ctx, const double *rot, const double *scale, double *res) {
    XM_TRY
    if (!ctx) throw xm::Error(XM_ERR_ARG, "null argument");
    if (ctx->team) ctx->team->edge_residuals_recovered(rot, scale, res); else ctx->impl->edge_residuals_recovered(rot, scale, res);
    return XM_OK;
    XM_CATCH
}
int xm_ctx_xm2_filter(xm_ctx_t *ctx, const double *rot, const double *scale, double percentile, double *threshold, int64_t *removed, double *w_out) {
    XM_TRY
    if (!ctx) throw xm::Error(XM_ERR_ARG, "null argument");
    const double thr = ctx->team ? ctx->team->xm2_filter(rot, scale, percentile, removed, w_out) : ctx->impl->xm2_filter(rot, scale, percentile, removed, w_out);
    if (threshold) *threshold = thr;
    return XM_OK;
    XM_CATCH
}
int xm_ctx_xm2_round(xm_ctx_t *ctx, const double *R, const double *s, int r, const xm_options_t *opt, xm_xm2_info_t *info, xm_result_t *res) {
    XM_TRY
    if (!ctx || !R || !s || !opt || !info || !res) throw xm::Error(XM_ERR_ARG, "null argument");
    // a multi-GPU context fans every step out to its ranks (each evaluates the filter itself: identical numbers, no exchange)
    auto solve_ctx = [&](const xm_options_t &o_, xm_result_t &r_) { if (ctx->team) ctx->team->solve(o_, r_); else ctx->impl->solve(o_, r_); };
    xm_options_t op = take_struct(opt, "xm_options_t");
    xm_result_t rs = take_struct(res, "xm_result_t");
    xm_xm2_info_t inf = take_struct(info, "xm_xm2_info_t");
    const uint32_t caller_res = res->struct_size, caller_inf = info->struct_size;
    const int64_t n = ctx->team ? ctx->team->cameras() : ctx->impl->cameras();
    // recover_XM's rotations and scales of the starting solution (utils/recoversolution.py:12-86)
    std::vector<double> rot((size_t)9 * n), scale((size_t)n);
    int neg = 0;
    if (xm_recover_rotations(n, r, R, s, rot.data(), scale.data(), &neg) != XM_OK) throw xm::Error(XM_ERR_HIP, g_err);
    const double pct = (inf.percentile > 0.0) ? inf.percentile : 90.0;
    inf.threshold = ctx->team ? ctx->team->xm2_filter(rot.data(), scale.data(), pct, &inf.removed, nullptr)
                              : ctx->impl->xm2_filter(rot.data(), scale.data(), pct, &inf.removed, nullptr);
    int64_t kept = 0;
    for (double w : (ctx->team ? ctx->team->weights() : ctx->impl->weights())) kept += (w != 0.0);
    // second pass: rank-3 solve without regulariser, then decide on lam from the spread of its scales (3_test_colmap_glomap.py:339-351)
    std::vector<double> R3((size_t)3 * n * 4, 0.0), s3((size_t)n, 1.0);
    xm_options_t o3 = op;
    o3.mode = XM_MODE_RANK3; o3.lam = 0.0; o3.max_rank = 3; o3.flags &= ~XM_FLAG_WARM_R; o3.R_ini = nullptr; o3.s_ini = nullptr; o3.trace = nullptr; o3.trace_cap = 0;
    xm_result_t r3;
    std::memset(&r3, 0, sizeof(r3));
    r3.R = R3.data(); r3.s = s3.data();
    solve_ctx(o3, r3);
    inf.rank3_status = r3.status; inf.rank3_tcg_iters = r3.tcg_iters;
    double mean = 0.0, var = 0.0;
    int64_t small = 0;
    for (int64_t i = 1; i < n; ++i) mean += s3[(size_t)i];
    mean = (n > 1) ? mean / (double)(n - 1) : 1.0;
    for (int64_t i = 1; i < n; ++i) var += (s3[(size_t)i] - mean) * (s3[(size_t)i] - mean);
    const double sd = (n > 1) ? std::sqrt(var / (double)(n - 1)) : 0.0;   // numpy.std: population standard deviation
    for (int64_t i = 0; i < n; ++i) small += (s3[(size_t)i] < 0.1);
    inf.s_avg = mean; inf.s_std = sd; inf.n_small = small;
    inf.regularised = (std::fabs(mean - 1.0) > 2.0 * sd || small > 10) ? 1 : 0;
    inf.lam_used = inf.regularised ? (double)kept / (double)n : 0.0;
    xm_options_t of = op;
    of.lam = inf.lam_used;
    if (op.flags & XM_FLAG_WARM_R) { of.mode = XM_MODE_REBUTTLE; of.R_ini = R3.data(); of.s_ini = s3.data(); }
    else { of.mode = XM_MODE_SOLVE; of.R_ini = nullptr; of.s_ini = nullptr; }
    solve_ctx(of, rs);
    give_result(res, rs, caller_res);
    inf.struct_size = caller_inf;
    std::memcpy(info, &inf, std::min<size_t>(caller_inf, sizeof(inf)));
    return XM_OK;
    XM_CATCH
}

int xm_comm_unique_id(unsigned char id[128]) { XM_TRY xm::comm_unique_id(id); return XM_OK; XM_CATCH }
int xm_comm_init(int rank, int world, int device, const unsigned char id[128], const char *rccl_path) {
    XM_TRY require_device(); xm::comm_init(rank, world, device, id, rccl_path); return XM_OK; XM_CATCH
}
int xm_comm_init_shm(int rank, int world, int device, const char *name, size_t bytes) {
    XM_TRY require_device(); xm::comm_init_shm(rank, world, device, name, bytes); return XM_OK; XM_CATCH
}
int xm_comm_init_ipc(int rank, int world, int device, const char *name, double spin_seconds) {
    XM_TRY require_device(); xm::comm_init_ipc(rank, world, device, name, spin_seconds); return XM_OK; XM_CATCH
}
int xm_comm_finalize(void) { XM_TRY xm::comm_finalize(); return XM_OK; XM_CATCH }
int xm_partition(int64_t n, int world, int rank, int64_t *c0, int64_t *c1) {
    if (n < 0 || world < 1 || rank < 0 || rank >= world || !c0 || !c1) { g_err = "bad argument"; return XM_ERR_ARG; }
    const int64_t per = xm::equal_range_len(n, world);
    *c0 = std::min<int64_t>(n, (int64_t)rank * per);
    *c1 = std::min<int64_t>(n, (int64_t)(rank + 1) * per);
    return XM_OK;
}

int xm_partition_blocks(int64_t n, const int64_t *rowptr, int world, int rank, int64_t *c0, int64_t *c1) {
    XM_TRY
    if (n < 0 || !rowptr || world < 1 || rank < 0 || rank >= world || !c0 || !c1) throw xm::Error(XM_ERR_ARG, "bad argument");
    std::vector<int64_t> cuts;
    xm::partition_cuts(n, world, rowptr, cuts);
    *c0 = cuts[(size_t)rank]; *c1 = cuts[(size_t)rank + 1];
    return XM_OK;
    XM_CATCH
}

}  // extern "C"

// host-only view of the multi-rank symmetric window plan (xm_symw.h) for the CPU test: geom = {T, Th, tie, t0, nsteps, nstrips, K, items};
// items: 3 ints each (strip, jb, je), NULL = only the sizes
int xm_symw_plan(int64_t ntot, int nloc, int cam0, int K, int32_t geom[8], int32_t *items) {
    XM_TRY
    xm::SymwPlan p;
    xm::symw_plan_build(ntot, nloc, cam0, K, p);
    if (geom) {
        geom[0] = p.g.T; geom[1] = p.g.Th; geom[2] = p.g.tie; geom[3] = p.g.t0; geom[4] = p.g.nsteps; geom[5] = p.g.nstrips; geom[6] = p.K;
        geom[7] = (int32_t)p.items.size();
    }
    if (items)
        for (size_t i = 0; i < p.items.size(); ++i) { items[3 * i] = p.items[i].s; items[3 * i + 1] = p.items[i].jb; items[3 * i + 2] = p.items[i].je; }
    return XM_OK;
    XM_CATCH
}
// Test export: one rank's share of the multi-rank symmetric product with every stage returned (include/xm_amd.h); everything is checked
// before the first device call.  The calls are those of Context::product_symw with the all-gather replaced by the caller's vectors.
int xm_symw_probe(xm_symw_probe_t *probe) {
    XM_TRY
    const std::string w("xm_symw_probe");
    if (!probe) throw xm::Error(XM_ERR_ARG, w + ": null argument");
    if (probe->struct_size != sizeof(xm_symw_probe_t)) throw xm::Error(XM_ERR_ARG, w + ": xm_symw_probe_t.struct_size is not sizeof(xm_symw_probe_t)");
    const xm_symw_probe_t p = *probe;
    if (!(p.o == 1 || (p.o >= 3 && p.o <= 5))) throw xm::Error(XM_ERR_ARG, w + ": o must be 1, 3, 4 or 5");
    if (p.ntot < 2 || p.ntot > XM_SYMW_PROBE_MAX_NTOT || (p.ntot & 1)) throw xm::Error(XM_ERR_ARG, w + ": ntot must be even, in [2, XM_SYMW_PROBE_MAX_NTOT]");
    if (p.nloc < 2 || (p.nloc & 1) || p.cam0 < 0 || (p.cam0 & 1) || (int64_t)p.cam0 + p.nloc > p.ntot)
        throw xm::Error(XM_ERR_ARG, w + ": nloc and cam0 must be even, with cam0 + nloc <= ntot");
    if (p.world < 1 || (int64_t)p.world * p.nloc != p.ntot || p.cam0 % p.nloc != 0) throw xm::Error(XM_ERR_ARG, w + ": world * nloc must be ntot and cam0 a multiple of nloc");
    if (p.nt < -1 || p.nt > 1 || p.scal_status < -1 || p.scal_status > 1) throw xm::Error(XM_ERR_ARG, w + ": nt and scal_status are -1, 0 or 1");
    if (!std::isfinite(p.alpha) || !std::isfinite(p.pad_value)) throw xm::Error(XM_ERR_ARG, w + ": alpha and pad_value must be finite (a padding column is masked by x * 0)");
    if (!p.Q || !p.W || !p.cs_all) throw xm::Error(XM_ERR_ARG, w + ": null Q, W or cs_all");
    require_device();
    const int o = p.o, OP = xm::pitch_of(o), rank = p.cam0 / p.nloc;
    const int64_t ld = xm::dense_ld(p.ntot), M = (int64_t)3 * p.ntot, rows = (int64_t)3 * p.nloc;
    xm::SymwProduct sp(p.ntot, p.nloc, p.cam0, ld, nullptr, p.K);
    sp.ensure(o, p.world);
    const xm::SymwPlan &pl = sp.plan();
    int nfull = 0;
    for (const xm::SymwItem &it : pl.items)
        for (int j = it.jb; j < it.je; ++j) nfull += xm::symw_full(pl.g, pl.g.t0 + j, it.s) ? 1 : 0;
    // Q at the solver's leading dimension, W at the solver's pitch
    std::vector<double> hq((size_t)rows * (size_t)ld, p.pad_value), hw((size_t)ld * OP + 16, 0.0);
    for (int64_t r = 0; r < rows; ++r) std::copy(p.Q + (size_t)r * M, p.Q + (size_t)(r + 1) * M, hq.begin() + (size_t)r * ld);
    for (int64_t c = 0; c < M; ++c)
        for (int k = 0; k < o; ++k) hw[(size_t)c * OP + k] = p.W[(size_t)c * o + k];
    xm::DevBuf<double> Q, W, out;
    xm::DevBuf<xm::TcgScal> scal;
    Q.alloc(hq.size(), false); W.alloc(hw.size(), false); out.alloc((size_t)rows * OP);
    XM_HIP_CHECK(hipMemcpy(Q.p, hq.data(), hq.size() * sizeof(double), hipMemcpyHostToDevice));
    XM_HIP_CHECK(hipMemcpy(W.p, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice));
    if (p.scal_status >= 0) {
        xm::TcgScal hs;
        std::memset(&hs, 0, sizeof(hs));
        hs.status = p.scal_status ? 2 : 0;
        scal.alloc(1);
        XM_HIP_CHECK(hipMemcpy(scal.p, &hs, sizeof(hs), hipMemcpyHostToDevice));
    }
    const size_t nprow = xm::symw_prow_count(pl, o), npcol = xm::symw_pcol_count(pl, o), ncs = sp.csum_count(o);
    std::vector<double> nan(std::max(std::max(nprow, npcol), ncs), std::numeric_limits<double>::quiet_NaN());
    XM_HIP_CHECK(hipMemcpy(sp.prow(), nan.data(), nprow * sizeof(double), hipMemcpyHostToDevice));
    XM_HIP_CHECK(hipMemcpy(sp.pcol(), nan.data(), npcol * sizeof(double), hipMemcpyHostToDevice));
    XM_HIP_CHECK(hipMemcpy(sp.csum_all(), p.cs_all, ncs * (size_t)p.world * sizeof(double), hipMemcpyHostToDevice));
    XM_HIP_CHECK(hipMemcpy(sp.csum_all() + (size_t)rank * ncs, nan.data(), ncs * sizeof(double), hipMemcpyHostToDevice));
    const int nt = (p.nt < 0) ? (xm::symw_nt_auto(p.nloc, ld) ? 1 : 0) : p.nt;
    sp.sweep(o, Q.p, W.p, scal.p, rank, nullptr, nt);
    xm::CamArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nloc = p.nloc; a.cam0 = p.cam0; a.out = out.p;
    sp.reduce(o, xm::EPI_PLAIN, p.alpha, a, p.world, nullptr);
    XM_HIP_CHECK(hipDeviceSynchronize());
    if (p.Prow) XM_HIP_CHECK(hipMemcpy(p.Prow, sp.prow(), nprow * sizeof(double), hipMemcpyDeviceToHost));
    if (p.Pcol) XM_HIP_CHECK(hipMemcpy(p.Pcol, sp.pcol(), npcol * sizeof(double), hipMemcpyDeviceToHost));
    XM_HIP_CHECK(hipMemcpy(p.cs_all + (size_t)rank * ncs, sp.csum_all() + (size_t)rank * ncs, ncs * sizeof(double), hipMemcpyDeviceToHost));
    if (p.csum) std::copy(p.cs_all + (size_t)rank * ncs, p.cs_all + (size_t)(rank + 1) * ncs, p.csum);
    if (p.Y) {
        std::vector<double> hy((size_t)rows * OP);
        XM_HIP_CHECK(hipMemcpy(hy.data(), out.p, hy.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < rows; ++r)
            for (int k = 0; k < o; ++k) p.Y[(size_t)r * o + k] = hy[(size_t)r * OP + k];
    }
    probe->K = pl.K; probe->nt = nt; probe->nitems = (int32_t)pl.items.size(); probe->nfull = nfull;
    return XM_OK;
    XM_CATCH
}
// host-only view of the two-level preconditioner's aggregates (xm_schur.h) for the CPU test: agg_of_camera[i] = aggregate of camera i, -1 for the
// anchor camera 0
int xm_schur_aggregate_plan(int64_t n, int64_t nobs, const int32_t *cam, const int32_t *lm, int B, int32_t *agg_of_camera) {
    XM_TRY
    if (!agg_of_camera) throw xm::Error(XM_ERR_ARG, "xm_schur_aggregate_plan: null output");
    std::vector<int32_t> order;
    xm::schur_aggregate_plan(n, nobs, cam, lm, B, order);
    agg_of_camera[0] = -1;
    for (size_t k = 0; k < order.size(); ++k) agg_of_camera[order[k]] = (int32_t)(k / (size_t)B);
    return XM_OK;
    XM_CATCH
}
// host-only view of the aggregates of the bundle adjustment's preconditioners (xm_ba.h) for the CPU test
int xm_ba_aggregate_plan(int64_t n, int64_t nobs, const int32_t *cam, const int32_t *lm, const uint8_t *used, int B, int32_t *agg_of_camera) {
    XM_TRY
    if (!agg_of_camera) throw xm::Error(XM_ERR_ARG, "xm_ba_aggregate_plan: null output");
    std::vector<int32_t> order;
    xm::ba_aggregate_plan(n, nobs, cam, lm, used, B, order);
    for (int64_t i = 0; i < n; ++i) agg_of_camera[i] = -1;
    for (size_t k = 0; k < order.size(); ++k) agg_of_camera[order[k]] = (int32_t)(k / (size_t)B);
    return XM_OK;
    XM_CATCH
}
// host-only run of the solvers' LM loop (xm_lm_loop.h) over a script of points and candidates, for the CPU test
int xm_lm_replay(int max_iters, double function_tol, double gradient_tol, double parameter_tol, int nonmonotonic, int max_nonmonotonic,
                 int64_t npoints, const double *points, int64_t nsteps, const double *steps, double *mu, uint8_t *accepted, int32_t info[7],
                 double *radius) {
    XM_TRY
    if (!points || !steps || !mu || !accepted || !info || !radius) throw xm::Error(XM_ERR_ARG, "xm_lm_replay: null array");
    const xm::LmRules rules{max_iters, function_tol, gradient_tol, parameter_tol, nonmonotonic != 0, max_nonmonotonic};
    int64_t ip = 0, is = 0;
    xm::LmHooks h;
    h.linearise = [](double, bool) {};
    h.read_point = [&](xm::LmRead) {
        if (ip >= npoints) throw xm::Error(XM_ERR_ARG, "xm_lm_replay: the script has no point left");
        const double *p = points + 2 * ip++;
        return xm::LmPoint{p[0], p[1], 0.0};
    };
    h.solve = [] { return xm::LmSolve{0, 0.0}; };
    h.read_candidate = [&](double) {
        if (is >= nsteps) throw xm::Error(XM_ERR_ARG, "xm_lm_replay: the script has no step left");
        const double *s = steps + 5 * is++;
        xm::LmCandidate c{s[0], s[1], s[2], s[3]};
        c.solved = s[4] != 0.0;
        return c;
    };
    h.accept = [](bool) {};
    h.to_best = [] {};
    const xm::LmResult r = xm::lm_loop(rules, h);
    for (size_t k = 0; k < r.trace.size(); ++k) { mu[k] = r.trace[k].mu; accepted[k] = r.trace[k].accepted ? 1 : 0; }
    info[0] = r.status; info[1] = r.iters; info[2] = r.accepted; info[3] = (int32_t)ip; info[4] = (int32_t)is; info[5] = r.current; info[6] = r.returned;
    *radius = r.radius;
    return XM_OK;
    XM_CATCH
}
// block (t, u) used by row step t? (the predicate of the sweep's masks)
int xm_symw_use(int T, int t, int u) {
    xm::SymwGeom g;
    g.T = T; g.Th = (T + 1) / 2; g.tie = (T % 2 == 0) ? 1 : 0; g.t0 = 0; g.nsteps = T; g.nstrips = (6 * T + xm::kSwStrip - 1) / xm::kSwStrip;
    return xm::symw_use(g, t, u) ? 1 : 0;
}

