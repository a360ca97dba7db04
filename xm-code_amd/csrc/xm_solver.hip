// xm_solver.hip — host driver: Riemannian staircase (XM_main.cu:180-310), RTR-tCG (trustregion.h:77-724) and the
// dual certificate (checkeig.h:42-368) on top of the kernels in xm_kernels.hip.
//
// Design notes (MI355X-first, not a translation of the reference's call sequence):
//  * one Q pass per tCG iteration and ONE per outer iteration (the reference spends three: cost, gradient and a
//    redundant 2*C*sR, trustregion.h:422/467/553): cost, gradient, projection and <g,g> all come out of the
//    gradient epilogue of the candidate point, which becomes the next iterate's state when the step is accepted.
//  * the inner loop never synchronises: alpha/beta/tau and the exit tests live in a device-resident scalar block;
//    the host enqueues iterations a few ahead and watches a host-mapped progress word.
//  * all per-camera state is row-major with an odd pitch (xm_common.h) so no transposes exist (the reference does 4
//    per inner iteration, Dense/transpose.h:7-22).
#include "xm_solver.h"
#include "xm_sell.h"
#include "xm_symw.h"
#include "xm_schur.h"
#include "xm_ba.h"
#include "xm_gp.h"
#include "xm_clean.h"
#include "xm_trackfilter.h"
#include "xm_triangulate.h"
#include "xm_prune.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace xm {

using clk = std::chrono::steady_clock;
static double secs_since(clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); }

void Context::log(const char *fmt, ...) const {
    if (!verbose_ || (comm_ && comm_->rank != 0)) return;
    va_list ap;
    va_start(ap, fmt);
    vprintf(fmt, ap);
    va_end(ap);
    fflush(stdout);
}

// Host <-> device transfers of the solve path go through the context's PINNED staging buffer: a copy from / to pageable memory makes
// the runtime wait for the stream while it holds its staging lock, and with several ranks in one process (peer communicators) a
// rank that waits like that for a peer's push can keep exactly that peer from enqueuing it (seen on the virtual-device runs: both
// ranks inside download_point, one in a pageable copy behind its wait kernel, the other on the lock).  Pinned copies are plain
// enqueues; the only blocking call is hipStreamSynchronize on the context's own stream.
void Context::to_host(void *dst, const void *src_dev, size_t bytes) {
    char *d = static_cast<char *>(dst);
    const char *s = static_cast<const char *>(src_dev);
    const size_t cap = hpin_count_ * sizeof(double);
    if (cap == 0) throw Error(XM_ERR_HIP, "staging buffer missing");
    for (size_t off = 0; off < bytes; off += cap) {
        const size_t n = std::min(cap, bytes - off);
        // Peer communicators: by KERNEL into the host-mapped staging buffer.  The copy engine (or, with HSA_ENABLE_SDMA=0, the runtime's
        // shared blit queue) is ONE in-order queue per device: with several ranks of a process on one device, rank A's copy that waits
        // there for A's wait kernel blocks rank B's copy, and B's push behind it is what A's wait kernel is waiting for (8 virtual ranks
        // stalled exactly so at the all-gather after the certificate).  A kernel on the rank's own stream shares nothing.
        if (comm_->peer() && n % 4 == 0) launch_copy_words(hpin_dev_, s + off, n, st_);
        else XM_HIP_CHECK(hipMemcpyAsync(hpin_, s + off, n, hipMemcpyDeviceToHost, st_));
        XM_HIP_CHECK(hipStreamSynchronize(st_));
        std::memcpy(d + off, hpin_, n);
    }
}
void Context::to_dev(void *dst_dev, const void *src, size_t bytes) {
    char *d = static_cast<char *>(dst_dev);
    const char *s = static_cast<const char *>(src);
    const size_t cap = hpin_count_ * sizeof(double);
    if (cap == 0) throw Error(XM_ERR_HIP, "staging buffer missing");
    for (size_t off = 0; off < bytes; off += cap) {
        const size_t n = std::min(cap, bytes - off);
        std::memcpy(hpin_, s + off, n);
        if (comm_->peer() && n % 4 == 0) launch_copy_words(d + off, hpin_dev_, n, st_);
        else XM_HIP_CHECK(hipMemcpyAsync(d + off, hpin_, n, hipMemcpyHostToDevice, st_));
        XM_HIP_CHECK(hipStreamSynchronize(st_));   // the staging buffer is reused by the next transfer
    }
}
void Context::ensure_pinned(size_t doubles) {
    if (doubles <= hpin_count_) return;
    if (hpin_) (void)hipHostFree(hpin_);
    hpin_ = nullptr; hpin_dev_ = nullptr; hpin_count_ = 0;
    XM_HIP_CHECK(hipHostMalloc((void **)&hpin_, doubles * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    XM_HIP_CHECK(hipHostGetDevicePointer((void **)&hpin_dev_, hpin_, 0));
    hpin_count_ = doubles;
}

// ------------------------------------------------------------------------------------------------------------------
// construction: lay Q out on the device
// ------------------------------------------------------------------------------------------------------------------
Context::Context(const xm_problem_t &prob, std::shared_ptr<Comm> comm) {
    comm_ = comm ? std::move(comm) : default_comm();
    cfg_ = Settings::resolve(prob.tuning);
    comm_->set_exchange_fence(!cfg_.exchange_lite);   // unconditionally: the communicator may be shared, the setting must not stick from an earlier context
    try {
        init(prob);
    } catch (...) {   // a later allocation failed (e.g. the 13.5 GB slab): release what the destructor would have released
        release_raw();
        throw;
    }
}

void Context::release_raw() {
    for (auto &e : ev_pool_) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    ev_pool_.clear();
    if (ownQ_ && dQ_) (void)hipFree(dQ_);
    dQ_ = nullptr;
    if (dQ32_) (void)hipFree(dQ32_);
    dQ32_ = nullptr;
    if (hstat_) (void)hipHostFree(hstat_);
    hstat_ = nullptr;
    if (hpin_) (void)hipHostFree(hpin_);
    hpin_ = nullptr;
    if (ev_w_) (void)hipEventDestroy(ev_w_);
    if (ev_p_) (void)hipEventDestroy(ev_p_);
    ev_w_ = ev_p_ = nullptr;
    if (st2_) (void)hipStreamDestroy(st2_);
    st2_ = nullptr;
    if (st_) (void)hipStreamDestroy(st_);
    st_ = nullptr;
}

// host-side validation of a 3x3-block CSR description (O(nb)): a malformed one would become out-of-bounds device reads
static void validate_bsr(const xm_problem_t &prob) {
    if (!prob.rowptr || !prob.colidx || !prob.blocks) throw Error(XM_ERR_ARG, "BSR3 needs rowptr/colidx/blocks");
    if (prob.rowptr[0] != 0) throw Error(XM_ERR_ARG, "BSR3: rowptr[0] must be 0");
    for (int64_t r = 0; r < prob.n; ++r)
        if (prob.rowptr[r + 1] < prob.rowptr[r]) throw Error(XM_ERR_ARG, "BSR3: rowptr is not monotone");
    if (prob.nb != 0 && prob.rowptr[prob.n] != prob.nb) throw Error(XM_ERR_ARG, "BSR3: rowptr[n] != nb");
    const int64_t nb = prob.rowptr[prob.n];
    for (int64_t q = 0; q < nb; ++q)
        if (prob.colidx[q] < 0 || (int64_t)prob.colidx[q] >= prob.n) throw Error(XM_ERR_ARG, "BSR3: column index out of range");
}

// edge list validation shared by the view-graph storage and attach_edges: in range, no self edge, no unordered pair twice (two edges
// on one pair would write the same off-diagonal block from two threads while the diagonal sums count both)
static void validate_edges(int64_t n, int64_t ne, const int32_t *ei, const int32_t *ej, const char *who) {
    if (ne < 0 || (ne > 0 && (!ei || !ej))) throw Error(XM_ERR_ARG, std::string(who) + ": bad edge arrays");
    std::vector<int64_t> key((size_t)ne);
    for (int64_t e = 0; e < ne; ++e) {
        if (ei[e] < 0 || ej[e] < 0 || ei[e] >= n || ej[e] >= n || ei[e] == ej[e]) throw Error(XM_ERR_ARG, std::string(who) + ": bad edge (out of range or i == j)");
        const int64_t a = std::min(ei[e], ej[e]), b = std::max(ei[e], ej[e]);
        key[(size_t)e] = a * n + b;
    }
    std::sort(key.begin(), key.end());
    for (int64_t e = 1; e < ne; ++e)
        if (key[(size_t)e] == key[(size_t)e - 1]) throw Error(XM_ERR_ARG, std::string(who) + ": the same pair of cameras is listed twice (as (i,j) or (j,i))");
}

// Q = sum_e w_e G_e as 3x3-block CSR, rows sorted by column, a diagonal block for every camera (XM_STORAGE_VIEWGRAPH)
static void build_viewgraph_csr(int64_t n, int64_t ne, const int32_t *ei, const int32_t *ej, const double *w, const double *M,
                                std::vector<int64_t> &rowptr, std::vector<int32_t> &colidx, std::vector<double> &blocks) {
    if (ne > 0 && (!w || !M)) throw Error(XM_ERR_ARG, "view-graph storage needs edge_w and edge_M");
    validate_edges(n, ne, ei, ej, "view-graph storage");
    rowptr.assign((size_t)n + 1, 0);
    for (int64_t e = 0; e < ne; ++e) { rowptr[(size_t)ei[e] + 1]++; rowptr[(size_t)ej[e] + 1]++; }
    for (int64_t c = 0; c < n; ++c) rowptr[(size_t)c + 1] += rowptr[(size_t)c] + 1;   // + the diagonal block
    const int64_t nb = rowptr[(size_t)n];
    colidx.assign((size_t)nb, 0);
    blocks.assign((size_t)nb * 9, 0.0);
    std::vector<int64_t> fill(rowptr.begin(), rowptr.end() - 1), eidx((size_t)nb, -1);
    std::vector<uint8_t> etr((size_t)nb, 0);
    std::vector<double> dsum((size_t)n, 0.0);
    for (int64_t e = 0; e < ne; ++e) {
        const int64_t a = fill[(size_t)ei[e]]++, b = fill[(size_t)ej[e]]++;
        colidx[(size_t)a] = ej[e]; eidx[(size_t)a] = e; etr[(size_t)a] = 0;
        colidx[(size_t)b] = ei[e]; eidx[(size_t)b] = e; etr[(size_t)b] = 1;
        dsum[(size_t)ei[e]] += w[e]; dsum[(size_t)ej[e]] += w[e];   // EDGE order: what diag_write_kernel does after a re-weighting
    }
    for (int64_t c = 0; c < n; ++c) colidx[(size_t)fill[(size_t)c]] = (int32_t)c;   // the diagonal entry, sorted into place below
    std::vector<int64_t> perm;
    std::vector<int32_t> cc;
    std::vector<int64_t> ee;
    std::vector<uint8_t> tt;
    for (int64_t c = 0; c < n; ++c) {
        const int64_t a = rowptr[(size_t)c], len = rowptr[(size_t)c + 1] - a;
        perm.resize((size_t)len); cc.resize((size_t)len); ee.resize((size_t)len); tt.resize((size_t)len);
        for (int64_t k = 0; k < len; ++k) perm[(size_t)k] = a + k;
        std::sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return colidx[(size_t)x] < colidx[(size_t)y]; });
        for (int64_t k = 0; k < len; ++k) { cc[(size_t)k] = colidx[(size_t)perm[(size_t)k]]; ee[(size_t)k] = eidx[(size_t)perm[(size_t)k]]; tt[(size_t)k] = etr[(size_t)perm[(size_t)k]]; }
        for (int64_t k = 0; k < len; ++k) {
            const int64_t q = a + k;
            colidx[(size_t)q] = cc[(size_t)k];
            double *bl = blocks.data() + (size_t)q * 9;
            if (ee[(size_t)k] < 0) { bl[0] = bl[4] = bl[8] = dsum[(size_t)c]; continue; }
            const double *m = M + (size_t)ee[(size_t)k] * 9;
            const double we = w[ee[(size_t)k]];
            for (int r = 0; r < 3; ++r)
                for (int k2 = 0; k2 < 3; ++k2) bl[r * 3 + k2] = -we * (tt[(size_t)k] ? m[k2 * 3 + r] : m[r * 3 + k2]);   // Q_ij = -w M, Q_ji = Q_ij^T
        }
    }
}

// Contiguous camera ranges of a row partition: cuts[r] .. cuts[r+1] belongs to rank r.  weights == nullptr: equal ranges of
// ceil(n / world) cameras (dense rows).  weights = the rowptr of a 3x3-block CSR matrix: ranges balanced by STORED BLOCKS -- rank r
// starts at the first camera whose rowptr reaches r/world of all blocks.
// cameras per rank of the equal partition: ceil(n / world), made EVEN when there is more than one rank (the symmetric window product of a
// multi-rank dense run works in steps of two cameras, xm_symw.h); the last rank takes the remainder, padding stays at the end
int64_t equal_range_len(int64_t n, int world) {
    int64_t per = (n + world - 1) / std::max(world, 1);
    if (world > 1 && (per & 1)) ++per;
    return per;
}
void partition_cuts(int64_t n, int world, const int64_t *weights, std::vector<int64_t> &cuts) {
    cuts.assign((size_t)world + 1, 0);
    const int64_t per = equal_range_len(n, world);
    for (int r = 0; r <= world; ++r) cuts[(size_t)r] = std::min<int64_t>(n, (int64_t)r * per);
    if (weights && world > 1) {
        const int64_t nb = weights[n] - weights[0];
        int64_t c = 0;
        for (int r = 1; r < world; ++r) {
            const int64_t target = weights[0] + (nb * r) / world;
            while (c < n && weights[c] < target) ++c;
            cuts[(size_t)r] = c;
        }
        cuts[(size_t)world] = n;
    }
}

// position of global camera g in the padded numbering (rank r's cameras start at r * nloc_)
int64_t Context::pos_of(int64_t g) const {
    int r = (int)std::min<int64_t>((int64_t)cam_cut_.size() - 2, g / std::max<int64_t>(1, nloc_));
    while (r > 0 && cam_cut_[(size_t)r] > g) --r;
    while (r + 2 < (int)cam_cut_.size() && cam_cut_[(size_t)r + 1] <= g) ++r;
    return (int64_t)r * nloc_ + (g - cam_cut_[(size_t)r]);
}

void Context::init(const xm_problem_t &prob_in) {
    const int world = comm_->world, rank = comm_->rank;
    xm_problem_t prob = prob_in;
    if (prob.n < 1) throw Error(XM_ERR_ARG, "n must be >= 1");
    if (3 * prob.n > 2000000000LL) throw Error(XM_ERR_ARG, "n too large");
    n_ = prob.n;
    storage_ = prob.storage;
    schur_dense_ = false;
    if (cfg_.schur_dense_q && storage_ == XM_STORAGE_SCHUR) {   // the dense Q built on the device from the observation list (xm_schur_dense.hip)
        if (cfg_.schur_solver == 2 || cfg_.schur_solver == 3)
            throw Error(XM_ERR_ARG, "xm_tuning_t.schur_dense_q needs the dense inverse of the reduced camera Laplacian (schur_solver 0 or 1, not the CG forms)");
        if (world > 1 || comm_->active()) throw Error(XM_ERR_ARG, "xm_tuning_t.schur_dense_q needs a single-rank context (no communicator, n_gpus <= 1)");
        if (n_ > kSchurDenseQMaxCams || n_ > cfg_.schur_dense_max)
            throw Error(XM_ERR_ARG, "xm_tuning_t.schur_dense_q: more than " + std::to_string(std::min<int64_t>(kSchurDenseQMaxCams, cfg_.schur_dense_max)) + " cameras");
        schur_dense_ = true;
    }
    if (cfg_.hess_f32) {   // (before anything is allocated)
        if (storage_ != XM_STORAGE_DENSE && !schur_dense_) throw Error(XM_ERR_ARG, "xm_tuning_t.hess_f32 needs XM_STORAGE_DENSE (storage " + std::to_string(storage_) + ")");
        if (world > 1 || comm_->active()) throw Error(XM_ERR_ARG, "xm_tuning_t.hess_f32 needs a single-rank context (no communicator, n_gpus <= 1)");
    }
    XM_HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));

    // view-graph storage: the edge list becomes 3x3-block CSR on the host (and is attached for the XM^2 calls further down)
    std::vector<int64_t> vg_rp; std::vector<int32_t> vg_ci; std::vector<double> vg_bl;
    const bool viewgraph = (storage_ == XM_STORAGE_VIEWGRAPH);
    if (viewgraph) {
        build_viewgraph_csr(n_, prob.ne, prob.edge_i, prob.edge_j, prob.edge_w, prob.edge_M, vg_rp, vg_ci, vg_bl);
        prob.rowptr = vg_rp.data(); prob.colidx = vg_ci.data(); prob.blocks = vg_bl.data(); prob.nb = vg_rp[(size_t)n_];
        storage_ = XM_STORAGE_BSR3;
    }
    if (storage_ == XM_STORAGE_BSR3 || storage_ == XM_STORAGE_BSR3_DENSE) validate_bsr(prob);

    // ---- row partition: contiguous camera ranges.  Dense rows: equal ranges.  Block-sparse: ranges balanced by STORED BLOCKS
    //  unless Settings.balance == 1 -- a hub-camera graph would otherwise land most of the matrix on one rank.  Every rank
    // is padded to the longest range with inert cameras (zero rows of Q, R = [I 0], s = 1: exact zeros in every sum), so all ranks
    // exchange equal chunks; a camera's record sits at position rank * nloc_ + (g - cut[rank]) of every replicated vector.
    partition_cuts(n_, world, (storage_ == XM_STORAGE_BSR3 && cfg_.balance == 0) ? prob.rowptr : nullptr, cam_cut_);
    int64_t longest = 1;
    for (int r = 0; r < world; ++r) longest = std::max(longest, cam_cut_[(size_t)r + 1] - cam_cut_[(size_t)r]);
    if (world > 1 && !((storage_ == XM_STORAGE_BSR3) && cfg_.balance == 0)) longest = std::max(longest, equal_range_len(n_, world));   // (a last rank with few cameras)
    nloc_ = (int)longest;
    cam0_ = rank * nloc_;
    g0_ = cam_cut_[(size_t)rank];
    ntot_ = (int64_t)nloc_ * world;
    ld_ = dense_ld(ntot_);
    const int64_t true_loc = cam_cut_[(size_t)rank + 1] - g0_;  // real cameras on this rank
    true_loc_ = true_loc;
    comm_->reserve((size_t)ld_ * (kMaxRank + 1) + 4096);   // staging of the largest all-gather (W at the top rank); collective

    if (storage_ == XM_STORAGE_DENSE) {
        if (prob.q_on_device) {
            dQ_ = const_cast<double *>(prob.q);
            ownQ_ = false;
        } else {
            // q may hold the whole matrix (q_row0 == 0, ldq >= 3n) or just a row strip that covers this rank's cameras
            const int64_t need0 = 3 * g0_, need1 = 3 * (g0_ + true_loc);
            if (!prob.q || prob.q_row0 < 0 || (true_loc > 0 && (prob.q_row0 > need0 || prob.q_row0 + prob.ldq < need1)))
                throw Error(XM_ERR_ARG, "dense Q needs q with the rows of this rank's cameras (ldq >= 3n for the whole matrix)");
            const size_t rows = (size_t)3 * nloc_;
            XM_HIP_CHECK(hipMalloc((void **)&dQ_, rows * (size_t)ld_ * sizeof(double)));
            ownQ_ = true;
            XM_HIP_CHECK(hipMemsetAsync(dQ_, 0, rows * (size_t)ld_ * sizeof(double), st_));
            if (true_loc > 0) {
                // rows [3 g0, 3 g0 + 3 true_loc) of the column-major host matrix, all 3n columns -> device slab
                // (column-major, leading dim = local rows), then an LDS-tiled transpose into the padded row-major layout.
                const int64_t lr = 3 * true_loc, cols = 3 * n_;
                DevBuf<double> slab;
                slab.alloc((size_t)lr * cols, false);
                XM_HIP_CHECK(hipMemcpy2D(slab.p, (size_t)lr * sizeof(double), prob.q + (3 * g0_ - prob.q_row0), (size_t)prob.ldq * sizeof(double),
                                         (size_t)lr * sizeof(double), (size_t)cols, hipMemcpyHostToDevice));
                launch_transpose_pad(slab.p, lr, lr, cols, dQ_, ld_, st_);
                XM_HIP_CHECK(hipStreamSynchronize(st_));
            }
        }
    } else if (storage_ == XM_STORAGE_BSR3_DENSE) {
        // described as 3x3-block CSR on the host, stored dense (the reference's format) on the device: every rank expands
        // only its own camera rows, so a 13.5 GB Q never exists on the host or on one GPU of a multi-GPU run
        const size_t rows = (size_t)3 * nloc_;
        XM_HIP_CHECK(hipMalloc((void **)&dQ_, rows * (size_t)ld_ * sizeof(double)));
        ownQ_ = true;
        XM_HIP_CHECK(hipMemsetAsync(dQ_, 0, rows * (size_t)ld_ * sizeof(double), st_));
        if (true_loc > 0) {
            const int64_t b0 = prob.rowptr[g0_], b1 = prob.rowptr[g0_ + true_loc];
            std::vector<int64_t> rp((size_t)true_loc + 1);
            for (int64_t i = 0; i <= true_loc; ++i) rp[(size_t)i] = prob.rowptr[g0_ + i] - b0;
            DevBuf<int64_t> drp; DevBuf<int32_t> dci; DevBuf<double> dbl;
            drp.alloc(rp.size(), false); dci.alloc((size_t)std::max<int64_t>(b1 - b0, 1), false); dbl.alloc((size_t)std::max<int64_t>(b1 - b0, 1) * 9, false);
            XM_HIP_CHECK(hipMemcpy(drp.p, rp.data(), rp.size() * sizeof(int64_t), hipMemcpyHostToDevice));
            if (b1 > b0) {
                XM_HIP_CHECK(hipMemcpy(dci.p, prob.colidx + b0, (size_t)(b1 - b0) * sizeof(int32_t), hipMemcpyHostToDevice));
                XM_HIP_CHECK(hipMemcpy(dbl.p, prob.blocks + b0 * 9, (size_t)(b1 - b0) * 9 * sizeof(double), hipMemcpyHostToDevice));
            }
            launch_dense_from_bsr(drp.p, dci.p, dbl.p, true_loc, 0, dQ_, ld_, st_);
        }
        XM_HIP_CHECK(hipStreamSynchronize(st_));
        storage_ = XM_STORAGE_DENSE;
    } else if (storage_ == XM_STORAGE_BSR3) {
        std::vector<int64_t> rp((size_t)nloc_ + 1, 0);
        const int64_t b0 = (true_loc > 0) ? prob.rowptr[g0_] : 0;
        for (int64_t i = 0; i <= nloc_; ++i) rp[(size_t)i] = ((true_loc > 0) ? prob.rowptr[g0_ + std::min<int64_t>(i, true_loc)] : 0) - b0;
        nb_loc_ = rp[(size_t)nloc_];
        // column indices in the padded numbering (identity for equal ranges, whose only padding is at the end)
        std::vector<int32_t> ci((size_t)std::max<int64_t>(nb_loc_, 1), 0);
        for (int64_t q = 0; q < nb_loc_; ++q) ci[(size_t)q] = (int32_t)pos_of(prob.colidx[b0 + q]);
        rowptr_.alloc((size_t)nloc_ + 1);
        colidx_.alloc((size_t)std::max<int64_t>(nb_loc_, 1));
        blocks_.alloc((size_t)std::max<int64_t>(nb_loc_, 1) * 9);
        XM_HIP_CHECK(hipMemcpy(rowptr_.p, rp.data(), rp.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        {
            std::vector<int4> ri;
            bsr_build_rowinfo(rp.data(), nloc_, ri);
            rowinfo_.alloc(std::max<size_t>(ri.size(), 1));
            if (!ri.empty()) XM_HIP_CHECK(hipMemcpy(rowinfo_.p, ri.data(), ri.size() * sizeof(int4), hipMemcpyHostToDevice));
        }
        if (nb_loc_ > 0) {
            XM_HIP_CHECK(hipMemcpy(colidx_.p, ci.data(), (size_t)nb_loc_ * sizeof(int32_t), hipMemcpyHostToDevice));
            XM_HIP_CHECK(hipMemcpy(blocks_.p, prob.blocks + b0 * 9, (size_t)nb_loc_ * 9 * sizeof(double), hipMemcpyHostToDevice));
        }
        // Large problems: sliced-ELL over per-XCD column slabs (xm_sell.h).  Below ~2.2 M blocks per GPU the one-launch CSR kernel wins --
        // measured (profiles/r06_kbench_bsr_policy.txt, o = 3, us; the CSR kernel reads its blocks with the default cache policy at these sizes):
        // 1.39 M blocks CSR 31.5 / sliced ELL 39.3, 2.05 M blocks 49.3 / 52.2, 2.79 M blocks 72.4 / 66.1 (round 5, non-temporal blocks:
        // 425 k 13.2 / 23.0, 929 k 25.5 / 32.0, 2.05 M 53.1 / 46.8); inside the solve at 425 k blocks
        // (Hessian epilogue, HIP events) 20.4 / 28.9 and 22.4 k / 18.3 k tCG iterations per second (r05_bench_rome_bsr*.json).  View-graph storage compresses the
        // stream with the quaternion codec (36 instead of 76 bytes per stored block).  Settings: sell, sell_slabs, sell_lmax,
        // sell_gather, sell_codec (xm_tuning_t).
        if (cfg_.sell == 1 || (cfg_.sell == 0 && nb_loc_ >= kSellMinBlocks)) {
            sell_gm_ = cfg_.sell_gather;
            const int codec = (cfg_.sell_codec == 2 || (cfg_.sell_codec == 0 && viewgraph)) ? SELL_CODEC_QUAT : SELL_CODEC_FULL;
            // layout: sorted virtual rows + a second launch for the per-camera sum (xm_sell.h).  A chunk-tiled ONE-launch layout was measured
            // in round 4 (profiles/r04_kbench_sell2.txt: 90.3 us against 82.3 us in two launches at 100 k cameras) and removed in round 5.
            sell_.reset(new SellMatrix(rp.data(), ci.data(), prob.blocks + b0 * 9, nloc_, ntot_, cfg_.sell_slabs, cfg_.sell_lmax, st_, codec, cam0_));
        }
    } else if (storage_ == XM_STORAGE_SCHUR) {
        // several ranks (round 4): every rank builds the factors from the whole observation list; the rows of VT^-1 and the cameras of the
        // last kernel of the chain are partitioned (xm_schur.h)
        SchurSettings sc;
        sc.host_assembly = cfg_.schur_host_assembly; sc.sym_min_rows = cfg_.sym_rows(1); sc.trace = cfg_.schur_trace;
        sc.solver = cfg_.schur_solver; sc.dense_max = cfg_.schur_dense_max;
        sc.pcg_first = cfg_.schur_pcg_first; sc.pcg_hess_digits = cfg_.schur_pcg_hess_digits;
        schur_.reset(new SchurOp(n_, prob.n_landmarks, prob.nobs, prob.obs_cam, prob.obs_lm, prob.obs_p, prob.obs_w, st_, comm_.get(), sc));
        w_cur_.assign(prob.obs_w, prob.obs_w + prob.nobs);
        if (schur_dense_) {   // the context keeps its SchurOp (lists, residuals, recovery, cleaning, bundle adjustment) and owns the dense Q beside it:
                              // from here on every product takes the dense dispatch
            if (schur_->names_a_pair_twice())
                throw Error(XM_ERR_ARG, "xm_tuning_t.schur_dense_q: the observation list names a (camera, landmark) pair twice (the device assembly assumes a landmark names a camera once)");
            const size_t rows = (size_t)3 * nloc_;
            XM_HIP_CHECK(hipMalloc((void **)&dQ_, rows * (size_t)ld_ * sizeof(double)));
            ownQ_ = true;
            XM_HIP_CHECK(hipMemsetAsync(dQ_, 0, rows * (size_t)ld_ * sizeof(double), st_));
            schur_->build_dense_q(dQ_, ld_, nullptr, st_);
            storage_ = XM_STORAGE_DENSE;
        }
    } else {
        throw Error(XM_ERR_ARG, "unknown storage");
    }
    // Symmetric half-traffic product: dense, Q exactly symmetric.  It pays from ~1300 cameras on (Settings::sym_rows: measured cross-over;
    // 13682 cameras 2000 -> 1110 us at o = 3, 1778 cameras 31.9 -> 25.8 us).  Settings.sym: auto = on for 3n >= sym_rows() and o <= 4; 1 forces
    // it for every size (o <= 5, 1e-9 relative asymmetry accepted); -1 disables it.  Single rank only: the kernel sweeps the upper
    // triangle of the WHOLE matrix (a rank's row strip is a rectangle).
    sym_ok_ = false;
    sym_max_o_ = 4;
    {
        const bool force = cfg_.sym == 1, off = cfg_.sym == -1;
        if (force) sym_max_o_ = 5;
        if (storage_ == XM_STORAGE_DENSE && world == 1 && !off && (force || 3 * n_ >= cfg_.sym_rows(1))) {
            const int grid = 2048;
            DevBuf<double> d;
            d.alloc((size_t)2 * grid);
            launch_asym(dQ_, ld_, 3 * n_, d.p, grid, st_);
            std::vector<double> h((size_t)2 * grid);
            XM_HIP_CHECK(hipMemcpyAsync(h.data(), d.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st_));
            XM_HIP_CHECK(hipStreamSynchronize(st_));
            double da = 0, mx = 0;
            bool nan = false;
            for (int i = 0; i < grid; ++i) {
                if (h[(size_t)i] != h[(size_t)i]) nan = true;   // a NaN entry anywhere: never symmetric
                else da = std::max(da, h[(size_t)i]);
                mx = std::max(mx, h[(size_t)grid + i]);
            }
            if (nan) da = std::nan("");
            q_asym_ = da; q_max_ = mx;
            // The lower triangle is never read on this path, so by default it is taken only for an EXACTLY symmetric matrix (what
            // utils/creatematrix.py:326-328 writes): round-off asymmetry in a Q.bin is honoured like cublasDgemm does, at every
            // size.  sym = 1 accepts |Q - Q^T| <= 1e-9 |Q| (results then differ from the general path by that much).
            sym_ok_ = force ? (da <= 1e-9 * mx) : (da == 0.0);
        }
    }
    if (cfg_.hess_f32) refresh_q32();
    // Several ranks: every rank streams half of its row strip through a cyclic half window (xm_symw.h) -- the upper triangle cut into row
    // strips would leave rank 0 with almost its whole strip.  Whether Q is symmetric cannot be seen from one strip.  The policy is the
    // single-GPU one: automatic (sym = 0) only for an EXACTLY symmetric matrix -- an order-independent checksum modulo 2^64 over the
    // strips (launch_symhash), all-gathered; forced (sym = 1) when a random vector multiplied both ways (general kernel / window
    // product) agrees to 1e-9 on every rank.
    symw_.reset();
    if (storage_ == XM_STORAGE_DENSE && world > 1 && comm_->active() && cfg_.sym != -1 && (nloc_ % 2) == 0 &&
        (cfg_.sym == 1 || 3 * n_ >= cfg_.sym_rows(world))) {
        sym_max_o_ = (cfg_.sym == 1) ? 5 : 4;
        symw_.reset(new SymwProduct(ntot_, nloc_, cam0_, ld_, st_));
        comm_->reserve(symw_csum_count(ntot_, sym_max_o_) * (size_t)world + 4096);
        symw_->ensure(sym_max_o_, world);   // once, for every rank of the staircase: no free between two collectives later on
        DevBuf<double> x, y1, y2, flag;
        x.alloc((size_t)ld_ + 16); y1.alloc((size_t)3 * nloc_); y2.alloc((size_t)3 * nloc_); flag.alloc((size_t)world);
        std::vector<double> hx((size_t)ld_, 0.0);
        unsigned long long lcg = 88172645463325252ull;
        for (int64_t i = 0; i < 3 * ntot_; ++i) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; hx[(size_t)i] = (double)(lcg >> 11) / 9007199254740992.0 - 0.5; }
        XM_HIP_CHECK(hipMemcpyAsync(x.p, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice, st_));
        CamArgs pa;
        std::memset(&pa, 0, sizeof(pa));
        pa.nloc = nloc_; pa.cam0 = cam0_;
        pa.out = y1.p;
        launch_qw_dense(1, EPI_PLAIN, dQ_, ld_, x.p, 1.0, pa, st_);
        pa.out = y2.p;
        symw_->sweep(1, dQ_, x.p, nullptr, rank, st_);
        comm_->allgather(symw_->csum_all(), symw_->csum_count(1), st_);
        symw_->reduce(1, EPI_PLAIN, 1.0, pa, world, st_);
        std::vector<double> h1((size_t)3 * nloc_), h2((size_t)3 * nloc_);
        XM_HIP_CHECK(hipMemcpyAsync(h1.data(), y1.p, h1.size() * sizeof(double), hipMemcpyDeviceToHost, st_));
        XM_HIP_CHECK(hipMemcpyAsync(h2.data(), y2.p, h2.size() * sizeof(double), hipMemcpyDeviceToHost, st_));
        XM_HIP_CHECK(hipStreamSynchronize(st_));
        double dmax = 0, ymax = 0;
        bool bad = false;
        for (size_t i = 0; i < h1.size(); ++i) {
            if (h1[i] != h1[i] || h2[i] != h2[i]) bad = true;
            dmax = std::max(dmax, std::fabs(h1[i] - h2[i])); ymax = std::max(ymax, std::fabs(h1[i]));
        }
        // the bound has to hold for the whole vector, not only for this rank's rows: every rank reports its own maxima
        std::vector<double> rep((size_t)world * 2, 0.0);
        DevBuf<double> repd;
        repd.alloc((size_t)world * 2);
        const double mine[2] = {bad ? 1e300 : dmax, ymax};
        XM_HIP_CHECK(hipMemcpyAsync(repd.p + (size_t)rank * 2, mine, sizeof(mine), hipMemcpyHostToDevice, st_));
        comm_->allgather(repd.p, 2, st_);
        XM_HIP_CHECK(hipMemcpyAsync(rep.data(), repd.p, rep.size() * sizeof(double), hipMemcpyDeviceToHost, st_));
        XM_HIP_CHECK(hipStreamSynchronize(st_));
        double dall = 0, yall = 0;
        for (int r = 0; r < world; ++r) { dall = std::max(dall, rep[(size_t)2 * r]); yall = std::max(yall, rep[(size_t)2 * r + 1]); }
        q_asym_ = dall; q_max_ = yall;
        if (!(dall <= 1e-9 * yall)) symw_.reset();   // identical decision on every rank (identical gathered numbers)
        if (symw_ && cfg_.sym != 1) {
            // automatic mode: exact symmetry, as on one GPU (there: launch_asym == 0).  The strips' checksums travel as bit patterns.
            const int grid = 1024;
            DevBuf<unsigned long long> hsh;
            hsh.alloc((size_t)2 * grid);
            launch_symhash(dQ_, ld_, 3 * (int64_t)cam0_, 3 * (int64_t)nloc_, 3 * ntot_, hsh.p, grid, st_);
            std::vector<unsigned long long> hh((size_t)2 * grid);
            XM_HIP_CHECK(hipMemcpyAsync(hh.data(), hsh.p, hh.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st_));
            XM_HIP_CHECK(hipStreamSynchronize(st_));
            unsigned long long mine2[2] = {0ull, 0ull};
            for (int b = 0; b < grid; ++b) { mine2[0] += hh[(size_t)2 * b]; mine2[1] |= hh[(size_t)2 * b + 1]; }
            static_assert(sizeof(unsigned long long) == sizeof(double), "checksums travel through the double all-gather");
            XM_HIP_CHECK(hipMemcpyAsync(repd.p + (size_t)rank * 2, mine2, sizeof(mine2), hipMemcpyHostToDevice, st_));
            comm_->allgather(repd.p, 2, st_);
            std::vector<unsigned long long> all((size_t)world * 2);
            XM_HIP_CHECK(hipMemcpyAsync(all.data(), repd.p, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st_));
            XM_HIP_CHECK(hipStreamSynchronize(st_));
            unsigned long long tot = 0ull, bad2 = 0ull;
            for (int r = 0; r < world; ++r) { tot += all[(size_t)2 * r]; bad2 |= all[(size_t)2 * r + 1]; }
            if (tot != 0ull || bad2 != 0ull) symw_.reset();   // identical on every rank
        }
        comm_->host_barrier();
    }
    XM_HIP_CHECK(hipHostMalloc((void **)&hstat_, 256, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(hstat_, 0, 256);
    XM_HIP_CHECK(hipHostGetDevicePointer((void **)&hstat_dev_, hstat_, 0));
    ensure_pinned((size_t)1 << 17);   // 1 MB to start with; setup_rank sizes it for the solve
    if (viewgraph) {
        attach_edges(prob.ne, prob.edge_i, prob.edge_j, prob.edge_M);
        w_cur_.assign(prob.edge_w, prob.edge_w + prob.ne);
    }
}

Context::~Context() { release_raw(); }

// ------------------------------------------------------------------------------------------------------------------
// per-rank workspace
// ------------------------------------------------------------------------------------------------------------------
void Context::setup_rank(int o) {
    // (Re)allocation frees device memory, and hipFree synchronises the WHOLE device.  With several ranks of one process on one device
    // (virtual devices) that would wait for a peer's wait kernel, which in turn waits for a push this rank has not enqueued yet: the
    // host barrier makes sure every rank has enqueued everything up to here before anybody frees (no-op for other communicators).
    if (comm_->active()) comm_->host_barrier();
    o_ = o;
    OP_ = pitch_of(o);
    const size_t mat = (size_t)nloc_ * 3 * OP_, vec = (size_t)nloc_;
    const int world = comm_->world;
    // grow-only workspace: sized once for the highest rank this solve can reach (the pitch grows with the rank), reused by every later
    // rank level and every later solve of the context
    const int o_top = std::max(o, (int)std::min<unsigned>(opt_ ? opt_->max_rank : 0u, (unsigned)kMaxRank));
    const size_t mat_top = (size_t)nloc_ * 3 * pitch_of(o_top);
    for (DevBuf<double> *b : {&R_, &Rc_, &D_, &rR_, &rRB_, &pR_, &pRB_, &vR_, &HvR_, &HpR_}) b->ensure(mat, st_, mat_top);
    for (DevBuf<double> *b : {&s_, &sc_, &rs_, &rsB_, &psA_, &psB_, &vs_, &Hvs_, &Hps_}) b->ensure(vec, st_);
    for (int k = 0; k < 2; ++k) {
        ps_[k].G.ensure(mat, st_, mat_top); ps_[k].rgR.ensure(mat, st_, mat_top); ps_[k].egs.ensure(vec, st_); ps_[k].rgs.ensure(vec, st_); ps_[k].S0.ensure(vec * 9, st_);
    }
    cur_ = 0;
    wpad_on_ = sell_ && cfg_.sell_wpad >= 0 && !comm_->active() && sell_supports(o) && o >= 3 && 3 * OP_ <= 16 && (cfg_.sell_wpad == 1 || sell_->padded_pays(o));
    if (wpad_on_ && !wpad_.p) wpad_.alloc((size_t)ntot_ * 16 + 16);   // zero-filled: the pad is never written
    W_.ensure((size_t)ld_ * OP_ + 16, st_, (size_t)ld_ * pitch_of(o_top) + 16);   // + slack: the sector-window gather of the sliced-ELL product reads whole 64-byte sectors around a record
    const int nA_loc = prod_grid(), nB_loc = tcg_blocks();
    nA_ = nA_loc * world;
    nB_ = nB_loc * world;
    partsA_.ensure((size_t)3 * nA_, st_);
    // tCG exchange buffers: two parity buffers of world chunks [rows of the image of Hp (multi-rank only) | 3*nA_loc | nB_loc]
    const size_t b_off = comm_->active() ? mat : 0;
    const size_t pb = (size_t)2 * (b_off * world + 3 * nA_ + nB_);
    if (comm_->peer() && world > 1 && cfg_.exchange != 1 && !symw_ && storage_ != XM_STORAGE_SCHUR && comm_->device_waits()) {   // (the window product and the matrix-free chain all-gather between their launches: lockstep loop)
        // direct peer exchange: the buffers live in memory every rank of the group can store into (collective, host-synchronised)
        partsB_.release();
        comm_->xchg_setup(pb, xchg_);
        partsB_peer_ = xchg_.buf[comm_->rank];
        xchg_.mute = (cfg_.debug_peer_mute && comm_->rank == 1) ? 1 : 0;
        xchg_.lite = cfg_.exchange_lite;
    } else {
        xchg_ = PeerXchg();
        partsB_peer_ = nullptr;
        partsB_.ensure(pb, st_, (size_t)2 * ((comm_->active() ? mat_top : 0) * world + 3 * nA_ + nB_));
    }
    if (comm_->active()) Afull_.ensure(mat * world, st_, mat_top * world); else Afull_.release();
    partsM_.ensure((size_t)std::max(std::max(nB_, flat_grid((int64_t)mat_top) * world), 4 * ((nloc_ + 255) / 256) * world), st_);   // (device-driven outer iteration: one model partial per wavefront of 64 cameras)
    // the symmetric product's workspace is made when the rank changes and kept, with the chunk plan it was made under, while it repeats: every
    // entry the reducer reads is written by the sweep in front of it, so nothing of an earlier run gets through
    if (!(sym_ok_ && o >= 3 && o <= sym_max_o_)) symv_.release();
    else if (!symv_ || symv_.nloc != nloc_ || symv_.ld != ld_ || symv_.o != o) symv_.ensure(nloc_, ld_, o);
    // column-split product for small strips (xm_kernels.hip:qw_dense_ks_kernel): multi-rank dense storage by default
    ks_ = 1;
    if (storage_ == XM_STORAGE_DENSE && !sym_ok_ && cfg_.split_k >= 0) {
        if (cfg_.split_k >= 2) ks_ = std::min(cfg_.split_k, std::max(1, (int)((ld_ + 255) / 256)));
        else if (comm_->active()) ks_ = qw_dense_split_k(nloc_, ld_);
    }
    if (ks_ > 1) {
        ksum_.alloc((size_t)ks_ * mat);
        kcount_.alloc((size_t)qw_grid(nloc_));
    }
    if (overlap_applies()) {
        if (!st2_) {
            XM_HIP_CHECK(hipStreamCreateWithFlags(&st2_, hipStreamNonBlocking));
            XM_HIP_CHECK(hipEventCreateWithFlags(&ev_w_, hipEventDisableTiming));
            XM_HIP_CHECK(hipEventCreateWithFlags(&ev_p_, hipEventDisableTiming));
        }
        Pstrip_.alloc(mat);
    }
    scal_.ensure(2, st_);
    spec_.ensure(1, st_);
    // history of the truncated CG for the replay of a rejected step: tcg_history slots of [p | Hp].  Grow-only and not zeroed: a replay reads
    // only what the steps of the rejected truncated CG wrote (hist_n_ records)
    hist_valid_ = false;
    if (replay_applies()) {
        const size_t H = (size_t)cfg_.tcg_history;
        if (hist_vec_.capacity < H * 2 * mat) hist_vec_.alloc(H * 2 * mat_top, false);
        if (hist_cam_.capacity < H * 2 * vec) hist_cam_.alloc(H * 2 * vec, false);
        if (hist_rec_.capacity < H) hist_rec_.alloc(H, false);
    }
    // the sliced-ELL product's partial-result buffer grows with o: (re)allocate it HERE, between the two barriers -- hipFree synchronises
    // the whole device, and with several ranks of one process on one device ("virtual devices") a free between two collectives waits for
    // a peer's spinning wait kernel that waits for this rank's next push (8 virtual ranks ran into exactly that at the first o = 4 product)
    if (sell_ && sell_supports(o)) (void)sell_->parts(o);
    // pinned staging: partial sums, a whole replicated point (download_point) and a Lanczos vector
    ensure_pinned(std::max<size_t>((size_t)2 * nA_ + (size_t)nB_ + partsM_.count + 64, (size_t)ld_ * OP_ + (size_t)ntot_ + 1024));
    if (comm_->active()) comm_->host_barrier();   // nobody enqueues the next collective while somebody is still freeing
}

// host column-major (true n) -> device row-major (pitch OP) rows of the local cameras; padding cameras get [I 0]
void Context::upload_point(const std::vector<double> &R_cm, int o, const std::vector<double> &s_ex) {
    const size_t m = (size_t)3 * n_;
    std::vector<double> Rr((size_t)nloc_ * 3 * OP_, 0.0), sl((size_t)nloc_, 1.0);
    for (int c = 0; c < nloc_; ++c) {
        const bool real = c < true_loc_;
        const int64_t g = g0_ + c;
        for (int a = 0; a < 3; ++a)
            for (int k = 0; k < o; ++k)
                Rr[((size_t)c * 3 + a) * OP_ + k] = real ? R_cm[(size_t)(3 * g + a) + (size_t)k * m] : (a == k ? 1.0 : 0.0);
        if (real) sl[(size_t)c] = s_ex[(size_t)g];
    }
    if (cam0_ == 0) sl[0] = 1.0;  // the anchor's scale is 1 inside the solver (trustregion.h:125-127)
    to_dev(R_.p, Rr.data(), Rr.size() * sizeof(double));
    to_dev(s_.p, sl.data(), sl.size() * sizeof(double));
}

// device -> host column-major for ALL cameras (gathers across ranks through the W buffer)
void Context::download_point(std::vector<double> &R_cm, std::vector<double> &s_ex) {
    const size_t m = (size_t)3 * n_, mat = (size_t)nloc_ * 3 * OP_;
    std::vector<double> full((size_t)ntot_ * 3 * OP_), sf((size_t)ntot_);
    // copies by KERNEL, not by the copy engine: the ranks of one process on one device share the engine's in-order queue, and a peer's
    // device-to-host copy that waits there for its wait kernel would block this copy, i.e. the push that wait kernel is waiting for
    launch_scale_copy(W_.p + (size_t)comm_->rank * mat, R_.p, 1.0, (int64_t)mat, st_);
    if (comm_->active()) comm_->allgather(W_.p, mat, st_);
    to_host(full.data(), W_.p, full.size() * sizeof(double));
    launch_scale_copy(W_.p + (size_t)comm_->rank * nloc_, s_.p, 1.0, (int64_t)nloc_, st_);
    if (comm_->active()) comm_->allgather(W_.p, (size_t)nloc_, st_);
    to_host(sf.data(), W_.p, sf.size() * sizeof(double));
    XM_HIP_CHECK(hipMemsetAsync(W_.p, 0, W_.count * sizeof(double), st_));
    R_cm.assign(m * (size_t)o_, 0.0);
    s_ex.assign((size_t)n_, 1.0);
    for (int64_t g = 0; g < n_; ++g) {
        const size_t q = (size_t)pos_of(g);
        for (int a = 0; a < 3; ++a)
            for (int k = 0; k < o_; ++k) R_cm[(size_t)(3 * g + a) + (size_t)k * m] = full[(q * 3 + a) * OP_ + k];
        s_ex[(size_t)g] = sf[q];
    }
}

// workgroups of the product kernels == number of per-workgroup partial sums per epilogue slot
int Context::prod_grid() const {
    if (storage_ == XM_STORAGE_BSR3 && sell_ && sell_supports(o_)) return sell_->reduce_grid(o_, nloc_);
    return (storage_ == XM_STORAGE_BSR3) ? bsr_grid(nloc_) : qw_grid(nloc_);   // dense and matrix-free: one wavefront per camera
}

// cg_step_kernel waits for its peers INSIDE the launch when the direct exchange is fused into it: every workgroup of every rank that
// shares this device has to be resident at once, or the resident ones wait for the others' turn for ever (until the bounded spin
// expires).  256 CUs x 4 workgroups is admitted whatever the kernel's register count (cg_step: 61 VGPRs, 106 SGPRs -> 6 per CU).
int Context::tcg_blocks() const {
    int g = flat_grid((int64_t)nloc_ * 3 * OP_);
    if (comm_->peer() && comm_->world > 1 && cfg_.exchange != 1 && !symw_ && storage_ != XM_STORAGE_SCHUR && comm_->device_waits()) g = std::min(g, std::max(8, 1024 / std::max(1, comm_->ranks_on_my_device())));
    return g;
}

CamArgs Context::cam_args(int state) const {
    CamArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nloc = nloc_;
    a.cam0 = cam0_;
    a.lam = opt_ ? opt_->lam : 0.0;
    a.R = R_.p;
    a.s = s_.p;
    const PointState &p = ps_[state];
    a.G = p.G.p; a.egs = p.egs.p; a.S0 = p.S0.p; a.rgR = p.rgR.p; a.rgs = p.rgs.p;
    a.pR = pR_.p; a.ps = psA_.p; a.rR = rR_.p; a.rs = rs_.p; a.HpR = HpR_.p; a.Hps = Hps_.p;
    a.Wloc = W_.p + (size_t)cam0_ * 3 * OP_;
    a.out = HpR_.p;
    a.partials = partsA_.p;
    a.scal = scal_.p;
    if (ks_ > 1) { a.ks = ks_; a.ksum = ksum_.p; a.kcount = kcount_.p; }
    return a;
}

void Context::product(int epi, int o, double alpha, const CamArgs &a) {
    if (w_pending_) {
        if (storage_ == XM_STORAGE_DENSE && (epi == EPI_PLAIN || epi == EPI_GRAD) && o == o_) {
            // local column strip on the second stream beside the all-gather, the rest after it
            w_pending_ = false;
            const int tc = qw_dense_tile_cols();
            const int64_t c0 = 3 * (int64_t)cam0_, c1 = 3 * ((int64_t)cam0_ + nloc_);
            CamArgs s1 = a, s2 = a;
            s1.range_mode = 1; s1.t_lo = (int)((c0 + tc - 1) / tc); s1.t_hi = (int)(c1 / tc); s1.out = Pstrip_.p; s1.addend = nullptr;
            s2.range_mode = 2; s2.t_lo = s1.t_lo; s2.t_hi = s1.t_hi; s2.addend = Pstrip_.p;
            comm_->note("overlap_split", (double)s1.t_lo, (double)s1.t_hi);
            XM_HIP_CHECK(hipEventRecord(ev_w_, st_));
            XM_HIP_CHECK(hipStreamWaitEvent(st2_, ev_w_, 0));
            launch_qw_dense_split(o, EPI_PLAIN, dQ_, ld_, W_.p, 1.0, s1, st2_);
            XM_HIP_CHECK(hipEventRecord(ev_p_, st2_));
            comm_->allgather(W_.p, (size_t)nloc_ * 3 * OP_, st_);
            XM_HIP_CHECK(hipStreamWaitEvent(st_, ev_p_, 0));
            launch_qw_dense_split(o, epi, dQ_, ld_, W_.p, alpha, s2, st_);
            if (res_) res_->qw_products++;
            return;
        }
        flush_gather();
    }
    if (storage_ == XM_STORAGE_DENSE && dQ32_ && o == o_ && (epi == EPI_HESS || epi == EPI_AUTO)) {
        // xm_tuning_t.hess_f32: the Hessian products of the tCG read the fp32 copy -- the symmetric pair wherever the f64 path takes it
        // (EPI_AUTO: the same launch computes the candidate's gradient from the f64 Q when the device-driven outer iteration asks for it)
        if (sym_ok_ && o >= 3 && o <= sym_max_o_ && symv_) launch_qw_sym_f32(o, epi, dQ32_, dQ_, ld_, W_.p, alpha, a, symv_, st_, sym_rev_);
        else { CamArgs ar = a; ar.rev = sym_rev_; launch_qw_dense_f32(o, epi, dQ32_, dQ_, ld_, W_.p, alpha, ar, st_); }
    } else if (storage_ == XM_STORAGE_DENSE) {
        if (symw_ && o == o_ && o >= 3 && o <= sym_max_o_ && epi != EPI_CERT) product_symw(epi, o, alpha, a);
        else if (sym_ok_ && o == o_ && o >= 3 && o <= sym_max_o_ && epi != EPI_CERT && symv_) launch_qw_sym(o, epi, dQ_, ld_, W_.p, alpha, a, symv_, st_, sym_rev_, fuse_step_);
        else { CamArgs ar = a; ar.rev = sym_rev_; launch_qw_dense(o, epi, dQ_, ld_, W_.p, alpha, ar, st_); }
    } else if (storage_ == XM_STORAGE_SCHUR) {
        schur_->product(o, epi, W_.p, alpha, a, st_);
    } else if (sell_ && sell_supports(o)) {
        // inside the tCG the kernels that write W keep a copy at the 128-byte record pitch (run_tcg): the gather reads that one
        const double *wp = (epi == EPI_HESS && o == o_) ? wpad() : ((epi == EPI_GRAD && o == o_) ? wpad_next_ : nullptr);
        wpad_next_ = nullptr;
        launch_qw_sell(o, epi, *sell_, W_.p, alpha, a, sell_gm_, st_, wp);
    } else {
        launch_qw_bsr3(o, epi, rowptr_.p, colidx_.p, blocks_.p, W_.p, alpha, a, st_, nb_loc_, rowinfo_.p);
    }
    if (res_) res_->qw_products++;
}

int Context::product_kind(int o) const {
    if (storage_ == XM_STORAGE_SCHUR) return XM_PRODUCT_SCHUR;
    if (storage_ == XM_STORAGE_DENSE) return ((symw_ || sym_ok_) && o >= 3 && o <= sym_max_o_) ? XM_PRODUCT_DENSE_SYM : XM_PRODUCT_DENSE;
    if (sell_ && sell_supports(o)) return sell_->codec() == SELL_CODEC_QUAT ? XM_PRODUCT_SELL_QUAT : XM_PRODUCT_SELL;
    return XM_PRODUCT_BSR3;
}

// multi-rank symmetric Q: sweep of this rank's half window, all-gather of the ranks' column sums, per-camera sum + epilogue (xm_symw.h)
void Context::product_symw(int epi, int o, double alpha, const CamArgs &a) {
    symw_->sweep(o, dQ_, W_.p, (epi == EPI_HESS) ? a.scal : (const TcgScal *)nullptr, comm_->rank, st_);
    comm_->allgather(symw_->csum_all(), symw_->csum_count(o), st_);
    symw_->reduce(o, epi, alpha, a, comm_->world, st_);
}

// "overlap the gather with the local (diagonal-strip) part of Q*W".  The rows of W this rank owns are final before the
// all-gather starts, so the column tiles of Q that lie entirely inside the rank's own column range can be multiplied on a second
// stream WHILE the collective runs; the rest of the product (all other tiles, + those raw sums, + the epilogue) follows the
// gather.  Applies to the dense products OUTSIDE the tCG (cost/gradient of a candidate point, line search, certificate right-hand
// side) — inside the tCG the product input comes from replicated data and there is no gather to hide.  It costs
// an extra launch, so it is used only when the per-rank matrix is large (XM_OVERLAP_MIN_MB, default 64; XM_OVERLAP=0 disables).
bool Context::overlap_applies() const {
    if (cfg_.overlap < 0 || !comm_->active() || storage_ != XM_STORAGE_DENSE || sym_ok_ || symw_) return false;
    if ((double)nloc_ * 3.0 * (double)ld_ * 8.0 < cfg_.overlap_min_mb * 1048576.0) return false;
    const int tc = qw_dense_tile_cols();
    const int64_t c0 = 3 * (int64_t)cam0_, c1 = 3 * ((int64_t)cam0_ + nloc_);
    return (c1 / tc) > ((c0 + tc - 1) / tc);
}

void Context::gather_W() {
    if (!comm_->active()) return;
    if (overlap_applies()) { w_pending_ = true; return; }   // resolved by the next product()
    comm_->allgather(W_.p, (size_t)nloc_ * 3 * OP_, st_);
}

void Context::flush_gather() {
    if (!w_pending_) return;
    w_pending_ = false;
    comm_->allgather(W_.p, (size_t)nloc_ * 3 * OP_, st_);
}

double Context::sum_parts(const double *dparts, int count) {
    if (comm_->peer()) launch_copy_words(hpin_dev_, dparts, (size_t)count * sizeof(double), st_);   // see to_host
    else XM_HIP_CHECK(hipMemcpyAsync(hpin_, dparts, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st_));
    XM_HIP_CHECK(hipStreamSynchronize(st_));
    double t = 0.0;
    for (int i = 0; i < count; ++i) t += hpin_[i];
    return t;
}

// Gradient epilogue on the point (Rp, sp) with the product input currently in W (already gathered).
// Fills ps_[state]; returns f and <rg,rg>_metric.   trustregion.h:162-170 + 186-194 + 307-317 + 483-484
void Context::eval_point(int state, const double *Rp, const double *sp, double &f, double &rr) {
    const int nA_loc = prod_grid();
    CamArgs a = cam_args(state);
    a.R = Rp;
    a.s = sp;
    a.partials = partsA_.p + (size_t)comm_->rank * 2 * nA_loc;
    product(EPI_GRAD, o_, 2.0, a);
    if (comm_->active()) comm_->allgather(partsA_.p, (size_t)2 * nA_loc, st_);
    launch_outer_finalize(partsA_.p, nA_loc, comm_->world, partsM_.p, 0, scal_.p, reinterpret_cast<double *>(hstat_dev_) + 8,
                          ++outer_seq_, grouping_, st_);
    volatile double *hres = wait_outer_result();
    f = hres[0];
    rr = hres[1];
}

// Wall-clock decisions must be identical on every rank (a rank that stops alone would leave the others inside a
// collective): the local flags are all-gathered and OR-ed.  Single rank: returns the flag.
bool Context::agree_any(bool local) {
    if (!comm_->active()) return local;
    const int world = comm_->world;
    double v = local ? 1.0 : 0.0;
    to_dev(partsM_.p + comm_->rank, &v, sizeof(double));
    comm_->allgather(partsM_.p, 1, st_);
    if (comm_->peer()) launch_copy_words(hpin_dev_, partsM_.p, (size_t)world * sizeof(double), st_);   // see to_host
    else XM_HIP_CHECK(hipMemcpyAsync(hpin_, partsM_.p, (size_t)world * sizeof(double), hipMemcpyDeviceToHost, st_));
    XM_HIP_CHECK(hipStreamSynchronize(st_));
    bool any = false;
    for (int r = 0; r < world; ++r) any = any || (hpin_[r] != 0.0);
    return any;
}

// Every host spin loop looks at the stream through this: a sticky error (launch failure, device fault, aborted collective) is
// neither hipSuccess nor hipErrorNotReady and must end the wait with XM_ERR_HIP instead of spinning for ever; so must a wait that
// exceeds the watchdog (XM_WATCHDOG_S seconds, default 600: a dead peer inside an RCCL collective never completes the stream).
bool Context::stream_idle(clk::time_point t_wait, const char *what) {
    const double limit = cfg_.watchdog_s;
    comm_->check_device_error();   // a bounded device-side wait of the peer exchange expired -> XM_ERR_COMM
    const hipError_t q = hipStreamQuery(st_);
    if (q == hipSuccess) return true;
    if (q != hipErrorNotReady) {
        (void)hipGetLastError();
        throw Error(XM_ERR_HIP, std::string("device error while waiting for ") + what + ": " + hipGetErrorString(q));
    }
    if (secs_since(t_wait) > limit)
        throw Error(XM_ERR_HIP, std::string("watchdog: no progress for ") + std::to_string((int)limit) + " s while waiting for " + what);
    return false;
}

// spin on the sequence word of the host-mapped result block (written last by outer_finalize_kernel)
volatile double *Context::wait_outer_result() {
    volatile unsigned long long *hseq = reinterpret_cast<volatile unsigned long long *>(hstat_) + 8 + 5;
    const unsigned long long seq = outer_seq_;
    const auto t_wait = clk::now();
    auto t_check = t_wait;
    while (*hseq != seq) {
        __builtin_ia32_pause();
        if (secs_since(t_check) > 500e-6) {
            if (stream_idle(t_wait, "the outer-iteration results")) {
                XM_HIP_CHECK(hipStreamSynchronize(st_));
                if (*hseq != seq) throw Error(XM_ERR_HIP, "outer-iteration results did not reach host-mapped memory");
            }
            t_check = clk::now();
        }
    }
    return reinterpret_cast<volatile double *>(hstat_) + 8;
}

void Context::drain_events() {
    for (size_t i = 0; i < ev_used_; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev_pool_[i].first, ev_pool_[i].second) == hipSuccess) qw_samples_.push_back(ms);
    }
    ev_used_ = 0;
}

// Sampled launches that turned out to be enqueued-ahead no-ops (a few microseconds) are not Q*W passes: keep the samples
// within a factor 2 of the upper quartile.
void Context::finish_profile() {
    drain_events();
    if (qw_samples_.empty()) return;
    std::vector<float> v = qw_samples_;
    std::sort(v.begin(), v.end());
    const float ref = v[(v.size() * 3) / 4];
    for (float x : v)
        if (x >= 0.5f * ref) { res_->qw_ms_sum += x; res_->qw_ms_count++; }
    qw_samples_.clear();
}

// ------------------------------------------------------------------------------------------------------------------
// truncated CG (trustregion.h:559-664): enqueue-ahead with a host-mapped progress word, no host sync per iteration
// ------------------------------------------------------------------------------------------------------------------
// one tCG iteration on the stream: the Hessian product of iteration i, the lockstep all-gather when the exchange is not fused, cg_step.
// Two-launch form (tcg_two_launch): the symmetric sweep of iteration i >= 1 carries cg_step(i - 1) in its own launch and derives its product
// input, the reducer follows; iteration 0 reads W as tcg_init wrote it and carries nothing.  The step of the LAST iteration T therefore runs in
// launch pair T + 1 -- the pair the host learns the end of the tCG from (run_tcg).
void Context::tcg_enqueue_iteration(int i, bool profile) {
    if (tcg_two_launch()) {
        const CgStepArgs P = (i > 0) ? cg_step_args(i - 1) : CgStepArgs();
        fuse_step_ = (i > 0) ? &P : nullptr;
        struct Clear { const CgStepArgs *&p; ~Clear() { p = nullptr; } } clear{fuse_step_};
        tcg_product(EPI_HESS, tcg_cam_args(tcg_parity(i & 1), false), i & 1, profile);
        return;
    }
    const CgStepArgs S = cg_step_args(i);
    tcg_product(EPI_HESS, tcg_cam_args(S.v, false), i & 1, profile);
    if (comm_->active() && xchg_.world <= 1) comm_->allgather(S.v.pcur, S.v.chunk, st_);   // lockstep: the exchange is not fused into cg_step
    launch_cg_step(o_, S, st_);
}

// Two launches per iteration: one GPU, host-driven outer iteration with run-ahead polling, the f64 symmetric pair at a rank whose sweep can derive its
// input (o = 3, 4 and a chunk plan whose rows fit the sweep's LDS).  Everything else -- several ranks, XM_FLAG_HOST_STEPPED, the device-driven outer
// iteration, hess_f32, rank 5 and up, the other storages -- and XM_FLAG_TCG_THREE_LAUNCH keep the three launches.
bool Context::tcg_two_launch() const {
    if (!opt_ || (opt_->flags & (XM_FLAG_HOST_STEPPED | XM_FLAG_TCG_THREE_LAUNCH))) return false;
    if (comm_->active() || comm_->world > 1 || storage_ != XM_STORAGE_DENSE || dQ32_ || symw_ || !sym_ok_ || !symv_ || wpad()) return false;
    if (o_ < 3 || o_ > sym_max_o_ || !symv_derives(symv_, o_)) return false;
    return !device_outer_applies(o_);
}

// tCG partial sums travel in ONE all-gather per iteration: chunk = [Hessian-epilogue partials of this iteration | |r|^2 partials the previous
// cg_step left in this parity's buffer] and, with more than one rank, in front of them this rank's rows of the image of Hp (see cg_step_kernel):
// the product input of the next iteration then follows from replicated data and needs no all-gather of its own.
TcgParity Context::tcg_parity(int par) const {
    const size_t nA = (size_t)prod_grid(), world = (size_t)comm_->world, rank = (size_t)comm_->rank;
    TcgParity v;
    v.scal_cur = scal_.p + par; v.scal_next = scal_.p + (par ^ 1);
    v.ps_cur = par ? psB_.p : psA_.p; v.ps_next = par ? psA_.p : psB_.p;
    v.rs_cur = par ? rsB_.p : rs_.p; v.rs_next = par ? rs_.p : rsB_.p;
    // (the device-driven outer iteration starts its truncated CGs inside its step launch, whatever the slot's parity: p and r stay in one buffer there)
    const bool one = opt_ && device_outer_applies(o_);
    v.pR_cur = (par && !one) ? pRB_.p : pR_.p; v.pR_next = (par || one) ? pR_.p : pRB_.p;
    v.rR_cur = (par && !one) ? rRB_.p : rR_.p; v.rR_next = (par || one) ? rR_.p : rRB_.p;
    v.b_off = comm_->active() ? (size_t)nloc_ * 3 * OP_ : 0;
    v.chunk = v.b_off + 3 * nA + (size_t)tcg_blocks();
    double *pB = xchg_.world > 1 ? partsB_peer_ : partsB_.p;   // fused peer exchange: the sums live in peer-addressable memory
    v.pcur = pB + (size_t)par * v.chunk * world;
    v.parts = v.pcur + rank * v.chunk + v.b_off;
    v.Bout = comm_->active() ? v.pcur + rank * v.chunk : nullptr;
    v.partsB_out = pB + (size_t)(par ^ 1) * v.chunk * world + rank * v.chunk + v.b_off + 3 * nA;
    return v;
}

void Context::cand_role(CamArgs &a, const PointState &P, const double *R, const double *s) const {
    a.cand = {R, s, P.G.p, P.egs.p, P.S0.p, P.rgR.p, P.rgs.p, partsA_.p};
}

CamArgs Context::tcg_cam_args(const TcgParity &v, bool cand) const {
    CamArgs a = cam_args(cur_);
    a.scal = v.scal_cur; a.pR = v.pR_cur; a.ps = v.ps_cur; a.rR = v.rR_cur; a.rs = v.rs_cur;
    a.partials = v.parts; a.Bout = v.Bout;
    if (cand) cand_role(a, ps_[cur_ ^ 1], Rc_.p, sc_.p);
    return a;
}

// Every product of a tCG slot.  Sampled by HIP events when `profile` (a launch that turns out an enqueued-ahead no-op is dropped by finish_profile()).
void Context::tcg_product(int epi, const CamArgs &a, int par, bool profile) {
    const bool timed = profile && (hess_launches_ % kProfileStride == 0) && ev_used_ < ev_pool_.size();
    if (timed) XM_HIP_CHECK(hipEventRecord(ev_pool_[ev_used_].first, st_));
    sym_rev_ = par;        // consecutive tCG iterations sweep the symmetric matrix in opposite directions (launch_qw_sym)
    product(epi, o_, 2.0, a);
    sym_rev_ = 1;          // every other product (gradient, cost): bottom-up, the direction iteration 0 of a tCG does not use
    if (timed) { XM_HIP_CHECK(hipEventRecord(ev_pool_[ev_used_].second, st_)); ev_used_++; }
    hess_launches_++;
}

// With the padded copy on (single rank, sliced ELL) nothing reads the native-pitch product input inside the tCG: the main launch gathers from
// the copy and the second launch rebuilds the diagonal term from its own operands -- the kernels skip those 7.2 MB of stores per iteration at
// 100 k cameras (Wloc == nullptr).
TcgInitArgs Context::tcg_init_args(double rr, double delta, const SpecCtl *spec) const {
    const PointState &P = ps_[cur_];
    TcgInitArgs a;
    a.nloc = nloc_;
    a.rgR = P.rgR.p; a.rgs = P.rgs.p; a.R = R_.p; a.s = s_.p;
    a.rR = rR_.p; a.rs = rs_.p; a.pR = pR_.p; a.ps = psA_.p; a.vR = vR_.p; a.vs = vs_.p; a.HvR = HvR_.p; a.Hvs = Hvs_.p;
    a.Wloc = wpad() ? nullptr : W_.p + (size_t)cam0_ * 3 * OP_; a.Wpad = wpad();
    a.scal0 = scal_.p; a.rr = rr; a.delta = delta;
    a.hstat = hstat_dev_; a.seq = (int)tcg_seq_; a.spec = spec;
    return a;
}

CgStepArgs Context::cg_step_args(int i) const {
    const bool model_rec = opt_ && (opt_->flags & XM_FLAG_MODEL_RECURRENCE);
    CgStepArgs a;
    a.nloc = nloc_; a.v = tcg_parity(i & 1);
    a.nA = prod_grid(); a.nB = tcg_blocks(); a.world = comm_->world;
    a.HpR = HpR_.p; a.Hps = Hps_.p; a.R = R_.p; a.s = s_.p;
    a.vR = vR_.p; a.vs = vs_.p; a.HvR = model_rec ? nullptr : HvR_.p; a.Hvs = model_rec ? nullptr : Hvs_.p;
    a.Wloc = wpad() ? nullptr : W_.p + (size_t)cam0_ * 3 * OP_; a.Wpad = wpad();
    a.hstat = hstat_dev_; a.mat = (int64_t)nloc_ * 3 * OP_;
    a.Afull = comm_->active() ? Afull_.p : nullptr; a.Wfull = W_.p;
    a.grouping = grouping_; a.xchg = xchg_;
    a.hist = tcg_hist();
    return a;
}

// Replay of a rejected step's truncated CG: where the host decides the rejection and the next truncated CG starts from bit-identical inputs.
// Several ranks, XM_FLAG_HOST_STEPPED, the device-driven outer iteration, the matrix-free storage and XM_FLAG_HOST_OUTER (the form of rounds 1-5,
// which the device-driven form is compared with) keep recomputing, and so does XM_FLAG_TCG_RECOMPUTE.
bool Context::replay_applies() const {
    if (!opt_ || (opt_->flags & (XM_FLAG_HOST_STEPPED | XM_FLAG_HOST_OUTER | XM_FLAG_TCG_RECOMPUTE))) return false;
    if (comm_->active() || comm_->world > 1 || storage_ == XM_STORAGE_SCHUR || o_ < 3) return false;
    return !device_outer_applies(o_);
}

TcgHist Context::tcg_hist() const {
    TcgHist h;
    const size_t H = (size_t)cfg_.tcg_history;
    if (!replay_applies() || !hist_vec_.p || !hist_cam_.p || !hist_rec_.p) return h;
    if (hist_vec_.capacity < H * 2 * (size_t)nloc_ * 3 * OP_ || hist_cam_.capacity < H * 2 * (size_t)nloc_ || hist_rec_.capacity < H) return h;   // (not set up for this rank)
    h.vec = hist_vec_.p; h.cam = hist_cam_.p; h.rec = hist_rec_.p; h.H = cfg_.tcg_history;
    return h;
}

// One launch instead of tcg_init and the iterations: the progress word says how the replayed truncated CG ended, or that the records do not reach
// the iteration at which this radius trips (the rejected one ran past the history).  The scalar block is scal_[0].
int Context::run_tcg_replay(double delta) {
    ++tcg_seq_;
    TcgReplayArgs a;
    const bool model_rec = (opt_->flags & XM_FLAG_MODEL_RECURRENCE) != 0;
    a.nloc = nloc_; a.hist = tcg_hist(); a.nrec = hist_n_; a.delta = delta;
    a.vR = vR_.p; a.vs = vs_.p; a.HvR = model_rec ? nullptr : HvR_.p; a.Hvs = model_rec ? nullptr : Hvs_.p;
    a.scal_out = scal_.p; a.hstat = hstat_dev_; a.seq = (int)tcg_seq_;
    launch_tcg_replay(o_, a, st_);
    volatile unsigned long long *hs = hstat_;
    const auto t_wait = clk::now();
    auto t_check = t_wait;
    for (;;) {
        const unsigned long long v = *hs;
        if ((unsigned int)(v >> 32) == tcg_seq_ && (v & 0xff) != 0) return (int)(v & 0xff) == kTcgNotCovered ? -1 : 0;
        __builtin_ia32_pause();
        if (secs_since(t_check) > 200e-6) {
            if (stream_idle(t_wait, "the replayed truncated CG")) {
                XM_HIP_CHECK(hipStreamSynchronize(st_));
                const unsigned long long w = *hs;
                if ((unsigned int)(w >> 32) != tcg_seq_ || (w & 0xff) == 0) throw Error(XM_ERR_HIP, "replayed truncated CG: no result reached host-mapped memory");
            }
            t_check = clk::now();
        }
    }
}

// May the start of the next truncated CG be enqueued behind outer_finalize_kernel before the host knows how the outer iteration ended?
// One GPU, run-ahead polling (not the host-stepped debugging mode), and no product that synchronises with the host inside the tCG.
bool Context::spec_applies() const {
    return !comm_->active() && opt_ && !(opt_->flags & XM_FLAG_HOST_STEPPED) && storage_ != XM_STORAGE_SCHUR && cfg_.debug_drop_finalize < 0;
}

// The host's view is switched to "the candidate was accepted" (R / s swapped, the candidate's gradient state current) for the duration of the
// enqueue: the launches carry the pointers of that world.  tcg_init starts only if the device reached the same verdict (SpecCtl.go), else it
// leaves the scalar block dormant and the iteration(s) behind it return at once.  Returns the iterations enqueued.
int Context::enqueue_spec_tcg() {
    std::swap(R_.p, Rc_.p);
    std::swap(s_.p, sc_.p);
    cur_ ^= 1;
    ++tcg_seq_;
    launch_tcg_init(o_, tcg_init_args(0.0, 0.0, spec_.p), st_);
    // ONE iteration behind tcg_init, and a run-ahead of two in run_tcg: measured against 2 / 3 on one box at Final-13682 size in block CSR
    // (profiles/r05_ab_rome.txt: 27.8 against 28.8 ms per solve; fewer launches that turn out to be no-ops when the tCG ends after ~5
    // iterations) and equal at Venice size
    const int n_spec = 1;
    for (int i = 0; i < n_spec; ++i) tcg_enqueue_iteration(i, false);   // (not sampled by the HIP-event profile: they may turn out dormant)
    std::swap(R_.p, Rc_.p);
    std::swap(s_.p, sc_.p);
    cur_ ^= 1;
    return n_spec;
}

#ifndef XM_TCG_PAIRS_AHEAD
#define XM_TCG_PAIRS_AHEAD 2   // (a build-time constant so that a variant build can measure the alternative)
#endif
constexpr int kTcgPairsAhead = XM_TCG_PAIRS_AHEAD;   // launch pairs the two-launch tCG keeps ahead of the progress word
int Context::run_tcg(double rr, double delta, int adopted) {
    const bool stepped = (opt_->flags & XM_FLAG_HOST_STEPPED) != 0;
    const bool profile = (opt_->flags & XM_FLAG_PROFILE_QW) != 0;
    if (comm_->active()) comm_->note("tcg_start", rr, delta);
    // the step before was rejected and the point kept: this truncated CG is the rejected one with a smaller radius (run_tcg_replay).  A live one
    // -- this one, when the records do not cover it -- overwrites the history.
    if (adopted == 0 && hist_valid_) {
        const int enq = run_tcg_replay(delta);
        if (enq >= 0) { tcg_replayed_ = true; return enq; }
    }
    hist_valid_ = false;
    tcg_replayed_ = false;
    if (adopted == 0) {
        ++tcg_seq_;
        launch_tcg_init(o_, tcg_init_args(rr, delta, nullptr), st_);
        gather_W();
    }
    // Iterations in flight ahead of the last one seen finished; the excess become no-op launches.  With a communicator the
    // loop must issue the SAME number of collectives on every rank although ranks poll at different moments: iteration j is
    // enqueued only once iteration j-2 is confirmed (so nobody can be past T+1 when the tCG ends in iteration T) and every
    // rank tops its queue up to exactly T+2 iterations after it has seen the end (identical scalar state on all ranks =>
    // identical T).  One iteration is always queued behind the running one, so the host round trip is hidden.
    // With the DIRECT PEER EXCHANGE (xchg_.world > 1) the exchange lives inside cg_step_kernel and launches past the end of the tCG
    // skip it, so there is nothing to keep in lockstep: the loop is the single-GPU loop.
    const bool fused = xchg_.world > 1;
    if (fused) xchg_.epoch_base = (++tcg_runs_) << 12;
    const bool lockstep = comm_->active() && !fused;
    // (single GPU: two iterations ahead, three for the smallest problems, whose iteration is shorter than the host's two launches)
    // TWO-LAUNCH FORM: launch pair j carries the step of iteration j - 1, so the pair the host learns the end of the tCG from -- its sweep's first
    // workgroup publishes the outcome at its head, the step's lead thread again -- is the one that takes the last step: it is always in the queue
    // already, and the cap is one pair more (pair kMaxInner carries the step that reports status 6).  The final scalar block is the one the last
    // enqueued pair wrote, scal_[(it - 1) & 1]: pairs behind the end copy it along like the no-op steps of the three-launch form.  Pairs ahead
    // (kTcgPairsAhead): 2 -- the pair behind the one that runs is in the queue, a third only adds a no-op pair per truncated CG; measured against 3
    // on the headline in two rounds, 0.5 us per iteration ahead in every run (profiles/r32_pairs_ahead.txt, r33_pairs_ahead.txt).
    const bool two = tcg_two_launch();
    const int cap = two ? kMaxInner + 1 : kMaxInner;
    const int run_ahead = two ? kTcgPairsAhead : ((lockstep || prod_grid() >= 64) ? 2 : 3);
    int fin_status = 0, fin_iter = 0;
    int it = adopted;  // iterations enqueued
    auto fin_par = [&]() { return (two ? std::max(it - 1, 0) : it) & 1; };
    auto enqueue = [&](int i) { tcg_enqueue_iteration(i, profile); };
    auto read_scal = [&](int par) {
        TcgScal sc;
        to_host(&sc, scal_.p + par, sizeof(TcgScal));
        return sc;
    };
    if (stepped) {
        for (;;) {
            TcgScal sc = read_scal(it & 1);
            if (sc.status != 0 || it >= kMaxInner) break;
            enqueue(it++);
        }
    } else {
        // progress word = [run : 32 | iteration : 24 | status : 8], written by tcg_init and every cg_step of THIS run (TcgScal.seq): a word
        // of an earlier run -- the previous tCG's last one, until this run's tcg_init has executed -- is not progress of this one
        volatile unsigned long long *hs = hstat_;
        auto last_progress = clk::now();
        auto last_change = last_progress;   // watchdog reference: the progress word last moved here
        unsigned long long seen = ~0ull;
        for (;;) {
            const unsigned long long v = *hs;
            if (v != seen) { seen = v; last_progress = clk::now(); last_change = last_progress; }
            const bool valid = (unsigned int)(v >> 32) == tcg_seq_;
            const int status = valid ? (int)(v & 0xff) : 0;
            const int done = valid ? (int)((v >> 8) & 0xffffff) : 0;
            if (status != 0) { fin_status = status; fin_iter = done; break; }
            if (it < cap && it - done < run_ahead) { enqueue(it++); continue; }
            __builtin_ia32_pause();
            if (secs_since(last_progress) > 200e-6) {
                // Nothing new for a while: if the stream has drained the progress word is stale (or this platform does not
                // make device writes to mapped host memory visible promptly) -> read the truth from the device.
                if (stream_idle(last_change, "the truncated-CG progress word")) {
                    TcgScal sc = read_scal(fin_par());
                    if (sc.status != 0) { fin_status = sc.status; fin_iter = sc.iter; break; }
                    if (it >= cap) { fin_status = 6; fin_iter = kMaxInner; break; }
                    *hstat_ = ((unsigned long long)tcg_seq_ << 32) | ((unsigned long long)(unsigned)sc.iter << 8);
                    if (it - sc.iter >= run_ahead) enqueue(it++);  // cannot happen, but never stall
                }
                last_progress = clk::now();
            }
        }
    }
    if (comm_->active()) comm_->note("tcg_end_before_topup", (double)it, (double)(fin_iter * 16 + fin_status));
    if (fin_status == 7) { comm_->check_device_error(); throw Error(XM_ERR_COMM, "peer exchange: a rank did not arrive inside the truncated CG"); }
    if (lockstep && !stepped) {
        const int T = (fin_status == 6) ? fin_iter - 1 : fin_iter;   // iteration in which the tCG ended
        while (it < std::min(kMaxInner, T + 2)) enqueue(it++);      // no-ops, but the same collectives on every rank
    }
    return two ? std::max(it - 1, 0) : it;  // the final scalar block is scal_[(return value) & 1]; the caller fetches it together with the other results
}

// ------------------------------------------------------------------------------------------------------------------
// Riemannian trust region (trustregion.h:77-724).  On entry R_/s_ hold the initial point.
// ------------------------------------------------------------------------------------------------------------------
TrResult Context::trust_region(int o, double &gradtol, double linesearch_step, const std::vector<double> &v_dir, double max_time) {
    TrResult out;
    const double dim = (double)n_ * (3.0 * o - 6.0) + (double)n_ - 1.0;  // trustregion.h:104
    const double delta_bar = std::sqrt(dim);
    double delta = delta_bar / 8.0;
    double *Wloc = W_.p + (size_t)cam0_ * 3 * OP_;
    double f = 0, rr = 0;

    log("start linesearch\n");
    if (linesearch_step != 0) {  // trustregion.h:360-408
        launch_scale_rows(o, nloc_, R_.p, s_.p, Wloc, st_);
        gather_W();
        double f0, tmp;
        eval_point(cur_ ^ 1, R_.p, s_.p, f0, tmp);
        double alpha = linesearch_step;
        // direction: v in the new last column only
        std::vector<double> D((size_t)nloc_ * 3 * OP_, 0.0);
        for (int c = 0; c < (int)true_loc_; ++c) {
            const int64_t g = g0_ + c;
            for (int a = 0; a < 3; ++a) D[((size_t)c * 3 + a) * OP_ + (o - 1)] = v_dir[(size_t)(3 * g + a)];
        }
        to_dev(D_.p, D.data(), D.size() * sizeof(double));
        double fn;
        for (;;) {
            launch_retract(o, nloc_, cam0_, R_.p, s_.p, D_.p, nullptr, -alpha, Rc_.p, nullptr, Wloc, st_, retraction_);
            gather_W();
            eval_point(cur_ ^ 1, Rc_.p, s_.p, fn, tmp);
            if (!(fn > f0)) break;
            alpha *= 0.5;
            if (alpha < 1e-20) { log("linesearch failed! BM stopped! \n"); out.primal = -1; out.ls_failed = true; out.stop_reason = -1; return out; }
        }
        if (f0 - fn > 0) {
            log("linesearch decrease %1.3e\n", f0 - fn);
            if (opt_->flags & XM_FLAG_FIX_STALE_SR) {
                std::swap(R_.p, Rc_.p);
                launch_scale_rows(o, nloc_, R_.p, s_.p, Wloc, st_);
            } else {
                // the reference keeps sR of the point BEFORE the line search for the first cost/gradient
                // (trustregion.h:394-422: R is replaced, sR is not)
                launch_scale_rows(o, nloc_, R_.p, s_.p, Wloc, st_);
                std::swap(R_.p, Rc_.p);
            }
            gather_W();
        } else {
            log("linesearch failed! BM stopped! \n");
            out.primal = -1; out.ls_failed = true; out.stop_reason = -1;
            return out;
        }
    } else {
        launch_scale_rows(o, nloc_, R_.p, s_.p, Wloc, st_);
        gather_W();
    }
    eval_point(cur_, R_.p, s_.p, f, rr);  // loss[0] and the gradient state of the first outer iteration
    if (device_outer_applies(o)) return trust_region_device(o, gradtol, f, rr, delta, delta_bar, max_time);
    if (tcg_two_launch()) tcg_two_launch_count_++;
    hist_valid_ = false;
    tcg_replayed_ = false;
    double loss = f;

    int endreason = 6, trstatus = 4, shrink_count = 0, inner_print = 1, k = 0;
    int adopted = 0;   // iterations of the NEXT truncated CG that are already running (enqueue_spec_tcg), adopted by the decision below
    long long totalite = 0;
    int stop_reason = 14;
    const auto start = clk::now();
    for (k = 0; k < kMaxOuter; ++k) {
        const double gradnorm = std::sqrt(rr);
        progress_line(k, inner_print, loss, gradnorm, endreason, trstatus);
        if (opt_->trace && res_->trace_len < opt_->trace_cap) {
            double *tr = opt_->trace + (size_t)res_->trace_len * 6;
            tr[0] = loss; tr[1] = gradnorm; tr[2] = inner_print; tr[3] = endreason; tr[4] = trstatus; tr[5] = delta;
            res_->trace_len++;
        }
        if (endreason == 5) { stop_reason = 5; break; }   // (close_trust_region() prints why)
        if (gradnorm < gradtol) { stop_reason = 10; break; }
        if (agree_any((double)(long long)secs_since(start) > max_time)) { stop_reason = 11; break; }
        endreason = 6; trstatus = 4;

        TcgScal fin;
        const int enq = run_tcg(rr, delta, adopted);
        adopted = 0;

        // model decrease, retraction and the candidate's cost/gradient are enqueued right behind the tCG and fetched with
        // ONE synchronisation (trustregion.h:667-678 needs four blocking reads + a sync here)
        const int nA_loc = prod_grid();
        const PointState &P = ps_[cur_];
        // the step's model decrease comes out of the retraction launch (the anchor's scale part of the step is zero by construction, as in
        // the flat kernel this replaces); the quad-per-camera form of the retraction is a micro-benchmark alternative only
        const int nB_loc = retract_grid(nloc_);
        const bool model_rec = (opt_->flags & XM_FLAG_MODEL_RECURRENCE) != 0;   // the model value sits in the tCG's scalar block: no sums, no gather
        launch_retract_model(o, nloc_, cam0_, R_.p, s_.p, vR_.p, vs_.p, Rc_.p, sc_.p, Wloc, wpad(), model_rec ? nullptr : HvR_.p, Hvs_.p, P.rgR.p, P.rgs.p,
                             partsM_.p + (size_t)comm_->rank * nB_loc, st_, retraction_ == XM_RETRACT_POLAR ? 1 : 0);
        if (comm_->active() && !model_rec) comm_->allgather(partsM_.p, (size_t)nB_loc, st_);
        gather_W();
        wpad_next_ = wpad();   // the gradient product below may gather from the padded copy the retraction has just written
        {
            CamArgs a = cam_args(cur_ ^ 1);
            a.R = Rc_.p;
            a.s = sc_.p;
            a.partials = partsA_.p + (size_t)comm_->rank * 2 * nA_loc;
            product(EPI_GRAD, o_, 2.0, a);
            if (comm_->active()) comm_->allgather(partsA_.p, (size_t)2 * nA_loc, st_);
        }
        // XM_DEBUG_DROP_FINALIZE=k (tests): the k-th outer iteration "loses" its result kernel, as a failed launch would: the host
        // must come back with XM_ERR_HIP from wait_outer_result() instead of spinning on a sequence word that never arrives
        const long long drop_at = cfg_.debug_drop_finalize;
        // Single GPU: the result kernel also evaluates the trust-region update and, when the step is accepted and the solve goes on, releases
        // the start of the NEXT truncated CG, enqueued right behind it (SpecCtl): the GPU works through the host's round trip
        const bool spec = spec_applies();
        const OuterArgs oa = {loss, delta, delta_bar, gradtol, shrink_count, (k + 1 >= kMaxOuter) ? 1 : 0};
        if (drop_at >= 0 && (long long)outer_seq_ + 1 == drop_at) ++outer_seq_;
        else
        launch_outer_finalize(partsA_.p, nA_loc, comm_->world, partsM_.p, model_rec ? 0 : nB_loc * comm_->world, scal_.p + (enq & 1),
                              reinterpret_cast<double *>(hstat_dev_) + 8, ++outer_seq_, grouping_, st_, spec ? &oa : nullptr, spec_.p);
        const int n_spec = spec ? enqueue_spec_tcg() : 0;
        volatile double *hres = wait_outer_result();
        double f_new = hres[0], rr_new = hres[1], loss_qu = hres[2];
        const bool spec_go = spec && hres[6] != 0.0;
        const double spec_delta = hres[7];
        fin.status = (int)hres[3];
        fin.iter = (int)hres[4];
        if (fin.status == 7) { comm_->check_device_error(); throw Error(XM_ERR_COMM, "peer exchange: a rank did not arrive inside the truncated CG"); }
        if (fin.status == 0) fin.status = 6;  // ran out of iterations
        endreason = fin.status;
        inner_print = fin.iter + 1;
        totalite += fin.iter + 1;
        if (tcg_replayed_) { tcg_replays_++; tcg_replayed_iters_ += fin.iter + 1; }   // counted like the iterations they stand for
        if (opt_->flags & XM_FLAG_PROFILE_QW) drain_events();
        if (loss_qu >= 0) { stop_reason = 12; break; }
        const double rou = (f_new - loss) / loss_qu;  // trustregion.h:680-701
        if (rou < 0.25) { delta *= 0.25; trstatus = 1; shrink_count++; }
        else if (rou > 0.75 && endreason <= 2) { delta = std::min(delta * 2, delta_bar); trstatus = 2; shrink_count = 0; }
        else shrink_count = 0;
        bool stop_delta = false;
        if (shrink_count > 3) {
            delta *= 1e-3; shrink_count = 0;
            log("delta shrinked to %1.3e\n", delta);
            if (delta < 1e-20) stop_delta = true;
        }
        const bool reject = (f_new > loss || rou < 0.1);  // trustregion.h:702
        if (stop_delta || !reject) {
            hist_valid_ = false;
            std::swap(R_.p, Rc_.p);
            std::swap(s_.p, sc_.p);
            cur_ ^= 1;
            if (stop_delta) { stop_reason = 13; break; }  // the reference leaves the new point in place but reports loss[k]
            loss = f_new;
            rr = rr_new;
            // the device came to the same verdict from the same numbers: the tCG it has started from this point IS the next one
            if (spec_go && std::memcmp(&spec_delta, &delta, sizeof(double)) == 0) adopted = n_spec;
        } else {
            trstatus = 3;  // keep point, state, loss and rr
            // ... so the next truncated CG is this one with the smaller radius: replayed from the history its steps wrote, if the speculative
            // start behind the result kernel stayed dormant (a live one has begun to overwrite it).  A replayed one leaves the history as it is.
            if (replay_applies() && !spec_go && hist_vec_.p) {
                if (!tcg_replayed_) hist_n_ = std::min(cfg_.tcg_history, fin.iter + 1);
                hist_valid_ = true;
            }
        }
        // Speculative launches that were not adopted found a dormant scalar block and returned at once: they are no products.
        // Invariant for the ones that WERE adopted when the loop is left right after (time limit, |grad| < gradtol by a rounding of the sqrt): a live
        // tcg_init + iteration from the new point may still be in the queue; they write only the tCG's own vectors (v, Hv, r, p, W and the
        // padded copy), which every later user re-creates before reading (certificate and line search rebuild W; tcg_seq_ guards the progress word).
        if (n_spec > 0 && adopted != n_spec && res_) res_->qw_products -= n_spec;
    }
    return close_trust_region(stop_reason, gradtol, totalite, k, loss, start);
}

// XM_FLAG_VERBOSE: the reference's progress line of outer iteration k (trustregion.h:504-525)
void Context::progress_line(int k, int inner, double loss, double gradnorm, int endreason, int trstatus) const {
    static const char *trn[] = {"", "TR- ", "TR+ ", "REJ ", "TR "};
    if (k > 0) log("%s", trn[(trstatus >= 0 && trstatus <= 4) ? trstatus : 0]);
    log("%d   %d   %1.3e   %1.3e", k, inner, loss, gradnorm);
    if (k > 0) log("   %s\n", endreason == 1 ? "nagative curvature" : endreason == 2 ? "exceed trust region" : endreason == 3 ? "reached norm tolerance"
                              : endreason == 5 ? "numerical issue" : "max iteration");
    else log("\n");
}

TrResult Context::close_trust_region(int stop_reason, double &gradtol, long long totalite, int k, double loss, clk::time_point start) {
    if (stop_reason == 5) log("Terminate because of rdotr touched machine precise\n");
    else if (stop_reason == 10) { log("Terminate because of small gradient norm\n"); gradtol /= 10; }
    else if (stop_reason == 11) log("Terminate because of time limit\n");
    else if (stop_reason == 12) log("error! loss_qu is larger than 0\n");
    else if (stop_reason == 13) log("delta is too small, BM stopped!\n");
    log("\nTotal iteration:     %lld\n", totalite);
    const double secs = secs_since(start);
    log("Time taken by function1: %lld ms\n", (long long)(secs * 1e3));
    res_->tcg_iters += totalite;
    res_->outer_iters += k;
    res_->tr_seconds += secs;
    res_->last_stop_reason = stop_reason;
    TrResult out;
    out.primal = loss; out.outer_iters = k; out.stop_reason = stop_reason;
    return out;
}

// ------------------------------------------------------------------------------------------------------------------
// The same trust region with the OUTER ITERATION ON THE DEVICE (single GPU; dense, symmetric-dense and block-CSR products).
// The host's part: the first cost / gradient (done by the caller), the tests at the top of outer iteration 0, the initial scalar block, and
// then one and the same pair of launches -- product(EPI_AUTO), outer_step -- enqueued `ahead` pairs in front of the progress word, until
// the word says PH_STOP.  Everything trustregion.h:527-708 decides between two truncated CGs is decided by outer_step_kernel from the same
// partial sums with the same formulas as trust_region() above; the candidate is COPIED over the current point when it is accepted, so R_ / s_ /
// ps_[cur_] are the current point before and after, and no buffer role ever depends on what the device decided.
// Buffers with two parity copies (tCG scalar block, scale parts of p and r, partial sums) go by the parity of the SLOT (the pair's index),
// and so does the sweep direction of the dense products: every launch of the sequence is fixed when it is enqueued.
// ------------------------------------------------------------------------------------------------------------------
bool Context::device_outer_applies(int o) const {
    if (!opt_ || (opt_->flags & (XM_FLAG_HOST_OUTER | XM_FLAG_HOST_STEPPED))) return false;
    if (comm_->active() || symw_ || storage_ == XM_STORAGE_SCHUR || o < 3 || cfg_.debug_drop_finalize >= 0) return false;
    if (storage_ == XM_STORAGE_BSR3 && sell_ && sell_supports(o)) return false;   // (the sliced-ELL pair of launches has no EPI_AUTO form)
    if (storage_ == XM_STORAGE_DENSE && ks_ > 1) return false;
    // dense products: the host-driven form is 1.5-2 % faster (profiles/r06_ab_outer.txt: 41.7 against 42.4 us per tCG iteration on the headline) --
    // the device-driven one on request; block-CSR products: the device-driven form is the faster one (34.7 against 35.5 us at 13 682 cameras)
    if (storage_ == XM_STORAGE_DENSE && !(opt_->flags & XM_FLAG_DEVICE_OUTER)) return false;
    return true;
}

// The step launch's arguments for launch pair `slot` of run `runid` (trust_region_device() and the test export outer_probe() take them from here).
OuterStepArgs Context::outer_step_args(int slot, bool model_rec, double delta_bar, double gradtol, unsigned int runid) const {
    const PointState &Pc = ps_[cur_], &Pn = ps_[cur_ ^ 1];
    const int par = slot & 1;
    const TcgParity v = tcg_parity(par);
    OuterStepArgs A;
    std::memset(&A, 0, sizeof(A));
    A.nloc = nloc_; A.cam0 = cam0_;
    A.scal_cur = v.scal_cur; A.scal_next = v.scal_next;
    A.os_cur = oscal_.p + par; A.os_next = oscal_.p + (par ^ 1);
    A.parts = v.parts; A.partsB_out = v.partsB_out;
    A.nA = prod_grid(); A.nB = tcg_blocks();
    A.HpR = HpR_.p; A.Hps = Hps_.p;
    A.R = R_.p; A.s = s_.p; A.Rc = Rc_.p; A.sc = sc_.p;
    A.pR = pR_.p; A.ps_cur = v.ps_cur; A.ps_next = v.ps_next;
    A.vR = vR_.p; A.vs = vs_.p; A.HvR = model_rec ? nullptr : HvR_.p; A.Hvs = model_rec ? nullptr : Hvs_.p; A.rR = rR_.p;
    A.rs_cur = v.rs_cur; A.rs_next = v.rs_next;
    A.Wloc = W_.p + (size_t)cam0_ * 3 * OP_; A.Wpad = nullptr;
    A.cur = {Pc.G.p, Pc.egs.p, Pc.S0.p, Pc.rgR.p, Pc.rgs.p};
    A.cand = {Pn.G.p, Pn.egs.p, Pn.S0.p, Pn.rgR.p, Pn.rgs.p};
    A.partsA = partsA_.p; A.partsM = partsM_.p; A.nM = retract_grid(nloc_);
    A.delta_bar = delta_bar; A.gradtol = gradtol; A.max_outer = kMaxOuter;
    A.trace = trace_dev_.p; A.trace_cap = kMaxOuter;
    A.stop_req = stop_req_.p;
    A.hprog = hstat_dev_ + 24;
    A.run = runid; A.slot = slot; A.grp = grouping_;
    return A;
}

TrResult Context::trust_region_device(int o, double &gradtol, double f, double rr, double delta, double delta_bar, double max_time) {
    const auto start = clk::now();
    const bool profile = (opt_->flags & XM_FLAG_PROFILE_QW) != 0;
    const bool model_rec = (opt_->flags & XM_FLAG_MODEL_RECURRENCE) != 0;
    const int nB = tcg_blocks();
    double loss = f;
    int stop_reason = 14, k = 0;
    long long totalite = 0;
    if (opt_->trace && res_->trace_len < opt_->trace_cap) {
        double *tr = opt_->trace + (size_t)res_->trace_len * 6;
        tr[0] = loss; tr[1] = std::sqrt(rr); tr[2] = 1; tr[3] = 6; tr[4] = 4; tr[5] = delta;
        res_->trace_len++;
    }
    // XM_FLAG_VERBOSE: the reference's progress lines are printed from the trace records -- the same text, but a stage's lines appear together
    // when its trust region has ended instead of one by one
    progress_line(0, 1, loss, std::sqrt(rr), 6, 4);
    bool run = true;
    if (std::sqrt(rr) < gradtol) { stop_reason = 10; run = false; }
    else if ((double)(long long)secs_since(start) > max_time) { stop_reason = 11; run = false; }
    long long slots_live = 0, slots_enq = 0;
    if (run) {
        if (trace_dev_.count < (size_t)kMaxOuter * 6) trace_dev_.alloc((size_t)kMaxOuter * 6);
        if (stop_req_.count < 1) stop_req_.alloc(1);
        XM_HIP_CHECK(hipMemsetAsync(stop_req_.p, 0, sizeof(int), st_));
        if (oscal_.count < 2) oscal_.alloc(2);
        TcgScal init;
        std::memset(&init, 0, sizeof(init));
        init.phase = PH_INIT; init.delta = delta; init.seq = (int)++tcg_seq_;
        OuterScal oinit;
        std::memset(&oinit, 0, sizeof(oinit));
        oinit.loss = loss; oinit.rr_point = rr;
        to_dev(scal_.p + 1, &init, sizeof(init));   // slot -1 has parity 1
        to_dev(oscal_.p + 1, &oinit, sizeof(oinit));
        const unsigned int runid = ++outer_run_;
        volatile unsigned long long *hp = hstat_ + 24;
        *hp = 0;
        auto step_args = [&](int slot) { return outer_step_args(slot, model_rec, delta_bar, gradtol, runid); };
        const int polar = retraction_ == XM_RETRACT_POLAR ? 1 : 0;
        auto enqueue_slot = [&](int slot) {
            // sampled like the host-driven loop's Hessian launches; a pair in the gradient role moves the same bytes, a drained pair after the
            // end is dropped by finish_profile() like a run-ahead no-op
            tcg_product(EPI_AUTO, tcg_cam_args(tcg_parity(slot & 1), true), slot & 1, profile);
            launch_outer_step(o_, polar, step_args(slot), nB, st_);
        };
        launch_outer_step(o_, polar, step_args(-1), nB, st_);
        const int ahead = 4;
        int enq = 0;
        bool time_sent = false;
        auto last_progress = clk::now();
        auto last_change = last_progress;
        unsigned long long seen = ~0ull;
        for (;;) {
            const unsigned long long v = *hp;
            if (v != seen) { seen = v; last_progress = clk::now(); last_change = last_progress; }
            const bool valid = (unsigned int)(v >> 32) == runid;
            const int done = valid ? (int)((v >> 8) & 0xffffff) : 0;
            const int phase = valid ? (int)(v & 0xff) : (int)PH_INIT;
            if (phase == PH_STOP) break;
            if (enq - done < ahead) { enqueue_slot(enq++); continue; }
            __builtin_ia32_pause();
            if (!time_sent && (double)(long long)secs_since(start) > max_time) {
                XM_HIP_CHECK(hipMemsetAsync(stop_req_.p, 1, sizeof(int), st_));   // (any non-zero pattern; lands within `ahead` pairs)
                time_sent = true;
            }
            if (secs_since(last_progress) > 200e-6) {
                // nothing new for a while: if the stream has drained the word is stale (or device writes to mapped host memory are not
                // visible promptly on this platform) -> read the truth from the device
                if (stream_idle(last_change, "the outer-iteration progress word")) {
                    TcgScal sc;
                    to_host(&sc, scal_.p + (enq & 1), sizeof(TcgScal));
                    if (sc.phase == PH_STOP) break;
                    *hp = ((unsigned long long)runid << 32) | ((unsigned long long)(unsigned)enq << 8) | (unsigned long long)(unsigned)sc.phase;
                }
                last_progress = clk::now();
            }
        }
        XM_HIP_CHECK(hipStreamSynchronize(st_));
        TcgScal fin;
        OuterScal ofin;
        to_host(&fin, scal_.p + (enq & 1), sizeof(TcgScal));
        to_host(&ofin, oscal_.p + (enq & 1), sizeof(OuterScal));
        if (fin.phase != PH_STOP) throw Error(XM_ERR_HIP, "device-driven outer iteration: the final scalar block is not in the stop phase");
        k = ofin.k; totalite = ofin.totalite; loss = ofin.loss; stop_reason = ofin.stop_reason;
        slots_live = ofin.slots; slots_enq = enq;
        // trace records 1 .. k (record k exists when iteration k's top was reached: always, except when the iteration cap ended the loop)
        const int last_rec = std::min(k, kMaxOuter - 1);
        if (opt_->trace && last_rec >= 1 && res_->trace_len < opt_->trace_cap) {
            const int take = std::min(last_rec, opt_->trace_cap - res_->trace_len);
            to_host(opt_->trace + (size_t)res_->trace_len * 6, trace_dev_.p + 6, (size_t)take * 6 * sizeof(double));
            res_->trace_len += take;
        }
        if (verbose_ && last_rec >= 1) {
            std::vector<double> recs((size_t)last_rec * 6);
            to_host(recs.data(), trace_dev_.p + 6, recs.size() * sizeof(double));
            double dprev = delta;
            for (int kk = 1; kk <= last_rec; ++kk) {
                const double *rec = &recs[(size_t)(kk - 1) * 6];
                if (rec[5] < dprev * 0.25 * 0.5) log("delta shrinked to %1.3e\n", rec[5]);   // (the 1e-3 cut after four shrinks in a row)
                progress_line(kk, (int)rec[2], rec[0], rec[1], (int)rec[3], (int)rec[4]);
                dprev = rec[5];
            }
        }
        if (profile) drain_events();
        res_->qw_products -= (slots_enq - slots_live);   // pairs drained after the end were no products
    }
    res_->outer_on_device++;
    return close_trust_region(stop_reason, gradtol, totalite, k, loss, start);
}

// ------------------------------------------------------------------------------------------------------------------
// smallest eigenpair of a symmetric tridiagonal matrix: Sturm bisection + inverse iteration
// ------------------------------------------------------------------------------------------------------------------
static int sturm_count(const std::vector<double> &a, const std::vector<double> &b, int m, double x) {
    int cnt = 0;
    double d = a[0] - x;
    if (d < 0) cnt++;
    for (int i = 1; i < m; ++i) {
        if (d == 0) d = 1e-300;
        d = (a[(size_t)i] - x) - b[(size_t)i - 1] * b[(size_t)i - 1] / d;
        if (d < 0) cnt++;
    }
    return cnt;
}
static void tridiag_min(const std::vector<double> &a, const std::vector<double> &b, int m, double &theta, std::vector<double> &y,
                        double &tmax) {
    double lo = a[0], hi = a[0];
    for (int i = 0; i < m; ++i) {
        const double r = (i > 0 ? std::fabs(b[(size_t)i - 1]) : 0.0) + (i < m - 1 ? std::fabs(b[(size_t)i]) : 0.0);
        lo = std::min(lo, a[(size_t)i] - r);
        hi = std::max(hi, a[(size_t)i] + r);
    }
    tmax = std::max(std::fabs(lo), std::fabs(hi));
    double l = lo, h = hi;
    for (int it = 0; it < 200 && h - l > 4e-16 * std::max(1.0, tmax); ++it) {
        const double mid = 0.5 * (l + h);
        if (sturm_count(a, b, m, mid) >= 1) h = mid; else l = mid;
    }
    theta = 0.5 * (l + h);
    // inverse iteration: (T - theta I) y = rhs, tridiagonal LU with partial pivoting
    y.assign((size_t)m, 1.0 / std::sqrt((double)m));
    if (m == 1) { y[0] = 1.0; return; }
    const double shift = theta - 1e-14 * std::max(1.0, tmax);
    std::vector<double> dl((size_t)m), dd((size_t)m), du((size_t)m), du2((size_t)m), rhs((size_t)m);
    for (int rep = 0; rep < 3; ++rep) {
        for (int i = 0; i < m; ++i) {
            dd[(size_t)i] = a[(size_t)i] - shift;
            du[(size_t)i] = (i < m - 1) ? b[(size_t)i] : 0.0;
            dl[(size_t)i] = (i < m - 1) ? b[(size_t)i] : 0.0;  // dl[i] = T(i+1,i)
            du2[(size_t)i] = 0.0;
            rhs[(size_t)i] = y[(size_t)i];
        }
        for (int i = 0; i < m - 1; ++i) {
            if (std::fabs(dd[(size_t)i]) >= std::fabs(dl[(size_t)i])) {
                if (dd[(size_t)i] == 0) dd[(size_t)i] = 1e-300;
                const double f = dl[(size_t)i] / dd[(size_t)i];
                dd[(size_t)i + 1] -= f * du[(size_t)i];
                rhs[(size_t)i + 1] -= f * rhs[(size_t)i];
            } else {  // swap rows i and i+1
                const double f = dd[(size_t)i] / dl[(size_t)i];
                const double t_dd = dd[(size_t)i + 1], t_du = du[(size_t)i + 1];
                dd[(size_t)i] = dl[(size_t)i];
                const double old_du = du[(size_t)i];
                du[(size_t)i] = t_dd;
                du2[(size_t)i] = (i < m - 2) ? t_du : 0.0;
                dd[(size_t)i + 1] = old_du - f * t_dd;
                if (i < m - 2) du[(size_t)i + 1] = -f * t_du;
                const double tr = rhs[(size_t)i];
                rhs[(size_t)i] = rhs[(size_t)i + 1];
                rhs[(size_t)i + 1] = tr - f * rhs[(size_t)i + 1];
            }
        }
        if (dd[(size_t)m - 1] == 0) dd[(size_t)m - 1] = 1e-300;
        y[(size_t)m - 1] = rhs[(size_t)m - 1] / dd[(size_t)m - 1];
        y[(size_t)m - 2] = (rhs[(size_t)m - 2] - du[(size_t)m - 2] * y[(size_t)m - 1]) / dd[(size_t)m - 2];
        for (int i = m - 3; i >= 0; --i)
            y[(size_t)i] = (rhs[(size_t)i] - du[(size_t)i] * y[(size_t)i + 1] - du2[(size_t)i] * y[(size_t)i + 2]) / dd[(size_t)i];
        double nrm = 0;
        for (int i = 0; i < m; ++i) nrm += y[(size_t)i] * y[(size_t)i];
        nrm = std::sqrt(nrm);
        if (!(nrm > 0) || !std::isfinite(nrm)) { y.assign((size_t)m, 0.0); y[0] = 1.0; break; }
        for (int i = 0; i < m; ++i) y[(size_t)i] /= nrm;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// lambda_min and its eigenvector of S = Q + diag(dz) - blockdiag(Lam) by Lanczos with full re-orthogonalisation.
// Replaces cusolverDnXsyevd on the 3n x 3n certificate matrix (checkeig.h:303-318, Dense/eig.h:35-73), O((3n)^3),
// by products with the same Q*W kernel (rank-1 input).  Lam_/dz live in ps_[cur^1].S0 / .egs (free at this point).
// ------------------------------------------------------------------------------------------------------------------
void Context::cert_product(const double *vj, const CamArgs &a, int j) {
    if (storage_ == XM_STORAGE_DENSE && sym_ok_ && symv_) launch_qw_sym(1, EPI_CERT, dQ_, ld_, vj, 1.0, a, symv_, st_, j);
    else if (storage_ == XM_STORAGE_DENSE) launch_qw_dense(1, EPI_CERT, dQ_, ld_, vj, 1.0, a, st_);
    else if (storage_ == XM_STORAGE_SCHUR) schur_->product(1, EPI_CERT, vj, 1.0, a, st_);
    else if (sell_) launch_qw_sell(1, EPI_CERT, *sell_, vj, 1.0, a, 0, st_);
    else launch_qw_bsr3(1, EPI_CERT, rowptr_.p, colidx_.p, blocks_.p, vj, 1.0, a, st_, nb_loc_, rowinfo_.p);
}

int Context::lanczos_min(std::vector<double> &x_out, double &theta_out, int &iters_out, double &resid_out) {
    const int64_t len = ld_;           // vectors are replicated, full length, zero beyond 3n
    const int64_t m3 = 3 * n_;
    const int env_mmax = cfg_.lanczos_mmax, env_restarts = cfg_.lanczos_restarts;   // small values: debugging aids (the tests force a non-converged run)
    const int mmax = (int)std::min<int64_t>(m3, std::max(2, env_mmax));
    // Small problems take the DENSE route of the reference (cusolverDnDsyevd on S, Dense/eig.h:35-73): Householder-free, the same
    // three-term recurrence with full re-orthogonalisation IS the reduction of S to tridiagonal form when it runs all 3n steps, and
    // the QL sweep on T then returns the smallest eigenvalue of S itself (no convergence test, Ritz residual = round-off).
    const bool exact = m3 <= cfg_.cert_dense_rows && m3 <= mmax;
    eig_exact_ = false;   // set after the run: only when the Krylov space was really exhausted
    // Lanczos workspace: owned by the context and grow-only, so that no device memory is freed between two collectives of a solve
    // (see setup_rank); the host barrier covers the (re)allocation
    DevBuf<double> &V = lzV_, &c = lzc_, &w = lzw_, &c2 = lzc2_, &ab = lzab_, &dscr = lzscr_;
    const size_t nscr = (size_t)(mmax + 1) * (size_t)dots_multi_segments(len);
    if (V.count < (size_t)len * (mmax + 1) || c.count < (size_t)mmax + 2 || w.count < (size_t)len || dscr.count < nscr) {
        if (comm_->active()) comm_->host_barrier();
        V.alloc((size_t)len * (mmax + 1));
        c.alloc((size_t)mmax + 2);
        w.alloc((size_t)len);
        c2.alloc((size_t)mmax + 2);
        dscr.alloc(nscr);
        ab.alloc((size_t)2 * (mmax + 1));
        if (comm_->active()) comm_->host_barrier();
    }
    std::vector<double> x((size_t)len, 0.0);
    unsigned long long lcg = 0x9E3779B97F4A7C15ull;
    double nrm = 0;
    std::vector<int64_t> posv((size_t)n_);   // global camera -> position (identity unless the partition is balanced by blocks)
    for (int64_t g = 0; g < n_; ++g) posv[(size_t)g] = pos_of(g);
    for (int64_t i = 0; i < m3; ++i) {   // drawn in GLOBAL order: the start vector does not depend on the partition
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        const double v = ((double)(lcg >> 11) / 9007199254740992.0) - 0.5;
        x[(size_t)(3 * posv[(size_t)(i / 3)] + i % 3)] = v;
        nrm += v * v;
    }
    nrm = std::sqrt(nrm);
    for (int64_t i = 0; i < len; ++i) x[(size_t)i] /= nrm;

    CamArgs a = cam_args(cur_);
    a.Lam = ps_[cur_ ^ 1].S0.p;
    a.dz = ps_[cur_ ^ 1].egs.p;
    double theta = 0, resid = 1e300, tmax = 1;
    std::vector<double> al, be, y;
    int total = 0;
    // device-side bookkeeping: c1 / c2 = Gram-Schmidt coefficients of the two passes, ab = [alpha_0.. | beta_0..]
    XM_HIP_CHECK(hipMemsetAsync(ab.p, 0, ab.count * sizeof(double), st_));
    std::vector<double> hab((size_t)2 * (mmax + 1));
    const int batch = 8;   // Lanczos steps enqueued between two host checks
    for (int restart = 0; restart < std::max(1, env_restarts); ++restart) {
        to_dev(V.p, x.data(), (size_t)len * sizeof(double));
        al.clear(); be.clear();
        bool done = false;
        int m_use = 0;
        for (int j0 = 0; j0 < mmax && !done; j0 += batch) {
            const int j1 = std::min(mmax, j0 + batch);
            for (int j = j0; j < j1; ++j) {
                const double *vj = V.p + (size_t)j * len;
                // w = S v_j : the product input is v_j itself (pitch 1); output rows land in w at this rank's offset
                a.Wloc = vj + (size_t)cam0_ * 3;
                a.out = w.p + (size_t)cam0_ * 3;
                cert_product(vj, a, j);
                res_->qw_products++;
                if (comm_->active()) comm_->allgather(w.p, (size_t)nloc_ * 3, st_);
                // classical Gram-Schmidt twice against V(:,0..j); alpha_j = c1[j] + c2[j]; beta_j = |w|; v_{j+1} = w / beta_j
                if (lz_fused_ok(j + 1) && !lz_unfused_) {   // seven launches per step: the sums of the partial dots are taken by the kernels that use them (same bits)
                    launch_dots_multi_parts(V.p, len, j + 1, w.p, len, dscr.p, st_);
                    launch_sub_vc_fin(w.p, V.p, len, dscr.p, j + 1, len, c.p, nullptr, nullptr, st_);
                    launch_dots_multi_parts(V.p, len, j + 1, w.p, len, dscr.p, st_);
                    launch_sub_vc_fin(w.p, V.p, len, dscr.p, j + 1, len, c2.p, c.p, ab.p + j, st_);
                    launch_dots_multi_parts(w.p, len, 1, w.p, len, dscr.p, st_);
                    launch_lz_next_fin(V.p + (size_t)(j + 1) * len, w.p, dscr.p, ab.p + (mmax + 1) + j, len, st_);
                } else {
                    launch_dots_multi(V.p, len, j + 1, w.p, len, c.p, dscr.p, st_);
                    launch_sub_vc(w.p, V.p, len, c.p, j + 1, len, st_);
                    launch_dots_multi(V.p, len, j + 1, w.p, len, c2.p, dscr.p, st_);
                    launch_sub_vc(w.p, V.p, len, c2.p, j + 1, len, st_);
                    launch_lz_alpha(c.p + j, c2.p + j, ab.p + j, st_);
                    launch_dots_multi(w.p, len, 1, w.p, len, c.p + mmax + 1, dscr.p, st_);
                    launch_lz_next(V.p + (size_t)(j + 1) * len, w.p, c.p + mmax + 1, ab.p + (mmax + 1) + j, len, st_);
                }
                total++;
            }
            to_host(hab.data(), ab.p, hab.size() * sizeof(double));
            for (int j = j0; j < j1; ++j) {
                al.push_back(hab[(size_t)j]);
                const double beta = hab[(size_t)(mmax + 1) + j];
                const int m = j + 1;
                tridiag_min(al, be, m, theta, y, tmax);
                resid = std::fabs(beta * y[(size_t)m - 1]);
                m_use = m;
                const bool exhausted = (m == (int)m3) || (beta < 1e-13 * std::max(1.0, tmax));   // full space, or an invariant subspace under full re-orthogonalisation
                if (exact && exhausted && std::isfinite(beta)) eig_exact_ = true;
                if ((!exact && resid <= 1e-9 * std::max(1.0, tmax)) || exhausted || !std::isfinite(beta)) { done = true; break; }
                be.push_back(beta);
            }
        }
        // Ritz vector x = V(:,0..m_use-1) y
        if ((int)y.size() != m_use) tridiag_min(al, be, m_use, theta, y, tmax);
        lz_m_use_ = m_use; lz_cycles_ = restart + 1;   // read by the test export cert_probe() only
        to_dev(dscr.p, y.data(), (size_t)m_use * sizeof(double));   // into the dots' scratch (free here, >= mmax + 1 doubles): c1 / c2 keep the last step's coefficients
        launch_gemv_n(w.p, V.p, len, dscr.p, m_use, len, st_);
        to_host(x.data(), w.p, (size_t)len * sizeof(double));
        double nn = 0;
        for (int64_t i = 0; i < len; ++i) nn += x[(size_t)i] * x[(size_t)i];
        nn = std::sqrt(nn);
        if (nn > 0) for (int64_t i = 0; i < len; ++i) x[(size_t)i] /= nn;
        if (done) break;
    }
    x_out.assign((size_t)m3, 0.0);
    for (int64_t i = 0; i < m3; ++i) x_out[(size_t)i] = x[(size_t)(3 * posv[(size_t)(i / 3)] + i % 3)];
    theta_out = theta;
    iters_out = total;
    resid_out = resid;
    return (resid <= 1e-6 * std::max(1.0, tmax)) ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------------------------
// dual certificate (checkeig.h:42-368)
// ------------------------------------------------------------------------------------------------------------------
// The certificate's multipliers at the point in R_ / s_ (certificate() and the test export cert_probe()): Lam -> ps_[cur_ ^ 1].S0, dz -> .egs, and the
// dual value's partial sums in partsM_, 2 g per rank with g = (nloc_ + 255) / 256, all-gathered.  Returns g.
int Context::cert_multipliers(int o, double lam) {
    double *Wloc = W_.p + (size_t)cam0_ * 3 * OP_;
    // Right-hand side pieces: C * sR  (checkeig.h:182 with the diagonal term folded into cert_prepare)
    launch_scale_rows(o, nloc_, R_.p, s_.p, Wloc, st_);
    gather_W();
    CamArgs a = cam_args(cur_);
    a.out = HpR_.p;
    product(EPI_PLAIN, o, 1.0, a);
    const int g = (nloc_ + 255) / 256;
    double *Lam = ps_[cur_ ^ 1].S0.p, *dz = ps_[cur_ ^ 1].egs.p;
    launch_cert_prepare(o, nloc_, cam0_, lam, HpR_.p, R_.p, s_.p, Lam, dz, partsM_.p + (size_t)comm_->rank * 2 * g, st_);
    if (comm_->active()) comm_->allgather(partsM_.p, (size_t)2 * g, st_);
    return g;
}

CertResult Context::certificate(int o, double primal, std::vector<double> &v_out) {
    CertResult cr;
    const auto t0 = clk::now();
    int64_t pst0[3] = {0, 0, 0};
    const int64_t pcg_unconverged_at_start = schur_info(pst0, nullptr) ? pst0[2] : 0;
    const int g = cert_multipliers(o, opt_->lam);
    const double dual = sum_parts(partsM_.p, 2 * g * comm_->world);   // y0+y3+y5 + lam*sum(1 - xii^2)  (checkeig.h:322-332)
    // lambda_min(S) and its eigenvector
    XM_HIP_CHECK(hipMemsetAsync(W_.p, 0, W_.count * sizeof(double), st_));
    double theta = 0, eig_resid = 0;
    int its = 0;
    // A Ritz value is an UPPER bound of lambda_min: a run that has not converged is optimistic and must never certify a point.
    const int not_converged = lanczos_min(v_out, theta, its, eig_resid);
    res_->lanczos_iters += its;
    res_->eig_residual = eig_resid;
    if (not_converged) {
        res_->cert_flags |= XM_CERT_EIG_NOT_CONVERGED;
        log("warning: Lanczos did not converge (Ritz residual %1.3e): the certificate is not accepted on this value\n", eig_resid);
    } else {
        res_->cert_flags &= ~XM_CERT_EIG_NOT_CONVERGED;
    }
    if (eig_exact_) res_->cert_flags |= XM_CERT_EIG_EXACT; else res_->cert_flags &= ~XM_CERT_EIG_EXACT;
    log("The min eig is: %1.3e \n", theta);
    log("Primal value: %g\nnew dual%g\n", primal, dual);
    const double K = 3.0 * (double)n_;
    const double gap = primal - dual - K * std::min(0.0, theta);   // checkeig.h:334-336
    log("Optimility gap: %g\n", gap);
    double bound = 1e-4;                                           // checkeig.h:349-358 (later branches unreachable)
    if (n_ > 2000) bound = 1e-3;
    // matrix-free storage: a product whose inner CG gave up is not the operator the certificate is about
    int64_t pst[3] = {0, 0, 0};
    const bool inexact = schur_info(pst, nullptr) && pst[2] > pcg_unconverged_at_start;
    if (inexact) {
        res_->cert_flags |= XM_CERT_INEXACT_OPERATOR;
        log("warning: %lld matrix-free products of this certificate did not reach the inner tolerance: not accepted\n", (long long)(pst[2] - pcg_unconverged_at_start));
    } else {
        res_->cert_flags &= ~XM_CERT_INEXACT_OPERATOR;
    }
    cr.accepted = !not_converged && !inexact && (gap / primal < 1e-3 || theta > -bound);
    cr.min_eig = theta; cr.dual = dual; cr.gap = gap; cr.lanczos_iters = its;
    if (cr.accepted) log("BM finished with rank %d\n", o); else log("BM order plus one\n");
    res_->cert_seconds += secs_since(t0);
    return cr;
}

// ------------------------------------------------------------------------------------------------------------------
// out = alpha * Q * W through whatever storage the context holds (tests, diagnostics): host matrices, column-major 3n x o
// ------------------------------------------------------------------------------------------------------------------
void Context::apply(int o, const double *Wh, double *out, double alpha) {
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_qw: single-rank contexts only");
    if (!Wh || !out) throw Error(XM_ERR_ARG, "xm_ctx_qw: null argument");
    xm_options_t opt;
    std::memset(&opt, 0, sizeof(opt));
    opt_ = &opt;
    setup_rank(o);
    const size_t m = (size_t)3 * n_;
    std::vector<double> rm((size_t)ld_ * OP_ + 2, 0.0);
    for (size_t r = 0; r < m; ++r)
        for (int k = 0; k < o; ++k) rm[r * OP_ + k] = Wh[r + (size_t)k * m];
    XM_HIP_CHECK(hipMemcpyAsync(W_.p, rm.data(), rm.size() * sizeof(double), hipMemcpyHostToDevice, st_));
    CamArgs a = cam_args(cur_);
    a.out = HpR_.p;
    product(EPI_PLAIN, o, alpha, a);
    std::vector<double> res((size_t)nloc_ * 3 * OP_);
    XM_HIP_CHECK(hipMemcpyAsync(res.data(), HpR_.p, res.size() * sizeof(double), hipMemcpyDeviceToHost, st_));
    XM_HIP_CHECK(hipMemsetAsync(W_.p, 0, W_.count * sizeof(double), st_));
    XM_HIP_CHECK(hipStreamSynchronize(st_));
    for (size_t r = 0; r < m; ++r)
        for (int k = 0; k < o; ++k) out[r + (size_t)k * m] = res[r * OP_ + k];
    opt_ = nullptr;
    solved_ = false;
}

// ------------------------------------------------------------------------------------------------------------------
// The certificate's eigen-solver (test export xm_ctx_cert_probe, include/xm_amd.h): setup_rank(), cert_multipliers() and lanczos_min() as
// certificate() runs them, then what the last restart cycle left in the Lanczos workspace.  Solver state as after rtr_probe().
// ------------------------------------------------------------------------------------------------------------------
void tridiag_min_export(const double *a, const double *b, int m, double *theta, double *y, double *tmax) {
    std::vector<double> av(a, a + m), bv(b, b + std::max(0, m - 1)), yv;
    tridiag_min(av, bv, m, *theta, yv, *tmax);
    std::copy(yv.begin(), yv.end(), y);
}

void Context::cert_probe(xm_cert_probe_t &q) {
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_cert_probe: single-rank contexts only");
    const int o = q.o;
    xm_options_t opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.lam = q.lam;
    opt.max_rank = (unsigned)o;
    xm_result_t res;
    std::memset(&res, 0, sizeof(res));
    struct Leave { Context *c; ~Leave() { c->opt_ = nullptr; c->res_ = nullptr; c->lz_unfused_ = false; c->solved_ = false; } } leave{this};
    opt_ = &opt;
    res_ = &res;
    grouping_ = 0;
    lz_unfused_ = (q.flags & XM_CERT_PROBE_UNFUSED) != 0;
    setup_rank(o);
    const size_t n = (size_t)n_, m3 = 3 * n;
    upload_point(std::vector<double>(q.R, q.R + m3 * (size_t)o), o, std::vector<double>(q.s, q.s + n));
    const int g = cert_multipliers(o, q.lam);
    std::vector<double> parts((size_t)2 * g);
    to_host(parts.data(), partsM_.p, parts.size() * sizeof(double));
    q.dual[0] = q.dual[1] = 0.0;
    for (int i = 0; i < g; ++i) { q.dual[0] += parts[(size_t)i]; q.dual[1] += parts[(size_t)g + i]; }   // in sum_parts()'s order
    if (q.Lam) to_host(q.Lam, ps_[cur_ ^ 1].S0.p, n * 9 * sizeof(double));
    if (q.dz) to_host(q.dz, ps_[cur_ ^ 1].egs.p, n * sizeof(double));
    XM_HIP_CHECK(hipMemsetAsync(W_.p, 0, W_.count * sizeof(double), st_));
    std::vector<double> x;
    double theta = 0, resid = 0;
    int its = 0;
    lz_m_use_ = lz_cycles_ = 0;
    q.ret = lanczos_min(x, theta, its, resid);
    const int64_t len = ld_;
    const int mmax = (int)std::min<int64_t>((int64_t)m3, std::max(2, cfg_.lanczos_mmax));   // as lanczos_min()
    const int m_use = lz_m_use_, cycles = lz_cycles_, steps_dev = its - (cycles - 1) * mmax;   // a cycle that is not the last runs all mmax steps
    q.eig_exact = eig_exact_ ? 1 : 0; q.iters = its; q.m_use = m_use; q.cycles = cycles; q.mmax = mmax; q.steps_dev = steps_dev;
    auto fused = [&](int steps) { int k = 0; for (int j = 0; j < steps; ++j) k += (lz_fused_ok(j + 1) && !lz_unfused_) ? 1 : 0; return k; };   // lanczos_min()'s test
    q.steps_fused = fused(steps_dev) + (cycles - 1) * fused(mmax);
    q.steps_unfused = its - q.steps_fused;
    q.nseg = dots_multi_segments(len); q.len = len; q.product_kind = product_kind(o);
    q.theta = theta; q.resid = resid;
    if (mmax > q.cap && (q.alpha || q.beta || q.V || q.c1 || q.c2 || q.y))
        throw Error(XM_ERR_ARG, "xm_ctx_cert_probe: the arrays hold cap = " + std::to_string(q.cap) + " steps, a cycle of this context takes " + std::to_string(mmax));
    if (steps_dev < m_use || steps_dev > mmax || cycles < 1) throw Error(XM_ERR_HIP, "xm_ctx_cert_probe: the step counts of lanczos_min() do not add up");
    std::vector<double> hab((size_t)2 * (mmax + 1));
    to_host(hab.data(), lzab_.p, hab.size() * sizeof(double));
    if (q.alpha) std::copy(hab.begin(), hab.begin() + steps_dev, q.alpha);
    if (q.beta) std::copy(hab.begin() + (mmax + 1), hab.begin() + (mmax + 1) + steps_dev, q.beta);
    if (q.c1) to_host(q.c1, lzc_.p, (size_t)steps_dev * sizeof(double));
    if (q.c2) to_host(q.c2, lzc2_.p, (size_t)steps_dev * sizeof(double));
    if (q.y) to_host(q.y, lzscr_.p, (size_t)m_use * sizeof(double));
    if (q.V) {
        std::vector<double> col((size_t)len);
        for (int j = 0; j <= steps_dev; ++j) {
            to_host(col.data(), lzV_.p + (size_t)j * len, (size_t)len * sizeof(double));
            for (size_t i = 0; i < m3; ++i) q.V[(size_t)j * m3 + i] = col[(size_t)(3 * pos_of((int64_t)(i / 3))) + i % 3];
        }
    }
    if (q.x) std::copy(x.begin(), x.end(), q.x);
    XM_HIP_CHECK(hipStreamSynchronize(st_));
}

// First stage of rtr_probe() and outer_probe(): cost and gradient at the uploaded point, by trust_region()'s eval_point or (aut) by the role-switching
// launch in its candidate role: trust_region_device()'s enqueue_slot with the candidate's buffers = this point's
void Context::probe_grad(bool aut, double &f, double &rr) {
    launch_scale_rows(o_, nloc_, R_.p, s_.p, W_.p + (size_t)cam0_ * 3 * OP_, st_);
    if (!aut) return eval_point(cur_, R_.p, s_.p, f, rr);
    TcgScal sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.phase = PH_CAND;
    to_dev(scal_.p, &sc, sizeof(sc));
    CamArgs a = tcg_cam_args(tcg_parity(0), false);
    cand_role(a, ps_[cur_], R_.p, s_.p);
    product(EPI_AUTO, o_, 2.0, a);   // (swept as a first cost / gradient, not by slot parity)
    launch_outer_finalize(partsA_.p, prod_grid(), 1, partsM_.p, 0, scal_.p, reinterpret_cast<double *>(hstat_dev_) + 8, ++outer_seq_, 0, st_);
    volatile double *hres = wait_outer_result();
    f = hres[0]; rr = hres[1];
}

// ------------------------------------------------------------------------------------------------------------------
// The trust region's kernels stage by stage (test export xm_ctx_rtr_probe, include/xm_amd.h): the context's own setup for rank o, cam_args(),
// product() and the launchers with the grids and arguments of trust_region() / tcg_enqueue_iteration() / trust_region_device() / certificate().
// Nothing a later solve reads survives: setup_rank() re-creates the workspace, the progress words are not touched (hstat = nullptr, seq 0), and
// the result block's sequence number only ever has to grow.
// ------------------------------------------------------------------------------------------------------------------
void Context::rtr_probe(xm_rtr_probe_t &q) {
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_rtr_probe: single-rank contexts only");
    const int o = q.o;
    const bool aut = (q.flags & XM_RTR_PROBE_AUTO) != 0, model_rec = (q.flags & XM_RTR_PROBE_MODEL_REC) != 0;
    const bool want_hess = q.pR && q.ps, want_init = (q.flags & XM_RTR_PROBE_TCG_INIT) != 0, want_step = (q.flags & XM_RTR_PROBE_CG_STEP) != 0;
    const bool want_cert = (q.flags & XM_RTR_PROBE_CERT) != 0;
    if (want_step && !want_hess) throw Error(XM_ERR_ARG, "xm_ctx_rtr_probe: XM_RTR_PROBE_CG_STEP needs pR and ps (the hess stage)");
    if (want_step && !(q.vR && q.vs && (model_rec || (q.HvR && q.Hvs)))) throw Error(XM_ERR_ARG, "xm_ctx_rtr_probe: XM_RTR_PROBE_CG_STEP needs v (and Hv unless XM_RTR_PROBE_MODEL_REC)");
    xm_options_t opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.lam = q.lam;
    opt.max_rank = (unsigned)o;
    opt.flags = (aut ? XM_FLAG_DEVICE_OUTER : 0u) | (model_rec ? XM_FLAG_MODEL_RECURRENCE : 0u);
    struct Leave { Context *c; ~Leave() { c->opt_ = nullptr; c->sym_rev_ = 1; c->solved_ = false; } } leave{this};
    opt_ = &opt;
    grouping_ = 0;
    setup_rank(o);
    const int nA = prod_grid(), nB = tcg_blocks();
    q.product_kind = product_kind(o); q.nA = nA; q.nB = nB; q.wpad = wpad() ? 1 : 0; q.w_native = wpad() ? 0 : 1;
    q.split_k = ks_; q.sell_gather = (sell_ && sell_supports(o)) ? sell_gm_ : -1;
    if (aut && !device_outer_applies(o)) throw Error(XM_ERR_ARG, "xm_ctx_rtr_probe: XM_RTR_PROBE_AUTO, but the device-driven outer iteration does not apply to this context at this rank");
    if (want_step && q.scal_in.iter > 0 && (!q.partsB_in || q.partsB_in_count != nB))
        throw Error(XM_ERR_ARG, "xm_ctx_rtr_probe: scal_in.iter > 0 needs partsB_in with nB = " + std::to_string(nB) + " partial sums");
    const size_t n = (size_t)n_, m3 = 3 * n, mat = (size_t)nloc_ * 3 * OP_;
    std::vector<double> hm(mat), hv((size_t)nloc_);
    auto up_mat = [&](double *dst, const double *src, double sign) {   // host column-major -> device rows of pitch OP (nullptr: zeros)
        std::fill(hm.begin(), hm.end(), 0.0);
        if (src)
            for (size_t c = 0; c < n; ++c)
                for (int a = 0; a < 3; ++a)
                    for (int k = 0; k < o; ++k) hm[(c * 3 + a) * OP_ + k] = sign * src[(3 * c + a) + (size_t)k * m3];
        to_dev(dst, hm.data(), mat * sizeof(double));
    };
    auto up_vec = [&](double *dst, const double *src, double sign, bool zero_anchor) {
        std::fill(hv.begin(), hv.end(), 0.0);
        if (src)
            for (size_t c = 0; c < n; ++c) hv[c] = sign * src[c];
        if (zero_anchor) hv[0] = 0.0;
        to_dev(dst, hv.data(), hv.size() * sizeof(double));
    };
    auto down_mat = [&](double *dst, const double *src) {
        if (!dst) return;
        to_host(hm.data(), src, mat * sizeof(double));
        for (size_t c = 0; c < n; ++c)
            for (int a = 0; a < 3; ++a)
                for (int k = 0; k < o; ++k) dst[(3 * c + a) + (size_t)k * m3] = hm[(c * 3 + a) * OP_ + k];
    };
    auto down_vec = [&](double *dst, const double *src, size_t per = 1) {
        if (dst) to_host(dst, src, n * per * sizeof(double));
    };
    auto scal_out = [](const TcgScal &sc, xm_rtr_scal_t &out) {
        out.rr = sc.rr; out.vv = sc.vv; out.vp = sc.vp; out.pp = sc.pp; out.delta = sc.delta; out.gradnorm = sc.gradnorm; out.last_step = sc.last_step;
        out.model = sc.model; out.status = sc.status; out.iter = sc.iter;
    };
    double *hres_dev = reinterpret_cast<double *>(hstat_dev_) + 8;
    double *Wloc = W_.p + (size_t)cam0_ * 3 * OP_;
    double *Wtcg = wpad() ? nullptr : Wloc;   // as run_tcg: with the padded copy on, the tCG's kernels do not write the native-pitch input
    const PointState &P = ps_[cur_];

    // ---- grad: trust_region()'s first cost / gradient
    upload_point(std::vector<double>(q.R, q.R + m3 * (size_t)o), o, std::vector<double>(q.s, q.s + n));
    double f = 0, rr = 0;
    probe_grad(aut, f, rr);
    q.f = f; q.rr = rr;
    down_mat(q.G, P.G.p); down_vec(q.egs, P.egs.p); down_vec(q.S0, P.S0.p, 9); down_mat(q.rgR, P.rgR.p); down_vec(q.rgs, P.rgs.p);

    // ---- tcg_init: run_tcg()'s start from the gradient state
    if (want_init) {
        TcgInitArgs I = tcg_init_args(rr, q.scal_in.delta, nullptr);
        I.hstat = nullptr; I.seq = 0;   // no host progress word (nor a run number for it)
        launch_tcg_init(o, I, st_);
        down_mat(q.init_rR, rR_.p); down_vec(q.init_rs, rs_.p); down_mat(q.init_pR, pR_.p); down_vec(q.init_ps, psA_.p);
        down_mat(q.init_vR, vR_.p); down_vec(q.init_vs, vs_.p); down_mat(q.init_HvR, HvR_.p); down_vec(q.init_Hvs, Hvs_.p);
        if (Wtcg) down_mat(q.init_W, Wloc);
        if (wpad()) down_vec(q.init_Wpad, wpad(), 16);
        TcgScal sc;
        to_host(&sc, scal_.p, sizeof(sc));
        scal_out(sc, q.init_scal);
    }

    // ---- hess: tcg_enqueue_iteration()'s product (trust_region_device()'s in the tCG role)
    if (want_hess) {
        const int iter = want_step ? q.scal_in.iter : 0, par = iter & 1;
        const TcgParity v = tcg_parity(par);
        // the product input W = s.*pR + ps.*R, and its padded copy where the context keeps one, by the kernel that writes them in a solve: the tCG's
        // start from "rg" = -p (the anchor's scale part is 0 in every direction a solve forms)
        up_mat(D_.p, q.pR, -1.0);
        up_vec(sc_.p, q.ps, -1.0, true);
        TcgInitArgs I = tcg_init_args(0.0, 0.0, nullptr);
        I.rgR = D_.p; I.rgs = sc_.p;    // "rg" = -p
        I.hstat = nullptr; I.seq = 0;   // no host progress word (nor a run number for it)
        launch_tcg_init(o, I, st_);
        up_mat(v.pR_cur, q.pR, 1.0); up_vec(v.ps_cur, q.ps, 1.0, false);   // the vectors as given: what they hold at the anchor must not get through
        up_mat(v.rR_cur, q.rR, 1.0); up_vec(v.rs_cur, q.rs, 1.0, false);
        TcgScal sc;
        std::memset(&sc, 0, sizeof(sc));
        if (want_step) {
            sc.rr = q.scal_in.rr; sc.vv = q.scal_in.vv; sc.vp = q.scal_in.vp; sc.pp = q.scal_in.pp; sc.delta = q.scal_in.delta; sc.gradnorm = q.scal_in.gradnorm;
            sc.model = q.scal_in.model; sc.iter = q.scal_in.iter;
        }
        sc.phase = PH_TCG;
        to_dev(v.scal_cur, &sc, sizeof(sc));
        tcg_product(aut ? EPI_AUTO : EPI_HESS, tcg_cam_args(v, aut), par, false);
        // the three sums by the summation tree of cg_step_kernel (sum_partials256: the same tree in every kernel that adds partial sums)
        launch_outer_finalize(v.parts, nA, 1, v.parts + (size_t)2 * nA, nA, v.scal_cur, hres_dev, ++outer_seq_, 0, st_);
        volatile double *hres = wait_outer_result();
        q.pHp = hres[0]; q.rHp = hres[1]; q.HpHp = hres[2];
        down_mat(q.HpR, HpR_.p); down_vec(q.Hps, Hps_.p);

        // ---- cg_step: tcg_enqueue_iteration()'s second launch
        if (want_step) {
            up_mat(vR_.p, q.vR, 1.0); up_vec(vs_.p, q.vs, 1.0, false);
            if (!model_rec) { up_mat(HvR_.p, q.HvR, 1.0); up_vec(Hvs_.p, q.Hvs, 1.0, false); }
            up_vec(v.ps_next, q.ps, 1.0, false); up_vec(v.rs_next, q.rs, 1.0, false);   // a branch that leaves them alone returns the input
            if (v.pR_next != v.pR_cur) { up_mat(v.pR_next, q.pR, 1.0); up_mat(v.rR_next, q.rR, 1.0); }
            if (q.scal_in.iter > 0) to_dev(v.parts + (size_t)3 * nA, q.partsB_in, (size_t)nB * sizeof(double));
            XM_HIP_CHECK(hipMemsetAsync(v.partsB_out, 0, (size_t)nB * sizeof(double), st_));
            CgStepArgs S = cg_step_args(iter);
            S.hstat = nullptr;       // no host progress word
            S.xchg = PeerXchg();     // no peer exchange
            S.grouping = 0;          // grouping 0
            launch_cg_step(o_, S, st_);
            launch_outer_finalize(partsA_.p, 0, 1, v.partsB_out, nB, v.scal_next, hres_dev, ++outer_seq_, 0, st_);
            hres = wait_outer_result();
            q.rr_parts = hres[2];
            TcgScal nx;
            to_host(&nx, v.scal_next, sizeof(nx));
            scal_out(nx, q.scal_out);
            down_mat(q.out_vR, vR_.p); down_vec(q.out_vs, vs_.p);
            if (!model_rec) { down_mat(q.out_HvR, HvR_.p); down_vec(q.out_Hvs, Hvs_.p); }
            down_mat(q.out_rR, v.rR_next); down_vec(q.out_rs, v.rs_next); down_mat(q.out_pR, v.pR_next); down_vec(q.out_ps, v.ps_next);
            if (Wtcg) down_mat(q.out_W, Wloc);
            if (wpad()) down_vec(q.out_Wpad, wpad(), 16);
            if (q.partsB_out) to_host(q.partsB_out, v.partsB_out, (size_t)nB * sizeof(double));
        }
    }

    // ---- cert: certificate()'s right-hand side, multipliers and operator
    if (want_cert) {
        launch_scale_rows(o, nloc_, R_.p, s_.p, Wloc, st_);
        CamArgs a = cam_args(cur_);
        a.out = HpR_.p;
        product(EPI_PLAIN, o, 1.0, a);
        const int g = (nloc_ + 255) / 256;
        double *Lam = ps_[cur_ ^ 1].S0.p, *dz = ps_[cur_ ^ 1].egs.p;
        launch_cert_prepare(o, nloc_, cam0_, q.lam, HpR_.p, R_.p, s_.p, Lam, dz, partsM_.p, st_);
        std::vector<double> parts((size_t)2 * g);
        to_host(parts.data(), partsM_.p, parts.size() * sizeof(double));
        q.dual[0] = q.dual[1] = 0.0;
        for (int i = 0; i < g; ++i) { q.dual[0] += parts[(size_t)i]; q.dual[1] += parts[(size_t)g + i]; }   // in sum_parts()'s order
        down_vec(q.Lam, Lam, 9); down_vec(q.dz, dz);
        if (q.X && q.SX && q.k > 0) {
            CamArgs c = cam_args(cur_);
            c.Lam = Lam; c.dz = dz;
            std::vector<double> x((size_t)ld_), y(m3);
            for (int j = 0; j < q.k; ++j) {   // as a Lanczos vector: replicated, pitch 1, zero beyond 3n
                std::fill(x.begin(), x.end(), 0.0);
                std::copy(q.X + (size_t)j * m3, q.X + (size_t)(j + 1) * m3, x.begin());
                to_dev(W_.p, x.data(), x.size() * sizeof(double));
                c.Wloc = W_.p + (size_t)cam0_ * 3;
                c.out = HpR_.p;
                cert_product(W_.p, c, j);
                to_host(y.data(), HpR_.p, m3 * sizeof(double));
                std::copy(y.begin(), y.end(), q.SX + (size_t)j * m3);
            }
        }
        XM_HIP_CHECK(hipMemsetAsync(W_.p, 0, W_.count * sizeof(double), st_));
    }
    XM_HIP_CHECK(hipStreamSynchronize(st_));
}

// ------------------------------------------------------------------------------------------------------------------
// The other half of an outer iteration stage by stage (test export xm_ctx_outer_probe, include/xm_amd.h): the retraction launches of
// trust_region() and its line search, and one step launch of trust_region_device() with the arguments outer_step_args() gives a solve.
// What a later solve reads is re-created as after rtr_probe(); the progress word of the device-driven form carries a run number of its own.
// ------------------------------------------------------------------------------------------------------------------
void Context::outer_probe(xm_outer_probe_t &q) {
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_outer_probe: single-rank contexts only");
    const int o = q.o;
    const bool want_ret = (q.flags & XM_OUTER_PROBE_RETRACT) != 0, want_ls = (q.flags & XM_OUTER_PROBE_RETRACT_LS) != 0;
    const bool want_step = (q.flags & XM_OUTER_PROBE_STEP) != 0, model_rec = (q.flags & XM_OUTER_PROBE_MODEL_REC) != 0;
    const bool aut = want_step || (q.flags & XM_OUTER_PROBE_AUTO) != 0;
    xm_options_t opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.lam = q.lam;
    opt.max_rank = (unsigned)o;
    opt.flags = (aut ? XM_FLAG_DEVICE_OUTER : 0u) | (model_rec ? XM_FLAG_MODEL_RECURRENCE : 0u);
    struct Leave { Context *c; ~Leave() { c->opt_ = nullptr; c->sym_rev_ = 1; c->solved_ = false; } } leave{this};
    opt_ = &opt;
    grouping_ = 0;
    setup_rank(o);
    const int nA = prod_grid(), nB = tcg_blocks(), nM = retract_grid(nloc_), nwave = (nloc_ + 63) >> 6;
    const int polar = (q.flags & XM_OUTER_PROBE_POLAR) ? 1 : (q.flags & XM_OUTER_PROBE_MGS) ? 0 : (retraction_ == XM_RETRACT_POLAR ? 1 : 0);
    const int phase = q.scal_in.phase;
    q.product_kind = product_kind(o); q.nA = nA; q.nB = nB; q.nM = nM; q.wpad = wpad() ? 1 : 0; q.w_native = wpad() ? 0 : 1; q.polar = polar;
    q.grid = nB; q.nwave = nwave; q.trace_written = 0; q.run = 0; q.progress = 0;
    for (int k = 0; k < 3; ++k) q.ret_pad[k] = -1;
    q.ls_pad[0] = q.ls_pad[1] = q.out_pad[0] = q.out_pad[1] = -1;
    if (aut && !device_outer_applies(o))
        throw Error(XM_ERR_ARG, "xm_ctx_outer_probe: XM_OUTER_PROBE_STEP / _AUTO, but the device-driven outer iteration does not apply to this context at this rank");
    if (want_step && phase == PH_TCG && q.scal_in.iter > 0 && (!q.partsB_in || q.partsB_in_count != nB))
        throw Error(XM_ERR_ARG, "xm_ctx_outer_probe: scal_in.iter > 0 needs partsB_in with nB = " + std::to_string(nB) + " partial sums");
    if (want_step && phase == PH_CAND && !model_rec && (!q.partsM_in || q.partsM_in_count != nwave))
        throw Error(XM_ERR_ARG, "xm_ctx_outer_probe: the candidate role needs partsM_in with one partial sum per wavefront: " + std::to_string(nwave));
    const size_t n = (size_t)n_, m3 = 3 * n, mat = (size_t)nloc_ * 3 * OP_;
    std::vector<double> hm(mat), hv((size_t)nloc_);
    auto up_mat = [&](double *dst, const double *src, double sign) {   // host column-major -> device rows of pitch OP (nullptr: zeros)
        std::fill(hm.begin(), hm.end(), 0.0);
        if (src)
            for (size_t c = 0; c < n; ++c)
                for (int a = 0; a < 3; ++a)
                    for (int k = 0; k < o; ++k) hm[(c * 3 + a) * OP_ + k] = sign * src[(3 * c + a) + (size_t)k * m3];
        to_dev(dst, hm.data(), mat * sizeof(double));
    };
    auto up_vec = [&](double *dst, const double *src, double sign, bool zero_anchor) {
        std::fill(hv.begin(), hv.end(), 0.0);
        if (src)
            for (size_t c = 0; c < n; ++c) hv[c] = sign * src[c];
        if (zero_anchor) hv[0] = 0.0;
        to_dev(dst, hv.data(), hv.size() * sizeof(double));
    };
    auto down_mat = [&](double *dst, const double *src) {
        if (!dst) return;
        to_host(hm.data(), src, mat * sizeof(double));
        for (size_t c = 0; c < n; ++c)
            for (int a = 0; a < 3; ++a)
                for (int k = 0; k < o; ++k) dst[(3 * c + a) + (size_t)k * m3] = hm[(c * 3 + a) * OP_ + k];
    };
    auto down_vec = [&](double *dst, const double *src, size_t per = 1) {
        if (dst) to_host(dst, src, n * per * sizeof(double));
    };
    // pad columns of an even rank: ones into a matrix the next launch writes as a whole (its other entries: zeros), and the count of what is left
    const bool padded = OP_ > o;
    auto poison_mat = [&](double *dst) {
        if (!padded) return;
        std::fill(hm.begin(), hm.end(), 0.0);
        for (size_t r = 0; r < (size_t)nloc_ * 3; ++r) hm[r * OP_ + o] = 1.0;
        to_dev(dst, hm.data(), mat * sizeof(double));
    };
    auto poison_pad_only = [&](double *dst) {   // the same for a matrix whose other entries must stay
        if (!padded) return;
        to_host(hm.data(), dst, mat * sizeof(double));
        for (size_t r = 0; r < (size_t)nloc_ * 3; ++r) hm[r * OP_ + o] = 1.0;
        to_dev(dst, hm.data(), mat * sizeof(double));
    };
    auto count_pad = [&](const double *src) {
        if (!padded) return 0;
        to_host(hm.data(), src, mat * sizeof(double));
        int bad = 0;
        for (size_t r = 0; r < (size_t)nloc_ * 3; ++r) bad += hm[r * OP_ + o] != 0.0;
        return bad;
    };
    std::vector<double> hw;
    auto poison_wpad = [&]() {   // only the pad column inside a record: what lies behind 3 OP doubles is never written by anybody
        if (!wpad() || !padded) return;
        hw.assign((size_t)nloc_ * 16, 0.0);
        for (size_t c = 0; c < (size_t)nloc_; ++c)
            for (int a = 0; a < 3; ++a) hw[c * 16 + a * OP_ + o] = 1.0;
        to_dev(wpad(), hw.data(), hw.size() * sizeof(double));
    };
    auto count_wpad = [&]() {
        if (!wpad()) return -1;
        if (!padded) return 0;
        hw.assign((size_t)nloc_ * 16, 0.0);
        to_host(hw.data(), wpad(), hw.size() * sizeof(double));
        int bad = 0;
        for (size_t c = 0; c < (size_t)nloc_; ++c)
            for (int a = 0; a < 3; ++a) bad += hw[c * 16 + a * OP_ + o] != 0.0;
        return bad;
    };
    auto tcg_in = [](const xm_outer_tcg_t &in) {
        TcgScal sc;
        std::memset(&sc, 0, sizeof(sc));
        sc.rr = in.rr; sc.vv = in.vv; sc.vp = in.vp; sc.pp = in.pp; sc.delta = in.delta; sc.gradnorm = in.gradnorm; sc.last_step = in.last_step;
        sc.model = in.model; sc.status = in.status; sc.iter = in.iter; sc.seq = in.seq; sc.phase = in.phase;
        return sc;
    };
    auto tcg_out = [](const TcgScal &sc, xm_outer_tcg_t &out) {
        out.rr = sc.rr; out.vv = sc.vv; out.vp = sc.vp; out.pp = sc.pp; out.delta = sc.delta; out.gradnorm = sc.gradnorm; out.last_step = sc.last_step;
        out.model = sc.model; out.status = sc.status; out.iter = sc.iter; out.seq = sc.seq; out.phase = sc.phase;
    };
    double *hres_dev = reinterpret_cast<double *>(hstat_dev_) + 8;
    double *Wloc = W_.p + (size_t)cam0_ * 3 * OP_;
    const PointState &P = ps_[cur_], &Pn = ps_[cur_ ^ 1];

    // ---- grad: as rtr_probe()
    upload_point(std::vector<double>(q.R, q.R + m3 * (size_t)o), o, std::vector<double>(q.s, q.s + n));
    double f = 0, rr = 0;
    probe_grad(aut, f, rr);
    q.f = f; q.rr = rr;
    down_mat(q.rgR, P.rgR.p); down_vec(q.rgs, P.rgs.p);

    // ---- retract: trust_region()'s retraction of the step with its model decrease, and the result kernel behind it
    if (want_ret) {
        up_mat(vR_.p, q.vR, 1.0); up_vec(vs_.p, q.vs, 1.0, true);
        if (!model_rec) { up_mat(HvR_.p, q.HvR, 1.0); up_vec(Hvs_.p, q.Hvs, 1.0, false); }
        if (q.ret_partsM) to_dev(partsM_.p, q.ret_partsM, (size_t)nM * sizeof(double));   // what the launch must leave alone without Hv
        TcgScal sc = tcg_in(q.scal_in);
        sc.phase = 0;
        to_dev(scal_.p, &sc, sizeof(sc));
        poison_mat(Rc_.p); poison_mat(Wloc); poison_wpad();
        launch_retract_model(o, nloc_, cam0_, R_.p, s_.p, vR_.p, vs_.p, Rc_.p, sc_.p, Wloc, wpad(), model_rec ? nullptr : HvR_.p, Hvs_.p, P.rgR.p, P.rgs.p,
                             partsM_.p, st_, polar);
        launch_outer_finalize(partsA_.p, 0, 1, partsM_.p, model_rec ? 0 : nM, scal_.p, hres_dev, ++outer_seq_, grouping_, st_);
        volatile double *hres = wait_outer_result();
        q.model = hres[2];
        down_mat(q.ret_Rc, Rc_.p); down_vec(q.ret_sc, sc_.p); down_mat(q.ret_W, Wloc);
        if (wpad()) down_vec(q.ret_Wpad, wpad(), 16);
        if (q.ret_partsM) to_host(q.ret_partsM, partsM_.p, (size_t)nM * sizeof(double));
        q.ret_pad[0] = count_pad(Rc_.p); q.ret_pad[1] = count_pad(Wloc); q.ret_pad[2] = count_wpad();
    }

    // ---- retract_ls: the line search's form (trust_region(): no scale step, no scales out)
    if (want_ls) {
        up_mat(D_.p, q.D, 1.0);
        poison_mat(Rc_.p); poison_mat(Wloc);
        launch_retract(o, nloc_, cam0_, R_.p, s_.p, D_.p, nullptr, q.t, Rc_.p, nullptr, Wloc, st_, polar);
        down_mat(q.ls_Rc, Rc_.p); down_mat(q.ls_W, Wloc);
        q.ls_pad[0] = count_pad(Rc_.p); q.ls_pad[1] = count_pad(Wloc);
    }

    // ---- step: one (product, step) pair of trust_region_device() in the role scal_in.phase names
    if (want_step) {
        const int par = q.slot & 1;
        const TcgParity v = tcg_parity(par);
        if (trace_dev_.count < (size_t)kMaxOuter * 6) trace_dev_.alloc((size_t)kMaxOuter * 6);
        if (stop_req_.count < 1) stop_req_.alloc(1);
        if (oscal_.count < 2) oscal_.alloc(2);
        const int stop_word = q.stop_req;
        to_dev(stop_req_.p, &stop_word, sizeof(int));
        const unsigned int runid = ++outer_run_;
        q.run = runid;
        volatile unsigned long long *hp = hstat_ + 24;
        *hp = 0;
        if (phase == PH_TCG) {   // the product input W = s.*pR + ps.*R by the kernel that writes it in a solve, as rtr_probe()
            up_mat(D_.p, q.pR, -1.0);
            up_vec(Hps_.p, q.ps, -1.0, true);
            TcgInitArgs I = tcg_init_args(0.0, 0.0, nullptr);
            I.rgR = D_.p; I.rgs = Hps_.p;   // "rg" = -p
            I.hstat = nullptr; I.seq = 0;   // no host progress word (nor a run number for it)
            I.Wloc = Wloc; I.Wpad = nullptr;   // the native-pitch input only, as outer_step_args() (the device-driven form keeps no padded copy)
            launch_tcg_init(o, I, st_);
        }
        up_mat(v.pR_cur, q.pR, 1.0); up_vec(v.ps_cur, q.ps, 1.0, false); up_vec(v.ps_next, q.ps, 1.0, false);
        up_mat(v.rR_cur, q.rR, 1.0); up_vec(v.rs_cur, q.rs, 1.0, false); up_vec(v.rs_next, q.rs, 1.0, false);
        up_mat(vR_.p, q.vR, 1.0); up_vec(vs_.p, q.vs, 1.0, false);
        up_mat(HvR_.p, q.HvR, 1.0); up_vec(Hvs_.p, q.Hvs, 1.0, false);
        if (q.Rc && q.sc) { up_mat(Rc_.p, q.Rc, 1.0); up_vec(sc_.p, q.sc, 1.0, false); }
        else {
            XM_HIP_CHECK(hipMemcpyAsync(Rc_.p, R_.p, mat * sizeof(double), hipMemcpyDeviceToDevice, st_));
            XM_HIP_CHECK(hipMemcpyAsync(sc_.p, s_.p, (size_t)nloc_ * sizeof(double), hipMemcpyDeviceToDevice, st_));
        }
        for (DevBuf<double> *b : {&ps_[cur_ ^ 1].G, &ps_[cur_ ^ 1].egs, &ps_[cur_ ^ 1].S0, &ps_[cur_ ^ 1].rgR, &ps_[cur_ ^ 1].rgs})
            XM_HIP_CHECK(hipMemsetAsync(b->p, 0, b->count * sizeof(double), st_));
        TcgScal sc = tcg_in(q.scal_in), sc_zero;
        std::memset(&sc_zero, 0, sizeof(sc_zero));
        to_dev(v.scal_cur, &sc, sizeof(sc));
        to_dev(v.scal_next, &sc_zero, sizeof(sc_zero));
        OuterScal os, os_zero;
        std::memset(&os, 0, sizeof(os));
        std::memset(&os_zero, 0, sizeof(os_zero));
        os.loss = q.os_in.loss; os.rr_point = q.os_in.rr_point; os.totalite = q.os_in.totalite; os.shrink_count = q.os_in.shrink_count; os.k = q.os_in.k;
        os.stop_reason = q.os_in.stop_reason; os.time_up = q.os_in.time_up; os.slots = q.os_in.slots;
        to_dev(oscal_.p + par, &os, sizeof(os));
        to_dev(oscal_.p + (par ^ 1), &os_zero, sizeof(os_zero));
        XM_HIP_CHECK(hipMemsetAsync(partsB_.p, 0, 2 * v.chunk * sizeof(double), st_));
        XM_HIP_CHECK(hipMemsetAsync(partsM_.p, 0, (size_t)std::max(nwave, nM) * sizeof(double), st_));
        if (q.partsM_in && q.partsM_in_count == nwave) to_dev(partsM_.p, q.partsM_in, (size_t)nwave * sizeof(double));
        const int krec = q.os_in.k + 1;
        const bool rec_ok = krec >= 1 && krec < kMaxOuter;
        if (rec_ok) XM_HIP_CHECK(hipMemsetAsync(trace_dev_.p + (size_t)krec * 6, 0xff, 6 * sizeof(double), st_));
        const CamArgs a = tcg_cam_args(v, true);   // trust_region_device()'s enqueue_slot
        if (phase == PH_TCG) {
            tcg_product(EPI_AUTO, a, par, false);
            launch_outer_finalize(v.parts, nA, 1, v.parts + (size_t)2 * nA, nA, v.scal_cur, hres_dev, ++outer_seq_, 0, st_);
            volatile double *hres = wait_outer_result();
            q.pHp = hres[0]; q.rHp = hres[1]; q.HpHp = hres[2];
            down_mat(q.HpR, HpR_.p); down_vec(q.Hps, Hps_.p);
            if (q.scal_in.iter > 0) to_dev(v.parts + (size_t)3 * nA, q.partsB_in, (size_t)nB * sizeof(double));
            poison_pad_only(Rc_.p); poison_pad_only(Wloc);
        } else if (phase == PH_CAND) {
            launch_scale_rows(o, nloc_, Rc_.p, sc_.p, Wloc, st_);   // what the retraction of the tCG's last launch leaves as the product input
            tcg_product(EPI_AUTO, a, par, false);
            // the three sums the decision takes: f and <rg,rg> by the result kernel's tree, m of the partials regrouped as outer_decide regroups them
            std::vector<double> grouped((size_t)nM, 0.0);
            if (!model_rec)
                for (int i = 0; i < nM; ++i) {
                    auto w = [&](int j) { return j < nwave ? q.partsM_in[j] : 0.0; };
                    grouped[(size_t)i] = (w(4 * i) + w(4 * i + 1)) + (w(4 * i + 2) + w(4 * i + 3));
                }
            to_dev(D_.p, grouped.data(), grouped.size() * sizeof(double));
            launch_outer_finalize(partsA_.p, nA, 1, D_.p, model_rec ? 0 : nM, v.scal_cur, hres_dev, ++outer_seq_, grouping_, st_);
            volatile double *hres = wait_outer_result();
            q.f_cand = hres[0]; q.rr_cand = hres[1]; q.m_cand = hres[2];
            down_mat(q.cand_G, Pn.G.p); down_vec(q.cand_egs, Pn.egs.p); down_vec(q.cand_S0, Pn.S0.p, 9); down_mat(q.cand_rgR, Pn.rgR.p); down_vec(q.cand_rgs, Pn.rgs.p);
        }
        OuterStepArgs A = outer_step_args(q.slot, model_rec, q.delta_bar, q.gradtol, runid);
        if (q.max_outer > 0) A.max_outer = q.max_outer;   // (a solve's is kMaxOuter)
        launch_outer_step(o_, polar, A, nB, st_);
        XM_HIP_CHECK(hipStreamSynchronize(st_));
        q.progress = *hp;
        TcgScal nx;
        OuterScal on;
        to_host(&nx, v.scal_next, sizeof(nx));
        to_host(&on, oscal_.p + (par ^ 1), sizeof(on));
        tcg_out(nx, q.scal_out);
        q.os_out.loss = on.loss; q.os_out.rr_point = on.rr_point; q.os_out.totalite = on.totalite; q.os_out.shrink_count = on.shrink_count; q.os_out.k = on.k;
        q.os_out.stop_reason = on.stop_reason; q.os_out.time_up = on.time_up; q.os_out.slots = on.slots; q.os_out.pad = 0;
        if (rec_ok) {
            to_host(q.trace, trace_dev_.p + (size_t)krec * 6, 6 * sizeof(double));
            q.trace_written = std::isnan(q.trace[0]) ? 0 : 1;
        }
        down_mat(q.out_R, R_.p); down_vec(q.out_s, s_.p); down_mat(q.out_Rc, Rc_.p); down_vec(q.out_sc, sc_.p);
        down_mat(q.out_vR, vR_.p); down_vec(q.out_vs, vs_.p); down_mat(q.out_HvR, HvR_.p); down_vec(q.out_Hvs, Hvs_.p);
        down_mat(q.out_rR, v.rR_next); down_vec(q.out_rs, v.rs_next); down_mat(q.out_pR, v.pR_next); down_vec(q.out_ps, v.ps_next);
        down_mat(q.out_W, Wloc);
        if (wpad()) down_vec(q.out_Wpad, wpad(), 16);
        if (q.out_partsB) to_host(q.out_partsB, v.partsB_out, (size_t)nB * sizeof(double));
        if (q.out_partsM) to_host(q.out_partsM, partsM_.p, (size_t)nwave * sizeof(double));
        down_mat(q.out_G, P.G.p); down_vec(q.out_egs, P.egs.p); down_vec(q.out_S0, P.S0.p, 9); down_mat(q.out_rgR, P.rgR.p); down_vec(q.out_rgs, P.rgs.p);
        if (phase == PH_TCG) { q.out_pad[0] = count_pad(Rc_.p); q.out_pad[1] = count_pad(Wloc); }
    }
    XM_HIP_CHECK(hipStreamSynchronize(st_));
}

// ------------------------------------------------------------------------------------------------------------------
// XM^2 re-weighting on the resident context (reference loop 3_test_colmap_glomap.py:299-351)
// ------------------------------------------------------------------------------------------------------------------
void Context::attach_edges(int64_t ne, const int32_t *ei, const int32_t *ej, const double *M) {
    if (ne < 0 || (ne > 0 && (!ei || !ej || !M))) throw Error(XM_ERR_ARG, "attach_edges: bad argument");
    validate_edges(n_, ne, ei, ej, "attach_edges");
    // the kernels address cameras by their position in the padded numbering (== the global index unless the row partition is
    // balanced by stored blocks)
    std::vector<int32_t> pi((size_t)std::max<int64_t>(ne, 1)), pj((size_t)std::max<int64_t>(ne, 1));
    for (int64_t e = 0; e < ne; ++e) { pi[(size_t)e] = (int32_t)pos_of(ei[e]); pj[(size_t)e] = (int32_t)pos_of(ej[e]); }
    ei = pi.data(); ej = pj.data();
    std::vector<int64_t> inc((size_t)ntot_ + 1, 0);
    for (int64_t e = 0; e < ne; ++e) { inc[(size_t)ei[e] + 1]++; inc[(size_t)ej[e] + 1]++; }
    for (int64_t c = 0; c < ntot_; ++c) inc[(size_t)c + 1] += inc[(size_t)c];
    std::vector<int32_t> ie((size_t)std::max<int64_t>(2 * ne, 1));
    {   // incidence lists in edge order (fixed -> the diagonal sums are bit-reproducible)
        std::vector<int64_t> next(inc.begin(), inc.end() - 1);
        for (int64_t e = 0; e < ne; ++e) { ie[(size_t)next[(size_t)ei[e]]++] = (int32_t)e; ie[(size_t)next[(size_t)ej[e]]++] = (int32_t)e; }
    }
    const size_t m = (size_t)std::max<int64_t>(ne, 1);
    ei_.alloc(m, false); ej_.alloc(m, false); eM_.alloc(m * 9, false); ew_.alloc(m); eres_.alloc(m);
    inc_ptr_.alloc(inc.size(), false); inc_edge_.alloc(ie.size(), false);
    pos_ij_.alloc(m); pos_ji_.alloc(m); pos_d_.alloc((size_t)nloc_);
    if (ne > 0) {
        XM_HIP_CHECK(hipMemcpy(ei_.p, ei, (size_t)ne * sizeof(int32_t), hipMemcpyHostToDevice));
        XM_HIP_CHECK(hipMemcpy(ej_.p, ej, (size_t)ne * sizeof(int32_t), hipMemcpyHostToDevice));
        XM_HIP_CHECK(hipMemcpy(eM_.p, M, (size_t)ne * 9 * sizeof(double), hipMemcpyHostToDevice));
    }
    XM_HIP_CHECK(hipMemcpy(inc_ptr_.p, inc.data(), inc.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    XM_HIP_CHECK(hipMemcpy(inc_edge_.p, ie.data(), ie.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    ne_ = ne;
    if (storage_ == XM_STORAGE_BSR3) {
        launch_edge_locate(ne, ei_.p, ej_.p, cam0_, nloc_, rowptr_.p, colidx_.p, pos_ij_.p, pos_ji_.p, pos_d_.p, st_);
        std::vector<int64_t> a(m), b(m), d((size_t)nloc_);
        XM_HIP_CHECK(hipMemcpyAsync(a.data(), pos_ij_.p, m * sizeof(int64_t), hipMemcpyDeviceToHost, st_));
        XM_HIP_CHECK(hipMemcpyAsync(b.data(), pos_ji_.p, m * sizeof(int64_t), hipMemcpyDeviceToHost, st_));
        XM_HIP_CHECK(hipMemcpyAsync(d.data(), pos_d_.p, (size_t)nloc_ * sizeof(int64_t), hipMemcpyDeviceToHost, st_));
        XM_HIP_CHECK(hipStreamSynchronize(st_));
        for (int64_t e = 0; e < ne; ++e)
            if (a[(size_t)e] == -2 || b[(size_t)e] == -2) { ne_ = 0; throw Error(XM_ERR_ARG, "attach_edges: an edge has no stored block in the BSR3 pattern"); }
        for (int64_t c = 0; c < true_loc_; ++c)
            if (d[(size_t)c] < 0 && inc[(size_t)(cam0_ + c) + 1] > inc[(size_t)(cam0_ + c)]) { ne_ = 0; throw Error(XM_ERR_ARG, "attach_edges: a camera with edges has no stored diagonal block"); }
    }
}

void Context::edge_residuals(double *res) {
    if (schur_) {   // matrix-free: the observations are the edges (one residual per observation, input order)
        if (!solved_) throw Error(XM_ERR_ARG, "edge_residuals: the context holds no solution yet");
        if (!res) throw Error(XM_ERR_ARG, "edge_residuals: null output");
        xm_options_t opt;
        std::memset(&opt, 0, sizeof(opt));
        const xm_options_t *keep = opt_;
        opt_ = &opt;
        launch_scale_rows(o_, nloc_, R_.p, s_.p, W_.p + (size_t)cam0_ * 3 * OP_, st_);
        gather_W();
        flush_gather();
        CamArgs a = cam_args(cur_);
        a.out = HpR_.p;
        schur_->residuals(o_, W_.p, res, a, st_);
        XM_HIP_CHECK(hipMemsetAsync(W_.p, 0, W_.count * sizeof(double), st_));
        XM_HIP_CHECK(hipStreamSynchronize(st_));
        opt_ = keep;
        return;
    }
    if (ne_ <= 0 && !ei_.p) throw Error(XM_ERR_ARG, "edge_residuals: no edges attached");
    if (!solved_) throw Error(XM_ERR_ARG, "edge_residuals: the context holds no solution yet");
    if (!res) throw Error(XM_ERR_ARG, "edge_residuals: null output");
    launch_scale_rows(o_, nloc_, R_.p, s_.p, W_.p + (size_t)cam0_ * 3 * OP_, st_);
    gather_W();
    flush_gather();
    launch_edge_residual(ne_, ei_.p, ej_.p, eM_.p, W_.p, o_, OP_, eres_.p, st_);
    if (ne_ > 0) to_host(res, eres_.p, (size_t)ne_ * sizeof(double));
    XM_HIP_CHECK(hipMemsetAsync(W_.p, 0, W_.count * sizeof(double), st_));
    XM_HIP_CHECK(hipStreamSynchronize(st_));
}

// residuals of a RECOVERED rank-3 solution on the device: the product input is W_i = s_i * R_i^T (camera i's 3 x 3 record)
const double *Context::residuals_recovered_device(const double *rot, const double *scale) {
    if (!rot || !scale) throw Error(XM_ERR_ARG, "edge_residuals_recovered: null argument");
    if (!schur_ && !ei_.p) throw Error(XM_ERR_ARG, "edge_residuals_recovered: no edges attached");
    // Under a row partition every rank holds the whole edge list and gets the whole recovered solution from the caller: each
    // evaluates all residuals (and, in xm2_filter, the same order statistic) itself -- identical numbers everywhere, no exchange.
    constexpr int OP = pitch_of(3);
    if (o_ < 3 || W_.count < (size_t)ld_ * OP + 2) setup_rank(3);
    std::vector<double> hW((size_t)ld_ * OP + 2, 0.0);
    for (int64_t i = 0; i < n_; ++i) {
        const size_t pi = (size_t)pos_of(i);   // the attached edges address cameras in the padded numbering
        for (int a = 0; a < 3; ++a)
            for (int k = 0; k < 3; ++k) hW[(pi * 3 + a) * OP + k] = scale[i] * rot[(size_t)k + 3 * ((size_t)3 * i + a)];
    }
    DevBuf<double> &dW = recW_;
    if (dW.count < hW.size()) dW.alloc(hW.size());
    to_dev(dW.p, hW.data(), hW.size() * sizeof(double));
    if (schur_) {
        xm_options_t opt;
        std::memset(&opt, 0, sizeof(opt));
        const xm_options_t *keep = opt_;
        opt_ = &opt;
        const int o_keep = o_, OP_keep = OP_;
        o_ = 3; OP_ = OP;
        CamArgs a = cam_args(cur_);
        a.out = HpR_.p;
        const double *r = schur_->residuals_device(3, dW.p, a, st_);
        o_ = o_keep; OP_ = OP_keep;
        opt_ = keep;
        return r;
    }
    launch_edge_residual(ne_, ei_.p, ej_.p, eM_.p, dW.p, 3, OP, eres_.p, st_);
    return eres_.p;
}
void Context::edge_residuals_recovered(const double *rot, const double *scale, double *res) {
    if (!res) throw Error(XM_ERR_ARG, "edge_residuals_recovered: null output");
    const double *r = residuals_recovered_device(rot, scale);
    const int64_t ne = schur_ ? schur_->nobs() : ne_;
    if (ne > 0) to_host(res, r, (size_t)ne * sizeof(double));
    XM_HIP_CHECK(hipStreamSynchronize(st_));
    if (comm_->active()) comm_->host_barrier();   // nobody runs ahead into a collective while a peer still (re)allocates here
}

// k-th smallest (0-based) of n non-negative doubles on the device: most-significant-digit radix select, 4 passes of 16 bits
static double radix_select(const double *x, int64_t n, int64_t k, unsigned int *dhist, hipStream_t st) {
    unsigned long long prefix = 0;
    std::vector<unsigned int> h(65536);
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 48 - 16 * pass;
        XM_HIP_CHECK(hipMemsetAsync(dhist, 0, 65536 * sizeof(unsigned int), st));
        launch_radix_hist(n, x, shift, prefix, dhist, st);
        XM_HIP_CHECK(hipMemcpyAsync(h.data(), dhist, 65536 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        XM_HIP_CHECK(hipStreamSynchronize(st));
        int64_t acc = 0;
        int bin = 65535;
        for (int b = 0; b < 65536; ++b) {
            if (acc + (int64_t)h[(size_t)b] > k) { bin = b; break; }
            acc += h[(size_t)b];
        }
        k -= acc;
        prefix = (prefix << 16) | (unsigned long long)bin;
    }
    double v;
    std::memcpy(&v, &prefix, sizeof(double));
    return v;
}

// Position h = (nlive - 1) * pct / 100 of a percentile: floor(h) exactly (the return value) and frac(h) to two roundings.  The plain
// (double)(nlive - 1) * pct / 100.0 has the right floor, but its fractional part carries the rounding of h itself: nlive * eps of the gap
// between the two order statistics, which is far more than the threshold's own round-off where they are decades apart.
static int64_t percentile_position(int64_t nlive, double pct, double &frac) {
    const double a = (double)(nlive - 1);
    const double hi = a * pct, lo = std::fma(a, pct, -hi);   // a * pct == hi + lo exactly
    int64_t k = (int64_t)std::floor(hi / 100.0);
    double r = (hi - 100.0 * (double)k) + lo;                // the difference is exact (k is within one of hi / 100); one rounding
    while (r < 0.0) { --k; r += 100.0; }                     // rounding keeps the sign and the side of 100: the floor is exact
    while (r >= 100.0) { ++k; r -= 100.0; }
    frac = r / 100.0;
    return k;
}

double Context::xm2_filter(const double *rot, const double *scale, double pct, int64_t *removed, double *w_out) {
    if (!(pct >= 0.0 && pct <= 100.0)) throw Error(XM_ERR_ARG, "xm2_filter: percentile must be in [0, 100]");
    const int64_t ne = schur_ ? schur_->nobs() : ne_;
    if ((int64_t)w_cur_.size() != ne || ne < 1) throw Error(XM_ERR_ARG, "xm2_filter: the context does not know its edge weights (view-graph / matrix-free storage, or call xm_ctx_set_edge_weights first)");
    // the select orders bit patterns, which is the order of the values for non-negative doubles only
    for (int64_t e = 0; e < ne; ++e)
        if (!(w_cur_[(size_t)e] >= 0.0)) throw Error(XM_ERR_ARG, "xm2_filter: a negative or NaN weight (edge " + std::to_string(e) + ")");
    int64_t nz = 0;
    for (int64_t e = 0; e < ne; ++e) nz += (w_cur_[(size_t)e] == 0.0);   // -0.0 counts: a weight of -0.0 is a weight of 0
    const int64_t nlive = ne - nz;
    if (nlive < 1) throw Error(XM_ERR_ARG, "xm2_filter: every edge has been removed already");
    const double *res = residuals_recovered_device(rot, scale);
    if (ew_.count < (size_t)ne) ew_.alloc((size_t)ne);
    if (eerr_.count < (size_t)ne) eerr_.alloc((size_t)ne);
    to_dev(ew_.p, w_cur_.data(), (size_t)ne * sizeof(double));
    launch_xm2_error(ne, ew_.p, res, eerr_.p, st_);
    DevBuf<unsigned int> hist;
    hist.alloc(65536 + 1);
    // numpy.percentile's "linear" rule at the exact position h = (n - 1) q / 100: x[floor h] + (h - floor h) (x[floor h + 1] - x[floor h])
    // -- over the edges that are still THERE: the reference deletes the removed ones before the next round's percentile
    // (3_test_colmap_glomap.py:321-328).  Here a removed edge keeps its place with weight 0 and error +0.0 (xm2_error_kernel): the nz zeros
    // sort in front of every live error (>= 0), so the k-th order statistic of the survivors is entry k + nz of the whole array.
    double frac = 0.0;
    const int64_t k0 = std::min<int64_t>(percentile_position(nlive, pct, frac), nlive - 1), k1 = std::min<int64_t>(k0 + 1, nlive - 1);
    const double x0 = radix_select(eerr_.p, ne, k0 + nz, hist.p, st_);
    const double x1 = (k1 == k0 || frac == 0.0) ? x0 : radix_select(eerr_.p, ne, k1 + nz, hist.p, st_);   // an integral position: the order statistic itself
    const double thr = x0 + frac * (x1 - x0);
    XM_HIP_CHECK(hipMemsetAsync(hist.p + 65536, 0, sizeof(unsigned int), st_));
    DevBuf<double> wn;
    wn.alloc((size_t)ne, false);
    launch_xm2_filter(ne, eerr_.p, ew_.p, thr, wn.p, hist.p + 65536, st_);
    unsigned int rm = 0;
    std::vector<double> w2((size_t)ne);
    to_host(w2.data(), wn.p, (size_t)ne * sizeof(double));
    to_host(&rm, hist.p + 65536, sizeof(unsigned int));
    if (removed) *removed = (int64_t)rm;
    set_edge_weights(w2.data());
    if (w_out) std::memcpy(w_out, w2.data(), (size_t)ne * sizeof(double));
    hist.release(); wn.release();
    if (comm_->active()) comm_->host_barrier();   // as above
    return thr;
}

void Context::recover_tp(const double *rot, const double *scale, double *t, double *p) {
    if (!schur_) throw Error(XM_ERR_ARG, "recover_tp: needs a matrix-free context (XM_STORAGE_SCHUR): the translations and landmarks are functions of the observations");
    schur_->recover_tp(rot, scale, t, p, st_);
}
void Context::bundle_adjust(const BaSettings &cfg, double *rot, double *t, double *p, BaOutcome &out) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no landmarks");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_bundle_adjust: single-rank contexts only");
    BaSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::bundle_adjust(*schur_, c, rot, t, p, out, st_);
}
void Context::ba_probe(const BaSettings &cfg, const double *rot, const double *t, const double *p, BaProbe &q) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_ba_probe: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no landmarks");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_ba_probe: single-rank contexts only");
    BaSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::ba_probe(*schur_, c, rot, t, p, q, st_);
}
void Context::global_positioning(const GpSettings &cfg, const double *rot, double *t, double *p, double *scales, GpOutcome &out) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_global_positioning: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no landmarks");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_global_positioning: single-rank contexts only");
    GpSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::global_positioning(*schur_, c, rot, t, p, scales, out, st_);
}
void Context::gp_probe(const GpSettings &cfg, const double *rot, const double *t, const double *p, GpProbe &q) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_gp_probe: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no landmarks");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_gp_probe: single-rank contexts only");
    GpSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::gp_probe(*schur_, c, rot, t, p, q, st_);
}
void Context::global_positioning_pairs(const GpSettings &cfg, GpPairsIn &pairs, const double *rot, double *t, double *p, double *scales,
                                       GpOutcome &out) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_global_positioning_pairs: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no landmarks");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_global_positioning_pairs: single-rank contexts only");
    GpSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::global_positioning_pairs(*schur_, c, pairs, rot, t, p, scales, out, st_);
}
void Context::gp_probe_pairs(const GpSettings &cfg, GpPairsIn &pairs, const double *rot, const double *t, const double *p, GpProbe &q,
                             GpPairProbe &pq) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_gp_probe_pairs: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no landmarks");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_gp_probe_pairs: single-rank contexts only");
    GpSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::gp_probe_pairs(*schur_, c, pairs, rot, t, p, q, pq, st_);
}
void Context::schur_probe(xm_schur_probe_t &q) {
    if (!schur_ || schur_dense_)
        throw Error(XM_ERR_ARG, "xm_ctx_schur_probe: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages keep no factors");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_schur_probe: single-rank contexts only");
    schur_->probe(q, st_);
}
void Context::reprojection_errors(const double *rot, const double *t, const double *p, double *sqerr, const double *focal, const double *dist) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_reprojection_errors: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no landmarks");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_reprojection_errors: single-rank contexts only");
    xm::reprojection_errors(*schur_, rot, t, p, focal, dist, sqerr, cfg_.watchdog_s, st_);
}
void Context::filter_tracks(const TfSettings &cfg, const double *rot, const double *t, const double *p, uint8_t *keep, uint8_t *reason, int32_t *lm_views,
                            uint8_t *lm_status, TfOutcome &out) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_filter_tracks: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no landmarks");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_filter_tracks: single-rank contexts only");
    TfSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::filter_tracks(*schur_, c, rot, t, p, keep, reason, lm_views, lm_status, out, st_);
}
void Context::triangulate_tracks(const TriSettings &cfg, const double *rot, const double *t, double *p, const uint8_t *candidate, uint8_t *keep,
                                 uint8_t *reason, int32_t *lm_views, uint8_t *lm_status, int32_t *lm_support, int32_t *lm_hypothesis, TriOutcome &out) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_triangulate_tracks: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no landmarks");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_triangulate_tracks: single-rank contexts only");
    TriSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::triangulate_tracks(*schur_, c, rot, t, p, candidate, keep, reason, lm_views, lm_status, lm_support, lm_hypothesis, out, st_);
}
void Context::prune_weakly_connected(const PruneSettings &cfg, int32_t *cluster_id, int32_t *obs_count, const PrunePairs *pairs, PruneOutcome &out) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_prune_weakly_connected: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no observations");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_prune_weakly_connected: single-rank contexts only");
    PruneSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::prune(*schur_, c, cluster_id, obs_count, pairs, out, st_);
}
void Context::clean_observations(const CleanSettings &cfg, uint8_t *keep, int32_t *cam_index, int32_t *lm_index, CleanOutcome &out) {
    if (!schur_)
        throw Error(XM_ERR_ARG, "xm_ctx_clean_observations: needs a matrix-free context (XM_STORAGE_SCHUR): the other storages hold no observations");
    if (comm_->active()) throw Error(XM_ERR_ARG, "xm_ctx_clean_observations: single-rank contexts only");
    CleanSettings c = cfg;
    c.watchdog_s = cfg_.watchdog_s;
    xm::clean_observations(*schur_, c, keep, cam_index, lm_index, out, st_);
}
void Context::dense_q(double *q, int64_t ldq) {
    if (!schur_dense_ || !dQ_) throw Error(XM_ERR_ARG, "xm_ctx_dense_q: the context holds no dense Q built from observations (xm_tuning_t.schur_dense_q)");
    if (!q || ldq < 3 * n_) throw Error(XM_ERR_ARG, "xm_ctx_dense_q: null output or ldq < 3n");
    // symmetric bit for bit: the row-major device matrix is its own column-major image
    XM_HIP_CHECK(hipMemcpy2DAsync(q, (size_t)ldq * sizeof(double), dQ_, (size_t)ld_ * sizeof(double), (size_t)3 * n_ * sizeof(double), (size_t)3 * n_,
                                  hipMemcpyDeviceToHost, st_));
    XM_HIP_CHECK(hipStreamSynchronize(st_));
}
int64_t Context::n_landmarks() const { return schur_ ? schur_->n_landmarks() : 0; }
int64_t Context::n_observations() const { return schur_ ? schur_->nobs() : 0; }
bool Context::schur_info(int64_t out[3], double *relres) const {
    if (!schur_ || !schur_->uses_pcg()) return false;
    schur_->pcg_stats(out, relres);
    return true;
}
int Context::schur_precond(int64_t *aggregates, int *block) const {
    *aggregates = 0; *block = 0;
    if (!schur_ || !schur_->uses_pcg()) return -1;
    if (!schur_->two_level()) return 0;
    *aggregates = schur_->aggregates(); *block = kSchurAggCams;
    return 1;
}

// fp32 copy of the dense Q for the tCG's Hessian products, made on the device (nothing crosses the host link, also for a q_on_device context)
void Context::refresh_q32() {
    const size_t rows = (size_t)3 * nloc_;
    if (!dQ32_) XM_HIP_CHECK(hipMalloc((void **)&dQ32_, rows * (size_t)ld_ * sizeof(float)));
    DevBuf<unsigned int> bad;
    bad.alloc(1);
    launch_dense_to_f32(dQ_, dQ32_, (int64_t)rows, ld_, bad.p, st_);
    unsigned int h = 0;
    XM_HIP_CHECK(hipMemcpyAsync(&h, bad.p, sizeof(h), hipMemcpyDeviceToHost, st_));
    XM_HIP_CHECK(hipStreamSynchronize(st_));
    if (h) throw Error(XM_ERR_ARG, "xm_tuning_t.hess_f32: " + std::to_string(h) + " entries of Q are not finite in fp32");
}

void Context::set_edge_weights(const double *w) {
    if (schur_) {
        schur_->set_weights(w, st_);
        w_cur_.assign(w, w + schur_->nobs());
        if (schur_dense_) {   // Q follows the factors on the device; nothing is uploaded
            schur_->build_dense_q(dQ_, ld_, nullptr, st_);
            if (dQ32_) refresh_q32();
        }
        return;
    }
    if (!ei_.p) throw Error(XM_ERR_ARG, "set_edge_weights: no edges attached");
    if (ne_ > 0 && !w) throw Error(XM_ERR_ARG, "set_edge_weights: null weights");
    if (sell_ && sell_->codec() == SELL_CODEC_QUAT)   // the codec reads the weight back as the norm of the block: -w M_e would come back as w M_e
        for (int64_t e = 0; e < ne_; ++e)
            if (!(w[e] >= 0.0)) throw Error(XM_ERR_ARG, "set_edge_weights: a negative or NaN weight (edge " + std::to_string(e) + ") under the view-graph codec");
    w_cur_.assign(w, w + ne_);
    if (ne_ > 0) to_dev(ew_.p, w, (size_t)ne_ * sizeof(double));
    const bool dense = (storage_ == XM_STORAGE_DENSE);
    launch_edge_write(dense, ne_, ei_.p, ej_.p, eM_.p, ew_.p, cam0_, nloc_, inc_ptr_.p, inc_edge_.p, pos_ij_.p, pos_ji_.p, pos_d_.p,
                      dense ? nullptr : blocks_.p, dense ? dQ_ : nullptr, ld_, st_);
    if (sell_) sell_->refill(colidx_.p, blocks_.p, st_);   // the sliced-ELL copy follows the CSR values
    if (dQ32_) refresh_q32();                              // and the fp32 copy the dense values
    XM_HIP_CHECK(hipStreamSynchronize(st_));
}

// ------------------------------------------------------------------------------------------------------------------
// staircase drivers (XM_main.cu:180-310 solve, :312-401 solve_rank3, :35-178 solve_rebuttle)
// ------------------------------------------------------------------------------------------------------------------
void Context::solve(const xm_options_t &opt, xm_result_t &res) {
    opt_ = &opt;
    res_ = &res;
    verbose_ = (opt.flags & XM_FLAG_VERBOSE) != 0;
    if (opt.retraction != XM_RETRACT_QR && opt.retraction != XM_RETRACT_POLAR) throw Error(XM_ERR_ARG, "unknown retraction");
    if (opt.sum_grouping < 0 || opt.sum_grouping > 2) throw Error(XM_ERR_ARG, "sum_grouping must be 0, 1 or 2");
    retraction_ = opt.retraction;
    grouping_ = opt.sum_grouping;
    tcg_two_launch_count_ = 0;
    tcg_replays_ = tcg_replayed_iters_ = 0;
    double *Rout = res.R, *sout = res.s;
    std::memset(&res, 0, sizeof(res));
    res.R = Rout; res.s = sout;
    if (!Rout || !sout) throw Error(XM_ERR_ARG, "result buffers missing");
    if (opt.max_rank > (unsigned)kMaxRank) throw Error(XM_ERR_ARG, "max_rank > 10 is not instantiated");
    if ((opt.flags & XM_FLAG_PROFILE_QW) && ev_pool_.empty()) {
        ev_pool_.resize(256);
        for (auto &e : ev_pool_) { XM_HIP_CHECK(hipEventCreate(&e.first)); XM_HIP_CHECK(hipEventCreate(&e.second)); }
    }
    ev_used_ = 0;
    hess_launches_ = 0;
    qw_samples_.clear();
    const auto t0 = clk::now();
    const size_t m = (size_t)3 * n_;
    log("+++++++++++++++++++++++++++++++++\nBegin XM\n+++++++++++++++++++++++++++++++++\n");
    unsigned o = 3;
    std::vector<double> v(m, 0.0), R0(m * 3, 0.0), Rk, s0((size_t)n_, 1.0), sk;
    if (opt.mode == XM_MODE_REBUTTLE && opt.s_ini) for (int64_t i = 0; i < n_; ++i) s0[(size_t)i] = opt.s_ini[i];
    const double s_anchor = s0[0];
    double gradtol = opt.tol, primal = 0;
    int status = XM_STATUS_NONE;
    auto identity_stack = [&]() {
        R0.assign(m * 3, 0.0);
        for (size_t i = 0; i < (size_t)n_; ++i) { R0[3 * i] = 1.0; R0[3 * i + m + 1] = 1.0; R0[3 * i + 2 * m + 2] = 1.0; }
    };
    int out_rank = 3;
    if (opt.mode == XM_MODE_RANK3) {
        log("+++++++++++++++++++++++++++++++++\nSolve TR with Rank   3\n+++++++++++++++++++++++++++++++++\n");
        identity_stack();
        setup_rank(3);
        upload_point(R0, 3, s0);
        TrResult tr = trust_region(3, gradtol, 0.0, v, opt.max_time);
        primal = tr.primal;
        download_point(R0, s0);
        out_rank = 3;
    } else {
        while (o <= opt.max_rank) {  // XM_main.cu:223
            log("+++++++++++++++++++++++++++++++++\nSolve TR with Rank   %u\n+++++++++++++++++++++++++++++++++\n", o);
            TrResult tr;
            setup_rank((int)o);
            if (o == 3) {
                identity_stack();
                // XM_FLAG_WARM_R is honoured in EVERY staircase mode (solve and solve_rebuttle differ only in s_ini): a caller who hands
                // over R_ini wants the warm start, and silently starting from the identity would only cost iterations
                if ((opt.flags & XM_FLAG_WARM_R) && !opt.R_ini) throw Error(XM_ERR_ARG, "XM_FLAG_WARM_R without R_ini");
                const bool warm = (opt.flags & XM_FLAG_WARM_R) && opt.R_ini;
                if (warm) std::memcpy(R0.data(), opt.R_ini, m * 3 * sizeof(double));
                upload_point(R0, 3, s0);
                if (warm) {   // rows of a previous solution truncated to rank 3 are re-orthonormalised (MGS of R + 0 * D)
                    XM_HIP_CHECK(hipMemsetAsync(D_.p, 0, D_.count * sizeof(double), st_));
                    launch_retract(3, nloc_, cam0_, R_.p, s_.p, D_.p, nullptr, 0.0, Rc_.p, nullptr, nullptr, st_, 0);
                    std::swap(R_.p, Rc_.p);
                }
                tr = trust_region(3, gradtol, 0.0, v, opt.max_time);
            } else {
                upload_point(R0, (int)o, s0);
                tr = trust_region((int)o, gradtol, 1.0, v, opt.max_time);
            }
            primal = tr.primal;
            if (primal < 0) { status = XM_STATUS_LS_FAILED; o += 1; break; }  // XM_main.cu:244-247 (R0 keeps [R | 0])
            log("+++++++++++++++++++++++++++++++++\nCheck Eigen value\n+++++++++++++++++++++++++++++++++\n");
            CertResult ce = certificate((int)o, primal, v);
            res.dual = ce.dual; res.min_eig = ce.min_eig; res.gap = ce.gap;
            download_point(Rk, sk);
            if (ce.accepted) {
                R0 = Rk; s0 = sk; o += 1; status = XM_STATUS_CERTIFIED;
                break;
            } else if (o < opt.max_rank) {  // XM_main.cu:265-271
                R0.assign(m * (o + 1), 0.0);
                std::copy(Rk.begin(), Rk.end(), R0.begin());
                s0 = sk;
                for (size_t i = 0; i < (size_t)n_; ++i) { v[3 * i] /= sk[i]; v[3 * i + 1] /= sk[i]; v[3 * i + 2] /= sk[i]; }  // XM_main.cu:8-16
            } else {
                R0 = Rk; s0 = sk; status = XM_STATUS_MAX_RANK;
            }
            o += 1;
        }
        if (o > opt.max_rank) log("BM stoped because max rank\n");
        out_rank = (int)o - 1;
    }
    res.rank = out_rank;
    if (out_rank >= 3 && R0.size() >= m * (size_t)out_rank) std::memcpy(Rout, R0.data(), m * (size_t)out_rank * sizeof(double));
    for (int64_t i = 0; i < n_; ++i) sout[i] = s0[(size_t)i];
    sout[0] = s_anchor;  // the callers' s_ex[0] is never touched by the reference (XM_main.cu:203-219)
    res.status = status;
    res.primal = primal;
    if (opt.flags & XM_FLAG_PROFILE_QW) finish_profile();
    // algorithmic bytes of one tCG product at the final rank
    const int of = std::max(3, std::min(out_rank, (int)opt.max_rank));
    res.sym_product = ((sym_ok_ || symw_) && storage_ == XM_STORAGE_DENSE) ? 1 : 0;
    res.hess_f32 = dQ32_ ? 1 : 0;
    const int64_t qel = dQ32_ ? 4 : 8;   // bytes per element of the matrix the tCG products read
    if (storage_ == XM_STORAGE_DENSE) res.qw_bytes = qel * (3 * n_) * (3 * n_) + 2LL * 8 * 3 * n_ * of;
    else if (storage_ == XM_STORAGE_SCHUR) res.qw_bytes = schur_->bytes_per_product(of);
    else res.qw_bytes = 76LL * nb_loc_ + 4LL * (n_ + 1) + 2LL * 8 * 3 * n_ * of;
    res.qw_stream_bytes = (storage_ == XM_STORAGE_DENSE) ? (symw_ ? symw_->stream_bytes() : (res.sym_product ? qel / 2 : qel) * (3 * n_) * (3 * n_))
                          : (storage_ == XM_STORAGE_BSR3) ? ((sell_ && sell_supports(of)) ? sell_->stream_bytes() : 76LL * nb_loc_) : 0;
    res.n_gpus = comm_->world;
    res.exchange = !comm_->active() ? 0 : (xchg_.world > 1 ? 2 : 1);
    res.seconds = secs_since(t0);
    // leave the end point resident at its final rank for edge_residuals(): R_/s_ hold the last trust-region point already,
    // unless the staircase escalated past it (then the last stage's buffers still describe the returned point)
    solved_ = true;
    opt_ = nullptr;
    res_ = nullptr;
}

}  // namespace xm
