// xm_symv_step.h — the pieces the half-traffic sweeps for a symmetric dense Q are built from (device only): qw_symv_kernel and
// qw_symv_f32_kernel (xm_kernels.hip) use all of them, qw_symw_kernel (xm_symw.hip: work list, window predicate) uses the step.
// A kernel keeps what is its own: where a Q value and the six rows of W come from, how the masks are formed, its load policy.
// Each piece carries an order the tests and symv_reduce_kernel rely on -- of the sums, of the requests, of the partial-sum records.
#pragma once

#include <type_traits>

#include "xm_device.h"

namespace xm {

constexpr int kSvStrip = 256;

// ----------------------------------------------------------------------------------------------------------------
// Half-traffic product for SYMMETRIC dense Q (single GPU, o <= 5): only the upper block triangle is read, every Q fragment is used
// twice.  A WORKGROUP owns a strip of 256 columns and 4 K consecutive steps of it; each of its four wavefronts (lane: 2 + 2 adjacent
// columns, W of its columns in registers for the whole sweep) walks K steps of two cameras (6 rows x 256 columns = 12 KB per step):
//   column direction  y_cols += Q_step^T w_rows : per-lane accumulators that live in registers for the whole chunk; the four
//                     wavefronts' sums are added in LDS (wavefront order 0..3: fixed) and written ONCE per workgroup;
//   row direction     y_rows  = Q_step w_cols   : 6 * o per-lane partial sums per step, summed over the 64 lanes through LDS
//                     (transposed write, 16-lane DPP row sums) and written as 6 * o doubles per step.
// Element (r, c) of step j (rows [6j, 6j+6)): used both ways when c >= 6j + 6, in the row direction only when 6j <= c < 6j + 6
// (the 6 x 6 diagonal block is read in full), not at all when c < 6j (its mirror image serves it).
// Round 6 (profiles/r06_kbench_symv.txt; Venice size, o = 3 / 4, pair of launches, us): workgroup on four strips with one chunk each and a
// select behind every load 29.8 / 34.0 -> workgroup on one strip, column sums combined in LDS (Pcol / 4: ~35 instead of ~100 partial records
// per camera), loads without a select and a peeled loop so that the next step's twelve requests stay in flight while the current step is
// multiplied (s_waitcnt vmcnt(12), not 0) 28.1 / 32.5 -> alternating sweep direction (rev) 27.4 / 31.9 -> K = 6 (one residency round of
// ~420 workgroups) 26.5 / 29.6.  The per-wavefront timestamps (TRACE) say where the time of the launch goes: all wavefronts start within
// 1 us, the first step completes after ~5-6 us (every wavefront asks for 20 KB at once: 25 MB at the ~7 TB/s the fabric delivers), every
// further step 2.1-2.5 us (= 7 TB/s over all wavefronts: the loop runs at the chip's saturation), the median wavefront ends at 20 us, the last at 24.
// The loads carry no select: a row past the end re-reads the last row and meets w_row = 0 in the column direction (its row sums land in
// rows of Prow nobody reads), the absent second half of the last strip re-reads the first half and meets w_col = 0.
// ----------------------------------------------------------------------------------------------------------------

// The chunk of the triangular sweep one wavefront walks: strip s (columns from c0), column-sum record sc of that strip, steps [jb, je) -- may
// be empty at the foot of the strip; steps j < jfull lie entirely above the diagonal (no masks); R rows of Prow per strip.
struct SymvChunk {
    bool empty;       // the workgroup has nothing to do: uniform over the workgroup, so a kernel may return on it before its barrier
    int s, sc, jb, je, jfull;
    int64_t c0, R;
};
// The live (strip, group) pairs form a staircase -- strip s has ~ (s + 1) * 42.7 / (4 K) groups -- and block b runs on XCD b mod 8: a grid of
// strips x groups is half empty and its live blocks land on the XCDs unevenly (K = 11 at 2 560 cameras: 180 ... 272 live wavefronts per XCD,
// one XCD beyond its 64 resident workgroups, a second dispatch round: 66.7 us instead of 48).  FOLDED grid: row y holds strip y and, behind
// it, strip S - 1 - y -- every row has about the same number of live blocks, (nearly) every block of the grid is live, and consecutive
// blocks are consecutive XCDs.
__device__ __forceinline__ SymvChunk symv_chunk(int bx, int by, int nloc, int64_t ld, int Kc, int Kf, int ysplit, int wave) {
    SymvChunk c{};
    c.empty = true;
    const int nsteps = (nloc + 1) >> 1;
    const int nstrips = (int)((ld + kSvStrip - 1) / kSvStrip);
    const int K = (by >= ysplit) ? Kf : Kc;                      // the rows dispatched last are cut finer: they are the launch's tail
    c.s = by; c.sc = bx;
    {
        int jA = (int)(((int64_t)c.s * kSvStrip + kSvStrip + 5) / 6);
        if (jA > nsteps) jA = nsteps;
        const int nA = (jA + 4 * K - 1) / (4 * K);
        if (c.sc >= nA) {
            if (nstrips - 1 - c.s == c.s) return c;              // the middle strip of an odd count has no partner
            c.s = nstrips - 1 - c.s; c.sc -= nA;
        }
    }
    c.c0 = (int64_t)c.s * kSvStrip;
    int jend = (int)((c.c0 + kSvStrip + 5) / 6);                 // steps whose rows start above the end of the strip
    if (jend > nsteps) jend = nsteps;
    if (c.sc * 4 * K >= jend) return c;
    c.jb = (c.sc * 4 + wave) * K;
    c.je = (c.jb + K < jend) ? c.jb + K : jend;
    c.jfull = (int)(c.c0 / 6);
    c.R = (int64_t)6 * nsteps;
    c.empty = false;
    return c;
}

// W of a step's six rows travels with the step's Q: lane l requests element l of the 6 * OP contiguous doubles (one more request, issued
// ahead of the step's Q rows), and the multiply reads w_row out of that register with v_readlane.  Scalar loads at the point of use (round 5)
// were waited for one by one inside the step -- up to six exposed round trips to L2 per step at o = 4, where a row's four values are a load
// of their own.  The request is clamped to the nrows * OP doubles of W, never predicated.
template <int O>
__device__ __forceinline__ double symv_wrow_request(const double *__restrict__ W, int j, int nrows, int lane) {
    constexpr int OP = pitch_of(O);
    const int64_t wlim = (int64_t)nrows * OP - 1;
    const int64_t wi = (int64_t)6 * j * OP + (lane < 6 * OP ? lane : 0);
    return W[wi < wlim ? wi : wlim];
}
// row r of the step out of the requested lane values; ok (wave-uniform: scalar select) is false for a row past the end (odd camera count)
// (P: pitch of a row among the lanes -- OP as requested from memory; O where a sweep that derives W keeps the rows without their pad, qw_symv_kernel)
template <int O, int P = pitch_of(O)>
__device__ __forceinline__ void symv_wrow_read(double wl, int r, bool ok, double (&wr)[O]) {
    constexpr int OP = P;
#pragma unroll
    for (int k = 0; k < O; ++k) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(wl), r * OP + k), hi = __builtin_amdgcn_readlane(__double2hiint(wl), r * OP + k);
        wr[k] = ok ? __hiloint2double(hi, lo) : 0.0;
    }
}

// One step of six rows.  qat(r, h, e): the lane's Q value of row r, column pair h, element e; wrow(r, wr): row r of W into wr[O];
// mr / mc: the caller's masks per column pair for the row / column direction (MASK = false: not applied); wc: W of the lane's columns;
// ca: the lane's column sums; L: this wavefront's 6 * O * 64 doubles of LDS; prow: the 6 * O doubles of this (strip, step).
// Row direction: one multiply, then three FMAs in the order pair 0 (e 0, 1), pair 1 (e 0, 1); the 64 lanes' addends are summed by a
// 16-lane row per value -- each lane four addends (a.x + a.y) + (b.x + b.y), then the DPP row sum.
template <int O, bool MASK, class QAt, class WRow>
__device__ __forceinline__ void symv_step(QAt qat, const double (&mr)[2], const double (&mc)[2], WRow wrow, const double (&wc)[2][2][O],
                                          double (&ca)[2][2][O], double *L, int lane, double *prow) {
    constexpr int V = 6 * O;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double wr[O];
        wrow(r, wr);
        double qr[2][2], qc[2][2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double x = qat(r, h, e);
                qr[h][e] = MASK ? x * mr[h] : x;
                qc[h][e] = MASK ? x * mc[h] : x;
            }
#pragma unroll
        for (int k = 0; k < O; ++k) {
            double t = qr[0][0] * wc[0][0][k];
            t = fma(qr[0][1], wc[0][1][k], t);
            t = fma(qr[1][0], wc[1][0][k], t);
            t = fma(qr[1][1], wc[1][1][k], t);
            L[(r * O + k) * 64 + lane] = t;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 2; ++e) ca[h][e][k] = fma(qc[h][e], wr[k], ca[h][e][k]);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // 64 addends per value: a 16-lane row takes value v = 4 i + (lane / 16), each lane four addends, DPP row sum
    const int g = lane >> 4, jl = lane & 15;
#pragma unroll
    for (int v0 = 0; v0 < V; v0 += 4) {
        const int v = v0 + g;
        double t = 0.0;
        if (v < V) {
            const double2 a = *reinterpret_cast<const double2 *>(L + v * 64 + 4 * jl), b = *reinterpret_cast<const double2 *>(L + v * 64 + 4 * jl + 2);
            t = (a.x + a.y) + (b.x + b.y);
        }
        t = group_sum<16>(t);
        if (jl == 0 && v < V) prow[v] = t;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The walk over a chunk [jb, je), double-buffered and peeled: while position i is multiplied out of one slot the requests of position i + 1
// are in flight into the other, and every request inside the loop is unconditional.  load(j, slot) requests step j into slot 0 / 1 (a
// std::integral_constant), run(j, slot) multiplies it.  The caller requests position 0 into slot 0 itself -- symv_walk_at(jb, je, rev, 0),
// when jb < je -- so that it can place its other requests and its look at the status word behind it.
// rev: the chunk is walked bottom-up (position i <-> step je - 1 - i).  Launches alternate the direction, so that a launch starts with
// the steps the previous one ended with: they are still in this XCD's L2 (4 MB; block b runs on XCD b mod 8 in every launch).
__device__ __forceinline__ int symv_walk_at(int jb, int je, int rev, int i) { return rev ? je - 1 - i : jb + i; }
template <class Load, class Run>
__device__ __forceinline__ void symv_walk(int jb, int je, int rev, Load load, Run run) {
    constexpr std::integral_constant<int, 0> A{};
    constexpr std::integral_constant<int, 1> B{};
    const int cnt = je - jb;
    if (cnt <= 0) return;
    int i = 0;
    while (i + 2 < cnt) {          // two more steps follow: both requests below are unconditional
        load(symv_walk_at(jb, je, rev, i + 1), B);
        run(symv_walk_at(jb, je, rev, i), A);
        load(symv_walk_at(jb, je, rev, i + 2), A);
        run(symv_walk_at(jb, je, rev, i + 1), B);
        i += 2;
    }
    if (i + 1 < cnt) {
        load(symv_walk_at(jb, je, rev, i + 1), B);
        run(symv_walk_at(jb, je, rev, i), A);
        run(symv_walk_at(jb, je, rev, i + 1), B);
    } else {
        run(symv_walk_at(jb, je, rev, i), A);
    }
}

// Column sums of the workgroup's four chunks, added in wavefront order: every wavefront of the workgroup must arrive (workgroup barrier).
// Wavefront h (0, 1) then writes the sums of every lane's column pair h -- 2 O contiguous doubles at pc -- where the caller's `writes` holds.
template <int O>
__device__ __forceinline__ void symv_colsum(const double (&ca)[2][2][O], double (*lds)[6 * O * 64], int wave, int lane, bool writes,
                                            double *pc) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int k = 0; k < O; ++k) lds[wave][((h * 2 + e) * O + k) * 64 + lane] = ca[h][e][k];
    __syncthreads();
    if (wave < 2 && writes) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int k = 0; k < O; ++k) {
                const int idx = ((wave * 2 + e) * O + k) * 64 + lane;
                pc[e * O + k] = ((lds[0][idx] + lds[1][idx]) + lds[2][idx]) + lds[3][idx];
            }
    }
}

}  // namespace xm
