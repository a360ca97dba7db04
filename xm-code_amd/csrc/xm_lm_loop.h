// xm_lm_loop.h — the Levenberg-Marquardt loop of the solvers of sparse normal equations (xm_ba.hip, xm_gp.hip, xm_vgcalib.hip): Ceres's
// trust-region rules (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc), written once.  Host arithmetic only and no HIP include:
// what a solver launches and reads stands behind the hooks, and a script can stand there in place of a device (xm_lm_replay).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <optional>
#include <vector>

#include "../../include/xm_amd.h"

namespace xm {

constexpr double kLmRadius0 = 1e4;          // initial_trust_region_radius; mu = 1 / radius
constexpr double kLmRadiusMax = 1e16;       // max_trust_region_radius
constexpr double kLmRadiusMin = 1e-32;      // min_trust_region_radius: below it, XM_BA_NO_PROGRESS
constexpr double kLmMinQuality = 1e-3;      // min_relative_decrease: a step is accepted when its quality lies above
constexpr double kLmMinShrink = 1.0 / 3.0;  // an accepted step grows the radius by at most 3
constexpr double kLmNu0 = 2.0;              // a rejected step divides the radius by nu and doubles nu

struct LmRules {
    int max_iters;
    double function_tol, gradient_tol, parameter_tol;
    bool nonmonotonic = false;   // with max_nonmonotonic: the bundle adjustment's option
    int max_nonmonotonic = 0;
};

// Ceres's TrustRegionStepEvaluator (Conn, Gould & Toint, Trust-Region Methods, Algorithm 10.1.2): costs of the minimum, the current, the
// reference and the candidate point, the model decreases accumulated since the reference and the candidate, and the accepted steps
// since the last new minimum.  Without non-monotonic steps only the current cost takes part
struct LmStepEvaluator {
    bool nonmonotonic = false;
    int max_steps = 0;
    double minimum = 0.0, current = 0.0, reference = 0.0, candidate = 0.0, dm_ref = 0.0, dm_cand = 0.0;
    int steps = 0;
    void start(double cost) { minimum = current = reference = candidate = cost; }
    double quality(double cost_new, double model_dec) const {
        const double rho = (current - cost_new) / model_dec;
        return nonmonotonic ? std::max(rho, (reference - cost_new) / (dm_ref + model_dec)) : rho;
    }
    bool accepted(double cost_new, double model_dec) {   // true: the point is the one of least cost so far
        current = cost_new;
        if (!nonmonotonic) return true;
        dm_cand += model_dec; dm_ref += model_dec;
        const bool new_minimum = cost_new < minimum;
        if (new_minimum) {
            minimum = candidate = cost_new; dm_cand = 0.0; steps = 0;
        } else {
            ++steps;
            if (cost_new > candidate) { candidate = cost_new; dm_cand = 0.0; }
        }
        if (steps == max_steps) { reference = candidate; dm_ref = dm_cand; }
        return new_minimum;
    }
};

struct LmPoint { double cost, gmax, used; };   // at the current point: F, |J^T r|_inf, used observations
struct LmSolve { int iters; double relres; };
struct LmCandidate {   // F at x + d, sum r.Jd + |Jd|^2 / 2, |d|^2, |x|^2; solved = false: an invalid step, as one without a model decrease
    double cost_new, model, step2, x2;
    bool solved = true;
    std::optional<double> relres;   // set: it replaces the solve's
};
enum LmRead { kLmReadFirst, kLmReadNext, kLmReadFinal };
struct LmHooks {
    std::function<void(double mu, bool point_changed)> linearise;   // launches only
    std::function<LmPoint(LmRead which)> read_point;                // waits; kLmReadFirst: throws when the cost is not finite
    std::function<LmSolve()> solve;
    std::function<LmCandidate(double mu)> read_candidate;           // launches the candidate and waits
    std::function<void(bool new_best)> accept;                      // the candidate becomes the current point
    std::function<void()> to_best;                                  // non-monotonic steps only: the point of least cost becomes the current one
    std::function<bool()> out_of_time;                              // empty: no time limit
};
struct LmIteration { double cost, cost_new, mu; bool accepted; int pcg_iters; double relres; };
struct LmResult {
    int status = XM_BA_NO_CONVERGENCE, iters = 0, accepted = 0;
    int64_t pcg_total = 0;
    double initial_cost = 0.0, final_cost = 0.0, gmax = 0.0, n_used = 0.0, radius = kLmRadius0;
    int current = 0, returned = 0;          // which accepted step's point the loop ended on and which it went back to (0: the start)
    std::vector<LmIteration> trace;         // one per iteration
    std::vector<double> point_costs;        // one per point read, the final one included
};

// the first cap iterations as rows of six doubles (cost, candidate cost, mu, accepted, PCG iterations, relative residual); the rows written
inline int lm_copy_trace(const LmResult &r, double *trace, int cap) {
    if (!trace) return 0;
    const int rows = (int)std::min<size_t>(r.trace.size(), (size_t)std::max(cap, 0));
    for (int k = 0; k < rows; ++k) {
        const LmIteration &it = r.trace[(size_t)k];
        double *rec = trace + (size_t)6 * k;
        rec[0] = it.cost; rec[1] = it.cost_new; rec[2] = it.mu; rec[3] = it.accepted ? 1.0 : 0.0; rec[4] = it.pcg_iters; rec[5] = it.relres;
    }
    return rows;
}

inline LmResult lm_loop(const LmRules &R, const LmHooks &h) {
    LmResult o;
    LmStepEvaluator ev{R.nonmonotonic, R.max_nonmonotonic};
    double radius = kLmRadius0, nu = kLmNu0;
    bool fresh = true;   // the point changed: its cost and gradient have not been read yet
    auto read = [&](LmRead which) {
        const LmPoint p = h.read_point(which);
        ev.current = p.cost; o.gmax = p.gmax;
        o.point_costs.push_back(p.cost);
        fresh = false;
        return p;
    };
    for (;;) {
        const double mu = 1.0 / radius;
        h.linearise(mu, fresh);
        if (fresh) {
            const bool first = o.point_costs.empty();
            const LmPoint p = read(first ? kLmReadFirst : kLmReadNext);
            if (first) { o.initial_cost = p.cost; o.n_used = p.used; ev.start(p.cost); }
            if (p.gmax <= R.gradient_tol) { o.status = XM_BA_CONVERGED_GRADIENT; break; }
        }
        if (o.iters >= R.max_iters) { o.status = XM_BA_MAX_ITERATIONS; break; }
        if (h.out_of_time && h.out_of_time()) { o.status = XM_BA_TIME_LIMIT; break; }
        const LmSolve sv = h.solve();
        o.pcg_total += sv.iters;
        const LmCandidate c = h.read_candidate(mu);
        o.iters++;
        const double F = ev.current, Fn = c.cost_new, model_dec = -c.model;
        const bool valid = c.solved && std::isfinite(Fn) && model_dec > 0.0;
        const double rho = valid ? ev.quality(Fn, model_dec) : -1.0;
        const bool accept = valid && rho > kLmMinQuality;
        o.trace.push_back({F, Fn, mu, accept, sv.iters, c.relres.value_or(sv.relres)});
        if (c.solved && std::sqrt(c.step2) <= R.parameter_tol * (std::sqrt(c.x2) + R.parameter_tol)) { o.status = XM_BA_CONVERGED_PARAMETER; break; }
        if (accept) {
            o.current = ++o.accepted;
            radius = std::min(kLmRadiusMax, radius / std::max(kLmMinShrink, 1.0 - std::pow(2.0 * rho - 1.0, 3)));
            nu = kLmNu0;
            const bool new_best = ev.accepted(Fn, model_dec);
            if (new_best) o.returned = o.current;
            h.accept(new_best);
            fresh = true;   // linearised at the loop's top, or below when this step is the last
            if (std::fabs(F - Fn) <= R.function_tol * F) { o.status = XM_BA_CONVERGED_FUNCTION; break; }
        } else {
            radius /= nu;
            nu *= 2.0;
            if (radius < kLmRadiusMin) { o.status = XM_BA_NO_PROGRESS; break; }
        }
    }
    if (o.returned != o.current) {   // non-monotonic steps: the caller gets the point of least cost, and its cost and gradient
        h.to_best();
        fresh = true;
    }
    if (fresh) {   // the last accepted point: its cost and gradient
        h.linearise(1.0 / radius, true);
        read(kLmReadFinal);
    }
    o.final_cost = ev.current;
    o.radius = radius;
    return o;
}

}  // namespace xm
