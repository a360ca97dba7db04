"""CPU tests of the Levenberg-Marquardt loop that the bundle adjustment, the global positioning and the view-graph calibration share
(xm_lm_loop.h), run over a script of points and candidates in place of a device (xm_lm_replay, host only).  The expected values are
derived here from Ceres's rules: radius 1e4 and nu 2 at the start, mu = 1 / radius, a step is accepted when its quality lies above 1e-3,
then radius = min(1e16, radius / max(1/3, 1 - (2 rho - 1)^3)) and nu = 2, else radius /= nu, nu *= 2 and a radius below 1e-32 is no
progress.  The radius arithmetic is repeated in IEEE doubles, so mu is compared bit for bit."""
import numpy as np

from xm_ba_loss_numpy import StepEvaluator

ONE = (1.0, 1.0, 1.0)   # |d|^2, |x|^2, solved: far from the parameter tolerance


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def grow(radius, rho):
    return min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))


def descent(n, start, dec, model_dec):
    """n candidates from the cost `start`, each dec lower than the last, and the points the loop reads when it accepts them all"""
    costs = start - dec * np.arange(n + 1)
    return [(c, 1.0) for c in costs], [(c, -model_dec) + ONE for c in costs[1:]]


def test_invalid_steps_halve_quarter_eighth_the_radius_until_no_progress(xmamd):
    r = xmamd.lm_replay([(100.0, 1.0)], [(50.0, +1.0) + ONE] * 20)
    k = np.arange(1, 16)
    assert r["status"] == "no_progress" and r["iters"] == 15 and r["n_accepted"] == 0 and not r["accepted"].any()
    assert np.array_equal(bits(r["mu"]), bits(1.0 / (1e4 / 2.0 ** (k * (k - 1) // 2))))
    assert r["points_read"] == 1 and r["steps_read"] == 15 and (r["current"], r["returned"]) == (0, 0)
    assert 1e4 / 2.0 ** 105 > 1e-32 > 1e4 / 2.0 ** 120 == r["radius"]


def test_quality_one_triples_the_radius_up_to_1e16(xmamd):
    points, steps = descent(30, 1000.0, 1.0, 1.0)
    r = xmamd.lm_replay(points, steps, max_iters=30, function_tol=0.0)
    assert r["status"] == "max_iterations" and r["iters"] == 30 and r["accepted"].all() and r["points_read"] == 31
    radius = [1e4]
    for _ in range(30):
        radius.append(grow(radius[-1], 1.0))
    assert np.array_equal(bits(r["mu"]), bits(1.0 / np.array(radius[:30])))
    assert radius[25] < 1e16 and all(x == 1e16 for x in radius[26:]) and r["radius"] == 1e16
    assert np.isclose(radius[25], 1e4 * 3.0 ** 25, rtol=1e-13) and 3.0 ** 25 < 1e12 < 3.0 ** 26


def test_quality_one_half_keeps_the_radius(xmamd):
    points, steps = descent(6, 1000.0, 1.0, 2.0)
    r = xmamd.lm_replay(points, steps, max_iters=6, function_tol=0.0)
    assert r["accepted"].all() and np.array_equal(bits(r["mu"]), bits(np.full(6, 1.0 / 1e4))) and r["radius"] == 1e4


def test_the_bar_lies_between_two_to_the_minus_ten_and_minus_nine(xmamd):
    below = xmamd.lm_replay([(1000.0, 1.0)], [(999.0, -1024.0) + ONE], max_iters=1)
    assert below["status"] == "max_iterations" and list(below["accepted"]) == [False] and below["radius"] == 1e4 / 2.0
    assert (below["points_read"], below["current"]) == (1, 0)
    above = xmamd.lm_replay([(1000.0, 1.0), (999.0, 1.0)], [(999.0, -512.0) + ONE], max_iters=1, function_tol=0.0)
    assert above["status"] == "max_iterations" and list(above["accepted"]) == [True] and above["radius"] == grow(1e4, 2.0 ** -9)
    assert (above["points_read"], above["current"], above["returned"]) == (2, 1, 1)


def test_gradient_tolerance_at_the_first_read(xmamd):
    r = xmamd.lm_replay([(100.0, 1e-11)], [(90.0, -10.0) + ONE], gradient_tol=1e-10)
    assert r["status"] == "gradient_tolerance" and (r["iters"], r["steps_read"], r["points_read"]) == (0, 0, 1)


def test_no_iteration_allowed(xmamd):
    r = xmamd.lm_replay([(100.0, 1.0)], [(90.0, -10.0) + ONE], max_iters=0)
    assert r["status"] == "max_iterations" and (r["iters"], r["steps_read"], r["points_read"]) == (0, 0, 1)


def test_parameter_tolerance_comes_before_acceptance_and_only_for_a_solved_step(xmamd):
    r = xmamd.lm_replay([(100.0, 1.0)], [(90.0, -10.0, 0.0, 1.0, 1.0)])
    assert r["status"] == "parameter_tolerance" and r["iters"] == 1 and r["n_accepted"] == 0 and list(r["accepted"]) == [True]
    assert (r["current"], r["returned"], r["points_read"]) == (0, 0, 1)   # the verdict is recorded, the step is not taken
    r = xmamd.lm_replay([(100.0, 1.0)], [(90.0, -10.0, 0.0, 1.0, 0.0)], max_iters=1)
    assert r["status"] == "max_iterations" and list(r["accepted"]) == [False] and r["radius"] == 1e4 / 2.0


def test_function_tolerance_after_acceptance_reads_the_final_point(xmamd):
    r = xmamd.lm_replay([(100.0, 1.0), (99.99995, 1.0)], [(99.99995, -(100.0 - 99.99995)) + ONE], function_tol=1e-6)
    assert r["status"] == "function_tolerance" and r["iters"] == 1 and list(r["accepted"]) == [True]
    assert (r["points_read"], r["steps_read"], r["current"], r["returned"]) == (2, 1, 1, 1)


def test_a_script_that_runs_out_is_an_argument_error(xmamd):
    for points, steps in (([], []), ([(100.0, 1.0)], []), ([(100.0, 1.0)], [(90.0, -10.0) + ONE])):
        try:
            xmamd.lm_replay(points, steps, function_tol=0.0)
        except xmamd.XmError as e:
            assert "error -2" in str(e) and "xm_lm_replay" in str(e)
        else:
            raise AssertionError("no error")


def model(points, steps, max_iters, nonmonotonic, max_nonmonotonic):
    """the rules above over the script with tests/xm_ba_loss_numpy.py's StepEvaluator (no tolerance is met in these scripts)"""
    radius, nu, ip, accepted, mus, flags = 1e4, 2.0, 1, 0, [], []
    F = points[0][0]
    ev = StepEvaluator(F, max_nonmonotonic)
    cur = best = 0
    for it in range(max_iters):
        Fn, m = steps[it][0], -steps[it][1]
        mus.append(1.0 / radius)
        rho = ev.quality(Fn, m) if nonmonotonic else (F - Fn) / m
        flags.append(m > 0.0 and rho > 1e-3)
        if flags[-1]:
            radius, nu, accepted = grow(radius, rho), 2.0, accepted + 1
            cur = accepted
            if ev.accepted(Fn, m) or not nonmonotonic:
                best = cur
            F = points[ip][0]; ip += 1
            assert F == Fn
        else:
            radius, nu = radius / nu, 2.0 * nu
    return dict(mu=np.array(mus), accepted=flags, current=cur, returned=best, points_read=ip + (best != cur), radius=radius, ev=ev)


# from cost 100 with max_nonmonotonic = 2: a new minimum (90); up to 95, accepted against the reference 100 alone; 93, the second step
# without a new minimum: the reference becomes the candidate 95; 99, which neither quality accepts; 92, accepted, not the least
NM_STEPS = [(90.0, -10.0) + ONE, (95.0, -5.0) + ONE, (93.0, -4.0) + ONE, (99.0, -2.0) + ONE, (92.0, -2.0) + ONE]


def test_nonmonotonic_steps_follow_the_step_evaluator(xmamd):
    points = [(c, 1.0) for c in (100.0, 90.0, 95.0, 93.0, 92.0, 90.0)]
    exp = model(points, NM_STEPS, 5, True, 2)
    assert exp["accepted"] == [True, True, True, False, True] and (exp["current"], exp["returned"]) == (4, 1)
    assert (90.0 - 95.0) / 5.0 < 1e-3 < (100.0 - 95.0) / 15.0          # the second step: up, on the reference's account
    assert (exp["ev"].reference, exp["ev"].dm_ref) == (95.0, 6.0)       # reset at the third step (dm_ref = 4), then + 2
    assert max((93.0 - 99.0) / 2.0, (95.0 - 99.0) / 6.0) < 1e-3         # the fourth step: rejected by both
    r = xmamd.lm_replay(points, NM_STEPS, max_iters=5, nonmonotonic=True, max_nonmonotonic=2)
    assert r["status"] == "max_iterations" and list(r["accepted"]) == exp["accepted"] and r["n_accepted"] == 4
    assert np.array_equal(bits(r["mu"]), bits(exp["mu"])) and r["radius"] == exp["radius"]
    assert (r["current"], r["returned"]) == (4, 1) and r["points_read"] == exp["points_read"] == 6 and r["steps_read"] == 5


def test_the_same_script_without_nonmonotonic_steps_follows_the_plain_rule(xmamd):
    points = [(100.0, 1.0), (90.0, 1.0)]
    exp = model(points, NM_STEPS, 5, False, 2)
    assert exp["accepted"] == [True, False, False, False, False]
    r = xmamd.lm_replay(points, NM_STEPS, max_iters=5, nonmonotonic=False, max_nonmonotonic=2)
    assert r["status"] == "max_iterations" and list(r["accepted"]) == exp["accepted"]
    assert np.array_equal(bits(r["mu"]), bits(exp["mu"])) and r["radius"] == exp["radius"] == grow(1e4, 1.0) / 2.0 ** 10
    assert (r["current"], r["returned"], r["points_read"], r["steps_read"]) == (1, 1, 2, 5)
