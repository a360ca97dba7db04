"""CPU tests of the aggregates of the two-level preconditioner of the matrix-free CG form (xm_tuning_t.schur_solver = 3;
xm_schur_aggregate_plan, host only): on a sequential capture whose cameras are renumbered at random, the breadth-first plan still puts
stretches of the trajectory together.  No GPU."""
import numpy as np
import pytest

import xm_seqscene as sq


def test_plan_partitions_the_cameras_along_the_trajectory(xmamd):
    N, B = 3000, 64
    S = sq.gen_sequential(N, seed=1)
    T, pi = sq.renumber(S, seed=2)
    agg = xmamd.schur_aggregate_plan(T["cam"], T["lm"], n=N, B=B)
    assert agg.shape == (N,) and agg[0] == -1
    nc = -(-(N - 1) // B)
    red = agg[1:]
    assert red.min() == 0 and red.max() == nc - 1                       # every reduced camera in exactly one aggregate, n_c = ceil((N-1)/B)
    sizes = np.bincount(red, minlength=nc)
    assert sizes.max() <= B and sizes.sum() == N - 1
    assert np.array_equal(agg, xmamd.schur_aggregate_plan(T["cam"], T["lm"], n=N, B=B))   # deterministic
    # the cameras of an aggregate, in the original (trajectory) numbering, span a short stretch
    orig = np.empty(N, dtype=np.int64)
    orig[pi] = np.arange(N)
    spans = np.array([np.ptp(orig[np.where(agg == a)[0]]) for a in range(nc)])
    assert np.mean(spans <= 2 * B) >= 0.95, np.sort(spans)[-10:]
    # the same plan, up to the numbering, as on the unpermuted scene
    agg0 = xmamd.schur_aggregate_plan(S["cam"], S["lm"], n=N, B=B)
    assert np.array_equal(agg0, agg[pi])


def test_plan_appends_unreached_cameras_and_skips_heavy_landmarks(xmamd):
    # two chains joined only by a landmark seen by 70 cameras (heavy: not expanded) -> the breadth-first search stays in the first chain
    cam = [0, 1, 1, 2, 3, 4, 4, 5] + list(range(70))
    lm = [0, 0, 1, 1, 2, 2, 3, 3] + [4] * 70
    agg = xmamd.schur_aggregate_plan(np.array(cam), np.array(lm), n=70, B=2)
    assert agg[0] == -1 and agg[1] == 0 and agg[2] == 0                 # reached from camera 0: cameras 1, 2
    assert (agg[3:] >= 1).all() and np.bincount(agg[1:]).max() <= 2
    assert agg[3] == 1 and agg[4] == 1                                   # unreached, appended in index order


def test_plan_refuses_more_than_4096_aggregates_and_bad_sizes(xmamd):
    N = 5000
    S = sq.gen_sequential(N, per_cam=2, seed=3)
    assert xmamd.schur_aggregate_plan(S["cam"], S["lm"], n=N, B=2).max() == (N - 2) // 2
    with pytest.raises(xmamd.XmError, match="4096"):
        xmamd.schur_aggregate_plan(S["cam"], S["lm"], n=N, B=1)
    for B in (0, 65):
        with pytest.raises(xmamd.XmError, match="cameras per aggregate"):
            xmamd.schur_aggregate_plan(S["cam"], S["lm"], n=N, B=B)
    with pytest.raises(xmamd.XmError, match="out of range"):
        xmamd.schur_aggregate_plan(S["cam"], S["lm"], n=N - 1, B=64)
