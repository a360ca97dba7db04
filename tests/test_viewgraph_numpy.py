"""CPU tests of the view-graph filter's restatements (tests/xm_viewgraph_numpy.py): the vectorised contract (b), run_numpy, which the device
is tested against, equals the sequential restatement (a) of the reference's C++ EXACTLY -- on the recorded SIMPLE2-derived case in both
passes, on a few hundred seeded small cases that cover every model and every rule, and on the hand-made cases of the GPU tests; the recorded
file holds what run_numpy gives; the hand-made cases give what they are built for.  Nothing here was compared with the reference's binary."""
import collections

import numpy as np

import xm_viewgraph_numpy as vn

ARRAYS = ("inlier", "pair_inliers", "pair_status", "registered", "moff_out", "f1_out", "f2_out")


def _same(a, b, what=""):
    for f in ARRAYS:
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), (what, f)
    assert a["info"] == b["info"] and tuple(sorted(a["info"])) == tuple(sorted(vn.INFO_FIELDS)), what


def test_recorded_case_both_restatements_and_the_file():
    a, ra, b, rb, rec = vn.load_case()
    assert vn.digest(a) == str(rec["digest"])
    assert rec["sizes"].tolist() == [a["foff"].size - 1, a["foff"][-1], a["pi"].size, a["f1"].size] == [93, 64549, 4210, 261680]
    _same(vn.sequential(a), ra, "pass A")
    _same(vn.sequential(b), rb, "pass B")
    assert np.array_equal(np.packbits(ra["inlier"]), rec["a_inlier_bits"]) and np.array_equal(np.diff(ra["pair_inliers"], prepend=np.int32(0)), rec["a_pair_inliers_diff"])
    for p, r in (("a", ra), ("b", rb)):
        assert np.array_equal(r["pair_status"], rec[p + "_status"]) and np.array_equal(r["registered"], rec[p + "_registered"])
        assert [r["info"][k] for k in vn.INFO_FIELDS] == rec[p + "_info"].tolist() and vn.digest_matches(r) == str(rec[p + "_matches"])
    # every status and every model occur; two images leave the largest component in pass B and their own pair ends outside it
    assert set(ra["pair_status"].tolist()) == {vn.VALID, vn.INVALID_IN, vn.FEW_INLIERS, vn.LOW_RATIO}
    assert set(rb["pair_status"].tolist()) == {vn.VALID, vn.INVALID_IN, vn.ROTATION, vn.OUTSIDE}
    assert set(a["model"].tolist()) == {vn.NONE, vn.E_, vn.F_, vn.H_}
    gone = np.flatnonzero((ra["registered"] != 0) & (rb["registered"] == 0))
    assert gone.tolist() == sorted(a["gone"].tolist()) and rb["info"]["largest"] == 91 and rb["info"]["components"] == 2
    # pass B reads pass A's output: its matches are A's kept inliers, all of them inliers again
    assert rb["info"]["matches"] == ra["info"]["matches_out"] == rb["info"]["inliers"] and np.array_equal(b["valid_in"], ra["pair_status"] == vn.VALID)


def test_seeded_cases_cover_every_model_and_rule():
    status, scored = collections.Counter(), collections.Counter()
    ties = fallback = nan = 0
    for seed in range(300):
        c = vn.random_case(seed)
        ra = vn.run_numpy(c)
        _same(vn.sequential(c), ra, seed)
        status.update(("A", s) for s in ra["pair_status"].tolist())
        for k in np.flatnonzero(ra["pair_inliers"] > 0):
            scored[int(c["model"][k])] += 1
        f = np.flatnonzero(c["model"] == vn.F_)
        fallback += int(np.sum(np.all(c["FH"][f][:, 0] == 0.0, axis=1)))
        nan += int(np.isnan(c["trel"]).any())
        b = vn.next_pass(c, ra, c["rot_true"])
        if seed % 2:
            b["registered_in"] = (np.arange(c["foff"].size - 1) % 3 != 1).astype(np.uint8)
        rb = vn.run_numpy(b)
        _same(vn.sequential(b), rb, (seed, "pass B"))
        status.update(("B", s) for s in rb["pair_status"].tolist())
    for s in (vn.VALID, vn.INVALID_IN, vn.FEW_INLIERS, vn.LOW_RATIO, vn.OUTSIDE):
        assert status[("A", s)] > 20, s
    for s in (vn.VALID, vn.INVALID_IN, vn.ROTATION, vn.OUTSIDE):
        assert status[("B", s)] > 0, s
    assert min(scored[vn.E_], scored[vn.F_], scored[vn.H_]) > 100 and scored[vn.NONE] == 0 and fallback > 5 and nan > 5


def test_hand_made_cases():
    P = vn.gpu_cases(vn.LIMITS)
    ref = {}
    for name, c in P.items():
        ref[name] = vn.run_numpy(c)
        if name != "sizes":                                  # (101 000 matches: restatement (a) runs over its small pairs below)
            _same(vn.sequential(c), ref[name], name)
    c = P["sizes"]
    cnt = np.diff(c["moff"])
    small = np.flatnonzero(cnt <= 300)
    d = dict(c)
    d["moff"] = np.concatenate([[0], np.cumsum(cnt[small])]).astype(np.int64)
    idx = np.concatenate([np.arange(c["moff"][k], c["moff"][k + 1]) for k in small])
    d["f1"], d["f2"] = c["f1"][idx], c["f2"][idx]
    for k in ("pi", "pj", "model", "Rrel", "trel", "FH"):
        d[k] = c[k][small]
    _same(vn.sequential(d), vn.run_numpy(d), "sizes, the small pairs")
    assert np.array_equal(vn.run_numpy(d)["inlier"], ref["sizes"]["inlier"][idx])
    i = ref["sizes"]["info"]
    assert i["pairs_wave"] > 0 and i["pairs_group"] > 0 and i["pairs_workspace"] >= 6
    _, want = vn.essential_edges_case()
    assert np.array_equal(ref["essential_edges"]["inlier"], want)
    _, want = vn.fundamental_edges_case()
    assert np.array_equal(ref["fundamental_edges"]["inlier"], want) and ref["fundamental_edges"]["pair_inliers"].tolist() == [0, 3, 3, 0, 2]
    assert ref["rules"]["pair_status"].tolist() == [vn.FEW_INLIERS, vn.VALID, vn.VALID, vn.LOW_RATIO, vn.FEW_INLIERS, vn.INVALID_IN, vn.FEW_INLIERS, vn.OUTSIDE]
    assert ref["rules_no_minimum"]["pair_status"].tolist() == [0, 0, 0, vn.LOW_RATIO, vn.LOW_RATIO, vn.INVALID_IN, vn.OUTSIDE, vn.OUTSIDE]
    assert ref["rotation"]["pair_status"].tolist() == [0, 0, vn.ROTATION, 0, 0, 0, 0, 0] and ref["rotation_off"]["pair_status"].tolist() == [0] * 8
    # the pair at the threshold: its cosine IS the option, and one ulp more drops it
    c = P["rotation"]
    up = dict(c, options=dict(c["options"], cos_max_rotation_error=np.nextafter(c["options"]["cos_max_rotation_error"], 2.0)))
    assert vn.run_numpy(up)["pair_status"].tolist()[1] == vn.ROTATION
    assert ref["two_equal"]["registered"].tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 1] and ref["none_valid"]["info"]["largest"] == 0
    assert ref["chain"]["info"]["largest"] == 1500 and ref["isolated_twice"]["registered"].tolist() == [0, 1, 1, 0, 1, 0, 0]


def test_permutation_and_errors():
    c = vn.random_case(4)
    r = vn.run_numpy(c)
    d, order, idx = vn.permuted(c, 8)
    q = vn.run_numpy(d)
    assert np.array_equal(q["registered"], r["registered"]) and np.array_equal(q["pair_status"], r["pair_status"][order])
    assert np.array_equal(q["inlier"], r["inlier"][idx]) and q["info"] == r["info"]
    bad = dict(c); bad["f2"] = c["f2"].copy(); bad["f2"][3] = 10 ** 6
    for fn in (vn.run_numpy, vn.sequential):
        try:
            fn(bad)
            raise AssertionError("accepted")
        except ValueError as e:
            assert "match 3" in str(e)
