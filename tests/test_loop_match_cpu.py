"""CPU checks of the two loop-closing searches (src/ORBmatcher.cc:290-403, 522-655): the Python restatements of tests/loop_cases.py,
which give the GPU tests their expected answers, are pinned against the C++ oracle where the oracle has the same rule, the
difference to the neighbouring overloads is shown on constructed inputs, and the new entry points exist and reject NULL handles."""
import ctypes as C

import numpy as np
import pytest

import kf_scene as ks
import loop_cases as lc


@pytest.mark.parametrize("nnodes", [7, 100])
@pytest.mark.parametrize("ratio", [0.75, 0.9])
@pytest.mark.parametrize("check_ori", [True, False])
def test_bow_restatement_equals_oracle_away_from_th_low(nnodes, ratio, check_ori):
    """SearchByBoW(pKF1, pKF2) accepts at bestDist1 < 50, SearchByBoW(pKF, F) - the oracle's - at <= 50: where no query's bestDist1 is
    exactly 50 the two are the same function of the flattened inputs, marks included."""
    import oracle_lib
    k0, d0, k2, d2 = lc.loop_pair()
    rng = np.random.default_rng(31)
    valid1, valid2 = rng.random(len(k0)) < 0.8, rng.random(len(k2)) < 0.5
    fidx, runs, qa, qd, _ = lc.bow_inputs(d0, k0["angle"], valid1, ks.feature_vector(d0, nnodes), ks.feature_vector(d2, nnodes), valid2)
    r = lc.restate_search_by_bow(k2["angle"], d2, fidx, runs, qa, qd, ratio, check_ori)
    assert (r["best1"] != 50).all()
    assert r["pre"] > 100 and r["contested"] >= 1 and (not check_ori or r["removed"] >= 1)
    onm, omatch, _ = oracle_lib.search_by_bow(d2, k2["angle"], fidx, runs, qd, qa, ratio, check_ori)
    assert r["nmatches"] == onm
    np.testing.assert_array_equal(r["match"], omatch)


@pytest.mark.parametrize("check_ori", [True, False])
def test_bow_boundary_49_and_50_bits(check_ori):
    """bestDist1 == 50 is rejected (:598 `<`) where the (pKF, F) overload accepts it (:228 `<=`); 49 is accepted by both"""
    import oracle_lib
    for nbits, mine, theirs in ((50, -1, 1), (49, 1, 1)):
        k2, d2, fidx, runs, qa, qd = lc.boundary_pair(nbits, np.random.default_rng(2))
        r = lc.restate_search_by_bow(k2["angle"], d2, fidx, runs, qa, qd, 0.75, check_ori)
        assert r["best1"][0] == nbits and r["match"][0] == mine and r["nmatches"] == (mine >= 0)
        onm, omatch, _ = oracle_lib.search_by_bow(d2, k2["angle"], fidx, runs, qd, qa, 0.75, check_ori)
        assert omatch[0] == theirs and onm == 1


def test_projection_restatement_equals_window_best_without_contention():
    """taken empty and no keypoint the best of two map points: every map point is searched as pslfe_kf_window_best searches it, and
    SearchByProjection(pKF, Scw, ...) keeps it at bestDist <= 50"""
    import oracle_lib
    (_, _), (k1, d1) = ks.keyframes()
    rng = np.random.default_rng(8)
    q = ks.proj_queries(k1, rng, th=10.0, jitter=3.0)
    qd = ks.noisy_desc(d1, rng, flips=30)
    bi, bd = oracle_lib.window_best(k1, d1, None, ks.BOUNDS, q, qd)
    want = np.where(bd <= 50, bi, -1)
    vals, counts = np.unique(want[want >= 0], return_counts=True)
    keep = ~np.isin(want, vals[counts > 1])
    assert keep.sum() > 500 and (want[keep] >= 0).sum() > 300
    r = lc.restate_search_by_projection_sim3(k1, d1, ks.BOUNDS, q[keep], qd[keep])
    np.testing.assert_array_equal(r["match"], want[keep])
    assert r["nmatches"] == (want[keep] >= 0).sum() and r["lost"] == 0
    back = np.full(len(k1), -1, np.int32)
    back[want[keep][want[keep] >= 0]] = np.nonzero(want[keep] >= 0)[0]
    np.testing.assert_array_equal(r["assigned"], back)


def test_projection_first_come_rule_by_hand():
    """two map points want keypoint 0: the first gets it, the second its runner-up (keypoint 1) when that is within TH_LOW and
    nothing otherwise; a keypoint taken on entry is never given away"""
    import oracle_lib
    rng = np.random.default_rng(4)
    k = np.zeros(3, oracle_lib.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = [100.0, 103.0, 400.0], [100.0, 101.0, 300.0], [1, 1, 1]
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    d = np.stack([base, lc.flip_bits(base, 20, rng), rng.integers(0, 256, 32, dtype=np.uint8)])
    q = np.zeros(2, oracle_lib.PROJQUERY_DTYPE)
    q["u"], q["v"], q["radius"], q["max_level"] = 101.0, 100.0, 12.0, 1
    qd = np.stack([lc.flip_bits(base, 3, rng), lc.flip_bits(base, 2, rng)])       # the second is even closer to keypoint 0
    r = lc.restate_search_by_projection_sim3(k, d, ks.BOUNDS, q, qd)
    assert r["match"].tolist() == [0, 1] and r["assigned"].tolist() == [0, 1, -1] and r["nmatches"] == 2 and r["lost"] == 1
    d[1] = lc.flip_bits(base, 90, rng)                                            # the runner-up is beyond TH_LOW now
    r = lc.restate_search_by_projection_sim3(k, d, ks.BOUNDS, q, qd)
    assert r["match"].tolist() == [0, -1] and r["nmatches"] == 1
    r = lc.restate_search_by_projection_sim3(k, d, ks.BOUNDS, q, qd, taken=np.array([1, 0, 0], np.uint8))
    assert r["match"].tolist() == [-1, -1] and r["assigned"].tolist() == [-1, -1, -1] and r["nmatches"] == 0


def test_new_entry_points_reject_null_handles():
    import psl_slam_amd as P
    lib = P.lib()
    nm = C.c_int(7)
    assert lib.pslfe_kf_search_by_bow(None, None, 0, None, 0, None, None, 0, C.c_float(0.75), 1, None, C.byref(nm)) == -1
    assert lib.pslfe_kf_search_by_bow_candidates(None, None, None, 1, None, None, None, None, None, C.c_float(0.75), 1, None, None) == -1
    assert lib.pslfe_kf_search_by_projection_sim3(None, None, 0, None, None, 0, None, None, None, C.byref(nm)) == -1
    assert b"pslfe_kf_search_by_projection_sim3" in lib.pslfe_last_error()
