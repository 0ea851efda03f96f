"""GPU parity of the two loop-closing searches through the C ABI against the restatements of tests/loop_cases.py:
pslfe_kf_search_by_bow / _candidates == ORBmatcher::SearchByBoW(pKF1, pKF2, ...) src/ORBmatcher.cc:522-655 and
pslfe_kf_search_by_projection_sim3 == ORBmatcher::SearchByProjection(pKF, Scw, ...) :290-403.  All comparisons are exact; every
case asserts on the restatement's output that it exercises what it is there for."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import kf_scene as ks
import loop_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _masks(k0, k2, seed=31):
    rng = np.random.default_rng(seed)
    return rng.random(len(k0)) < 0.8, rng.random(len(k2)) < 0.5     # about half of KF2's features have a good map point


@pytest.mark.parametrize("nnodes", [1, 7, 100])
@pytest.mark.parametrize("ratio", [0.75, 0.9])
@pytest.mark.parametrize("check_ori", [True, False])
def test_search_by_bow(nnodes, ratio, check_ori):
    """nnodes = 1: one node holds every feature (a run of several hundred rows walked by one wave)"""
    import psl_slam_amd as P
    k0, d0, k2, d2 = lc.loop_pair()
    valid1, valid2 = _masks(k0, k2)
    fidx, runs, qa, qd, _ = lc.bow_inputs(d0, k0["angle"], valid1, ks.feature_vector(d0, nnodes), ks.feature_vector(d2, nnodes), valid2)
    r = lc.restate_search_by_bow(k2["angle"], d2, fidx, runs, qa, qd, ratio, check_ori)
    assert r["pre"] > 100 and r["contested"] >= 1 and (not check_ori or r["removed"] >= 1)
    g = P.FrameGrid(2048, 1)
    g.set(0, k2, d2, ks.BOUNDS)
    nm, match = P.KeyFrameMatcher().SearchByBoW(g, 0, fidx, runs, qa, qd, ratio, check_ori)
    np.testing.assert_array_equal(match, r["match"])
    assert nm == r["nmatches"]
    assert valid2[match[match >= 0]].all() and len(set(match[match >= 0].tolist())) == (match >= 0).sum()


def test_search_by_bow_edges():
    """an empty query list, a node present in only one of the two vectors, and the 49 / 50-bit pair around TH_LOW"""
    import psl_slam_amd as P
    kf = P.KeyFrameMatcher()
    k0, d0, k2, d2 = lc.loop_pair()
    g = P.FrameGrid(2048, 1)
    g.set(0, k2, d2, ks.BOUNDS)
    nm, match = kf.SearchByBoW(g, 0, np.arange(10, dtype=np.int32), np.zeros((0, 2), np.int32), [], np.zeros((0, 32), np.uint8))
    assert nm == 0 and len(match) == 0
    valid1, valid2 = _masks(k0, k2)
    fv1, fv2 = ks.feature_vector(d0, 7), ks.feature_vector(d2, 7)
    del fv1[min(fv1)], fv2[max(fv2)]                                 # each vector has a node the other lacks
    fidx, runs, qa, qd, idx1 = lc.bow_inputs(d0, k0["angle"], valid1, fv1, fv2, valid2)
    assert 0 < len(qd) < valid1.sum()
    r = lc.restate_search_by_bow(k2["angle"], d2, fidx, runs, qa, qd, 0.75, True)
    nm, match = kf.SearchByBoW(g, 0, fidx, runs, qa, qd, 0.75, True)
    np.testing.assert_array_equal(match, r["match"])
    assert nm == r["nmatches"] and r["pre"] > 100
    for nbits, want in ((50, -1), (49, 1)):
        kb, db, fidx, runs, qa, qd = lc.boundary_pair(nbits, np.random.default_rng(2))
        g.set(0, kb, db, ks.BOUNDS)
        for ori in (True, False):
            r = lc.restate_search_by_bow(kb["angle"], db, fidx, runs, qa, qd, 0.75, ori)
            nm, match = kf.SearchByBoW(g, 0, fidx, runs, qa, qd, 0.75, ori)
            assert r["match"][0] == want and match[0] == want and nm == r["nmatches"] == (want >= 0)
    with pytest.raises(P.PslfeError):    # a run that leaves the feature vector
        kf.SearchByBoW(g, 0, np.arange(3, dtype=np.int32), [(2, 5)], [0.0], d0[:1])
    with pytest.raises(P.PslfeError):    # a feature in two nodes is not a FeatureVector
        kf.SearchByBoW(g, 0, np.array([0, 1, 1], np.int32), [(0, 2), (2, 1)], [0.0, 0.0], d0[:2])


def test_search_by_bow_full_store_in_one_node():
    """4096 KF2 features (the frame store's capacity), all with a map point, under one node: the longest run there can be"""
    import psl_slam_amd as P
    import oracle_lib
    rng = np.random.default_rng(29)
    n = 4096
    d2 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    k2 = np.zeros(n, oracle_lib.KEYPOINT_DTYPE)
    k2["x"], k2["y"], k2["angle"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n), rng.uniform(0, 360, n)
    src = rng.integers(0, n, 300)                      # with repeats: several queries want the same feature
    qd = ks.noisy_desc(d2[src], rng, flips=12)
    fidx = rng.permutation(n).astype(np.int32)
    runs = np.tile(np.array([[0, n]], np.int32), (len(src), 1))
    qa = rng.uniform(0, 360, len(src)).astype(np.float32)
    r = lc.restate_search_by_bow(k2["angle"], d2, fidx, runs, qa, qd, 0.75, True)
    assert r["pre"] > 100 and r["contested"] >= 1 and r["removed"] >= 1
    g = P.FrameGrid(n, 1)
    g.set(0, k2, d2, ks.BOUNDS)
    nm, match = P.KeyFrameMatcher().SearchByBoW(g, 0, fidx, runs, qa, qd, 0.75, True)
    np.testing.assert_array_equal(match, r["match"])
    assert nm == r["nmatches"]


def _candidates(C, nnodes, seed=17):
    """candidate 0 = KF2 of loop_pair, the others perturbed copies of it: fewer features, flipped descriptor bits, reshuffled
    map-point masks; the last one (C > 1) shares no node with the current keyframe"""
    k0, d0, k2, d2 = lc.loop_pair()
    valid1, valid2 = _masks(k0, k2)
    rng = np.random.default_rng(seed)
    fv1 = ks.feature_vector(d0, nnodes)
    cands, inputs = [], []
    for c in range(C):
        kc, dc, vc = (k2, d2, valid2) if c == 0 else lc.perturbed(k2, d2, valid2, rng, keep=len(k2) - 37 * (c % 9))
        fv2 = ks.feature_vector(dc, nnodes)
        if C > 1 and c == C - 1:
            fv2 = {nd + 1000: v for nd, v in fv2.items()}
        cands.append((kc, dc))
        inputs.append(lc.bow_inputs(d0, k0["angle"], valid1, fv1, fv2, vc))
    return cands, inputs


@pytest.mark.parametrize("C", [1, 5, 64])
def test_search_by_bow_candidates(C):
    """every candidate's rows equal the single call's and the restatement's"""
    import psl_slam_amd as P
    cands, inputs = _candidates(C, 7)
    g = P.FrameGrid(2048, C)
    for c, (kc, dc) in enumerate(cands):
        g.set(c, kc, dc, ks.BOUNDS)
    kf = P.KeyFrameMatcher()
    nms, matches = kf.SearchByBoWCandidates(g, list(range(C)), [i[0] for i in inputs], [i[1] for i in inputs], [i[2] for i in inputs],
                                            [i[3] for i in inputs])
    assert len({len(kc) for kc, _ in cands}) == min(C, 9)
    total = 0
    for c, (fidx, runs, qa, qd, _) in enumerate(inputs):
        r = lc.restate_search_by_bow(cands[c][0]["angle"], cands[c][1], fidx, runs, qa, qd, 0.75, True)
        np.testing.assert_array_equal(matches[c], r["match"])
        assert nms[c] == r["nmatches"]
        nm1, m1 = kf.SearchByBoW(g, c, fidx, runs, qa, qd)
        np.testing.assert_array_equal(matches[c], m1)
        assert nm1 == nms[c]
        if C > 1 and c == C - 1:
            assert len(qd) == 0 and len(fidx) > 0 and nms[c] == 0
        else:
            assert r["pre"] > 100 and r["contested"] >= 1 and r["removed"] >= 1
        total += nms[c]
    assert total > 100 * max(C - 1, 1)


@pytest.mark.parametrize("taken_mode", ["none", "sparse", "full"])
def test_search_by_projection_sim3(taken_mode):
    """th = 10 and six map points per keypoint, as mvpLoopMapPoints has them: the map points contend for the keypoints"""
    import psl_slam_amd as P
    (_, _), (k1, d1) = ks.keyframes()
    rng = np.random.default_rng(41)
    q, qd = lc.loop_map_points(k1, d1, rng, th=10.0, copies=6)
    assert len(q) == 6 * len(k1)
    taken = {"none": None, "sparse": (rng.random(len(k1)) < 0.2).astype(np.uint8), "full": np.ones(len(k1), np.uint8)}[taken_mode]
    r = lc.restate_search_by_projection_sim3(k1, d1, ks.BOUNDS, q, qd, taken)
    if taken_mode == "full":
        assert r["nmatches"] == 0
    else:
        assert r["nmatches"] >= 50 and r["lost"] >= 1
    g = P.FrameGrid(2048, 1)
    g.set(0, k1, d1, ks.BOUNDS)
    nm, match, assigned = P.KeyFrameMatcher().SearchByProjectionSim3(g, 0, q, qd, taken)
    np.testing.assert_array_equal(match, r["match"])
    np.testing.assert_array_equal(assigned, r["assigned"])
    assert nm == r["nmatches"]
    if taken is not None:
        assert not taken[match[match >= 0]].any()


def test_search_by_projection_sim3_long_lists_and_empty():
    """every keypoint carries the same descriptor and the windows are wide: each map point has far more acceptable candidates than
    its list caches, and the earlier map points have taken them - the window scan path; then no map points at all"""
    import psl_slam_amd as P
    (_, _), (k1, d1) = ks.keyframes()
    rng = np.random.default_rng(43)
    k = k1[:400].copy()
    k["octave"] = 1
    d = np.repeat(d1[:1], len(k), 0)
    q = ks.proj_queries(k[rng.permutation(len(k))[:300]], rng, th=60.0, jitter=1.0, p_drop=0.0)
    q["max_level"] = 1
    q["radius"] = 60.0
    qd = ks.noisy_desc(np.repeat(d1[:1], len(q), 0), rng, flips=10)
    r = lc.restate_search_by_projection_sim3(k, d, ks.BOUNDS, q, qd)
    assert r["nmatches"] >= 250 and r["lost"] >= 100 and r["deep"] >= 20
    g = P.FrameGrid(2048, 1)
    g.set(0, k, d, ks.BOUNDS)
    kf = P.KeyFrameMatcher()
    nm, match, assigned = kf.SearchByProjectionSim3(g, 0, q, qd)
    np.testing.assert_array_equal(match, r["match"])
    np.testing.assert_array_equal(assigned, r["assigned"])
    assert nm == r["nmatches"]
    nm, match, assigned = kf.SearchByProjectionSim3(g, 0, q[:0], qd[:0])
    assert nm == 0 and len(match) == 0 and (assigned == -1).all() and len(assigned) == len(k)


def test_search_by_projection_sim3_many_candidates_on_one_lane():
    """400 keypoints in one grid cell, so window candidate j is keypoint j and a wave's lane j % 64 evaluates it.  Keypoints 0, 64,
    ..., 384 - one lane's whole share - are the only ones within TH_LOW, with growing distances; seven identical map points take
    them one after the other.  The lane keeps four keys, so every list is cut short after four entries: map points 4, 5 and 6 must
    still find keypoints 256, 320 and 384."""
    import psl_slam_amd as P
    import oracle_lib
    rng = np.random.default_rng(47)
    n = 400
    k = np.zeros(n, oracle_lib.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = rng.uniform(100.5, 104.5, n), rng.uniform(100.5, 104.5, n), 1
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    near = list(range(0, n, 64))
    for t, i in enumerate(near):
        d[i] = lc.flip_bits(base, 3 * (t + 1), rng)
    q = np.zeros(len(near), oracle_lib.PROJQUERY_DTYPE)
    q["u"], q["v"], q["radius"], q["max_level"] = 102.0, 102.0, 20.0, 1
    qd = np.repeat(base[None, :], len(q), 0)
    grid = lc.KeyFrameGrid(k, ks.BOUNDS)
    assert grid.area(np.float32(102.0), np.float32(102.0), np.float32(20.0)) == list(range(n))   # candidate number == keypoint
    dist = np.array([lc._distance(a, lc._ints(base[None, :])[0]) for a in lc._ints(d)])
    ok = np.nonzero(dist <= 50)[0]
    assert ok.tolist() == near and len(near) == 7 and len({i % 64 for i in ok}) == 1      # 7 acceptable candidates, all on lane 0
    r = lc.restate_search_by_projection_sim3(k, d, ks.BOUNDS, q, qd)
    assert r["match"].tolist() == near and r["lost"] == 6
    g = P.FrameGrid(2048, 1)
    g.set(0, k, d, ks.BOUNDS)
    nm, match, assigned = P.KeyFrameMatcher().SearchByProjectionSim3(g, 0, q, qd)
    np.testing.assert_array_equal(match, r["match"])
    np.testing.assert_array_equal(assigned, r["assigned"])
    assert nm == 7


def test_cpp_consumer_equals_restatement(tmp_path):
    """tools/dropin/loop_main.cpp: the matcher sequence of ComputeSim3 on pslfe.hpp, built with g++, run as a child process"""
    exe = str(tmp_path / "loop_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "dropin", "loop_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    C, nnodes = 4, 7
    k0, d0, k2, d2 = lc.loop_pair()
    valid1, valid2 = _masks(k0, k2)
    rng = np.random.default_rng(19)
    node = lambda desc: ((desc[:, 0].astype(np.int32) * 7 + desc[:, 5]) % nnodes).astype(np.int32)   # kf_scene.feature_vector's hash
    cands = [(k2, d2, valid2)] + [lc.perturbed(k2, d2, valid2, rng, keep=len(k2) - 50 * c) for c in range(1, C)]
    proj = []
    for c in range(C):
        q, qd = lc.loop_map_points(k0, d0, rng, th=10.0, copies=3)
        proj.append((q, qd, (rng.random(len(k0)) < 0.1).astype(np.uint8)))
    blob = [struct.pack("<i4f", C, *ks.BOUNDS)]
    for k, d, good in [(k0, d0, valid1)] + cands:
        blob += [struct.pack("<i", len(k)), np.ascontiguousarray(k).tobytes(), np.ascontiguousarray(d, np.uint8).tobytes(), node(d).tobytes(),
                 np.ascontiguousarray(good, np.uint8).tobytes()]
    for q, qd, tk in proj:
        blob += [struct.pack("<i", len(q)), np.ascontiguousarray(q).tobytes(), qd.tobytes(), tk.tobytes()]
    path = str(tmp_path / "loop.bin")
    with open(path, "wb") as f:
        f.write(b"".join(blob))
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    fv1 = ks.feature_vector(d0, nnodes)
    want = []
    for kc, dc, vc in cands:
        fidx, runs, qa, qd, _ = lc.bow_inputs(d0, k0["angle"], valid1, fv1, ks.feature_vector(dc, nnodes), vc)
        want.append(lc.restate_search_by_bow(kc["angle"], dc, fidx, runs, qa, qd, 0.75, True))
    assert got["nmatches"] == [w["nmatches"] for w in want] and min(got["nmatches"]) > 50
    for c in range(C):
        assert got["match"][c] == want[c]["match"].tolist()
    best = int(np.argmax(got["nmatches"]))
    assert got["best"] == best
    r = lc.restate_search_by_projection_sim3(k0, d0, ks.BOUNDS, *proj[best])
    assert got["proj_nmatches"] == r["nmatches"] and r["nmatches"] >= 50 and r["lost"] >= 1
    assert got["proj_match"] == r["match"].tolist() and got["assigned"] == r["assigned"].tolist()
