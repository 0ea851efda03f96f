"""GPU parity of the keyframe database (pslfe_kfdb, the KeyFrameDatabase mirrors) with the restatement of
src/KeyFrameDatabase.cc and DBoW2::L1Scoring::score in tests/kfdb_cases.py.  Every comparison is exact: integer fields, f64 scores as
bytes, candidate lists with their order.  Every case asserts on the restatement's output that it exercises what it is there for."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import kfdb_cases as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bow(vocab, desc):
    import oracle_lib
    o = oracle_lib.compute_bow(*vocab, desc, 4)
    return o["bow_id"], o["bow_val"]


@pytest.fixture(scope="module")
def world():
    W = kc.seeded_world(2)
    bows = {s: _bow(W["vocab"], d) for s, d in W["desc"].items()}
    qbows = [_bow(W["vocab"], q["desc"]) for q in W["queries"]]
    return W, bows, qbows


def _check_query(db, rows, seq, q, exclude=()):
    """one query against the dense restatement; returns (words, max_common) of the device"""
    K = db.max_keyframes
    ex = None
    if exclude:
        ex = np.zeros(K, np.uint8)
        ex[list(exclude)] = 1
    words, first, score, maxc = db.query(q, ex)
    dense, rmax = kc.dense_query(rows, q, set(exclude))
    rw, rf, rs = np.zeros(K, np.int32), np.full(K, -1, np.int32), np.zeros(K, np.float64)
    for s, (w, f, sc) in dense.items():
        rw[s], rf[s], rs[s] = w, f, sc
    np.testing.assert_array_equal(words, rw)
    np.testing.assert_array_equal(first, rf)
    assert score.tobytes() == rs.tobytes()
    assert maxc == rmax
    return words, maxc


@pytest.mark.parametrize("max_words", [300, 4096])
def test_geometry_cases(max_words):
    """row lengths 0, 1, 63, 64, 65, 129, max_words x query lengths 0, 1, 65, max_words; 43 slots (no multiple of the 4 waves of a
    workgroup), 41 of them live"""
    import psl_slam_amd as P
    rows, queries, slot = kc.geometry_case(max_words)
    assert sorted(len(r[0]) for r in rows.values())[:2] == [0, 1] and {63, 64, 65, 129, max_words} <= {len(r[0]) for r in rows.values()}
    assert [len(q[0]) for q in queries] == [0, 1, 65, max_words, 65]
    db = P.KeyFrameDatabase(43, max_words)
    for s in sorted(rows):
        db.add(s, rows[s])
    seq = {s: s for s in rows}
    res = [_check_query(db, rows, seq, q) for q in queries]
    assert res[0][1] == 0 and not res[0][0].any()                                   # the empty query
    assert res[1][0][slot["len65"]] == 1 and rows[slot["len65"]][0][-1] == queries[1][0][0]   # one common word, the row's last entry
    r129 = rows[slot["len129"]][0]
    assert r129[63] in queries[2][0] and r129[64] in queries[2][0] and res[2][0][slot["len129"]] == 2   # both sides of a chunk boundary
    assert res[3][0][slot["full"]] == max_words == res[3][1]                        # all in common
    assert res[4][1] == 0 and not res[4][0].any()                                   # none in common
    s = db.Score(queries[3], [slot["full"]])
    assert abs(s[0] - 1.0) <= (1.5 * (max_words - 1) + 1) * 2.0 ** -53 and s[0] == kc.score(queries[3], rows[slot["full"]])
    db.close()


def _apply(db, W, bows):
    for op, s in W["ops"]:
        if op == "add":
            db.add(s, bows[s])
        else:
            db.erase(s)


def test_seeded_world_queries_scores_and_candidates(world):
    """adds in a shuffled order, an erased slot in the middle of the live range, a slot erased and added again, connected keyframes
    as the exclusion mask: the raw query, Score, and both candidate lists against the inverted-file restatement"""
    import psl_slam_amd as P
    W, bows, qbows = world
    stats = {}
    ref, want = kc.run_world(W, bows, qbows, stats)
    assert sum(1 for r in want if r["loop"]) * 4 >= 3 * len(want) and sum(1 for r in want if r["reloc"]) * 4 >= 3 * len(want)
    assert stats.get("filtered", 0) >= 1 and stats.get("duplicates", 0) >= 1
    db = P.KeyFrameDatabase(W["nslots"] + 3, 512)
    _apply(db, W, bows)
    live, seq = db.state()
    assert [s for s in range(db.max_keyframes) if live[s]] == sorted(ref.kf) and all(seq[s] == ref.seq[s] for s in ref.kf)
    lo, hi = min(ref.kf), max(ref.kf)
    assert any(lo < s < hi for s in W["erased"]) and ref.seq[W["readded"]] == max(ref.seq.values())
    ties = hidden_max = readded_late = 0
    for q, qb in zip(W["queries"], qbows):
        words, maxc = _check_query(db, ref.rows(), ref.seq, qb, q["connected"])
        allw, _ = _check_query(db, ref.rows(), ref.seq, qb)
        hidden_max += int(allw.max() > maxc)            # an excluded slot that would have held the maximum
        dense, _ = kc.dense_query(ref.rows(), qb, set(q["connected"]))
        order = kc.dense_sharing(dense, ref.seq)
        firsts = [dense[s][1] for s in order]
        ties += int(len(set(firsts)) < len(firsts))     # slots with an equal first_word: placed by their add sequence
        same = [s for s in order if dense[s][1] == dense[W["readded"]][1]] if W["readded"] in order else []
        readded_late += int(len(same) > 1 and same[-1] == W["readded"])
    assert ties >= 1 and hidden_max >= 1 and readded_late >= 1
    db2 = P.KeyFrameDatabase(W["nslots"] + 3, 512)     # the candidate lists need the per-slot scores of one run of queries
    _apply(db2, W, bows)
    for q, qb, r in zip(W["queries"], qbows, want):
        sc = db2.Score(qb, q["connected"])
        assert sc.tobytes() == np.array([kc.score(qb, bows[s]) for s in q["connected"]], np.float64).tobytes()
        min_score = np.float32(1)
        for x in sc:
            if np.float32(x) < min_score:
                min_score = np.float32(x)
        assert min_score.tobytes() == r["min_score"].tobytes()
        assert db2.DetectLoopCandidates(qb, q["connected"], min_score, q["neighbours"]) == r["loop"]
        assert db2.DetectRelocalizationCandidates(qb, q["neighbours"]) == r["reloc"]
    db.close()
    db2.close()


def test_identical_vectors_clear_and_empty_database(world):
    import psl_slam_amd as P
    W, bows, qbows = world
    v = bows[0]
    db = P.KeyFrameDatabase(5, 512)
    words, first, score, maxc = db.query(v)
    assert maxc == 0 and not words.any() and (first == -1).all() and not score.any()
    db.add(3, v)
    db.add(1, v)
    words, first, score, maxc = db.query(v)
    assert maxc == len(v[0]) and words[1] == words[3] == maxc and first[1] == first[3] == v[0][0]
    assert score[1] == score[3] == kc.score(v, v)
    assert db.DetectRelocalizationCandidates(v, {}) == [3, 1]      # equal first_word: the order of the adds
    db.erase(0)                                                    # a dead slot: nothing happens
    db.clear()
    assert not db.state()[0].any() and db.query(v)[3] == 0
    db.add(3, v)                                                   # free again after clear
    assert db.query(v)[3] == len(v[0])
    db.close()


def test_words_equal_to_min_common_words_are_rejected():
    """maxCommonWords = 10 -> minCommonWords = (int)(10 * 0.8f) = 8; the slot with exactly 8 common words is not scored although
    it would score best (strict >)"""
    import psl_slam_amd as P
    q = kc.hand_bow(np.arange(10), np.ones(10))
    rows = {0: kc.hand_bow(np.arange(0, 40), seed=1),        # 10 common words, much weight elsewhere
            1: kc.hand_bow(np.arange(0, 8), np.ones(8)),     # 8 common words, all its weight on them
            2: kc.hand_bow(np.arange(0, 9), np.ones(9))}     # 9
    w = kc.RefWorld()
    db = P.KeyFrameDatabase(6, 64)
    for s, r in rows.items():
        w.add(s, r)
        db.add(s, r)
    assert kc.score(q, rows[1]) > kc.score(q, rows[0])
    words, _, _, maxc = db.query(q)
    assert maxc == 10 and list(words[:3]) == [10, 8, 9]
    want = w.reloc(q, {})
    assert 1 not in want and 2 in want
    assert db.DetectRelocalizationCandidates(q, {}) == want
    assert db.DetectLoopCandidates(q, [], 0.0, {}) == w.loop(q, [], 0.0, {}) and 1 not in w.loop(q, [], 0.0, {})
    db.close()


@pytest.mark.parametrize("with_query_a", [True, False])
def test_stale_reloc_score_of_a_neighbour(with_query_a):
    """Query A scores slot 0.  Query B shares one word with slot 0 (below minCommonWords) and ten with slot 1, whose neighbour is
    slot 0: slot 0 counts in B's accumulation with the mRelocScore query A left (src/KeyFrameDatabase.cc:273-281 has no
    minCommonWords test) and, scoring higher, becomes the candidate.  Without query A the score is the defined initial 0.0f."""
    import psl_slam_amd as P
    rows = {0: kc.hand_bow(np.arange(100, 120), np.ones(20)), 1: kc.hand_bow(np.arange(0, 30), seed=3)}
    qa = kc.hand_bow(np.arange(100, 120), np.ones(20))
    qb = kc.hand_bow(np.concatenate([np.arange(0, 10), [100]]), np.ones(11))
    neighbours = {1: [0]}
    w = kc.RefWorld()
    db = P.KeyFrameDatabase(4, 64)
    for s, r in rows.items():
        w.add(s, r)
        db.add(s, r)
    if with_query_a:
        assert db.DetectRelocalizationCandidates(qa, neighbours) == w.reloc(qa, neighbours) == [0]
    want = w.reloc(qb, neighbours)
    assert want == ([0] if with_query_a else [1])
    assert db.DetectRelocalizationCandidates(qb, neighbours) == want
    db.erase(0)          # a slot that is used again starts from 0.0f
    w.erase(0)
    db.add(0, rows[0])
    w.add(0, rows[0])
    assert db.DetectRelocalizationCandidates(qb, neighbours) == w.reloc(qb, neighbours) == [1]
    db.close()


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def test_device_path_from_compute_bow_device(world):
    """9 frames through pslfe_compute_bow_device, added device to device at a stride above every count; 3 queries in one launch with
    a mask per query == three one-query calls == the restatement; Score == the query's scores"""
    import psl_slam_amd as P
    W, bows, qbows = world
    ctx = P.default_context()
    V = P.ORBVocabulary(*W["vocab"], ctx=ctx)
    slots = sorted(W["desc"])[:9]
    nf, stride = 12, 512
    desc, counts = np.zeros((nf, stride, 32), np.uint8), np.zeros(nf, np.int32)
    for f, d in enumerate([W["desc"][s] for s in slots] + [q["desc"] for q in W["queries"][:3]]):
        desc[f, :len(d)], counts[f] = d, len(d)
    assert counts.max() < stride
    i4 = lambda *shape: _dev(ctx, np.zeros(shape, np.int32))
    f8 = lambda *shape: _dev(ctx, np.zeros(shape, np.float64))
    d_desc, d_counts = _dev(ctx, desc), _dev(ctx, counts)
    d_fword, d_fw, d_fnid, d_bid, d_bval, d_bstart, d_nbow = i4(nf, stride), f8(nf, stride), i4(nf, stride), i4(nf, stride), f8(nf, stride), i4(nf, stride + 1), i4(nf)
    d_fvn, d_fvs, d_fvi, d_nfv = i4(nf, stride), i4(nf, stride + 1), i4(nf, stride), i4(nf)
    P._check(P.lib().pslfe_compute_bow_device(V._h, *[C.c_void_p(x) for x in (d_desc, d_counts)], nf, stride, 4,
                                              *[C.c_void_p(x) for x in (d_fword, d_fw, d_fnid, d_bid, d_bval, d_bstart, d_nbow, d_fvn, d_fvs, d_fvi, d_nfv)]),
             "pslfe_compute_bow_device")
    K = 11
    db = P.KeyFrameDatabase(K, stride, ctx=ctx)
    db.add_device(1, d_bid, d_bval, d_nbow, 9, stride)           # slots 1 .. 9
    live, seq = db.state()
    assert list(np.flatnonzero(live)) == list(range(1, 10)) and list(seq[1:10]) == list(range(9))
    exclude = np.zeros((3, K), np.uint8)
    exclude[0, 2] = exclude[1, [1, 5, 9]] = 1
    d_ex, d_words, d_first, d_score, d_maxc = _dev(ctx, exclude), i4(3, K), i4(3, K), f8(3, K), i4(3)
    db.query_device(d_bid + 9 * stride * 4, d_bval + 9 * stride * 8, d_nbow + 9 * 4, 3, stride, d_ex, d_words, d_first, d_score, d_maxc)
    ctx.synchronize()
    words, first = _down(P, ctx, d_words, np.zeros((3, K), np.int32)), _down(P, ctx, d_first, np.zeros((3, K), np.int32))
    score, maxc = _down(P, ctx, d_score, np.zeros((3, K), np.float64)), _down(P, ctx, d_maxc, np.zeros(3, np.int32))
    rows = {1 + f: bows[s] for f, s in enumerate(slots)}
    for q in range(3):
        w1, f1, s1, m1 = db.query(qbows[q], exclude[q])
        np.testing.assert_array_equal(words[q], w1)
        np.testing.assert_array_equal(first[q], f1)
        assert score[q].tobytes() == s1.tobytes() and maxc[q] == m1 > 0
        ex = set(int(s) for s in np.flatnonzero(exclude[q]))
        _check_query(db, rows, None, qbows[q], ex)
        some = [9, 1, 4, 4]
        assert db.Score(qbows[q], some).tobytes() == db.query(qbows[q])[2][some].tobytes()
    for d in (d_desc, d_counts, d_fword, d_fw, d_fnid, d_bid, d_bval, d_bstart, d_nbow, d_fvn, d_fvs, d_fvi, d_nfv, d_ex, d_words, d_first, d_score, d_maxc):
        ctx.device_free(d)
    db.close()
    V.close()


def test_errors():
    import psl_slam_amd as P
    db = P.KeyFrameDatabase(4, 8)
    v = kc.hand_bow([1, 5, 9])
    db.add(2, v)
    for bad in (lambda: db.add(2, v),                                   # a live slot
                lambda: db.add(4, v), lambda: db.add(-1, v),             # slot out of range
                lambda: db.erase(4),
                lambda: db.add(0, kc.hand_bow(np.arange(9))),            # n > max_words
                lambda: db.query(kc.hand_bow(np.arange(9))),
                lambda: db.Score(v, [1]),                                # a dead slot
                lambda: db.Score(v, [7]),
                lambda: db.add(0, (np.array([5, 1, 9], np.int32), v[1])),    # ids not ascending
                lambda: db.add(0, (np.array([1, 1, 9], np.int32), v[1])),
                lambda: db.query((np.array([3, 2], np.int32), np.array([0.5, 0.5]))),
                lambda: P.KeyFrameDatabase(0, 8), lambda: P.KeyFrameDatabase(4, 4097)):
        with pytest.raises(P.PslfeError):
            bad()
    assert db.state()[0].tolist() == [0, 0, 1, 0]       # nothing of the above changed the database
    assert db.query(v)[3] == 3 and db.Score(v, []).shape == (0,)
    db.close()


def test_cpp_consumer_equals_restatement(world, tmp_path):
    """tools/dropin/kfdb_main.cpp: add / erase / Score / both Detect* on pslfe.hpp, built with g++, run as a child process"""
    W, bows, qbows = world
    exe = str(tmp_path / "kfdb_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "dropin", "kfdb_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    K = W["nslots"] + 3
    blob = [struct.pack("<iii", K, 512, len(W["ops"]))]
    for op, s in W["ops"]:
        ids, vals = bows[s] if op == "add" else kc.hand_bow([])
        blob += [struct.pack("<iii", 0 if op == "add" else 1, s, len(ids)), np.ascontiguousarray(ids, np.int32).tobytes(),
                 np.ascontiguousarray(vals, np.float64).tobytes()]
    neighbours = W["queries"][0]["neighbours"]
    for s in range(K):
        nb = neighbours.get(s, [])
        blob += [struct.pack("<i", len(nb)), np.array(nb, np.int32).tobytes()]
    blob.append(struct.pack("<i", len(qbows)))
    for q, qb in zip(W["queries"], qbows):
        blob += [struct.pack("<i", len(qb[0])), qb[0].tobytes(), qb[1].tobytes(), struct.pack("<i", len(q["connected"])),
                 np.array(q["connected"], np.int32).tobytes()]
    path = str(tmp_path / "kfdb.bin")
    with open(path, "wb") as f:
        f.write(b"".join(blob))
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])["queries"]
    _, want = kc.run_world(W, bows, qbows)
    assert len(got) == len(want) and any(r["loop"] for r in want)
    for g, r, q, qb in zip(got, want, W["queries"], qbows):
        ref_scores = np.array([kc.score(qb, bows[s]) for s in q["connected"]], np.float64)
        assert g["score_bits"] == ref_scores.view(np.uint64).tolist()
        assert g["min_score_bits"] == int(np.array(r["min_score"], np.float32).view(np.uint32))
        assert g["loop"] == r["loop"] and g["reloc"] == r["reloc"]
