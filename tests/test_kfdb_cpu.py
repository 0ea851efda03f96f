"""CPU checks of the keyframe database: properties of the restatement of DBoW2::L1Scoring::score (tests/kfdb_cases.py), the dense
per-slot formulation the device uses against the inverted-file walk of KeyFrameDatabase, that the seeded cases of the GPU tests are
not vacuous, and the new entry points' behaviour without a GPU."""
import ctypes as C

import numpy as np
import pytest

import kfdb_cases as kc


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


def test_score_of_a_vector_with_itself():
    """score(v, v) is the sequential sum of |v_i|.  With v_i = fl(x_i / N), N the sequential sum of n raw values: N carries a
    relative error of at most (n-1) 2^-53, every quotient 2^-53, every one of the n-1 additions of partial sums below 1 at most
    2^-54; the halving and the two subtractions of equal magnitudes are exact.  |score - 1| <= (1.5 (n-1) + 1) 2^-53, which is
    within 2^-50 for n <= 5: the bound is asserted there, and the derived one on the long BowVectors of the vocabulary."""
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 5):
        for _ in range(50):
            v = kc.hand_bow(np.arange(n) * 7, rng.uniform(0.1, 9.0, n))
            assert abs(kc.score(v, v) - 1.0) <= 2.0 ** -50


def test_score_of_long_vectors_with_themselves(world):
    _, bows, _ = world
    for v in bows.values():
        n = len(v[0])
        assert n > 100 and abs(kc.score(v, v) - 1.0) <= (1.5 * (n - 1) + 1) * 2.0 ** -53


def test_score_of_disjoint_vectors_is_exactly_zero(world):
    _, bows, _ = world
    a = next(iter(bows.values()))
    b = (a[0] + 100000, a[1])
    assert kc.score(a, b) == 0.0 and kc.score(b, a) == 0.0
    assert kc.score(a, kc.hand_bow([])) == 0.0 and kc.score(kc.hand_bow([]), kc.hand_bow([])) == 0.0
    even, odd = kc.hand_bow(np.arange(0, 200, 2), seed=1), kc.hand_bow(np.arange(1, 200, 2), seed=2)   # interleaved, every lower_bound taken
    assert kc.score(even, odd) == 0.0


def test_score_is_symmetric_bit_for_bit():
    """A term |a-b| - a - b is the same in both argument orders whenever a - b is exact: both orders then give -2 min(a, b) without
    a rounding.  That is so for values within a factor of two of each other (Sterbenz) and for values on a common dyadic grid; the
    sums are then the same additions.  Both kinds are asserted.  For arbitrary f64 values the two orders can differ in the last bit
    ((|a-b| - a) - b rounds once, (|a-b| - b) - a twice when a > 2b), so the argument order - query first - belongs to the contract
    (DESIGN.md §3)."""
    rng = np.random.default_rng(4)
    for _ in range(100):
        ids1, ids2 = np.sort(rng.choice(300, 150, replace=False)), np.sort(rng.choice(300, 150, replace=False))
        a, b = (ids1.astype(np.int32), rng.uniform(1.0, 2.0, 150) * 2.0 ** -9), (ids2.astype(np.int32), rng.uniform(1.0, 2.0, 150) * 2.0 ** -9)
        assert kc.score(a, b) == kc.score(b, a) and 0.0 < kc.score(a, b) < 1.0
        g1, g2 = (a[0], rng.integers(1, 1 << 12, 150) / 2.0 ** 20), (b[0], rng.integers(1, 1 << 12, 150) / 2.0 ** 20)
        assert kc.score(g1, g2) == kc.score(g2, g1) and kc.score(g1, g2) > 0.0


def test_score_equals_the_plain_sum_over_common_words(world):
    """the lower_bound jumps skip nothing: the same additions as a walk over the common words in ascending order"""
    _, bows, qbows = world
    for q in qbows[:3]:
        qd = dict(zip(q[0].tolist(), q[1].tolist()))
        for r in bows.values():
            s = 0.0
            for w, wi in zip(r[0].tolist(), r[1].tolist()):
                if w in qd:
                    vi = qd[w]
                    s += abs(vi - wi) - abs(vi) - abs(wi)
            assert kc.score(q, r) == -s / 2.0


def _walk(db, bow, connected_ids=()):
    """the inverted-file walk alone (src/KeyFrameDatabase.cc:86-104): lKFsSharingWords and the word counts it leaves"""
    seen, order, words = set(), [], {}
    for w in bow[0]:
        for k in db.mvInvertedFile.get(int(w), []):
            if id(k) not in seen:
                words[k.slot] = 0
                if k.slot not in connected_ids:
                    seen.add(id(k))
                    order.append(k.slot)
            words[k.slot] += 1
    return order, words


def test_dense_formulation_equals_the_inverted_file_walk():
    """random add / erase / re-add sequences: words, and the list order as ascending (first_word, add sequence)"""
    rng = np.random.default_rng(9)
    for trial in range(20):
        w = kc.RefWorld()
        nslots, U = 12, 40
        for step in range(60):
            s = int(rng.integers(0, nslots))
            if s in w.kf:
                w.erase(s)
            else:
                w.add(s, kc.hand_bow(np.sort(rng.choice(U, int(rng.integers(0, 15)), replace=False)), seed=step))
            if step % 5:
                continue
            q = kc.hand_bow(np.sort(rng.choice(U, int(rng.integers(0, 12)), replace=False)), seed=1000 + step)
            excl = set(int(x) for x in rng.choice(nslots, int(rng.integers(0, 4)), replace=False))
            order, words = _walk(w.db, q, excl)
            dense, maxc = kc.dense_query(w.rows(), q, excl)
            assert kc.dense_sharing(dense, w.seq) == order
            assert all(dense[s][0] == words[s] for s in order)
            assert maxc == max([words[s] for s in order], default=0)
            assert all(d[0] == 0 and d[1] == -1 and d[2] == 0.0 for s, d in dense.items() if s not in order)


def test_seeded_cases_are_not_vacuous(world):
    """what tests/test_kfdb_gpu.py relies on, checked on the restatement alone"""
    W, bows, qbows = world
    stats = {}
    _, res = kc.run_world(W, bows, qbows, stats)
    assert sum(1 for r in res if r["loop"]) * 4 >= 3 * len(res) and sum(1 for r in res if r["reloc"]) * 4 >= 3 * len(res)
    assert stats.get("filtered", 0) >= 1 and stats.get("duplicates", 0) >= 1
    assert any(len(r["reloc"]) > 1 for r in res)


def test_new_entry_points_reject_null_handles():
    import psl_slam_amd as P
    P.build()
    lib = P.lib()
    h, n = C.c_void_p(), C.c_int()
    assert lib.pslfe_kfdb_create(None, 8, 16, C.byref(h)) == -1 and lib.pslfe_kfdb_create(None, 8, 16, None) == -1
    assert lib.pslfe_kfdb_add(None, 0, None, None, 0) == -1
    assert lib.pslfe_kfdb_add_device(None, 0, None, None, None, 1, 16) == -1
    assert lib.pslfe_kfdb_erase(None, 0) == -1 and lib.pslfe_kfdb_clear(None) == -1 and lib.pslfe_kfdb_state(None, None, None) == -1
    assert lib.pslfe_kfdb_query(None, None, None, 0, None, None, None, None, C.byref(n)) == -1
    assert lib.pslfe_kfdb_query_device(None, None, None, None, 1, 16, None, None, None, None, None) == -1
    assert lib.pslfe_kfdb_score(None, None, None, 0, None, 0, None) == -1
    assert b"pslfe_kfdb_score" in lib.pslfe_last_error()
    lib.pslfe_kfdb_destroy(None)
