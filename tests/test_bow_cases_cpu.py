"""The cases of tests/bow_cases.py without a GPU: the oracle of Frame::ComputeBoW (oracle/bow_oracle.cpp) equals the plain-Python
restatement on every case in every field, bit for bit, and every case is what its name says (its own check on the oracle's output)."""
import numpy as np
import pytest

import bow_cases as bc


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_oracle_equals_plain_python_and_case_is_what_it_says(name):
    c = bc.case(name)
    o = bc.oracle(name)
    c.check(o)
    r = bc.py_fields(c.vocab, c.desc, c.levelsup)
    c.check(r)
    for key in bc.FIELDS:
        assert o[key].dtype == r[key].dtype and o[key].shape == r[key].shape, key
        assert o[key].tobytes() == r[key].tobytes(), key


def test_every_case_of_the_list_exists():
    want = [f"n{n}" for n in (1, 2, 255, 256, 257, 511, 512, 513, 4095)] + [
        "n4096_distinct", "one_word", "all_stopped_1", "all_stopped_300", "k1_first", "k1_last", "k255_of_400", "k256_of_400", "k257_of_400",
        "straddle", "two_words", "split_few_words", "split_few_nodes"] + [f"root_{k}_children" for k in (1, 63, 64, 65, 128, 129)] + [
        "chain32_levelsup4", "twins_64_apart_3_67", "twins_64_apart_0_128", "twins_adjacent_lanes", "dist_0", "dist_256", "wide_1000",
        "levelsup_0", "levelsup_L-1", "levelsup_L", "levelsup_L+1", "levelsup_40", "early_leaf_levelsup1", "early_leaf_levelsup2",
        "ids_above_16_bits"]
    assert set(want) <= set(bc.CASE_NAMES)
    v = bc.vocab("count")
    leaf_w = [v[2][i] for i, c in enumerate(v[0]) if not c]
    assert len(leaf_w) == 4096 and 0.03 < sum(1 for w in leaf_w if w == 0) / 4096 < 0.07
    assert bc.vocab("chain32")[4] == 32 and bc.vocab("early_leaf")[4] == 5


def test_one_word_is_the_sequential_sum_and_normalises_to_one():
    """BowVector::addWeight adds the weight once per occurrence: 4096 additions in f64, which is not 4096 * w for the weight the case
    is built on (nor for most weights: a few candidates are scanned here); normalize(L1) then divides the value by itself."""
    c, o = bc.case("one_word"), bc.oracle("one_word")
    w = float(o["weight"][0])
    assert (o["weight"] == w).all() and (o["word"] == o["word"][0]).all()
    v = w
    for _ in range(4095):
        v += w
    assert v != 4096 * w
    per, bow, fv = bc.py_transform(c.vocab, c.desc, c.levelsup)
    assert list(bow.values()) == [v / v] == [1.0] and o["bow_val"].tobytes() == np.array([1.0]).tobytes()
    # the restatement's value before normalize(L1): one word, so norm == the value itself
    raw = {}
    for word, wt, _ in per:
        raw[word] = raw[word] + wt if word in raw else wt
    assert list(raw.values()) == [v]
    p = bc.pool()
    cand = [float(p["weight"][p["members"][x][0]]) for x in p["kept"][:32]]
    differ = [x for x in cand if bc.seq_sum(x, 4096) != 4096 * x]
    assert w in differ and len(differ) >= 8, (len(differ), len(cand))


def test_two_words_tells_sums_from_products():
    """after normalisation one word is 1.0 whatever was added; two words are not: v = w added 2048 times each, and the normalised pair
    differs from the one 2048 * w gives, so a kernel that multiplied would fail the GPU test on this case"""
    o = bc.oracle("two_words")
    wa, wb = (float(o["weight"][o["word"] == i][0]) for i in o["bow_id"])
    sa, sb, pa, pb = bc.seq_sum(wa, 2048), bc.seq_sum(wb, 2048), 2048 * wa, 2048 * wb
    assert o["bow_val"].tolist() == [sa / (sa + sb), sb / (sa + sb)]
    assert o["bow_val"].tolist() != [pa / (pa + pb), pb / (pa + pb)]


@pytest.mark.parametrize("name", ["all_stopped_1", "all_stopped_300"])
def test_all_stopped_frames_are_empty(name):
    o = bc.oracle(name)
    assert len(o["bow_id"]) == 0 and len(o["bow_val"]) == 0 and len(o["fv_node"]) == 0
    assert o["fv_start"].tolist() == [0] and len(o["fv_idx"]) == 0 and not (o["weight"] > 0).any()
    per, bow, fv = bc.py_transform(bc.case(name).vocab, bc.case(name).desc, 2)
    assert bow == {} and fv == {}
