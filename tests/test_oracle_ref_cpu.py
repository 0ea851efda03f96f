"""The oracle's restatements pinned against the reference's own code: the files of the reference tree that compile standalone
(no OpenCV / Eigen), built by `make -C oracle _ref` into oracle/_ref/, and their outputs on the inputs below, stored in
tests/golden/ref_pins.npz (tests/golden/make_golden.py ref; outputs only, no reference source):
  * add_src/lineIterator.cpp - the Bresenham walk behind Frame::AssignFeaturesToGridForLine (src/Frame.cc:286-309, row a22);
  * Thirdparty/line_descriptor/src/ED_Lib/NFA.cpp:106-240 - nfa() / log_gamma(), the in-tree TWIN of the arithmetic inside the
    LSD the reference links (OpenCV's lsd.cpp, not in the tree; row a10).  The twin multiplies by a tabulated 1/i where lsd.cpp
    divides by i: log_gamma and every value that needs no series are compared bit for bit; of the summed tails 98.7 % are
    bit-identical too, the rest differ in the last bits, and a handful stop the series one term apart (the truncation test sits on
    that last bit): then the values differ by up to ~4e-5 relative, far inside the series' own 10 % error budget; no accept / reject
    decision (value > 0) differs;
  * Thirdparty/DBoW2/DBoW2/BowVector.cpp:34-84 + FeatureVector.cpp:31-45 - the accumulation Frame::ComputeBoW links (row f2).
The inputs come from seeded generators; the stored CRC of each input set proves they are the ones the stored outputs were made from."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib
from ref_cases import BOW_EDGE_CASES, LOGNTS, NFA_EXACT, bow_inputs, crc, log_gamma_args, nfa_args, nfa_cases, walk_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ref_pins.npz")
def golden():
    return np.load(GOLD)


def test_oracle_grid_walk_equals_the_reference_line_iterator():
    g = golden()
    orc = oracle_lib.load()
    orc.pso_line_iterator_walk.argtypes = [C.c_double] * 4 + [C.c_void_p, C.c_int]
    cases = walk_cases()
    assert crc(cases) == g["walk_cases_crc"], "the walk inputs are not the ones ref_pins.npz was made from"
    b = np.zeros((4096, 2), np.int32)
    for c, na, ca in zip(cases, g["walk_counts"], g["walk_crc"]):
        nb = orc.pso_line_iterator_walk(*[float(v) for v in c], b.ctypes.data, 4096)
        assert na == nb and ca == crc(b[:nb]), c
    assert int(g["walk_counts"].sum()) > 100000


def test_oracle_log_gamma_and_nfa_equal_the_reference_twin():
    g = golden()
    orc = oracle_lib.load()
    orc.pso_lsd_log_gamma.argtypes, orc.pso_lsd_log_gamma.restype = [C.c_double], C.c_double
    orc.pso_lsd_nfa_lognt.argtypes, orc.pso_lsd_nfa_lognt.restype = [C.c_int, C.c_int, C.c_double, C.c_double], C.c_double
    xs, cases = log_gamma_args(), nfa_cases()
    assert crc(xs, cases) == g["nfa_inputs_crc"], "the log_gamma / nfa inputs are not the ones ref_pins.npz was made from"
    old = orc.pso_set_nfa_math(0)   # the host's libm: what the reference calls
    try:
        for x, a in zip(xs, g["lgamma_ref"]):
            b = orc.pso_lsd_log_gamma(float(x))
            assert a == b, (x, a, b)
        exact = series = flips = far = 0
        worst = 0.0
        for i, ((n, k), a) in enumerate(zip(cases, g["nfa_ref"])):
            b = orc.pso_lsd_nfa_lognt(*nfa_args(i, n, k))
            if a == b:
                exact += 1
            else:   # only the summed tail may differ: (n-i+1) * (1/i) in the twin, (n-i+1) / i in lsd.cpp
                series += 1
                err = abs(a - b) / max(abs(a), abs(b), 1e-300)
                worst = max(worst, err)
                far += int(err > 1e-11)   # the series stopped one term apart
                assert err < 1e-3, (n, k, a, b)
            flips += int((a > 0) != (b > 0))
        assert flips == 0 and exact > 0.98 * len(cases) and far < 1e-3 * len(cases), (flips, exact, series, far, worst)
        # the cases that need no series are bit-identical by construction; check that family explicitly
        for (n, k, p), a in zip(NFA_EXACT, g["nfa_exact_ref"]):
            assert a == orc.pso_lsd_nfa_lognt(n, k, p, LOGNTS[0]), (n, k, p)
    finally:
        orc.pso_set_nfa_math(old)


def test_oracle_bow_accumulation_equals_the_reference_dbow2():
    """The (word, weight, node) stream the oracle's tree descent produces, accumulated by the reference's own BowVector::addWeight /
    normalize(L1) / FeatureVector::addFeature, gives the oracle's BowVector (f64 values bit for bit) and FeatureVector."""
    g = golden()
    checked = 0
    for case, (o, n) in enumerate(bow_inputs()):
        assert crc(*(o[key] for key in ("word", "weight", "nid"))) == g[f"bow{case}_in_crc"], f"case {case}: the oracle's descent changed"
        assert np.array_equal(g[f"bow{case}_id"], o["bow_id"]) and g[f"bow{case}_val"].tobytes() == o["bow_val"].tobytes()
        assert np.array_equal(g[f"bow{case}_fv_node"], o["fv_node"]) and np.array_equal(g[f"bow{case}_fv_start"], o["fv_start"])
        assert np.array_equal(g[f"bow{case}_fv_idx"], o["fv_idx"])
        checked += len(o["bow_id"])
    assert checked > 400


def test_oracle_bow_edge_cases_equal_the_reference_dbow2():
    """The same on the streams of four cases of tests/bow_cases.py (tests/golden/bow_edge_pins.npz, make_golden.py bow_edge_pins): one
    word added 4096 times - the reference's value before normalisation is the sequential sum, after it 1.0 -, two words 2048 times
    each, segments that straddle ranks 255 | 256 and 511 | 512, and a frame of stopped words only (empty vectors, norm 0)."""
    import bow_cases as bc
    g = np.load(os.path.join(ROOT, "tests", "golden", "bow_edge_pins.npz"))
    for name in BOW_EDGE_CASES:
        o = bc.oracle(name)
        assert crc(*(o[key] for key in ("word", "weight", "nid"))) == g[f"{name}_in_crc"], f"{name}: the case or the oracle's descent changed"
        assert np.array_equal(g[f"{name}_id"], o["bow_id"]) and g[f"{name}_val"].tobytes() == o["bow_val"].tobytes(), name
        assert np.array_equal(g[f"{name}_fv_node"], o["fv_node"]) and np.array_equal(g[f"{name}_fv_start"], o["fv_start"]), name
        assert np.array_equal(g[f"{name}_fv_idx"], o["fv_idx"]), name
    assert g["one_word_val"].tolist() == [1.0] and len(g["two_words_id"]) == 2 and len(g["straddle_id"]) == 592
    assert len(g["all_stopped_300_id"]) == 0 and g["all_stopped_300_fv_start"].tolist() == [0]
