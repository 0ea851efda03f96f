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
import zlib

import numpy as np
import pytest

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ref_pins.npz")
LOGNTS = [5 * (np.log10(512.0) + np.log10(384.0)) / 2 + np.log10(11.0), 5 * (np.log10(1024.0) + np.log10(768.0)) / 2 + np.log10(11.0)]
# nfa() cases that need no series: bit-identical by construction (logNT = LOGNTS[0])
NFA_EXACT = [(0, 0, 0.125), (50, 0, 0.125), (64, 64, 0.0625), (3000, 2900, 0.125), (4000, 5, 0.125)]
# (k, L, ragged, descriptors, levelsup) of the DBoW2 cases; the vocabulary of case i is bow_vocab.make_vocab(k, L, i, ragged, 0.1)
BOW_CASES = [(10, 3, False, 1000, 2), (6, 4, True, 700, 2), (10, 3, False, 0, 4), (3, 5, True, 1500, 4), (10, 2, False, 2000, 1), (4, 3, False, 5, 3)]


def walk_cases():
    """[n][4] float64 end points (grid units) of the line grid walks."""
    rng = np.random.default_rng(9)
    cases = [(0, 0, 63.9, 47.9), (10.5, 3.2, 10.5, 40.0), (5, 5, 5, 5), (63.2, 1.0, 0.4, 46.5), (-3.5, 10.0, 20.0, -8.0), (2.0, 2.0, 2.9, 2.1),
             (0.0, 47.99, 63.99, 0.0), (30.0, 10.0, 30.0, 10.0)]
    cases += [tuple(rng.uniform(-8, 72, 4) * np.array([1, 0.75, 1, 0.75])) for _ in range(20000)]
    # the grid coordinates Frame.cc feeds it: key-line end points times (64 / width, 48 / height), computed in float
    for _ in range(5000):
        p = rng.uniform(0, 640, 4).astype(np.float32) * np.array([1, 0.75, 1, 0.75], np.float32)
        inv = np.array([np.float32(64) / np.float32(640), np.float32(48) / np.float32(480)] * 2, np.float32)
        cases.append(tuple(float(v) for v in p * inv))
    return np.array(cases, np.float64)


def log_gamma_args():
    """log_gamma: both branches (Lanczos x <= 15, Windschitl above), every integer argument nfa() can pass for a 640x480 ... 1280x960 image."""
    return np.array(list(range(1, 3000)) + list(range(3000, 400000, 37)) + [15.0, 15.5, 16.0, 0.5, 2.25, 1e6 + 1], np.float64)


def nfa_cases():
    """[n][2] int32 (n, k) of nfa(n, k, p, logNT): the ranges rect_improve produces - rectangle pixel counts up to a few thousand, aligned
    counts 0..n.  Case i takes p = 1/8 halved (i % 6) times (LSD_REFINE_ADV) and LOGNTS[i & 1], the scaled 512x384 and 1024x768 images."""
    rng = np.random.default_rng(3)
    cases = [(0, 0), (1, 0), (1, 1), (7, 7), (10, 3), (100, 100), (100, 0), (5000, 1), (5000, 4999)]
    for _ in range(60000):
        n = int(rng.integers(1, 9000)) if rng.random() < 0.7 else int(rng.integers(1, 200))
        u = rng.random()
        k = int(rng.integers(0, n + 1)) if u < 0.4 else int(min(n, max(0, round(n * rng.uniform(0.0, 0.45)))))
        cases.append((n, k))
    return np.array(cases, np.int32)


def nfa_args(i, n, k):
    return int(n), int(k), 0.125 / (1 << (i % 6)), LOGNTS[i & 1]


def bow_inputs():
    """Per DBoW2 case: the oracle's (word, weight, node) stream of the tree descent (oracle_lib.compute_bow) and n."""
    import bow_vocab
    rng = np.random.default_rng(12)
    for case, (k, L, ragged, n, levelsup) in enumerate(BOW_CASES):
        vocab = bow_vocab.make_vocab(k, L, case, ragged, stopped=0.1)
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        if n > 10:
            desc[n // 2:] = desc[: n - n // 2]   # repeated words: addWeight's accumulate branch
        yield oracle_lib.compute_bow(*vocab[:4], vocab[4], desc, levelsup), n


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.uint32(c)


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
