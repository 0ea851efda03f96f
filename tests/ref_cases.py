"""Seeded inputs of the pins against the reference's standalone files (tests/golden/ref_pins.npz).  Shared by
tests/test_oracle_ref_cpu.py, which checks the oracle against the stored outputs, and tests/golden/make_golden.py ref, which makes them."""
import zlib

import numpy as np

import oracle_lib

LOGNTS = [5 * (np.log10(512.0) + np.log10(384.0)) / 2 + np.log10(11.0), 5 * (np.log10(1024.0) + np.log10(768.0)) / 2 + np.log10(11.0)]
# nfa() cases that need no series: bit-identical by construction (logNT = LOGNTS[0])
NFA_EXACT = [(0, 0, 0.125), (50, 0, 0.125), (64, 64, 0.0625), (3000, 2900, 0.125), (4000, 5, 0.125)]
# (k, L, ragged, descriptors, levelsup) of the DBoW2 cases; the vocabulary of case i is bow_vocab.make_vocab(k, L, i, ragged, 0.1)
BOW_CASES = [(10, 3, False, 1000, 2), (6, 4, True, 700, 2), (10, 3, False, 0, 4), (3, 5, True, 1500, 4), (10, 2, False, 2000, 1), (4, 3, False, 5, 3)]
# the bow_cases cases whose (word, weight, node) streams tests/golden/bow_edge_pins.npz holds the reference's accumulation of
BOW_EDGE_CASES = ("one_word", "two_words", "straddle", "all_stopped_300")


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
