"""Non-GPU checks of what tests/test_debug_math_gpu.py and tests/test_nfa_direct_gpu.py rest on: the host twins of pslfe_debug_math
(oracle/math_oracle.cpp: the host compile of the product's math headers), the argument grids (tests/math_grids.py) and the list of NFA
trials (tests/nfa_cases.py) - which must reach every branch of k_lsd_nfa_setup / k_lsd_nfa_series it was built for."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import math_grids
import nfa_cases
import oracle_lib

MIN_TAKEN = 20


@pytest.fixture(scope="module")
def replayed():
    tot, contradictions, by_p = Counter(), [], Counter()
    for tag, n, k, p in nfa_cases.cases():
        r = nfa_cases.replay(n, k, p)
        for key, v in r.items():
            if isinstance(key, tuple):
                contradictions.append(key[1:])
            else:
                tot[key] += v
        if tag == "random" and r["series ends by the truncation test"]:
            by_p[p] += 1
    return tot, contradictions, by_p


def test_nfa_cases_reach_every_branch(replayed):
    tot, contradictions, by_p = replayed
    assert 3000 <= len(nfa_cases.cases()) <= 8000
    want = ["n == 0", "k == 0", "n == k, p from the table", "n == k, p off the table", "k == n - 1", "k == 1", "p off the table",
            "first term underflows, k > n p", "first term underflows, k <= n p", "first term subnormal",
            "truncation test on a subnormal tail: exact path", "truncation test of the last term (q == 1): exact path",
            "series starts within 2 of the end of the unrolled path", "series with n - k < 8", "series with n at 65535 .. 65537",
            "series starts within 2 of the end of the reciprocal table, unrolled", "unrolled path walks across the end of the reciprocal table",
            "unrolled block, quotients from the reciprocal table", "unrolled block, quotients divided",
            "stage 1: stop", "stage 1: go on", "stage 1: undecided", "series ends by the truncation test"]
    want += ["p row %d" % j for j in range(11)]
    for a in ("n + 1", "k + 1", "n - k + 1"):
        want += ["log_gamma(%s) from the table" % a, "log_gamma(%s) evaluated" % a, "log_gamma(%s) at 65535 .. 65537" % a]
    print({k: tot[k] for k in want})
    short = {k: tot[k] for k in want if tot[k] < MIN_TAKEN}
    assert not short, f"branches taken fewer than {MIN_TAKEN} times: {short}"
    # every probability: at least 200 random trials whose series ends by the truncation test
    assert all(by_p[p] >= 200 for p in nfa_cases.P_ALL), by_p
    # stage 1 of lsdn_tail_test_fast replayed in exact arithmetic never decides against the reference's own test
    assert not contradictions, contradictions[:5]


def test_oracle_evaluates_every_nfa_case():
    """the reference values of test_nfa_direct_gpu.py exist: no NaN, a tail where the replay sees a series, and enough trials
    that win against a threshold just below their value (the near-threshold test needs at least 500)"""
    cs = nfa_cases.cases()
    n, k, p = (np.array([c[i] for c in cs]) for i in (1, 2, 3))
    old = oracle_lib.set_nfa_math(1)
    try:
        v, tail = oracle_lib.lsd_nfa_lognt_tail(n, k, p, nfa_cases.LOG_NT)
        v1, tail1 = oracle_lib.lsd_nfa_lognt_tail(n, k, p / 2, nfa_cases.LOG_NT)
        one = oracle_lib.load()
        one.pso_lsd_nfa_lognt.restype = C.c_double
        one.pso_lsd_nfa_lognt.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
        for i in range(0, len(cs), 97):   # the sibling returns the value of the function it was added beside
            assert one.pso_lsd_nfa_lognt(int(n[i]), int(k[i]), float(p[i]), nfa_cases.LOG_NT) == v[i]
    finally:
        oracle_lib.set_nfa_math(old)
    assert np.isfinite(v).all() and np.isfinite(tail).all() and np.isfinite(v1).all() and np.isfinite(tail1).all()
    series = np.array([nfa_cases.replay(*c[1:])["series"] > 0 for c in cs])
    assert ((tail > 0) == series).all(), "the oracle sums a series exactly where the replay of the kernels' branches does"
    assert (tail[series] < 2.2250738585072014e-308).sum() >= MIN_TAKEN, "subnormal tails"
    nneg = 8   # thresholds below the value in the near-threshold test: -1e-3, -1e-5, -1e-6, -4e-7, -1e-7, -1e-9, -1 ulp (and three phases)
    assert series.sum() * nneg >= 500
    # v = -log10(tail) - logNT wherever there was a series
    assert np.allclose(v[series & (tail > 1e-300)], -np.log10(tail[series & (tail > 1e-300)]) - nfa_cases.LOG_NT, rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", sorted(math_grids.GRIDS))
def test_grid_is_usable(name):
    """the twin evaluates the whole grid: no NaN comes out (none goes in), and the outputs are not degenerate"""
    fn = math_grids.GRIDS[name]
    a, b, distinct = math_grids.grid(name)
    assert len(a) <= (1 << 22) + (1 << 21) and not np.isnan(a).any() and (b is None or not np.isnan(b).any())
    out = oracle_lib.math_eval(fn, a, b)
    for o in (out if isinstance(out, tuple) else (out,)):
        assert len(o) == len(a)
        if o.dtype.kind == "f" and fn not in ("fdiv", "ddiv"):
            assert not np.isnan(o).any(), f"{fn}: NaN for {a[np.isnan(o)][:4]}"
        got = len(np.unique(o.view(np.uint32 if o.itemsize == 4 else np.uint64)))
        print(name, len(a), "arguments,", got, "distinct outputs")
        assert got >= distinct, f"{name}: only {got} distinct outputs"


def test_twins_agree_with_numpy_where_ieee_fixes_the_result():
    a, b, _ = math_grids.grid("ddiv")
    with np.errstate(all="ignore"):
        assert oracle_lib.math_eval("ddiv", a, b).tobytes() == (a / b).tobytes()
        a, b, _ = math_grids.grid("fdiv")
        q = oracle_lib.math_eval("fdiv", a, b)
        ok = ~np.isnan(q)
        assert q[ok].tobytes() == (a / b)[ok].tobytes()
        a, _, _ = math_grids.grid("dsqrt")
        assert oracle_lib.math_eval("dsqrt", a).tobytes() == np.sqrt(a).tobytes()
        a, _, _ = math_grids.grid("sqrtf")
        assert oracle_lib.math_eval("sqrtf", a).tobytes() == np.sqrt(a).tobytes()
    a, _, _ = math_grids.grid("cvround_d")
    assert (oracle_lib.math_eval("cvround_d", a) == np.rint(a).astype(np.int64)).all()
    a, b, _ = math_grids.grid("ratio_inv")
    inside = (a < 65536) & (b < 16384)
    assert oracle_lib.math_eval("ratio_inv", a, b)[inside].tobytes() == (a / b)[inside].tobytes()   # psl_f64math.h: equal to the division there


def test_log_gamma_twin_is_the_oracles_log_gamma():
    """lsdn_log_gamma (the product's text, compiled for the host) against the oracle's restatement of the reference's log_gamma over
    the same restated log / sinh: the same bytes for every integer argument 1 .. 70000"""
    x = np.arange(1, 70001, dtype=np.float64)
    old = oracle_lib.set_nfa_math(1)
    try:
        ref = oracle_lib.lsd_log_gamma(x)
    finally:
        oracle_lib.set_nfa_math(old)
    assert oracle_lib.math_eval("log_gamma", x).tobytes() == ref.tobytes()
