"""The trials (n, k, p) on which tests/test_nfa_direct_gpu.py drives k_lsd_nfa_setup / k_lsd_nfa_series directly, and a replay of the
branch conditions of those kernels (line_kernels3.h) in plain Python, with which tests/test_debug_math_cpu.py checks that the list
reaches every branch it was built for.  No GPU, no oracle: the replay uses Python's libm, which is enough to tell which branch a
trial takes (the cases keep clear of the few places where a last-ulp difference could change that).

nfa(n, k, p) = -log10(P[B(n, p) >= k]) - logNT: the first term of the binomial tail from log_gamma, then the tail summed term by term
until the reference's truncation test (evaluated only while (n - i + 1) / i < 1, i.e. beyond i = (n + 1) / 2) says stop.
"""
import math
from collections import Counter

import numpy as np

P0 = 22.5 / 180                                   # LineParams.p: the tolerance of the first test
P_ROWS = [P0 / 2 ** j for j in range(11)]         # the rows of the kernels' log(p) table (PSL_NFA_NP = 11)
P_OFF = [P0 / 2 ** 11, 0.1, 0.3, 0.25]            # not in the table: evaluated directly on the device
P_ALL = P_ROWS + P_OFF
W, H = 640, 480
LOG_NT = 5 * (math.log10(round(W * 0.8)) + math.log10(round(H * 0.8))) / 2 + math.log10(11.0)   # as prepare() computes it (to an ulp)
RATIO_AMAX, RATIO_BMAX, LG_N = 65536, 16384, 65536
DBL_MIN = 2.2250738585072014e-308


def log10_first_term(n, k, p):
    return (math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1) + k * math.log(p) + (n - k) * math.log1p(-p)) / math.log(10)


def _build():
    rng = np.random.default_rng(20260)
    out = []

    def add(tag, n, k, p):
        n, k = int(n), int(k)
        assert 0 <= k <= n and 0 < p < 1, (tag, n, k, p)
        out.append((tag, n, k, float(p)))

    for p in P_ALL:
        # trivial cases
        for _ in range(2):
            add("n==0", 0, 0, p)
        for n in (1, 50):
            add("k==0", n, 0, p)
        for n in (1, 7, 16, 300, 2000):
            add("n==k", n, n, p)
        for n in (2, 40, 500):
            add("k==n-1", n, n - 1, p)
        for n in (2, 10, 300, 5000):
            add("k==1", n, 1, p)
        # k against the mode n p
        for n in (16, 100, 1000, 4000, 20000, 70000):
            m = int(n * p)
            for k in sorted({min(max(1, v), n - 1) for v in (m // 2, m - 1, m, m + 1, m + 2, 2 * m + 3, 4 * m + 8)}):
                add("mode", n, k, p)
        # the first term underflows to 0 (or to less than 100 ulps of the smallest subnormal): far above the mode, and - for the
        # larger p only - far below it
        for n, k in ((1000, 500), (2000, 1500), (20000, 12000), (70000, 40000), (70000, 69000)):
            if log10_first_term(n, k, p) < -330:
                add("underflow above", n, k, p)
        for n, k in ((70000, 3), (70000, 10), (70000, 40), (60000, 5)):
            if k <= n * p and log10_first_term(n, k, p) < -330:
                add("underflow below", n, k, p)
        # a subnormal first term (4.9e-322 .. 2.2e-308) close to n: the whole tail stays subnormal, so the truncation test meets a
        # subnormal sum
        for d in (1, 3, 6, 12):
            got = 0
            for k in range(d + 1, 4000):
                if -320.5 < log10_first_term(k + d, k, p) < -308.6:
                    add("subnormal tail", k + d, k, p)
                    got += 1
                    if got == 2:
                        break
        # ... and far below the mode: the series climbs out of the subnormal range
        if (70000 * math.log1p(-p)) / math.log(10) < -340:
            for k in range(1, 3000):
                if -320.5 < log10_first_term(70000, k, p) < -308.6:
                    add("subnormal first term", 70000, k, p)
        # the unrolled path ends where 2 (i + 7) > n + 1: k + 1 around (n + 1) / 2 - 7; and n - k < 8 never enters it
        for n in (30, 31, 100, 101, 400, 401, 1000, 1001):
            for dlt in range(-2, 3):
                k = (n + 1) // 2 - 7 + dlt - 1
                if k >= 1 and log10_first_term(n, k, p) > -300:
                    add("unroll boundary", n, k, p)
        for n in (20, 64, 200):
            for d in range(1, 8):
                add("n-k<8", n, n - d, p)
        # the series of n >= 65536 divide; the log_gamma table ends at 65535
        for n in (65534, 65535, 65536, 65537):
            m = int(n * p)
            for k in (max(1, m - 50), max(1, m), m + 200):
                add("n around 65536", n, k, p)
        for k in (65534, 65535, 65536):
            add("k+1 around 65536", 70000, k, p)          # (the first term underflows: the value comes from log1term)
        for d in (65534, 65535, 65536):
            add("n-k+1 around 65536", d + max(2, int(70000 * p)), max(2, int(70000 * p)), p)
        # k beyond n / 2 with a value near 0 (a tail near 10^-logNT): the truncation test is met by terms that still matter and
        # |-log10(tail) - logNT| is small, the only place where it does not stop at once (err ~ term * m against 0.1 |v| tail)
        near = [(n, k) for n in range(2, 121) for k in range((n + 1) // 2, n) if -LOG_NT - 4 < log10_first_term(n, k, p) < -LOG_NT + 3]
        for n, k in near[::max(1, len(near) // 60)]:
            add("value near 0", n, k, p)
        for n, k in near:   # the closest ones, where the test goes on for a term or two, all of them
            if -LOG_NT - 1.2 < log10_first_term(n, k, p) < -LOG_NT + 0.6:
                add("value next to 0", n, k, p)
        # random trials that run into the truncation test
        cnt = 0
        while cnt < 210:
            n = int(round(math.exp(rng.uniform(math.log(8), math.log(3000)))))
            m, sd = n * p, math.sqrt(n * p * (1 - p))
            k = int(rng.integers(1, max(2, min(n - 8, int(m + 14 * sd + 12)) + 1)))
            if k < 1 or k > n - 2 or log10_first_term(n, k, p) < -290:
                continue
            add("random", n, k, p)
            cnt += 1
    # the reciprocal table ends at i + 7 == 16384: a series that walks across i = 16376 in the unrolled path needs 2 (i + 7) <= n + 1
    # and n < 65536, i.e. a mode n p near 16376 with p >= 1/4 - probabilities outside the table
    for n, p in ((54587, 0.3), (56000, 0.3), (60000, 0.3), (65500, 0.25), (65535, 0.25)):
        for k1 in list(range(16374, 16379)) + list(range(16301, 16309)):
            add("ratio table end", n, k1 - 1, p)
    return out


_CASES = None


def cases():
    """[(tag, n, k, p)] in a fixed order"""
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def table_row(p):
    """The row of the log(p) table the kernels use for p (jp), or -1"""
    for j, q in enumerate(P_ROWS):
        if p == q:
            return j
    return -1


def replay(n, k, p, log_nt=LOG_NT):
    """Counter of the branches k_lsd_nfa_setup / k_lsd_nfa_series take for nfa(n, k, p) with stop = +inf"""
    r = Counter()
    jp = table_row(p)
    r["p row %d" % jp if jp >= 0 else "p off the table"] += 1
    if n == 0:
        r["n == 0"] += 1
        return r
    if k == 0:
        r["k == 0"] += 1
        return r
    if n == k:
        r["n == k, p from the table" if jp >= 0 else "n == k, p off the table"] += 1
        return r
    if k == n - 1:
        r["k == n - 1"] += 1
    if k == 1:
        r["k == 1"] += 1
    for name, a in (("n + 1", n + 1), ("k + 1", k + 1), ("n - k + 1", n - k + 1)):
        r["log_gamma(%s) from the table" % name if a < LG_N else "log_gamma(%s) evaluated" % name] += 1
        if LG_N - 1 <= a <= LG_N + 1:
            r["log_gamma(%s) at 65535 .. 65537" % name] += 1
    p_term = p / (1.0 - p)
    l10 = log10_first_term(n, k, p)
    term = math.exp(l10 * math.log(10)) if l10 > -400 else 0.0
    if term == 0.0 or term / max(term, DBL_MIN) <= 100.0 * 2.2204460492503131e-16:
        r["first term underflows, k > n p" if k > n * p else "first term underflows, k <= n p"] += 1
        return r
    if term < DBL_MIN:
        r["first term subnormal"] += 1
    r["series"] += 1
    if n in (65535, 65536, 65537):
        r["series with n at 65535 .. 65537"] += 1
    i = k + 1
    if abs(i - ((n + 1) // 2 - 7)) <= 2:
        r["series starts within 2 of the end of the unrolled path"] += 1
    if n - k < 8:
        r["series with n - k < 8"] += 1
    # which quotient form the unrolled path uses, block by block (the blocks only cover i <= (n + 1) / 2 - 7)
    ii, crossed = i, False
    while ii + 7 <= n and 2 * (ii + 7) <= n + 1:
        table = ii + 7 < RATIO_BMAX and n < RATIO_AMAX
        r["unrolled block, quotients from the reciprocal table" if table else "unrolled block, quotients divided"] += 1
        if n < RATIO_AMAX and abs(ii - (RATIO_BMAX - 8)) <= 8:
            crossed = True
        ii += 8
    if crossed:
        r["unrolled path walks across the end of the reciprocal table"] += 1
    if abs(i - (RATIO_BMAX - 8)) <= 2 and 2 * (i + 7) <= n + 1:
        r["series starts within 2 of the end of the reciprocal table, unrolled"] += 1
    # the terms up to i = (n + 1) / 2 are added without a test
    i0 = (n + 1) // 2
    bt = term
    if i <= i0:
        idx = np.arange(i, i0 + 1, dtype=np.float64)
        terms = np.cumprod(np.concatenate(([term], (n - idx + 1) / idx * p_term)))
        bt = float(np.cumsum(terms)[-1])
        term = float(terms[-1])
        i = i0 + 1
    while i <= n:
        m = (n - i + 1) / i * p_term
        term *= m
        bt += term
        q = n - i + 1
        r["truncation test"] += 1
        pw = m if q == 1 else m ** q
        err = term * ((1.0 - pw) / (1.0 - m) - 1.0)
        exact = err < 0.1 * abs(-math.log10(bt) - log_nt) * bt if bt > 0 else True
        e = math.frexp(bt)[1] - 1
        if bt < DBL_MIN:
            r["truncation test on a subnormal tail: exact path"] += 1
        elif q < 2:
            r["truncation test of the last term (q == 1): exact path"] += 1
        else:   # stage 1 of lsdn_tail_test_fast
            tb = 0.1 * bt
            a0, a1 = -e * 0.30102999566398120 - log_nt, -(e + 1) * 0.30102999566398120 - log_nt
            f0, f1 = abs(a0), abs(a1)
            lhi = max(f0, f1) + 1e-9
            llo = min(f0, f1) - 1e-9 if (a0 > 0) == (a1 > 0) else 0.0
            err_l, err_u = term * (m - 5e-16), term * (m * (1.0 + 1.2 * m) + 5e-16)
            if err_u * 1.000001 < tb * max(llo, 0.0):
                r["stage 1: stop"] += 1
                if not exact:
                    r["stage 1 stops where the reference goes on"] += 1
                    r[("contradiction", n, k, p, i)] += 1
            elif err_l * 0.999999 >= tb * lhi:
                r["stage 1: go on"] += 1
                if exact:
                    r["stage 1 goes on where the reference stops"] += 1
                    r[("contradiction", n, k, p, i)] += 1
            else:
                r["stage 1: undecided"] += 1
        if exact:
            r["series ends by the truncation test"] += 1
            return r
        i += 1
    r["series ends with i > n"] += 1
    return r
