"""Argument grids for pslfe_debug_math (tests/test_debug_math_gpu.py; checked without a GPU against the host twin in
tests/test_debug_math_cpu.py).  Per function: every representable value within 2048 ulps of every branch threshold in the function's
text, a sweep with an odd stride (coprime to every power of two) through the range the kernels use, and the special pairs of the
two-argument functions.  About 2^22 arguments per function at the most.  No NaN arguments: the headers exclude them, and a NaN's
payload is not part of any contract.

grid(name) -> (a, b or None, the least number of distinct values that each output of a healthy grid takes)
"""
import numpy as np

ULPS = 2048
DISTINCT = 1 << 16   # a grid of millions of arguments whose outputs take fewer distinct values than this feeds a constant branch
PI = np.pi


def f32_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def f64_bits(b):
    return np.asarray(b, np.uint64).view(np.float64)


def bits32(x):
    return int(np.float32(x).view(np.uint32))


def bits64(x):
    return int(np.float64(x).view(np.uint64))


def around32(bit_patterns, signs=(0, 1), top=0x7f800000):
    """the floats within ULPS of each (positive) bit pattern, with each sign; nothing beyond `top` (infinity)"""
    out = []
    for b in bit_patterns:
        r = np.arange(max(0, b - ULPS), min(top, b + ULPS) + 1, dtype=np.uint32)
        for s in signs:
            out.append(f32_bits(r | np.uint32(s << 31)))
    return np.concatenate(out)


def around64(bit_patterns, signs=(0, 1)):
    out = []
    for b in bit_patterns:
        r = np.arange(max(0, b - ULPS), b + ULPS + 1, dtype=np.uint64)
        for s in signs:
            out.append(f64_bits(r | np.uint64(s << 63)))
    return np.concatenate(out)


def sweep32(lo, hi, count, sign=0):
    """about `count` floats of [lo, hi] (0 <= lo < hi), an odd stride apart in their bit patterns"""
    a, b = bits32(lo), bits32(hi)
    stride = max(1, (b - a) // count) | 1
    return f32_bits(np.arange(a, b + 1, stride, dtype=np.uint32) | np.uint32(sign << 31))


def sweep64(lo, hi, count, sign=0):
    a, b = bits64(lo), bits64(hi)
    stride = max(1, (b - a) // count) | 1
    return f64_bits(np.arange(a, b + 1, stride, dtype=np.uint64) | np.uint64(sign << 63))


def linear64(lo, hi, count):
    """`count` doubles of [lo, hi], equally spaced in value (count odd: coprime to the binary grid)"""
    return lo + (hi - lo) * (np.arange(count | 1, dtype=np.float64) / float(count | 1))


def hi_word(h):
    """the two 64-bit patterns at which a comparison of the high word against h changes"""
    return [h << 32, (h + 1) << 32]


def _finite32(rng, n):
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    x = f32_bits(b).copy()
    x[~np.isfinite(x)] = np.float32(1.5)
    return x


def _finite64(rng, n):
    x = f64_bits(rng.integers(0, 1 << 63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))).copy()
    x[~np.isfinite(x)] = 1.5
    return x


def grid(name):
    rng = np.random.default_rng(sum(map(ord, name)))   # a fixed seed per function
    cat = np.concatenate
    if name == "atanf":   # |x| limits 2^-29, 0.4375, 0.6875, 1.1875, 2.4375, 2^25; every finite float range
        a = cat([around32([0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000, 0x7f800000, 0x00800000, 0]),
                 sweep32(0.0, np.inf, 1 << 21), sweep32(0.0, np.inf, 1 << 21, 1)])
        return a, None, DISTINCT
    if name == "tanf":    # |x| < 120; limits 2^-13, 0.6744, pi/4, and the reduced argument next to the multiples of pi/2
        near = [bits32(np.float32(k * PI / 2)) for k in range(1, 77)] + [bits32(np.float32(k * PI / 4)) for k in (1, 3, 5, 7, 9)]
        a = cat([around32([0x39000000, 0x3f2ca140, 0x3f490fda, 0x00800000, 0] + near), sweep32(0.0, 8.0, 1 << 21), sweep32(0.0, 8.0, 1 << 19, 1),
                 sweep32(8.0, 119.99, 1 << 19), sweep32(8.0, 119.99, 1 << 19, 1)])
        return a, None, DISTINCT
    if name == "sincosf":  # abstop12 limits: 2^-12 and abstop12(pi/4) (0.75 as a float comparison); [0, 2 pi]; |x| < 120
        near = [bits32(np.float32(k * PI / 4)) for k in range(1, 153, 3)]
        a = cat([around32([0x39800000, 0x3f400000, 0x3f490fdb, 0x00800000, 0] + near), sweep32(0.0, 2 * PI, 1 << 21), sweep32(0.0, 119.99, 1 << 20),
                 sweep32(0.0, 119.99, 1 << 20, 1)])
        return a, None, DISTINCT
    if name == "fast_atan2":
        m = np.arange(-512, 513, dtype=np.float32)
        yy, xx = np.meshgrid(m, m, indexing="ij")          # IC_Angle's moments and k_lsd_grad's differences are integers
        ry, rx = _finite32(rng, 1 << 20), _finite32(rng, 1 << 20)
        big = cat([sweep32(1e-30, 1e30, 2000), sweep32(1e-30, 1e30, 2000, 1)])
        small = np.array([0.0, -0.0, 2.2204460492503131e-16, -2.2204460492503131e-16, 1.1e-16, 4.4e-16], np.float32)
        sy, sx = np.meshgrid(small, big, indexing="ij")
        eq = cat([sweep32(1e-38, 3e38, 20000), sweep32(1e-38, 3e38, 20000, 1)])
        a = cat([yy.ravel(), ry, sy.ravel(), sx.ravel(), eq, eq, small.repeat(len(small))])
        b = cat([xx.ravel(), rx, sx.ravel(), sy.ravel(), eq, -eq, np.tile(small, len(small))])
        return a, b, DISTINCT
    if name == "atan2f":
        sp = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1e-45, -1e-45, 3.4e38, -3.4e38, 1.17549435e-38, 2.5, -2.5], np.float32)
        v = cat([sp, sweep32(1e-44, 3e38, 1000), sweep32(1e-44, 3e38, 1000, 1)])
        sy, sx = np.meshgrid(sp, v, indexing="ij")
        ry, rx = _finite32(rng, 1 << 21), _finite32(rng, 1 << 21)
        # exponent gaps: |y / x| around 2^26, 2^60 and their reciprocals (the k > 60 / k < -60 branches) and x == 1
        y0 = sweep32(1e-10, 1e10, 1 << 14)
        gaps = []
        for e in (-62, -61, -60, -59, -27, -26, -25, 25, 26, 27, 59, 60, 61, 62):
            for sgn in (1.0, -1.0):
                with np.errstate(over="ignore", under="ignore"):
                    x = (y0.astype(np.float64) * 2.0 ** e).astype(np.float32) * np.float32(sgn)
                ok = np.isfinite(x)
                gaps.append((y0[ok], x[ok]))
                gaps.append((-y0[ok], x[ok]))
        one = cat([sweep32(0.0, 3e38, 1 << 16), sweep32(0.0, 3e38, 1 << 16, 1)])
        a = cat([sy.ravel(), sx.ravel(), ry, one] + [g[0] for g in gaps])
        b = cat([sx.ravel(), sy.ravel(), rx, np.ones_like(one)] + [g[1] for g in gaps])
        return a, b, DISTINCT
    if name == "fdiv":    # random bit patterns (quotients over- and underflow), subnormal operands, subnormal quotients
        a, b = _finite32(rng, 1 << 21), _finite32(rng, 1 << 21)
        sub = f32_bits(rng.integers(1, 1 << 23, 1 << 19, dtype=np.uint64).astype(np.uint32))
        nrm = _finite32(rng, 1 << 19)
        lo = f32_bits(rng.integers(0x00800000, 0x20000000, 1 << 20, dtype=np.uint64).astype(np.uint32))      # 1e-38 .. 1e-19
        hi = f32_bits(rng.integers(0x3f800000, 0x5f800000, 1 << 20, dtype=np.uint64).astype(np.uint32))      # 1 .. 1.8e19
        a, b = cat([a, sub, nrm, sub, lo]), cat([b, nrm, sub, sub[::-1], hi])
        a = a.copy()
        a[(a == 0) & (b == 0)] = np.float32(1.0)    # 0 / 0 is a NaN
        return a, b, DISTINCT
    if name == "sqrtf":
        b = rng.integers(0, 0x7f800000, 1 << 22, dtype=np.uint64).astype(np.uint32)
        return cat([f32_bits(b), f32_bits(np.arange(0, 1 << 16, dtype=np.uint32)), around32([0x00800000, 0x3f800000, 0x7f7fffff], signs=(0,), top=0x7f7fffff)]), None, DISTINCT
    if name == "cvround_f":   # every x.5 of +-2^20 (round half to even)
        k = np.arange(-(1 << 20), 1 << 20, dtype=np.float64) + 0.5
        return cat([k.astype(np.float32), sweep32(0.0, 2147483520.0, 1 << 18), sweep32(0.0, 2147483520.0, 1 << 18, 1)]), None, DISTINCT
    if name == "cvround_f_limits":
        return np.array([2147483648.0, -2147483648.0], np.float32), None, 1
    if name in ("log", "log10"):
        th = []
        for k in (0x3ff, 0x400, 0x3fe, 0x3f0, 0x40f, 0x001, 0x7fe):   # binades 1, 2, 1/2, 2^-15, 2^16, the first normal one, the last
            for mant in (0x00000, 0x00001, 0xffffe, 0xfffff, 0x6a09b, 0x6a09c, 0x6147a, 0x6b851):   # |f| < 2^-20 window, sqrt(2) split, ii | j
                th += hi_word((k << 20) | mant)
        th += [0x0010000000000000, 0x0000000000000800, 0x7fefffffffffffff - ULPS]
        fam = [np.arange(1, 200001, dtype=np.float64), 1.0 + 200000.0 * rng.random(1 << 20), 10.0 ** (-300.0 * rng.random(1 << 20)),
               np.maximum(rng.random(1 << 20), 1e-300)]   # the four families of oracle/f64math_check.c
        a = cat([around64(th, signs=(0,))] + fam + [sweep64(5e-324, 1.7e308, 1 << 20)])
        return a[a > 0], None, DISTINCT
    if name == "exp":
        th = []
        for h in (0x3fd62e42, 0x3ff0a2b2, 0x3e300000, 0x40862e42):
            th += hi_word(h)
        th += [bits64(708.3964185322641), bits64(7.45133219101941108420e+02), bits64(7.09782712893383973096e+02), bits64(744.44007192138122)]
        a = cat([around64(th), linear64(-745.0, 40.0, 1 << 21), sweep64(1e-10, 745.2, 1 << 19, 1), sweep64(1e-10, 709.9, 1 << 19)])
        return a, None, DISTINCT
    if name == "pow_pos":   # nfa(): mult_term^(n - i + 1), mult_term < p / (1 - p), integer exponents
        a = cat([rng.random(1 << 21) * 0.43, 10.0 ** (-12.0 * rng.random(1 << 20))])
        a = np.maximum(a, 1e-300)
        b = cat([np.floor(2.0 + rng.random(1 << 21) ** 3 * 70000.0), np.floor(2.0 + rng.random(1 << 20) * 200.0)])
        return a, b, DISTINCT
    if name == "sinh_small":   # log_gamma's sinh(1 / x), x > 15
        return cat([1.0 / np.arange(16, 70001, dtype=np.float64), sweep64(1e-9, 1.0 / 15.0, 1 << 21)]), None, DISTINCT
    if name == "log_gamma":    # every integer argument nfa() can have at 640x480 and beyond the table, and the Lanczos / Windschitl split
        return cat([np.arange(1, 70001, dtype=np.float64), around64([bits64(15.0), bits64(16.0)], signs=(0,)), 1.0 + 199999.0 * rng.random(1 << 19)]), None, DISTINCT
    if name in ("glibc_sin", "glibc_cos"):   # |x| < 105414350; ranges of f64math_check.c (mode sincos)
        th = [bits64(0.126), bits64(0.855469), bits64(2.426265), bits64(2.0 ** -26), bits64(2.0 ** -27)] + \
             [bits64(k * PI / 2) for k in range(1, 9)] + [bits64(k / 128.0) for k in (16, 17, 64, 109, 110)]
        a = cat([around64(th), linear64(-PI / 2, PI / 2, 1 << 20), linear64(0.0, 9.5, 1 << 20), linear64(-1000.0, 1000.0, 1 << 20),
                 linear64(-PI / 2, PI / 2, 1 << 18) * 1e-4, sweep64(1e-300, 1.05e8, 1 << 18), sweep64(1e-300, 1.05e8, 1 << 18, 1)])
        return a, None, DISTINCT
    if name == "cos_sin_f64":  # [0, 4 pi]; the quadrant changes at the odd multiples of pi / 4
        th = [bits64(k * PI / 4) for k in range(1, 17)]
        return cat([around64(th, signs=(0,)), linear64(0.0, 4 * PI, 1 << 21), sweep64(1e-300, 4 * PI, 1 << 20)]), None, DISTINCT
    if name == "cos_sin_2pi_f32":   # k_lsd_grad: a float number of degrees in [0, 360] times pi / 180
        deg = cat([sweep32(0.0, 360.0, 1 << 22), around32([bits32(d) for d in (45.0, 90.0, 135.0, 180.0, 225.0, 270.0, 315.0, 360.0 - 1e-3)], signs=(0,)),
                   np.array([0.0, 360.0], np.float32)])
        deg = deg[deg <= 360.0]
        return deg.astype(np.float64) * (3.14159265358979323846 / 180.0), None, DISTINCT
    if name == "ratio_inv":    # k_lsd_nfa_series: a = n - i + 1 < PSL_RATIO_AMAX, b = i < PSL_RATIO_BMAX; and the pairs next to the table's limits
        a = np.floor(rng.random(1 << 22) * 65536.0)
        b = np.floor(1.0 + rng.random(1 << 22) * 16383.0)
        ea, eb = np.meshgrid(np.arange(65536 - 40, 65536 + 8, dtype=np.float64), np.arange(16384 - 24, 16384 + 8, dtype=np.float64), indexing="ij")
        na, nb = np.meshgrid(np.array([54587.0, 56000.0, 60000.0, 65500.0, 65535.0]), np.arange(16290.0, 16400.0), indexing="ij")
        return cat([a, ea.ravel(), na.ravel() - nb.ravel() + 1]), cat([b, eb.ravel(), nb.ravel()]), 1 << 20
    if name == "ddiv":
        a, b = _finite64(rng, 1 << 21), _finite64(rng, 1 << 21)
        sub = f64_bits(rng.integers(1, 1 << 52, 1 << 19, dtype=np.uint64))
        nrm = _finite64(rng, 1 << 19)
        lo = f64_bits(rng.integers(0x0010000000000000, 0x2000000000000000, 1 << 20, dtype=np.uint64))
        hi = f64_bits(rng.integers(0x3ff0000000000000, 0x5ff0000000000000, 1 << 20, dtype=np.uint64))
        ints_a, ints_b = np.floor(rng.random(1 << 20) * 70000.0), np.floor(1.0 + rng.random(1 << 20) * 70000.0)   # nfa()'s (n - i + 1) / i
        a, b = cat([a, sub, nrm, sub, lo, ints_a]), cat([b, nrm, sub, sub[::-1], hi, ints_b])
        a = a.copy()
        a[(a == 0) & (b == 0)] = 1.0
        return a, b, DISTINCT
    if name == "dsqrt":
        b = rng.integers(0, 0x7ff0000000000000, 1 << 22, dtype=np.uint64)
        return cat([f64_bits(b), f64_bits(np.arange(0, 1 << 16, dtype=np.uint64)), f64_bits(rng.integers(1, 1 << 52, 1 << 18, dtype=np.uint64))]), None, DISTINCT
    if name == "cvround_d":
        k = np.arange(-(1 << 20), 1 << 20, dtype=np.float64) + 0.5
        return cat([k, linear64(-2147483647.0, 2147483647.0, 1 << 18), sweep64(1e-300, 2147483647.4, 1 << 18), sweep64(1e-300, 2147483648.4, 1 << 18, 1)]), None, DISTINCT
    if name == "cvround_d_limits":
        return np.array([2147483648.0, -2147483648.0, 2147483647.5, -2147483648.5], np.float64), None, 1
    raise KeyError(name)


# grid name -> function name of psl_slam_amd.MATH_FUNCTIONS
GRIDS = {n: n for n in ("atanf", "tanf", "sincosf", "fast_atan2", "atan2f", "fdiv", "sqrtf", "cvround_f", "log", "exp", "log10", "pow_pos",
                        "sinh_small", "log_gamma", "glibc_sin", "glibc_cos", "cos_sin_f64", "cos_sin_2pi_f32", "ratio_inv", "ddiv", "dsqrt",
                        "cvround_d")}
GRIDS["cvround_f_limits"] = "cvround_f"   # +-2^31: the conversion's range ends there
GRIDS["cvround_d_limits"] = "cvround_d"
