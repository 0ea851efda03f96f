"""CPU checks of the map refresh (pslfe_kf_update_normal_and_depth, pslfe_kf_line_update_average_dir, pslfe_kf_scene_median_depth and
their device forms): the restatement of tests/map_upkeep_cases.py, which gives the GPU tests their expected rows, agrees with an
evaluation of the same formulas without rounding; its two forms are one; the seeded case is sensitive to the order of the sums, so that
a kernel that reorders them cannot pass; the median restatement is numpy's sort; the new symbols exist and check their arguments before
they touch a device; the C++ mirror compiles."""
import ctypes as C
import os
import subprocess
import tempfile
from decimal import Decimal

import numpy as np
import pytest

import map_upkeep_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 257


@pytest.fixture(scope="module")
def points():
    case = mc.point_case(M)
    mp, off, okf, ce, rk, rl, skip = case
    return case, mc.restate_points_scalar(mp, off, okf, ce, rk, rl, mc.SCALE, skip)


@pytest.fixture(scope="module")
def lines():
    case = mc.line_case(M)
    ml, off, okf, ce, rk, rl, skip = case
    return case, mc.restate_lines_scalar(ml, off, okf, ce, rk, rl, mc.SCALE, skip)


def _live(off, skip):
    return np.nonzero((np.diff(off) > 0) & (skip == 0))[0]


def test_seeded_cases_carry_load(points, lines):
    for (rows, off, okf, ce, rk, rl, skip), _ in (points, lines):
        lens = np.diff(off)
        assert set(lens.tolist()) == set(mc.RUN_LENGTHS)
        live = _live(off, skip)
        assert set(lens[live].tolist()) == set(mc.RUN_LENGTHS) - {0}       # every length is refreshed at least once
        assert abs(int(skip.sum()) - M // 3) <= 1
        assert (rk[lens == 0] == -1).all() and (rl[skip != 0] < 0).any()   # references that must not be read
    ml = lines[0][0]
    assert any((ml["sp"][i] == ml["ep"][i]).all() for i in _live(lines[0][1], lines[0][6]))


def test_untouched_rows_keep_the_canary_and_positions_are_only_read(points, lines):
    for ((rows, off, okf, ce, rk, rl, skip), out), fields, pos in ((points, mc.POINT_OUT, ("x", "y", "z")), (lines, mc.LINE_OUT, ("sp", "ep"))):
        live = np.zeros(M, bool)
        live[_live(off, skip)] = True
        assert out[~live].tobytes() == rows[~live].tobytes()
        for f in pos:
            assert out[f].tobytes() == rows[f].tobytes()
        for f in fields:
            assert not np.isnan(out[f][live]).any() and np.isnan(rows[f]).all()


def test_both_forms_of_the_restatement_are_one(points, lines):
    (mp, off, okf, ce, rk, rl, skip), want = points
    assert mc.restate_points(mp, off, okf, ce, rk, rl, mc.SCALE, skip).tobytes() == want.tobytes()
    (ml, off, okf, ce, rk, rl, skip), want = lines
    assert mc.restate_lines(ml, off, okf, ce, rk, rl, mc.SCALE, skip).tobytes() == want.tobytes()
    for n in (1, 63, 65):
        mp, off, okf, ce, rk, rl, skip = mc.point_case(n)
        assert mc.restate_points(mp, off, okf, ce, rk, rl, mc.SCALE, skip).tobytes() == \
            mc.restate_points_scalar(mp, off, okf, ce, rk, rl, mc.SCALE, skip).tobytes()


def _ulps(got, exact, ulp):
    return float(abs(Decimal(float(got)) - exact) / Decimal(float(ulp)))


COMPOUND = 2.5   # ulps of max_dist against the unrounded dist times the factor: derived in the point test's docstring


def _range_ulps(want, d, exact_dist, level, i):
    """(ulps of the float dist against the unrounded one, ulps of max_dist against the exact product of that float and the scale factor,
    ulps of max_dist against the unrounded dist times the scale factor: the first two compounded)"""
    scale = Decimal(float(mc.SCALE[level]))
    md = want["max_dist"][i]
    return (_ulps(d, exact_dist, np.spacing(d)), _ulps(md, Decimal(float(d)) * scale, np.spacing(md)), _ulps(md, exact_dist * scale, np.spacing(md)))


def test_point_restatement_agrees_with_the_unrounded_formulas(points):
    """The limit is the accumulated rounding of the sequential sum.  A term has a component of at most 1 and carries under 1.5 ulp(1) of
    rounding (the subtraction, the float reciprocal, the product); the k-th addition rounds a partial sum below k, half an ulp(k) <=
    k/2 ulp(1); the n additions and the final scaling by (float)(1/n) therefore leave under n/4 + 2 ulp(1) in a component of the normal:
    (n + 2) float ulps of 1 hold with room.
    dist is `const float dist` in the reference: it is held to 1 ulp of the unrounded norm of the unrounded differences, and max_dist =
    dist*levelScaleFactor to 1 ulp of the exact product of that float and the factor.  Against the unrounded dist times the factor the
    roundings compound: dist is off by at most 1 ulp(dist), a relative 2^-23; an ulp of max_dist is at least a relative 2^-24 of it, so
    that is at most 2 ulp(max_dist), and the product adds half an ulp: COMPOUND = 2.5 ulps, asserted (1.48 on this case)."""
    (mp, off, okf, ce, rk, rl, skip), want = points
    ulp1 = np.spacing(np.float32(1.0))
    worst = np.zeros(4)
    for i in _live(off, skip):
        n = int(off[i + 1] - off[i])
        normal, dist = mc.exact_point(mp, off, okf, ce, rk, rl, mc.SCALE, i)
        for c, f in enumerate(("nx", "ny", "nz")):
            u = _ulps(want[f][i], normal[c], ulp1)
            worst[0] = max(worst[0], u / (n + 2))
            assert u <= n + 2, (i, f, n, u)
        worst[1:] = np.maximum(worst[1:], _range_ulps(want, mc.point_dist(mp, ce, rk, i), dist, rl[i], i))
        assert want["min_dist"][i] == want["max_dist"][i] / mc.SCALE[-1]
    print("worst normal error / (n + 2) ulps; dist, max_dist, compounded max_dist in ulps:", worst.tolist())
    assert worst[1] <= 1.0 and worst[2] <= 1.0 and worst[3] <= COMPOUND


def test_line_restatement_agrees_with_the_unrounded_formulas(lines):
    """the double equivalents: (n + 2) double ulps of 1 on a component of the normal.  dist and max_dist are floats, held as for points
    from the float Mat MP = 0.5*(SP+EP) on.  MP's own rounding comes before a subtraction that can cancel, so against the unrounded
    half-sum no number of ulps of dist holds; what holds is 1 ulp(dist) plus what half an ulp of every component of MP can move the norm
    by, sqrt(sum (ulp(MP_c)/2)^2) (map_upkeep_cases.exact_line_dist_unrounded), and that is asserted too (1.47 ulps of dist at worst on
    this case)."""
    (ml, off, okf, ce, rk, rl, skip), want = lines
    ulp1 = np.spacing(np.float64(1.0))
    worst = np.zeros(4)
    from_unrounded = 0.0
    for i in _live(off, skip):
        n = int(off[i + 1] - off[i])
        normal, dist = mc.exact_line(ml, off, okf, ce, rk, rl, mc.SCALE, i)
        if (ml["sp"][i] == ml["ep"][i]).all():
            assert np.isfinite(want["normal"][i]).all()
        for c in range(3):
            u = _ulps(want["normal"][i][c], normal[c], ulp1)
            worst[0] = max(worst[0], u / (n + 2))
            assert u <= n + 2, (i, c, n, u)
        d = mc.line_dist(ml, ce, rk, i)
        worst[1:] = np.maximum(worst[1:], _range_ulps(want, d, dist, rl[i], i))
        unrounded, slack = mc.exact_line_dist_unrounded(ml, ce, rk, i)
        assert abs(Decimal(float(d)) - unrounded) <= Decimal(float(np.spacing(d))) + slack, (i, d, unrounded, slack)
        from_unrounded = max(from_unrounded, _ulps(d, unrounded, np.spacing(d)))
        assert want["min_dist"][i] == want["max_dist"][i] / mc.SCALE[-1]
    print("worst normal error / (n + 2) ulps; dist, max_dist, compounded max_dist in ulps:", worst.tolist(),
          "; dist against the unrounded half-sum:", from_unrounded)
    assert worst[1] <= 1.0 and worst[2] <= 1.0 and worst[3] <= COMPOUND


def test_seeded_point_case_is_sensitive_to_the_order_of_the_sum(points):
    """a kernel that adds the terms of a run in another order (reversed, or as a tree or shuffle reduction) gives other bytes"""
    (mp, off, okf, ce, rk, rl, skip), want = points
    rev = mc.restate_points_scalar(mp, off, okf, ce, rk, rl, mc.SCALE, skip, order="reversed")
    tree = mc.restate_points_scalar(mp, off, okf, ce, rk, rl, mc.SCALE, skip, order="pairwise")
    words = lambda a: np.stack([a[f] for f in ("nx", "ny", "nz")], 1).view(np.uint32)
    live = _live(off, skip)
    nrev = int((words(rev)[live] != words(want)[live]).any(1).sum())
    ntree = int((words(tree)[live] != words(want)[live]).any(1).sum())
    assert nrev >= 1 and ntree >= 1, (nrev, ntree)
    short = live[np.diff(off)[live] <= 2]                      # one or two terms: every order is the same sum
    assert len(short) and (words(rev)[short] == words(want)[short]).all() and (words(tree)[short] == words(want)[short]).all()
    for f in ("min_dist", "max_dist"):
        assert rev[f].tobytes() == want[f].tobytes()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 1000, 2049])
def test_median_restatement_is_numpy_sort(K, n):
    poses, xs = mc.median_case(K, n)
    dup = 0
    for q in (1, 2, 3):
        got = mc.restate_median(poses, xs, q)
        for k in range(K):
            z = np.sort(mc.depths(poses[k], xs[k]))
            assert got[k] == (z[(n - 1) // q] if n else np.float32(-1.0))
            dup += int(n > 1 and (np.diff(z) == 0).any())
    assert dup or n < 64


def test_new_entry_points_exist_and_check_their_arguments():
    import psl_slam_amd as P
    P.build()
    lib = P.lib()
    E = -1  # PSLFE_E_INVALID
    p = lambda a: C.c_void_p(a.ctypes.data)
    i32 = lambda *v: np.array(v, np.int32)
    off, okf = i32(0, 2, 2, 3), i32(0, 1, 1)
    ce = np.zeros((2, 3), np.float32)
    rk, rl = i32(0, -1, 1), i32(0, -5, 7)                     # row 1 has no observation: its reference is not looked at
    sf = np.ones(16, np.float32)
    for name, dtype in (("pslfe_kf_update_normal_and_depth", P.MAPPOINT_DTYPE), ("pslfe_kf_line_update_average_dir", P.MAPLINE_DTYPE)):
        rows = np.zeros(3, dtype)
        before = rows.tobytes()

        def host(fn=getattr(lib, name), k=None, g=p(rows), M=3, o=p(off), ok=p(okf), c=p(ce), nkf=2, r=p(rk), l=p(rl), sk=None, s=p(sf), nl=8):
            return fn(k, g, M, o, ok, c, nkf, r, l, sk, s, nl)

        def dev(**kw):
            return host(fn=getattr(lib, name + "_device"), **kw)

        skip_first = np.array([1, 0, 0], np.uint8)
        bad = [dict(M=-1), dict(nkf=-1), dict(g=None), dict(o=None), dict(ok=None), dict(c=None), dict(r=None), dict(l=None), dict(s=None),
               dict(nl=0), dict(nl=17)]
        host_only = [dict(o=p(i32(1, 2, 2, 3))), dict(o=p(i32(0, 2, 1, 3))), dict(ok=p(i32(0, 2, 1))), dict(ok=p(i32(0, -1, 1))),
                     dict(r=p(i32(2, -1, 1))), dict(r=p(i32(0, -1, -1))), dict(l=p(i32(8, -5, 7))), dict(l=p(i32(0, -5, -1))), dict(nl=7),
                     dict(nkf=1)]
        for kw in bad + host_only + [dict(), dict(sk=p(skip_first), r=p(i32(-3, -1, 1)))]:   # the last two: all but the handle is fine
            assert host(**kw) == E, (name, kw)
            assert name.encode() in lib.pslfe_last_error()
        assert b"NULL handle" in lib.pslfe_last_error()
        for kw in bad + [dict()]:
            assert dev(**kw) == E, (name, kw)
            assert (name + "_device").encode() in lib.pslfe_last_error()
        assert b"NULL handle" in lib.pslfe_last_error()
        # an empty call is PSLFE_OK and looks at nothing else; a negative count is refused first
        for fn in (lib[name], lib[name + "_device"]):
            assert fn(None, None, 0, None, None, None, 0, None, None, None, None, 0) == 0
            assert fn(None, None, 0, None, None, None, -1, None, None, None, None, 0) == E
        # no observation at all, no keyframe: the two arrays behind them may be NULL in the host form
        assert host(o=p(i32(0, 0, 0, 0)), ok=None, c=None, nkf=0) == E and b"NULL handle" in lib.pslfe_last_error()
        assert rows.tobytes() == before

    T = np.zeros(2, P.POSE_DTYPE)
    x = np.zeros((5, 3), np.float32)
    moff, depth = i32(0, 2, 5), np.full(2, 7, np.float32)

    def median(k=None, t=p(T), K=2, xs=p(x), o=p(moff), q=2, d=p(depth)):
        return lib.pslfe_kf_scene_median_depth(k, t, K, xs, o, q, d)

    for kw in (dict(K=-1), dict(t=None), dict(o=None), dict(d=None), dict(q=0), dict(q=-2), dict(o=p(i32(1, 2, 5))), dict(o=p(i32(0, 3, 2))),
               dict(xs=None), dict()):
        assert median(**kw) == E, kw
        assert b"pslfe_kf_scene_median_depth" in lib.pslfe_last_error()
    assert b"NULL handle" in lib.pslfe_last_error()
    assert median(K=0, t=None, o=None, d=None, xs=None) == 0 and (depth == 7).all()
    assert lib.pslfe_kf_set_upkeep_sum(None, 0) == E

    for name in ("UpdateNormalAndDepth", "update_normal_and_depth_device", "LineUpdateAverageDir", "line_update_average_dir_device",
                 "ComputeSceneMedianDepth", "set_upkeep_sum"):
        assert callable(getattr(P.KeyFrameMatcher, name))


def test_cpp_mirror_and_consumer_compile():
    src = r"""
#include "pslfe.hpp"
void use(pslfe::KeyFrameMatcher& m, std::vector<PslMapPointGeom>& mp, std::vector<PslMapLineGeom>& ml, const std::vector<int32_t>& off,
         const std::vector<float>& centres, const std::vector<uint8_t>& skip, const std::vector<float>& scale, const std::vector<PslPose>& Tcw) {
    m.UpdateNormalAndDepth(mp, off, off, centres, off, off, skip, scale);
    m.LineUpdateAverageDir(ml, off, off, centres, off, off, skip, scale);
    m.UpdateNormalAndDepthDevice(mp.data(), 1, off.data(), off.data(), centres.data(), 1, off.data(), off.data(), nullptr, scale);
    m.LineUpdateAverageDirDevice(ml.data(), 1, off.data(), off.data(), centres.data(), 1, off.data(), off.data(), nullptr, scale);
    m.SetUpkeepSum(PSLFE_UPKEEP_SUM_TILED);
    std::vector<float> d = m.ComputeSceneMedianDepth(Tcw, centres, off, 2);
}
"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "use_map_upkeep.cpp")
        with open(path, "w") as fh:
            fh.write(src)
        inc = ["-I", os.path.join(ROOT, "psl-slam_amd", "host"), "-I", os.path.join(ROOT, "include")]
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", *inc, path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", os.path.join(ROOT, "tools", "dropin", "map_main.cpp")],
                           capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
