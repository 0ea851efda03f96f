"""The KeyFrame-rate matchers (psl-slam_amd/csrc/pslfe_kf.hip, kf_line_kernels.h) at their gate, tie and capacity edges: the
hand-built cases of tests/kf_cases.py through psl_slam_amd.KeyFrameMatcher (window_best, Fuse, FuseSim3, SearchBySim3,
SearchForTriangulation, LineFuse, ComputeDistinctiveDescriptors), against the answer written down with each case and against the
sequential CPU oracle.  All outputs are integers and all comparisons exact.  tests/test_kf_cases_cpu.py shows, without a GPU, that
the written-down answers are the oracle's and that every case reaches the regime it is built for."""
import ctypes as C
import functools

import numpy as np
import pytest

import kf_cases as K

pytestmark = pytest.mark.gpu

CASES = K.all_cases()
E_INVALID, E_CAPACITY = -1, -4     # include/pslfe.h:28-31
_grids = {}


def _of(fn):
    return [c for c in CASES if c.fn == fn]


def _grid(P, slots=1):
    if slots not in _grids:
        _grids[slots] = P.FrameGrid(512, slots)
    return _grids[slots]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return K.run_oracle(next(c for c in CASES if c.name == name))


def _hold(got, case):
    """the kernel's answer == the written-down one == the oracle's"""
    ref = _oracle(case.name)
    assert len(got) == len(case.expected) == len(ref)
    for g, e, r in zip(got, case.expected, ref):
        np.testing.assert_array_equal(g, e)
        np.testing.assert_array_equal(g, r)


@pytest.mark.parametrize("case", _of("window"), ids=repr)
def test_window_best_and_both_fuses(case):
    import psl_slam_amd as P
    i = case.inp
    g = _grid(P)
    g.set(0, i["kps"], i["desc"], K.BOUNDS, i["uright"])
    kf = P.KeyFrameMatcher()
    bi, bd = kf.window_best(g, 0, i["q"], i["qd"], i["chi2"], i["inv_sigma2"])
    _hold((bi, bd), case)
    fi, fused = kf.Fuse(g, 0, i["q"], i["qd"], i["inv_sigma2"]) if i["chi2"] else kf.FuseSim3(g, 0, i["q"], i["qd"])
    np.testing.assert_array_equal(fi, case.expected[0])
    np.testing.assert_array_equal(fused, case.expected[1] <= K.TH_LOW)


@pytest.mark.parametrize("case", _of("sim3"), ids=repr)
def test_search_by_sim3(case):
    import psl_slam_amd as P
    i = case.inp
    g = _grid(P, 2)
    g.set(0, i["kps1"], i["desc1"], K.BOUNDS)
    g.set(1, i["kps2"], i["desc2"], K.BOUNDS)
    nf, match = P.KeyFrameMatcher().SearchBySim3(g, 0, g, 1, i["q12"], i["qd1"], i["q21"], i["qd2"])
    _hold((nf, match), case)


def _triangulate(P, case):
    i = case.inp
    g = _grid(P)
    g.set(0, i["kps2"], i["desc2"], K.BOUNDS, i["uright2"])
    return P.KeyFrameMatcher().SearchForTriangulation(g, 0, i["fidx2"], i["taken2"], i["q"], i["qd"], i["F12"], i["epipole"], i["sf"], i["sig2"],
                                                      i["only_stereo"], i["check_ori"])


@pytest.mark.parametrize("case", _of("tri"), ids=repr)
def test_search_for_triangulation(case):
    import psl_slam_amd as P
    _hold(_triangulate(P, case), case)


@pytest.mark.parametrize("which,code", [(0, E_INVALID), (1, E_CAPACITY)], ids=["nq-4097", "nfidx-65536"])
def test_search_for_triangulation_refuses_what_it_cannot_hold(which, code):
    """PSL_QMAX + 1 queries: PSLFE_E_INVALID; 65536 feature-vector entries, one more than the 16-bit run position holds:
    PSLFE_E_CAPACITY; neither call writes `match`"""
    import psl_slam_amd as P
    case = K.tri_overflow()[which]
    i = case.inp
    with pytest.raises(P.PslfeError, match=f"code {code}:"):
        _triangulate(P, case)
    kf = P.KeyFrameMatcher()
    g = _grid(P)
    match = np.full(len(i["q"]), -7, np.int32)
    nm = C.c_int(-7)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = P.lib().pslfe_kf_search_for_triangulation(kf._h, g._h, C.c_int(0), p(i["fidx2"]), C.c_int(len(i["fidx2"])), p(i["taken2"]), p(i["q"]),
                                                   p(i["qd"]), C.c_int(len(i["q"])), p(i["F12"]), C.c_float(i["epipole"][0]),
                                                   C.c_float(i["epipole"][1]), C.c_int(0), C.c_int(0), p(i["sf"]), p(i["sig2"]),
                                                   C.c_int(len(i["sf"])), p(match), C.byref(nm))
    assert rc == code
    assert (match == -7).all()
    # one less of either is served
    j = dict(i, q=i["q"][:K.QMAX], qd=i["qd"][:K.QMAX], fidx2=i["fidx2"][:K.FIDX_MAX])
    nm, match = _triangulate(P, K.Case("served", "tri", None, {}, **j))
    assert nm == len(j["q"]) and (match == 0).all()


@pytest.mark.parametrize("case", _of("line"), ids=repr)
def test_line_fuse(case):
    import psl_slam_amd as P
    i = case.inp
    _hold(P.KeyFrameMatcher().LineFuse(i["kls"], i["desc"], i["q"], i["qd"]), case)


@pytest.mark.parametrize("case", _of("distinct"), ids=repr)
def test_distinctive_descriptors(case):
    import psl_slam_amd as P
    i = case.inp
    _hold((P.KeyFrameMatcher().ComputeDistinctiveDescriptors(i["desc"], i["offsets"]),), case)
