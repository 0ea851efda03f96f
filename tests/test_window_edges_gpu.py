"""The ORB window searches (psl-slam_amd/csrc/pslfe_match.hip, match_kernels.h) at their capacity, tie and contention edges: the
hand-built cases of tests/window_cases.py through the four host entry points and through the two batched device forms, against
the answer written down with each case and against the sequential CPU oracle.  All comparisons are exact.
tests/test_window_cases_cpu.py shows, without a GPU, that the written-down answers are the oracle's and that every case reaches
the regime it is built for (rows r = 1..3 of the resolving threads, a fixpoint of 300 iterations, the rescan of an exhausted
candidate list, ties across cells and across the 64-candidate rounds, a window of all 4096 keypoints, the image borders)."""
import ctypes as C
import functools

import numpy as np
import pytest

import window_cases as W

pytestmark = pytest.mark.gpu

HOST_CASES = W.host_cases()
_grids = {}


def _grid(P, cap, frames=1):
    if (cap, frames) not in _grids:
        _grids[(cap, frames)] = P.FrameGrid(cap, frames)
    return _grids[(cap, frames)]


def _capacity(case):
    """4096 for the capacity cases, else the smallest power of two that holds the case's keypoints"""
    return 1 << max(int(len(case.kps) - 1).bit_length(), 0)


def _run_host(P, case):
    g = _grid(P, _capacity(case))
    g.set(0, case.kps, case.desc, case.bounds, case.uright)
    o = case.opts
    m = P.ORBmatcher(o.get("nnratio", 0.9), o.get("check_ori", False))
    if case.fn == "last":
        return m.SearchByProjectionLast(g, 0, case.q, case.qd, case.taken)
    if case.fn == "map":
        return m.SearchByProjectionMap(g, 0, case.q, case.qd, case.taken)
    if case.fn == "kf":
        return m.SearchByProjectionKF(g, 0, case.q, case.qd, case.taken, ORBdist=o["orb_dist"])
    return m.SearchByBoW(g, 0, o["fidx"], o["runs"], o["qangle"], case.qd)


@pytest.mark.parametrize("case", HOST_CASES, ids=repr)
def test_host_form_equals_expected_and_oracle(case):
    import psl_slam_amd as P
    if case.name.startswith(("capacity", "whole")):
        assert _capacity(case) == 4096
    nm, match, assigned = _run_host(P, case)
    rnm, rmatch, rassigned = W.run_oracle(case)
    np.testing.assert_array_equal(match, case.expected)
    np.testing.assert_array_equal(assigned, case.assigned)
    assert nm == case.nmatches
    np.testing.assert_array_equal(match, rmatch)
    np.testing.assert_array_equal(assigned, rassigned)
    assert nm == rnm


def test_grid_of_the_capacity_frame_equals_the_oracles():
    """all 4096 keypoints of the lattice in the CSR grid, in the reference's order; and the border frame's dropped keypoints"""
    import psl_slam_amd as P
    import oracle_lib
    for case in (W.capacity("last"), W.borders(), W.pile_up("last")):
        g = _grid(P, _capacity(case))
        g.set(0, case.kps, case.desc, case.bounds)
        start, idx = g.debug_grid(0)
        rstart, ridx = oracle_lib.grid_build(case.kps, case.bounds)
        np.testing.assert_array_equal(start, rstart)
        np.testing.assert_array_equal(idx, ridx)
        assert len(idx) == case.facts.get("grid_kept", len(case.kps))


# ---- the batched device forms ----------------------------------------------------------------------------------------------------
NPAIRS, QSTRIDE = 64, 1280
LAUNCHES = {"staged-64x1280": (1280, 64), "wave-63x1280": (1280, 63), "wave-64x1281": (1281, 64)}


@functools.lru_cache(maxsize=None)
def _batch(mode):
    """64 pairs for one launch: the device cases, repeated with rotated query order (and, in mode 1, from the third round on with
    a random `taken` mask) to fill 64; the last two pairs are cut to 0 queries and to 1.  -> per pair (case, nq, oracle's answer)"""
    cases = W.device_cases(mode)
    rng = np.random.default_rng(40 + mode)
    pairs = []
    for p in range(NPAIRS):
        base, rnd = cases[p % len(cases)], p // len(cases)
        c = base
        if rnd or p >= NPAIRS - 2:
            c = base.retarget(base.fn, **({"check_ori": True} if mode == 0 else {}))
            shift = (37 * rnd) % max(len(c.q), 1)
            c.q, c.qd = np.roll(base.q, shift), np.roll(base.qd, shift, axis=0)
            if mode == 1 and rnd >= 2:
                c.taken = (rng.random(len(c.kps)) < 0.1).astype(np.uint8)
            if p >= NPAIRS - 2:
                c.q, c.qd = c.q[:p - (NPAIRS - 2)], c.qd[:p - (NPAIRS - 2)]
        elif mode == 0:
            c = base.with_opts(base.name, check_ori=True)
        pairs.append((c, len(c.q), W.run_oracle(c)))
    assert sorted({nq for _, nq, _ in pairs})[:2] == [0, 1] and max(nq for _, nq, _ in pairs) == QSTRIDE
    return pairs


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


@functools.lru_cache(maxsize=None)
def _launch(mode, name):
    """one launch of the batch -> (match [npairs][QSTRIDE], nmatches [npairs]); rows behind a pair's queries keep the fill -7"""
    import psl_slam_amd as P
    cap, npairs = LAUNCHES[name]
    pairs = _batch(mode)
    g = _grid(P, cap, NPAIRS)
    ctx = g.ctx
    q = np.zeros((NPAIRS, QSTRIDE), P.PROJQUERY_DTYPE)
    qd = np.zeros((NPAIRS, QSTRIDE, 32), np.uint8)
    nq = np.zeros(NPAIRS, np.int32)
    taken = np.zeros((NPAIRS, cap), np.uint8)
    for p, (c, n, _) in enumerate(pairs):
        g.set(p, c.kps, c.desc, c.bounds, c.uright)
        q[p, :n], qd[p, :n], nq[p] = c.q, c.qd, n
        if c.taken is not None:
            taken[p, :len(c.kps)] = c.taken
    ds = [_dev(ctx, a) for a in (q, qd, nq, np.full((NPAIRS, QSTRIDE), -7, np.int32), np.full(NPAIRS, -99, np.int32), taken)]
    try:
        d_q, d_qd, d_nq, d_match, d_nm, d_taken = ds
        if mode == 0:
            P.search_by_projection_last_device(g, 0, npairs, d_q, d_qd, d_nq, QSTRIDE, True, d_match, d_nm)
        else:
            P.search_by_projection_map_device(g, 0, npairs, d_q, d_qd, d_nq, QSTRIDE, d_taken, 0.8, d_match, d_nm)
        ctx.synchronize()
        match = _down(P, ctx, d_match, np.zeros((NPAIRS, QSTRIDE), np.int32))
        nm = _down(P, ctx, d_nm, np.zeros(NPAIRS, np.int32))
    finally:
        for d in ds:
            ctx.device_free(d)
    return match[:npairs], nm[:npairs]


@pytest.mark.parametrize("name", LAUNCHES)
@pytest.mark.parametrize("mode", [0, 1])
def test_device_form_every_pair_equals_the_oracle(mode, name):
    match, nm = _launch(mode, name)
    for p, (c, n, (rnm, rmatch, _)) in enumerate(_batch(mode)[:len(match)]):
        assert np.array_equal(match[p, :n], rmatch), f"pair {p} ({c.name}): matches differ from the oracle at {np.flatnonzero(match[p, :n] != rmatch)[:8]}"
        assert nm[p] == rnm, f"pair {p} ({c.name}): {nm[p]} matches, the oracle has {rnm}"
        assert (match[p, n:] == -7).all(), f"pair {p} ({c.name}): rows behind the pair's {n} queries were written"
        if c.expected is not None:
            assert np.array_equal(match[p, :n], c.expected), f"pair {p} ({c.name}): matches differ from the construction"


@pytest.mark.parametrize("mode", [0, 1])
def test_device_launches_agree_row_for_row(mode):
    """the staged kernel (64 pairs, capacity 1280), the wave-per-query kernel below 64 pairs and the one above capacity 1280"""
    staged, wave63, wave1281 = (_launch(mode, name) for name in LAUNCHES)
    assert np.array_equal(staged[0][:63], wave63[0]) and np.array_equal(staged[1][:63], wave63[1])
    assert np.array_equal(staged[0], wave1281[0]) and np.array_equal(staged[1], wave1281[1])
