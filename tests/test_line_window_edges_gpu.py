"""The line window search (psl-slam_amd/csrc/pslfe_linematch.hip: LSDmatcher::SearchByProjection, modes 0 and 1) at its capacity,
tie and contention edges: the hand-built cases of tests/line_window_cases.py through the one-frame entry point and through the
batched two-launch form, against the answer written down with each case and against the sequential CPU oracle.  All comparisons
are exact.  tests/test_line_window_cases_cpu.py shows, without a GPU, that the written-down answers are the oracle's and that
every case reaches the regime it is built for (the best and the second best in one wave lane, grids of 8191 / 8192 / 8193 / 65536
entries, a line accepted by the third probe point only, the gate that removes a candidate)."""
import ctypes as C
import functools

import numpy as np
import pytest

import line_window_cases as LW

pytestmark = pytest.mark.gpu

HOST_CASES = LW.host_cases()
E_CAPACITY = -4


def _host(P, case, want_grid=False):
    return P.LSDmatcher(case.nnratio).SearchByProjection(case.kls, case.desc, case.eq, case.bounds, case.q, case.qd, mode=case.mode,
                                                         dir3d=case.dir3d if case.mode == 1 else None, taken=case.taken, want_grid=want_grid)


@pytest.mark.parametrize("case", HOST_CASES, ids=repr)
def test_host_form_equals_expected_and_oracle(case):
    import psl_slam_amd as P
    nm, match, assigned = _host(P, case)
    rnm, rmatch, rassigned = LW.run_oracle(case)
    np.testing.assert_array_equal(match, case.expected)
    np.testing.assert_array_equal(assigned, case.assigned)
    assert nm == case.nmatches
    np.testing.assert_array_equal(match, rmatch)
    np.testing.assert_array_equal(assigned, rassigned)
    assert nm == rnm


@pytest.mark.parametrize("case", LW.grid_cases(), ids=repr)
def test_host_form_grid_equals_the_oracles(case):
    """mGridForLine of the Bresenham shapes and of the full frames, cell by cell in the reference's order"""
    import psl_slam_amd as P
    import oracle_lib
    nm, match, assigned, gs, gi = _host(P, case, want_grid=True)
    rgs, rgi = oracle_lib.line_grid_build(case.kls, case.bounds)
    np.testing.assert_array_equal(gs, rgs)
    np.testing.assert_array_equal(gi, rgi)
    assert len(gi) == case.facts.get("grid_n", len(gi))
    np.testing.assert_array_equal(match, case.expected)


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def test_above_capacity_is_refused_before_any_launch():
    import psl_slam_amd as P
    c = LW.capacity_one_frame(0)
    kls, eq, desc = (np.concatenate([a, a[:1]]) for a in (c.kls, c.eq, c.desc))
    assert len(kls) == LW.LINE_MAX + 1
    with pytest.raises(P.PslfeError, match=f"code {E_CAPACITY}"):
        P.LSDmatcher().SearchByProjection(kls, desc, eq, c.bounds, c.q[:4], c.qd[:4], mode=0)
    ctx = P.default_context()
    d = _dev(ctx, np.zeros(4096, np.uint8))
    try:
        with pytest.raises(P.PslfeError, match=f"code {E_CAPACITY}"):
            P.line_search_by_projection_device(1, d, d, d, d, LW.BATCH_MAX + 1, 0, 0, c.bounds, d, d, d, 1, 0, 0, 0.95, d, 0, d, 0, ctx=ctx)
    finally:
        ctx.device_free(d)


# ---- the batched form ----------------------------------------------------------------------------------------------------------------
NPAIRS, SENTINEL = 64, -7
LAUNCHES = [(0, 0.95), (1, 0.3), (1, 0.75)]


def _empty(base, name, lines):
    n = 0 if lines else len(base.kls)
    q, qd = (base.q, base.qd) if lines else (base.q[:0], base.qd[:0])
    return LW.Case(name, base.mode, base.kls[:n], base.eq[:n], base.desc[:n], q, qd, None, {}, base.nnratio, dir3d=base.dir3d[:n])


@functools.lru_cache(maxsize=None)
def _batch(mode, nnratio):
    """64 pairs of one launch: the small cases, repeated with rotated query order and, from the second round on, a seeded `taken`
    mask, up to 58; then a pair without lines, one without queries and the four capacity pairs.
    -> per pair (case, written-down answer or None, the oracle's answer, entries of the oracle's grid)"""
    import oracle_lib
    cases = LW.device_cases(mode)
    rng = np.random.default_rng(70 + mode)
    pairs = []
    for p in range(NPAIRS - 6):
        base, rnd = cases[p % len(cases)], p // len(cases)
        shift = (7 * rnd) % len(base.q)
        taken = base.taken if rnd == 0 else (rng.random(len(base.kls)) < 0.1).astype(np.uint8)
        c = base.retarget(f"{base.name}-round{rnd}", nnratio=nnratio, q=np.roll(base.q, shift), qd=np.roll(base.qd, shift, axis=0), taken=taken)
        written = base if rnd == 0 and (mode == 0 or np.float32(base.nnratio) == np.float32(nnratio)) else None
        pairs.append((c, written))
    pairs.append((_empty(LW.chain(mode), "no-lines", True).retarget("no-lines", nnratio=nnratio), None))
    pairs.append((_empty(LW.chain(mode), "no-queries", False).retarget("no-queries", nnratio=nnratio), None))
    for e in (8191, 8192, 8193, 65536):
        base = LW.capacity_batched(mode, e)
        pairs.append((base.retarget(base.name, nnratio=nnratio), base))     # distance 0 is matched under any ratio
    out = []
    for c, written in pairs:
        entries = int(oracle_lib.line_grid_build(c.kls, c.bounds)[0][-1]) if len(c.kls) else 0
        out.append((c, written, LW.run_oracle(c), entries))
    assert len(out) == NPAIRS and [e for _, _, _, e in out[-4:]] == [8191, 8192, 8193, 65536]
    return out


def _launch(P, cases, mode, nnratio, kl_stride, qstride):
    """one batched launch of `cases` -> (match [npairs][qstride], assigned [npairs][kl_stride], nmatches [npairs], nfallback);
    the outputs are filled with SENTINEL first"""
    ctx = P.default_context()
    npairs = len(cases)
    kls = np.zeros((npairs, kl_stride), P.KEYLINE_DTYPE)
    desc = np.zeros((npairs, kl_stride, 32), np.uint8)
    eq = np.zeros((npairs, kl_stride, 3), np.float64)
    l3 = np.zeros((npairs, kl_stride, 6), np.float64)
    taken = np.zeros((npairs, kl_stride), np.uint8)
    q = np.zeros((npairs, qstride), P.LINEQUERY_DTYPE)
    qd = np.zeros((npairs, qstride, 32), np.uint8)
    nkl, nq = np.zeros(npairs, np.int32), np.zeros(npairs, np.int32)
    for p, c in enumerate(cases):
        n, m = len(c.kls), len(c.q)
        kls[p, :n], desc[p, :n], eq[p, :n], l3[p, :n, :3], nkl[p] = c.kls, c.desc, c.eq, c.dir3d, n   # mvLines3D rows: (dir3d, 0)
        q[p, :m], qd[p, :m], nq[p] = c.q, c.qd, m
        if c.taken is not None:
            taken[p, :n] = c.taken
    outs = [np.full((npairs, qstride), SENTINEL, np.int32), np.full((npairs, kl_stride), SENTINEL, np.int32),
            np.full(npairs, SENTINEL, np.int32), np.full(1, SENTINEL, np.int32)]
    ds = [_dev(ctx, a) for a in (kls, desc, eq, nkl, l3, q, qd, nq, taken, *outs)]
    try:
        d_kls, d_desc, d_eq, d_nkl, d_l3, d_q, d_qd, d_nq, d_taken, d_match, d_asg, d_nm, d_nfb = ds
        P.line_search_by_projection_device(npairs, d_kls, d_desc, d_eq, d_nkl, kl_stride, d_l3 if mode == 1 else 0, kl_stride, LW.BOUNDS,
                                           d_q, d_qd, d_nq, qstride, d_taken, mode, nnratio, d_match, d_asg, d_nm, d_nfb, ctx=ctx)
        ctx.synchronize()
        res = [_down(P, ctx, d, a) for d, a in zip((d_match, d_asg, d_nm, d_nfb), outs)]
    finally:
        for d in ds:
            ctx.device_free(d)
    return res[0], res[1], res[2], int(res[3][0])


@pytest.mark.parametrize("mode,nnratio", LAUNCHES)
def test_device_form_every_pair_equals_the_oracle(mode, nnratio):
    import psl_slam_amd as P
    pairs = _batch(mode, nnratio)
    match, asg, nm, nfb = _launch(P, [c for c, _, _, _ in pairs], mode, nnratio, LW.BATCH_MAX, 64)
    for p, (c, written, (rnm, rmatch, rasg), entries) in enumerate(pairs):
        n, m = len(c.kls), len(c.q)
        assert np.array_equal(match[p, :m], rmatch[:m]), f"pair {p} ({c.name}): matches {match[p, :m]} differ from the oracle's {rmatch[:m]}"
        assert np.array_equal(asg[p, :n], rasg[:n]), f"pair {p} ({c.name}): assignments differ from the oracle"
        assert nm[p] == rnm, f"pair {p} ({c.name}): {nm[p]} matches, the oracle has {rnm}"
        assert (match[p, m:] == SENTINEL).all() and (asg[p, n:] == SENTINEL).all(), f"pair {p} ({c.name}): rows behind the pair's counts were written"
        if written is not None:
            assert np.array_equal(match[p, :m], written.expected) and np.array_equal(asg[p, :n], written.assigned), \
                f"pair {p} ({c.name}): differs from the construction"
    big = [p for p, (_, _, _, entries) in enumerate(pairs) if entries > LW.SMALL_GRID]
    assert big == [NPAIRS - 2, NPAIRS - 1]             # 8193 and 65536 entries; the 8192 pair fits the first launch
    assert nfb == len(big)


@pytest.mark.parametrize("mode", [0, 1])
def test_second_launch_handles_more_pairs_than_workgroups(mode):
    """320 pairs of 129 .. 136 full-width lines: every grid has more than 8192 entries, and the second launch has at most one
    workgroup per CU, so a workgroup searches several pairs one after the other in the same LDS"""
    import psl_slam_amd as P
    import oracle_lib
    cases = [LW.overflow_pair(mode, p) for p in range(320)]
    assert all(oracle_lib.line_grid_build(c.kls, c.bounds)[0][-1] > LW.SMALL_GRID for c in cases[:16])
    match, asg, nm, nfb = _launch(P, cases, mode, 0.8, 136, 8)
    assert nfb == len(cases)
    total = 0
    for p, c in enumerate(cases):
        rnm, rmatch, rasg = LW.run_oracle(c)
        n, m = len(c.kls), len(c.q)
        assert np.array_equal(match[p, :m], rmatch) and nm[p] == rnm, f"pair {p}: matches {match[p, :m]} differ from the oracle's {rmatch}"
        assert np.array_equal(asg[p, :n], rasg) and (asg[p, n:] == SENTINEL).all(), f"pair {p}: assignments differ from the oracle"
        total += rnm
    assert total > len(cases)
