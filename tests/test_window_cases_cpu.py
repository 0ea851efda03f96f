"""The hand-built window-search cases of tests/window_cases.py against the sequential CPU oracle (oracle/match_oracle.cpp): the
answer written down from each construction must be the oracle's, exactly - the construction and the oracle are two independent
statements of the reference - and every regime a case claims to reach (`facts`) is recomputed here from oracle_lib.grid_build and
plain numpy.  A case that does not reach its regime fails here, without a GPU.  tests/test_window_edges_gpu.py then holds the
kernels to both."""
import numpy as np
import pytest

import window_cases as W

CASES = W.host_cases()
INF = 1 << 30


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_expected_is_the_oracles_answer(case):
    nm, match, assigned = W.run_oracle(case)
    np.testing.assert_array_equal(match, case.expected)
    np.testing.assert_array_equal(assigned, case.assigned)
    assert nm == case.nmatches


@pytest.mark.parametrize("mode", [0, 1])
def test_device_cases_fit_one_launch_and_agree_with_the_oracle(mode):
    for case in W.device_cases(mode):
        assert len(case.kps) <= 1280 and len(case.q) <= 1280 and case.fn == ("last", "map")[mode]
        if case.expected is not None:
            nm, match, assigned = W.run_oracle(case.with_opts(check_ori=True) if mode == 0 else case)
            np.testing.assert_array_equal(match, case.expected)


def _cell_range(lo, hi, inv, ncell):
    c0, c1 = max(0, int(np.floor(lo * inv))), min(ncell - 1, int(np.ceil(hi * inv)))
    return (c0, c1) if c0 < ncell and c1 >= 0 else None


class _Analysis:
    """Per query, from the oracle's CSR grid: the candidates of the window's cell range in visiting order (what the wide pass
    walks: T of them), those that pass the gates, and these sorted by (distance, visiting position) as the kernels' keys are."""

    def __init__(self, case, sample):
        import oracle_lib
        self.case = case
        self.start, self.idx = oracle_lib.grid_build(case.kps, case.bounds)
        self.T, self.gated, self.lists = {}, {}, {}
        k, q, f32 = case.kps, case.q, np.float32
        inv = f32(64) / f32(case.bounds[2] - case.bounds[0]), f32(48) / f32(case.bounds[3] - case.bounds[1])
        bits = np.unpackbits(case.desc, axis=1).astype(np.int16)
        for i in sample:
            if case.fn == "bow":
                s, n = case.opts["runs"][i]
                cand = case.opts["fidx"][s:s + n]
                ok = np.ones(len(cand), bool)
            else:
                u, v, r = q["u"][i], q["v"][i], q["radius"][i]
                cx = _cell_range(f32(f32(u - f32(case.bounds[0])) - r), f32(f32(u - f32(case.bounds[0])) + r), inv[0], 64)
                cy = _cell_range(f32(f32(v - f32(case.bounds[1])) - r), f32(f32(v - f32(case.bounds[1])) + r), inv[1], 48)
                cand = np.zeros(0, np.int32)
                if cx and cy:
                    cand = np.concatenate([self.idx[self.start[ix * 48 + cy[0]]:self.start[ix * 48 + cy[1] + 1]] for ix in range(cx[0], cx[1] + 1)])
                ok = (np.abs(k["x"][cand] - u) < r) & (np.abs(k["y"][cand] - v) < r)
                lo, hi = q["min_level"][i], q["max_level"][i]
                if lo > 0 or hi >= 0:
                    ok &= ~(k["octave"][cand] < lo) & ~((hi >= 0) & (k["octave"][cand] > hi))
                if case.taken is not None:
                    ok &= case.taken[cand] == 0
                if case.uright is not None and case.fn != "kf":
                    ur = case.uright[cand]
                    ok &= ~((ur > 0) & (np.abs(q["ur"][i] - ur) > r))
            pos = np.flatnonzero(ok)
            dist = np.abs(bits[cand[pos]] - np.unpackbits(case.qd[i]).astype(np.int16)).sum(1)
            order = np.lexsort((pos, dist))
            self.T[i], self.gated[i] = len(cand), len(pos)
            self.lists[i] = (cand[pos][order], dist[order], pos[order])

    def blocks(self, i):
        return self.case.fn in ("kf", "bow") or bool(self.case.q["blocks"][i])

    def threshold(self):
        return {"last": W.TH_HIGH, "map": W.TH_HIGH, "bow": W.TH_LOW}.get(self.case.fn) or self.case.opts["orb_dist"]

    def jacobi_depth(self):
        """iterations of "every query picks its best candidate not taken by an earlier query of the previous iteration" in
        which a pick changes (the decision of SearchByProjection(cur,last): best distance <= threshold)"""
        nq, th = len(self.case.q), self.threshold()
        choice, blk, depth = np.full(nq, -2), np.full(len(self.case.kps), INF), 0
        while True:
            new = np.full(nq, -1)
            for i in range(nq):
                c, d, _ = self.lists[i]
                free = np.flatnonzero(~(blk[c] < i))
                if len(free) and d[free[0]] <= th:
                    new[i] = c[free[0]]
            if (new == choice).all():
                return depth
            choice, depth = new, depth + 1
            blk = np.full(len(self.case.kps), INF)
            for i in range(nq):
                if new[i] >= 0 and self.blocks(i):
                    blk[new[i]] = min(blk[new[i]], i)

    def exhausted(self, chosen):
        """queries whose TOPK best gated candidates hold fewer keypoints free of earlier queries than the decision reads (one;
        two in SearchByProjection(F, MapPoints)) while the window holds more: these must rescan the window"""
        need = 2 if self.case.fn == "map" else 1
        blk, count = np.full(len(self.case.kps), INF), 0
        for i in range(len(self.case.q)):
            c = self.lists[i][0]
            if len(c) > W.TOPK and (~(blk[c[:W.TOPK]] < i)).sum() < need:
                count += 1
            if chosen[i] >= 0 and self.blocks(i):
                blk[chosen[i]] = min(blk[chosen[i]], i)
        return count


@pytest.mark.parametrize("case", [c for c in CASES if c.opts.get("check_ori", True)], ids=repr)
def test_case_reaches_the_regime_it_claims(case):
    import oracle_lib
    nq, f = len(case.q), dict(case.facts)
    sample = range(nq) if nq <= 3200 else sorted(set(range(4)) | set(range(nq - 4, nq)) | set(range(0, nq, 97)))
    A = _Analysis(case, sample)
    full = len(A.T) == nq
    _, chosen, _ = W.run_oracle(case.with_opts(check_ori=False)) if case.fn != "map" else W.run_oracle(case)   # picks before the rotation filter
    if "grid_kept" in f:
        assert len(A.idx) == f.pop("grid_kept")
    if "dropped" in f:
        assert sorted(set(range(len(case.kps))) - set(A.idx.tolist())) == f.pop("dropped")
    if "nq" in f:
        assert nq == f.pop("nq")
    if "max_index" in f:
        assert int(case.expected.max()) == f.pop("max_index")
    if "window_T" in f:
        assert max(A.T.values()) == f.pop("window_T")
    if "window_T_all" in f:
        assert set(A.T.values()) == {f.pop("window_T_all")}
    if "gated_max" in f:
        assert max(A.gated.values()) == f.pop("gated_max")
    if "one_cell" in f:
        assert np.diff(A.start).max() == f.pop("one_cell")
    if "first_contended_query" in f:
        assert full and min(i for i in A.T if A.T[i] > 0) == f.pop("first_contended_query")
    if "empty_runs" in f:
        assert full and sum(1 for i in A.T if A.T[i] == 0) == f.pop("empty_runs")
    if "tie_ranks" in f:
        lo, hi = f.pop("tie_ranks")
        c, d, pos = A.lists[0]
        assert sorted(pos[d == d.min()].tolist()) == list(range(lo, hi + 1))
        assert pos[:W.TOPK].min() < 64 <= pos[:W.TOPK].max() and len(set(d[:W.TOPK])) == 1   # the cached list is a tie across two rounds
        cells = {(int(np.searchsorted(A.start, p, side="right")) - 1) for p in range(len(A.idx))}
        assert len(cells) > 8
    if "list_exhausted" in f:
        assert full and A.exhausted(chosen) == f.pop("list_exhausted")
    if "depth" in f:
        want = f.pop("depth")
        if case.fn != "map":
            assert full and A.jacobi_depth() == want
    if "hist" in f:
        bins = [W.rot_bin(case.q["angle"][i], case.kps["angle"][c]) for i, c in enumerate(chosen) if c >= 0]
        assert {b: bins.count(b) for b in set(bins)} == f.pop("hist")
    if "shared_keypoint" in f:
        c, cnt = np.unique(chosen[chosen >= 0], return_counts=True)
        assert (cnt.max() == 2) == f.pop("shared_keypoint")
    assert not f, f"facts nobody checks: {f}"


def test_restatements_match_the_oracle_grid():
    """window_cases.features_in_area (the float32 restatement behind the border and rotation answers) visits what the oracle's grid
    holds, in its order, for windows all over and around the image"""
    case = W.borders(False, False)   # no taken mask, no mvuRight: the analysis gates on the window and the level band alone
    A = _Analysis(case, range(len(case.q)))
    for i, e in enumerate(case.q):
        got = W.features_in_area(case.kps, case.bounds, e["u"], e["v"], e["radius"], e["min_level"], e["max_level"])
        c, _, pos = A.lists[i]
        assert got == c[np.argsort(pos)].tolist(), i
