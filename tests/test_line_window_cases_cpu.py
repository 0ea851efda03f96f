"""The hand-built line window cases of tests/line_window_cases.py against the sequential CPU oracle (oracle/linematch_oracle.cpp):
the answer written down from each construction must be the oracle's, exactly, and every regime a case claims to reach (`facts`)
is recomputed here from oracle_lib.line_grid_build and plain numpy - the candidate list of GetFeaturesInAreaForLine with the probe
point that accepted each line, the gate that removed a candidate, the list positions (and wave lanes) of the best and the second
best, the grid's entry count and the cells of a line.  A case that does not reach its regime fails here, without a GPU.
tests/test_line_window_edges_gpu.py then holds the kernels to both."""
import numpy as np
import pytest

import line_window_cases as LW

CASES = LW.host_cases()
F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_expected_is_the_oracles_answer(case):
    nm, match, assigned = LW.run_oracle(case)
    np.testing.assert_array_equal(match, case.expected)
    np.testing.assert_array_equal(assigned, case.assigned)
    assert nm == case.nmatches


def test_device_cases_fit_one_launch():
    for mode in (0, 1):
        cs = LW.device_cases(mode)
        assert len(cs) >= 8 and all(c.mode == mode and len(c.kls) <= LW.BATCH_MAX and len(c.q) <= 64 for c in cs)
    for p in (0, 7, 319):
        c = LW.overflow_pair(0, p)
        assert 129 <= len(c.kls) <= 136 and len(c.q) == 8


def _candidates(case, start, idx, e):
    """Frame::GetFeaturesInAreaForLine src/Frame.cc:752-826 in float32, statement by statement, over the oracle's CSR grid
    -> [(line, probe)] in list order"""
    k, eq = case.kls, case.eq
    mnx, mny = F32(case.bounds[0]), F32(case.bounds[1])
    iw, ih = F32(64) / F32(case.bounds[2] - case.bounds[0]), F32(48) / F32(case.bounds[3] - case.bounds[1])
    xs = [e["x1"], F32(F64(F32(e["x1"] + e["x2"])) / 2.0), e["x2"]]
    ys = [e["y1"], F32(F64(F32(e["y1"] + e["y2"])) / 2.0), e["y2"]]
    d1x, d1y = F32(e["x1"] - e["x2"]), F32(e["y1"] - e["y2"])
    n1 = np.sqrt(F32(F32(d1x * d1x) + F32(d1y * d1y)))
    with np.errstate(invalid="ignore", divide="ignore"):
        d1x, d1y = F32(d1x / n1), F32(d1y / n1)
    r, out, seen = e["radius"], [], set()
    for p in range(3):
        c0x = max(0, int(np.floor(F32(F32(F32(xs[p] - mnx) - r) * iw))))
        if c0x >= 64: continue
        c1x = min(63, int(np.ceil(F32(F32(F32(xs[p] - mnx) + r) * iw))))
        if c1x < 0: continue
        c0y = max(0, int(np.floor(F32(F32(F32(ys[p] - mny) - r) * ih))))
        if c0y >= 48: continue
        c1y = min(47, int(np.ceil(F32(F32(F32(ys[p] - mny) + r) * ih))))
        if c1y < 0: continue
        for ix in range(c0x, c1x + 1):
            for j in idx[start[ix * 48 + c0y]:start[ix * 48 + c1y + 1]]:
                if j in seen: continue
                d2x, d2y = F32(k["startPointX"][j] - k["endPointX"][j]), F32(k["startPointY"][j] - k["endPointY"][j])
                n2 = np.sqrt(F32(F32(d2x * d2x) + F32(d2y * d2y)))
                with np.errstate(invalid="ignore", divide="ignore"):
                    cos = abs(F32(F32(d1x * F32(d2x / n2)) + F32(d1y * F32(d2y / n2))))
                if cos < e["th_cos"]: continue
                dist = F32(eq[j, 0] * F64(xs[p]) + eq[j, 1] * F64(ys[p]) + eq[j, 2])
                if abs(dist) < r:
                    out.append((int(j), p)); seen.add(j)
    return out


def _gate(case, e, j):
    """the gate of the search loop that removes line j for query e, or None (add_src/LSDmatcher.cpp:170-195 / :300-313)"""
    k = case.kls[j]
    if case.mode == 0:
        vc = np.array([F32(k["ePointInOctaveX"] - k["sPointInOctaveX"]), F32(k["ePointInOctaveY"] - k["sPointInOctaveY"])], F64)
        vl = np.array([e["vx"], e["vy"]], F64)
        if abs((vc[0] * vl[0] + vc[1] * vl[1]) / (np.sqrt(vc[0] * vc[0] + vc[1] * vc[1]) * np.sqrt(vl[0] * vl[0] + vl[1] * vl[1]))) < LW.COS10:
            return "dir"
        mx, mn = max(e["length"], k["lineLength"]), min(e["length"], k["lineLength"])
        return "len" if F64(F32(mn / mx)) < 0.75 else None
    f, w = case.dir3d[j], e["wdir"]
    dot = F32(f[0] * w[0] + f[1] * w[1] + f[2] * w[2])
    mf, mw = F32(np.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])), F32(np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]))
    return "dir3d" if F64(abs(F32(dot / F32(mf * mw)))) < LW.COS15 else None


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_reaches_the_regime_it_claims(case):
    import oracle_lib
    f = {k: v for k, v in case.facts.items()}
    start, idx = oracle_lib.line_grid_build(case.kls, case.bounds)
    _, chosen, _ = LW.run_oracle(case)
    if "grid_n" in f:
        assert len(idx) == start[-1] == f.pop("grid_n")
    if "max_cell" in f:
        assert np.diff(start).max() <= f.pop("max_cell")
    if "cells" in f:
        cell_of = np.repeat(np.arange(64 * 48), np.diff(start))
        for line, cells in f.pop("cells").items():
            got = sorted((int(c) // 48, int(c) % 48) for c in cell_of[idx == line])
            assert got == sorted(cells), f"line {line}"
    named = set()
    for key in ("ncand", "list", "probe", "gate", "best_second", "lanes"):
        named |= set(f.get(key, {}))
    blocked = np.zeros(len(case.kls), bool) if case.taken is None else np.asarray(case.taken, bool).copy()
    bits = np.unpackbits(case.desc, axis=1).astype(np.int16)
    for qi, e in enumerate(case.q):
        if qi in named:
            cand = _candidates(case, start, idx, e)
            lines = [j for j, _ in cand]
            if qi in f.get("ncand", {}):
                assert len(cand) == f["ncand"][qi], f"query {qi}"
            if qi in f.get("list", {}):
                assert lines == list(f["list"][qi]), f"query {qi}"
            if qi in f.get("probe", {}):
                assert {j: p for j, p in cand if j in f["probe"][qi]} == f["probe"][qi], f"query {qi}"
            why = {j: ("taken" if blocked[j] else _gate(case, e, j)) for j in lines}
            if qi in f.get("gate", {}):
                assert {j: w for j, w in why.items() if w} == f["gate"][qi], f"query {qi}"
            left = [(int(np.abs(bits[j] - np.unpackbits(case.qd[qi]).astype(np.int16)).sum()), pos) for pos, j in enumerate(lines) if not why[j]]
            left.sort()
            pos12 = tuple(left[i][1] if i < len(left) else -1 for i in range(2))
            if qi in f.get("best_second", {}):
                assert pos12 == tuple(f["best_second"][qi]), f"query {qi}"
            if qi in f.get("lanes", {}):
                assert tuple(p % 64 if p >= 0 else -1 for p in pos12) == tuple(f["lanes"][qi]), f"query {qi}"
        if chosen[qi] >= 0:
            blocked[chosen[qi]] = bool(e["blocks"])
    for key in ("ncand", "list", "probe", "gate", "best_second", "lanes"):
        f.pop(key, None)
    assert not f, f"facts nobody checks: {f}"


def test_the_claimed_regimes_are_all_there():
    """the regimes these cases exist for, each present in some case's facts"""
    by = {c.name: c for c in CASES}
    assert [by[f"capacity-batched-mode0-{e}"].facts["grid_n"] for e in (8191, 8192, 8193, 65536)] == [8191, 8192, 8193, 65536]
    assert len(by["capacity-one-frame-mode0-n2048"].kls) == LW.LINE_MAX
    assert by["same-lane-mode1-3-67-131-0.6-oct0"].facts["lanes"][0] == (3, 3) and by["same-lane-mode1-67-3-131-0.4-oct1"].facts["best_second"][0] == (67, 3)
    assert by["probe-order-mode0"].facts["probe"][0][0] == 2 and by["probe-order-mode0"].facts["probe"][3][5] == 1
    assert {w for c in CASES for g in c.facts.get("gate", {}).values() for w in g.values()} == {"taken", "dir", "len", "dir3d"}
