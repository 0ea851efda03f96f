"""CPU checks of the hand-made stereo cases (tests/stereo_cases.py): on every case the restatement the GPU test compares with
(oracle/stereo_oracle.cpp), the numpy transcription of src/Frame.cc:1165-1340 and the written-down answers agree byte for byte, on
the pyramids OracleORB builds from the case's images; and every regime a case claims is recomputed here from its inputs and the
oracle's taps.  A case whose regime does not hold fails; none is skipped."""
import numpy as np
import pytest

import stereo_cases as sc
from stereo_cases import F32, INV, NLEVELS, SCALE

CASES = sc.all_cases() + [sc.capacity_case(2031)]


def hamming(a, b):
    return int(np.unpackbits(a ^ b).sum())


def bin_of(y, rows):
    return int(y) if 0 <= y < rows else (rows - 1 if y >= rows else 0)


def gate_pass(c, iL):
    """the right keypoints that pass the row, octave and x gates for left keypoint iL, ascending"""
    kL, kR = c["kL"][iL], c["kR"]
    if not (0 <= kL["y"] < c["h"]) or F32(kL["x"]) < 0:
        return []
    row, maxD = int(kL["y"]), sc.max_d(c["cam"])
    out = []
    for iR in range(len(kR)):
        lo, hi = sc.row_span(kR["y"][iR], kR["octave"][iR])
        if lo <= row <= hi and abs(int(kR["octave"][iR]) - int(kL["octave"])) <= 1 and F32(kL["x"] - maxD) <= kR["x"][iR] <= kL["x"]:
            out.append(iR)
    return out


def sweep(c, iL, iR):
    """vDists of the level-0 sweep for the pair (iL, iR): 11 integers"""
    L, R = c["left"].astype(np.int64), c["right"].astype(np.int64)
    xl, y0, xr = (int(sc._round(v)) for v in (c["kL"]["x"][iL], c["kL"]["y"][iL], c["kR"]["x"][iR]))
    wl = L[y0 - 5:y0 + 6, xl - 5:xl + 6] - L[y0, xl]
    return [int(np.abs(wl - (R[y0 - 5:y0 + 6, xr + i - 5:xr + i + 6] - R[y0, xr + i])).sum()) for i in range(-5, 6)]


def check_fact(c, f, taps):
    kL, kR, h = c["kL"], c["kR"], c["h"]
    ur, dep, idx, sad = taps
    kind = f[0]
    if kind == "row":
        _, iL, iR, rel = f
        lo, hi = sc.row_span(kR["y"][iR], kR["octave"][iR])
        assert int(kL["y"][iL]) == dict(below=lo - 1, min=lo, max=hi, above=hi + 1)[rel]
        assert kR["y"][iR] != np.floor(kR["y"][iR])                      # a fractional y: the float sum decides
    elif kind == "reach":
        _, iL, iR, k = f
        assert int(kL["y"][iL]) - bin_of(kR["y"][iR], h) == k == int(np.ceil(F32(2.0) * SCALE[NLEVELS - 1])) + 1
    elif kind == "span":
        assert sc.row_span(kR["y"][f[1]], kR["octave"][f[1]]) == (f[2], f[3])
    elif kind == "candidates":
        assert len(gate_pass(c, f[1])) >= f[2]
    elif kind == "bins":
        assert len({bin_of(y, h) for y in kR["y"]}) == f[1]
    elif kind == "count":
        assert (len(kL), len(kR)) == (f[1], f[2])
    elif kind == "scanpos":
        _, iL, win, pos, n = f
        row, band = int(kL["y"][iL]), int(np.ceil(F32(2.0) * SCALE[NLEVELS - 1])) + 3
        bins = np.array([bin_of(y, h) for y in kR["y"]])
        run = (bins >= max(row - band, 0)) & (bins <= min(row + band, h - 1))
        assert (bins == bins[win]).sum() == 1 and (run & (bins < bins[win])).sum() == pos
        gp = gate_pass(c, iL)
        assert len(gp) == n == run.sum() and n >= 65 and win in gp
        if pos >= 64:
            assert pos == 64 or pos == n - 1
    elif kind == "octave":
        assert int(kR["octave"][f[2]]) - int(kL["octave"][f[1]]) == f[3]
    elif kind == "x":
        _, iL, iR, rel = f
        uL, uR, maxD = F32(kL["x"][iL]), F32(kR["x"][iR]), sc.max_d(c["cam"])
        minU = F32(uL - maxD)
        assert uR == dict(minU=minU, maxU=uL)[rel] if rel in ("minU", "maxU") else \
            (uR == sc.down(minU) if rel == "minU-" else uR == sc.up(uL))
        if c["cam"] is sc.CAM_B:
            assert maxD != F32(c["cam"][0]) and minU != F32(uL - F32(c["cam"][0]))   # maxD as computed, not fx
    elif kind == "minu_negative":
        assert F32(kL["x"][f[1]] - sc.max_d(c["cam"])) < 0
    elif kind == "best":
        _, iL, a = f
        assert min(hamming(c["dL"][iL], c["dR"][j]) for j in gate_pass(c, iL)) == a
    elif kind == "tie":
        _, iL, first, n, a = f
        d = {j: hamming(c["dL"][iL], c["dR"][j]) for j in gate_pass(c, iL)}
        tied = sorted(j for j in d if d[j] == a)
        assert min(d.values()) == a and len(tied) == n and tied[0] == first
        assert all(bin_of(kR["y"][first], h) > bin_of(kR["y"][j], h) for j in tied[1:])   # scanned last
    elif kind == "window":
        _, iL, xl, y0, xr = f
        assert idx[iL] >= 0 and kL["octave"][iL] == 0
        assert (sc._round(kL["x"][iL]), sc._round(kL["y"][iL]), sc._round(kR["x"][idx[iL]])) == (xl, y0, xr)
    elif kind == "half":
        for v in (kL["x"][f[1]], kL["y"][f[1]], kR["x"][f[2]]):
            assert F32(v) - np.floor(F32(v)) == F32(0.5) and sc._round(v) == np.floor(v) + 1
    elif kind == "binc":
        _, iL, iR, inc = f
        d = sweep(c, iL, iR)
        assert d.index(min(d)) - 5 == inc
        if abs(inc) < 5:
            assert sad[iL] == min(d)
        else:
            assert sad[iL] == -1
    elif kind == "minima":
        d = sweep(c, f[1], f[2])
        assert tuple(i - 5 for i, v in enumerate(d) if v == min(d)) == f[3]
    elif kind == "delta":
        d = sweep(c, f[1], f[2])
        b = d.index(min(d))
        d1, d2, d3 = F32(d[b - 1]), F32(d[b]), F32(d[b + 1])
        assert d2 == d3 and F32(F32(d1 - d3) / F32(F32(2) * F32(F32(d1 + d3) - F32(F32(2) * d2)))) == F32(f[3])
    elif kind == "cell":
        _, iL, iR, inc, row, t = f
        L, R = c["left"].astype(np.int64), c["right"].astype(np.int64)
        xl, y0, xr = (int(sc._round(v)) for v in (kL["x"][iL], kL["y"][iL], kR["x"][iR]))
        per_row = np.abs((L[y0 - 5:y0 + 6, xl - 5:xl + 6] - L[y0, xl]) - (R[y0 - 5:y0 + 6, xr + inc - 5:xr + inc + 6] - R[y0, xr + inc])).sum(1)
        assert per_row[row + 5] == sad[iL] > 0 and per_row.sum() == sad[iL] and (t < 64) == ((inc, row) < (0, 4))
    elif kind == "disparity":
        _, iL, best, d = f
        assert float(F32(F32(kL["x"][iL]) - F32(best))) == d
    elif kind == "below":
        _, iL, best, maxD = f
        d = F32(F32(kL["x"][iL]) - F32(best))
        assert d < F32(maxD) == sc.max_d(c["cam"]) and sc.up(sc.up(d)) >= F32(maxD) and sad[iL] >= 0 and ur[iL] == F32(best)
    elif kind == "lwindow":
        _, iL, iR, level, suL, svL, sR0 = f
        s = INV[level]
        assert kL["octave"][iL] == level >= 1 and idx[iL] == iR
        assert (sc._round(F32(kL["x"][iL] * s)), sc._round(F32(kL["y"][iL] * s)), sc._round(F32(kR["x"][iR] * s))) == (suL, svL, sR0)
    elif kind == "lhalf":
        _, iL, iR, level = f
        for v in (kL["y"][iL], kR["x"][iR]):
            q = F32(v * INV[level])
            assert q - np.floor(q) == F32(0.5)
    elif kind == "accepted":
        _, iL, iR, level, inc = f
        s = INV[level]
        xl, y0, xr = (int(sc._round(F32(v * s))) for v in (kL["x"][iL], kL["y"][iL], kR["x"][iR]))
        L, R = (sc.oracle_levels(c[k])[level].astype(np.int64) for k in ("left", "right"))
        wl = L[y0 - 5:y0 + 6, xl - 5:xl + 6] - L[y0, xl]
        d = [int(np.abs(wl - (R[y0 - 5:y0 + 6, xr + i - 5:xr + i + 6] - R[y0, xr + i])).sum()) for i in range(-5, 6)]
        assert d.index(min(d)) - 5 == inc and sad[iL] == min(d) > 0 and idx[iL] == iR
    elif kind == "lhalf_at":
        assert f[2] >= 10
    elif kind == "vdists":
        assert tuple(sweep(c, f[1], f[2])) == f[3] and min(f[3]) > 32767
    elif kind == "median":
        _, M, med, th, nrej = f
        acc = np.sort(sad[sad >= 0])
        assert len(acc) == M and acc[M // 2] == med and float(sc.th_dist(med)) == th
        assert ((sad >= 0) & (ur < 0)).sum() == nrej and ((sad >= 0) & (dep < 0)).sum() == nrej
    else:
        raise AssertionError(f"unknown fact {f}")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_restatement_transcription_and_written_answers_agree(case):
    c = case
    levL, levR = sc.oracle_levels(c["left"]), sc.oracle_levels(c["right"])
    assert levL[0].tobytes() == c["left"].tobytes() and levR[0].tobytes() == c["right"].tobytes()
    got = sc.restated(c)
    want = sc.transcription(c["kL"], c["dL"], c["kR"], c["dR"], levL, levR, SCALE, INV, c["cam"][9], c["cam"][0])
    for g, x, name in zip(got, want, ("uright", "depth", "idx", "sad")):
        assert g.tobytes() == x.tobytes(), f"{c['name']}: {name} differs"
    sc.assert_expected(c, got, c["name"])
    assert (c["kL"]["octave"] >= 0).all() and (c["kL"]["octave"] < NLEVELS).all() and np.isfinite(c["kL"]["x"]).all()
    assert (c["kR"]["octave"] >= 0).all() and (c["kR"]["octave"] < NLEVELS).all() and np.isfinite(c["kR"]["y"]).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_claimed_regimes_hold(case):
    c = case
    taps = sc.restated(c)
    # descriptors of different probes can never be chosen
    if len(c["kL"]) and len(c["kR"]):
        D = np.unpackbits(c["dL"][:, None, :] ^ c["dR"][None, :, :], axis=2).sum(2)
        assert (D[c["gL"][:, None] != c["gR"][None, :]] >= sc.TH_HIGH).all()
    for f in c["facts"]:
        check_fact(c, f, taps)
    assert c["facts"] or c["expected"]["idx"]


def test_every_group_of_the_issue_has_a_fact():
    kinds = {f[0] for c in CASES for f in c["facts"]}
    assert kinds >= {"row", "reach", "span", "candidates", "bins", "count", "scanpos", "octave", "x", "minu_negative", "best", "tie",
                     "window", "half", "binc", "minima", "delta", "median", "cell", "disparity", "below", "lwindow", "lhalf", "accepted", "vdists"}
    for c in CASES:                                  # every upper-level window case has its .5-product probe
        if c["name"].startswith("windows-") and "-L" in c["name"]:
            assert any(f[0] == "lhalf" for f in c["facts"]), c["name"]
    assert {c["geom"] for c in CASES} == {"base", "odd", "pitch"} and sc.GEOMS["odd"]["h"] % 4 and sc.GEOMS["pitch"]["pad"] > 0
    assert all(n in [c["name"] for c in CASES] for n in sc.BATCH)


def test_device_seeds_reach_every_counter():
    """The seeds of the random kinds' device run (tests/test_stereo_edges_gpu.py), with the oracle alone: over the repetitions the
    restatement accepts, rejects at a window or sweep edge and filters at least one keypoint where tests/test_stereo_cpu.py asserts
    its counters."""
    for kind in sc.DEVICE_KINDS:
        rng = np.random.default_rng(sc.device_seed(kind))
        seen = dict(sad=0, filtered=0, edge=0)
        for rep in range(sc.DEVICE_REPS):
            left, right, kL, dL, kR, dR = sc.random_device_pair(rng, kind)
            cam = (sc.CAM_A, sc.CAM_B)[rep % 2]
            ur, dep, idx, sad = __import__("oracle_lib").restate_stereo(kL, dL, kR, dR, sc.oracle_levels(left), sc.oracle_levels(right), SCALE,
                                                                        INV, cam[9], cam[0])
            seen["sad"] += int((sad >= 0).sum())
            seen["filtered"] += int(((sad >= 0) & (ur < 0)).sum())
            seen["edge"] += int(((idx >= 0) & (sad < 0)).sum())
        if kind in ("noise", "noise_r", "ties"):
            assert seen["sad"] > 0 and seen["edge"] > 0 and seen["filtered"] > 0, (kind, seen)
