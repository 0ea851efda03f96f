"""The hand-built cases of tests/kf_cases.py for the KeyFrame-rate matchers against the sequential CPU oracle (oracle/kf_oracle.cpp):
the answer written down from each construction must be the oracle's, exactly - the construction and the oracle are two independent
statements of the reference - and every regime a case claims to reach (`facts`) is recomputed here from oracle_lib.grid_build and
plain numpy.  A case that does not reach its regime fails here, without a GPU.  tests/test_kf_edges_gpu.py then holds the kernels
to both."""
import numpy as np
import pytest

import kf_cases as K
from window_cases import rot_bin

CASES = K.all_cases()
F32 = np.float32


def _of(fn):
    return [c for c in CASES if c.fn == fn]


def _ham(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def test_dtypes_are_the_oracles():
    import oracle_lib
    assert K.TRIQUERY_DTYPE == oracle_lib.TRIQUERY_DTYPE and K.LINEFUSEQUERY_DTYPE == oracle_lib.LINEFUSEQUERY_DTYPE
    assert K.KEYLINE_DTYPE == oracle_lib.KEYLINE_DTYPE


def test_every_kind_of_case_is_there():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert {c.fn for c in CASES} == {"window", "sim3", "tri", "line", "distinct"}
    assert {len(c.inp["q"]) for c in _of("window") if "counts" in c.name} == {1, 2, 3, 5}
    assert max(len(c.inp["q"]) for c in _of("tri")) == K.QMAX and max(len(c.inp["fidx2"]) for c in _of("tri")) == K.FIDX_MAX


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_expected_is_the_oracles_answer(case):
    got = K.run_oracle(case)
    assert len(got) == len(case.expected)
    for g, e in zip(got, case.expected):
        np.testing.assert_array_equal(g, e)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_stays_inside_the_oracles_preconditions(case):
    i = case.inp
    if case.fn == "window":
        assert len(i["q"]) == len(i["qd"]) and len(i["kps"]) == len(i["desc"])
        if i["chi2"]:
            assert i["kps"]["octave"].min() >= 0 and i["kps"]["octave"].max() < len(i["inv_sigma2"]) <= 16
    elif case.fn == "sim3":
        assert len(i["q12"]) == len(i["kps1"]) == len(i["qd1"]) and len(i["q21"]) == len(i["kps2"]) == len(i["qd2"])
    elif case.fn == "tri":
        n2, nf = len(i["kps2"]), len(i["fidx2"])
        assert nf <= K.FIDX_MAX and len(i["q"]) <= K.QMAX and len(i["taken2"]) == n2
        assert (i["q"]["start"] >= 0).all() and (i["q"]["len"] >= 0).all() and (i["q"]["start"] + i["q"]["len"] <= nf).all()
        assert nf == 0 or (i["fidx2"].min() >= 0 and i["fidx2"].max() < n2)
        assert i["kps2"]["octave"].min() >= 0 and i["kps2"]["octave"].max() < len(i["sf"]) == len(i["sig2"])
    elif case.fn == "line":
        assert len(i["desc"]) <= len(i["kls"]) and len(i["q"]) == len(i["qd"])
    else:
        assert i["offsets"][0] == 0 and (np.diff(i["offsets"]) >= 0).all() and i["offsets"][-1] == len(i["desc"])


# ---- window ------------------------------------------------------------------------------------------------------------------------
def _raw_range(lo, hi, inv):
    return int(np.floor(lo * inv)), int(np.ceil(hi * inv))


def _window(case, start, idx, i):
    """-> (candidates of query i's cell range in visiting order, or None without a window; raw cell ranges before the clamp)"""
    q, b = case.inp["q"][i], K.BOUNDS
    inv = F32(64) / F32(b[2] - b[0]), F32(48) / F32(b[3] - b[1])
    u, v, r = q["u"], q["v"], q["radius"]
    rx = _raw_range(F32(F32(u - F32(b[0])) - r), F32(F32(u - F32(b[0])) + r), inv[0])
    ry = _raw_range(F32(F32(v - F32(b[1])) - r), F32(F32(v - F32(b[1])) + r), inv[1])
    cx, cy = (max(0, rx[0]), min(63, rx[1])), (max(0, ry[0]), min(47, ry[1]))
    if cx[0] >= 64 or cx[1] < 0 or cy[0] >= 48 or cy[1] < 0:
        return None, rx, ry
    runs = [idx[start[ix * 48 + cy[0]]:start[ix * 48 + cy[1] + 1]] for ix in range(cx[0], cx[1] + 1)]
    return np.concatenate(runs) if runs else np.zeros(0, np.int32), rx, ry


def _gated(case, cand, i):
    """positions in `cand` that pass the window and the level gate, and their distances"""
    k, q = case.inp["kps"], case.inp["q"][i]
    lvl = q["max_level"]
    ok = (np.abs(k["x"][cand] - q["u"]) < q["radius"]) & (np.abs(k["y"][cand] - q["v"]) < q["radius"])
    ok &= ~((k["octave"][cand] < lvl - 1) | (k["octave"][cand] > lvl))
    pos = np.flatnonzero(ok)
    return pos, np.array([_ham(case.inp["qd"][i], case.inp["desc"][cand[p]]) for p in pos], np.int64)


@pytest.mark.parametrize("case", [c for c in _of("window") if not c.name.endswith("-passall")], ids=repr)
def test_window_case_reaches_the_regime_it_claims(case):
    import oracle_lib
    f, inp = dict(case.facts), case.inp
    start, idx = oracle_lib.grid_build(inp["kps"], K.BOUNDS)
    W = {i: _window(case, start, idx, i) for i in range(len(inp["q"])) if inp["q"]["radius"][i] >= 0}
    for i, n in f.pop("T", {}).items():
        assert len(W[i][0]) == n, i
    for i, want in f.pop("tie_positions", {}).items():
        pos, dist = _gated(case, W[i][0], i)
        assert dist.min() == case.expected[1][i] and pos[dist == dist.min()].tolist() == want, i
    for i in f.pop("first_visited_has_not_the_lowest_index", []):
        pos, dist = _gated(case, W[i][0], i)
        tie = W[i][0][pos[dist == dist.min()]]
        assert tie[0] == case.expected[0][i] and tie[0] > tie.min(), i
    if "dropped" in f:
        assert sorted(set(range(len(inp["kps"]))) - set(idx.tolist())) == sorted(f.pop("dropped"))
    for i in f.pop("clipped", []):
        cand, rx, ry = W[i]
        assert cand is not None and (rx[0] < 0 or rx[1] > 63 or ry[0] < 0 or ry[1] > 47) and case.expected[0][i] >= 0, i
    for i in f.pop("outside", []):
        assert W[i][0] is None, i
    for i, want in f.pop("octaves_seen", {}).items():
        pos, _ = _gated(case, W[i][0], i)
        assert sorted(inp["kps"]["octave"][W[i][0][pos]].tolist()) == want, i
    if "nq" in f:
        assert len(inp["q"]) == f.pop("nq")
    for qi, kp, stereo, octave in f.pop("products", []):
        k, q, tab = inp["kps"][kp], inp["q"][qi], inp["inv_sigma2"]
        ur = F32(-1) if inp["uright"] is None else inp["uright"][kp]
        assert bool(ur >= 0) == stereo and k["octave"] == octave and q["max_level"] - 1 <= octave <= q["max_level"]
        ex, ey = F32(q["u"] - k["x"]), F32(q["v"] - k["y"])
        e2 = F32(F32(ex * ex) + F32(ey * ey))
        if stereo:
            er = F32(q["ur"] - ur)
            e2 = F32(e2 + F32(er * er))
        product = F32(e2 * tab[octave])
        accepted = not (float(product) > (7.8 if stereo else 5.99))
        assert accepted == (case.expected[0][qi] == kp) and (accepted or case.expected[0][qi] == -1), (qi, float(product))
        assert W[qi][0].tolist() == [kp]
    if case.name == "window-chi2":
        tab = inp["inv_sigma2"]
        assert float(tab[0]) > 7.8 and not tab[0] > F32(7.8) and float(tab[1]) < 7.8     # a float compare accepts the first probe
        assert float(tab[2]) > 5.99 > float(tab[3]) and 5.99 < float(tab[4]) < 7.8
        assert (tab[5] < 1e-3) and tab[6] > 7.8 and tab[7] < 1e-3                        # the query's level would decide differently
        assert np.signbit(inp["uright"][5]) and inp["uright"][5] == 0
    assert not f, f"facts nobody checks: {f}"


def test_the_pass_all_table_passes_every_candidate():
    """the -passall variants share the answer of their chi2-off case: no candidate inside its window comes near a limit"""
    for case in (c for c in _of("window") if c.name.endswith("-passall")):
        k, inp = case.inp["kps"], case.inp
        assert inp["chi2"] and (inp["uright"] < 0).all()
        for q in inp["q"][inp["q"]["radius"] >= 0]:
            near = (np.abs(k["x"] - q["u"]) < q["radius"]) & (np.abs(k["y"] - q["v"]) < q["radius"])
            e2 = (q["u"] - k["x"][near]).astype(np.float64) ** 2 + (q["v"] - k["y"][near]).astype(np.float64) ** 2
            assert (e2 * float(K.PASS_ALL[0]) < 1.0).all()


# ---- sim3 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _of("sim3"), ids=repr)
def test_sim3_case_reaches_the_regime_it_claims(case):
    f = dict(case.facts)
    nf, match = case.expected
    assert nf == (match >= 0).sum()
    if "agree_per_wave" in f:
        per = [int((match[w:w + 64] >= 0).sum()) for w in range(0, len(match), 64)]
        assert per == f.pop("agree_per_wave") and len(match) > 256 and per[0] and per[3] and per[4]
    assert not f


# ---- tri ---------------------------------------------------------------------------------------------------------------------------
def _line_gate(inp, qi, k2):
    """-> (den, dsqr) of CheckDistEpipolarLine in float32"""
    q, F, kp = inp["q"][qi], inp["F12"], inp["kps2"][k2]
    a = F32(F32(F32(q["x"] * F[0]) + F32(q["y"] * F[3])) + F[6])
    b = F32(F32(F32(q["x"] * F[1]) + F32(q["y"] * F[4])) + F[7])
    c = F32(F32(F32(q["x"] * F[2]) + F32(q["y"] * F[5])) + F[8])
    num = F32(F32(F32(a * kp["x"]) + F32(b * kp["y"])) + c)
    den = F32(F32(a * a) + F32(b * b))
    return den, (F32(F32(num * num) / den) if den != 0 else None)


def _epipole_d2(inp, k2):
    kp = inp["kps2"][k2]
    dx, dy = F32(F32(inp["epipole"][0]) - kp["x"]), F32(F32(inp["epipole"][1]) - kp["y"])
    return F32(F32(dx * dx) + F32(dy * dy)), F32(F32(100) * inp["sf"][kp["octave"]])


@pytest.mark.parametrize("case", [c for c in _of("tri") if c.facts], ids=repr)
def test_tri_case_reaches_the_regime_it_claims(case):
    f, inp = dict(case.facts), case.inp
    q, fidx = inp["q"], inp["fidx2"]
    run = lambda qi: fidx[q["start"][qi]:q["start"][qi] + q["len"][qi]]
    if "run_len" in f:
        assert set(q["len"].tolist()) == {f.pop("run_len")}
    for qi, want in f.pop("tie_entries", {}).items():
        d = np.array([_ham(inp["qd"][qi], inp["desc2"][k]) for k in run(qi)])
        assert d.min() <= K.TH_LOW and np.flatnonzero(d == d.min()).tolist() == want
        assert case.expected[1][qi] == run(qi)[want[-1]]
        assert len(want) < 2 or run(qi)[want[-1]] != run(qi)[want].max()     # the last visited has not the highest index either
    if "nfidx" in f:
        assert len(fidx) == f.pop("nfidx") and (q["start"] + q["len"] - 1).max() == f.pop("last_entry_read")
    if "den" in f:
        assert all(_line_gate(inp, qi, run(qi)[0])[0] == f["den"] for qi in range(len(q)))
        f.pop("den")
    note = dict(f.pop("note", {}))
    if note:
        sig2, ur = inp["sig2"], inp["uright2"]
        mono = lambda qi: not q["stereo"][qi] and not ur[run(qi)[0]] >= 0
        qi = note.pop("bar")
        d = [_ham(inp["qd"][qi], inp["desc2"][k]) for k in run(qi)]
        assert d[0] < d[1] <= K.TH_LOW and _line_gate(inp, qi, run(qi)[0])[1] > 3.84 * 100 and _line_gate(inp, qi, run(qi)[1])[1] == 0
        d2, lim = _epipole_d2(inp, run(note["epi_at"])[0])
        assert d2 == lim == 100 and mono(note.pop("epi_at"))
        d2, lim = _epipole_d2(inp, run(note["epi_below"])[0])
        assert d2 == K.down(100.0) or 99.99 < d2 < lim == 100
        assert mono(note.pop("epi_below"))
        for name, octave in (("epi_octave1", 1), ("epi_octave7", 7)):
            qi = note.pop(name)
            d2, lim = _epipole_d2(inp, run(qi)[0])
            assert inp["kps2"]["octave"][run(qi)[0]] == octave and d2 == 100 < lim and mono(qi)
        for name in ("epi_stereo2", "epi_stereo1", "epi_mono"):
            qi = note.pop(name)
            assert _epipole_d2(inp, run(qi)[0])[0] == 0 and mono(qi) == (name == "epi_mono")
        qi = note.pop("line_over")
        s = sig2[inp["kps2"]["octave"][run(qi)[0]]]
        assert _line_gate(inp, qi, run(qi)[0])[1] == 4 and 3.84 * float(s) > 4.0 and F32(F32(3.84) * s) == 4   # a float compare rejects
        qi = note.pop("line_under")
        assert _line_gate(inp, qi, run(qi)[0])[1] == 4 and 3.84 * float(sig2[inp["kps2"]["octave"][run(qi)[0]]]) < 4.0
        qi = note.pop("line_octave7")
        assert inp["kps2"]["octave"][run(qi)[0]] == len(sig2) - 1 and _line_gate(inp, qi, run(qi)[0])[1] == 9 > 3.84 * float(sig2[0])
        assert not note
    if "hist" in f:
        import oracle_lib
        _, picks = oracle_lib.search_for_triangulation(inp["kps2"], inp["desc2"], inp["uright2"], inp["taken2"], fidx, q, inp["qd"], inp["F12"],
                                                       inp["epipole"], inp["sf"], inp["sig2"], inp["only_stereo"], False)
        bins = [rot_bin(q["angle"][i], inp["kps2"]["angle"][c]) for i, c in enumerate(picks) if c >= 0]
        assert {b: bins.count(b) for b in set(bins)} == f.pop("hist")
    if "wrapped" in f:
        assert int((q["angle"] < inp["kps2"]["angle"][[run(i)[0] for i in range(len(q))]]).sum()) == f.pop("wrapped") > 0
    if "nq" in f:
        assert len(q) == f.pop("nq")
    assert not f, f"facts nobody checks: {f}"


def test_tri_overflow_inputs_are_one_past_the_limits():
    many, long_ = K.tri_overflow()
    assert len(many.inp["q"]) == K.QMAX + 1 and len(many.inp["fidx2"]) == 1
    assert len(long_.inp["fidx2"]) == K.FIDX_MAX + 1 and len(long_.inp["q"]) == 1


# ---- line --------------------------------------------------------------------------------------------------------------------------
def _direction(x1, y1, x2, y2):
    dx, dy = F32(F32(x1) - F32(x2)), F32(F32(y1) - F32(y2))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt(F32(F32(dx * dx) + F32(dy * dy)))
        return F32(dx / n), F32(dy / n)


def _cos_sita(inp, qi, k):
    q, kl = inp["q"][qi], inp["kls"][k]
    a, b = _direction(q["x1"], q["y1"], q["x2"], q["y2"]), _direction(kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"])
    with np.errstate(invalid="ignore"):
        return np.abs(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])))


def _line_candidates(inp, qi):
    """keylines that pass every gate of the search for query qi, and their distances"""
    q, out = inp["q"][qi], []
    for k, kl in enumerate(inp["kls"]):
        mx, my = 0.5 * float(F32(q["x1"] + q["x2"])), 0.5 * float(F32(q["y1"] + q["y2"]))
        if F32((mx - float(kl["pt_x"])) ** 2 + (my - float(kl["pt_y"])) ** 2) > F32(q["radius"] * q["radius"]):
            continue
        if _cos_sita(inp, qi, k) < F32(0.998) or kl["octave"] < q["level"] - 1 or kl["octave"] > q["level"] or k >= len(inp["desc"]):
            continue
        out.append((k, _ham(inp["qd"][qi], inp["desc"][k])))
    return out


@pytest.mark.parametrize("case", _of("line"), ids=repr)
def test_line_case_reaches_the_regime_it_claims(case):
    f, inp = dict(case.facts), case.inp
    assert len(inp["kls"]) == f.pop("n") and len(inp["desc"]) == f.pop("ndesc")
    cos = dict(f.pop("cos", {}))
    if cos:
        c35, c37 = _cos_sita(inp, *cos.pop("3.5")), _cos_sita(inp, *cos.pop("3.7"))
        assert c37 < F32(0.998) <= c35 and abs(float(c35) - 0.998135) < 1e-6 and abs(float(c37) - 0.997916) < 1e-6
        for name in ("nan-query", "nan-keyline"):
            assert np.isnan(_cos_sita(inp, *cos.pop(name)))
        assert not cos
    for qi, want in f.pop("ties", {}).items():
        cand = _line_candidates(inp, qi)
        best = min(d for _, d in cand)
        assert [k for k, d in cand if d == best] == want and case.expected[0][qi] == want[0]
        assert want[1] in (want[0] + 1, want[0] + 64)
    if case.name == "line-edges":
        sole = [qi for qi in range(len(inp["q"])) if inp["q"]["radius"][qi] >= 0 and [d for _, d in _line_candidates(inp, qi)] == [256]]
        assert len(sole) == 1 and case.expected[0][sole[0]] == -1 and case.expected[1][sole[0]] == 256   # the complement as the sole candidate
    if case.name.startswith("line-ndesc"):
        assert any(k >= len(inp["desc"]) for k in range(len(inp["kls"])))
    assert not f, f"facts nobody checks: {f}"


# ---- distinct ----------------------------------------------------------------------------------------------------------------------
def test_distinct_medians_are_the_written_down_ones():
    case, = _of("distinct")
    runs = K.distinct_runs()
    med = dict(case.facts["medians"])
    off = case.inp["offsets"]
    seen = set()
    for p, (name, rows, want, winner) in enumerate(runs):
        D = case.inp["desc"][off[p]:off[p + 1]]
        N = len(D)
        assert N == len(rows)
        if N == 0:
            assert winner == -1 and med.pop(name) == []
            continue
        dist = np.array([[_ham(a, b) for b in D] for a in D])
        assert (dist == np.abs(np.subtract.outer(rows, rows))).all()
        m = np.sort(dist, axis=1)[:, int(0.5 * (N - 1))]
        assert m.tolist() == med.pop(name) == want and int(np.argmin(m)) == winner == case.expected[0][p]
        seen.add(name)
        if name == "even-lower-median":                       # the upper median, and the median without the self distance, pick row 1
            assert int(np.argmin(np.sort(dist, axis=1)[:, N // 2])) == 1 != winner
        if name == "self-distance-counts":
            other = np.array([np.sort(np.delete(dist[i], i))[int(0.5 * (N - 2))] for i in range(N)])
            assert int(np.argmin(other)) == 2 != winner
        if name == "median-tie-lowest-row":
            assert (m == m.min()).sum() > 1 and winner > 0
        if name == "median-256":
            assert m.max() == 256
    assert not med and {"N=1", "N=2", "N=130"} <= seen
