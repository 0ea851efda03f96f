"""The hand-built ORB extractor inputs of tests/orb_cases.py against the oracle, before tests/test_orb_edges_gpu.py runs the HIP
kernels on them: the written-down FAST answers equal the oracle's candidates, every regime claim of the table holds in the geometry
restatement, and the oracle's resize - the arbiter of the pyramid comparisons at the new scale factors - equals the numpy
restatement at those ratios.  No GPU.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import orb_cases as oc
import synth_frames as sf

THRESHOLDS = [(20, 7), (7, 20), (7, 7), (40, 40), (21, 8), (255, 0)]


def _oracle_candidates(img, ini, mn):
    o = oracle_lib.OracleORB(100, 1.2, 1, ini, mn)
    o(img)
    return o.candidates(0)


@pytest.fixture(scope="module")
def lattice():
    return oc.dot_lattice()


@pytest.mark.parametrize("ini,mn", THRESHOLDS)
def test_dot_lattice_rule_equals_oracle(lattice, ini, mn):
    img, dots = lattice
    exp = oc.expected_candidates(dots, ini, mn)
    got = _oracle_candidates(img, ini, mn)
    assert got.shape == exp.shape and len(exp) > 100, (got.shape, exp.shape)
    np.testing.assert_array_equal(got, exp)


def test_dot_lattice_holds_what_it_was_built_for(lattice):
    """Independent of expected_candidates: the contrasts, the seams, the two cell kinds and the frame, read off the dots."""
    img, dots = lattice
    L = oc.geometry(oc.DOT_W, oc.DOT_H, 1.2, 1, 1)["levels"][0]
    assert (L["nCols"], L["nRows"], L["wCell"], L["hCell"], L["W"], L["H"]) == (9, 6, 32, 35, 288, 208)
    inner = [(x, y, c) for x, y, c in dots if 3 <= x < L["W"] - 3 and 3 <= y < L["H"] - 3]
    frame = [(x, y, c) for x, y, c in dots if not (3 <= x < L["W"] - 3 and 3 <= y < L["H"] - 3)]
    assert {c for _, _, c in inner} == {s * c for c in oc.CONTRASTS for s in (1, -1)} - {-155} | {-100}
    assert {(x - 3) % 32 for x, _, _ in inner} >= {0, 31} and {(y - 3) % 35 for _, y, _ in inner} >= {0, 34}    # both seams, both axes
    assert len(frame) > 50 and all(abs(c) == 60 for _, _, c in frame)
    assert any(x < 0 for x, _, _ in frame) and any(0 <= x < 3 for x, _, _ in frame) and any(x >= L["W"] - 3 for x, _, _ in frame)
    assert any(y < 0 for _, y, _ in frame) and any(0 <= y < 3 for _, y, _ in frame) and any(y >= L["H"] - 3 for _, y, _ in frame)
    cells = {}
    for x, y, c in inner:
        cells.setdefault(((y - 3) // 35, (x - 3) // 32), []).append((x, y, abs(c) - 1))
    assert len(cells) == 54
    strong = {k for k, v in cells.items() if any(s >= 20 for _, _, s in v)}
    assert 20 <= len(strong) <= 34                                   # both kinds are well represented
    got = {tuple(r) for r in _oracle_candidates(img, 20, 7)}
    want = set()
    for k, v in cells.items():
        assert any(s < 7 for _, _, s in v) and any(7 <= s < 20 for _, _, s in v)
        want |= {d for d in v if d[2] >= (20 if k in strong else 7)}
    assert got == want                                               # weak dots of strong cells vanish, S >= 7 of weak cells all appear
    assert not got & {(x, y, 59) for x, y, _ in frame}


@pytest.mark.parametrize("bg,sign", [(0, 1), (255, -1)])
def test_score_ceiling(bg, sign):
    dots = [(x, y, sign * c) for x, y, c in oc.ceiling_dots()]
    got = _oracle_candidates(oc.dot_image(dots, bg=bg), 20, 7)
    assert got.tolist() == [[67, 38, 254], [170, 115, 7]]
    np.testing.assert_array_equal(oc.expected_candidates(dots, 20, 7), got)


def test_adjacent_pairs_follow_the_strict_nms():
    dots, hand = oc.pair_dots()
    got = _oracle_candidates(oc.dot_image(dots), 20, 7)
    np.testing.assert_array_equal(got, hand)
    np.testing.assert_array_equal(oc.expected_candidates(dots, 20, 7), hand)
    assert len(hand) == 22 and len(dots) == 49


@pytest.mark.parametrize("case", oc.REGIMES, ids=lambda c: c["name"])
def test_regime_claims_hold_and_the_oracle_runs(case):
    claims = oc.regime_claims(case)
    assert len(claims) >= 2 or case["name"].startswith("th_"), "a row of the table must state its regime"
    for text, ok in claims:
        assert ok, f"{case['name']}: {text}"
    if not case["accept"]:
        return
    g = oc.case_geometry(case)
    o = oracle_lib.OracleORB(**oc.case_config(case))
    k, d = o(oc.case_image(case))
    assert len(k) > 0 and d.shape == (len(k), 32)
    # the restatement's level sizes and quotas are the oracle's
    assert o.quota() == [L["quota"] for L in g["levels"]]
    for l, L in enumerate(g["levels"]):
        w, h = C.c_int(), C.c_int()
        assert o.L.pso_orb_level_size(o.h, l, C.byref(w), C.byref(h)) == 0
        assert (w.value, h.value) == (L["w"], L["h"])
    if case["name"] == "quota_0":
        assert len(k) == 44 and all(len(o.level_keypoints(l)) > 0 for l in range(7))   # the octree returns its first split whatever N is
    if case["name"] == "nini_bound":
        assert len(k) == 80                                                             # == kp_cap = 4 * nIni
    if case["name"] == "cap_512":
        assert len(k) == 511
    if case["name"] == "th_7_20":
        assert 7 <= k["response"].min() < 20                                            # corners the 20-floor would drop
    if case["name"] == "th_255_0":
        assert k["response"].min() >= 1


def test_width_sweep_claims_hold_and_the_oracle_runs():
    for text, ok in oc.width_sweep_claims():
        assert ok, text
    for case in oc.WIDTH_SWEEP:
        k, _ = oracle_lib.OracleORB(**oc.case_config(case))(oc.case_image(case))
        assert len(k) > 0, case["name"]


@pytest.mark.parametrize("sw,sh,ratio", [(321, 243, 1.1), (323, 241, 1.3), (325, 247, 1.35), (321, 241, 1.5), (323, 243, 2.0), (320, 240, 2.0)])
def test_oracle_resize_equals_numpy_at_the_new_ratios(oracle, sw, sh, ratio):
    """Odd source sizes: the last column and row are clamped taps at every ratio."""
    src = sf.random_gray(sw, sh, 5 + sw, "noise")
    dw, dh = int(np.rint(sw / ratio)), int(np.rint(sh / ratio))
    dst = np.zeros((dh, dw), np.uint8)
    oracle.pso_resize_linear_u8(src.ctypes.data, sw, sh, dst.ctypes.data, dw, dh)
    np.testing.assert_array_equal(dst, oc.resize_numpy(src, dw, dh))
    sx, _, _ = oc.resize_tables(sw, dw)
    assert sx.max() + 1 >= sw - 1                                    # the right tap reaches the last column
