"""The hand-built association cases of tests/assoc_cases.py against the sequential CPU oracle (oracle/assoc_oracle.cpp): every
written-down answer must be the oracle's, exactly, and the regimes the cases claim are recomputed here.  tests/test_assoc_gpu.py
then holds the kernels of psl-slam_amd/csrc/pslfe_assoc.hip to both."""
import numpy as np
import pytest

import assoc_cases as AC

GEOM_TH = (0.95, 1.0, 0.05)


@pytest.mark.parametrize("desc_th", GEOM_TH)
def test_geom_expected_is_the_oracles_answer(desc_th):
    import oracle_lib
    c = AC.geom_case()
    n, m12, asg = oracle_lib.search_by_geom_appearance(c.kl_last, c.d_last, c.kl_cur, c.d_cur, c.has, desc_th, c.bounds)
    en, em12, easg = c.expected(desc_th)
    np.testing.assert_array_equal(m12, em12)
    np.testing.assert_array_equal(asg, easg)
    assert n == en


def test_geom_case_reaches_its_regimes():
    import oracle_lib
    c = AC.geom_case()
    assert len(c.kl_last) == 300 > 256
    idx, dist = oracle_lib.hamming_knn2(c.d_last, c.d_cur)
    crowd = np.arange(250, 290)
    assert (idx[crowd, 0] == 0).all()                                    # 40 last-frame lines share their nearest neighbour
    n, m12, asg = c.expected(0.95)
    passing = [i for i in crowd if c.spec[i][4] == "match"]
    assert asg[0] == max(passing) == 286 and min(passing) == 250 and c.has[289] == 0 and m12[289] == 0
    tie = [i for i, s in enumerate(c.spec) if s[4] == "tie"]
    assert len(tie) == 2 and (dist[tie, 0] == dist[tie, 1]).all() and (c.expected(1.0)[1][tie] == -1).all()
    for j in (1, 2):                                                     # 0.0 and -0.0: skipped, left at the knn answer, never assigned
        aimed = [i for i, s in enumerate(c.spec) if s[0] == j]
        assert len(aimed) == 2 and c.kl_cur["startPointX"][j] == 0 and (m12[aimed] == j).all() and asg[j] == -1
    assert {s[4] for s in c.spec} == {"match", "dir", "far", "skip0", "nomap", "tie"}
    # the end-point gate at exactly a tenth of the image
    k, l = c.kl_cur[3], c.kl_last
    assert abs(np.float32(k["sPointInOctaveX"] - l["sPointInOctaveX"][4])) == AC.DELTA_W and c.spec[4][4] == "match"
    assert abs(np.float32(k["sPointInOctaveX"] - l["sPointInOctaveX"][5])) > AC.DELTA_W and c.spec[5][4] == "far"
    assert abs(np.float32(k["sPointInOctaveY"] - l["sPointInOctaveY"][6])) == AC.DELTA_H and c.spec[6][4] == "match"
    # one current line: knnMatch has no second neighbour, nothing matches
    n1, m1, a1 = oracle_lib.search_by_geom_appearance(c.kl_last, c.d_last, c.kl_cur[:1], c.d_cur[:1], c.has, 0.95, c.bounds)
    assert n1 == 0 and (m1 == -1).all() and (a1 == -1).all()


BF_CASES = AC.bf_cases()


@pytest.mark.parametrize("case", BF_CASES, ids=repr)
def test_bf_expected_is_the_oracles_answer(case):
    import oracle_lib
    np.testing.assert_array_equal(oracle_lib.frame_bf_match(case.d1, case.d2, case.nnratio, case.TH), case.expected)


def test_bf_cases_reach_their_regimes():
    assert sorted(len(c.d1) for c in BF_CASES if c.name.startswith("bf-spread"))[::2] == [255, 256, 257]
    assert {len(c.d1) for c in BF_CASES} >= {1, 2, 255, 256, 257} and any(len(c.d2) == 2 for c in BF_CASES)
    for c in BF_CASES:
        if c.name.startswith("bf-spread"):
            n1 = len(c.d1)
            dev = np.abs(c.margin - np.sort(c.margin)[n1 // 2])
            assert (dev == np.sort(dev)[n1 // 2]).sum() >= 3 and np.sort(dev)[n1 // 2] == 36      # the rank-n1/2 deviation is one of many
            assert {26.0, 27.0} <= set(c.margin.tolist()) and 26 < c.th < 27
            assert (c.expected >= 0).any() and (c.expected < 0).any() and {0, 1, 2} >= set(c.expected[c.expected >= 0].tolist())


PLANE_CASES = AC.plane_cases()


@pytest.mark.parametrize("case", PLANE_CASES, ids=repr)
def test_planes_expected_is_the_oracles_answer(case):
    import oracle_lib
    n, assoc = oracle_lib.associate_planes(case.planes, case.points, case.map, case.dTh, case.aTh, case.live, case.bad)
    np.testing.assert_array_equal(assoc, case.expected)
    assert n == case.nmatches


def test_plane_angle_cases_sit_on_the_threshold():
    c = [c for c in PLANE_CASES if c.name.startswith("angle")][0]
    dots = (c.planes[:, :3] * c.map[0, :3]).sum(1)
    assert dots[0] == np.float32(c.aTh) and dots[1] == -np.float32(c.aTh) and dots[2] == np.nextafter(np.float32(0.5), np.float32(1)) == -dots[3]
