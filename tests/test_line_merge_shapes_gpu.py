"""k_line_merge on hand-made segment lists, one list per launch, against the CPU oracle, every KeyLine field bit for bit.

The lists aim at the places where the kernel's LDS working set changes shape: the empty and the tiny list, singleton raw clusters
only (the copy path and the offset scan of the sub-cluster stage), one raw cluster of hundreds of lines (frontiers wider than a
wave, a long sub-cluster walk, and more adjacency words than the LDS cap holds: the HBM fallback), nine hubs that share their
neighbours (more list entries than the LDS cap holds: the other HBM fallback), the last list of the 512-line instance and the first of the 1024-line one, and exact ties in the angle rank, in the
stable length sort and at the `cs <= 2` boundary between copied and walked raw clusters.  The expected keyline counts are
what the CPU oracle returns for these lists; they pin the lists, the comparison with the oracle is the test."""
import numpy as np
import pytest

from line_cases import kl_equal

pytestmark = pytest.mark.gpu

W, H = 640, 480


def _piece(x0, y0, ang, t0, t1, off=0.0):
    """The piece [t0, t1] of the line through (x0, y0) at angle `ang`, shifted sideways by `off`."""
    c, s = np.cos(ang), np.sin(ang)
    return [x0 + t0 * c - off * s, y0 + t0 * s + off * c, x0 + t1 * c - off * s, y0 + t1 * s + off * c]


def tiny(n):
    """n short collinear pieces, a 2-px gap between neighbours: they merge into one line."""
    return np.array([[10, 100, 70, 100], [72, 100, 130, 100], [132, 100, 200, 100]][:n], np.float32).reshape(-1, 4)


def separated():
    """300 segments at 300 different angles on a 20 x 15 grid.  Lines close in angle lie far apart, so nothing merges: every raw
    cluster is a singleton.  Every fourth one is 40 px long and falls to FilterShortLines."""
    seg = []
    for cell in range(300):
        a = (cell * 127) % 300                       # neighbours in the grid are 127 angle steps apart
        ang = -np.pi / 2 + (a + 0.5) * np.pi / 300
        cx, cy = 16 + 32 * (cell % 20), 16 + 32 * (cell // 20)
        half = 20.0 if cell % 4 == 0 else 30.0 + (cell % 7)
        seg.append(_piece(cx, cy, ang, -half, half))
    return np.array(seg, np.float32)


def collinear(n, nlines, seed):
    """n overlapping pieces, 60 to 120 px long, of `nlines` long lines with different directions: pieces of a line lie within 3 px
    of it and within 30 mrad of its direction, so a line's pieces form one raw cluster but not one clique."""
    rng = np.random.default_rng(seed)
    base = [(20.0, 240.0, 0.0), (20.0, 40.0, 0.35), (60.0, 470.0, -0.6), (300.0, 10.0, 1.3), (20.0, 300.0, 0.12)][:nlines]
    span = [600.0, 560.0, 520.0, 440.0, 580.0]
    seg = []
    for i in range(n):
        k = i % nlines
        x0, y0, ang = base[k]
        ln = rng.uniform(60.0, 120.0)
        t0 = rng.uniform(0.0, span[k] - ln)
        seg.append(_piece(x0, y0, ang + rng.uniform(-0.03, 0.03), t0, t0 + ln, rng.uniform(-3.0, 3.0)))
    return np.array(seg, np.float32)


def hubs():
    """Nine 300-px lines through one point, three directions 60 mrad apart times three offsets 5.2 px apart, so that no two of them
    pass the pair test, and 480 short pieces between them, each a neighbour of four of the nine.  The long lines open the first
    nine lists of the one raw cluster and each takes its 200 neighbours: 2418 list entries, more than the LDS list holds."""
    rng = np.random.default_rng(6)
    seg = [_piece(320.0, 240.0, a, -150.0, 150.0, o) for a in (-0.06, 0.0, 0.06) for o in (-5.2, 0.0, 5.2)]
    for i in range(480):
        a = (0.03 if i & 1 else -0.03) + rng.uniform(-0.005, 0.005)
        o = (2.6 if i & 2 else -2.6) + rng.uniform(-0.5, 0.5)
        tc, half = rng.uniform(-20.0, 20.0), rng.uniform(30.0, 40.0)
        seg.append(_piece(320.0, 240.0, a, tc - half, tc + half, o))
    return np.array(seg, np.float32)


def ties():
    """60 rows, 8 px apart, of horizontal 100-px segments end to end, two in the even rows and three in the odd ones: 150 equal
    angles, 150 equal lengths, raw clusters of exactly 2 and exactly 3 lines."""
    seg = []
    for r in range(60):
        y = 4.0 + 8.0 * r
        for k in range(2 + r % 2):
            seg.append([20.0 + 100.0 * k, y, 120.0 + 100.0 * k, y])
    return np.array(seg, np.float32)


CASES = {
    "n0": (lambda: tiny(0), 0), "n1": (lambda: tiny(1), 1), "n2": (lambda: tiny(2), 1), "n3": (lambda: tiny(3), 1),
    "separated300": (separated, 225),
    "one_line400": (lambda: collinear(400, 1, 1), 4),
    "five_lines400": (lambda: collinear(400, 5, 2), 15),
    "five_lines512": (lambda: collinear(512, 5, 3), 17),
    "five_lines513": (lambda: collinear(513, 5, 4), 16),
    "hubs489": (hubs, 4),
    "ties150": (ties, 60),
}


@pytest.fixture(scope="module")
def extractor():
    import psl_slam_amd as P
    return P.LINEextractor()


@pytest.mark.parametrize("name", list(CASES))
def test_merge_of_a_hand_made_list(name, extractor):
    import oracle_lib
    make, expect = CASES[name]
    seg = make()
    ref = oracle_lib.optimize_and_merge(seg, W, H, cap=4096)
    got = extractor.optimize_and_merge(seg, W, H, cap=4096)
    print(f"{name}: {len(seg)} segments -> {len(got)} keylines (oracle {len(ref)})")
    assert len(ref) == expect, f"{name}: the oracle returns {len(ref)} keylines, the case was made for {expect}"
    kl_equal(got, ref, name)
