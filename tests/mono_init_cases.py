"""Frame pairs for the monocular initialiser's matcher: random keypoint sets and constructed edge cases with descriptors at controlled
Hamming distances.  Shared by tests/test_mono_init_cpu.py, tests/test_mono_init_gpu.py and tools/bench_mono_init.py."""
import numpy as np

from oracle_lib import KEYPOINT_DTYPE

F32 = np.float32
BOUNDS = (0.0, 0.0, 640.0, 480.0)


class Case:
    """F1 / F2 keypoints and descriptors built up piece by piece."""

    def __init__(self):
        self.k1, self.d1, self.k2, self.d2, self.prev = [], [], [], [], []

    @staticmethod
    def _kp(x, y, angle, octave):
        k = np.zeros((), KEYPOINT_DTYPE)
        k["x"], k["y"], k["angle"], k["octave"], k["size"] = x, y, angle, octave, 31.0
        return k

    def f2(self, x, y, desc, angle=0.0, octave=0):
        self.k2.append(self._kp(x, y, angle, octave))
        self.d2.append(np.asarray(desc, np.uint8))
        return len(self.k2) - 1

    def f1(self, x, y, desc, angle=0.0, octave=0, prev=None):
        self.k1.append(self._kp(x, y, angle, octave))
        self.d1.append(np.asarray(desc, np.uint8))
        self.prev.append((x, y) if prev is None else prev)
        return len(self.k1) - 1

    def arrays(self):
        k1 = np.array(self.k1, KEYPOINT_DTYPE) if self.k1 else np.zeros(0, KEYPOINT_DTYPE)
        k2 = np.array(self.k2, KEYPOINT_DTYPE) if self.k2 else np.zeros(0, KEYPOINT_DTYPE)
        d1 = np.array(self.d1, np.uint8).reshape(-1, 32)
        d2 = np.array(self.d2, np.uint8).reshape(-1, 32)
        prev = np.array(self.prev, F32).reshape(-1, 2)
        return k1, d1, k2, d2, prev


def random_desc(rng):
    return rng.integers(0, 256, 32, dtype=np.uint8)


def flip(desc, rng, k):
    """desc with k distinct bits flipped."""
    b = np.unpackbits(desc)
    b[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(b)


def constructed(c, rng):
    """The edge cases of the matcher on one frame pair (window 20): returns the ids the assertions need."""
    ids = {}
    # steal chain: three queries compete for one F2 keypoint with distances 40, 30, 20; each takes it from the one before
    base = random_desc(rng)
    k = c.f2(100, 100, base)
    ids["chain"] = (k, [c.f1(101, 100, flip(base, rng, d)) for d in (40, 30, 20)])
    # tie: two F2 keypoints at the same distance; the first in visiting order (lower grid column) has the higher index
    base = random_desc(rng)
    right = c.f2(312, 100, base)
    left = c.f2(288, 100, base)
    ids["tie"] = (c.f1(300, 100, flip(base, rng, 10)), left, right)
    # the filter removes the best and changes the second best: an earlier query holds X at 10; the later query sees X at 12
    # (filtered), Y at 20, Z at 22
    base = random_desc(rng)
    X = c.f2(500, 100, base)
    c.f1(500, 100, flip(base, rng, 10))
    qd = flip(base, rng, 12)
    Y = c.f2(505, 100, flip(qd, rng, 20))
    Z = c.f2(495, 100, flip(qd, rng, 22))
    ids["filt"] = (c.f1(501, 101, qd), X, Y, Z)
    # a single survivor: bestDist2 stays INT_MAX
    base = random_desc(rng)
    k = c.f2(100, 300, base)
    ids["single"] = (c.f1(100, 300, flip(base, rng, 45)), k)
    # octave > 0: the query is skipped, and an F2 keypoint of octave 2 is no candidate
    base = random_desc(rng)
    k = c.f2(300, 300, base)
    q = c.f1(300, 300, base, octave=1)
    k_hi = c.f2(303, 300, base, octave=2)
    ids["skip"] = (q, c.f1(303, 300, flip(base, rng, 60)), k, k_hi)
    # prev outside the grid: an empty window
    base = random_desc(rng)
    c.f2(500, 300, base)
    ids["out"] = c.f1(500, 300, flip(base, rng, 5), prev=(-500.0, 2000.0))
    return ids


def stolen_decides(c, rng):
    """24 plain matches in bin 0; a query A matched in bin 6, later taken over by B (bin 0); two more matches C, D in bin 6.
    Bin 6 holds 3 entries against 25 in bin 0 (3 >= 2.5): C and D survive only because A's entry still counts.  Window 10."""
    for j in range(24):
        base = random_desc(rng)
        c.f2(20 + 25 * j, 400, base, angle=100.0)
        c.f1(20 + 25 * j, 400, flip(base, rng, 5), angle=100.0)
    base = random_desc(rng)
    kA = c.f2(100, 100, base, angle=10.0)
    A = c.f1(100, 100, flip(base, rng, 30), angle=190.0)      # rot 180 -> bin 6
    CD = []
    for j in range(2):
        b = random_desc(rng)
        c.f2(300 + 40 * j, 200, b, angle=20.0)
        CD.append(c.f1(300 + 40 * j, 200, flip(b, rng, 8), angle=200.0))
    B = c.f1(101, 100, flip(base, rng, 10), angle=10.0)       # bin 0, takes kA
    return A, B, kA, CD


def one_tenth(c, rng):
    """max2 == max3 == 0.1 * max1 exactly (0.1f * 10.0f rounds to 1.0f): both bins are kept, a fourth is cleared.  Window 10."""
    for j in range(10):
        b = random_desc(rng)
        c.f2(20 + 25 * j, 50, b)
        c.f1(20 + 25 * j, 50, flip(b, rng, 5))
    out = []
    for j, rot in enumerate((150.0, 240.0, 300.0)):
        b = random_desc(rng)
        c.f2(100 + 60 * j, 300, b)
        out.append(c.f1(100 + 60 * j, 300, flip(b, rng, 5), angle=rot))
    return out


def random_pair(rng, n1, n2, w=640, h=480, p0=0.5):
    k2 = np.zeros(n2, KEYPOINT_DTYPE)
    k2["x"], k2["y"] = rng.uniform(-5, w + 5, n2), rng.uniform(-5, h + 5, n2)
    k2["octave"] = np.where(rng.random(n2) < p0, 0, rng.integers(1, 8, n2))
    k2["angle"] = rng.uniform(0, 360, n2)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    k1 = np.zeros(n1, KEYPOINT_DTYPE)
    if n2:
        src = rng.integers(0, n2, n1)
        k1["x"] = k2["x"][src] + rng.normal(0, 30, n1)
        k1["y"] = k2["y"][src] + rng.normal(0, 30, n1)
        k1["angle"] = np.mod(k2["angle"][src] + np.where(rng.random(n1) < 0.7, rng.normal(0, 5, n1), rng.uniform(0, 360, n1)), 360)
        d1 = np.stack([flip(d2[s], rng, int(rng.integers(0, 70))) for s in src]) if n1 else np.zeros((0, 32), np.uint8)
    else:
        d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    k1["octave"] = np.where(rng.random(n1) < 0.6, 0, rng.integers(1, 8, n1))
    prev = np.stack([k1["x"], k1["y"]], 1).astype(F32)
    return k1, d1, k2, d2, prev
