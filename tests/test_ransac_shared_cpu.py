"""psl-slam_amd/csrc/ransac_kernels.h alone: tests/ransac_host.cpp includes nothing else of the library, is built with g++ under the
address and undefined-behaviour sanitizers and run as a child process.  Bit for bit:
  psl_rs_draw<3>, <4>, <8>       against the swap-and-pop with the vector written out (sim3_solver_cases.draw)
  psl_rs_jacobi_svd<float, 1>    against initializer_cases.jacobi at the Initializer's shapes
  psl_rs_jacobi_svd<double, 1>   against pnp_cases.jacobi_sweeps (jacobi_rows before its normalisation) at PnP's shapes
  ES = 4                         the first of four interleaved workspaces against the same matrix at ES = 1
The two numpy restatements are independent readings; they are what pins the two instantiations of the one template.  The Initializer
runs the float one.  PnP runs its own psl_pnp_jacobi (the same sweeps on offsets into its workspace: pnp_solver_kernels.h says why),
which tests/test_pnp_solver_cpu.py holds to the same pnp_cases.jacobi_rows, so the double instantiation and PnP's copy cannot drift
apart unnoticed.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import initializer_cases as ic
import pnp_cases as pc
import sim3_solver_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
EPS = {"f": float(F(2) * F(np.finfo(F).eps)), "d": 10 * float(np.finfo(D).eps)}   # 2 * FLT_EPSILON, 10 * DBL_EPSILON
SEEDS = (0, 1, 2, 1234567, 0x80000001)
# (rows n of At, their length m, with Vt)
SHAPES_F = ((9, 16, 1), (8, 9, 0), (3, 3, 1), (4, 4, 1))                              # ComputeH21, ComputeF21, the 3x3s, Triangulate
SHAPES_D = ((12, 12, 0), (3, 3, 1), (3, 3, 0), (3, 6, 1), (4, 6, 1), (5, 6, 1))       # M^T M, the 3x3s, cvSolve of 6 x n
KINDS = ("random", "tie", "zero_row", "orthogonal")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ransac") / "ransac_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "ransac_host.cpp")], check=True, capture_output=True)
    return exe


def _run(host_exe, tmp_path, lines):
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    p = subprocess.run([host_exe, path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    return [[int(w, 16) for w in ln.split()] for ln in p.stdout.splitlines()]


def _bits(a):
    a = np.ascontiguousarray(a)
    return [int(v) for v in a.reshape(-1).view(np.uint32 if a.dtype == F else np.uint64)]


def _hex(a):
    return " ".join("%x" % v for v in _bits(a))


def matrix(kind, n, m, dtype, seed):
    """n rows of length m (n <= m).  tie: rows 0 and n - 1 are 5 e0 and 5 e1, the others small and in the other columns, so two singular
    values are exactly equal and the one of row 0 has to stay first; zero_row: row 1 is exactly zero; orthogonal: signed multiples of
    distinct unit vectors in no order, so that no pair rotates and the first sweep is the last"""
    rng = np.random.default_rng(1000 * n + 10 * m + seed)
    A = rng.standard_normal((n, m))
    if kind == "tie":
        A[:, :2] = 0
        A[1:n - 1] *= 0.25
        A[0], A[n - 1] = 0, 0
        A[0, 0], A[n - 1, 1] = 5, 5
    elif kind == "zero_row":
        A[1] = 0
    elif kind == "orthogonal":
        A[:] = 0
        cols, scale = rng.permutation(m)[:n], rng.permutation(n) + 1.0
        for i in range(n):
            A[i, cols[i]] = scale[i] * (-1) ** i
    return A.astype(dtype)


def ref_float(A, want_v):
    a = A.astype(F)[:, :, None].copy()
    W, V = ic.jacobi(a, bool(want_v))
    return _bits(a[:, :, 0]) + _bits(W[:, 0]) + (_bits(V[:, :, 0]) if want_v else [])


def ref_double(A, want_v):
    At = [[float(v) for v in row] for row in A]
    W, Vt = pc.jacobi_sweeps(At, bool(want_v))
    return _bits(np.array(At, D)) + _bits(np.array(W, D)) + (_bits(np.array(Vt, D)) if want_v else [])


def _svd_case(t, es, A, want_v, others=()):
    n, m = A.shape
    eps = "%x" % struct.unpack("<Q", struct.pack("<d", EPS[t]))[0]
    return ["svd %s %d %d %d %d %s" % (t, es, m, n, want_v, eps)] + [_hex(M) for M in (A,) + tuple(others)]


@pytest.mark.parametrize("K", [3, 4, 8])
def test_draw_equals_the_written_out_swap_and_pop(host_exe, tmp_path, K):
    """N = K draws every index and hits every override slot; 25 draws per stream; seed 0 is seeded as 1"""
    its = 25
    cases = [(N, seed) for N in (K, K + 1, K + 2, 300) for seed in SEEDS]
    got = _run(host_exe, tmp_path, ["draw %d %d %d %d" % (K, N, seed, its) for N, seed in cases])
    assert len(got) == len(cases)
    for (N, seed), g in zip(cases, got):
        G = sc.GlibcRand(seed)
        want = [i for _ in range(its) for i in sc.draw(G, N, K)]
        assert g == want, (K, N, seed)
        if N == K:
            assert all(sorted(g[K * i:K * i + K]) == list(range(K)) for i in range(its))
    by = dict(zip(cases, got))
    assert all(by[(N, 0)] == by[(N, 1)] and by[(N, 1)] != by[(N, 2)] for N in (K + 1, 300))


@pytest.mark.parametrize("t,shapes,ref", [("f", SHAPES_F, ref_float), ("d", SHAPES_D, ref_double)], ids=["float", "double"])
def test_jacobi_svd_equals_the_numpy_reading(host_exe, tmp_path, t, shapes, ref):
    """a, W and Vt of every edge matrix at every shape its consumer uses"""
    dtype = F if t == "f" else D
    cases = [(kind, n, m, v, matrix(kind, n, m, dtype, 0)) for n, m, v in shapes for kind in KINDS]
    lines = [ln for _, _, _, v, A in cases for ln in _svd_case(t, 1, A, v)]
    got = _run(host_exe, tmp_path, lines)
    assert len(got) == len(cases)
    for (kind, n, m, v, A), g in zip(cases, got):
        assert g == ref(A, v), (t, kind, n, m, v)
        w = np.array(g[n * m:n * m + n], np.uint64).view(D)
        assert (np.diff(w) <= 0).all(), (kind, n, m)
        if kind == "tie":       # the two equal values lead, and row 0 (5 e0) stayed in front of row n - 1 (5 e1)
            rows = np.array(g[:n * m], np.uint32 if t == "f" else np.uint64).view(dtype).reshape(n, m)
            assert w[0] == w[1] == 5 and rows[0, 0] == 5 and rows[1, 1] == 5, (n, m)
        if kind == "zero_row":
            assert w[-1] == 0 and w[-2] > 0, (n, m)
        if kind == "orthogonal":   # nothing rotated: the rows are those of the input, sorted
            assert sorted(g[:n * m]) == sorted(_bits(A)) and list(w) == list(range(n, 0, -1)), (n, m)


@pytest.mark.parametrize("t,n,m", [("f", 9, 16), ("d", 4, 6)], ids=["float", "double"])
def test_interleaved_workspaces_are_addressed_by_their_stride(host_exe, tmp_path, t, n, m):
    """ES = 4: the first workspace gives what the same matrix gives at ES = 1, while the three others hold other matrices"""
    dtype = F if t == "f" else D
    A = matrix("random", n, m, dtype, 0)
    others = (matrix("random", n, m, dtype, 1), matrix("tie", n, m, dtype, 2), matrix("zero_row", n, m, dtype, 3))
    one, four = _run(host_exe, tmp_path, _svd_case(t, 1, A, 1) + _svd_case(t, 4, A, 1, others))
    assert four == one and one == (ref_float if t == "f" else ref_double)(A, 1)
