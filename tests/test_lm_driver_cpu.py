"""The Levenberg driver psl_lm_levenberg of psl-slam_amd/csrc/lm_kernels.h at its rarely taken exits, on scripted problems of six
unknowns: sums() returns a fixed H, b and chi2, chi() the next value of a list, candidate() records the step it is handed and
accept() counts its calls.  tests/lm_driver_host.cpp runs psl_lm_optimize<6> on the scripts as a stand-alone program under the address
and undefined-behaviour sanitizers; lm_cases.levenberg runs the same scripts in numpy.  The iterations run, the accept calls and
every step handed to candidate are compared bit for bit (lambda enters every step, so the steps pin lambda too).  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import lm_cases as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NH = 6, 21
INF, NAN = math.inf, math.nan
B = (-0.3, 0.2, -0.1, 0.4, -0.5, 0.6)        # b before the sign


def sums(chi2, diag=(2.0,) * 6, b=B):
    """acc of sums(): H (diag on the diagonal, 0.1 elsewhere; upper triangle row by row), b before the sign, chi2"""
    H = [diag[j] if j == k else 0.1 for j in range(N) for k in range(j, N)]
    return np.array(H + list(b) + [chi2])


NEG = (2.0, 2.0, 2.0, -3.0, 2.0, 2.0)        # not positive definite until lambda passes 3: lambda_init = 3e-5, so six trials fail
HUGE = (-1e9,) + B[1:]                       # x[0] = 1e9 / (2 + lambda) leaves THETA_MAX = 1.05e8 once lambda passes 7.5: six trials

# name: (iterations allowed, the acc of every sums() call, the value of every chi() call, (iterations run, accepts, candidates))
SCRIPTS = {
    # every iteration is accepted but gains 0.1 of 1000: _nBad ends the call at its third iteration
    "nbad": (10, [sums(1000.0), sums(999.9), sums(999.8)], [999.9, 999.8, 999.7], (3, 3, 3)),
    # ten rejected trials: Terminate after one iteration
    "ten_trials": (10, [sums(1000.0)], [2000.0] * 10, (1, 0, 10)),
    # rho == 0: not accepted, the trial loop ends, Terminate
    "rho_zero": (10, [sums(1000.0)], [1000.0], (1, 0, 1)),
    # the solve fails six times, then a candidate is formed and accepted; the next iteration solves at once
    "failed_solve": (2, [sums(1000.0, NEG), sums(900.0, NEG)], [900.0, 800.0], (2, 2, 2)),
    # a NaN chi2: rejected, the trial loop ends, no Terminate; the next iteration runs at twice the lambda
    "nan_chi": (2, [sums(1000.0), sums(1000.0)], [NAN, 900.0], (2, 1, 2)),
    # +inf: rejected, lambda grows, the next trial is accepted
    "inf_chi": (1, [sums(1000.0)], [INF, 900.0], (1, 1, 2)),
    # the angle guard refuses six steps as failed solves (no candidate), the seventh is formed
    "refused_angle": (1, [sums(1000.0, b=HUGE)], [900.0], (1, 1, 1)),
    # chi2 = +inf at the estimate and a failed solve: rho = +inf > 0 with no candidate - lambda shrinks to a third, accept is not
    # called; the next iteration (a definite H) forms its candidate at that lambda
    "inf_estimate": (2, [sums(INF, NEG), sums(1000.0)], [900.0], (2, 1, 1)),
}


class Scripted:
    n = N

    def __init__(self, script):
        self.sums_list, self.chi_list = list(script[1]), list(script[2])
        self.sums_at = self.chi_at = self.accepts = 0
        self.xs = []

    def sums(self):
        self.sums_at += 1
        return self.sums_list[self.sums_at - 1]

    def candidate(self, x):
        self.xs.append([float(v) for v in x])

    def chi(self):
        self.chi_at += 1
        return self.chi_list[self.chi_at - 1]

    def accept(self):
        self.accepts += 1


@pytest.fixture(scope="module")
def witness():
    """name -> (iterations run, the Scripted problem after lm_cases.levenberg)"""
    out = {}
    for name, script in SCRIPTS.items():
        P = Scripted(script)
        out[name] = (lm.levenberg(P, script[0]), P)
    return out


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_script_takes_the_exit_it_is_written_for(witness, name):
    """the restatement consumes exactly what the script lists and runs the iterations, accepts and candidates worked out above"""
    its, P = witness[name]
    script = SCRIPTS[name]
    assert (its, P.accepts, len(P.xs)) == script[3]
    assert P.sums_at == len(script[1]) and P.chi_at == len(script[2])


def test_lambda_of_the_steps_after_a_rare_branch(witness):
    """the step handed over after the branch is the solve at the lambda the branch must leave, from lambda_init = 1e-5 max |H_jj|"""
    b = [-v for v in B]
    grown = lambda lam, k: lam * 2.0 ** (k * (k + 1) // 2)       # k rejected trials in a row: * 2, * 4, * 8, ...
    xs = witness["nan_chi"][1].xs
    assert xs[0] == lm.solve(N, sums(0.0), 1e-5 * 2.0, b) and xs[1] == lm.solve(N, sums(0.0), grown(1e-5 * 2.0, 1), b)
    xs = witness["inf_chi"][1].xs
    assert xs[1] == lm.solve(N, sums(0.0), grown(1e-5 * 2.0, 1), b)
    xs = witness["ten_trials"][1].xs
    assert all(xs[k] == lm.solve(N, sums(0.0), grown(1e-5 * 2.0, k), b) for k in range(10))
    xs = witness["failed_solve"][1].xs
    assert lm.solve(N, sums(0.0, NEG), grown(1e-5 * 3.0, 5), b) is None and xs[0] == lm.solve(N, sums(0.0, NEG), grown(1e-5 * 3.0, 6), b)
    xs = witness["refused_angle"][1].xs
    hb = [-v for v in HUGE]
    assert abs(lm.solve(N, sums(0.0), grown(1e-5 * 2.0, 5), hb)[0]) > lm.THETA_MAX
    assert xs[0] == lm.solve(N, sums(0.0), grown(1e-5 * 2.0, 6), hb) and abs(xs[0][0]) < lm.THETA_MAX
    xs = witness["inf_estimate"][1].xs
    assert xs[0] == lm.solve(N, sums(0.0), (1e-5 * 3.0) * (1.0 / 3.0), b)


def test_driver_under_sanitizers_equals_restatement(witness, tmp_path):
    """psl_lm_optimize<6>, an instance of psl_lm_levenberg, on every script: the iterations run, the accept calls and the bits of
    every step handed to candidate equal lm_cases.levenberg's, and the sanitizers stay silent"""
    exe, path, out = str(tmp_path / "lm_driver_host"), str(tmp_path / "scripts.bin"), str(tmp_path / "out.bin")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "lm_driver_host.cpp")], check=True, capture_output=True)
    with open(path, "wb") as f:
        np.array([len(SCRIPTS)], np.int32).tofile(f)
        for iterations, sums_list, chi_list, _ in SCRIPTS.values():
            np.array([iterations, len(sums_list), len(chi_list)], np.int32).tofile(f)
            np.array(sums_list, np.float64).tofile(f)
            np.array(chi_list, np.float64).tofile(f)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    with open(out, "rb") as f:
        for name in SCRIPTS:
            ref_its, P = witness[name]
            its, accepts, ncand, sums_at, chi_at = (int(v) for v in np.fromfile(f, np.int32, 5))
            xs = np.fromfile(f, np.float64, N * ncand)
            assert (its, accepts, ncand) == (ref_its, P.accepts, len(P.xs)), name
            assert (sums_at, chi_at) == (P.sums_at, P.chi_at), name
            assert xs.tobytes() == np.array(P.xs, np.float64).tobytes(), (name, xs, P.xs)
        assert f.read() == b""
