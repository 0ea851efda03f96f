"""Times the Sim3 RANSAC (pslfe_sim3_solve / pslfe_sim3_solve_device) against the plain C++ loop of the same header
(tools/dropin/sim3_solver_main.cpp built with -DPSL_SIM3_SOLVER_HOST_ONLY, one core of the same machine).

  python tools/bench_sim3_solver.py [--out profiles/sim3_solver_bench.json] [--reps 5] [--label TEXT]

One candidate through the host form; K = 1, 1024 and 12288 candidates per launch through the device form, at 100 and 300 pairs per
candidate, as one find() (up to 300 iterations) and as one round of iterate(5).  The candidates are those of
tests/sim3_solver_cases.py (make_pairs: 40 % of the pairs agree with one Sim3, the others do not; LoopClosing's parameters 0.99, 20,
300); the K candidates of a launch cycle through 32 data sets and candidate k is seeded SEED0 + k, so the first 32 candidates of a
launch are the host loop's 32 and are compared with it: a status, an iteration count, an inlier count or a flag that differs is
counted in "mismatches" and makes the tool exit 1.  Prints one JSON line and writes it to --out.  Launch times are host wall-clock
around launch + synchronise (best, median and largest of the repetitions after one warm-up)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NSEEDS = 32
SEED0 = 7000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_solver_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--candidates", type=int, nargs="*", default=[1, 1024, 12288])
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (PyTorch's HIP runtime first, as bench.py loads it)
    import psl_slam_amd as P
    import sim3_solver_cases as sc
    ctx = P.default_context()
    cams = []
    for cam in sc.cameras():
        rec = np.zeros((), P.CAMERA_DTYPE)
        for k, v in cam.items():
            rec[k] = v
        cams.append(rec)
    tmpdir = tempfile.TemporaryDirectory()
    tmp = tmpdir.name
    exe = os.path.join(tmp, "sim3_solver_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_SIM3_SOLVER_HOST_ONLY", "-o", exe,
                    os.path.join(ROOT, "tools", "dropin", "sim3_solver_main.cpp")], check=True, capture_output=True)

    def down(d, a):
        P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
        return a

    res = {"tool": "bench_sim3_solver", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "reps": args.reps,
           "host_loop": "tools/dropin/sim3_solver_main.cpp -DPSL_SIM3_SOLVER_HOST_ONLY, g++ -O2, one core", "rows": []}
    if args.label:
        res["label"] = args.label
    mismatch = 0
    for npairs in (100, 300):
        data = [sc.make_pairs(9000 + s, npairs, int(0.4 * npairs), False)[:2] for s in range(NSEEDS)]
        path, out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        with open(path, "wb") as f:
            np.array([NSEEDS, npairs, 0, sc.MIN_INLIERS, sc.MAX_ITS, sc.MAX_ITS], np.int32).tofile(f)
            np.array([sc.PROB], np.float64).tofile(f)
            cams[0].tofile(f)
            cams[1].tofile(f)
            for s, (pr, sg) in enumerate(data):
                np.array([SEED0 + s], np.uint32).tofile(f)
                np.array([npairs], np.int32).tofile(f)
                pr.tofile(f)
                np.ascontiguousarray(sg, np.float32).tofile(f)
        p = subprocess.run([exe, path, out, str(max(args.reps, 2))], capture_output=True, text=True, check=True)
        loop_ms = json.loads(p.stdout.strip().splitlines()[-1])["loop_ms"] / NSEEDS
        loop = []
        with open(out, "rb") as f:
            for _ in range(NSEEDS):
                r = np.fromfile(f, sc.RESULT_DTYPE, 1)[0]
                fl = np.fromfile(f, np.uint8, npairs)
                nt = int(np.fromfile(f, np.int32, 1)[0])
                np.fromfile(f, sc.TRACE_DTYPE, nt)
                loop.append((r, fl))
        solver = P.Sim3Solver(data[0][0], data[0][1], np.arange(npairs, dtype=np.int32), npairs, cams[0], cams[1], False, SEED0, ctx=ctx)
        best = None
        for _ in range(args.reps + 1):
            solver.SetRansacParameters(sc.PROB, sc.MIN_INLIERS, sc.MAX_ITS)
            solver._best_inliers = 0
            t0 = time.perf_counter()
            solver.find()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None or dt < best else best
        mismatch += int(solver.result.tobytes() != loop[0][0].tobytes() or (solver.row_inliers != loop[0][1]).any())
        row = {"pairs": npairs, "host_loop_ms_per_candidate": round(loop_ms, 4), "host_form_ms": round(best, 4),
               "mean_iterations": round(float(np.mean([int(r["iterations"]) for r, _ in loop])), 2), "device": []}
        for K in args.candidates:
            Pr, Sg = np.zeros((K, npairs), P.SIM3PAIR_DTYPE), np.zeros((K, npairs, 2), np.float32)
            for k in range(K):
                Pr[k], Sg[k] = data[k % NSEEDS]
            d_P, d_S, d_n = (ctx.device_array(a)[0] for a in (Pr, Sg, np.full(K, npairs, np.int32)))
            d_r, d_f = (ctx.device_array(a)[0] for a in (np.zeros(K, P.SIM3SOLVERRESULT_DTYPE), np.zeros((K, npairs), np.uint8)))
            entry = {"candidates": K}
            for what, nit in (("find", sc.MAX_ITS), ("iterate5", 5)):
                times = []
                for _ in range(args.reps + 1):      # the first is the warm-up
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    P.Sim3Solver.SolveDevice(K, d_P, d_S, d_n, npairs, cams[0], cams[1], False, SEED0, nit, d_r, d_f, ctx=ctx)
                    ctx.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
                times = sorted(times[1:]) or times
                entry[what] = {"launch_ms": round(times[0], 4), "ms_per_candidate": round(times[0] / K, 6),
                               "launch_ms_median": round(times[len(times) // 2], 4), "launch_ms_max": round(times[-1], 4)}
                if what == "find":
                    r, fl = down(d_r, np.zeros(K, P.SIM3SOLVERRESULT_DTYPE)), down(d_f, np.zeros((K, npairs), np.uint8))
                    for k in range(min(K, NSEEDS)):
                        mismatch += int(r[k].tobytes() != loop[k][0].tobytes() or (fl[k] != loop[k][1]).any())
            for d in (d_P, d_S, d_n, d_r, d_f):
                ctx.device_free(d)
            row["device"].append(entry)
        res["rows"].append(row)
    res["mismatches"] = mismatch
    tmpdir.cleanup()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 1 if mismatch else 0


if __name__ == "__main__":
    sys.exit(main())
