"""Times the EPnP RANSAC (pslfe_pnp_solve / pslfe_pnp_solve_device) against the plain C++ loop of the same header
(tools/dropin/pnp_main.cpp built with -DPSL_PNP_HOST_ONLY, one core of the same machine; the JSON names the core).

  python tools/bench_pnp_solver.py [--out profiles/pnp_solver_bench.json] [--reps 5] [--label TEXT]

One candidate through the host form; K = 1, 1024 and 12288 candidates per launch through the device form, at 30 and 200 rows per
candidate, as one find() and as one iterate(5) on a fresh solver.  The reference's loop condition is an ||, so a first iterate(5) runs
on to mRansacMaxIts like find() unless a Refine succeeds first: the two differ little, and both are recorded.  The candidates are
those of tests/pnp_cases.py (make_rows: half of the rows agree with one pose, 0.3 px of noise; Relocalization's parameters 0.99, 10,
300, 4, 0.5, 5.991, a budget of 35); the K candidates of a launch cycle through 32 data sets and candidate k is seeded SEED0 + k, so
the first 32 candidates of a launch are the host loop's 32 and are compared with it: a result record or a flag that differs is counted
in "mismatches" and makes the tool exit 1.  Prints one JSON line and writes it to --out.  Launch times are host wall-clock around
launch + synchronise (best, median and largest of the repetitions after one warm-up).  Nothing is gated on these times."""
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


def _core():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_solver_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--candidates", type=int, nargs="*", default=[1, 1024, 12288])
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (PyTorch's HIP runtime first, as bench.py loads it)
    import psl_slam_amd as P
    import pnp_cases as pc
    ctx = P.default_context()
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in pc.CAM.items():
        cam[k] = v
    prm = pc.RELOC
    kw = dict(prob=prm["prob"], min_inliers=prm["min_inliers"], max_its=prm["max_its"], min_set=4, epsilon=prm["epsilon"], th2=prm["th2"])
    tmpdir = tempfile.TemporaryDirectory()
    tmp = tmpdir.name
    exe = os.path.join(tmp, "pnp_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_PNP_HOST_ONLY", "-o", exe, os.path.join(ROOT, "tools", "dropin", "pnp_main.cpp")],
                   check=True, capture_output=True)

    def down(d, a):
        P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
        return a

    res = {"tool": "bench_pnp_solver", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "reps": args.reps,
           "host_loop": "tools/dropin/pnp_main.cpp -DPSL_PNP_HOST_ONLY, g++ -O2, one core of " + _core(), "rows": []}
    if args.label:
        res["label"] = args.label
    mismatch = 0
    for nrows in (30, 200):
        data = [pc.make_rows(9000 + s, nrows, nrows // 2, noise_px=0.3)[0] for s in range(NSEEDS)]
        its = pc.ransac_parameters(nrows, prm["prob"], prm["min_inliers"], prm["max_its"], 4, prm["epsilon"])[0]
        cases = [dict(rows=r, cam=pc.CAM, seed=SEED0 + s, params=prm, find_its=its) for s, r in enumerate(data)]
        path, out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        pc.write_cases(path, cases, "find", P.CAMERA_DTYPE)
        p = subprocess.run([exe, path, out, str(max(args.reps, 2))], capture_output=True, text=True, check=True)
        loop_ms = json.loads(p.stdout.strip().splitlines()[-1])["loop_ms"] / NSEEDS
        with open(out, "rb") as f:
            loop = [calls[-1] for calls, _ in pc.read_section(f, cases)]
        best = None
        for _ in range(args.reps + 1):
            solver = P.PnPsolver(data[0], np.arange(nrows, dtype=np.int32), nrows, cam, SEED0, ctx=ctx)
            solver.SetRansacParameters(prm["prob"], prm["min_inliers"], prm["max_its"], 4, prm["epsilon"], prm["th2"])
            t0 = time.perf_counter()
            solver.find()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None or dt < best else best
        mismatch += int(not pc.same_result(solver.result, loop[0][0]) or (solver.row_inliers != loop[0][1]).any())
        row = {"rows": nrows, "budget": its, "host_loop_ms_per_candidate": round(loop_ms, 4), "host_form_ms": round(best, 4),
               "mean_iterations": round(float(np.mean([int(r["iterations"]) for r, _ in loop])), 2),
               "poses_returned": int(sum(int(r["status"]) & 1 for r, _ in loop)), "device": []}
        for K in args.candidates:
            R = np.zeros((K, nrows), P.PNPROW_DTYPE)
            for k in range(K):
                R[k] = data[k % NSEEDS]
            d_R, d_n = (ctx.device_array(a)[0] for a in (R, np.full(K, nrows, np.int32)))
            d_r, d_b, d_f = (ctx.device_array(a)[0] for a in (np.zeros(K, P.PNPRESULT_DTYPE), np.zeros((K, nrows), np.uint8), np.zeros((K, nrows), np.uint8)))
            entry = {"candidates": K}
            for what, nit in (("find", its), ("iterate5", 5)):
                times = []
                for _ in range(args.reps + 1):      # the first is the warm-up
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    P.PnPsolver.SolveDevice(K, d_R, d_n, nrows, cam, SEED0, nit, 0, d_b, d_r, d_f, ctx=ctx, **kw)
                    ctx.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
                times = sorted(times[1:]) or times
                entry[what] = {"launch_ms": round(times[0], 4), "ms_per_candidate": round(times[0] / K, 6),
                               "launch_ms_median": round(times[len(times) // 2], 4), "launch_ms_max": round(times[-1], 4)}
                if what == "find":
                    r, fl = down(d_r, np.zeros(K, P.PNPRESULT_DTYPE)), down(d_f, np.zeros((K, nrows), np.uint8))
                    for k in range(min(K, NSEEDS)):
                        mismatch += int(not pc.same_result(r[k], loop[k][0]) or (fl[k] != loop[k][1]).any())
            for d in (d_R, d_n, d_r, d_b, d_f):
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
