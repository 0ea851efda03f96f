"""Times the Sim3 optimisation (pslfe_sim3_optimize / pslfe_sim3_optimize_device) against the plain C++ host loop of the same
restatement (tools/dropin/sim3_main.cpp built with -DPSL_SIM3_HOST_ONLY, one core of the same machine).

  python tools/bench_sim3_opt.py [--out profiles/sim3_opt_bench.json] [--reps 5] [--label TEXT]

One candidate through the host form; K = 1, 1024 and 12288 candidates per launch through the device form, at 100 and 300 pairs per
candidate (seeded cases of tests/sim3_opt_cases.py: free scale, 30 % planted outliers, 0.5 px noise, start 2 degrees, 5 cm and 3 %
off; the K candidates of a launch cycle through 32 different seeds).  Every run is checked against the host loop: a flag or a
return value that differs is counted in "mismatches" and makes the tool exit 1.  Prints one JSON line and writes it to --out.
Needs the test tree: the cases come from tests/sim3_opt_cases.py, so that the tool and the tests optimise the same kind of
candidate.  Launch times are host wall-clock around launch + synchronise (best, median and largest of the repetitions after one
warm-up)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_opt_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--candidates", type=int, nargs="*", default=[1, 1024, 12288])
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (PyTorch's HIP runtime first, as bench.py loads it)
    import psl_slam_amd as P
    import sim3_opt_cases as sc
    ctx = P.default_context()
    cams = []
    for cam in sc.cameras():
        rec = np.zeros((), P.CAMERA_DTYPE)
        for k, v in cam.items():
            rec[k] = v
        cams.append(rec)
    tmpdir = tempfile.TemporaryDirectory()
    tmp = tmpdir.name
    exe = os.path.join(tmp, "sim3_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_SIM3_HOST_ONLY", "-o", exe,
                    os.path.join(ROOT, "tools", "dropin", "sim3_main.cpp")], check=True, capture_output=True)

    def down(d, a):
        P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
        return a

    res = {"tool": "bench_sim3_opt", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "reps": args.reps,
           "host_loop": "tools/dropin/sim3_main.cpp -DPSL_SIM3_HOST_ONLY, g++ -O2, one core", "rows": []}
    if args.label:
        res["label"] = args.label
    mismatch = 0
    for npairs in (100, 300):
        cases = [sc.make_case(9000 + s, npairs, 0.3, False) for s in range(NSEEDS)]
        path, out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        with open(path, "wb") as f:
            np.array([NSEEDS, npairs, 0], np.int32).tofile(f)
            np.array([sc.TH2], np.float32).tofile(f)
            cams[0].tofile(f)
            cams[1].tofile(f)
            for c in cases:
                c["S12"].tofile(f)
                np.array([npairs], np.int32).tofile(f)
                c["pairs"].tofile(f)
        p = subprocess.run([exe, path, out, str(args.reps)], capture_output=True, text=True, check=True)
        loop_ms = json.loads(p.stdout.strip().splitlines()[-1])["loop_ms"] / NSEEDS
        loop = []
        with open(out, "rb") as f:
            for c in cases:
                np.fromfile(f, sc.SIM3D_DTYPE, 1)
                nin = int(np.fromfile(f, np.int32, 1)[0])
                np.fromfile(f, sc.INFO_DTYPE, 1)
                loop.append((nin, np.fromfile(f, np.uint8, npairs)))
        best = None
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            nin, _, bad = P.Optimizer.OptimizeSim3(cases[0]["S12"], cases[0]["pairs"], cams[0], cams[1], sc.TH2, False, ctx=ctx)
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None or dt < best else best
        mismatch += int(nin != loop[0][0] or (bad != loop[0][1]).any())
        row = {"pairs": npairs, "host_loop_ms_per_candidate": round(loop_ms, 4), "host_form_ms": round(best, 4), "device": []}
        for K in args.candidates:
            S = np.zeros(K, P.SIM3_DTYPE)
            Pr = np.zeros((K, npairs), P.SIM3PAIR_DTYPE)
            for k in range(K):
                S[k], Pr[k] = cases[k % NSEEDS]["S12"], cases[k % NSEEDS]["pairs"]
            d_S, d_P, d_n = (ctx.device_array(a)[0] for a in (S, Pr, np.full(K, npairs, np.int32)))
            d_o, d_b, d_g = (ctx.device_array(a)[0] for a in (np.zeros(K, P.SIM3D_DTYPE), np.zeros((K, npairs), np.uint8), np.zeros(K, np.int32)))
            times = []
            for _ in range(args.reps + 1):      # the first is the warm-up
                ctx.synchronize()
                t0 = time.perf_counter()
                P.Optimizer.OptimizeSim3Device(K, d_S, d_P, d_n, npairs, cams[0], cams[1], sc.TH2, False, d_o, d_b, d_g, ctx=ctx)
                ctx.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            times = sorted(times[1:]) or times
            g, o = down(d_g, np.zeros(K, np.int32)), down(d_b, np.zeros((K, npairs), np.uint8))
            for k in range(K):
                mismatch += int(g[k] != loop[k % NSEEDS][0] or (o[k] != loop[k % NSEEDS][1]).any())
            for d in (d_S, d_P, d_n, d_o, d_b, d_g):
                ctx.device_free(d)
            row["device"].append({"candidates": K, "launch_ms": round(times[0], 4), "ms_per_candidate": round(times[0] / K, 6),
                                  "launch_ms_median": round(times[len(times) // 2], 4), "launch_ms_max": round(times[-1], 4)})
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
