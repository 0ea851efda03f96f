"""Times the pose optimisation (pslfe_pose_optimize / pslfe_pose_optimize_device) against the plain C++ host loop of the same
restatement (tools/dropin/pose_main.cpp built with -DPSL_POSE_HOST_ONLY, one core of the same machine).

  python tools/bench_pose_opt.py [--out profiles/pose_opt_bench.json] [--reps 5]

One frame through the host form; K = 1, 32, 1024 and 12288 frames per launch through the device form, at 300 and 1000 edges per
frame (seeded cases of tests/pose_opt_cases.py: mixed edges, 30 % planted outliers, 0.5 px noise, start 2 degrees and 5 cm off; the
K frames of a launch cycle through 32 different seeds).  Exits 1 if the device form and the host loop differ in any flag or return
value.  Prints one JSON line and writes it to --out.  Needs the test tree: the cases come from tests/pose_opt_cases.py, so that the
tool and the tests optimise the same kind of frame."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_opt_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 32, 1024, 12288])
    args = ap.parse_args()
    import torch  # noqa: F401  (PyTorch's HIP runtime first, as bench.py loads it)
    import psl_slam_amd as P
    import pose_opt_cases as pc
    ctx = P.default_context()
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in pc.camera().items():
        cam[k] = v
    tmpdir = tempfile.TemporaryDirectory()
    tmp = tmpdir.name
    exe = os.path.join(tmp, "pose_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_POSE_HOST_ONLY", "-o", exe,
                    os.path.join(ROOT, "tools", "dropin", "pose_main.cpp")], check=True, capture_output=True)

    def down(d, a):
        P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
        return a

    res = {"tool": "bench_pose_opt", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "reps": args.reps,
           "host_loop": "tools/dropin/pose_main.cpp -DPSL_POSE_HOST_ONLY, g++ -O2, one core", "rows": []}
    mismatch = 0
    for nedges in (300, 1000):
        cases = [pc.make_case(7000 + s, nedges, "mixed", 0.3) for s in range(NSEEDS)]
        # the host loop on one core: the 32 frames, best of reps
        path, out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        with open(path, "wb") as f:
            np.array([NSEEDS, nedges], np.int32).tofile(f)
            cam.tofile(f)
            for c in cases:
                c["Tcw"].tofile(f)
                np.array([nedges], np.int32).tofile(f)
                c["edges"].tofile(f)
        p = subprocess.run([exe, path, out, str(args.reps)], capture_output=True, text=True, check=True)
        loop_ms = json.loads(p.stdout.strip().splitlines()[-1])["loop_ms"] / NSEEDS
        loop = []
        with open(out, "rb") as f:
            for c in cases:
                np.fromfile(f, pc.POSE_DTYPE, 1)
                ng = int(np.fromfile(f, np.int32, 1)[0])
                np.fromfile(f, pc.INFO_DTYPE, 1)
                loop.append((ng, np.fromfile(f, np.uint8, nedges)))
        # one frame through the host form
        best = None
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            ng, _, outl = P.Optimizer.PoseOptimization(cases[0]["Tcw"], cases[0]["edges"], cam, ctx=ctx)
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None or dt < best else best
        mismatch += int(ng != loop[0][0] or (outl != loop[0][1]).any())
        row = {"edges": nedges, "host_loop_ms_per_frame": round(loop_ms, 4), "host_form_ms": round(best, 4), "device": []}
        for K in args.frames:
            T = np.zeros(K, P.POSE_DTYPE)
            E = np.zeros((K, nedges), P.POSEEDGE_DTYPE)
            for k in range(K):
                T[k], E[k] = cases[k % NSEEDS]["Tcw"], cases[k % NSEEDS]["edges"]
            n = np.full(K, nedges, np.int32)
            d_T, d_E, d_n = (ctx.device_array(a)[0] for a in (T, E, n))
            d_To, d_o, d_g = (ctx.device_array(a)[0] for a in (np.zeros(K, P.POSE_DTYPE), np.zeros((K, nedges), np.uint8), np.zeros(K, np.int32)))
            best = None
            for _ in range(args.reps + 1):      # the first is the warm-up
                ctx.synchronize()
                t0 = time.perf_counter()
                P.Optimizer.PoseOptimizationDevice(K, d_T, d_E, d_n, nedges, cam, d_To, d_o, d_g, ctx=ctx)
                ctx.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None or dt < best else best
            g, o = down(d_g, np.zeros(K, np.int32)), down(d_o, np.zeros((K, nedges), np.uint8))
            for k in range(K):
                mismatch += int(g[k] != loop[k % NSEEDS][0] or (o[k] != loop[k % NSEEDS][1]).any())
            for d in (d_T, d_E, d_n, d_To, d_o, d_g):
                ctx.device_free(d)
            row["device"].append({"frames": K, "launch_ms": round(best, 4), "ms_per_frame": round(best / K, 6)})
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
