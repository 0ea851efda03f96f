"""Times the pose optimisation (pslfe_pose_optimize / pslfe_pose_optimize_device) against the plain C++ host loop of the same
restatement (tools/dropin/pose_main.cpp built with -DPSL_POSE_HOST_ONLY, one core of the same machine).

  python tools/bench_pose_opt.py [--out profiles/pose_opt_bench.json] [--reps 5] [--lil N] [--label TEXT] [--merge FILE ...]

One frame through the host form; K = 1, 32, 1024 and 12288 frames per launch through the device form, at 300 and 1000 edges per
frame (seeded cases of tests/pose_opt_cases.py: mixed edges, 30 % planted outliers, 0.5 px noise, start 2 degrees and 5 cm off; the
K frames of a launch cycle through 32 different seeds).  Exits 1 if the device form and the host loop differ in any flag or return
value.  Prints one JSON line and writes it to --out.  Needs the test tree: the cases come from tests/pose_opt_cases.py, so that the
tool and the tests optimise the same kind of frame.

--lil N (default 0: the point-edge entry points, as above) adds N LIL edges per frame (tests/pose_lil_cases.py: 30 % planted
outliers) and times pslfe_pose_optimize_lil / pslfe_pose_optimize_lil_device against the same host loop with the LIL rows in its
case file; its default --out is profiles/pose_opt_bench_lil.json.  Every device row also carries the median and the largest launch time of the
repetitions.  --label names the run in its JSON; --merge embeds the JSON lines of earlier runs (another build of the library
alternated with this one, repeated runs of the same build) under "other_runs", so that one file holds a comparison and its
run-to-run spread."""
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 32, 1024, 12288])
    ap.add_argument("--lil", type=int, default=0, help="LIL edges per frame")
    ap.add_argument("--label", default=None)
    ap.add_argument("--merge", nargs="*", default=[])
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "pose_opt_bench_lil.json" if args.lil else "pose_opt_bench.json")
    nlil = args.lil
    import torch  # noqa: F401  (PyTorch's HIP runtime first, as bench.py loads it)
    import psl_slam_amd as P
    import pose_opt_cases as pc
    if nlil:
        import pose_lil_cases as lc
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
           "host_loop": "tools/dropin/pose_main.cpp -DPSL_POSE_HOST_ONLY, g++ -O2, one core",
           "lil_edges": nlil, "rows": []}
    if args.label:
        res["label"] = args.label
    mismatch = 0
    for nedges in (300, 1000):
        cases = [lc.make_case(7000 + s, nedges, "mixed", 0.3, nlil, 0.3) if nlil else pc.make_case(7000 + s, nedges, "mixed", 0.3)
                 for s in range(NSEEDS)]
        # the host loop on one core: the 32 frames, best of reps
        path, out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        with open(path, "wb") as f:
            np.array([NSEEDS, nedges, nlil], np.int32).tofile(f)
            cam.tofile(f)
            for c in cases:
                c["Tcw"].tofile(f)
                np.array([nedges, nlil], np.int32).tofile(f)
                c["edges"].tofile(f)
                if nlil:
                    c["lil"].tofile(f)
        p = subprocess.run([exe, path, out, str(args.reps)], capture_output=True, text=True, check=True)
        loop_ms = json.loads(p.stdout.strip().splitlines()[-1])["loop_ms"] / NSEEDS
        loop = []
        with open(out, "rb") as f:
            for c in cases:
                np.fromfile(f, pc.POSE_DTYPE, 1)
                ng = int(np.fromfile(f, np.int32, 1)[0])
                np.fromfile(f, pc.INFO_DTYPE, 1)
                loop.append((ng, np.fromfile(f, np.uint8, nedges + nlil)))      # the point flags, then the LIL flags
        # one frame through the host form
        best = None
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            if nlil:
                ng, _, outl, outl_lil = P.Optimizer.PoseOptimization(cases[0]["Tcw"], cases[0]["edges"], cam, ctx=ctx, lil=cases[0]["lil"])
                outl = np.concatenate([outl, outl_lil])
            else:
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
            extra = ()
            if nlil:
                Ll = np.zeros((K, nlil), P.POSELIL_DTYPE)
                for k in range(K):
                    Ll[k] = cases[k % NSEEDS]["lil"]
                extra = tuple(ctx.device_array(a)[0] for a in (Ll, np.full(K, nlil, np.int32), np.zeros((K, nlil), np.uint8)))
            best, times = None, []
            for _ in range(args.reps + 1):      # the first is the warm-up
                ctx.synchronize()
                t0 = time.perf_counter()
                if nlil:
                    P.Optimizer.PoseOptimizationLilDevice(K, d_T, d_E, d_n, nedges, extra[0], extra[1], nlil, cam, d_To, d_o, extra[2], d_g, ctx=ctx)
                else:
                    P.Optimizer.PoseOptimizationDevice(K, d_T, d_E, d_n, nedges, cam, d_To, d_o, d_g, ctx=ctx)
                ctx.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None or dt < best else best
                times.append(dt)
            times = sorted(times[1:]) or times
            g, o = down(d_g, np.zeros(K, np.int32)), down(d_o, np.zeros((K, nedges), np.uint8))
            if nlil:
                o = np.concatenate([o, down(extra[2], np.zeros((K, nlil), np.uint8))], 1)
            for k in range(K):
                mismatch += int(g[k] != loop[k % NSEEDS][0] or (o[k] != loop[k % NSEEDS][1]).any())
            for d in (d_T, d_E, d_n, d_To, d_o, d_g) + extra:
                ctx.device_free(d)
            row["device"].append({"frames": K, "launch_ms": round(best, 4), "ms_per_frame": round(best / K, 6),
                                  "launch_ms_median": round(times[len(times) // 2], 4), "launch_ms_max": round(times[-1], 4)})
        res["rows"].append(row)
    res["mismatches"] = mismatch
    if args.merge:
        res["other_runs"] = []
        for path in args.merge:
            with open(path) as f:
                res["other_runs"].append(json.loads(f.read().strip().splitlines()[-1]))
    tmpdir.cleanup()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 1 if mismatch else 0


if __name__ == "__main__":
    sys.exit(main())
