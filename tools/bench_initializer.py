"""Times the monocular map initialisation (pslfe_init_initialize / pslfe_init_initialize_device) against the plain C++ loop of the same
header (tools/dropin/init_main.cpp built with -DPSL_INIT_HOST_ONLY, one core of the same machine; the JSON names the core).

  python tools/bench_initializer.py [--out profiles/initializer_bench.json] [--reps 5] [--label TEXT]

One pair through the host form; K = 1, 1024 and 12288 pairs per launch through the device form, at 100, 500 and 2000 matches per pair,
with the reference's 200 iterations and sigma 1.0.  The pairs are those of tests/initializer_cases.py (make_scene: the general scene,
0.3 px of noise, one match in ten inconsistent, a quarter more keypoints than matches in each frame); the K pairs of a launch cycle
through 16 scenes and pair p is seeded SEED0 + p, so the first 16 pairs of a launch are the host loop's 16 and are compared with it: a
result record, a point or a flag that differs is counted in "mismatches" and makes the tool exit 1.  Prints one JSON line and writes it
to --out.  Launch times are host wall-clock around launch + synchronise (best, median and largest of the repetitions after one
warm-up).  Nothing is gated on these times."""
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

NSEEDS = 16
SEED0 = 9000
MAX_ITS = 200


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initializer_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, nargs="*", default=[1, 1024, 12288])
    ap.add_argument("--matches", type=int, nargs="*", default=[100, 500, 2000])
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (PyTorch's HIP runtime first, as bench.py loads it)
    import psl_slam_amd as P
    import initializer_cases as ic
    ctx = P.default_context()
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in ic.CAM.items():
        cam[k] = v
    tmpdir = tempfile.TemporaryDirectory()
    tmp = tmpdir.name
    exe = os.path.join(tmp, "init_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_INIT_HOST_ONLY", "-o", exe,
                    os.path.join(ROOT, "tools", "dropin", "init_main.cpp")], check=True, capture_output=True)

    def down(d, a):
        P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
        return a

    res = {"tool": "bench_initializer", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "reps": args.reps,
           "iterations": MAX_ITS, "host_loop": "tools/dropin/init_main.cpp -DPSL_INIT_HOST_ONLY, g++ -O2, one core of " + _core(), "rows": []}
    if args.label:
        res["label"] = args.label
    mismatch = 0
    for nm in args.matches:
        extra = nm // 4
        scenes = [ic.make_scene(500 + s, nm, consistent=0.9, extra1=extra, extra2=extra, noise_px=0.3)[:3] for s in range(NSEEDS)]
        cases = [dict(keys1=k1, keys2=k2, matches=m, seed=SEED0 + s, max_its=MAX_ITS, sigma=1.0) for s, (k1, k2, m) in enumerate(scenes)]
        path, out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        ic.write_cases(path, cases, P.CAMERA_DTYPE)
        p = subprocess.run([exe, path, out, str(max(args.reps, 2))], capture_output=True, text=True, check=True)
        loop_ms = json.loads(p.stdout.strip().splitlines()[-1])["loop_ms"] / NSEEDS
        with open(out, "rb") as f:
            loop = ic.read_section(f, cases)
        n1 = nm + extra
        best = None
        for _ in range(args.reps + 1):
            init = P.Initializer(scenes[0][0], cam, 1.0, MAX_ITS, seed=SEED0, ctx=ctx)
            t0 = time.perf_counter()
            init.Initialize(scenes[0][1], scenes[0][2])
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None or dt < best else best
        mismatch += int(init.result.tobytes() != loop[0]["res"].tobytes())
        row = {"matches": nm, "keypoints": n1, "host_loop_ms_per_pair": round(loop_ms, 4), "host_form_ms": round(best, 4),
               "initialized": int(sum(int(r["res"]["status"]) & 1 for r in loop)), "device": []}
        for K in args.pairs:
            k1, k2, m = np.zeros((K, n1, 2), np.float32), np.zeros((K, n1, 2), np.float32), np.zeros((K, n1), np.int32)
            for k in range(K):
                k1[k], k2[k], m[k] = scenes[k % NSEEDS]
            bufs = [ctx.device_array(a)[0] for a in (k1, k2, np.full(K, n1, np.int32), np.full(K, n1, np.int32), m, np.zeros(K, P.INITRESULT_DTYPE),
                                                     np.zeros((K, n1, 3), np.float32), np.zeros((K, n1), np.uint8))]
            times = []
            for _ in range(args.reps + 1):      # the first is the warm-up
                ctx.synchronize()
                t0 = time.perf_counter()
                P.Initializer.InitializeDevice(K, bufs[0], bufs[2], bufs[1], bufs[3], 8, n1, bufs[4], n1, cam, bufs[5], bufs[6], bufs[7],
                                               iterations=MAX_ITS, seed0=SEED0, ctx=ctx)
                ctx.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            times = sorted(times[1:]) or times
            r, p3, tr = down(bufs[5], np.zeros(K, P.INITRESULT_DTYPE)), down(bufs[6], np.zeros((K, n1, 3), np.float32)), down(bufs[7], np.zeros((K, n1), np.uint8))
            for k in range(min(K, NSEEDS)):
                mismatch += int(r[k].tobytes() != loop[k]["res"].tobytes() or p3[k].tobytes() != loop[k]["p3d"].tobytes() or
                                (tr[k] != loop[k]["tri"]).any())
            for d in bufs:
                ctx.device_free(d)
            row["device"].append({"pairs": K, "launch_ms": round(times[0], 4), "ms_per_pair": round(times[0] / K, 6),
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
