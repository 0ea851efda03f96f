"""First timings of the local bundle adjustment (pslfe_ba_local_device) against the plain C++ host loop of the same header
(tools/dropin/ba_main.cpp built with -DPSL_BA_HOST_ONLY at -O2, one core of the same machine).  Not gated and not part of bench.py.

  python tools/bench_local_ba.py [--out profiles/local_ba_bench.json] [--reps 5] [--problems 1 64 1024] [--sizes small large]
                                 [--lils 60 300 [--lil-obs 4]]

--lils gives, per size, the number of VertexLIL rows planted into every scene (tests/ba_lil_cases.plant_lils, --lil-obs observations
each): such a size runs pslfe_ba_local_lil_device against tools/dropin/ba_lil_main.cpp; a size with 0 LILs (the default) runs the
point-only entry point against ba_main.cpp exactly as before.

Two sizes (seeded scenes of tests/ba_cases.py: mixed edges, 0.5 px noise, start 1 degree / 3 cm / 5 cm off):
  small   10 keyframes (8 free + 2 fixed) / 500 points / ~3 k edges
  large   30 free + 20 fixed keyframes / 3000 points / ~20 k edges
One problem and K = 64 / 1024 problems per launch (the K problems cycle through NSEEDS different scenes); one warm-up launch, then
--reps timed ones, each from the launch to the end of a stream synchronisation; the median and the fastest are reported.  The host
loop runs the NSEEDS scenes once per repetition (best of 3).  Exits 1 if the device form and the host loop differ in any output
byte of the first NSEEDS problems.  Prints one JSON line and writes it to --out.  Needs the test tree for the scenes."""
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

NSEEDS = 4
SIZES = {"small": dict(nfree=8, nfixed=2, npts=500, pobs=0.6), "large": dict(nfree=30, nfixed=20, npts=3000, pobs=0.1333)}


def _cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _lil_size(P, ctx, bc, lc, args, result, size, spec, scenes, caps, nlil, exe, tmp, down):
    """one size with nlil LILs per scene through pslfe_ba_local_lil_device and the one-core loop of ba_lil_main.cpp"""
    scenes = [lc.plant_lils(c, 9000 + s, nlil, args.lil_obs) for s, c in enumerate(scenes)]
    caps = (*caps, nlil, max(len(c["ledges"]) for c in scenes))
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in scenes[0]["cam"].items():
        cam[k] = v
    path, out = os.path.join(tmp, "cases_lil.bin"), os.path.join(tmp, "out_lil.bin")
    lc.write_cases(path, scenes, 2, caps)
    p = subprocess.run([exe, path, out, "3"], check=True, capture_output=True, text=True)
    loop_ms = json.loads(p.stdout)["loop_ms"] / NSEEDS
    loop = lc.read_sections(out, scenes, 1)[0]
    row = {"keyframes": caps[0], "free": spec["nfree"], "points": caps[1], "edges": [len(c["edges"]) for c in scenes], "lils": nlil,
           "lil_edges": [len(c["ledges"]) for c in scenes], "iterations": [[int(v) for v in r["info"]["iterations"]] for r in loop],
           "host_loop_ms_per_problem": loop_ms, "launches": {}}
    keys = ("kf", "mp", "edges", "lil", "ledges")
    dts = (P.BAKEYFRAME_DTYPE, P.MAPPOINT_DTYPE, P.BAEDGE_DTYPE, P.MAPLIL_DTYPE, P.BALILEDGE_DTYPE)
    ok = True
    for K in args.problems:
        ba = P.BundleAdjuster(K, *caps, ctx=ctx)
        cs = [scenes[k % NSEEDS] for k in range(K)]
        rows = [np.concatenate([np.ascontiguousarray(c[k], dt) for c in cs]) for k, dt in zip(keys, dts)]
        off = [np.cumsum([0] + [len(c[k]) for c in cs]).astype(np.int32) for k in keys]
        outs = [np.zeros_like(rows[0]), np.zeros_like(rows[1]), np.zeros(len(rows[2]), np.uint8), np.zeros_like(rows[3]), np.zeros(len(rows[4]), np.uint8)]
        d = [ctx.device_array(a)[0] for a in (*rows, *off, *outs, np.zeros(K, P.BAINFO_DTYPE))]
        times = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            P.Optimizer.LocalBundleAdjustmentAndInseclinesDevice(ba, K, d[0], d[5], d[1], d[6], d[2], d[7], d[3], d[8], d[4], d[9], cam, 2, d[10], d[11], d[12],
                                                                 d[13], d[14], 0, d[15])
            ctx.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        times = sorted(times[1:])
        got = [down(d[10 + i], outs[i]) for i in range(5)]
        for k in range(min(K, NSEEDS)):
            for i, (key, o) in enumerate(zip(("kf", "mp", "erase", "lil", "erase_lil"), (0, 1, 2, 3, 4))):
                ok = ok and got[i][off[o][k]:off[o][k + 1]].tobytes() == loop[k][key].tobytes()
        for p_ in d:
            ctx.device_free(p_)
        ba.close()
        row["launches"][str(K)] = {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1],
                                   "median_ms_per_problem": times[len(times) // 2] / K}
        print(size, "with", nlil, "LILs, K =", K, row["launches"][str(K)], "host loop ms", loop_ms, file=sys.stderr, flush=True)
    result["sizes"][size + "_lil"] = row
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_ba_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--problems", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--sizes", nargs="*", default=["small", "large"])
    ap.add_argument("--lils", type=int, nargs="*", default=[])
    ap.add_argument("--lil-obs", type=int, default=4)
    args = ap.parse_args()
    import torch  # PyTorch's HIP runtime first, as bench.py loads it
    import psl_slam_amd as P
    import ba_cases as bc
    import ba_lil_cases as lc
    ctx = P.default_context()
    tmpdir = tempfile.TemporaryDirectory()
    exe = os.path.join(tmpdir.name, "ba_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_BA_HOST_ONLY", "-o", exe, os.path.join(ROOT, "tools", "dropin", "ba_main.cpp")],
                   check=True)
    exe_lil = os.path.join(tmpdir.name, "ba_lil_host")
    if any(args.lils):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_BA_HOST_ONLY", "-o", exe_lil,
                        os.path.join(ROOT, "tools", "dropin", "ba_lil_main.cpp")], check=True)
    down = lambda d, a: (P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "download"), a)[1]
    result = {"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
              "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "host_core": _cpu_name(), "reps": args.reps, "sizes": {}}
    ok = True
    for si, size in enumerate(args.sizes):
        spec = SIZES[size]
        nlil = args.lils[si] if si < len(args.lils) else 0
        scenes = [bc.make_scene(9000 + s, spec["nfree"], spec["nfixed"], spec["npts"], "mixed", pobs=spec["pobs"]) for s in range(NSEEDS)]
        caps = (spec["nfree"] + spec["nfixed"], spec["npts"], max(len(c["edges"]) for c in scenes))
        if nlil:
            ok = _lil_size(P, ctx, bc, lc, args, result, size, spec, scenes, caps, nlil, exe_lil, tmpdir.name, down) and ok
            continue
        cam = np.zeros((), P.CAMERA_DTYPE)
        for k, v in scenes[0]["cam"].items():
            cam[k] = v
        # one core
        path, out = os.path.join(tmpdir.name, "cases.bin"), os.path.join(tmpdir.name, "out.bin")
        bc.write_cases(path, scenes, 2, caps)
        p = subprocess.run([exe, path, out, "3"], check=True, capture_output=True, text=True)
        loop_ms = json.loads(p.stdout)["loop_ms"] / NSEEDS
        loop = bc.read_sections(out, scenes, 1)[0]
        row = {"keyframes": caps[0], "free": spec["nfree"], "points": caps[1], "edges": [len(c["edges"]) for c in scenes],
               "iterations": [[int(v) for v in r["info"]["iterations"]] for r in loop], "host_loop_ms_per_problem": loop_ms, "launches": {}}
        for K in args.problems:
            ba = P.BundleAdjuster(K, *caps, ctx=ctx)
            cs = [scenes[k % NSEEDS] for k in range(K)]
            kf = np.concatenate([np.ascontiguousarray(c["kf"], P.BAKEYFRAME_DTYPE) for c in cs])
            mp = np.concatenate([np.ascontiguousarray(c["mp"], P.MAPPOINT_DTYPE) for c in cs])
            ed = np.concatenate([np.ascontiguousarray(c["edges"], P.BAEDGE_DTYPE) for c in cs])
            off = [np.cumsum([0] + [len(c[k]) for c in cs]).astype(np.int32) for k in ("kf", "mp", "edges")]
            d = [ctx.device_array(a)[0] for a in (kf, mp, ed, *off, np.zeros(len(kf), P.BAKEYFRAME_DTYPE), np.zeros(len(mp), P.MAPPOINT_DTYPE),
                                                  np.zeros(len(ed), np.uint8), np.zeros(K, P.BAINFO_DTYPE))]
            times = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                P.Optimizer.LocalBundleAdjustmentDevice(ba, K, d[0], d[3], d[1], d[4], d[2], d[5], cam, 2, d[6], d[7], d[8], d[9])
                ctx.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            times = sorted(times[1:])
            ko, mo, er = down(d[6], np.zeros(len(kf), P.BAKEYFRAME_DTYPE)), down(d[7], np.zeros(len(mp), P.MAPPOINT_DTYPE)), down(d[8], np.zeros(len(ed), np.uint8))
            for k in range(min(K, NSEEDS)):
                same = (ko[off[0][k]:off[0][k + 1]].tobytes() == loop[k]["kf"].tobytes() and mo[off[1][k]:off[1][k + 1]].tobytes() == loop[k]["mp"].tobytes()
                        and er[off[2][k]:off[2][k + 1]].tobytes() == loop[k]["erase"].tobytes())
                ok = ok and same
            for p_ in d:
                ctx.device_free(p_)
            ba.close()
            row["launches"][str(K)] = {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1],
                                       "median_ms_per_problem": times[len(times) // 2] / K}
            print(size, "K =", K, row["launches"][str(K)], "host loop ms", loop_ms, file=sys.stderr, flush=True)
        result["sizes"][size] = row
    result["device_equals_host_loop"] = ok
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
