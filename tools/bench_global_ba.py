"""First timings of the global bundle adjustment (pslfe_gba_optimize_device: one problem over the whole device) against (a) the same
driver on one host core (tools/dropin/gba_main.cpp built with -DPSL_GBA_HOST_ONLY at -O2) and (b), where the shape fits both,
pslfe_ba_local_device with K = 1 and rounds = 1 at (5, robust) on a stereo-only scene: the arithmetic and the bits are equal there,
so the ratio is the execution model alone.  Not gated and not part of bench.py.

  python tools/bench_global_ba.py [--out profiles/global_ba_bench.json] [--reps 5] [--sizes large map200 map1000] [--no-host map1000] [--host-repeat 3]

Shapes:
  large     the local BA's large shape, stereo edges only: 30 free + 20 fixed keyframes / 3000 points / ~20 k edges (ba_cases.make_scene)
  map200    200 keyframes / 20 000 points / 120 k edges on the windowed scene (gba_cases.make_window_scene, 6 keyframes per point)
  map1000   1000 keyframes / 100 000 points / 600 k edges, device only by default (the one-core loop takes minutes there)
One call from entry to return (the call is synchronous), one warm-up, then --reps timed calls; the median, the fastest and the
slowest are reported.  The one-core loop is the best of --host-repeat (3) runs of the program, the first of which warms its
caches.  On `large` the local kernel and the global form alternate, three runs each per repetition block.  Exits 1 if the device form and the one-core loop (or, on `large`, the local kernel in the free keyframes and all points) differ in an output
byte.  Prints one JSON line and writes it to --out.  Needs the test tree for the scenes."""
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


def _cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _stats(times):
    t = sorted(times)
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "runs": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_ba_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", nargs="*", default=["large", "map200", "map1000"])
    ap.add_argument("--no-host", nargs="*", default=["map1000"])
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--host-repeat", type=int, default=3)
    args = ap.parse_args()
    import torch  # PyTorch's HIP runtime first, as bench.py loads it
    import psl_slam_amd as P
    import ba_cases as bc
    import gba_cases as gc
    ctx = P.default_context()
    tmp = tempfile.TemporaryDirectory()
    exe = os.path.join(tmp.name, "gba_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_GBA_HOST_ONLY", "-o", exe, os.path.join(ROOT, "tools", "dropin", "gba_main.cpp")],
                   check=True)
    down = lambda d, a: (P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "download"), a)[1]
    result = {"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
              "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "host_core": _cpu_name(), "reps": args.reps,
              "iterations": args.iterations, "robust": 1, "sizes": {}}
    ok = True
    for size in args.sizes:
        if size == "large":
            c = bc.make_scene(9000, 30, 20, 3000, "stereo", pobs=0.1333)
        elif size == "map200":
            c = gc.make_window_scene(9100, 200, 20000, "mixed", window=6)
        elif size == "map1000":
            c = gc.make_window_scene(9200, 1000, 100000, "mixed", window=6)
        else:
            raise SystemExit(f"unknown size {size}")
        kf, mp, ed = (np.ascontiguousarray(c[k], dt) for k, dt in (("kf", P.BAKEYFRAME_DTYPE), ("mp", P.MAPPOINT_DTYPE), ("edges", P.BAEDGE_DTYPE)))
        caps = (len(kf), len(mp), len(ed))
        cam = np.zeros((), P.CAMERA_DTYPE)
        for k, v in c["cam"].items():
            cam[k] = v
        row = {"keyframes": len(kf), "points": len(mp), "edges": len(ed)}
        gba = P.GlobalBundleAdjuster(*caps, ctx=ctx)
        d_kf, d_mp, d_ed = (ctx.device_array(a)[0] for a in (kf, mp, ed))
        d_ko, d_mo, d_ni = (ctx.device_array(a)[0] for a in (np.zeros_like(kf), np.zeros_like(mp), np.zeros(len(mp), np.uint8)))

        def run_global():
            t0 = time.perf_counter()
            info = P.Optimizer.BundleAdjustmentDevice(gba, d_kf, len(kf), d_mp, len(mp), d_ed, len(ed), cam, args.iterations, 1, d_ko, d_mo, d_ni)
            return (time.perf_counter() - t0) * 1e3, info

        run_global()
        if size == "large":       # (b): the one-workgroup kernel against the whole-device form, alternating, three runs each per block
            ba = P.BundleAdjuster(1, *caps, ctx=ctx)
            off = [ctx.device_array(np.array([0, n], np.int32))[0] for n in caps]
            l_ko, l_mo, l_er, l_info = (ctx.device_array(a)[0] for a in (np.zeros_like(kf), np.zeros_like(mp), np.zeros(len(ed), np.uint8), np.zeros(1, P.BAINFO_DTYPE)))

            def run_local():
                t0 = time.perf_counter()
                P.Optimizer.LocalBundleAdjustmentDevice(ba, 1, d_kf, off[0], d_mp, off[1], d_ed, off[2], cam, 1, l_ko, l_mo, l_er, l_info)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e3

            run_local()
            tl, tg = [], []
            for _ in range(max(1, (args.reps + 2) // 3)):
                tl += [run_local() for _ in range(3)]
                tg += [run_global()[0] for _ in range(3)]
            row["local_K1_rounds1"], row["global"] = _stats(tl), _stats(tg)
            row["local_over_global"] = row["local_K1_rounds1"]["median_ms"] / row["global"]["median_ms"]
            lk, lm = down(l_ko, np.zeros_like(kf)), down(l_mo, np.zeros_like(mp))
            gk, gm = down(d_ko, np.zeros_like(kf)), down(d_mo, np.zeros_like(mp))
            free = kf["fixed"] == 0
            row["global_equals_local"] = bool(gk[free].tobytes() == lk[free].tobytes() and gm.tobytes() == lm.tobytes())
            ok = ok and row["global_equals_local"]
            for p_ in (*off, l_ko, l_mo, l_er, l_info):
                ctx.device_free(p_)
            ba.close()
        else:
            times = []
            for _ in range(args.reps):
                times.append(run_global()[0])
            row["global"] = _stats(times)
        _, info = run_global()
        row["info"] = {k: (int(info[k]) if k in ("status", "iterations", "free_keyframes", "included_points") else float(info[k])) for k in info.dtype.names}
        if size not in args.no_host:   # (a): the same driver on one core
            path, out = os.path.join(tmp.name, "cases.bin"), os.path.join(tmp.name, "out.bin")
            gc.write_cases(path, [c], args.iterations, 1, caps)
            p = subprocess.run([exe, path, out, str(args.host_repeat)], check=True, capture_output=True, text=True)
            row["host_loop_ms"], row["host_loop_runs"] = json.loads(p.stdout)["loop_ms"], args.host_repeat   # the best of that many runs
            loop = gc.read_sections(out, [c], 1)[0][0]
            gk, gm, gn = down(d_ko, np.zeros_like(kf)), down(d_mo, np.zeros_like(mp)), down(d_ni, np.zeros(len(mp), np.uint8))
            row["device_equals_host_loop"] = bool(gk.tobytes() == loop["kf"].tobytes() and gm.tobytes() == loop["mp"].tobytes() and
                                                  gn.tobytes() == loop["not_included"].tobytes() and int(info["iterations"]) == int(loop["info"]["iterations"]))
            ok = ok and row["device_equals_host_loop"]
            row["host_loop_over_global"] = row["host_loop_ms"] / row["global"]["median_ms"]
        for p_ in (d_kf, d_mp, d_ed, d_ko, d_mo, d_ni):
            ctx.device_free(p_)
        gba.close()
        print(size, row, file=sys.stderr, flush=True)
        result["sizes"][size] = row
    result["all_equal"] = ok
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
