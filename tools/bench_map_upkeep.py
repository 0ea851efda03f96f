"""Measurement of the map refresh: MapPoint::UpdateNormalAndDepth / MapLine::UpdateAverageDir for the whole map (what the reference runs
after a loop correction or a global BA: 100 000 points with 8 observations on average from 500 keyframes, 20 000 lines) and for the points
of one new keyframe (1 000), through
  host    pslfe_kf_update_normal_and_depth / pslfe_kf_line_update_average_dir: host arrays in, refreshed rows back, a host clock around
          the call (uploads, kernel, download, synchronisation);
  device  the *_device forms on arrays that are already in HBM: a host clock around `reps` queued calls and one synchronisation, per call;
          and the kernel alone as the event-timed stage;
  loop    tools/bench_map_upkeep_host.cpp: a plain C++ loop with the same arithmetic on one core of the host, written for this tool.
The whole-map sizes are timed with both layouts of the run-order sums (PSLFE_UPKEEP_SUM_WALK / _TILED), alternating.  Every device result
(host form and device form, each layout) is compared with the host loop's, byte for byte, and a difference ends the run with exit status 1.
Prints one JSON line and writes it to --out (default profiles/map_upkeep_bench.json).

Usage: python tools/bench_map_upkeep.py [--reps 20] [--quick] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HOST_SRC = os.path.join(ROOT, "tools", "bench_map_upkeep_host.cpp")
HOST_LIB = os.path.join(ROOT, "tools", "libbench_map_upkeep_host.so")


def host_loop():
    if not os.path.exists(HOST_LIB) or os.path.getmtime(HOST_LIB) < os.path.getmtime(HOST_SRC):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", HOST_LIB, HOST_SRC], check=True)
    return C.CDLL(HOST_LIB)


def clock(run, reps, sync=None, per=1):
    for _ in range(3):
        run()
    if sync:
        sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(per):
            run()
        if sync:
            sync()
        ts.append((time.perf_counter() - t0) * 1e3 / per)
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def measure(P, mc, ctx, H, kind, M, nkf, reps, layouts):
    rng = np.random.default_rng(M + nkf)
    lens = mc.whole_map_lengths(M, rng)
    make = mc.point_case if kind == "points" else mc.line_case
    rows, off, okf, ce, rk, rl, skip = make(M, seed=7, nkf=nkf, lens=lens)
    skip = (np.random.default_rng(3).random(M) < 0.02).astype(np.uint8)          # a map has few bad points
    rl = np.where(rl < 0, 0, rl).astype(np.int32)
    stage = "kf.update_normal_and_depth" if kind == "points" else "kf.line_update_average_dir"
    loop = H.host_update_normal_and_depth if kind == "points" else H.host_line_update_average_dir
    p = lambda a: C.c_void_p(a.ctypes.data)
    want = rows.copy()
    loop_args = (p(want), M, p(off), p(okf), p(ce), p(rk), p(rl), p(skip), p(mc.SCALE), len(mc.SCALE))
    res = dict(kind=kind, rows=M, observations=int(off[-1]), keyframes=nkf, host_loop_ms=clock(lambda: loop(*loop_args), reps))
    d = [ctx.device_array(a)[0] for a in (rows, off, okf, ce, rk, rl, skip)]
    kfs = {}
    for layout in layouts:
        kfs[layout] = P.KeyFrameMatcher(ctx)
        kfs[layout].set_upkeep_sum(P.UPKEEP_SUM_TILED if layout == "tiled" else P.UPKEEP_SUM_WALK)
    out = {}

    def host_form(layout):
        fn = kfs[layout].UpdateNormalAndDepth if kind == "points" else kfs[layout].LineUpdateAverageDir
        out[layout] = fn(rows, off, okf, ce, rk, rl, mc.SCALE, skip)

    def device_form(layout):
        fn = kfs[layout].update_normal_and_depth_device if kind == "points" else kfs[layout].line_update_average_dir_device
        fn(d[0], M, d[1], d[2], d[3], nkf, d[4], d[5], d[6], mc.SCALE)

    for name, run, kw in (("host_form_ms", host_form, {}), ("device_form_ms", device_form, dict(sync=ctx.synchronize, per=10))):
        runs = {l: [] for l in layouts}
        for _ in range(2):                                        # the layouts alternate so that a drift of the host hits both
            for l in layouts:
                runs[l].append(clock(lambda: run(l), reps, **kw))
        res[name] = {l: dict(median=min(r["median"] for r in runs[l]), runs=runs[l]) for l in layouts}
    res["kernel_ms"] = {}
    for l in layouts:
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(reps):
            device_form(l)
        ctx.synchronize()
        res["kernel_ms"][l] = ctx.stage_time(stage)[0] / reps
        ctx.profile(False)
    res["equal_host_loop"] = {}
    for l in layouts:                                             # the device form once more on fresh rows, downloaded and compared
        P._check(P.lib().pslfe_device_upload(ctx._h, C.c_void_p(d[0]), p(rows), C.c_size_t(rows.nbytes)), "pslfe_device_upload")
        device_form(l)
        ctx.synchronize()
        got = np.zeros_like(rows)
        P._check(P.lib().pslfe_device_download(ctx._h, p(got), C.c_void_p(d[0]), C.c_size_t(got.nbytes)), "pslfe_device_download")
        res["equal_host_loop"][l] = dict(host_form=bool(out[l].tobytes() == want.tobytes()), device_form=bool(got.tobytes() == want.tobytes()))
    for x in d:
        ctx.device_free(x)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_upkeep_bench.json"))
    a = ap.parse_args()
    import map_upkeep_cases as mc
    import psl_slam_amd as P
    H = host_loop()
    ctx = P.default_context()
    reps = 3 if a.quick else a.reps
    both = ("walk", "tiled")
    sizes = [("points", 2000, 50, both)] if a.quick else [("points", 100000, 500, both), ("lines", 20000, 500, both), ("points", 1000, 20, both),
                                                           ("lines", 200, 20, both)]
    rows = [measure(P, mc, ctx, H, kind, M, nkf, reps, layouts) for kind, M, nkf, layouts in sizes]
    res = dict(bench="map_upkeep", reps=reps, nlevels=len(mc.SCALE), rows=rows,
               note="ms per refresh of all rows.  host_form_ms: host arrays in and out, host clock.  device_form_ms: arrays resident in HBM, "
                    "host clock over 10 queued calls and one synchronisation, per call.  kernel_ms: the event-timed stage.  host_loop_ms: "
                    "tools/bench_map_upkeep_host.cpp on one host core (written for this tool).  Run lengths: geometric, mean 8, at least 2; "
                    "2 % of the rows skipped.")
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    bad = [(r["kind"], r["rows"], l, k) for r in rows for l, e in r["equal_host_loop"].items() for k, same in e.items() if not same]
    if bad:
        print("results differ from the host loop:", bad, file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
