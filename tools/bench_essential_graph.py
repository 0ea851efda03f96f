"""First timings of the essential-graph optimisation (pslfe_eg_optimize_device) against the plain C++ host loop of the same header
(tools/dropin/essential_main.cpp built with -DPSL_EG_HOST_ONLY at -O2, one core of the same machine).  Not gated and not part of
bench.py.

  python tools/bench_essential_graph.py [--out profiles/essential_graph_bench.json] [--reps 5] [--graphs 1 64 1024] [--sizes short long]

Two shapes (seeded rings of tests/essential_cases.py: odometry drift accumulated along the chain, the last two keyframes corrected,
free scale, 2 map points per keyframe):
  short   50 keyframes / 150 edges: (i, i - 1), (i, i - 2), (i, i - 3) and one loop edge, like a short sequence
  long    300 keyframes / 1200 edges: (i, i - 1) .. (i, i - 4) and two loop edges, like a long one
One graph and K = 64 / 1024 graphs per launch (the K graphs cycle through NSEEDS different rings); one warm-up launch, then --reps
timed ones, each from the launch to the end of a stream synchronisation; the median and the fastest are reported.  The host loop
runs the NSEEDS rings once per repetition (best of 3).  Exits 1 if the device form and the host loop differ in any output byte of
the first NSEEDS graphs.  Prints one JSON line and writes it to --out.  Needs the test tree for the rings."""
import argparse
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
SIZES = {"short": dict(n=50, span=(1, 2, 3), loops=1), "long": dict(n=300, span=(1, 2, 3, 4), loops=2)}


def _cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _envelope(c):
    """the envelope doubles the graph needs (the rule of essential_kernels.h), without running the restatement"""
    import essential_cases as ec
    g = ec.Graph(c["kf"], c["edges"], c["mp"], c["mp_ref"], False, caps=(1 << 20, 1 << 24, 1 << 26, 1 << 62))
    assert g.check() == 0
    return g.env_size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_graph_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graphs", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--sizes", nargs="+", default=["short", "long"])
    args = ap.parse_args()
    import ctypes as C
    import essential_cases as ec
    import psl_slam_amd as P
    ctx = P.default_context()
    tmp = tempfile.mkdtemp(prefix="eg_bench_")
    exe = os.path.join(tmp, "essential_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_EG_HOST_ONLY", "-o", exe, os.path.join(ROOT, "tools", "dropin", "essential_main.cpp")],
                   check=True)

    def down(d, a):
        P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
        return a

    result = {"device": "MI355X (gfx950)", "host_cpu": _cpu_name(), "reps": args.reps, "sizes": {}, "counters": "none collected"}
    ok = True
    for size in args.sizes:
        spec = SIZES[size]
        rings = [ec.ring(spec["n"], 100 + s, drift=0.002, scale_drift=0.001, span=spec["span"], loops=spec["loops"], npoints=2 * spec["n"])
                 for s in range(NSEEDS)]
        caps = (spec["n"], max(len(c["edges"]) for c in rings), 2 * spec["n"], max(_envelope(c) for c in rings))
        path, out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        ec.write_cases(path, rings, False, caps)
        p = subprocess.run([exe, path, out, "3"], check=True, capture_output=True, text=True)
        loop_ms = json.loads(p.stdout)["loop_ms"] / NSEEDS
        loop = ec.read_sections(out, rings, 1)[0]
        row = {"keyframes": spec["n"], "edges": [len(c["edges"]) for c in rings], "points": 2 * spec["n"], "envelope_doubles": caps[3],
               "iterations": [int(r["info"]["iterations"]) for r in loop], "host_loop_ms_per_graph": loop_ms, "launches": {}}
        for K in args.graphs:
            eg = P.EssentialGraph(K, *caps, ctx=ctx)
            cs = [rings[k % NSEEDS] for k in range(K)]
            rows = [np.concatenate([np.ascontiguousarray(c[k], dt).reshape(-1) for c in cs])
                    for k, dt in (("kf", P.EGKEYFRAME_DTYPE), ("edges", P.EGEDGE_DTYPE), ("mp", P.MAPPOINT_DTYPE), ("mp_ref", np.int32))]
            off = [np.cumsum([0] + [len(c[k]) for c in cs]).astype(np.int32) for k in ("kf", "edges", "mp")]
            outs = [np.zeros(len(rows[0]), P.POSE_DTYPE), np.zeros((len(rows[0]), 8)), np.zeros_like(rows[2]), np.zeros(K, P.EGINFO_DTYPE)]
            d = [ctx.device_array(a)[0] for a in (*rows, *off, *outs)]
            times = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                P.Optimizer.OptimizeEssentialGraphDevice(eg, K, d[0], d[4], d[1], d[5], d[2], d[3], d[6], False, d[7], d[8], d[9], d[10])
                ctx.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            times = sorted(times[1:])
            pose, S, mp = down(d[7], outs[0]), down(d[8], outs[1]), down(d[9], outs[2])
            info = down(d[10], outs[3])
            for k in range(min(K, NSEEDS)):
                a, b, m0, m1 = off[0][k], off[0][k + 1], off[2][k], off[2][k + 1]
                same = (info[k].tobytes() == loop[k]["info"].tobytes() and pose[a:b].tobytes() == loop[k]["pose"].tobytes() and
                        S[a:b].tobytes() == loop[k]["S"].tobytes() and mp[m0:m1].tobytes() == loop[k]["mp"].tobytes())
                ok = ok and same
            for x in d:
                ctx.device_free(x)
            eg.close()
            med = times[len(times) // 2]
            row["launches"][str(K)] = {"median_ms": med, "fastest_ms": times[0], "ms_per_graph": med / K, "speedup_vs_host_core": loop_ms / (med / K)}
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
