"""Measurement of the candidate loop of LoopClosing::ComputeSim3 (src/LoopClosing.cc:252-284): ONE call of
pslfe_kf_search_by_bow_candidates for C loop candidates of n features each against one current keyframe, next to C calls of
pslfe_orb_search_by_bow (the (pKF, F) overload: the same candidate work, `<=` instead of `<` at TH_LOW) on the same inputs.  Both
take host buffers and return when the results are back, so the time is a host clock around the call(s); the device share of the set
call is its event-timed stage `kf.bow_candidates`.  Inputs: random 256-bit descriptors, each candidate a noisy copy of the current
keyframe in another feature order, a FeatureVector of 100 nodes (level 2 of a k = 10 vocabulary, what levelsup = 4 gives for L = 6),
half of the candidate's features with a good map point.  Prints one JSON line (and writes it with --out).  Also meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_loop_match.py --quick`.

Usage: python tools/bench_loop_match.py [--cands 1,4,16,64] [--features 1000,2000] [--reps 20] [--quick] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NNODES = 100


def make_inputs(P, n, ncand, rng):
    """per candidate: keypoints, descriptors, (fidx2, queries, qdesc) of the (KF1, KF2) search"""
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a1 = rng.uniform(0, 360, n).astype(np.float32)
    node1 = rng.integers(0, NNODES, n)
    good1 = rng.random(n) < 0.8
    out = []
    for _ in range(ncand):
        perm = rng.permutation(n)
        flips = rng.integers(0, 256, (n, 14))
        d2 = d1[perm].copy()
        for j in range(14):
            on = rng.random(n) < 0.7
            d2[np.arange(n)[on], flips[on, j] >> 3] ^= (1 << (flips[on, j] & 7)).astype(np.uint8)
        k2 = np.zeros(n, P.KEYPOINT_DTYPE)
        k2["x"], k2["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
        k2["angle"] = np.mod(a1[perm] + 10 + rng.normal(0, 4, n), 360).astype(np.float32)
        node2 = np.where(rng.random(n) < 0.85, node1[perm], rng.integers(0, NNODES, n))
        good2 = rng.random(n) < 0.5
        fidx, run = [], {}
        for nd in range(NNODES):
            keep = np.nonzero((node2 == nd) & good2)[0]
            run[nd] = (len(fidx), len(keep))
            fidx.extend(keep.tolist())
        order = np.concatenate([np.nonzero((node1 == nd) & good1)[0] for nd in range(NNODES)])
        q = np.zeros(len(order), P.BOWQUERY_DTYPE)
        q["start"] = [run[nd][0] for nd in node1[order]]
        q["len"] = [run[nd][1] for nd in node1[order]]
        q["angle"] = a1[order]
        out.append((k2, d2, np.array(fidx, np.int32), q, np.ascontiguousarray(d1[order])))
    return out


def measure(P, ctx, n, ncand, reps, rng):
    lib = P.lib()
    cands = make_inputs(P, n, ncand, rng)
    g = P.FrameGrid(max(n, 1), ncand, ctx=ctx)
    for c, (k2, d2, _, _, _) in enumerate(cands):
        g.set(c, k2, d2, (0.0, 0.0, 640.0, 480.0))
    kf = P.KeyFrameMatcher(ctx)
    slots = np.arange(ncand, dtype=np.int32)
    fidx = np.concatenate([c[2] for c in cands])
    q = np.concatenate([c[3] for c in cands])
    qd = np.concatenate([c[4] for c in cands])
    foff = np.concatenate([[0], np.cumsum([len(c[2]) for c in cands])]).astype(np.int32)
    qoff = np.concatenate([[0], np.cumsum([len(c[3]) for c in cands])]).astype(np.int32)
    match = np.full(len(q), -1, np.int32)
    nms = np.zeros(ncand, np.int32)
    ptr = P._ptr

    def set_call():
        P._check(lib.pslfe_kf_search_by_bow_candidates(kf._h, g._h, ptr(slots), C.c_int(ncand), ptr(fidx), ptr(foff), ptr(q), ptr(qd), ptr(qoff),
                                                       C.c_float(0.75), C.c_int(1), ptr(match), ptr(nms)), "pslfe_kf_search_by_bow_candidates")

    match1 = [np.full(len(c[3]), -1, np.int32) for c in cands]
    assigned1 = np.full(n, -1, np.int32)
    nm1 = C.c_int()

    def per_candidate_calls():
        for c, (_, _, f, qq, dd) in enumerate(cands):
            P._check(lib.pslfe_orb_search_by_bow(g._h, C.c_int(c), ptr(f), C.c_int(len(f)), ptr(qq), ptr(dd), C.c_int(len(qq)), C.c_float(0.75),
                                                 C.c_int(1), ptr(match1[c]), ptr(assigned1), C.byref(nm1)), "pslfe_orb_search_by_bow")

    def clock(run):
        for _ in range(3):
            run()
        ctx.synchronize()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    # the two paths alternate so that a drift of the host hits both
    a1, b1 = clock(set_call), clock(per_candidate_calls)
    a2, b2 = clock(set_call), clock(per_candidate_calls)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        set_call()
    ctx.synchronize()
    stage_ms = ctx.stage_time("kf.bow_candidates")[0] / reps
    ctx.profile(False)
    same = sum(int((match[qoff[c]:qoff[c + 1]] == match1[c]).all()) for c in range(ncand))
    return dict(features=n, candidates=ncand, queries=int(len(q)), fidx=int(len(fidx)), matches=int(nms.sum()),
                set_call_ms=dict(median=min(a1[0], a2[0]), runs=[a1, a2]), per_candidate_calls_ms=dict(median=min(b1[0], b2[0]), runs=[b1, b2]),
                set_call_device_stage_ms=stage_ms, ratio_calls_over_set=min(b1[0], b2[0]) / min(a1[0], a2[0]),
                candidates_with_equal_rows=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cands", default="1,4,16,64")
    ap.add_argument("--features", default="1000,2000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import psl_slam_amd as P
    ctx = P.default_context()
    cands = [4] if a.quick else [int(v) for v in a.cands.split(",")]
    feats = [1000] if a.quick else [int(v) for v in a.features.split(",")]
    rng = np.random.default_rng(5)
    rows = [measure(P, ctx, n, c, 5 if a.quick else a.reps, rng) for n in feats for c in cands]
    res = dict(bench="loop_match", nnodes=NNODES, nnratio=0.75, reps=a.reps, rows=rows,
               note="ms per ComputeSim3 candidate loop, host clock, host buffers in and out; candidates_with_equal_rows counts candidates "
                    "whose rows agree between the two overloads (they differ only where bestDist1 == 50)")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
