"""Generates the committed golden vectors from the CPU oracle (oracle/libpsl_oracle.so).

The reference ships no fixtures and cannot be built here, so these vectors
certify HIP == oracle and guard the oracle against regressions; they do NOT certify
oracle == OpenCV (parity unpinned).  Run:  python tests/golden/make_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import oracle_lib  # noqa: E402
import synth_frames as sf  # noqa: E402

CASES = [
    # name, w, h, style, seed, t, nfeatures, nlevels
    ("orb_640x480_desk", 640, 480, "desk", sf.SEED, 0, 1000, 8),
    ("orb_640x480_struct", 640, 480, "struct", sf.SEED + 1, 2, 1000, 8),
    ("orb_320x240_desk", 320, 240, "desk", sf.SEED + 2, 1, 500, 4),
]


def main():
    for name, w, h, style, seed, t, nf, nl in CASES:
        img = sf.Scene(w, h, style, seed).gray(t)
        orc = oracle_lib.OracleORB(nf, 1.2, nl, 20, 7)
        kps, desc = orc(img)
        cands = [len(orc.candidates(l)) for l in range(nl)]
        np.savez_compressed(os.path.join(HERE, name + ".npz"), image=img, kps=kps, desc=desc,
                            cfg=np.array([nf, nl, 20, 7], np.int32), ncand=np.array(cands, np.int32))
        print(name, img.shape, len(kps), cands)
    # matching golden: frame pair of the desk scene, queries = frame 0 keypoints at their own pixels
    sc = sf.Scene(640, 480, "desk", sf.SEED)
    orc = oracle_lib.OracleORB(1000, 1.2, 8, 20, 7)
    k0, d0 = orc(sc.gray(0))
    k1, d1 = orc(sc.gray(1))
    scale = sf.orb_scale_factors()
    q = np.zeros(len(k0), oracle_lib.PROJQUERY_DTYPE)
    q["u"], q["v"] = k0["x"], k0["y"]
    q["radius"] = np.float32(15.0) * scale[k0["octave"]]
    q["min_level"], q["max_level"] = k0["octave"] - 1, k0["octave"] + 1
    q["angle"], q["blocks"] = k0["angle"], 1
    bounds = (0.0, 0.0, 640.0, 480.0)
    nm, match, assigned = oracle_lib.search_by_projection_last(k1, d1, None, bounds, q, d0, None, True)
    idx, dist = oracle_lib.hamming_knn2(d0[:200], d1[:200])
    np.savez_compressed(os.path.join(HERE, "match_640x480_desk.npz"), k1=k1, d1=d1, queries=q, qdesc=d0,
                        nmatches=np.int32(nm), match=match, assigned=assigned, knn_idx=idx, knn_dist=dist)
    print("match", nm)


def lines():
    img = sf.Scene(640, 480, "struct", sf.SEED + 1).gray(2)
    kls, desc, eq = oracle_lib.line_extract(img, 200)
    seg = oracle_lib.lsd_detect(img)            # LSD_REFINE_ADV, the default
    oracle_lib.set_lsd_refine(1)
    seg_std = oracle_lib.lsd_detect(img)        # LSD_REFINE_STD
    oracle_lib.set_lsd_refine(2)
    L = np.stack([kls[n] for n in ("startPointX", "startPointY", "endPointX", "endPointY")], 1).astype(np.float32)
    fans = oracle_lib.lil_pair(L, 20.0, np.float32(np.pi / 4), 640, 480)
    np.savez_compressed(os.path.join(HERE, "line_640x480_struct.npz"), image=img, segments=seg, segments_std=seg_std, kls=kls, desc=desc, eq=eq, fans=fans)
    print("lines", len(seg), len(kls), len(fans))


def glue():
    import glue_scene
    kls, fans, depth, cam, _ = glue_scene.scene(seed=3)
    r = oracle_lib.frame_glue(kls, fans, depth, cam, seed=1)
    # the depth image is re-rendered by glue_scene (1.2 MB as f32); its CRC pins it
    import zlib
    np.savez_compressed(os.path.join(HERE, "glue_640x480_corner.npz"), kls=kls, fans=fans, depth_crc=np.uint32(zlib.crc32(depth.tobytes())),
                        seed=np.uint32(1), **{"out_" + k: v for k, v in r.items()})
    print("glue", int((np.abs(r["lines3d"]).sum(1) > 0).sum()), len(r["pair"]), len(r["planes"]))


def ref():
    """ref_pins.npz: the outputs of the reference's standalone files (oracle/_ref, `make -C oracle _ref REF=<reference tree>`) on the
    inputs of tests/test_oracle_ref_cpu.py, which pins the oracle against them without a reference tree.  Outputs and input CRCs only."""
    import ctypes as C
    import ref_cases as T
    rdir = os.path.join(ROOT, "oracle", "_ref")
    out = {}
    # the line grid walk (add_src/lineIterator.cpp): cells per walk and their CRC
    li = C.CDLL(os.path.join(rdir, "libref_lineiterator.so"))
    li.ref_line_iterator_walk.argtypes = [C.c_double] * 4 + [C.c_void_p, C.c_int]
    cases = T.walk_cases()
    a = np.zeros((4096, 2), np.int32)
    counts, crcs = [], []
    for c in cases:
        n = li.ref_line_iterator_walk(*[float(v) for v in c], a.ctypes.data, 4096)
        counts.append(n)
        crcs.append(T.crc(a[:n]))
    out.update(walk_cases_crc=T.crc(cases), walk_counts=np.array(counts, np.int32), walk_crc=np.array(crcs, np.uint32))
    # nfa() / log_gamma() (Thirdparty/line_descriptor/src/ED_Lib/NFA.cpp)
    nfa = C.CDLL(os.path.join(rdir, "libref_nfa.so"))
    nfa.ref_log_gamma.argtypes, nfa.ref_log_gamma.restype = [C.c_double], C.c_double
    nfa.ref_nfa.argtypes, nfa.ref_nfa.restype = [C.c_int, C.c_int, C.c_double, C.c_double], C.c_double
    xs, nk = T.log_gamma_args(), T.nfa_cases()
    out.update(nfa_inputs_crc=T.crc(xs, nk), lgamma_ref=np.array([nfa.ref_log_gamma(float(x)) for x in xs]),
               nfa_ref=np.array([nfa.ref_nfa(*T.nfa_args(i, n, k)) for i, (n, k) in enumerate(nk)]),
               nfa_exact_ref=np.array([nfa.ref_nfa(n, k, p, T.LOGNTS[0]) for n, k, p in T.NFA_EXACT]))
    # BowVector / FeatureVector accumulation (Thirdparty/DBoW2), fed the oracle's (word, weight, node) stream
    db = C.CDLL(os.path.join(rdir, "libref_dbow2.so"))
    db.ref_bow_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_void_p]
    for case, (o, n) in enumerate(T.bow_inputs()):
        m = max(n, 1)
        bow_id, bow_val = np.zeros(m, np.int32), np.zeros(m, np.float64)
        fv_node, fv_start, fv_idx = np.zeros(m, np.int32), np.zeros(m + 1, np.int32), np.zeros(m, np.int32)
        nf = C.c_int()
        w, wt, nid = (np.ascontiguousarray(o[key]) for key in ("word", "weight", "nid"))
        nb = db.ref_bow_accumulate(w.ctypes.data, wt.ctypes.data, nid.ctypes.data, n, bow_id.ctypes.data, bow_val.ctypes.data, fv_node.ctypes.data,
                                   fv_start.ctypes.data, fv_idx.ctypes.data, C.byref(nf))
        nf = nf.value
        out.update({f"bow{case}_in_crc": T.crc(w, wt, nid), f"bow{case}_id": bow_id[:nb], f"bow{case}_val": bow_val[:nb],
                    f"bow{case}_fv_node": fv_node[:nf], f"bow{case}_fv_start": fv_start[:nf + 1], f"bow{case}_fv_idx": fv_idx[:fv_start[nf]]})
    np.savez_compressed(os.path.join(HERE, "ref_pins.npz"), **out)
    print("ref", len(cases), int(out["walk_counts"].sum()), len(xs), len(nk))


def bow_edge_pins():
    """bow_edge_pins.npz: the reference's BowVector / FeatureVector accumulation (oracle/_ref/libref_dbow2.so) on the (word, weight,
    node) streams of the bow_cases cases below: one word 4096 times, two words 2048 times each, segments across ranks 255 | 256 and
    511 | 512, every feature stopped.  Outputs and input CRCs only; tests/test_oracle_ref_cpu.py holds the oracle to them."""
    import ctypes as C
    import bow_cases as bc
    import ref_cases as T
    db = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_dbow2.so"))
    db.ref_bow_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_void_p]
    out = {}
    for name in T.BOW_EDGE_CASES:
        o = bc.oracle(name)
        n = len(o["word"])
        bow_id, bow_val = np.zeros(n, np.int32), np.zeros(n, np.float64)
        fv_node, fv_start, fv_idx = np.zeros(n, np.int32), np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
        nf = C.c_int()
        w, wt, nid = (np.ascontiguousarray(o[key]) for key in ("word", "weight", "nid"))
        nb = db.ref_bow_accumulate(w.ctypes.data, wt.ctypes.data, nid.ctypes.data, n, bow_id.ctypes.data, bow_val.ctypes.data, fv_node.ctypes.data,
                                   fv_start.ctypes.data, fv_idx.ctypes.data, C.byref(nf))
        nf = nf.value
        out.update({f"{name}_in_crc": T.crc(w, wt, nid), f"{name}_id": bow_id[:nb], f"{name}_val": bow_val[:nb], f"{name}_fv_node": fv_node[:nf],
                    f"{name}_fv_start": fv_start[:nf + 1], f"{name}_fv_idx": fv_idx[:fv_start[nf]]})
        print("bow_edge", name, n, nb, nf)
    np.savez_compressed(os.path.join(HERE, "bow_edge_pins.npz"), **out)


def pose_pins():
    """pose_restatement_pins.npz: what pose_opt_cases.optimize and pose_lil_cases.optimize return on every case of their CASE_NAMES in
    both orders (tests/test_pose_lil_cpu.py compares the restatement with it bit for bit).  Written from the two separate drivers the
    restatement had before they became one; written again, it only pins the restatement against itself."""
    import pose_lil_cases as lc
    import pose_opt_cases as pc
    out = {}

    def put(key, pose, flags, ngood, info, margin):
        out[key + "/pose"] = np.frombuffer(pose.tobytes(), np.uint8)
        for k, f in flags.items():
            out[f"{key}/{k}"] = np.zeros(0, np.uint8) if f is None else np.asarray(f, np.uint8)
            out[f"{key}/{k}_none"] = np.bool_(f is None)
        out[key + "/ngood"], out[key + "/info"], out[key + "/margin"] = np.int32(ngood), np.frombuffer(info.tobytes(), np.uint8), np.float64(margin)

    for nm in pc.CASE_NAMES:
        c = pc.case(nm)
        for order in ("device", "edge"):
            pose, outlier, ngood, info, margin = pc.optimize(c["Tcw"], c["edges"], c["cam"], order)
            put(f"points/{nm}/{order}", pose, {"outlier": outlier}, ngood, info, margin)
    for nm in lc.CASE_NAMES:
        c = lc.case(nm)
        for order in ("device", "edge"):
            pose, outlier, outlier_lil, ngood, info, margin = lc.optimize(c["Tcw"], c["edges"], c["lil"], c["cam"], order)
            put(f"lil/{nm}/{order}", pose, {"outlier": outlier, "outlier_lil": outlier_lil}, ngood, info, margin)
    np.savez_compressed(os.path.join(HERE, "pose_restatement_pins.npz"), **out)
    print("pose_pins", len(pc.CASE_NAMES), len(lc.CASE_NAMES), len(out))


def sim3_pins():
    """sim3_restatement_pins.npz: what sim3_opt_cases.optimize returns on every case of its CASE_NAMES in both orders
    (tests/test_sim3_opt_cpu.py compares the restatement with it bit for bit).  Written from the restatement while it had its own
    copy of the iterations and trials and its own solve7; written again, it only pins the restatement against itself."""
    import sim3_opt_cases as sc
    out = {}
    for nm in sc.CASE_NAMES:
        c = sc.case(nm)
        for order in ("device", "edge"):
            S, bad, nin, info, margin = sc.run_case(c, order)
            key = f"{nm}/{order}"
            out[key + "/S12_out"], out[key + "/bad"] = np.frombuffer(S.tobytes(), np.uint8), np.asarray(bad, np.uint8)
            out[key + "/nin"], out[key + "/info"], out[key + "/margin"] = np.int32(nin), np.frombuffer(info.tobytes(), np.uint8), np.float64(margin)
    np.savez_compressed(os.path.join(HERE, "sim3_restatement_pins.npz"), **out)
    print("sim3_pins", len(sc.CASE_NAMES), len(out))


if __name__ == "__main__":
    which = sys.argv[1:] or ["lines", "main", "glue"]
    if "pose_pins" in which:
        pose_pins()
    if "sim3_pins" in which:
        sim3_pins()
    if "ref" in which:
        ref()
    if "bow_edge_pins" in which:
        bow_edge_pins()
    if "lines" in which:
        lines()
    if "main" in which:
        main()
    if "glue" in which:
        glue()
