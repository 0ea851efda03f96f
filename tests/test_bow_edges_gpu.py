"""Frame::ComputeBoW on the device (psl-slam_amd/csrc/pslfe_bow.hip: k_bow_descend, k_bow_vectors) at its count, tree, stop-word and
batch edges: the cases of tests/bow_cases.py through the host form and through the batched device form against the CPU oracle, which
tests/test_bow_cases_cpu.py holds to the plain-Python restatement on the same cases.  Every comparison is exact: integer arrays as
arrays, f64 values as bytes.  Every case's own check (that it reaches the edge it is named after) is asserted on the device's output."""
import ctypes as C

import numpy as np
import pytest

import bow_cases as bc

pytestmark = pytest.mark.gpu

_V = {}


def _vocab(P, tree):
    """one vocabulary object per tree, shared by its cases"""
    if tree not in _V:
        _V[tree] = P.ORBVocabulary(*bc.vocab(tree))
    return _V[tree]


def _same(got, ref, what=""):
    for key in bc.FIELDS:
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape, (what, key)
        if got[key].dtype == np.float64:
            assert got[key].tobytes() == ref[key].tobytes(), (what, key)
        else:
            np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")


# ---- (a) the host form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_host_form_equals_oracle(name):
    import psl_slam_amd as P
    c = bc.case(name)
    got = _vocab(P, c.tree).transform(c.desc, c.levelsup)
    _same(got, bc.oracle(name), name)
    c.check(got)


# ---- (b) the batched form -------------------------------------------------------------------------------------------------------
OUTPUTS = (("fword", np.int32, 0), ("fweight", np.float64, 0), ("fnid", np.int32, 0), ("bow_id", np.int32, 0), ("bow_val", np.float64, 0),
           ("bow_start", np.int32, 1), ("nbow", np.int32, None), ("fv_node", np.int32, 0), ("fv_start", np.int32, 1), ("fv_idx", np.int32, 0),
           ("nfv", np.int32, None))


def _aa(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = 0xAA
    return a


def _is_aa(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xAA).all())


def _download(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def _launch(P, V, descs, counts, stride, levelsup, keep=False):
    """pslfe_compute_bow_device on frames of descs[f] (at most stride rows are stored) with the given counts; every output holds
    0xAA bytes before.  -> {name: array [nframes][...]} and, with keep, the device addresses by name (the caller frees them)"""
    ctx = V.ctx
    nf = len(counts)
    desc = np.full((nf, stride, 32), 0x55, np.uint8)        # rows past a frame's count: not zeros
    for f, d in enumerate(descs):
        desc[f, :min(len(d), stride)] = d[:stride]
    host = {nm: _aa((nf,) if extra is None else (nf, stride + extra), dt) for nm, dt, extra in OUTPUTS}
    dev = {nm: ctx.device_array(a)[0] for nm, a in host.items()}
    dev["desc"], dev["counts"] = ctx.device_array(desc)[0], ctx.device_array(np.asarray(counts, np.int32))[0]
    P._check(P.lib().pslfe_compute_bow_device(V._h, C.c_void_p(dev["desc"]), C.c_void_p(dev["counts"]), nf, stride, levelsup,
                                              *[C.c_void_p(dev[nm]) for nm, _, _ in OUTPUTS]), "pslfe_compute_bow_device")
    ctx.synchronize()
    out = {nm: _download(P, ctx, dev[nm], a) for nm, a in host.items()}
    if keep:
        return out, dev
    for d in dev.values():
        ctx.device_free(d)
    return out


def _bow_start(ref):
    """the start offsets of the BowVector pass: the kept features ranked by word"""
    counts = np.unique(ref["word"][ref["weight"] > 0], return_counts=True)[1]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _check_frame(out, f, n, ref, what):
    """frame f of a launch used n features: all eleven outputs equal ref, every byte past the used extents is still 0xAA"""
    row = {nm: out[nm][f] for nm, _, _ in OUTPUTS}
    nb, nfv = int(row["nbow"]), int(row["nfv"])
    assert n == len(ref["word"]) and nb == len(ref["bow_id"]) and nfv == len(ref["fv_node"]), what
    kept = int(ref["fv_start"][nfv])
    got = dict(word=row["fword"][:n], weight=row["fweight"][:n], nid=row["fnid"][:n], bow_id=row["bow_id"][:nb], bow_val=row["bow_val"][:nb],
               fv_node=row["fv_node"][:nfv], fv_start=row["fv_start"][:nfv + 1], fv_idx=row["fv_idx"][:kept])
    _same(got, ref, what)
    np.testing.assert_array_equal(row["bow_start"][:nb + 1], _bow_start(ref), err_msg=what)
    for nm, used in (("fword", n), ("fweight", n), ("fnid", n), ("bow_id", nb), ("bow_val", nb), ("fv_node", nfv), ("fv_start", nfv + 1),
                     ("fv_idx", kept)):
        assert _is_aa(row[nm][used:]), (what, nm, "written past its extent")
    return row


def _oracle(tree, desc, levelsup):
    import oracle_lib
    return oracle_lib.compute_bow(*bc.vocab(tree), desc, levelsup)


def _launch_and_check(P, tree, descs, counts, stride, levelsup, what, keep=False):
    V = _vocab(P, tree)
    used = [min(max(c, 0), stride) for c in counts]        # the contract of pslfe_compute_bow_device (include/pslfe.h)
    frames = [np.ascontiguousarray(d[:n]).reshape(-1, 32) for d, n in zip(descs, used)]
    refs = [_oracle(tree, d, levelsup) for d in frames]
    res = _launch(P, V, descs, counts, stride, levelsup, keep)
    out = res[0] if keep else res
    for f, (d, n, ref) in enumerate(zip(frames, used, refs)):
        _check_frame(out, f, n, ref, f"{what} frame {f}")
        _same(V.transform(d, levelsup), ref, f"{what} frame {f} host form")
    if len(counts) > 1:     # a frame's result does not depend on its neighbours: the same frames in reverse order
        rev = _launch(P, V, descs[::-1], counts[::-1], stride, levelsup)
        for f in range(len(counts)):
            g = len(counts) - 1 - f
            for nm, _, _ in OUTPUTS:
                a, b = out[nm][f], rev[nm][g]
                if nm == "bow_start":      # scratch past its nbow + 1 entries
                    a, b = a[:int(out["nbow"][f]) + 1], b[:int(rev["nbow"][g]) + 1]
                assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (what, f, nm)
    return res, refs


EMPTY = np.zeros((0, 32), np.uint8)


def _d(name):
    return bc.case(name).desc


def test_batched_one_frame():
    """a single frame at a stride that is its count and no multiple of 4"""
    import psl_slam_amd as P
    _launch_and_check(P, "count", [_d("n257")], [257], 257, 2, "one frame")


def _stride513_frames():
    return [EMPTY, _d("n1"), _d("n513_distinct"), _d("n257"), EMPTY, _d("n512"), _d("k1_first")], [0, 1, 513, 257, 0, 512, 300]


def test_batched_seven_frames_stride_513():
    """counts 0, 1, the stride itself, 257, 0, 512, 300 at a stride of 513: the grid is (513 + 3) / 4 blocks wide"""
    import psl_slam_amd as P
    descs, counts = _stride513_frames()
    (out, refs) = _launch_and_check(P, "count", descs, counts, 513, 2, "stride 513")
    assert out["nbow"][0] == 0 and out["nbow"][2] == 513 and out["nfv"][0] == 0 and out["fv_start"][0, 0] == 0 and out["fv_start"][4, 0] == 0


def test_batched_three_frames_stride_5_small_tree():
    import psl_slam_amd as P
    d = _d("levelsup_0")
    _launch_and_check(P, "levels", [d[:5], d[5:8], EMPTY], [5, 3, 0], 5, 1, "stride 5")


def test_batched_two_frames_stride_4096():
    """PSL_BOW_NMAX features in both frames: 3000 groups of one, and one group of 4096"""
    import psl_slam_amd as P
    (out, refs) = _launch_and_check(P, "count", [_d("n4096_distinct"), _d("one_word")], [4096, 4096], 4096, 0, "stride 4096")
    assert out["nbow"].tolist() == [3000, 1] and out["nfv"].tolist() == [3000, 1] and out["bow_val"][1, 0] == 1.0


def test_batched_counts_outside_the_stride_are_clamped():
    """counts 301, 1000, -1, 300 at stride 300: a count above the stride is the stride, a negative count is an empty frame, and
    nobody's neighbour is touched (the contract in include/pslfe.h)"""
    import psl_slam_amd as P
    rng = np.random.default_rng(5)
    descs = [_d("n512")[:300], _d("n513")[:300], rng.integers(0, 256, (300, 32), dtype=np.uint8), _d("n511")[:300]]
    (out, refs) = _launch_and_check(P, "count", descs, [301, 1000, -1, 300], 300, 2, "clamped counts")
    assert [len(r["word"]) for r in refs] == [300, 300, 0, 300]
    assert out["nbow"][2] == 0 and out["nfv"][2] == 0 and out["fv_start"][2, 0] == 0 and _is_aa(out["fword"][2])


# ---- (c) optional pointers of the host form -------------------------------------------------------------------------------------
def _host_call(P, V, desc, levelsup, skip=None):
    n = len(desc)
    o = dict(word=_aa(n, np.int32), weight=_aa(n, np.float64), nid=_aa(n, np.int32), bow_id=_aa(n, np.int32), bow_val=_aa(n, np.float64),
             fv_node=_aa(n, np.int32), fv_start=_aa(n + 1, np.int32), fv_idx=_aa(n, np.int32))
    p = {k: (None if k == skip else P._ptr(a)) for k, a in o.items()}
    nb, nf = C.c_int(-7), C.c_int(-7)
    rc = P.lib().pslfe_compute_bow(V._h, P._ptr(desc), n, levelsup, p["word"], p["weight"], p["nid"], p["bow_id"], p["bow_val"], C.byref(nb),
                                   p["fv_node"], p["fv_start"], p["fv_idx"], C.byref(nf))
    return rc, o, nb.value, nf.value


@pytest.mark.parametrize("skip", bc.FIELDS)
def test_host_form_optional_pointers(skip):
    """any per-feature or vector pointer may be NULL; the others are what the full call gives, and nothing is written past the
    counts (fv_idx is copied by a count read back from the device)"""
    import psl_slam_amd as P
    c, ref = bc.case("k257_of_400"), bc.oracle("k257_of_400")
    V = _vocab(P, c.tree)
    rc0, full, nb0, nf0 = _host_call(P, V, c.desc, c.levelsup)
    rc, o, nb, nf = _host_call(P, V, c.desc, c.levelsup, skip)
    assert rc0 == rc == 0 and (nb, nf) == (nb0, nf0) == (len(ref["bow_id"]), len(ref["fv_node"]))
    used = dict(word=400, weight=400, nid=400, bow_id=nb, bow_val=nb, fv_node=nf, fv_start=nf + 1, fv_idx=257)
    for k in bc.FIELDS:
        assert full[k][:used[k]].tobytes() == ref[k].tobytes(), k
        assert _is_aa(full[k][used[k]:]), k
        if k == skip:
            assert _is_aa(o[k])
        else:
            assert o[k].tobytes() == full[k].tobytes(), k


# ---- (d) whole-call errors ------------------------------------------------------------------------------------------------------
def _invalid(P, rc, fn):
    assert rc == -1, (fn, rc)        # PSLFE_E_INVALID
    assert fn in P.lib().pslfe_last_error().decode(), (fn, P.lib().pslfe_last_error())


def test_errors_leave_the_handle_usable():
    import psl_slam_amd as P
    c, ref = bc.case("levelsup_L-1"), bc.oracle("levelsup_L-1")
    V = _vocab(P, c.tree)
    ctx, lib = V.ctx, P.lib()
    d_any = ctx.device_array(np.zeros(4096, np.uint8))[0]          # a valid address for every pointer argument; never launched on
    ptrs = [V._h] + [C.c_void_p(d_any)] * 13

    def device_form(nframes=1, stride=8, levelsup=2, null=None):
        p = [None if i == null else x for i, x in enumerate(ptrs)]
        return lib.pslfe_compute_bow_device(p[0], p[1], p[2], nframes, stride, levelsup, *p[3:])

    for kw in (dict(nframes=0), dict(nframes=-1), dict(stride=0), dict(stride=4097), dict(levelsup=-1)):
        _invalid(P, device_form(**kw), "pslfe_compute_bow_device")
    for i in range(14):
        _invalid(P, device_form(null=i), "pslfe_compute_bow_device")
    ctx.device_free(d_any)

    big = np.zeros((4097, 32), np.uint8)
    nb, nf = C.c_int(), C.c_int()
    host = lambda desc, n, levelsup=2: lib.pslfe_compute_bow(V._h, P._ptr(desc), n, levelsup, *[None] * 5, C.byref(nb), None, None, None, C.byref(nf))
    _invalid(P, host(big, 4097), "pslfe_compute_bow")
    _invalid(P, host(big, -1), "pslfe_compute_bow")
    _invalid(P, host(None, 3), "pslfe_compute_bow")
    _invalid(P, host(big, 3, -1), "pslfe_compute_bow")
    _invalid(P, lib.pslfe_compute_bow(None, P._ptr(big), 3, 2, *[None] * 5, C.byref(nb), None, None, None, C.byref(nf)), "pslfe_compute_bow")
    _invalid(P, lib.pslfe_compute_bow(V._h, P._ptr(big), 3, 2, *[None] * 5, None, None, None, None, C.byref(nf)), "pslfe_compute_bow")
    _invalid(P, lib.pslfe_compute_bow(V._h, P._ptr(big), 3, 2, *[None] * 5, C.byref(nb), None, None, None, None), "pslfe_compute_bow")

    # the vocabulary: root -> 1, 2; 1 -> 3, 4
    cb, cc, ids = np.array([0, 2, 4, 4, 4], np.int32), np.array([2, 2, 0, 0, 0], np.int32), np.array([1, 2, 3, 4], np.int32)
    nd, nw, nwd = np.zeros((5, 32), np.uint8), np.ones(5), np.arange(5, dtype=np.int32)

    def create(nnodes=5, cb=cb, cc=cc, ids=ids, L=2):
        h = C.c_void_p()
        rc = lib.pslfe_vocab_create(ctx._h, nnodes, P._ptr(cb), P._ptr(cc), P._ptr(ids), len(ids), P._ptr(nd), P._ptr(nw), P._ptr(nwd), L, C.byref(h))
        if rc == 0:
            lib.pslfe_vocab_destroy(h)
        else:
            assert not h.value
        return rc

    assert create() == 0                                                       # the tree itself is fine
    _invalid(P, create(L=0), "pslfe_vocab_create")
    _invalid(P, create(L=33), "pslfe_vocab_create")
    _invalid(P, create(ids=np.array([1, 2, 3, 0], np.int32)), "pslfe_vocab_create")     # a child link to node 0
    _invalid(P, create(cc=np.array([2, 3, 0, 0, 0], np.int32)), "pslfe_vocab_create")   # a child range past nchild
    _invalid(P, create(cb=np.array([0, 3, 4, 4, 4], np.int32)), "pslfe_vocab_create")
    _invalid(P, create(cc=np.array([0, 2, 0, 0, 0], np.int32)), "pslfe_vocab_create")   # a root without children
    _invalid(P, create(nnodes=1), "pslfe_vocab_create")

    got = V.transform(c.desc, c.levelsup)                                      # the same handle, afterwards
    _same(got, ref, "after the errors")
    c.check(got)


# ---- (e) the chain to the consumers ---------------------------------------------------------------------------------------------
def test_count_equals_stride_row_through_the_keyframe_database():
    """frames 2 and 3 of the stride-513 launch (513 and 257 features; the first has 513 distinct kept words: nbow == stride ==
    max_words) added device to device, queried on the device with frame 5: == kfdb_cases.dense_query on the oracle's BowVectors"""
    import psl_slam_amd as P
    import kfdb_cases as kc
    descs, counts = _stride513_frames()
    stride = 513
    (out, dev), refs = _launch_and_check(P, "count", descs, counts, stride, 2, "stride 513", keep=True)
    ctx = _vocab(P, "count").ctx
    assert out["nbow"][2] == stride
    K = 4
    db = P.KeyFrameDatabase(K, stride, ctx=ctx)
    db.add_device(1, dev["bow_id"] + 2 * stride * 4, dev["bow_val"] + 2 * stride * 8, dev["nbow"] + 2 * 4, 2, stride)      # slots 1, 2
    res = dict(words=_aa(K, np.int32), first=_aa(K, np.int32), score=_aa(K, np.float64), maxc=_aa(1, np.int32))
    d_res = {k: ctx.device_array(a)[0] for k, a in res.items()}
    db.query_device(dev["bow_id"] + 5 * stride * 4, dev["bow_val"] + 5 * stride * 8, dev["nbow"] + 5 * 4, 1, stride, None, d_res["words"],
                    d_res["first"], d_res["score"], d_res["maxc"])
    ctx.synchronize()
    for k, a in res.items():
        _download(P, ctx, d_res[k], a)
    bow = lambda f: (refs[f]["bow_id"], refs[f]["bow_val"])
    dense, rmax = kc.dense_query({1: bow(2), 2: bow(3)}, bow(5))
    rw, rf, rs = np.zeros(K, np.int32), np.full(K, -1, np.int32), np.zeros(K, np.float64)
    for s, (w, f, sc) in dense.items():
        rw[s], rf[s], rs[s] = w, f, sc
    np.testing.assert_array_equal(res["words"], rw)
    np.testing.assert_array_equal(res["first"], rf)
    assert res["score"].tobytes() == rs.tobytes() and res["maxc"][0] == rmax
    assert rw[1] > 10 and rw[2] > 10 and rs[1] > 0
    w1, f1, s1, m1 = db.query(bow(5))                           # the host query on the oracle's vector: the same
    assert (w1 == rw).all() and (f1 == rf).all() and s1.tobytes() == rs.tobytes() and m1 == rmax
    for d in list(dev.values()) + list(d_res.values()):
        ctx.device_free(d)
    db.close()


def test_early_leaf_feature_vector_through_search_by_bow():
    """the FeatureVector of early_leaf at levelsup = 1, node 0 of the early leaves included, is what SearchByBoW takes as it is
    written: the device's runs through pslfe_orb_search_by_bow == the oracle's runs through the oracle's search"""
    import psl_slam_amd as P
    import oracle_lib
    import window_cases as W
    c = bc.case("early_leaf_levelsup1")
    V = _vocab(P, c.tree)
    rng = np.random.default_rng(3)
    dF = c.desc
    dK = dF[rng.permutation(len(dF))[:220]].copy()
    dK[:, 7] ^= 1

    def inputs(oF, oK):
        startF = {int(nd): (int(oF["fv_start"][g]), int(oF["fv_start"][g + 1] - oF["fv_start"][g])) for g, nd in enumerate(oF["fv_node"])}
        runs, qd, nodes = [], [], []
        for g, nd in enumerate(oK["fv_node"]):
            if int(nd) in startF:
                for i in oK["fv_idx"][oK["fv_start"][g]:oK["fv_start"][g + 1]]:
                    runs.append(startF[int(nd)]); qd.append(dK[i]); nodes.append(int(nd))
        return oF["fv_idx"], np.array(runs, np.int32).reshape(-1, 2), np.array(qd, np.uint8).reshape(-1, 32), nodes

    ofidx, oruns, oqd, nodes = inputs(bc.oracle(c.name), oracle_lib.compute_bow(*c.vocab, dK, 1))
    gfidx, gruns, gqd, _ = inputs(V.transform(dF, 1), V.transform(dK, 1))
    np.testing.assert_array_equal(gfidx, ofidx)
    np.testing.assert_array_equal(gruns, oruns)
    np.testing.assert_array_equal(gqd, oqd)
    angle = np.zeros(len(oruns), np.float32)
    kps = W.keypoints(np.stack([rng.uniform(20, 1000, len(dF)), rng.uniform(20, 700, len(dF))], 1))
    g = P.FrameGrid(512, 1, ctx=V.ctx)
    g.set(0, kps, dF, W.BOUNDS)
    nm, match, assigned = P.ORBmatcher(0.9, False).SearchByBoW(g, 0, gfidx, gruns, angle, gqd)
    rnm, rmatch, rassigned = oracle_lib.search_by_bow(dF, kps["angle"], ofidx, oruns, oqd, angle, 0.9, False)
    assert nm == rnm and nm > 50
    np.testing.assert_array_equal(match, rmatch)
    np.testing.assert_array_equal(assigned, rassigned)
    assert any(nd == 0 and m >= 0 for nd, m in zip(nodes, rmatch))      # a match inside the run of node 0, the unset nid
