"""Frame::ComputeBoW restated in plain Python, and the named cases of the ComputeBoW edge tests.

py_transform()   DBoW2 TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup) with TF_IDF weights and L1_NORM
                 scoring, the vocabulary's settings: the tree descent, BowVector::addWeight / normalize(L1) and
                 FeatureVector::addFeature, statement by statement.  Only the Hamming distances of one feature to the children of
                 one node are a numpy expression.  Python floats are IEEE f64, as WordValue is.
case(name)       one of CASE_NAMES: a vocabulary (TREES), descriptors, a levelsup and a check on the oracle's output that the case is
                 what its name says (K = the number of features that are kept, i.e. whose word is not stopped).

The count cases are selections from a pool of random descriptors whose words the oracle reported (select()), on a vocabulary of
4096 leaves: random descriptors alone give no control over K, the multiplicities or the ranks at which a word's features lie.  The
tree cases have hand-made vocabularies.  Nothing here imports product code; the oracle (oracle/bow_oracle.cpp) is used to learn the
words of the pool, never as the answer of a check on itself: the checks are conditions on its output, recomputed from the tree."""
import functools

import numpy as np

import bow_vocab

FIELDS = ("word", "weight", "nid", "bow_id", "bow_val", "fv_node", "fv_start", "fv_idx")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(f, nodes):
    """FORB::distance of one descriptor to each row of nodes"""
    return _POP[np.bitwise_xor(np.asarray(nodes, np.uint8).reshape(-1, 32), f)].sum(1)


def py_transform(vocab, desc, levelsup):
    """-> per feature (word, weight, nid); BowVector {word: value}; FeatureVector {node: [feature indices]}.

    nid is the node met at level L - levelsup; when that level is 0 or less it is 0, the root, as the reference says
    (TemplatedVocabulary.h, the descent: `if(nid_level <= 0 && nid != NULL) *nid = 0; // root`).  A feature whose leaf lies above
    level L - levelsup > 0 never meets that level: the reference leaves nid unset then (the descent's only other assignment is
    `if(nid != NULL && current_level == nid_level) *nid = final_id;`, and transform declares `NodeId nid;` without a value) and files the
    feature under whatever the variable holds.  0 is this project's choice for that unset value."""
    children, nd, nw, nwd, L = vocab
    bow, fv = {}, {}
    per = []
    for i, f in enumerate(desc):
        node, lvl, nid = 0, 0, 0
        while len(children[node]):
            lvl += 1
            ch = children[node]
            d = hamming(f, nd[np.asarray(ch)])
            node = int(ch[int(np.argmin(d))])      # the first minimum in child order: `if(d < best_d)`
            if lvl == L - levelsup:
                nid = node
        word, w = int(nwd[node]), float(nw[node])
        per.append((word, w, nid))
        if w > 0:
            if word in bow:
                bow[word] += w
            else:
                bow[word] = w
            fv.setdefault(nid, []).append(i)
    norm = 0.0
    for k in sorted(bow):
        norm += abs(bow[k])
    if norm > 0:
        for k in bow:
            bow[k] /= norm
    return per, bow, fv


def py_fields(vocab, desc, levelsup):
    """py_transform flattened to the fields of oracle_lib.compute_bow"""
    per, bow, fv = py_transform(vocab, desc, levelsup)
    start, idx = [0], []
    for nd in sorted(fv):
        idx += fv[nd]
        start.append(len(idx))
    return dict(word=np.array([p[0] for p in per], np.int32), weight=np.array([p[1] for p in per], np.float64),
                nid=np.array([p[2] for p in per], np.int32), bow_id=np.array(sorted(bow), np.int32),
                bow_val=np.array([bow[k] for k in sorted(bow)], np.float64), fv_node=np.array(sorted(fv), np.int32),
                fv_start=np.array(start, np.int32), fv_idx=np.array(idx, np.int32))


def seq_sum(w, m):
    """BowVector::addWeight m times on one word: the weight added once per occurrence"""
    v = w
    for _ in range(m - 1):
        v += w
    return v


# ---- the vocabularies -------------------------------------------------------------------------------------------------------
def _flat_tree(children, seed, stopped_every=0):
    """random descriptors; leaves numbered as words in node order; positive weights, every stopped_every-th word stopped"""
    rng = np.random.default_rng(seed)
    nn = len(children)
    nd = rng.integers(0, 256, (nn, 32), dtype=np.uint8)
    nwd, nw = np.zeros(nn, np.int32), np.zeros(nn, np.float64)
    w = 0
    for i in range(nn):
        if not len(children[i]):
            nwd[i] = w
            nw[i] = 0.0 if stopped_every and w % stopped_every == 3 else float(rng.uniform(0.1, 9.0))
            w += 1
    return nd, nw, nwd


def _root_tree(k, seed, stopped_every=7):
    children = [list(range(1, k + 1))] + [[] for _ in range(k)]
    return (children,) + _flat_tree(children, seed, stopped_every if k >= 8 else 0) + (1,)


def _chain_tree():
    children = [[i + 1] for i in range(32)] + [[]]
    return (children,) + _flat_tree(children, 41) + (32,)


TWINS = ((3, 67), (0, 128), (5, 6))      # child positions of the root with equal descriptors


def _twins_tree():
    children, nd, nw, nwd, L = _root_tree(129, 42, 0)
    for c, c2 in TWINS:
        nd[1 + c2] = nd[1 + c]
    return children, nd, nw, nwd, L


COMPLEMENT_Q = np.random.default_rng(43).integers(0, 256, 32, dtype=np.uint8)


def _complement_tree():
    """root -> 1, 2; 1 -> 3; 2 -> 4.  Node 1 is the complement of COMPLEMENT_Q (distance 256), node 2 differs from it in one bit
    (255, wins); node 4, the only child of node 2, is the complement again: the winning child at distance 256."""
    children = [[1, 2], [3], [4], [], []]
    nd, nw, nwd = _flat_tree(children, 44)
    nd[1] = ~COMPLEMENT_Q
    nd[2] = ~COMPLEMENT_Q
    nd[2, 0] ^= 1
    nd[4] = ~COMPLEMENT_Q
    return children, nd, nw, nwd, 2


def _early_leaf_tree():
    """L = 5: 4 nodes at level 1, 3 children each; every third node of level 2 is a leaf, and of the 3 children of the others one
    is a leaf at level 3; the rest go on with 2 children per node to level 5."""
    children, depth = [[]], [0]

    def grow(parent, k):
        for _ in range(k):
            children.append([])
            depth.append(depth[parent] + 1)
            children[parent].append(len(children) - 1)

    grow(0, 4)
    for nd in list(children[0]):
        grow(nd, 3)
    lvl2 = [i for i, d in enumerate(depth) if d == 2]
    for j, nd in enumerate(lvl2):
        if j % 3 != 0:
            grow(nd, 3)
    lvl3 = [i for i, d in enumerate(depth) if d == 3]
    for j, nd in enumerate(lvl3):
        if j % 3 != 1:
            grow(nd, 2)
    for lvl in (4,):
        for nd in [i for i, d in enumerate(depth) if d == lvl]:
            grow(nd, 2)
    return (children,) + _flat_tree(children, 45, 9) + (5,)


def _big_tree(k=10, L=5, seed=46):
    """complete k-ary tree in breadth-first numbering, written as arrays: node i has the children k i + 1 .. k i + k; the
    (k^L - 1) / (k - 1) inner nodes come first.  k = 10, L = 5: 111,111 nodes, 100,000 words."""
    rng = np.random.default_rng(seed)
    inner = (k ** L - 1) // (k - 1)
    nn = inner + k ** L
    child_count = np.where(np.arange(nn) < inner, k, 0).astype(np.int32)
    child_begin = np.arange(nn, dtype=np.int64) * k + 1
    children = [range(int(b), int(b) + int(c)) for b, c in zip(child_begin, child_count)]
    nd = rng.integers(0, 256, (nn, 32), dtype=np.uint8)
    nwd = np.maximum(np.arange(nn, dtype=np.int32) - inner, 0)
    nw = np.where(np.arange(nn) < inner, 0.0, np.where(rng.random(nn) < 0.05, 0.0, rng.uniform(0.1, 9.0, nn)))
    return children, nd, nw, nwd, L


def _count_tree():
    return bow_vocab.make_vocab(8, 4, seed=21)


def _shared_words_tree():
    """the count tree with 64 leaves to a word: few words under many nodes (split_few_words)"""
    children, nd, nw, nwd, L = _count_tree()
    leaf = np.array([not c for c in children])
    word = nwd // 64
    wt = np.random.default_rng(47).uniform(0.1, 9.0, 64)
    wt[5] = 0.0
    return children, nd, np.where(leaf, wt[word], 0.0), np.where(leaf, word, 0).astype(np.int32), L


TREES = {"count": _count_tree, "shared_words": _shared_words_tree, "chain32": _chain_tree, "twins": _twins_tree,
         "complement": _complement_tree, "wide1000": lambda: _root_tree(1000, 48), "levels": lambda: bow_vocab.make_vocab(5, 3, seed=31),
         "early_leaf": _early_leaf_tree, "big": _big_tree}
ROOT_COUNTS = (1, 63, 64, 65, 128, 129)
for _k in ROOT_COUNTS:
    TREES[f"root{_k}"] = functools.partial(_root_tree, _k, 50 + _k)


@functools.lru_cache(maxsize=None)
def vocab(tree):
    return TREES[tree]()


def depths(children):
    d = np.zeros(len(children), np.int32)
    for i, ch in enumerate(children):     # parents come before their children in every tree here
        for c in ch:
            d[c] = d[i] + 1
    return d


# ---- the pool and the selection -----------------------------------------------------------------------------------------------
POOL = 32768


@functools.lru_cache(maxsize=None)
def pool():
    """random descriptors on the count tree (every 8th a copy of a leaf descriptor: distance 0) and what the oracle says of them"""
    import oracle_lib
    v = vocab("count")
    rng = np.random.default_rng(77)
    desc = rng.integers(0, 256, (POOL, 32), dtype=np.uint8)
    leaves = [i for i, c in enumerate(v[0]) if not c]
    desc[::8] = v[1][rng.choice(leaves, len(desc[::8]))]
    o = oracle_lib.compute_bow(*v, desc, 0)
    order = np.argsort(o["word"], kind="stable")
    words, first = np.unique(o["word"][order], return_index=True)
    members = dict(zip((int(w) for w in words), np.split(order, first[1:])))
    kept = [int(w) for w in words if o["weight"][members[int(w)][0]] > 0]
    stopped = [int(w) for w in words if not o["weight"][members[int(w)][0]] > 0]
    return dict(desc=desc, word=o["word"], weight=o["weight"], nid=o["nid"], members=members, kept=kept, stopped=stopped)


def select(pool_result, want):
    """want: (word, count) in feature order -> pool indices.  A word met again goes on through the pool's features of that word,
    and starts over when they run out.  A word the pool has no feature of is a KeyError: enlarge the pool."""
    cursor, idx = {}, []
    for w, m in want:
        have = pool_result["members"][int(w)]
        for _ in range(int(m)):
            c = cursor.get(w, 0)
            idx.append(int(have[c % len(have)]))
            cursor[w] = c + 1
    return np.array(idx, np.int64)


def _stopped_want(p, m):
    return [(p["stopped"][j % len(p["stopped"])], 1) for j in range(m)]


def _shuffled(want, seed):
    return [want[j] for j in np.random.default_rng(seed).permutation(len(want))]


class Case:
    def __init__(self, name, tree, desc, levelsup, check):
        self.name, self.tree, self.levelsup, self._check = name, tree, int(levelsup), check
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)

    def __repr__(self):
        return self.name

    @property
    def vocab(self):
        return vocab(self.tree)

    def check(self, o):
        """asserts on the oracle's (or anybody's) output o that the case is what its name says"""
        assert len(o["word"]) == len(self.desc)
        self._check(self, o)


def kept_count(o):
    return int((o["weight"] > 0).sum())


def multiplicities(o):
    """the multiset of the kept words' multiplicities, ascending"""
    return sorted(np.unique(o["word"][o["weight"] > 0], return_counts=True)[1].tolist())


def segments(keys):
    """(first rank, length) of each run of equal keys after sorting: the segments psl_bow_group finds"""
    _, first, count = np.unique(np.sort(keys), return_index=True, return_counts=True)
    return list(zip(first.tolist(), count.tolist()))


def _count_case(name, want, levelsup, check):
    p = pool()
    return Case(name, "count", p["desc"][select(p, want)], levelsup, check)


def _chk_counts(n, K=None, mult=None, nbow=None, nfv=None):
    def check(case, o):
        assert len(o["word"]) == n
        if K is not None:
            assert kept_count(o) == K
        if mult is not None:
            assert multiplicities(o) == mult
        if nbow is not None:
            assert len(o["bow_id"]) == nbow
        if nfv is not None:
            assert len(o["fv_node"]) == nfv
    return check


def _random_n(n):
    def check(case, o):
        K = kept_count(o)
        assert len(o["word"]) == n and K <= n
        if n >= 255:    # K after the stop words differs from n, and the two passes differ in their group counts
            assert 0 < K < n and len(o["fv_node"]) != len(o["bow_id"])
    p = pool()
    idx = np.random.default_rng(100 + n).permutation(POOL)[:n]
    return Case(f"n{n}", "count", p["desc"][idx], 2, check)


def _n4096_distinct():
    p = pool()
    want = [(w, 1) for w in p["kept"][:3000]] + _stopped_want(p, 1096)
    return _count_case("n4096_distinct", _shuffled(want, 1), 0, _chk_counts(4096, K=3000, mult=[1] * 3000, nbow=3000, nfv=3000))


def _n513_distinct():
    p = pool()
    want = [(w, 1) for w in p["kept"][100:613]]
    return _count_case("n513_distinct", _shuffled(want, 2), 2, _chk_counts(513, K=513, mult=[1] * 513, nbow=513))


def one_word_id():
    """the first kept word of the pool whose weight added 4096 times is not 4096 times the weight"""
    p = pool()
    for w in p["kept"]:
        wt = float(p["weight"][p["members"][w][0]])
        if seq_sum(wt, 4096) != 4096 * wt:
            return w
    raise AssertionError("no weight of the pool tells a sum from a product")


def two_word_ids():
    """the first two kept words, 2048 times each, whose normalised values differ between sums and products of their weights"""
    p = pool()
    ws = p["kept"][:40]
    wt = {w: float(p["weight"][p["members"][w][0]]) for w in ws}
    for a in ws:
        for b in ws:
            if a < b:
                sa, sb, pa, pb = seq_sum(wt[a], 2048), seq_sum(wt[b], 2048), 2048 * wt[a], 2048 * wt[b]
                if (sa / (sa + sb), sb / (sa + sb)) != (pa / (pa + pb), pb / (pa + pb)):
                    return a, b
    raise AssertionError("no pair of weights of the pool tells sums from products")


def _one_word():
    def check(case, o):
        _chk_counts(4096, K=4096, mult=[4096], nbow=1, nfv=1)(case, o)
        assert o["bow_val"].tolist() == [1.0]
    return _count_case("one_word", [(one_word_id(), 4096)], 2, check)


def _two_words():
    a, b = two_word_ids()
    return _count_case("two_words", [(a, 1), (b, 1)] * 2048, 2, _chk_counts(4096, K=4096, mult=[2048, 2048], nbow=2))


def _all_stopped(n):
    def check(case, o):
        _chk_counts(n, K=0, mult=[], nbow=0, nfv=0)(case, o)
        assert o["fv_start"].tolist() == [0] and len(o["fv_idx"]) == 0
    return _count_case(f"all_stopped_{n}", _stopped_want(pool(), n), 2, check)


def _k1(where):
    p = pool()
    at = 0 if where == "first" else 299
    want = _stopped_want(p, 299)
    want.insert(at, (p["kept"][7], 1))

    def check(case, o):
        _chk_counts(300, K=1, mult=[1], nbow=1, nfv=1)(case, o)
        assert np.flatnonzero(o["weight"] > 0).tolist() == [at] and o["fv_idx"].tolist() == [at]
    return _count_case(f"k1_{where}", want, 2, check)


def _k_of_400(K):
    p = pool()
    rng = np.random.default_rng(300 + K)
    gaps = np.linspace(0, 399, 400 - K).astype(int)       # the stopped features, spread over the frame
    assert len(set(gaps.tolist())) == 400 - K
    kept = iter(rng.choice(p["kept"][:120], K))           # 120 words: multiplicities above one
    stop = iter(_stopped_want(p, 400 - K))
    is_stop = np.zeros(400, bool)
    is_stop[gaps] = True
    want = [next(stop) if s else (int(next(kept)), 1) for s in is_stop]

    def check(case, o):
        _chk_counts(400, K=K)(case, o)
        s = np.flatnonzero(~(o["weight"] > 0))
        assert s[0] == 0 and s[-1] == 399 and np.diff(s).max() <= 4      # interleaved
        assert max(multiplicities(o)) > 1
    return _count_case(f"k{K}_of_400", want, 2, check)


STRADDLE_RANKS = ((254, 5), (510, 5))


def _straddle():
    """K = 600 of n = 640: 254 single words, a word five times (ranks 254 .. 258), 251 singles, a word five times (510 .. 514), 85
    singles; levelsup = 0 makes the leaf the node, so the FeatureVector pass has the same segments at the same ranks."""
    p = pool()
    U = p["kept"][:592]
    want = [(w, 1) for w in U[:254]] + [(U[254], 5)] + [(w, 1) for w in U[255:506]] + [(U[506], 5)] + [(w, 1) for w in U[507:]]
    want = [(w, 1) for w, m in want for _ in range(m)] + _stopped_want(p, 40)

    def check(case, o):
        _chk_counts(640, K=600, mult=[1] * 590 + [5, 5], nbow=592, nfv=592)(case, o)
        keep = o["weight"] > 0
        for keys in (o["word"][keep], o["nid"][keep]):
            seg = segments(keys)
            assert [s for s in seg if s[1] > 1] == list(STRADDLE_RANKS)
        assert all(int(o["fv_start"][g + 1] - o["fv_start"][g]) == 5 for g in (254, 506))
    return _count_case("straddle", _shuffled(want, 3), 0, check)


def _split(which):
    rng = np.random.default_rng(8)
    desc = pool()["desc"][rng.permutation(POOL)[:1000]]
    if which == "few_words":     # levelsup = 0: the node is the leaf; 64 leaves share a word
        def check(case, o):
            assert len(o["fv_node"]) - len(o["bow_id"]) > 256 and len(o["bow_id"]) > 1
        return Case("split_few_words", "shared_words", desc, 0, check)

    def check(case, o):          # levelsup = L: the only node is the root
        assert len(o["bow_id"]) - len(o["fv_node"]) > 256 and o["fv_node"].tolist() == [0]
    return Case("split_few_nodes", "count", desc, 4, check)


# ---- the tree cases -----------------------------------------------------------------------------------------------------------
def _flip(d, bits, rng):
    d = d.copy()
    for b in rng.choice(256, bits, replace=False):
        d[b >> 3] ^= 1 << (b & 7)
    return d


def _root_case(k):
    children, nd, nw, nwd, L = vocab(f"root{k}")
    rng = np.random.default_rng(60 + k)
    desc = np.concatenate([nd[1:], rng.integers(0, 256, (40, 32), dtype=np.uint8)])

    def check(case, o):
        assert len(case.vocab[0][0]) == k and (o["word"][:k] == np.arange(k)).all()      # every child position wins once
    return Case(f"root_{k}_children", f"root{k}", desc, 0, check)


def _chain(levelsup):
    rng = np.random.default_rng(70)

    def check(case, o):
        ch = case.vocab[0]
        assert len(ch) == 33 and all(len(c) == 1 for c in ch[:32]) and case.vocab[4] == 32
        assert (o["nid"] == 32 - levelsup).all() and (o["word"] == 0).all() and kept_count(o) == len(o["word"])
    return Case(f"chain32_levelsup{levelsup}", "chain32", rng.integers(0, 256, (6, 32), dtype=np.uint8), levelsup, check)


def _twins(c, c2, name):
    children, nd, nw, nwd, L = vocab("twins")
    rng = np.random.default_rng(80 + c)
    desc = np.array([_flip(nd[1 + c], bits, rng) for bits in (0, 1, 2, 3, 8, 21, 40)], np.uint8)

    def check(case, o):
        for f, w in zip(case.desc, o["word"]):
            d = hamming(f, nd[1:])
            assert d[c] == d[c2] == d.min() and (d == d.min()).sum() == 2
            assert w == nwd[1 + c] != nwd[1 + c2]
    return Case(name, "twins", desc, 0, check)


def _dist_0():
    children, nd, nw, nwd, L = vocab("root64")

    def check(case, o):
        for f, w in zip(case.desc, o["word"]):
            d = hamming(f, nd[1:])
            assert d.min() == 0 and nwd[1 + int(np.argmin(d))] == w
    return Case("dist_0", "root64", nd[1:][::-1], 0, check)


def _dist_256():
    children, nd, nw, nwd, L = vocab("complement")
    rng = np.random.default_rng(90)
    desc = np.array([COMPLEMENT_Q] * 3 + [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(3)], np.uint8)

    def check(case, o):
        q = case.desc[0]
        assert hamming(q, nd[[1, 2]]).tolist() == [256, 255] and children[2] == [4] and hamming(q, nd[[4]]).tolist() == [256]
        assert (o["word"][:3] == nwd[4]).all() and (o["nid"][:3] == 2).all()
    return Case("dist_256", "complement", desc, 1, check)


def _wide():
    children, nd, nw, nwd, L = vocab("wide1000")
    at = [0, 63, 64, 65, 127, 128, 959, 960, 999]
    rng = np.random.default_rng(91)
    desc = np.concatenate([nd[1:][at], rng.integers(0, 256, (100, 32), dtype=np.uint8)])

    def check(case, o):
        assert len(children[0]) == 1000 and o["word"][:len(at)].tolist() == at and len(set(o["word"].tolist())) > 60
    return Case("wide_1000", "wide1000", desc, 0, check)


def _levels(levelsup, name):
    children, nd, nw, nwd, L = vocab("levels")
    assert L == 3
    rng = np.random.default_rng(92)
    desc = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    leaves = [i for i, c in enumerate(children) if not c]
    desc[::2] = nd[rng.choice(leaves, 100)]
    leaf_of_word = {int(nwd[i]): i for i in leaves}

    def check(case, o):
        if levelsup == 0:
            assert [leaf_of_word[int(w)] for w in o["word"]] == o["nid"].tolist()
        elif levelsup < L:
            d = depths(children)
            assert (d[o["nid"]] == L - levelsup).all() and len(o["fv_node"]) > 1
        else:
            assert not o["nid"].any() and o["fv_node"].tolist() == [0] and kept_count(o) > 0
    return Case(name, "levels", desc, levelsup, check)


def _early_leaf(levelsup):
    children, nd, nw, nwd, L = vocab("early_leaf")
    rng = np.random.default_rng(93)
    desc = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    leaves = [i for i, c in enumerate(children) if not c]
    desc[::3] = nd[rng.choice(leaves, 100)]
    d = depths(children)
    leaf_of_word = {int(nwd[i]): i for i in leaves}

    def check(case, o):
        assert L == 5 and {2, 3, 5} == set(d[leaves].tolist())
        zero = o["nid"] == 0
        assert 1 <= zero.sum() < len(zero)
        depth = np.array([d[leaf_of_word[int(w)]] for w in o["word"]])
        assert (zero == (depth < L - levelsup)).all()       # exactly the features that end above level L - levelsup
        assert (zero & (o["weight"] > 0)).any() and o["fv_node"][0] == 0 and len(o["fv_node"]) > 1
    return Case(f"early_leaf_levelsup{levelsup}", "early_leaf", desc, levelsup, check)


def _big(levelsup, name):
    rng = np.random.default_rng(94)
    desc = rng.integers(0, 256, (500, 32), dtype=np.uint8)

    def check(case, o):
        children, nd, nw, nwd, L = case.vocab
        assert len(children) == 111111 and int(nwd.max()) == 99999
        assert int(o["word"].max()) > 65535 and int(o["bow_id"].max()) > 65535
        if levelsup == 0:
            assert int(o["fv_node"].max()) > 65535
    return Case(name, "big", desc, levelsup, check)


_BUILDERS = {}
for _n in (1, 2, 255, 256, 257, 511, 512, 513, 4095):
    _BUILDERS[f"n{_n}"] = functools.partial(_random_n, _n)
_BUILDERS.update({
    "n4096_distinct": _n4096_distinct, "one_word": _one_word,      # one_word is the second n = 4096 form: every feature in one word
    "n513_distinct": _n513_distinct,
    "all_stopped_1": functools.partial(_all_stopped, 1), "all_stopped_300": functools.partial(_all_stopped, 300),
    "k1_first": functools.partial(_k1, "first"), "k1_last": functools.partial(_k1, "last"),
    "k255_of_400": functools.partial(_k_of_400, 255), "k256_of_400": functools.partial(_k_of_400, 256),
    "k257_of_400": functools.partial(_k_of_400, 257),
    "straddle": _straddle, "two_words": _two_words,
    "split_few_words": functools.partial(_split, "few_words"), "split_few_nodes": functools.partial(_split, "few_nodes")})
for _k in ROOT_COUNTS:
    _BUILDERS[f"root_{_k}_children"] = functools.partial(_root_case, _k)
_BUILDERS.update({
    "chain32_levelsup4": functools.partial(_chain, 4), "chain32_levelsup31": functools.partial(_chain, 31),
    "twins_64_apart_3_67": functools.partial(_twins, 3, 67, "twins_64_apart_3_67"),
    "twins_64_apart_0_128": functools.partial(_twins, 0, 128, "twins_64_apart_0_128"),
    "twins_adjacent_lanes": functools.partial(_twins, 5, 6, "twins_adjacent_lanes"),
    "dist_0": _dist_0, "dist_256": _dist_256, "wide_1000": _wide,
    "levelsup_0": functools.partial(_levels, 0, "levelsup_0"), "levelsup_L-1": functools.partial(_levels, 2, "levelsup_L-1"),
    "levelsup_L": functools.partial(_levels, 3, "levelsup_L"), "levelsup_L+1": functools.partial(_levels, 4, "levelsup_L+1"),
    "levelsup_40": functools.partial(_levels, 40, "levelsup_40"),
    "early_leaf_levelsup1": functools.partial(_early_leaf, 1), "early_leaf_levelsup2": functools.partial(_early_leaf, 2),
    "ids_above_16_bits": functools.partial(_big, 4, "ids_above_16_bits"),
    "ids_above_16_bits_nodes": functools.partial(_big, 0, "ids_above_16_bits_nodes")})
CASE_NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    assert c.name == name
    return c


@functools.lru_cache(maxsize=None)
def oracle(name, levelsup=None):
    """the oracle's output on a case (at another levelsup: the batched launches have one for all their frames); shared, read-only"""
    import oracle_lib
    c = case(name)
    o = oracle_lib.compute_bow(*c.vocab, c.desc, c.levelsup if levelsup is None else levelsup)
    for a in o.values():
        a.setflags(write=False)
    return o
