"""The keyframe database of the reference restated in Python, and the cases of the kfdb tests.

score()                    DBoW2::L1Scoring::score, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68: the merge walk with lower_bound.
                           Python floats are IEEE f64, as WordValue is.
RefKeyFrame / RefKeyFrameDatabase
                           KeyFrameDatabase, src/KeyFrameDatabase.cc:33-309: a real inverted file (word -> list of keyframes in
                           the order of their add), the per-keyframe mnLoopQuery / mnLoopWords / mLoopScore and mnRelocQuery /
                           mnRelocWords / mRelocScore members, and both covisibility tails.  np.float32 wherever the reference says
                           float.  mLoopScore and mRelocScore start at 0.0f: the reference leaves them uninitialised
                           (src/KeyFrame.cc:35), the project defines the value.
dense_*                    the per-slot formulation the device uses (words, first_word, order by (first_word, add sequence)).

A BowVector is a pair (ids int32 ascending, vals float64).  Nothing here is compiled from the reference; parity with
ScoringObject.cpp itself is not pinned."""
from bisect import bisect_left

import numpy as np

F32 = np.float32


def score(v1, v2):
    """L1Scoring::score(v1, v2) -> f64"""
    id1, val1 = [int(x) for x in v1[0]], [float(x) for x in v1[1]]
    id2, val2 = [int(x) for x in v2[0]], [float(x) for x in v2[1]]
    i1, i2, e1, e2 = 0, 0, len(id1), len(id2)
    s = 0.0
    while i1 != e1 and i2 != e2:
        vi, wi = val1[i1], val2[i2]
        if id1[i1] == id2[i2]:
            s += abs(vi - wi) - abs(vi) - abs(wi)
            i1 += 1
            i2 += 1
        elif id1[i1] < id2[i2]:
            i1 = bisect_left(id1, id2[i2])      # v1.lower_bound(v2_it->first)
        else:
            i2 = bisect_left(id2, id1[i1])
    return -s / 2.0


class RefKeyFrame:
    def __init__(self, slot, bow):
        self.slot = slot
        self.mBowVec = (np.asarray(bow[0], np.int32).copy(), np.asarray(bow[1], np.float64).copy())
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = -1, 0, F32(0.0)
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = -1, 0, F32(0.0)


class RefKeyFrameDatabase:
    """neighbours(kf) -> the keyframes of pKFi->GetBestCovisibilityKeyFrames(10).  Every Detect* call is a new query keyframe /
    frame, i.e. a new mnId."""

    def __init__(self):
        self.mvInvertedFile = {}
        self.next_id = 0

    def add(self, pKF):
        for w in pKF.mBowVec[0]:
            self.mvInvertedFile.setdefault(int(w), []).append(pKF)

    def erase(self, pKF):
        for w in pKF.mBowVec[0]:
            lKFs = self.mvInvertedFile.get(int(w), [])
            for k, x in enumerate(lKFs):
                if x is pKF:
                    del lKFs[k]
                    break

    def clear(self):
        self.mvInvertedFile = {}

    def DetectLoopCandidates(self, bow, connected, minScore, neighbours, stats=None):
        mnId = self.next_id
        self.next_id += 1
        minScore = F32(minScore)
        spConnectedKeyFrames = set(id(k) for k in connected)
        lKFsSharingWords = []
        for w in bow[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnLoopQuery != mnId:
                    pKFi.mnLoopWords = 0
                    if id(pKFi) not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        if not lKFsSharingWords:
            return []
        lScoreAndMatch = []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = F32(score(bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore, accScore, pBestKF = si, si, pKFi
            for pKF2 in neighbours(pKFi):
                if pKF2.mnLoopQuery == mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        return _retain(lAccScoreAndMatch, minScoreToRetain, stats)

    def DetectRelocalizationCandidates(self, bow, neighbours, stats=None):
        mnId = self.next_id
        self.next_id += 1
        lKFsSharingWords = []
        for w in bow[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnRelocQuery != mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(score(bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore, accScore, pBestKF = si, si, pKFi
            for pKF2 in neighbours(pKFi):
                if pKF2.mnRelocQuery != mnId:
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        return _retain(lAccScoreAndMatch, minScoreToRetain, stats)


def _retain(lAccScoreAndMatch, minScoreToRetain, stats):
    """:175-196 / :289-308; stats (a dict) counts what the 0.75 filter and spAlreadyAddedKF removed"""
    spAlreadyAddedKF, out = set(), []
    for si, pKFi in lAccScoreAndMatch:
        if si > minScoreToRetain:
            if id(pKFi) not in spAlreadyAddedKF:
                out.append(pKFi)
                spAlreadyAddedKF.add(id(pKFi))
            elif stats is not None:
                stats["duplicates"] = stats.get("duplicates", 0) + 1
        elif stats is not None:
            stats["filtered"] = stats.get("filtered", 0) + 1
    return out


# ---- the dense per-slot formulation (what the device computes) --------------------------------------------------------------
def dense_query(rows, bow, exclude=()):
    """rows: {slot: bow} of the live slots -> {slot: (words, first_word, score)} and max_common; excluded slots as if dead"""
    qids = set(int(w) for w in bow[0])
    out, max_common = {}, 0
    for s, r in rows.items():
        if s in exclude:
            continue
        common = [int(w) for w in r[0] if int(w) in qids]
        out[s] = (len(common), common[0] if common else -1, score(bow, r) if common else 0.0)
        max_common = max(max_common, len(common))
    return out, max_common


def dense_sharing(dense, seq):
    """lKFsSharingWords as slots: words > 0, ascending (first_word, add sequence)"""
    return sorted((s for s, d in dense.items() if d[0] > 0), key=lambda s: (dense[s][1], seq[s]))


class RefWorld:
    """A database of slots driven like the mirrors: add / erase / clear by slot, neighbours as slot lists, results as slot lists."""

    def __init__(self):
        self.db = RefKeyFrameDatabase()
        self.kf = {}          # live slot -> RefKeyFrame
        self.seq = {}         # live slot -> add sequence
        self.next_seq = 0

    def add(self, slot, bow):
        assert slot not in self.kf
        self.kf[slot] = RefKeyFrame(slot, bow)
        self.db.add(self.kf[slot])
        self.seq[slot] = self.next_seq
        self.next_seq += 1

    def erase(self, slot):
        if slot in self.kf:
            self.db.erase(self.kf.pop(slot))
            del self.seq[slot]

    def clear(self):
        self.db.clear()
        self.kf, self.seq = {}, {}

    def rows(self):
        return {s: k.mBowVec for s, k in self.kf.items()}

    def _neigh(self, neighbours):
        return lambda k: [self.kf[s] for s in neighbours.get(k.slot, ()) if s in self.kf]

    def loop(self, bow, connected, min_score, neighbours, stats=None):
        r = self.db.DetectLoopCandidates(bow, [self.kf[s] for s in connected if s in self.kf], min_score, self._neigh(neighbours), stats)
        return [k.slot for k in r]

    def reloc(self, bow, neighbours, stats=None):
        return [k.slot for k in self.db.DetectRelocalizationCandidates(bow, self._neigh(neighbours), stats)]

    def score(self, bow, slots):
        return np.array([score(bow, self.kf[s].mBowVec) for s in slots], np.float64)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def hand_bow(ids, vals=None, seed=0):
    """a hand-made L1-normalised row over the given ascending ids"""
    ids = np.asarray(ids, np.int32)
    if vals is None:
        vals = np.random.default_rng(seed).uniform(0.1, 9.0, len(ids))
    vals = np.asarray(vals, np.float64)
    if len(vals):
        vals = vals / np.sum(np.abs(vals))
    return ids, vals


def place_descriptors(vocab, nplaces, nviews, nfeat, seed, keep=0.7, fresh=0.2):
    """nplaces places seen nviews times each: a place is a fixed set of leaf descriptors, a view keeps a random part of them
    (bit-exact copies) and adds some random ones.  -> list of (place, view, desc [n][32])"""
    rng = np.random.default_rng(seed)
    children, node_desc = vocab[0], vocab[1]
    leaves = np.array([i for i, c in enumerate(children) if not c])
    out = []
    for p in range(nplaces):
        base = node_desc[rng.choice(leaves, nfeat)]
        for v in range(nviews):
            d = base[rng.random(nfeat) < keep]
            extra = node_desc[rng.choice(leaves, max(int(nfeat * fresh), 1))]
            out.append((p, v, np.ascontiguousarray(np.concatenate([d, extra]), np.uint8)))
    return out


def geometry_case(max_words, seed=3):
    """Rows of lengths 0, 1, 63, 64, 65, 129, max_words (and random others) in 41 slots, and queries of lengths 0, 1, 65, max_words:
    none in common, all in common (the query is the longest row), exactly one in common as the last entry of a row, hits on both
    sides of a 64-entry chunk boundary.  -> rows {slot: bow}, queries [bow], slot_of {"len65": s, "len129": s, "full": s}"""
    rng = np.random.default_rng(seed)
    U = 3 * max_words
    lens = [0, 1, 63, 64, 65, 129, max_words] + [int(x) for x in rng.integers(2, min(max_words, 200) + 1, 34)]
    rows = {}
    for s, n in enumerate(lens):
        rows[s] = hand_bow(np.sort(rng.choice(U, n, replace=False)), seed=100 + s)
    r65, r129, full = rows[4], rows[5], rows[6]
    others = np.setdiff1d(np.arange(U), r129[0])
    q65 = np.union1d(r129[0][63:65], rng.choice(others, 63, replace=False))   # of row 129 exactly its entries 63 and 64
    queries = [hand_bow([]), hand_bow([int(r65[0][-1])], [1.0]), hand_bow(q65, seed=7), (full[0].copy(), full[1].copy()),
               hand_bow(np.arange(U, U + 65), seed=8)]
    return rows, queries, {"len65": 4, "len129": 5, "full": 6}


def seeded_world(seed, nplaces=8, nviews=5, nfeat=300):
    """Keyframes = views of places in a shuffled order of adds, some erased, one erased and added again; one loop query and one
    relocalisation query per place.  -> dict(vocab, desc {slot: descriptors}, ops [("add" | "erase", slot)], queries
    [dict(desc, connected, neighbours)]); the BowVectors are the caller's to compute (oracle or device)."""
    import bow_vocab
    rng = np.random.default_rng(seed)
    vocab = bow_vocab.make_vocab(10, 3, seed=seed)
    views = place_descriptors(vocab, nplaces, nviews + 1, nfeat, seed + 1)
    slot_of, desc, qdesc = {}, {}, {}
    order = rng.permutation(nplaces * nviews)
    k = 0
    for p, v, d in views:
        if v == nviews:
            qdesc[p] = d                 # the extra view of a place is the query
        else:
            slot_of[(p, v)] = int(order[k])
            desc[int(order[k])] = d
            k += 1
    add_order = [int(s) for s in rng.permutation(nplaces * nviews)]
    ops = [("add", s) for s in add_order]
    erased = [slot_of[(1, 2)], slot_of[(3, 0)]]
    readded = slot_of[(2, 1)]
    ops += [("erase", s) for s in erased] + [("erase", readded), ("add", readded)]
    live = [s for s in desc if s not in erased]
    neighbours = {}
    for (p, v), s in slot_of.items():
        same = [slot_of[(p, w)] for w in range(nviews) if w != v]
        nb = [int(x) for x in rng.permutation(same)[:int(rng.integers(0, 4))]]
        nb += [int(x) for x in rng.choice(nplaces * nviews, int(rng.integers(0, 3)), replace=False)]
        neighbours[s] = nb
    queries = []
    for p in range(nplaces):
        connected = [slot_of[((p + 1) % nplaces, w)] for w in range(nviews)] + [slot_of[(p, int(rng.integers(0, nviews)))]]
        queries.append(dict(place=p, desc=qdesc[p], connected=[s for s in connected if s in live], neighbours=neighbours))
    return dict(vocab=vocab, desc=desc, ops=ops, queries=queries, nslots=nplaces * nviews, erased=erased, readded=readded)


def run_world(world, bows, qbows, stats=None):
    """the restatement on a seeded world -> (RefWorld, [dict(min_score, loop, reloc)] per query)"""
    w = RefWorld()
    for op, s in world["ops"]:
        if op == "add":
            w.add(s, bows[s])
        else:
            w.erase(s)
    out = []
    for q, qb in zip(world["queries"], qbows):
        sc = w.score(qb, q["connected"])
        min_score = F32(1)
        for x in sc:                      # LoopClosing::DetectLoop :126-138
            if F32(x) < min_score:
                min_score = F32(x)
        out.append(dict(min_score=min_score, loop=w.loop(qb, q["connected"], min_score, q["neighbours"], stats),
                        reloc=w.reloc(qb, q["neighbours"], stats)))
    return w, out
