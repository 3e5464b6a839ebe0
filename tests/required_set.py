"""Fixtures for doc sets as the ONLY required clause - "b c #F", a lone #F, *:* (plain Python, no GPU) - and the composed reference.

The reference builds ReqOptScorer(F, DisjunctionSumScorer(b, c)) for such a query (boolean_query.rs:253-262): with M = live AND sets
every doc of M is collected, total_hits = |M|, a doc scores the disjunction's own sum where a SHOULD clause holds it and +0.0
elsewhere. composed() says that with the oracle's parts alone: per leaf the docs of M ascending, scored by Searcher.score_docs (0.0
where unmatched), streamed through topk_stream under the canonical rule, the leaves merged by that rule, total = |M|.
tests/test_required_set_cpu.py holds it against the oracle's own ReqOptScorer search before a GPU sees any of this.

BIG is the leaf of the C-ABI tests: 3 * HEAD_CHUNK_WORDS * 64 + 65 docs, i.e. three whole chunks of the head build and a last one of
two words, with short lists only (the sets come from words, not from postings):
  T[n]     the first n docs of SEQ = 5000 + 37 i - n in SIZES: k - 1, k and k + 1 for every k of KS, and 0 (an absent term)
  R[0..11] seeded lists of 200 .. 750 docs over the whole leaf: the clauses of the two-, nine- and twelve-clause disjunctions
The placements of O = docs(T[n]) AND M against the head of M (the first k docs of M):
  inside   M = the docs at and right behind every SEQ doc: O starts M, every other doc of the head is scored and must be skipped
  behind   M = [0, 2000), SEQ and a few docs around every chunk edge: the head of every k holds no scored doc
  outside  M = docs that are no SEQ doc: O is empty, the row is the head
  (deleted: M = inside on a leaf whose live docs delete SEQ - the same, through live AND set)"""
import numpy as np

import segment_spectrum as ss

HEAD_CHUNK_WORDS = 2048                       # RGPU_DOCSET_HEAD_CHUNK_WORDS (tests hold it against rucene_amd._lib)
CHUNK_DOCS = HEAD_CHUNK_WORDS * 64
BIG_MAX_DOC = 3 * CHUNK_DOCS + 65
KS = (1, 10, 64, 65, 128, 129, 1024)
SIZES = sorted({0} | {n for k in KS for n in (k - 1, k, k + 1)})
SEQ = (5000 + 37 * np.arange(max(SIZES))).astype(np.int32)
N_R = 12
T = {n: i for i, n in enumerate(SIZES)}      # size -> term id
R = [len(SIZES) + i for i in range(N_R)]
N_TERMS = len(SIZES) + N_R
NORMS = ("rank", "raw", "none")
PLACEMENTS = ("inside", "behind", "outside")


def _freqs(rng, n):
    return np.minimum(10, rng.geometric(0.5, size=n)).astype(np.int32)


def big_lists():
    rng = np.random.default_rng([BIG_MAX_DOC, 81])
    lists = [(SEQ[:n].copy(), _freqs(rng, n)) for n in SIZES]
    for i in range(N_R):
        d = np.sort(rng.choice(BIG_MAX_DOC, size=200 + 50 * i, replace=False)).astype(np.int32)
        if i == 0:
            d = np.unique(np.concatenate([d, [0, CHUNK_DOCS - 1, CHUNK_DOCS, BIG_MAX_DOC - 1]])).astype(np.int32)   # doc 0, a chunk edge, the last doc
        lists.append((d, _freqs(rng, d.size)))
    return lists


class Big:
    """BIG with one kind of norms and one .doc format; `alive` (a bool mask or None) makes the live variants of one build"""
    _built = {}

    def __init__(self, norms="rank", version=1, alive=None, doc_base=0):
        from rucene_amd import indexgen
        key = (norms, version)
        if key not in Big._built:
            rng = np.random.default_rng([BIG_MAX_DOC, 82])
            if norms == "rank":
                nb = rng.integers(95, 125, size=BIG_MAX_DOC).astype(np.uint8)
            elif norms == "raw":
                nb = ss.RAW_BYTES[rng.integers(0, ss.RAW_BYTES.size, size=BIG_MAX_DOC)]
            else:
                nb = None
            lists = big_lists()
            Big._built[key] = (lists, nb, indexgen.build_explicit(BIG_MAX_DOC, lists, norms=nb, version=version))
        self.lists, self.norms, self.seg = Big._built[key]
        self.max_doc, self.doc_base, self.sttf = BIG_MAX_DOC, doc_base, ss.STTF_PER_DOC * BIG_MAX_DOC
        self.alive = np.ones(BIG_MAX_DOC, bool) if alive is None else np.asarray(alive, bool)
        self.live_docs = None if alive is None else ss.live_words(self.alive)
        self.has = None

    def oracle_segment(self, oracle):
        return oracle.Segment(self.seg.doc_bytes, self.norms, self.max_doc, self.seg.terms, doc_base=self.doc_base, live_docs=self.live_docs,
                              sum_total_term_freq=self.sttf)


class Small:
    """A small leaf with BIG's vocabulary, for the multi-leaf mirror tests: T[n] holds the first min(n, max_doc // 3) docs of
    0, 3, 6 ..., R[i] a seeded fifth of the docs; live docs as tests/segment_spectrum.py makes them"""
    _built = {}

    def __init__(self, max_doc, live="none", salt=0, doc_base=0):
        from rucene_amd import indexgen
        key = (max_doc, salt)
        if key not in Small._built:
            rng = np.random.default_rng([max_doc, salt, 84])
            every_third = np.arange(0, max_doc, 3, dtype=np.int32)
            lists = [(every_third[:n].copy(), _freqs(rng, every_third[:n].size)) for n in SIZES]
            for _ in range(N_R):
                d = np.flatnonzero(rng.random(max_doc) < 0.2).astype(np.int32)
                lists.append((d, _freqs(rng, d.size)))
            nb = rng.integers(95, 125, size=max_doc).astype(np.uint8)
            Small._built[key] = (lists, nb, indexgen.build_explicit(max_doc, lists, norms=nb))
        self.lists, self.norms, self.seg = Small._built[key]
        self.max_doc, self.doc_base, self.sttf = max_doc, doc_base, ss.STTF_PER_DOC * max_doc
        self.alive = ss.alive_mask(max_doc, live, salt)
        self.live_docs = None if live == "none" else ss.live_words(self.alive)

    def oracle_segment(self, oracle):
        return oracle.Segment(self.seg.doc_bytes, self.norms, self.max_doc, self.seg.terms, doc_base=self.doc_base, live_docs=self.live_docs,
                              sum_total_term_freq=self.sttf)


def has_table(fx):
    """[term][doc] membership of a fixture leaf's lists"""
    has = np.zeros((len(fx.lists), fx.max_doc), bool)
    for t, (d, _) in enumerate(fx.lists):
        has[t, d] = True
    return has


def seq_mask():
    m = np.zeros(BIG_MAX_DOC, bool)
    m[SEQ] = True
    return m


def edge_docs():
    """a few docs on either side of every chunk edge, and the leaf's last three"""
    e = [d for c in (1, 2, 3) for d in range(c * CHUNK_DOCS - 2, c * CHUNK_DOCS + 3)] + list(range(BIG_MAX_DOC - 3, BIG_MAX_DOC))
    return np.array(e, np.int64)


def placement_mask(name):
    m = np.zeros(BIG_MAX_DOC, bool)
    if name == "inside":
        m[SEQ] = True
        m[SEQ + 1] = True
    elif name == "behind":
        m[:2000] = True
        m[SEQ] = True
        m[edge_docs()] = True
    else:
        assert name == "outside"
        m[:3000] = True
        m[5000:6000] = True
        m[edge_docs()] = True
        m[SEQ] = False
    return m


def sizes_of(k):
    """how many docs O holds, per row of the shapes test: 0, 1, k - 1, k, k + 1"""
    return sorted({0, 1, k - 1, k, k + 1})


# ---- sets for rgpu_docset_head ----------------------------------------------------------------------------------------------------
HEAD_NS = (0, 1, 64, 65, 1024)


def head_sets(n):
    """name -> bool mask, the sets rgpu_docset_head is asked for with n (n >= 1 where a set is made around rank n)"""
    N = BIG_MAX_DOC
    out = {}

    def of(docs):
        m = np.zeros(N, bool)
        m[np.asarray(docs, np.int64)] = True
        return m
    out["empty"] = np.zeros(N, bool)
    out["doc 0"] = of([0])
    out["last doc"] = of([N - 1])
    out["every doc"] = np.ones(N, bool)
    out["every second doc"] = of(np.arange(0, N, 2))
    out["bits 63 | 64"] = of([63, 64, 127, 128, CHUNK_DOCS + 63, CHUNK_DOCS + 64])
    out["last chunk only"] = of([3 * CHUNK_DOCS, 3 * CHUNK_DOCS + 1, 3 * CHUNK_DOCS + 63, 3 * CHUNK_DOCS + 64, N - 1])
    m = max(n, 2)
    # the last doc of chunk 0 and the first of chunk 1 at ranks (m - 2, m - 1) and (m - 1, m): the head ends behind | on the edge
    out["chunk edge, both in"] = of(list(range(3, 3 * (m - 2) + 3, 3)) + [CHUNK_DOCS - 1, CHUNK_DOCS, CHUNK_DOCS + 5])
    out["chunk edge, one in"] = of(list(range(3, 3 * (m - 1) + 3, 3)) + [CHUNK_DOCS - 1, CHUNK_DOCS, CHUNK_DOCS + 5])
    for name, size in (("n - 1 docs", max(n - 1, 0)), ("n docs", n), ("n + 1 docs", n + 1)):
        out[name] = of(7 * np.arange(size) + 6)
    out["spread"] = np.random.default_rng([N, 83]).random(N) < 0.01
    out["spread"][N - 1] = True   # (the last chunk holds 65 docs: the draw alone seldom reaches it)
    return out


def head_deletions(mask, n):
    """name -> alive mask: the set's first doc, its doc at rank n - 1, the whole first chunk, every doc of the set deleted"""
    docs = np.flatnonzero(mask)
    out = {}
    for name, gone in (("first doc", docs[:1]), ("rank n - 1", docs[max(n - 1, 0):max(n, 1)]), ("first chunk", np.arange(CHUNK_DOCS)), ("the whole set", docs)):
        alive = np.ones(BIG_MAX_DOC, bool)
        alive[gone] = False
        out[name] = alive
    return out


# ---- the composed reference ---------------------------------------------------------------------------------------------------------
def composed(oracle, osr, leaves_m, should_ids, k):
    """leaves_m: [(doc_base, bool mask of M over the leaf's docs)] in leaf order; osr: an oracle Searcher over the same leaves (its
    live docs are not consulted: M holds live docs only). -> (docs, scores, total): the canonical top k of "every doc of M, scored
    by the disjunction of should_ids where it matches, 0.0 elsewhere" and |M|."""
    rows, total = [], 0
    for base, m in leaves_m:
        docs = (np.flatnonzero(m) + base).astype(np.int32)
        total += docs.size
        scores = np.zeros(docs.size, np.float32)
        if docs.size and len(should_ids):
            sc, matched = osr.score_docs(oracle.OP_OR, list(should_ids), docs)
            scores = np.where(matched, sc, np.float32(0.0)).astype(np.float32)
        rows.append(oracle.topk_stream(docs, scores, k, oracle.TIE_CANONICAL))
    d = np.concatenate([r[0] for r in rows]).astype(np.int64)
    s = np.concatenate([r[1] for r in rows]).astype(np.float32)
    order = np.lexsort((d, -s.astype(np.float64)))[:k]
    return d[order], s[order], total


def assert_row(hits_row, total, want, what, exact=True):
    """a k-row of the call under test against composed()'s: docs, score bits, the -1 padding, the total"""
    d, s, t = want
    n = d.size
    assert int(total) == t, (what, "total", int(total), t)
    assert hits_row["doc"][:n].tolist() == d.tolist(), (what, "docs", hits_row["doc"][:n].tolist()[:12], d.tolist()[:12])
    assert (hits_row["doc"][n:] == -1).all() and (hits_row["score"][n:] == 0).all(), (what, "padding")
    if exact:
        assert hits_row["score"][:n].view(np.int32).tolist() == s.view(np.int32).tolist(), (what, "score bits")
