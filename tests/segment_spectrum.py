"""Segment-size fixtures (plain Python, no GPU): the segments a freshly written directory really holds - next to one or two large
merged segments a tail of flushed ones of 1, 7 or 130 docs, some with every doc deleted - one leaf at a time and many at once.

SIZES are max_doc values on both sides of every rounding the library does by segment size: the 32- and 64-doc words of doc bitmaps
(built for lists of 512 docs and more: the sizes from 1023 up) and of live docs, the 128-doc block, two blocks and a tail, a whole
64-block chunk of an every-doc list. Every leaf has the same
vocabulary, so a term id means the same shape everywhere:

  EVERY      every doc (a VInt tail alone below 128 docs; whole blocks at 128 / 256 / 1024 / 8192; a one-doc tail one above them)
  FIRST      doc 0 alone            } singletons; the same doc in a one-doc leaf
  LAST       doc max_doc - 1 alone  }
  EVEN       every second doc
  FIFTH      a seeded random fifth of the docs, at least one
  ABSENT     df 0 everywhere
  SOMETIMES  every third doc counted back from the last one, in leaves whose max_doc is not a multiple of 3; absent in the others
  CONST      every doc, freq 3: with one norm byte throughout, every doc scores the same
  FILLER     every doc of a HOLLOW leaf (a leaf in which all the terms above are absent), absent elsewhere; never queried

Freqs are geometric, capped at 10. Norms: "rank" - seeded bytes of a narrow range (at most 30 distinct: rank mode); "raw" - 70
distinct bytes, every one of them present once max_doc reaches 70 (65 or more distinct: raw mode); "none"; or one constant byte.
sum_total_term_freq is 60 * max_doc. Live docs per leaf: LIVE = none / seeded (about 60 % alive) / the last doc deleted / doc 0
deleted / everything deleted, as u64 words (packbits, little bit order, padded to whole words).

Multi-leaf indexes (lists of Leaf with cumulative doc_base): many() - one leaf of every size, ascending or shuffled, live variants
mixed in, one leaf all deleted, one hollow; tail() - a 50 000-doc leaf neither first nor last among 40 leaves of 1 to 200 docs;
twins() - the two largest leaves are equally large and differ in their statistics; ties() - 24 leaves of 64 docs and one norm byte,
where CONST scores 1536 docs alike and PLATEAU (in place of SOMETIMES) puts a band of equal scores across a leaf boundary;
crumbs() - leaves of 1, 1, 2, 3, 1, 31 and 7 docs: fewer docs in the whole index than k.

The reference here is plain numpy and independent of the oracle: set algebra over the input lists, the live masks and the doc
bases gives every query's matching docs (and so its hit count); for ties() it gives whole rows. tests/test_segment_spectrum_cpu.py
holds the oracle against it before a GPU sees any of this."""
import collections

import numpy as np

SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193]
EVERY, FIRST, LAST, EVEN, FIFTH, ABSENT, SOMETIMES, CONST, FILLER = range(9)
PLATEAU = SOMETIMES                # ties(): the band of equal scores across a leaf boundary takes this id
QUERIED = list(range(FILLER))      # FILLER is decoded, never searched
N_TERMS = FILLER + 1
LIVE = ("none", "seeded", "last", "first", "all")
NORMS = ("rank", "raw", "none")
STTF_PER_DOC = 60
KS = (1, 10, 128, 129, 300)
RAW_BYTES = np.arange(60, 130, dtype=np.uint8)   # 70 distinct SmallFloat bytes
TIES_BYTE = 110

_EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def _freqs(rng, n):
    return np.minimum(10, rng.geometric(0.5, size=n)).astype(np.int32)   # as _postings of tests/test_gpu_parity.py


def live_words(alive):
    """A boolean mask as live-docs words: packbits, little bit order, padded to whole u64 words."""
    b = np.packbits(np.asarray(alive, bool), bitorder="little")
    return np.concatenate([b, np.zeros((-b.size) % 8, np.uint8)]).view(np.uint64)


def alive_mask(max_doc, live, salt=0):
    assert live in LIVE
    alive = np.ones(max_doc, bool)
    if live == "seeded":
        alive = np.random.default_rng([max_doc, salt, 60]).random(max_doc) < 0.6
    elif live == "last":
        alive[-1] = False
    elif live == "first":
        alive[0] = False
    elif live == "all":
        alive[:] = False
    return alive


class _Built:
    """The postings, norms and .doc bytes of one (max_doc, norms, salt, hollow, overrides): shared by its live variants."""

    def __init__(self, max_doc, norms, salt, hollow, overrides):
        from rucene_amd import indexgen
        rng = np.random.default_rng([max_doc, salt, 1])
        every = np.arange(max_doc, dtype=np.int32)
        fifth = np.flatnonzero(rng.random(max_doc) < 0.2).astype(np.int32)
        if fifth.size == 0:
            fifth = np.array([int(rng.integers(0, max_doc))], np.int32)
        lists = [None] * N_TERMS
        lists[EVERY] = (every, _freqs(rng, max_doc))
        lists[FIRST] = (every[:1], _freqs(rng, 1))
        lists[LAST] = (every[-1:], _freqs(rng, 1))
        lists[EVEN] = (every[::2], _freqs(rng, every[::2].size))
        lists[FIFTH] = (fifth, _freqs(rng, fifth.size))
        lists[ABSENT] = _EMPTY
        third = np.arange((max_doc - 1) % 3, max_doc, 3, dtype=np.int32)
        lists[SOMETIMES] = (third, _freqs(rng, third.size)) if max_doc % 3 else _EMPTY
        lists[CONST] = (every, np.full(max_doc, 3, np.int32))
        lists[FILLER] = _EMPTY
        if hollow:
            lists = [_EMPTY] * FILLER + [(every, _freqs(rng, max_doc))]
        for t, (d, f) in (overrides or {}).items():
            lists[t] = (np.asarray(d, np.int32), np.asarray(f, np.int32))
        if norms == "rank":
            nb = rng.integers(95, 125, size=max_doc).astype(np.uint8)
        elif norms == "raw":
            nb = RAW_BYTES[rng.integers(0, RAW_BYTES.size, size=max_doc)]
            at = rng.permutation(max_doc)[:RAW_BYTES.size]
            nb[at] = RAW_BYTES[:at.size]   # every byte present whatever the draw, as far as the docs go
            assert np.unique(nb).size >= min(65, max_doc), (max_doc, np.unique(nb).size)
        elif norms == "none":
            nb = None
        else:
            nb = np.full(max_doc, int(norms), np.uint8)
        self.max_doc, self.lists, self.norms = max_doc, lists, nb
        self.seg = indexgen.build_explicit(max_doc, lists, norms=nb)
        self.sttf = STTF_PER_DOC * max_doc
        self.has = np.zeros((N_TERMS, max_doc), bool)
        for t, (d, _) in enumerate(lists):
            self.has[t, d] = True
        dfs = self.seg.terms["doc_freq"]
        assert [int(x) for x in dfs] == [d.size for d, _ in lists]


_built = {}


class Leaf:
    def __init__(self, max_doc, norms="rank", live="none", salt=0, hollow=False, overrides=None, doc_base=0):
        key = (max_doc, norms, salt, hollow, None if overrides is None else tuple(sorted((t, tuple(d), tuple(f)) for t, (d, f) in overrides.items())))
        if key not in _built:
            _built[key] = _Built(max_doc, norms, salt, hollow, overrides)
        self.built = b = _built[key]
        self.max_doc, self.lists, self.norms, self.seg, self.sttf, self.has = max_doc, b.lists, b.norms, b.seg, b.sttf, b.has
        self.live, self.doc_base, self.hollow = live, doc_base, hollow
        self.alive = alive_mask(max_doc, live, salt)
        self.live_docs = None if live == "none" else live_words(self.alive)
        assert self.live_docs is None or self.live_docs.size == (max_doc + 63) // 64

    def oracle_segment(self, oracle):
        return oracle.Segment(self.seg.doc_bytes, self.norms, self.max_doc, self.seg.terms, doc_base=self.doc_base, live_docs=self.live_docs,
                              sum_total_term_freq=self.sttf)


def _based(leaves):
    base = 0
    for leaf in leaves:
        leaf.doc_base = base
        base += leaf.max_doc
    return leaves


def stats_leaf(leaves):
    """The first of the largest leaves (searcher.rs:306-363)."""
    return int(np.argmax([leaf.max_doc for leaf in leaves]))   # (argmax: the first maximum)


# ---- multi-leaf indexes -------------------------------------------------------------------------------------------------------------
def many(shuffled, norms="rank"):
    sizes = list(SIZES)
    if shuffled:
        sizes = [sizes[i] for i in np.random.default_rng(24).permutation(len(sizes))]
    leaves = []
    for i, n in enumerate(sizes):
        live = LIVE[i % 4]             # none, seeded, last, first in turn ...
        if n == 193:
            live = "all"               # ... one leaf all deleted ...
        leaves.append(Leaf(n, norms, live, salt=2, hollow=(n == 65)))   # ... and one without the queried terms
    assert stats_leaf(leaves) == sizes.index(8193)
    return _based(leaves)


def tail(norms="rank"):
    rng = np.random.default_rng(40)
    sizes = rng.integers(1, 201, size=40).tolist()
    sizes[3], sizes[30] = 1, 200
    leaves = [Leaf(n, norms, LIVE[(i * 7) % 5] if i % 3 else "none", salt=3) for i, n in enumerate(sizes)]
    leaves.insert(17, Leaf(50_000, norms, "seeded", salt=3))
    assert stats_leaf(leaves) == 17
    return _based(leaves)


TWINS_STATS_LEAF = 1


def twins(norms="rank"):
    leaves = [Leaf(129, norms, "seeded", salt=4), Leaf(1024, norms, "none", salt=5), Leaf(33, norms, "last", salt=4),
              Leaf(1024, norms, "first", salt=6), Leaf(64, norms, "none", salt=4)]
    a, b = leaves[1], leaves[3]
    assert a.lists[FIFTH][0].size != b.lists[FIFTH][0].size   # the twins score FIFTH differently: the choice between them shows
    assert stats_leaf(leaves) == TWINS_STATS_LEAF
    return _based(leaves)


TIES_LEAVES, TIES_DOCS = 24, 64
PLATEAU_LO, PLATEAU_HI = 3 * 64 + 40, 4 * 64 + 30   # global docs [232, 286): 24 docs of leaf 3 and 30 of leaf 4, freq 5
TIES_KS = (1, 10, 100, 129)
PLATEAU_KS = (1, 10, 30, 54, 60)                      # 30: the k-th place falls inside the band, six docs into leaf 4


def ties():
    leaves = []
    for i in range(TIES_LEAVES):
        g = np.arange(i * TIES_DOCS, (i + 1) * TIES_DOCS)
        # PLATEAU: freq 5 inside the band; freq 1 on every fourth doc outside it, in every leaf but the first (df 0 in the
        # statistics leaf: idf of an unseen term)
        inside = (g >= PLATEAU_LO) & (g < PLATEAU_HI)
        take = inside | ((g % 4 == 1) & (i > 0))
        local = np.flatnonzero(take)
        over = {PLATEAU: (local, np.where(inside[local], 5, 1))}
        leaves.append(Leaf(TIES_DOCS, str(TIES_BYTE), "none", salt=100 + i, overrides=over))
    return _based(leaves)


def crumbs(norms="rank"):
    lives = ["none", "all", "last", "seeded", "none", "first", "all"]
    return _based([Leaf(n, norms, lv, salt=7 + i) for i, (n, lv) in enumerate(zip([1, 1, 2, 3, 1, 31, 7], lives))])


INDEXES = {"many-ascending": lambda: many(False), "many-shuffled": lambda: many(True), "many-raw": lambda: many(True, "raw"), "tail": tail,
           "twins": twins, "ties": ties, "crumbs": crumbs, "crumbs-no-norms": lambda: crumbs("none")}


# ---- queries ------------------------------------------------------------------------------------------------------------------------
Query = collections.namedtuple("Query", "must should must_not filt msm", defaults=((), (), (), (), 0))

TERMS = [Query(must=(t,)) for t in QUERIED]
ANDS = [Query(must=m) for m in [(EVERY, EVEN), (EVEN, FIFTH), (FIRST, LAST), (EVERY, ABSENT), (FIRST, EVEN), (LAST, SOMETIMES), (CONST, FIFTH),
                                (EVERY, EVEN, FIFTH), (CONST, EVERY, LAST), (EVEN, SOMETIMES, FIFTH), (FIRST, ABSENT, EVERY), (EVERY, CONST, FIRST)]]
ORS = [Query(should=s) for s in [(FIRST, LAST), (ABSENT, FIFTH), (EVEN, SOMETIMES), (ABSENT, ABSENT), (EVERY, CONST),
                                 (FIRST, LAST, EVEN, FIFTH, ABSENT), (EVERY, EVEN, FIFTH, SOMETIMES, CONST),
                                 (EVERY, FIRST, LAST, EVEN, FIFTH, ABSENT, SOMETIMES, CONST, EVEN),
                                 (FIRST, LAST, FIFTH, ABSENT, SOMETIMES, FIRST, LAST, FIFTH, ABSENT)]]
WIDE = [Query(should=s) for s in [tuple(QUERIED) + (EVERY, EVEN), (FIRST, LAST) * 5, (ABSENT,) * 10, (FIFTH, SOMETIMES, FIRST, LAST, ABSENT) * 2 + (EVEN,),
                                  (CONST,) * 10, (EVERY, EVEN, FIFTH, SOMETIMES) * 3]]
NOTS = [Query(must=m, should=s, must_not=n) for m, s, n in [
    ((EVERY,), (), (EVEN,)), ((EVERY,), (), (EVERY,)), ((CONST,), (), (FIRST, LAST)), ((EVEN,), (), (ABSENT,)), ((LAST,), (), (FIRST,)),
    ((FIRST,), (), (LAST,)), ((EVERY, EVEN), (), (FIFTH,)), ((EVERY, FIFTH), (), (EVEN, SOMETIMES)), ((ABSENT, EVERY), (), (FIRST,)),
    ((), (FIRST, LAST), (EVEN,)), ((), (EVERY, FIFTH, SOMETIMES), (EVEN, FIRST)), ((), (EVEN, ABSENT), (EVERY,))]]
FILTERS = [Query(must=m, filt=f) for m, f in [((EVERY,), (EVEN,)), ((EVEN, FIFTH), (EVERY,)), ((), (EVERY, FIFTH)), ((CONST,), (LAST,)),
                                                 ((FIRST,), (LAST,)), ((EVERY,), (ABSENT,)), ((SOMETIMES,), (EVEN, FIFTH))]]
MSM2 = [Query(should=s, must_not=n, msm=2) for s, n in [((EVERY, EVEN, FIFTH), ()), ((FIRST, LAST), ()), ((FIRST, LAST, ABSENT, SOMETIMES), ()),
                                                         ((EVERY, CONST, EVEN, FIFTH), (FIRST,)), ((ABSENT, EVERY), ()),
                                                         (tuple(QUERIED) + (EVEN, FIFTH), (LAST,)), ((EVEN, FIFTH, SOMETIMES), (EVEN,))]]
EXACT = TERMS + ANDS + ORS          # bit-exact rows through _check_against_oracle
GROUPS = {"terms": TERMS, "ands": ANDS, "ors": ORS, "wide": WIDE, "nots": NOTS, "filters": FILTERS, "msm2": MSM2}
ALL_QUERIES = [q for g in GROUPS.values() for q in g]
assert all(len(q.should) >= 10 for q in WIDE) and sorted(len(q.should) for q in ORS)[-1] == 9 and {2, 5, 9} <= {len(q.should) for q in ORS}


def spec(oracle, q):
    """A plain TERM / AND / OR query as the (op, term ids) of _check_against_oracle."""
    assert not (q.must_not or q.filt or q.msm) and bool(q.must) != bool(q.should)
    if q.must:
        return (oracle.OP_TERM if len(q.must) == 1 else oracle.OP_AND, list(q.must))
    return (oracle.OP_OR, list(q.should))


def not_spec(oracle, q):
    """A query with MUST_NOT clauses as the (op, positive ids, MUST_NOT ids) of _check_not_queries."""
    assert q.must_not and not (q.filt or q.msm) and bool(q.must) != bool(q.should)
    pos = list(q.must or q.should)
    return (oracle.OP_OR if q.should else (oracle.OP_TERM if len(pos) == 1 else oracle.OP_AND), pos, list(q.must_not))


def oracle_rows(oracle, osr, queries, k):
    """The oracle's canonical rows of any of the queries above: [(docs, scores, total_hits)]. FILTER clauses are required clauses
    of boost 0 (as tests/test_gpu_norm_spectrum.py asks for them); everything else goes through one search_batch."""
    out = [None] * len(queries)
    rest = [i for i, q in enumerate(queries) if not q.filt]
    for i, q in enumerate(queries):
        if q.filt:
            assert not (q.should or q.must_not or q.msm)
            out[i] = osr.search(oracle.OP_AND, list(q.must + q.filt), k, tie_mode=oracle.TIE_CANONICAL, boosts=[1.0] * len(q.must) + [0.0] * len(q.filt))
    if rest:
        qs = [queries[i] for i in rest]
        assert all(bool(q.must) != bool(q.should) for q in qs)
        pos = [list(q.must or q.should) for q in qs]
        ops = [oracle.OP_OR if q.should else (oracle.OP_TERM if len(q.must) == 1 and not q.must_not else oracle.OP_AND) for q in qs]
        offs = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int32)
        noffs = np.concatenate([[0], np.cumsum([len(q.must_not) for q in qs])]).astype(np.int32)
        tids = np.concatenate([np.asarray(p, np.int64) for p in pos])
        nids = np.concatenate([np.asarray(q.must_not, np.int64) for q in qs] + [np.zeros(0, np.int64)])
        cd, cs, cc, ct, _, _ = osr.search_batch(ops, offs, tids, k, tie_mode=oracle.TIE_CANONICAL, threads=4, not_offsets=noffs, not_ids=nids,
                                                min_should_match=np.asarray([q.msm for q in qs], np.int32))
        for j, i in enumerate(rest):
            n = int(cc[j])
            out[i] = (cd[j, :n].copy(), cs[j, :n].copy(), int(ct[j]))
    return out


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------
def ref_leaf_docs(leaf, q):
    """Local doc ids of one leaf that match q: set algebra over the input lists and the live mask."""
    m = leaf.alive.copy()
    for t in q.must + q.filt:
        m &= leaf.has[t]
    if q.should and (q.msm > 0 or not (q.must or q.filt)):
        count = np.zeros(leaf.max_doc, np.int32)
        for t in q.should:            # a clause given twice counts twice, as two scorers do
            count += leaf.has[t]
        m &= count >= max(1, q.msm)
    for t in q.must_not:
        m &= ~leaf.has[t]
    return np.flatnonzero(m).astype(np.int64)


def ref_docs(leaves, q):
    """Global doc ids, ascending, that match q anywhere in the index."""
    return np.concatenate([ref_leaf_docs(leaf, q) + leaf.doc_base for leaf in leaves])


def ref_ties_row(leaves, term, k):
    """ties(): the whole expected doc row of CONST or PLATEAU. One norm byte throughout and one weight per term: BM25 is strictly
    increasing in freq, so the ranking is freq descending, then global doc id ascending."""
    docs = np.concatenate([leaf.lists[term][0].astype(np.int64) + leaf.doc_base for leaf in leaves])
    freqs = np.concatenate([leaf.lists[term][1] for leaf in leaves])
    return docs[np.lexsort((docs, -freqs))][:k]


def leaf_of(leaves, docs):
    """Index of the leaf that holds each global doc id."""
    bases = np.array([leaf.doc_base for leaf in leaves])
    return np.searchsorted(bases, np.asarray(docs), side="right") - 1


# ---- tiny positions segments --------------------------------------------------------------------------------------------------------
POSITION_SIZES = [1, 2, 64, 129, 257]
PHRASES = [([0, 1], 0), ([1, 0], 0), ([0, 0], 0), ([0, 1, 2], 0), ([2, 2, 1], 0), ([0, 4], 0), ([3, 0], 0), ([0, 1, 4], 0),
           ([0, 1], 2), ([1, 0], 2), ([2, 2], 2), ([0, 1, 2], 2), ([1, 0, 1], 2), ([4, 1], 2), ([0, 3], 2), ([2, 4, 0], 2)]   # (terms, slop)
PHRASE_KS = (1, 10)


def positions_postings(max_doc):
    """Docs of 1..12 tokens over terms 0..2 (doc 0 and the last doc always start "0 1 2 0 0 1"), term 3 as the last token of the last
    doc alone, behind a 0, term 4 absent -> (postings per term as [(doc, [positions])], norms, doc_count, sum_total_term_freq)."""
    rng = np.random.default_rng([max_doc, 9])
    postings = [[] for _ in range(5)]
    sum_ttf = 0
    for d in range(max_doc):
        toks = rng.integers(0, 3, size=int(rng.integers(1, 13))).tolist()
        if d in (0, max_doc - 1):
            toks = [0, 1, 2, 0, 0, 1] + toks
        if d == max_doc - 1:
            toks += [0, 3]
        sum_ttf += len(toks)
        where = {}
        for p, t in enumerate(toks):
            where.setdefault(t, []).append(p)
        for t, ps in where.items():
            postings[t].append((d, ps))
    norms = rng.integers(95, 125, size=max_doc).astype(np.uint8)
    return postings, norms, max_doc, sum_ttf
