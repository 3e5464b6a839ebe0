"""Fixtures for the clause-order disjunction kernels, k_score_terms and k_or_windows (plain Python, no GPU): one posting list on
each side of every threshold rucene_amd/csrc/kernels/search_or.hpp and search_or_group (rucene_amd/csrc/rgpu_api.hip) branch on.

The main leaf has max_doc 8229 = 8 * 1024 + 37 = 32 * 256 + 37 = 2 * 4096 + 37: at every window width W of WINDOWS the last window
holds 37 docs, and every 1024 edge is a 256 edge too. The second leaf (33025 docs = 129 whole windows of 256 and one more that holds a single
doc) is for the two-windows-per-item plan alone. Every list is built from max_doc by the same rules, so a term id means the same shape on
both leaves:

  EDGE_1K, EDGE_256     docs 0, w - 1, w, w + 1 and max_doc - 1 for every multiple w of 1024 / of 256 that is no multiple of 1024
  FROM_0 .. FROM_128    every doc from s on, s in 0, 1, 127, 128: the 128-doc block at a window edge w1 ends on w1 - 1 (s = 0, 128), ends
                        on w1 (s = 1), starts on w1 - 1 (s = 127), starts on w1 (s = 0, 128); VInt tails of 37, 36, 38, 37 postings
  TAIL_0, TAIL_1,       FROM_0, FROM_1 and FROM_127 cut to whole blocks plus a VInt tail of 0, 1 and 127 postings
  TAIL_127
  SPAN                  one block of every fifth doc from 200 on (it crosses the edges 256, 512 and 768: a whole 256-doc window and
                        more), then every doc from 3000 on until the list is dense-eligible at every W
  BELOW_W, ABOVE_W      seeded lists of dense_bound(W) - 1 and dense_bound(W) docs for W = 256, 1024, 4096: either side of the rule
                        "df * W >= 64 * max_doc" of search_or_group, each with at least one block. On the main leaf these are
                        2057 | 2058, 514 | 515 and 128 | 129; the last pair doubles as the one-block list without a tail and with a
                        one-posting tail (DF_128, DF_129)
  TWIN_A, TWIN_B        two different seeded lists of one doc_freq above every bound: the tie of the dense selection
  STRETCH_n             n consecutive docs and nothing else, n in 63, 64, 65, 128, 129, each inside one 256-doc window (so inside one
                        window at every W); STRETCH_64 and STRETCH_129 end on their window's last doc
  FIRST_OF_WINDOW,      singletons (they live in the term-dictionary entry): doc 1024, doc max_doc - 1
  LAST_DOC
  DF_127                a VInt tail alone
  ABSENT                df 0
  COPY                  FROM_1's postings under another term id
  FREQ11_DENSE,         blocks of three kinds in turn: every freq <= 7 (freq bit width <= 3: the dense path's short cut), freqs <= 10 with
  FREQ11_SPARSE         a 10 (the score table by ballot), freqs <= 10 but for a single 11 (the formula by ballot); the sparse list's
                        VInt tail holds a single 11 as well. The dense list is eligible at every W, the sparse one at 4096 only
  BIG_FREQ              freqs of 2^20 + 3 inside a block and 2^21 in the tail
  CONST                 docs 900 .. 1200, freq 3; every one of these docs has the norm byte TIE_BYTE, so the 301 docs tie, across the
                        window (and item) edge 1024 at every W below 4096 and across the 256 edges 1024 and 1152

Every other freq is geometric, capped at 10. Norms: "rank" (30 distinct bytes), "raw" (70 distinct: raw mode), "none". Live docs:
"none" or "seeded" - about 85 % alive, and deleted for certain: both sides of the edges 256, 1024 and 4096 and ONLY_DENSE_DOC, a
doc no list below the default window's dense bound holds. `.doc` version 1 or 0.

Queries are segment_spectrum.Query records in four families. A, B and C are exact (fewer than ten SHOULD clauses, or
min_should_match >= 2, which forces the reference to clause-order sums); D is ten or more clauses with min_should_match <= 1, which
the reference sums in heap order (oracle/parity.py's rule). The reference next to the oracle's disjunction scorer is OrRef: hit
sets by numpy set algebra over the lists, a doc's score the f32 clause-order sum `0.0f + s_0 + s_1 ...` of the oracle's per-term
scores. tests/test_or_spectrum_cpu.py proves every property named here, and the oracle against OrRef, before a GPU sees any of it."""
import numpy as np

import segment_spectrum as ss
from segment_spectrum import Query

MAX_DOC = 8229
BIG_MAX_DOC = 33025
WINDOWS = (256, 1024, 4096)
DEFAULT_W = 1024
OR_DENSE_MAX = 4          # dense clauses per query
DENSE_CANDIDATES = 16     # the dense mask is 16 bits wide
OR_PREFETCH = 8           # run heads held in registers
SCORE_TABLE_FREQS = 10
BLOCK = 128
KS = (1, 10, 64, 65, 128, 129, 300)
NORMS = ("rank", "raw", "none")
LIVE = ("none", "seeded")
VERSIONS = (1, 0)
STTF_PER_DOC = 60
RAW_BYTES = np.arange(60, 130, dtype=np.uint8)
TIE_BYTE = 110
CONST_LO, CONST_HI, CONST_FREQ = 900, 1201, 3
DELETED_AT_EDGES = (255, 256, 1023, 1024, 4095, 4096)

NAMES = ["EDGE_1K", "EDGE_256", "FROM_0", "FROM_1", "FROM_127", "FROM_128", "TAIL_0", "TAIL_1", "TAIL_127", "SPAN", "BELOW_256", "ABOVE_256",
         "BELOW_1K", "ABOVE_1K", "BELOW_4K", "ABOVE_4K", "TWIN_A", "TWIN_B", "STRETCH_63", "STRETCH_64", "STRETCH_65", "STRETCH_128", "STRETCH_129",
         "FIRST_OF_WINDOW", "LAST_DOC", "DF_127", "ABSENT", "COPY", "FREQ11_DENSE", "FREQ11_SPARSE", "BIG_FREQ", "CONST"]
(EDGE_1K, EDGE_256, FROM_0, FROM_1, FROM_127, FROM_128, TAIL_0, TAIL_1, TAIL_127, SPAN, BELOW_256, ABOVE_256, BELOW_1K, ABOVE_1K, BELOW_4K, ABOVE_4K,
 TWIN_A, TWIN_B, STRETCH_63, STRETCH_64, STRETCH_65, STRETCH_128, STRETCH_129, FIRST_OF_WINDOW, LAST_DOC, DF_127, ABSENT, COPY, FREQ11_DENSE,
 FREQ11_SPARSE, BIG_FREQ, CONST) = range(len(NAMES))
N_TERMS = len(NAMES)
DF_128, DF_129 = BELOW_4K, ABOVE_4K
FROM = {FROM_0: 0, FROM_1: 1, FROM_127: 127, FROM_128: 128}
TAILS = {TAIL_0: (FROM_0, 0), TAIL_1: (FROM_1, 1), TAIL_127: (FROM_127, 127)}      # cut copy -> (its source, tail_n)
PAIRS = {256: (BELOW_256, ABOVE_256), 1024: (BELOW_1K, ABOVE_1K), 4096: (BELOW_4K, ABOVE_4K)}
# (first doc, length): each inside one 256-doc window; 960 + 64 = 1024 and 4223 + 129 = 4352 = 17 * 256 end on a window's last doc
STRETCHES = {STRETCH_63: (300, 63), STRETCH_64: (960, 64), STRETCH_65: (1300, 65), STRETCH_128: (2148, 128), STRETCH_129: (4223, 129)}
SPAN_FIRST, SPAN_STEP, SPAN_DENSE_FROM = 200, 5, 3000
BIG_FREQS = {5: (1 << 20) + 3, 150: 1 << 21}   # posting index -> freq: inside block 0, inside the VInt tail (df 200)
FIVE_DENSE = (FROM_0, FROM_1, TAIL_0, FROM_127, FROM_128)   # five lists above every bound, doc_freq descending: the fifth goes through a run

_EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def dense_bound(max_doc, W):
    """The smallest doc_freq search_or_group's rule `df * W >= 64 * max_doc` lets through."""
    return -(-64 * max_doc // W)


def eligible(leaf, t, W):
    """The list may be a dense clause at window width W (rank-mode norms and a place among the first 16 clauses besides)."""
    df = leaf.lists[t][0].size
    return df >= BLOCK and df * W >= 64 * leaf.max_doc


def dense_choice(leaf, should, W, dense_max=OR_DENSE_MAX):
    """Clause indexes search_or_group marks dense: up to dense_max times the longest eligible list not yet taken among the first 16
    clauses, ties to the earlier clause (the rule of its comment, written out again)."""
    present = [t for t in should if leaf.lists[t][0].size > 0]    # a clause without a scorer in the leaf drops out first
    chosen = []
    for _ in range(dense_max):
        best = -1
        for i, t in enumerate(present[:DENSE_CANDIDATES]):
            if i in chosen or not eligible(leaf, t, W):
                continue
            if best < 0 or leaf.lists[t][0].size > leaf.lists[present[best]][0].size:
                best = i
        if best < 0:
            break
        chosen.append(best)
    return sorted(chosen)


def _freqs(rng, n, cap=10):
    return np.minimum(cap, rng.geometric(0.5, size=n)).astype(np.int32)


def ballot_freqs(rng, df, tail_eleven):
    """Blocks of three kinds in turn (b % 3): 0 - every freq <= 7; 1 - <= 10 with a 10; 2 - <= 10 with a 10 and a single 11."""
    f = _freqs(rng, df)
    for b in range(df // BLOCK):
        blk = f[b * BLOCK:(b + 1) * BLOCK]
        if b % 3 == 0:
            np.minimum(blk, 7, out=blk)
        else:
            blk[(7 * b) % BLOCK] = 10
        if b % 3 == 2:
            blk[(37 * b + 5) % BLOCK] = 11    # (37 b + 5 = 7 b mod 128 has no solution with b % 3 == 2 below 64 blocks: asserted by the CPU test)
    if tail_eleven:
        f[df // BLOCK * BLOCK + 3] = 11
    return f


def build_lists(max_doc):
    """Every list of NAMES for one max_doc -> [(docs, freqs)] by term id."""
    rng = np.random.default_rng([max_doc, 7])
    every = np.arange(max_doc, dtype=np.int32)
    lists = [None] * N_TERMS

    def plain(docs):
        docs = np.asarray(docs, np.int32)
        return docs, _freqs(rng, docs.size)

    def drawn(df):
        return plain(np.sort(rng.choice(max_doc, size=df, replace=False)))

    def edges(ws):
        d = {0, max_doc - 1}
        for w in ws:
            d.update((w - 1, w, w + 1))
        return plain(sorted(x for x in d if 0 <= x < max_doc))

    lists[EDGE_1K] = edges(range(1024, max_doc, 1024))
    lists[EDGE_256] = edges(w for w in range(256, max_doc, 256) if w % 1024)
    for t, s in FROM.items():
        lists[t] = plain(every[s:])
    for t, (src, tail_n) in TAILS.items():
        d, f = lists[src]
        n = (d.size - tail_n) // BLOCK * BLOCK + tail_n
        if n == d.size:
            n -= BLOCK
        lists[t] = (d[:n].copy(), f[:n].copy())
    n_dense = dense_bound(max_doc, 256) + 100 - BLOCK
    lists[SPAN] = plain(np.concatenate([SPAN_FIRST + SPAN_STEP * every[:BLOCK], SPAN_DENSE_FROM + every[:n_dense]]))
    for W, (below, above) in PAIRS.items():
        lists[below], lists[above] = drawn(dense_bound(max_doc, W) - 1), drawn(dense_bound(max_doc, W))
    lists[TWIN_A], lists[TWIN_B] = drawn(dense_bound(max_doc, 256) + 500), drawn(dense_bound(max_doc, 256) + 500)
    for t, (first, n) in STRETCHES.items():
        lists[t] = plain(first + every[:n])
    lists[FIRST_OF_WINDOW] = plain([1024])
    lists[LAST_DOC] = plain([max_doc - 1])
    lists[DF_127] = drawn(127)
    lists[ABSENT] = _EMPTY
    lists[COPY] = (lists[FROM_1][0].copy(), lists[FROM_1][1].copy())
    d, _ = drawn((dense_bound(max_doc, 256) // BLOCK + 2) * BLOCK + 5)
    lists[FREQ11_DENSE] = (d, ballot_freqs(rng, d.size, False))
    d, _ = drawn(3 * BLOCK + 50)
    lists[FREQ11_SPARSE] = (d, ballot_freqs(rng, d.size, True))
    d, f = drawn(200)
    for at, v in BIG_FREQS.items():
        f[at] = v
    lists[BIG_FREQ] = (d, f)
    lists[CONST] = (every[CONST_LO:CONST_HI].copy(), np.full(CONST_HI - CONST_LO, CONST_FREQ, np.int32))
    return lists


def build_norms(max_doc, kind):
    rng = np.random.default_rng([max_doc, 8])
    if kind == "none":
        return None
    if kind == "rank":
        nb = rng.integers(95, 125, size=max_doc).astype(np.uint8)
    else:
        assert kind == "raw"
        nb = RAW_BYTES[rng.integers(0, RAW_BYTES.size, size=max_doc)]
        at = rng.permutation(np.concatenate([np.arange(CONST_LO), np.arange(CONST_HI, max_doc)]))[:RAW_BYTES.size]
        nb[at] = RAW_BYTES    # every byte present whatever the draw, outside CONST's docs
    nb[CONST_LO:CONST_HI] = TIE_BYTE
    return nb


def only_dense_doc(lists, max_doc):
    """The first doc from 5000 on that no list below the default window's dense bound holds (FROM_0 holds every doc)."""
    sparse = np.zeros(max_doc, bool)
    for d, _ in lists:
        if d.size < max(BLOCK, dense_bound(max_doc, DEFAULT_W)):
            sparse[d] = True
    return 5000 + int(np.flatnonzero(~sparse[5000:])[0])


class _Built:
    """Lists, norms and .doc bytes of one (max_doc, norms, version): shared by the live variants."""

    def __init__(self, max_doc, norms, version):
        from rucene_amd import indexgen
        self.lists = build_lists(max_doc)
        self.norms = build_norms(max_doc, norms)
        self.seg = indexgen.build_explicit(max_doc, self.lists, norms=self.norms, version=version)
        self.has = np.zeros((N_TERMS, max_doc), bool)
        for t, (d, _) in enumerate(self.lists):
            self.has[t, d] = True
        assert [int(x) for x in self.seg.terms["doc_freq"]] == [d.size for d, _ in self.lists]


_built = {}


class Leaf:
    """One fixture leaf; the attributes tests/segment_spectrum.py's Leaf has, so that its set algebra and the dismax / boosting
    references take it."""

    def __init__(self, max_doc=MAX_DOC, norms="rank", live="none", version=1):
        assert norms in NORMS and live in LIVE and version in VERSIONS
        key = (max_doc, norms, version)
        if key not in _built:
            _built[key] = _Built(max_doc, norms, version)
        b = _built[key]
        self.key = key + (live,)
        self.max_doc, self.lists, self.norms, self.seg, self.has = max_doc, b.lists, b.norms, b.seg, b.has
        self.norms_kind, self.live, self.version, self.doc_base, self.sttf = norms, live, version, 0, STTF_PER_DOC * max_doc
        self.only_dense_doc = only_dense_doc(self.lists, max_doc)
        self.alive = np.ones(max_doc, bool)
        if live == "seeded":
            self.alive = np.random.default_rng([max_doc, 9]).random(max_doc) < 0.85
            self.alive[list(DELETED_AT_EDGES) + [self.only_dense_doc]] = False
        self.live_docs = None if live == "none" else ss.live_words(self.alive)

    def oracle_segment(self, oracle):
        return oracle.Segment(self.seg.doc_bytes, self.norms, self.max_doc, self.seg.terms, doc_base=0, live_docs=self.live_docs,
                              sum_total_term_freq=self.sttf)

    def tail_n(self, t):
        df = self.lists[t][0].size
        return 0 if df == 1 else df % BLOCK    # (a singleton lives in its dictionary entry)


# ---- queries ------------------------------------------------------------------------------------------------------------------------
ALL_TERMS = list(range(N_TERMS))
# sparse at every W on both leaves (below dense_bound(4096), or shorter than a block): they fill clause positions without ever being dense
SPARSE_POOL = (EDGE_1K, EDGE_256, DF_127, FIRST_OF_WINDOW, LAST_DOC, STRETCH_63, STRETCH_64, STRETCH_65)
DENSE_POOL = (FROM_0, FROM_1, EDGE_1K, COPY, FROM_127)   # every doc of EDGE_1K from 127 on is held by all five


def _fill(n, special, pool=SPARSE_POOL):
    """n SHOULD clauses: `special` {index: term}, the pool in turn everywhere else."""
    return tuple(special.get(i, pool[i % len(pool)]) for i in range(n))


def _family_a():
    qs = [Query(should=(t, ABSENT)) for t in ALL_TERMS]   # every list alone (a single SHOULD clause is a TermQuery: ABSENT keeps it an OR)
    qs += [Query(should=s) for s in [(EDGE_1K, EDGE_256), (EDGE_256, EDGE_1K), (EDGE_1K, EDGE_1K), (EDGE_1K, FROM_0), (EDGE_256, FROM_1),
                                     (EDGE_1K, LAST_DOC), (FIRST_OF_WINDOW, LAST_DOC), (EDGE_256, CONST), (CONST, EDGE_1K, EDGE_256)]]
    for i, s in enumerate(STRETCHES):                      # a stretch at clause index 7, at 8, and two of them at 7 and 8
        other = list(STRETCHES)[(i + 1) % len(STRETCHES)]
        seven = (EDGE_1K, EDGE_256, DF_127, BELOW_4K, FIRST_OF_WINDOW, LAST_DOC, BIG_FREQ)
        qs += [Query(should=seven + (s,)), Query(should=seven + (FREQ11_SPARSE, s)), Query(should=seven + (s, other))]
    qs += [Query(should=s) for s in [
        (EDGE_1K, DF_127, STRETCH_64),                                     # no dense-eligible clause at any W
        (EDGE_1K, FROM_1, DF_127),                                         # one
        (FROM_0, EDGE_256, FROM_127),                                      # two
        (TWIN_A, FROM_128, TWIN_B),                                        # three, two of them of equal doc_freq
        (FROM_0, FROM_1, FROM_127, FROM_128),                              # four
        (FROM_128, FROM_0, EDGE_1K, FROM_1, TAIL_0, FROM_127),             # five: FROM_128, the shortest, goes through a run
        (TWIN_B, TWIN_A, FROM_0, FROM_1, FROM_127, SPAN),                  # six: the fourth place is a tie, TWIN_B (the earlier) takes it
        (TAIL_0, TAIL_1, TAIL_127, SPAN), (SPAN, EDGE_256), (FREQ11_DENSE, FREQ11_SPARSE, BIG_FREQ), (CONST, FREQ11_DENSE),
        (BELOW_256, ABOVE_256), (BELOW_1K, ABOVE_1K), (BELOW_4K, ABOVE_4K), (BELOW_256, ABOVE_256, BELOW_1K, ABOVE_1K, BELOW_4K, ABOVE_4K),
        (FROM_0, FROM_0), (FROM_1, EDGE_1K, FROM_1), (COPY, FROM_1), (TAIL_127, TAIL_127, TAIL_127)]]   # the same dense term twice
    return qs


def _family_b():
    qs = []
    for n in (10, 16, 17, 33, 63, 64):
        qs.append(Query(should=_fill(n, {}), msm=2))
        qs += [Query(should=_fill(n, {}, DENSE_POOL), msm=m) for m in (2, n, n + 1)]
    qs += [Query(should=_fill(17, {15: FROM_0}), msm=2), Query(should=_fill(17, {16: FROM_0}), msm=2),     # dense-eligible at 15 | 16
           Query(should=_fill(20, {3: FROM_1, 15: FROM_127, 16: FROM_0, 19: TAIL_0}), msm=2),
           Query(should=_fill(64, {0: FROM_128, 8: STRETCH_63, 15: STRETCH_64, 16: STRETCH_65, 40: STRETCH_128, 63: STRETCH_129}), msm=2),
           Query(should=_fill(64, {8: STRETCH_129, 15: STRETCH_128, 16: STRETCH_64, 63: STRETCH_65}, (EDGE_1K, EDGE_256, FROM_1, DF_127)), msm=3),
           Query(should=(EDGE_1K,) * 12, msm=2), Query(should=(EDGE_1K,) * 12, msm=12), Query(should=(EDGE_1K,) * 12, msm=13),   # duplicates count twice
           Query(should=(EDGE_256, EDGE_256, FROM_0, DF_127), msm=2), Query(should=(FROM_0, FROM_0, ABSENT), msm=2),
           Query(should=(FROM_0, FROM_1, EDGE_256, CONST), msm=4), Query(should=(FIRST_OF_WINDOW, LAST_DOC), msm=2)]
    return qs


NOT_SETS = ((EDGE_256,), (DF_127, EDGE_1K), (STRETCH_64, FIRST_OF_WINDOW, BELOW_4K), (ABSENT, STRETCH_129), (LAST_DOC,), (EDGE_1K, EDGE_256, CONST))


def _family_c(a):
    qs = [Query(should=q.should, must_not=NOT_SETS[i % len(NOT_SETS)]) for i, q in enumerate(a)]   # clause positions shifted by n_not
    qs += [Query(should=(FROM_1, EDGE_1K), must_not=(FROM_0,)), Query(should=(EDGE_1K, DF_127), must_not=(FROM_0,)),      # every doc prohibited
           Query(should=(FROM_0, FROM_1, FROM_127), must_not=(EDGE_1K,)), Query(should=(FROM_128, TAIL_0), must_not=(EDGE_256, EDGE_1K)),
           Query(should=_fill(61, {5: FROM_0, 15: FROM_1}), must_not=(EDGE_256, STRETCH_64, DF_127), msm=2),            # 61 + 3 = 64 positions
           Query(should=_fill(40, {0: FROM_127}), must_not=_fill(24, {0: BELOW_1K}), msm=2),                               # 40 + 24
           Query(should=(FIRST_OF_WINDOW, STRETCH_65), must_not=(EDGE_1K,)),                                               # docs only MUST_NOT holds
           Query(should=(STRETCH_63, ABSENT), must_not=(FROM_128, EDGE_256)),
           Query(should=(FROM_0, FROM_1, EDGE_256, DF_127), must_not=(EDGE_1K,), msm=2),
           Query(should=(FROM_0, FROM_1, EDGE_256, DF_127), must_not=(EDGE_1K, CONST), msm=3),
           Query(should=(FROM_0, EDGE_1K, EDGE_1K), must_not=(EDGE_1K,), msm=2)]
    return qs


def _family_d():
    ten = [Query(should=_fill(10, {})), Query(should=_fill(10, {0: FROM_0, 3: FROM_1, 5: FROM_127, 9: FROM_128})),
           Query(should=_fill(16, {15: FROM_0})), Query(should=(EDGE_1K, EDGE_256) * 6), Query(should=_fill(12, {8: STRETCH_129, 2: SPAN}), msm=1)]
    more = [Query(should=_fill(17, {15: FROM_1, 16: FROM_0})), Query(should=_fill(33, {8: STRETCH_128, 16: TAIL_1})),
            Query(should=_fill(64, {15: STRETCH_129, 16: STRETCH_65, 63: STRETCH_64, 1: FREQ11_DENSE})),
            Query(should=_fill(12, {4: FROM_0}), must_not=(EDGE_1K,)), Query(should=_fill(10, {}), must_not=(FROM_127, DF_127))]
    return ten, more


FAMILY_A = _family_a()
FAMILY_B = _family_b()
FAMILY_C = _family_c(FAMILY_A)
FAMILY_D10, FAMILY_D17 = _family_d()   # D10: routed to k_or_windows only when forced; D17: always (17 or more clauses, or MUST_NOT)
FAMILY_D = FAMILY_D10 + FAMILY_D17
EXACT = {"A": FAMILY_A, "B": FAMILY_B, "C": FAMILY_C}


def is_heap_order(q, leaf=None):
    """The reference sums this query's clauses in heap order: ten or more SHOULD clauses with a scorer, min_should_match <= 1."""
    n = len(q.should) if leaf is None else sum(1 for t in q.should if leaf.lists[t][0].size > 0)
    return n >= 10 and q.msm <= 1


def mixed():
    """A, B and C dealt into one batch in turn -> (queries, {family: row indexes in family order})."""
    out, rows = [], {name: [] for name in EXACT}
    for i in range(max(len(f) for f in EXACT.values())):
        for name, fam in EXACT.items():
            if i < len(fam):
                rows[name].append(len(out))
                out.append(fam[i])
    return out, rows


def cycled(n):
    """n queries: A, B and C in turn, over and over."""
    each = mixed()[0]
    return [each[i % len(each)] for i in range(n)]


def oracle_rows(oracle, osr, queries, k):
    return ss.oracle_rows(oracle, osr, queries, k)


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------
def ref_docs(leaf, q):
    """Docs that match q, ascending: set algebra over the input lists and the live mask (a clause given twice counts twice)."""
    return ss.ref_leaf_docs(leaf, q)


class OrRef:
    """Rows that do not go through the oracle's disjunction scorer: ref_docs for the hit set, and per doc the f32 sum, in clause order
    from `0.0f + s`, of the oracle's TermScorer scores (Searcher.score_docs with OP_TERM) of the SHOULD clauses that hold it."""

    def __init__(self, oracle, leaf, osr=None):
        self.oracle, self.leaf = oracle, leaf
        self.osr = osr or oracle.Searcher([leaf.oracle_segment(oracle)])
        self._clauses = {}

    def clause(self, t):
        if t not in self._clauses:
            docs = self.leaf.lists[t][0]
            docs = docs[self.leaf.alive[docs]].astype(np.int32)
            scores, matched = self.osr.score_docs(self.oracle.OP_TERM, [t], docs)
            assert matched.all(), ("the oracle's TermScorer does not hold a live doc of the fixture's list", t)
            scores.setflags(write=False)
            self._clauses[t] = (docs, scores)
        return self._clauses[t]

    def scores(self, q):
        """-> (matching docs ascending, their f32 clause-order sums)."""
        total = np.zeros(self.leaf.max_doc, np.float32)
        touched = np.zeros(self.leaf.max_doc, bool)
        for t in q.should:
            d, s = self.clause(t)
            total[d] = (np.where(touched[d], total[d], np.float32(0.0)) + s).astype(np.float32)   # score = 0.0; score += s
            touched[d] = True
        docs = ref_docs(self.leaf, q)
        assert touched[docs].all()
        return docs.astype(np.int32), total[docs]

    def row(self, q, k):
        """-> (docs, scores, total_hits): score descending, doc ascending, cut at k."""
        docs, sc = self.scores(q)
        order = np.lexsort((docs, -sc.astype(np.float64)))[:k]
        return docs[order], sc[order], int(docs.size)
