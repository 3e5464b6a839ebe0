"""Fixtures and the reference for BooleanQuery with exact PhraseQuery clauses (+"a b" +c -d #e: rgpu_search_phrase_bool_batch). Plain
Python / numpy; tests/test_phrase_bool_cpu.py proves them, tests/test_gpu_phrase_bool.py runs them on the device.

The oracle has no boolean-over-phrase scorer, so expected rows are composed (as tests/boosting_ref.py composes a BoostingQuery's):
per leaf, PositionsIndex.phrase_search(k = max_doc, live_docs = None) gives each phrase's {doc: f32 score}; an oracle.Segment over the
same .doc bytes and Searcher.search(OP_TERM, k = max_doc) give each term clause's scores with the same collection statistics (its
TermScorer walked with next(): score_docs would advance through a positions field's skip data, which the oracle's plain Segment
does not parse); the docs
are intersected, MUST_NOT and deleted docs dropped, the scores summed in np.float32 in the stable cost order of THAT leaf's doc freqs
(conjunction_scorer.rs:27-42, 87-95: first addend as it is, the rest +=), and the row ranked canonically (score desc, doc asc).
A leaf in which a required term or a phrase term has no posting matches nothing. FILTER clauses score +0.0.

A phrase's weight is computed by the oracle from the doc freqs of the index it searches, and the reference from the statistics
leaf's: in the multi-leaf index every leaf holds the phrase terms in the same number of docs as the statistics leaf (the term
clauses' doc freqs differ between leaves — that is what makes the cost order differ).

Fixtures (holdings {doc: {term: [positions]}} as in tests/phrase_rescore.py):
  main()    700 docs. Phrase terms PA (df 40, all inside PB's docs), PB (df 129: posting 127 = doc 254, posting 128 = the tail, doc
            256), PC (df 60). Term clauses of the four kinds the scoring kernel tells apart: S (df 1, the singleton doc 24), R20
            (df 20), R30 (df 30), T40 (df 40: the phrase's cost), T129 (df 129, PB's docs: a match on the last posting of the full block and
            on the first of the tail), D600 (df 600: a doc bitmap in the candidate conjunction). MUST_NOT terms N1 (holds what would
            be the top hit), N2, N3 and ABSENT. Doc 72 holds PC eleven times: past the 64-candidate kernel's lists, in a plane
            other than 0 of +"PA PB" +"PB PC".
  groups()  400 docs, X and Y in docs 0..299, "X Y" a phrase except in the odd docs below 128. Lead terms L63 / L64 / L65 (63, 64, 65
            candidates), L192 (docs 0..191: the conjunction emits a full block's even postings, then its odd ones, then the tail,
            so the middle 64-slot group holds the odd docs — no survivor between two groups that have some), LZ (docs the phrase
            terms lack: a query with no candidate), LK (docs 0..299: 236 hits for the k ladder).
  leaves()  main() as the statistics leaf; a second leaf with the same phrase lists but T129 cut to 20 docs (below the phrase's cost
            there: the order of +T129 +"PA PB" +D600 differs between the two leaves) and no R20; a third leaf without PA."""
from collections import namedtuple

import numpy as np

import phrase_rescore as pr

f32 = np.float32
UNSUPPORTED, ILLEGAL_ARGUMENT, ILLEGAL_STATE = -5, -2, -1
CANDIDATES = "k_search_and(phrase-bool candidates)"
FANOUT = "k_phrase_bool_fanout"
SCORE = "k_phrase_bool_score"

Ph = namedtuple("Ph", "terms positions boost")
Ph.__new__.__defaults__ = (None, 1.0)


class Q:
    """musts / filters: term ids (int) and Ph clauses, in query order; must_nots: term ids."""

    def __init__(self, musts, must_nots=(), filters=(), name=""):
        self.musts, self.must_nots, self.filters, self.name = list(musts), list(must_nots), list(filters), name

    def required(self):
        """BooleanWeight::must_weights: (clause, scores?) — MUST clauses in query order, then FILTER clauses"""
        return [(c, True) for c in self.musts] + [(c, False) for c in self.filters]

    def build(self):
        import rucene_amd
        T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery

        def mk(c):
            return P(c.terms, c.positions, boost=c.boost) if isinstance(c, Ph) else T(c)
        return B.build([mk(c) for c in self.musts], [], filters=[mk(c) for c in self.filters], must_nots=[T(t) for t in self.must_nots])

    def __repr__(self):
        return "Q(%s%r -%r #%r)" % (self.name + ": " if self.name else "", self.musts, self.must_nots, self.filters)


def phrase_positions(c):
    return list(range(len(c.terms))) if c.positions is None else list(c.positions)


def clause_cost(fx, c):
    """a term's cost: its doc_freq in the leaf; an exact phrase's: the smallest doc_freq among its terms"""
    return min(len(fx.postings[t]) for t in c.terms) if isinstance(c, Ph) else len(fx.postings[c])


def cost_order(fx, q):
    """indexes into q.required() in the order ConjunctionScorer adds the scores: a stable sort by cost"""
    req = q.required()
    return sorted(range(len(req)), key=lambda i: clause_cost(fx, req[i][0]))


def sum_in_order(addends):
    s = f32(addends[0])
    for a in addends[1:]:
        s = f32(s + f32(a))
    return s


def rank(scored):
    """{doc: f32} -> (docs, scores) canonically: score desc, doc asc"""
    d = np.array(sorted(scored), dtype=np.int32)
    s = np.array([scored[int(x)] for x in d], dtype=np.float32)
    order = np.lexsort((d, -s.astype(np.float64)))
    return d[order], s[order]


def live_words(max_doc, deleted):
    alive = np.ones(max_doc, dtype=bool)
    alive[list(deleted)] = False
    return np.packbits(np.concatenate([alive, np.zeros(-alive.size % 64, dtype=bool)]), bitorder="little").view(np.uint64).copy()


class Index:
    """Leaves (tests/phrase_rescore.py Fixture) with doc bases and deleted docs, beside the oracle's view of them."""

    def __init__(self, oracle, fxs, version=1, deleted=None):
        self.oracle, self.fxs, self.version = oracle, list(fxs), version
        self.bases = [int(b) for b in np.concatenate([[0], np.cumsum([fx.max_doc for fx in self.fxs])[:-1]])]
        self.deleted = [set() for _ in self.fxs] if deleted is None else [set(d) for d in deleted]
        self.ixs = [fx.index(oracle, version=version) for fx in self.fxs]
        self.max_doc = sum(fx.max_doc for fx in self.fxs)
        assert all(fx.max_doc <= self.fxs[0].max_doc for fx in self.fxs), "leaf 0 is the statistics leaf"
        self.stats = (self.max_doc, self.fxs[0].doc_count, self.fxs[0].sum_ttf)
        segs = []
        for fx, ix, base in zip(self.fxs, self.ixs, self.bases):
            segs.append(oracle.Segment(np.frombuffer(ix.files()[0], np.uint8), fx.norms, fx.max_doc, self.term_states(ix, len(fx.postings), oracle.TERM_STATE_DTYPE),
                                       doc_base=base, doc_count=fx.doc_count, sum_total_term_freq=fx.sum_ttf))
        self.segs = segs
        self.osr = oracle.Searcher(segs)
        self._phrase, self._term, self._rows = {}, {}, {}

    @staticmethod
    def term_states(ix, n, dtype):
        terms = np.zeros(n, dtype=dtype)
        for t in range(n):
            st = ix.term_state(t)
            terms[t] = (st["doc_start_fp"], st["skip_offset"], st["total_term_freq"], st["doc_freq"], st["singleton_doc_id"])
        return terms

    def live(self, li):
        return live_words(self.fxs[li].max_doc, self.deleted[li]) if self.deleted[li] else None

    def gpu_leaves(self):
        return [pr.leaf_of(ix, fx, doc_base=base, live_docs=self.live(li)) for li, (ix, fx, base) in enumerate(zip(self.ixs, self.fxs, self.bases))]

    def phrase_scores(self, li, c):
        """{leaf-local doc: f32} of an exact phrase in leaf li, boost 1 (the oracle: every doc the scorer matches, deleted or not)"""
        key = (li, tuple(c.terms), tuple(phrase_positions(c)))
        if key not in self._phrase:
            fx = self.fxs[li]
            for t in c.terms:
                assert len(fx.postings[t]) == len(self.fxs[0].postings[t]), "a phrase term's doc_freq is the statistics leaf's in every leaf that holds it"
            self._phrase[key] = fx.second(self.ixs[li], list(c.terms), 0, phrase_positions(c), 1.0, stats=self.stats)
        return self._phrase[key]

    def term_scores(self, li, t):
        """{leaf-local doc: f32} of a term clause in leaf li, weighed with the statistics leaf's doc_freq"""
        key = (li, t)
        if key not in self._term:
            # (the TermScorer walked with next(): the oracle's plain Segment reads a positions field's blocks, not its skip data)
            docs, scores, total = self.osr.search(self.oracle.OP_TERM, [t], self.max_doc, tie_mode=self.oracle.TIE_CANONICAL)
            assert docs.size == total == sum(len(fx.postings[t]) for fx in self.fxs)
            for lj, fx in enumerate(self.fxs):
                mine = (docs >= self.bases[lj]) & (docs < self.bases[lj] + fx.max_doc)
                self._term[(lj, t)] = {int(d) - self.bases[lj]: f32(s) for d, s in zip(docs[mine], scores[mine])}
                assert sorted(self._term[(lj, t)]) == fx.docs_of(t)
        return self._term[key]

    def clause_scores(self, li, c, scoring=True):
        raw = self.phrase_scores(li, c) if isinstance(c, Ph) else self.term_scores(li, c)
        zero = not scoring or (isinstance(c, Ph) and c.boost == 0.0)
        return {d: (f32(0.0) if zero else s) for d, s in raw.items()}

    def leaf_rows(self, li, q, order=None):
        """{global doc: f32 sum} of leaf li; order: indexes into q.required() (default: the leaf's stable cost order)"""
        fx = self.fxs[li]
        req = q.required()
        if any(clause_cost(fx, c) == 0 for c, _ in req):
            return {}
        per = [self.clause_scores(li, c, scoring) for c, scoring in req]
        docs = set(per[0])
        for p in per[1:]:
            docs &= set(p)
        for t in q.must_nots:
            docs -= set(fx.docs_of(t))
        docs -= self.deleted[li]
        order = cost_order(fx, q) if order is None else order
        return {d + self.bases[li]: sum_in_order([per[i][d] for i in order]) for d in docs}

    def rows(self, q):
        """-> (docs, scores) of every hit, canonical order"""
        key = repr(q)
        if key not in self._rows:
            scored = {}
            for li in range(len(self.fxs)):
                scored.update(self.leaf_rows(li, q))
            d, s = rank(scored)
            d.setflags(write=False)
            s.setflags(write=False)
            self._rows[key] = (d, s)
        return self._rows[key]

    def close(self):
        for ix in self.ixs:
            ix.close()


def check_row(row, total, want, what):
    """One row of the hit array ({doc, score}[k]) against (docs, scores) of every hit: docs, score bits, {-1, 0} padding, total_hits."""
    d, s = want
    k = row.size
    n = min(k, d.size)
    assert int(total) == d.size, (what, "total_hits", int(total), d.size)
    assert row["doc"][:n].tolist() == d[:n].tolist(), (what, "docs", row["doc"][:n].tolist()[:10], d[:n].tolist()[:10])
    assert row["score"][:n].view(np.uint32).tolist() == s[:n].view(np.uint32).tolist(), (what, "score bits", row["score"][:4], s[:4])
    assert (row["doc"][n:] == -1).all() and (row["score"][n:].view(np.uint32) == 0).all(), (what, "padding")


# ---- main() -------------------------------------------------------------------------------------------------------------------------
PA, PB, PC, S, R20, T40, T129, D600, N1, N2, N3, ABSENT, R30 = range(13)
MAIN_TERMS, MAIN_DOCS = 13, 700
PB_DOCS = [2 * i for i in range(129)]                         # 0 .. 256; posting 127 = doc 254, the tail = doc 256
PA_DOCS = sorted([6 * i for i in range(38)] + [254, 256])     # df 40, inside PB's docs
PC_DOCS = [4 * i for i in range(60)]                          # 0 .. 236
T40_DOCS = sorted([6 * i for i in range(30)] + [301 + 2 * i for i in range(8)] + [254, 256])   # df 40
R20_DOCS = sorted([12 * i for i in range(19)] + [254])        # df 20
R30_DOCS = [6 * i for i in range(30)]                         # df 30
SINGLETON_DOC, ELEVEN_DOC = 24, 72
AB = Ph((PA, PB))           # "PA PB": cost 40
BC = Ph((PB, PC))           # "PB PC": cost 60
ABC = Ph((PA, PB, PC))
ABA = Ph((PA, PB, PA))      # a repeated term
GAP = Ph((PA, PC), (0, 15))  # PA at p, PC at p + 15


def _ab_matches(d):
    return d in PA_DOCS and d % 12 != 6


def _main_holdings(t129_docs=None, with_r20=True, with_pa=True, max_doc=MAIN_DOCS):
    h = {}

    def put(d, t, ps):
        if d < max_doc:
            cur = h.setdefault(d, {}).setdefault(t, [])
            cur.extend(ps)
            cur.sort()
    for d in PB_DOCS:
        put(d, PB, [7, 11] if d % 24 == 0 else [7])
    if with_pa:
        for d in PA_DOCS:
            ps = ([6, 10] if d % 24 == 0 else [6]) if _ab_matches(d) else [3]
            put(d, PA, ps + ([8] if d % 30 == 0 else []))          # "PA PB PA" in the docs 0, 30, 60, ...
    for d in PC_DOCS:
        if d % 8 == 0 and d in PB_DOCS:
            put(d, PB, [20])
            put(d, PC, [21] + (list(range(30, 40)) if d == ELEVEN_DOC else []))
        else:
            put(d, PC, [25])
        if with_pa and d % 48 == 0 and d in PA_DOCS:
            put(d, PC, [12])                                       # "PA PB PC" at 10, 11, 12
    put(SINGLETON_DOC, S, [40])
    if with_r20:
        for d in R20_DOCS:
            put(d, R20, [41, 43] if d % 36 == 0 else [41])
    for d in R30_DOCS:
        put(d, R30, [47] if d % 5 else [47, 57])
    for d in T40_DOCS:
        put(d, T40, [44] if d % 4 else [44, 45, 46])
    for d in (PB_DOCS if t129_docs is None else t129_docs):
        put(d, T129, [48] if d % 10 else [48, 49])
    for d in range(max_doc):
        if d % 7 != 3:
            put(d, D600, [50] if d % 3 else [50, 52])
    for d in (0, ELEVEN_DOC, 254):   # (doc 72 scores highest under +"PA PB" +D600)
        put(d, N1, [55])
    put(24, N2, [55])
    for d in (36, 48, 500):
        put(d, N3, [55])
    return h


def main():
    if "pb-main" not in pr._built:
        fx = pr.Fixture("pb-main", MAIN_DOCS, MAIN_TERMS, _main_holdings(), 21)
        assert [len(fx.postings[t]) for t in (PA, PB, PC, S, R20, T40, T129, D600, ABSENT)] == [40, 129, 60, 1, 20, 40, 129, 600, 0]
        assert len(fx.postings[R30]) == 30
        assert fx.docs_of(T129)[127] == 254 and fx.docs_of(T129)[128] == 256
        pr._built["pb-main"] = fx
    return pr._built["pb-main"]


# the cost cases: three addends or more, so that two orders can differ in bits. "PA PB" costs 40. WRONG_ORDERS: what a scorer would
# add in that kept the query's order, or broke a tie the other way (indexes into required()).
ORDER_CASES = [
    Q([D600, AB, R20], name="term cost below the phrase's"),                   # R20, AB, D600
    Q([R20, AB, T40], name="equal cost, the phrase earlier"),                  # R20, AB, T40
    Q([R20, T40, AB], name="equal cost, the term earlier"),                    # R20, T40, AB
    Q([D600, T129, AB], name="term cost above the phrase's"),                  # AB, T129, D600
    Q([AB, R20, R30], name="the phrase third of three"),                       # R20, R30, AB
    Q([D600, AB, T129, R20, T40], name="five clauses"),                        # R20, AB, T40, T129, D600
]
WRONG_ORDERS = [[0, 1, 2], [0, 2, 1], [0, 2, 1], [0, 1, 2], [0, 1, 2], [0, 1, 2, 3, 4]]
MAIN_QUERIES = ORDER_CASES + [
    Q([AB, S], name="singleton clause"),
    Q([AB, T40], name="tail-only clause"),
    Q([AB, T129], name="block + one clause"),
    Q([AB, D600], name="bitmap clause"),
    Q([AB, BC], name="two phrases sharing PB"),
    Q([AB, BC, ABC, GAP], name="four phrases"),
    Q([AB, PA], name="a phrase and its own term"),
    Q([ABA, T129], name="a repeated term beside a term"),
    Q([GAP, D600], name="a gapped phrase"),
    Q([AB, BC, D600], name="eleven positions in plane 1"),
    Q([AB, D600], [N1], name="MUST_NOT removes the top hit"),
    Q([AB, D600], [N1, N2, N3], name="three MUST_NOT"),
    Q([AB, D600], [ABSENT], name="MUST_NOT absent from the leaf"),
    Q([AB], [N2], name="a lone phrase with MUST_NOT"),
    Q([AB, D600], filters=[T40], name="FILTER term"),
    Q([T129, D600], filters=[AB], name="FILTER phrase"),
    Q([Ph((PA, PB), None, 0.0), T129, D600], name="boost 0"),
    Q([AB, ABSENT], name="a required term absent"),
    Q([Ph((PA, ABSENT)), D600], name="a phrase term absent"),
]


# ---- groups() -----------------------------------------------------------------------------------------------------------------------
X, Y, L63, L64, L65, L192, LZ, LK = range(8)
XY = Ph((X, Y))
GROUPS_DOCS = 400


def _xy_matches(d):
    return d < 300 and not (d < 128 and d % 2 == 1)


def groups():
    if "pb-groups" not in pr._built:
        h = {}
        for d in range(300):
            h[d] = {X: [1, 5] if d % 9 == 0 else [1], Y: ([2, 6] if d % 9 == 0 else [2]) if _xy_matches(d) else [3]}
        for t, docs in ((L63, range(63)), (L64, range(100, 164)), (L65, range(200, 265)), (L192, range(192)), (LZ, range(300, 310)), (LK, range(300))):
            for d in docs:
                h.setdefault(d, {})[t] = [9] if d % 4 else [9, 10]
        pr._built["pb-groups"] = pr.Fixture("pb-groups", GROUPS_DOCS, 8, h, 22)
    return pr._built["pb-groups"]


GROUP_QUERIES = [Q([XY, L63], name="63 candidates"), Q([XY, L64], name="64 candidates"), Q([XY, L65], name="65 candidates"),
                 Q([XY, L192], name="a group without survivors"), Q([XY, LZ], name="no candidate"), Q([XY, LK], name="236 hits")]


# ---- leaves() -----------------------------------------------------------------------------------------------------------------------
def leaves():
    if "pb-leaves" not in pr._built:
        second = pr.Fixture("pb-leaf1", MAIN_DOCS, MAIN_TERMS, _main_holdings(t129_docs=PB_DOCS[100:120], with_r20=False), 23)
        third = pr.Fixture("pb-leaf2", 300, MAIN_TERMS, _main_holdings(with_pa=False, max_doc=300), 24)
        pr._built["pb-leaves"] = (main(), second, third)
    return pr._built["pb-leaves"]


LEAF_QUERIES = [Q([T129, AB, D600], name="the cost order differs between the leaves"), Q([R20, AB, T40], name="a leaf without the MUST term"),
                Q([AB, BC, D600], [N1], name="two phrases over three leaves"), Q([AB, D600], filters=[T40], name="FILTER over three leaves")]
