"""Fixtures and the reference for BooleanQuery of SHOULD / MUST_NOT clauses with exact PhraseQuery clauses among the SHOULD ones
("a b" "c d" e -f: rgpu_search_phrase_or_batch). Plain Python / numpy; tests/test_phrase_or_cpu.py proves them,
tests/test_gpu_phrase_or.py runs them on the device.

The oracle has no boolean-over-phrase scorer, so expected rows are composed from tests/phrase_bool.py's Index: per leaf, the
clauses that exist there (a phrase with a term of doc_freq 0 and a term of doc_freq 0 drop out) give their {doc: f32 score} lists
from the oracle (Index.clause_scores); a doc of their union scores np.float32(0.0), then += each clause that holds it, in query
order, all in f32 (disjunction_scorer.rs:213-225); it is a hit when at least min_should_match of the present clauses hold it
(:317-329; a dropped clause leaves min_should_match as it is); MUST_NOT docs and deleted docs are removed; the row is ranked
canonically (score desc, doc asc).

Fixtures (holdings {doc: {term: [positions]}} as in tests/phrase_rescore.py):
  main()   3100 docs = four run-building buckets of 1024 docs (the last one short) and thirteen 256-doc windows.
           WIDE   "W1 W2": 405 candidates (three full blocks and a tail of the lead: at one block per conjunction item the candidates
                  are appended by four wavefronts in whatever order they finish), two thirds of them matches; matches on docs 0, 255,
                  256 (a window's last doc and the next one's first), 1023, 1024, 2047 (bucket edges) and 3099 (max_doc - 1).
           C0 / C1 / C63 / C64 / C65   phrases with that many matches in bucket 1 (docs 1024..2047) beside candidates that do not
                  match; the last three also match once in bucket 0 and once in bucket 2 (the buckets' offsets in the run).
           FULL   matches every doc of bucket 0 and of bucket 2, none of bucket 1 (candidates there, no match).
           ONE    cost 1 (its lead is a singleton term), TWO cost 2.
           DENSE  a term of 2066 docs (a dense clause of the window kernel: df * W >= 64 * max_doc for every window width),
           T300   a sparse term, T5 five docs (0, 7, 14, 1024, 2047: WIDE matches 0, 1024 and 2047 are not phrase-only),
           NOT1   a MUST_NOT term on docs 21, 1023 and 3099 (1023 and 3099: docs only WIDE matches), ABSENT.
  tests/phrase_bool.py's main() and leaves() serve the sum-order, shared-term, gapped, boost-0 and multi-leaf cases."""
import numpy as np

import phrase_bool as pb
import phrase_rescore as pr
from phrase_bool import Ph, check_row, rank  # noqa: F401  (re-exported for the tests)

f32 = np.float32
UNSUPPORTED, ILLEGAL_ARGUMENT, ILLEGAL_STATE = -5, -2, -1
CANDIDATES = "k_search_and(phrase-or candidates)"
RUN_KERNELS = ("k_phrase_run_fill", "k_phrase_run_count", "k_phrase_run_scan", "k_phrase_run_scatter", "k_phrase_run_sort")
WINDOWS = "k_or_windows"
BUCKET = 1024   # PHRASE_OR_BUCKET (kernels/search_phrase_or.hpp)


class Q:
    """shoulds: term ids (int) and Ph clauses, in query order; must_nots: term ids; msm: min_should_match as given to build()."""

    def __init__(self, shoulds, must_nots=(), msm=0, name=""):
        self.shoulds, self.must_nots, self.msm, self.name = list(shoulds), list(must_nots), msm, name

    def build(self, raw=False):
        """raw: the BooleanQuery as it is, also where BooleanQuery::build would hand back its only clause (a lone phrase)"""
        import rucene_amd
        T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery

        def mk(c):
            return P(c.terms, c.positions, boost=c.boost) if isinstance(c, Ph) else T(c)
        shoulds, nots = [mk(c) for c in self.shoulds], [T(t) for t in self.must_nots]
        if raw:
            return B([], shoulds, self.msm if self.msm > 0 else 1, nots, [])
        return B.build([], shoulds, must_nots=nots, min_should_match=self.msm)

    def __repr__(self):
        return "Q(%s%r -%r msm %d)" % (self.name + ": " if self.name else "", self.shoulds, self.must_nots, self.msm)


def present(fx, q):
    """the SHOULD clauses that have a scorer in this leaf, in query order"""
    return [c for c in q.shoulds if pb.clause_cost(fx, c) > 0]


def leaf_rows(ix, li, q, order=None):
    """{global doc: f32 sum} of leaf li; order: a permutation of the present clauses' indexes (default: query order)"""
    fx = ix.fxs[li]
    cs = present(fx, q)
    if not cs:
        return {}
    per = [ix.clause_scores(li, c) for c in cs]
    per = per if order is None else [per[i] for i in order]
    gone = set(ix.deleted[li])
    for t in q.must_nots:
        gone |= set(fx.docs_of(t))
    out = {}
    for d in sorted(set().union(*[set(p) for p in per]) - gone):
        s, n = f32(0.0), 0
        for p in per:
            if d in p:
                s = f32(s + f32(p[d]))
                n += 1
        if n >= q.msm:
            out[d + ix.bases[li]] = s
    return out


def rows(ix, q):
    """-> (docs, scores) of every hit, canonical order (cached on the Index, left unchanged)"""
    key = ("phrase-or", repr(q))
    if key not in ix._rows:
        scored = {}
        for li in range(len(ix.fxs)):
            scored.update(leaf_rows(ix, li, q))
        d, s = rank(scored)
        d.setflags(write=False)
        s.setflags(write=False)
        ix._rows[key] = (d, s)
    return ix._rows[key]


# ---- main() -------------------------------------------------------------------------------------------------------------------------
(W1, W2, C0A, C0B, C1A, C1B, C63A, C63B, C64A, C64B, C65A, C65B, F1, F2, S1, S2, D1, D2, DENSE, T300, T5, NOT1, ABSENT) = range(23)
MAIN_TERMS, MAIN_DOCS = 23, 3100
WIDE, C0, C1, C63, C64, C65 = Ph((W1, W2)), Ph((C0A, C0B)), Ph((C1A, C1B)), Ph((C63A, C63B)), Ph((C64A, C64B)), Ph((C65A, C65B))
FULL, ONE, TWO = Ph((F1, F2)), Ph((S1, S2)), Ph((D1, D2))
WIDE_EDGES = (0, 255, 256, 1023, 1024, 2047, 3099)
WIDE_DOCS = sorted(set(range(0, 2793, 7)) | set(WIDE_EDGES))
WIDE_MATCHES = [d for d in WIDE_DOCS if d in WIDE_EDGES or d % 3 != 1]
T5_DOCS = (0, 7, 14, 1024, 2047)
NOT1_DOCS = (21, 1023, 3099)
COUNTS = {0: C0, 1: C1, 63: C63, 64: C64, 65: C65}


def count_matches(n):
    """the docs phrase C<n> matches: n in bucket 1; from 63 on, one more in bucket 0 and one in bucket 2"""
    return ([500] if n >= 63 else []) + [1100 + 3 * i for i in range(n)] + ([2500] if n >= 63 else [])


def _main_holdings():
    h = {}

    def put(d, t, ps):
        cur = h.setdefault(d, {}).setdefault(t, [])
        cur.extend(ps)
        cur.sort()

    def pair(c, match, miss, base):
        ta, tb = c.terms
        for d in match:   # every eleventh doc holds the phrase twice
            put(d, ta, [base, base + 10] if d % 11 == 0 else [base])
            put(d, tb, [base + 1, base + 11] if d % 11 == 0 else [base + 1])
        for d in miss:    # both terms, not next to each other
            put(d, ta, [base])
            put(d, tb, [base + 4])
    pair(WIDE, WIDE_MATCHES, [d for d in WIDE_DOCS if d not in WIDE_MATCHES], 1)
    for d in range(5, 3000, 61):          # W2 alone: W1 is the rarer term and leads the conjunction
        if d not in WIDE_DOCS:
            put(d, W2, [3])
    for n, c in COUNTS.items():
        pair(c, count_matches(n), [600] + list(range(1400, 1410)), 20)
    pair(FULL, list(range(0, 1024)) + list(range(2048, 3072)), list(range(1500, 1510)), 40)
    put(1500, S1, [60])                   # cost 1: a singleton lead
    for d, p in ((1500, 61), (1600, 61), (1700, 70)):
        put(d, S2, [p])
    for d in (10, 3000):                  # cost 2
        put(d, D1, [62])
    for d in (10, 2000, 3000):
        put(d, D2, [63])
    for d in range(MAIN_DOCS):
        if d % 3 != 0:
            put(d, DENSE, [80, 81] if d % 5 == 0 else [80])
    for d in list(range(2, MAIN_DOCS, 10))[:300]:
        put(d, T300, [85] if d % 4 else [85, 87])
    for d in T5_DOCS:
        put(d, T5, [90])
    for d in NOT1_DOCS:
        put(d, NOT1, [95])
    return h


def main():
    if "po-main" not in pr._built:
        fx = pr.Fixture("po-main", MAIN_DOCS, MAIN_TERMS, _main_holdings(), 31)
        assert len(fx.postings[W1]) == len(WIDE_DOCS) == 405 and len(fx.postings[W2]) > 405      # three full blocks and a tail lead the conjunction
        assert [len(fx.postings[t]) for t in (S1, S2, D1, D2, T300, T5, ABSENT)] == [1, 3, 2, 3, 300, 5, 0]
        assert len(fx.postings[DENSE]) * 256 >= 64 * MAIN_DOCS                                    # dense under the narrowest window
        pr._built["po-main"] = fx
    return pr._built["po-main"]


PHRASE_ONLY = [d for d in WIDE_MATCHES if d not in T5_DOCS]   # the docs of [WIDE, T5] that only the phrase holds

ORDER_QUERIES = [Q([WIDE, T300], name="candidates appended by four wavefronts"), Q([WIDE], name="the lone wide phrase")]
BUCKET_QUERIES = [Q([c, T5], name="%d matches in bucket 1" % n) for n, c in COUNTS.items()] + [
    Q([FULL, T5], name="an empty bucket between two full ones"), Q([ONE, T5], name="cost 1"), Q([TWO, T5], name="cost 2"),
    Q([C0], name="candidates, no match, alone"), Q([ONE], name="cost 1 alone"), Q([C64, C65, C63, FULL], name="four phrases, no term")]
WINDOW_QUERIES = [Q([WIDE, DENSE], name="a dense term beside the phrase"), Q([DENSE, WIDE, T300], name="dense, phrase, sparse"),
                  Q([WIDE, T5], name="window edges")]
MSM_QUERIES = [Q([WIDE, DENSE, T300], msm=2, name="msm 2 of 3"), Q([WIDE, DENSE, T300], msm=3, name="msm n"),
               Q([WIDE, DENSE, T300], msm=4, name="msm n + 1"), Q([WIDE, ABSENT, DENSE], msm=2, name="msm 2, a clause absent"),
               Q([WIDE, Ph((W1, ABSENT)), T5], msm=3, name="msm 3, a phrase dropped: nothing can reach it")]
NOT_QUERIES = [Q([WIDE, T300], [NOT1], name="MUST_NOT removes phrase-only docs"), Q([WIDE, T5], [NOT1, ABSENT, NOT1], name="MUST_NOT twice and absent"),
               Q([WIDE], [NOT1], name="a lone phrase with MUST_NOT"), Q([WIDE, DENSE], [T300], msm=2, name="msm and MUST_NOT")]
MAIN_QUERIES = ORDER_QUERIES + BUCKET_QUERIES + WINDOW_QUERIES + MSM_QUERIES + NOT_QUERIES + [
    Q([Ph((W1, ABSENT)), ABSENT], name="every clause absent"), Q([ABSENT, WIDE, ABSENT], name="absent terms around the phrase")]

# ---- tests/phrase_bool.py's main(): the sum order ------------------------------------------------------------------------------------
AB, BC, GAP = pb.AB, pb.BC, pb.GAP
AB0 = Ph((pb.PA, pb.PB), None, 0.0)
SUM_ORDER = [Q([AB, pb.D600, pb.T129], name="P T T"), Q([pb.D600, AB, pb.T129], name="T P T"), Q([pb.D600, pb.T129, AB], name="T T P")]
PB_QUERIES = SUM_ORDER + [
    Q([AB, AB], name="the same phrase twice"), Q([AB, BC], name="two phrases sharing PB"), Q([GAP, pb.R20], name="a gapped phrase"),
    Q([AB0, pb.R20], name="boost 0: the phrase-only docs count"), Q([AB0, pb.R20, pb.T40], msm=2, name="boost 0 counts towards msm"),
    Q([AB, BC, pb.ABC, GAP, pb.D600, pb.T129, pb.T40, pb.R20, pb.S], name="nine clauses, four phrases"),
    Q([pb.S, AB], [pb.N1], name="a singleton term clause"), Q([Ph((pb.PB, pb.PC)), pb.D600], name="eleven positions in a doc")]
LEAF_QUERIES = [Q([AB, pb.R20], name="a leaf without the term, a leaf without the phrase"),
                Q([AB, Ph((pb.PA, pb.PC), (0, 15))], name="a leaf without every clause"),
                Q([pb.T129, AB, pb.D600], [pb.N1], msm=2, name="msm and MUST_NOT over three leaves")]


# ---- heavy(): a doc that holds a phrase term 1025 times — past the widest position lists, the match stage refuses the call --------------
H1, H2, H3 = range(3)
HEAVY = Ph((H1, H2))
HEAVY_DOC = 5


def heavy():
    if "po-heavy" not in pr._built:
        h = {d: {H1: [0], H2: [1], H3: [4]} for d in range(10)}
        h[HEAVY_DOC] = {H1: [2 * i for i in range(1025)], H2: [1], H3: [3000]}
        pr._built["po-heavy"] = pr.Fixture("po-heavy", 40, 3, h, 32)
    return pr._built["po-heavy"]
