"""Fixtures for doc sets - cached filters as FILTER / MUST_NOT masks (plain Python, no GPU).

EQUIV is the leaf of the CPU proof (tests/test_docset_cpu.py): a query Q with a FILTER term f and a MUST_NOT term g on live docs L
collects what Q alone collects on live docs L AND docs(f) AND NOT docs(g). Its filter terms are cheaper than every clause of Q
(F_CHEAP), between them (F_MID) and dearer than all of them (F_DEAR), so the zero-score clause stands first, in the middle and last
in ConjunctionScorer's cost order; the MUST + SHOULD query matches 1500 docs, so ReqOptScorer's skipping rule (after 100 docs) fires.

COLLECT is the leaf rgpu_docset_collect_batch is held against: lists of 1 (a singleton in the term-dictionary entry), 127 (a VInt
tail alone), 128 (one block, no tail), 129, 2176 and 2304 postings (17 | 18 blocks: either side of a work item of four blocks, and
of a tail), one holding every second doc (dense enough for a doc bitmap), an absent term, and sixteen seeded lists for wide
disjunctions. max_doc 20001: the last word holds one doc. The reference is numpy set algebra over the raw lists; live docs are NOT
applied (the query cache fills its sets without them, search/cache/query_cache.rs:335-342).

Queries are segment_spectrum.Query records; pack() writes them as the rgpu_query[] / rgpu_query_term[] of the C ABI."""
import numpy as np

import segment_spectrum as ss
from segment_spectrum import Query

# ---- the equivalence leaf -------------------------------------------------------------------------------------------------------
EQ_MAX_DOC = 3001
EQ_NAMES = ["A", "B", "C", "F_CHEAP", "F_MID", "F_DEAR", "G", "S1", "S2"]
A, B, C, F_CHEAP, F_MID, F_DEAR, G, S1, S2 = range(len(EQ_NAMES))
EQ_DFS = {A: 1500, B: 600, C: 250, F_CHEAP: 120, F_MID: 1000, F_DEAR: 2500, G: 700, S1: 900, S2: 300}
EQ_FILTERS = (F_CHEAP, F_MID, F_DEAR)
# (must, should): TERM, conjunctions of two and three clauses in two clause orders, MUST + SHOULD (ReqOptScorer)
EQ_QUERIES = [((A,), ()), ((A, B), ()), ((B, A), ()), ((A, B, C), ()), ((C, A, B), ()), ((A,), (S1, S2)), ((B, A), (S1,))]
EQ_KS = (10, 200)


def _freqs(rng, n):
    return np.minimum(10, rng.geometric(0.5, size=n)).astype(np.int32)


def _drawn(rng, max_doc, df):
    d = np.sort(rng.choice(max_doc, size=df, replace=False)).astype(np.int32)
    return d, _freqs(rng, df)


class _Leaf:
    """lists -> .doc bytes, term states, the per-term membership table; live variants share one build"""

    def __init__(self, max_doc, lists, norms, version=1, sttf_per_doc=60):
        from rucene_amd import indexgen
        self.max_doc, self.lists, self.norms, self.version = max_doc, lists, norms, version
        self.seg = indexgen.build_explicit(max_doc, lists, norms=norms, version=version)
        self.terms = self.seg.terms
        self.sttf = sttf_per_doc * max_doc
        self.has = np.zeros((len(lists), max_doc), bool)
        for t, (d, _) in enumerate(lists):
            self.has[t, d] = True
        assert [int(x) for x in self.terms["doc_freq"]] == [d.size for d, _ in lists]

    def oracle_segment(self, oracle, alive=None, doc_base=0):
        return oracle.Segment(self.seg.doc_bytes, self.norms, self.max_doc, self.terms, doc_base=doc_base,
                              live_docs=None if alive is None else ss.live_words(alive), sum_total_term_freq=self.sttf)


_cache = {}


def equiv_leaf():
    if "equiv" not in _cache:
        rng = np.random.default_rng([EQ_MAX_DOC, 11])
        lists = [_drawn(rng, EQ_MAX_DOC, EQ_DFS[t]) for t in range(len(EQ_NAMES))]
        # C inside B inside A, and half of F_CHEAP inside C: every conjunction below keeps docs under every filter
        a = np.arange(0, EQ_MAX_DOC - 1, 2, dtype=np.int32)
        b = np.sort(rng.choice(a, size=EQ_DFS[B], replace=False))
        c = np.sort(rng.choice(b, size=EQ_DFS[C], replace=False))
        cheap = np.unique(np.concatenate([rng.choice(c, size=EQ_DFS[F_CHEAP] // 2, replace=False), lists[F_CHEAP][0]]))[:EQ_DFS[F_CHEAP]]
        for t, d in ((A, a), (B, b), (C, c), (F_CHEAP, cheap)):
            lists[t] = (d.astype(np.int32), _freqs(rng, d.size))
        _cache["equiv"] = _Leaf(EQ_MAX_DOC, lists, rng.integers(95, 125, size=EQ_MAX_DOC).astype(np.uint8))
    return _cache["equiv"]


def seeded_alive(max_doc, salt=0, share=0.6):
    return np.random.default_rng([max_doc, salt, 61]).random(max_doc) < share


# ---- the collect leaf -----------------------------------------------------------------------------------------------------------
CO_MAX_DOC = 20001
CO_NAMES = ["ONE", "DF127", "DF128", "DF129", "DF2176", "DF2304", "DENSE", "ABSENT", "MID"] + ["R%d" % i for i in range(16)]
ONE, DF127, DF128, DF129, DF2176, DF2304, DENSE, ABSENT, MID = range(9)
R = list(range(9, 25))
CO_DFS = {ONE: 1, DF127: 127, DF128: 128, DF129: 129, DF2176: 2176, DF2304: 2304, DENSE: 10001, ABSENT: 0, MID: 700}
CO_TERM_LISTS = (ONE, DF127, DF128, DF129, DF2176, DF2304, DENSE)


def collect_lists():
    if "collect_lists" not in _cache:
        rng = np.random.default_rng([CO_MAX_DOC, 12])
        lists = [None] * len(CO_NAMES)
        for t, df in CO_DFS.items():
            lists[t] = _drawn(rng, CO_MAX_DOC, df) if df else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        lists[ONE] = (np.array([CO_MAX_DOC - 1], np.int32), np.array([3], np.int32))        # the one doc of the last word
        lists[DENSE] = (np.arange(0, CO_MAX_DOC, 2, dtype=np.int32), _freqs(rng, 10001))    # doc 0 and doc max_doc - 1 included
        d, f = lists[DF127]
        d[0] = 0                                                                             # (sorted and distinct still: the draw's docs are distinct and >= 0)
        lists[DF127] = (np.unique(d), f[:np.unique(d).size])
        for i, t in enumerate(R):
            lists[t] = _drawn(rng, CO_MAX_DOC, 40 + 37 * i)
        # runs of neighbouring docs inside one list: many postings of one block in one 32-bit word, and a run across a word edge
        d = np.unique(np.concatenate([lists[MID][0][:600], np.arange(4000, 4100, dtype=np.int32)]))[:700]
        lists[MID] = (d.astype(np.int32), _freqs(rng, d.size))
        _cache["collect_lists"] = lists
    return _cache["collect_lists"]


def collect_leaf(version=1):
    key = ("collect", version)
    if key not in _cache:
        rng = np.random.default_rng([CO_MAX_DOC, 13])
        _cache[key] = _Leaf(CO_MAX_DOC, collect_lists(), rng.integers(95, 125, size=CO_MAX_DOC).astype(np.uint8), version=version)
    return _cache[key]


def collect_docs_only(oracle, version=1):
    """The collect lists as an IndexOptions::Docs field (no freq blocks, plain-delta tails) -> (doc_bytes, term states)"""
    key = ("docs-only", version)
    if key not in _cache:
        w = oracle.Writer(CO_MAX_DOC, version=version, write_freqs=False)
        terms = np.zeros(len(CO_NAMES), dtype=oracle.TERM_STATE_DTYPE)
        terms["skip_offset"], terms["singleton_doc_id"] = -1, -1
        for t, (d, _) in enumerate(collect_lists()):
            if d.size:   # (an absent term has no postings to write: doc_freq 0)
                terms[t] = w.write_term(d, np.ones_like(d))
        doc_bytes = w.close()
        terms["total_term_freq"] = -1
        _cache[key] = (np.frombuffer(bytes(doc_bytes), np.uint8).copy(), terms)
    return _cache[key]


def _with_nots(qs):
    """every query with 0, 1 and 2 MUST_NOT clauses (one of the two absent in every third query)"""
    out = []
    for i, q in enumerate(qs):
        out += [q, q._replace(must_not=(MID,)), q._replace(must_not=(DF2176, ABSENT if i % 3 == 0 else R[3]))]
    return out


COLLECT_TERMS = _with_nots([Query(must=(t,)) for t in CO_TERM_LISTS]) + [Query(must=(ABSENT,)), Query(must=(DENSE,), must_not=(DENSE,))]
COLLECT_ANDS = _with_nots([Query(must=m) for m in [
    (DF129, DF2304), (DF2304, DF129),                       # the lead given first / last
    (R[2], DF2176, MID), (MID, DF2176, R[2]),
    (DF2176, ABSENT), (ABSENT, DF129, MID),                 # one clause absent: the empty set
    (DF2304, DENSE), (DENSE, MID, DF2176), (DENSE, ONE),    # a dense clause; a singleton lead
    (DF128, DF128), (MID, MID, DF127)]])                    # a repeated term
COLLECT_ORS = _with_nots([Query(should=s) for s in [
    (DF2304,), tuple(R[:9]), tuple(R[:10]), tuple(R[:16]),  # 1, 9, 10 and 16 clauses
    (ABSENT, DF129), (ABSENT, ABSENT), (DENSE, ONE, DF127), (MID, MID)]]) + [Query(should=(), must_not=(MID,))]
COLLECT_QUERIES = COLLECT_TERMS + COLLECT_ANDS + COLLECT_ORS


def ref_set(has, q):
    """The docs q matches, live docs not applied: a bool array over the leaf's docs"""
    max_doc = has.shape[1]
    if q.must:
        m = np.ones(max_doc, bool)
        for t in q.must:
            m &= has[t]
    else:
        m = np.zeros(max_doc, bool)
        for t in q.should:
            m |= has[t]
    for t in q.must_not:
        m &= ~has[t]
    return m


def pack(terms, queries, gpu, weight=1.0, sim_table=0, as_and=False):
    """ss.Query records (must XOR should, must_not; msm as given) over a flat table of term states -> (QUERY_DTYPE[], QUERY_TERM_DTYPE[]);
    a one-clause conjunction is RGPU_OP_TERM unless as_and"""
    qs = np.zeros(len(queries), dtype=gpu.QUERY_DTYPE)
    n = sum(len(q.must) + len(q.should) + len(q.must_not) for q in queries)
    ts = np.zeros(max(n, 1), dtype=gpu.QUERY_TERM_DTYPE)
    at = 0
    for i, q in enumerate(queries):
        assert not (q.must and q.should) and not q.filt
        pos = q.must or q.should
        op = (gpu.OP_OR | (q.msm << 8)) if not q.must else (gpu.OP_TERM if len(q.must) == 1 and not as_and else gpu.OP_AND)
        qs[i] = (op, len(pos), at, len(q.must_not))
        for t in tuple(pos) + tuple(q.must_not):
            ts[at]["state"] = terms[t]
            if terms[t]["doc_freq"] <= 0:
                ts[at]["state"]["doc_freq"], ts[at]["state"]["skip_offset"], ts[at]["state"]["singleton_doc_id"] = 0, -1, -1
            ts[at]["weight"], ts[at]["sim_table"] = weight, sim_table
            at += 1
    return qs, ts[:max(n, 1)]


# ---- masks for the parity sweep --------------------------------------------------------------------------------------------------
MASKS = ("empty", "full", "single", "half", "not-live")
SWEEP_SIZES = (1, 64, 65, 8193)
SWEEP_KS = (1, 10, 128, 129, 300)   # 300: more than the hits of most rows


def mask_of(name, max_doc, alive):
    """A doc set as a bool array: nothing, everything, one doc (the last), a seeded half, the complement of the live docs"""
    if name == "empty":
        return np.zeros(max_doc, bool)
    if name == "full":
        return np.ones(max_doc, bool)
    if name == "single":
        m = np.zeros(max_doc, bool)
        m[max_doc - 1] = True
        return m
    if name == "half":
        m = np.random.default_rng([max_doc, 62]).random(max_doc) < 0.5
        m[0] = True   # (a one-doc leaf keeps its doc)
        return m
    assert name == "not-live"
    return ~np.asarray(alive, bool)
