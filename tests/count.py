"""Model and fixtures for hit counts without scoring - rgpu_count_batch, IndexSearcher::count (plain Python, no GPU).

The model is numpy set algebra over the postings that build a fixture, written from the reference's rules
(query/boolean_query.rs:196-275), not from the library's plan:
  * a MUST clause absent from the leaf: 0; a SHOULD or MUST_NOT clause absent from the leaf drops out, min_should_match stays;
  * no SHOULD clause left, or an OR of MUST_NOT clauses only: 0;
  * min_should_match counts clauses, not distinct terms;
  * every present MUST_NOT clause excludes its docs: two or more are a DisjunctionSumScorer(.., false, min_should_match), but
    ReqNotScorer only advance()s it and advance() does not look at the count (disjunction_scorer.rs:75-89, req_not_scorer.rs:47-78),
    so min_should_match never narrows the exclusion - tests/test_count_cpu.py holds that against the oracle;
  * a BoostingQuery's leaf without a posting of a demoting term: 0 (boosting_query.rs:102-118); otherwise those clauses are ignored;
  * optional clauses beside MUST clauses and a dismax's tie-breaker never change which docs match.

WINDOW is the leaf the window kernel's edges are held against, W = COUNT_WINDOW_DOCS read out of kernels/count.hpp: max_doc =
2 W + 37 (a short last window); postings at W - 1 and W; a block ending at W - 1 with the next starting at W; one sparse block
across all three windows; VInt tails of 0, 1 and 127 postings straddling the first edge; singletons at 0, W - 1, W and max_doc - 1;
an absent term; 64 lists that all hold one doc; seeded lists for conjunctions (two of equal doc_freq) and thresholds; every doc."""
import collections
import os
import re

import numpy as np

import segment_spectrum as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    """(COUNT_WINDOW_DOCS, counter bits) as kernels/count.hpp has them"""
    text = open(os.path.join(ROOT, "rucene_amd", "csrc", "kernels", "count.hpp")).read()
    w = re.search(r"constexpr int COUNT_WINDOW_DOCS = (\d+);", text)
    b = re.search(r"constexpr int COUNT_COUNTER_BITS = (\d+);", text)
    return int(w.group(1)), int(b.group(1))


W, COUNTER_BITS = kernel_constants()
MAX_DOC = 2 * W + 37
assert MAX_DOC <= 3 * W + 37

# op: "term" | "and" | "or" | "dismax"; pos / nots / opt / demote: term ids; msm: the min_should_match byte
CQ = collections.namedtuple("CQ", "op pos nots msm opt demote", defaults=((), 0, (), ()))

NAMES = ["EDGE", "BLK", "SPARSE", "TAIL0", "TAIL1", "TAIL127", "S0", "SW1", "SW", "SLAST", "ABSENT", "A", "B", "C", "EQ1", "EQ2", "ALL", "TAILONLY"]
EDGE, BLK, SPARSE, TAIL0, TAIL1, TAIL127, S0, SW1, SW, SLAST, ABSENT, A, B, C, EQ1, EQ2, ALL, TAILONLY = range(len(NAMES))
H = list(range(len(NAMES), len(NAMES) + 64))   # 64 lists that all hold doc H_DOC
H_DOC = W + 5
N_TERMS = len(NAMES) + 64


def _freqs(rng, n):
    return np.minimum(10, rng.geometric(0.5, size=n)).astype(np.int32)


def window_lists():
    rng = np.random.default_rng([W, 90])
    i32 = lambda x: np.asarray(x, np.int32)
    draw = lambda df: np.sort(rng.choice(MAX_DOC, size=df, replace=False)).astype(np.int32)
    docs = [None] * N_TERMS
    docs[EDGE] = i32([W - 1, W])
    docs[BLK] = np.arange(W - 128, W + 128, dtype=np.int32)                       # block 0 ends at W - 1, block 1 starts at W
    docs[SPARSE] = np.unique(np.linspace(5, 2 * W + 30, 128).astype(np.int32))    # one block, docs in all three windows
    docs[TAIL0] = np.arange(W - 64, W + 64, dtype=np.int32)                       # 128: a block across the edge, no tail
    docs[TAIL1] = np.concatenate([np.arange(W - 128, W, dtype=np.int32), i32([W])])        # the block ends at W - 1, a tail of one at W
    docs[TAIL127] = np.concatenate([np.arange(W - 300, W - 44, 2, dtype=np.int32), np.arange(W - 40, W + 87, dtype=np.int32)])  # 128 + 127 across the edge
    docs[S0], docs[SW1], docs[SW], docs[SLAST] = i32([0]), i32([W - 1]), i32([W]), i32([MAX_DOC - 1])
    docs[ABSENT] = i32([])
    docs[A], docs[B], docs[C] = draw(700), draw(300), draw(1500)
    docs[EQ1], docs[EQ2] = draw(300), draw(300)
    docs[ALL] = np.arange(MAX_DOC, dtype=np.int32)
    docs[TAILONLY] = np.sort(np.concatenate([rng.choice(docs[A], size=50, replace=False), i32([W - 1, W])]))
    docs[TAILONLY] = np.unique(docs[TAILONLY])                                    # < 128 postings: a VInt tail alone, mostly inside A
    for i, t in enumerate(H):
        docs[t] = i32([H_DOC, H_DOC + 1 + i])
    assert docs[SPARSE].size == 128 and docs[TAIL127].size == 255 and docs[TAILONLY].size < 128
    return [(d, _freqs(rng, d.size)) for d in docs]


class Leaf:
    def __init__(self, max_doc, lists, version=1, norms="rank"):
        from rucene_amd import indexgen
        rng = np.random.default_rng([max_doc, 91])
        self.norms = {"rank": rng.integers(95, 125, size=max_doc).astype(np.uint8),
                      "raw": ss.RAW_BYTES[rng.integers(0, ss.RAW_BYTES.size, size=max_doc)], "none": None}[norms]
        if norms == "raw":
            self.norms[:ss.RAW_BYTES.size] = ss.RAW_BYTES[:max_doc]
        self.max_doc, self.lists, self.version = max_doc, lists, version
        self.seg = indexgen.build_explicit(max_doc, lists, norms=self.norms, version=version)
        self.terms = self.seg.terms
        self.sttf = 60 * max_doc
        self.has = np.zeros((len(lists), max_doc), bool)
        for t, (d, _) in enumerate(lists):
            self.has[t, d] = True
        self.df = np.array([d.size for d, _ in lists])
        assert [int(x) for x in self.terms["doc_freq"]] == self.df.tolist()

    def oracle_segment(self, oracle, alive=None):
        return oracle.Segment(self.seg.doc_bytes, self.norms, self.max_doc, self.terms,
                              live_docs=None if alive is None else ss.live_words(alive), sum_total_term_freq=self.sttf)


_cache = {}


def window_leaf(version=1, norms="rank"):
    key = ("window", version, norms)
    if key not in _cache:
        _cache[key] = Leaf(MAX_DOC, window_lists(), version, norms)
    return _cache[key]


def seeded(max_doc, salt, share=0.6):
    return np.random.default_rng([max_doc, salt, 92]).random(max_doc) < share


def masks(max_doc):
    """name -> (alive or None, set or None): deletions, sets and both"""
    first, last = np.ones(max_doc, bool), np.ones(max_doc, bool)
    first[0], last[-1] = False, False
    return {"none": (None, None), "first-deleted": (first, None), "last-deleted": (last, None), "seeded-deleted": (seeded(max_doc, 1), None),
            "all-deleted": (np.zeros(max_doc, bool), None), "set": (None, seeded(max_doc, 2, 0.5)), "every-doc-set": (None, np.ones(max_doc, bool)),
            "empty-set": (None, np.zeros(max_doc, bool)), "set-under-deletions": (seeded(max_doc, 1), seeded(max_doc, 2, 0.5))}


def mask_of(max_doc, alive, docset):
    m = np.ones(max_doc, bool)
    if alive is not None:
        m &= alive
    if docset is not None:
        m &= docset
    return m


# ---- the model ------------------------------------------------------------------------------------------------------------------
def model_docs(has, df, q):
    """The docs q matches in a leaf (live docs not applied): a bool array"""
    max_doc = has.shape[1]
    none = np.zeros(max_doc, bool)
    if q.op in ("term", "and"):
        if any(df[t] == 0 for t in q.pos):
            return none
        m = np.ones(max_doc, bool)
        for t in q.pos:
            m &= has[t]
    else:
        present = [t for t in q.pos if df[t] > 0]
        if not present:
            return none
        need = max(1, q.msm) if q.op == "or" else 1
        m = np.sum([has[t] for t in present], axis=0) >= need
    if q.demote and not any(df[t] > 0 for t in q.demote):
        return none
    for t in q.nots:
        if df[t] > 0:
            m = m & ~has[t]
    return m


def model_count(has, df, mask, q):
    return int((model_docs(has, df, q) & mask).sum())


# ---- packing ----------------------------------------------------------------------------------------------------------------------
def pack(terms, queries, gpu, sim_table=0, weight=1.0):
    """CQ records -> (QUERY_DTYPE[], QUERY_TERM_DTYPE[]): positive, optional, MUST_NOT, demoting clauses in the ABI's order"""
    qs = np.zeros(len(queries), dtype=gpu.QUERY_DTYPE)
    n = sum(len(q.pos) + len(q.opt) + len(q.nots) + len(q.demote) for q in queries)
    ts = np.zeros(max(n, 1), dtype=gpu.QUERY_TERM_DTYPE)
    at = 0
    for i, q in enumerate(queries):
        base = {"term": gpu.OP_TERM, "and": gpu.OP_AND, "or": gpu.OP_OR, "dismax": gpu.OP_DISMAX}[q.op]
        if q.op == "dismax":
            assert not (q.nots or q.opt or q.demote or q.msm)
            qs[i] = (base, len(q.pos), at, int(np.float32(0.25).view(np.int32)))
        else:
            qs[i] = (base | (q.msm << 8) | (len(q.opt) << 16), len(q.pos), at, gpu.not_with_demote(len(q.nots), len(q.demote)))
        for j, t in enumerate(tuple(q.pos) + tuple(q.opt) + tuple(q.nots) + tuple(q.demote)):
            ts[at]["state"] = terms[t]
            if terms[t]["doc_freq"] <= 0:
                ts[at]["state"]["doc_freq"], ts[at]["state"]["skip_offset"], ts[at]["state"]["singleton_doc_id"] = 0, -1, -1
            ts[at]["weight"] = 0.5 if j >= len(q.pos) + len(q.opt) + len(q.nots) else weight   # a demoting clause carries negative_boost
            ts[at]["sim_table"] = sim_table
            at += 1
    return qs, ts


# ---- the rows -----------------------------------------------------------------------------------------------------------------------
T = lambda t, **kw: CQ("term", (t,), **kw)
AND = lambda *p, **kw: CQ("and", p, **kw)
OR = lambda *p, **kw: CQ("or", p, **kw)

WINDOW_ROWS = (
    [T(t, nots=(S0 if t == SLAST else SLAST,)) for t in (EDGE, BLK, SPARSE, TAIL0, TAIL1, TAIL127, S0, SW1, SW, SLAST)]   # every edge list alone in the window kernel (a present MUST_NOT clause sends a lone term there)
    + [OR(EDGE, BLK, SPARSE), OR(TAIL0, TAIL1, TAIL127), OR(S0, SW1, SW, SLAST), OR(A, B, C), OR(SPARSE, S0, SLAST, ABSENT),
       OR(A, B, nots=(C,)), OR(BLK, TAIL127, nots=(EDGE, SW)), T(A, nots=(B,)), T(SPARSE, nots=(EDGE,)), AND(A, nots=(C,)), T(ALL, nots=(A,))])
THRESHOLD_ROWS = (
    [OR(A, B, C, msm=m) for m in (0, 1, 2, 3, 4)]                                                       # msm 0 | 1 | 2 | n | n + 1
    + [OR(A, A, msm=2), OR(A, A, B, msm=2), OR(A, A, msm=3),                                            # a repeated term counts twice
       OR(*H, msm=64), OR(*H[:63], msm=64), OR(*H[:63], msm=63), OR(*H, msm=2),                         # 64 | 63 clauses that all hold one doc
       OR(A, B, nots=(C,)), OR(A, B, msm=2, nots=(C, EQ1)), OR(A, B, msm=2, nots=(C, ABSENT)),          # MUST_NOT: one; two under msm 2; one + absent
       OR(A, B, C, msm=2, nots=(EQ1, EQ1)), OR(A, B, msm=3, nots=(C, EQ1)),
       OR(A, B, nots=(ALL,)), T(A, nots=(ALL,)), OR(nots=(A,)), OR(ABSENT, ABSENT), OR(ABSENT, ABSENT, nots=(A,)),
       OR(TAIL127, EDGE, BLK, msm=2), OR(SPARSE, S0, SLAST, ALL, msm=2)])
CONJ_ROWS = [AND(A, C), AND(C, A), AND(A, B, C), AND(A, ABSENT), AND(A, nots=(A,)), AND(A, A), AND(A, A, C), AND(TAILONLY, A), AND(SW, BLK),
             AND(EQ1, EQ2), AND(EQ2, EQ1), AND(A, C, nots=(B,)), AND(A, C, nots=(B, EQ1)), AND(A, C, nots=(ABSENT,)), AND(A, C, nots=(C,)),
             AND(BLK, TAIL0), AND(ALL, SPARSE), AND(EDGE, TAIL1, TAIL127)]
TERM_ROWS = [T(t) for t in (EDGE, BLK, SPARSE, TAIL0, TAIL1, TAIL127, S0, SW1, SW, SLAST, ABSENT, A, ALL, TAILONLY)] + [OR(A), OR(A, ABSENT), OR(A, A, msm=2), AND(B, B)]
ABI_ROWS = [CQ("dismax", (A, B, C)), CQ("dismax", (ABSENT, SPARSE)), CQ("dismax", (ABSENT,)),
            CQ("and", (A, C), opt=(B, EQ1)), CQ("term", (A,), opt=(B,), msm=2), CQ("and", (A, C), nots=(EQ1,), opt=(B,)),
            CQ("term", (A,), nots=(C, EQ1), opt=(B, EQ2), msm=2), CQ("and", (A, C), nots=(B, EQ1), opt=(EQ2,), msm=2),
            CQ("term", (A,), demote=(B,)), CQ("term", (A,), demote=(ABSENT,)), CQ("or", (A, B), demote=(ABSENT, C)), CQ("and", (A, C), nots=(B,), demote=(ABSENT,)),
            CQ("or", (A, B), msm=2, demote=(EQ1,))]
ALL_ROWS = WINDOW_ROWS + THRESHOLD_ROWS + CONJ_ROWS + TERM_ROWS + ABI_ROWS


def oracle_form(q):
    """(op name, positive ids, MUST_NOT ids, msm) of a row the oracle's search_batch can take - the optional and demoting clauses and a
    dismax's tie-breaker, which never change the docs, left out (None where that rewriting is not the identity on the docs)"""
    if q.demote and ABSENT in q.demote and all(t == ABSENT for t in q.demote):
        return None   # the one leaf rule: nothing to hold against a plain query
    if q.op == "dismax":
        return ("or", q.pos, (), 0)
    if q.op in ("term", "and"):
        return ("and" if (len(q.pos) > 1 or q.nots) else "term", q.pos, q.nots, 0)
    return ("or", q.pos, q.nots, q.msm)
