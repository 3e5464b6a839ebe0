"""Fixtures for exact phrases under doc-set masks (rgpu_search_phrase_batch_masked, _phrase_bool_batch_masked, _phrase_or_batch_masked).
Plain Python / numpy; tests/test_phrase_masked_cpu.py proves the equivalence they rest on, tests/test_gpu_phrase_masked.py runs them on
the device.

The equivalence (DESIGN, the masked phrase calls): no scorer of an exact phrase is two-phase, so "Q #F -X" collects what Q collects on a
twin leaf whose live docs are live AND F AND NOT X - docs, f32 score bits and total. On the oracle a zero-weight FILTER / MUST_NOT term
clause whose postings ARE the set stands in for the doc set: tests/phrase_bool.py and tests/phrase_or.py compose such queries already.

Fixtures:
  PROOFS   over tests/phrase_bool.py's main() (700 docs): (kind, the query with its set clauses, the query without them, F terms, X
           terms). The filter clause is the cheapest (R20, df 20 < the phrase's 40), in the middle (T129) and the dearest (D600) child
           of the conjunction; X is N1 (it holds the top hit) or N3.
  grid()   17 000 docs for the device. B is in every doc (a doc bitmap in the candidate conjunction); "A<n> B" has exactly n candidates
           for n = 130, 8191, 8193, 16385 (one, two and three chunks of the chunked collector) and is a phrase wherever d % 5 != 2.
           A130 = docs 0, 63, 64, 100, 103, ... 475, 16 999: one full block and a tail of two, so the marking conjunction emits the
           block's even postings to slots 0..63, its odd ones to 64..127 and the tail to 128, 129. C (two docs in three, every doc of A130) is the term clause
           of the boolean forms, N a MUST_NOT term (docs 0, 64, 6000), "D2 E2" a second phrase (docs 0..299), ABSENT a term no doc
           holds. DELETED: every doc with d % 11 == 5 (A130's 115, 148, ... among them).
  MASKS    name -> docs of the grid's masks (see masks())."""
import numpy as np

import phrase_bool as pb
import phrase_or as po
import phrase_rescore as pr

Ph = pb.Ph
UNSUPPORTED, ILLEGAL_ARGUMENT = -5, -2
COMPACT = {"phrase": "k_search_and(masked phrase candidates)", "bool": "k_search_and(masked phrase-bool candidates)",
           "or": "k_search_and(masked phrase-or candidates)"}
MARKED = {kind: name.replace(" candidates)", ", marked)") for kind, name in COMPACT.items()}
UNMASKED = {"phrase": "k_search_and(phrase candidates)", "bool": pb.CANDIDATES, "or": po.CANDIDATES}
SWITCH = "RGPU_PHRASE_MASK_COMPACT"

# ---- the proof's cases (tests/phrase_bool.py main()) --------------------------------------------------------------------------------
AB, BC = pb.AB, pb.BC
PROOFS = [
    # a bare phrase: +"a b" #f
    ("bool", pb.Q([AB], filters=[pb.R20]), pb.Q([AB]), [pb.R20], []),
    ("bool", pb.Q([AB], filters=[pb.T129]), pb.Q([AB]), [pb.T129], []),
    ("bool", pb.Q([AB], filters=[pb.D600]), pb.Q([AB]), [pb.D600], []),
    ("bool", pb.Q([AB], [pb.N1], filters=[pb.D600]), pb.Q([AB]), [pb.D600], [pb.N1]),
    # +"a b" +c #F -X with the filter cheapest, in the middle, dearest
    ("bool", pb.Q([AB, pb.D600], filters=[pb.R20]), pb.Q([AB, pb.D600]), [pb.R20], []),
    ("bool", pb.Q([AB, pb.D600], filters=[pb.T129]), pb.Q([AB, pb.D600]), [pb.T129], []),
    ("bool", pb.Q([AB, pb.T40], filters=[pb.D600]), pb.Q([AB, pb.T40]), [pb.D600], []),
    ("bool", pb.Q([pb.D600, AB, pb.T129], [pb.N1], filters=[pb.R20]), pb.Q([pb.D600, AB, pb.T129]), [pb.R20], [pb.N1]),
    ("bool", pb.Q([AB, BC, pb.D600], [pb.N1, pb.N3], filters=[pb.T129]), pb.Q([AB, BC, pb.D600], [pb.N3]), [pb.T129], [pb.N1]),   # -d stays, -X goes
    ("bool", pb.Q([AB, pb.D600], filters=[pb.T129, pb.T40]), pb.Q([AB, pb.D600], filters=[pb.T40]), [pb.T129], []),               # #e stays, #F goes
    # "a b" c -X, min_should_match <= 1
    ("or", po.Q([AB, pb.D600], [pb.N1]), po.Q([AB, pb.D600]), [], [pb.N1]),
    ("or", po.Q([pb.T129, AB, BC], [pb.N1, pb.N3]), po.Q([pb.T129, AB, BC], [pb.N3]), [], [pb.N1]),
    ("or", po.Q([AB], [pb.N3], msm=1), po.Q([AB]), [], [pb.N3]),
]


def twin_deleted(fx, deleted, filters, excludes):
    """the deleted docs of the twin leaf: live AND (every F) AND NOT (any X), as the complement"""
    gone = set(deleted)
    for t in filters:
        gone |= set(range(fx.max_doc)) - set(fx.docs_of(t))
    for t in excludes:
        gone |= set(fx.docs_of(t))
    return gone


def reference_rows(kind, ix, q):
    return ix.rows(q) if kind == "bool" else po.rows(ix, q)


# ---- grid() ---------------------------------------------------------------------------------------------------------------------------
B, A130, A8191, A8193, A16385, C, N, D2, E2, ABSENT = range(10)
GRID_TERMS, GRID_DOCS = 10, 17000
A130_DOCS = sorted({0, 63, 64, GRID_DOCS - 1} | {100 + 3 * i for i in range(126)})
A_DOCS = {A130: A130_DOCS, A8191: list(range(8191)), A8193: list(range(8193)), A16385: list(range(GRID_DOCS - 16385, GRID_DOCS))}
N_DOCS = (0, 64, 6000)
DELETED = frozenset(d for d in range(GRID_DOCS) if d % 11 == 5)
P130, P8191, P8193, P16385, PDE = Ph((A130, B)), Ph((A8191, B)), Ph((A8193, B)), Ph((A16385, B)), Ph((D2, E2))
BY_COUNT = {130: P130, 8191: P8191, 8193: P8193, 16385: P16385}


def phrase_holds(d):
    return d % 5 != 2


def grid():
    if "pm-grid" not in pr._built:
        h = {}
        for d in range(GRID_DOCS):
            h[d] = {B: [2] if phrase_holds(d) else [4]}
            if d % 3 != 2:
                h[d][C] = [10, 12] if d % 9 == 0 else [10]
        for t, docs in A_DOCS.items():
            for d in docs:
                h[d][t] = [1]
        for d in N_DOCS:
            h[d][N] = [11]
        for d in range(300):
            h[d][D2] = [20]
            h[d][E2] = [21] if d % 4 else [23]
        fx = pr.Fixture("pm-grid", GRID_DOCS, GRID_TERMS, h, 31)
        assert [len(fx.postings[t]) for t in (A130, A8191, A8193, A16385, B, ABSENT)] == [130, 8191, 8193, 16385, GRID_DOCS, 0]
        pr._built["pm-grid"] = fx
    return pr._built["pm-grid"]


def masks():
    """name -> sorted doc ids. `first n`: the first n docs of A130 (in doc order) and every doc that lacks A130 - n survivors of 130
    candidates on a leaf without deletions."""
    others = [d for d in range(GRID_DOCS) if d not in set(A130_DOCS)]
    block, tail = A130_DOCS[:128], A130_DOCS[128:]
    out = {"first %d" % n: sorted(A130_DOCS[:n] + others[::7]) for n in (0, 1, 63, 64, 65)}
    out["middle group empty"] = sorted(block[0::2] + tail)            # slots 64..127 (the block's odd postings) hold no survivor
    out["edges"] = [0, 63, 64, GRID_DOCS - 1]
    out["empty"] = []
    out["full"] = list(range(GRID_DOCS))
    out["disjoint"] = others
    out["overlaps deletions"] = sorted(set(A130_DOCS[::2]) | set(sorted(DELETED)[::2]) | {6000, 8190, 8192, GRID_DOCS - 1})
    out["handful"] = [0, 3, 64, 4097, 8190, 8192, 12000, 16384, GRID_DOCS - 1]
    out["other"] = sorted(set(range(0, GRID_DOCS, 2)) | {63})
    return out


def words_of(max_doc, docs):
    bits = np.zeros(max_doc + (-max_doc % 64), dtype=bool)
    bits[list(docs)] = True
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()
