"""Cross-field fixtures and reference (plain Python, no GPU) for rgpu_search_fields_batch.

Fixtures. A leaf of two or three fields is ONE explicit index (indexgen.build_explicit) whose term list is the concatenation of the
fields' terms - one .doc file, as a Lucene segment has - plus one norms array per field (None: the field omits norms), one
sum_total_term_freq per field and one set of live docs. A clause is (field, term): `term` counts inside the field. docs_only_leaf()
splices the postings of a field written with IndexOptions::Docs (the oracle's restated writer, write_freqs = false) behind a
DocsAndFreqs field's, in one file: the footer is the first file's, the second field's file pointers move by the splice offset.

Reference. Per field an oracle Segment over the SAME .doc bytes, that field's term states and norms, with an oracle.Searcher of its
own: collection statistics, idf, norm cache and TermScorer are the field's. Per clause `score_docs(OP_TERM, [t], docs)` from its
field's searcher (as tests/dismax_ref.py does); the composition follows BooleanWeight::create_scorer in np.float32:

  group     disjuncts with doc_freq 0 drop; none left: no scorer; one left: that TermScorer's score; otherwise over the disjuncts that
            hold the doc, in disjunct order, sum from 0.0f and max from -inf, then max + (sum - max) * tie as three f32 operations
  SHOULD    groups with a scorer, clause order: 0.0f + g1 + g2 ...; a hit is held by max(1, min_should_match) groups
  MUST      a group without a scorer: nothing matches; otherwise the stable cost order (a term's doc_freq, a dismax group's sum over its
            present disjuncts), first addend as it is, the others added one by one; a hit is held by every group
  MUST_NOT  the union of the clauses' postings is excluded; live docs apply; rows are score desc, doc asc

A query is a dict: occur ("should" / "must"), groups (a list of ("term", (f, t)) or ("dismax", tie, [(f, t), ...])), msm, must_not
(a list of (f, t)). tests/test_cross_field_cpu.py holds this composition against the oracle's own OP_OR / OP_AND searches and
tests/dismax_ref.py where every clause sits in one field."""
import numpy as np

K1 = 1.2
W = 512   # FIELDS_WINDOW_DOCS of kernels/search_fields.hpp


def live_words(alive):
    b = np.packbits(np.asarray(alive, bool), bitorder="little")
    return np.concatenate([b, np.zeros((-b.size) % 8, np.uint8)]).view(np.uint64)


def freqs_of(rng, n):
    return np.minimum(10, rng.geometric(0.5, size=n)).astype(np.int32)


def spread(rng, max_doc, df, must_hold=()):
    """df distinct docs of [0, max_doc), ascending, the given ones among them"""
    must = np.unique(np.asarray(must_hold, np.int64))
    rest = np.setdiff1d(np.arange(max_doc), must)
    pick = rng.permutation(rest)[:df - must.size]
    out = np.sort(np.concatenate([must, pick])).astype(np.int32)
    assert out.size == df
    return out


class Field:
    def __init__(self, lists, norms, sttf, has_freqs=True):
        self.lists = [(np.asarray(d, np.int32), np.asarray(f, np.int32)) for d, f in lists]
        self.norms = None if norms is None else np.asarray(norms, np.uint8)
        self.sttf, self.has_freqs = int(sttf), has_freqs
        self.terms = None   # term states, filled by the leaf


class FieldView:
    """One field of a leaf with the attributes tests/dismax_ref.DismaxRef asks of a leaf"""

    def __init__(self, leaf, f):
        self.leaf, self.f = leaf, f
        self.lists, self.alive, self.doc_base, self.max_doc = leaf.fields[f].lists, leaf.alive, 0, leaf.max_doc

    def oracle_segment(self, oracle):
        return self.leaf.oracle_segment(oracle, self.f)


class CrossLeaf:
    def __init__(self, max_doc, fields, alive=None, version=1, doc_bytes=None, doc_base=0):
        from rucene_amd import indexgen
        self.max_doc, self.fields, self.version, self.doc_base = max_doc, fields, version, doc_base
        self.alive = np.ones(max_doc, bool) if alive is None else np.asarray(alive, bool)
        self.live_docs = None if alive is None else live_words(self.alive)
        if doc_bytes is None:   # one explicit index over the concatenation of the fields' terms
            seg = indexgen.build_explicit(max_doc, [l for fld in fields for l in fld.lists], norms=None, version=version)
            self.doc_bytes = seg.doc_bytes
            at = 0
            for fld in fields:
                fld.terms = seg.terms[at:at + len(fld.lists)].copy()
                at += len(fld.lists)
        else:                   # the caller spliced the file and set the fields' term states
            self.doc_bytes = doc_bytes
        for fld in fields:
            assert [int(x) for x in fld.terms["doc_freq"]] == [d.size for d, _ in fld.lists]
        self._searchers = {}

    def oracle_segment(self, oracle, f):
        fld = self.fields[f]
        return oracle.Segment(self.doc_bytes, fld.norms, self.max_doc, fld.terms, doc_base=self.doc_base, live_docs=self.live_docs,
                              sum_total_term_freq=fld.sttf, has_freqs=fld.has_freqs)

    def searcher(self, oracle, f):
        if f not in self._searchers:
            self._searchers[f] = oracle.Searcher([self.oracle_segment(oracle, f)], k1=K1)
        return self._searchers[f]

    def view(self, f):
        return FieldView(self, f)


def docs_only_leaf(oracle, max_doc, body, ident, alive=None, version=1):
    """Field 0 `body` (DocsAndFreqs) and field 1 `ident` (Docs, written without freqs) in one .doc file."""
    wa = oracle.Writer(max_doc, version=version, write_freqs=True)
    body.terms = np.array([wa.write_term(d, f) for d, f in body.lists], dtype=oracle.TERM_STATE_DTYPE)
    a = wa.close()
    wb = oracle.Writer(max_doc, version=version, write_freqs=False)
    ident.terms = np.array([wb.write_term(d, np.ones_like(d)) for d, _ in ident.lists], dtype=oracle.TERM_STATE_DTYPE)
    b = wb.close()
    ident.lists = [(d, np.ones_like(d)) for d, _ in ident.lists]
    ident.has_freqs = False
    # both files open with the same header (same segment id and suffix): its length is where the first multi-doc term starts
    many_a, many_b = body.terms[body.terms["doc_freq"] >= 2], ident.terms[ident.terms["doc_freq"] >= 2]
    assert many_a.size and many_b.size
    header = int(many_b["doc_start_fp"].min())
    assert header == int(many_a["doc_start_fp"].min()) and bytes(a[:header]) == bytes(b[:header])
    spliced = np.concatenate([a[:-16], b[header:-16], a[-16:]])
    ident_own = ident.terms.copy()           # the oracle reads the field from its own file
    ident.terms = ident.terms.copy()
    ident.terms["doc_start_fp"] += a.size - 16 - header
    ident.terms["total_term_freq"] = -1      # a Docs field's dictionary keeps none
    leaf = CrossLeaf(max_doc, [body, ident], alive=alive, version=version, doc_bytes=spliced)
    leaf.oracle_segment = lambda orc, f, _leaf=leaf: (
        orc.Segment(b, ident.norms, max_doc, ident_own, live_docs=_leaf.live_docs, sum_total_term_freq=ident.sttf, has_freqs=False) if f == 1 else
        orc.Segment(a, body.norms, max_doc, body.terms, live_docs=_leaf.live_docs, sum_total_term_freq=body.sttf))
    return leaf


def should(groups, msm=0, must_not=()):
    return dict(occur="should", groups=list(groups), msm=msm, must_not=list(must_not))


def must(groups, msm=0, must_not=()):
    return dict(occur="must", groups=list(groups), msm=msm, must_not=list(must_not))


def term(f, t):
    return ("term", (f, t))


def dismax(tie, clauses):
    return ("dismax", float(tie), list(clauses))


def group_clauses(g):
    return [g[1]] if g[0] == "term" else list(g[2])


class CrossRef:
    def __init__(self, oracle, leaf, searchers=None):
        """searchers: per field an oracle.Searcher over ALL leaves of an index (the weights are the statistics leaf's); None: the
        leaf alone"""
        self.oracle, self.leaf, self.searchers = oracle, leaf, searchers
        self._clauses = {}

    def searcher(self, f):
        return self.leaf.searcher(self.oracle, f) if self.searchers is None else self.searchers[f]

    def df(self, c):
        return int(self.leaf.fields[c[0]].lists[c[1]][0].size)

    def weight(self, c):
        """-> (weight at boost 1, the field's 256-entry norm cache): what a GPU clause carries"""
        return self.searcher(c[0]).term_weight(c[1], 1.0)

    def clause(self, c):
        """-> (live docs that hold term t of field f, ascending; the field's TermScorer's f32 score of each)"""
        if c not in self._clauses:
            docs = self.leaf.fields[c[0]].lists[c[1]][0]
            docs = docs[self.leaf.alive[docs]].astype(np.int32)
            scores, matched = self.searcher(c[0]).score_docs(self.oracle.OP_TERM, [c[1]], docs + np.int32(self.leaf.doc_base))
            assert matched.all(), ("the oracle's TermScorer does not hold a live doc of the fixture's list", c)
            self._clauses[c] = (docs, scores)
        return self._clauses[c]

    def group(self, g):
        """-> None (no scorer in the leaf) or (held mask, f32 score per doc, cost)"""
        n = self.leaf.max_doc
        present = [c for c in group_clauses(g) if self.df(c) > 0]
        if not present:
            return None
        cost = sum(self.df(c) for c in present)
        held = np.zeros(n, bool)
        if len(present) == 1:
            d, s = self.clause(present[0])
            score = np.zeros(n, np.float32)
            score[d] = s
            held[d] = True
            return held, score, cost
        total, best = np.zeros(n, np.float32), np.zeros(n, np.float32)
        for c in present:
            d, s = self.clause(c)
            first = ~held[d]
            total[d] = np.where(first, np.float32(0.0), total[d]) + s     # score_sum = 0.0; score_sum += sub_score
            best[d] = np.where(first, s, np.maximum(best[d], s))         # score_max = score_max.max(sub_score), from -inf
            held[d] = True
        diff = (total - best).astype(np.float32)
        prod = (diff * np.float32(g[1])).astype(np.float32)
        return held, (best + prod).astype(np.float32), cost

    def order(self, q):
        """The groups with a scorer in summation order, or None when the leaf is dead for the query"""
        gs = [self.group(g) for g in q["groups"]]
        if q["occur"] == "must":
            if any(g is None for g in gs):
                return None
            return [gs[i] for i in sorted(range(len(gs)), key=lambda i: gs[i][2])]   # (sorted() is stable)
        gs = [g for g in gs if g is not None]
        return gs or None

    def scores(self, q, order=None):
        """-> (matching live docs ascending, their f32 scores); `order`: another summation order (tests show that it matters)"""
        n = self.leaf.max_doc
        gs = self.order(q) if order is None else order
        if gs is None:
            return np.zeros(0, np.int32), np.zeros(0, np.float32)
        acc, count = np.zeros(n, np.float32), np.zeros(n, np.int32)
        for held, score, _ in gs:
            first = held & (count == 0)
            later = held & (count > 0)
            acc[first] = score[first] if q["occur"] == "must" else (np.float32(0.0) + score[first]).astype(np.float32)
            acc[later] = (acc[later] + score[later]).astype(np.float32)
            count[held] += 1
        need = len(gs) if q["occur"] == "must" else max(1, q["msm"])
        hit = (count >= need) & self.leaf.alive
        for c in q["must_not"]:
            hit[self.leaf.fields[c[0]].lists[c[1]][0]] = False
        docs = np.flatnonzero(hit).astype(np.int32)
        return docs, acc[docs]

    def rows(self, q, k=None):
        docs, sc = self.scores(q)
        o = np.lexsort((docs, -sc.astype(np.float64)))
        n = docs.size if k is None else min(int(k), docs.size)
        return docs[o][:n], sc[o][:n], int(docs.size)


def index_refs(oracle, leaves):
    """Leaves with cumulative doc bases -> one CrossRef per leaf that scores with per-field searchers over the whole index"""
    base = 0
    for leaf in leaves:
        leaf.doc_base = base
        base += leaf.max_doc
    searchers = {f: oracle.Searcher([leaf.oracle_segment(oracle, f) for leaf in leaves], k1=K1) for f in range(len(leaves[0].fields))}
    return [CrossRef(oracle, leaf, searchers) for leaf in leaves]


def index_rows(refs, q, k):
    """The merged row of an index: every leaf sums in its OWN order (presence and costs are per leaf), global ids, score desc, doc asc"""
    parts = [r.scores(q) for r in refs]
    docs = np.concatenate([d + np.int32(r.leaf.doc_base) for r, (d, _) in zip(refs, parts)])
    sc = np.concatenate([s for _, s in parts])
    o = np.lexsort((docs, -sc.astype(np.float64)))
    return docs[o][:k], sc[o][:k], int(docs.size)


def check_row(row, total, ref, q, what):
    """One row of search_fields_batch ({doc, score}[k]) against CrossRef: doc ids, score bits, -1 padding and the hit count, exact"""
    k = row.size
    d, s, tot = ref.rows(q, k)
    assert int(total) == tot, (what, "total", int(total), tot)
    n = min(k, tot)
    assert (row["doc"][n:] == -1).all() and (row["score"][n:] == 0).all(), (what, "padding", row["doc"][:8], n)
    assert (row["doc"][:n] == d).all(), (what, "docs", row["doc"][:8], d[:8])
    assert (row["score"][:n].view(np.int32) == s.view(np.int32)).all(), (what, "score bits", row["score"][:4], s[:4])


# ---- the C ABI's arrays -------------------------------------------------------------------------------------------------------------
def pack(ref, queries, sim_tables, field_of=lambda f: f):
    """queries (dicts) -> (rgpu_fields_query[], rgpu_field_group[], rgpu_field_clause[]); sim_tables[f]: the field's table handle;
    field_of: fixture field -> the segment's field slot"""
    from rucene_amd import _lib
    Q, G, C = [], [], []

    def clause(c, scored=True):
        row = np.zeros(1, _lib.FIELD_CLAUSE_DTYPE)[0]
        row["state"] = ref.leaf.fields[c[0]].terms[c[1]]
        if scored:
            row["weight"], row["sim_table"] = ref.weight(c)[0], sim_tables[c[0]]
        row["field"] = field_of(c[0])
        C.append(row)
    for q in queries:
        g0 = len(G)
        for g in q["groups"]:
            c0 = len(C)
            for c in group_clauses(g):
                clause(c)
            tie = np.float32(g[1] if g[0] == "dismax" else 0.0)
            G.append((c0, len(C) - c0, int(tie.view(np.uint32)), _lib.GROUP_DISMAX if g[0] == "dismax" else _lib.GROUP_TERM))
        n0 = len(C)
        for c in q["must_not"]:
            clause(c, scored=False)
        Q.append((_lib.OCCUR_MUST if q["occur"] == "must" else _lib.OCCUR_SHOULD, g0, len(G) - g0, q["msm"], n0, len(C) - n0))
    return (np.array(Q, _lib.FIELDS_QUERY_DTYPE), np.array(G, _lib.FIELD_GROUP_DTYPE),
            np.array(C, _lib.FIELD_CLAUSE_DTYPE) if C else np.zeros(0, _lib.FIELD_CLAUSE_DTYPE))
