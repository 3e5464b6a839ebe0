"""Expected rows of a BoostingQuery whose negative side is a union of term clauses, composed from the oracle (plain Python, no GPU),
over the fixtures of tests/segment_spectrum.py.

The reference (search/query/boosting_query.rs:102-118, search/scorer/boosting_scorer.rs:40-81): a leaf yields a scorer only when both
the positive and the negative weight have one there - a leaf in which no negative term has a posting matches nothing; iteration,
matching and total_hits are the positive scorer's alone; score() is the positive score, multiplied once in f32 by negative_boost when
the negative scorer (postings, not live docs) holds the doc. The oracle has no boosting scorer, so the rows are put together from
what it has: the positive's full match list and f32 scores from Searcher.search / search_not with k = the index's doc count (global
ids, every leaf scored with the statistics leaf's weights), minus the docs of the leaves in which no negative term has a posting,
the scores of the docs in the union of the fixture's negative lists multiplied in np.float32, sorted by (score desc, doc asc).
tests/test_boosting_cpu.py holds this composition against the oracle."""
import numpy as np

import segment_spectrum as ss


class Positive:
    """(op name, scored term ids, MUST_NOT term ids, min_should_match) - hashable, and what both mirrors are asked with."""

    def __init__(self, op, terms, must_not=(), msm=0):
        assert op in ("term", "and", "or") and (op != "term" or len(terms) == 1) and not (msm and must_not)
        self.op, self.terms, self.must_not, self.msm = op, tuple(terms), tuple(must_not), int(msm)

    def key(self):
        return (self.op, self.terms, self.must_not, self.msm)

    def __repr__(self):
        return "%s%r%s%s" % (self.op, self.terms, " -%r" % (self.must_not,) if self.must_not else "", " msm %d" % self.msm if self.msm else "")


class BoostingRef:
    """One index (a list of segment_spectrum.Leaf with their doc bases) and its oracle Searcher; a positive's full row is computed
    once and shared by every negative side and boost."""

    def __init__(self, oracle, leaves, osr=None):
        self.oracle, self.leaves = oracle, list(leaves)
        self.osr = osr or oracle.Searcher([leaf.oracle_segment(oracle) for leaf in self.leaves])
        self.max_doc = sum(leaf.max_doc for leaf in self.leaves)
        self._positive, self._rows = {}, {}

    def positive(self, p):
        """-> (every matching doc, canonical order; its f32 score; total_hits) of the positive query alone."""
        if p.key() not in self._positive:
            o = self.oracle
            op = {"term": o.OP_TERM, "and": o.OP_AND, "or": o.OP_OR}[p.op]
            k = max(self.max_doc, 1)
            if p.must_not:
                d, s, tot = self.osr.search_not(op, list(p.terms), list(p.must_not), k, tie_mode=o.TIE_CANONICAL)
            else:
                d, s, tot = self.osr.search(op, list(p.terms), k, tie_mode=o.TIE_CANONICAL, min_should_match=p.msm)
            assert d.size == tot, ("k = the doc count returns every hit", p, d.size, tot)
            d.setflags(write=False)
            s.setflags(write=False)
            self._positive[p.key()] = (d, s, tot)
        return self._positive[p.key()]

    def present(self, p):
        """The largest number of positive clauses that have a scorer in one leaf (an OR of ten or more sums in heap order there)."""
        return max(sum(1 for t in p.terms if leaf.lists[t][0].size > 0) for leaf in self.leaves)

    def negative_mask(self, negative):
        """-> (per global doc: some negative term holds it - postings, live or not; per global doc: its leaf has a negative scorer)."""
        held = np.zeros(self.max_doc, bool)
        scorer = np.zeros(self.max_doc, bool)
        for leaf in self.leaves:
            lo = leaf.doc_base
            for t in negative:
                held[lo + leaf.lists[t][0].astype(np.int64)] = True
            scorer[lo:lo + leaf.max_doc] = any(leaf.lists[t][0].size > 0 for t in negative)
        return held, scorer

    def rows(self, p, negative, boost, k=None):
        """-> (docs, scores, total_hits): the canonical row (score desc, doc asc), cut at k when k is given."""
        key = (p.key(), tuple(negative), float(np.float32(boost)))
        if key not in self._rows:
            d, s, _ = self.positive(p)
            held, scorer = self.negative_mask(negative)
            keep = scorer[d]
            d, s = d[keep], s[keep].copy()
            s[held[d]] = (s[held[d]] * np.float32(boost)).astype(np.float32)
            order = np.lexsort((d, -s.astype(np.float64)))
            self._rows[key] = (d[order], s[order])
        d, s = self._rows[key]
        n = d.size if k is None else min(int(k), d.size)
        return d[:n], s[:n], int(d.size)


def check_row(row, total, ref, p, negative, boost, exact, what, rtol=1e-5):
    """One row of search_batch ({doc, score}[k]) against BoostingRef. exact: doc ids, score bits, -1 padding and the hit count as they
    are. Otherwise (a positive of ten or more present SHOULD clauses, asked for with k >= the hit count): the hit count exact, the
    whole doc set exact - no doc left out, none twice - and every score within rtol of the reference's."""
    k = row.size
    d, s, tot = ref.rows(p, negative, boost)
    assert int(total) == tot, (what, "total", int(total), tot)
    n = min(k, tot)
    got_d, got_s = row["doc"][:n], row["score"][:n]
    assert (row["doc"][n:] == -1).all() and (got_d >= 0).all(), (what, "padding", row["doc"][:8], n)
    assert (row["score"][n:] == 0).all(), (what, "padding scores")
    if exact:
        assert (got_d == d[:n]).all(), (what, "docs", got_d[:8], d[:8])
        assert (got_s.view(np.int32) == s[:n].view(np.int32)).all(), (what, "score bits", got_s[:4], s[:4])
        return
    assert n == tot, (what, "a tolerance row is asked for with k >= the hit count")
    assert np.unique(got_d).size == n and sorted(got_d.tolist()) == sorted(d.tolist()), (what, "doc set")
    by_doc = dict(zip(d.tolist(), s.tolist()))
    want = np.array([by_doc[x] for x in got_d.tolist()], np.float32)
    np.testing.assert_allclose(got_s, want, rtol=rtol, atol=0, err_msg=str(what))
    assert ((np.diff(got_s) < 0) | ((np.diff(got_s) == 0) & (np.diff(got_d) > 0))).all(), (what, "order")


def hollow_leaves_with_positive_docs(leaves, p, negative):
    """Leaves without a negative scorer in which the positive query still matches live docs: what the hollow-leaf rule drops."""
    q = ss.Query(must=p.terms if p.op != "or" else (), should=p.terms if p.op == "or" else (), must_not=p.must_not, msm=p.msm)
    return [i for i, leaf in enumerate(leaves)
            if not any(leaf.lists[t][0].size > 0 for t in negative) and ss.ref_leaf_docs(leaf, q).size > 0]
