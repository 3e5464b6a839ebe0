"""Expected rows of a DisjunctionMaxQuery over term clauses, composed from the oracle's own per-clause scorers (plain Python, no
GPU), over the fixtures of tests/segment_spectrum.py.

The reference (search/query/disjunction_max_query.rs:142-161, search/scorer/disjunction_scorer.rs:246-262): per leaf the disjuncts
without a scorer drop out; a doc any remaining disjunct holds is a match; over those disjuncts in clause order
`sum = 0.0f; sum += s_i; max = max(max, s_i)`, and the score is `max + (sum - max) * tie` in f32. The oracle has no dismax scorer, so
the rows are put together from what it has: per clause the fixture's doc list and `Searcher.score_docs(OP_TERM, [t], docs)` - the
TermScorer's own f32 score of each doc, global ids, every leaf scored with the statistics leaf's weights - folded in np.float32
exactly as above (three separate f32 operations for the last step), restricted to live docs, sorted by (score desc, doc asc).
A clause absent from a leaf contributes nothing there. tests/test_dismax_cpu.py holds this composition against the oracle's OP_TERM
and OP_OR searches."""
import numpy as np


class DismaxRef:
    """One index (a list of segment_spectrum.Leaf with their doc bases) and its oracle Searcher; clause scores are computed once per
    term and shared by every query."""

    def __init__(self, oracle, leaves, osr=None):
        self.oracle, self.leaves = oracle, list(leaves)
        self.osr = osr or oracle.Searcher([leaf.oracle_segment(oracle) for leaf in self.leaves])
        self.max_doc = sum(leaf.max_doc for leaf in self.leaves)
        self.alive = np.concatenate([leaf.alive for leaf in self.leaves])
        self._clauses, self._rows = {}, {}

    def clause(self, t):
        """-> (global ids of the live docs that hold term t, ascending; the TermScorer's f32 score of each)."""
        if t not in self._clauses:
            docs = np.concatenate([leaf.lists[t][0].astype(np.int64) + leaf.doc_base for leaf in self.leaves] + [np.zeros(0, np.int64)])
            docs = docs[self.alive[docs]].astype(np.int32)
            scores, matched = self.osr.score_docs(self.oracle.OP_TERM, [t], docs)
            assert matched.all(), ("the oracle's TermScorer does not hold a live doc of the fixture's list", t)
            scores.setflags(write=False)
            docs.setflags(write=False)
            self._clauses[t] = (docs, scores)
        return self._clauses[t]

    def present(self, clauses):
        """The largest number of disjuncts that have a scorer in one leaf (ten or more: the reference sums in heap order there)."""
        return max(sum(1 for t in clauses if leaf.lists[t][0].size > 0) for leaf in self.leaves)

    def scores(self, clauses, tie):
        """-> (matching docs ascending, their f32 dismax scores)."""
        total = np.zeros(self.max_doc, np.float32)
        best = np.zeros(self.max_doc, np.float32)
        touched = np.zeros(self.max_doc, bool)
        for t in clauses:
            d, s = self.clause(t)
            first = ~touched[d]
            total[d] = np.where(first, np.float32(0.0), total[d]) + s          # score_sum = 0.0; score_sum += sub_score
            best[d] = np.where(first, s, np.maximum(best[d], s))              # score_max = score_max.max(sub_score), from -inf
            touched[d] = True
        docs = np.flatnonzero(touched).astype(np.int32)
        m, a = best[docs], total[docs]
        diff = (a - m).astype(np.float32)
        prod = (diff * np.float32(tie)).astype(np.float32)
        return docs, (m + prod).astype(np.float32)

    def rows(self, clauses, tie, k=None):
        """-> (docs, scores, total_hits): the canonical row (score desc, doc asc), cut at k when k is given."""
        key = (tuple(clauses), float(tie))
        if key not in self._rows:
            docs, sc = self.scores(clauses, tie)
            order = np.lexsort((docs, -sc.astype(np.float64)))
            self._rows[key] = (docs[order], sc[order])
        docs, sc = self._rows[key]
        n = docs.size if k is None else min(int(k), docs.size)
        return docs[:n], sc[:n], int(docs.size)


def check_row(row, total, ref, clauses, tie, exact, what, rtol=1e-5):
    """One row of search_batch ({doc, score}[k]) against DismaxRef. exact: doc ids, score bits, -1 padding and the hit count as they
    are. Otherwise (ten or more disjuncts in a leaf and tie > 0, where the reference pins the sum no tighter than rtol): the hit
    count exact, every returned doc a match with its score within rtol of the reference's, rows in canonical order, and every
    matching doc that beats the row's last score by more than rtol in the row - with k >= the hit count that is the whole doc set."""
    k = row.size
    d, s, tot = ref.rows(clauses, tie)
    assert int(total) == tot, (what, "total", int(total), tot)
    n = min(k, tot)
    got_d, got_s = row["doc"][:n], row["score"][:n]
    assert (row["doc"][n:] == -1).all() and (got_d >= 0).all(), (what, "padding", row["doc"][:8], n)
    if exact:
        assert (got_d == d[:n]).all(), (what, "docs", got_d[:8], d[:8])
        assert (got_s.view(np.int32) == s[:n].view(np.int32)).all(), (what, "score bits", got_s[:4], s[:4])
        return
    assert np.unique(got_d).size == n, (what, "a doc twice")
    by_doc = dict(zip(d.tolist(), s.tolist()))
    assert all(x in by_doc for x in got_d.tolist()), (what, "a doc that does not match")
    want = np.array([by_doc[x] for x in got_d.tolist()], np.float32)
    np.testing.assert_allclose(got_s, want, rtol=rtol, atol=0, err_msg=str(what))
    assert ((np.diff(got_s) < 0) | ((np.diff(got_s) == 0) & (np.diff(got_d) > 0))).all(), (what, "order")
    if n == tot:
        assert sorted(got_d.tolist()) == sorted(d.tolist()), (what, "doc set")
    else:
        must = d[s.astype(np.float64) > float(got_s[-1]) * (1 + rtol)]
        assert set(must.tolist()) <= set(got_d.tolist()), (what, "a better doc is missing")
