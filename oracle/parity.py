"""ORACLE — TEST INFRASTRUCTURE ONLY. Not shipped, not on the product path.

The parity rule for disjunctions the reference itself sums in heap order (DisjunctionSumScorer over a DisiPriorityQueue:
>= 10 SHOULD clauses, min_should_match <= 1 — search/scorer/disjunction_scorer.rs:41-45, 213-225; util/disi.rs:188-230).
There the reference pins a doc's score only up to the rounding of an f32 sum of non-negative terms, so "the same top-k"
cannot mean "the same bits". It means (north_star: bit-exact doc-id sets, scores within 1e-5 relative):

  1. TopDocs::total_hits is equal;
  2. the same number of rows is filled;
  3. every returned doc MATCHES the query and the oracle's own score OF THAT DOC (IndexSearcher::score_docs: the query's
     scorer advanced to it) is within `rtol` of the returned score — a wrong doc with a plausible score fails here;
  4. every oracle hit whose score exceeds the oracle's k-th score by more than `rtol` relative is returned — docs may
     only be exchanged inside the band of scores that tie with the k-th within the tolerance;
  5. rows are ordered (score desc; equal scores by doc id asc).

`docs_differing` = how many oracle hits are missing from the returned row (0 = identical doc-id sets).
"""
import numpy as np


class HeapOrderParityError(AssertionError):
    pass


def check_heap_order_row(osearcher, op, term_ids, got_docs, got_scores, got_total, want_docs, want_scores, want_n, want_total,
                         rtol=1e-5, min_should_match=0, what=""):
    """One query's row against the oracle's (canonical mode). `got_*`: the k-row under test, unused slots doc -1;
    `want_*`: the oracle's row, `want_n` slots filled. Returns docs_differing; raises HeapOrderParityError."""
    return _check_row(lambda gd: osearcher.score_docs(op, term_ids, gd, min_should_match=min_should_match), got_docs, got_scores, got_total,
                      want_docs, want_scores, want_n, want_total, rtol, what)


def check_heap_order_opt_row(full_docs, full_scores, got_docs, got_scores, got_total, k, rtol=1e-5, what=""):
    """The same rule for a MUST + SHOULD row (ReqOptScorer) whose ten or more optional clauses the reference sums in heap order.
    ReqOptScorer's skipping rule runs from doc to doc, so the oracle's score of one doc cannot be asked for on its own: `full_*` is
    the oracle's COMPLETE canonical row (search_opt with k >= total_hits), every match with the score the rule gave it. A doc the
    rule decided otherwise for misses its score by a whole optional sum and fails 3. Returns docs_differing."""
    full_docs, full_scores = np.asarray(full_docs), np.asarray(full_scores, dtype=np.float32)
    order = np.argsort(full_docs, kind="stable")
    by_doc, by_doc_scores = full_docs[order], full_scores[order]

    def score_of(gd):
        at = np.minimum(np.searchsorted(by_doc, gd), max(by_doc.size - 1, 0))
        matched = (by_doc[at] == gd) if by_doc.size else np.zeros(gd.size, bool)
        return np.where(matched, by_doc_scores[at] if by_doc.size else 0.0, 0.0).astype(np.float32), matched

    n = min(int(k), int(full_docs.size))
    return _check_row(score_of, got_docs, got_scores, got_total, full_docs[:n], full_scores[:n], n, int(full_docs.size), rtol, what)


def _check_row(score_of, got_docs, got_scores, got_total, want_docs, want_scores, want_n, want_total, rtol, what):
    """Rules 1 to 5. score_of(docs) -> (the oracle's score of each, whether it matches)."""
    def fail(msg):
        raise HeapOrderParityError("%s: %s" % (what, msg))

    n = int(want_n)
    got_docs = np.asarray(got_docs)
    got_scores = np.asarray(got_scores, dtype=np.float32)
    if int(got_total) != int(want_total):
        fail("total_hits %d != %d" % (int(got_total), int(want_total)))
    if not (got_docs[n:] == -1).all() or (got_docs[:n] < 0).any():
        fail("filled rows: want %d, got %s" % (n, got_docs.tolist()))
    if n == 0:
        return 0
    gd, gs = got_docs[:n], got_scores[:n]
    wd, ws = np.asarray(want_docs)[:n], np.asarray(want_scores, dtype=np.float32)[:n]
    if np.unique(gd).size != n:
        fail("a doc is returned twice")
    # 5. order
    ds = np.diff(gs.astype(np.float64))
    if (ds > 0).any():
        fail("scores not in descending order")
    if (np.diff(gd)[ds == 0] <= 0).any():
        fail("equal scores not in ascending doc order")
    # 3. the oracle's score of the returned docs
    os_, matched = score_of(gd)
    if not matched.all():
        fail("returned docs that do not match the query: %s" % gd[~matched].tolist())
    bad = np.abs(os_.astype(np.float64) - gs.astype(np.float64)) > rtol * np.abs(os_.astype(np.float64))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        fail("doc %d: returned score %r, oracle scores it %r" % (int(gd[i]), float(gs[i]), float(os_[i])))
    # 4. everything clearly above the oracle's k-th score must be there
    kth = float(ws[n - 1])
    clear = ws.astype(np.float64) > kth * (1.0 + rtol)
    missing = np.setdiff1d(wd[clear], gd)
    if missing.size:
        fail("oracle hits above the k-th score band are missing: %s" % missing.tolist())
    return int(np.setdiff1d(wd, gd).size)


def check_heap_order_batch(osearcher, op, term_rows, got_hits, got_totals, want_docs, want_scores, want_counts, want_totals,
                           rtol=1e-5, what=""):
    """Rows of a uniform batch (`term_rows`: [n_queries, n_clauses] term ids; `got_hits`: structured rows with "doc" /
    "score"). Returns the total docs_differing over the batch."""
    differing = 0
    for i in range(len(term_rows)):
        differing += check_heap_order_row(osearcher, op, term_rows[i], got_hits[i]["doc"], got_hits[i]["score"], got_totals[i],
                                          want_docs[i], want_scores[i], want_counts[i], want_totals[i], rtol=rtol,
                                          what="%s query %d %s" % (what, i, list(map(int, term_rows[i]))))
    return differing
