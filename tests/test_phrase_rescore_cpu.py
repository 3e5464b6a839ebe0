"""tests/phrase_rescore.py proven without a GPU: the restated rescorer against the oracle's QueryRescorer, the fixtures against the
oracle's phrase scorers, and the argument checks rgpu_rescore_phrase_batch makes before it needs a device."""
import numpy as np

import phrase_rescore as pr
import phrase_spectrum as ps


def test_rescore_ref_is_the_oracles_query_rescorer(oracle):
    """With a TERM second query rescore_ref must give oracle.Searcher.rescore's rows bit for bit: the doc -> score map comes from
    Searcher.score_docs (the second query's scorer advanced from doc to doc). Every mode, windows below / at / above the row
    length, weights other than 1, second terms that match some, all and none of the hits."""
    from rucene_amd import indexgen
    seg = indexgen.build_zipf(4000, 300)
    oseg = oracle.Segment(seg.doc_bytes, seg.norms, seg.max_doc, seg.terms, sum_total_term_freq=seg.sum_total_term_freq)
    osr = oracle.Searcher([oseg])
    rng = np.random.default_rng(5)
    n = 40
    some = matched_all = matched_none = 0
    for term in (0, 3, 40, 299):
        tdocs = oseg.decode_term(seg.terms[term])[0]
        for pick in ("mixed", "all", "none"):
            if pick == "all":
                if tdocs.size < n:
                    continue
                docs = rng.choice(tdocs, size=n, replace=False)
            elif pick == "none":
                docs = rng.choice(np.setdiff1d(np.arange(seg.max_doc), tdocs), size=n, replace=False)
            else:
                docs = rng.choice(seg.max_doc, size=n, replace=False)
            row = pr.make_row(docs.tolist(), 100 + term)
            scores, matched = osr.score_docs(oracle.OP_TERM, [term], [d for d, _ in row])
            second = {d: s for (d, _), s, m in zip(row, scores, matched) if m}
            some += 0 < len(second) < n
            matched_all += len(second) == n
            matched_none += len(second) == 0
            for mode in pr.MODES:
                for window, qw, rw in ((n, 1.0, 1.0), (n - 1, 0.7, 2.5), (1, 1.3, 0.25), (n + 5, 0.5, 3.0), (0, 0.7, 1.0), (17, 1.0, 0.0)):
                    want = pr.rescore_ref(row, second, window, qw, rw, mode)
                    wd, ws = osr.rescore(oracle.OP_TERM, [term], [d for d, _ in row], [s for _, s in row], window, qw, rw, mode)
                    assert [d for d, _ in want] == wd.tolist(), (term, pick, mode, window)
                    assert np.array([s for _, s in want], np.float32).view(np.uint32).tolist() == ws.view(np.uint32).tolist(), (term, pick, mode, window)
    assert some and matched_all and matched_none


def test_membership_fixture_is_what_its_case_table_says(oracle):
    """Every designed doc is where DESIGN says: postings kinds (df 1 / a tail only / a full block and a tail of one), the hits at
    posting 127 and 128 of B, the docs on every side of "every term holds the doc", and the phrase matches the oracle finds."""
    fx = pr.membership()
    D = pr.DESIGN
    ix = fx.index(oracle)
    try:
        sdocs, tdocs, bdocs = fx.docs_of(pr.S), fx.docs_of(pr.T), fx.docs_of(pr.B)
        assert len(sdocs) == 1 and ix.term_state(pr.S)["doc_freq"] == 1 and ix.term_state(pr.S)["singleton_doc_id"] == pr.SINGLETON_DOC
        assert 1 < len(tdocs) < 128 and len(bdocs) == 129 and fx.docs_of(pr.ABSENT) == [] and ix.term_state(pr.ABSENT)["doc_freq"] == 0
        assert bdocs.index(D["match-block-last"]) == 127 and bdocs.index(D["match-tail-only"]) == 128
        for name in ("match-block-last", "match-tail-only", "match", "terms-no-phrase"):
            assert D[name] in tdocs and D[name] in bdocs, name
        assert D["lacks-rarest"] in bdocs and D["lacks-rarest"] not in tdocs and tdocs[0] < D["lacks-rarest"] < tdocs[-1]
        assert D["lacks-most-frequent"] in tdocs and D["lacks-most-frequent"] not in bdocs and bdocs[0] < D["lacks-most-frequent"] < bdocs[-1]
        assert D["below-first-postings"] < min(tdocs[0], bdocs[0]) and D["above-last-postings"] > max(tdocs[-1], bdocs[-1])
        assert D["below-rarest-first"] < tdocs[0] and D["below-rarest-first"] in bdocs
        assert D["above-most-frequent-last"] > bdocs[-1] and D["above-most-frequent-last"] == tdocs[-1]
        assert len(tdocs) < len(bdocs)   # cost order: T leads, B follows
        assert [d for d, f in ix.phrase_freqs([pr.T, pr.B])] == sorted(pr.MATCHES) and all(f == 1 for _, f in ix.phrase_freqs([pr.T, pr.B]))
        assert [d for d, _ in ix.phrase_freqs([pr.S, pr.T, pr.B])] == [pr.SINGLETON_DOC]
        assert sorted(fx.second(ix, [pr.T, pr.B])) == sorted(pr.MATCHES)
        sd, sf = ix.sloppy_freqs([pr.B, pr.T], 2)   # "B T" is two moves away from "T B"
        assert sd.tolist() == sorted(pr.MATCHES) and (sf > np.finfo(np.float32).eps).all()
        assert fx.second(ix, [pr.T, pr.ABSENT]) == {}
        assert set(fx.second(ix, [pr.T, pr.B], boost=0.0).values()) == {np.float32(0.0)}
        # T's 40 positions are one trailing VInt block (a hit there goes on to the one-candidate kernel); B's lie in a packed block
        assert ps.place(fx.postings[pr.T], 264)["kind"] == "trailing" and ps.place(fx.postings[pr.B], 264)["kind"] == "packed"
    finally:
        ix.close()


def test_leaves_and_wide_fixtures(oracle):
    """The three leaves: equal doc freqs of T and B in the two leaves that hold both (the statistics leaf's weight is the right one
    in either), other matches in the second, no T in the third. wide(): every phrase matches some hits and misses others, no doc
    holds a term more than ten times."""
    l0, l1, l2 = pr.leaves()
    assert l0.max_doc >= l1.max_doc > l2.max_doc
    for t in (pr.T, pr.B):
        assert l0.docs_of(t) == l1.docs_of(t)
    assert l2.docs_of(pr.T) == [] and l2.docs_of(pr.S) == [] and len(l2.docs_of(pr.B)) == 60
    for fx in (l0, l1):   # the slop-2 phrase [T, S] (two terms the third leaf lacks) matches one doc in each of the others
        ixl = fx.index(oracle)
        try:
            assert ixl.sloppy_freqs([pr.T, pr.S], 2)[0].tolist() == [pr.SINGLETON_DOC] and fx.docs_of(pr.S) == [pr.SINGLETON_DOC]
        finally:
            ixl.close()
    ix1 = l1.index(oracle)
    try:
        assert [d for d, _ in ix1.phrase_freqs([pr.T, pr.B])] == sorted(pr.LEAF1_MATCHES)
    finally:
        ix1.close()
    fx = pr.wide()
    assert max(len(p) for pl in fx.postings for _, p in pl) <= ps.LANE_CAP
    ix = fx.index(oracle)
    try:
        for q in pr.WIDE_PHRASES:
            n = len(fx.second(ix, q.terms, q.slop))
            assert 0 < n < fx.max_doc, (q, n)
        assert len(fx.second(ix, pr.SEVEN, 2)) > len(fx.second(ix, pr.SEVEN, 0))
    finally:
        ix.close()


def test_rescore_phrase_entry_point_checks_its_arguments():
    """rgpu_rescore_phrase_batch without a device: null pointers and empty batches are RGPU_ERR_ILLEGAL_ARGUMENT, and the rows stay
    as they came."""
    from rucene_amd import _lib as gpu
    L = gpu.lib()
    assert "rgpu_rescore_phrase_batch" in gpu.EXPORTS
    qs = np.zeros(1, gpu.PHRASE_QUERY_DTYPE)
    ts = np.zeros(2, gpu.PHRASE_TERM_DTYPE)
    req = np.zeros(1, gpu.RESCORE_REQUEST_DTYPE)
    hits = pr.as_hits([[(3, 1.5), (9, 1.0)]], 4)
    before = hits.copy()
    f = L.rgpu_rescore_phrase_batch
    assert f(None, qs.ctypes.data, 1, ts.ctypes.data, 2, req.ctypes.data, 4, hits.ctypes.data, 1) == pr.ILLEGAL_ARGUMENT   # no segment
    assert f(None, None, 1, ts.ctypes.data, 2, req.ctypes.data, 4, hits.ctypes.data, 1) == pr.ILLEGAL_ARGUMENT
    assert f(None, qs.ctypes.data, 0, ts.ctypes.data, 2, req.ctypes.data, 4, hits.ctypes.data, 1) == pr.ILLEGAL_ARGUMENT
    assert f(None, qs.ctypes.data, 1, None, 0, None, 4, None, 0) == pr.ILLEGAL_ARGUMENT
    assert (hits == before).all()
    assert gpu.lib().rgpu_abi_version() == 6
